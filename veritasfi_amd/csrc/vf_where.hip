// vf_where.hip -- a metadata filter evaluated on gfx950 (vf_index_search_device with VF_SEARCH_WHERE; the program, the checks and the
// output geometry: vf_where.h; the grammar and the key maps: veritasfi_amd/where.py).
//
// Kernels
//   k_where_eval   one workgroup (four waves) per tile of tile_rows rows, one lane per row, 64 rows per wave step.  A lane runs
//                  where_eval_row over its row: leaves and ops are the same for every lane, so their loads are uniform; a leaf's
//                  column pointer comes out of the uploaded table and is given its global address space back (a pointer out of memory
//                  is a flat one to the compiler: k_scan_subset_m), the key load is then one coalesced 512-byte read per wave, the
//                  validity word one broadcast read per half wave.  The wave's 64 verdicts are one ballot; lane 0 writes them as two
//                  uint32 words in the BM25 filter's layout.  Rows at or past n vote 0, so the tail bits are zero; a wave step wholly past
//                  n writes nothing (the bitmap ends at ceil(n / 64) steps).  The tile's popcount goes to tile_counts: no atomics, nothing to zero.
//   k_where_scan   ONE workgroup: the exclusive prefix of the tile counts, 256 at a time with a running carry, and the total m.
//   k_where_ids    one workgroup per tile: a wave re-reads its two bitmap words; a lane whose bit is set writes id_offset + row at
//                  prefix[tile] + (passing rows of the tile below it) -- where_rank_in_tile's rule, with the tile's per-step popcounts in
//                  LDS.  The list is strictly ascending by construction and is what VF_SEARCH_SUBSET takes.
// Every index is bounded by what the host checked before the launch: rows < n, bitmap words < 2 * ceil(n / 64), tiles < where_tiles,
// an id's position < m <= n <= ids_cap.
#include "vf_internal.h"
#include "vf_where.h"

namespace vf {

typedef const int64_t __attribute__((address_space(1)))* global_i64_ptr;
typedef const uint32_t __attribute__((address_space(1)))* global_u32_ptr;
constexpr int kWhereThreads = 256, kWhereWaves = kWhereThreads / kWhereWaveRows;
static_assert(kWhereTileRows / kWhereWaveRows <= kWhereThreads, "k_where_ids: one thread per wave step of a tile");

__global__ __launch_bounds__(kWhereThreads) void k_where_eval(WhereArgs a) {
    __shared__ u32 wave_count[kWhereWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int steps = a.tile_rows / kWhereWaveRows;
    const long long g0 = (long long)blockIdx.x * steps;
    const WhereColumnPtr* __restrict__ columns = a.columns;
    const WhereLeaf* __restrict__ leaves = a.leaves;
    const uint8_t* __restrict__ ops = a.ops;
    const int64_t* __restrict__ sets = a.sets;
    u32 count = 0;
    for (int s = wave; s < steps; s += kWhereWaves) {
        const long long g = g0 + s, row = g * kWhereWaveRows + lane;
        if (g * kWhereWaveRows >= a.n) break;
        bool pass = false;
        if (row < a.n)
            pass = where_eval_row(leaves, ops, a.n_ops, sets,
                                  [&](int c) -> int64_t { return ((global_i64_ptr)columns[c].keys)[row]; },
                                  [&](int c) -> bool {
                                      const uint32_t* v = columns[c].valid;
                                      return v == nullptr || ((((global_u32_ptr)v)[row >> 5] >> (row & 31)) & 1u) != 0;
                                  });
        const u64 bits = __ballot(pass);
        if (lane == 0) { a.bitmap[2 * g] = (u32)bits; a.bitmap[2 * g + 1] = (u32)(bits >> 32); }
        count += (u32)__popcll(bits);
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 total = 0;
#pragma unroll
        for (int w = 0; w < kWhereWaves; ++w) total += wave_count[w];
        a.tile_counts[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(kWhereThreads) void k_where_scan(const u32* __restrict__ counts, long long n_tiles, long long* __restrict__ prefix,
                                                              long long* __restrict__ m_out) {
    __shared__ long long part[kWhereThreads];
    long long carry = 0;
    for (long long base = 0; base < n_tiles; base += kWhereThreads) {
        const long long t = base + threadIdx.x;
        const long long v = t < n_tiles ? (long long)counts[t] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < kWhereThreads; off <<= 1) {
            const long long add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (t < n_tiles) prefix[t] = carry + part[threadIdx.x] - v;
        carry += part[kWhereThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *m_out = carry;
}

__global__ __launch_bounds__(kWhereThreads) void k_where_ids(WhereArgs a) {
    __shared__ u32 step_count[kWhereTileRows / kWhereWaveRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int steps = a.tile_rows / kWhereWaveRows;
    const long long g0 = (long long)blockIdx.x * steps, groups = where_groups(a.n);
    const u32* __restrict__ bitmap = a.bitmap;
    if ((int)threadIdx.x < steps) {
        const long long g = g0 + threadIdx.x;
        step_count[threadIdx.x] = g < groups ? (u32)where_popcount64(where_group_bits(bitmap, g)) : 0u;
    }
    __syncthreads();
    const long long base = a.tile_prefix[blockIdx.x];
    for (int s = wave; s < steps; s += kWhereWaves) {
        const long long g = g0 + s;
        if (g >= groups) break;
        const u64 bits = where_group_bits(bitmap, g);
        u32 below = 0;
        for (int j = 0; j < s; ++j) below += step_count[j];
        if ((bits >> lane) & 1ull)
            a.ids[base + below + where_popcount64(bits & (lane ? (~0ull >> (64 - lane)) : 0ull))] = a.id_offset + g * kWhereWaveRows + lane;
    }
}

hipError_t launch_where(const WhereArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (!where_tile_rows_ok(a.tile_rows) || a.n_ops < 1 || a.n_ops > kWhereMaxOps || !a.columns || !a.leaves || !a.ops || !a.bitmap || !a.tile_counts ||
        !a.tile_prefix || !a.m_out)
        return hipErrorInvalidValue;
    const long long tiles = where_tiles(a.n, a.tile_rows);
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_where_eval, dim3((unsigned)tiles), dim3(kWhereThreads), 0, s, a);
    hipLaunchKernelGGL(k_where_scan, dim3(1), dim3(kWhereThreads), 0, s, a.tile_counts, tiles, a.tile_prefix, a.m_out);
    if (a.ids) hipLaunchKernelGGL(k_where_ids, dim3((unsigned)tiles), dim3(kWhereThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace vf
