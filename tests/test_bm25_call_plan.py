"""What kind of call a vf_bm25_search is and what it launches (veritasfi_amd/csrc/vf_bm25_call.h), EXECUTED on the CPU: a host-compiled
driver (tests/bm25_call_driver.py, UBSan) prints what the decoder and the launch plan return over a fixed crossing of arguments, and
every line is held to the value written out here from the rules of include/veritasfi_hip.h and of the kernels' scratch.  No GPU.

Decoder: every combination of the three flag bits x struct pointer null or not x phase -1 .. 5 x nq in {0, 1, 64}.  Plan: n in {1, 31, 4096, 4097, 32768, 32769, 70001} x the k of {1, 2, 4096, 4097, n} that fit x nq in {1, slot_cap,
slot_cap + 1} x every kind x m in {0, 1, k - 1, k, n}."""
import pytest

import bm25_call_driver as drv

# the header's enumerations, in its order
PLAIN, FILTERED, SUB_STAGE, SUB_SEARCH, PREP_PREPARE, PREP_ARM, PREP_RELEASE, PREP_SEARCH = range(8)
ACCEPTED, PREPARED_NOT_ALONE, NULL_PREPARED, PREPARED_PHASE, NULL_FILTER, SUBSTATS_PHASE, SUBSTATS_ALONE = range(7)
SCATTER_PLAIN, SCATTER_FILTERED, SCATTER_SUB_POS, SCATTER_SUB_COL = range(4)

# include/veritasfi_hip.h, per combination of (VF_BM25_PREPARED, VF_BM25_FILTER, VF_BM25_SUBSTATS): the refusal of a null struct (None: no
# struct is read), then the kind by phase (a kind alone: the phase is not read) and the refusal of any other phase.  The refusals stand
# in the entry point's order: a combination of flags is refused before the struct is looked at, a null struct before its phase.
RULES = {
    (0, 0, 0): (None, PLAIN, None),
    (0, 0, 1): (None, SUBSTATS_ALONE, None),                      # the statistics are those of a filter's rows
    (0, 1, 0): (NULL_FILTER, FILTERED, None),
    (0, 1, 1): (NULL_FILTER, {1: SUB_STAGE, 2: SUB_SEARCH}, SUBSTATS_PHASE),
    (1, 0, 0): (NULL_PREPARED, {1: PREP_PREPARE, 2: PREP_ARM, 3: PREP_SEARCH, 4: PREP_RELEASE}, PREPARED_PHASE),
    (1, 0, 1): (None, PREPARED_NOT_ALONE, None),                  # VF_BM25_PREPARED goes alone
    (1, 1, 0): (None, PREPARED_NOT_ALONE, None),
    (1, 1, 1): (None, PREPARED_NOT_ALONE, None),
}
REFUSED_WHATEVER_THE_STRUCT = {(0, 0, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)}


def _decoded(flags, null, phase, nq):
    """(kind, refusal, nq, subset) the decoder must return; kind and nq are -1 for a refusal; the filter's mode is not the decoder's to know."""
    key = (flags & 1, flags >> 1 & 1, flags >> 2 & 1)
    if_null, by_phase, bad_phase = RULES[key]
    if key in REFUSED_WHATEVER_THE_STRUCT:
        return (-1, by_phase, -1, 0)
    if null and if_null is not None:
        return (-1, if_null, -1, 0)
    kind = by_phase.get(phase) if isinstance(by_phase, dict) else by_phase
    if kind is None:
        return (-1, bad_phase, -1, 0)
    return (kind, ACCEPTED, nq, 0)


def _planned(n, k, nq, kind, subset, m):
    """(no_launch, small, S, scatter, tail_f, tail_blocks, tblk_stride, pad_from, pad_out) of a call."""
    if kind in (PREP_PREPARE, PREP_ARM, PREP_RELEASE):   # they search nothing
        return (1, 0, 0, 0, 0, 0, 0, 0, 0)
    blocks, cap = drv.words(n) // 1024, drv.slot_cap(n)
    filtered = kind != PLAIN
    small = k <= 4096
    S = min(nq, cap) if small or kind == SUB_STAGE else 1   # the deep-k scratch holds one query; a stage makes its search's slots
    scatter = {PLAIN: SCATTER_PLAIN, SUB_SEARCH: SCATTER_SUB_POS}.get(kind, SCATTER_SUB_COL if kind == PREP_SEARCH and subset else SCATTER_FILTERED)
    tail_blocks = 1 if small and not filtered else blocks
    tblk_stride = 0 if not small else (blocks if filtered else 1)
    pad_from = min(m, k) if filtered else k
    return (int(filtered and m == 0), int(small), S, scatter, int(filtered), tail_blocks, tblk_stride, pad_from, int(filtered and pad_from < k))


@pytest.fixture(scope="module")
def outcome(tmp_path_factory):
    run = drv.run(drv.build(tmp_path_factory.mktemp("bm25_call_plan")))
    print(run.stdout[-2000:])
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-3000:])
    lines = {"D": {}, "P": {}}
    for line in run.stdout.splitlines():
        if line[:2] in ("D ", "P "):
            args, got = line[2:].split(" -> ")
            key = tuple(int(x) for x in args.split())
            assert key not in lines[line[0]], line
            lines[line[0]][key] = tuple(int(x) for x in got.split())
    return run.stdout, lines


def test_every_flag_combination_and_phase_decodes_to_its_kind_or_its_first_refusal(outcome):
    stdout, lines = outcome
    want = {(flags, null, phase, nq): _decoded(flags, null, phase, nq)
            for flags in range(8) for null in (0, 1) for phase in drv.PHASES for nq in drv.NQS}
    assert f"decode: {8 * 2 * 7 * 3} cases" in stdout and len(want) == 8 * 2 * 7 * 3
    wrong = {key: (lines["D"].get(key), want[key]) for key in want if lines["D"].get(key) != want[key]}
    assert not wrong and len(lines["D"]) == len(want), dict(list(wrong.items())[:10])
    # every kind and every refusal was met
    assert {v[0] for v in want.values()} == set(range(8)) | {-1} and {v[1] for v in want.values()} == set(range(7))


def test_the_plan_of_every_kind_at_the_sizes_where_it_changes(outcome):
    stdout, lines = outcome
    want = {}
    for n in drv.SIZES:
        for k in drv.ks(n):
            for nq in (1, drv.slot_cap(n), drv.slot_cap(n) + 1):
                for kind in range(8):
                    for subset in ((0, 1) if kind == PREP_SEARCH else (0,)):
                        for m in drv.ms(n, k):
                            want[(n, k, nq, kind, subset, m)] = _planned(n, k, nq, kind, subset, m)
    assert f"plan: {len(want)} cases" in stdout
    wrong = {key: (lines["P"].get(key), want[key]) for key in want if lines["P"].get(key) != want[key]}
    assert not wrong and len(lines["P"]) == len(want), dict(list(wrong.items())[:10])
    # what the issue names: one tail block for the unfiltered small-k call, words / 1024 for every filtered and every deep-k one
    for (n, k, nq, kind, subset, m), p in want.items():
        if kind in (PREP_PREPARE, PREP_ARM, PREP_RELEASE):
            continue
        assert p[5] == (1 if kind == PLAIN and k <= 4096 else drv.words(n) // 1024)
        assert p[0] == int(kind != PLAIN and m == 0)
    assert drv.words(70001) // 1024 == 3 and drv.words(32768) // 1024 == 1 and drv.words(32769) // 1024 == 2
