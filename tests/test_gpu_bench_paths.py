"""The N > 1 code paths of bench.py, run on the one-GPU box as fresh child processes so that the driver's `-m gpu` pass executes
them (round-3 review, item 4): (i) the self-launched rank -- this process never touches the GPU before it starts the child, the
child's launcher parent never does at all -- meets itself over RCCL, ships every bucket of 4 batches through ONE
all_gather_into_tensor + ONE merge launch and checks the merged result against the per-shard CPU oracle; (ii) the
single-process form, two shards on device 0 behind one handle (peer copies + merge)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(flags, extra_env, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_bench_self_launched_rank_exchanges_over_rccl_and_verifies():
    out, err = _bench(["--gpus", "1", "--rows", "400000", "--steps", "8", "--warmup", "2", "--verify", "--no-rerank"],
                      {"VF_BENCH_LAUNCH": "1", "VF_BENCH_FORCE_EXCHANGE": "1"})
    assert out["rccl"] is not None and out["rccl"]["backend"] == "nccl" and out["rccl"]["world"] == 1, out["rccl"]
    assert out["verify"] is not None and out["verify"]["verified"] is True, out["verify"]
    assert out["config"]["batches_per_exchange"] == 4 and out["n_gpus"] == 1 and out["steps"] == 8
    assert out["value"] > 0 and out["roofline"]["frac"] > 0
    assert "verify ok" in err


@pytest.mark.gpu
def test_bench_single_process_two_shards_on_one_device():
    out, _ = _bench(["--single-process", "--gpus", "2", "--devices", "0,0", "--rows", "400000", "--steps", "8", "--warmup", "2",
                     "--no-rerank", "--no-cpu-baseline"], {})
    assert out["n_gpus"] == 2 and out["value"] > 0
    assert "ONE handle" in out["config"]["workload"]
    assert out["search_stats"]["exact_reruns_last_batch"] == 0


@pytest.mark.gpu
def test_bench_four_ranks_share_the_one_gpu():
    """`bench.py --gpus 4` as the driver starts it on a node -- the launcher, four rank processes, row shards, every bucket through ONE
    all-gather + ONE 4-part merge launch, the data-parallel re-rank (25 pairs per rank + an all-gather of the logits), the per-shard
    oracle check of the merged result -- rehearsed on the one-GPU box: VF_BENCH_SHARE_DEVICE=1 puts every rank on device 0 and carries
    the collectives over gloo (RCCL refuses two ranks on one device; the pool allows six processes on a card, so four ranks + this
    process).  Nothing here is a performance figure."""
    out, err = _bench(["--gpus", "4", "--rows", "500000", "--steps", "8", "--warmup", "2", "--rerank-pairs", "100", "--rerank-tokens", "64",
                       "--full"],
                      {"VF_BENCH_SHARE_DEVICE": "1"}, timeout=800)
    assert out["n_gpus"] == 4 and out["config"]["rows_per_gpu"] == [125_000] * 4 and out["config"]["batches_per_exchange"] == 4
    assert out["rccl"]["backend"] == "gloo" and out["rccl"]["world"] == 4 and len({d["pid"] for d in out["rccl"]["devices"]}) == 4
    assert out["verify"] is not None and out["verify"]["verified"] is True, out["verify"]
    assert out["rerank"]["pairs_on_rank0"] == 25 and out["rerank_p50_ms"] > 0, out["rerank"]
    assert out["value"] > 0
