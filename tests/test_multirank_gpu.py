"""N > 1 ranks with the REAL kernels: two fresh rank processes of bench.py on one GPU box, the
rendezvous and the far-end broadcast over gloo (WMIX_BENCH_ONE_GPU_GLOO=1: every rank on cuda:0; on an 8-GPU node the same
code runs with backend nccl = RCCL, one rank per GPU -- only the backend string differs).  Each rank shards its own streams,
rank 0 alone owns the far-end, and every rank replays its sampled streams through the oracle: rank 1's AEC output can only be
right if the broadcast delivered every packet."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_two_ranks_real_kernels_far_end_through_the_broadcast():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(WMIX_BENCH_ONE_GPU_GLOO="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    # children of their own: this process makes no GPU call for them
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "chain", "--streams", "512",
                        "--steps", "6", "--warmup", "2", "--prime", "60", "--spinup", "4", "--no-cpu", "--full"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dist_backend"] == "gloo" and d["launched_by"] == "bench.py"
    assert len(d["per_rank_ms_per_step"]) == 2 and all(x > 0 for x in d["per_rank_ms_per_step"])
    ranks = d["parity_checked_ranks"]
    assert len(ranks) == 2
    for p in ranks:
        assert p["max_lsb"] == 0 and p["packets_compared"] > 0 and p["steps_replayed"] >= 60 + 2 + 4 + 6
    # whole-job aggregate over both ranks
    assert d["value"] > 0 and d["config"]["streams_per_gpu"] == 512


def test_rccl_itself_under_the_multi_rank_code_path():
    """backend nccl = RCCL under the same calls (process group on the rank's device, the far-end broadcast as bytes, the
    gathers, the barriers): the driver's launch line with one rank and WMIX_BENCH_FORCE_DIST=1 -- two ranks cannot share a
    device under RCCL, so on a 1-GPU box a group of one is what can be run.  The chain is still checked against the oracle."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(WMIX_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29617", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "chain", "--streams", "512",
                        "--steps", "6", "--warmup", "2", "--prime", "60", "--spinup", "4", "--no-cpu", "--full"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["dist_backend"] == "nccl" and d["rccl_ranks"] == 1 and d["launched_by"] == "torchrun"
    assert "RCCL broadcast" in d["config"]["far_end"]
    assert len(d["parity_checked_ranks"]) == 1 and d["parity_checked_ranks"][0]["max_lsb"] == 0
    assert d["parity_checked_ranks"][0]["packets_compared"] > 0
    # --far-chunk 8: ONE RCCL broadcast per 8 steps, the next chunk in flight while this one computes
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29621", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "chain", "--streams", "512",
                        "--steps", "6", "--warmup", "2", "--prime", "60", "--spinup", "4", "--no-cpu", "--full", "--far-chunk", "8"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert "one collective per 8 step" in d["config"]["far_end"] and d["parity_checked_ranks"][0]["max_lsb"] == 0
    assert d["parity_checked_ranks"][0]["packets_compared"] > 0


def test_one_rank_under_the_launcher_measures_what_the_direct_line_measures():
    """The driver's SCALE run starts N = 1 through torch.distributed.run like every other N; its line must be the direct
    `python bench.py` line (same timed region, same steady state), or the scaling curve's first point is off (round-3 VERDICT).
    Also: the rank's device is its LOCAL_RANK and is reported."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    common = ["--gpus", "1", "--workload", "chain", "--steps", "40", "--warmup", "5", "--no-cpu", "--full"]
    a = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common, env=env, capture_output=True, text=True, timeout=900)
    assert a.returncode == 0, a.stderr[-3000:]
    b = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29619", os.path.join(ROOT, "bench.py")] + common, env=env, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    da = json.loads([l for l in a.stdout.splitlines() if l.startswith("{")][0])
    db = json.loads([l for l in b.stdout.splitlines() if l.startswith("{")][0])
    assert da["launched_by"] == "direct" and db["launched_by"] == "torchrun" and da["n_gpus"] == db["n_gpus"] == 1
    # same box, back to back: run-to-run spread of the step is ~1 %; 5 % is the bound that says "the same measurement"
    assert abs(da["ms_per_step"] - db["ms_per_step"]) / da["ms_per_step"] < 0.05, (da["ms_per_step"], db["ms_per_step"])
    assert da["parity_checked"]["max_lsb"] == 0 and db["parity_checked"]["max_lsb"] == 0
    for d in (da, db):
        assert d["rank_devices"][0]["device"] == d["rank_devices"][0]["local_rank"] == 0 and d["rank_devices"][0]["name"]
