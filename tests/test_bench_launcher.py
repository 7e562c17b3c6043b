"""bench.py's own N > 1 launcher on a CPU-only box: `python bench.py --gpus 2` (no torchrun environment) must start two
rank processes, rendezvous on 127.0.0.1 (gloo here, RCCL on GPUs), exchange the far-end packet every step and print ONE
JSON line with n_gpus = 2 -- VERDICT r01 item 2.  The stub workload has no compute; the plumbing is what is tested."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_gpus_flag_starts_that_many_ranks():
    r = _run(["--gpus", "2", "--workload", "stub_cpu", "--steps", "5", "--warmup", "2", "--prime", "3", "--no-cpu", "--full"])
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["warmup"] == 2
    assert d["dist_backend"] == "gloo" and d["launched_by"] == "bench.py"
    assert len(d["per_rank_ms_per_step"]) == 2
    # rank 0's far-end value reached every step: 1 + 2 + ... + (3 + 2 + 5 + 5 extra breakdown steps)
    assert d["config"]["far_sum"] == sum(range(1, 16))
    assert d["value"] > 0 and d["scaling"] == "weak"


def test_gpus_flag_must_match_world_size():
    r = _run(["--gpus", "4", "--workload", "stub_cpu", "--steps", "1", "--warmup", "0", "--prime", "0", "--no-cpu"],
             {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def test_torchrun_launch_still_works():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29617", os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--workload", "stub_cpu", "--steps", "3", "--warmup", "1", "--prime", "0", "--no-cpu"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["launched_by"] == "torchrun"


def test_a_dead_rank_ends_the_launch_with_its_code():
    """Round-2 ADVICE: a rank that dies must not leave the parent waiting for the survivors' collective timeout."""
    import time
    t0 = time.monotonic()
    r = _run(["--gpus", "2", "--workload", "stub_cpu", "--steps", "5", "--warmup", "2", "--prime", "3", "--no-cpu"],
             {"WMIX_STUB_FAIL_RANK": "1"}, timeout=120)
    assert r.returncode == 7, (r.returncode, r.stderr)
    assert "ranks failed" in r.stderr and "(1, 7)" in r.stderr
    assert time.monotonic() - t0 < 90


def test_eight_ranks_shard_a_non_divisible_stream_count():
    """World size 8 -- what the driver's SCALE run launches and no test had ever started (round-3 VERDICT): 37 streams over 8
    ranks (contiguous ranges, the remainder on the first ranks), the far-end broadcast to all of them every step, EVERY rank's own
    parity record on rank 0's one line, inside a time bound."""
    import time
    t0 = time.monotonic()
    r = _run(["--gpus", "8", "--workload", "stub_cpu", "--total-streams", "37", "--steps", "6", "--warmup", "2", "--prime", "4", "--no-cpu",
              "--full"], timeout=300)
    took = time.monotonic() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["dist_backend"] == "gloo" and d["scaling"] == "strong" and d["total_streams"] == 37
    assert d["per_rank_frames_per_step"] == [5, 5, 5, 5, 5, 4, 4, 4] and len(d["per_rank_ms_per_step"]) == 8
    ranks = d["parity_checked_ranks"]
    assert len(ranks) == 8 and all(p["max_lsb"] == 0 and p["packets_compared"] > 0 for p in ranks)
    # the ranges tile [0, 37) in rank order
    edges = [p["range"] for p in ranks]
    assert edges[0][0] == 0 and edges[-1][1] == 37 and all(a[1] == b[0] for a, b in zip(edges[:-1], edges[1:]))
    # whole-job aggregate: 37 streams x 6 steps over the slowest rank's time
    assert abs(d["value"] - 37 * 6 / (d["ms_per_step"] * 6e-3)) / d["value"] < 1e-6
    assert took < 240, took


def test_eight_ranks_far_end_in_chunks():
    """--far-chunk K (round-4 VERDICT "next" 6; SURVEY section 5: one broadcast per batch of K frames): rank 0 sends the far-end of K
    steps with ONE collective; every stream of every rank still hears every packet, in order, for K = 1, 8 and a K beyond the
    whole run.  18 steps in all (4 priming + 2 warm-up + 6 timed + 6 breakdown)."""
    import pytest
    for K, want_bcast in ((1, 18), (8, 3), (100, 1)):
        r = _run(["--gpus", "8", "--workload", "stub_cpu", "--total-streams", "37", "--steps", "6", "--warmup", "2", "--prime", "4", "--no-cpu",
                  "--full", "--far-chunk", str(K)], timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert d["n_gpus"] == 8 and d["config"]["far_chunk"] == K and d["config"]["broadcasts"] == want_bcast
        assert d["config"]["far_sum"] == sum(range(1, 19))
        ranks = d["parity_checked_ranks"]
        assert len(ranks) == 8 and all(p["max_lsb"] == 0 and p["packets_compared"] > 0 for p in ranks), K


def test_eight_ranks_under_the_drivers_own_launch_line():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8",
                        "--master-addr", "127.0.0.1", "--master-port", "29631", os.path.join(ROOT, "bench.py"), "--gpus", "8",
                        "--workload", "stub_cpu", "--steps", "3", "--warmup", "1", "--prime", "0", "--no-cpu", "--full"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 8 and d["launched_by"] == "torchrun" and d["scaling"] == "weak"
    assert d["per_rank_frames_per_step"] == [4] * 8 and len(d["parity_checked_ranks"]) == 8


def test_a_rank_without_streams_is_refused():
    r = _run(["--gpus", "4", "--workload", "stub_cpu", "--total-streams", "3", "--steps", "1", "--warmup", "0", "--prime", "0", "--no-cpu"],
             timeout=120)
    assert r.returncode != 0 and "without a stream" in r.stderr


def test_rank_stdout_is_kept_and_shown_when_the_launch_fails():
    r = _run(["--gpus", "2", "--workload", "stub_cpu", "--steps", "2", "--warmup", "0", "--prime", "0", "--no-cpu"],
             {"WMIX_STUB_FAIL_RANK": "1", "WMIX_STUB_CHATTER": "1"}, timeout=120)
    assert r.returncode == 7 and "---- stdout of rank 1 ----" in r.stderr and "stub rank 1 says hello" in r.stderr


def test_a_plain_run_times_its_steps_and_nothing_more(tmp_path):
    """Without --full the line carries the headline figure alone: no breakdown steps, no parity replay, no CPU baseline.
    --dump-outputs writes what the last timed step left for the caller, and the same arguments write the same arrays."""
    import numpy as np
    got = []
    for i in range(2):
        d = tmp_path / str(i)
        r = _run(["--gpus", "2", "--workload", "stub_cpu", "--steps", "5", "--warmup", "2", "--prime", "3", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
        assert not {"parity_checked", "parity_checked_ranks", "stage_ms"} & set(line)
        # 3 priming + 2 warm-up + 5 timed steps, not one more
        assert line["config"]["far_sum"] == sum(range(1, 11)) and line["config"]["broadcasts"] == 10
        got.append(np.load(d / "acc.npy"))
    # rank 0's stream s added the far-end of every step (1 .. 10) and its global id s % 5 once per step
    want = sum(range(1, 11)) + 10 * np.arange(4)[:, None] + np.zeros((1, 160))
    assert got[0].dtype == np.float64 and np.array_equal(got[0], want) and np.array_equal(got[0], got[1])


def test_dump_outputs_stays_within_64_mb_with_a_fixed_sample(tmp_path):
    """Outputs larger than the dump's budget (the G.711 line's 2^20 frames) keep the same seeded rows on every run."""
    import importlib.util

    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    g = torch.Generator().manual_seed(3)
    big = {"codes": torch.randint(0, 256, (1 << 20, 80), dtype=torch.uint8, generator=g),
           "decoded": torch.randint(-32768, 32768, (1 << 20, 80), dtype=torch.int16, generator=g)}
    for d in ("a", "b"):
        b._dump_outputs(big, str(tmp_path / d))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 * 10 ** 6
    a, c = np.load(tmp_path / "a" / "decoded.npy"), np.load(tmp_path / "b" / "decoded.npy")
    assert a.dtype == np.float32 and a.shape[1] == 80 and 0 < a.shape[0] < 1 << 20 and np.array_equal(a, c)
    # the sampled rows are input rows, in input order
    rows = {bytes(r) for r in big["decoded"].numpy()}
    assert all(bytes(r.astype(np.int16)) in rows for r in a[:64])
