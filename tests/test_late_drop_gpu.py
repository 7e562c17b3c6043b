"""Late ticks of the paced heartbeat (wmx_rt_try_submit, examples/host_paced.c --late drop): a tick released while its group's previous one
is still on its way is shed whole -- nothing moves and no stream's state advances, so every stream equals an oracle handle fed the same
packages minus the dropped ones (the reference's receiver loads nothing for a packet it never got, src/wmixTask.c:1278-1316).  Past
capacity the default queues and falls behind for good; the drop policy holds the latency to about one tick.  And the slot rule both rest
on: a submit retires its slot on every sub-batch before sub-batch 0 uploads a far-end from host memory that the others read."""
import json
import os
import subprocess
import time

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import loader as L
from wmix_amd import synth

pytestmark = pytest.mark.gpu

HOST = os.path.join(ROOT, "examples", "host_paced")


def _same(kind, got, want):
    if kind == "rtp":
        assert np.array_equal(got, want)
    else:
        from test_aec_gpu import check_float_path
        check_float_path(got, want)


class _Case:
    """n distinct ticks of S streams; far-end from host memory.  kind "pcm": 16 kHz 20 ms packages and one shared far-end; "pcm_calls":
    a far-end per stream; "rtp": 172-byte RTP/PCMA datagrams (8 kHz, 20 ms).  The rows of tick t: rows[t] [S, row]."""

    def __init__(self, port, kind, S, n, seed, n_distinct=None):
        self.port, self.kind, self.S, self.n = port, kind, S, n
        D = n_distinct or S  # streams with a signal of their own; stream s plays pattern s % D
        self.D = D
        if kind == "rtp":
            from test_pipeline_gpu import make_datagrams
            far, pk = make_datagrams(port, D, n, seed)
            self.far = far.reshape(n, 160)
            self.rows = np.ascontiguousarray(pk.transpose(1, 0, 2))                            # [n, D, 172]
        elif kind == "pcm":
            far = synth.far_end(seed, n * 2, 160)
            near = synth.near_end(seed + 1, D, n * 2, 160, far=far)
            self.far = far.reshape(n, 320)
            self.rows = np.ascontiguousarray(near.reshape(D, n, 320).transpose(1, 0, 2))      # [n, D, 320]
        else:
            fars = np.stack([synth.far_end(seed + 7 * s, n * 2, 160) for s in range(D)])
            near = np.stack([synth.near_end(seed + 1000 + s, 1, n * 2, 160, far=fars[s])[0] for s in range(D)])
            self.far = np.ascontiguousarray(fars.reshape(D, n, 320).transpose(1, 0, 2))       # [n, D, 320]
            self.rows = np.ascontiguousarray(near.reshape(D, n, 320).transpose(1, 0, 2))
        self.of = np.arange(S) % D

    def rt(self, dev, sub, slots):
        from wmix_amd.realtime import RtBatch
        if self.kind == "rtp":
            return RtBatch(self.S, dev, sub_batch=sub, slots=slots, kind="rtp")
        return RtBatch(self.S, dev, sub_batch=sub, slots=slots, kind="pcm", chn=1, freq=16000, interval_ms=20, far_rows=self.kind == "pcm_calls")

    def fill(self, rt, slot, t, streams=None):
        """tick t's rows (and far-end) into the slot: every stream, or only `streams`"""
        if self.kind == "pcm_calls":
            if streams is None:
                rt.fill_far(slot, self.far[t][self.of])
            for s in streams or ():
                b, r = rt.locate(s)
                rt.h_far_rows[b][slot][r] = self.far[t][self.of[s]]
        else:
            rt.h_far[slot][:] = self.far[t].reshape(rt.far_shape)
        if streams is None:
            rt.fill(slot, self.rows[t][self.of])
        for s in streams or ():
            b, r = rt.locate(s)
            rt.h_in[b][slot][r] = self.rows[t][self.of[s]]

    def oracle(self, s, ticks):
        """stream s fed the packages of `ticks` in that order: its rows [len(ticks), row]"""
        p, ticks = self.of[s], np.asarray(ticks)
        if self.kind == "rtp":
            return L.run_rtp_chain(self.port, np.ascontiguousarray(self.far[ticks]).reshape(-1), np.ascontiguousarray(self.rows[ticks, p]))
        far = self.far[ticks] if self.kind == "pcm" else self.far[ticks, p]
        return L.run_chain(self.port, 1, 16000, 5, 15, np.ascontiguousarray(far).reshape(-1), np.ascontiguousarray(self.rows[ticks, p]).reshape(-1), 320,
                           prefix="orc", interval_ms=20).reshape(len(ticks), -1)


@pytest.mark.parametrize("kind", ["pcm", "pcm_calls", "rtp"])
def test_a_dropped_tick_changes_nothing(cuda, oracle_port, kind):
    """a tick offered right behind one in flight is shed (WMX_DROPPED): the slot it would have taken is still next, the count moves,
    nothing else does -- every stream equals its oracle handle fed the 72 ticks minus the dropped ones"""
    S, n, sub = 13, 72, 4
    c = _Case(oracle_port, kind, S, n, 9900 + len(kind))
    rt = c.rt(cuda, sub, slots=3)
    assert rt.B == 4
    got, kept, drops = {}, [], 0
    pending = None  # (tick, slot) queued, rows not read yet

    def land():
        rt.wait()
        got[pending[0]] = rt.gather(pending[1])

    for t in range(n):
        slot = rt.next_slot
        c.fill(rt, slot, t)
        if t % 6 == 5:  # tick t - 1 is on its way (its last download is not even queued): shed, whatever the device's speed
            assert pending is not None
            before = rt.dropped
            assert rt.try_submit() is False
            assert rt.next_slot == slot and rt.dropped == before + 1 and rt.failed_steps() == 0
            drops += 1
            land()
            pending = None
            continue
        if pending is not None and t % 3 == 0:  # seen landing by the events alone: the same tick offered until it is taken
            rt.poll()  # queues the download still owed
            while not rt.try_submit():
                drops += 1
            got[pending[0]] = rt.gather(pending[1])  # landed (try_submit said so); its slot is not the new tick's
        else:
            if pending is not None:
                land()
            assert rt.try_submit() is True
        assert rt.next_slot == (slot + 1) % 3
        pending = (t, slot)
        kept.append(t)
    if pending is not None:
        land()
    assert rt.dropped == drops and rt.failed_steps() == 0
    rt.close()
    assert len(kept) == n - n // 6
    for s in range(S):
        _same(kind, np.stack([got[t][s] for t in kept]), c.oracle(s, kept))


def test_overload_queue_diverges_drop_holds(cuda, oracle_port):
    """overload by construction: the period is half of one tick.  Queued, every tick starts where the last one ended and the latency
    grows without bound; shed, it stays within two ticks, about every other tick is dropped, and the sampled streams are the oracle's"""
    from wmix_amd.realtime import latency_summary, paced_groups
    S, sub, n = 24576, 8192, 200
    sample = [0, 1, 8191, 8192, 16385, 24575]
    c = _Case(oracle_port, "pcm", S, n, 9950, n_distinct=8)
    # the tick's own time: the 90th percentile of 32 blocking ticks (after 16 more to warm up)
    probe = c.rt(cuda, sub, slots=2)
    c.fill(probe, 0, 0)
    c.fill(probe, 1, 1)
    times = []
    for k in range(48):
        t0 = time.perf_counter()
        probe.tick(None)
        times.append(time.perf_counter() - t0)
    probe.close()
    tick_ms = float(np.percentile(times[16:], 90)) * 1e3
    period = tick_ms / 2

    rq = c.rt(cuda, sub, slots=2)
    lat, lag, _ = paced_groups(lambda g: rq.submit(None), lambda g: rq.poll(), lambda g: rq.wait(), 1, period, n)
    rq.close()
    assert lat[-1] > 50 * period, (lat[-1], period)

    rd = c.rt(cuda, sub, slots=2)
    released = [0]
    slot_of, got = {}, {}

    def try_submit(g):
        t, slot = released[0], rd.next_slot
        released[0] += 1
        c.fill(rd, slot, t, sample)
        if not rd.try_submit():
            return False
        slot_of[t] = slot
        return True

    lat, lag, _ = paced_groups(None, lambda g: rd.poll(), lambda g: rd.wait(), 1, period, n, try_submit=try_submit,
                               after=lambda j, g: got.__setitem__(j, rd.gather(slot_of[j], sample)))
    dropped = np.isnan(lat)
    assert rd.dropped == int(dropped.sum()) and released[0] == n
    rd.close()
    s = latency_summary(lat, lag, period, dropped=dropped)
    assert s["max_ms"] <= 2 * tick_ms and 0.3 * n <= s["dropped"] <= 0.75 * n, (s, tick_ms)
    kept = list(np.flatnonzero(~dropped))
    assert sorted(got) == kept
    for col, st in enumerate(sample):
        _same("pcm", np.stack([got[t][col] for t in kept]), c.oracle(st, kept))


def test_free_running_submits_with_a_host_far_end(cuda, oracle_port):
    """wmx_rt_submit with nobody waiting, a far-end from host memory that differs every tick, 3 sub-batches, 2 slots: tick t + 2's far-end
    must not go up into sub-batch 0's slot while the later sub-batches of tick t still read it.  32 ticks free-running, then 12 waited
    for: a far-end read wrong lives on in the echo canceller's history, and every stream is the oracle's or it is not."""
    S, sub, n, n_free = 49152, 16384, 44, 32
    last = [32768, 40000, 49151]  # the last sub-batch: its download of tick t is queued by the submit of t + 1, so after submit(t + 2)
    sample = [0, 16383, 16384, 24000] + last  # has taken slot t % 2 back, tick t's rows are there until well after the call returns
    c = _Case(oracle_port, "pcm", S, n, 9970, n_distinct=8)
    rt = c.rt(cuda, sub, slots=2)
    assert rt.B == 3
    got = {}
    for t in range(n_free):  # the far-end and the sampled rows only: a host that writes fast runs right behind the device
        c.fill(rt, t % 2, t, sample)
        assert rt.submit(None) == t % 2
        if t >= 2:
            got[t - 2] = rt.gather(t % 2, last)
    rt.wait()
    for t in range(n_free, n):
        c.fill(rt, t % 2, t, sample)
        assert rt.tick(None) == t % 2
        got[t] = rt.gather(t % 2, sample)
    assert rt.failed_steps() == 0
    rt.close()
    for col, st in enumerate(sample):
        want = c.oracle(st, range(n))
        _same("pcm", np.stack([got[t][col] for t in range(n_free, n)]), want[n_free:])
        if st in last:
            _same("pcm", np.stack([got[t][last.index(st)] for t in range(n_free - 2)]), want[:n_free - 2])


def _replay_paced(kind, far, rows, pattern_row, ticks, interval_ms=20):
    """bench.paced_replay for the ticks a stream consumed (tick t works on pattern tick t % slots)"""
    import bench
    port = L.port()
    form, freq = bench.PACED_KINDS[kind]
    t = np.asarray(ticks) % rows.shape[0]
    far_seq = np.ascontiguousarray(far[t] if far.ndim == 2 else far[t, pattern_row % far.shape[1]]).reshape(-1)
    if form == "pcm":
        return L.run_chain(port, 1, freq, 5, 15, far_seq, np.ascontiguousarray(rows[t, pattern_row]).reshape(-1), freq // 100 * (interval_ms // 10),
                           prefix="orc", interval_ms=interval_ms).reshape(len(t), -1)
    return L.run_rtp_chain(port, far_seq, np.ascontiguousarray(rows[t, pattern_row]))


@pytest.mark.parametrize("phases,calls", [(1, 0), (2, 1)])
def test_host_paced_late_drop(cuda, tmp_path, phases, calls):
    """examples/host_paced.c --late drop with a period shorter than a tick: dropped group-ticks are counted and marked NaN, the latency
    stays bounded, and the kept rows of the sampled streams replay through the oracle (every tick a stream consumed, start-up included)"""
    import bench
    assert os.path.exists(HOST), "examples/host_paced is built by __graft_entry__.build()"
    S, sub, slots, ticks, prime, keep, n_pat, tick_ms = 196608, 32768, 4, 200, 60, 24, 64, 3.0
    far, rows = bench.paced_pattern("pcm16k", slots, 20, n_pattern=n_pat, n_far=16 if calls else 1)
    pat = tmp_path / "pattern.bin"
    with open(pat, "wb") as f:
        f.write(np.ascontiguousarray(far).tobytes())
        f.write(np.ascontiguousarray(rows).tobytes())
    sample = [0, 1, 32767, 65536, 98303, 131073, 196607]
    dump, lat, lag = tmp_path / "dump.bin", tmp_path / "lat.f64", tmp_path / "lag.f64"
    cmd = [HOST, "--streams", str(S), "--sub", str(sub), "--slots", str(slots), "--tick-ms", str(tick_ms), "--ticks", str(ticks), "--prime", str(prime),
           "--kind", "pcm", "--freq", "16000", "--interval-ms", "20", "--pattern", str(pat), "--n-pattern", str(n_pat), "--dump", str(dump), "--keep",
           str(keep), "--sample", ",".join(map(str, sample)), "--lat", str(lat), "--lag", str(lag), "--phases", str(phases), "--calls", str(calls),
           "--n-far", "16", "--late", "drop"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["late"] == "drop" and d["rc"] == 0 and d["failed_steps"] == 0 and d["group_ticks"] == ticks * phases
    lat_ms, lag_ms = np.fromfile(lat, np.float64), np.fromfile(lag, np.float64)
    dropped = np.isnan(lat_ms)
    assert np.array_equal(dropped, np.isnan(lag_ms)) and d["dropped"] == int(dropped.sum()) > 0, d
    assert d["max_ms"] == pytest.approx(np.nanmax(lat_ms), abs=1e-3) and abs(np.nanpercentile(lat_ms, 50) - d["p50_ms"]) < 1e-3
    # bounded: queued, 200 ticks at a period shorter than the tick would end hundreds of ms late
    assert d["max_ms"] < 4 * d["p50_ms"] + 5.0 and d["max_ms"] < 100.0, d
    raw = np.fromfile(dump, np.uint8)
    nbytes = keep * len(sample) * rows.shape[2] * 2
    got = raw[:nbytes].view(np.int16).reshape(keep, len(sample), rows.shape[2])
    tick_of = raw[nbytes:].view(np.int32).reshape(keep, len(sample))
    bounds = [S * g // phases for g in range(phases + 1)]
    for col, s in enumerate(sample):
        g = next(q for q in range(phases) if bounds[q] <= s < bounds[q + 1])
        gone = dropped[g::phases]  # the group's ticks in release order
        consumed = list(range(prime)) + [prime + k for k in range(ticks) if not gone[k]]
        last = [prime + k if not gone[k] else -1 for k in range(ticks - keep, ticks)]
        assert list(tick_of[:, col]) == last, (s, list(tick_of[:, col]), last)
        want = _replay_paced("pcm16k", far, rows, s % n_pat, consumed)
        for i, t in enumerate(last):
            if t >= 0:
                assert np.array_equal(got[i, col], want[consumed.index(t)]), (s, t)
