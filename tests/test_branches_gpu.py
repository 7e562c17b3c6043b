"""GPU parity on the catalogue of tests/branch_inputs.py: inputs chosen for the branches of the reference that the suite's other
signals never take (quiet and fading levels, level steps against the 500-block model windows, output that saturates on both sides,
start-up with a jumping reported delay, reported delays below 0 and above 500 ms, ...).  One test per stage and configuration
group: the group's entries ride as the streams of one batch (entries with different far ends get a far-end group of their own where
the stage has them; entries with different delay schedules never share a batch), 7 packets per launch so that launch boundaries fall
inside the events, every stream against its own per-handle oracle run.  Integer stages: bit for bit.  Float AEC: check_float_path
(0 differing samples on a host whose powf is the product's).  tests/test_oracle_extremes.py holds the oracle to the real reference
on the same entries."""
import numpy as np
import pytest

import branch_inputs as B

pytestmark = pytest.mark.gpu
PER_LAUNCH = 7


def _config(e):
    if e.stage in ("aec", "aecm"):
        # one batch = one handle configuration and ONE schedule of reported delays (which depends on the length); the fixed-point
        # canceller's batch has one far end
        return (e.stage, e.chn, e.freq, e.interval, e.schedule, e.n) + ((e.far,) if e.stage == "aecm" else ())
    if e.stage == "agc":
        return (e.stage, e.chn, e.freq, e.value)
    if e.stage == "vad":
        return (e.stage, e.chn, e.freq, e.interval)
    return (e.stage, e.chn, e.freq)


GROUPS = {}
for _e in B.CATALOGUE:
    GROUPS.setdefault(_config(_e), []).append(_e)
assert all(len(g) <= 32 and max(e.n for e in g) <= 1500 for g in GROUPS.values())


def _padded(rows):
    """streams of one batch have one length: shorter entries are followed by digital silence (every stage is causal, so the entry's own
    packets come out as they would alone; only those are compared)"""
    out = np.zeros((len(rows), max(r.size for r in rows)), np.int16)
    for i, r in enumerate(rows):
        out[i, :r.size] = r
    return out


def _gpu_canceller_calls(cuda, stage, e0, fars, stream_far, near, delays):
    """aec_process2 call by call with the reported delay of each call: launches of up to PER_LAUNCH calls that report the same delay;
    a call whose delay lies outside [0, 500] ms is a launch of its own, which must return -1, leave its output unwritten and still
    move the state (src/webrtc.c:382-387).  Returns (outputs [S, N], return code per call)."""
    import torch
    if stage == "aec":
        from wmix_amd.aec import AecBatch
        ab = AecBatch(near.shape[0], e0.chn, e0.freq, e0.interval, stream_far=stream_far if fars.shape[0] > 1 else None)
    else:
        from wmix_amd.aecm import AecmBatch
        assert fars.shape[0] == 1
        ab = AecmBatch(near.shape[0], e0.chn, e0.freq, e0.interval)
    S, n = near.shape[0], delays.size
    dfar = torch.from_numpy(np.ascontiguousarray(fars.reshape(fars.shape[0], n, ab.pkt))).to(cuda)
    if fars.shape[0] == 1:
        dfar = dfar[0]
    d = torch.from_numpy(np.ascontiguousarray(near.reshape(S, n, ab.pkt))).to(cuda)
    rcs = np.zeros(n, np.int32)
    c = 0
    while c < n:
        r = 1
        if 0 <= delays[c] <= 500:
            while c + r < n and r < PER_LAUNCH - c % PER_LAUNCH and delays[c + r] == delays[c]:
                r += 1
        rc, _ = ab.process2(dfar[..., c:c + r, :], d[:, c:c + r], delay_ms=int(delays[c]))
        rcs[c:c + r] = rc
        c += r
    out = d.cpu().numpy().reshape(S, -1)
    ab.close()
    return out, rcs


@pytest.mark.parametrize("key", sorted(GROUPS), ids=lambda k: "-".join(str(x) for x in k))
def test_catalogue_group_vs_per_handle_oracle(cuda, oracle_port, key):
    from test_aec_gpu import check_float_path, gpu_aec
    from test_aecm_gpu import run_gpu as gpu_aecm
    from test_ns_gpu import run_gpu as gpu_ns
    from test_nsx_gpu import run_gpu as gpu_nsx
    from test_vadagc_gpu import gpu_agc, gpu_vad
    group, stage = GROUPS[key], key[0]
    e0 = group[0]
    data = [B.make(e) for e in group]
    want = [B.run(oracle_port, e, "orc", data=dt) for e, dt in zip(group, data)]
    near = _padded([dt[1] for dt in data])
    want_rcs = None
    if stage == "ns":
        got = gpu_ns(cuda, e0.chn, e0.freq, near.copy(), packets_per_launch=PER_LAUNCH)
    elif stage == "nsx":
        got = gpu_nsx(cuda, e0.chn, e0.freq, near.copy(), packets_per_launch=PER_LAUNCH)
    elif stage == "agc":
        got = gpu_agc(cuda, e0.chn, e0.freq, e0.value, near.copy(), packets_per_launch=PER_LAUNCH)
    elif stage == "vad":
        got = gpu_vad(cuda, e0.chn, e0.freq, e0.interval, 1, near.copy(), calls_per_launch=PER_LAUNCH)
    else:
        delays = data[0][2]
        assert all(np.array_equal(dt[2], delays) for dt in data)
        far_names = sorted({e.far for e in group})
        fars = np.stack([next(dt[0] for e, dt in zip(group, data) if e.far == f) for f in far_names])
        stream_far = np.array([far_names.index(e.far) for e in group], np.int32)
        want_rcs = want[0][1]
        assert all(np.array_equal(w[1], want_rcs) for w in want)  # the code depends on the reported delay alone
        if (want_rcs == 0).all() and (delays == delays[0]).all() and len(far_names) == 1:
            if stage == "aec":
                got = gpu_aec(cuda, e0.chn, e0.freq, e0.interval, int(delays[0]), fars[0], near.copy(), pkts_per_launch=PER_LAUNCH)
            else:
                got, rc = gpu_aecm(cuda, e0.chn, e0.freq, e0.interval, fars[0], near.copy(), delay=int(delays[0]), packets_per_launch=PER_LAUNCH)
                assert rc == 0
        else:
            got, rcs = _gpu_canceller_calls(cuda, stage, e0, fars, stream_far, near.copy(), delays)
            assert np.array_equal(rcs, want_rcs), "return codes differ at calls %r" % np.flatnonzero(rcs != want_rcs)[:8].tolist()
    for i, (e, (w, _)) in enumerate(zip(group, want)):
        g = got[i, :w.size]
        if stage == "aec":
            check_float_path(g, w)
        else:
            d = np.flatnonzero(g != w)
            assert d.size == 0, "%s: %d of %d samples differ, first at sample %d (packet %d)" % (e.name, d.size, w.size, d[0], d[0] // (B.packet(e) * e.chn))
