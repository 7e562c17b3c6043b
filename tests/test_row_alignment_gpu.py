"""Rows that are not 16-byte aligned: wmx_vad_process and wmx_agc_process choose their kernel from the geometry of the rows they
are given (wmix_amd/csrc/vad.hip, agc.hip: the four-wave pipelines want both strides % 8 == 0 and the pointers % 16 == 0, everything
else goes to the one-lane kernels; inside vad_kernel a register path with 16-byte accesses makes the same choice again).  Every other
test hands them fresh allocations with strides that are multiples of eight samples.  Here the same streams go through seven
geometries of one flat, sentinel-filled buffer -- a caller's 2-byte header in front of the rows, a ring of odd slot sizes -- stream-major
and packet-major, and through wmx_chain_process and a PCM pipe on such rows; every stream against its own per-handle oracle run,
np.array_equal; the bytes between the rows keep the sentinel after every launch; the exported state after the aligned and the
most crooked geometry is the same, byte for byte.

70 streams (one full 64-stream block and one with six live lanes), 96 calls in launches of 37, 37 and 22."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import loader as L

sys.path.insert(0, GOLDEN)
from make_vadagc_golden import agc_input, agc_pkg, vad_input, vad_pkg  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
S, N, LAUNCHES = 70, 96, (37, 37, 22)
TAIL = 8  # sentinel elements behind the last row
# element offset of the first row, pad behind every row, pad behind every group of rows (a stream's, or packet-major a packet's)
GEO = {"g0": (0, 0, 0),   # the control: the pipelines
       "g1": (8, 8, 8),   # every row at another multiple of 16 bytes: still the pipelines
       "g2": (1, 0, 0),   # pointer at 2 mod 16
       "g3": (4, 0, 0),   # pointer at 8 mod 16: 8-byte aligned, not 16
       "g4": (0, 4, 0),   # stride at 8 mod 16: every other row off
       "g5": (0, 0, 1),   # only the odd groups' rows are off: stream 0 looks aligned
       "g6": (3, 5, 7)}   # all at once
VAD_SHAPES = [(1, 8000, 10, 1),    # 80-sample packet: the register paths
              (1, 16000, 10, 1),   # 160-sample packet, the chain's own shape: the register paths
              (1, 16000, 20, 1),   # 320-sample packet: the memory paths
              (1, 32000, 10, 1),   # ratio 4
              (2, 16000, 10, 1),   # the two-channel pipeline
              (1, 8000, 20, 2),    # only the first packet of a call may change
              (2, 16000, 10, 2),   # always one-lane: the whole-call down-mix and expansion
              (3, 16000, 10, 1)]   # always one-lane
AGC_SHAPES = [(1, 8000), (1, 16000), (1, 32000), (2, 16000), (3, 16000)]
AGC_GAIN = 9
AGC_OWN_GAINS = {5: 20, 40: 3, 67: 30}  # stream -> agc_init's value; 67 sits in the ragged block


def geometry(geo, row, packet_major):
    """-> element offset, stream stride, packet stride, buffer elements"""
    off, pad_row, pad_group = GEO[geo]
    if packet_major:
        ss = row + pad_row
        ps = S * ss + pad_group
    else:
        ps = row + pad_row
        ss = N * ps + pad_group
    return off, ss, ps, off + (S - 1) * ss + (N - 1) * ps + row + TAIL


class Rows:
    """One flat int16 device buffer full of the sentinel with the rows [S, N, row] of a geometry in it."""

    def __init__(self, cuda, geo, row, packet_major, x=None):
        import torch
        self.off, self.ss, self.ps, n_el = geometry(geo, row, packet_major)
        self.packet_major, self.row = packet_major, row
        self.buf = torch.full((n_el,), SENTINEL, dtype=torch.int16, device=cuda)
        assert self.buf.data_ptr() % 16 == 0, "the allocator's own pointer is not 16-byte aligned: the geometries mean nothing"
        self.rows = torch.as_strided(self.buf, (S, N, row), (self.ss, self.ps, 1), self.off)
        self.outside = torch.ones(n_el, dtype=torch.bool, device=cuda)
        torch.as_strided(self.outside, (S, N, row), (self.ss, self.ps, 1), self.off).fill_(False)
        assert int(self.outside.sum()) == n_el - S * N * row  # (the rows do not overlap)
        if x is not None:
            self.rows.copy_(x)
        self.before = self.buf.clone()

    def launch_view(self, c0, c1):
        """calls c0 .. c1 in the shape the batch classes take: [S, n, row], or packet-major [n, S, row]"""
        v = self.rows[:, c0:c1]
        return v.permute(1, 0, 2) if self.packet_major else v

    def sentinel_intact(self):
        return bool((self.buf[self.outside] == SENTINEL).all())

    def unchanged(self):
        import torch
        return torch.equal(self.buf, self.before)

    def host(self):
        return self.rows.cpu().numpy().reshape(S, -1)


def square_wave(frames, chn):
    """full scale, 32767 / -32768, half a period of four frames, the same in every channel"""
    return np.repeat(np.where(np.arange(frames) // 4 % 2 == 0, 32767, -32768).astype(np.int16), chn)


_REF = {}


def vad_reference(port, shape):
    """-> input [S, samples], the oracle's output per stream; made once per shape"""
    if ("vad", shape) not in _REF:
        chn, freq, ims, k = shape
        x = np.stack([vad_input(chn, freq, ims, k, n_calls=N, seed=2100 + 7 * s) for s in range(S)])
        x[3] = 0
        x[4] = square_wave(x.shape[1] // chn, chn)
        want = np.stack([L.run_vad(port, chn, freq, ims, x[s], k * vad_pkg(freq, ims), prefix="orc") for s in range(S)])
        _REF["vad", shape] = (x, want)
    return _REF["vad", shape]


def agc_reference(port, shape, own_gains):
    if ("agc", shape, own_gains) not in _REF:
        chn, freq = shape
        x = np.stack([agc_input(chn, freq, n_calls=N, seed=2300 + 11 * s) for s in range(S)])
        x[3] = 0
        x[4] = square_wave(x.shape[1] // chn, chn)
        if not own_gains:
            want = np.stack([L.run_agc(port, chn, freq, AGC_GAIN, x[s], agc_pkg(freq), prefix="orc") for s in range(S)])
        else:
            want = agc_reference(port, shape, False)[1].copy()
            for s, v in AGC_OWN_GAINS.items():
                want[s] = L.run_agc_handle(port, chn, freq, v, x[s], agc_pkg(freq), prefix="orc")
                assert not np.array_equal(want[s], agc_reference(port, shape, False)[1][s])  # (the gain of its own is audible)
        _REF["agc", shape, own_gains] = (x, want)
    return _REF["agc", shape, own_gains]


def streams_changed(x, want):
    return int((x != want).any(axis=1).sum())


def vad_shifts_seen(x, want, row, pkt):
    """The attenuation shifts 0 .. 4 that some call of some stream shows beyond doubt (mono: out = in >> shift on the call's first
    packet): a shift counts when it is the only one of the five that explains the packet."""
    seen = set()
    a = x.reshape(S, N, row)[:, :, :pkt].astype(np.int32)
    b = want.reshape(S, N, row)[:, :, :pkt].astype(np.int32)
    fits = np.stack([((a >> r) == b).all(axis=2) for r in range(5)])  # [5, S, N]
    only = fits.sum(axis=0) == 1
    for r in range(5):
        if (fits[r] & only).any():
            seen.add(r)
    return seen


_DEV_IN = {}


def device_input(cuda, key, x, row):
    import torch
    if key not in _DEV_IN:
        _DEV_IN[key] = torch.from_numpy(np.ascontiguousarray(x.reshape(S, N, row))).to(cuda)
    return _DEV_IN[key]


_EXPORTS = {}


def run_vad(cuda, port, shape, geo, packet_major):
    """The shape's streams through VadBatch on the rows of one geometry.  -> output [S, samples], whether the sentinel survived each
    launch, the exported state of every stream."""
    from wmix_amd.vad import VadBatch
    chn, freq, ims, k = shape
    x, _ = vad_reference(port, shape)
    vb = VadBatch(S, chn, freq, ims)
    row = k * vb.pkt  # a call's packets in one piece; the pad goes behind the call
    r = Rows(cuda, geo, row, packet_major, device_input(cuda, ("vad", shape), x, row))
    intact, c = [], 0
    for n in LAUNCHES:
        v = r.launch_view(c, c + n)
        (vb.process_packet_major if packet_major else vb.process)(v, k)
        intact.append(r.sentinel_intact())
        c += n
    got = r.host()
    blobs = [vb.export_stream(s).tobytes() for s in range(S)]
    vb.close()
    _EXPORTS["vad", shape, geo, packet_major] = blobs
    return got, intact, blobs


def vad_cases():
    for shape in VAD_SHAPES:
        for geo in GEO:
            for packet_major in (False, True):
                if packet_major and shape[3] > 1:
                    continue  # a call's packets in one piece per stream
                yield pytest.param(shape, geo, packet_major, id="%dx%d_%dms_k%d-%s-%s" % (shape + (geo, "packet_major" if packet_major else "stream_major")))


@pytest.mark.parametrize("shape,geo,packet_major", list(vad_cases()))
def test_vad_rows_of_every_geometry(cuda, oracle_port, shape, geo, packet_major):
    chn, freq, ims, k = shape
    x, want = vad_reference(oracle_port, shape)
    # not a vacuous comparison, by the oracle alone: the gate moved the samples of most streams, and the mono shapes were in every
    # attenuation 0 .. 4
    assert streams_changed(x, want) >= S // 2
    if chn == 1:
        pkt = vad_pkg(freq, ims)
        assert vad_shifts_seen(x, want, k * pkt, pkt) == {0, 1, 2, 3, 4}
    got, intact, _ = run_vad(cuda, oracle_port, shape, geo, packet_major)
    assert all(intact), ("written outside the rows, per launch:", intact)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, ("streams that differ from the oracle:", bad[:16], "first sample:", int(np.flatnonzero(got[bad[0]] != want[bad[0]])[0]))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape,packet_major", [pytest.param(sh, pm, id="%dx%d_%dms_k%d-%s" % (sh + ("packet_major" if pm else "stream_major",)))
                                                for sh in VAD_SHAPES for pm in (False, True) if not (pm and sh[3] > 1)])
def test_vad_state_is_the_same_through_either_kernel(cuda, oracle_port, shape, packet_major):
    """The same history through the aligned rows (g0) and the most crooked ones (g6) leaves the same state, not only the same audio."""
    blobs = {}
    for geo in ("g0", "g6"):
        key = ("vad", shape, geo, packet_major)
        blobs[geo] = _EXPORTS[key] if key in _EXPORTS else run_vad(cuda, oracle_port, shape, geo, packet_major)[2]
    assert len(blobs["g0"][0]) > 100  # (a blob of the state's size, not a header)
    diff = [s for s in range(S) if blobs["g0"][s] != blobs["g6"][s]]
    assert diff == []
    assert blobs["g0"][0] != blobs["g0"][1]  # (states of two streams with different input do differ)


def run_agc(cuda, port, shape, geo_in, geo_out, packet_major, own_gains):
    """geo_out None: in place.  -> output [S, samples], per launch whether the sentinel of the output buffer survived and the input
    buffer is byte for byte what it was (out of place), the exported state of every stream."""
    from wmix_amd.agc import AgcBatch
    chn, freq = shape
    x, _ = agc_reference(port, shape, own_gains)
    ab = AgcBatch(S, chn, freq, AGC_GAIN)
    for s, v in AGC_OWN_GAINS.items() if own_gains else ():
        ab.reset_streams_gain([s], v)
    d_x = device_input(cuda, ("agc", shape), x, ab.pkt)
    rin = Rows(cuda, geo_in, ab.pkt, packet_major, d_x)
    rout = rin if geo_out is None else Rows(cuda, geo_out, ab.pkt, packet_major)
    intact, c = [], 0
    for n in LAUNCHES:
        vi, vo = rin.launch_view(c, c + n), rout.launch_view(c, c + n)
        (ab.process_packet_major if packet_major else ab.process)(vi, None if geo_out is None else vo)
        intact.append(rout.sentinel_intact() and (geo_out is None or rin.unchanged()))
        c += n
    got = rout.host()
    blobs = [ab.export_stream(s).tobytes() for s in range(S)]
    ab.close()
    _EXPORTS["agc", shape, geo_in, geo_out, packet_major, own_gains] = blobs
    return got, intact, blobs


def agc_cases():
    for shape in AGC_SHAPES:
        for own_gains in (False, True):
            for packet_major in (False, True):
                pairs = [(g, None) for g in GEO] + [(g, g) for g in GEO] + [("g0", "g2"), ("g2", "g0")]  # either one alone: one-lane
                for gi, go in pairs:
                    yield pytest.param(shape, gi, go, packet_major, own_gains,
                                       id="%dx%d-%s-%s-%s-%s" % (shape + (gi, "in_place" if go is None else "to_" + go,
                                                                          "packet_major" if packet_major else "stream_major",
                                                                          "own_gains" if own_gains else "one_gain")))


@pytest.mark.parametrize("shape,geo_in,geo_out,packet_major,own_gains", list(agc_cases()))
def test_agc_rows_of_every_geometry(cuda, oracle_port, shape, geo_in, geo_out, packet_major, own_gains):
    x, want = agc_reference(oracle_port, shape, own_gains)
    assert streams_changed(x, want) >= S // 2  # not a vacuous comparison, by the oracle alone
    got, intact, _ = run_agc(cuda, oracle_port, shape, geo_in, geo_out, packet_major, own_gains)
    assert all(intact), ("written outside the output rows, or the input changed, per launch:", intact)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, ("streams that differ from the oracle:", bad[:16], "first sample:", int(np.flatnonzero(got[bad[0]] != want[bad[0]])[0]))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("own_gains", [False, True], ids=["one_gain", "own_gains"])
@pytest.mark.parametrize("packet_major", [False, True], ids=["stream_major", "packet_major"])
@pytest.mark.parametrize("shape", AGC_SHAPES, ids=lambda s: "%dx%d" % s)
def test_agc_state_is_the_same_through_either_kernel(cuda, oracle_port, shape, packet_major, own_gains, in_place):
    blobs = {}
    for geo in ("g0", "g6"):
        key = ("agc", shape, geo, None if in_place else geo, packet_major, own_gains)
        blobs[geo] = _EXPORTS[key] if key in _EXPORTS else run_agc(cuda, oracle_port, shape, *key[2:])[2]
    assert len(blobs["g0"][0]) > 60
    diff = [s for s in range(S) if blobs["g0"][s] != blobs["g6"][s]]
    assert diff == []
    assert blobs["g0"][0] != blobs["g0"][1]


# ---- wmx_chain_process on such rows: its tail stages get them as they are (tools_dev/fuzz_parity.py: run_case with explicit fields)
NS, AEC, AGC, VAD, NSX, AECM = 1, 2, 4, 8, 16, 32
CHAINS = {"ns_aec_agc_vad_1x16000": dict(stages=NS | AEC | AGC | VAD, chn=1, freq=16000, interval_ms=10, packets_per_call=1),
          "nsx_aecm_agc_vad_1x8000": dict(stages=NS | NSX | AEC | AECM | AGC | VAD, chn=1, freq=8000, interval_ms=10, packets_per_call=2),
          "ns_agc_vad_2x32000": dict(stages=NS | AGC | VAD, chn=2, freq=32000, interval_ms=10, packets_per_call=1),
          "agc_vad_1x16000_20ms": dict(stages=AGC | VAD, chn=1, freq=16000, interval_ms=20, packets_per_call=2)}
_CHAIN_WANT = {}


def fuzz_module():
    sys.path.insert(0, os.path.join(ROOT, "tools_dev"))
    import fuzz_parity as F
    return F


def chain_cases():
    layouts = ("stream rows, padded per call", "tick-major: [call][stream][packets]", "packet-major: [packet][stream]", "stream rows, padded per packet")
    for name, c in CHAINS.items():
        in_one_piece = c["interval_ms"] == 20 or (c["chn"] == 2 and bool(c["stages"] & VAD))  # as draw() has it
        for li, lay in enumerate(layouts[:2] if in_one_piece else layouts):
            for pad, offset in ((4, 0), (0, 2), (5, 3)):
                for in_place in (True, False):
                    yield pytest.param(name, lay, pad, offset, in_place, id="%s-layout%d-pad%d-off%d-%s" % (name, li, pad, offset, "in_place" if in_place else "out_of_place"))


@pytest.mark.parametrize("name,layout,pad,offset,in_place", list(chain_cases()))
def test_chain_on_rows_off_the_16_byte_grid(cuda, oracle_port, name, layout, pad, offset, in_place):
    F = fuzz_module()
    assert layout in F.LAYOUTS
    c = F.draw(np.random.default_rng(1))  # draw()'s dictionary, every field that matters set here
    c.update(CHAINS[name], streams=S, calls=30, layout=layout, pad=pad, offset=offset, pad_fill=SENTINEL, in_place=in_place,
             agc_value=9, delay_ms=0, all_streams=True)
    bad, pad_ok = F.run_case(c, cuda, oracle_port, 91000 + 13 * list(CHAINS).index(name), want_cache=_CHAIN_WANT.setdefault(name, {}))
    assert bad == 0 and pad_ok, c
    assert c["samples_the_chain_changed"] > 0, c


def test_pcm_pipe_on_rows_two_bytes_apart_from_the_grid(cuda, oracle_port, wmx):
    """wmx_pipe_step_resident only asks a PCM pipe for even strides: with in_stride = out_stride = row bytes + 2 the chain's tail
    stages get rows at every even offset from the 16-byte grid.  70 streams, 20 ticks, in place, against the oracle's chain."""
    import torch
    from wmix_amd import synth
    from wmix_amd._lib import check
    from wmix_amd.pipeline import PcmChain
    freq, T, pkg = 16000, 20, 160
    far = synth.far_end(9300, T, pkg)
    near = synth.near_end(9301, S, T, pkg, far=far).reshape(S, -1)
    want = np.stack([L.run_chain(oracle_port, 1, freq, 5, 15, far, near[s], pkg, prefix="orc", interval_ms=10) for s in range(S)])
    assert streams_changed(near, want) >= S // 2
    stride = pkg + 1  # int16 elements: row bytes + 2
    n_el = T * S * stride + TAIL
    buf = torch.full((n_el,), SENTINEL, dtype=torch.int16, device=cuda)
    assert buf.data_ptr() % 16 == 0
    rows = torch.as_strided(buf, (T, S, pkg), (S * stride, stride, 1), 0)
    rows.copy_(torch.from_numpy(np.ascontiguousarray(near.reshape(S, T, pkg).transpose(1, 0, 2))).to(cuda))
    outside = torch.ones(n_el, dtype=torch.bool, device=cuda)
    torch.as_strided(outside, (T, S, pkg), (S * stride, stride, 1), 0).fill_(False)
    dfar = torch.from_numpy(far.reshape(T, 1, pkg).copy()).to(cuda)
    ch = PcmChain(S, cuda, 1, freq, 10, 5, 15)
    assert wmx.wmx_pipe_datagram_bytes(ch._h) == 2 * pkg
    assert rows[0, 1].data_ptr() % 16 == 2
    for t in range(T):
        check(wmx.wmx_pipe_step_resident(ch._h, rows[t].data_ptr(), 2 * stride, dfar[t].data_ptr(), rows[t].data_ptr(), 2 * stride,
                                         torch.cuda.current_stream().cuda_stream), "wmx_pipe_step_resident")
    got = rows.cpu().numpy().transpose(1, 0, 2).reshape(S, -1)
    ch.close()
    assert bool((buf[outside] == SENTINEL).all())
    assert np.array_equal(got, want)
