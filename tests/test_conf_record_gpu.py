"""wmx_conf_recorders / _record / _record_stop / _export_record / _step_resident_rec (wmix_amd/csrc/conf.hip; rtp_record_rings_kernel in
rtp.hip) through the Python mirror: what a leg hears, as PCM, against tests/conf_record_replay.py -- the reference's wmix_load_data, its
drain and ONE wmix_pcm_zoom call per package.  Every test asserts two things: the recorded rows equal the replay's sample for sample
(integers, 0 LSB), and the datagrams of the same story with and without recording are byte-identical.

The small stories: 6 legs, max_packets 3, 12 ticks, the layout [[0, 1, 2, 5], [3, 4]]; leg 5 is the RECORDER of the first conference: a
member, muted, never fed.  play_correct is two packages, so that the rows hold audio from the third tick on."""
import numpy as np
import pytest

from conf_duck_replay import plain_duck_story, with_duck
from conf_harness import MODES, bridge
from conf_inputs import G, K, SEED, arrivals
from conf_record_replay import with_recording
from conf_replay_model import ConfReplay
from conf_stories import all_stages, all_stages_floor, all_stages_script
from leg_record_model import Refused

pytestmark = pytest.mark.gpu

N, T6, LAYOUT6, RECORDER = 6, 12, [[0, 1, 2, 5], [3, 4]], 5
ESTATE = -10003
FORMATS = [(1, 8000), (2, 8000), (1, 16000), (2, 44100), (1, 4000)]  # the last: the zoom's shrink branch
RECORD_CALLS = ("recorders", "record", "record_stop")
REPLAYED = {}


# ---------------------------------------------------------------- stories: setup and before as lists of (setter, args, kwargs)
def calls(target, todo, recording):
    """the calls on the handle or the model; recording False: the same story without its recording calls.  ("hook", (f,), {}) hands
    the target to a function of another module's story; ("record_hook", (f,), {}) does the same and counts as a recording call"""
    for name, args, kw in todo:
        if name in ("hook", "record_hook"):
            if recording or name == "hook":
                args[0](target)
        elif recording or name not in RECORD_CALLS:
            getattr(target, name)(*args, **kw)


def small_script(talkers=None):
    pk, recv = arrivals(SEED, T6, N)
    recv[:, RECORDER] = 0  # never fed
    if talkers is not None:
        recv[:, [g for g in range(N) if g not in talkers]] = 0
    return pk, recv


def small_setup(chn, freq, max_taps=3, legs=(RECORDER, 1)):
    mask = np.zeros(N, np.uint8)
    mask[RECORDER] = 1
    todo = [("set_conferences", (LAYOUT6,), {}), ("mute", (mask,), {}), ("set_play_correct", (640,), {}), ("recorders", (max_taps, chn, freq), {})]
    return todo + ([("record", (list(legs),), {"ticks": 0})] if legs else [])


def replayed(lib, key, n, pk, recv, setup, before, base=ConfReplay, **wrong):
    """the story's replay with its recording calls and without them, made once in a session"""
    if key not in REPLAYED:
        both = []
        for recording in (True, False):
            m = with_recording(base, **wrong)(lib, n, recv.shape[2])
            calls(m, setup, recording)
            out = np.zeros((recv.shape[0], n, 172), np.uint8)
            for t in range(recv.shape[0]):
                calls(m, before.get(t, []), recording)
                out[t] = m.tick(pk[t], recv[t])
            both.append((out, m))
        REPLAYED[key] = {"want": both[0][0], "model": both[0][1], "plain": both[1][0], "legs": both[0][1].export_legs()}
    return REPLAYED[key]


# ---------------------------------------------------------------- the handle over a story, with the slots' recorded rows
def run_rec(cb, pk, recv, mode, before, after=None):
    """conf_harness.run with the recorded rows -> (datagrams, per tick the legs per tap, per tick the rows per tap)"""
    import torch
    n_t, n = recv.shape[:2]
    out, legs, rows, queued = np.zeros((n_t, n, 172), np.uint8), [None] * n_t, [None] * n_t, []

    def collect(depth):
        while len(queued) > depth:
            t0, k0 = queued.pop(0)
            cb.wait(k0)
            out[t0] = cb.rows_out[k0]
            if cb.max_taps:
                legs[t0], rows[t0] = (a.copy() for a in cb.recorded(k0))

    for t in range(n_t):
        calls(cb, before.get(t, []), True)
        if mode == "resident":
            d_in = np.zeros((n, recv.shape[2], cb.in_row), np.uint8)
            d_in[:, :, :172] = pk[t]
            d_in, d_recv = torch.from_numpy(d_in).cuda(), torch.from_numpy(recv[t]).cuda()
            if cb.max_taps:
                o, lg, rw = cb.step_resident_rec(d_in, d_recv)
                out[t], legs[t], rows[t] = o.cpu().numpy(), lg.cpu().numpy(), rw.cpu().numpy()
            else:
                out[t] = cb.step_resident(d_in, d_recv).cpu().numpy()
        else:
            k = cb.next_slot()
            cb.rows_in[k][:, :, :172] = pk[t]
            cb.recv[k][:] = recv[t]
            assert cb.submit() == k
            queued.append((t, k))
            collect(1 if mode == "ahead" else 0)
        if after:
            after(t, cb)
    collect(0)
    return out, legs, rows


def handle_over(n, slots, pk, recv, setup, before, mode):
    cb, seen = bridge(n, slots, None, recv.shape[2]), []
    calls(cb, setup, True)
    got = run_rec(cb, pk, recv, mode, before, after=lambda t, c: seen.append(c.export_record()))
    end = cb.export_legs()
    row_bytes = cb.rec_row_bytes
    cb.close()
    return got, seen, end, row_bytes


def rows_equal(got_legs, got_rows, m, ticks):
    """every tap of every tick: the same leg, and where there is a row the replay's samples, all of them; -> the rows compared"""
    compared = 0
    for t in range(ticks):
        assert np.array_equal(got_legs[t], m.rec_legs[t]), ("rec_legs, tick", t, got_legs[t], m.rec_legs[t])
        for i, g in enumerate(m.rec_legs[t]):
            if g >= 0:
                want = m.rec_rows[t][i]
                assert want.size == m.rec_row_samples == got_rows[t].shape[1]
                assert np.array_equal(got_rows[t][i], want), ("tick", t, "tap", i, "leg", g, np.flatnonzero(got_rows[t][i] != want)[:8])
                compared += 1
    return compared


def handle_equals_replay(e, n, slots, pk, recv, setup, before, mode):
    (got, legs, rows), seen, end, row_bytes = handle_over(n, slots, pk, recv, setup, before, mode)
    m = e["model"]
    assert row_bytes == 2 * m.rec_row_samples
    compared = rows_equal(legs, rows, m, recv.shape[0])
    for t in range(recv.shape[0]):
        for field in ("leg", "left", "written"):
            assert np.array_equal(seen[t][field], m.rec_seen[t][field]), (field, "tick", t, seen[t][field], m.rec_seen[t][field])
    assert np.array_equal(got, e["want"]), np.argwhere((got != e["want"]).any(2))[:6]
    assert np.array_equal(e["want"], e["plain"])  # the same story without its recording calls: byte for byte
    for field in ("head", "tick", "dropped", "env", "speaking"):
        assert np.array_equal(end[field], e["legs"][field]), field
    return compared, legs, rows


# ---------------------------------------------------------------- 1. formats
@pytest.mark.parametrize("chn,freq", FORMATS)
def test_formats(cuda, oracle_port, wmx, chn, freq):
    from oracle.loader import mix_zoom
    pk, recv = small_script()
    setup = small_setup(chn, freq)
    e = replayed(oracle_port, ("formats", chn, freq), N, pk, recv, setup, {})
    compared, legs, rows = handle_equals_replay(e, N, 3, pk, recv, setup, {}, "ahead")
    assert compared == 2 * T6
    assert e["model"].rec_row_samples == mix_zoom(oracle_port, 1, 8000, np.zeros(160, np.int16), chn, freq).size
    heard = [int(np.count_nonzero(rows[t][tap])) for t in range(2, T6) for tap in (0, 1)]
    # the recorder hears leg 1 as well: where leg 1 has talked the two rows differ
    assert min(heard) > 0 and sum(not np.array_equal(rows[t][0], rows[t][1]) for t in range(2, T6)) >= 5
    if (chn, freq) == (1, 8000):  # the row is what the leg's datagram of the tick encodes
        for t in range(T6):
            for tap, g in enumerate((RECORDER, 1)):
                assert [wmx.linear2alaw(int(v)) for v in rows[t][tap]] == e["want"][t, g, 12:].tolist(), (t, g)


def test_a_tapped_leg_does_not_hear_itself(cuda, oracle_port):
    """only leg 1 talks: the recorder's rows hold it, leg 1's own rows hold nothing"""
    pk, recv = small_script(talkers=[1])
    setup = small_setup(1, 8000)
    e = replayed(oracle_port, "one talker", N, pk, recv, setup, {})
    compared, legs, rows = handle_equals_replay(e, N, 3, pk, recv, setup, {}, "wait")
    assert compared == 2 * T6
    assert sum(int(np.count_nonzero(rows[t][0])) for t in range(T6)) > 160 and not any(rows[t][1].any() for t in range(T6))


# ---------------------------------------------------------------- 2. lifetime
REFUSALS = []


def third_start(c):
    """both taps are taken: a third start is refused and changes nothing"""
    from wmix_amd._lib import WmxError
    was = c.export_record()
    try:
        c.record([0, 2], ticks=0)
        REFUSALS.append(False)
    except (Refused, WmxError) as err:
        REFUSALS.append(isinstance(err, Refused) or "rc=%d" % ESTATE in str(err))
    now = c.export_record()
    assert all(np.array_equal(now[f], was[f]) for f in was)


def test_lifetime(cuda, oracle_port):
    pk, recv = small_script()
    setup = small_setup(1, 8000, max_taps=2, legs=(1,))  # leg 1: tap 0, until stopped
    before = {2: [("record", ([3],), {"ticks": 4})],       # tap 1, rows in exactly ticks 2 .. 5
              3: [("record_hook", (third_start,), {})],
              7: [("reset_legs", ([1],), {})],             # ends leg 1's tap: tick 7 has no row of it
              8: [("record", ([4, 0],), {"ticks": 0})],    # the freed taps are taken again, the lowest first
              10: [("record_stop", ([4],), {})]}           # stopped mid-story
    REFUSALS.clear()
    e = replayed(oracle_port, "lifetime", N, pk, recv, setup, before)
    compared, legs, rows = handle_equals_replay(e, N, 3, pk, recv, setup, before, "ahead")
    assert REFUSALS == [True, True]  # the model's and the handle's
    m = e["model"]
    assert [int(lg[1]) for lg in legs] == [-1, -1, 3, 3, 3, 3, -1, -1, 0, 0, 0, 0]
    assert [int(lg[0]) for lg in legs] == [1] * 7 + [-1, 4, 4, -1, -1]
    assert m.rec_seen[5]["leg"][1] == -1 and m.rec_seen[5]["written"][1] == 4 and m.rec_seen[5]["left"][1] == 0
    assert m.rec_seen[7]["written"][0] == 0 and m.rec_seen[11]["written"].tolist() == [2, 4]
    assert compared == 7 + 4 + 2 + 4


# ---------------------------------------------------------------- 3. with everything else on
def test_over_the_all_stages_story(cuda, oracle_port):
    """codecs, sequence, conceal, speakers, mutes, a leg that leaves, is reset and joins elsewhere: taps on legs 8, 3 and 1 from the first
    tick; leg 3's ends with its reset_legs at tick 15 (it starts again at 22, for five rows), leg 8's with its reset at tick 30"""
    pk, recv = all_stages_script()
    setup0, before0 = all_stages(all_stages_floor(oracle_port, pk, recv))
    setup = [("hook", (setup0,), {}), ("set_play_correct", (640,), {}), ("recorders", (4, 2, 8000), {}), ("record", ([8, 3, 1],), {"ticks": 0})]
    before = {t: [("hook", (f,), {})] for t, f in before0.items()}
    before[22] = [("record", ([3],), {"ticks": 5})]
    e = replayed(oracle_port, "all stages", G, pk, recv, setup, before)
    compared, legs, rows = handle_equals_replay(e, G, 3, pk, recv, setup, before, "ahead")
    assert [int(lg[0]) for lg in legs] == [8] * 30 + [-1] * 10 and [int(lg[2]) for lg in legs] == [1] * 40
    assert [int(lg[1]) for lg in legs] == [3] * 15 + [-1] * 7 + [3] * 5 + [-1] * 13
    assert compared == 30 + 40 + 15 + 5


def test_over_a_duck_story_the_tap_stands_behind_the_prompts(cuda, oracle_port):
    """tests/conf_duck_replay.py's story: leg 0 plays a ducked prompt from the first tick, leg 1 from tick 25; both are tapped.  The row
    holds the divided conference and the undivided prompt -- the replay's -- and the replay whose taps stand IN FRONT OF the prompts'
    calls records other rows, so the comparison can tell.  play_correct is 0 here: every call lands at the play head, in the very
    package the tick plays, so that WHERE in the tick the tap stands is heard in the row of the same tick"""
    pk, recv, setup0, before0 = plain_duck_story()
    setup = [("hook", (setup0,), {}), ("set_play_correct", (0,), {}), ("recorders", (2, 1, 16000), {}), ("record", ([1, 0],), {"ticks": 0})]
    before = {t: [("hook", (f,), {})] for t, f in before0.items()}
    e = replayed(oracle_port, "duck", G, pk, recv, setup, before, base=with_duck(ConfReplay))
    wrong = replayed(oracle_port, "duck, tap first", G, pk, recv, setup, before, base=with_duck(ConfReplay), tap_first=True)
    compared, legs, rows = handle_equals_replay(e, G, 3, pk, recv, setup, before, "ahead")
    assert compared == 2 * 40 and e["model"].rp.ducked_calls > 20
    assert np.array_equal(wrong["want"], e["want"])  # the datagrams do not depend on where the tap stands; the rows do
    differ = [t for t in range(40) for tap in (0, 1) if not np.array_equal(wrong["model"].rec_rows[t][tap], e["model"].rec_rows[t][tap])]
    assert len(differ) > 10 and any(t >= 25 for t in differ) and any(t < 12 for t in differ)  # leg 1's prompt from tick 25, leg 0's from tick 0
    assert all(not np.array_equal(rows[t][0], wrong["model"].rec_rows[t][0]) or not np.array_equal(rows[t][1], wrong["model"].rec_rows[t][1])
               for t in differ)


# ---------------------------------------------------------------- 4. modes
@pytest.mark.parametrize("slots,mode", MODES)
def test_modes(cuda, oracle_port, slots, mode):
    pk, recv = small_script()
    setup = small_setup(1, 8000)
    e = replayed(oracle_port, ("formats", 1, 8000), N, pk, recv, setup, {})
    compared, _, _ = handle_equals_replay(e, N, slots, pk, recv, setup, {}, mode)
    assert compared == 2 * T6


def test_plain_step_resident_with_a_running_tap_is_refused_and_changes_nothing(cuda, oracle_port, wmx):
    import torch
    pk, recv = small_script()
    setup = small_setup(1, 8000)
    e = replayed(oracle_port, ("formats", 1, 8000), N, pk, recv, setup, {})
    cb = bridge(N, 3, None, K)
    calls(cb, setup, True)
    got, legs, rows = run_rec(cb, pk[:5], recv[:5], "resident", {})
    was = (cb.export_legs(), cb.export_record(), [cb.sender_state(g) for g in range(N)], cb.export_ring(RECORDER))
    d_in = torch.zeros((N, K, cb.in_row), dtype=torch.uint8, device="cuda")
    d_in[:, :, :172] = torch.from_numpy(pk[5]).cuda()
    d_out = torch.zeros((N, 172), dtype=torch.uint8, device="cuda")
    rc = wmx.wmx_conf_step_resident(cb._h, d_in.data_ptr(), torch.from_numpy(recv[5]).cuda().data_ptr(), d_out.data_ptr(), None)
    assert rc == ESTATE and b"wmx_conf_step_resident_rec" in wmx.wmx_last_error()
    now = (cb.export_legs(), cb.export_record(), [cb.sender_state(g) for g in range(N)], cb.export_ring(RECORDER))
    for a, b in zip(was[:2], now[:2]):
        assert all(np.array_equal(a[f], b[f]) for f in a)
    assert was[2] == now[2] and np.array_equal(was[3][0], now[3][0]) and was[3][1:] == now[3][1:] and not d_out.any()
    cb.record_stop()  # with no tap running the plain step is the step again
    rest, _, _ = run_rec(cb, pk[5:], recv[5:], "resident", {})
    plain = cb.step_resident(d_in, torch.from_numpy(recv[5]).cuda())
    assert plain.shape == (N, 172)
    cb.close()
    assert np.array_equal(np.concatenate([got, rest]), e["want"])


# ---------------------------------------------------------------- 5. without a store
def test_without_a_store(cuda, oracle_port, wmx):
    pk, recv = small_script()
    setup = small_setup(1, 8000)
    e = replayed(oracle_port, ("formats", 1, 8000), N, pk, recv, setup, {})
    cb = bridge(N, 3, None, K)
    calls(cb, setup, False)
    assert all(wmx.wmx_conf_rec(cb._h, k) is None and wmx.wmx_conf_rec_legs(cb._h, k) is None for k in range(3))
    assert wmx.wmx_conf_rec_row_bytes(cb._h) == 0 and cb.max_taps == 0
    idx = np.array([1], np.int32)
    assert wmx.wmx_conf_record(cb._h, idx.ctypes.data, 1, 0, None, None) == ESTATE
    assert wmx.wmx_conf_record_stop(cb._h, None, 0, None) == ESTATE
    assert wmx.wmx_conf_export_record(cb._h, None, None, None, None) == ESTATE
    got, _, _ = run_rec(cb, pk, recv, "ahead", {})
    cb.reset_legs([1])  # and a reset of a handle without a store has no recording to end
    assert wmx.wmx_conf_rec(cb._h, 0) is None
    cb.close()
    assert np.array_equal(got, e["plain"])


def test_what_the_recording_calls_refuse(cuda, wmx):
    cb = bridge(N, 3, LAYOUT6, K)
    EINVAL = -10001
    assert wmx.wmx_conf_recorders(cb._h, 0, 1, 8000) == EINVAL and wmx.wmx_conf_recorders(cb._h, 2, 3, 8000) == EINVAL
    assert wmx.wmx_conf_recorders(cb._h, 2, 1, 48001) == EINVAL and wmx.wmx_conf_recorders(cb._h, 2, 1, 0) == EINVAL
    assert wmx.wmx_conf_rec(cb._h, 0) is None
    cb.recorders(2, 2, 48000)
    assert cb.rec_row_bytes == 2 * 1920 and wmx.wmx_conf_recorders(cb._h, 2, 1, 8000) == ESTATE
    bad = np.array([1, N], np.int32)
    assert wmx.wmx_conf_record(cb._h, bad.ctypes.data, 2, 0, None, None) == EINVAL
    assert wmx.wmx_conf_record(cb._h, bad.ctypes.data, 1, -1, None, None) == EINVAL
    assert wmx.wmx_conf_record(cb._h, None, 0, 0, None, None) == EINVAL
    assert wmx.wmx_conf_record_stop(cb._h, bad.ctypes.data, 2, None) == EINVAL
    assert cb.export_record()["leg"].tolist() == [-1, -1]
    assert cb.record([4], seconds=0).tolist() == [0] and cb.export_record()["left"].tolist() == [0, 0]  # until stopped
    assert cb.record([4], ticks=1).tolist() == [0] and cb.export_record()["left"].tolist() == [1, 0]  # the reference's time == 0: one package
    assert cb.record([4], seconds=2).tolist() == [0] and cb.export_record()["left"].tolist() == [100, 0]
    cb.close()
