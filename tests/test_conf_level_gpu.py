"""wmx_conf_level (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with every leg's rows going through the
leg's own AGC.  The replay is ConfReplay of tests/conf_replay_model.py with tests/leg_dtmf_model.py, tests/leg_denoise_model.py and
tests/leg_level_model.py inserted where include/wmix_amd.h places the stages: behind the sequencer, DTMF detection first (on the row as
it arrived), then the suppressor, then the AGC, then the selection, the concealment and the load on the levelled rows.  Layout, K = 3,
the runner, the script generators and the handle / replay comparison are those of tests/test_conf_denoise_gpu.py.  Every datagram of
every tick and speaking / env after every tick are compared, head, tick and dropped at the end.  Bytes and integers, np.array_equal."""
import numpy as np
import pytest

import test_conf_denoise_gpu as dn
from leg_codec_model import LAW_U, PCMU
from leg_level_model import LegsLevelModel
from leg_plc_model import ulaw_decode
from leg_seq_model import repaired_rows
from test_bridge_gpu import EINVAL
from test_conf_denoise_gpu import DenoiseReplay, MODES, handle, with_key
from test_conf_dtmf_gpu import ulaw_encode
from test_conf_gpu import G, LAYOUT, SEED, T, bridge, run
from test_conf_replay_model import CODEC_AT, RESET8_AT, all_stages, gap_behind, retyped
from test_conf_sequence_gpu import clean_script, impair, rows_of, seq_raw_of
from test_host_tick_bridge_rtp_gpu import arrivals

pytestmark = pytest.mark.gpu

VALUE = 20
REFUSED = (187, 200)  # compression gains the AGC's gain table cannot be made for: 0 .. 186 dB are the ones it can


class LevelReplay(DenoiseReplay):
    """DenoiseReplay with the AGC behind the suppressor; the setters are those of wmix_amd/conf.py"""

    def __init__(self, lib, n_legs, max_packets=3):
        super().__init__(lib, n_legs, max_packets)
        self.lv, self.level_on, self.level_value = None, False, None

    def level(self, on, value=VALUE):
        if on:
            if self.lv is None:
                self.lv = LegsLevelModel(self.dn.lib, self.n, value)
            elif value != self.level_value:
                self.lv.set_gain(value)  # agc_addition for every leg
            self.level_value = value
        self.level_on = bool(on)

    def set_leg_gain(self, legs, value):
        self.lv.set_gain(value, legs)

    def reset_legs(self, legs=None):
        super().reset_legs(legs)
        if self.lv is not None:
            self.lv.reset(legs)

    def tick(self, pk_t, recv_t):
        assert recv_t.shape == (self.n, self.K) and self.layout
        pcm, lens = self.rp.decode(pk_t, recv_t, self.K)
        heard = lens
        if self.seq_on:
            _, heard, self.lists = self.seq.tick(seq_raw_of(pk_t, recv_t), lens, self.max_gap)
        lists = self.lists if self.seq_on else None
        if self.dtmf_on:  # on the row as it arrived
            self.keys.tick(pk_t, recv_t, pcm, heard, lists, self.dtmf_pt, self.dtmf_suppress)
        if self.denoise_on:
            self.dn.tick(pcm, heard, lists)
        if self.level_on:  # directly behind the suppressor: a suppressed key goes in as the zeros it became
            self.lv.tick(pcm, heard, lists)
        self.levels += [int(np.abs(pcm[g, k, :160].astype(np.int64)).sum()) for g, k in np.argwhere(heard == 320)]
        mute = self.host_mute
        if self.max_speakers > 0:
            _, mute = self.spk.step_legs(self.layout, pcm, heard, 320, self.max_speakers, self.floor, self.decay_shift, self.host_mute)
        if self.seq_on and self.conceal_on:  # the history is levelled audio, and is not fed to the AGC again
            rows, rlens = self.plc.tick(pcm, heard, self.lists)
            load = np.zeros((self.n, rows.shape[1], 161), np.int16)
            load[:, :, :160] = rows
        elif self.seq_on:
            load, rlens = repaired_rows(pcm, self.lists)
        else:
            load, rlens = pcm, lens
        self.load_mute = None if mute is None else np.array(mute, np.uint8)
        return self.rp.tick(load, rlens, self.layout, mute)


def replay(lib, n, pk, recv, setup, before=None, max_packets=3):
    """-> (datagrams [ticks, n, 172], export_legs() after every tick, the model)"""
    m = LevelReplay(lib, n, max_packets)
    setup(m)
    out, legs = np.zeros((recv.shape[0], n, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if before and t in before:
            before[t](m)
        out[t] = m.tick(pk[t], recv[t])
        legs.append(m.export_legs())
    return out, legs, m


REPLAYED = {}  # a story's replay, made once and shared by the modes that run it


def handle_equals_replay(key, lib, n, story, slots, mode):
    """story() -> (pk, recv, setup, before)"""
    if key not in REPLAYED:
        pk, recv, setup, before = story()
        REPLAYED[key] = (pk, recv, setup, before) + replay(lib, n, pk, recv, setup, before)
    pk, recv, setup, before, want, legs, m = REPLAYED[key]
    got, seen = handle(n, slots, pk, recv, setup, before, mode)
    for t in range(recv.shape[0]):
        for name in ("speaking", "env"):
            assert np.array_equal(seen[t][name], legs[t][name]), (name, "tick", t, seen[t][name], legs[t][name])
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    for name in ("head", "tick", "dropped"):
        assert np.array_equal(seen[-1][name], legs[-1][name]), (name, seen[-1][name], legs[-1][name])
    return REPLAYED[key]


def gains_of(cb):
    from wmix_amd._lib import lib
    agc = lib().wmx_conf_leveller(cb._h)
    return [lib().wmx_agc_stream_gain(agc, g) for g in range(cb.n_legs)]


# ---- a. level alone
def alone():
    def setup(c):
        c.set_conferences(LAYOUT)
        c.level(True, VALUE)

    return arrivals(SEED, T, G) + (setup, None)


@pytest.mark.parametrize("slots,mode", MODES)
def test_level_alone(cuda, oracle_port, slots, mode):
    pk, recv, _, _, want, _, m = handle_equals_replay("alone", oracle_port, G, alone, slots, mode)
    plain, _, _ = replay(oracle_port, G, pk, recv, lambda c: c.set_conferences(LAYOUT))
    assert not np.array_equal(want[:, :9], plain[:, :9]) and np.array_equal(want[:, 9], plain[:, 9])  # leg 9 hears nobody
    assert all(len(h) > 0 for h in m.lv.history)  # a leg in no conference is levelled all the same: the load is where it is left out


# ---- b. every stage on, on an impaired schedule
def everything(lib):
    script, _ = impair(retyped(with_key(clean_script(2)), {2: CODEC_AT}), 3)
    gap_behind(script, 3, 15)
    gap_behind(script, 8, RESET8_AT)
    pk, recv = rows_of(script)

    def story(floor, level=True):
        # codecs, sequence, conceal, speakers(2, floor); mutes, a leg that leaves, joins elsewhere, changes its codec; two resets
        setup0, before = all_stages(floor)

        def setup(c):
            setup0(c)
            c.dtmf(True, True, 101)
            c.denoise(True)
            c.level(level, VALUE)

        return setup, before

    # the floor: four in ten of the rows the selection is shown -- levelled rows -- lie below it
    floor = int(np.percentile(replay(lib, G, pk, recv, *story(0))[2].levels, 40))
    return (pk, recv) + story(floor), story(floor, False)


@pytest.mark.parametrize("slots,mode", [(3, "ahead"), (3, "resident")])
def test_every_stage_on(cuda, oracle_port, slots, mode):
    if "off" not in REPLAYED:
        REPLAYED["with"], REPLAYED["off"] = everything(oracle_port)
    pk, recv, _, _, want, _, m = handle_equals_replay("everything", oracle_port, G, lambda: REPLAYED["with"], slots, mode)
    st = m.export_sequence()
    assert m.keys.export()["count"][dn.KEY_LEG] >= 1 and m.export_conceal().sum() >= 1 and not m.export_legs()["dropped"].any()
    assert st["lost"].any() and st["late"].any() and st["dup"].any()
    if "everything off" not in REPLAYED:  # the same story with level off sends other bytes
        REPLAYED["everything off"] = replay(oracle_port, G, pk, recv, *REPLAYED["off"])[0]
    assert not np.array_equal(REPLAYED["everything off"], want)


# ---- c. level switched on a running handle, a leg reset, off and on again
def switched():
    def setup(c):
        c.set_conferences(LAYOUT)

    before = {8: lambda c: c.level(True, VALUE), 12: lambda c: c.set_leg_gain([1, 6], 9), 16: lambda c: c.reset_legs([1]),
              22: lambda c: c.level(False), 26: lambda c: c.reset_legs([6]), 30: lambda c: c.level(True, VALUE)}
    return arrivals(SEED, T, G) + (setup, before)


@pytest.mark.parametrize("slots,mode", MODES[1:])
def test_level_switched_on_a_running_handle_and_a_reset_leg(cuda, oracle_port, slots, mode):
    """on at tick 8; legs 1 and 6 get a gain of their own at 12; leg 1 is a new call at tick 16 (its AGC starts again, on the gain it
    has); off at 22 -- the state stays as it stood, but for leg 6, reset at tick 26 while the stage is off -- and on again at 30 with
    the value of before: no leg's gain changes"""
    pk, recv, setup, before, want, _, m = handle_equals_replay("switched", oracle_port, G, switched, slots, mode)
    plain, _, _ = replay(oracle_port, G, pk, recv, setup, {t: f for t, f in before.items() if t in (16, 26)})
    assert np.array_equal(want[:8], plain[:8]) and not np.array_equal(want[8:22], plain[8:22]) and not np.array_equal(want[30:], plain[30:])
    assert m.lv.gain == [VALUE, 9] + [VALUE] * 4 + [9] + [VALUE] * 3
    # the reset matters: without it leg 0 hears leg 1 through an AGC that has adapted; and so does the gain it kept
    kept, _, _ = replay(oracle_port, G, pk, recv, setup, {t: f for t, f in before.items() if t != 16})
    assert not np.array_equal(kept[16:, 0], want[16:, 0])
    same_gain, _, _ = replay(oracle_port, G, pk, recv, setup, {t: f for t, f in before.items() if t != 12})
    assert not np.array_equal(same_gain[12:, 0], want[12:, 0])


def test_the_gains_and_the_state_are_kept_through_off_and_on(cuda):
    pk, recv = arrivals(SEED, T, G)
    cb = bridge()
    cb.level(True, VALUE)
    cb.set_leg_gain([1, 6], 9)
    fresh = cb.leveller_state(3)
    run(cb, pk[:6], recv[:6], "ahead")
    moved = [cb.leveller_state(g) for g in range(G)]
    assert not np.array_equal(moved[3], fresh)
    cb.level(False)
    run(cb, pk[6:9], recv[6:9], "ahead")
    assert all(np.array_equal(cb.leveller_state(g), moved[g]) for g in range(G))  # off: the state does not move
    cb.reset_legs([1, 3])
    cb.level(True, VALUE)
    assert np.array_equal(cb.leveller_state(3), fresh) and gains_of(cb) == [VALUE, 9] + [VALUE] * 4 + [9] + [VALUE] * 3
    assert not np.array_equal(cb.leveller_state(1), fresh) and np.array_equal(cb.leveller_state(1)[:-4], fresh[:-4])  # all but its gain
    assert all(np.array_equal(cb.leveller_state(g), moved[g]) for g in range(G) if g not in (1, 3))
    cb.reset_legs()  # every leg
    assert all(np.array_equal(cb.leveller_state(g)[:-4], fresh[:-4]) for g in range(G)) and gains_of(cb)[6] == 9
    cb.level(True, 12)  # another value: every leg
    assert gains_of(cb) == [12] * G
    cb.close()


# ---- d. another value on a made handle, and one leg's volume
def regained():
    def setup(c):
        c.set_conferences(LAYOUT)
        c.level(True, VALUE)

    before = {14: lambda c: c.level(True, 9), 24: lambda c: c.set_leg_gain([2], 30)}
    return arrivals(SEED, T, G) + (setup, before)


@pytest.mark.parametrize("slots,mode", MODES[1:])
def test_another_value_and_one_legs_gain_are_agc_addition_at_that_tick(cuda, oracle_port, slots, mode):
    pk, recv, setup, before, want, _, m = handle_equals_replay("regained", oracle_port, G, regained, slots, mode)
    assert m.lv.gain == [9, 9, 30] + [9] * 7 and all(a for a in m.lv.additions)
    base = REPLAYED["alone"][4] if "alone" in REPLAYED else replay(oracle_port, G, pk, recv, setup)[0]
    only14, _, _ = replay(oracle_port, G, pk, recv, setup, {14: before[14]})
    assert np.array_equal(want[:14], base[:14]) and not np.array_equal(want[14:24], base[14:24])
    assert np.array_equal(want[:24], only14[:24]) and not np.array_equal(want[24:, 3:5], only14[24:, 3:5])  # legs 3 and 4 hear leg 2


# ---- e. before the first switch-on, NULL, and a value that is refused
def test_level_off_on_a_handle_that_was_never_on_changes_nothing(cuda, wmx):
    pk, recv = arrivals(SEED, T, G)
    sent = []
    for touch in (False, True):
        cb = bridge()
        if touch:
            cb.level(False)
            for v in REFUSED:  # the first switch-on refused: nothing is made
                assert wmx.wmx_conf_level(cb._h, 1, v) == EINVAL and b"compression gain" in wmx.wmx_last_error()
        sent.append(run(cb, pk, recv, "ahead"))
        assert cb.leveller_state(0) is None and not wmx.wmx_conf_leveller(cb._h)
        cb.close()
    assert np.array_equal(sent[0], sent[1])
    assert wmx.wmx_conf_level(None, 1, VALUE) == EINVAL and wmx.wmx_conf_level(None, 0, VALUE) == EINVAL and not wmx.wmx_conf_leveller(None)


def test_a_refused_value_changes_nothing_on_a_running_handle(cuda, wmx, oracle_port):
    pk, recv, setup, _ = alone()
    want = REPLAYED["alone"][4] if "alone" in REPLAYED else replay(oracle_port, G, pk, recv, setup)[0]

    def refused(c):
        for v in REFUSED:
            assert wmx.wmx_conf_level(c._h, 1, v) == EINVAL and b"compression gain" in wmx.wmx_last_error()
            with pytest.raises(Exception, match="compression gain"):
                c.set_leg_gain([2], v)
        assert gains_of(c) == [VALUE] * G

    cb = bridge()
    setup(cb)
    got = run(cb, pk, recv, "ahead", before={10: refused, 20: refused})
    cb.close()
    assert np.array_equal(got, want)


# ---- f. what it is for
def voiced(amp, ticks, seed=5):
    """220 + 660 + 1 500 Hz, each at `amp`, 3 000 of every 4 000 samples on, under noise of 2 % of amp"""
    n = ticks * 160
    t = np.arange(n)
    x = sum(np.sin(2 * np.pi * f * t / 8000) for f in (220, 660, 1500)) * (t % 4000 < 3000) + 0.02 * np.random.default_rng(seed).normal(0, 1, n)
    return np.clip(np.round(amp * x), -32768, 32767).astype(np.int16)


def one_talker(talker, amp, ticks):
    """a conference of three: `talker` sends the voiced bursts as mu-law packets, one a tick; the others send nothing"""
    x = voiced(amp, ticks)
    script = [[[(t, 0, ulaw_encode(x[160 * t:160 * t + 160]))] if g == talker else [] for g in range(3)] for t in range(ticks)]
    return rows_of(script, legs=3, ticks=ticks)


def test_a_quiet_leg_is_heard_nearer_to_a_loud_one(cuda):
    """A conference of three, level(True, 20).  Leg 0 sends voiced bursts at amplitude 10 000, leg 1 the same signal at amplitude 1 000,
    each alone in a run of 6 s; what leg 2 is sent, decoded, over the last 2 s has an rms r0 while leg 0 talks and r1 while leg 1 talks.
    r0 / r1 with level on is at most 0.7 of r0 / r1 with level off.  The oracle alone (one agc of value 20 over the mu-law round trip
    of each signal, the last 2 s) gives 15 406 / 5 613 = 2.745 against 10 596 / 1 061 = 9.987 going in: 0.275 of it; the handle
    measured 15 378 / 5 568 = 2.762 against 10 596 / 1 061 = 9.987: 0.277 (what leg 2 is sent has been through the mu-law encoder once
    more).  The cap is a condition on the wiring, not a measure of quality."""
    ticks, tail = 300, 100
    rms = {}
    for on in (False, True):
        for talker, amp in ((0, 10000), (1, 1000)):
            pk, recv = one_talker(talker, amp, ticks)
            cb = bridge(3, 3, [[0, 1, 2]])
            cb.set_codecs(None, PCMU, LAW_U)
            cb.level(on, VALUE)
            out = run(cb, pk, recv, "ahead")
            cb.close()
            heard = ulaw_decode(out[-tail:, 2, 12:].reshape(-1)).astype(np.float64)
            rms[on, talker] = float(np.sqrt((heard ** 2).mean()))
    off, on = rms[False, 0] / rms[False, 1], rms[True, 0] / rms[True, 1]
    print("rms of the last 2 s: off %.1f / %.1f = %.3f, on %.1f / %.1f = %.3f, on / off %.3f"
          % (rms[False, 0], rms[False, 1], off, rms[True, 0], rms[True, 1], on, on / off))
    assert 9.0 < off < 11.0 and on <= 0.7 * off, rms
