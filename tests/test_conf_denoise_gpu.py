"""wmx_conf_denoise (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with every leg's rows going through the
leg's own fixed-point noise suppressor.  The replay is ConfReplay of tests/conf_replay_model.py with tests/leg_dtmf_model.py and
tests/leg_denoise_model.py inserted where include/wmix_amd.h places the stages: behind the sequencer, DTMF detection first (on the
row as it arrived), then the suppressor, then the selection, the concealment and the load on the cleaned rows.  Layout (conferences of
2, 3 and 4), K = 3, the runner and the script generators are those of tests/test_conf_gpu.py and tests/test_conf_all_stages_gpu.py.
Every datagram of every tick and speaking / env after every tick are compared, head, tick and dropped at the end.  Bytes and
integers, np.array_equal."""
import numpy as np
import pytest

from conf_replay_model import ConfReplay
from leg_denoise_model import LegsDenoiseModel
from leg_dtmf_model import LegsDtmfModel
from leg_plc_model import ulaw_decode
from leg_seq_model import repaired_rows
from leg_codec_model import LAW_U, PCMU
from test_conf_dtmf_gpu import key_codes, ulaw_encode
from test_conf_gpu import G, K, LAYOUT, SEED, T, bridge, run
from test_conf_replay_model import CODEC_AT, RESET8_AT, all_stages, gap_behind, retyped
from test_conf_sequence_gpu import clean_script, impair, rows_of, seq_raw_of
from test_host_tick_bridge_rtp_gpu import arrivals

pytestmark = pytest.mark.gpu

MODES = [(1, "wait"), (3, "ahead"), (3, "resident")]
KEY_LEG, KEY_AT, KEY_PACKETS = 6, 22, 5  # leg 6 negotiated mu-law (tests/test_conf_codecs_gpu.py) and presses `5` once the host's mute has left it


class DenoiseReplay(ConfReplay):
    """ConfReplay with the DTMF stage and the suppressor; the setters are those of wmix_amd/conf.py"""

    def __init__(self, lib, n_legs, max_packets=3):
        super().__init__(lib, n_legs, max_packets)
        self.keys, self.dn = LegsDtmfModel(n_legs), LegsDenoiseModel(lib, n_legs)
        self.dtmf_on, self.dtmf_suppress, self.dtmf_pt, self.denoise_on = False, False, 101, False
        self.levels = []  # of every row the selection was shown, as it was shown it: for a story's choice of floor

    def dtmf(self, on, suppress=False, event_pt=101):
        self.dtmf_on, self.dtmf_suppress, self.dtmf_pt = bool(on), bool(suppress), event_pt

    def denoise(self, on):
        self.denoise_on = bool(on)

    def reset_legs(self, legs=None):
        super().reset_legs(legs)
        self.keys.reset(legs)
        self.dn.reset(legs)

    def tick(self, pk_t, recv_t):
        assert recv_t.shape == (self.n, self.K) and self.layout
        pcm, lens = self.rp.decode(pk_t, recv_t, self.K)
        heard = lens
        if self.seq_on:
            _, heard, self.lists = self.seq.tick(seq_raw_of(pk_t, recv_t), lens, self.max_gap)
        lists = self.lists if self.seq_on else None
        if self.dtmf_on:  # on the row as it arrived
            self.keys.tick(pk_t, recv_t, pcm, heard, lists, self.dtmf_pt, self.dtmf_suppress)
        if self.denoise_on:  # a suppressed key goes in as the zeros it became
            self.dn.tick(pcm, heard, lists)
        self.levels += [int(np.abs(pcm[g, k, :160].astype(np.int64)).sum()) for g, k in np.argwhere(heard == 320)]
        mute = self.host_mute
        if self.max_speakers > 0:
            _, mute = self.spk.step_legs(self.layout, pcm, heard, 320, self.max_speakers, self.floor, self.decay_shift, self.host_mute)
        if self.seq_on and self.conceal_on:
            rows, rlens = self.plc.tick(pcm, heard, self.lists)
            load = np.zeros((self.n, rows.shape[1], 161), np.int16)
            load[:, :, :160] = rows
        elif self.seq_on:
            load, rlens = repaired_rows(pcm, self.lists)
        else:
            load, rlens = pcm, lens
        self.load_mute = None if mute is None else np.array(mute, np.uint8)
        return self.rp.tick(load, rlens, self.layout, mute)


def replay(lib, n, pk, recv, setup, before=None, max_packets=K):
    """-> (datagrams [ticks, n, 172], export_legs() after every tick, the model)"""
    m = DenoiseReplay(lib, n, max_packets)
    setup(m)
    out, legs = np.zeros((recv.shape[0], n, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if before and t in before:
            before[t](m)
        out[t] = m.tick(pk[t], recv[t])
        legs.append(m.export_legs())
    return out, legs, m


def handle(n, slots, pk, recv, setup, before, mode):
    """-> (datagrams, export_legs() after every tick)"""
    cb, seen = bridge(n, slots, None, recv.shape[2]), []
    setup(cb)
    got = run(cb, pk, recv, mode, before=before, after=lambda t, c: seen.append(c.export_legs()))
    cb.close()
    return got, seen


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


# ---- a. denoise alone
def alone():
    def setup(c):
        c.set_conferences(LAYOUT)
        c.denoise(True)

    return arrivals(SEED, T, G) + (setup, None)


@pytest.mark.parametrize("slots,mode", MODES)
def test_denoise_alone(cuda, oracle_port, slots, mode):
    pk, recv, _, _, want, _, m = handle_equals_replay("alone", oracle_port, G, alone, slots, mode)
    plain, _, _ = replay(oracle_port, G, pk, recv, lambda c: c.set_conferences(LAYOUT))
    assert not np.array_equal(want[:, :9], plain[:, :9]) and np.array_equal(want[:, 9], plain[:, 9])  # leg 9 hears nobody
    assert all(len(h) > 0 for h in m.dn.history)  # a leg in no conference is cleaned all the same: the load is where it is left out


# ---- b., c. every stage on, on a clean and on an impaired schedule
def with_key(script):
    """leg 6's next KEY_PACKETS packets from tick KEY_AT on carry the key `5`"""
    keys = key_codes(5, KEY_PACKETS)
    for t in range(KEY_AT, len(script)):
        for i, (s, pt, _) in enumerate(script[t][KEY_LEG]):
            if keys:
                script[t][KEY_LEG][i] = (s, pt, keys.pop(0))
    assert not keys
    return script


def everything(lib, impaired):
    script = retyped(with_key(clean_script(2)), {2: CODEC_AT})
    if impaired:
        script, _ = impair(script, 3)
    gap_behind(script, 3, 15)
    gap_behind(script, 8, RESET8_AT)
    pk, recv = rows_of(script)
    def story(floor):
        # codecs, sequence, conceal, speakers(2, floor); mutes, a leg that leaves, joins elsewhere, changes its codec; two resets
        setup0, before = all_stages(floor)

        def setup(c):
            setup0(c)
            c.dtmf(True, True, 101)
            c.denoise(True)

        return setup, before

    # the floor: four in ten of the rows the selection is shown -- cleaned rows -- lie below it
    floor = int(np.percentile(replay(lib, G, pk, recv, *story(0))[2].levels, 40))
    return (pk, recv) + story(floor)


@pytest.mark.parametrize("impaired,slots,mode", [(False, 3, "ahead"), (False, 3, "resident"), (True, 1, "wait"), (True, 3, "ahead"), (True, 3, "resident")])
def test_every_stage_on(cuda, oracle_port, impaired, slots, mode):
    e = handle_equals_replay(("everything", impaired), oracle_port, G, lambda: everything(oracle_port, impaired), slots, mode)
    m = e[6]
    assert m.keys.export()["count"][KEY_LEG] >= 1 and m.export_conceal().sum() >= 1 and not m.export_legs()["dropped"].any()
    if impaired:
        st = m.export_sequence()
        assert st["lost"].any() and st["late"].any() and st["dup"].any()


def test_every_stage_matters_to_the_bytes(oracle_port):
    """on the model alone: the story of b. without the suppressor, and without the DTMF stage in front of it, sends other bytes"""
    pk, recv, setup, before = everything(oracle_port, False)
    want = REPLAYED[("everything", False)][4] if ("everything", False) in REPLAYED else replay(oracle_port, G, pk, recv, setup, before)[0]

    def without(name):
        def other(c):
            setup(c)
            c.denoise(False) if name == "denoise" else c.dtmf(False)
        return replay(oracle_port, G, pk, recv, other, before)[0]

    assert not np.array_equal(without("denoise"), want) and not np.array_equal(without("dtmf"), want)


# ---- d., e. a reset leg, and denoise switched on a running handle
def switched():
    def setup(c):
        c.set_conferences(LAYOUT)

    before = {8: lambda c: c.denoise(True), 16: lambda c: c.reset_legs([1]), 22: lambda c: c.denoise(False),
              26: lambda c: c.reset_legs([6]), 30: lambda c: c.denoise(True)}
    return arrivals(SEED, T, G) + (setup, before)


@pytest.mark.parametrize("slots,mode", MODES[1:])
def test_denoise_switched_on_a_running_handle_and_a_reset_leg(cuda, oracle_port, slots, mode):
    """on at tick 8; leg 1 is a new call at tick 16 (its suppressor starts again); off at 22 -- the state stays as it stood, but for leg 6,
    reset at tick 26 while the stage is off -- and on again at 30"""
    pk, recv, setup, before, want, _, _ = handle_equals_replay("switched", oracle_port, G, switched, slots, mode)
    plain, _, _ = replay(oracle_port, G, pk, recv, setup, {t: f for t, f in before.items() if t in (16, 26)})
    assert np.array_equal(want[:8], plain[:8]) and not np.array_equal(want[8:22], plain[8:22]) and not np.array_equal(want[30:], plain[30:])
    # the reset matters: without it leg 0 hears leg 1 through a suppressor that has adapted
    kept, _, _ = replay(oracle_port, G, pk, recv, setup, {t: f for t, f in before.items() if t != 16})
    assert not np.array_equal(kept[16:, 0], want[16:, 0])


def test_denoise_off_on_a_handle_that_was_never_on_changes_nothing(cuda):
    pk, recv = arrivals(SEED, T, G)
    sent = []
    for touch in (False, True):
        cb = bridge()
        if touch:
            cb.denoise(False)
        sent.append(run(cb, pk, recv, "ahead"))
        assert cb.denoiser_state(0) is None
        cb.close()
    assert np.array_equal(sent[0], sent[1])


def test_the_denoiser_state_of_a_leg_is_a_stream_blob(cuda, wmx):
    from wmix_amd.nsx import NsxBatch
    pk, recv = arrivals(SEED, T, G)
    cb = bridge()
    cb.denoise(True)
    fresh = cb.denoiser_state(3)
    other = NsxBatch(1, 1, 8000)
    assert np.array_equal(fresh, other.export_stream(0))
    run(cb, pk[:6], recv[:6], "ahead")
    moved = cb.denoiser_state(3)
    assert not np.array_equal(moved, fresh)
    other.import_stream(0, moved)  # a leg migrates: the blob is the suppressor's own
    assert np.array_equal(other.export_stream(0), moved)
    cb.denoise(False)
    run(cb, pk[6:9], recv[6:9], "ahead")
    assert np.array_equal(cb.denoiser_state(3), moved)  # off: the state does not move
    cb.reset_legs([3])
    assert np.array_equal(cb.denoiser_state(3), fresh) and not np.array_equal(cb.denoiser_state(2), cb.denoiser_state(3))
    cb.reset_legs()  # every leg
    assert all(np.array_equal(cb.denoiser_state(g), fresh) for g in range(G))
    assert wmx.wmx_conf_denoise(None, 1) == -10001 and not wmx.wmx_conf_denoiser(None)
    other.close()
    cb.close()


# ---- f. what it is for
def noise_script(n_legs, ticks, sigma=400.0, seed=11):
    """leg 0 sends stationary noise as mu-law packets, one a tick; the others send nothing"""
    rng = np.random.default_rng(seed)
    x = np.clip(np.round(rng.normal(0, sigma, ticks * 160)), -32768, 32767).astype(np.int16)
    script = [[[(t, 0, ulaw_encode(x[160 * t:160 * t + 160]))]] + [[] for _ in range(n_legs - 1)] for t in range(ticks)]
    return rows_of(script, legs=n_legs, ticks=ticks)


def test_a_noisy_leg_is_heard_quieter(cuda):
    """One leg of a pair sends stationary noise, sigma = 400, for 300 ticks, of which the first 60 and more are lead-in: the suppressor's
    start-up (its first 50 blocks) and the settling of its noise estimate.  What the other leg is sent, decoded, over the last 25 ticks
    has an rms below 0.75 of the same run with denoise off.  The oracle alone gives 0.125 on this input (50 against 402: stationary
    white noise ends at the suppressor's gain floor, 2048 / 16384), and the handle measured 50.9 against 401.0; the cap is a condition
    on the wiring, not a measure of quality."""
    ticks = 300
    pk, recv = noise_script(2, ticks)
    rms = []
    for on in (False, True):
        cb = bridge(2, 3, [[0, 1]])
        cb.set_codecs(None, PCMU, LAW_U)
        cb.denoise(on)
        out = run(cb, pk, recv, "ahead")
        cb.close()
        heard = ulaw_decode(out[-25:, 1, 12:].reshape(-1)).astype(np.float64)
        rms.append(float(np.sqrt((heard ** 2).mean())))
        assert (out[60:, 0, 12:] == 0xFF).all()  # the noisy leg hears the silent one
    print("rms of the last 25 ticks: off %.1f, on %.1f, ratio %.3f" % (rms[0], rms[1], rms[1] / rms[0]))
    assert 300 < rms[0] < 500 and rms[1] < 0.75 * rms[0], rms


def test_a_noisy_leg_does_not_hold_the_talker_slot(cuda, oracle_port):
    """A conference of three with speakers(1): leg 0 sends stationary noise.  The floor lies between the envelope of its rows as they
    arrive and as the suppressor leaves them, both taken from the replay: with denoise off the leg is speaking, with it on it is not
    -- tick by tick as the replay says."""
    ticks, tail = 130, 10
    pk, recv = noise_script(3, ticks)

    def story(on, floor):
        def setup(c):
            c.set_conferences([[0, 1, 2]])
            c.set_codecs(None, PCMU, LAW_U)
            c.speakers(1, floor, 3)
            c.denoise(on)
        return setup

    env = {on: np.array([st["env"][0] for st in replay(oracle_port, 3, pk, recv, story(on, 0))[1]], np.int64) for on in (False, True)}
    assert env[True][-tail:].max() < env[False][-tail:].min(), (env[True][-tail:], env[False][-tail:])
    floor = int(env[True][-tail:].max() + env[False][-tail:].min()) // 2
    for on in (False, True):
        want, legs, _ = replay(oracle_port, 3, pk, recv, story(on, floor))
        got, seen = handle(3, 3, pk, recv, story(on, floor), None, "ahead")
        assert np.array_equal(got, want)
        for t in range(ticks):
            assert np.array_equal(seen[t]["speaking"], legs[t]["speaking"]) and np.array_equal(seen[t]["env"], legs[t]["env"]), ("tick", t)
        assert all(bool(st["speaking"][0]) == (not on) for st in seen[-tail:]), [st["speaking"][0] for st in seen[-tail:]]
