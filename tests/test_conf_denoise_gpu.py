"""wmx_conf_denoise (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with every leg's rows going through the
leg's own fixed-point noise suppressor.  The replay is ConfReplay of tests/conf_replay_model.py, which has tests/leg_dtmf_model.py and
tests/leg_denoise_model.py where include/wmix_amd.h places the stages: behind the sequencer, DTMF detection first (on the row as it
arrived), then the suppressor, then the selection, the concealment and the load on the cleaned rows.  Layout (conferences of 2, 3 and
4), K = 3 and the scripts are those of tests/conf_inputs.py, the stories those of tests/conf_stories.py, the runner and the handle /
replay comparison those of tests/conf_harness.py: every datagram of every tick and speaking / env after every tick are compared, and
at the end head, tick and dropped and what the sequencer, the concealment and the codecs export.  Bytes and integers, np.array_equal."""
import numpy as np
import pytest

from conf_harness import MODES, bridge, expected, handle, handle_equals_replay, run
from conf_inputs import G, K, KEY_LEG, LAYOUT, SEED, T, arrivals, noise_script, ulaw_decode
from conf_replay_model import replay_story
from conf_stories import alone, everything, switched
from leg_codec_model import LAW_U, PCMU

pytestmark = pytest.mark.gpu


# ---- a. denoise alone
@pytest.mark.parametrize("slots,mode", MODES)
def test_denoise_alone(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(expected(("denoise", "alone"), oracle_port, G, K, lambda: alone("denoise")), slots, mode)
    pk, recv, want, m = e["pk"], e["recv"], e["want"], e["model"]
    plain, _, _ = replay_story(oracle_port, G, K, pk, recv, lambda c: c.set_conferences(LAYOUT))
    assert not np.array_equal(want[:, :9], plain[:, :9]) and np.array_equal(want[:, 9], plain[:, 9])  # leg 9 hears nobody
    assert all(len(h) > 0 for h in m.dn.history)  # a leg in no conference is cleaned all the same: the load is where it is left out


# ---- b., c. every stage on, on a clean and on an impaired schedule
def every_stage(lib, impaired):
    return expected(("denoise", "everything", impaired), lib, G, K, lambda: everything(lib, impaired))


@pytest.mark.parametrize("impaired,slots,mode", [(False, 3, "ahead"), (False, 3, "resident"), (True, 1, "wait"), (True, 3, "ahead"), (True, 3, "resident")])
def test_every_stage_on(cuda, oracle_port, impaired, slots, mode):
    m = handle_equals_replay(every_stage(oracle_port, impaired), slots, mode)["model"]
    assert m.keys.export()["count"][KEY_LEG] >= 1 and m.export_conceal().sum() >= 1 and not m.export_legs()["dropped"].any()
    if impaired:
        st = m.export_sequence()
        assert st["lost"].any() and st["late"].any() and st["dup"].any()


def test_every_stage_matters_to_the_bytes(oracle_port):
    """on the model alone: the story of b. without the suppressor, and without the DTMF stage in front of it, sends other bytes"""
    e = every_stage(oracle_port, False)
    pk, recv, setup, before, want = e["pk"], e["recv"], e["setup"], e["before"], e["want"]

    def without(name):
        def other(c):
            setup(c)
            c.denoise(False) if name == "denoise" else c.dtmf(False)
        return replay_story(oracle_port, G, K, pk, recv, other, before)[0]

    assert not np.array_equal(without("denoise"), want) and not np.array_equal(without("dtmf"), want)


# ---- d., e. a reset leg, and denoise switched on a running handle
@pytest.mark.parametrize("slots,mode", MODES[1:])
def test_denoise_switched_on_a_running_handle_and_a_reset_leg(cuda, oracle_port, slots, mode):
    """on at tick 8; leg 1 is a new call at tick 16 (its suppressor starts again); off at 22 -- the state stays as it stood, but for leg 6,
    reset at tick 26 while the stage is off -- and on again at 30"""
    e = handle_equals_replay(expected(("denoise", "switched"), oracle_port, G, K, lambda: switched("denoise")), slots, mode)
    pk, recv, setup, before, want = e["pk"], e["recv"], e["setup"], e["before"], e["want"]
    plain, _, _ = replay_story(oracle_port, G, K, pk, recv, setup, {t: f for t, f in before.items() if t in (16, 26)})
    assert np.array_equal(want[:8], plain[:8]) and not np.array_equal(want[8:22], plain[8:22]) and not np.array_equal(want[30:], plain[30:])
    # the reset matters: without it leg 0 hears leg 1 through a suppressor that has adapted
    kept, _, _ = replay_story(oracle_port, G, K, pk, recv, setup, {t: f for t, f in before.items() if t != 16})
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

    env = {on: np.array([st["env"][0] for st in replay_story(oracle_port, 3, K, pk, recv, story(on, 0))[1]], np.int64) for on in (False, True)}
    assert env[True][-tail:].max() < env[False][-tail:].min(), (env[True][-tail:], env[False][-tail:])
    floor = int(env[True][-tail:].max() + env[False][-tail:].min()) // 2
    for on in (False, True):
        want, legs, _ = replay_story(oracle_port, 3, K, pk, recv, story(on, floor))
        got, seen, _ = handle(3, 3, pk, recv, story(on, floor), None, "ahead")
        assert np.array_equal(got, want)
        for t in range(ticks):
            assert np.array_equal(seen[t]["speaking"], legs[t]["speaking"]) and np.array_equal(seen[t]["env"], legs[t]["env"]), ("tick", t)
        assert all(bool(st["speaking"][0]) == (not on) for st in seen[-tail:]), [st["speaking"][0] for st in seen[-tail:]]
