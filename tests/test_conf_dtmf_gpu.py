"""wmx_conf_dtmf (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge listening to its legs' keypads.  Layout, K
and the script generator (key_script) are those of tests/conf_inputs.py, the runner that of tests/conf_harness.py.  Leg 6 -- one of the four
of the last conference -- negotiated mu-law by payload type and is silent (code 0xFF is a sample of exactly 0) but for the key it
presses; leg 3 sends its keys as RFC 4733 packets beside its audio.  What the other legs are sent is compared between handles: with
suppression on, a script with the key is sent as the script without it; with DTMF off, or on without suppression, nothing that is sent
changes.  Which blocks are tones is tests/leg_dtmf_model.py's to say.  Bytes and integers, np.array_equal."""
import numpy as np
import pytest

from conf_harness import bridge, run
from conf_inputs import EINVAL, EVENT_LEG, G, KEY_AT, KEY_LEG, key_script
from leg_dtmf_model import FROM_PACKET, digits_of

pytestmark = pytest.mark.gpu


def handle(seq=False, conceal=False, speakers=True):
    cb = bridge()
    cb.set_codecs([KEY_LEG], "by_pt", "a")
    if speakers:
        cb.speakers(2, 100, 3)
    if seq:
        cb.sequence(True, 3)
    if conceal:
        cb.conceal(True)
    return cb


def keys_read(cb):
    st = cb.export_dtmf()
    return [digits_of(st["count"][g], st["ring"][g]) for g in range(G)]


@pytest.mark.parametrize("seq,conceal,mode", [(False, False, "ahead"), (True, False, "resident"), (True, True, "wait")])
def test_a_suppressed_key_is_reported_once_and_heard_by_nobody(cuda, seq, conceal, mode):
    with_key, silent = key_script(5, 5), key_script(5, 0)
    assert not np.array_equal(with_key[0], silent[0]) and np.array_equal(with_key[1], silent[1])
    speaking = {}

    def sent(script, dtmf, name):
        cb = handle(seq, conceal)
        if dtmf:
            cb.dtmf(True, suppress=True)
        speaking[name] = []
        out = run(cb, script[0], script[1], mode, after=lambda t, c: speaking[name].append(c.export_legs()["speaking"].copy()))
        keys = keys_read(cb)
        cb.close()
        return out, keys

    got, keys = sent(with_key, True, "on")
    want, none = sent(silent, False, "silent")
    heard, unheard = sent(with_key, False, "plain")
    assert keys == [[("5", False)] if g == KEY_LEG else [] for g in range(G)], keys
    assert none == [[]] * G and unheard == [[]] * G
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert not any(sp[KEY_LEG] for sp in speaking["on"])
    # what suppression is for: unsuppressed, the key takes a talker slot and the legs of its conference are sent it
    pressed = range(KEY_AT, KEY_AT + 5)
    assert all(speaking["plain"][t][KEY_LEG] for t in pressed) and not np.array_equal(heard[:, [5, 7, 8]], want[:, [5, 7, 8]])
    assert np.array_equal(heard[:, :5], want[:, :5])  # the other conferences never heard it


def test_without_suppression_the_key_is_reported_and_nothing_sent_changes(cuda):
    pk, recv = key_script(9, 5)
    sent = []
    for dtmf in (False, True):
        cb = handle()
        if dtmf:
            cb.dtmf(True)
        sent.append(run(cb, pk, recv, "ahead"))
        assert keys_read(cb)[KEY_LEG] == ([("9", False)] if dtmf else [])
        cb.close()
    assert np.array_equal(sent[0], sent[1])


def test_a_key_sent_as_event_packets_is_reported_once_with_bit_7(cuda):
    events = [(8, 7, 16000, False), (9, 7, 16000, False), (10, 7, 16000, False), (11, 7, 16000, True),  # one press of `7`
              (14, 11, 24000, False), (15, 11, 24000, True),                                              # one of `#`
              (17, 16, 32000, False)]                                                                       # flash: no key
    pk, recv = key_script(5, 0, events)
    sent, refused = [], []
    for dtmf in (False, True):
        cb = handle(speakers=False)
        if dtmf:
            cb.dtmf(True, suppress=True, event_pt=101)
        sent.append(run(cb, pk, recv, "ahead"))
        refused.append(cb.export_codecs()["refused"])
        st = cb.export_dtmf()
        if dtmf:
            assert st["count"].tolist() == [2 if g == EVENT_LEG else 0 for g in range(G)]
            assert st["ring"][EVENT_LEG, :2].tolist() == [7 | FROM_PACKET, 11 | FROM_PACKET]
            assert digits_of(st["count"][EVENT_LEG], st["ring"][EVENT_LEG]) == [("7", True), ("#", True)]
        else:
            assert not st["count"].any() and not st["ring"].any()
        cb.close()
    # the packets stay refused for the audio path, counted as before, and nothing that is sent changes
    assert np.array_equal(refused[0], refused[1]) and refused[0][EVENT_LEG] == len(events) and refused[0].sum() == len(events)
    assert np.array_equal(sent[0], sent[1])
    # another negotiated payload type: these packets are not its events
    cb = handle(speakers=False)
    cb.dtmf(True, event_pt=96)
    run(cb, pk, recv, "ahead")
    assert not cb.export_dtmf()["count"].any()
    cb.close()


def test_dtmf_switched_off_again_is_dtmf_never_touched(cuda):
    pk, recv = key_script(5, 5)
    sent = []
    for touch in (False, True):
        cb = handle(seq=True)
        if touch:
            cb.dtmf(True, suppress=True)
            cb.dtmf(False)
        sent.append(run(cb, pk, recv, "ahead"))
        assert not cb.export_dtmf()["count"].any()
        cb.close()
    assert np.array_equal(sent[0], sent[1])
    # switched off in mid-run: the key pressed afterwards is heard again and not reported
    cb, ref = handle(), handle()
    cb.dtmf(True, suppress=True)
    got = run(cb, pk, recv, "ahead", before={KEY_AT - 2: lambda c: c.dtmf(False)})
    assert np.array_equal(got, run(ref, pk, recv, "ahead")) and not cb.export_dtmf()["count"].any()
    cb.close()
    ref.close()


def test_a_reset_leg_reports_nothing_of_the_old_call(cuda):
    """The key fills the packets of ticks 10 and 11, and leg 3 sends the same event with the same timestamp at ticks 9 and 12.  Left
    alone that is one `5` in band -- and one `4` from a packet, the second being a retransmission.  With both legs reset in front of tick
    11 the second tone packet is the new call's first (nothing in band), and its event packet meets a leg with no last timestamp
    (reported, as the new call's first report)."""
    events = [(9, 4, 777, False), (12, 4, 777, False)]
    pk, recv = key_script(5, 2, events)
    cb = handle()
    cb.dtmf(True, suppress=True)
    run(cb, pk, recv, "ahead")
    assert keys_read(cb)[KEY_LEG] == [("5", False)] and keys_read(cb)[EVENT_LEG] == [("4", True)]
    cb.close()
    seen = {}

    def reset(c):
        seen["before"] = c.export_dtmf()
        c.reset_legs([KEY_LEG, EVENT_LEG])
        seen["after"] = c.export_dtmf()

    cb = handle()
    cb.dtmf(True, suppress=True)
    run(cb, pk, recv, "ahead", before={KEY_AT + 1: reset})
    assert seen["before"]["count"][EVENT_LEG] == 1 and not seen["after"]["count"].any() and not seen["after"]["ring"].any()
    keys = keys_read(cb)
    assert keys[KEY_LEG] == [] and keys[EVENT_LEG] == [("4", True)], keys
    cb.close()


def test_dtmf_refusals(cuda, wmx):
    assert wmx.wmx_conf_dtmf(None, 1, 0, 101) == EINVAL and wmx.wmx_conf_export_dtmf(None, None, None, None) == EINVAL
    pk, recv = key_script(5, 5)
    cb, ref = handle(), handle()
    cb.dtmf(True, suppress=True)
    for pt in (95, 128, 0, -1):
        assert wmx.wmx_conf_dtmf(cb._h, 1, 0, pt) == EINVAL and b"event_pt" in wmx.wmx_last_error()
        assert wmx.wmx_conf_dtmf(ref._h, 0, 0, pt) == EINVAL
    assert wmx.wmx_conf_export_dtmf(cb._h, None, None, None) == 0  # either pointer may be NULL
    # the refused calls changed nothing: suppression is still on, the key is reported and not heard
    got = run(cb, pk, recv, "ahead")
    silent = key_script(5, 0)
    assert np.array_equal(got, run(ref, silent[0], silent[1], "ahead"))
    assert keys_read(cb)[KEY_LEG] == [("5", False)] and not ref.export_dtmf()["count"].any()
    cb.close()
    ref.close()
