"""examples/host_conf.c --denoise: the C example with every leg's rows going through the leg's own noise suppressor (wmx_conf_denoise),
alone and beside --sequence / --conceal, --ulaw-every and --dtmf, at the sizes tests/test_host_conf_gpu.py runs it.  The datagrams it
sends are those of the Python handle with the same switches over the same script, as in tests/test_host_conf_conceal_gpu.py; that
handle is held against the replay in tests/test_conf_denoise_gpu.py.  Bytes, np.array_equal."""
import numpy as np
import pytest

from leg_codec_model import LAW_U, PCMU
from test_conf_gpu import K, run
from test_host_conf_gpu import G, LAYOUT, SEED, T, host_conf
from test_host_tick_bridge_rtp_gpu import arrivals, fnv1a

pytestmark = pytest.mark.gpu

DTMF_FROM, DTMF_PACKETS = 5, 5


def ulaw_script():
    """--ulaw-every 1: every G.711 datagram carries payload type 0"""
    pk, recv = arrivals(SEED, T, G)
    audio = (recv > 0) & np.isin(pk[:, :, :, 1] & 0x7F, (8, 0))
    pk[:, :, :, 1] = np.where(audio, 0x80, pk[:, :, :, 1])
    return pk, recv


def dtmf_script(wmx):
    """--dtmf, as the head of examples/host_conf.c states it: in ticks 5 .. 9 leg 0 sends one packet of the key `5` -- two integer
    oscillators, A-law -- and leg 1 one RFC 4733 packet of `#`, in place of what the script had drawn; their sequence numbers go on
    counting the packets that arrive"""
    pk, recv = arrivals(SEED, T, G)
    osc, coef = [[0, -((4000 * 9315) >> 14)], [0, -((4000 * 14206) >> 14)]], (26956, 16325)
    for g in (0, 1):
        seq = 0
        for t in range(T):
            if not DTMF_FROM <= t < DTMF_FROM + DTMF_PACKETS:
                for k in np.flatnonzero(recv[t, g] > 0):
                    pk[t, g, k, 2], pk[t, g, k, 3] = (seq >> 8) & 255, seq & 255
                    seq = (seq + 1) & 0xFFFF
                continue
            row = np.zeros(172, np.uint8)
            row[0], row[2], row[3] = 0x80, (seq >> 8) & 255, seq & 255
            seq = (seq + 1) & 0xFFFF
            recv[t, g] = [172, 0, 0]
            if g == 0:
                row[1] = 0x88
                for i in range(160):
                    v = 0
                    for f in range(2):
                        y = ((coef[f] * osc[f][0]) >> 14) - osc[f][1]
                        osc[f][1], osc[f][0] = osc[f][0], y
                        v += y
                    row[12 + i] = wmx.linear2alaw(v)
            else:
                ts, duration = 160 * DTMF_FROM, 160 * (t - DTMF_FROM + 1)
                row[1] = (0x80 if t == DTMF_FROM else 0) | 101
                row[4:8] = [(ts >> 24) & 255, (ts >> 16) & 255, (ts >> 8) & 255, ts & 255]
                row[12], row[13] = 11, (0x80 if t == DTMF_FROM + DTMF_PACKETS - 1 else 0) | 10
                row[14], row[15] = (duration >> 8) & 255, duration & 255
                recv[t, g, 0] = 16
            pk[t, g, 0] = row
    return pk, recv


@pytest.mark.parametrize("extra", [(), ("--sequence", "3", "--conceal"), ("--ulaw-every", "1"), ("--dtmf",)])
def test_host_conf_denoise_sends_what_the_python_handle_sends(tmp_path, cuda, wmx, extra):
    from wmix_amd.conf import ConfBridge
    info, got = host_conf(tmp_path, "--denoise", *extra)
    plain, other = host_conf(tmp_path, *extra)
    assert info["rc"] == 0 and info["denoise"] == 1 and "denoise" not in plain and not np.array_equal(got, other)
    pk, recv = ulaw_script() if "--ulaw-every" in extra else (dtmf_script(wmx) if "--dtmf" in extra else arrivals(SEED, T, G))
    cb = ConfBridge(G, 3, K)
    cb.set_conferences(LAYOUT)
    if "--sequence" in extra:
        cb.sequence(True, 3)
        cb.conceal(True)
    if "--ulaw-every" in extra:
        cb.set_codecs(None, PCMU, LAW_U)
    if "--dtmf" in extra:
        cb.dtmf(True, suppress=True, event_pt=101)
    cb.denoise(True)
    want = run(cb, pk, recv, "ahead")
    keys = cb.export_dtmf()
    cb.close()
    assert info["datagrams_in"] == int((recv > 0).sum())
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert info["datagrams_fnv1a"] == fnv1a(want)
    if "--dtmf" in extra:  # the keypad is judged on the row as it arrived: both keys are read as without --denoise
        assert info["dtmf_keys"] == plain["dtmf_keys"] == [{"leg": 0, "key": "5", "packet": 0}, {"leg": 1, "key": "#", "packet": 1}]
        assert keys["count"].tolist() == [1, 1] + [0] * (G - 2)
    if "--sequence" in extra:
        assert info["concealed"] == plain["concealed"] > 0  # what is lost is lost before the suppressor
