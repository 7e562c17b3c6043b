"""examples/host_conf.c --denoise: the C example with every leg's rows going through the leg's own noise suppressor (wmx_conf_denoise),
alone and beside --sequence / --conceal, --ulaw-every and --dtmf, at the sizes tests/test_host_conf_gpu.py runs it.  The datagrams it
sends are those of the Python handle with the same switches over the same script, as in tests/test_host_conf_conceal_gpu.py; that
handle is held against the replay in tests/test_conf_denoise_gpu.py.  Bytes, np.array_equal."""
import numpy as np
import pytest

from conf_harness import host_conf, run
from conf_inputs import G, K, LAYOUT, SEED, T, arrivals, dtmf_script, fnv1a, ulaw_every_script
from leg_codec_model import LAW_U, PCMU

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("extra", [(), ("--sequence", "3", "--conceal"), ("--ulaw-every", "1"), ("--dtmf",)])
def test_host_conf_denoise_sends_what_the_python_handle_sends(tmp_path, cuda, wmx, extra):
    from wmix_amd.conf import ConfBridge
    info, got = host_conf(tmp_path, "--denoise", *extra)
    plain, other = host_conf(tmp_path, *extra)
    assert info["rc"] == 0 and info["denoise"] == 1 and "denoise" not in plain and not np.array_equal(got, other)
    pk, recv = ulaw_every_script(range(G)) if "--ulaw-every" in extra else (dtmf_script(wmx) if "--dtmf" in extra else arrivals(SEED, T, G))
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
