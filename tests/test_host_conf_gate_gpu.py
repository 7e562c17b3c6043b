"""examples/host_conf.c --gate: the C example with every leg's rows going through the leg's own voice-activity gate (wmx_conf_gate),
alone and beside --sequence / --conceal, --denoise --level and --dtmf, at the sizes tests/test_host_conf_gpu.py runs it.  The datagrams
it sends are those of the Python handle with the same switches over the same script, as in tests/test_host_conf_level_gpu.py; that
handle is held against the replay in tests/test_conf_gate_gpu.py.  Bytes, np.array_equal."""
import numpy as np
import pytest

from conf_harness import host_conf, run
from conf_inputs import G, K, LAYOUT, SEED, T, arrivals, dtmf_script, fnv1a

pytestmark = pytest.mark.gpu

VALUE = 20


@pytest.mark.parametrize("extra", [(), ("--sequence", "3", "--conceal"), ("--denoise", "--level", str(VALUE)), ("--dtmf",)])
def test_host_conf_gate_sends_what_the_python_handle_sends(tmp_path, cuda, wmx, extra):
    from wmix_amd.conf import ConfBridge
    info, got = host_conf(tmp_path, "--gate", *extra)
    plain, other = host_conf(tmp_path, *extra)
    assert info["rc"] == 0 and info["gate"] == 1 and not np.array_equal(got, other)
    assert not {"gate", "voiced", "unvoiced"} & set(plain)
    pk, recv = dtmf_script(wmx) if "--dtmf" in extra else arrivals(SEED, T, G)
    cb = ConfBridge(G, 3, K)
    cb.set_conferences(LAYOUT)
    if "--sequence" in extra:
        cb.sequence(True, 3)
        cb.conceal(True)
    if "--dtmf" in extra:
        cb.dtmf(True, suppress=True, event_pt=101)
    if "--denoise" in extra:
        cb.denoise(True)
        cb.level(True, VALUE)
    cb.gate(True)
    want = run(cb, pk, recv, "ahead")
    keys = cb.export_dtmf() if "--dtmf" in extra else None
    st = cb.export_gate()
    assert cb.gater_state(0) is not None
    cb.close()
    assert info["datagrams_in"] == int((recv > 0).sum())
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert info["datagrams_fnv1a"] == fnv1a(want)
    assert info["voiced"] == int(st["voiced"].sum()) > 0 and info["unvoiced"] == int(st["unvoiced"].sum())
    if "--dtmf" in extra:  # the keypad is judged on the row as it arrived: both keys are read as without --gate
        assert info["dtmf_keys"] == plain["dtmf_keys"] == [{"leg": 0, "key": "5", "packet": 0}, {"leg": 1, "key": "#", "packet": 1}]
        assert keys["count"].tolist() == [1, 1] + [0] * (G - 2)
    if "--sequence" in extra:
        assert info["concealed"] == plain["concealed"] > 0  # what is lost is lost before the gate
    if "--denoise" in extra:
        assert info["denoise"] == 1 and info["level"] == VALUE


def test_host_conf_without_the_flag_has_no_gate_key(tmp_path, cuda):
    info, _ = host_conf(tmp_path)
    assert info["rc"] == 0 and not {"gate", "voiced", "unvoiced"} & set(info)
