"""examples/host_conf.c --dtmf: the C example listening to its legs' keypads with suppression on (wmx_conf_dtmf), at the sizes
tests/test_host_conf_gpu.py runs it.  Leg 0 presses `5` in band and leg 1 sends `#` as RFC 4733 packets; both are read back through the
C ABI, and the legs of the other conferences are sent what they are sent without the flag.  Bytes, np.array_equal."""
import numpy as np
import pytest

from conf_harness import host_conf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra", [(), ("--sequence", "3", "--conceal"), ("--ulaw-every", "1")])
def test_host_conf_dtmf_reads_both_keys_back(tmp_path, extra):
    plain, want = host_conf(tmp_path, *extra)
    info, got = host_conf(tmp_path, "--dtmf", *extra)
    assert info["rc"] == 0 and info["dtmf"] == 1 and "dtmf" not in plain and "dtmf_keys" not in plain
    assert info["dtmf_keys"] == [{"leg": 0, "key": "5", "packet": 0}, {"leg": 1, "key": "#", "packet": 1}], info["dtmf_keys"]
    # legs 0 and 1 are one conference: nobody else's datagrams change
    assert np.array_equal(got[:, 2:], want[:, 2:]) and not np.array_equal(got[:, :2], want[:, :2])
    # leg 1 hears leg 0 alone: the 100 ms of the key, suppressed, reach it as silence.  Wherever leg 0's cursor stands against the play
    # head they cover four whole datagrams; the script without the flag has noise there, but for a tick in four where nothing arrives
    silence = 0xFF if extra == ("--ulaw-every", "1") else 0xD5
    quiet = [int((out[:, 1, 12:] == silence).all(1).sum()) for out in (got, want)]
    assert quiet[0] >= quiet[1] + 3, quiet
