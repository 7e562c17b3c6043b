"""examples/host_conf.c --sequence 3 --conceal: the C example with its legs sequenced and the gaps concealed (wmx_conf_conceal), at the
sizes tests/test_host_conf_sequence_gpu.py runs it.  Its default script holds datagrams of payload type 96, which consume a sequence
number and bring no audio -- gaps -- so there the datagrams and the counters are those of the Python handle with both switched on over
the same script; on an in-order script in which every datagram is audio the flag changes no datagram.  Bytes, np.array_equal."""
import numpy as np
import pytest

from conf_harness import host_conf, run
from conf_inputs import G, K, LAYOUT, SEED, T, arrivals, fnv1a

pytestmark = pytest.mark.gpu

COUNTERS = ("lost", "late", "dup", "resync", "overflow")


def test_host_conf_conceal_on_its_default_script_sends_what_the_python_handle_sends(tmp_path, cuda):
    from wmix_amd.conf import ConfBridge
    info, got = host_conf(tmp_path, "--sequence", "3", "--conceal")
    pk, recv = arrivals(SEED, T, G)
    cb = ConfBridge(G, 3, K)
    cb.set_conferences(LAYOUT)
    cb.sequence(True, 3)
    cb.conceal(True)
    want = run(cb, pk, recv, "ahead")
    st, concealed = cb.export_sequence(), cb.export_conceal()
    cb.close()
    assert info["rc"] == 0 and info["sequence"] == 3 and info["conceal"] == 1
    assert np.array_equal(got, want) and info["datagrams_fnv1a"] == fnv1a(want)
    assert [info[c] for c in COUNTERS] == [int(st[c].sum()) for c in COUNTERS]
    assert info["concealed"] == int(concealed.sum()) == info["lost"] > 0
    silent, other = host_conf(tmp_path, "--sequence", "3")
    assert not np.array_equal(got, other) and "conceal" not in silent and "concealed" not in silent


def test_host_conf_conceal_on_an_in_order_script_changes_no_datagram(tmp_path):
    plain, want = host_conf(tmp_path, "--audio-only", "--sequence", "3")
    info, got = host_conf(tmp_path, "--audio-only", "--sequence", "3", "--conceal")
    assert info["rc"] == 0 and info["conceal"] == 1 and info["concealed"] == 0 and info["lost"] == 0
    assert info["datagrams_fnv1a"] == plain["datagrams_fnv1a"] == fnv1a(want) and np.array_equal(got, want)
    assert (got[:, :9, 12:] != 0xD5).any()
