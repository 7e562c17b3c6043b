"""examples/host_conf.c --sequence G: the C example with its legs sequenced (wmx_conf_sequence).  On an in-order script in which every
datagram is audio (--audio-only) it sends what it sends without the flag, and every counter is zero.  Its default script holds datagrams
of payload type 96, which consume a sequence number and bring no audio -- gaps to the sequencer -- so there the datagrams and the counters
are those of the Python handle with sequencing on over the same script.  Bytes, np.array_equal."""
import numpy as np
import pytest

from conf_harness import host_conf, run
from conf_inputs import G, K, LAYOUT, SEED, T, arrivals, fnv1a

pytestmark = pytest.mark.gpu

COUNTERS = ("lost", "late", "dup", "resync", "overflow")


def test_host_conf_sequence_on_an_in_order_script_changes_no_datagram(tmp_path):
    plain, want = host_conf(tmp_path, "--audio-only")
    info, got = host_conf(tmp_path, "--audio-only", "--sequence", "3")
    assert info["rc"] == 0 and info["sequence"] == 3 and "sequence" not in plain and "lost" not in plain
    assert info["datagrams_fnv1a"] == plain["datagrams_fnv1a"] == fnv1a(want) and np.array_equal(got, want)
    assert [info[c] for c in COUNTERS] == [0] * 5 and info["datagrams_in"] == plain["datagrams_in"] > T * G // 2
    assert (got[:, :9, 12:] != 0xD5).any()


def test_host_conf_sequence_on_its_default_script_sends_what_the_python_handle_sends(tmp_path, cuda):
    from wmix_amd.conf import ConfBridge
    info, got = host_conf(tmp_path, "--sequence", "3")
    pk, recv = arrivals(SEED, T, G)
    cb = ConfBridge(G, 3, K)
    cb.set_conferences(LAYOUT)
    cb.sequence(True, 3)
    want = run(cb, pk, recv, "ahead")
    st = cb.export_sequence()
    cb.close()
    assert np.array_equal(got, want) and [info[c] for c in COUNTERS] == [int(st[c].sum()) for c in COUNTERS]
    assert info["lost"] > 0 and info["late"] == info["dup"] == 0  # the datagrams of payload type 96, and nothing else
    plain, other = host_conf(tmp_path)
    assert not np.array_equal(got, other) and "sequence" not in plain
