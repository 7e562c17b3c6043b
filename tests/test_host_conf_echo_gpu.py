"""examples/host_conf.c --echo D: the C example with every leg's rows going through the leg's own echo canceller (wmx_conf_echo), alone
and beside --sequence / --conceal and --denoise --level --gate, at the sizes tests/test_host_conf_gpu.py runs it.  The datagrams it sends
are those of ConfEchoReplay (tests/conf_echo_replay.py) with the same switches over the same script, and those of the Python handle,
which tests/test_conf_echo_gpu.py holds against the same replay.  Bytes, np.array_equal."""
import numpy as np
import pytest

from conf_echo_replay import replay_echo_story
from conf_harness import host_conf, run
from conf_inputs import G, K, LAYOUT, SEED, T, arrivals, fnv1a

pytestmark = pytest.mark.gpu

DELAY, VALUE = 20, 20


@pytest.mark.parametrize("extra", [(), ("--sequence", "3", "--conceal"), ("--denoise", "--level", str(VALUE), "--gate")])
def test_host_conf_echo_sends_what_the_replay_and_the_python_handle_send(tmp_path, cuda, oracle_port, extra):
    from wmix_amd.conf import ConfBridge
    info, got = host_conf(tmp_path, "--echo", str(DELAY), *extra)
    plain, other = host_conf(tmp_path, *extra)
    assert info["rc"] == 0 and info["echo"] == DELAY and not np.array_equal(got, other)
    assert not {"echo", "echo_running"} & set(plain)
    pk, recv = arrivals(SEED, T, G)

    def setup(c):
        c.set_conferences(LAYOUT)
        if "--sequence" in extra:
            c.sequence(True, 3)
            c.conceal(True)
        if "--denoise" in extra:
            c.denoise(True)
            c.level(True, VALUE)
            c.gate(True)
        c.echo(True, DELAY)

    want, _, m = replay_echo_story(oracle_port, G, K, pk, recv, setup)
    cb = ConfBridge(G, 3, K)
    setup(cb)
    sent = run(cb, pk, recv, "ahead")
    st = cb.export_echo()
    cb.close()
    assert info["datagrams_in"] == int((recv > 0).sum())
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert np.array_equal(sent, want) and info["datagrams_fnv1a"] == fnv1a(want)
    assert info["echo_running"] == int((st["startup"] == 0).sum()) == int((m.export_echo()["startup"] == 0).sum()) > 0


def test_host_conf_without_the_flag_has_no_echo_key(tmp_path, cuda):
    info, _ = host_conf(tmp_path)
    assert info["rc"] == 0 and not {"echo", "echo_running"} & set(info)
