"""paced_groups(.., try_submit=..) (wmix_amd/realtime.py) without a GPU: the late-tick policy of the paced heartbeat.  With a period
shorter than the tick, the default loop queues every release behind the tick in flight and the latency grows without bound (the backlog
never drains); with try_submit a release that finds its group's previous tick still on its way is shed, the latency stays one tick, and
the drops follow from the arithmetic.  Fake "devices" that take a fixed time stand in for wmx_rt, on a virtual clock as in
tests/test_paced_logic.py."""
import math

import numpy as np
import pytest


class _Clock:
    def __init__(self):
        self.t = 100.0

    def perf_counter(self):
        self.t += 1e-6
        return self.t

    def sleep(self, s):
        self.t += max(0.0, s)


@pytest.fixture
def clock(monkeypatch):
    from wmix_amd import realtime
    c = _Clock()
    monkeypatch.setattr(realtime, "time", c)
    return c


class _Devices:
    """one device per group: a tick submitted at t is back at max(t, when the group's previous tick is back) + tick_ms"""

    def __init__(self, clock, tick_ms):
        self.clock, self.tick = clock, tick_ms * 1e-3
        self.done_at, self.queued_behind_itself, self.submitted, self.shed = {}, 0, 0, 0

    def submit(self, g):
        now = self.clock.perf_counter()
        if self.done_at.get(g, 0.0) > now:
            self.queued_behind_itself += 1
        self.done_at[g] = max(now, self.done_at.get(g, 0.0)) + self.tick
        self.submitted += 1

    def try_submit(self, g):
        if self.done_at.get(g, 0.0) > self.clock.perf_counter():
            self.shed += 1
            return False
        self.submit(g)
        return True

    def poll(self, g):
        return self.clock.perf_counter() >= self.done_at[g]

    def wait(self, g):
        self.clock.t = max(self.clock.t, self.done_at[g])


def test_queue_falls_behind_for_good(clock):
    from wmix_amd.realtime import latency_summary, paced_groups
    d = _Devices(clock, 12.0)
    lat, lag, _ = paced_groups(d.submit, d.poll, d.wait, 1, 5.0, 60)
    assert not np.isnan(lat).any() and d.submitted == 60
    assert np.all(np.diff(lat) > 6.9) and lat[-1] > 59 * 7.0  # every tick 7 ms later than the one before: no bound
    s = latency_summary(lat, lag, 5.0)
    assert "dropped" not in s and s["misses"] == 60


@pytest.mark.parametrize("groups,period_ms,tick_ms", [(1, 5.0, 8.0), (1, 5.0, 12.0), (3, 20.0, 27.0), (4, 10.0, 19.5)])
def test_drop_bounds_the_latency(clock, groups, period_ms, tick_ms):
    from wmix_amd.realtime import latency_summary, paced_groups
    n_ticks = 60
    d = _Devices(clock, tick_ms)
    seen = []
    lat, lag, _ = paced_groups(d.submit, d.poll, d.wait, groups, period_ms, n_ticks, after=lambda j, g: seen.append(j), try_submit=d.try_submit)
    dropped = np.isnan(lat)
    assert np.array_equal(dropped, np.isnan(lag)) and d.queued_behind_itself == 0
    # a group's tick is back tick_ms after it went; the next release that finds it back is ceil(tick / period) periods later
    every = math.ceil(tick_ms / period_ms)
    assert d.shed == int(dropped.sum()) == groups * (n_ticks - math.ceil(n_ticks / every))
    assert d.submitted == groups * n_ticks - d.shed and sorted(seen) == list(np.flatnonzero(~dropped))
    kept = lat[~dropped]
    assert kept.max() <= tick_ms + period_ms and kept.min() >= tick_ms
    s = latency_summary(lat, lag, period_ms, dropped=dropped)
    assert s["dropped"] == d.shed and s["ticks"] == d.submitted and s["max_ms"] <= tick_ms + period_ms
    assert not np.isnan(lat[s["worst_tick"]])


def test_drop_changes_nothing_below_capacity(clock):
    """a tick shorter than the period is never shed: the same latencies as the default loop"""
    from wmix_amd.realtime import latency_summary, paced_groups
    d = _Devices(clock, 3.0)
    lat, lag, _ = paced_groups(d.submit, d.poll, d.wait, 4, 20.0, 30, try_submit=d.try_submit)
    assert d.shed == 0 and not np.isnan(lat).any() and lat.max() < 3.1
    assert latency_summary(lat, lag, 20.0, dropped=np.isnan(lat))["dropped"] == 0
