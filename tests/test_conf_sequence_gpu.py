"""wmx_conf_sequence (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with its legs reordered, de-duplicated and
gap-filled by RTP sequence number.  The layout, T and K are those of tests/test_conf_gpu.py; the script generator is this file's own --
every packet is audio (PCMA or PCMU), so that a clean script has no gap.  The reference for an impaired script is the tick-by-tick
replay of tests/test_conf_gpu.py (one reference ring per leg, a cursor per source leg) fed the REPAIRED rows: the call lists of
tests/leg_seq_model.py laid out as four slots, a silence call being a row of zeros.  Bytes and integers, np.array_equal."""
import numpy as np
import pytest

from leg_seq_model import COUNTERS, LegsSeqModel, repaired_rows
from speakers_legs_model import SpeakersLegsModel
from test_conf_gpu import G, K, LAYOUT, T, Replay, bridge, run

pytestmark = pytest.mark.gpu

IN_CONF = sorted(g for c in LAYOUT for g in c)
QUIET = np.array([0xD5, 0x55, 0xD4, 0x54, 0xD7, 0x57], np.uint8)  # A-law codes of the smallest samples


def clean_script(seed, steady=False, quiet=False, legs=G, ticks=T):
    """packets[t][g]: the list of (seq, payload type, 160 codes) that leg g delivers in tick t, in order, every one PCMA or PCMU.
    steady: one packet per tick and leg; else none, one or two.  The legs start at different numbers, one just below the uint16 wrap."""
    rng = np.random.default_rng(seed)
    seq = [int(s) for s in rng.choice([0, 65520, 1234, 40000], size=legs)]
    seq[2] = 65520
    packets = []
    for t in range(ticks):
        packets.append([])
        for g in range(legs):
            now = []
            for _ in range(1 if steady else int(rng.choice([0, 1, 1, 1, 1, 2]))):
                codes = rng.choice(QUIET, size=160) if quiet else rng.integers(0, 256, size=160).astype(np.uint8)
                now.append((seq[g], int(rng.choice([8, 8, 0])), codes))
                seq[g] = (seq[g] + 1) % 65536
            packets[t].append(now)
    return packets


def impair(packets, seed, in_conf=IN_CONF, ticks=T, slots=K, restarts=((1, 12), (4, 20), (7, 28))):
    """-> (the impaired script, how often each kind was applied on a leg that is in a conference): packets swapped inside a tick,
    sent twice, lost (the number is consumed, nothing arrives), delivered a tick late, and three senders that restart at a far number.
    No leg ends up with more than `slots` packets in a tick."""
    rng = np.random.default_rng(seed)
    out = [[list(now) for now in tick] for tick in packets]
    kinds = dict.fromkeys(("swap", "dup", "loss", "late", "restart"), 0)
    for g, since in restarts:
        for t in range(since, ticks):
            out[t][g] = [((s + 20000) % 65536, pt, codes) for s, pt, codes in out[t][g]]
        kinds["restart"] += 1
    for t in range(2, ticks - 1):
        for g in in_conf:
            now, what = out[t][g], int(rng.integers(0, 12))
            if what == 0 and len(now) == 2:
                now.reverse()
                kinds["swap"] += 1
            elif what == 1 and 1 <= len(now) < slots:
                now.insert(int(rng.integers(0, len(now) + 1)), now[int(rng.integers(0, len(now)))])
                kinds["dup"] += 1
            elif what == 2 and now:
                now.pop(int(rng.integers(0, len(now))))
                kinds["loss"] += 1
            elif what in (3, 4) and now and len(out[t + 1][g]) < slots:
                out[t + 1][g].insert(0, now.pop(0))  # of two, the first: the second is loaded before it comes
                kinds["late"] += 1
    return out, kinds


def rows_of(packets, seed=1, legs=G, ticks=T, slots=K):
    """the script as the handle takes it: datagram rows [T, G, K, 172] and what recvfrom returned [T, G, K]; now and then slot 1 is a
    failed recvfrom between two datagrams, or the only datagram sits in slot 2 (with other slot counts: the slot in front of the last,
    the last)"""
    rng = np.random.default_rng(seed)
    pk, recv = np.full((ticks, legs, slots, 172), 0xEE, np.uint8), np.zeros((ticks, legs, slots), np.int32)
    for t in range(ticks):
        for g in range(legs):
            now = packets[t][g]
            assert len(now) <= slots
            at = list(range(len(now)))
            if len(now) < slots and now and rng.integers(0, 4) == 0:
                at[-1] = slots - 1
                recv[t, g, slots - 2] = -1
            for k, (s, pt, codes) in zip(at, now):
                recv[t, g, k] = 172
                pk[t, g, k, :12] = 0
                pk[t, g, k, 0], pk[t, g, k, 1] = 0x80, 0x80 | pt
                pk[t, g, k, 2], pk[t, g, k, 3] = s >> 8, s & 255
                pk[t, g, k, 12:] = codes
    return pk, recv


def seq_raw_of(pk_t, recv_t):
    """what wmx_rtp_ingest_legs leaves: header bytes 2..3 as stored for a slot where something arrived, 0 otherwise"""
    raw = pk_t[:, :, 2].astype(np.uint16) | (pk_t[:, :, 3].astype(np.uint16) << 8)
    return np.where(recv_t > 0, raw, 0).astype(np.uint16)


def replay_seq(lib, pk, recv, max_gap=3, fresh_at=None, select=None, rewrite=True):
    """the tick-by-tick replay fed the model's repaired rows -> (datagrams [T, G, 172], the model, per tick (speaking, env)).
    rewrite=False: the selection is fed the lens as ingest left them (what the device must NOT do)"""
    rp, model, spk = Replay(lib, G), LegsSeqModel(G), SpeakersLegsModel(G)
    out, sel = np.zeros((T, G, 172), np.uint8), []
    for t in range(T):
        if fresh_at and t in fresh_at:
            rp.fresh(fresh_at[t])
            model.reset(fresh_at[t])
            spk.reset(fresh_at[t])
        pcm, lens = rp.decode(pk[t], recv[t])
        _, new_lens, lists = model.tick(seq_raw_of(pk[t], recv[t]), lens, max_gap)
        mute = None
        if select:
            sp, mute = spk.step_legs(LAYOUT, pcm, new_lens if rewrite else lens, 320, select[0], select[1], select[2], None)
            sel.append((sp.copy(), spk.env.copy()))
        rows, rlens = repaired_rows(pcm, lists)
        out[t] = rp.tick(rows, rlens, LAYOUT, mute)
    return out, model, sel


def counters_equal(cb, model):
    got, want = cb.export_sequence(), model.export()
    for name in want:
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])


@pytest.fixture(scope="module")
def clean(cuda):
    pk, recv = rows_of(clean_script(1))
    cb = bridge()
    off = run(cb, pk, recv, "ahead")
    cb.close()
    return pk, recv, off


@pytest.mark.parametrize("slots,mode", [(1, "wait"), (3, "ahead"), (3, "resident")])
def test_a_clean_script_is_sent_as_with_sequencing_off(cuda, clean, slots, mode):
    pk, recv, off = clean
    cb = bridge(slots=slots)
    cb.sequence(True)
    got = run(cb, pk, recv, mode)
    assert np.array_equal(got, off), np.argwhere((got != off).any(2))[:6]
    st = cb.export_sequence()
    assert not any(st[name].any() for name in COUNTERS) and st["synced"].all()
    assert (off[:, IN_CONF, 12:] != 0xD5).any()
    cb.close()


def test_an_impaired_script_is_sent_as_the_replay_of_the_repaired_rows(cuda, oracle_port):
    script, kinds = impair(clean_script(2), 3)
    assert all(n >= 3 for n in kinds.values()), kinds  # on legs that are in a conference
    pk, recv = rows_of(script)
    want, model, _ = replay_seq(oracle_port, pk, recv)
    plain, clean_model, _ = replay_seq(oracle_port, *rows_of(clean_script(2)))
    assert not any(clean_model.export()[name].any() for name in COUNTERS) and not np.array_equal(want, plain)
    seen = model.export()
    assert all(seen[name][IN_CONF].sum() >= 3 for name in ("lost", "late", "dup", "resync")), {n: seen[n] for n in COUNTERS}
    for slots, mode in ((3, "ahead"), (3, "resident")):
        cb = bridge(slots=slots)
        cb.sequence(True, 3)
        got = run(cb, pk, recv, mode)
        assert np.array_equal(got, want), (mode, np.argwhere((got != want).any(2))[:6])
        counters_equal(cb, model)
        assert not cb.export_legs()["dropped"].any()
        cb.close()
    # sequencing off, the same script is sent otherwise
    cb = bridge()
    got = run(cb, pk, recv, "ahead")
    assert not np.array_equal(got, want)
    cb.close()


def test_lost_packets_do_not_shift_a_legs_cursor(cuda):
    """What the feature is for.  Losses only, on a steady script: with sequencing on every leg's cursor ends where the lossless run's
    ends; with it off, 320 bytes earlier per lost packet."""
    steady = clean_script(4, steady=True)
    rng = np.random.default_rng(5)
    lossy, lost = [[list(now) for now in tick] for tick in steady], np.zeros(G, np.uint32)
    for g in IN_CONF:
        for t in sorted(rng.choice(np.arange(4, T - 4), size=int(rng.integers(1, 5)), replace=False)):
            lossy[t][g] = []
            lost[g] += 1
    assert lost[IN_CONF].all() and lost.sum() >= 15

    def ticks_after(script, on):
        cb = bridge()
        cb.sequence(on, 3)
        run(cb, *rows_of(script), "ahead")
        st, sq = cb.export_legs(), cb.export_sequence()
        cb.close()
        return st["tick"].astype(np.int64), sq

    lossless, _ = ticks_after(steady, False)
    assert (lossless[IN_CONF] == lossless[0]).all() and lossless[9] == 0
    on, sq = ticks_after(lossy, True)
    assert np.array_equal(on, lossless) and np.array_equal(sq["lost"], lost)
    off, _ = ticks_after(lossy, False)
    assert np.array_equal(off, lossless - 320 * lost.astype(np.int64))


def test_talker_selection_does_not_hear_a_late_packet(cuda, oracle_port):
    """Leg 6's packet of tick 10 is the loudest thing its conference ever hears, and it arrives at tick 12, behind the packets of ticks
    11 and 12: late.  The selection runs on the rewritten d_len, so leg 6 is not the talker because of it."""
    script = clean_script(6, steady=True, quiet=True)
    s, pt, _ = script[10][6][0]
    script[12][6].append((s, 8, np.tile(np.array([0x2A, 0xAA], np.uint8), 80)))
    script[10][6] = []
    pk, recv = rows_of(script)
    select = (1, 0, 3)
    want, model, sel = replay_seq(oracle_port, pk, recv, select=select)
    _, _, deaf = replay_seq(oracle_port, pk, recv, select=select, rewrite=False)
    assert model.export()["late"][6] == 1 and model.export()["lost"][6] == 1
    assert not np.array_equal(sel[12][1], deaf[12][1]) and deaf[12][0][6] == 1  # fed the lens as ingest left them, leg 6 would speak
    seen = []
    cb = bridge()
    cb.sequence(True, 3)
    cb.speakers(*select)
    got = run(cb, pk, recv, "ahead", after=lambda t, c: seen.append(c.export_legs()))
    for t in range(T):
        assert np.array_equal(seen[t]["speaking"], sel[t][0]) and np.array_equal(seen[t]["env"], sel[t][1]), ("speaking / env, tick", t)
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    counters_equal(cb, model)
    cb.close()


def test_a_new_call_may_start_at_any_sequence_number(cuda, oracle_port):
    """reset_legs on leg 3 at tick 15; from then on its sender counts from an unrelated number.  No resync and nothing late is counted,
    and every datagram is the replay's in which leg 3's ring, cursor, sender and sequence state were made fresh at tick 15."""
    script = clean_script(7, steady=True)
    for t in range(15, T):
        script[t][3] = [((s + 30000) % 65536, pt, codes) for s, pt, codes in script[t][3]]
    pk, recv = rows_of(script)
    want, model, _ = replay_seq(oracle_port, pk, recv, fresh_at={15: [3]})
    stale, stale_model, _ = replay_seq(oracle_port, pk, recv)
    assert stale_model.export()["resync"][3] == 1 and not any(model.export()[name].any() for name in COUNTERS)
    cb = bridge()
    cb.sequence(True, 3)
    got = run(cb, pk, recv, "ahead", before={15: lambda c: c.reset_legs([3])})
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    counters_equal(cb, model)
    assert got[15, 3, 2:4].tolist() == [0, 0] and not np.array_equal(got[15:, 3], stale[15:, 3])
    cb.close()


def test_sequence_refusals(cuda, wmx):
    from test_bridge_gpu import EINVAL
    cb = bridge()
    assert wmx.wmx_conf_sequence(cb._h, 1, 4) == EINVAL and wmx.wmx_conf_sequence(cb._h, 1, -1) == EINVAL
    assert wmx.wmx_conf_sequence(None, 1, 3) == EINVAL
    assert wmx.wmx_conf_export_sequence(None, None, None, None, None, None, None, None, None) == EINVAL
    st = cb.export_sequence()
    assert not any(st[name].any() for name in st)
    cb.close()
