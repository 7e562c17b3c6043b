"""What the conference tests feed the handle, its models and the C examples: the family's shape, the scripted arrivals and the G.711
codes.  numpy and tests/leg_dtmf_model.py's signals only: no oracle, no GPU, nothing of wmix_amd."""
import numpy as np

from leg_dtmf_model import block_digit, tone

LAYOUT = [[0, 1], [2, 3, 4], [5, 6, 7, 8]]  # leg 9 is in no conference
T, G, K, SEED = 40, 10, 3, 20260
IN_CONF = sorted(g for c in LAYOUT for g in c)
EINVAL, NULL_HEAD = -10001, 0xFFFFFFFF  # what the C ABI refuses with; the head of a cursor that has never loaded

MASK = (1 << 64) - 1
QUIET = np.array([0xD5, 0x55, 0xD4, 0x54, 0xD7, 0x57], np.uint8)  # A-law codes of the smallest samples
ZERO = np.full(160, 0xFF, np.uint8)  # mu-law: 160 samples of 0
# the legs of the codec tests: who negotiated what, who changes its codec and who is a new call, and when
ULAW_LEGS, BY_PT_LEG, STRICT_A_LEG, LATER_ULAW_LEG, CHANGE_AT, RESET_LEG, RESET_AT = [1, 3, 6], 4, 7, 2, 15, 6, 25
EVERY = 3  # examples/host_conf.c --ulaw-every 3
ULAW = [g for g in range(G) if g % EVERY == EVERY - 1]


# ---------------------------------------------------------------- the C examples' script
class Lcg:
    def __init__(self, seed):
        self.s = seed

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & MASK
        return self.s >> 33


def arrivals(seed, T, G):
    """the example's script (examples/host_tick.c, bridge_rtp): datagram rows [T, G, 3, 172] and what recvfrom returned [T, G, 3]"""
    rnd = Lcg(seed)
    pk = np.full((T, G, 3, 172), 0xEE, np.uint8)
    recv = np.zeros((T, G, 3), np.int32)
    seq = [0] * G
    for t in range(T):
        for g in range(G):
            u = rnd.next() % 8
            recv[t, g] = [172 if u >= 2 else 0, 172 if u == 2 else (-1 if u == 3 else 0), 172 if u == 3 else 0]
            for k in range(3):
                if recv[t, g, k] <= 0:
                    continue
                v = rnd.next() % 16
                pk[t, g, k, :12] = 0
                pk[t, g, k, 0] = 0x80
                pk[t, g, k, 1] = 0x80 | (96 if v == 0 else (0 if v == 1 else 8))
                pk[t, g, k, 2], pk[t, g, k, 3] = (seq[g] >> 8) & 255, seq[g] & 255
                seq[g] = (seq[g] + 1) & 0xFFFF
                pk[t, g, k, 12:] = [rnd.next() & 255 for _ in range(160)]
    return pk, recv


def fnv1a(data):
    h = 1469598103934665603
    for b in data.tobytes():
        h = ((h ^ b) * 1099511628211) & MASK
    return "%016x" % h


def ulaw_every_script(legs=ULAW):
    """the example's script under --ulaw-every: arrivals() with every G.711 datagram of a mu-law leg carrying payload type 0"""
    pk, recv = arrivals(SEED, T, G)
    for g in legs:
        audio = (recv[:, g] > 0) & np.isin(pk[:, g, :, 1] & 0x7F, (8, 0))
        pk[:, g, :, 1] = np.where(audio, 0x80, pk[:, g, :, 1])
    return pk, recv


DTMF_FROM, DTMF_PACKETS = 5, 5


def dtmf_script(wmx):
    """--dtmf, as the head of examples/host_conf.c states it: in ticks 5 .. 9 leg 0 sends one packet of the key `5` -- two integer
    oscillators, A-law (wmx.linear2alaw) -- and leg 1 one RFC 4733 packet of `#`, in place of what the script had drawn; their sequence
    numbers go on counting the packets that arrive"""
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


# ---------------------------------------------------------------- G.711
def alaw_decode(codes):
    """G.711 A-law codes -> int16 (ITU-T G.711, the usual table-free form)"""
    c = np.asarray(codes, np.int64) ^ 0x55
    seg, mant = (c >> 4) & 7, c & 15
    mag = np.where(seg == 0, (mant << 4) + 8, ((mant << 4) + 0x108) << np.maximum(seg - 1, 0))
    return np.where(c & 0x80, mag, -mag).astype(np.int16)


def ulaw_decode(codes):
    """G.711 mu-law codes -> int16"""
    c = ~np.asarray(codes, np.int64) & 0xFF
    mag = ((((c & 15) << 3) + 0x84) << ((c >> 4) & 7)) - 0x84
    return np.where(c & 0x80, -mag, mag).astype(np.int16)


def ulaw_encode(x):
    """int16 -> G.711 mu-law codes (sign, segment, mantissa of the biased magnitude, inverted)"""
    out = np.zeros(len(x), np.uint8)
    for i, v in enumerate(int(s) for s in x):
        mag = min(abs(v), 32635) + 0x84
        seg = mag.bit_length() - 8
        out[i] = ~((0x80 if v < 0 else 0) | (seg << 4) | ((mag >> (seg + 3)) & 0xF)) & 0xFF
    return out


# ---------------------------------------------------------------- scripts of audio packets, impaired and laid out as rows
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


# ---------------------------------------------------------------- a codec per leg
def rewritten_script():
    """arrivals() with the payload type of every G.711 datagram rewritten: 0 on the mu-law legs (and on leg 2 from the tick it goes to
    mu-law), alternating 8 / 0 per packet on the BY_PT leg, 8 with every fifth packet 0 on the strict A-law leg.  Payload type 96
    (one packet in sixteen) stays on every leg, the default legs keep their 8s and 0s."""
    pk, recv = arrivals(SEED, T, G)
    nth = [0] * G
    for t in range(T):
        for g in range(G):
            for k in range(K):
                if recv[t, g, k] <= 0 or (pk[t, g, k, 1] & 0x7F) not in (8, 0):
                    continue
                pt = pk[t, g, k, 1] & 0x7F
                if g in ULAW_LEGS or (g == LATER_ULAW_LEG and t >= CHANGE_AT):
                    pt = 0
                elif g == BY_PT_LEG:
                    pt = 8 if nth[g] % 2 == 0 else 0
                elif g == STRICT_A_LEG:
                    pt = 0 if nth[g] % 5 == 4 else 8
                nth[g] += 1
                pk[t, g, k, 1] = 0x80 | pt
    return pk, recv


def retyped(packets, ulaw_from=None):
    """the payload types of a script rewritten per leg, by the rule of rewritten_script(): 0 on the mu-law legs (and on the legs of
    ulaw_from = {leg: tick} from that tick), alternating 8 / 0 per packet on the BY_PT leg, 8 with every fifth packet 0 on the strict
    A-law leg; the default legs keep their 8s and 0s"""
    nth, out = {}, []
    for t, tick in enumerate(packets):
        out.append([])
        for g, now in enumerate(tick):
            new = []
            for s, pt, codes in now:
                n = nth.get(g, 0)
                if g in ULAW_LEGS or (ulaw_from and g in ulaw_from and t >= ulaw_from[g]):
                    pt = 0
                elif g == BY_PT_LEG:
                    pt = 8 if n % 2 == 0 else 0
                elif g == STRICT_A_LEG:
                    pt = 0 if n % 5 == 4 else 8
                nth[g] = n + 1
                new.append((s, pt, codes))
            out[-1].append(new)
    return out


def gap_behind(script, g, t):
    """leg g delivers one packet in tick t and in tick t + 1 what it delivered anyway, which starts two numbers on: a gap of one in the
    tick behind a reset_legs at t (where it delivered nothing in tick t + 1: the packet in front of its next one)"""
    if not script[t + 1][g]:
        s, pt, codes = next(now[g][0] for now in script[t + 2:] if now[g])
        script[t + 1][g] = [((s - 1) % 65536, pt, codes[::-1].copy())]
    s, pt, codes = script[t + 1][g][0]
    script[t][g] = [((s - 2) % 65536, pt, codes[::-1].copy())]


# ---------------------------------------------------------------- keys, tones, noise and voices
def key_codes(code, packets):
    """the key as mu-law packets, every one of which the rule calls a tone of `code` once decoded"""
    rows = [ulaw_encode(tone(code, 4000.0, 4500.0, n0=160 * i, ph_row=0.4, ph_col=1.9)) for i in range(packets)]
    assert all(block_digit(ulaw_decode(r)) == code for r in rows)
    return rows


KEY_TICKS, KEY_LEG, EVENT_LEG, KEY_AT = 24, 6, 3, 10  # key_script(): leg 6 presses in band from tick 10 on, leg 3 sends event packets


def key_script(code=5, packets=5, events=()):
    """-> (datagram rows, recv) of KEY_TICKS ticks: quiet talkers, one packet per tick and leg; leg 6 sends zeros, and from tick KEY_AT
    on `packets` packets of the key (0: none); events: (tick, event, timestamp, end) packets leg 3 sends behind its audio"""
    script = clean_script(3, steady=True, quiet=True, ticks=KEY_TICKS)
    keys = key_codes(code, packets)
    for t in range(KEY_TICKS):
        s, _, _ = script[t][KEY_LEG][0]
        script[t][KEY_LEG] = [(s, 0, keys[t - KEY_AT] if KEY_AT <= t < KEY_AT + packets else ZERO)]
    for t, event, ts, end in events:
        s = script[t][EVENT_LEG][-1][0]
        payload = np.zeros(160, np.uint8)
        payload[:4] = [event, (0x80 if end else 0) | 10, 0, 160]
        script[t][EVENT_LEG].append(((s + 100) % 65536, 101, payload))
    pk, recv = rows_of(script, ticks=KEY_TICKS)
    for t, event, ts, end in events:
        k = [k for k in range(pk.shape[2]) if recv[t, EVENT_LEG, k] > 0 and (pk[t, EVENT_LEG, k, 1] & 0x7F) == 101]
        assert len(k) == 1
        pk[t, EVENT_LEG, k[0], 4:8] = [(ts >> 24) & 0xFF, (ts >> 16) & 0xFF, (ts >> 8) & 0xFF, ts & 0xFF]
    return pk, recv


def with_key(script, at=22, packets=5):
    """leg 6 -- it negotiated mu-law in the codec tests -- presses `5`: its next `packets` packets from tick `at` on carry the key (by
    tick 22 the host's mute of the all-stages story has left it)"""
    keys = key_codes(5, packets)
    for t in range(at, len(script)):
        for i, (s, pt, _) in enumerate(script[t][KEY_LEG]):
            if keys:
                script[t][KEY_LEG][i] = (s, pt, keys.pop(0))
    assert not keys
    return script


def tone_script(lost_at):
    """a steady, quiet script in which leg 6 sends a tone of period 50 -- one period of loud A-law codes, tiled through its packets --
    and loses the packet of tick lost_at"""
    script = clean_script(8, steady=True, quiet=True)
    loud = np.array([c for c in range(256) if 2000 <= abs(int(alaw_decode([c])[0])) <= 8000], np.uint8)
    one = np.random.default_rng(12).choice(loud, size=50)
    for t in range(T):
        s, _, _ = script[t][6][0]
        script[t][6] = [(s, 8, one[(t * 160 + np.arange(160)) % 50])]
    script[lost_at][6] = []
    return script, alaw_decode(one)


def noise_script(n_legs, ticks, sigma=400.0, seed=11):
    """leg 0 sends stationary noise as mu-law packets, one a tick; the others send nothing"""
    rng = np.random.default_rng(seed)
    x = np.clip(np.round(rng.normal(0, sigma, ticks * 160)), -32768, 32767).astype(np.int16)
    script = [[[(t, 0, ulaw_encode(x[160 * t:160 * t + 160]))]] + [[] for _ in range(n_legs - 1)] for t in range(ticks)]
    return rows_of(script, legs=n_legs, ticks=ticks)


def voiced(amp, ticks, seed=5):
    """220 + 660 + 1 500 Hz, each at `amp`, 3 000 of every 4 000 samples on, under noise of 2 % of amp"""
    n = ticks * 160
    t = np.arange(n)
    x = sum(np.sin(2 * np.pi * f * t / 8000) for f in (220, 660, 1500)) * (t % 4000 < 3000) + 0.02 * np.random.default_rng(seed).normal(0, 1, n)
    return np.clip(np.round(amp * x), -32768, 32767).astype(np.int16)


def one_talker(talker, amp, ticks):
    """a conference of three: `talker` sends the voiced bursts as mu-law packets, one a tick; the others send nothing"""
    x = voiced(amp, ticks)
    script = [[[(t, 0, ulaw_encode(x[160 * t:160 * t + 160]))] if g == talker else [] for g in range(3)] for t in range(ticks)]
    return rows_of(script, legs=3, ticks=ticks)
