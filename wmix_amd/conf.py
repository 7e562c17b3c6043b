"""Host-side mirror of wmx_conf (wmix_amd/csrc/conf.hip): a conference bridge of RTP/G.711 legs in one handle, datagram in, datagram out.
The slots' pinned host rows are numpy views; everything else happens in the library."""
import ctypes as C

import numpy as np
import torch

from ._lib import check, host_rows, lib
from .rtp import CODEC, LAW

OUT_ROW = 172


class ConfBridge:
    def __init__(self, n_legs, slots=3, max_packets=3, law="a"):
        self._h = C.c_void_p()
        rc = lib().wmx_conf_create(C.byref(self._h), n_legs, slots, max_packets, LAW[law])
        if rc != 0:
            self._h = None
            check(rc, "wmx_conf_create")
        self.n_legs, self.slots, self.max_packets = n_legs, slots, max_packets
        self.in_row = lib().wmx_conf_in_row_bytes(self._h)
        L = lib()
        # datagram rows [n_legs, max_packets, 176], what recvfrom returned [n_legs, max_packets], datagrams out [n_legs, 172]
        self.rows_in = [host_rows(L.wmx_conf_in(self._h, k), (n_legs, max_packets, self.in_row), np.uint8) for k in range(slots)]
        self.recv = [host_rows(L.wmx_conf_recv(self._h, k), (n_legs, max_packets), np.int32) for k in range(slots)]
        self.rows_out = [host_rows(L.wmx_conf_out(self._h, k), (n_legs, OUT_ROW), np.uint8) for k in range(slots)]
        self.max_taps, self.rec_row_bytes, self.rec_rows, self.rec_legs = 0, 0, None, None  # until recorders()

    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    def set_conferences(self, conferences):
        """a list of conferences, each the ordered list of its legs (MixBatch.set_conferences); an empty list clears the layout"""
        off = np.zeros(len(conferences) + 1, np.int32)
        off[1:] = np.cumsum([len(c) for c in conferences])
        members = np.ascontiguousarray([r for c in conferences for r in c], dtype=np.int32)
        check(lib().wmx_conf_set_conferences(self._h, len(conferences), off.ctypes.data, members.ctypes.data if members.size else None,
                                             self._stream()), "wmx_conf_set_conferences")

    def mute(self, mask=None):
        """the host's mute by leg (non-zero = loaded nowhere), None = nobody"""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        assert m is None or m.size == self.n_legs
        check(lib().wmx_conf_mute(self._h, None if m is None else m.ctypes.data, self._stream()), "wmx_conf_mute")

    def speakers(self, max_speakers, floor=0, decay_shift=3):
        """talker selection in front of the load (0 = off)"""
        check(lib().wmx_conf_speakers(self._h, max_speakers, floor, decay_shift), "wmx_conf_speakers")

    def sequence(self, on, max_gap=3):
        """reorder, de-duplicate and gap-fill the legs by RTP sequence number (wmx_conf_sequence); off = the reference's arrival order"""
        check(lib().wmx_conf_sequence(self._h, 1 if on else 0, max_gap), "wmx_conf_sequence")

    def export_sequence(self):
        """dict(next: uint16, synced: uint8, lost, late, dup, resync, overflow: uint32; [n_legs] each) as the work queued on the current
        stream leaves them"""
        r = {k: np.zeros(self.n_legs, np.uint32) for k in ("lost", "late", "dup", "resync", "overflow")}
        r["next"], r["synced"] = np.zeros(self.n_legs, np.uint16), np.zeros(self.n_legs, np.uint8)
        check(lib().wmx_conf_export_sequence(self._h, r["next"].ctypes.data, r["synced"].ctypes.data, r["lost"].ctypes.data, r["late"].ctypes.data,
                                             r["dup"].ctypes.data, r["resync"].ctypes.data, r["overflow"].ctypes.data, self._stream()),
              "wmx_conf_export_sequence")
        return r

    def conceal(self, on):
        """with sequencing on: a gap's silence calls are synthesised from the leg's own history and the packet behind the gap is
        cross-faded in (wmx_conf_conceal), between submits; off (the default) = zeros"""
        check(lib().wmx_conf_conceal(self._h, 1 if on else 0), "wmx_conf_conceal")

    def export_conceal(self):
        """concealed: uint32 [n_legs], the packets synthesised per leg, as the work queued on the current stream leaves them"""
        concealed = np.zeros(self.n_legs, np.uint32)
        check(lib().wmx_conf_export_conceal(self._h, concealed.ctypes.data, self._stream()), "wmx_conf_export_conceal")
        return concealed

    def dtmf(self, on, suppress=False, event_pt=101):
        """listen to every leg's keypad, in band and in RFC 4733 packets of payload type event_pt (wmx_conf_dtmf), between submits;
        suppress: a key pressed in band is not mixed and wins no talker slot; off (the default) = the launches of before"""
        check(lib().wmx_conf_dtmf(self._h, 1 if on else 0, 1 if suppress else 0, event_pt), "wmx_conf_dtmf")

    def export_dtmf(self):
        """dict(count: uint32 [n_legs], the digits reported per leg; ring: uint8 [n_legs, 8], report n at ring[n & 7] -- the RFC 4733
        event number 0 .. 15, bit 7 set when it came from a packet) as the work queued on the current stream leaves them"""
        r = {"count": np.zeros(self.n_legs, np.uint32), "ring": np.zeros((self.n_legs, 8), np.uint8)}
        check(lib().wmx_conf_export_dtmf(self._h, r["count"].ctypes.data, r["ring"].ctypes.data, self._stream()), "wmx_conf_export_dtmf")
        return r

    def denoise(self, on):
        """every leg's rows go through the leg's own fixed-point noise suppressor behind the DTMF detection and in front of talker
        selection (wmx_conf_denoise), between submits; off (the default) = the launches of before, and the suppressor's state stays"""
        check(lib().wmx_conf_denoise(self._h, 1 if on else 0), "wmx_conf_denoise")

    def _stage_state(self, getter, prefix, leg):
        """the stream blob of one leg in the batch `getter` gives (<prefix>_export_stream), None while the handle has none"""
        L = lib()
        batch = getattr(L, getter)(self._h)
        if not batch:
            return None
        blob = np.zeros(getattr(L, prefix + "_stream_state_bytes")(batch), np.uint8)
        check(getattr(L, prefix + "_export_stream")(batch, int(leg), blob.ctypes.data), prefix + "_export_stream")
        return blob

    def denoiser_state(self, leg):
        """the stream blob of one leg's suppressor (wmx_nsx_export_stream on wmx_conf_denoiser), None before the first denoise(True)"""
        return self._stage_state("wmx_conf_denoiser", "wmx_nsx", leg)

    def level(self, on, value=20):
        """every leg's rows go through the leg's own AGC with compression gain `value` dB, directly behind the denoiser and in front of
        talker selection (wmx_conf_level), between submits; on a handle that has levelled before, another value is agc_addition for
        every leg; off (the default) = the launches of before, and the AGC's state and gains stay"""
        check(lib().wmx_conf_level(self._h, 1 if on else 0, int(value)), "wmx_conf_level")

    def leveller_state(self, leg):
        """the stream blob of one leg's AGC (wmx_agc_export_stream on wmx_conf_leveller), None before the first level(True)"""
        return self._stage_state("wmx_conf_leveller", "wmx_agc", leg)

    def set_leg_gain(self, legs, value):
        """one leg's volume: agc_addition(value) for the listed legs' AGC (wmx_agc_set_gain_streams on wmx_conf_leveller), between
        submits, ordered on the current stream; the state stays.  Needs a handle that has levelled before."""
        L = lib()
        agc = L.wmx_conf_leveller(self._h)
        if not agc:
            raise ValueError("set_leg_gain: no leveller yet (level(True, value) makes it)")
        idx = np.ascontiguousarray(legs, dtype=np.int32)
        check(L.wmx_agc_set_gain_streams(agc, idx.ctypes.data, idx.size, int(value), self._stream()), "wmx_agc_set_gain_streams")

    def gate(self, on):
        """every leg's rows go through the leg's own voice-activity gate (WebRtcVad mode 3; the row is shifted right by the leg's
        `reduce`, 0 .. 4) directly behind the leveller and in front of talker selection (wmx_conf_gate), between submits; a fresh gate
        is shut (`reduce` 4): a new call is heard in full from its fifth row.  off (the default) = the launches of before, and the
        gate's state and counters stay"""
        check(lib().wmx_conf_gate(self._h, 1 if on else 0), "wmx_conf_gate")

    def gater_state(self, leg):
        """the stream blob of one leg's VAD (wmx_vad_export_stream on wmx_conf_gater), None before the first gate(True)"""
        return self._stage_state("wmx_conf_gater", "wmx_vad", leg)

    def export_gate(self):
        """dict(reduce: uint8 [n_legs], 0 .. 4; voiced, unvoiced: uint32 [n_legs], the rows judged voice and not) as the work queued on
        the current stream leaves them; before the first gate(True): reduce 4, counts 0"""
        r = {"reduce": np.zeros(self.n_legs, np.uint8), "voiced": np.zeros(self.n_legs, np.uint32), "unvoiced": np.zeros(self.n_legs, np.uint32)}
        check(lib().wmx_conf_export_gate(self._h, r["reduce"].ctypes.data, r["voiced"].ctypes.data, r["unvoiced"].ctypes.data, self._stream()),
              "wmx_conf_export_gate")
        return r

    def echo(self, on, delay_ms=20):
        """every leg's rows go through the leg's own fixed-point echo canceller between the denoiser and the leveller, with what the
        handle sent to that leg as the far end and delay_ms (0 .. 500) as every leg's reported delay (wmx_conf_echo), between submits;
        off (the default) = the launches of before, and the cancellers' state stays"""
        check(lib().wmx_conf_echo(self._h, 1 if on else 0, int(delay_ms)), "wmx_conf_echo")

    def canceller_state(self, leg):
        """the blob of one leg's canceller -- near state, far end, control plane, delay (wmx_aecm_export_stream on wmx_conf_canceller);
        None before the first echo(True)"""
        return self._stage_state("wmx_conf_canceller", "wmx_aecm", leg)

    def set_leg_echo_delay(self, legs, delay_ms):
        """the reported delay of the listed legs' cancellers (wmx_aecm_set_delay_legs on wmx_conf_canceller), between submits, ordered on
        the current stream.  Needs a handle that has cancelled before."""
        L = lib()
        aecm = L.wmx_conf_canceller(self._h)
        if not aecm:
            raise ValueError("set_leg_echo_delay: no canceller yet (echo(True, delay_ms) makes it)")
        idx = np.ascontiguousarray(legs, dtype=np.int32)
        check(L.wmx_aecm_set_delay_legs(aecm, idx.ctypes.data, idx.size, int(delay_ms), self._stream()), "wmx_aecm_set_delay_legs")

    def export_echo(self):
        """dict(startup, far_ms, known_delay, delay_blocks: int32 [n_legs]) as the work queued on the current stream leaves them; before
        the first echo(True): 1, 0, 0, -2"""
        r = {name: np.zeros(self.n_legs, np.int32) for name in ("startup", "far_ms", "known_delay", "delay_blocks")}
        check(lib().wmx_conf_export_echo(self._h, r["startup"].ctypes.data, r["far_ms"].ctypes.data, r["known_delay"].ctypes.data,
                                         r["delay_blocks"].ctypes.data, self._stream()), "wmx_conf_export_echo")
        return r

    def set_codecs(self, legs, in_codec, out_law):
        """a G.711 codec per leg, as each call negotiated it (wmx_conf_set_codecs), between submits: in_codec "reference" (the default:
        A-law whatever arrives), "pcma", "pcmu" or "by_pt" (or WMX_CODEC_* 0 .. 3), out_law "a" / "u"; legs None = every leg"""
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_conf_set_codecs(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size, CODEC[in_codec],
                                        LAW[out_law], self._stream()), "wmx_conf_set_codecs")

    def export_codecs(self):
        """dict(in_codec, out_law: uint8 [n_legs]; refused: uint32 [n_legs]) as the work queued on the current stream leaves them"""
        r = {"in_codec": np.zeros(self.n_legs, np.uint8), "out_law": np.zeros(self.n_legs, np.uint8), "refused": np.zeros(self.n_legs, np.uint32)}
        check(lib().wmx_conf_export_codecs(self._h, r["in_codec"].ctypes.data, r["out_law"].ctypes.data, r["refused"].ctypes.data, self._stream()),
              "wmx_conf_export_codecs")
        return r

    def prompts(self, max_clips, max_samples):
        """make the prompt store, once (wmx_conf_prompts): max_clips clips of max_samples samples of 1 x 8000 int16 in all, between
        submits, blocking; from then on a tick in which a leg can be playing has one more launch, the legs' prompts, behind the load of
        the legs"""
        check(lib().wmx_conf_prompts(self._h, int(max_clips), int(max_samples)), "wmx_conf_prompts")

    def add_clip(self, pcm, freq=8000, channels=1):
        """append a clip -> its index (wmx_conf_add_clip; blocking).  pcm: int16, interleaved when channels == 2; anything but
        1 x 8000 goes through the reference's own converter first (pcm_zoom of wmix_amd/mix.py)"""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
        if (channels, freq) != (1, 8000) and pcm.size:
            from .mix import pcm_zoom
            pcm = np.ascontiguousarray(pcm_zoom(channels, freq, torch.from_numpy(pcm).cuda().reshape(1, -1), 1, 8000)[0].cpu().numpy())
        clip = C.c_int(-1)
        check(lib().wmx_conf_add_clip(self._h, pcm.ctypes.data if pcm.size else None, pcm.size, C.byref(clip)), "wmx_conf_add_clip")
        return clip.value

    def play(self, legs, clip, repeat=1, gap_ticks=0, reduce=0):
        """the listed legs (None = every leg) start `clip` from its first sample (wmx_conf_play), between submits, ordered on the current
        stream: repeat passes (0 = until stopped), gap_ticks ticks of 20 ms between two; a play over a playing leg replaces it.
        reduce (0 .. 15, the reference's argument; wmx_conf_play_duck): while the prompt makes calls the rest of the conference reaches
        the leg divided by reduce + 1, the prompt undivided on top; the gap between two passes is not ducked"""
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        ptr, n = (None, 0) if idx is None else (idx.ctypes.data, idx.size)
        if reduce:
            check(lib().wmx_conf_play_duck(self._h, ptr, n, int(clip), int(repeat), int(gap_ticks), int(reduce), self._stream()),
                  "wmx_conf_play_duck")
        else:
            check(lib().wmx_conf_play(self._h, ptr, n, int(clip), int(repeat), int(gap_ticks), self._stream()), "wmx_conf_play")

    def stop(self, legs=None):
        """the listed legs (None = every leg) go idle (wmx_conf_stop); what is in their rings plays out"""
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_conf_stop(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size, self._stream()),
              "wmx_conf_stop")

    def export_prompts(self):
        """dict(clip: int32 [n_legs], -1 when idle; pos, left, done: uint32 [n_legs] -- the samples consumed of the current pass, the
        passes left (0 while playing: until stopped), the prompts that ran to their end since the leg's reset) as the work queued on the
        current stream leaves them; without a store: -1, 0, 0, 0"""
        r = {"clip": np.zeros(self.n_legs, np.int32), "pos": np.zeros(self.n_legs, np.uint32), "left": np.zeros(self.n_legs, np.uint32),
             "done": np.zeros(self.n_legs, np.uint32)}
        check(lib().wmx_conf_export_prompts(self._h, r["clip"].ctypes.data, r["pos"].ctypes.data, r["left"].ctypes.data, r["done"].ctypes.data,
                                            self._stream()), "wmx_conf_export_prompts")
        return r

    def export_duck(self):
        """uint8 [n_legs]: the divisor the next tick's load applies to what the others add to each leg's ring, 1 for none
        (wmx_conf_export_duck), as the work queued on the current stream leaves it"""
        r = np.ones(self.n_legs, np.uint8)
        check(lib().wmx_conf_export_duck(self._h, r.ctypes.data, self._stream()), "wmx_conf_export_duck")
        return r

    def recorders(self, max_taps, channels=1, freq=8000):
        """make the recording store, once (wmx_conf_recorders): max_taps taps of one format, channels (1, 2) x freq (up to 48 000),
        between submits, blocking; every slot gets its rows.  From then on a tick in which a tap is running has one more launch in front
        of the egress and downloads the rows with the datagrams"""
        check(lib().wmx_conf_recorders(self._h, int(max_taps), int(channels), int(freq)), "wmx_conf_recorders")
        L = lib()
        self.max_taps, self.rec_row_bytes = int(max_taps), L.wmx_conf_rec_row_bytes(self._h)
        self.rec_rows = [host_rows(L.wmx_conf_rec(self._h, k), (self.max_taps, self.rec_row_bytes // 2), np.int16) for k in range(self.slots)]
        self.rec_legs = [host_rows(L.wmx_conf_rec_legs(self._h, k), (self.max_taps,), np.int32) for k in range(self.slots)]

    def record(self, legs, seconds=0, ticks=None):
        """the listed legs start recording with the next tick (wmx_conf_record) -> the taps they took, int32.  What is recorded is what the
        leg HEARS: its conference without itself, its prompt on top -- a recorder of a whole conference is one more leg of it, muted and
        never fed.  seconds: 50 x seconds rows, 0 = until stopped (the reference's `time` == 0 is one package: ticks=1); ticks, where
        given, is the count of rows itself.  A leg that has a tap is restarted in place; too few free taps raises and starts nothing"""
        idx = np.ascontiguousarray(legs, dtype=np.int32)
        taps = np.full(idx.size, -1, np.int32)
        n = int(ticks) if ticks is not None else 50 * int(seconds)
        check(lib().wmx_conf_record(self._h, idx.ctypes.data, idx.size, n, taps.ctypes.data, self._stream()), "wmx_conf_record")
        return taps

    def record_stop(self, legs=None):
        """the listed legs' taps (None = every tap) are free from the next tick on (wmx_conf_record_stop)"""
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_conf_record_stop(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size, self._stream()),
              "wmx_conf_record_stop")

    def recorded(self, slot):
        """-> (legs int32 [max_taps], rows int16 [max_taps, row_samples]) of a slot, views of its pinned rows, valid after wait(slot):
        row i is valid exactly when legs[i] >= 0, and is that leg's"""
        return self.rec_legs[slot], self.rec_rows[slot]

    def export_record(self):
        """dict(leg: int32 [max_taps], -1 when free; left, written: uint32 [max_taps] -- the rows still to record (0 while running: until
        stopped) and the rows written since the tap was started) as the work queued on the current stream leaves them"""
        r = {"leg": np.zeros(self.max_taps, np.int32), "left": np.zeros(self.max_taps, np.uint32), "written": np.zeros(self.max_taps, np.uint32)}
        check(lib().wmx_conf_export_record(self._h, r["leg"].ctypes.data, r["left"].ctypes.data, r["written"].ctypes.data, self._stream()),
              "wmx_conf_export_record")
        return r

    def step_resident_rec(self, d_in, d_recv, d_out=None):
        """step_resident with the taps: -> (datagrams uint8 [n_legs, 172], legs int32 [max_taps], rows int16 [max_taps, row_samples]),
        all on the device"""
        if d_out is None:
            d_out = torch.zeros((self.n_legs, OUT_ROW), dtype=torch.uint8, device=d_in.device)
        assert d_in.is_cuda and d_in.dtype == torch.uint8 and d_in.is_contiguous() and tuple(d_in.shape) == (self.n_legs, self.max_packets, self.in_row)
        assert d_recv.is_cuda and d_recv.dtype == torch.int32 and d_recv.is_contiguous() and tuple(d_recv.shape) == (self.n_legs, self.max_packets)
        assert d_out.is_cuda and d_out.dtype == torch.uint8 and d_out.is_contiguous() and tuple(d_out.shape) == (self.n_legs, OUT_ROW)
        rows = torch.zeros((self.max_taps, self.rec_row_bytes // 2), dtype=torch.int16, device=d_in.device)
        legs = torch.full((self.max_taps,), -1, dtype=torch.int32, device=d_in.device)
        check(lib().wmx_conf_step_resident_rec(self._h, d_in.data_ptr(), d_recv.data_ptr(), d_out.data_ptr(), rows.data_ptr(), rows.stride(0),
                                               legs.data_ptr(), self._stream()), "wmx_conf_step_resident_rec")
        return d_out, legs, rows

    def set_play_correct(self, n_bytes):
        check(lib().wmx_conf_set_play_correct(self._h, n_bytes), "wmx_conf_set_play_correct")

    def reset_legs(self, legs=None):
        """a new call in a used slot: fresh cursor, dropped = 0, env = 0, the ring zeroed, seq = timestamp = 0, the sequence rule unsynced,
        refused = 0, the concealment history and count zero, no key down and no digit reported, the noise suppressor, the AGC and the
        gate as new (the gate shut, its counters zero), no prompt playing and none counted; the leg keeps its codec and its compression
        gain (None = every leg)"""
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_conf_reset_legs(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size, self._stream()),
              "wmx_conf_reset_legs")

    def next_slot(self):
        return lib().wmx_conf_next_slot(self._h)

    def submit(self):
        """queue the next slot (its rows_in / recv hold the tick's arrivals); returns the slot, whose rows_out are valid after wait(slot)"""
        k = C.c_int(-1)
        check(lib().wmx_conf_submit(self._h, C.byref(k), self._stream()), "wmx_conf_submit")
        return k.value

    def wait(self, slot=-1):
        check(lib().wmx_conf_wait(self._h, slot), "wmx_conf_wait")

    def poll(self, slot=-1):
        rc = lib().wmx_conf_poll(self._h, slot)
        if rc < 0:
            check(rc, "wmx_conf_poll")
        return bool(rc)

    def step_resident(self, d_in, d_recv, d_out=None):
        """the launches alone: d_in uint8 CUDA [n_legs, max_packets, 176], d_recv int32 CUDA [n_legs, max_packets] -> uint8 [n_legs, 172]"""
        assert d_in.is_cuda and d_in.dtype == torch.uint8 and d_in.is_contiguous() and tuple(d_in.shape) == (self.n_legs, self.max_packets, self.in_row)
        assert d_recv.is_cuda and d_recv.dtype == torch.int32 and d_recv.is_contiguous() and tuple(d_recv.shape) == (self.n_legs, self.max_packets)
        if d_out is None:
            d_out = torch.zeros((self.n_legs, OUT_ROW), dtype=torch.uint8, device=d_in.device)
        assert d_out.is_cuda and d_out.dtype == torch.uint8 and d_out.is_contiguous() and tuple(d_out.shape) == (self.n_legs, OUT_ROW)
        check(lib().wmx_conf_step_resident(self._h, d_in.data_ptr(), d_recv.data_ptr(), d_out.data_ptr(), self._stream()), "wmx_conf_step_resident")
        return d_out

    def export_legs(self):
        """dict(head, tick, dropped, env: uint32 [n_legs]; speaking: uint8 [n_legs]) as the work queued on the current stream leaves them"""
        r = {k: np.zeros(self.n_legs, np.uint32) for k in ("head", "tick", "dropped", "env")}
        r["speaking"] = np.zeros(self.n_legs, np.uint8)
        check(lib().wmx_conf_export_legs(self._h, r["head"].ctypes.data, r["tick"].ctypes.data, r["dropped"].ctypes.data, r["env"].ctypes.data,
                                         r["speaking"].ctypes.data, self._stream()), "wmx_conf_export_legs")
        return r

    def export_ring(self, leg):
        """(ring int16, head_off, tick) of one leg's ring (wmx_mix_export)"""
        ring = np.zeros(8000, np.int16)
        h, t = C.c_uint32(0), C.c_uint32(0)
        check(lib().wmx_mix_export(lib().wmx_conf_mix(self._h), leg, ring.ctypes.data, C.byref(h), C.byref(t)), "wmx_mix_export")
        return ring, h.value, t.value

    def sender_state(self, leg):
        s, t = C.c_uint16(0), C.c_uint32(0)
        check(lib().wmx_rtp_export(lib().wmx_conf_senders(self._h), leg, C.byref(s), C.byref(t)), "wmx_rtp_export")
        return s.value, t.value

    def close(self):
        """destroys the handle and its pinned rows: rows_in, recv and rows_out become None, and views taken from them earlier are invalid
        from here on"""
        if self._h:
            self.rows_in = self.recv = self.rows_out = self.rec_rows = self.rec_legs = None  # views of memory that goes away
            lib().wmx_conf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
