"""Host-side mirror of wmix's resample + mix functions (src/wmix.h:40-49, 113-127) for batches.
All sample arithmetic happens in wmix_amd/csrc/mix.hip; the cursor walks are index-only host loops."""
import ctypes as C

import numpy as np
import torch

from ._lib import check, lib

NULL_HEAD = 0xFFFFFFFF


def len_of_out(in_chn, in_freq, in_len, out_chn, out_freq):
    return lib().wmix_len_of_out(in_chn, in_freq, in_len, out_chn, out_freq)


def len_of_in(in_chn, in_freq, out_chn, out_freq, out_len):
    return lib().wmix_len_of_in(in_chn, in_freq, out_chn, out_freq, out_len)


def pcm_zoom(in_chn, in_freq, pcm, out_chn, out_freq):
    """pcm: int16 CUDA [n_streams, n_in] -> int16 CUDA [n_streams, n_out] (n_out from the reference's own walk)."""
    assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 2 and pcm.stride(1) == 1
    in_len = pcm.shape[1] * 2
    # capacity: frames * rate ratio (+ slack); wmix_len_of_out is unit-agnostic and does not bound the byte count
    n_out = (int(np.ceil(pcm.shape[1] / in_chn * max(out_freq / in_freq, 1.0))) + 4) * out_chn
    out = torch.zeros(pcm.shape[0], n_out, dtype=torch.int16, device=pcm.device)
    got = C.c_uint32(0)
    check(lib().wmx_pcm_zoom(in_chn, in_freq, pcm.data_ptr(), in_len, out_chn, out_freq, out.data_ptr(), n_out * 2, pcm.stride(0),
                             out.stride(0), pcm.shape[0], C.byref(got), torch.cuda.current_stream().cuda_stream), "wmx_pcm_zoom")
    return out[:, : got.value // 2]


class MixBatch:
    def __init__(self, n_groups, ring_chn=1, ring_freq=8000):
        self._h = C.c_void_p()
        rc = lib().wmx_mix_create(C.byref(self._h), n_groups, ring_chn, ring_freq)
        if rc != 0:
            self._h = None
            check(rc, "wmx_mix_create")
        self.n_groups = n_groups
        self.ring_bytes = lib().wmx_mix_ring_bytes(self._h)

    def set_play_correct(self, n_bytes):
        """VIEW_PLAY_CORRECT of the reference's platform build (platform/<name>/plat.h): alsa 200 ms of ring (the default), hi3516 / t31 0"""
        check(lib().wmx_mix_set_play_correct(self._h, n_bytes), "wmx_mix_set_play_correct")

    def set(self, head_off=0, tick=0, reduce_mode=1):
        check(lib().wmx_mix_set(self._h, head_off, tick, reduce_mode), "wmx_mix_set")

    def load(self, src, src_bytes, freq, channels, head=NULL_HEAD, tick=0, reduce=1, sample=16):
        """src int16 CUDA [n_groups, n_src, >= src_bytes/2 + channels]; returns (head, tick) after the call."""
        assert src.is_cuda and src.dtype == torch.int16 and src.dim() == 3 and src.stride(2) == 1 and src.shape[0] == self.n_groups
        h, t = C.c_uint32(head), C.c_uint32(tick)
        check(lib().wmx_mix_load(self._h, src.data_ptr(), src_bytes, freq, channels, sample, src.shape[1], src.stride(0), src.stride(1),
                                 reduce, C.byref(h), C.byref(t), torch.cuda.current_stream().cuda_stream), "wmx_mix_load")
        return h.value, t.value

    def load_minus(self, src, parties, src_bytes, freq, channels, mute=None, head=NULL_HEAD, tick=0, reduce=1, sample=16):
        """The bridge load (wmx_mix_load_minus): the rings are n_groups / parties conferences of `parties` consecutive rings, and ring q
        of a conference receives every source of that conference except its own, in index order.  src int16 CUDA [n_conf, parties,
        >= src_bytes/2 + look-ahead]; mute: None or uint8 CUDA [n_groups], non-zero = that source is loaded nowhere.  Returns (head,
        tick) after the call."""
        assert src.is_cuda and src.dtype == torch.int16 and src.dim() == 3 and src.stride(2) == 1
        assert src.shape[1] == parties and src.shape[0] * parties == self.n_groups
        if mute is not None:
            assert mute.is_cuda and mute.dtype == torch.uint8 and mute.is_contiguous() and mute.numel() == self.n_groups
        h, t = C.c_uint32(head), C.c_uint32(tick)
        check(lib().wmx_mix_load_minus(self._h, parties, src.data_ptr(), src_bytes, freq, channels, sample, src.stride(0), src.stride(1),
                                       mute.data_ptr() if mute is not None else None, reduce, C.byref(h), C.byref(t),
                                       torch.cuda.current_stream().cuda_stream), "wmx_mix_load_minus")
        return h.value, t.value

    def set_conferences(self, conferences):
        """The layout of load_minus_conf (wmx_mix_set_conferences): a list of conferences, each the ordered list of its members' ring
        indices -- not necessarily consecutive or ascending; a ring in at most one; 0 or 1 members = a placeholder that keeps its index;
        at most 32 members.  An empty list clears the layout."""
        off = np.zeros(len(conferences) + 1, np.int32)
        off[1:] = np.cumsum([len(c) for c in conferences])
        members = np.ascontiguousarray([r for c in conferences for r in c], dtype=np.int32)
        check(lib().wmx_mix_set_conferences(self._h, len(conferences), off.ctypes.data, members.ctypes.data if members.size else None,
                                            torch.cuda.current_stream().cuda_stream), "wmx_mix_set_conferences")

    def conferences(self):
        return lib().wmx_mix_conferences(self._h)

    def load_minus_conf(self, src, src_bytes, freq, channels, mute=None, head=None, tick=None, reduce=1, sample=16):
        """The bridge load over the layout (wmx_mix_load_minus_conf): the ring of every member of a conference receives the sources of
        the conference's other members, in list order, from the conference's own cursor.  src int16 CUDA [n_groups, >= src_bytes/2 +
        look-ahead], row r = the source of ring r; mute: None or uint8 CUDA [n_groups] by ring; head / tick: one per conference (None =
        no cursor yet).  Returns (heads, ticks) after the call as uint32 arrays."""
        assert src.is_cuda and src.dtype == torch.int16 and src.dim() == 2 and src.stride(1) == 1 and src.shape[0] == self.n_groups
        if mute is not None:
            assert mute.is_cuda and mute.dtype == torch.uint8 and mute.is_contiguous() and mute.numel() == self.n_groups
        n = max(self.conferences(), 0)
        h = np.full(n, NULL_HEAD, np.uint32) if head is None else np.array(head, dtype=np.uint32)
        t = np.zeros(n, np.uint32) if tick is None else np.array(tick, dtype=np.uint32)
        assert h.size == n and t.size == n
        check(lib().wmx_mix_load_minus_conf(self._h, src.data_ptr(), src_bytes, freq, channels, sample, src.stride(0),
                                            mute.data_ptr() if mute is not None else None, reduce, h.ctypes.data, t.ctypes.data,
                                            torch.cuda.current_stream().cuda_stream), "wmx_mix_load_minus_conf")
        return h, t

    def load_minus_legs(self, src, src_bytes, freq, channels, lens, mute=None, reduce=1, sample=16):
        """The bridge load with a cursor per leg (wmx_mix_load_minus_legs), over the layout in force: legs whose packets come early, late
        or not at all.  src int16 CUDA [n_groups, max_packets, >= src_bytes/2 + look-ahead], packet k of ring r; lens uint32 (or
        int32) CUDA [n_groups, max_packets]: slot k of leg r is a call if and only if lens[r, k] == src_bytes; mute: None or uint8
        CUDA [n_groups] by ring (a muted leg's cursor moves, no ring changes).  The cursors live on the device: export_leg_cursors."""
        assert src.is_cuda and src.dtype == torch.int16 and src.dim() == 3 and src.stride(2) == 1 and src.shape[0] == self.n_groups
        assert lens.is_cuda and lens.dtype in (torch.int32, torch.uint32) and lens.is_contiguous() and tuple(lens.shape) == tuple(src.shape[:2])
        if mute is not None:
            assert mute.is_cuda and mute.dtype == torch.uint8 and mute.is_contiguous() and mute.numel() == self.n_groups
        check(lib().wmx_mix_load_minus_legs(self._h, src.data_ptr(), src_bytes, freq, channels, sample, src.stride(0), src.stride(1),
                                            src.shape[1], lens.data_ptr(), mute.data_ptr() if mute is not None else None, reduce,
                                            torch.cuda.current_stream().cuda_stream), "wmx_mix_load_minus_legs")

    def load_minus_legs_calls(self, src, src_bytes, freq, channels, lens, calls, mute=None, reduce=1, sample=16):
        """load_minus_legs fed a call list per leg (wmx_mix_load_minus_legs_calls; RtpSenders.sequence_legs writes the lists): calls
        int32 (or uint32) CUDA [n_groups]; leg r makes its list's calls in list order, a silence call moves the cursor and adds nothing,
        a data call whose slot's lens != src_bytes is made as silence."""
        assert src.is_cuda and src.dtype == torch.int16 and src.dim() == 3 and src.stride(2) == 1 and src.shape[0] == self.n_groups
        assert lens.is_cuda and lens.dtype in (torch.int32, torch.uint32) and lens.is_contiguous() and tuple(lens.shape) == tuple(src.shape[:2])
        assert calls.is_cuda and calls.dtype in (torch.int32, torch.uint32) and calls.is_contiguous() and calls.numel() == self.n_groups
        if mute is not None:
            assert mute.is_cuda and mute.dtype == torch.uint8 and mute.is_contiguous() and mute.numel() == self.n_groups
        check(lib().wmx_mix_load_minus_legs_calls(self._h, src.data_ptr(), src_bytes, freq, channels, sample, src.stride(0), src.stride(1),
                                                  src.shape[1], lens.data_ptr(), calls.data_ptr(), mute.data_ptr() if mute is not None else None,
                                                  reduce, torch.cuda.current_stream().cuda_stream), "wmx_mix_load_minus_legs_calls")

    def reset_leg_cursors(self, rings=None):
        """a fresh cursor and dropped = 0 for the listed rings (None = every ring): what a new call in a reused slot does"""
        idx = None if rings is None else np.ascontiguousarray(rings, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_mix_reset_leg_cursors(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size,
                                              torch.cuda.current_stream().cuda_stream), "wmx_mix_reset_leg_cursors")

    def export_leg_cursors(self):
        """(head, tick, dropped), uint32 [n_groups] each, as the work queued on the current stream leaves them"""
        h, t, d = (np.zeros(self.n_groups, np.uint32) for _ in range(3))
        check(lib().wmx_mix_export_leg_cursors(self._h, h.ctypes.data, t.ctypes.data, d.ctypes.data, torch.cuda.current_stream().cuda_stream),
              "wmx_mix_export_leg_cursors")
        return h, t, d

    def _mute_pair(self, mute, out):
        if mute is not None:
            assert mute.is_cuda and mute.dtype == torch.uint8 and mute.is_contiguous() and mute.numel() == self.n_groups
        if out is None:
            out = torch.empty(self.n_groups, dtype=torch.uint8, device="cuda")
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == self.n_groups
        return mute.data_ptr() if mute is not None else None, out

    def select_speakers(self, src, parties, src_bytes, max_speakers, floor=0, decay_shift=3, mute=None, out=None):
        """Talker selection in front of load_minus (wmx_mix_select_speakers): of every conference only the loudest max_speakers legs stay
        un-muted.  src as for load_minus; mute: the host's mute, None or uint8 CUDA [n_groups]; out: uint8 CUDA [n_groups] to write (made
        when None).  Returns the mask to pass to load_minus as `mute`."""
        assert src.is_cuda and src.dtype == torch.int16 and src.dim() == 3 and src.stride(2) == 1
        assert src.shape[1] == parties and src.shape[0] * parties == self.n_groups
        mp, out = self._mute_pair(mute, out)
        check(lib().wmx_mix_select_speakers(self._h, parties, src.data_ptr(), src_bytes, src.stride(0), src.stride(1), mp, max_speakers, floor,
                                            decay_shift, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "wmx_mix_select_speakers")
        return out

    def select_speakers_conf(self, src, src_bytes, max_speakers, floor=0, decay_shift=3, mute=None, out=None):
        """The same over the layout (wmx_mix_select_speakers_conf), in front of load_minus_conf: src [n_groups, >= src_bytes / 2], row r =
        the source of ring r.  Rings outside every conference of two or more members come out muted."""
        assert src.is_cuda and src.dtype == torch.int16 and src.dim() == 2 and src.stride(1) == 1 and src.shape[0] == self.n_groups
        mp, out = self._mute_pair(mute, out)
        check(lib().wmx_mix_select_speakers_conf(self._h, src.data_ptr(), src_bytes, src.stride(0), mp, max_speakers, floor, decay_shift,
                                                 out.data_ptr(), torch.cuda.current_stream().cuda_stream), "wmx_mix_select_speakers_conf")
        return out

    def select_speakers_legs(self, src, src_bytes, lens, max_speakers, floor=0, decay_shift=3, mute=None, out=None):
        """The same over leg packets (wmx_mix_select_speakers_legs), in front of load_minus_legs: src [n_groups, max_packets, >= src_bytes /
        2] and lens [n_groups, max_packets] as there; a leg's level is the largest level among its slots that are calls, 0 without one."""
        assert src.is_cuda and src.dtype == torch.int16 and src.dim() == 3 and src.stride(2) == 1 and src.shape[0] == self.n_groups
        assert lens.is_cuda and lens.dtype in (torch.int32, torch.uint32) and lens.is_contiguous() and tuple(lens.shape) == tuple(src.shape[:2])
        mp, out = self._mute_pair(mute, out)
        check(lib().wmx_mix_select_speakers_legs(self._h, src.data_ptr(), src_bytes, src.stride(0), src.stride(1), src.shape[1], lens.data_ptr(),
                                                 mp, max_speakers, floor, decay_shift, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "wmx_mix_select_speakers_legs")
        return out

    def reset_rings(self, rings=None):
        """zero the listed rings (None = every ring): a new call in a reused slot does not hear what the old one loaded ahead"""
        idx = None if rings is None else np.ascontiguousarray(rings, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_mix_reset_rings(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size,
                                        torch.cuda.current_stream().cuda_stream), "wmx_mix_reset_rings")

    def reset_speakers(self, rings=None):
        """env = 0 for the listed rings (None = every ring): what a new call in a reused slot does"""
        idx = None if rings is None else np.ascontiguousarray(rings, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_mix_reset_speakers(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size,
                                           torch.cuda.current_stream().cuda_stream), "wmx_mix_reset_speakers")

    def export_speakers(self):
        """(speaking uint8 [n_groups], env uint32 [n_groups]) as the work queued on the current stream leaves them"""
        env, speaking = np.zeros(self.n_groups, np.uint32), np.zeros(self.n_groups, np.uint8)
        check(lib().wmx_mix_export_speakers(self._h, env.ctypes.data, speaking.ctypes.data, torch.cuda.current_stream().cuda_stream),
              "wmx_mix_export_speakers")
        return speaking, env

    def drain(self, n_bytes):
        out = torch.empty(self.n_groups, n_bytes // 2, dtype=torch.int16, device="cuda")
        check(lib().wmx_mix_drain(self._h, out.data_ptr(), n_bytes, out.stride(0), torch.cuda.current_stream().cuda_stream), "wmx_mix_drain")
        return out

    def export(self, group=0):
        ring = np.zeros(self.ring_bytes // 2, np.int16)
        h, t = C.c_uint32(0), C.c_uint32(0)
        check(lib().wmx_mix_export(self._h, group, ring.ctypes.data, C.byref(h), C.byref(t)), "wmx_mix_export")
        return ring, h.value, t.value

    def close(self):
        if self._h:
            lib().wmx_mix_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
