"""Host-side mirror of wmix's VAD wrapper (src/webrtc.h:32-36) for batches of streams.
All arithmetic happens in wmix_amd/csrc/vad.hip."""
import ctypes as C

import numpy as np
import torch

from ._legs import process_legs
from .lifetime import Lifetime
from ._lib import check, lib


class VadBatch(Lifetime):
    _mod = "vad"

    def __init__(self, n_streams, chn, freq, interval_ms=10):
        self._h = C.c_void_p()
        rc = lib().wmx_vad_create(C.byref(self._h), n_streams, chn, freq, interval_ms)
        if rc != 0:
            self._h = None
            check(rc, "wmx_vad_create")
        self.n_streams, self.chn, self.freq = n_streams, chn, freq
        self.pkt = lib().wmx_vad_packet_samples(self._h)

    def process(self, pcm, packets_per_call=1):
        """pcm int16 CUDA [n_streams, n_calls, packets_per_call*pkt], modified in place."""
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 3 and pcm.stride(2) == 1
        assert pcm.shape[0] == self.n_streams and pcm.shape[2] == packets_per_call * self.pkt
        check(lib().wmx_vad_process(self._h, pcm.data_ptr(), packets_per_call, pcm.shape[1], pcm.stride(0), pcm.stride(1),
                                    torch.cuda.current_stream().cuda_stream), "wmx_vad_process")
        return pcm

    def process_packet_major(self, pcm, packets_per_call=1):
        """pcm int16 CUDA [n_calls, n_streams, packets_per_call*pkt], modified in place."""
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 3 and pcm.stride(2) == 1
        assert pcm.shape[1] == self.n_streams and pcm.shape[2] == packets_per_call * self.pkt
        check(lib().wmx_vad_process(self._h, pcm.data_ptr(), packets_per_call, pcm.shape[0], pcm.stride(1), pcm.stride(0),
                                    torch.cuda.current_stream().cuda_stream), "wmx_vad_process")
        return pcm

    def process_legs(self, pcm, lens, calls=None, voice=None):
        """the legs of a conference bridge (wmx_vad_process_legs; a 1 x 8000 batch of 20 ms packets): pcm int16 CUDA [n_streams,
        max_packets, >= 160], gated in place; lens uint32 (or int32 bits) CUDA [n_streams, max_packets], 320 where the slot holds a row;
        calls None (the readable slots in slot order) or the call lists [n_streams] the sequencer leaves; voice None or 4-byte words CUDA
        [2, n_streams], incremented per row taken that is judged voice / not voice.  A leg with no row this tick touches nothing."""
        assert voice is None or (voice.is_cuda and voice.element_size() == 4 and voice.is_contiguous() and tuple(voice.shape) == (2, self.n_streams))
        return process_legs(self, "wmx_vad_process_legs", pcm, lens, calls, None if voice is None else voice.data_ptr())

    def export_reduce(self):
        """`reduce` (0 .. 4) of every stream as the work queued on the current stream leaves it: int16 [n_streams]"""
        r = np.zeros(self.n_streams, np.int16)
        check(lib().wmx_vad_export_reduce(self._h, r.ctypes.data, torch.cuda.current_stream().cuda_stream), "wmx_vad_export_reduce")
        return r

    def close(self):
        if self._h:
            lib().wmx_vad_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
