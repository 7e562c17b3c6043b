"""Host-side mirror of wmix's AEC wrapper built with the reference's AECM switch (src/webrtc.c:168-191) for batches of
near-end streams that share one far-end: the fixed-point echo canceller.  Same call shapes as wmix_amd/aec.py; all
arithmetic is in wmix_amd/csrc/aecm.hip."""
import ctypes as C

import torch

from .lifetime import Lifetime
from ._legs import process_legs
from ._lib import check, lib


class AecmBatch(Lifetime):
    _mod = "aecm"

    def __init__(self, n_streams, chn, freq, interval_ms=10, n_cohorts=1):
        self._h = C.c_void_p()
        self.n_cohorts = int(n_cohorts)
        rc = lib().wmx_aecm_create_cohorts(C.byref(self._h), n_streams, chn, freq, interval_ms, self.n_cohorts)
        if rc != 0:
            self._h = None
            check(rc, "wmx_aecm_create")
        self.n_streams, self.chn, self.freq = n_streams, chn, freq
        self.pkt = lib().wmx_aecm_packet_samples(self._h)
        self.state_bytes = lib().wmx_aecm_state_bytes(self._h)

    # ---- echo control for the legs of a conference bridge (wmx_aecm_create_legs: one canceller per leg, no cohorts)
    @classmethod
    def create_legs(cls, n_legs):
        """n_legs cancellers, each aec_init(1, 8000, 20) with far-end buffers and a control plane of its own on the device"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        rc = lib().wmx_aecm_create_legs(C.byref(self._h), n_legs)
        if rc != 0:
            self._h = None
            check(rc, "wmx_aecm_create_legs")
        self.n_streams, self.chn, self.freq, self.n_cohorts = n_legs, 1, 8000, 0
        self.pkt = lib().wmx_aecm_packet_samples(self._h)
        self.state_bytes = lib().wmx_aecm_state_bytes(self._h)
        return self

    def process_legs(self, pcm, lens, calls=None, far=None, far_leg_stride=None):
        """wmx_aecm_process_legs on the current stream: the rows this tick brought each leg (pcm int16 CUDA [n_legs, max_packets,
        >= 160], lens, calls as the other stages' process_legs; pcm None and lens None: no rows), then the row it was sent (far int16
        CUDA [n_legs, >= 160], or an address with far_leg_stride; None: rows only)"""
        if far is not None and not isinstance(far, int):
            assert far.is_cuda and far.dtype == torch.int16 and far.dim() == 2 and far.shape[0] == self.n_streams and far.shape[1] >= 160
            assert far.stride(1) == 1
            far, far_leg_stride = far.data_ptr(), far.stride(0)
        extras = (far, int(far_leg_stride or 0))
        if pcm is None:
            assert lens is None and calls is None
            check(lib().wmx_aecm_process_legs(self._h, None, 0, 0, 1, None, None, *extras, torch.cuda.current_stream().cuda_stream),
                  "wmx_aecm_process_legs")
            return None
        return process_legs(self, "wmx_aecm_process_legs", pcm, lens, calls, *extras)

    def set_delay_legs(self, delay_ms, legs=None):
        """the reported delay (0 .. 500 ms) of the listed legs, None: of all; kept across reset_streams"""
        import numpy as np
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        check(lib().wmx_aecm_set_delay_legs(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size, int(delay_ms),
                                            torch.cuda.current_stream().cuda_stream), "wmx_aecm_set_delay_legs")

    def export_legs(self):
        """-> (ec_startup, far ring fill in ms, knownDelay, the estimator's last_delay): numpy int32 [n_legs] each"""
        out = torch.zeros((4, self.n_streams), dtype=torch.int32, device="cuda")
        check(lib().wmx_aecm_export_legs(self._h, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "wmx_aecm_export_legs")
        return tuple(out.cpu().numpy())

    def _run(self, mode, far, near, out, n_packets, stream_stride, packet_stride, delay_ms):
        fp = far.data_ptr() if far is not None else None
        fs = far.stride(0) if far is not None else 0
        rc = lib().wmx_aecm_run(self._h, mode, fp, fs, near.data_ptr() if near is not None else None,
                                out.data_ptr() if out is not None else None, n_packets, stream_stride, packet_stride, delay_ms,
                                torch.cuda.current_stream().cuda_stream)
        if rc not in (0, -1):
            check(rc, "wmx_aecm_run")
        return rc

    def run_cohorts(self, far, near, delays, cohort_on=None, out=None, mode=3):
        """As AecBatch.run_cohorts: one reported delay (and optional on/off byte) per cohort; returns (rc, per-cohort codes)."""
        import numpy as np
        assert far.is_cuda and far.dtype == torch.int16 and far.dim() == 2 and far.shape[1] == self.pkt and far.stride(1) == 1
        assert near.is_cuda and near.dtype == torch.int16 and near.dim() == 3 and near.stride(2) == 1 and near.shape[0] == self.n_streams
        out = near if out is None else out
        d = np.ascontiguousarray(delays, dtype=np.int32)
        assert d.shape == (self.n_cohorts,)
        on = None if cohort_on is None else np.ascontiguousarray(cohort_on, dtype=np.uint8)
        codes = np.zeros(self.n_cohorts, np.int32)
        rc = lib().wmx_aecm_run_cohorts(self._h, mode, far.data_ptr(), far.stride(0), 0, near.data_ptr(), out.data_ptr(), near.shape[1],
                                        near.stride(0), near.stride(1), d.ctypes.data, None if on is None else on.ctypes.data,
                                        codes.ctypes.data, torch.cuda.current_stream().cuda_stream)
        if rc not in (0, -1):
            check(rc, "wmx_aecm_run_cohorts")
        return rc, codes

    def process2(self, far, near, out=None, delay_ms=0):
        """aec_process2: far int16 CUDA [n_packets, pkt] (shared), near [n_streams, n_packets, pkt]."""
        assert far.is_cuda and far.dtype == torch.int16 and far.dim() == 2 and far.shape[1] == self.pkt and far.stride(1) == 1
        assert near.is_cuda and near.dtype == torch.int16 and near.dim() == 3 and near.stride(2) == 1
        assert near.shape == (self.n_streams, far.shape[0], self.pkt)
        out = near if out is None else out
        assert out.stride() == near.stride()
        return self._run(3, far, near, out, far.shape[0], near.stride(0), near.stride(1), delay_ms), out

    def process2_packet_major(self, far, near, out=None, delay_ms=0):
        """near int16 CUDA [n_packets, n_streams, pkt] (one step of all streams contiguous)."""
        assert far.is_cuda and far.dtype == torch.int16 and far.dim() == 2 and far.shape[1] == self.pkt and far.stride(1) == 1
        assert near.is_cuda and near.dtype == torch.int16 and near.dim() == 3 and near.stride(2) == 1
        assert near.shape == (far.shape[0], self.n_streams, self.pkt)
        out = near if out is None else out
        assert out.stride() == near.stride()
        return self._run(3, far, near, out, far.shape[0], near.stride(1), near.stride(0), delay_ms), out

    def set_frame_far(self, far):
        assert far.is_cuda and far.dtype == torch.int16 and far.dim() == 2 and far.shape[1] == self.pkt
        return self._run(1, far, None, None, far.shape[0], 0, 0, 0)

    def process(self, near, out=None, delay_ms=0):
        assert near.is_cuda and near.dtype == torch.int16 and near.dim() == 3 and near.shape[0] == self.n_streams
        out = near if out is None else out
        return self._run(2, None, near, out, near.shape[1], near.stride(0), near.stride(1), delay_ms), out

    def close(self):
        if self._h:
            lib().wmx_aecm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
