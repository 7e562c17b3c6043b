"""Host-side mirror of the RTP / G.711 packet edge (src/rtp.h, src/wmixTask.c:1019-1351) over torch device tensors.
All arithmetic happens in wmix_amd/csrc/rtp.hip."""
import ctypes as C

import torch

from ._lib import check, lib

LAW = {"a": 0, "u": 1, 0: 0, 1: 1}
# WMX_CODEC_* (include/wmix_amd.h): what a leg negotiated for the packets it sends us
CODEC = {"reference": 0, "pcma": 1, "pcmu": 2, "by_pt": 3, 0: 0, 1: 1, 2: 2, 3: 3}


class RtpSenders:
    """n streams of wmix_thread_rtp_send_pcma state (sequence number, timestamp)."""

    def __init__(self, n_streams, law="a"):
        self._h = C.c_void_p()
        check(lib().wmx_rtp_create(C.byref(self._h), n_streams, LAW[law]), "wmx_rtp_create")
        self.n = n_streams

    def egress(self, pcm, in_chn, in_freq, out_chn, out_freq, packets=None):
        """pcm int16 CUDA [n_streams, samples] -> uint8 CUDA [n_streams, packet_bytes] datagrams (header + codes)."""
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 2 and pcm.shape[0] == self.n and pcm.stride(1) == 1
        if packets is None:
            packets = torch.zeros((self.n, 12 + pcm.shape[1] * max(1, (out_chn * out_freq + in_chn * in_freq - 1) // (in_chn * in_freq))),
                                  dtype=torch.uint8, device=pcm.device)
        size = C.c_uint32(0)
        check(lib().wmx_rtp_egress(self._h, in_chn, in_freq, pcm.data_ptr(), pcm.shape[1] * 2, pcm.stride(0), out_chn, out_freq,
                                   packets.data_ptr(), packets.stride(0), C.byref(size), torch.cuda.current_stream().cuda_stream),
              "wmx_rtp_egress")
        return packets[:, : size.value]

    def egress_rings(self, mix, packets=None):
        """Play and send in one kernel (wmx_rtp_egress_rings): the 20 ms at the head of every 1 x 8000 ring of `mix` (a MixBatch with as
        many rings as there are senders) -> uint8 CUDA [n_streams, 172]; the rings are zeroed there and head and tick advance as in
        MixBatch.drain(320)."""
        if packets is None:
            packets = torch.zeros((self.n, 172), dtype=torch.uint8, device="cuda")
        assert packets.is_cuda and packets.dtype == torch.uint8 and packets.dim() == 2 and packets.shape[0] == self.n and packets.stride(1) == 1
        size = C.c_uint32(0)
        check(lib().wmx_rtp_egress_rings(self._h, mix._h, packets.data_ptr(), packets.stride(0), C.byref(size),
                                         torch.cuda.current_stream().cuda_stream), "wmx_rtp_egress_rings")
        return packets[:, : size.value]

    def reset_streams(self, streams=None):
        """seq = timestamp = 0 for the listed senders (None = all): a new call"""
        import numpy as np
        idx = None if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_rtp_reset_streams(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size,
                                          torch.cuda.current_stream().cuda_stream), "wmx_rtp_reset_streams")

    def sequence_legs(self, seq_raw, lens, max_gap=3, calls=None):
        """Reorder, de-duplicate and gap-fill by RTP sequence number (wmx_rtp_sequence_legs), between ingest_legs and the load: seq_raw
        int16 (or uint16) CUDA [n_streams, max_packets] and lens int32 (or uint32) CUDA [n_streams, max_packets] as ingest_legs leaves
        them.  lens is REWRITTEN (0 for a slot that makes no call); -> calls int32 CUDA [n_streams], the call lists for
        MixBatch.load_minus_legs_calls."""
        assert seq_raw.is_cuda and seq_raw.dtype in (torch.int16, torch.uint16) and seq_raw.is_contiguous() and seq_raw.dim() == 2
        assert seq_raw.shape[0] == self.n
        assert lens.is_cuda and lens.dtype in (torch.int32, torch.uint32) and lens.is_contiguous() and tuple(lens.shape) == tuple(seq_raw.shape)
        if calls is None:
            calls = torch.zeros(self.n, dtype=torch.int32, device=lens.device)
        assert calls.is_cuda and calls.dtype in (torch.int32, torch.uint32) and calls.is_contiguous() and calls.numel() == self.n
        check(lib().wmx_rtp_sequence_legs(self._h, seq_raw.shape[1], max_gap, seq_raw.data_ptr(), lens.data_ptr(), calls.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "wmx_rtp_sequence_legs")
        return calls

    def reset_sequence(self, legs=None):
        """unsynced and counters 0 for the listed legs (None = all): a new call may start at any sequence number"""
        import numpy as np
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_rtp_reset_sequence(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size,
                                           torch.cuda.current_stream().cuda_stream), "wmx_rtp_reset_sequence")

    def export_sequence(self):
        """dict(next: uint16, synced: uint8, lost, late, dup, resync, overflow: uint32; [n_streams] each) as the work queued on the
        current stream leaves them"""
        import numpy as np
        r = {k: np.zeros(self.n, np.uint32) for k in ("lost", "late", "dup", "resync", "overflow")}
        r["next"], r["synced"] = np.zeros(self.n, np.uint16), np.zeros(self.n, np.uint8)
        check(lib().wmx_rtp_export_sequence(self._h, r["next"].ctypes.data, r["synced"].ctypes.data, r["lost"].ctypes.data, r["late"].ctypes.data,
                                            r["dup"].ctypes.data, r["resync"].ctypes.data, r["overflow"].ctypes.data,
                                            torch.cuda.current_stream().cuda_stream), "wmx_rtp_export_sequence")
        return r

    def conceal_legs(self, pcm, lens, calls, rows_out=None, lens_out=None):
        """Conceal lost packets from each leg's own history (wmx_rtp_conceal_legs), between sequence_legs and the load: pcm int16 CUDA
        [n_streams, max_packets, >= 160], lens int32 (or uint32) CUDA [n_streams, max_packets] and calls int32 (or uint32) CUDA
        [n_streams] as sequence_legs leaves them; none of them is written.  -> (rows int16 CUDA [n_streams, 4, 160] in call order,
        lens_out int32 CUDA [n_streams, 4]: 320 per call), what MixBatch.load_minus_legs takes with four slots.  Rows behind a leg's
        calls are not written."""
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 3 and pcm.stride(2) == 1 and pcm.shape[0] == self.n and pcm.shape[2] >= 160
        k = pcm.shape[1]
        assert lens.is_cuda and lens.dtype in (torch.int32, torch.uint32) and lens.is_contiguous() and tuple(lens.shape) == (self.n, k)
        assert calls.is_cuda and calls.dtype in (torch.int32, torch.uint32) and calls.is_contiguous() and calls.numel() == self.n
        if rows_out is None:
            rows_out = torch.zeros((self.n, 4, 160), dtype=torch.int16, device=pcm.device)
        if lens_out is None:
            lens_out = torch.zeros((self.n, 4), dtype=torch.int32, device=pcm.device)
        assert rows_out.is_cuda and rows_out.dtype == torch.int16 and rows_out.is_contiguous() and tuple(rows_out.shape) == (self.n, 4, 160)
        assert lens_out.is_cuda and lens_out.dtype in (torch.int32, torch.uint32) and lens_out.is_contiguous() and tuple(lens_out.shape) == (self.n, 4)
        check(lib().wmx_rtp_conceal_legs(self._h, k, pcm.data_ptr(), pcm.stride(0), pcm.stride(1), lens.data_ptr(), calls.data_ptr(),
                                         rows_out.data_ptr(), lens_out.data_ptr(), torch.cuda.current_stream().cuda_stream), "wmx_rtp_conceal_legs")
        return rows_out, lens_out

    def reset_conceal(self, legs=None):
        """a fresh history and concealed = 0 for the listed legs (None = all)"""
        import numpy as np
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_rtp_reset_conceal(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size,
                                          torch.cuda.current_stream().cuda_stream), "wmx_rtp_reset_conceal")

    def export_conceal(self):
        """dict(hist: int16 [n_streams, 320], newest last; concealed: uint32 [n_streams]) as the work queued on the current stream
        leaves them"""
        import numpy as np
        r = {"hist": np.zeros((self.n, 320), np.int16), "concealed": np.zeros(self.n, np.uint32)}
        check(lib().wmx_rtp_export_conceal(self._h, r["hist"].ctypes.data, r["concealed"].ctypes.data, torch.cuda.current_stream().cuda_stream),
              "wmx_rtp_export_conceal")
        return r

    def detect_dtmf_legs(self, packets, recv_bytes, pcm, lens, calls=None, event_pt=101, suppress=False):
        """DTMF per leg, heard in band and read from RFC 4733 packets (wmx_rtp_detect_dtmf_legs), between ingest_legs (and
        sequence_legs) and the selection / the load: packets uint8 CUDA [n_streams, max_packets, >= 172] and recv_bytes int32 CUDA
        [n_streams, max_packets] as ingest_legs was given them, pcm int16 CUDA [n_streams, max_packets, >= 160] and lens as it (or
        sequence_legs) left them, calls the call lists of sequence_legs or None for slot order.  With suppress the rows of pcm that
        are a tone are ZEROED in place; nothing else is written.  The digits are read with export_dtmf()."""
        assert packets.is_cuda and packets.dtype == torch.uint8 and packets.dim() == 3 and packets.stride(2) == 1 and packets.shape[0] == self.n
        k = packets.shape[1]
        assert recv_bytes.is_cuda and recv_bytes.dtype == torch.int32 and recv_bytes.is_contiguous() and tuple(recv_bytes.shape) == (self.n, k)
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 3 and pcm.stride(2) == 1 and tuple(pcm.shape[:2]) == (self.n, k)
        assert pcm.shape[2] >= 160 and packets.shape[2] >= 172
        assert lens.is_cuda and lens.dtype in (torch.int32, torch.uint32) and lens.is_contiguous() and tuple(lens.shape) == (self.n, k)
        assert calls is None or (calls.is_cuda and calls.dtype in (torch.int32, torch.uint32) and calls.is_contiguous() and calls.numel() == self.n)
        check(lib().wmx_rtp_detect_dtmf_legs(self._h, k, packets.data_ptr(), packets.stride(0), packets.stride(1), recv_bytes.data_ptr(),
                                             pcm.data_ptr(), pcm.stride(0), pcm.stride(1), lens.data_ptr(),
                                             None if calls is None else calls.data_ptr(), event_pt, 1 if suppress else 0,
                                             torch.cuda.current_stream().cuda_stream), "wmx_rtp_detect_dtmf_legs")

    def reset_dtmf(self, legs=None):
        """nothing reported, no key down and no event timestamp for the listed legs (None = all)"""
        import numpy as np
        idx = None if legs is None else np.ascontiguousarray(legs, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_rtp_reset_dtmf(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size,
                                       torch.cuda.current_stream().cuda_stream), "wmx_rtp_reset_dtmf")

    def export_dtmf(self):
        """dict(count: uint32 [n_streams], the digits reported per leg; ring: uint8 [n_streams, 8], report n at ring[n & 7], bit 7 set
        when it came from a packet) as the work queued on the current stream leaves them"""
        import numpy as np
        r = {"count": np.zeros(self.n, np.uint32), "ring": np.zeros((self.n, 8), np.uint8)}
        check(lib().wmx_rtp_export_dtmf(self._h, r["count"].ctypes.data, r["ring"].ctypes.data, torch.cuda.current_stream().cuda_stream),
              "wmx_rtp_export_dtmf")
        return r

    def recorders(self, max_taps, channels=1, freq=8000):
        """the recording store, once (wmx_rtp_recorders): max_taps taps of one format -> the int16 samples of a row"""
        check(lib().wmx_rtp_recorders(self._h, int(max_taps), int(channels), int(freq)), "wmx_rtp_recorders")
        self.max_taps = int(max_taps)
        return lib().wmx_rtp_record_row_bytes(self._h) // 2

    def record(self, streams, ticks=0):
        """the listed streams start recording, `ticks` rows each, 0 = until stopped (wmx_rtp_record) -> the taps they took, int32"""
        import numpy as np
        idx = np.ascontiguousarray(streams, dtype=np.int32)
        taps = np.full(idx.size, -1, np.int32)
        check(lib().wmx_rtp_record(self._h, idx.ctypes.data, idx.size, int(ticks), taps.ctypes.data, torch.cuda.current_stream().cuda_stream),
              "wmx_rtp_record")
        return taps

    def _record_end(self, name, streams):
        import numpy as np
        idx = None if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(getattr(lib(), name)(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size,
                                   torch.cuda.current_stream().cuda_stream), name)

    def record_stop(self, streams=None):
        """the listed streams' taps (None = every tap) are free from the next tick on: wmx_rtp_record_stop"""
        self._record_end("wmx_rtp_record_stop", streams)

    def reset_record(self, streams=None):
        """the same with written = 0, what a new call needs: wmx_rtp_reset_record"""
        self._record_end("wmx_rtp_reset_record", streams)

    def record_rings(self, mix, rows=None, legs=None):
        """one tick of every tap in front of egress_rings(mix) (wmx_rtp_record_rings) -> (legs int32 CUDA [max_taps], rows int16 CUDA
        [max_taps, row_samples]): a running tap's row and leg, -1 and no row for a free one; the rings are not zeroed"""
        n = lib().wmx_rtp_record_row_bytes(self._h) // 2
        dev = torch.device("cuda", torch.cuda.current_device())
        rows = torch.zeros((self.max_taps, n), dtype=torch.int16, device=dev) if rows is None else rows
        legs = torch.full((self.max_taps,), -1, dtype=torch.int32, device=dev) if legs is None else legs
        assert rows.is_cuda and rows.dtype == torch.int16 and rows.stride(1) == 1 and tuple(rows.shape) == (self.max_taps, n)
        assert legs.is_cuda and legs.dtype == torch.int32 and legs.is_contiguous() and tuple(legs.shape) == (self.max_taps,)
        check(lib().wmx_rtp_record_rings(self._h, mix._h, rows.data_ptr(), rows.stride(0), legs.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "wmx_rtp_record_rings")
        return legs, rows

    def export_record(self):
        """dict(leg: int32, left, written: uint32; [max_taps] each) as the work queued on the current stream leaves them"""
        import numpy as np
        r = {"leg": np.zeros(self.max_taps, np.int32), "left": np.zeros(self.max_taps, np.uint32), "written": np.zeros(self.max_taps, np.uint32)}
        check(lib().wmx_rtp_export_record(self._h, r["leg"].ctypes.data, r["left"].ctypes.data, r["written"].ctypes.data,
                                          torch.cuda.current_stream().cuda_stream), "wmx_rtp_export_record")
        return r

    def set_codecs(self, streams, in_codec, out_law):
        """in_codec ("reference", "pcma", "pcmu", "by_pt") and out_law ("a", "u") of the listed streams (None = all): wmx_rtp_set_codecs"""
        import numpy as np
        idx = None if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
        if idx is not None and idx.size == 0:
            return
        check(lib().wmx_rtp_set_codecs(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else idx.size, CODEC[in_codec],
                                       LAW[out_law], torch.cuda.current_stream().cuda_stream), "wmx_rtp_set_codecs")

    def export_codecs(self):
        """dict(in_codec, out_law: uint8 [n_streams]; refused: uint32 [n_streams]) as the work queued on the current stream leaves them"""
        import numpy as np
        r = {"in_codec": np.zeros(self.n, np.uint8), "out_law": np.zeros(self.n, np.uint8), "refused": np.zeros(self.n, np.uint32)}
        check(lib().wmx_rtp_export_codecs(self._h, r["in_codec"].ctypes.data, r["out_law"].ctypes.data, r["refused"].ctypes.data,
                                          torch.cuda.current_stream().cuda_stream), "wmx_rtp_export_codecs")
        return r

    def ingest_legs(self, packets, recv_bytes, look_ahead=0):
        """ingest_legs() below for this handle's streams as legs, each with its own codec (wmx_rtp_ingest_legs_codecs): a slot that
        arrived and makes no call under the leg's in_codec is counted in export_codecs()["refused"]"""
        assert packets.is_cuda and packets.dtype == torch.uint8 and packets.dim() == 3 and packets.stride(2) == 1 and packets.shape[0] == self.n
        n, k = packets.shape[:2]
        assert recv_bytes.is_cuda and recv_bytes.dtype == torch.int32 and recv_bytes.is_contiguous() and tuple(recv_bytes.shape) == (n, k)
        pcm = torch.zeros((n, k, 160 + look_ahead), dtype=torch.int16, device=packets.device)
        lens = torch.zeros((n, k), dtype=torch.int32, device=packets.device)
        seq = torch.zeros((n, k), dtype=torch.int16, device=packets.device)
        check(lib().wmx_rtp_ingest_legs_codecs(self._h, k, packets.data_ptr(), packets.stride(0), packets.stride(1), recv_bytes.data_ptr(),
                                               pcm.data_ptr(), pcm.stride(0), pcm.stride(1), lens.data_ptr(), seq.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "wmx_rtp_ingest_legs_codecs")
        return pcm, lens, seq

    def state(self, stream=0):
        s, t = C.c_uint16(0), C.c_uint32(0)
        check(lib().wmx_rtp_export(self._h, stream, C.byref(s), C.byref(t)), "wmx_rtp_export")
        return s.value, t.value

    def close(self):
        if self._h:
            lib().wmx_rtp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ingest(packets):
    """packets uint8 CUDA [n, >= 172] -> (pcm int16 [n, 160], pcm_bytes int32 [n], seq_raw int16 [n])"""
    assert packets.is_cuda and packets.dtype == torch.uint8 and packets.dim() == 2 and packets.stride(1) == 1
    n = packets.shape[0]
    pcm = torch.zeros((n, 160), dtype=torch.int16, device=packets.device)
    nbytes = torch.zeros(n, dtype=torch.int32, device=packets.device)
    seq = torch.zeros(n, dtype=torch.int16, device=packets.device)
    check(lib().wmx_rtp_ingest(n, packets.data_ptr(), packets.stride(0), pcm.data_ptr(), pcm.stride(0), nbytes.data_ptr(), seq.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "wmx_rtp_ingest")
    return pcm, nbytes, seq


def ingest_legs(packets, recv_bytes, look_ahead=0):
    """Legs that deliver up to max_packets datagrams in a tick (wmx_rtp_ingest_legs), laid out for MixBatch.load_minus_legs.
    packets uint8 CUDA [n_legs, max_packets, >= 172]; recv_bytes int32 CUDA [n_legs, max_packets], what recvfrom returned per slot
    (<= 0: nothing there).  -> (pcm int16 [n_legs, max_packets, 160 + look_ahead], lens int32 [n_legs, max_packets] (320 or 0),
    seq_raw int16 [n_legs, max_packets]); the PCM row of a slot that made no call is zero."""
    assert packets.is_cuda and packets.dtype == torch.uint8 and packets.dim() == 3 and packets.stride(2) == 1
    n, k = packets.shape[:2]
    assert recv_bytes.is_cuda and recv_bytes.dtype == torch.int32 and recv_bytes.is_contiguous() and tuple(recv_bytes.shape) == (n, k)
    pcm = torch.zeros((n, k, 160 + look_ahead), dtype=torch.int16, device=packets.device)
    lens = torch.zeros((n, k), dtype=torch.int32, device=packets.device)
    seq = torch.zeros((n, k), dtype=torch.int16, device=packets.device)
    check(lib().wmx_rtp_ingest_legs(n, k, packets.data_ptr(), packets.stride(0), packets.stride(1), recv_bytes.data_ptr(), pcm.data_ptr(),
                                    pcm.stride(0), pcm.stride(1), lens.data_ptr(), seq.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "wmx_rtp_ingest_legs")
    return pcm, lens, seq
