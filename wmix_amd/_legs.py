"""What the batch classes' process_legs share (nsx.py, agc.py, vad.py): the checks of the bridge's rows and the call."""
import torch

from ._lib import check, lib


def process_legs(batch, entry, pcm, lens, calls, *extras):
    """entry(batch._h, pcm, leg stride, packet stride, max_packets, lens, calls, *extras, stream) on the current stream.  pcm int16 CUDA
    [n_streams, max_packets, >= 160]; lens 4-byte words CUDA [n_streams, max_packets]; calls None or 4-byte words CUDA [n_streams];
    extras: pointers (or None) the entry point takes behind the call lists."""
    n = batch.n_streams
    assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 3 and pcm.shape[0] == n and pcm.stride(2) == 1
    k = pcm.shape[1]
    assert lens.is_cuda and lens.element_size() == 4 and lens.is_contiguous() and tuple(lens.shape) == (n, k)
    assert calls is None or (calls.is_cuda and calls.element_size() == 4 and calls.is_contiguous() and tuple(calls.shape) == (n,))
    check(getattr(lib(), entry)(batch._h, pcm.data_ptr(), pcm.stride(0), pcm.stride(1), k, lens.data_ptr(),
                                None if calls is None else calls.data_ptr(), *extras, torch.cuda.current_stream().cuda_stream), entry)
    return pcm
