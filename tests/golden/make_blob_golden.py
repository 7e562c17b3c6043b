"""Generates tests/golden/blob_golden.npz: the BYTES of the stream blobs (wmx_<m>_export_stream, include/wmix_amd.h "stream
migration") of all six batched stages and of a chain, so that a change to the code that writes a blob is held against what the
build before it wrote.  The migration tests export and import with one build; an exporter and an importer that are wrong in the
same way pass them.

The committed file was written by the library built from commit f99ee39 ("aec, aecm: share one cohort machinery instead of two
hand-kept copies"), the last one whose six stages each wrote their blob by hand.  It is NOT regenerated when the exporting code
changes -- only when a blob's content changes on purpose (a new format version), and then from the build that introduces it.

Needs a GPU and a built library (WMIX_AMD_LIB may name another build):  python tests/golden/make_blob_golden.py

What is in it (3-4 streams, mono):
  fresh_<stage>_<freq>   the state *_create leaves, every stage; NS and NSX also at 8 kHz (their plane sizes follow the rate)
  run_<stage>_<freq>     the integer stages (NSX, AECM, AGC, VAD: bit-deterministic) after N_RUN packets of wmix_amd.synth input,
                         exported from stream RUN_STREAM of RUN_STREAMS, not stream 0: a field-major plane read with the wrong
                         stride shows there
  run_agc_own_gain       the AGC stream that was reset with a compression gain of its own: the blob's trailer is that gain
  fresh_chain_float/_fixed  a chain with every stage on, in its float and in its fixed-point build
The float stages' processed state depends on the host's libm (tests/test_aec_gpu.py: check_float_path), so none is kept here;
tests/test_blob_format_gpu.py holds those blobs against the debug readers instead.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from wmix_amd import synth  # noqa: E402

FRESH_STREAMS, FRESH_STREAM = 3, 1
RUN_STREAMS, RUN_STREAM, N_RUN = 4, 2, 300
AGC_VALUE, AGC_OWN_STREAM, AGC_OWN_VALUE = 5, 3, 18


def stage_makers():
    """name -> (frequencies, make(n_streams, freq)); in the heartbeat's order"""
    from wmix_amd.aec import AecBatch
    from wmix_amd.aecm import AecmBatch
    from wmix_amd.agc import AgcBatch
    from wmix_amd.ns import NsBatch
    from wmix_amd.nsx import NsxBatch
    from wmix_amd.vad import VadBatch
    return {
        "ns": ((16000, 8000), lambda n, f: NsBatch(n, 1, f)),
        "nsx": ((16000, 8000), lambda n, f: NsxBatch(n, 1, f)),
        "aec": ((16000,), lambda n, f: AecBatch(n, 1, f, 10)),
        "aecm": ((16000,), lambda n, f: AecmBatch(n, 1, f, 10)),
        "agc": ((16000,), lambda n, f: AgcBatch(n, 1, f, AGC_VALUE)),
        "vad": ((16000,), lambda n, f: VadBatch(n, 1, f, 10)),
    }


def run_inputs(freq, dev):
    """(far [N_RUN, pkt], near [RUN_STREAMS, N_RUN, pkt]) on the device"""
    import torch
    pkt = freq // 100
    far = synth.far_end(7700, N_RUN, pkt)
    near = synth.near_end(7701, RUN_STREAMS, N_RUN, pkt, far=far).reshape(RUN_STREAMS, N_RUN, pkt)
    return torch.from_numpy(far.reshape(N_RUN, pkt)).to(dev), torch.from_numpy(near).to(dev)


def run_stage(name, batch, freq, dev):
    """N_RUN packets through a batch of RUN_STREAMS streams, 25 packets a call"""
    far, near = run_inputs(freq, dev)
    for a in range(0, N_RUN, 25):
        if name in ("aec", "aecm"):
            rc, _ = batch.process2(far[a:a + 25], near[:, a:a + 25])
            assert rc == 0
        else:
            batch.process(near[:, a:a + 25])


def chain_stages():
    from wmix_amd.chain import AEC, AECM, AGC, NS, NSX, VAD
    return {"float": NS | AEC | AGC | VAD, "fixed": NS | NSX | AEC | AECM | AGC | VAD}


def fresh_blobs():
    from wmix_amd.chain import ChainBatch
    out = {}
    for name, (freqs, make) in stage_makers().items():
        for freq in freqs:
            b = make(FRESH_STREAMS, freq)
            out["fresh_%s_%d" % (name, freq)] = b.export_stream(FRESH_STREAM)
            b.close()
    for build, stages in chain_stages().items():
        c = ChainBatch(FRESH_STREAMS, 1, 16000, 10, AGC_VALUE, stages=stages)
        out["fresh_chain_%s" % build] = c.export_stream(FRESH_STREAM)
        c.close()
    return out


def run_blobs(dev):
    out = {}
    makers = stage_makers()
    for name in ("nsx", "aecm", "agc", "vad"):
        freqs, make = makers[name]
        for freq in freqs:
            b = make(RUN_STREAMS, freq)
            if name == "agc":
                b.reset_streams_gain([AGC_OWN_STREAM], AGC_OWN_VALUE)
            run_stage(name, b, freq, dev)
            out["run_%s_%d" % (name, freq)] = b.export_stream(RUN_STREAM)
            if name == "agc":
                out["run_agc_own_gain"] = b.export_stream(AGC_OWN_STREAM)
            b.close()
    return out


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "the blobs are exported from the device"
    out = fresh_blobs()
    out.update(run_blobs(torch.device("cuda:0")))
    path = os.path.join(ROOT, "tests", "golden", "blob_golden.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path))
