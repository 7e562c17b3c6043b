"""The runtime calls of one steady-state submit, counted by a -DWMX_FAULT_INJECTION build of the library (every call that goes through
WMX_HIP, wmx_debug_hip_calls()), for the four forms that rotate slots (wmix_amd/csrc/slot_ring.h): the PCM pipe and the RTP pipe (3
slots), wmx_rt_submit over three sub-batches and wmx_conf_submit (3 slots).  The submit counted is the seventh, past the first
rotation, with nothing waited for in between: the slot it takes is still in flight and the download of the step before is still owed.

    WMIX_AMD_ALLOW_VARIANT_BUILD=1 WMIX_AMD_LIB=tools_dev/build/lib_faults.so python tools_dev/slot_calls.py

prints one JSON line {form: calls}; profiles/slots/slot_ring_ab.json holds it for the builds before and after the slot ring."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from wmix_amd import _lib  # noqa: E402
from wmix_amd.conf import ConfBridge  # noqa: E402
from wmix_amd.pipeline import PcmChain, RtpChain  # noqa: E402
from wmix_amd.realtime import RtBatch  # noqa: E402


def main():
    L = _lib.lib()
    assert "WMX_FAULT_INJECTION" in _lib.build_info(), "needs a build that counts its runtime calls"
    L.wmx_debug_fail_nth_hip_call.argtypes = [C.c_long]
    L.wmx_debug_hip_calls.restype = C.c_long
    dev, slot = torch.device("cuda:0"), C.c_int(-1)

    def seventh(submit):
        for _ in range(6):
            assert submit() == 0, L.wmx_last_error()
        L.wmx_debug_fail_nth_hip_call(0)  # disarmed, and the count starts again
        assert submit() == 0, L.wmx_last_error()
        return L.wmx_debug_hip_calls()

    out = {}
    for name, make in (("pipe_pcm", lambda: PcmChain(24, dev, 1, 16000, 10, 5, 15, slots=3)), ("pipe_rtp", lambda: RtpChain(24, dev, slots=3))):
        c = make()
        out[name] = seventh(lambda: L.wmx_pipe_submit(c._h, None, C.byref(slot), None))
        L.wmx_pipe_wait(c._h, -1)
        c.close()
    r = RtBatch(24, dev, sub_batch=10, slots=3, kind="pcm", chn=1, freq=16000, interval_ms=10)
    out["rt_3_sub_batches"] = seventh(lambda: L.wmx_rt_submit(r._h, None, C.byref(slot), None))
    r.wait()
    r.close()
    cb = ConfBridge(10, slots=3, max_packets=3)
    cb.set_conferences([[0, 1], [2, 3, 4], [5, 6, 7, 8]])
    out["conf"] = seventh(lambda: L.wmx_conf_submit(cb._h, C.byref(slot), None))
    cb.wait()
    cb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
