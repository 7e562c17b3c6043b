"""A model of the bridge's per-leg voice-activity gate (wmx_vad_process_legs), written from the text in include/wmix_amd.h: per leg one
handle of the oracle's VAD (oracle/orc_vad.c, orc_vad_init(1, 8000, 20): a packet of 160 samples, one row) that lives as long as the
call; per tick the leg's PCM rows, lens and, with sequencing, the call list.  The rows a leg's load will consume -- without a list the
slots with len == 320 in slot order, with one the list's data calls that name such a slot, in list order; a silence call feeds nothing
-- are each one orc_vad_run of 160 frames on the leg's handle, in place.

The oracle's handle is mirrored as a ctypes structure only to READ `reduce` (oracle/orc_vad.h); right behind init the mirror is held
against what vad_init leaves (pkg == 160, reduce == 4).  Voice or not is read from the step `reduce` made: a decision that is voice
moves it down, or leaves it at 0; one that is not moves it up, or leaves it at 4.  From 0 a row that is not voice goes to 1 and from 4
a row that is voice goes to 3, so staying on a rail is never ambiguous and the step alone tells.
Nothing of wmix_amd is imported or read."""
import ctypes as C

import numpy as np

from leg_rows_model import ROW, legs_fed


class OrcVadCore(C.Structure):  # orc_vad_core, oracle/orc_vad.h
    _fields_ = [("ds_state", C.c_int32 * 4), ("noise_means", C.c_int16 * 12), ("speech_means", C.c_int16 * 12), ("noise_stds", C.c_int16 * 12),
                ("speech_stds", C.c_int16 * 12), ("frame_counter", C.c_int32), ("over_hang", C.c_int16), ("num_of_speech", C.c_int16),
                ("index_vector", C.c_int16 * 96), ("low_value_vector", C.c_int16 * 96), ("mean_value", C.c_int16 * 6),
                ("upper_state", C.c_int16 * 5), ("lower_state", C.c_int16 * 5), ("hp_filter_state", C.c_int16 * 4)]


class OrcVad(C.Structure):  # orc_vad
    _fields_ = [("core", OrcVadCore), ("chn", C.c_int), ("freq", C.c_int), ("interval_ms", C.c_int), ("pkg", C.c_int), ("reduce", C.c_int)]


_i16p = np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS")
_BOUND = {}


def bind(lib):
    """(init, run, release) of the oracle's VAD handle, prototypes set once"""
    if id(lib) not in _BOUND:
        init, run, release = lib.orc_vad_init, lib.orc_vad_run, lib.orc_vad_release
        init.restype, init.argtypes = C.POINTER(OrcVad), [C.c_int, C.c_int, C.c_int]
        run.restype, run.argtypes = None, [C.POINTER(OrcVad), _i16p, C.c_int]
        release.restype, release.argtypes = None, [C.POINTER(OrcVad)]
        _BOUND[id(lib)] = (init, run, release)
    return _BOUND[id(lib)]


def was_voice(before, after):
    """the decision, after hangover, that moved `reduce` from before to after"""
    assert abs(after - before) <= 1 and 0 <= after <= 4
    return after < before or (after == before == 0)


class LegsGateModel:
    """n legs; tick() takes what the ingest, the sequencer, the DTMF stage, the denoiser and the leveller left and leaves what the
    kernel leaves"""

    def __init__(self, lib, n):
        self.init, self.run, self.release = bind(lib)
        self.h = [None] * n
        self.voiced, self.unvoiced = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.trace = [[] for _ in range(n)]  # `reduce` behind every row the leg was fed since its last reset
        self.reset()

    def reset(self, legs=None):
        """vad_release + vad_init, and the leg's two counters back to zero"""
        for g in (range(len(self.h)) if legs is None else legs):
            if self.h[g]:
                self.release(self.h[g])
            self.h[g] = self.init(1, 8000, 20)
            assert self.h[g] and self.h[g].contents.pkg == ROW and self.h[g].contents.reduce == 4  # the mirror reads the right words
            self.voiced[g] = self.unvoiced[g] = 0
            self.trace[g] = []

    @property
    def reduce(self):
        return np.array([h.contents.reduce for h in self.h], np.uint8)

    def feed(self, g, row):
        """one row of leg g -> the gated row"""
        buf = np.ascontiguousarray(row[:ROW], np.int16).copy()
        before = self.h[g].contents.reduce
        self.run(self.h[g], buf, ROW)
        after = self.h[g].contents.reduce
        if was_voice(before, after):
            self.voiced[g] += 1
        else:
            self.unvoiced[g] += 1
        self.trace[g].append(after)
        return buf

    def tick(self, pcm, lens, lists=None):
        """pcm int16 [n, K, >= 160] (rewritten in place), lens [n, K], lists: None or per leg the call list -> per leg the slots fed"""
        fed = legs_fed(lens, lists)
        for g, slots in enumerate(fed):
            for slot in slots:
                pcm[g][slot][:ROW] = self.feed(g, pcm[g][slot])
        return fed

    def export(self):
        return {"reduce": self.reduce, "voiced": self.voiced.copy(), "unvoiced": self.unvoiced.copy()}

    def close(self):
        for g, h in enumerate(self.h):
            if h:
                self.release(h)
                self.h[g] = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gate(lib, rows):
    """rows int16 [n, 160], one leg's whole ordered history from a fresh handle -> (the gated rows, `reduce` behind every row)"""
    m = LegsGateModel(lib, 1)
    out = np.array([m.feed(0, r) for r in np.ascontiguousarray(rows, np.int16).reshape(-1, ROW)], np.int16).reshape(-1, ROW)
    trace = list(m.trace[0])
    m.close()
    return out, trace
