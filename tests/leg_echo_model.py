"""The model of the echo control of the bridge's legs (wmx_aecm_process_legs), written from the text in include/wmix_amd.h: per leg ONE
canceller handle of the oracle in the AECM build (orc_aecm_init(1, 8000, 20)) that lives as long as the call does.  Per tick every row
the leg's load will consume (legs_fed of leg_rows_model.py) is one aec_process of 160 frames with the leg's reported delay, in place,
in feeding order; then the tick's far row -- what was sent to the leg -- is one aec_setFrameFar of 160 frames.  The exports are read
from a ctypes mirror of orc_aecm (oracle/orc_aecm.h), checked right behind init.  Nothing of wmix_amd is imported or read."""
import ctypes as C

import numpy as np

from leg_rows_model import ROW, legs_fed

MAXD = 100


class R16(C.Structure):
    _fields_ = [("data", C.c_void_p), ("count", C.c_int), ("rd", C.c_int), ("wr", C.c_int), ("diff_wrap", C.c_int)]

    def avail_read(self):
        return self.count - self.rd + self.wr if self.diff_wrap else self.wr - self.rd


class OrcAecm(C.Structure):  # oracle/orc_aecm.h, field for field
    _fields_ = [("fs", C.c_int), ("known_delay", C.c_int), ("time_for_delay_change", C.c_int), ("ec_startup", C.c_int),
                ("check_buff_size", C.c_int), ("delay_change", C.c_int),
                ("buf_size_start", C.c_short), ("counter", C.c_short), ("sum", C.c_short), ("first_val", C.c_short),
                ("check_buf_size_ctr", C.c_short), ("ms_in_snd", C.c_short), ("filt_delay", C.c_short), ("last_delay_diff", C.c_short),
                ("farend_old", C.c_int16 * 160), ("farend", R16), ("farend_store", C.c_int16 * 4000),
                ("first_vad", C.c_int), ("far_history_pos", C.c_int), ("far_q_domains", C.c_int * MAXD), ("current_vad", C.c_int),
                ("far_fr", R16), ("near_fr", R16), ("out_fr", R16),
                ("far_fr_store", C.c_int16 * 144), ("near_fr_store", C.c_int16 * 144), ("out_fr_store", C.c_int16 * 144),
                ("mult", C.c_int16), ("nlp_flag", C.c_int16), ("fixed_delay", C.c_int16), ("cng_mode", C.c_int16),
                ("seed", C.c_uint32), ("tot_count", C.c_uint32), ("far_history", C.c_uint16 * (65 * MAXD)),
                ("dfa_clean_q", C.c_int16), ("dfa_clean_q_old", C.c_int16), ("dfa_noisy_q", C.c_int16), ("dfa_noisy_q_old", C.c_int16),
                ("near_log", C.c_int16 * 64), ("far_log", C.c_int16), ("echo_adapt_log", C.c_int16 * 64), ("echo_stored_log", C.c_int16 * 64),
                ("ch_stored", C.c_int16 * 65), ("ch_adapt16", C.c_int16 * 65), ("ch_adapt32", C.c_int32 * 65),
                ("x_buf", C.c_int16 * 128), ("d_buf", C.c_int16 * 128), ("out_buf", C.c_int16 * 64),
                ("echo_filt", C.c_int32 * 65), ("near_filt", C.c_int16 * 65), ("noise_est", C.c_int32 * 65),
                ("noise_low_ctr", C.c_int * 65), ("noise_high_ctr", C.c_int * 65), ("noise_est_ctr", C.c_int16),
                ("mse_adapt_old", C.c_int32), ("mse_stored_old", C.c_int32), ("mse_threshold", C.c_int32),
                ("far_energy_min", C.c_int16), ("far_energy_max", C.c_int16), ("far_energy_maxmin", C.c_int16),
                ("far_energy_vad", C.c_int16), ("far_energy_mse", C.c_int16), ("vad_update_count", C.c_int16),
                ("startup_state", C.c_int16), ("mse_channel_count", C.c_int16), ("sup_gain", C.c_int16), ("sup_gain_old", C.c_int16),
                ("sup_a", C.c_int16), ("sup_d", C.c_int16), ("sup_diff_ab", C.c_int16), ("sup_diff_bd", C.c_int16),
                ("mean_far", C.c_int32 * 65), ("mean_near", C.c_int32 * 65), ("mean_bit_counts", C.c_int32 * (MAXD + 1)),
                ("far_initialized", C.c_int), ("near_initialized", C.c_int), ("far_bit_counts", C.c_int * MAXD),
                ("bin_far_hist", C.c_uint32 * MAXD), ("minimum_probability", C.c_int32),
                ("last_delay_probability", C.c_int), ("last_delay", C.c_int), ("chn", C.c_int), ("pkg", C.c_int)]


def bind(lib):
    """the oracle's handle API -> (init, run, release)"""
    vp = C.c_void_p
    init, run, release = lib.orc_aecm_init, lib.orc_aecm_run, lib.orc_aecm_release
    init.restype, init.argtypes = vp, [C.c_int, C.c_int, C.c_int]
    run.restype, run.argtypes = C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int]
    release.restype, release.argtypes = None, [vp]
    return init, run, release


class Leg:
    """one handle: aec_init(1, 8000, 20); process(row) in place with the reported delay, far(row)"""

    def __init__(self, lib, delay_ms=0):
        self._init, self._run, self._release = bind(lib)
        self.delay_ms, self.h = int(delay_ms), None
        self.restart()

    def restart(self):
        self.close()
        self.h = self._init(1, 8000, 20)
        assert self.h
        m = self.mirror()
        # the mirror reads the right words: first and last fields, and the far ring in between
        assert (m.fs, m.ec_startup, m.known_delay, m.farend.count, m.last_delay, m.chn, m.pkg) == (8000, 1, 0, 4000, -2, 1, 160)

    def mirror(self):
        return OrcAecm.from_address(self.h)

    def process(self, row):
        """row int16 [160] -> the canceller's output"""
        src, out = np.ascontiguousarray(row, np.int16), np.zeros(ROW, np.int16)
        assert self._run(self.h, 2, None, src.ctypes.data, out.ctypes.data, ROW, self.delay_ms) == 0
        return out

    def far(self, row):
        src = np.ascontiguousarray(row, np.int16)
        assert src.shape == (ROW,) and self._run(self.h, 1, src.ctypes.data, None, None, ROW, 0) == 0

    def export(self):
        """(ec_startup, far ring fill in ms, knownDelay, the estimator's last_delay)"""
        m = self.mirror()
        return m.ec_startup, m.farend.avail_read() // 8, m.known_delay, m.last_delay

    def ring(self):
        """the control plane's far ring: (rd, wr, diff_wrap)"""
        m = self.mirror()
        return m.farend.rd, m.farend.wr, m.farend.diff_wrap

    def close(self):
        if self.h:
            self._release(self.h)
            self.h = None


class LegsEchoModel:
    def __init__(self, lib, n, delays=0):
        delays = [delays] * n if np.isscalar(delays) else list(delays)
        assert len(delays) == n and all(0 <= d <= 500 for d in delays)
        self.legs = [Leg(lib, d) for d in delays]

    def tick(self, pcm, lens, lists=None, active=None):
        """pcm int16 [n, K, >= 160] (rewritten in place), lens [n, K], lists: None or per leg the call list -> per leg the slots fed"""
        fed = legs_fed(lens, lists)
        for g, slots in enumerate(fed):
            if active is not None and not active[g]:
                fed[g] = []
                continue
            for slot in slots:
                pcm[g][slot][:ROW] = self.legs[g].process(pcm[g][slot][:ROW])
        return fed

    def far(self, rows, active=None):
        """rows int16 [n, >= 160]: what this tick sent to each leg"""
        for g, leg in enumerate(self.legs):
            if active is None or active[g]:
                leg.far(np.array(rows[g][:ROW], np.int16))

    def reset(self, legs=None):
        """aec_release + aec_init for the listed legs; the reported delay stays"""
        for g in (range(len(self.legs)) if legs is None else legs):
            self.legs[g].restart()

    def export(self):
        """-> startup, far_ms, known_delay, delay_blocks: int32 [n] each"""
        return tuple(np.array(v, np.int32) for v in zip(*[leg.export() for leg in self.legs]))

    def close(self):
        for leg in self.legs:
            leg.close()
