/* oracle/orc_spl.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Whole-array entry points to the restatement's SPL primitives and real FFTs, so that a Python test can sweep millions of arguments in
 * one call (tests/spl_inputs.py).  Nothing is computed here: every element goes through the exported routine the modules themselves
 * call (orc_vad.c, orc_agc.c, orc_nsx.c). */
#include <stddef.h>
#include <stdint.h>
#include "orc_agc.h"
#include "orc_nsx.h"
#include "orc_vad.h"

/* kind 0: orc_norm_w32(a), 1: orc_norm_u32(a), 2: orc_div_w32_w16(a, (int16_t)b), 3: orc_spl_sqrt(a); b is read by kind 2 only.
 * Returns 0, or -1 for another kind. */
int orc_spl_sweep(int kind, const int32_t *a, const int32_t *b, int32_t *y, size_t n)
{
    if (kind < 0 || kind > 3) return -1;
    for (size_t i = 0; i < n; i++) {
        switch (kind) {
            case 0: y[i] = orc_norm_w32(a[i]); break;
            case 1: y[i] = orc_norm_u32((uint32_t)a[i]); break;
            case 2: y[i] = orc_div_w32_w16(a[i], (int16_t)b[i]); break;
            default: y[i] = orc_spl_sqrt(a[i]); break;
        }
    }
    return 0;
}

/* in: [n_batch][n] samples, out: [n_batch][n + 2] (n / 2 + 1 complex bins), n = 1 << order */
void orc_spl_real_fft_batch(int order, int n_batch, const int16_t *in, int16_t *out)
{
    const size_t n = (size_t)1 << order;
    for (int k = 0; k < n_batch; k++) orc_spl_real_fft(order, in + k * n, out + k * (n + 2));
}

/* in: [n_batch][n + 2], out: [n_batch][n], scale: [n_batch] the inverse transform's scale counts */
void orc_spl_real_ifft_batch(int order, int n_batch, const int16_t *in, int16_t *out, int32_t *scale)
{
    const size_t n = (size_t)1 << order;
    for (int k = 0; k < n_batch; k++) scale[k] = orc_spl_real_ifft(order, in + k * (n + 2), out + k * n);
}
