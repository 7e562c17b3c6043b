/* oracle/orc_libm.c -- TEST INFRASTRUCTURE ONLY.
 * The reference's way of calling libm in the float NS / AEC paths: promote to double, call glibc, round to float
 * (ns_core.c:228 `(float)log((double)magn)`, :748 `exp`, :700 `tanh`, aec_core.c:278 powf).  Bulk versions, used by
 * tests/test_libm_tables.py to sweep the product's table-driven replacements (wmix_amd/csrc/libm_dev.h). */
#include <math.h>
#include <stddef.h>

void orc_libm_log(const float *x, float *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = (float)log((double)x[i]);
}
void orc_libm_exp(const float *x, float *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = (float)exp((double)x[i]);
}
void orc_libm_tanh(const float *x, float *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = (float)tanh((double)x[i]);
}
/* the start-up pink-noise model, ns_core.c:1111-1153: `num / pow(base, exp)` on floats, which C evaluates in double and the assignment rounds */
void orc_libm_div_pow(const float *num, const float *base, const float *e, float *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = (float)((double)num[i] / pow((double)base[i], (double)e[i]));
}
/* the same three expressions BEFORE the rounding to float: how far each double lies from the nearest float rounding boundary decides
 * whether another fp64 library, a few double ulps away, must round to the same float (tests/test_libm_gpu.py) */
void orc_libm_log_dbl(const float *x, double *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = log((double)x[i]);
}
void orc_libm_exp_dbl(const float *x, double *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = exp((double)x[i]);
}
void orc_libm_div_pow_dbl(const float *num, const float *base, const float *e, double *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = (double)num[i] / pow((double)base[i], (double)e[i]);
}
/* aec_core.c:278 calls the float routine powf directly */
void orc_libm_powf(const float *x, const float *e, float *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = powf(x[i], e[i]);
}
/* the same power evaluated in double and rounded once: what a correctly rounded powf would return in all but ~2^-29 of cases */
void orc_libm_pow_d(const float *x, const float *e, float *y, size_t n)
{
    for (size_t i = 0; i < n; i++) y[i] = (float)pow((double)x[i], (double)e[i]);
}
