/*
 * mad_pm_quantile.h -- inspection entry points of mad_pm.h's quantile mode ("Contrast from a
 * quantile" there): the contrast a quantile gives for an image, and the device selection alone.
 * They are to the quantile mode what mad_pm_gradient is to the gradient passes: parity checks and
 * tools call them, the filter does not need them.  Both work on a context of either contrast mode
 * and allocate their device scratch on first use.
 */
#ifndef MAD_PM_QUANTILE_H
#define MAD_PM_QUANTILE_H

#include "mad_pm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K = sqrt(s_q) of a host image (any mad_dtype) at the context's noise scale, spacing and
 * precision: s_q the k-th smallest squared gradient magnitude with
 * k = min(N - 1, max(0, (int64)ceil(q N) - 1)), exactly what a quantile-mode tensor generation of
 * this image uses (0 when s_q = 0).  0 < q <= 1, else MAD_ERR_INVALID; N >= 2^32 is
 * MAD_ERR_UNSUPPORTED.
 * The gradient is step 1 of mad_ced.h as well, so a user of the structure-tensor filters (EED)
 * can hand the result to mad_ced_desc.contrast with the same noise scale, spacing and precision. */
int mad_pm_contrast(mad_pm_ctx *ctx, const void *image, int32_t dtype, double q, double *contrast);

/* The device selection alone: *out = the k-th smallest (0-based) of the n host values, exactly
 * (the same bits).  n >= 1 and 0 <= k < n, else MAD_ERR_INVALID (the context stays usable);
 * n >= 2^32 is MAD_ERR_UNSUPPORTED.  The values must be non-negative and finite: the selection
 * orders bit patterns, so a negative value, an infinity or a NaN is undefined input (-0.0 orders
 * above every positive value). */
int mad_pm_select(mad_pm_ctx *ctx, const double *values, int64_t n, int64_t k, double *out);

#ifdef __cplusplus
}
#endif
#endif
