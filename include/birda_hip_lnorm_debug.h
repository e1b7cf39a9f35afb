/* birda_hip_lnorm_debug.h -- one channel LayerNorm launch (OP_LNORM of the model container) of libbirda_hip.so alone, on operands of
 * the caller's, for the tests that hold lnorm_kernel to float64 element by element (tests/test_convnext_gpu.py).
 *
 * Like include/birda_hip_layer_debug.h, not part of the boundary birda binds (include/birda_hip.h); a header of its own so that the
 * existing debug entry points stay exactly what they were.  birda_amd/_lib.py binds it in LNORM_DEBUG_SYMBOLS, and
 * tests/test_binding_docs_lnorm.py holds that table to this header.
 */
#ifndef BIRDA_HIP_LNORM_DEBUG_H
#define BIRDA_HIP_LNORM_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: a LayerNorm over the C channels of each of n_pixels_total pixels, alone, on host operands, through the launcher a
 * forward pass takes: out[p][c] = (X[p][c] - mean_p) / sqrt(var_p + eps) * gamma[c] + beta[c], var_p the biased variance of pixel p.
 * X and out are [n_pixels_total][C] (an NHWC tensor of any image and segment count, flattened), gamma and beta [C].
 * name (may be NULL): receives the name of the instantiation that ran, e.g. "lnorm_kernel<32,1>" (lanes a pixel, 16-byte pieces a
 * lane: C alone decides).
 * The same 64 KiB guard bands of quiet NaN around every device buffer and the same never-written payload 0x7fc0beef in out as the
 * entry points of include/birda_hip_layer_debug.h ("wrote outside out" fails the call).  What create refuses is refused here,
 * BH_ERR_UNSUPPORTED with "not built" in bh_last_error(): C not a multiple of 4, below 4 or above 2048; an eps that is not finite
 * and > 0 is BH_ERR_INVALID.  Tests only. */
BH_API int bh_debug_lnorm(int device, const float *X, const float *gamma, const float *beta, float eps, float *out,
                          size_t n_pixels_total, size_t C, char *name, size_t name_len);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_LNORM_DEBUG_H */
