/* birda_hip_bnact_debug.h -- one norm + activation launch (a folded BatchNormalization and its activation; OP_BNACT of the model
 * container) of libbirda_hip.so alone, on operands of the caller's, for the tests that hold bnact_kernel to float64 element by
 * element (tests/test_bnact_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); a header of its own so that the existing
 * debug entry points stay exactly what they were.  birda_amd/_lib.py binds it in BNACT_DEBUG_SYMBOLS, and
 * tests/test_binding_docs_bnact.py holds that table to this header.
 */
#ifndef BIRDA_HIP_BNACT_DEBUG_H
#define BIRDA_HIP_BNACT_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: one norm + activation launch alone, on host operands, through the launcher a forward pass takes.
 * X and out are [n_pixels_total][C] floats (an NHWC tensor, its pixels counted over every segment), scale and shift [C]:
 * out[p][c] = act(fma(X[p][c], scale[c], shift[c])), one fused multiply-add and the activation in the form that keeps a NaN and
 * the two infinite limits (act(+inf) = +inf, act(-inf) = 0).
 * act: an activation code of the model container -- 1 RELU, 2 RELU6, 3 SWISH, 4 GELU_ERF, 5 GELU_TANH, 7 HSWISH.
 * name (may be NULL): receives the name of the kernel that ran, "bnact_kernel" (one instantiation: the activation is a run-time
 * argument).
 * X sits inside 64 KiB guard bands of quiet NaN (a read past it shows up as NaN in out); out and its guards hold the NaN payload
 * 0x7fc0beef before the launch, so an element never written keeps it and a write past out fails the call ("wrote outside out").
 * C % 4 != 0 or C > 65 536 is BH_ERR_UNSUPPORTED with "not built" in bh_last_error(); an activation outside the six (0 none, 6
 * sigmoid, 8 hard sigmoid, anything else) is BH_ERR_INVALID, as are tensors past 2^31 elements.  Tests only. */
BH_API int bh_debug_bnact(int device, const float *X, const float *scale, const float *shift, int act, float *out, size_t n_pixels_total,
                          size_t C, char *name, size_t name_len);

/* The same launch on DEVICE buffers of the caller's (dX and dOut [n_seg][pixels][C] floats, dScale and dShift [C], which the caller has
 * allocated at those sizes), on the null stream, without a copy, a guard band or a wait: what tools/bnact_layer_times.py puts between
 * two events.  act and name as above.  Refusals as above.  The timing tool only. */
BH_API int bh_debug_bnact_on_device(int device, const float *dX, const float *dScale, const float *dShift, int act, float *dOut, size_t n_seg,
                                    size_t pixels, size_t C, char *name, size_t name_len);

/* The yardstick that tool times the kernel against, on DEVICE buffers of the caller's in the same way: scale_kernel, the squeeze-excite
 * layer's dOut[n][p][c] = dX[n][p][c] * dGate[n][c] (dGate [n_seg][C] floats) -- the nearest existing kernel, one read and one write of the
 * same tensor.  name receives "scale_kernel".  C % 4 != 0 or C > 65 536 is BH_ERR_UNSUPPORTED ("not built").  The timing tool only. */
BH_API int bh_debug_scale_on_device(int device, const float *dX, const float *dGate, float *dOut, size_t n_seg, size_t pixels, size_t C,
                                    char *name, size_t name_len);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_BNACT_DEBUG_H */
