/* birda_hip_concat_debug.h -- one channel concatenation / channel window / channel shuffle launch (OP_CONCAT of the model
 * container) of libbirda_hip.so alone, on operands of the caller's, for the tests that hold it bit for bit
 * (tests/test_concat_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that those keep
 * exactly the symbols the ABI tests list.  birda_amd/_lib.py binds it in CONCAT_DEBUG_SYMBOLS, and
 * tests/test_binding_docs_concat.py holds that table to this header.
 */
#ifndef BIRDA_HIP_CONCAT_DEBUG_H
#define BIRDA_HIP_CONCAT_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: one concat launch alone, on host operands, through the launcher a forward pass takes.
 * X[0 .. n_src - 1], n_src 1 .. 4, are NHWC [n_seg][h][w][total_k]; Y is NHWC [n_seg][h][w][C], C = the sum of the lengths.
 * shape = {h, w, groups, then for every source: total, off, len}: Y's channels are channels off .. off + len - 1 of source 0, then
 * those of source 1, ...; groups > 1 shuffles them, Y[p][c] = cat[p][(c % groups) * (C / groups) + c / groups] (0, 1: no shuffle).
 * kernel (may be NULL): receives the name of the instantiation that ran, "concat_kernel<PLAIN>" or "concat_kernel<SHUFFLE>".
 * Every X sits inside 64 KiB guard bands of quiet NaN; Y and its guards hold the NaN payload 0x7fc0beef before the launch, so an
 * element never written keeps it and a write past Y fails the call ("wrote outside Y").  The launch is a copy: every 32-bit
 * pattern arrives as it was sent.
 * A shape the model validator would refuse (a total, offset or length that is not a multiple of 4, a window past its source, a
 * group count that does not divide C, a dimension out of range) returns BH_ERR_UNSUPPORTED.  Tests only. */
BH_API int bh_debug_concat(int device, const float *const *X, int n_src, float *Y, size_t n_seg, const int32_t *shape, char *kernel,
                           size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_CONCAT_DEBUG_H */
