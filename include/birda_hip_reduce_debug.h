/* birda_hip_reduce_debug.h -- one reduce layer (max / mean / max + mean over one image axis or both; OP_REDUCE of the model container)
 * of libbirda_hip.so alone, on operands of the caller's, for the tests that hold reduce_kernel to float64 element by element
 * (tests/test_reduce_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); a header of its own so that the existing
 * debug entry points stay exactly what they were.  birda_amd/_lib.py binds it in REDUCE_DEBUG_SYMBOLS, and
 * tests/test_binding_docs_reduce.py holds that table to this header.
 */
#ifndef BIRDA_HIP_REDUCE_DEBUG_H
#define BIRDA_HIP_REDUCE_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: one reduce layer alone, one launch, on host operands, through the launcher a forward pass takes.
 * X is NHWC [n_seg][in_h][in_w][c], Y is NHWC [n_seg][out_h][out_w][c].
 * shape = {in_h, in_w, out_h, out_w, c, kh, kw}: kh is in_h (the rows are reduced) or 1, kw is in_w or 1, out_h = in_h / kh,
 * out_w = in_w / kw.
 * mode 0: max (a NaN tap makes the output NaN); 1: mean, one f32 sum and one division; 2: max + mean of the same window.
 * split 0: the launcher's own choice of how many lanes share one output value, as in every forward pass (the layer's shape alone
 * decides: 1 or 8); 1 or 8 force that form (tools/reduce_layer_times.py times the forms against each other).
 * kernel (may be NULL): receives the name of the instantiation that ran, e.g. "reduce_kernel<MAXMEAN,8>" (the mode, the lanes).
 * X sits inside 64 KiB guard bands of quiet NaN (a read past it shows up as NaN in Y); Y and its guards hold the NaN payload
 * 0x7fc0beef before the launch, so an element never written keeps it and a write past Y fails the call ("wrote outside Y").
 * What create refuses is refused here, BH_ERR_UNSUPPORTED with "not built" in bh_last_error(): c % 4 != 0, mode > 2, a window that is
 * neither the whole axis nor 1, a 1x1 window, more than 65 536 taps, an output image that is not in / window, and mode 1 over both
 * axes of an image with more than one row and column (the global average pool's record).  A split other than 0, 1, 8 is
 * BH_ERR_INVALID.  Tests only. */
BH_API int bh_debug_reduce(int device, const float *X, float *Y, size_t n_seg, const int32_t *shape, int mode, int split, char *kernel,
                           size_t kernel_cap);

/* The same launch on DEVICE buffers of the caller's (dX [n_seg][in_h][in_w][c], dY [n_seg][out_h][out_w][c] floats, which the caller
 * has allocated at those sizes), on the null stream, without a copy, a guard band or a wait: what tools/reduce_layer_times.py puts
 * between two events.  shape, mode, split and kernel as above; mode 3 runs the global average pool's gap_kernel over the same tensor
 * (the window must be the whole image), the yardstick the both-axes max is timed against.  Refusals as above.  The timing tool only. */
BH_API int bh_debug_reduce_on_device(int device, const float *dX, float *dY, size_t n_seg, const int32_t *shape, int mode, int split,
                                     char *kernel, size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_REDUCE_DEBUG_H */
