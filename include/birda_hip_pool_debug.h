/* birda_hip_pool_debug.h -- one windowed pooling layer (MaxPool / AveragePool; OP_POOL of the model container) of libbirda_hip.so
 * alone, on operands of the caller's, for the tests that hold it to float64 element by element (tests/test_pool_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that those keep
 * exactly the symbols the ABI tests list.  birda_amd/_lib.py binds it in POOL_DEBUG_SYMBOLS, and tests/test_binding_docs_pool.py
 * holds that table to this header.
 */
#ifndef BIRDA_HIP_POOL_DEBUG_H
#define BIRDA_HIP_POOL_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: one pool layer alone, on host operands, through the launcher a forward pass takes.
 * X is NHWC [n_seg][in_h][in_w][c], Y is NHWC [n_seg][out_h][out_w][c].
 * shape = {in_h, in_w, out_h, out_w, c, kh, kw, sh, sw, pad_t, pad_l}; out_h, out_w are taken as given (a window's taps past the
 * image are skipped, so the bottom / right padding is whatever they imply).
 * mode 0: max (a NaN tap makes the output NaN); 1: mean over the in-image taps (count_include_pad = 0); 2: mean over kh * kw.
 * kernel (may be NULL): receives the name of the instantiation that ran, e.g. "pool_kernel<MAX>".
 * X sits inside 64 KiB guard bands of quiet NaN (a read past it shows up as NaN in Y); Y and its guards hold the NaN payload
 * 0x7fc0beef before the launch, so an element never written keeps it and a write past Y fails the call ("wrote outside Y").
 * A shape the model validator would refuse (c % 4 != 0, mode > 2, pad_t >= kh, pad_l >= kw, a window without a pixel of the
 * image, a dimension out of range) returns BH_ERR_UNSUPPORTED.  Tests only. */
BH_API int bh_debug_pool(int device, const float *X, float *Y, size_t n_seg, const int32_t *shape, int mode, char *kernel,
                         size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_POOL_DEBUG_H */
