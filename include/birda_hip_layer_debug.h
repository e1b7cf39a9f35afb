/* birda_hip_layer_debug.h -- the layer kernels of libbirda_hip.so alone, on operands of the caller's, for the tests that hold them
 * to float64 element by element (tests/test_layer_gemm_gpu.py).
 *
 * Like include/birda_hip_debug.h and include/birda_hip_audit.h, not part of the boundary birda binds (include/birda_hip.h); its own
 * header so that the debug header keeps exactly the diagnostics the ABI tests list.  birda_amd/_lib.py binds it in
 * LAYER_DEBUG_SYMBOLS, and tests/test_binding_docs.py holds that table to this header.
 */
#ifndef BIRDA_HIP_LAYER_DEBUG_H
#define BIRDA_HIP_LAYER_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: one full convolution alone, on host operands, through the launcher a forward pass takes --
 * C[n][oh][ow][cout] = act(conv(X, W) + bias) (+ R, may be NULL).
 * X is NHWC [n_seg][in_h][in_w][cin]; W uses the loaders' layout [kh][kw][cin][cout].
 * shape = {in_h, in_w, out_h, out_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l}; out_h, out_w >= 1 are taken as given (output taps
 * past the image read zero, so the bottom / right padding is whatever they imply, a crop included).
 * terms 0: conv_gemm_kernel (f32 MFMA); terms 1 / 3: conv_gemm16_kernel (f16 / split f16), at any cout; terms 2: the same kernel's
 * two-term products on compact planes -- BH_ERR_UNSUPPORTED unless every weight is an f16 value after the pre-scale.
 * act: the model file's activation code (0 none, 1 ReLU, 2 ReLU6, 3 swish, 4 GELU, 5 tanh-GELU, 6 sigmoid, 7 hard swish, 8 hard sigmoid).
 * kernel (may be NULL): receives the name of the instantiation that ran, e.g. "conv_gemm_kernel<BM=64,NT=5>".
 * Every device buffer sits inside 64 KiB guard bands of quiet NaN (a read past an input shows up as NaN in C); C and its guards
 * hold the NaN payload 0x7fc0beef before the launch, so an element never written keeps it and a write past C fails the call
 * ("wrote outside C").  Shapes the kernels do not take are refused: BH_ERR_UNSUPPORTED.  Tests only. */
BH_API int bh_debug_conv_gemm(int device, const float *X, const float *W, const float *bias, const float *R, float *C,
                              size_t n_seg, const int32_t *shape, int act, int terms, char *kernel, size_t kernel_cap);

/* Diagnostic: a pointwise / dense layer or the fused head convolution + pool alone, on host operands, with the same guard bands
 * and kernel name as bh_debug_conv_gemm.
 * pool_rows == 0: C[M][N] = act(A[M][K] W[K][N] + bias) (+ R[M][N], may be NULL).
 *   terms 0: the f32 GEMM (K % 4 == 0); terms 1 / 3: the split-f16 GEMMs (K % 32 == 0, none / GELU / swish / ReLU6 / hard swish); terms 2:
 *   their two-term products on compact planes (BH_ERR_UNSUPPORTED unless W is made of f16 values), also for the head kernel.
 * pool_rows == P > 0: C[M / P][N] = the mean over each run of P rows of act(A W + bias): the head kernel (terms 1 / 3, R == NULL,
 *   P <= 80, K % 32 == 0, N % 128 == 0, GELU / swish / ReLU6 / hard swish).  Tests only. */
BH_API int bh_debug_layer_gemm(int device, const float *A, const float *W, const float *bias, const float *R, float *C,
                               size_t M, size_t K, size_t N, size_t pool_rows, int act, int terms, char *kernel, size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_LAYER_DEBUG_H */
