/* birda_hip_resact_debug.h -- the layer kernels of libbirda_hip.so alone in their after-the-add form, act(conv + bias + R): the
 * end of a ResNet block (a layer record whose `reserved` word is RES_ACT_AFTER), on operands of the caller's, for the tests that
 * hold that form to float64 element by element (tests/test_resact_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that
 * include/birda_hip_layer_debug.h keeps exactly its two entries.  birda_amd/_lib.py binds it in RESACT_DEBUG_SYMBOLS, and
 * tests/test_binding_docs_resact.py holds that table to this header.
 */
#ifndef BIRDA_HIP_RESACT_DEBUG_H
#define BIRDA_HIP_RESACT_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: bh_debug_conv_gemm (include/birda_hip_layer_debug.h) with the activation applied AFTER the residual add --
 * C[n][oh][ow][cout] = act(conv(X, W) + bias + R).  The same arguments, layouts, guard bands, 0x7fc0beef payload and kernel name
 * ("conv_gemm16_kernel<3,RELU,AFTER>"; the f32 kernel takes the position at run time and keeps its name).  R is required
 * (BH_ERR_INVALID without it).  terms 0: conv_gemm_kernel, any activation code but 0; terms 1 / 2 / 3: conv_gemm16_kernel, ReLU,
 * ReLU6, swish, GELU or hard swish (1 .. 4, 7).  Anything else: BH_ERR_UNSUPPORTED.  Tests only. */
BH_API int bh_debug_conv_gemm_after(int device, const float *X, const float *W, const float *bias, const float *R, float *C,
                                    size_t n_seg, const int32_t *shape, int act, int terms, char *kernel, size_t kernel_cap);

/* Diagnostic: bh_debug_layer_gemm with the activation applied after the residual add -- C[M][N] = act(A[M][K] W[K][N] + bias +
 * R[M][N]).  The same arguments, guard bands and kernel name ("pw_gemm16s_kernel<3,RELU,AFTER,NTB=2>").  R is required and
 * pool_rows must be 0 (the head kernel has no residual).  terms 0: the f32 GEMM (K % 4 == 0), any activation code but 0; terms
 * 1 / 2 / 3: the split-f16 GEMMs (K % 32 == 0), ReLU, ReLU6, swish, GELU or hard swish.  Tests only. */
BH_API int bh_debug_layer_gemm_after(int device, const float *A, const float *W, const float *bias, const float *R, float *C,
                                     size_t M, size_t K, size_t N, size_t pool_rows, int act, int terms, char *kernel, size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_RESACT_DEBUG_H */
