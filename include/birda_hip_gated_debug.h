/* birda_hip_gated_debug.h -- the f32 gated project GEMM of a squeeze-excite block (kernels_conv.hip pw_gemm_kernel<BM, NT, GATE>,
 * sixteen instantiations behind launch_pw_gemm_gated) of libbirda_hip.so alone on operands of the caller's, for the tests that hold
 * it to float64 element by element (tests/test_gated_gemm.py, tests/test_gated_gemm_f32_gpu.py).  The split-f16 gated GEMMs have
 * bh_debug_gated_gemm (birda_hip_debug.h), which refuses terms 0; bh_debug_layer_gemm (birda_hip_layer_debug.h) never passes a gate.
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that those keep
 * exactly the symbols the ABI tests list.  birda_amd/_lib.py binds it in GATED_DEBUG_SYMBOLS, and tests/test_binding_docs_gated.py
 * holds that table to this header.
 */
#ifndef BIRDA_HIP_GATED_DEBUG_H
#define BIRDA_HIP_GATED_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: C = act((A x gate[row / rows_per_seg]) W + bias) (+ R) on the f32 MFMA kernel, through the call SliceRun::fused_se
 * makes for a precision="f32" classifier (launch_pw_gemm_gated, the residual added after the activation).
 * A [M][K] (the depthwise output D), gate [M / rows_per_seg][K], W [K][N], bias [N], R [M][N] or NULL, C [M][N].  W comes unpadded;
 * its rows are padded to a multiple of 4 floats as create pads them.  act: the activation code of the model file (a project
 * convolution has none, 0; the epilogue's run-time switch serves every code).
 * kernel (may be NULL): receives the instantiation's name, e.g. "pw_gemm_kernel<BM=64,NT=3,GATE>".
 * Every operand, the gate included, sits inside 64 KiB guard bands of quiet NaN; C and its guards hold the NaN payload 0x7fc0beef
 * before the launch, so an element never written keeps it and a write past C fails the call.
 * A null A, gate, W, bias or C, M, K, N or rows_per_seg of 0, M % rows_per_seg != 0, an act out of range or operands past 2^31
 * elements return BH_ERR_INVALID; K % 4 != 0 (the kernel's 16-byte loads) returns BH_ERR_UNSUPPORTED.  Either way nothing is
 * launched and C is left as it was.  Tests only. */
BH_API int bh_debug_gated_gemm_f32(int device, const float *A, const float *gate, const float *W, const float *bias, const float *R,
                                   float *C, size_t M, size_t K, size_t N, size_t rows_per_seg, int act, char *kernel,
                                   size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_GATED_DEBUG_H */
