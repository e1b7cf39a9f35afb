/* birda_hip_dilated_debug.h -- one dilated layer of libbirda_hip.so alone, on operands of the caller's, for the tests that hold the
 * dilated gather to float64 element by element (tests/test_dilated_gpu.py): a full NHWC convolution (OP_CONV) on the implicit-GEMM
 * kernels, or a depthwise convolution (OP_DWCONV) on the layer kernel.
 *
 * Like include/birda_hip_layer_debug.h, not part of the boundary birda binds (include/birda_hip.h); a header of its own so that the
 * existing debug entry points and their shape arrays stay exactly what they were.  birda_amd/_lib.py binds it in
 * DILATED_DEBUG_SYMBOLS, and tests/test_binding_docs_dilated.py holds that table to this header.
 */
#ifndef BIRDA_HIP_DILATED_DEBUG_H
#define BIRDA_HIP_DILATED_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: one convolution whose taps stand dil_h rows and dil_w columns apart, alone, on host operands, through the launcher a
 * forward pass takes -- tap (dy, dx) of output pixel (oy, ox) reads input pixel (oy sh - pad_t + dy dil_h, ox sw - pad_l + dx dil_w);
 * taps outside the image read zero.
 * op 1 (OP_CONV): C[n][oh][ow][cout] = act(conv(X, W) + bias) (+ R, may be NULL), or act(conv(X, W) + bias + R) when after != 0 (R
 *   and an activation required).  X is NHWC [n_seg][in_h][in_w][cin]; W the loaders' layout [kh][kw][cin][cout].  terms as for
 *   the undilated entry of include/birda_hip_layer_debug.h: 0 conv_gemm_kernel (f32 MFMA); 1 / 3 conv_gemm16_kernel (f16 / split f16); 2 its two-term products on
 *   compact planes -- BH_ERR_UNSUPPORTED unless every weight is an f16 value after the pre-scale.
 * op 2 (OP_DWCONV): C[n][oh][ow][c] = act(dwconv(X, W) + bias); cin == cout = c, W [kh][kw][c]; R == NULL, terms == 0, after == 0.
 *   Square 3x3 / 5x5 / 7x7 windows, one stride of 1 or 2; the 7x7 window ("dwconv_kernel<7,1>", "dwconv_kernel<7,2,DIL>") has this entry alone,
 *   at dilation 1 too: the plain-layer diagnostic of include/birda_hip_gate_debug.h keeps the 3x3 / 5x5 windows it always took.
 * shape = {in_h, in_w, out_h, out_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l, dil_h, dil_w}; out_h, out_w >= 1 are taken as given
 * (the bottom / right padding is whatever they imply, a crop included).
 * act: the model file's activation code (0 none, 1 ReLU, 2 ReLU6, 3 swish, 4 GELU, 5 tanh-GELU, 6 sigmoid, 7 hard swish, 8 hard sigmoid).
 * kernel (may be NULL): receives the name of the instantiation that ran -- "conv_gemm_kernel<BM=64,NT=5,DIL>",
 * "conv_gemm16_kernel<3,GELU,DIL>", "conv_gemm16_kernel<3,RELU,AFTER,DIL>", "dwconv_kernel<3,1,DIL>" for a dilated layer (the dilated
 * tap walk is a compile-time flag of the kernels), the undilated layer's name without ",DIL" at dilation 1.  With dil_h == dil_w == 1 the call is
 * the undilated diagnostic of the same layer (include/birda_hip_layer_debug.h, birda_hip_resact_debug.h, birda_hip_gate_debug.h):
 * the same launch, bits and name.
 * The same 64 KiB guard bands of quiet NaN around every device buffer and the same never-written payload 0x7fc0beef in C as
 * those entry points ("wrote outside C" fails the call).  What create refuses is refused here, BH_ERR_UNSUPPORTED: a dilation
 * outside 1 .. 16, a dilation other than 1 on an axis with one tap, kernels / strides / channel counts the layer kernels do not
 * take.  Tests only. */
BH_API int bh_debug_dilated_layer(int device, int op, const float *X, const float *W, const float *bias, const float *R, float *C,
                                  size_t n_seg, const int32_t *shape, int act, int terms, int after, char *kernel, size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_DILATED_DEBUG_H */
