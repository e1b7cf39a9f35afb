/* birda_hip_gconv_debug.h -- one grouped convolution (OP_GCONV of the model container: ResNeXt / RegNet blocks, grouped 1x1
 * layers) of libbirda_hip.so alone, on operands of the caller's, for the tests that hold its three kernel instantiations to
 * float64 element by element (tests/test_gconv_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that those keep
 * exactly the symbols the ABI tests list.  birda_amd/_lib.py binds it in GCONV_DEBUG_SYMBOLS, and tests/test_binding_docs_gconv.py
 * holds that table to this header.
 */
#ifndef BIRDA_HIP_GCONV_DEBUG_H
#define BIRDA_HIP_GCONV_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: one grouped convolution alone, on host operands, with the weight preparation bh_classifier_create does (the per-tile
 * weight blocks, the f16 planes and their power-of-two pre-scale), through the launcher a forward pass takes.
 * X is NHWC [n_seg][in_h][in_w][cin], C is NHWC [n_seg][out_h][out_w][cout], bias [cout].
 * W is the container's compact layout [kh][kw][cin / groups][cout]: output channel o reads input channels
 * (o / (cout / groups)) * (cin / groups) + 0 .. cin / groups - 1.
 * shape = {in_h, in_w, out_h, out_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l, groups}; out_h, out_w are taken as given (taps
 * outside the image read as zero, so the bottom / right padding is whatever they imply).
 * act: any activation code of the container (0 none, 1 ReLU, 2 ReLU6, 3 swish, 4 erf-GELU, 5 tanh-GELU, 6 sigmoid, 7 hard swish, 8 hard sigmoid).
 * terms 0: gconv_kernel (f32 MFMA); 3: gconv16_kernel<3> (hi / lo split f16 operands); 1: gconv16_kernel<1> (plain f16).
 * There is no two-term form: terms 2, and any shape gconv_supports rejects (groups < 2, a group count that does not divide the
 * channels, a group width that is not a multiple of 4, a kernel outside 1 .. 7, a stride outside 1 .. 2), return BH_ERR_UNSUPPORTED.
 * kernel (may be NULL): receives the name of the instantiation that ran, e.g. "gconv16_kernel<3>".
 * X, the weight blocks and the bias sit inside 64 KiB guard bands of quiet NaN (a read past an operand shows up as NaN in C); C and
 * its guards hold the NaN payload 0x7fc0beef before the launch, so an element never written keeps it and a write past C fails the
 * call ("wrote outside C").  Tests only. */
BH_API int bh_debug_gconv(int device, const float *X, const float *W, const float *bias, float *C, size_t n_seg, const int32_t *shape,
                          int act, int terms, char *kernel, size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_GCONV_DEBUG_H */
