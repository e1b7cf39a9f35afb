/* birda_hip_gate_debug.h -- the squeeze-excite gate in its three forms, and the plain f32 layer kernels (depthwise, the NCHW stem's
 * direct convolution, global average pool, gate multiply) of libbirda_hip.so, each alone on operands of the caller's, for the tests
 * that hold them to float64 element by element (tests/test_gate_layers.py, tests/test_gate_layers_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that those keep
 * exactly the symbols the ABI tests list.  birda_amd/_lib.py binds it in GATE_DEBUG_SYMBOLS, and tests/test_binding_docs_gate.py
 * holds that table to this header.
 */
#ifndef BIRDA_HIP_GATE_DEBUG_H
#define BIRDA_HIP_GATE_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: the gate of one squeeze-excite block, gate = act2(b2 + act1(b1 + pooled W1) W2), pooled = (sum over tiles of part) / P,
 * through the launcher a forward pass takes.
 * part [n_seg][tiles][C] (the per-tile channel sums pass A of a fused block leaves; the feature map itself, tiles == P, for the gate of
 * a block that runs layer by layer), W1 [C][Cr], b1 [Cr], W2 [Cr][C], b2 [C], gate [n_seg][C].  W1 and W2 come unpadded; their rows
 * are padded to a multiple of 4 floats as create pads them.  act1 / act2: activation codes of the model file.
 * form -1: the form a fused block of these widths takes in a forward pass; 0: the one-launch kernel; 1: the two sixteen-segment
 * launches; 2: the pool and two GEMMs.  A forced form that does not support the widths (form 1: its partial sums do not fit n_seg x C
 * floats; form 0: LDS; form 2: C or Cr not a multiple of 4), and form -1 where no form does, returns BH_ERR_UNSUPPORTED and
 * launches nothing.
 * kernel (may be NULL): receives the names of the kernels that ran joined by '+', e.g. "se_hidden_kernel+se_gate16_kernel".
 * Every operand sits inside 64 KiB guard bands of quiet NaN; gate, the scratch buffers (n_seg x C floats for the pooled rows / the
 * partial hidden sums, n_seg x Cr for the hidden rows: what a forward pass gives them) and their guards hold the NaN payload
 * 0x7fc0beef before the launch, so an element never written keeps it and a write past any of them fails the call.  Tests only. */
BH_API int bh_debug_se_gate(int device, const float *part, size_t n_seg, size_t tiles, size_t P, size_t C, size_t Cr, const float *W1,
                            const float *b1, int act1, const float *W2, const float *b2, int act2, int form, float *gate, char *kernel,
                            size_t kernel_cap);

/* Diagnostic: one plain f32 layer alone through the launcher a forward pass takes.  op is the model file's code:
 *   2 (OP_DWCONV) X NHWC [n_seg][in_h][in_w][c], W [kh][kw][c], bias [c] -> Y NHWC [n_seg][out_h][out_w][c] = act(conv + bias)
 *   1 (OP_CONV)   the stem on the direct kernel: X planar [n_seg][cin][in_h][in_w], W [kh][kw][cin][c], bias [c] -> Y NHWC
 *   4 (OP_GAP)    X [n_seg][in_h * in_w][c] -> Y [n_seg][c], the mean over the image (W, bias, gate unused; out_h = out_w = 1)
 *   6 (OP_SCALE)  X [n_seg][out_h * out_w][c], gate [n_seg][c] -> Y = X x gate (W, bias unused)
 * shape = {in_h, in_w, out_h, out_w, c, kh, kw, sh, sw, pad_t, pad_l, cin}, the first eleven as the pool diagnostic (birda_hip_pool_debug.h) lays them out; out_h, out_w are
 * taken as given (taps past the image are skipped).  act: the activation code (depthwise and stem convolution only).
 * kernel (may be NULL): receives the instantiation's name, e.g. "dwconv_kernel<3,2>", "conv_direct_kernel<NC=4>", "gap_kernel".
 * Guard bands and the unwritten payload as above.  What create refuses for the op -- c not a multiple of 4; a depthwise window
 * other than square 3x3 / 5x5 with one stride of 1 or 2; stem weights beyond 64 KiB of LDS -- returns BH_ERR_UNSUPPORTED with the
 * rule in bh_last_error(), and nothing is launched.  Tests only. */
BH_API int bh_debug_plain_layer(int device, int op, const float *X, const float *W, const float *bias, const float *gate, float *Y,
                                size_t n_seg, const int32_t *shape, int act, char *kernel, size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_GATE_DEBUG_H */
