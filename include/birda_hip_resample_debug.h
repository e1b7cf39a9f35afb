/* birda_hip_resample_debug.h -- the resampler of libbirda_hip.so alone (birda_amd/csrc/resample.hip): the plan of a rate pair as it
 * lies on the device, and one launch of resample_kernel<FT> / resample16_kernel<FT> on operands of the caller's with no classifier
 * around it, for the tests that hold the operator tap by tap and both kernels element by element to float64
 * (tests/test_resampler_kernel_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that those keep
 * exactly the symbols the ABI tests list.  birda_amd/_lib.py binds it in RESAMPLE_DEBUG_SYMBOLS, and
 * tests/test_binding_docs_resample.py holds that table to this header.
 */
#ifndef BIRDA_HIP_RESAMPLE_DEBUG_H
#define BIRDA_HIP_RESAMPLE_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: builds (or fetches) the plan of the rate pair on `device` and copies it back.
 * params[8] = {hop, N, nblk, K, dmin, form, FT, s}: a frame is `hop` input samples and N outputs,
 *     y[N m + p] = sum_{k < K} x[hop m + dmin + k] T[p][k];
 *     nblk = ceil(N / 160) column blocks; form 0: polyphase, 1: block (a frame = one block of the FFT resampler);
 *     FT: the frame row tiles (of 16) a workgroup owns, as launch_resample will pick it (4, 2 or 1);
 *     s: the f16 planes hold T * 2^s (op16_unscale = 2^-s).
 * op (may be NULL): receives d_op exactly as it lies on the device, nblk * K * 160 floats, fragment-major
 *     [nblk][K / 16][10][64 lanes][4]: element (cb, g, mt, lane, c) = T[p = 160 cb + 16 mt + (lane & 15)][k = 16 g + 4 (lane >> 4) + c].
 * op16 (may be NULL): receives d_op16 as it lies on the device, 2 * nblk * K * 160 halves (uint16_t bit patterns),
 *     [2 nblk][K / 32][5]{hi, lo}[64 lanes][8]: element (cb, st, mt, plane, lane, j) is the plane's half of
 *     T[p = 80 cb + 16 mt + (lane & 15)][k = 32 st + 8 (lane >> 4) + j] * 2^s.
 * op_cap / op16_cap: the buffers' capacities in elements (floats / halves); a non-NULL buffer that is too small is BH_ERR_INVALID,
 * with the needed count in bh_last_error().  The layouts are not undone here: the test does that, as a second statement of them.
 * A pair the resampler refuses returns BH_ERR_UNSUPPORTED with the plan's message.  Tests only. */
BH_API int bh_debug_resample_plan(int device, uint32_t from_rate, uint32_t to_rate, int32_t *params, float *op, size_t op_cap,
                                  uint16_t *op16, size_t op16_cap);

/* Diagnostic: one launch_resample on host operands, no classifier.
 * in: [n_seg][in_stride] floats, src_len valid samples a row (what lies between src_len and in_stride is the caller's: the
 * tests put NaN there); out: [n_seg][out_stride] floats, all of it copied back.  split_f16 0: resample_kernel<FT> (f32 MFMA),
 * 1: resample16_kernel<FT> (split-f16 MFMA).  kernel (may be NULL): receives the instantiation's name, e.g.
 * "resample_kernel<FT=2>", "resample16_kernel<FT=4>".
 * `in` sits inside 64 KiB guard bands of quiet NaN; `out` and its guards hold the NaN payload 0x7fc0beef before the launch, so an
 * element never written keeps it -- inside [0, out_len) that is a bug, inside [out_len, out_stride) it is the contract -- and a
 * write outside the buffer fails the call ("wrote outside out").
 * BH_ERR_INVALID: a null buffer, n_seg == 0, out_len == 0, equal rates, src_len > in_stride, out_len > out_stride, src_len or
 * out_len above 2^31 - 1, n_seg above 65 535 (the grid's z limit), n_seg * stride past 2^31 elements -- all before anything is
 * allocated, copied or launched.  BH_ERR_UNSUPPORTED: a pair the resampler refuses.  Tests only. */
BH_API int bh_debug_resample(int device, const float *in, size_t n_seg, size_t in_stride, size_t src_len, uint32_t from_rate,
                             uint32_t to_rate, float *out, size_t out_stride, size_t out_len, int split_f16, char *kernel,
                             size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_RESAMPLE_DEBUG_H */
