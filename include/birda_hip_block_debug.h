/* birda_hip_block_debug.h -- one fused MBConv block of libbirda_hip.so alone (mbconv_kernel: expand -> depthwise -> project), on
 * operands of the caller's, for the tests that hold every instantiation of mbconv_cfgs.inc to float64 element by element
 * (tests/test_mbconv_block.py, tests/test_mbconv_block_gpu.py).
 *
 * Like include/birda_hip_debug.h, include/birda_hip_audit.h and include/birda_hip_layer_debug.h, not part of the boundary birda
 * binds (include/birda_hip.h); its own header so that those keep exactly the diagnostics their binding tests list.
 * birda_amd/_lib.py binds it in BLOCK_DEBUG_SYMBOLS, and tests/test_binding_docs.py holds that table to this header.
 */
#ifndef BIRDA_HIP_BLOCK_DEBUG_H
#define BIRDA_HIP_BLOCK_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The block's shape, 23 int32:
 *   {H, W, Cin, Cexp, Cout, Ho, Wo, pad_t, pad_l, KS, ST, act, precision, noexp, se, dblk,
 *    stem_c, stem_h, stem_w, stem_k, stem_s, stem_pt, stem_pl}
 * H x W is the image the depthwise convolution reads, Ho x Wo what it leaves (taps past the image read zero: the bottom / right
 * padding is what Ho, Wo imply).  act: the model file's code of the expand and depthwise activation (2 ReLU6, 3 swish, 4 GELU);
 * the project convolution has none.  precision: 0 f32 MFMA, 1 plain f16, 3 split f16 -- the planner is asked for exactly that one.
 * noexp: no expand convolution (Cexp == Cin).  se: pass A of a squeeze-excite block (D and the per-tile channel sums instead of Y);
 * dblk: D blocked, [row tile of 16 pixels][Cexp / 16][16 rows][16 channels] (se only; Cexp and Ho Wo multiples of 16).
 * stem_c > 0: the stem form -- the "expand" is the stem_k x stem_k stride-stem_s convolution of the planar spectrogram
 * [n][stem_c][stem_h][stem_w], H x W its output and Cin = stem_k stem_k stem_c.
 *
 * The plan record, 24 int32 (the rest zero):
 *   [0] the full configuration index (activation copy included), [1] TH as planned, [2] tiles_y, [3] tiles_x, [4] nchunks, [5] KG,
 *   [6] 1 when the entry has a pass-A instantiation, [7] the row's own TH, [8] S, [9] CE, [10] NTOP, [11] LDS bytes,
 *   [12] the channel split BH_FLAG_LOW_LATENCY gives the block (bh_debug_mbconv_block: the one that ran), [13] the planned entry has
 *   a one-segment twin (mb_plan_twin), [14] a narrow-tile twin (mb_plan_narrow), [15] the twin's pooled sums are the block's bit for
 *   bit (mb_twin_sums_match), [16] IH, [17] IW, [18] mpad_max, [19] pw_gemm16_gated_wants_blocked for the block, [20] PERSIST.
 * [6] and [7] are filled for a valid force_cfg even when the shape is refused. */

/* Host only, no device touched: what mb_plan makes of the shape.
 * force_cfg: a base index of mbconv_cfgs.inc (the block's activation selects the copy) or -1 for the planner's own choice.
 * variant 0: the planned entry; 1: its one-segment twin (mb_plan_twin); 2: its narrow-tile twin (mb_plan_narrow).
 * name (may be NULL): the instantiation as a profiler prints its template arguments, "mbconv<KS,ST,...,COLTH,SE>".
 * A shape no block can have: BH_ERR_INVALID.  A shape the planner refuses (or a twin that does not exist): BH_ERR_UNSUPPORTED, the
 * planner's reason in bh_last_error(). */
BH_API int bh_debug_mbconv_plan(const int32_t *shape, int force_cfg, int variant, int32_t *record, char *name, size_t name_cap);

/* One fused block on host operands, through the code a forward pass goes through: mb_plan for the choice, create's weight
 * preparation (scale exponents, hi / lo planes, folded taps), launch_mbconv.  Operands in the loaders' layouts:
 *   X NHWC [n][H][W][Cin] (stem: planar [n][stem_c][stem_h][stem_w]); We [Cin][Cexp] (stem: rows in [kh][kw][channel] order), be [Cexp]
 *   (both ignored for noexp); Wd [KS KS][Cexp], bd [Cexp]; Wp [Cexp][Cout], bp [Cout]; R [n][Ho][Wo][Cout] or NULL;
 *   gate [n][Cexp] or NULL (no-expand and stem blocks: multiplied into the depthwise output in front of the project convolution).
 * ksplit 0: one workgroup walks all chunks; non-zero: the split BH_FLAG_LOW_LATENCY gives the block (record[12]; 1 when it gives
 * none), followed by the reduction of the partial sums.
 * se == 0: Y [n][Ho][Wo][Cout].  se == 1: pool_part [n][tiles_y tiles_x][Cexp] and, unless D is NULL (sums only), D as dblk says;
 * R, gate and ksplit must be unset.
 * Every device buffer sits inside 64 KiB guard bands of quiet NaN; the outputs and their guards hold the NaN payload 0x7fc0beef
 * before the launch, so an element never written keeps it and a write past an output fails the call.  A refused shape launches
 * nothing.  Tests only. */
BH_API int bh_debug_mbconv_block(int device, const int32_t *shape, size_t n_seg, const float *X, const float *We, const float *be,
                                 const float *Wd, const float *bd, const float *Wp, const float *bp, const float *R, const float *gate,
                                 int force_cfg, int variant, int ksplit, float *Y, float *D, float *pool_part, int32_t *record,
                                 char *name, size_t name_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_BLOCK_DEBUG_H */
