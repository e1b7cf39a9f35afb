/* birda_hip_terms_debug.h -- which split-f16 GEMM layers run two-term products, for the tests that hold the rule
 * (tests/test_onnx_fp16.py, tests/test_fp16_model_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h), and a header of its own so that each
 * of those keeps exactly the diagnostics the ABI tests list.  birda_amd/_lib.py binds it in TERMS_DEBUG_SYMBOLS.
 */
#ifndef BIRDA_HIP_TERMS_DEBUG_H
#define BIRDA_HIP_TERMS_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only (no device): would bh_classifier_create run the [K][N] weight matrix W on two terms?  1: every weight is an f16 value
 * after the power-of-two pre-scale that puts the largest weight in the f16 range (the lo plane of the split is all zero); 0: not;
 * negative: a bh_status.  The answer of the very routine that builds the planes at create. */
BH_API int bh_debug_w16_two_terms(const float *W, size_t K, size_t N);

/* Per layer of the classifier's model: the terms its split-f16 GEMM runs with (1, 2 or 3), 0 for a layer without f16 operand
 * planes (inside a fused block, depthwise, pool, every layer under BH_FLAG_F32).  Writes min(cap, layers) values to terms
 * (nullable) and returns the number of layers. */
BH_API int bh_debug_layer_terms(const bh_classifier *c, int32_t *terms, size_t cap);

/* The instantiation the split-f16 GEMM of model layer `layer` launched in the classifier's last forward, as the launchers name it
 * (e.g. "pw_gemm16_skinny_kernel<2,NONE>"); empty before any forward and for layers that run elsewhere (fused blocks, f32); a squeeze-excite block's
 * gated project GEMM is recorded on its project layer.  Returns the name's length (written when cap allows) or a negative bh_status. */
BH_API int bh_debug_layer_kernel(const bh_classifier *c, uint32_t layer, char *out, size_t cap);

/* The instantiation the last bh_debug_gated_gemm call (birda_hip_debug.h) launched, as launch_pw_gemm16_gated names it -- e.g.
 * "pw_gemm16_wide_kernel<2,NT=9,RB=2,PF=4>"; empty before any.  Returns the name's length (written when cap allows). */
BH_API int bh_debug_last_gated_kernel(char *out, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_TERMS_DEBUG_H */
