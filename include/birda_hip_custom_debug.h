/* birda_hip_custom_debug.h -- the dense stack of a custom classifier (api_custom.hip: cc_upload_rows / cc_run, which also serve the
 * bat two-stage path and the geomodel range filter) of libbirda_hip.so alone: every class's activated output for host rows, no
 * ranking, for the tests that hold it to float64 element by element (tests/test_custom_stack_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that those keep
 * exactly the symbols the ABI tests list.  birda_amd/_lib.py binds it in CUSTOM_DEBUG_SYMBOLS, and
 * tests/test_binding_docs_custom.py holds that table to this header.
 */
#ifndef BIRDA_HIP_CUSTOM_DEBUG_H
#define BIRDA_HIP_CUSTOM_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: the last layer's activated output (the model's output activation not applied) for n host rows [n][input_dim],
 * through the upload and the launches bh_custom_classifier_predict_batch takes, in the classifier's own buffers and on its
 * stream.  out is [n][n_classes].
 * kernel (may be NULL): receives the name of the last GEMM launched, e.g. "pw_gemm_kernel<BM=64,NT=2>".
 * Tests only. */
BH_API int bh_debug_custom_logits(bh_custom_classifier *cc, const float *rows, size_t n, float *out, char *kernel, size_t kernel_cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_CUSTOM_DEBUG_H */
