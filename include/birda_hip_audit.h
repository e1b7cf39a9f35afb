/* birda_hip_audit.h -- introspection of the plans libbirda_hip.so makes at create, for the tests that hold those plans to what the
 * forward pass does (tests/test_arena_plan_gpu.py, tests/test_launch_scale_gpu.py).
 *
 * Like include/birda_hip_debug.h, not part of the boundary birda binds (include/birda_hip.h); its own header so that the debug
 * header keeps exactly the diagnostics the ABI tests list.  birda_amd/_lib.py binds it in AUDIT_SYMBOLS, and
 * tests/test_binding_docs.py holds that table to this header.
 */
#ifndef BIRDA_HIP_AUDIT_H
#define BIRDA_HIP_AUDIT_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The path the forward pass takes at a layer (bh_audit_arena_plan's `path`) */
#define BH_PATH_LAYER 0     /* the layer alone */
#define BH_PATH_FUSED 1     /* [expand ->] depthwise -> project in one launch */
#define BH_PATH_FUSED_SE 2  /* a squeeze-excite block: pass A, the gate, the gated project GEMM */
#define BH_PATH_HEAD_GAP 3  /* head 1x1 conv + the pool after it in one launch */
#define BH_PATH_SE_GATE 4   /* pool -> 1x1 -> 1x1 of a block that runs layer by layer, as the two gate launches */
#define BH_PATH_INNER 5     /* the layer runs inside the launch of an earlier one */
#define BH_PATH_CONCAT 6    /* a chain of concat records (an N-way Concat) gathered in one launch */

/* The activation arena's plan.  n == 0: the plan of the context itself (its forwards of up to max_batch segments); n > 0: the plan
 * the same planner makes for n segments (what a concurrent lane of an n-segment sub-slice gets; host logic only, any n).  Per
 * tensor t (0 = spectrogram, i = output of layer i-1): its offset and its planned size in floats (0: never in the arena); per
 * layer: the path the forward takes there (BH_PATH_*).  `cap` entries each (>= layers + 1).  Returns the number of tensors, or a
 * negative BH_ERR_*. */
BH_API int bh_audit_arena_plan(bh_classifier *c, bh_batch_context *ctx, size_t n, uint64_t *off_floats, uint64_t *size_floats,
                               uint8_t *path, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_AUDIT_H */
