/* birda_hip_pcm_debug.h -- the segments the device PCM front end of libbirda_hip.so cut (kernels_frontend.hip segment_pcm_kernel<FMT>
 * and the slice logic of api.hip predict_pcm16_core), read back after a bh_predict_pcm* call for the tests that hold them to the
 * decoder's arithmetic bit for bit (tests/test_pcm_segments.py, tests/test_pcm_segments_gpu.py).
 *
 * Like the other debug headers, not part of the boundary birda binds (include/birda_hip.h); its own header so that those keep
 * exactly the symbols the ABI tests list.  birda_amd/_lib.py binds it in PCM_DEBUG_SYMBOLS, and tests/test_binding_docs_pcm.py
 * holds that table to this header.
 */
#ifndef BIRDA_HIP_PCM_DEBUG_H
#define BIRDA_HIP_PCM_DEBUG_H

#include "birda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: the rows the LAST slice of the last bh_predict_pcm / _rows / _fd_rows / _at call on this context left on the device
 * (a slice = up to the context's capacity of consecutive segments; a later call of any kind on the context overwrites them).
 * which 0: the model's input, [rows][sample_count] -- the cut segments themselves, or what the resampler made of them when the
 *          source rate differs from the model's; row_floats must equal sample_count.
 * which 1: the cut segments before resampling, at row stride seg = ceil(sample_count x source_rate / model rate), written only by a
 *          call whose source rate differs from the model's.  The rows sit back to back at that call's seg, so row_floats must be
 *          that seg (the entry cannot know it; it refuses only what exceeds the widest seg the context has served, which is what
 *          the buffer was allocated for).
 * Waits for the context's streams (compute, upload, lanes), then copies rows x row_floats floats to host.  Needs no
 * BIRDA_HIP_KEEP_TENSORS context -- such a context runs no lanes, and the lanes are part of what the tests look at -- and changes
 * nothing on the device.
 * BH_ERR_INVALID, with the rule in bh_last_error(): rows == 0 or beyond what the context's buffers hold; row_floats != sample_count
 * (which 0); row_floats == 0 or beyond the raw buffer's row length, or no resampling call has allocated the raw buffer yet
 * (which 1); which other than 0 / 1.  Tests only. */
BH_API int bh_debug_read_segments(bh_classifier *c, bh_batch_context *ctx, int which, float *host, size_t rows, size_t row_floats);

#ifdef __cplusplus
}
#endif

#endif /* BIRDA_HIP_PCM_DEBUG_H */
