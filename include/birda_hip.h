/*
 * birda_hip.h -- C ABI of libbirda_hip.so, the MI355X (gfx950) implementation of birda's
 * classifier hot path: raw f32 segments -> [resample] -> STFT/mel front-end -> conv stack
 * -> logits -> activation/top-k.
 *
 * birda reaches this path through the Rust API of the third-party crate birdnet-onnx
 * (reference src/inference/classifier.rs:9-13); there is no FFI in the reference, so every
 * entry point below names the Rust call it replaces (file:line under /root/reference).
 * A maintainer binds these with `extern "C"` behind `BirdClassifier`.
 *
 * Conventions: plain pointers and sizes only; every function returns BH_OK (0) or a
 * negative bh_status and never aborts; bh_last_error() returns a thread-local message
 * (the `reason` of Error::Inference / Error::ClassifierBuild, classifier.rs:281-283,472-474).
 * A classifier handle may be used from one thread at a time per batch context (the
 * reference calls `&self` methods from the main thread only, processor.rs:647-671).
 * There is NO CPU fallback: without a HIP device every compute entry point fails with
 * BH_ERR_NO_DEVICE.
 */
#ifndef BIRDA_HIP_H
#define BIRDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BH_API __attribute__((visibility("default")))

typedef enum {
    BH_OK = 0,
    BH_ERR_INVALID = -1,   /* bad argument (wrong segment length, null pointer, batch > context) */
    BH_ERR_IO = -2,        /* model / labels file unreadable or malformed */
    BH_ERR_NO_DEVICE = -3, /* no HIP device / device index out of range */
    BH_ERR_HIP = -4,       /* a HIP runtime call failed; message carries hipGetErrorString */
    BH_ERR_LABELS = -5,    /* label count != model output width (inference/mod.rs:34-37) */
    BH_ERR_UNSUPPORTED = -6, /* a well-formed model whose spectrogram front-end the kernels cannot express, or cannot be read (bh_config.model_path) */
    BH_ERR_INTERNAL = -7,  /* host allocation failure or another C++ exception stopped at the ABI boundary */
    BH_ERR_NONFINITE = -8  /* an f16-operand forward produced inf / NaN logits (operand outside the f16 range) */
} bh_status;

#define BH_MAX_TOP_K 32
/* The widest output a classifier may have: the activation / top-k stage holds one segment's logits in the LDS of its workgroup,
 * 32 768 f32 = 128 KB of the CU's 160 KB.  bh_classifier_create and bh_custom_classifier_create refuse a model with more classes
 * (BH_ERR_UNSUPPORTED; the message states this limit and the model's class count) -- a BHM1 / BHC1 container and an .onnx file
 * alike.  (A geomodel is not ranked and is not held to it.) */
#define BH_MAX_CLASSES 32768

/* ClassifierBuilder::new().model_path().labels_path().top_k().min_confidence()
 * (classifier.rs:269-273) + execution-provider choice (classifier.rs:662-691 -> device). */
typedef struct {
    const char *model_path;  /* the model's .onnx file, as ClassifierBuilder::model_path() takes it (classifier.rs:269-283), or a
                              * BHM1 container (bh_onnx_to_bhm, birda_amd/modelfile.py); told apart by the file's first bytes.
                              * THE FRONT-END RULE for an .onnx file: nothing about the model is assumed.  The conv stack is
                              * read off the graph (birda_amd/csrc/onnx_conv.hpp) and so is the spectrogram front-end in front
                              * of it (birda_amd/csrc/onnx_frontend.hpp): its nodes are run on probe signals by a float64
                              * evaluator inside the library, frame length / step, the window x DFT x mel operator, the
                              * power-law exponent (the LEARNED mag_scale), affine, flip and epsilon are fitted to the
                              * responses, and the fit is verified against the closed form the kernels compute on random
                              * audio (<= 2e-5 of the spectrogram's scale).  A graph whose front-end the kernels cannot
                              * express -- or that uses an operator the evaluator does not run -- is REFUSED (BH_ERR_UNSUPPORTED, the
                              * message names the operator or the property), never approximated.  Only a graph that starts
                              * at the spectrogram [N, C, H, W] (no front-end to read) takes the published front-end of its
                              * family from the table in onnx_conv.hpp; the sample rate, which no graph states, comes from the
                              * same table keyed by the input length (classifier.rs:360-377).  Cost: ~1-3 s of the create for
                              * a BirdNET-sized front-end; bh_onnx_to_bhm runs the conversion once, ahead of time. */
    const char *labels_path; /* one label per line; NULL = no labels (logits-only use) */
    uint32_t top_k;          /* DEFAULT_TOP_K = 5, constants.rs:178 */
    float min_confidence;    /* DEFAULT_MIN_CONFIDENCE = 0.1, constants.rs:25 */
    int32_t device;          /* HIP device ordinal (one process per GPU) */
    uint32_t flags;          /* BH_FLAG_* below; 0 = BH_FLAG_AUTO */
} bh_config;

/* GEMM operand precision of the fused conv blocks (accumulation is always f32):
 *   BH_FLAG_AUTO   (0, the default) BH_FLAG_F16X3 compute that never fails a batch on operand range: a row whose logits come
 *                  out inf / NaN although its samples were finite (an activation reached the f16 maximum 65 504) is computed
 *                  again on the library's own f32 kernels -- that row only, the other rows of the call are untouched -- and
 *                  the event is recorded in bh_classifier_provider_status().fallback_reason and
 *                  bh_classifier_fallback_segments().  The f32 weights are built the first time it happens (a second copy of
 *                  the model on the device).  Mirrors the reference, whose dispatch never fails a batch on operand range
 *                  (processor.rs:269-277) and whose provider selection degrades with a recorded reason (classifier.rs:742-754).
 *   BH_FLAG_F16X3  every f32 operand split into f16 hi + lo, three f16 MFMAs per product:
 *                  ~1e-7 of sum|a b| like the f32 chain, 4.4x its MFMA rate; operands < 65504, else BH_ERR_NONFINITE
 *   BH_FLAG_F16    operands rounded to f16 once (BASELINE config 5): ~1e-3 relative; same range rule
 *   BH_FLAG_F32    v_mfma_f32_16x16x4_f32: exact f32 fmaf chains (0.6x the throughput of the split-f16 path)
 * The environment variable BIRDA_HIP_PRECISION = auto | f32 | f16x3 | f16 overrides the flag. */
/*   BH_FLAG_LOW_LATENCY  (or-ed onto the precision) forwards of at most 32 segments split the expanded channels of the late blocks
 *                  over 2 or 4 workgroups each and add the partial sums in a fixed order: 0.69-0.79 -> 0.34-0.57 ms for a call of 1-32 segments
 *                  (a one-minute file at a time; the reference's per-file loop, processor.rs:582-603).  The split is a property of the
 *                  BLOCK, never of the launch, so within the regime a segment's results still do not depend on the launch it ran in;
 *                  they differ from the large-launch path's by the summation order (~1e-7 of the logit scale, inside the fp32
 *                  tolerance).  Off by default: without it every launch size gives the same bits. */
#define BH_FLAG_LOW_LATENCY 0x10u
/*   BH_FLAG_FULL_PLANES  (or-ed onto the precision) every split-f16 GEMM layer keeps three terms on full hi / lo weight planes, also
 *                  where its weights are f16 values and two terms on compact planes give the same numbers (the default under
 *                  BH_FLAG_AUTO / BH_FLAG_F16X3).  For comparing the two forms on one file in one process; no effect under
 *                  BH_FLAG_F16 and BH_FLAG_F32. */
#define BH_FLAG_FULL_PLANES 0x20u
#define BH_FLAG_PRECISION_MASK 0x3u
#define BH_FLAG_AUTO 0x0u
#define BH_FLAG_F16X3 0x1u
#define BH_FLAG_F16 0x2u
#define BH_FLAG_F32 0x3u
/* First index of a top-k row whose logits were inf / NaN although the segment's samples were finite (the other slots are -1):
 * what the non-finite counter counted.  Host entry points never hand such a row out under BH_FLAG_AUTO (it has been re-run);
 * in the other modes the call that produced it returns BH_ERR_NONFINITE.  Device-resident callers (bh_forward_device) see it
 * in d_topk_index until bh_batch_context_synchronize has re-run the row (BH_FLAG_AUTO) or reported it. */
#define BH_TOPK_NONFINITE -2

/* birdnet_onnx::ModelConfig{sample_rate, segment_duration, sample_count} + labels().len()
 * (classifier.rs:295-297,306,360-377) */
typedef struct {
    uint32_t sample_rate;
    float segment_duration;
    uint32_t sample_count;
    uint32_t n_classes;
    uint32_t embedding_dim;
    uint32_t output_activation; /* 0 none, 1 sigmoid (v2.4), 2 softmax (Perch) */
    uint32_t spec_channels, spec_h, spec_w;
    uint32_t n_layers;
    uint64_t macs_per_segment;  /* conv stack multiply-accumulates (for MFMA utilisation) */
    uint64_t mel_flops_per_segment;
    uint32_t model_type;        /* BH_MODEL_* */
    uint32_t precision;         /* BH_FLAG_AUTO / F16X3 / F16 / F32 the classifier was built with */
} bh_model_info;

/* birdnet_onnx::PredictionResult{predictions: Vec<Prediction{species, confidence, index}>}
 * as consumed at processor.rs:363-385; `species` = bh_classifier_label(index[i]). */
typedef struct {
    uint32_t n_pred;
    int32_t index[BH_MAX_TOP_K];
    float confidence[BH_MAX_TOP_K];
} bh_result;

typedef struct bh_classifier bh_classifier;
typedef struct bh_batch_context bh_batch_context;

/* available_execution_providers() / provider metadata (classifier.rs:259; provider.rs:17-85) */
BH_API int bh_device_count(void);
BH_API const char *bh_backend_name(void); /* "HIP (gfx950)" */
BH_API const char *bh_last_error(void);

/* ---- execution-provider arm (classifier.rs:662-1089) and default batch size (lib.rs:256-288) ----------
 * ExecutionProviderStatus{requested, actual, fallback_reason} (classifier.rs:23-30), plus what
 * `birda providers` prints about a backend (lib.rs:1173-1247). */
typedef struct {
    char requested[32];        /* the device text the caller asked for, lower-cased: "auto", "gpu", "hip", "rocm", "cpu" */
    char actual[32];           /* "HIP" when a gfx950 device serves the run, else "CPU" (= this library is not used) */
    char fallback_reason[256]; /* "" = None */
    int32_t device;            /* HIP ordinal that would serve, -1 when actual is "CPU" */
    uint32_t device_count;
    char device_name[128];     /* hipDeviceProp_t::name */
    char arch[32];             /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    uint32_t compute_units;
    uint64_t hbm_bytes;
} bh_provider_status;
/* select_execution_provider's arm for this backend.  requested (ASCII, any case):
 *   "cpu"            -> actual "CPU", no reason (InferenceDevice::Cpu, :696-705): the caller keeps its ORT CPU path
 *   "auto" / "gpu"   -> "HIP" when a device exists (this backend goes first in gpu_priority), else actual "CPU" with
 *                       fallback_reason "No GPU providers available" (:742-754, :843-854)
 *   "hip" / "rocm"   -> explicit (configure_explicit_provider, :924-984): "HIP", or BH_ERR_NO_DEVICE when no device
 *                       exists (provider_unavailable_error); nothing else is accepted (BH_ERR_INVALID).
 * device_ordinal < 0 picks ordinal 0. */
BH_API int bh_select_provider(const char *requested, int32_t device_ordinal, bh_provider_status *out);
/* The status a built classifier runs under (BirdClassifier::execution_provider_status). */
BH_API int bh_classifier_provider_status(const bh_classifier *c, bh_provider_status *out);
/* segments BH_FLAG_AUTO has re-run on the f32 kernels so far (0: the split-f16 path served everything) */
BH_API uint64_t bh_classifier_fallback_segments(const bh_classifier *c);

/* ModelType (config/types.rs:375-388) as carried in the model container's header */
#define BH_MODEL_BIRDNET_V24 0u
#define BH_MODEL_PERCH_V2 1u
#define BH_MODEL_BIRDNET_V30 2u
#define BH_MODEL_BSG_FINLAND 3u
#define BH_MIN_BATCH_SIZE 1   /* constants.rs:44 */
#define BH_MAX_BATCH_SIZE 512 /* constants.rs:55 */
/* determine_default_batch_size(model_type, ep_status) (lib.rs:256-288; constants.rs:58-73) with this backend's arm:
 * (_, "CPU") 8; (v2.4 | BSG, "CUDA") 64; (v3.0 | Perch, "CUDA") 32; (_, "TensorRT") 32; (_, "HIP") 512; else 16.
 * 512 = MAX_BATCH_SIZE, the largest batch birda's validator admits (cli/validators.rs:140): every launch of the late blocks then
 * has >= 256 workgroups and one batch context holds ~2 GB.  provider_actual NULL = "HIP". */
BH_API size_t bh_default_batch_size(uint32_t model_type, const char *provider_actual);
/* the same for a built classifier (its model family, provider "HIP") */
BH_API size_t bh_classifier_default_batch_size(const bh_classifier *c);

/* ClassifierBuilder::build() (classifier.rs:281-283).  Loads the model, uploads weights,
 * precomputes the folded STFT*mel operators, validates the label count.
 * FLOAT16 MODEL FILES (the `fp16` variant of a published model, which the reference's installer picks for a GPU provider) are
 * read with this meaning: a float16 constant is the exact real number it encodes; Cast between floating types is the identity;
 * the graph is evaluated in the library's own (f32-grade) arithmetic.  The result is at least as exact as any float16 runtime's;
 * it does not imitate that runtime's intermediate rounding or its overflow at 65 504.  The file's input and outputs must be
 * float32 (as the published files' are, behind / in front of a Cast): a float16 graph input or output is refused by name.
 * GEMM layers outside the fused blocks whose weights are f16 values -- every layer of such a file whose BatchNormalization was
 * folded before export -- run two f16 MFMAs per product on half the weight bytes, with the three-term result element for
 * element (bh_classifier_weight_summary; BH_FLAG_FULL_PLANES keeps three terms). */
BH_API int bh_classifier_create(const bh_config *cfg, bh_classifier **out);
/* The conversion bh_classifier_create runs on an .onnx file, as a step of its own (host only, no device): ONNX graph -> BHM1
 * container on disk.  For deployments that convert once and hand the container to every process afterwards (a 437-MB Perch
 * file is parsed and re-laid in ~1 s; the container loads at the disk's rate). */
BH_API int bh_onnx_to_bhm(const char *onnx_path, const char *bhm_path);
/* Diagnostic for a file the front-end rule refuses (and the hook the evaluator's own unit tests use): evaluates ONE tensor of
 * the graph with the library's float64 front-end evaluator.  feed_name (NULL = nothing fed: `target` must be computable from
 * constants) may be a graph input or ANY intermediate tensor -- only the nodes between it and `target` run; feed is row-major
 * with feed_rank dims.  out receives at most out_cap values; out_dims (capacity 8) / out_rank the shape.  Returns BH_OK,
 * BH_ERR_IO for an unreadable file or an operator outside the evaluator's set (named in bh_last_error), BH_ERR_INVALID when
 * out_cap is too small (out_dims / out_rank are still filled).  Host only, no device. */
BH_API int bh_onnx_eval(const char *onnx_path, const char *feed_name, const double *feed, const int64_t *feed_dims, uint32_t feed_rank,
                        const char *target, double *out, size_t out_cap, int64_t *out_dims, uint32_t *out_rank);
BH_API void bh_classifier_destroy(bh_classifier *c);

/* .config() / .labels() (classifier.rs:360-377) */
BH_API int bh_classifier_info(const bh_classifier *c, bh_model_info *info);
BH_API const char *bh_classifier_label(const bh_classifier *c, uint32_t index);

/* BirdClassifier::ensure_warm / warmup (classifier.rs:414-466): one all-zero inference per
 * distinct batch size, recorded only on success. */
BH_API int bh_classifier_ensure_warm(bh_classifier *c, size_t batch_size);
BH_API int bh_classifier_is_warm(const bh_classifier *c, size_t batch_size);

/* create_batch_context(max_batch_size) / ctx.input_buffer_bytes()
 * (classifier.rs:559-565; processor.rs:582-603).  Owns every device buffer a batch needs. */
BH_API int bh_batch_context_create(bh_classifier *c, size_t max_batch, bh_batch_context **out);
BH_API void bh_batch_context_destroy(bh_batch_context *ctx);
BH_API size_t bh_batch_context_bytes(const bh_batch_context *ctx);       /* input buffer bytes */
/* The context's pinned host staging buffer (bh_batch_context_bytes of it).  Between calls it is the caller's to fill: segments or
 * a PCM16 stream assembled THERE and handed to bh_predict_batch_contig / bh_predict_pcm16(_at) go up without another host copy,
 * and a parked context keeps the allocation alive from file to file (a fresh 300-MB hipHostMalloc + hipHostFree costs 35 ms). */
BH_API void *bh_batch_context_host_buffer(bh_batch_context *ctx, size_t *bytes);
/* How the host-fed entry points split a slice of this context (bh_predict_batch*, bh_predict_pcm*): 0 = automatically (the
 * default: sub-slices small enough that the device starts after an eighth of the upload, on the context's own streams), 1 = whole
 * slices, n = n equal sub-slices.  A caller that keeps several contexts busy at once -- bhh_process_files, three packs in flight --
 * overlaps one context's upload with another's forward itself, and a forward over the whole slice is the efficient one then.
 * Results do not depend on it.  Reset to 0 when the context is destroyed (parked). */
BH_API int bh_batch_context_set_sub_slices(bh_batch_context *ctx, uint32_t n);
BH_API size_t bh_batch_context_device_bytes(const bh_batch_context *ctx); /* all device memory */
/* Host-fed slices of this context whose sub-slices could not be placed side by side in the arena and therefore ran one after the
 * other on one stream (slower, same results): 0 in every configuration the library chooses itself; a diagnostic for forced splits. */
BH_API uint64_t bh_batch_context_lane_fallbacks(const bh_batch_context *ctx);
/* A destroyed context is PARKED in its classifier (up to THREE: bhh_process_files keeps three packs in flight) and handed to the next
 * create of that size -- or of down to half that size, in which case it serves the request with its larger buffers while the entry
 * points that take a context enforce the capacity that was ASKED for (bh_predict_batch_with_context, _source_rate; the slicing
 * entry points -- _contig, _logits, bh_predict_pcm*, bh_forward_device -- cut any n into slices of the context's real capacity,
 * so the request size does not bound them).  The per-file pipeline creates a context per file (processor.rs:582-603), and 4 GB of
 * hipMalloc + 576 MB of pinned staging cost more than a short file's inference.  Worst-case resident footprint of the parking:
 * three contexts of the largest batch ever asked for, for the v2.4-shaped model at 1 000 segments 3 x (4.1 GB device + 0.58 GB
 * pinned host).  bh_classifier_trim releases the parked contexts and the classifier's internal one (bh_predict /
 * bh_predict_batch); returns the device bytes freed.  Call between runs, from the predicting thread. */
BH_API size_t bh_classifier_trim(bh_classifier *c);

/* Classifier::predict(&[f32]) (classifier.rs:469-475): exactly sample_count samples. */
BH_API int bh_predict(bh_classifier *c, const float *segment, size_t n_samples, bh_result *out);

/* Classifier::predict_batch(&[&[f32]]) (classifier.rs:478-488): independent host slices,
 * order preserved, one result per input.  Uses an internal context sized on demand. */
BH_API int bh_predict_batch(bh_classifier *c, const float *const *segments, size_t n,
                            size_t n_samples, bh_result *out);

/* Classifier::predict_batch_with_context (classifier.rs:571-582). n <= ctx max_batch. */
BH_API int bh_predict_batch_with_context(bh_classifier *c, bh_batch_context *ctx,
                                         const float *const *segments, size_t n,
                                         size_t n_samples, bh_result *out);

/* Contiguous host fast path [n][sample_count] (same semantics as predict_batch).  When `base` is pinned host memory
 * (bh_host_alloc / bh_host_register below) the segments are uploaded straight from it; pageable memory is first gathered
 * into the context's own pinned staging by worker threads (a host memcpy: the bound of this entry point). */
BH_API int bh_predict_batch_contig(bh_classifier *c, bh_batch_context *ctx, const float *base,
                                   size_t n, bh_result *out);
/* Pinned host memory for segment buffers.  The reference's decode thread fills `Vec<f32>` segments
 * (audio/decode.rs:150-202) that predict_batch borrows as &[&[f32]] (processor.rs:341): a host that keeps its segments in
 * one buffer from bh_host_alloc -- or registers the allocation it already has -- gets the upload at PCIe rate. */
BH_API int bh_host_alloc(size_t bytes, void **out);
BH_API void bh_host_free(void *p);
BH_API int bh_host_register(void *p, size_t bytes);
BH_API int bh_host_unregister(void *p);

/* Raw outputs.  Not exposed to birda today; BASELINE.json's max |dlogit| needs them.
 * logits: host [n][n_classes]; embeddings (nullable): host [n][embedding_dim]
 * (PredictionResult.embeddings, processor.rs:325-329). */
BH_API int bh_predict_batch_logits(bh_classifier *c, bh_batch_context *ctx, const float *base,
                                   size_t n, float *logits, float *embeddings);

/* ---- range filter / species list on the kept top-k --------------------- */
/* BirdClassifier::apply_range_filter (classifier.rs:587-645) runs on every PredictionResult between the
 * classifier call and detection extraction (processor.rs:320); here it is the tail of the top-k kernel, so
 * every entry point (bh_predict*, bh_forward_device's d_topk_*) returns filtered predictions.
 * set_range_filter = filter_predictions (geomodel_filter.rs:46-82) with GeomodelScores flattened onto class
 * indices: scores[c] is the occurrence score of classifier label c, NaN where score_of() is None (no
 * geomodel entry; birda_host.h bhh_project_scores builds the table as geomodel.rs:58-162 does).
 *   score >= threshold: keep (confidence * score when rerank);  score < threshold: drop;
 *   NaN: keep only when keep_unmatched and not rerank (:33-35).  rerank re-sorts by confidence descending.
 * Dropped slots close up; the tail is -1 / 0 padded.  set_species_list = the species-list retain
 * (classifier.rs:617-640), used only while no range filter is set (:587, :617), keep[c] != 0 keeps class c.
 * The caller still applies `confidence >= min_confidence` per detection (processor.rs:375): rerank lowers
 * confidences after the classifier's own threshold.  Call between batches, from the predicting thread. */
BH_API int bh_classifier_set_range_filter(bh_classifier *c, const float *scores, size_t n_classes,
                                          float threshold, int keep_unmatched, int rerank);
BH_API int bh_classifier_set_species_list(bh_classifier *c, const uint8_t *keep, size_t n_classes);
BH_API int bh_classifier_clear_filters(bh_classifier *c);
/* Output activation + top-k + min-confidence + the filter above on caller-held logits (host [n][n_classes], e.g. kept
 * from bh_predict_batch_logits): the stage birdnet_onnx runs after Session::run, on the same kernel the predict entry
 * points use.  Lets a caller change filters / thresholds without re-running the network. */
BH_API int bh_topk_from_logits(bh_classifier *c, const float *logits, size_t n, bh_result *out);

/* ---- device-resident path (bench / multi-GPU sharding: inputs already in HBM) -------- */
/* d_segments: device f32 [n][sample_count]; d_logits: device f32 [n][n_classes];
 * d_topk_index/d_topk_conf (nullable): device [n][top_k], -1 / 0 padded.
 * Enqueues on the context stream; call bh_batch_context_synchronize before reading.
 * n may exceed the context's max_batch: it is processed in max_batch slices. */
BH_API int bh_forward_device(bh_classifier *c, bh_batch_context *ctx, const float *d_segments,
                             size_t n, float *d_logits, int32_t *d_topk_index,
                             float *d_topk_conf);
/* Waits for the context's stream.  When a forward enqueued since the last check produced inf / NaN logits for a segment whose
 * samples were all finite (in the f16 operand modes: an activation reached 65 504):
 *   BH_FLAG_AUTO        those rows (BH_TOPK_NONFINITE in d_topk_index) of every bh_forward_device call since the last
 *                       synchronise are computed again on the f32 kernels, in place (logits and top-k rows), from the calls'
 *                       d_segments -- which must therefore stay valid until the synchronise -- and BH_OK is returned;
 *   the other modes     BH_ERR_NONFINITE (once; the counter is cleared).
 * The host entry points (bh_predict*) do the same before they return their results.  Counted by the top-k stage, i.e. only for
 * forwards that were given top-k buffers. */
BH_API int bh_batch_context_synchronize(bh_batch_context *ctx);
BH_API void *bh_batch_context_stream(bh_batch_context *ctx); /* hipStream_t */

/* (bh_debug_read_tensor and bh_debug_gated_gemm -- what the parity tests and the tuning tools call, and
 * birda never does -- are declared in include/birda_hip_debug.h: this header is the boundary birda binds, VERDICT r5 weak #12.) */
BH_API uint64_t bh_tensor_floats(const bh_classifier *c, uint32_t tensor);

/* Per-stage kernel timing, summed over every bh_forward_device call since profiling was last switched ON
 * (set_profiling(ctx, 1) starts a new measurement; the events are recorded on the context stream around every
 * launch and read here, after a stream synchronise: nothing inside a forward waits for them):
 * stage 0 = min/max, 1 = mel front-end, 2 = full convolutions (the unfused stem and every k x k group-1 layer), 3 = depthwise, 4 = pointwise,
 * 5 = pool, 6 = dense, 7 = top-k, 8 = fused MBConv blocks (expand + depthwise + project in
 * one launch).  ms[] receives BH_N_STAGES floats (HIP-event times). */
#define BH_N_STAGES 9
BH_API int bh_batch_context_set_profiling(bh_batch_context *ctx, int enabled);
BH_API int bh_batch_context_stage_ms(bh_batch_context *ctx, float *ms, uint32_t *launches);

/* Per-launch timing of the same measurement, indexed by the layer a launch starts at (a fused block is booked
 * on its expand layer); every launch since set_profiling(ctx, 1) is summed and counted in launches[]. */
BH_API int bh_batch_context_layer_ms(bh_batch_context *ctx, float *ms, uint32_t *launches, size_t n_layers);

/* Number of expand -> depthwise -> project triples that run as one fused launch; cfgs
 * (nullable) receives the tile configuration index of each.  Environment (tuning / A-B aids, read at
 * create): BIRDA_HIP_FUSE=0 disables fusion (BIRDA_HIP_FUSE_SE=0: of the squeeze-excite blocks only, which then run as expand /
 * depthwise / pool / 1x1 / 1x1 / scale / project layers), BIRDA_HIP_MB_CFG=<i> forces configuration i where it is
 * valid, BIRDA_HIP_MB_PREFER=<i,j,...> tries those first, BIRDA_HIP_MB_WHY=1 prints to stderr, for a block that found no tile
 * configuration, how many entries each rule refused (tools/plan_coverage.py), BIRDA_HIP_KEEP_FUSED=1 materialises the fused blocks' outputs for
 * bh_debug_read_tensor (birda_hip_debug.h), BIRDA_HIP_HEAD_GAP=0 keeps the head conv and the global average pool as two launches,
 * BIRDA_HIP_MEL_F32=1 keeps the front-end on the f32 MFMA in the f16 modes, BIRDA_HIP_MEL32=0/1 forces the 16-frame-fragment /
 * 32-frame-fragment front-end kernel (default: by hop).  BIRDA_HIP_COPY_THREADS=<n> (default min(8, hardware
 * threads / 2)) sets the host threads that gather the caller's segments into pinned memory in the
 * bh_predict_batch* entry points.  (The complete list of names the shipped library reads is held by
 * tests/test_abi_and_host.py::test_environment_names_in_the_shipped_library_are_the_documented_ones; A/B knobs of earlier
 * rounds -- BIRDA_HIP_STEM_F32, BIRDA_HIP_RESAMPLE_F32, BIRDA_HIP_MB_STAMPS, ... -- are gone: an alternative is measured as a second build.) */
BH_API int bh_classifier_fused_blocks(const bh_classifier *c, int32_t *cfgs, size_t cap);

/* How the weights of the GEMM layers outside the fused blocks (full convolutions, 1x1 convolutions, dense layers: the layers with
 * f16 operand planes) are held.  Writes min(cap, BH_WS_COUNT) values to out (nullable), indexed by BH_WS_*, and returns
 * BH_WS_COUNT (or a negative bh_status).  (An array rather than a struct, like bh_classifier_fused_blocks: later values are added
 * at the end.) */
#define BH_WS_FLOAT16_FILE 0          /* 1: the model file's convolution / dense weights were float16 tensors (an .onnx file) */
#define BH_WS_GEMM_LAYERS 1           /* GEMM layers outside fused blocks that run on f16 operand planes (0 under BH_FLAG_F32) */
#define BH_WS_TWO_TERM_LAYERS 2       /* ... of which run two-term products on compact planes (weights that are f16 values) */
#define BH_WS_PLANE_BYTES 3           /* device bytes of all those layers' planes */
#define BH_WS_TWO_TERM_PLANE_BYTES 4  /* device bytes of the two-term layers' planes (half of what BH_FLAG_FULL_PLANES holds for them) */
#define BH_WS_COUNT 5
BH_API int bh_classifier_weight_summary(const bh_classifier *c, uint64_t *out, size_t cap);

/* The same plan for a model FILE, without a device (host logic only: which expand -> depthwise -> project triples fuse and the tile
 * configuration the planner picks for each under precision `flags`).  Returns the number of fused blocks (or a negative
 * bh_status); cfgs / layers (nullable) receive configuration index and first layer of each.  Used by the CPU test that holds the
 * set of shipped tile configurations to what the planner can reach, and by tools/plan_models.py. */
BH_API int bh_plan_fused_blocks(const char *model_path, uint32_t flags, int32_t *cfgs, int32_t *layers, size_t cap);

/* Name of the front-end (STFT x mel) kernel instantiation this classifier launches, as a profiler prints it
 * (e.g. "bh::mel_kernel<6, 3, 1>"): lets the bench match its HIP-event timings and the committed PMC counters to the exact
 * kernel.  After a forward pass it is what the launcher reported for the last launch; before any, the one create planned.
 * Returns the string length. */
BH_API int bh_classifier_frontend_kernel(const bh_classifier *c, char *out, size_t cap);

/* Template arguments of tile configuration `cfg` as a profiler prints them after
 * "mbconv_kernel<" (to match bench timings with rocprofv3 rows); returns the string length. */
BH_API int bh_mb_config_name(int32_t cfg, char *out, size_t cap);
/* The configuration index space is `base + k * n_base`, k the activation family: 0 GELU, 1 swish, 2 ReLU6, 3 hard swish.  Callers of
 * bh_mb_config_name derive n_base as ONE THIRD of the indices it names, so it keeps naming exactly the first three families
 * (0 .. 3 n_base - 1) and answers 0 from 3 n_base on; the two entries below see the whole space: the number of families (4), and
 * the name of any configuration 0 .. families * n_base - 1 (same text as above; 0 past the end). */
BH_API int bh_mb_config_families(void);
BH_API int bh_mb_config_name_ex(int32_t cfg, char *out, size_t cap);

/* decode_and_stream + process_batch for source-rate input (processor.rs:84-87, 220-277): every
 * slice holds n_src_samples = ceil(sample_count * source_rate / sample_rate) samples at
 * source_rate; they are uploaded as they are, resampled and resized to sample_count on the device,
 * and classified.  ctx may be NULL (internal context).  Equal rates forward to predict_batch. */
BH_API int bh_predict_batch_source_rate(bh_classifier *c, bh_batch_context *ctx, const float *const *segments,
                                        size_t n, size_t n_src_samples, uint32_t source_rate, bh_result *out);

/* ---- decoded PCM in, detections out (the file front-end on the device) -------
 * StreamingDecoder::next_segment over a stream of n_frames (decode.rs:150-202): start sample of
 * every segment, including the short trailing one an overlap leaves behind.  Returns the count;
 * starts (nullable) receives min(count, cap) entries. */
BH_API size_t bh_segment_starts(size_t n_frames, size_t segment_samples, size_t overlap_samples, uint64_t *starts,
                                size_t cap);
/* One decoded stream of interleaved PCM16 (host): uploaded once as int16, then on the device
 * append_samples' scaling and mono mix (decode.rs:353-411), next_segment's windows and zero padding,
 * resample_chunk + resize when source_rate differs from the model rate (processor.rs:84-87), and the
 * classifier.  overlap_samples is counted at the model rate (processor.rs:520).  out receives one
 * result per segment; start_samples (nullable) their start positions at the source rate. */
BH_API int bh_predict_pcm16(bh_classifier *c, bh_batch_context *ctx, const int16_t *pcm, size_t n_frames,
                            uint32_t channels, uint32_t source_rate, size_t overlap_samples, bh_result *out,
                            size_t out_cap, size_t *n_segments, uint64_t *start_samples);
/* The same for the other sample formats a WAV file carries (the host decoder's, audio/decode.rs:353-411): 24-bit PCM is widened
 * as symphonia does (value << 8, then / 2^31), 32-bit PCM / 2^31, float32 as is.  `pcm` is the interleaved stream in the file's
 * own byte layout (little endian). */
#define BH_PCM_S16 1u
#define BH_PCM_S24 2u
#define BH_PCM_S32 3u
#define BH_PCM_F32 4u
BH_API int bh_predict_pcm(bh_classifier *c, bh_batch_context *ctx, const void *pcm, uint32_t sample_format, size_t n_frames,
                          uint32_t channels, uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap,
                          size_t *n_segments, uint64_t *start_samples);
BH_API int bh_predict_pcm_at(bh_classifier *c, bh_batch_context *ctx, const void *pcm, uint32_t sample_format, size_t n_frames,
                             uint32_t channels, uint32_t source_rate, const uint64_t *start_samples, size_t n_segments, bh_result *out);
/* bh_predict_pcm with the rows handed over AS THEY COMPLETE: the stream is computed in sub-slices (a few hundred segments each,
 * uploaded and classified one behind the other), and `on_rows` is called on the calling thread for each finished run of
 * consecutive segments -- in order, rows = &out[first_segment], start_samples = their starts at the source rate -- while the
 * device is still busy with the later ones.  This is where process_batch's per-batch work goes (thresholding, building and
 * formatting detections, processor.rs:363-407): a 1 000-segment file's 5 000 detections are collected under the forward instead
 * of after it.  Every row has been delivered exactly once when the call returns BH_OK; on an error some may not have been.
 * The callback must not call back into this context and must not unwind into the library. */
typedef void (*bh_rows_fn)(void *user, size_t first_segment, size_t n_segments, const bh_result *rows, const uint64_t *start_samples);
BH_API int bh_predict_pcm_rows(bh_classifier *c, bh_batch_context *ctx, const void *pcm, uint32_t sample_format, size_t n_frames,
                               uint32_t channels, uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap,
                               size_t *n_segments, uint64_t *start_samples, bh_rows_fn on_rows, void *user);
/* bh_predict_pcm_rows on a stream that still lies in a FILE: the `n_frames` frames start at byte `file_offset` of the open descriptor
 * `fd` (a WAV file's data chunk).  The library's copy workers `pread` the bytes straight into the context's pinned staging buffer --
 * one copy out of the page cache, no mapping of the file, no page faults -- where bh_predict_pcm_rows on a mapped file copies the
 * same bytes behind a minor fault per page (70 000 for a 1 000-segment file).  BH_ERR_UNSUPPORTED when one slice of the stream
 * exceeds the staging buffer (more than two channels of 32-bit samples): map the file and call bh_predict_pcm_rows then.
 * BH_ERR_IO when the file ends inside the stream.  The descriptor is not closed and its offset is not moved.  (Measured on the pool's
 * hosts: no faster than the mapped route end to end -- the inference under the copy is what a file costs; bhh_process_file takes it
 * with BIRDA_HOST_PREAD=1.) */
BH_API int bh_predict_pcm_fd_rows(bh_classifier *c, bh_batch_context *ctx, int fd, uint64_t file_offset, uint32_t sample_format, size_t n_frames,
                                  uint32_t channels, uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap,
                                  size_t *n_segments, uint64_t *start_samples, bh_rows_fn on_rows, void *user);
/* The same with the segment starts given (frames, not decreasing, each < n_frames; a segment that runs past n_frames is zero
 * padded): several short recordings packed into ONE stream -- each followed by a segment's length of silence, so that its
 * trailing segment pads with zeros as next_segment does (decode.rs:188-196) -- go through one upload and one forward
 * (bhh_process_files, include/birda_host.h). */
BH_API int bh_predict_pcm16_at(bh_classifier *c, bh_batch_context *ctx, const int16_t *pcm, size_t n_frames, uint32_t channels,
                               uint32_t source_rate, const uint64_t *start_samples, size_t n_segments, bh_result *out);

/* ---- resampler (reference src/audio/resample.rs:10-105; rubato Fft<f32>, FixedSync::Both,
 * chunk 1024, one new resampler per segment).  The device kernel applies rubato's block
 * operator as a GEMM (birda_amd/csrc/resample.hip: polyphase with period (from, to) / gcd where the block operator is shift-
 * invariant -- up-sampling, decimation by at most 1.5 --, one rubato block a frame beyond: 88.2 ... 500 kHz recordings); identity when
 * the rates are equal.
 * Tolerance vs the block-FFT restatement in the oracle: 2e-5 absolute on |x| <= 1 inputs (that number also covers the block
 * operator's own shift-variance where it decimates in polyphase form).  The kernels themselves are held to their own operator:
 * every output within 7 x 1.2 tau B of the float64 sum over the device's table, tau = 4e-7 max(1, sqrt(K / 1024)), B = sum |t| |x|
 * (+ the f16 planes' subnormal floors in the split-f16 kernel), and the table within one f32 rounding of the float64 operator
 * (tests/test_resampler_kernel_gpu.py, tests/test_resampler.py).
 * src_len, out_len and n_in above 2^31 - 1, and more than 65 535 segments in one bh_resample_device launch between different rates,
 * are BH_ERR_INVALID. */
/* resample(samples, from, to) -> Vec<f32> (resample.rs:10-91): host in, host out */
BH_API int bh_resample(bh_classifier *c, const float *in, size_t n_in, uint32_t from_rate,
                       uint32_t to_rate, float *out, size_t out_cap, size_t *n_out);
/* the length resample() returns for n_in input samples (whole blocks + ceil of the tail, :58-88) */
BH_API int bh_resample_output_len(size_t n_in, uint32_t from_rate, uint32_t to_rate, size_t *n_out);
/* Whether the device resampler has an operator for this rate pair (equal rates: always).  The reference builds its rubato resampler
 * per segment and takes what it gets (resample.rs:19-33, an error only from rubato's constructor); here a pair whose rates share too
 * small a divisor -- a header that says 47 999 Hz -- has no operator that fits a CU, and the caller learns it BEFORE it decodes,
 * stages or uploads anything at that rate: BH_OK, or BH_ERR_UNSUPPORTED with the reason in bh_last_error(). */
BH_API int bh_resample_supported(bh_classifier *c, uint32_t from_rate, uint32_t to_rate);
/* decode_and_stream's per-segment step for a batch (processor.rs:84-87): every row of d_in
 * [n_seg][in_stride] holds src_len source-rate samples of one raw segment; row i of d_out
 * [n_seg][out_stride] receives resample_chunk(..) followed by resize(out_len, 0.0).  Enqueued on
 * the context stream; d_out may be passed straight to bh_forward_device. */
BH_API int bh_resample_device(bh_classifier *c, bh_batch_context *ctx, const float *d_in, size_t in_stride,
                              size_t src_len, uint32_t from_rate, uint32_t to_rate, float *d_out,
                              size_t out_stride, size_t out_len, size_t n_seg);

/* ---- two-stage inference: a custom classifier on the backbone's embeddings ----------------
 * birdnet_onnx::CustomClassifier (built at reference src/lib.rs:883-901 for `--bat <region>`, used at
 * src/pipeline/processor.rs:319-360): a small model that maps the backbone's embedding (1024-d for BirdNET v2.4) to
 * its own classes.  The reference runs it through ONNX Runtime on embeddings copied back to the host; here the
 * embeddings stay in HBM and the dense layers run on the MFMA right behind the backbone.  [EXT] The published
 * BattyBirdNET classifiers are Gemm (+ activation) stacks ending in a sigmoid; the container below (BHC1,
 * birda_amd/modelfile.py write_custom_classifier) states exactly that: dense layers [in][out] + bias + activation, an
 * output activation, labels. */
typedef struct bh_custom_classifier bh_custom_classifier;
/* CustomClassifier::builder().model_path().labels_path().build(); top_k = predictions kept per segment (0 = all classes
 * up to BH_MAX_TOP_K), ordered by confidence; min_confidence is applied by the caller (processor.rs:375) */
BH_API int bh_custom_classifier_create(const char *model_path, const char *labels_path, int32_t device, uint32_t top_k,
                                       bh_custom_classifier **out);
BH_API void bh_custom_classifier_destroy(bh_custom_classifier *cc);
BH_API uint32_t bh_custom_classifier_num_classes(const bh_custom_classifier *cc); /* cc.num_classes() */
BH_API uint32_t bh_custom_classifier_input_dim(const bh_custom_classifier *cc);   /* cc.input_dim() */
BH_API const char *bh_custom_classifier_label(const bh_custom_classifier *cc, uint32_t index);
/* cc.predict_batch(&embeddings): host embeddings [n][input_dim] in, one result per row */
BH_API int bh_custom_classifier_predict_batch(bh_custom_classifier *cc, const float *embeddings, size_t n, bh_result *out);
/* process_batch in bat mode (processor.rs:319-360): backbone forward on the segments, the embedding tensor handed to the
 * custom classifier on the device, ITS predictions returned (they replace the backbone's, :369-372).  The backbone must
 * expose an embedding of cc's input_dim.  logits_out (nullable): host [n][cc classes], for parity checks. */
BH_API int bh_predict_batch_two_stage(bh_classifier *c, bh_batch_context *ctx, bh_custom_classifier *cc,
                                      const float *const *segments, size_t n, size_t n_samples, bh_result *out, float *logits_out);

/* ---- BSG post-processing of the kept predictions -------------------------------------------
 * BirdClassifier::apply_bsg_postprocessing (classifier.rs:508-545) -> birdnet_onnx::BsgPostProcessor::{calibrate,
 * process}: per-species calibration always, species-distribution-model (SDM) adjustment when latitude, longitude and day
 * of year are known.  [EXT] The processor lives in birdnet-onnx; the form used here is the published BSG one, logistic
 * calibration in logit space and a multiplicative occurrence prior:
 *     conf' = sigmoid(intercept[c] + slope[c] * logit(conf)),   conf'' = conf' * prior[c]   (prior NULL = calibration only)
 * applied to the kept top-k (as the reference applies it to PredictionResult), which are then re-sorted by confidence.
 * Runs in the top-k kernel's tail, before the range filter stage (which BSG models skip, processor.rs:316-317).  The tables
 * are per class index; reading the calibration CSV / SDM maps into them is host work outside this library. */
BH_API int bh_classifier_set_bsg(bh_classifier *c, const float *intercept, const float *slope, const float *prior /* nullable */,
                                 size_t n_classes);
BH_API int bh_classifier_clear_bsg(bh_classifier *c);

/* ---- range filter: the geomodel query ------------------------------------------------------
 * birda's RangeFilter (reference src/inference/range_filter.rs:19-51) wraps birdnet_onnx::RangeFilter: a small model that
 * maps (latitude, longitude, week) to one occurrence score per species of ITS OWN label set (12 012 for the published
 * geomodel; the reference's fixture, tests/fixtures/fixture-geomodel.onnx, is Gemm(3 -> 5) + Sigmoid).  Here the dense
 * stack runs on the device (the f32 MFMA GEMM of the custom classifier, sigmoid in its epilogue).
 * model_path: the geomodel's .onnx file itself -- read by the library's own protobuf walk (birda_amd/csrc/onnx_dense.hpp:
 * Gemm / MatMul + Add / Relu / Sigmoid chains; anything else is refused by operator name) -- or a BHC1 container written by
 * birda_amd/convert.py.  labels_path: the GEOMODEL's labels, one per line (blank lines skipped); a label count that differs
 * from the model's output width is BH_ERR_LABELS (RangeFilter::from_config's validation, range_filter.rs:13-18; reference
 * test tests/geomodel_range_filter.rs:104-124).  threshold: species scoring below it are left out of `indices` (birda
 * queries at 0.0 and thresholds afterwards, geomodel_range_filter.rs:90-102).
 * The scores feed bhh_project_scores (birda_host.h) -> bh_classifier_set_range_filter. */
typedef struct bh_range_filter bh_range_filter;
BH_API int bh_range_filter_create(const char *model_path, const char *labels_path, int32_t device, float threshold,
                                  bh_range_filter **out);
BH_API void bh_range_filter_destroy(bh_range_filter *rf);
BH_API uint32_t bh_range_filter_num_species(const bh_range_filter *rf);
BH_API const char *bh_range_filter_label(const bh_range_filter *rf, uint32_t index);
/* RangeFilter::predict(latitude, longitude, month, day) -> Vec<LocationScore> (range_filter.rs:39-51): scores[i] = occurrence
 * score of geomodel species i for ALL species (cap >= num_species); indices (nullable) receives the species with
 * score >= threshold in index order, n_kept (nullable) their count.  Latitude / longitude are narrowed to f32 as the
 * reference narrows them (:46).  [EXT] birdnet-onnx turns (month, day) into BirdNET's week -- 48 per year, four per month:
 * week = min(48, (month - 1) * 4 + (day - 1) / 7 + 1) = bh_birdnet_week, WITHOUT a clamp of the week inside the month (days
 * 29-31 count towards the next month's first week).  The crate's source is not in the reference tree; the form is pinned by
 * birda's own call site instead: `--week w` reaches the query as week_to_start_day(w) -> (month, day)
 * (config/range_filter.rs:120-123, utils/date.rs:57-70), and this is the one four-weeks-per-month form that maps every one of
 * the 48 start days back to its week (a clamp to four weeks per month, rounds 2-3, sent `--week 5` = January 31 to week 4;
 * birda's own 7.6-day `date_to_week`, bhh_date_to_week, inverts 10 of 48).  Open risk, stated: a crate that clamps would give
 * days 29-31 the previous week.  predict_week takes the model's third input as is. */
BH_API int bh_range_filter_predict(bh_range_filter *rf, double latitude, double longitude, uint32_t month, uint32_t day,
                                   float *scores, size_t cap, uint32_t *indices, size_t *n_kept);
BH_API int bh_range_filter_predict_week(bh_range_filter *rf, float latitude, float longitude, float week, float *scores,
                                        size_t cap, uint32_t *indices, size_t *n_kept);
BH_API uint32_t bh_birdnet_week(uint32_t month, uint32_t day);

/* ---- several shards in one process (birda_amd/csrc/multi.hip) -----------------------------------
 * Segments are independent through every stage (processor.rs:363-367): shard g of G owns a contiguous block of the
 * global list and nothing is exchanged but the results.  The reference has no counterpart (it scales out as N
 * processes over one directory with lock files, src/locking/file_lock.rs:36-88); a Rust host drives all the GPUs of a
 * node through these calls from one BirdClassifier. */
typedef struct bh_multi bh_multi;
#define BH_GATHER_AUTO 0u /* RCCL all-gather of the packed top-k rows when every shard has its own device and the
                             communicator comes up, else hipMemcpyDtoH per device */
#define BH_GATHER_HOST 1u
#define BH_GATHER_RCCL 2u /* fail at create when RCCL cannot serve */
typedef struct {
    const char *model_path, *labels_path;
    uint32_t top_k;
    float min_confidence;
    uint32_t flags;         /* BH_FLAG_* */
    const int32_t *devices; /* HIP ordinal of every shard; an ordinal may repeat (logical devices: several shards, each with
                               its own context, stream and host thread, on one GPU) */
    uint32_t n_devices;     /* 0 = one shard per visible device */
    uint32_t max_batch;     /* micro-batch of every shard's context; 0 = bh_default_batch_size */
    uint32_t gather;        /* BH_GATHER_* */
} bh_multi_config;
BH_API int bh_multi_create(const bh_multi_config *cfg, bh_multi **out);
BH_API void bh_multi_destroy(bh_multi *m);
BH_API const char *bh_multi_last_error(void);
BH_API uint32_t bh_multi_shards(const bh_multi *m);
BH_API int bh_multi_shard_device(const bh_multi *m, uint32_t shard);
BH_API const char *bh_multi_gather_backend(const bh_multi *m); /* "rccl" or "host (<why>)" */
BH_API bh_classifier *bh_multi_classifier(bh_multi *m, uint32_t shard); /* labels, info, filters (shared per device) */
BH_API bh_batch_context *bh_multi_context(bh_multi *m, uint32_t shard);
/* the partition: [lo, hi) = [shard * n / G, (shard + 1) * n / G); concatenating the shards restores the list */
BH_API void bh_shard_range(size_t n_total, uint32_t shard, uint32_t n_shards, size_t *lo, size_t *hi);
/* mixed-rate lists (BASELINE config 5) are balanced by SOURCE SAMPLES: item i goes to the shard its midpoint falls in
 * on the cumulative-weight axis; bounds receives n_shards + 1 cut points (contiguous, order-preserving) */
BH_API int bh_shard_ranges_weighted(const uint64_t *weights, size_t n, uint32_t n_shards, size_t *bounds);
/* predict_batch over all shards: host segments [n][sample_count] in, one result per segment in list order */
BH_API int bh_multi_predict_batch_contig(bh_multi *m, const float *base, size_t n, bh_result *out);
/* decode_and_stream's resample step + predict_batch for a list whose items differ in rate / length: per shard one batch
 * per (rate, length) present, results back in list order; bounds_out (nullable) receives the n_shards + 1 cut points */
BH_API int bh_multi_predict_batch_source_rate(bh_multi *m, const float *const *segments, const uint32_t *source_rates,
                                              const size_t *n_src_samples, size_t n, bh_result *out, size_t *bounds_out);
/* device-resident input: d_segments[g] = shard g's [n_per_shard[g]][sample_count] f32 on ITS device; the packed top-k
 * rows are gathered (RCCL all-gather onto shard 0's device + one download, or one download per device) and returned in
 * shard order */
BH_API int bh_multi_forward_device(bh_multi *m, const float *const *d_segments, const size_t *n_per_shard, bh_result *out);

#ifdef __cplusplus
}
#endif
#endif /* BIRDA_HIP_H */
