// api_internal.hpp -- what the translation units of the C ABI share.  Round 4 split the one 2 600-line api.hip (VERDICT r3 weak
// #11) into
//   api.hip         the batch contexts, the forward pass over a slice, lanes, the predict, PCM and resampler entry points, and the
//                   diagnostics that read a classifier's or a context's state
//   api_create.hip  bh_classifier_create, phase by phase (config, front end, fused blocks, layers, schedules), and what undoes it
//   api_plan.hip    host-side planning at create: the folded STFT x mel operator, the arena's liveness plan, the fused blocks'
//                   descriptors, and every re-laid weight (the GEMM layers' rows, planes and fragments, the fused blocks')
//   api_custom.hip  custom classifiers on embeddings (bat two-stage inference) and the geomodel range filter
//   api_debug.hip   the kernel diagnostics that take no classifier, on one launch harness; it alone includes their headers
// The shared helpers live in namespace bhi (hidden visibility: nothing of it leaves the library).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <map>
#include <vector>

#include "../../include/birda_hip.h"
#include "../../include/birda_hip_debug.h"
#include "../../include/birda_hip_audit.h"
#include "../../include/birda_hip_terms_debug.h"
#include "../../include/birda_hip_pcm_debug.h"
#include "kernels.hpp"
#include "trace.hpp"
#include "model.hpp"
#include "onnx_dense.hpp"
#include "onnx_conv.hpp"

struct bh_classifier;
struct bh_batch_context;

namespace bhi {

extern thread_local std::string g_err;
int fail(int code, const char *fmt, ...);
int on_exception() noexcept;

#define HIPCHK(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(BH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

enum Stage { ST_MINMAX = 0, ST_MEL, ST_STEM, ST_DW, ST_PW, ST_GAP, ST_DENSE, ST_TOPK, ST_MBCONV };   // (ST_STEM: every full convolution)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A device copy of a host buffer, owned by the object whose list `owned` is: its destructor frees the list, so whatever create
// refuses afterwards, nothing is left on the device.  *dst is written on success only.
template <class P> int upload_owned(std::vector<float *> &owned, const void *src, size_t bytes, P *dst) {
    float *d = nullptr;
    owned.reserve(owned.size() + 1);         // (so that nothing can fail between the allocation and its entry in the list)
    HIPCHK(hipMalloc((void **)&d, bytes ? bytes : 4));
    const hipError_t e = bytes ? hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) { (void)hipFree(d); return fail(BH_ERR_HIP, "hipMemcpy of %zu bytes to the device failed: %s", bytes, hipGetErrorString(e)); }
    owned.push_back(d);
    *dst = (P)d;
    return BH_OK;
}

// What create has made of one layer (api_create.hip prepare_layer, plan_fusion, mark_paths): the weights its kernels read, and the
// path it starts.  build_schedule (api_plan.hip) turns the marks into the schedules; SliceRun (api.hip) launches from the rest.
struct LayerState {
    float *w = nullptr;                      // f32 weights as the kernels want them: re-laid (owned), or the layer's part of d_blob
    int ldw = 0;                             // padded row length of w (pw / dense / full convolutions)
    void *planes = nullptr;                  // f16 hi / lo fragment planes (GEMM layers outside fused blocks), or null
    float unscale = 1.0f;                    // 2^-s of those planes (they hold W * 2^s, kernels.hpp f16_scale_exponent)
    int terms = 0;                           // the terms the planes are run with -- 3 (1 under BH_FLAG_F16), or 2 on compact planes; 0: no planes
    size_t plane_bytes = 0;                  // device bytes of the planes
    std::atomic<const char *> kernel{nullptr};   // what its GEMM / grouped / concat launcher launched last (a string literal), or null
    int fused_at = -1;                       // index into mb (expand layer of a fused block) or -1 (plan_fusion's record)
    char head_gap = 0;                       // 1 = this 1x1 conv + GELU and the global average pool after it run as one launch
    // 1 = this pool layer and the two 1x1 layers after it (the gate of a squeeze-excite block that runs layer by layer) run as the two
    char gap_gate = 0;                       // gate launches (gap_gate_chain): the pool's tensor holds the hidden partial sums until the gate is written
    char concat_chain = 0;                   // records of the concat chain that starts here and runs as ONE launch (0: none; concat_chain_len)
};

// squeeze-excite gates of at least this many channels take the two-launch gate (launch_se_gate16) where it supports their shape
#ifndef BH_SE_GATE16_MIN
#define BH_SE_GATE16_MIN 577
#endif

// One step of the forward, in stream order: the launches that stand for layers first .. last, and every arena tensor they touch
// (tensor t = the output of layer t - 1; tensor 0 = the spectrogram).  The schedule -- built once, at create (api_plan.hip
// build_schedule) -- is the one statement of what the forward launches: forward_slice walks it, plan_arena derives every tensor's
// lifetime and size from it, bh_audit_arena_plan reports its paths.
struct Step {
    uint8_t path = BH_PATH_LAYER;          // BH_PATH_* (birda_hip_audit.h)
    uint32_t first = 0, last = 0;          // the layers it stands for
    int block = -1;                        // fused paths: index into mb / mb_small / mb_narrow / se
    std::vector<uint32_t> reads;           // [0] the input of layer `first`, [1] the residual of layer `last` where it has one
    std::vector<uint32_t> writes;          // [0] the output of layer `last`: the step's result; [1] (SE block) the depthwise output D
    // tensors whose slot the step borrows; floats != 0: per segment, instead of the tensor's own size
    struct Scratch { uint32_t t; size_t floats; };
    std::vector<Scratch> scratch;          // SE block: SE_* below; gate fast path: the pool's and the hidden layer's tensors
};
enum { SE_POOLED = 0, SE_HIDDEN, SE_GATE, SE_SUMS };   // Step::scratch of a fused squeeze-excite block

}  // namespace bhi

struct bh_classifier {
    ~bh_classifier();                        // (api_create.hip) releases everything below, of a half-built classifier too
    bh::Model model;
    int device = -1;                         // (-1: create has not reached the device yet)
    uint32_t top_k = 5;
    float min_conf = 0.1f;
    std::vector<std::string> labels;
    float *d_blob = nullptr;                 // raw model blob (dw / conv weights, biases); one of d_owned
    std::vector<bhi::LayerState> layer;      // per layer, sized once at create (the record holds an atomic: it does not move)
    bool full_planes = false;                // BH_FLAG_FULL_PLANES: no layer takes two terms
    // What a forward launches: the product's schedule (fused blocks, head conv + pool, the gate fast path), the layer-by-layer one of
    // BIRDA_HIP_KEEP_TENSORS contexts, and the one of debug contexts that still run the fused blocks (BIRDA_HIP_KEEP_FUSED)
    std::vector<bhi::Step> sched, sched_layers, sched_keep_fused;
    std::vector<float *> d_owned;            // every upload_owned buffer: the blob, the re-laid weights, the front-end operators
    bh::FrontendParams fe{};
    bh::FrontendParams *d_fe = nullptr;      // device copy read by the mel kernel
    std::atomic<const char *> fe_kernel{nullptr};   // what launch_mel launched last (a string literal); nullptr before any forward
    std::vector<bh::MbDesc> mb;              // fused MBConv blocks (kernels_mbconv.hip)
    int twin_max_segments = 256;             // launches up to this size take the twins (one workgroup per CU at most either way)
    std::vector<bh::MbDesc> mb_small;        // per block: its small-launch twin (cfg < 0: none), same weights (mb_plan_twin)
    std::vector<bh::MbDesc> mb_narrow;       // per block: its few-segment twin on narrow tiles (cfg < 0: none), same weights (mb_plan_narrow)
    // per block: the layers of a squeeze-excite block (MbDesc::se; iP == 0: a plain block) and the floats per segment of its per-tile
    // channel sums, which live in the arena slot of the (never materialised) OP_SCALE output
    struct SeInfo { uint32_t iD = 0, iGap = 0, iPw1 = 0, iPw2 = 0, iScale = 0, iP = 0; size_t part_floats = 0; };
    std::vector<SeInfo> se;
    // squeeze-excite blocks: the D one group of segments may hold between pass A and the gated project GEMM (api.hip SliceRun::fused_se);
    // 0 = whole launches (round 5).  Measured: profiles/r6_i_se_groups.txt
    size_t se_group_bytes = 0;
    bool low_latency = false;                // BH_FLAG_LOW_LATENCY (birda_hip.h)
    int narrow_max_workgroups = 256;         // launches whose narrow tiles number at most this take them: one workgroup a CU at most (round 5, swept
                                             // per layer at 32 .. 256 segments, profiles/r5_g_narrow_tiles_sweep.txt: beyond, every extra workgroup streams
                                             // the block's 2 MB of weights again -- at 512 a launch of 160-256 segments lost 3-4 %)
    int precision = 0;                       // GEMM operands of the fused blocks: 0 f32, 3 f16 hi/lo split, 1 f16
    // BH_FLAG_AUTO (the default): split-f16 compute, and a row whose logits come out inf / NaN from finite samples (an activation
    // left the f16 range) is computed again on the library's own f32 kernels -- by `fb`, a second classifier of the same model
    // file built with BH_FLAG_F32 the first time that happens.  The reference's dispatch never fails a batch on operand range
    // (processor.rs:269-277) and its provider selection degrades with a recorded reason (classifier.rs:742-754).
    bool auto_fallback = false;
    std::string model_path;
    bh_classifier *fb = nullptr;
    std::mutex fb_mu;
    std::atomic<unsigned long long> fallback_segments{0};
    uint64_t mel_flops = 0;
    bh::TopkFilter filter;                   // range filter / species list applied to the kept top-k (device tables below)
    float *d_class_score = nullptr;
    unsigned char *d_species_keep = nullptr;
    float *d_bsg = nullptr;                  // intercept | slope | prior, n_classes each
    std::mutex warm_mu;
    std::set<size_t> warmed;                 // WarmupRegistry, classifier.rs:221-246
    bh_batch_context *internal_ctx = nullptr;
    std::mutex internal_mu;
    // Up to three destroyed batch contexts are parked here and handed to the next bh_batch_context_create of the same size: the
    // per-file pipeline creates and destroys a context per file (reference processor.rs:582-603), bhh_process_files keeps three in
    // flight, and a context is ~1 GB of hipMalloc plus pinned staging memory -- milliseconds per file at GPU throughput.
    // The streams of this classifier's batch contexts, created HERE, back to back, when the classifier is created: N_STREAM_SETS
    // sets of {compute, upload, lane 1, lane 2}.  The HIP runtime deals a process's streams onto a few hardware queues (four by
    // default) in creation order, and streams that share a queue run one behind the other; created lazily per context (round 3),
    // whether context B's upload stream shared a queue with context A's compute stream depended on every stream the process had
    // ever created -- the files leg ran 90-99 k segments/s at the end of the bench process and 106-112 k in a process of its own.
    // With whole sets of four created in one go, stream j of every set lands on queue (j + const) mod 4: uploads only ever share a
    // queue with other uploads, whatever the process did before.  A context takes a free set at create and hands it back at
    // destroy (parked contexts keep theirs); with all sets taken it creates streams of its own, as before.
    static constexpr int N_STREAM_SETS = 4;
    struct StreamSet { hipStream_t s[4] = {nullptr, nullptr, nullptr, nullptr}; bool used = false; };
    StreamSet stream_sets[N_STREAM_SETS];
    std::mutex stream_mu;
    static constexpr int N_PARKED = 3;
    bh_batch_context *parked_ctx[N_PARKED] = {nullptr, nullptr, nullptr};
    std::mutex parked_mu;
};

// The gather workers of a batch context (host-fed entry points: pageable slices -> pinned staging).  Created on first need and kept:
// eight thread starts per call were 0.18 ms of a 2-ms call of 64 segments.  One job at a time (a context serves one call at a time);
// start() hands fn(t), t = 1 .. n - 1, to the workers and returns, wait() returns when all of them are done.
struct GatherPool {
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::vector<std::thread> threads;
    std::function<void(unsigned)> job;
    unsigned active = 0, pending = 0;     // workers taking part in the current job / still running it
    uint64_t epoch = 0;
    bool quit = false;
    void start(unsigned n_workers, std::function<void(unsigned)> fn) {
        std::unique_lock<std::mutex> l(mu);
        while (threads.size() < n_workers) {
            const unsigned t = (unsigned)threads.size() + 1;
            threads.emplace_back([this, t] { loop(t); });
        }
        job = std::move(fn);
        active = pending = n_workers;
        epoch++;
        cv_work.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> l(mu);
        cv_done.wait(l, [this] { return pending == 0; });
        job = nullptr;
    }
    void loop(unsigned t) {
        uint64_t seen = 0;
        for (;;) {
            std::function<void(unsigned)> fn;
            {
                std::unique_lock<std::mutex> l(mu);
                cv_work.wait(l, [&] { return quit || (epoch != seen && t <= active); });
                if (quit) return;
                seen = epoch;
                fn = job;
            }
            if (fn) fn(t);
            std::unique_lock<std::mutex> l(mu);
            if (--pending == 0) cv_done.notify_all();
        }
    }
    ~GatherPool() {
        { std::unique_lock<std::mutex> l(mu); quit = true; cv_work.notify_all(); }
        for (auto &th : threads) th.join();
    }
};

struct bh_batch_context {
    ~bh_batch_context();                     // (api.hip) frees the buffers, hands the stream set back; of a half-built context too
    bh_classifier *c = nullptr;
    std::unique_ptr<GatherPool> pool;        // (created by the first host-fed call that wants workers)
    size_t max_batch = 0;        // what the buffers hold
    size_t asked_batch = 0;      // what bh_batch_context_create was asked for (a parked context of up to twice that may serve it): the
                                 // capacity the entry points enforce
    bool keep_tensors = false;
    bool keep_fused = false;   // BIRDA_HIP_KEEP_FUSED=1: a debug context still runs the fused blocks (their outputs are readable)
    int stream_set = -1;                     // index into the classifier's stream_sets, or -1: the streams are this context's own
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;       // H2D of host batches, ahead of the compute stream
    std::vector<hipEvent_t> copy_ev;         // one per sub-slice in flight
    std::vector<hipEvent_t> done_ev;         // bh_predict_pcm*: a sub-slice's rows are in the pinned result buffers
    // Two compute lanes for the sub-slices of a host-fed slice (lanes_begin below): sub-slice k runs on stream (k & 1 ? stream2 :
    // stream) in its own part of the arena, so the launch chain of one sub-slice (21 dependent launches: ~0.85 ms however few
    // segments it holds) runs under the other's kernels instead of after them.
    static constexpr int MAX_LANES = 4;
    hipStream_t lane_stream[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};   // [0] = stream
    hipEvent_t fork_ev = nullptr, join_ev[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    int n_lanes = 3;
    int lanes_in_use = 1;        // of the slice being enqueued
    struct ArenaPlan { std::vector<size_t> t_off; size_t total = 0; };
    std::map<size_t, ArenaPlan> plans;       // arena plan of an n-segment forward (n < max_batch), built on first use
    size_t arena_cap = 0;                    // floats allocated (arena_floats + slack for the lanes' alignment losses)
    uint64_t lane_fallbacks = 0;             // slices whose sub-slice plans did not fit the arena side by side and ran on one stream
    uint32_t forced_sub_slices = 0;          // bh_batch_context_set_sub_slices: 0 automatic, 1 whole slices, n equal sub-slices
    float *d_input = nullptr;    // [max_batch][sample_count]
    float *d_minmax = nullptr;   // [max_batch][8][2]
    unsigned *d_inbad = nullptr; // [max_batch][8]: the slice of the segment holds an inf / NaN sample
    float *d_arena = nullptr;
    size_t arena_floats = 0;
    std::vector<size_t> t_off;   // per tensor offset (floats) into the arena
    float *d_logits = nullptr;   // [max_batch][n_classes]
    int32_t *d_topk_idx = nullptr;
    float *d_topk_conf = nullptr;
    float *h_input = nullptr;    // pinned staging
    int16_t *d_pcm = nullptr;    // bh_predict_pcm16: the slice's span of the decoded stream (grow-only)
    size_t pcm_cap = 0;          // bytes
    unsigned long long *d_starts = nullptr;
    float *d_partial = nullptr;              // BH_FLAG_LOW_LATENCY: the channel-split blocks' partial project sums (allocated on first use)
    size_t starts_cap = 0;       // entries
    float *d_raw = nullptr;      // source-rate segments awaiting the resampler [max_batch][raw_len]
    float *h_raw = nullptr;
    size_t raw_len = 0;
    int32_t *h_topk_idx = nullptr;
    float *h_topk_conf = nullptr;
    unsigned *d_nonfinite = nullptr;   // segments whose logits came out inf / NaN from finite samples (top-k kernel), since the last check
    unsigned *h_nonfinite = nullptr;   // pinned
    // bh_forward_device calls (with top-k buffers) since the last bh_batch_context_synchronize: what BH_FLAG_AUTO re-runs from
    struct Pending { const float *d_seg; size_t n; float *d_logits; int32_t *d_idx; float *d_conf; };
    std::vector<Pending> pending;
    static constexpr size_t MAX_PENDING = 256;   // a full list is settled by bh_forward_device itself (api.hip settle_pending)
    size_t device_bytes = 0;
    size_t last_n = 0;
    const float *last_logits = nullptr;
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_stage;
    std::vector<int> ev_layer;   // layer index of the launch an event closes (-1: front-end / top-k)
    float stage_ms[BH_N_STAGES] = {0};
    uint32_t stage_launches[BH_N_STAGES] = {0};
};

// api_custom.hip: a dense stack on embeddings (custom classifier) or on (latitude, longitude, week) (the geomodel)
struct bh_custom_classifier {
    ~bh_custom_classifier();
    bh::CustomModel model;
    int device = -1;              // (-1: create has not reached the device yet)
    uint32_t top_k = 0;
    std::vector<std::string> labels;
    float *d_blob = nullptr;
    std::vector<float *> d_w;     // per layer: W with rows padded to a multiple of 4 (or a pointer into d_blob)
    std::vector<int> ldw;
    std::vector<float *> d_owned; // every upload_owned buffer, the blob included
    // scratch, grown on demand: activations of the two widest layers, logits, top-k rows, host copies
    float *d_act[2] = {nullptr, nullptr};
    float *d_in = nullptr;
    int32_t *d_idx = nullptr;
    float *d_conf = nullptr;
    size_t cap_rows = 0;
    uint32_t max_width = 0;
    uint32_t k0 = 0;              // input width padded to a multiple of 4 (the GEMM's k step): rows of d_in have this stride
    hipStream_t stream = nullptr;
    std::mutex mu;
};

// host_pipeline.cpp: memcpy into pinned staging memory with non-temporal stores (what the DMA engine, not a core, reads next)
extern "C" void bh_internal_stream_copy(void *dst, const void *src, size_t bytes);

namespace bhi {

// api_plan.hip
uint16_t f32_to_f16(float f);
float f16_to_f32(uint16_t h);
std::vector<float> build_gf(const bh::BranchRec &b, const float *W, int nm_pad, int prec, int *scale_exp);
std::vector<Step> build_schedule(const bh_classifier &c, bool fused, bool chains);
void plan_arena(const bh::Model &m, const std::vector<Step> &sched, size_t max_batch, bool keep, std::vector<size_t> &off, size_t &total,
                std::vector<size_t> *sizes = nullptr);
bool gap_gate_chain(const bh::Model &m, size_t i);
int concat_chain_len(const bh::Model &m, size_t i);
// the last layer of the fused block d planned at layer i: its project convolution, which in a squeeze-excite block comes four
// layers later (pool, 1x1, 1x1, scale: SeInfo::iP)
inline size_t fused_block_last(size_t i, const bh::MbDesc &d) { return i + (d.noexp ? 1 : 2) + (d.se ? 4 : 0); }
bool describe_fused_block(const bh::Model &m, const std::vector<int> &readers, size_t i, int precision, int force_cfg, bh::MbDesc &d);
std::vector<int> tensor_readers(const bh::Model &m);
// a planned fused block's weights in the kernel's layouts (host vectors; bp empty when spa == 0: the layer's own biases serve)
struct MbHostWeights { std::vector<float> we, wp, wd, bp; int spa = 0; };
void mb_prepare_weights(bh::MbDesc &d, const float *We, const float *be, const float *Wd, const float *bd, const float *Wp, const float *bp,
                        MbHostWeights &out);
// the GEMM layers' weights in their kernels' layouts (host vectors): create uploads them, the diagnostics of api_debug.hip too
std::vector<uint16_t> w16_planes(const float *W, int K, int N, float *unscale, bool *lo_zero = nullptr);
std::vector<uint16_t> w16_compact(const std::vector<uint16_t> &planes);
std::vector<float> conv_gemm_rows(const float *W, const bh::ConvParams &p, int ld);
std::vector<float> gconv_matrix(const float *W, const bh::ConvParams &p, int G, int *K_out);
std::vector<float> gconv_fragments(const std::vector<float> &wt, int K, int nt);
std::vector<float> pw_gemm_rows(const float *W, size_t K, size_t N, size_t ld);
int plan_fusion(bh_classifier *c);
// api.hip
constexpr uint32_t FLAG_INTERNAL_NO_ENV = 0x80000000u;   // (the fallback classifier: BIRDA_HIP_PRECISION must not turn it into f16 again)
bool res_act_after(const bh::LayerRec &L);
bh::ConvParams conv_params(const bh::LayerRec &L);
std::array<bh::ConcatSource, 2> concat_sources(const bh::Model &m, const bh::LayerRec &L, const float *a, const float *b);
bool load_any_model(const char *path, bh::Model &m, std::string &err);
int model_load_status(const std::string &err);
inline void ctx_destroy(bh_batch_context *ctx) { delete ctx; }
int se_gate_form(int C, int Cr);
int mb_ksplit_of(const bh::MbDesc &d);
int resample_ranges(const char *who, size_t src_len, size_t out_len, size_t n_seg);
// a kernel's name (null: none) into out / cap, written only where it fits with its terminator; returns its length
inline int copy_name(const char *name, char *out, size_t cap) {
    const size_t n = name ? strlen(name) : 0;
    if (out && cap > n) { if (n) memcpy(out, name, n); out[n] = 0; }
    return (int)n;
}
int read_labels(const char *path, std::vector<std::string> &out);
int check_ctx(bh_classifier *c, bh_batch_context *ctx);
int predict_slices(bh_classifier *c, bh_batch_context *ctx, const float *const *segments, const float *contig,
                   size_t n, bh_result *out, float *logits_out, float *emb_out, bool whole_slice = false);
// api_custom.hip: host rows into the stack's input buffer; the stack (+ activation / top-k when out is given) on device rows.
// last_gemm (nullable) receives the name of the last GEMM launched
int cc_upload_rows(bh_custom_classifier *cc, const float *rows, size_t n);
int cc_run(bh_custom_classifier *cc, const float *d_emb, size_t in_stride, size_t n, hipStream_t s, bh_result *out, float *logits_out,
           const char **last_gemm = nullptr);

}  // namespace bhi
