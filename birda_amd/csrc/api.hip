// libbirda_hip.so -- C ABI (include/birda_hip.h) and the host executor for the gfx950 hot path.
//
// Plays the role of birdnet_onnx::Classifier + ONNX Runtime in the reference
// (src/inference/classifier.rs:191-646): owns the model, the device weights, the batch
// contexts and the per-layer kernel schedule.  No CPU compute path exists here: every
// numeric result comes from the kernels in kernels_frontend.hip / kernels_conv.hip.
#include "api_internal.hpp"
#include <unistd.h>
#include <cerrno>

namespace bhi {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    // A failed runtime call leaves its code in the thread's last-error slot, and the NEXT forward's launch check (hipGetLastError() at the
    // end of forward_slice) would report it as its own: a recording whose header asks for more device memory than there is made the
    // following, innocent file fail with "out of memory" (round 6, tools/fuzz_wav_decoder.py).  Reading the slot clears it; an
    // error that is really sticky (a dead context) comes back by itself.
    if (code == BH_ERR_HIP) (void)hipGetLastError();
    return code;
}

// Called from the catch (...) of every extern "C" entry point: no C++ exception (bad_alloc from a vector sized by the
// caller, system_error from std::thread) may cross the C ABI.
int on_exception() noexcept {
    try { throw; }
    catch (const std::bad_alloc &) { return fail(BH_ERR_INTERNAL, "out of host memory"); }
    catch (const std::exception &e) { return fail(BH_ERR_INTERNAL, "internal error: %s", e.what()); }
    catch (...) { return fail(BH_ERR_INTERNAL, "internal error (unknown exception)"); }
}

}  // namespace bhi

using namespace bhi;

namespace bhi {

// the layer applies its activation AFTER the residual add (model.hpp RES_ACT_AFTER; `reserved` is the pool mode on OP_POOL)
bool res_act_after(const bh::LayerRec &L) {
    return (L.op == bh::OP_CONV || L.op == bh::OP_PWCONV || L.op == bh::OP_DENSE) && L.reserved == bh::RES_ACT_AFTER;
}

bh::ConvParams conv_params(const bh::LayerRec &L) {
    return bh::ConvParams{(int)L.in_h, (int)L.in_w, (int)L.out_h, (int)L.out_w, (int)L.cin, (int)L.cout, (int)L.kh, (int)L.kw,
                          (int)L.sh, (int)L.sw, (int)L.pad_t, (int)L.pad_l, (int)L.in_layout, (int)L.act, res_act_after(L) ? 1 : 0,
                          (int)L.skip_h + 1, (int)L.skip_w + 1};   // (the record holds dilation - 1: model.hpp)
}

// The sources of an OP_CONCAT record as launch_concat takes them (model.hpp: w_off / b_off are channel offsets there, res_tensor a
// second input).  validate_model has held the windows to their tensors.
std::array<bh::ConcatSource, 2> concat_sources(const bh::Model &m, const bh::LayerRec &L, const float *a, const float *b) {
    const uint64_t img = (uint64_t)L.in_h * L.in_w;
    std::array<bh::ConcatSource, 2> src{};
    src[0] = bh::ConcatSource{a, (int)(m.tensor_floats[L.in_tensor] / img / 4), (int)L.w_off, (int)L.cin};
    if (L.res_tensor != bh::NO_TENSOR)
        src[1] = bh::ConcatSource{b, (int)(m.tensor_floats[L.res_tensor] / img / 4), (int)L.b_off, (int)(L.cout - L.cin)};
    return src;
}

// Which of its three forms the gate of a fused squeeze-excite block of C expanded and Cr hidden channels takes -- its widths alone
// decide, never the launch: 1 = the two sixteen-segment launches (launch_se_gate16) from BH_SE_GATE16_MIN channels where they
// support the shape, 2 = the pool and two GEMMs (launch_se_gate_gemm) for the other widths beyond 576, 0 = the one-launch kernel
// (launch_se_gate).  -1: no form takes it (plan_fusion keeps such a block layer by layer).  SliceRun::fused_se and bh_debug_se_gate
// both ask here.
int se_gate_form(int C, int Cr) {
    if (C >= BH_SE_GATE16_MIN && bh::se_gate16_supports(C, Cr)) return 1;
    if (C > 576) return 2;
    return bh::se_gate_supports(C, Cr) ? 0 : -1;
}

int read_labels(const char *path, std::vector<std::string> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return fail(BH_ERR_IO, "cannot open labels file %s", path);
    std::string cur;
    int ch;
    bool any = false;
    while ((ch = fgetc(f)) != EOF) {
        any = true;
        if (ch == '\n') {
            if (!cur.empty() && cur.back() == '\r') cur.pop_back();
            out.push_back(cur);
            cur.clear();
        } else cur.push_back((char)ch);
    }
    if (any && !cur.empty()) {
        if (cur.back() == '\r') cur.pop_back();
        out.push_back(cur);
    }
    fclose(f);
    if (!out.empty() && out[0].size() >= 3 && (unsigned char)out[0][0] == 0xEF && (unsigned char)out[0][1] == 0xBB &&
        (unsigned char)out[0][2] == 0xBF)
        out[0] = out[0].substr(3);
    return BH_OK;
}
void ctx_mark(bh_batch_context *ctx, int stage, int layer = -1) {
    if (!ctx->profiling) return;
    hipEvent_t e;
    // timing-only events: without the system-scope fence (an L2 write-back + invalidate between every two kernels, which the
    // un-profiled pipeline never sees)
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return;
    (void)hipEventRecord(e, ctx->stream);
    ctx->ev.push_back(e);
    ctx->ev_stage.push_back(stage);
    ctx->ev_layer.push_back(layer);
}
// the schedule a context's forwards walk and its arena is planned from
const std::vector<Step> &schedule_of(const bh_batch_context *ctx) {
    return !ctx->keep_tensors ? ctx->c->sched : ctx->keep_fused ? ctx->c->sched_keep_fused : ctx->c->sched_layers;
}
// (whatever fails below, ~bh_batch_context releases what the context has taken so far, the stream set included)
int ctx_create(bh_classifier *c, size_t max_batch, bool keep, bh_batch_context **out) {
    if (!c || !out || max_batch == 0) return fail(BH_ERR_INVALID, "batch context: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    auto ctx = std::make_unique<bh_batch_context>();
    ctx->c = c;
    ctx->max_batch = max_batch;
    ctx->asked_batch = max_batch;
    ctx->keep_tensors = keep;
    if (const char *kf = getenv("BIRDA_HIP_KEEP_FUSED")) ctx->keep_fused = kf[0] == '1';
    const auto &m = c->model;
    {   // a stream set of the classifier (api_internal.hpp: created at classifier create, a fixed stream -> hardware-queue pattern)
        std::lock_guard<std::mutex> g(c->stream_mu);
        for (int k = 0; k < bh_classifier::N_STREAM_SETS && ctx->stream_set < 0; k++)
            if (!c->stream_sets[k].used && c->stream_sets[k].s[0]) { c->stream_sets[k].used = true; ctx->stream_set = k; }
    }
    if (ctx->stream_set >= 0) {
        const auto &ss = c->stream_sets[ctx->stream_set];
        ctx->stream = ss.s[0]; ctx->copy_stream = ss.s[1]; ctx->lane_stream[1] = ss.s[2]; ctx->lane_stream[2] = ss.s[3];
        for (int l = 1; l <= 2; l++) HIPCHK(hipEventCreateWithFlags(&ctx->join_ev[l], hipEventDisableTiming));
    } else {
        HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    }
    const size_t in_bytes = max_batch * (size_t)m.h.sample_count * sizeof(float);
    HIPCHK(hipMalloc((void **)&ctx->d_input, in_bytes));
    HIPCHK(hipMalloc((void **)&ctx->d_minmax, max_batch * 16 * sizeof(float)));
    HIPCHK(hipMalloc((void **)&ctx->d_inbad, max_batch * 8 * sizeof(unsigned)));
    plan_arena(m, schedule_of(ctx.get()), max_batch, keep, ctx->t_off, ctx->arena_floats);
    // (slack for the lanes: the plans of a slice's sub-slices, side by side, exceed the whole slice's plan by up to 64 floats of
    //  alignment per tensor and sub-plan; the automatic split makes up to 9 sub-slices, bh_batch_context_set_sub_slices more --
    //  16 sub-plans fit, beyond that lanes_begin falls back to one stream and counts it: bh_batch_context_lane_fallbacks)
    ctx->arena_cap = ctx->arena_floats + 16 * 64 * (m.layers.size() + 1);
    HIPCHK(hipMalloc((void **)&ctx->d_arena, ctx->arena_cap * sizeof(float)));
    ctx->lane_stream[0] = ctx->stream;   // (the other lanes' streams are created when a slice first needs them: lanes_begin)
    HIPCHK(hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming));
    HIPCHK(hipMalloc((void **)&ctx->d_logits, max_batch * (size_t)m.h.n_classes * sizeof(float)));
    HIPCHK(hipMalloc((void **)&ctx->d_topk_idx, max_batch * c->top_k * sizeof(int32_t)));
    HIPCHK(hipMalloc((void **)&ctx->d_topk_conf, max_batch * c->top_k * sizeof(float)));
    HIPCHK(hipHostMalloc((void **)&ctx->h_input, in_bytes, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&ctx->h_topk_idx, max_batch * c->top_k * sizeof(int32_t), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&ctx->h_topk_conf, max_batch * c->top_k * sizeof(float), hipHostMallocDefault));
    HIPCHK(hipMalloc((void **)&ctx->d_nonfinite, sizeof(unsigned)));
    HIPCHK(hipMemset(ctx->d_nonfinite, 0, sizeof(unsigned)));
    HIPCHK(hipHostMalloc((void **)&ctx->h_nonfinite, sizeof(unsigned), hipHostMallocDefault));
    *ctx->h_nonfinite = 0;
    ctx->device_bytes = in_bytes + max_batch * 16 * sizeof(float) + ctx->arena_floats * sizeof(float) +
                        max_batch * (size_t)m.h.n_classes * sizeof(float) + max_batch * c->top_k * 8;
    *out = ctx.release();
    return BH_OK;
}

// where a sub-slice of a host-fed slice runs: its stream, its own part of the arena with the plan of an n-segment forward, and its
// first segment's index within the slice, which places its rows of the per-segment scratch
struct SliceLane { hipStream_t s; float *arena; const size_t *t_off; size_t seg0; };
// BH_FLAG_LOW_LATENCY: launches of up to this many segments split a late block's expanded channels over workgroups, 2 deep from 6
// chunks, 4 deep from 12, 8 deep from 32 (fused blocks without a gate: pass A of a squeeze-excite block has no project sums to split)
constexpr size_t kLowLatencyMaxSegments = 32;
int mb_ksplit_of(const bh::MbDesc &d) {
    return (d.se || d.Cout % 4) ? 1 : d.nchunks >= 32 ? 8 : d.nchunks >= 12 ? 4 : d.nchunks >= 6 ? 2 : 1;
}
// What the steps of one slice share.  T(t): where tensor t of a step's lists lives -- its planned bytes of the arena, and for the
// last layer's output the caller's logits buffer.
struct SliceRun {
    bh_classifier *c; bh_batch_context *ctx; size_t n; hipStream_t s; float *arena; const size_t *t_off; float *d_logits; bool in_lane;
    float *T(uint32_t t) const { return t == c->model.layers.size() ? d_logits : arena + t_off[t]; }
    const float *in(const Step &st) const { return T(st.reads[0]); }
    const float *res(const Step &st) const { return st.reads.size() > 1 ? T(st.reads[1]) : nullptr; }
    float *out(const Step &st) const { return T(st.writes[0]); }
    int layer(const Step &st) const, fused(const Step &st) const, fused_se(const Step &st) const, head_gap(const Step &st) const,
        se_gate(const Step &st) const, concat(const Step &st) const;       // one per path
};
// the fused block of a step as this launch runs it
// (a launch of at most 256 segments: the one-segment-per-workgroup twin where the block has one -- the two-segment tiles would leave
//  half of the CUs, or more, without a workgroup)
// (a launch of a few dozen segments: the narrow-tile twin -- two or four workgroups per image -- while those still number no more
//  than two per CU: what such a launch lasts is one workgroup's walk through the chunks)
static bh::MbDesc mb_for_launch(const bh_classifier *c, int block, size_t n) {
    const bh::MbDesc &twin = c->mb_small[block], &narrow = c->mb_narrow[block];
    return (narrow.cfg >= 0 && n * (size_t)narrow.tiles_x <= (size_t)c->narrow_max_workgroups) ? narrow
         : (twin.cfg >= 0 && n <= (size_t)c->twin_max_segments) ? twin : c->mb[block];
}

// one layer, one launch
int SliceRun::layer(const Step &st) const {
    const uint32_t i = st.first;
    const auto &L = c->model.layers[i];
    LayerState &S = c->layer[i];
    const float *in = this->in(st), *res = this->res(st), *bias = c->d_blob + L.b_off;
    float *out = this->out(st);
    // on its f16 planes, where it has them; a context that keeps every tensor runs every layer on the f32 kernels
    const bool f16 = !ctx->keep_tensors && S.planes;
    // (a layer with its activation after the residual add is a layer like any other: the position rides in p / after, the f32
    //  kernels branch on it at run time -- BIRDA_HIP_KEEP_TENSORS contexts and the BH_FLAG_AUTO re-run land there -- and the
    //  split-f16 launchers pick the AFTER instantiations)
    const bh::ConvParams p = conv_params(L);
    const int after = p.res_after;
    const char *launched = "";      // what a GEMM launcher reports; null: it launched nothing (no such instantiation)
    switch (L.op) {
    case bh::OP_CONV:
        // the NCHW stem on the direct kernel (when it is not fused into the first block); every NHWC full convolution is an
        // implicit GEMM on the MFMA (kernels_conv.hip), split-f16 where it has planes
        if (L.in_layout == 1)
            launched = bh::launch_conv_direct(in, S.w, bias, out, p, (int)n, s);
        else if (f16)
            launched = bh::launch_conv_gemm16(in, S.planes, bias, res, out, p, (int)n, S.terms, S.unscale, s);
        else
            launched = bh::launch_conv_gemm(in, S.w, bias, res, out, p, (int)n, S.ldw, s);
        ctx_mark(ctx, ST_STEM, (int)i);
        break;
    case bh::OP_DWCONV:
        launched = bh::launch_dwconv(in, S.w, bias, out, p, (int)n, s);
        ctx_mark(ctx, ST_DW, (int)i);
        break;
    case bh::OP_PWCONV: case bh::OP_DENSE: {   // a 1x1 convolution is the dense layer over every pixel's row
        const int rows = (int)(L.op == bh::OP_PWCONV ? n * L.out_h * L.out_w : n);
        if (f16)
            launched = bh::launch_pw_gemm16(in, S.planes, bias, res, out, rows, (int)L.cin, (int)L.cout, (int)L.act, S.terms, S.unscale, s, after);
        else
            launched = bh::launch_pw_gemm(in, S.w, bias, res, out, rows, (int)L.cin, (int)L.cout, S.ldw, (int)L.act, s, after);
        ctx_mark(ctx, L.op == bh::OP_PWCONV ? ST_PW : ST_DENSE, (int)i);
        break;
    }
    case bh::OP_GAP:
        bh::launch_gap(in, out, (int)n, (int)(L.in_h * L.in_w), (int)L.cout, s);
        ctx_mark(ctx, ST_GAP, (int)i);
        break;
    case bh::OP_SCALE:   // squeeze-excite: the feature map times its [n][C] gate (res = the gate tensor)
        bh::launch_scale(in, res, out, (int)n, (int)(L.out_h * L.out_w), (int)L.cout, s);
        ctx_mark(ctx, ST_DW, (int)i);
        break;
    case bh::OP_GCONV:   // a grouped convolution (L.reserved: the group count): per-tile weight blocks, split-f16 where it has planes
        launched = f16 ? bh::launch_gconv16(in, S.planes, bias, out, p, (int)L.reserved, (int)n, S.terms, S.unscale, s)
                       : bh::launch_gconv(in, S.w, bias, out, p, (int)L.reserved, (int)n, s);
        ctx_mark(ctx, ST_STEM, (int)i);
        break;
    case bh::OP_POOL:    // MaxPool / AveragePool: f32 in every precision mode (L.reserved: the pool mode)
        bh::launch_pool(in, out, p, (int)L.reserved, (int)n, s);
        ctx_mark(ctx, ST_GAP, (int)i);
        break;
    case bh::OP_CONCAT: {   // channel windows of one or two tensors, optionally shuffled: a copy, the same in every precision mode
        const auto src = concat_sources(c->model, L, in, res);   // (res: the second input, not a residual)
        launched = bh::launch_concat(src.data(), L.res_tensor == bh::NO_TENSOR ? 1 : 2, out, (int)L.out_h, (int)L.out_w, (int)L.reserved, (int)n, s);
        ctx_mark(ctx, ST_GAP, (int)i);
        break;
    }
    case bh::OP_LNORM: {   // LayerNorm over the channels, pixel by pixel: f32 in every precision mode (L.reserved: the bits of eps)
        float eps;
        memcpy(&eps, &L.reserved, sizeof eps);
        launched = bh::launch_lnorm(in, c->d_blob + L.w_off, bias, out, (unsigned long long)n * L.out_h * L.out_w, (int)L.cout, eps, s);
        ctx_mark(ctx, ST_GAP, (int)i);
        break;
    }
    case bh::OP_REDUCE:   // max / mean / max + mean over H, W or both: f32 in every precision mode (L.reserved: the mode)
        launched = bh::launch_reduce(in, out, p, (int)L.reserved, (int)n, s);
        ctx_mark(ctx, ST_GAP, (int)i);
        break;
    case bh::OP_BNACT:    // a folded BatchNormalization + activation: f32 in every precision mode (w_off: scale[C], b_off: shift[C])
        launched = bh::launch_bnact(in, c->d_blob + L.w_off, bias, out, (unsigned long long)n * L.out_h * L.out_w, (int)L.cout, (int)L.act, s);
        ctx_mark(ctx, ST_GAP, (int)i);
        break;
    default: return fail(BH_ERR_UNSUPPORTED, "layer %u: unsupported op %u", i, L.op);
    }
    // (bh_debug_layer_kernel: the split-f16 launchers' names; a grouped convolution's and a concat's f32 kernels are kept too)
    // (... and a dilated depthwise layer's, the dilated form of dwconv_kernel)
    // (... and a 7x7 depthwise layer's and a LayerNorm's: the layers of a ConvNeXt block)
    // (... and a reduce layer's: the split is part of the name)
    // (... and a norm + activation layer's)
    if (f16 || L.op == bh::OP_GCONV || L.op == bh::OP_CONCAT || L.op == bh::OP_LNORM || L.op == bh::OP_REDUCE || L.op == bh::OP_BNACT || (L.op == bh::OP_DWCONV && (bh::conv_dilated(p) || L.kh == 7)))
        S.kernel.store(launched, std::memory_order_relaxed);
    // (create's predicates and validate_model keep this from happening; if it does, the output tensor was not written)
    if (!launched && n) {
        if (L.op == bh::OP_LNORM) return fail(BH_ERR_INTERNAL, "layer %u: no kernel instantiation for a layer norm over %u channels", i, L.cout);
        if (L.op == bh::OP_REDUCE) return fail(BH_ERR_INTERNAL, "layer %u: no kernel instantiation for a reduce of mode %u over a %ux%u window", i, L.reserved, L.kh, L.kw);
        if (L.op == bh::OP_BNACT) return fail(BH_ERR_INTERNAL, "layer %u: no kernel instantiation for a norm + activation layer over %u channels with activation %u", i, L.cout, L.act);
        if (L.op == bh::OP_DWCONV || (L.op == bh::OP_CONV && L.in_layout == 1))
            return fail(BH_ERR_INTERNAL, "layer %u: no kernel instantiation for a %ux%u stride %ux%u window, %u -> %u channels", i, L.kh, L.kw, L.sh, L.sw, L.cin, L.cout);
        return fail(BH_ERR_INTERNAL, "layer %u: no kernel instantiation for activation %u %s the residual add", i, L.act, after ? "after" : "before");
    }
    return BH_OK;
}

// expand -> depthwise -> project (depthwise -> project for a block without an expand convolution) in one launch
int SliceRun::fused(const Step &st) const {
    bh::MbDesc d = mb_for_launch(c, st.block, n);
    d.X = in(st);
    d.Y = out(st);
    d.R = res(st);
    // BH_FLAG_LOW_LATENCY, a launch of at most 32 segments on the context's own stream: a block of many chunks runs 2 or 4
    // workgroups deep, each walking its share of the expanded channels (kernels.hpp MbDesc::ksplit) -- a handful of
    // workgroups on the whole chip each streaming ALL of a late block's weights is what such a forward lasts.  The depth is
    // the block's alone (never the launch's), so within the regime a segment's bits still do not depend on its launch.
    const int ksp = (c->low_latency && !in_lane && n <= kLowLatencyMaxSegments) ? mb_ksplit_of(d) : 1;
    if (ksp > 1) {
        if (!ctx->d_partial) {
            size_t need = 0;
            for (const auto &b : c->mb) need = std::max(need, (size_t)mb_ksplit_of(b) * kLowLatencyMaxSegments * b.Ho * b.Wo * b.Cout);
            HIPCHK(hipMalloc((void **)&ctx->d_partial, std::max<size_t>(need, 4) * sizeof(float)));
        }
        d.ksplit = ksp;
        d.partial = ctx->d_partial;
        bh::launch_mbconv(d, (int)n, s);
        bh::launch_mb_reduce_partials(ctx->d_partial, d.Y, ksp, n * (size_t)d.Ho * d.Wo * d.Cout, d.prec != 0 ? d.p_unscale : 1.0f, s);
    } else
    bh::launch_mbconv(d, (int)n, s);
    ctx_mark(ctx, ST_MBCONV, (int)st.first);
    return BH_OK;
}

// A squeeze-excite block in three launches: pass A (expand -> depthwise: D and the per-tile channel sums), the gate
// (pool -> 1x1 -> 1x1), the project GEMM on D x gate (+ residual).  The expanded tensor stays in LDS, the scaled one
// never exists; D crosses HBM once each way.
int SliceRun::fused_se(const Step &st) const {
    const bh::MbDesc d = mb_for_launch(c, st.block, n);
    const auto &S = c->se[st.block];
    const auto &G1 = c->model.layers[S.iPw1], &G2 = c->model.layers[S.iPw2], &LP = c->model.layers[S.iP];
    const LayerState &W1 = c->layer[S.iPw1], &W2 = c->layer[S.iPw2];
    LayerState &WP = c->layer[S.iP];
    // (the gate: one launch, a workgroup per segment (se_gate_kernel), or the pool + the two dense layers as GEMMs over all
    //  segments, through the arena slots of the layers they stand for.  Either way every sum runs in a fixed order.)
    // (which of the two a BLOCK takes depends on its width alone, never on the launch: up to 576 expanded channels the
    //  one-launch kernel is the faster one -- three launches cost ~27 us per 1 000 segments whatever their size, measured
    //  13-36 against 27-50 us; beyond, its per-segment re-read of both weight matrices is: 59-490 against 37-143 us)
    // (round 6: beyond 576 channels two launches of sixteen-segment workgroups -- the pooled rows x W1 split over channel
    //  slices, then hidden x W2 -- instead of pool + two GEMMs of a handful of tiles: kernels_conv.hip se_hidden_kernel)
    // (one selection for whole launches and for the groups below: a segment's bits do not depend on how its launch is cut)
    auto launch_gate = [&](const float *part, int tiles, int P, float *pooled, float *hidden, float *gate, size_t ns) {
        const int form = se_gate_form(d.Cexp, (int)G1.cout);
        if (form == 1)
            bh::launch_se_gate16(part, tiles, P, pooled, W1.w, c->d_blob + G1.b_off, W1.ldw, (int)G1.act,
                                 W2.w, c->d_blob + G2.b_off, W2.ldw, (int)G2.act, gate, (int)ns, d.Cexp, (int)G1.cout, s);
        else if (form == 2)
            bh::launch_se_gate_gemm(part, tiles, P, pooled, hidden, W1.w, c->d_blob + G1.b_off, W1.ldw, (int)G1.act,
                                    W2.w, c->d_blob + G2.b_off, W2.ldw, (int)G2.act, gate, (int)ns, d.Cexp, (int)G1.cout, s);
        else
            bh::launch_se_gate(part, tiles, P, W1.w, c->d_blob + G1.b_off, W1.ldw, (int)G1.act,
                               W2.w, c->d_blob + G2.b_off, W2.ldw, (int)G2.act, gate, (int)ns, d.Cexp, (int)G1.cout, s);
    };
    // (a block without an expand convolution computes D twice instead of keeping it: pass A leaves only the channel sums,
    //  the gated one-launch block below does the rest -- kernels.hpp MbDesc::gate)
    // (round 6: the same for the STEM block -- its input, the planar spectrogram, is a tenth of its D -- was built (the stem
    //  instantiations take MbDesc::gate) and measured on the Perch-sized plan: 38.75 -> 38.45 k segments/s, three alternations
    //  on one box at one clock, profiles/r6_n_stem_recompute.txt: the sums-only pass costs more than D's round trip saves.
    //  Not taken: the forward pass keeps a stem block's D.)
    const bool recompute = d.noexp != 0;
    // (D blocked for the f16 gated GEMMs: kernels.hpp MbDesc::dblk)
    const bool dblk = !recompute && WP.planes && bh::pw_gemm16_gated_wants_blocked(d.Cexp, d.Cout, d.Ho * d.Wo);
    // Round 6 (VERDICT r5 next #3a): a block whose D is large -- the early stages: 1.5-2.3 MB a segment -- runs its three
    // launches per GROUP of segments, so that the D pass A writes is still in the 256 MB Infinity Cache when the gated
    // project GEMM reads it (at 1 000 segments a launch it crosses HBM both ways).  The tiling -- hence every pooled sum's
    // order, hence the bits -- is the whole launch's; only the launches are cut.  c->se_group_bytes: the D one group may
    // hold (0: never); blocks whose whole D fits, and those that compute D twice, run as before.
    const size_t d_seg_bytes = (size_t)d.Ho * d.Wo * d.Cexp * sizeof(float);
    size_t grp = (!d.noexp && !d.stem && c->se_group_bytes && d_seg_bytes * n > c->se_group_bytes) ? std::max<size_t>(c->se_group_bytes / d_seg_bytes, 16) : n;
    if (grp < n) grp -= grp % (size_t)std::max(d.S, 1);     // (whole S-segment workgroups per group)
    const bool grouped = grp < n;     // (one ST_MBCONV mark for the block; a whole launch marks each of its three)
    const size_t P = (size_t)d.Ho * d.Wo, tiles = (size_t)d.tiles_x * d.tiles_y;
    const size_t in_seg = d.stem ? (size_t)d.stem_c * d.stem_h * d.stem_w : (size_t)d.H * d.W * d.Cin;
    const float *x = in(st), *r = res(st);
    float *y = out(st), *D = T(st.writes[1]), *sums = T(st.scratch[SE_SUMS].t);
    float *pooled = T(st.scratch[SE_POOLED].t), *hidden = T(st.scratch[SE_HIDDEN].t), *gate = T(st.scratch[SE_GATE].t);
    auto run = [&](size_t s0, size_t ng) {      // segments s0 .. s0 + ng - 1
        bh::MbDesc a = d;
        a.X = x + s0 * in_seg;
        a.Dout = recompute ? nullptr : D + s0 * P * d.Cexp;
        a.pool_part = sums + s0 * tiles * d.Cexp;
        a.gate = nullptr;
        a.dblk = dblk;
        bh::launch_mbconv(a, (int)ng, s);
        if (!grouped) ctx_mark(ctx, ST_MBCONV, (int)st.first);
        float *gg = gate + s0 * d.Cexp;
        launch_gate(a.pool_part, (int)tiles, (int)P, pooled + s0 * d.Cexp, hidden + s0 * G1.cout, gg, ng);
        if (!grouped) ctx_mark(ctx, ST_GAP, (int)S.iGap);
        float *yg = y + s0 * P * d.Cout;
        const float *rg = r ? r + s0 * P * d.Cout : nullptr;
        if (recompute) {      // depthwise -> x gate -> project (+ residual) in one launch, the block's own weights and tiling
            bh::MbDesc g = a;
            g.se = 0; g.gate = gg; g.Y = yg; g.R = rg; g.Dout = nullptr; g.pool_part = nullptr;
            bh::launch_mbconv(g, (int)ng, s);
        } else
        if (WP.planes)
            WP.kernel.store(bh::launch_pw_gemm16_gated(a.Dout, gg, (int)P, WP.planes, c->d_blob + LP.b_off, rg, yg, (int)(ng * P), d.Cexp, d.Cout,
                                                       WP.terms, WP.unscale, a.dblk, s), std::memory_order_relaxed);
        else
            bh::launch_pw_gemm_gated(a.Dout, gg, (int)P, WP.w, c->d_blob + LP.b_off, rg, yg, (int)(ng * P), d.Cexp, d.Cout, WP.ldw, (int)LP.act, s);
        if (!grouped) ctx_mark(ctx, ST_PW, (int)S.iP);
    };
    if (grouped) {
        for (size_t s0 = 0; s0 < n; s0 += grp) run(s0, std::min(grp, n - s0));
        ctx_mark(ctx, ST_MBCONV, (int)st.first);
    } else
        run(0, n);
    return BH_OK;
}

// head conv + GELU and the global average pool after it in one launch
int SliceRun::head_gap(const Step &st) const {
    const uint32_t i = st.first;
    const auto &L = c->model.layers[i];
    LayerState &S = c->layer[i];
    S.kernel.store(bh::launch_head_gap16(in(st), S.planes, c->d_blob + L.b_off, out(st), (int)n, (int)(L.out_h * L.out_w), (int)L.cin, (int)L.cout,
                                         (int)L.act, S.terms, S.unscale, s), std::memory_order_relaxed);
    ctx_mark(ctx, ST_PW, (int)i);
    return BH_OK;
}

// The gate of a squeeze-excite block that runs LAYER BY LAYER (wider than the fused entries -- the v3.0-sized model's
// 640 -> 3 840 -> 640 blocks -- or left there by the f32 planner): pool -> 1x1 -> 1x1 were a pool launch and two GEMMs of
// M = n rows, the first with a handful of tiles under a K loop of the whole width (171 us per 256 segments for 3 840 ->
// 160).  On a small image the two gate launches of the fused path take the whole chain: se_hidden_kernel pools the
// depthwise output itself (its "tiles" are the image's pixels, in order), the pool layer's own tensor holds the partial
// sums.  Which path a block takes depends on its shapes alone.
// (the chain's shapes are checked once, at create: gap_gate_chain.  A model that ENDS in such a gate gets it in d_logits.)
int SliceRun::se_gate(const Step &st) const {
    const uint32_t i = st.first;
    const auto &L = c->model.layers[i], &G1 = c->model.layers[i + 1], &G2 = c->model.layers[i + 2];
    const int P = (int)(L.in_h * L.in_w);
    const LayerState &W1 = c->layer[i + 1], &W2 = c->layer[i + 2];
    bh::launch_se_gate16(in(st), P, P, T(st.scratch[0].t), W1.w, c->d_blob + G1.b_off, W1.ldw, (int)G1.act, W2.w,
                         c->d_blob + G2.b_off, W2.ldw, (int)G2.act, out(st), (int)n, (int)L.cout, (int)G1.cout, s);
    ctx_mark(ctx, ST_GAP, (int)i);
    return BH_OK;
}

// a chain of concat records (an N-way Concat; concat_chain_len) as one launch: the leaves -- A of the first record, then every
// record's B, st.reads in that order -- gathered straight into the last record's tensor, with the last record's shuffle
int SliceRun::concat(const Step &st) const {
    const auto &m = c->model;
    const auto &F = m.layers[st.first], &Z = m.layers[st.last];
    const uint64_t img = (uint64_t)F.in_h * F.in_w;
    bh::ConcatSource src[4];
    int n_src = 0;
    auto leaf = [&](uint32_t t, uint64_t off, uint32_t len) {
        if (n_src < 4) src[n_src] = bh::ConcatSource{T(t), (int)(m.tensor_floats[t] / img / 4), (int)off, (int)len};
        n_src++;
    };
    leaf(F.in_tensor, F.w_off, F.cin);
    for (uint32_t j = st.first; j <= st.last; j++)
        if (m.layers[j].res_tensor != bh::NO_TENSOR) leaf(m.layers[j].res_tensor, m.layers[j].b_off, m.layers[j].cout - m.layers[j].cin);
    if (n_src > 4 || (size_t)n_src != st.reads.size()) return fail(BH_ERR_INTERNAL, "layer %u: a concat chain of %d leaves", st.first, n_src);
    const char *name = bh::launch_concat(src, n_src, out(st), (int)Z.out_h, (int)Z.out_w, (int)Z.reserved, (int)n, s);
    for (uint32_t j = st.first; j <= st.last; j++) c->layer[j].kernel.store(name, std::memory_order_relaxed);
    ctx_mark(ctx, ST_GAP, (int)st.first);
    return BH_OK;
}

// one slice (n <= max_batch) of the forward pass, enqueued on the lane's stream and arena (nullptr: the context's stream and whole
// arena): the front end, then the context's schedule step by step
int forward_slice(bh_classifier *c, bh_batch_context *ctx, const float *d_seg, size_t n, float *d_logits,
                  int32_t *d_idx, float *d_conf, const SliceLane *lane = nullptr) {
    const auto &m = c->model;
    const SliceRun r{c, ctx, n, lane ? lane->s : ctx->stream, lane ? lane->arena : ctx->d_arena, lane ? lane->t_off : ctx->t_off.data(),
                     d_logits, lane != nullptr};
    hipStream_t s = r.s;
    float *const d_minmax = ctx->d_minmax + (lane ? lane->seg0 * 16 : 0);
    unsigned *const d_inbad = ctx->d_inbad + (lane ? lane->seg0 * 8 : 0);
    bh::TraceRange tr_slice("bh_forward_slice");   // ROCTx ranges (BIRDA_HIP_ROCTX=1): the slice, its front end, every layer group
    ctx_mark(ctx, -1);
    {
        bh::TraceRange tr("front_end: minmax + mel");
        bh::launch_minmax(d_seg, d_minmax, d_inbad, (int)n, (int)m.h.sample_count, s);
        ctx_mark(ctx, ST_MINMAX);
        const char *mel_name = bh::launch_mel(d_seg, d_minmax, r.T(0), c->fe, c->d_fe, (int)n, s);
        if (!mel_name)   // (create refuses what launch_mel has no instantiation for: a missing kernel is an error, never a silent skip)
            return fail(BH_ERR_UNSUPPORTED, "front-end: no kernel instantiation for %d mels at precision %d", c->fe.br[0].n_mels, c->fe.prec);
        c->fe_kernel.store(mel_name, std::memory_order_relaxed);
        ctx_mark(ctx, ST_MEL);
    }
    for (const Step &st : schedule_of(ctx)) {
        static const char *const kOpNames[] = {"layer", "conv", "depthwise", "pointwise", "pool", "dense", "scale", "window_pool", "grouped_conv", "layer", "concat"};
        const uint32_t op = m.layers[st.first].op;
        bh::TraceRange tr(st.block >= 0 ? "fused_mbconv_block" : op < sizeof(kOpNames) / sizeof(kOpNames[0]) ? kOpNames[op] : kOpNames[0]);
        int rc = BH_OK;
        switch (st.path) {
        case BH_PATH_LAYER: rc = r.layer(st); break;
        case BH_PATH_FUSED: rc = r.fused(st); break;
        case BH_PATH_FUSED_SE: rc = r.fused_se(st); break;
        case BH_PATH_HEAD_GAP: rc = r.head_gap(st); break;
        case BH_PATH_SE_GATE: rc = r.se_gate(st); break;
        case BH_PATH_CONCAT: rc = r.concat(st); break;
        }
        if (rc != BH_OK) return rc;
    }
    if (d_idx && d_conf) {
        bh::TraceRange tr("topk");
        bh::launch_topk(d_logits, (int)n, (int)m.h.n_classes, (int)m.h.output_activation, (int)c->top_k,
                        c->min_conf, c->filter, d_idx, d_conf, d_inbad, ctx->d_nonfinite, s);
        ctx_mark(ctx, ST_TOPK);
    }
    HIPCHK(hipGetLastError());
    ctx->last_n = n;
    ctx->last_logits = d_logits;
    return BH_OK;
}

// The non-finite counter of the forwards enqueued so far: fetch_nonfinite() goes on the stream BEFORE the synchronise that
// ends a call, nonfinite_status() after it.  A hit is an error, not a silent NaN row: in the f16 operand modes an activation
// at or beyond 65 504 turns into inf inside bh_split2 / the f16 conversions (weights cannot: they are pre-scaled at create).
hipError_t fetch_nonfinite(bh_batch_context *ctx) {
    return hipMemcpyAsync(ctx->h_nonfinite, ctx->d_nonfinite, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream);
}
int nonfinite_status(bh_classifier *c, bh_batch_context *ctx) {
    const unsigned bad = *ctx->h_nonfinite;
    if (!bad) return BH_OK;
    *ctx->h_nonfinite = 0;
    (void)hipMemsetAsync(ctx->d_nonfinite, 0, sizeof(unsigned), ctx->stream);
    return fail(BH_ERR_NONFINITE, "%u segment(s) with finite samples produced inf / NaN logits%s", bad,
                c->precision != 0 ? ": an activation left the f16 operand range (|x| >= 65504); build the classifier with BH_FLAG_AUTO (the default: such rows are re-run in f32) or BH_FLAG_F32"
                                  : " (f32 overflow inside the network)");
}

void clear_nonfinite(bh_batch_context *ctx) {
    *ctx->h_nonfinite = 0;
    (void)hipMemsetAsync(ctx->d_nonfinite, 0, sizeof(unsigned), ctx->stream);
}

// ---- BH_FLAG_AUTO: the rows the split-f16 forward could not represent, again on the f32 kernels -----------------------------
int internal_ctx(bh_classifier *c, size_t n, bh_batch_context **out);

int fallback_classifier(bh_classifier *c, bh_classifier **out) {
    std::lock_guard<std::mutex> g(c->fb_mu);
    if (!c->fb) {
        bh_config cfg{};
        cfg.model_path = c->model_path.c_str();
        cfg.labels_path = nullptr;
        cfg.top_k = c->top_k; cfg.min_confidence = c->min_conf; cfg.device = c->device;
        cfg.flags = BH_FLAG_F32 | FLAG_INTERNAL_NO_ENV;
        const int rc = bh_classifier_create(&cfg, &c->fb);
        if (rc != BH_OK) { c->fb = nullptr; return rc; }
    }
    *out = c->fb;
    return BH_OK;
}

// Rows `bad` of one forward (inputs d_seg [.][sample_count], outputs as given; d_idx / d_conf / d_emb nullable) computed again by
// the f32 classifier and written over the split-f16 ones.  The caller has synchronised whatever produced those rows.  Top-k
// goes through the PRIMARY classifier's filters (range filter / species list / BSG: device tables of the same device).
int redo_rows_f32(bh_classifier *c, const float *d_seg, const std::vector<size_t> &bad, float *d_logits, int32_t *d_idx, float *d_conf,
                  float *d_emb) {
    if (bad.empty()) return BH_OK;
    bh_classifier *fb = nullptr;
    int rc = fallback_classifier(c, &fb);
    if (rc != BH_OK) return rc;
    std::lock_guard<std::mutex> g(fb->internal_mu);
    const auto &h = c->model.h;
    const size_t S = h.sample_count, NC = h.n_classes, TK = c->top_k, ED = h.embedding_dim;
    fb->filter = c->filter;
    fb->min_conf = c->min_conf;
    constexpr size_t CH = 64;
    bh_batch_context *fx = nullptr;
    rc = internal_ctx(fb, std::min(bad.size(), CH), &fx);
    if (rc != BH_OK) return rc;
    for (size_t q0 = 0; q0 < bad.size(); q0 += CH) {
        const size_t nq = std::min(CH, bad.size() - q0);
        for (size_t j = 0; j < nq; j++)
            HIPCHK(hipMemcpyAsync(fx->d_input + j * S, d_seg + bad[q0 + j] * S, S * sizeof(float), hipMemcpyDeviceToDevice, fx->stream));
        rc = forward_slice(fb, fx, fx->d_input, nq, fx->d_logits, fx->d_topk_idx, fx->d_topk_conf);
        if (rc != BH_OK) return rc;
        const float *f_emb = (d_emb && ED) ? fx->d_arena + fx->t_off[h.embedding_tensor] : nullptr;
        for (size_t j = 0; j < nq; j++) {
            const size_t i = bad[q0 + j];
            if (d_logits) HIPCHK(hipMemcpyAsync(d_logits + i * NC, fx->d_logits + j * NC, NC * sizeof(float), hipMemcpyDeviceToDevice, fx->stream));
            if (d_idx) HIPCHK(hipMemcpyAsync(d_idx + i * TK, fx->d_topk_idx + j * TK, TK * sizeof(int32_t), hipMemcpyDeviceToDevice, fx->stream));
            if (d_conf) HIPCHK(hipMemcpyAsync(d_conf + i * TK, fx->d_topk_conf + j * TK, TK * sizeof(float), hipMemcpyDeviceToDevice, fx->stream));
            if (f_emb) HIPCHK(hipMemcpyAsync(d_emb + i * ED, f_emb + j * ED, ED * sizeof(float), hipMemcpyDeviceToDevice, fx->stream));
        }
        HIPCHK(fetch_nonfinite(fx));
        HIPCHK(hipStreamSynchronize(fx->stream));
        if (*fx->h_nonfinite) {
            const unsigned n_bad = *fx->h_nonfinite;
            clear_nonfinite(fx);
            return fail(BH_ERR_NONFINITE, "%u segment(s) with finite samples produced inf / NaN logits on the f32 kernels too (f32 overflow inside the network)", n_bad);
        }
    }
    c->fallback_segments += bad.size();
    return BH_OK;
}

// Rows [r0, r0 + nr) of a host-fed slice whose results are in the context's buffers (inputs in ctx->d_input, host copies of the
// top-k rows in h_topk_*), after the synchronise that ended the slice: under BH_FLAG_AUTO the rows the top-k stage marked
// (BH_TOPK_NONFINITE in their first slot) are re-run and their host copies refreshed; *redone says whether any were.
int settle_rows(bh_classifier *c, bh_batch_context *ctx, size_t r0, size_t nr, float *d_emb, bool *redone) {
    *redone = false;
    if (!c->auto_fallback) return BH_OK;
    const size_t TK = c->top_k;
    std::vector<size_t> bad;
    for (size_t i = r0; i < r0 + nr; i++)
        if (ctx->h_topk_idx[i * TK] == BH_TOPK_NONFINITE) bad.push_back(i);
    if (bad.empty()) return BH_OK;
    const int rc = redo_rows_f32(c, ctx->d_input, bad, ctx->d_logits, ctx->d_topk_idx, ctx->d_topk_conf, d_emb);
    if (rc != BH_OK) return rc;
    for (size_t i : bad) {
        HIPCHK(hipMemcpy(ctx->h_topk_idx + i * TK, ctx->d_topk_idx + i * TK, TK * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ctx->h_topk_conf + i * TK, ctx->d_topk_conf + i * TK, TK * sizeof(float), hipMemcpyDeviceToHost));
    }
    *redone = true;
    return BH_OK;
}

// The model file as the caller has it: the BHM1 container, or -- what birda's ClassifierBuilder::model_path() is (reference
// classifier.rs:269-283) -- the .onnx file itself, read by the library's own graph walk (onnx_conv.hpp).  Told apart by the magic.
bool load_any_model(const char *path, bh::Model &m, std::string &err) {
    char magic[4] = {0, 0, 0, 0};
    if (FILE *f = fopen(path, "rb")) { const size_t got = fread(magic, 1, 4, f); fclose(f); if (got != 4) memset(magic, 0, 4); }
    else { err = std::string("cannot open model file ") + path; return false; }
    if (!memcmp(magic, "BHM1", 4)) return bh::load_model(path, m, err);
    if (bh::onnxc::load_onnx_model(path, m, err)) return true;
    if (err.find("not an ONNX ModelProto") != std::string::npos) err = std::string(path) + ": neither a BHM1 container nor an ONNX model (no ModelProto graph)";
    return false;
}

// A well-formed file whose front-end the kernels cannot express (or the evaluator cannot run) is BH_ERR_UNSUPPORTED, not a
// malformed file: onnx_conv.hpp marks that refusal with this phrase.
int model_load_status(const std::string &err) {
    return err.find(bh::onnxc::kFrontendRefusal) != std::string::npos ? BH_ERR_UNSUPPORTED : BH_ERR_IO;
}

int check_ctx(bh_classifier *c, bh_batch_context *ctx) {
    if (!c || !ctx) return fail(BH_ERR_INVALID, "null classifier or batch context");
    if (ctx->c != c) return fail(BH_ERR_INVALID, "batch context belongs to another classifier");
    return BH_OK;
}

// Host threads that gather the caller's segment slices into the pinned staging buffer
// (BIRDA_HIP_COPY_THREADS; default min(8, hardware threads / 2)).  One thread moves ~10 GB/s, a fifth of
// what the PCIe link takes.
unsigned copy_threads() {
    static const unsigned n = [] {
        if (const char *e = getenv("BIRDA_HIP_COPY_THREADS")) return (unsigned)std::max(1, atoi(e));
        const unsigned hw = std::thread::hardware_concurrency();
        return std::max(1u, std::min(8u, hw / 2));
    }();
    return n;
}

// Sub-slices of a host-fed slice: each is computed as soon as its own samples are on the copy stream.  A forward has a floor of
// about a millisecond however few segments it holds (21 launches whose workgroups walk their chunk loops serially) and the late
// blocks need >= 128 segments to fill the GPU.
//   * `lanes` (the normal case, lanes_begin below: sub-slices alternate between the context's compute streams, so one's launch
//     chain runs under another's kernels): EQUAL sub-slices of an eighth of the slice, at least 128 segments -- the first one
//     starts the device after 1/8 of the upload, and the floors overlap (measured, 1 000 PCM16 segments from pinned memory:
//     8 sub-slices on 3 lanes 8.8 ms, 6 on 2 lanes 9.1, 4 on 2 lanes 9.5, round 3's growing split in sequence 10.4;
//     12 sub-slices of 84 segments 10.4 again).
//   * in sequence on one stream (profiling / debug contexts, the resampling path, BIRDA_HIP_LANES=0) the split depends on which side
//     is the longer one (a small pipeline model, upload 55 GB/s, forward 0.85 ms + t per segment):
//       - the upload is SHORTER than the compute (PCM16 mono into the v2.4-shaped model: 5.2 against 6.3 us per segment; anything
//         into the Perch-sized one): few sub-slices of GROWING size -- a small first one starts the compute stream early, the last,
//         more than half of the slice, runs at the full-batch rate while nothing is left to upload: (1/8, 1/3, rest) = 9.5 ms per
//         1 000 segments against 11.0 for four quarters;
//       - the upload is LONGER (f32 segments: 10.5 us): the forward of the last sub-slice is all that is left after the last byte
//         has arrived, so it must be small: equal quarters (12.9 ms against 14.8 for the growing split).
// Boundaries are multiples of `align` segments.
bool lanes_possible(const bh_batch_context *ctx) {
    return !ctx->profiling && !ctx->keep_tensors && ctx->n_lanes >= 2;
}
std::vector<size_t> sub_slice_cuts(const bh_classifier *c, size_t nb, size_t align, bool single, size_t bytes_per_segment, bool lanes = false,
                                   uint32_t ctx_forced = 0) {
    std::vector<size_t> cuts;
    const int forced = (int)ctx_forced;   // (bh_batch_context_set_sub_slices: n equal sub-slices; 0: the automatic split)
    auto up = [&](size_t v) { return std::min(nb, (v + align - 1) / align * align); };
    if (forced == 1) {
    } else if (!single && forced > 1 && nb >= 256) {
        const size_t sub = up((nb + forced - 1) / forced);
        for (size_t v = sub; v < nb; v += sub) cuts.push_back(v);
    } else if (!single && lanes && nb >= 256) {
        const size_t sub = up(std::max<size_t>(128, (nb + 7) / 8));
        // a first sub-slice of 64 segments where the upload is the shorter side (PCM16: 5.2 against 6.3 us per segment): the device
        // starts after 0.33 ms instead of 0.65 and the short forward's floor runs under the next sub-slices (pinned PCM16
        // 111-114 k -> 115-117 k segments/s; 32 or 96 segments: no gain; pinned f32 segments, upload-bound, lose 2 % to it)
        const double upload_us = (double)bytes_per_segment / 55e3;
        const double compute_us = (2.0 * (double)c->model.macs_per_segment() + (double)c->mel_flops) / 130e6;
        const size_t first = upload_us < compute_us ? 64 : 0;
        size_t v0 = sub;
        constexpr double growth = 1.5;
        if (upload_us < compute_us && nb >= 512) {
            // the upload is the SHORTER side (PCM16: 5.2 against 6.5 us per segment): after the first sub-slices the data is always
            // there, and what a sub-slice costs beyond its segments (the launch chain, the late blocks' half-empty grids) is paid
            // per sub-slice -- so the sizes GROW, 64, 96, 160, 224, 320 ..., each next one arriving about when the one before
            // finishes.  Measured, 1 000 PCM16 segments from pinned memory, one box, interleaved (profiles/r5_d_subslice_growth.txt):
            // equal 128s 110.3 k segments/s, growth 1.25 116.7, 1.35 116.6, 1.5 119.4, 1.75 113.6, 2.0 99.5; bhh_process_file 91.4 ->
            // 97.0 k
            double size = 64.0;
            size_t v = 0;
            while (true) {
                const size_t sz = std::max<size_t>(align, (size_t)(size / 32.0 + 0.5) * 32);
                if (v + sz + 96 > nb) break;
                v += sz;
                cuts.push_back(up(v));
                size *= growth;
            }
        } else {
        if (first && first < sub && nb >= 512) { cuts.push_back(up(first)); v0 = up(first) + sub; }
        for (size_t v = v0; v + 64 <= nb; v += sub) cuts.push_back(v);   // (a tail under 64 segments joins the last sub-slice)
        }
        // the upload is the LONGER side (f32 segments): what is left when the last byte has arrived is the last sub-slice's forward,
        // so that one is kept short -- 64 segments (a forward of 64 lasts 0.9 ms, one of 128 1.2: tools/gpu_latency.py)
        if (upload_us >= compute_us) {
            const size_t last = cuts.empty() ? 0 : cuts.back();
            const size_t tail = (nb - 64) / align * align;
            if (tail > last + 32 && nb - tail >= 32) cuts.push_back(tail);
        }
    } else
    if (!single && nb >= 512) {
        const double upload_us = (double)bytes_per_segment / 55e3;
        const double compute_us = (2.0 * (double)c->model.macs_per_segment() + (double)c->mel_flops) / 130e6;   // ~130 TFLOP/s over the whole forward
        if (upload_us < compute_us) {
            const size_t c1 = up(std::max<size_t>(128, nb / 8)), c2 = up(std::max<size_t>(c1 + 128, nb * 9 / 20));
            if (c1 < nb) cuts.push_back(c1);
            if (c2 < nb && c2 > c1) cuts.push_back(c2);
        } else {
            const size_t sub = up(std::max<size_t>(128, (nb + 3) / 4));
            for (size_t v = sub; v < nb; v += sub) cuts.push_back(v);
        }
    }
    cuts.push_back(nb);
    return cuts;
}

// The sub-slices of one host-fed slice as concurrent lanes: the plan of each sub-slice's own size, side by side in the arena,
// alternating between the context's two compute streams.  A forward is a chain of 21 dependent launches (~0.85 ms however few
// segments it holds, and the late blocks need >= 128 segments to fill the chip); one after the other on one stream the chains of
// three sub-slices were 2.5 ms of a 10.4 ms slice.  False -- run them in sequence on the context's stream, as before -- for
// single-slice calls, profiling / debug contexts, BIRDA_HIP_LANES=0, or if the plans do not fit the arena.
bool lanes_begin(bh_classifier *c, bh_batch_context *ctx, const std::vector<size_t> &cuts, std::vector<SliceLane> &lanes) {
    lanes.clear();
    if (cuts.size() < 2 || !lanes_possible(ctx)) return false;
    if (ctx->plans.size() > 64) ctx->plans.clear();
    // streams for as many lanes as this slice has sub-slices, created on first use: the runtime maps a process's streams onto a few
    // hardware queues (four by default) in creation order, and every stream that exists -- used or not -- shifts that mapping
    const int want = (int)std::min<size_t>((size_t)ctx->n_lanes, cuts.size());
    for (int l = 1; l < want; l++)
        if (!ctx->lane_stream[l]) {
            if (hipStreamCreateWithFlags(&ctx->lane_stream[l], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&ctx->join_ev[l], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
        }
    ctx->lanes_in_use = want;
    size_t base = 0;
    for (size_t si = 0; si < cuts.size(); si++) {
        const size_t s0 = si ? cuts[si - 1] : 0, ns = cuts[si] - s0;
        auto it = ctx->plans.find(ns);
        if (it == ctx->plans.end()) {
            bh_batch_context::ArenaPlan p;
            plan_arena(c->model, c->sched, ns, false, p.t_off, p.total);
            it = ctx->plans.emplace(ns, std::move(p)).first;
        }
        if (base + it->second.total > ctx->arena_cap) { lanes.clear(); ctx->lane_fallbacks++; return false; }
        lanes.push_back({ctx->lane_stream[si % (size_t)want], ctx->d_arena + base, it->second.t_off.data(), s0});
        base += align_up(it->second.total, 64);
    }
    // the other lanes' streams start behind everything enqueued on the context's stream so far
    bool ok = hipEventRecord(ctx->fork_ev, ctx->stream) == hipSuccess;
    for (int l = 1; ok && l < want; l++) ok = hipStreamWaitEvent(ctx->lane_stream[l], ctx->fork_ev, 0) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); lanes.clear(); }
    return ok;
}
// ... and the context's stream continues behind them (result downloads, the next slice)
hipError_t lanes_end(bh_batch_context *ctx, const std::vector<SliceLane> &lanes) {
    if (lanes.empty()) return hipSuccess;
    for (int l = 1; l < ctx->lanes_in_use; l++) {
        hipError_t e = hipEventRecord(ctx->join_ev[l], ctx->lane_stream[l]);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->join_ev[l], 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
void lanes_sync(bh_batch_context *ctx) {
    for (int l = 1; l < bh_batch_context::MAX_LANES; l++)
        if (ctx->lane_stream[l]) (void)hipStreamSynchronize(ctx->lane_stream[l]);
}

// host slices -> results through ctx.
// A slice of up to max_batch segments is pipelined three ways: worker threads gather 32-segment chunks into
// pinned memory; each chunk's H2D copy is enqueued on the copy stream as soon as it is complete; and the
// slice is computed in up to four sub-slices on the compute stream, each waiting only for its own copies
// (reference: the decode thread filling the channel while the main thread runs batches,
// src/pipeline/processor.rs:647-671).
int predict_slices(bh_classifier *c, bh_batch_context *ctx, const float *const *segments, const float *contig,
                   size_t n, bh_result *out, float *logits_out, float *emb_out, bool whole_slice) {
    const auto &m = c->model;
    const size_t S = m.h.sample_count, NC = m.h.n_classes, TK = c->top_k;
    HIPCHK(hipSetDevice(c->device));
    if (segments)
        for (size_t i = 0; i < n; i++)
            if (!segments[i]) return fail(BH_ERR_INVALID, "segment %zu is null", i);
    // A contiguous list in PINNED (hipHostMalloc / hipHostRegister: bh_host_alloc, bh_host_register) memory goes to the device
    // straight from the caller's buffer: the gather into the context's own pinned staging -- a host memcpy, the bound of this
    // entry point for pageable input -- is skipped.
    bool pinned_src = false;
    if (contig && n > 0) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, contig) == hipSuccess) pinned_src = attr.type == hipMemoryTypeHost;
        else (void)hipGetLastError();   // pageable memory: "invalid value", not an error of this call
    }
    for (size_t b0 = 0; b0 < n; b0 += ctx->max_batch) {
        const size_t nb = std::min(ctx->max_batch, n - b0);
        constexpr size_t CH = 32;
        const size_t nchunks = (nb + CH - 1) / CH;
        // sub-slices (sub_slice_cuts above), in whole chunks; debug contexts keep one (bh_debug_read_tensor reads the last)
        // (whole_slice: the caller reads an arena tensor of the slice afterwards -- the embeddings of the two-stage path)
        const bool one = ctx->keep_tensors || emb_out || whole_slice;
        std::vector<size_t> cuts = sub_slice_cuts(c, nb, CH, one, S * sizeof(float), lanes_possible(ctx), ctx->forced_sub_slices);
        std::vector<SliceLane> lanes;
        if (!lanes_begin(c, ctx, cuts, lanes) && cuts.size() > 1) cuts = sub_slice_cuts(c, nb, CH, one, S * sizeof(float), false, ctx->forced_sub_slices);
        const size_t nsub = cuts.size();
        while (ctx->copy_ev.size() < nsub) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ctx->copy_ev.push_back(e);
        }
        // Every worker takes ITS share of every chunk, chunk after chunk (round 5): with one whole chunk per thread the first eight
        // chunks all completed together, 1.3 ms into a 512-segment call, and the upload -- the longer side -- started that late.
        // Now chunk 0 is on the copy stream after a few segments' worth of copying.  Streaming stores: bh_internal_stream_copy.
        auto gather_part = [&](size_t j, unsigned t, unsigned nt) {
            const size_t i1 = std::min(nb, (j + 1) * CH);
            for (size_t i = j * CH + t; i < i1; i += nt) {
                const float *src = segments ? segments[b0 + i] : contig + (b0 + i) * S;
                bh_internal_stream_copy(ctx->h_input + i * S, src, S * sizeof(float));
            }
        };
        // (a call of a few segments copies them itself: eight thread starts cost more than 18 MB of memcpy)
        const unsigned nthreads = (pinned_src || nb < 16) ? 1u : (unsigned)std::min<size_t>(copy_threads(), CH);
        std::vector<std::atomic<int>> done(nchunks);
        for (auto &d : done) d.store(0, std::memory_order_relaxed);
        if (nthreads > 1) {
            if (!ctx->pool) ctx->pool.reset(new GatherPool());
            ctx->pool->start(nthreads - 1, [&](unsigned t) {
                for (size_t j = 0; j < nchunks; j++) { gather_part(j, t, nthreads); done[j].fetch_add(1, std::memory_order_release); }
            });
        }
        int rc = BH_OK;
        size_t si_next = 0;
        for (size_t j = 0; j < nchunks && rc == BH_OK; j++) {
            if (!pinned_src) gather_part(j, 0, nthreads);     // (the calling thread is worker 0)
            if (nthreads > 1) while (done[j].load(std::memory_order_acquire) < (int)nthreads - 1) std::this_thread::yield();
            const size_t i0 = j * CH, i1 = std::min(nb, (j + 1) * CH);
            const float *h_src = pinned_src ? contig + (b0 + i0) * S : ctx->h_input + i0 * S;
            if (hipMemcpyAsync(ctx->d_input + i0 * S, h_src, (i1 - i0) * S * sizeof(float), hipMemcpyHostToDevice,
                               ctx->copy_stream) != hipSuccess) { rc = fail(BH_ERR_HIP, "H2D copy failed"); break; }
            if (i1 == cuts[si_next]) {   // a sub-slice is complete on the copy stream: compute it
                const size_t si = si_next++, s0 = si ? cuts[si - 1] : 0, ns = i1 - s0;
                const SliceLane *lane = lanes.empty() ? nullptr : &lanes[si];
                if (hipEventRecord(ctx->copy_ev[si], ctx->copy_stream) != hipSuccess ||
                    hipStreamWaitEvent(lane ? lane->s : ctx->stream, ctx->copy_ev[si], 0) != hipSuccess) { rc = fail(BH_ERR_HIP, "stream event failed"); break; }
                rc = forward_slice(c, ctx, ctx->d_input + s0 * S, ns, ctx->d_logits + s0 * NC, ctx->d_topk_idx + s0 * TK,
                                   ctx->d_topk_conf + s0 * TK, lane);
            }
        }
        if (nthreads > 1) ctx->pool->wait();
        if (rc == BH_OK && lanes_end(ctx, lanes) != hipSuccess) rc = fail(BH_ERR_HIP, "stream event failed");
        if (rc != BH_OK) {
            (void)hipStreamSynchronize(ctx->copy_stream); lanes_sync(ctx); (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
        if (out) {
            HIPCHK(hipMemcpyAsync(ctx->h_topk_idx, ctx->d_topk_idx, nb * TK * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(ctx->h_topk_conf, ctx->d_topk_conf, nb * TK * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        }
        if (logits_out)
            HIPCHK(hipMemcpyAsync(logits_out + b0 * NC, ctx->d_logits, nb * NC * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (emb_out)
            HIPCHK(hipMemcpyAsync(emb_out + b0 * m.h.embedding_dim, ctx->d_arena + ctx->t_off[m.h.embedding_tensor],
                                  nb * (size_t)m.h.embedding_dim * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (!out && c->auto_fallback)   // (logits-only calls: the marks of the top-k rows are how the bad rows are found)
            HIPCHK(hipMemcpyAsync(ctx->h_topk_idx, ctx->d_topk_idx, nb * TK * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(fetch_nonfinite(ctx));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (*ctx->h_nonfinite && c->auto_fallback) {   // BH_FLAG_AUTO: those rows again, on the f32 kernels
            bool redone = false;
            float *d_emb = (emb_out || whole_slice) ? ctx->d_arena + ctx->t_off[m.h.embedding_tensor] : nullptr;
            const int rr = settle_rows(c, ctx, 0, nb, d_emb, &redone);
            if (rr != BH_OK) return rr;
            clear_nonfinite(ctx);
            if (redone && logits_out) HIPCHK(hipMemcpy(logits_out + b0 * NC, ctx->d_logits, nb * NC * sizeof(float), hipMemcpyDeviceToHost));
            if (redone && emb_out)
                HIPCHK(hipMemcpy(emb_out + b0 * m.h.embedding_dim, ctx->d_arena + ctx->t_off[m.h.embedding_tensor],
                                 nb * (size_t)m.h.embedding_dim * sizeof(float), hipMemcpyDeviceToHost));
        }
        if (out)
            for (size_t i = 0; i < nb; i++) {
                bh_result &r = out[b0 + i];
                r.n_pred = 0;
                for (uint32_t k = 0; k < c->top_k; k++) {
                    const int32_t id = ctx->h_topk_idx[i * c->top_k + k];
                    if (id < 0) break;
                    r.index[r.n_pred] = id;
                    r.confidence[r.n_pred] = ctx->h_topk_conf[i * c->top_k + k];
                    r.n_pred++;
                }
            }
        const int nf = nonfinite_status(c, ctx);   // the rows are filled (marked rows come out empty); the call still fails
        if (nf != BH_OK) return nf;
    }
    return BH_OK;
}
int internal_ctx(bh_classifier *c, size_t n, bh_batch_context **out) {
    if (c->internal_ctx && c->internal_ctx->max_batch >= n) { *out = c->internal_ctx; return BH_OK; }
    if (c->internal_ctx) { ctx_destroy(c->internal_ctx); c->internal_ctx = nullptr; }
    int rc = ctx_create(c, n, false, &c->internal_ctx);
    *out = c->internal_ctx;
    return rc;
}

}  // namespace bhi

// The one place a context's device and pinned memory, events and streams are released: a context ctx_create gave up half way
// (null pointers, no stream set yet) goes through it as well.  The streams are drained before anything they may read is freed.
bh_batch_context::~bh_batch_context() {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto e : ev) (void)hipEventDestroy(e);
    for (auto e : copy_ev) (void)hipEventDestroy(e);
    for (auto e : done_ev) (void)hipEventDestroy(e);
    const bool own_streams = stream_set < 0;   // (a set of the classifier's goes back to it, below)
    if (copy_stream) { (void)hipStreamSynchronize(copy_stream); if (own_streams) (void)hipStreamDestroy(copy_stream); }
    for (int l = 1; l < MAX_LANES; l++) {
        if (lane_stream[l]) { (void)hipStreamSynchronize(lane_stream[l]); if (own_streams || l > 2) (void)hipStreamDestroy(lane_stream[l]); }
        if (join_ev[l]) (void)hipEventDestroy(join_ev[l]);
    }
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    (void)hipFree(d_input); (void)hipFree(d_minmax); (void)hipFree(d_inbad); (void)hipFree(d_arena);
    (void)hipFree(d_logits); (void)hipFree(d_topk_idx); (void)hipFree(d_topk_conf);
    (void)hipHostFree(h_input); (void)hipHostFree(h_topk_idx); (void)hipHostFree(h_topk_conf);
    (void)hipFree(d_raw); (void)hipHostFree(h_raw);
    (void)hipFree(d_pcm); (void)hipFree(d_starts); (void)hipFree(d_partial);
    (void)hipFree(d_nonfinite); (void)hipHostFree(h_nonfinite);
    if (stream && own_streams) (void)hipStreamDestroy(stream);
    if (!own_streams) { std::lock_guard<std::mutex> g(c->stream_mu); c->stream_sets[stream_set].used = false; }
}

extern "C" {

int bh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *bh_backend_name(void) { return "HIP (gfx950)"; }

// ---- provider arm + default batch size (reference classifier.rs:662-1089, lib.rs:256-288) ---------------
static void fill_device_facts(int32_t ordinal, bh_provider_status *o) {
    hipDeviceProp_t prop;
    if (ordinal < 0 || hipGetDeviceProperties(&prop, ordinal) != hipSuccess) { (void)hipGetLastError(); return; }
    snprintf(o->device_name, sizeof o->device_name, "%s", prop.name);
    snprintf(o->arch, sizeof o->arch, "%s", prop.gcnArchName);
    o->compute_units = (uint32_t)prop.multiProcessorCount;
    o->hbm_bytes = (uint64_t)prop.totalGlobalMem;
}

int bh_select_provider(const char *requested, int32_t device_ordinal, bh_provider_status *out) try {
    if (!requested || !out) return fail(BH_ERR_INVALID, "select_provider: null argument");
    memset(out, 0, sizeof *out);
    std::string req(requested);
    for (char &ch : req) if (ch >= 'A' && ch <= 'Z') ch = (char)(ch + 32);
    snprintf(out->requested, sizeof out->requested, "%s", req.c_str());
    const int ndev = bh_device_count();
    out->device_count = (uint32_t)std::max(ndev, 0);
    out->device = -1;
    auto use_hip = [&]() {
        out->device = device_ordinal < 0 ? 0 : device_ordinal;
        snprintf(out->actual, sizeof out->actual, "HIP");
        fill_device_facts(out->device, out);
    };
    if (req == "cpu") { snprintf(out->actual, sizeof out->actual, "CPU"); return BH_OK; }
    if (req == "auto" || req == "gpu") {
        if (ndev > 0 && device_ordinal < ndev) { use_hip(); return BH_OK; }
        snprintf(out->actual, sizeof out->actual, "CPU");
        snprintf(out->fallback_reason, sizeof out->fallback_reason, "No GPU providers available");
        return BH_OK;
    }
    if (req == "hip" || req == "rocm") {
        if (ndev <= 0) return fail(BH_ERR_NO_DEVICE, "HIP provider requested but no HIP device is available");
        if (device_ordinal >= ndev) return fail(BH_ERR_NO_DEVICE, "device %d out of range (0..%d)", device_ordinal, ndev - 1);
        use_hip();
        return BH_OK;
    }
    return fail(BH_ERR_INVALID, "select_provider: '%s' is not served by this backend (auto, gpu, hip, rocm, cpu)", requested);
} catch (...) { return on_exception(); }

int bh_classifier_provider_status(const bh_classifier *c, bh_provider_status *out) try {
    if (!c || !out) return fail(BH_ERR_INVALID, "provider_status: null argument");
    memset(out, 0, sizeof *out);
    snprintf(out->requested, sizeof out->requested, "hip");
    snprintf(out->actual, sizeof out->actual, "HIP");
    out->device = c->device;
    out->device_count = (uint32_t)std::max(bh_device_count(), 0);
    fill_device_facts(c->device, out);
    // BH_FLAG_AUTO degraded some rows to the f32 kernels: recorded as the reference records a provider fall-back (classifier.rs:742-754)
    if (const unsigned long long nfb = c->fallback_segments.load())
        snprintf(out->fallback_reason, sizeof out->fallback_reason,
                 "%llu segment(s) re-run on the f32 kernels: an activation left the f16 operand range of the split-f16 path", nfb);
    return BH_OK;
} catch (...) { return on_exception(); }

uint64_t bh_classifier_fallback_segments(const bh_classifier *c) { return c ? (uint64_t)c->fallback_segments.load() : 0; }

size_t bh_default_batch_size(uint32_t model_type, const char *provider_actual) {
    const char *p = provider_actual ? provider_actual : "HIP";
    if (!strcmp(p, "CPU")) return 8;                                                                  // batch_size::CPU
    if (!strcmp(p, "CUDA")) return (model_type == BH_MODEL_BIRDNET_V24 || model_type == BH_MODEL_BSG_FINLAND) ? 64 : 32;
    if (!strcmp(p, "TensorRT")) return 32;
    // the largest batch birda's own validator admits (MAX_BATCH_SIZE = 512, constants.rs:55, cli/validators.rs:140): one forward is a
    // chain of 21 dependent launches and the late blocks need >= 512 segments to fill the chip twice over -- measured
    // device-resident, 130 k segments/s at 256 against 144 k at 512; a 512-segment context is 2.1 GB of the 288
    if (!strcmp(p, "HIP")) return 512;
    return 16;                                                                                        // batch_size::OTHER_GPU
}

size_t bh_classifier_default_batch_size(const bh_classifier *c) {
    return c ? bh_default_batch_size(c->model.h.family, "HIP") : 0;
}
const char *bh_last_error(void) { return g_err.c_str(); }

// ---- range filter / species list (reference classifier.rs:587-645) -------------------------
int bh_classifier_set_range_filter(bh_classifier *c, const float *scores, size_t n_classes, float threshold,
                                   int keep_unmatched, int rerank) try {
    if (!c || !scores) return fail(BH_ERR_INVALID, "set_range_filter: null argument");
    if (n_classes != c->model.h.n_classes)
        return fail(BH_ERR_INVALID, "set_range_filter: %zu scores for %u classes", n_classes, c->model.h.n_classes);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());   // no launch may still read the table being replaced
    if (!c->d_class_score) HIPCHK(hipMalloc((void **)&c->d_class_score, n_classes * sizeof(float)));
    HIPCHK(hipMemcpy(c->d_class_score, scores, n_classes * sizeof(float), hipMemcpyHostToDevice));
    c->filter.class_score = c->d_class_score;
    c->filter.threshold = threshold;
    c->filter.keep_unmatched = keep_unmatched ? 1 : 0;
    c->filter.rerank = rerank ? 1 : 0;
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_classifier_set_species_list(bh_classifier *c, const uint8_t *keep, size_t n_classes) try {
    if (!c || !keep) return fail(BH_ERR_INVALID, "set_species_list: null argument");
    if (n_classes != c->model.h.n_classes)
        return fail(BH_ERR_INVALID, "set_species_list: %zu flags for %u classes", n_classes, c->model.h.n_classes);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    if (!c->d_species_keep) HIPCHK(hipMalloc((void **)&c->d_species_keep, n_classes));
    HIPCHK(hipMemcpy(c->d_species_keep, keep, n_classes, hipMemcpyHostToDevice));
    c->filter.species_keep = c->d_species_keep;
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_topk_from_logits(bh_classifier *c, const float *logits, size_t n, bh_result *out) try {
    if (!c || (n && (!logits || !out))) return fail(BH_ERR_INVALID, "topk_from_logits: null argument");
    if (!n) return BH_OK;
    HIPCHK(hipSetDevice(c->device));
    const size_t nc = c->model.h.n_classes, tk = c->top_k;
    float *d_l = nullptr, *d_c = nullptr;
    int32_t *d_i = nullptr;
    std::vector<int32_t> hi(n * tk);
    std::vector<float> hc(n * tk);
    hipError_t e = hipMalloc((void **)&d_l, n * nc * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&d_i, n * tk * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&d_c, n * tk * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_l, logits, n * nc * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        bh::launch_topk(d_l, (int)n, (int)nc, (int)c->model.h.output_activation, (int)tk, c->min_conf, c->filter, d_i, d_c, nullptr, nullptr, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(hi.data(), d_i, n * tk * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(hc.data(), d_c, n * tk * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d_l); (void)hipFree(d_i); (void)hipFree(d_c);
    if (e != hipSuccess) return fail(BH_ERR_HIP, "topk_from_logits: %s", hipGetErrorString(e));
    for (size_t i = 0; i < n; i++) {
        bh_result &r = out[i];
        r.n_pred = 0;
        for (size_t k = 0; k < tk; k++) {
            if (hi[i * tk + k] < 0) break;
            r.index[r.n_pred] = hi[i * tk + k];
            r.confidence[r.n_pred] = hc[i * tk + k];
            r.n_pred++;
        }
    }
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_classifier_clear_filters(bh_classifier *c) try {
    if (!c) return fail(BH_ERR_INVALID, "clear_filters: null classifier");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    {   // the range filter / species list only: BSG tables have their own clear
        bh::TopkFilter f{};
        f.bsg_intercept = c->filter.bsg_intercept; f.bsg_slope = c->filter.bsg_slope; f.bsg_prior = c->filter.bsg_prior;
        c->filter = f;
    }
    return BH_OK;
} catch (...) { return on_exception(); }

// ---- BSG post-processing tables (reference classifier.rs:508-545) ------------------------------------------
int bh_classifier_set_bsg(bh_classifier *c, const float *intercept, const float *slope, const float *prior, size_t n_classes) try {
    if (!c || !intercept || !slope) return fail(BH_ERR_INVALID, "set_bsg: null argument");
    if (n_classes != c->model.h.n_classes) return fail(BH_ERR_INVALID, "set_bsg: %zu entries for %u classes", n_classes, c->model.h.n_classes);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    if (!c->d_bsg) HIPCHK(hipMalloc((void **)&c->d_bsg, 3 * n_classes * sizeof(float)));
    HIPCHK(hipMemcpy(c->d_bsg, intercept, n_classes * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_bsg + n_classes, slope, n_classes * sizeof(float), hipMemcpyHostToDevice));
    if (prior) HIPCHK(hipMemcpy(c->d_bsg + 2 * n_classes, prior, n_classes * sizeof(float), hipMemcpyHostToDevice));
    c->filter.bsg_intercept = c->d_bsg;
    c->filter.bsg_slope = c->d_bsg + n_classes;
    c->filter.bsg_prior = prior ? c->d_bsg + 2 * n_classes : nullptr;
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_classifier_clear_bsg(bh_classifier *c) try {
    if (!c) return fail(BH_ERR_INVALID, "clear_bsg: null classifier");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    c->filter.bsg_intercept = c->filter.bsg_slope = c->filter.bsg_prior = nullptr;
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_classifier_info(const bh_classifier *c, bh_model_info *info) {
    if (!c || !info) return fail(BH_ERR_INVALID, "classifier_info: null argument");
    const auto &h = c->model.h;
    info->sample_rate = h.sample_rate; info->segment_duration = h.segment_duration; info->sample_count = h.sample_count;
    info->n_classes = h.n_classes; info->embedding_dim = h.embedding_dim; info->output_activation = h.output_activation;
    info->spec_channels = h.n_branches; info->spec_h = h.spec_h; info->spec_w = h.spec_w;
    info->n_layers = h.n_layers; info->macs_per_segment = c->model.macs_per_segment();
    info->mel_flops_per_segment = c->mel_flops;
    info->model_type = h.family;
    info->precision = c->auto_fallback ? BH_FLAG_AUTO : c->precision == 3 ? BH_FLAG_F16X3 : c->precision == 1 ? BH_FLAG_F16 : BH_FLAG_F32;
    return BH_OK;
}

const char *bh_classifier_label(const bh_classifier *c, uint32_t index) {
    if (!c || index >= c->labels.size()) return nullptr;
    return c->labels[index].c_str();
}

int bh_classifier_is_warm(const bh_classifier *c, size_t batch_size) {
    if (!c) return 0;
    auto *cc = const_cast<bh_classifier *>(c);
    std::lock_guard<std::mutex> g(cc->warm_mu);
    return cc->warmed.count(batch_size) ? 1 : 0;
}

int bh_classifier_ensure_warm(bh_classifier *c, size_t batch_size) try {
    if (!c || batch_size == 0) return fail(BH_ERR_INVALID, "ensure_warm: bad arguments");
    if (bh_classifier_is_warm(c, batch_size)) return BH_OK;
    // warmup(batch_size): all-zero segments through the real path (classifier.rs:443-466)
    std::vector<float> zero(c->model.h.sample_count, 0.0f);
    std::vector<const float *> segs(batch_size, zero.data());
    std::vector<bh_result> res(batch_size);
    bool had_ctx;
    { std::lock_guard<std::mutex> g(c->internal_mu); had_ctx = c->internal_ctx != nullptr; }
    int rc = bh_predict_batch(c, segs.data(), batch_size, zero.size(), res.data());
    if (!had_ctx) {
        // the warm-up's context is not kept: callers that batch create their own (process_file does, right after this
        // call), and a second full-size arena for the classifier's lifetime would only double the memory
        std::lock_guard<std::mutex> g(c->internal_mu);
        if (c->internal_ctx) { ctx_destroy(c->internal_ctx); c->internal_ctx = nullptr; }
    }
    if (rc != BH_OK) return rc;  // recorded only after success (classifier.rs:424)
    std::lock_guard<std::mutex> g(c->warm_mu);
    c->warmed.insert(batch_size);
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_batch_context_create(bh_classifier *c, size_t max_batch, bh_batch_context **out) try {
    const char *keep = getenv("BIRDA_HIP_KEEP_TENSORS");
    const bool keep_t = keep && keep[0] == '1';
    if (c && out && !keep_t) {
        std::lock_guard<std::mutex> g(c->parked_mu);
        // a parked context of this size, or failing that one up to twice as large (files of slightly different lengths cap their
        // effective batch differently, processor.rs:531-545: an exact match alone would rebuild 4 GB of arena for each of them)
        bh_batch_context **pick = nullptr;
        for (bh_batch_context *&p : c->parked_ctx)
            if (p && !p->keep_tensors && p->max_batch == max_batch) { pick = &p; break; }
        if (!pick)
            for (bh_batch_context *&p : c->parked_ctx)
                if (p && !p->keep_tensors && p->max_batch > max_batch && p->max_batch <= 2 * max_batch && (!pick || p->max_batch < (*pick)->max_batch)) pick = &p;
        if (pick) {
            *out = *pick;
            *pick = nullptr;
            (*out)->asked_batch = max_batch;
            (*out)->pending.clear();
            return BH_OK;
        }
    }
    return ctx_create(c, max_batch, keep_t, out);
} catch (...) { return on_exception(); }

size_t bh_classifier_trim(bh_classifier *c) {
    if (!c) return 0;
    size_t freed = 0;
    bh_batch_context *gone[bh_classifier::N_PARKED + 1] = {};
    int n = 0;
    {
        std::lock_guard<std::mutex> g(c->parked_mu);
        for (bh_batch_context *&p : c->parked_ctx)
            if (p) { gone[n++] = p; p = nullptr; }
    }
    {
        std::lock_guard<std::mutex> g(c->internal_mu);
        if (c->internal_ctx) { gone[n++] = c->internal_ctx; c->internal_ctx = nullptr; }
    }
    (void)hipSetDevice(c->device);
    for (int i = 0; i < n; i++) { freed += gone[i]->device_bytes; ctx_destroy(gone[i]); }
    return freed;
}

void bh_batch_context_destroy(bh_batch_context *ctx) {
    if (!ctx) return;
    bh_classifier *c = ctx->c;
    if (!ctx->keep_tensors && !ctx->profiling) {   // parked for the next create of this size (see bh_classifier::parked_ctx)
        ctx->forced_sub_slices = 0;
        ctx->pending.clear();   // (a caller that destroys without a synchronise: the next owner must not repair into ITS freed buffers)
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(ctx->stream);
        *ctx->h_nonfinite = 0;
        (void)hipMemsetAsync(ctx->d_nonfinite, 0, sizeof(unsigned), ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        bh_batch_context *old = nullptr;
        {
            std::lock_guard<std::mutex> g(c->parked_mu);
            bh_batch_context **slot = nullptr;
            for (bh_batch_context *&p : c->parked_ctx)
                if (!p) { slot = &p; break; }
            if (!slot) {      // all taken: one of a different size goes, else the oldest (first) one; the newcomer is the youngest (last)
                int gone = 0;
                for (int i = 0; i < bh_classifier::N_PARKED; i++)
                    if (c->parked_ctx[i]->max_batch != ctx->max_batch) { gone = i; break; }
                old = c->parked_ctx[gone];
                for (int i = gone; i + 1 < bh_classifier::N_PARKED; i++) c->parked_ctx[i] = c->parked_ctx[i + 1];
                slot = &c->parked_ctx[bh_classifier::N_PARKED - 1];
            }
            *slot = ctx;
        }
        if (old) ctx_destroy(old);
        return;
    }
    ctx_destroy(ctx);
}
size_t bh_batch_context_bytes(const bh_batch_context *ctx) {
    return ctx ? ctx->max_batch * (size_t)ctx->c->model.h.sample_count * sizeof(float) : 0;
}
size_t bh_batch_context_device_bytes(const bh_batch_context *ctx) { return ctx ? ctx->device_bytes : 0; }
uint64_t bh_batch_context_lane_fallbacks(const bh_batch_context *ctx) { return ctx ? ctx->lane_fallbacks : 0; }
int bh_batch_context_set_sub_slices(bh_batch_context *ctx, uint32_t n) {
    if (!ctx) return fail(BH_ERR_INVALID, "null batch context");
    ctx->forced_sub_slices = n;
    return BH_OK;
}
void *bh_batch_context_host_buffer(bh_batch_context *ctx, size_t *bytes) {
    if (bytes) *bytes = ctx ? bh_batch_context_bytes(ctx) : 0;
    return ctx ? ctx->h_input : nullptr;
}

int bh_predict(bh_classifier *c, const float *segment, size_t n_samples, bh_result *out) try {
    const float *segs[1] = {segment};
    return bh_predict_batch(c, segs, 1, n_samples, out);
} catch (...) { return on_exception(); }

int bh_predict_batch(bh_classifier *c, const float *const *segments, size_t n, size_t n_samples, bh_result *out) try {
    if (!c || !segments || !out) return fail(BH_ERR_INVALID, "predict_batch: null argument");
    if (n == 0) return BH_OK;
    if (n_samples != c->model.h.sample_count)
        return fail(BH_ERR_INVALID, "segment has %zu samples, model expects %u", n_samples, c->model.h.sample_count);
    std::lock_guard<std::mutex> g(c->internal_mu);
    bh_batch_context *ctx = nullptr;
    int rc = internal_ctx(c, n, &ctx);
    if (rc != BH_OK) return rc;
    return predict_slices(c, ctx, segments, nullptr, n, out, nullptr, nullptr);
} catch (...) { return on_exception(); }

int bh_predict_batch_with_context(bh_classifier *c, bh_batch_context *ctx, const float *const *segments, size_t n,
                                  size_t n_samples, bh_result *out) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if (!segments || !out) return fail(BH_ERR_INVALID, "predict_batch_with_context: null argument");
    if (n > ctx->asked_batch) return fail(BH_ERR_INVALID, "batch of %zu exceeds context capacity %zu", n, ctx->asked_batch);
    if (n_samples != c->model.h.sample_count)
        return fail(BH_ERR_INVALID, "segment has %zu samples, model expects %u", n_samples, c->model.h.sample_count);
    return predict_slices(c, ctx, segments, nullptr, n, out, nullptr, nullptr);
} catch (...) { return on_exception(); }

int bh_host_alloc(size_t bytes, void **out) try {
    if (!out || bytes == 0) return fail(BH_ERR_INVALID, "host_alloc: null argument or zero size");
    *out = nullptr;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(BH_ERR_HIP, "hipHostMalloc of %zu bytes failed", bytes); }
    return BH_OK;
} catch (...) { return on_exception(); }

void bh_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int bh_host_register(void *p, size_t bytes) try {
    if (!p || bytes == 0) return fail(BH_ERR_INVALID, "host_register: null argument or zero size");
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return fail(BH_ERR_HIP, "hipHostRegister of %zu bytes failed", bytes); }
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_host_unregister(void *p) try {
    if (!p) return BH_OK;
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return fail(BH_ERR_HIP, "hipHostUnregister failed"); }
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_predict_batch_contig(bh_classifier *c, bh_batch_context *ctx, const float *base, size_t n, bh_result *out) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if (!base || !out) return fail(BH_ERR_INVALID, "predict_batch_contig: null argument");
    return predict_slices(c, ctx, nullptr, base, n, out, nullptr, nullptr);
} catch (...) { return on_exception(); }

int bh_predict_batch_logits(bh_classifier *c, bh_batch_context *ctx, const float *base, size_t n, float *logits,
                            float *embeddings) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if (!base || !logits) return fail(BH_ERR_INVALID, "predict_batch_logits: null argument");
    return predict_slices(c, ctx, nullptr, base, n, nullptr, logits, embeddings);
} catch (...) { return on_exception(); }

// BH_FLAG_AUTO on the device-resident path: the marked rows of every forward enqueued since the last settle, again on the f32
// kernels (forwards that shared their buffers have been overwritten by the last one of them, whose rows these are).  Ends with
// the stream idle, the pending list empty and the counter cleared.
static int settle_pending(bh_classifier *c, bh_batch_context *ctx) {
    HIPCHK(fetch_nonfinite(ctx));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (*ctx->h_nonfinite && c->auto_fallback) {
        std::vector<int32_t> h_idx;
        std::vector<size_t> bad;
        for (const auto &p : ctx->pending) {
            h_idx.resize(p.n * c->top_k);
            HIPCHK(hipMemcpy(h_idx.data(), p.d_idx, h_idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            bad.clear();
            for (size_t i = 0; i < p.n; i++)
                if (h_idx[i * c->top_k] == BH_TOPK_NONFINITE) bad.push_back(i);
            const int rc = redo_rows_f32(c, p.d_seg, bad, p.d_logits, p.d_idx, p.d_conf, nullptr);
            if (rc != BH_OK) { ctx->pending.clear(); clear_nonfinite(ctx); return rc; }
        }
        clear_nonfinite(ctx);
    }
    ctx->pending.clear();
    return BH_OK;
}

int bh_forward_device(bh_classifier *c, bh_batch_context *ctx, const float *d_segments, size_t n, float *d_logits,
                      int32_t *d_topk_index, float *d_topk_conf) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if (!d_segments || !d_logits) return fail(BH_ERR_INVALID, "forward_device: null device pointer");
    HIPCHK(hipSetDevice(c->device));
    const auto &h = c->model.h;
    for (size_t b0 = 0; b0 < n; b0 += ctx->max_batch) {
        const size_t nb = std::min(ctx->max_batch, n - b0);
        const bool track = c->auto_fallback && d_topk_index && d_topk_conf;   // what bh_batch_context_synchronize re-runs marked rows from
        const bh_batch_context::Pending p{d_segments + b0 * h.sample_count, nb, d_logits + b0 * h.n_classes,
                                          d_topk_index ? d_topk_index + b0 * c->top_k : nullptr,
                                          d_topk_conf ? d_topk_conf + b0 * c->top_k : nullptr};
        bool known = !track;
        if (track)
            for (const auto &q : ctx->pending) known |= q.d_seg == p.d_seg && q.n == p.n && q.d_logits == p.d_logits && q.d_idx == p.d_idx && q.d_conf == p.d_conf;
        // a full list is settled HERE (an internal synchronise + repair of what is enqueued so far) rather than dropped: the header
        // promises BH_OK with the rows re-run however many distinct forwards a caller enqueues between two synchronises
        if (!known && ctx->pending.size() >= bh_batch_context::MAX_PENDING) {
            rc = settle_pending(c, ctx);
            if (rc != BH_OK) return rc;
        }
        rc = forward_slice(c, ctx, p.d_seg, nb, p.d_logits, p.d_idx, p.d_conf);
        if (rc != BH_OK) return rc;
        if (!known) ctx->pending.push_back(p);
    }
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_batch_context_synchronize(bh_batch_context *ctx) try {
    if (!ctx) return fail(BH_ERR_INVALID, "synchronize: null context");
    bh_classifier *c = ctx->c;
    HIPCHK(hipSetDevice(c->device));
    const int rc = settle_pending(c, ctx);
    if (rc != BH_OK) return rc;
    return nonfinite_status(c, ctx);   // BH_ERR_NONFINITE once per occurrence: the counter is cleared
} catch (...) { return on_exception(); }
void *bh_batch_context_stream(bh_batch_context *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

uint64_t bh_tensor_floats(const bh_classifier *c, uint32_t tensor) {
    if (!c || tensor >= c->model.tensor_floats.size()) return 0;
    return c->model.tensor_floats[tensor];
}

int bh_debug_read_tensor(bh_classifier *c, bh_batch_context *ctx, uint32_t tensor, float *host, size_t max_floats) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if (!ctx->keep_tensors) return fail(BH_ERR_INVALID, "context was not created with BIRDA_HIP_KEEP_TENSORS=1");
    if (tensor >= c->model.tensor_floats.size()) return fail(BH_ERR_INVALID, "tensor %u out of range", tensor);
    const size_t nfl = c->model.tensor_floats[tensor] * ctx->last_n;
    if (nfl > max_floats) return fail(BH_ERR_INVALID, "host buffer too small (%zu < %zu)", max_floats, nfl);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const float *src = (tensor == c->model.layers.size()) ? ctx->last_logits : ctx->d_arena + ctx->t_off[tensor];
    HIPCHK(hipMemcpy(host, src, nfl * sizeof(float), hipMemcpyDeviceToHost));
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_audit_arena_plan(bh_classifier *c, bh_batch_context *ctx, size_t n, uint64_t *off_floats, uint64_t *size_floats, uint8_t *path,
                        size_t cap) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    const auto &m = c->model;
    const size_t nl = m.layers.size(), nt = nl + 1;
    if (!off_floats || !size_floats || !path || cap < nt) return fail(BH_ERR_INVALID, "arena_plan: %zu entries needed", nt);
    const bool keep = ctx->keep_tensors;
    std::vector<size_t> off, sz;
    size_t total = 0;
    // n == 0: the context's own plan (what its forwards of max_batch segments use); else the plan a lane of n segments gets
    const std::vector<Step> &sched = schedule_of(ctx);
    plan_arena(m, sched, n ? n : ctx->max_batch, keep, off, total, &sz);
    if (!n) off = ctx->t_off;
    for (size_t t = 0; t < nt; t++) { off_floats[t] = off[t]; size_floats[t] = sz[t]; }
    // the path the forward takes at each layer: its schedule's
    for (size_t i = 0; i < cap; i++) path[i] = BH_PATH_INNER;
    for (const Step &st : sched) path[st.first] = st.path;
    return (int)nt;
} catch (...) { return on_exception(); }

int bh_batch_context_layer_ms(bh_batch_context *ctx, float *ms, uint32_t *launches, size_t n_layers) try {
    if (!ctx || !ms) return fail(BH_ERR_INVALID, "layer_ms: null argument");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n_layers; i++) { ms[i] = 0.f; if (launches) launches[i] = 0; }
    for (size_t i = 1; i < ctx->ev.size(); i++) {
        const int ly = ctx->ev_layer[i];
        if (ly < 0 || (size_t)ly >= n_layers) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, ctx->ev[i - 1], ctx->ev[i]) == hipSuccess) { ms[ly] += t; if (launches) launches[ly]++; }
    }
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_classifier_fused_blocks(const bh_classifier *c, int32_t *cfgs, size_t cap) {
    if (!c) return 0;
    for (size_t i = 0; i < c->mb.size() && cfgs && i < cap; i++) cfgs[i] = c->mb[i].cfg;
    return (int)c->mb.size();
}

int bh_onnx_to_bhm(const char *onnx_path, const char *bhm_path) try {
    if (!onnx_path || !bhm_path) return fail(BH_ERR_INVALID, "onnx_to_bhm: null path");
    bh::Model m;
    std::string err;
    if (!bh::onnxc::load_onnx_model(onnx_path, m, err)) return fail(model_load_status(err), "%s", err.c_str());
    if (!bh::onnxc::write_bhm(bhm_path, m, err)) return fail(BH_ERR_IO, "%s", err.c_str());
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_onnx_eval(const char *onnx_path, const char *feed_name, const double *feed, const int64_t *feed_dims, uint32_t feed_rank,
                 const char *target, double *out, size_t out_cap, int64_t *out_dims, uint32_t *out_rank) try {
    if (!onnx_path || !target || !out_dims || !out_rank || (feed_name && (!feed || (feed_rank && !feed_dims)))) return fail(BH_ERR_INVALID, "onnx_eval: null argument");
    if (feed_rank > bh::onnxf::EVAL_MAX_RANK) return fail(BH_ERR_INVALID, "onnx_eval: feed of rank %u", feed_rank);
    std::vector<uint8_t> buf;
    std::string err;
    bh::onnxc::Graph g;
    if (!bh::onnxc::read_file(onnx_path, buf, err) || !bh::onnxc::parse_graph(bh::onnxd::Span{buf.data(), buf.size()}, g, err)) return fail(BH_ERR_IO, "%s: %s", onnx_path, err.c_str());
    try {
        bh::onnxf::Evaluator ev(g);
        bh::onnxf::Evaluator::Env feeds;
        if (feed_name) {
            bh::onnxf::Arr a;
            a.d.assign(feed_dims, feed_dims + feed_rank);
            a.v.assign(feed, feed + bh::onnxf::shape_elems(a.d));
            feeds[feed_name] = std::move(a);
        }
        const auto r = ev.run(feeds, {std::string(target)});
        const bh::onnxf::Arr &t = r[0];
        *out_rank = (uint32_t)t.rank();
        for (size_t i = 0; i < t.rank() && i < 8; i++) out_dims[i] = t.d[i];
        if (t.size() > out_cap || !out) return fail(BH_ERR_INVALID, "onnx_eval: tensor '%s' has %zu values, room for %zu", target, t.size(), out_cap);
        for (size_t i = 0; i < t.size(); i++) out[i] = t.f(i);
    } catch (const bh::onnxf::EvalError &e) {
        // (a well-formed graph the evaluator cannot run -- an operator outside its set, a shape beyond its bounds -- is the same
        //  condition bh_classifier_create reports as BH_ERR_UNSUPPORTED; a file that does not parse was BH_ERR_IO above)
        return fail(BH_ERR_UNSUPPORTED, "%s: %s", onnx_path, e.what());
    } catch (const std::bad_alloc &) { return fail(BH_ERR_UNSUPPORTED, "%s: out of memory while evaluating the graph", onnx_path); }
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_classifier_weight_summary(const bh_classifier *c, uint64_t *out, size_t cap) {
    if (!c) return fail(BH_ERR_INVALID, "weight_summary: null classifier");
    uint64_t v[BH_WS_COUNT] = {0};
    v[BH_WS_FLOAT16_FILE] = c->model.file_f16 ? 1 : 0;
    for (const LayerState &S : c->layer) {
        if (!S.planes) continue;
        v[BH_WS_GEMM_LAYERS]++;
        v[BH_WS_PLANE_BYTES] += S.plane_bytes;
        if (S.terms == 2) { v[BH_WS_TWO_TERM_LAYERS]++; v[BH_WS_TWO_TERM_PLANE_BYTES] += S.plane_bytes; }
    }
    for (size_t i = 0; i < cap && i < (size_t)BH_WS_COUNT; i++)
        if (out) out[i] = v[i];
    return BH_WS_COUNT;
}

// per layer: the terms its split-f16 GEMM runs (1, 2 or 3), 0 for a layer without operand planes (inside a fused block, f32, ...)
int bh_debug_layer_terms(const bh_classifier *c, int32_t *terms, size_t cap) {
    if (!c) return fail(BH_ERR_INVALID, "debug_layer_terms: null classifier");
    for (size_t i = 0; i < c->layer.size() && i < cap; i++)
        if (terms) terms[i] = c->layer[i].terms;
    return (int)c->layer.size();
}

// the instantiation the split-f16 GEMM of `layer` launched last (a launcher's name string), "" before any forward / for a layer
// that takes none of those launchers; a grouped convolution names its f32 kernel as well; returns its length
int bh_debug_layer_kernel(const bh_classifier *c, uint32_t layer, char *out, size_t cap) {
    if (!c || layer >= c->layer.size()) return fail(BH_ERR_INVALID, "debug_layer_kernel: bad arguments");
    return copy_name(c->layer[layer].kernel.load(std::memory_order_relaxed), out, cap);
}

int bh_plan_fused_blocks(const char *model_path, uint32_t flags, int32_t *cfgs, int32_t *layers, size_t cap) try {
    if (!model_path) return fail(BH_ERR_INVALID, "plan_fused_blocks: null model path");
    bh::Model m;
    std::string err;
    if (!load_any_model(model_path, m, err)) return fail(model_load_status(err), "%s", err.c_str());
    const uint32_t p = flags & BH_FLAG_PRECISION_MASK;
    const int precision = p == BH_FLAG_F32 ? 0 : p == BH_FLAG_F16 ? 1 : 3;
    const std::vector<int> readers = tensor_readers(m);
    size_t n = 0;
    for (size_t i = 0; i + 2 < m.layers.size(); i++) {
        bh::MbDesc d{};
        if (!describe_fused_block(m, readers, i, precision, -1, d)) continue;
        if (n < cap) { if (cfgs) cfgs[n] = d.cfg; if (layers) layers[n] = (int32_t)i; }
        n++;
        bh::MbDesc tw{};
        if (bh::mb_plan_twin(d, tw)) {   // the block's small-launch twin is part of what the library must ship: listed behind it
            if (n < cap) { if (cfgs) cfgs[n] = tw.cfg; if (layers) layers[n] = (int32_t)i; }
            n++;
        }
        if (bh::mb_plan_narrow(d, tw)) {   // ... and its few-segment twin
            if (n < cap) { if (cfgs) cfgs[n] = tw.cfg; if (layers) layers[n] = (int32_t)i; }
            n++;
        }
        i = fused_block_last(i, d);
    }
    return (int)n;
} catch (...) { return on_exception(); }

// (the first three families only: callers derive n_base as a third of what this names -- birda_hip.h)
int bh_mb_config_name(int32_t cfg, char *out, size_t cap) {
    const int n3 = bh::mb_config_count() / bh::mb_config_families() * 3;
    return cfg >= 0 && cfg < n3 ? bh::mb_config_name(cfg, out, cap) : 0;
}
int bh_mb_config_families(void) { return bh::mb_config_families(); }
int bh_mb_config_name_ex(int32_t cfg, char *out, size_t cap) {
    return bh::mb_config_name(cfg, out, cap);
}

int bh_classifier_frontend_kernel(const bh_classifier *c, char *out, size_t cap) {
    if (!c) return 0;
    char buf[64];
    const int nmp = c->fe.br[0].nm_pad;
    // what the last forward launched (launch_mel's own answer); before any forward, the dispatch restated from the plan
    if (const char *ran = c->fe_kernel.load(std::memory_order_relaxed)) snprintf(buf, sizeof buf, "%s", ran);
    else if (c->fe.prec == 32) snprintf(buf, sizeof buf, "bh::mel32_kernel<%d>", nmp / 32);
    else snprintf(buf, sizeof buf, "bh::mel_kernel<%d, %d, 1>", nmp / 16, c->fe.prec);   // (third argument: HALVES, kernels_frontend.hip)
    return copy_name(buf, out, cap);
}

int bh_batch_context_set_profiling(bh_batch_context *ctx, int enabled) try {
    if (!ctx) return fail(BH_ERR_INVALID, "set_profiling: null context");
    if (enabled) {   // a new measurement: drop the events of the previous one (after they have fired)
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (auto e : ctx->ev) (void)hipEventDestroy(e);
        ctx->ev.clear(); ctx->ev_stage.clear(); ctx->ev_layer.clear();
    }
    ctx->profiling = enabled != 0;
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_batch_context_stage_ms(bh_batch_context *ctx, float *ms, uint32_t *launches) try {
    if (!ctx || !ms) return fail(BH_ERR_INVALID, "stage_ms: null argument");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < BH_N_STAGES; i++) { ctx->stage_ms[i] = 0.f; ctx->stage_launches[i] = 0; }
    for (size_t i = 1; i < ctx->ev.size(); i++) {
        const int st = ctx->ev_stage[i];
        if (st < 0) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, ctx->ev[i - 1], ctx->ev[i]) == hipSuccess) {
            ctx->stage_ms[st] += t;
            ctx->stage_launches[st]++;
        }
    }
    for (int i = 0; i < BH_N_STAGES; i++) { ms[i] = ctx->stage_ms[i]; if (launches) launches[i] = ctx->stage_launches[i]; }
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_predict_batch_source_rate(bh_classifier *c, bh_batch_context *ctx, const float *const *segments, size_t n,
                                 size_t n_src_samples, uint32_t source_rate, bh_result *out) try {
    if (!c || !segments || !out) return fail(BH_ERR_INVALID, "predict_batch_source_rate: null argument");
    if (n == 0) return BH_OK;
    const auto &h = c->model.h;
    if (source_rate == h.sample_rate) {
        if (ctx) return bh_predict_batch_with_context(c, ctx, segments, n, n_src_samples, out);
        return bh_predict_batch(c, segments, n, n_src_samples, out);
    }
    std::unique_lock<std::mutex> lock(c->internal_mu, std::defer_lock);
    if (!ctx) {
        lock.lock();
        int rc0 = internal_ctx(c, n, &ctx);
        if (rc0 != BH_OK) return rc0;
    } else {
        int rc0 = check_ctx(c, ctx);
        if (rc0 != BH_OK) return rc0;
        if (n > ctx->asked_batch) return fail(BH_ERR_INVALID, "batch of %zu exceeds context capacity %zu", n, ctx->asked_batch);
    }
    HIPCHK(hipSetDevice(c->device));
    {   // the rate pair first: a header that names a rate the resampler has no operator for is "unsupported", not the "out of memory" its
        // source-rate staging buffer would end in
        const char *perr = nullptr;
        if (!bh::resample_plan(source_rate, h.sample_rate, &perr))
            return fail(BH_ERR_UNSUPPORTED, "%s (%u -> %u Hz)", perr ? perr : "resampler", source_rate, h.sample_rate);
    }
    if (ctx->raw_len < n_src_samples) {
        (void)hipFree(ctx->d_raw); (void)hipHostFree(ctx->h_raw);
        ctx->d_raw = nullptr; ctx->h_raw = nullptr; ctx->raw_len = 0;
        HIPCHK(hipMalloc((void **)&ctx->d_raw, ctx->max_batch * n_src_samples * sizeof(float)));
        HIPCHK(hipHostMalloc((void **)&ctx->h_raw, ctx->max_batch * n_src_samples * sizeof(float), hipHostMallocDefault));
        ctx->raw_len = n_src_samples;
    }
    for (size_t b0 = 0; b0 < n; b0 += ctx->max_batch) {
        const size_t nb = std::min(ctx->max_batch, n - b0);
        for (size_t i = 0; i < nb; i++) {
            if (!segments[b0 + i]) return fail(BH_ERR_INVALID, "segment %zu is null", b0 + i);
            memcpy(ctx->h_raw + i * n_src_samples, segments[b0 + i], n_src_samples * sizeof(float));
        }
        HIPCHK(hipMemcpyAsync(ctx->d_raw, ctx->h_raw, nb * n_src_samples * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        // resample_chunk + resize(segment_samples, 0.0) per segment (processor.rs:86-87), on device
        int rc = bh_resample_device(c, ctx, ctx->d_raw, n_src_samples, n_src_samples, source_rate, h.sample_rate,
                                    ctx->d_input, h.sample_count, h.sample_count, nb);
        if (rc != BH_OK) return rc;
        rc = forward_slice(c, ctx, ctx->d_input, nb, ctx->d_logits, ctx->d_topk_idx, ctx->d_topk_conf);
        if (rc != BH_OK) return rc;
        HIPCHK(hipMemcpyAsync(ctx->h_topk_idx, ctx->d_topk_idx, nb * c->top_k * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->h_topk_conf, ctx->d_topk_conf, nb * c->top_k * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(fetch_nonfinite(ctx));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (*ctx->h_nonfinite && c->auto_fallback) {
            bool redone = false;
            const int rr = settle_rows(c, ctx, 0, nb, nullptr, &redone);
            if (rr != BH_OK) return rr;
            clear_nonfinite(ctx);
        }
        for (size_t i = 0; i < nb; i++) {
            bh_result &r = out[b0 + i];
            r.n_pred = 0;
            for (uint32_t k = 0; k < c->top_k; k++) {
                const int32_t id = ctx->h_topk_idx[i * c->top_k + k];
                if (id < 0) break;
                r.index[r.n_pred] = id;
                r.confidence[r.n_pred] = ctx->h_topk_conf[i * c->top_k + k];
                r.n_pred++;
            }
        }
        const int nf = nonfinite_status(c, ctx);
        if (nf != BH_OK) return nf;
    }
    return BH_OK;
} catch (...) { return on_exception(); }

size_t bh_segment_starts(size_t n_frames, size_t segment_samples, size_t overlap_samples, uint64_t *starts, size_t cap) {
    // StreamingDecoder::next_segment over a stream of n_frames (decode.rs:150-202): take = min(seg, left);
    // emit at the running start; advance take - overlap, or stop when that is <= 0 (the buffer is cleared)
    if (overlap_samples >= segment_samples || segment_samples == 0) return 0;
    size_t n = 0, pos = 0;
    while (pos < n_frames) {
        const size_t take = std::min(segment_samples, n_frames - pos);
        if (starts && n < cap) starts[n] = pos;
        n++;
        if (take <= overlap_samples) break;
        pos += take - overlap_samples;
    }
    return n;
}

// (fd >= 0: the stream is bytes [fd_off, ...) of that file and `pcm` is null -- the gather workers pread it into the pinned staging)
static int predict_pcm16_core(bh_classifier *c, bh_batch_context *ctx, const void *pcm, uint32_t fmt, size_t n_frames, uint32_t channels,
                              uint32_t source_rate, const std::vector<uint64_t> &starts, size_t seg, bh_result *out,
                              bh_rows_fn on_rows = nullptr, void *user = nullptr, int fd = -1, uint64_t fd_off = 0);
static inline size_t pcm_bytes_per_sample(uint32_t fmt) { return fmt == BH_PCM_S16 ? 2 : fmt == BH_PCM_S24 ? 3 : (fmt == BH_PCM_S32 || fmt == BH_PCM_F32) ? 4 : 0; }

int bh_predict_pcm16(bh_classifier *c, bh_batch_context *ctx, const int16_t *pcm, size_t n_frames, uint32_t channels,
                     uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap, size_t *n_segments,
                     uint64_t *start_samples) {
    return bh_predict_pcm(c, ctx, pcm, BH_PCM_S16, n_frames, channels, source_rate, overlap_samples, out, out_cap, n_segments, start_samples);
}

int bh_predict_pcm(bh_classifier *c, bh_batch_context *ctx, const void *pcm, uint32_t sample_format, size_t n_frames, uint32_t channels,
                   uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap, size_t *n_segments,
                   uint64_t *start_samples) {
    return bh_predict_pcm_rows(c, ctx, pcm, sample_format, n_frames, channels, source_rate, overlap_samples, out, out_cap, n_segments,
                               start_samples, nullptr, nullptr);
}

static int predict_pcm_rows_any(bh_classifier *c, bh_batch_context *ctx, const void *pcm, int fd, uint64_t fd_off, uint32_t sample_format, size_t n_frames,
                                uint32_t channels, uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap, size_t *n_segments,
                                uint64_t *start_samples, bh_rows_fn on_rows, void *user);

int bh_predict_pcm_rows(bh_classifier *c, bh_batch_context *ctx, const void *pcm, uint32_t sample_format, size_t n_frames, uint32_t channels,
                        uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap, size_t *n_segments,
                        uint64_t *start_samples, bh_rows_fn on_rows, void *user) try {
    if (!pcm) return fail(BH_ERR_INVALID, "predict_pcm: bad arguments");
    return predict_pcm_rows_any(c, ctx, pcm, -1, 0, sample_format, n_frames, channels, source_rate, overlap_samples, out, out_cap, n_segments, start_samples, on_rows, user);
} catch (...) { return on_exception(); }

int bh_predict_pcm_fd_rows(bh_classifier *c, bh_batch_context *ctx, int fd, uint64_t file_offset, uint32_t sample_format, size_t n_frames, uint32_t channels,
                           uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap, size_t *n_segments,
                           uint64_t *start_samples, bh_rows_fn on_rows, void *user) try {
    if (fd < 0) return fail(BH_ERR_INVALID, "predict_pcm_fd: bad file descriptor");
    return predict_pcm_rows_any(c, ctx, nullptr, fd, file_offset, sample_format, n_frames, channels, source_rate, overlap_samples, out, out_cap, n_segments, start_samples, on_rows, user);
} catch (...) { return on_exception(); }

static int predict_pcm_rows_any(bh_classifier *c, bh_batch_context *ctx, const void *pcm, int fd, uint64_t fd_off, uint32_t sample_format, size_t n_frames,
                                uint32_t channels, uint32_t source_rate, size_t overlap_samples, bh_result *out, size_t out_cap, size_t *n_segments,
                                uint64_t *start_samples, bh_rows_fn on_rows, void *user) {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if ((!pcm && fd < 0) || !out || !n_segments || channels == 0 || !pcm_bytes_per_sample(sample_format)) return fail(BH_ERR_INVALID, "predict_pcm: bad arguments");
    const auto &h = c->model.h;
    const bool resampling = source_rate != h.sample_rate;
    if (source_rate == 0) return fail(BH_ERR_INVALID, "predict_pcm: a sample rate of 0");
    if (resampling) {   // the rate pair before a frame of the stream is read or staged
        const int rs = bh_resample_supported(c, source_rate, h.sample_rate);
        if (rs != BH_OK) return rs;
    }
    // segment and overlap lengths at the source rate (processor.rs:67-82)
    const size_t seg = resampling ? (size_t)std::ceil((double)h.sample_count * source_rate / h.sample_rate) : h.sample_count;
    const size_t ovl = resampling ? (size_t)std::ceil((double)overlap_samples * source_rate / h.sample_rate) : overlap_samples;
    if (ovl >= seg) return fail(BH_ERR_INVALID, "overlap (%zu) must be shorter than the segment (%zu)", ovl, seg);
    const size_t nseg = bh_segment_starts(n_frames, seg, ovl, nullptr, 0);
    *n_segments = nseg;
    if (nseg > out_cap) return fail(BH_ERR_INVALID, "predict_pcm16: %zu segments, room for %zu", nseg, out_cap);
    if (nseg == 0) return BH_OK;
    std::vector<uint64_t> starts(nseg);
    bh_segment_starts(n_frames, seg, ovl, starts.data(), nseg);
    if (start_samples) memcpy(start_samples, starts.data(), nseg * sizeof(uint64_t));
    return predict_pcm16_core(c, ctx, pcm, sample_format, n_frames, channels, source_rate, starts, seg, out, on_rows, user, fd, fd_off);
}

int bh_predict_pcm16_at(bh_classifier *c, bh_batch_context *ctx, const int16_t *pcm, size_t n_frames, uint32_t channels,
                        uint32_t source_rate, const uint64_t *start_samples, size_t n_segments, bh_result *out) {
    return bh_predict_pcm_at(c, ctx, pcm, BH_PCM_S16, n_frames, channels, source_rate, start_samples, n_segments, out);
}

int bh_predict_pcm_at(bh_classifier *c, bh_batch_context *ctx, const void *pcm, uint32_t sample_format, size_t n_frames, uint32_t channels,
                      uint32_t source_rate, const uint64_t *start_samples, size_t n_segments, bh_result *out) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if (!pcm || !out || !start_samples || channels == 0 || !pcm_bytes_per_sample(sample_format)) return fail(BH_ERR_INVALID, "predict_pcm_at: bad arguments");
    if (n_segments == 0) return BH_OK;
    const auto &h = c->model.h;
    if (source_rate == 0) return fail(BH_ERR_INVALID, "predict_pcm_at: a sample rate of 0");
    if (source_rate != h.sample_rate) {
        const int rs = bh_resample_supported(c, source_rate, h.sample_rate);
        if (rs != BH_OK) return rs;
    }
    const size_t seg = source_rate != h.sample_rate ? (size_t)std::ceil((double)h.sample_count * source_rate / h.sample_rate) : h.sample_count;
    std::vector<uint64_t> starts(start_samples, start_samples + n_segments);
    for (size_t i = 0; i < n_segments; i++)
        if (starts[i] >= n_frames || (i && starts[i] < starts[i - 1]))
            return fail(BH_ERR_INVALID, "predict_pcm16_at: segment %zu starts at %llu (stream of %zu frames; starts must not decrease)", i,
                        (unsigned long long)starts[i], n_frames);
    return predict_pcm16_core(c, ctx, pcm, sample_format, n_frames, channels, source_rate, starts, seg, out);
} catch (...) { return on_exception(); }

static int predict_pcm16_core(bh_classifier *c, bh_batch_context *ctx, const void *pcm, uint32_t fmt, size_t n_frames, uint32_t channels,
                              uint32_t source_rate, const std::vector<uint64_t> &starts, size_t seg, bh_result *out,
                              bh_rows_fn on_rows, void *user, int fd, uint64_t fd_off) {
    int rc = BH_OK;
    const auto &h = c->model.h;
    const bool resampling = source_rate != h.sample_rate;
    const size_t nseg = starts.size();
    HIPCHK(hipSetDevice(c->device));
    // The stream travels once, as int16 (a quarter of the f32 segments when they overlap by half), slice by
    // slice: worker threads gather 8-MiB pieces of the slice's span into the pinned staging buffer, each
    // piece's H2D copy is enqueued on the copy stream as soon as it is complete, and a sub-slice of
    // segments is cut, resampled and classified as soon as the frames it needs are on their way.
    if (ctx->starts_cap < nseg) {
        (void)hipFree(ctx->d_starts); ctx->d_starts = nullptr; ctx->starts_cap = 0;
        HIPCHK(hipMalloc((void **)&ctx->d_starts, nseg * sizeof(unsigned long long)));
        ctx->starts_cap = nseg;
    }
    HIPCHK(hipMemcpyAsync(ctx->d_starts, starts.data(), nseg * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (resampling && ctx->raw_len < seg) {
        (void)hipFree(ctx->d_raw); (void)hipHostFree(ctx->h_raw);
        ctx->d_raw = nullptr; ctx->h_raw = nullptr; ctx->raw_len = 0;
        if (hipMalloc((void **)&ctx->d_raw, ctx->max_batch * seg * sizeof(float)) != hipSuccess ||
            hipHostMalloc((void **)&ctx->h_raw, ctx->max_batch * seg * sizeof(float), hipHostMallocDefault) != hipSuccess)
            return fail(BH_ERR_HIP, "predict_pcm16: scratch allocation failed");
        ctx->raw_len = seg;
    }
    const size_t frame_bytes = (size_t)channels * pcm_bytes_per_sample(fmt);
    const size_t stage_cap = ctx->max_batch * (size_t)h.sample_count * sizeof(float);   // the pinned input staging buffer
    bool pcm_pinned = false;
    if (pcm) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, pcm) == hipSuccess) pcm_pinned = attr.type == hipMemoryTypeHost;
        else (void)hipGetLastError();
    }
    std::atomic<int> read_failed{0};     // (fd route: a short or failed pread in any worker)
    for (size_t b0 = 0; b0 < nseg; b0 += ctx->max_batch) {
        const size_t nb = std::min(ctx->max_batch, nseg - b0);
        const size_t f0 = starts[b0], f1 = std::min<size_t>(n_frames, starts[b0 + nb - 1] + seg);   // frames of this slice
        const size_t bytes = (f1 - f0) * frame_bytes;
        if (ctx->pcm_cap < bytes) {
            (void)hipFree(ctx->d_pcm); ctx->d_pcm = nullptr; ctx->pcm_cap = 0;
            HIPCHK(hipMalloc((void **)&ctx->d_pcm, bytes));
            ctx->pcm_cap = bytes;
        }
        // the segment kernel indexes the stream by absolute frame: hand it the slice buffer's virtual origin
        const char *d_origin = reinterpret_cast<const char *>(ctx->d_pcm) - f0 * frame_bytes;   // (never dereferenced below frame f0)
        const char *src = reinterpret_cast<const char *>(pcm) + f0 * frame_bytes;
        const bool staged = !pcm_pinned && bytes <= stage_cap;   // (more than two channels: the span can exceed the staging buffer)
        if (fd >= 0 && !staged) return fail(BH_ERR_UNSUPPORTED, "predict_pcm_fd: a slice of %zu bytes exceeds the staging buffer (%zu): hand the stream over mapped instead", bytes, stage_cap);
        char *stage = reinterpret_cast<char *>(ctx->h_input);
        const size_t PIECE = (size_t)8 << 20;
        const size_t npieces = (staged || pcm_pinned) ? (bytes + PIECE - 1) / PIECE : 1;
        const size_t bps = (size_t)((double)bytes / (double)nb);
        const bool can_lane = !resampling && lanes_possible(ctx);   // (the resampler's scratch is one per context)
        std::vector<size_t> cuts = sub_slice_cuts(c, nb, 1, false, bps, can_lane, ctx->forced_sub_slices);
        std::vector<SliceLane> lanes;
        if (can_lane && !lanes_begin(c, ctx, cuts, lanes) && cuts.size() > 1) cuts = sub_slice_cuts(c, nb, 1, false, bps, false, ctx->forced_sub_slices);
        const size_t nsub = cuts.size();
        while (ctx->copy_ev.size() < nsub) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ctx->copy_ev.push_back(e);
        }
        while (ctx->done_ev.size() < nsub) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ctx->done_ev.push_back(e);
        }
        // (every worker its share of every piece, piece after piece: the first piece is on the copy stream at once; see predict_slices)
        // (workers from 1 MB on -- a one-minute file is 1.9 MB of PCM16, 0.16 ms on one thread out of the 0.95 its whole call lasts:
        //  one file at a time 18.2 -> 21.7 k segments/s with BH_FLAG_LOW_LATENCY; round 5's threshold was 16 MB)
        const unsigned nthreads = (staged && bytes >= ((size_t)1 << 20)) ? copy_threads() : 1;
        std::vector<std::atomic<int>> done(npieces);
        for (auto &d : done) d.store(0, std::memory_order_relaxed);
        auto gather_part = [&](size_t j, unsigned t, unsigned nt) {
            const size_t o = j * PIECE, len = std::min(PIECE, bytes - o);
            const size_t share = ((len + nt - 1) / nt + 4095) & ~(size_t)4095, a = std::min(len, (size_t)t * share), b = std::min(len, a + share);
            if (b <= a) return;
            if (fd >= 0) {
                // the file's bytes straight into the pinned staging buffer: one copy out of the page cache, no mapping, no faults
                // (round 6; the mapped route copies the same bytes behind 70 000 minor faults a 1 000-segment file)
                size_t got = 0;
                while (got < b - a) {
                    const ssize_t r = pread(fd, stage + o + a + got, b - a - got, (off_t)(fd_off + f0 * frame_bytes + o + a + got));
                    if (r <= 0) { if (r < 0 && errno == EINTR) continue; read_failed.store(1, std::memory_order_relaxed); return; }
                    got += (size_t)r;
                }
            } else bh_internal_stream_copy(stage + o + a, src + o + a, b - a);
        };
        if (nthreads > 1) {
            if (!ctx->pool) ctx->pool.reset(new GatherPool());
            ctx->pool->start(nthreads - 1, [&](unsigned t) {
                for (size_t j = 0; j < npieces; j++) { gather_part(j, t, nthreads); done[j].fetch_add(1, std::memory_order_release); }
            });
        }
        size_t si = 0;   // next sub-slice to launch
        rc = BH_OK;
        for (size_t j = 0; j < npieces && rc == BH_OK; j++) {
            size_t sent;   // bytes of the span on the copy stream after this piece
            if (staged) {
                gather_part(j, 0, nthreads);     // (the calling thread is worker 0)
                if (nthreads > 1) while (done[j].load(std::memory_order_acquire) < (int)nthreads - 1) std::this_thread::yield();
                if (read_failed.load(std::memory_order_relaxed)) { rc = fail(BH_ERR_IO, "predict_pcm_fd: the file ended or could not be read inside the stream"); break; }
                const size_t o = j * PIECE, len = std::min(PIECE, bytes - o);
                if (hipMemcpyAsync(reinterpret_cast<char *>(ctx->d_pcm) + o, stage + o, len, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess)
                    { rc = fail(BH_ERR_HIP, "predict_pcm16: upload failed"); break; }
                sent = o + len;
            } else if (pcm_pinned) {   // pinned caller memory (bh_host_alloc / bh_host_register): piece by piece straight from it
                const size_t o = j * PIECE, len = std::min(PIECE, bytes - o);
                if (hipMemcpyAsync(reinterpret_cast<char *>(ctx->d_pcm) + o, src + o, len, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess)
                    { rc = fail(BH_ERR_HIP, "predict_pcm16: upload failed"); break; }
                sent = o + len;
            } else {
                if (hipMemcpyAsync(ctx->d_pcm, src, bytes, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess)
                    { rc = fail(BH_ERR_HIP, "predict_pcm16: upload failed"); break; }
                sent = bytes;
            }
            const size_t frames_sent = f0 + sent / frame_bytes;
            while (si < nsub && rc == BH_OK) {
                const size_t s0 = si ? cuts[si - 1] : 0, ns = cuts[si] - s0;
                const size_t need = std::min<size_t>(n_frames, starts[b0 + s0 + ns - 1] + seg);
                if (need > frames_sent && sent < bytes) break;   // its last frames are not on their way yet
                const SliceLane *lane = lanes.empty() ? nullptr : &lanes[si];
                hipStream_t ls = lane ? lane->s : ctx->stream;
                if (hipEventRecord(ctx->copy_ev[si], ctx->copy_stream) != hipSuccess ||
                    hipStreamWaitEvent(ls, ctx->copy_ev[si], 0) != hipSuccess) { rc = fail(BH_ERR_HIP, "stream event failed"); break; }
                float *d_in = ctx->d_input + s0 * h.sample_count;
                if (resampling) {
                    float *d_rw = ctx->d_raw + s0 * seg;
                    bh::launch_segment_pcm(d_origin, (int)fmt, n_frames, (int)channels, ctx->d_starts + b0 + s0, (int)ns, (int)seg, d_rw, seg, ctx->stream);
                    rc = bh_resample_device(c, ctx, d_rw, seg, seg, source_rate, h.sample_rate, d_in, h.sample_count, h.sample_count, ns);
                    if (rc != BH_OK) break;
                } else {
                    bh::launch_segment_pcm(d_origin, (int)fmt, n_frames, (int)channels, ctx->d_starts + b0 + s0, (int)ns, (int)seg, d_in, seg, ls);
                }
                rc = forward_slice(c, ctx, d_in, ns, ctx->d_logits + s0 * h.n_classes, ctx->d_topk_idx + s0 * c->top_k,
                                   ctx->d_topk_conf + s0 * c->top_k, lane);
                // the sub-slice's rows follow its forward down the same stream: they are on the host -- and handed to the caller,
                // below -- while the later sub-slices are still being computed
                if (rc == BH_OK &&
                    (hipMemcpyAsync(ctx->h_topk_idx + s0 * c->top_k, ctx->d_topk_idx + s0 * c->top_k, ns * c->top_k * sizeof(int32_t), hipMemcpyDeviceToHost, ls) != hipSuccess ||
                     hipMemcpyAsync(ctx->h_topk_conf + s0 * c->top_k, ctx->d_topk_conf + s0 * c->top_k, ns * c->top_k * sizeof(float), hipMemcpyDeviceToHost, ls) != hipSuccess ||
                     hipEventRecord(ctx->done_ev[si], ls) != hipSuccess))
                    rc = fail(BH_ERR_HIP, "predict_pcm16: result download failed");
                si++;
            }
        }
        if (nthreads > 1) ctx->pool->wait();
        if (rc == BH_OK && lanes_end(ctx, lanes) != hipSuccess) rc = fail(BH_ERR_HIP, "stream event failed");
        if (rc != BH_OK) {
            (void)hipStreamSynchronize(ctx->copy_stream); lanes_sync(ctx); (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
        if (fetch_nonfinite(ctx) != hipSuccess) return fail(BH_ERR_HIP, "predict_pcm16: result download failed");
        bool poisoned = false;   // a sub-slice with marked rows and no BH_FLAG_AUTO: its rows and the later ones are not handed out
        for (size_t sj = 0; sj < nsub; sj++) {
            const size_t s0 = sj ? cuts[sj - 1] : 0, ns = cuts[sj] - s0;
            if (hipEventSynchronize(ctx->done_ev[sj]) != hipSuccess) {
                lanes_sync(ctx); (void)hipStreamSynchronize(ctx->stream);
                return fail(BH_ERR_HIP, "predict_pcm16: result download failed");
            }
            // Rows the top-k stage marked (logits inf / NaN from finite samples: an activation left the f16 range) are looked for
            // BEFORE the sub-slice's rows go to the caller: BH_FLAG_AUTO re-runs them on the f32 kernels here; otherwise nothing
            // from this sub-slice on is delivered and the call ends in BH_ERR_NONFINITE (what was delivered before is valid).
            bool marked = false;
            for (size_t i = s0; i < s0 + ns && !marked; i++) marked = ctx->h_topk_idx[i * c->top_k] == BH_TOPK_NONFINITE;
            if (marked && c->auto_fallback) {
                bool redone = false;
                const int rr = settle_rows(c, ctx, s0, ns, nullptr, &redone);
                if (rr != BH_OK) { lanes_sync(ctx); (void)hipStreamSynchronize(ctx->stream); clear_nonfinite(ctx); return rr; }
            } else if (marked) poisoned = true;
            for (size_t i = s0; i < s0 + ns; i++) {
                bh_result &r = out[b0 + i];
                r.n_pred = 0;
                for (uint32_t k = 0; k < c->top_k; k++) {
                    const int32_t id = ctx->h_topk_idx[i * c->top_k + k];
                    if (id < 0) break;
                    r.index[r.n_pred] = id;
                    r.confidence[r.n_pred] = ctx->h_topk_conf[i * c->top_k + k];
                    r.n_pred++;
                }
            }
            if (on_rows && !poisoned) on_rows(user, b0 + s0, ns, out + b0 + s0, starts.data() + b0 + s0);
        }
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(BH_ERR_HIP, "predict_pcm16: result download failed");
        if (c->auto_fallback && *ctx->h_nonfinite) clear_nonfinite(ctx);   // (every marked row was re-run above)
        const int nf = nonfinite_status(c, ctx);
        if (nf != BH_OK) return nf;
    }
    return BH_OK;
}

// Diagnostic (include/birda_hip_pcm_debug.h): what the last slice of the last bh_predict_pcm* call left in d_input (which 0) or
// d_raw (which 1), read back as it lies; nothing of the product path passes through here.
int bh_debug_read_segments(bh_classifier *c, bh_batch_context *ctx, int which, float *host, size_t rows, size_t row_floats) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if (!host) return fail(BH_ERR_INVALID, "read_segments: null host buffer");
    if (which != 0 && which != 1) return fail(BH_ERR_INVALID, "read_segments: which = %d (0: model-rate input, 1: raw source-rate rows)", which);
    if (rows == 0 || rows > ctx->max_batch) return fail(BH_ERR_INVALID, "read_segments: %zu rows, the context holds %zu", rows, ctx->max_batch);
    const float *src;
    if (which == 0) {
        if (row_floats != c->model.h.sample_count)
            return fail(BH_ERR_INVALID, "read_segments: rows of %zu floats, the model's input has %u", row_floats, c->model.h.sample_count);
        src = ctx->d_input;
    } else {
        if (!ctx->d_raw || ctx->raw_len == 0) return fail(BH_ERR_INVALID, "read_segments: no resampling call has run on this context: there are no raw rows");
        if (row_floats == 0 || row_floats > ctx->raw_len)
            return fail(BH_ERR_INVALID, "read_segments: raw rows of %zu floats, the raw buffer's rows hold %zu", row_floats, ctx->raw_len);
        src = ctx->d_raw;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(ctx->copy_stream));
    lanes_sync(ctx);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(host, src, rows * row_floats * sizeof(float), hipMemcpyDeviceToHost));
    return BH_OK;
} catch (...) { return on_exception(); }
}  // extern "C"

namespace bhi {
// What launch_resample and its kernels take as int: a row's lengths, and the segment count that becomes the grid's z dimension.
// Looks at the numbers alone -- called before a buffer is allocated, copied or read.
int resample_ranges(const char *who, size_t src_len, size_t out_len, size_t n_seg) {
    if (src_len > (size_t)INT32_MAX || out_len > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "%s: %zu source samples -> %zu outputs a segment: the resampler indexes a row with 32-bit integers (2^31 - 1 at most)",
                    who, src_len, out_len);
    if (n_seg > 65535)
        return fail(BH_ERR_INVALID, "%s: %zu segments in one launch: the grid's z dimension takes 65 535 at most", who, n_seg);
    return BH_OK;
}
}  // namespace bhi

extern "C" {

int bh_resample_output_len(size_t n_in, uint32_t from_rate, uint32_t to_rate, size_t *n_out) try {
    if (!n_out || from_rate == 0 || to_rate == 0) return fail(BH_ERR_INVALID, "resample_output_len: bad arguments");
    *n_out = bh::resample_output_len(n_in, from_rate, to_rate);
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_resample_supported(bh_classifier *c, uint32_t from_rate, uint32_t to_rate) try {
    if (!c || from_rate == 0 || to_rate == 0) return fail(BH_ERR_INVALID, "resample_supported: bad arguments");
    if (from_rate == to_rate) return BH_OK;
    HIPCHK(hipSetDevice(c->device));
    const char *err = nullptr;
    if (!bh::resample_plan(from_rate, to_rate, &err)) return fail(BH_ERR_UNSUPPORTED, "%s (%u -> %u Hz)", err ? err : "resampler", from_rate, to_rate);
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_resample_device(bh_classifier *c, bh_batch_context *ctx, const float *d_in, size_t in_stride, size_t src_len,
                       uint32_t from_rate, uint32_t to_rate, float *d_out, size_t out_stride, size_t out_len,
                       size_t n_seg) try {
    int rc = check_ctx(c, ctx);
    if (rc != BH_OK) return rc;
    if (!d_in || !d_out || from_rate == 0 || to_rate == 0 || src_len > in_stride || out_len > out_stride)
        return fail(BH_ERR_INVALID, "resample_device: bad arguments");
    // (equal rates are a strided copy of any row count; the lengths are refused alike, so that a caller meets one rule)
    if ((rc = resample_ranges("resample_device", src_len, out_len, from_rate == to_rate ? 0 : n_seg)) != BH_OK) return rc;
    if (n_seg == 0) return BH_OK;
    HIPCHK(hipSetDevice(c->device));
    if (from_rate == to_rate) {  // resample.rs:11-13: identity; then resize(segment_samples, 0.0)
        const size_t ncopy = std::min(src_len, out_len);
        HIPCHK(hipMemcpy2DAsync(d_out, out_stride * sizeof(float), d_in, in_stride * sizeof(float), ncopy * sizeof(float),
                                n_seg, hipMemcpyDeviceToDevice, ctx->stream));
        if (out_len > ncopy)
            HIPCHK(hipMemset2DAsync(d_out + ncopy, out_stride * sizeof(float), 0, (out_len - ncopy) * sizeof(float), n_seg,
                                    ctx->stream));
        return BH_OK;
    }
    const char *err = nullptr;
    const bh::ResamplePlan *pl = bh::resample_plan(from_rate, to_rate, &err);
    if (!pl) return fail(BH_ERR_UNSUPPORTED, "%s (%u -> %u Hz)", err ? err : "resampler", from_rate, to_rate);
    bh::launch_resample(*pl, d_in, in_stride, (int)src_len, d_out, out_stride, (int)out_len, (int)n_seg,
                        c->precision != 0, ctx->stream);
    HIPCHK(hipGetLastError());
    return BH_OK;
} catch (...) { return on_exception(); }

int bh_resample(bh_classifier *c, const float *in, size_t n_in, uint32_t from_rate, uint32_t to_rate, float *out,
                size_t out_cap, size_t *n_out) try {
    if (!c || !in || !out || !n_out) return fail(BH_ERR_INVALID, "resample: null argument");
    if (from_rate == 0 || to_rate == 0) return fail(BH_ERR_INVALID, "resample: a sample rate of 0");   // (was a division by zero: tools/fuzz_args.py)
    const size_t need = bh::resample_output_len(n_in, from_rate, to_rate);
    if (need > out_cap) return fail(BH_ERR_INVALID, "resample: output buffer too small (%zu < %zu)", out_cap, need);
    int rrc = resample_ranges("resample", n_in, need, 1);
    if (rrc != BH_OK) return rrc;
    *n_out = need;
    if (need == 0) return BH_OK;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->internal_mu);
    bh_batch_context *ctx = nullptr;
    int rc = internal_ctx(c, 1, &ctx);
    if (rc != BH_OK) return rc;
    float *d_in = nullptr, *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_in, n_in * sizeof(float)));
    if (hipMalloc((void **)&d_out, need * sizeof(float)) != hipSuccess) { (void)hipFree(d_in); return fail(BH_ERR_HIP, "resample: hipMalloc failed"); }
    rc = BH_OK;
    if (hipMemcpyAsync(d_in, in, n_in * sizeof(float), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = fail(BH_ERR_HIP, "resample: H2D failed");
    if (rc == BH_OK) rc = bh_resample_device(c, ctx, d_in, n_in, n_in, from_rate, to_rate, d_out, need, need, 1);
    if (rc == BH_OK && hipMemcpyAsync(out, d_out, need * sizeof(float), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(BH_ERR_HIP, "resample: D2H failed");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == BH_OK) rc = fail(BH_ERR_HIP, "resample: stream sync failed");
    (void)hipFree(d_in); (void)hipFree(d_out);
    return rc;
} catch (...) { return on_exception(); }

}  // extern "C"
