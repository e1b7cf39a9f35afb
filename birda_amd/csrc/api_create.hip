// api_create.hip -- bh_classifier_create, phase by phase, and the destructor that undoes it.  The new classifier lives in a unique_ptr
// until the last phase is through: whatever a phase refuses or fails at, ~bh_classifier releases what the phases before it took.
#include "api_internal.hpp"

using namespace bhi;

// The one place a classifier's device memory and streams are released, a half-built classifier's too (null pointers, streams not
// yet created).  Contexts and the fallback classifier go first: their destructors drain the streams they hold, which are this one's.
bh_classifier::~bh_classifier() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    delete fb;
    delete internal_ctx;
    for (bh_batch_context *p : parked_ctx) delete p;
    for (auto &ss : stream_sets)
        for (auto &st : ss.s) if (st) (void)hipStreamDestroy(st);
    for (float *d : d_owned) (void)hipFree(d);
    (void)hipFree(d_class_score); (void)hipFree(d_species_keep); (void)hipFree(d_bsg);
}

namespace {

// Phase 1: the model file, the labels, the device and its streams, the GEMM operand precision.
int configure(const bh_config *cfg, bh_classifier *c) {
    std::string err;
    if (!load_any_model(cfg->model_path, c->model, err)) return fail(model_load_status(err), "%s", err.c_str());
    const auto &m = c->model;
    static_assert(BH_MAX_CLASSES == bh::TOPK_MAX_CLASSES, "the documented class-count ceiling is the top-k kernel's row");
    if (m.h.n_classes > BH_MAX_CLASSES)   // (before anything touches a device: the top-k launch would fail with a bare HIP error)
        return fail(BH_ERR_UNSUPPORTED, "the model has %u classes: the activation / top-k stage holds at most %d (a segment's logits in 128 KB of LDS)",
                    m.h.n_classes, BH_MAX_CLASSES);
    if (cfg->labels_path) {
        int rc = read_labels(cfg->labels_path, c->labels);
        if (rc != BH_OK) return rc;
        if (c->labels.size() != m.h.n_classes)
            return fail(BH_ERR_LABELS, "label count %zu does not match model output width %u", c->labels.size(), m.h.n_classes);
    }
    int ndev = bh_device_count();
    if (ndev <= 0) return fail(BH_ERR_NO_DEVICE, "no HIP device available (libbirda_hip has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(BH_ERR_NO_DEVICE, "device %d out of range (0..%d)", cfg->device, ndev - 1);
    c->device = cfg->device;
    c->top_k = cfg->top_k;
    c->min_conf = cfg->min_confidence;
    HIPCHK(hipSetDevice(c->device));
    for (auto &ss : c->stream_sets)          // the batch contexts' streams, all of them now (api_internal.hpp)
        for (auto &st : ss.s) HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (m.h.n_branches > bh::MAX_BRANCHES) return fail(BH_ERR_UNSUPPORTED, "too many front-end branches");
    // GEMM operand precision (decided here: the front-end operator layout depends on it)
    const uint32_t pf = cfg->flags & BH_FLAG_PRECISION_MASK;
    c->precision = pf == BH_FLAG_F32 ? 0 : pf == BH_FLAG_F16 ? 1 : 3;
    c->auto_fallback = pf == BH_FLAG_AUTO;
    c->low_latency = (cfg->flags & BH_FLAG_LOW_LATENCY) != 0;
    c->full_planes = (cfg->flags & BH_FLAG_FULL_PLANES) != 0;
    c->model_path = cfg->model_path;
    if (const char *pe = (cfg->flags & FLAG_INTERNAL_NO_ENV) ? nullptr : getenv("BIRDA_HIP_PRECISION")) {
        if (!strcmp(pe, "f32")) { c->precision = 0; c->auto_fallback = false; }
        else if (!strcmp(pe, "f16x3")) { c->precision = 3; c->auto_fallback = false; }
        else if (!strcmp(pe, "auto")) { c->precision = 3; c->auto_fallback = true; }
        else if (!strcmp(pe, "f16")) { c->precision = 1; c->auto_fallback = false; }
        else return fail(BH_ERR_INVALID, "BIRDA_HIP_PRECISION must be auto, f32, f16x3 or f16");
    }
    return BH_OK;
}

// Phase 2: the folded STFT x mel operator of every branch and the parameter block the mel kernel reads (f32-grade products in every
// mode: f32 MFMA, or split f16 in the f16 modes).
int build_front_end(bh_classifier *c) {
    const auto &m = c->model;
    // f16x3 and f16: the front-end GEMM on the split-f16 MFMA (f32-grade products, faster than the f32 MFMA;
    // BIRDA_HIP_MEL_F32=1 keeps it on the f32 MFMA: A/B aid)
    int fe_prec = (c->precision != 0 && !(getenv("BIRDA_HIP_MEL_F32") && getenv("BIRDA_HIP_MEL_F32")[0] == '1')) ? 3 : 0;
    for (uint32_t b = 0; b < m.h.n_branches; b++)
        if (m.branches[b].frame_length % 256) fe_prec = 0;   // 32-deep steps split over 4 waves
    if (fe_prec == 3) {
        // mel32_kernel (Y rows staged along k: no LDS bank conflicts whatever the hop) where mel_kernel's frame-strided
        // reads collapse onto a few banks: hops that are multiples of 16 samples (Perch: 320 -> every frame on one bank;
        // 483 -> 258 us per 600 segments).  BirdNET's hops (278 / 280) stay on mel_kernel (790 vs 1006 us per 1000).
        // BIRDA_HIP_MEL32=0/1 forces the choice (A/B aid).
        bool want = false, can = true;
        for (uint32_t b = 0; b < m.h.n_branches; b++) {
            if (m.branches[b].frame_step % 16 == 0) want = true;
            if (align_up(m.branches[b].n_mels, 16) % 32 || m.branches[b].frame_length % 512) can = false;   // 32-mel tiles, 64-k chunks per wave
        }
        if (const char *e = getenv("BIRDA_HIP_MEL32")) want = e[0] == '1';
        if (want && can) fe_prec = 32;
    }
    if (m.h.sample_count % 4) return fail(BH_ERR_UNSUPPORTED, "front-end: sample_count %u must be a multiple of 4 (16-byte span loads)", m.h.sample_count);
    c->fe.prec = fe_prec;
    c->fe.n_branches = (int)m.h.n_branches;
    c->fe.sample_count = (int)m.h.sample_count;
    c->fe.norm_eps = m.h.norm_eps;
    for (uint32_t b = 0; b < m.h.n_branches; b++) {
        const auto &br = m.branches[b];
        const int nm_pad = (int)align_up(br.n_mels, 16);
        if (nm_pad < 32 || nm_pad > 128)
            return fail(BH_ERR_UNSUPPORTED, "front-end: n_mels %u not built (17 .. 128)", br.n_mels);
        if (b > 0 && nm_pad != c->fe.br[0].nm_pad) return fail(BH_ERR_UNSUPPORTED, "front-end: branches differ in n_mels");
        if (br.frame_length % 128 || br.fft_length != br.frame_length)
            return fail(BH_ERR_UNSUPPORTED, "front-end: frame_length %u must be a multiple of 128 and equal fft_length", br.frame_length);
        // (no condition on the hop: a tile's span starts at sample tile * 48 (or 32) * hop, a multiple of 4 for any hop, so the
        //  16-byte span loads stay aligned; what bounds the hop is the span's size, checked against the LDS below)
        int gf_s = 0;
        const std::vector<float> gf = build_gf(br, m.blob.data() + br.mel_w_off, nm_pad, fe_prec, &gf_s);
        auto &p = c->fe.br[b];
        int rc = upload_owned(c->d_owned, gf.data(), gf.size() * sizeof(float), &p.gf);
        if (rc != BH_OK) return rc;
        p.L = (int)br.frame_length; p.H = (int)br.frame_step; p.K = p.L / 2;
        p.n_mels = (int)br.n_mels; p.nm_pad = nm_pad; p.n_frames = (int)br.n_frames;
        p.expo = 1.0f / (1.0f + expf(br.mag_scale));
        p.log2_bias = -2.0f * (float)gf_s * p.expo;
        p.out_scale = br.out_scale; p.out_shift = br.out_shift; p.flip = (int)(br.flags & 1u);
        c->mel_flops += 2ull * (uint64_t)p.K * nm_pad * br.n_frames;
    }
    if (bh::mel_lds_bytes(c->fe) > 160 * 1024)
        return fail(BH_ERR_UNSUPPORTED, "front-end: a tile of frames at this hop and frame length spans %zu KB of samples, more than a CU's 160 KB of LDS",
                    bh::mel_lds_bytes(c->fe) / 1024);
    return upload_owned(c->d_owned, &c->fe, sizeof c->fe, &c->d_fe);
}

// Phase 3, one layer: refused where no kernel is built for its shape; its f32 weights as its kernel reads them (every mode: the
// BIRDA_HIP_KEEP_TENSORS contexts and the BH_FLAG_AUTO re-run land there); in the f16 modes its operand planes.  in_block: the layer
// is inside a fused block, whose launch carries its own weights (plan_fusion); se_project: it is the project convolution of a fused
// squeeze-excite block, which runs outside the block's launch, on the gated GEMM.
int prepare_layer(bh_classifier *c, size_t i, bool in_block, bool se_project) {
    const auto &m = c->model;
    const auto &L = m.layers[i];
    LayerState &S = c->layer[i];
    const float *W = m.blob.data() + L.w_off;
    const bh::ConvParams p = conv_params(L);
    const bool f16 = c->precision != 0;
    S.w = c->d_blob + L.w_off;
    auto own_rows = [&](const std::vector<float> &w) { return upload_owned(c->d_owned, w.data(), w.size() * sizeof(float), &S.w); };
    // Two-term products: decided by the data, per layer -- a layer whose lo plane is all zero AFTER BatchNormalization folding and
    // the power-of-two pre-scale (a float16 model file's weights, or f16 values in any container) runs TERMS == 2 on compact planes,
    // half the bytes; every other layer, and every layer under BH_FLAG_FULL_PLANES, BH_FLAG_F16 or BH_FLAG_F32, is what it was.
    auto own_planes = [&](const float *w, int K, int N, bool may_compact) {
        bool lo_zero = false;
        std::vector<uint16_t> planes = w16_planes(w, K, N, &S.unscale, &lo_zero);
        S.terms = c->precision == 3 ? 3 : 1;
        if (may_compact && c->precision == 3 && lo_zero && !c->full_planes) { planes = w16_compact(planes); S.terms = 2; }
        S.plane_bytes = planes.size() * sizeof(uint16_t);
        return upload_owned(c->d_owned, planes.data(), S.plane_bytes, &S.planes);
    };
    switch (L.op) {
    case bh::OP_PWCONV: case bh::OP_DENSE: {
        if (L.cin % 4) return fail(BH_ERR_UNSUPPORTED, "layer %zu: cin %u not a multiple of 4", i, L.cin);
        S.ldw = (int)align_up(L.cout, 4);
        if (S.ldw != (int)L.cout) {  // pad rows so 16-B loads stay aligned
            const int rc = own_rows(pw_gemm_rows(W, L.cin, L.cout, (size_t)S.ldw));
            if (rc != BH_OK) return rc;
        }
        if (!f16 || in_block) return BH_OK;
        // (activation after the add: the AFTER instantiations' activations, and the full convolutions' width rule -- 64 output
        //  channels or fewer stay on the f32 MFMA -- so that the end of a ResNet block runs where its 3x3 twin would)
        // (a squeeze-excite block's project convolution: the gated GEMM takes planes of ANY K % 4 == 0, zero-padded to whole 32-deep
        //  steps; the block's gate layers run in se_gate_kernel on f32 weights as they are)
        const bool takes = res_act_after(L) ? bh::pw_gemm16_after_supports((int)L.cin, (int)L.act) && L.cout > 64
                         : se_project       ? L.cin % 4 == 0 && L.act == bh::ACT_NONE
                                            : bh::pw_gemm16_supports((int)L.cin, (int)L.act);
        return takes ? own_planes(W, (int)L.cin, (int)L.cout, true) : (int)BH_OK;
    }
    case bh::OP_DWCONV:
        if (!bh::dwconv_supports(p))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: depthwise %ux%u stride %u dilation %dx%d channels %u not built", i, L.kh, L.kw, L.sh, p.dil_h, p.dil_w, L.cout);
        return BH_OK;
    case bh::OP_CONV: {
        if (L.in_layout == 1) {   // the NCHW stem: the direct kernel, weights in LDS
            if (bh::conv_dilated(p)) return fail(BH_ERR_UNSUPPORTED, "layer %zu: dilation %dx%d on the NCHW stem convolution is not built", i, p.dil_h, p.dil_w);
            if (!bh::conv_direct_supports(p)) return fail(BH_ERR_UNSUPPORTED, "layer %zu: direct conv shape not built", i);
            return BH_OK;
        }
        // NHWC: the implicit GEMM, W rows padded per tap to whole 32-deep steps
        if (!bh::conv_gemm_supports(p))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: full convolution %ux%u stride %ux%u dilation %dx%d, %u -> %u channels, layout %u not built "
                        "(kernel 1..7, stride 1 / 2, dilation 1..16, channels multiples of 4, NHWC)", i, L.kh, L.kw, L.sh, L.sw, p.dil_h, p.dil_w, L.cin, L.cout, L.in_layout);
        S.ldw = (int)align_up(L.cout, 4);
        const int rc = own_rows(conv_gemm_rows(W, p, S.ldw));
        if (rc != BH_OK) return rc;
        // planes over the per-tap padded K (64 output channels or fewer stay on the f32 MFMA: the split-f16 kernel's 128-column tile
        //  would idle half or more of its MFMAs there, and the f32 kernel is the faster -- 1.08 against 2.22 ms for 3x3 32 -> 32 at
        //  64 x 249 x 256 segments, profiles/conv_gemm.txt -- and exact; shapes alone decide)
        //  (a layer with its activation after the add: the same rule, over the activations THAT form is instantiated for)
        if (!f16 || !(res_act_after(L) ? bh::conv_gemm16_after_supports(p) : bh::conv_gemm16_supports(p)) || L.cout <= 64) return BH_OK;
        const uint32_t cpad = (uint32_t)align_up(L.cin, 32);
        return own_planes(conv_gemm_rows(W, p, (int)L.cout).data(), (int)(L.kh * L.kw * cpad), (int)L.cout, true);
    }
    case bh::OP_GCONV: {   // per-tile weight blocks: f32 MFMA fragments, and planes over the per-tile K
        if (!bh::gconv_supports(p, (int)L.reserved))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: grouped convolution %ux%u stride %ux%u, %u -> %u channels in %u groups not built "
                        "(kernel 1..7, stride 1 / 2, group widths multiples of 4, NHWC, no residual)", i, L.kh, L.kw, L.sh, L.sw, L.cin, L.cout, L.reserved);
        int K = 0;
        const std::vector<float> wt = gconv_matrix(W, p, (int)L.reserved, &K);
        const int rc = own_rows(gconv_fragments(wt, K, (int)(L.cout + 15) / 16));
        if (rc != BH_OK || !f16) return rc;
        // (three terms -- f16x3 / auto, a float16 file included -- or one, never two)
        return own_planes(wt.data(), K, (int)((L.cout + 15) / 16 * 16), false);
    }
    case bh::OP_GAP: case bh::OP_SCALE: case bh::OP_POOL:
        if (L.cout % 4) return fail(BH_ERR_UNSUPPORTED, "layer %zu: channels %u not a multiple of 4", i, L.cout);
        if (L.op == bh::OP_POOL && !bh::pool_supports(p, (int)L.reserved))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: pool %ux%u stride %ux%u pad %u,%u mode %u not built", i, L.kh, L.kw, L.sh, L.sw, L.pad_t, L.pad_l, L.reserved);
        return BH_OK;
    case bh::OP_LNORM:   // (validate_model has held the record; the kernel's width range is create's rule)
        if (!bh::lnorm_supports((int)L.cout))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: layer norm over %u channels not built (a multiple of 4, 4 .. 2048)", i, L.cout);
        return BH_OK;
    case bh::OP_REDUCE:   // (validate_model has held the record: the launcher takes what it accepts)
        if (!bh::reduce_supports(p, (int)L.reserved))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: reduce of a %ux%u image over a %ux%u window, %u channels, mode %u not built", i, L.in_h, L.in_w, L.kh, L.kw, L.cout, L.reserved);
        return BH_OK;
    case bh::OP_BNACT:   // (the op needs nothing but the blob: what validate_model accepts, the launcher takes)
        if (!bh::bnact_supports((int)L.cout, (int)L.act))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: norm + activation over %u channels with activation %u not built", i, L.cout, L.act);
        return BH_OK;
    case bh::OP_CONCAT: {
        const auto src = concat_sources(m, L, nullptr, nullptr);
        if (!bh::concat_supports((int)L.out_h, (int)L.out_w, src.data(), L.res_tensor == bh::NO_TENSOR ? 1 : 2, (int)L.reserved))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: concat of channels %llu + %u and %llu + %u into %u (shuffle groups %u) on a %ux%u image not built "
                        "(offsets and lengths multiples of 4, inside their sources; groups dividing the channels)", i, (unsigned long long)L.w_off, L.cin,
                        (unsigned long long)L.b_off, L.cout - L.cin, L.cout, L.reserved, L.out_h, L.out_w);
        return BH_OK;
    }
    default: return BH_OK;
    }
}

// Phase 3: every layer, then what is asked of the stack as a whole.
int prepare_layers(bh_classifier *c) {
    const auto &m = c->model;
    std::vector<char> in_block(m.layers.size(), 0), se_project(m.layers.size(), 0);
    for (size_t i = 0; i < m.layers.size(); i++)
        if (c->layer[i].fused_at >= 0) {
            const bh::MbDesc &d = c->mb[c->layer[i].fused_at];
            const size_t last = fused_block_last(i, d);
            for (size_t k = i; k <= last; k++) in_block[k] = 1;
            if (d.se) { in_block[last] = 0; se_project[last] = 1; }
        }
    for (size_t i = 0; i < m.layers.size(); i++) {
        const int rc = prepare_layer(c, i, in_block[i] != 0, se_project[i] != 0);
        if (rc != BH_OK) return rc;
    }
    if (m.layers.empty() || m.layers.back().cout != m.h.n_classes)
        return fail(BH_ERR_IO, "model: last layer width != n_classes");
    // (an OP_CONCAT record's res_tensor is its second input, not a residual: the check below does not look at it)
    // a residual on a layer whose kernel cannot add one is refused, not dropped: depthwise and pool layers (a fused block's
    // residual sits on its project convolution; the planner fuses no depthwise layer that carries one) and the NCHW stem
    for (size_t i = 0; i < m.layers.size(); i++) {
        const auto &L = m.layers[i];
        if (L.res_tensor != bh::NO_TENSOR && (L.op == bh::OP_DWCONV || L.op == bh::OP_GAP || L.op == bh::OP_POOL || L.op == bh::OP_REDUCE || L.op == bh::OP_BNACT || L.op == bh::OP_GCONV || (L.op == bh::OP_CONV && L.in_layout == 1)))
            return fail(BH_ERR_UNSUPPORTED, "layer %zu: a residual on a %s layer is not supported (only convolutions, 1x1 and full NHWC, "
                        "and dense layers add one)", i, L.op == bh::OP_DWCONV ? "depthwise" : (L.op == bh::OP_GAP || L.op == bh::OP_POOL) ? "pool" : L.op == bh::OP_REDUCE ? "reduce" : L.op == bh::OP_BNACT ? "norm + activation"
                                                        : L.op == bh::OP_GCONV ? "grouped convolution" : "stem convolution");
    }
    return BH_OK;
}

// Phase 5: the launches that stand for several layers outside the fused blocks, marked on their first layer.
void mark_paths(bh_classifier *c) {
    const auto &m = c->model;
    const char *hg = getenv("BIRDA_HIP_HEAD_GAP");
    for (size_t i = 0; i < m.layers.size(); i++) {
        LayerState &S = c->layer[i];
        S.gap_gate = gap_gate_chain(m, i) ? 1 : 0;
        S.concat_chain = (char)concat_chain_len(m, i);
        // head conv + GELU followed by the global average pool (and read by nothing else): one launch
        if (i + 1 >= m.layers.size() || (hg && hg[0] == '0')) continue;
        const auto &L = m.layers[i], &G = m.layers[i + 1];
        if (!S.planes || L.op != bh::OP_PWCONV || L.res_tensor != bh::NO_TENSOR || G.op != bh::OP_GAP ||
            G.in_tensor != i + 1 || !bh::head_gap16_supports((int)(L.out_h * L.out_w), (int)L.cin, (int)L.cout, (int)L.act))
            continue;
        bool other_reader = m.h.embedding_tensor == i + 1;
        for (size_t j = 0; j < m.layers.size(); j++)
            if (j != i + 1 && (m.layers[j].in_tensor == i + 1 || m.layers[j].res_tensor == i + 1)) other_reader = true;
        if (!other_reader) S.head_gap = 1;
    }
}

}  // namespace

extern "C" {

int bh_classifier_create(const bh_config *cfg, bh_classifier **out) try {
    if (!cfg || !out || !cfg->model_path) return fail(BH_ERR_INVALID, "classifier_create: null config/model_path");
    *out = nullptr;
    if (cfg->top_k == 0 || cfg->top_k > BH_MAX_TOP_K) return fail(BH_ERR_INVALID, "top_k must be 1..%d", BH_MAX_TOP_K);
    auto c = std::make_unique<bh_classifier>();
    int rc = configure(cfg, c.get());
    if (rc == BH_OK) rc = build_front_end(c.get());
    if (rc == BH_OK) rc = upload_owned(c->d_owned, c->model.blob.data(), c->model.blob.size() * sizeof(float), &c->d_blob);
    if (rc != BH_OK) return rc;
    c->layer = std::vector<LayerState>(c->model.layers.size());
    rc = plan_fusion(c.get());      // (phase 4 before phase 3: a layer inside a fused block takes no planes)
    if (rc == BH_OK) rc = prepare_layers(c.get());
    if (rc != BH_OK) return rc;
    mark_paths(c.get());
    c->sched = build_schedule(*c, true, true);
    c->sched_layers = build_schedule(*c, false, false);
    c->sched_keep_fused = build_schedule(*c, true, false);
    if (const char *e = getenv("BIRDA_HIP_SE_GROUP_MB")) c->se_group_bytes = (size_t)atol(e) << 20;   // (MB of D per group of segments; 0: whole launches)
    *out = c.release();
    return BH_OK;
} catch (...) { return on_exception(); }

void bh_classifier_destroy(bh_classifier *c) { delete c; }

}  // extern "C"
