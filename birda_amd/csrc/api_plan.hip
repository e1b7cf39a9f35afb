// api_plan.hip -- host-side planning at classifier create (split out of api.hip in round 4, api_internal.hpp): the folded STFT x mel
// operator of a front-end branch, the liveness plan of the activation arena, and the fused MBConv blocks -- which layer triples run
// as one launch (reference: the Conv / activation / Add nodes birdnet_onnx::Classifier hands to ONNX Runtime,
// src/inference/classifier.rs:478-488), their tile configuration and their weights re-laid as per-chunk LDS-DMA blocks.
#include "api_internal.hpp"

using namespace bhi;

namespace bhi {


uint16_t f32_to_f16(float f);
float f16_to_f32(uint16_t h);

// Gf for one branch (see kernels_frontend.hip): double precision on the host, once.
// prec 0: f32 fragment-major; prec 3: f16 hi / lo planes for the split MFMA (same byte count).
std::vector<float> build_gf(const bh::BranchRec &b, const float *W, int nm_pad, int prec, int *scale_exp) {
    const int L = (int)b.frame_length, K = L / 2, nb = (int)b.n_bins, nm = (int)b.n_mels;
    std::vector<double> ct(L);
    for (int i = 0; i < L; i++) ct[i] = std::cos(2.0 * M_PI * (double)i / (double)L);
    std::vector<int> rows;
    for (int k = 0; k < nb; k++) {
        bool nz = false;
        for (int m = 0; m < nm && !nz; m++) nz = W[(size_t)k * nm + m] != 0.0f;
        if (nz) rows.push_back(k);
    }
    std::vector<float> gf((size_t)K * nm_pad, 0.0f);
    std::vector<double> acc(nm);
    for (int j = 0; j < K; j++) {
        const int n = j + 1;
        const double wn = 0.5 - 0.5 * ct[n % L];
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int k : rows) {
            const double cv = ct[(size_t)((long long)k * n % L)];
            const float *wr = W + (size_t)k * nm;
            for (int m = 0; m < nm; m++) acc[m] += cv * (double)wr[m];
        }
        const double scale = (j == K - 1) ? 0.5 * wn : wn;  // the centre sample is added to itself
        for (int m = 0; m < nm; m++) gf[(size_t)j * nm_pad + m] = (float)(scale * acc[m]);
    }
    // f16 planes hold Gf * 2^s (kernels.hpp f16_scale_exponent); the kernel's power law undoes it (BranchParams::log2_bias)
    *scale_exp = 0;
    if (prec != 0) {
        float mx = 0.0f;
        for (float v : gf) mx = std::max(mx, std::fabs(v));
        *scale_exp = bh::f16_scale_exponent(mx);
        for (float &v : gf) v = std::ldexp(v, *scale_exp);
    }
    // MFMA-fragment-major relayout (kernels.hpp BranchParams::gf)
    const int mt_n = nm_pad / 16;
    std::vector<float> frag((size_t)K * nm_pad);
    if (prec == 32) {  // mel32_kernel: [step of 16 k][mel tile of 32][plane hi, lo][64 lanes][8 halves]; within a chunk of 64 k the
        // staged Y rows pair k with k + 32 in one dword, so element jj of step s holds k = 64 (s / 4) + 8 (s % 4) + 4 (lane >> 5) + jj / 2 + 32 (jj % 2)
        uint16_t *h = reinterpret_cast<uint16_t *>(frag.data());
        const int mt32 = nm_pad / 32;
        for (int st = 0; st < K / 16; st++)
            for (int mt = 0; mt < mt32; mt++)
                for (int lane = 0; lane < 64; lane++)
                    for (int jj = 0; jj < 8; jj++) {
                        const float v = gf[(size_t)(64 * (st >> 2) + 8 * (st & 3) + 4 * (lane >> 5) + (jj >> 1) + 32 * (jj & 1)) * nm_pad + 32 * mt + (lane & 31)];
                        const uint16_t hi = f32_to_f16(v);
                        const size_t base = (((size_t)st * mt32 + mt) * 2) * 64 * 8;
                        h[base + (size_t)lane * 8 + jj] = hi;
                        h[base + 64 * 8 + (size_t)lane * 8 + jj] = f32_to_f16(v - f16_to_f32(hi));
                    }
        return frag;
    }
    if (prec != 0) {  // [step of 32 k][mel tile][plane hi, lo][64 lanes][8 halves]: k = 32 s + 4 jj + (lane >> 4)
        // (the k of a step are dealt to the four lane groups round-robin, not in runs of 8: the kernel's frame-strided LDS
        //  reads of the matching samples then fall on distinct banks -- kernels_frontend.hip, mel_kernel)
        uint16_t *h = reinterpret_cast<uint16_t *>(frag.data());
        for (int st = 0; st < K / 32; st++)
            for (int mt = 0; mt < mt_n; mt++)
                for (int lane = 0; lane < 64; lane++)
                    for (int jj = 0; jj < 8; jj++) {
                        const float v = gf[(size_t)(32 * st + 4 * jj + (lane >> 4)) * nm_pad + 16 * mt + (lane & 15)];
                        const uint16_t hi = f32_to_f16(v);
                        const size_t base = (((size_t)st * mt_n + mt) * 2) * 64 * 8;
                        h[base + (size_t)lane * 8 + jj] = hi;
                        h[base + 64 * 8 + (size_t)lane * 8 + jj] = f32_to_f16(v - f16_to_f32(hi));
                    }
        return frag;
    }
    for (int g = 0; g < K / 16; g++)
        for (int mt = 0; mt < mt_n; mt++)
            for (int lane = 0; lane < 64; lane++)
                for (int c = 0; c < 4; c++) {
                    const int k = 16 * g + 4 * (lane >> 4) + c, mel = 16 * mt + (lane & 15);
                    frag[(((size_t)g * mt_n + mt) * 64 + lane) * 4 + c] = gf[(size_t)k * nm_pad + mel];
                }
    return frag;
}
// What a forward launches, from the decisions create has made (plan_fusion: LayerState::fused_at / mb / se; api_create.hip mark_paths:
// head_gap, gap_gate, concat_chain): no decision is made here.  fused: the fused blocks run as such; chains: so do head conv + pool and the gate fast path.
std::vector<Step> build_schedule(const bh_classifier &c, bool fused, bool chains) {
    const auto &m = c.model;
    const uint32_t nl = (uint32_t)m.layers.size();
    std::vector<Step> sched;
    for (uint32_t i = 0; i < nl; i++) {
        Step st;
        st.first = st.last = i;
        if (fused && c.layer[i].fused_at >= 0) {
            // one launch reads the block input while it writes the project's output; the tensors in between stay in LDS
            st.block = c.layer[i].fused_at;
            st.path = c.mb[st.block].se ? BH_PATH_FUSED_SE : BH_PATH_FUSED;
            st.last = (uint32_t)fused_block_last(i, c.mb[st.block]);
            if (c.mb[st.block].se) {
                // a squeeze-excite block = pass A (reads the block input; writes the depthwise output D and, into the slot of the
                // OP_SCALE output -- the scaled tensor never exists --, the per-tile channel sums), the gate launch (sums -> gate
                // tensor; the pooled sums and the hidden layer in their layers' slots) and the gated project GEMM (D, gate, residual
                // -> the block output).  The sums are written long before the step their LAYER would have written that slot at.
                const auto &S = c.se[st.block];
                st.writes = {S.iD + 1};
                st.scratch = {{S.iGap + 1, 0}, {S.iPw1 + 1, 0}, {S.iPw2 + 1, 0}, {S.iScale + 1, S.part_floats}};
            }
        } else if (chains && c.layer[i].head_gap) {
            // head conv + pool in one launch: workgroups still read the conv's input while finished ones store pooled rows; the
            // conv's output never exists
            st.path = BH_PATH_HEAD_GAP;
            st.last = i + 1;
        } else if (chains && c.layer[i].gap_gate) {
            // the gate of a block that runs layer by layer in two launches (gap_gate_chain): se_hidden_kernel reads the pool's input
            // and writes its partial sums into the pool layer's tensor, se_gate16_kernel reads them while it writes the gate -- the
            // same n x C floats.  (The hidden layer's slot is kept as well: its values stay in LDS.)
            st.path = BH_PATH_SE_GATE;
            st.last = i + 2;
            st.scratch = {{i + 1, 0}, {i + 2, 0}};
        } else if (chains && c.layer[i].concat_chain) {
            // an N-way Concat: one launch gathers the leaves straight into the last record's tensor; the records' own outputs in
            // between never exist (they get no bytes, as a fused block's inner tensors get none)
            st.path = BH_PATH_CONCAT;
            st.last = i + (uint32_t)c.layer[i].concat_chain - 1;
        }
        st.reads = {m.layers[i].in_tensor};
        if (st.path == BH_PATH_CONCAT) {          // every leaf: A of the first record, then every record's B
            for (uint32_t j = i; j <= st.last; j++)
                if (m.layers[j].res_tensor != bh::NO_TENSOR) st.reads.push_back(m.layers[j].res_tensor);
        } else
        if (m.layers[st.last].res_tensor != bh::NO_TENSOR) st.reads.push_back(m.layers[st.last].res_tensor);
        st.writes.insert(st.writes.begin(), st.last + 1);
        i = st.last;
        sched.push_back(std::move(st));
    }
    return sched;
}

// liveness-based arena plan over the schedule: tensor t is born at step t (tensor 0 = front-end); a tensor that a step reads, writes
// or borrows lives through that step's last layer -- a launch that stands for several layers touches tensors earlier, or later,
// than their layers would --; the output of a layer inside a step that the step does not touch gets no bytes; the embedding
// tensor and the logits live to the end.  (keep: every tensor at its own size, end to end.)
void plan_arena(const bh::Model &m, const std::vector<Step> &sched, size_t max_batch, bool keep, std::vector<size_t> &off, size_t &total,
                std::vector<size_t> *sizes) {
    const size_t nt = m.layers.size() + 1;
    std::vector<size_t> last(nt, 0), sz(nt);
    for (size_t t = 0; t < nt; t++) { last[t] = t; sz[t] = align_up(m.tensor_floats[t] * max_batch, 64); }
    if (!keep)
        for (const Step &st : sched) {
            auto touch = [&](uint32_t t) { last[t] = std::max(last[t], (size_t)st.last + 1); };
            for (uint32_t t : st.reads) touch(t);
            for (uint32_t t : st.writes) touch(t);
            for (const auto &u : st.scratch) {
                touch(u.t);
                if (u.floats) sz[u.t] = align_up(u.floats * max_batch, 64);
            }
            for (size_t t = (size_t)st.first + 1; t <= st.last; t++)
                if (last[t] <= st.last) sz[t] = 0;       // (an inner tensor nothing above has touched)
        }
    last[m.h.embedding_tensor] = nt;
    last[nt - 1] = nt;
    if (sizes) *sizes = sz;
    off.assign(nt, 0);
    total = 0;
    if (keep) {
        for (size_t t = 0; t < nt; t++) { off[t] = total; total += sz[t]; }
        return;
    }
    struct Live { size_t off, size, last; };
    std::vector<Live> live;
    for (size_t t = 0; t < nt; t++) {
        // tensors whose last reader ran before step t are dead (step t writes tensor t while
        // reading tensors with last >= t)
        live.erase(std::remove_if(live.begin(), live.end(), [&](const Live &l) { return l.last < t; }), live.end());
        std::sort(live.begin(), live.end(), [](const Live &a, const Live &b) { return a.off < b.off; });
        size_t pos = 0;
        for (const auto &l : live) {
            if (pos + sz[t] <= l.off) break;
            pos = std::max(pos, l.off + l.size);
        }
        off[t] = pos;
        live.push_back({pos, sz[t], last[t]});
        total = std::max(total, pos + sz[t]);
    }
}
// A record with dilation (model.hpp skip_h / skip_w) is never part of a launch that stands for several layers: the fused tile kernel's
// depthwise phase, pass A of a squeeze-excite block, the channel split of a low-latency launch (a fused launch, split) and the gate
// launches all compute the undilated layer.  Every matcher below asks here; such a block runs layer by layer.
static bool layer_dilated(const bh::LayerRec &L) { return L.skip_h != 0 || L.skip_w != 0; }
// (An OP_REDUCE record -- like OP_POOL and OP_LNORM -- is in none of the op lists the matchers below accept, the global pool's places
//  included: a gate or a head whose pool is a reduce runs layer by layer, and its tensors have ordinary liveness.  The same holds for
//  an OP_BNACT record: a run that contains one is no block any matcher knows, the 1x1 -> global pool head behind one included, and the
//  arena planner sees an ordinary layer that reads in_tensor and writes its own.)

// The pool layer i opens a squeeze-excite gate that runs as the two gate launches (se_hidden_kernel, se_gate16_kernel) instead of pool
// + two GEMMs: an image of at most 64 pixels, at least BH_SE_GATE16_MIN channels, pool -> 1x1 (C -> Cr) -> 1x1 (Cr -> C) with no
// other reader of the pooled or the hidden tensor, and a shape se_gate16 supports.  Shapes alone decide; the answer is recorded in
// bh_classifier::gap_gate, and build_schedule makes a step of it.
bool gap_gate_chain(const bh::Model &m, size_t i) {
    const size_t nl = m.layers.size();
    if (i + 2 >= nl) return false;
    const auto &L = m.layers[i], &G1 = m.layers[i + 1], &G2 = m.layers[i + 2];
    if (L.op != bh::OP_GAP || L.in_h * L.in_w > 64 || L.cout < BH_SE_GATE16_MIN) return false;
    if (layer_dilated(L) || layer_dilated(G1) || layer_dilated(G2)) return false;   // (validate_model refuses such records; the matcher does not rely on it)
    bool ok = G1.op == bh::OP_PWCONV && G2.op == bh::OP_PWCONV && G1.in_h * G1.in_w == 1 && G2.in_h * G2.in_w == 1 &&
              G1.in_tensor == i + 1 && G2.in_tensor == i + 2 && G1.res_tensor == bh::NO_TENSOR && G2.res_tensor == bh::NO_TENSOR &&
              G1.cin == L.cout && G2.cin == G1.cout && G2.cout == L.cout && m.h.embedding_tensor != i + 1 && m.h.embedding_tensor != i + 2 &&
              bh::se_gate16_supports((int)L.cout, (int)G1.cout);
    for (size_t j = i + 1; ok && j < nl; j++)          // nobody else may read the pooled or the hidden tensor
        if ((j > i + 1 && m.layers[j].in_tensor == i + 1) || (j > i + 2 && m.layers[j].in_tensor == i + 2) ||
            m.layers[j].res_tensor == i + 1 || m.layers[j].res_tensor == i + 2) ok = false;
    return ok;
}

// The OP_CONCAT records from layer i on that run as one launch: each of records 2 .. k reads its predecessor whole as A and brings a B
// of its own; the predecessor has no other reader, is not the embedding tensor and carries no shuffle (a shuffle is allowed on the
// last record only); all on one image; at most four leaf sources in total.  -> k (2 .. 4), or 0: the record runs alone.  Shapes
// alone decide; the answer is recorded in bh_classifier::concat_chain, and build_schedule makes a step of it (a longer chain
// splits into steps: the next one starts at the record behind this one's last).
int concat_chain_len(const bh::Model &m, size_t i) {
    const size_t nl = m.layers.size();
    if (i >= nl || m.layers[i].op != bh::OP_CONCAT) return 0;
    int leaves = m.layers[i].res_tensor == bh::NO_TENSOR ? 1 : 2, k = 1;
    for (size_t j = i + 1; j < nl && leaves < 4; j++) {
        const auto &P = m.layers[j - 1], &L = m.layers[j];
        if (L.op != bh::OP_CONCAT || L.in_tensor != j || L.res_tensor == bh::NO_TENSOR || L.res_tensor == j || L.w_off != 0 || L.cin != P.cout ||
            L.in_h != P.out_h || L.in_w != P.out_w || P.reserved > 1 || m.h.embedding_tensor == j) break;
        bool other = false;
        for (size_t q = j + 1; q < nl && !other; q++) other = m.layers[q].in_tensor == j || m.layers[q].res_tensor == j;
        if (other) break;
        leaves++; k++;
    }
    return k >= 2 ? k : 0;
}

// IEEE binary16 round-to-nearest-even of a float, and back (host side of the hi/lo operand split)
uint16_t f32_to_f16(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x47800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));   // overflow / nan
    if (x < 0x38800000u) {                                                                     // subnormal half
        if (x < 0x33000000u) return (uint16_t)sign;
        const int shift = 113 - (int)(x >> 23);
        uint32_t m = (x & 0x7fffffu) | 0x800000u;
        const uint32_t half = m >> (shift + 13), rem = m & ((1u << (shift + 13)) - 1), mid = 1u << (shift + 12);
        return (uint16_t)(sign | (half + ((rem > mid || (rem == mid && (half & 1))) ? 1 : 0)));
    }
    const uint32_t e = ((x >> 23) - 112) << 10, m = (x >> 13) & 0x3ffu, rem = x & 0x1fffu;
    uint32_t h = e | m;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) h++;
    return (uint16_t)(sign | h);
}
float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ffu;
    uint32_t x;
    if (e == 0) {
        if (m == 0) x = sign;
        else { int k = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; k++; } x = sign | ((uint32_t)(113 - k) << 23) | ((mm & 0x3ffu) << 13); }
    } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
    else x = sign | ((e + 112) << 23) | (m << 13);
    float f; memcpy(&f, &x, 4);
    return f;
}

// The block that starts at layer i as a fused launch: expand(1x1, or the stem conv) -> depthwise -> project(1x1) whose
// intermediates have no other reader, described and handed to the tile planner.  Host logic only (no device): plan_fusion uses
// it per block at create, bh_plan_fused_blocks walks a model file with it.
// The squeeze-excite block that starts at layer i, if there is one: [expand 1x1 | stem conv] -> depthwise -> GlobalAveragePool ->
// 1x1 (C -> Cr) -> 1x1 (Cr -> C) -> OP_SCALE (depthwise output x gate) -> project 1x1, the depthwise output read by the pool and
// the scale only, every other intermediate by its successor only (EfficientNet's MBConv as tf2onnx / torch exporters spell it:
// onnx_conv.hpp, convert.py).
bool match_se_block(const bh::Model &m, const std::vector<int> &readers, size_t i, bh_classifier::SeInfo &S, bool &noexp) {
    const size_t nl = m.layers.size();
    noexp = m.layers[i].op == bh::OP_DWCONV;
    const size_t iD = noexp ? i : i + 1;
    if (iD + 5 >= nl) return false;
    const auto &D = m.layers[iD], &G = m.layers[iD + 1], &A1 = m.layers[iD + 2], &A2 = m.layers[iD + 3], &SC = m.layers[iD + 4], &P = m.layers[iD + 5];
    if (D.op != bh::OP_DWCONV || G.op != bh::OP_GAP || A1.op != bh::OP_PWCONV || A2.op != bh::OP_PWCONV || SC.op != bh::OP_SCALE || P.op != bh::OP_PWCONV) return false;
    if (layer_dilated(D)) return false;   // pass A's depthwise phase is the undilated layer: the block runs layer by layer
    const uint32_t tD = (uint32_t)iD + 1;   // the depthwise output tensor
    if (G.in_tensor != tD || A1.in_tensor != iD + 2 || A2.in_tensor != iD + 3 || SC.in_tensor != tD || SC.res_tensor != iD + 4 || P.in_tensor != iD + 5) return false;
    if (readers[tD] != 2 || readers[iD + 2] != 1 || readers[iD + 3] != 1 || readers[iD + 4] != 1 || readers[iD + 5] != 1) return false;
    if (!noexp && (m.layers[i + 1].in_tensor != i + 1 || readers[i + 1] != 1)) return false;
    if (G.res_tensor != bh::NO_TENSOR || A1.res_tensor != bh::NO_TENSOR || A2.res_tensor != bh::NO_TENSOR || D.res_tensor != bh::NO_TENSOR) return false;
    if (A1.in_h * A1.in_w != 1 || A2.in_h * A2.in_w != 1 || A1.cin != D.cout || A2.cout != D.cout || A1.cout != A2.cin || P.cin != D.cout) return false;
    if (!bh::se_gate_supports((int)D.cout, (int)A1.cout)) return false;
    S = bh_classifier::SeInfo{};
    S.iD = (uint32_t)iD; S.iGap = (uint32_t)iD + 1; S.iPw1 = (uint32_t)iD + 2; S.iPw2 = (uint32_t)iD + 3; S.iScale = (uint32_t)iD + 4; S.iP = (uint32_t)iD + 5;
    return true;
}

// The tile planner in the block's precision, then in the next more exact one that has an entry for its shape: a plain-f16 block
// (BH_FLAG_F16) without a plain-f16 instantiation runs on the split-f16 one -- more exact AND faster than the f32 MFMA -- and only
// then, as a split-f16 block without an entry does, on the f32 MFMA.
static bool plan_in_some_precision(bh::MbDesc &d, int force_cfg) {
    const int order[3] = {d.prec, d.prec == 1 ? 3 : 0, 0};
    for (int k = 0; k < 3; k++) {
        if (k > 0 && order[k] == order[k - 1]) continue;
        d.prec = order[k];
        if (bh::mb_plan(d, force_cfg)) return true;
    }
    return false;
}

bool describe_fused_block(const bh::Model &m, const std::vector<int> &readers, size_t i, int precision, int force_cfg, bh::MbDesc &d) {
    const size_t nl = m.layers.size();
    {
        bh_classifier::SeInfo S;
        bool noexp = false;
        static const bool se_off = [] { const char *e = getenv("BIRDA_HIP_FUSE_SE"); return e && e[0] == '0'; }();
        if (!se_off && match_se_block(m, readers, i, S, noexp)) {
            const auto &E = m.layers[i], &D = m.layers[S.iD], &P = m.layers[S.iP];
            const bool stem = !noexp && E.op == bh::OP_CONV && E.in_layout == 1 && E.kh == E.kw && E.sh == E.sw && E.in_tensor == 0;
            if (!noexp && E.op != bh::OP_PWCONV && !stem) return false;
            if (!noexp && E.res_tensor != bh::NO_TENSOR) return false;
            if (D.kh != D.kw || D.sh != D.sw || (!noexp && E.cout != D.cout) || D.in_layout != 0) return false;
            // (the gated project GEMM has no activation on the f16 MFMA; project convolutions of MBConv blocks have none)
            if (P.act != bh::ACT_NONE) return false;
            // (an activation AFTER the residual add is not in the fused or the gated kernels' epilogues either: layer by layer)
            if (P.reserved == bh::RES_ACT_AFTER) return false;
            d = bh::MbDesc{};
            d.se = 1;
            d.dblk = 0;      // (set per forward: api.hip SliceRun::fused_se)
            d.noexp = noexp ? 1 : 0;
            d.H = (int)(noexp ? D.in_h : E.in_h); d.W = (int)(noexp ? D.in_w : E.in_w);
            d.Cin = (int)(noexp ? D.cout : E.cin); d.Cexp = (int)D.cout; d.Cout = (int)P.cout;
            if (stem) {
                d.stem = 1; d.stem_c = (int)E.cin; d.stem_h = (int)E.in_h; d.stem_w = (int)E.in_w; d.stem_k = (int)E.kh;
                d.stem_s = (int)E.sh; d.stem_pt = (int)E.pad_t; d.stem_pl = (int)E.pad_l;
                d.H = (int)E.out_h; d.W = (int)E.out_w; d.Cin = (int)(E.kh * E.kw * E.cin);
            }
            d.Ho = (int)D.out_h; d.Wo = (int)D.out_w; d.pad_t = (int)D.pad_t; d.pad_l = (int)D.pad_l;
            d.KS = (int)D.kh; d.ST = (int)D.sh;
            d.act_e = (int)(noexp ? D.act : E.act); d.act_d = (int)D.act; d.act_p = (int)P.act;
            d.prec = precision;
            return plan_in_some_precision(d, force_cfg);
        }
    }
    if (i + 1 < nl && m.layers[i].op == bh::OP_DWCONV && m.layers[i + 1].op == bh::OP_PWCONV) {
        // depthwise -> project (+ residual) WITHOUT an expand convolution (the expand-ratio-1 blocks of EfficientNet after the
        // first): fused with the block input standing in for the expanded tensor (MbDesc::noexp)
        const auto &D = m.layers[i], &P = m.layers[i + 1];
        if (P.in_tensor != i + 1 || readers[i + 1] != 1 || D.res_tensor != bh::NO_TENSOR) return false;
        if (D.kh != D.kw || D.sh != D.sw || D.cout != P.cin || D.in_layout != 0 || layer_dilated(D)) return false;
        if (P.reserved == bh::RES_ACT_AFTER) return false;   // act(project + x): never a fused block's project convolution
        d = bh::MbDesc{};
        d.noexp = 1;
        d.H = (int)D.in_h; d.W = (int)D.in_w; d.Cin = (int)D.cout; d.Cexp = (int)D.cout; d.Cout = (int)P.cout;
        d.Ho = (int)D.out_h; d.Wo = (int)D.out_w; d.pad_t = (int)D.pad_t; d.pad_l = (int)D.pad_l;
        d.KS = (int)D.kh; d.ST = (int)D.sh;
        d.act_e = (int)D.act; d.act_d = (int)D.act; d.act_p = (int)P.act;   // (no expand activation: the kernel template is keyed on one)
        d.prec = precision;
        return plan_in_some_precision(d, force_cfg);
    }
    if (i + 2 >= nl) return false;
    const auto &E = m.layers[i], &D = m.layers[i + 1], &P = m.layers[i + 2];
    const bool stem = E.op == bh::OP_CONV && E.in_layout == 1 && E.kh == E.kw && E.sh == E.sw && E.in_tensor == 0;
    if ((E.op != bh::OP_PWCONV && !stem) || D.op != bh::OP_DWCONV || P.op != bh::OP_PWCONV) return false;
    if (D.in_tensor != i + 1 || P.in_tensor != i + 2 || readers[i + 1] != 1 || readers[i + 2] != 1) return false;
    if (E.res_tensor != bh::NO_TENSOR || D.res_tensor != bh::NO_TENSOR) return false;
    if (D.kh != D.kw || D.sh != D.sw || E.cout != D.cout || D.cout != P.cin || layer_dilated(D) || layer_dilated(E)) return false;
    if (P.reserved == bh::RES_ACT_AFTER) return false;   // act(project + x): never a fused block's project convolution
    d = bh::MbDesc{};
    d.H = (int)E.in_h; d.W = (int)E.in_w; d.Cin = (int)E.cin; d.Cexp = (int)E.cout; d.Cout = (int)P.cout;
    if (stem) {  // the depthwise conv sees the stem's output image; the stem itself is gathered
        d.stem = 1; d.stem_c = (int)E.cin; d.stem_h = (int)E.in_h; d.stem_w = (int)E.in_w; d.stem_k = (int)E.kh;
        d.stem_s = (int)E.sh; d.stem_pt = (int)E.pad_t; d.stem_pl = (int)E.pad_l;
        d.H = (int)E.out_h; d.W = (int)E.out_w; d.Cin = (int)(E.kh * E.kw * E.cin);
    }
    d.Ho = (int)D.out_h; d.Wo = (int)D.out_w; d.pad_t = (int)D.pad_t; d.pad_l = (int)D.pad_l;
    d.KS = (int)D.kh; d.ST = (int)D.sh;
    d.act_e = (int)E.act; d.act_d = (int)D.act; d.act_p = (int)P.act;
    d.prec = precision;
    // (the split-f16 MFMA and the f32 MFMA agree to ~1e-7 of sum|a b|; measured (profiles/), f16x3 is the faster one on every
    //  block, the stem's 18-column im2col GEMM included: the stem block takes the model's precision like every other)
    return plan_in_some_precision(d, force_cfg);
}

std::vector<int> tensor_readers(const bh::Model &m) {
    std::vector<int> readers(m.layers.size() + 1, 0);
    for (const auto &L : m.layers) {
        readers[L.in_tensor]++;
        if (L.res_tensor != bh::NO_TENSOR) readers[L.res_tensor]++;
    }
    readers[m.h.embedding_tensor]++;
    return readers;
}

// f16 operand planes of a [K][N] weight matrix for the split-f16 GEMMs: [ceil(K / 32)][ceil(N / 16)]{hi, lo}[64 lanes][8 halves],
// lane (n & 15, k group) holding k = 32 step + 8 (lane >> 4) + 0..7 of column n, scaled by a power of two (1 / *unscale) that puts
// the largest weight in the f16 range, zero beyond K and N
// *lo_zero (may be null): every weight IS an f16 value after the power-of-two pre-scale -- its hi half holds it exactly, so every lo
// entry is zero and nothing was lost below the f16 subnormal grid either (a residual under half a subnormal step also rounds to a
// zero lo entry: such a matrix does NOT qualify; inf / NaN weights neither).  The layer may then run two-term products
// (kernels_conv.hip TERMS == 2) on the compact form of these planes (w16_compact)
std::vector<uint16_t> w16_planes(const float *W, int K, int N, float *unscale, bool *lo_zero) {
    const int nt = (N + 15) / 16, ksteps = (K + 31) / 32;
    std::vector<uint16_t> planes((size_t)ksteps * nt * 2 * 64 * 8, 0);
    float wmax = 0.0f;
    for (size_t q = 0; q < (size_t)K * N; q++) wmax = std::max(wmax, std::fabs(W[q]));
    const int ws = bh::f16_scale_exponent(wmax);
    *unscale = std::ldexp(1.0f, -ws);
    bool exact = true;
    for (int st = 0; st < ksteps; st++)
        for (int t = 0; t < nt; t++)
            for (int lane = 0; lane < 64; lane++)
                for (int jj = 0; jj < 8; jj++) {
                    const int k = 32 * st + 8 * (lane >> 4) + jj, n = 16 * t + (lane & 15);
                    const float v = (n < N && k < K) ? std::ldexp(W[(size_t)k * N + n], ws) : 0.0f;
                    const uint16_t hi = f32_to_f16(v);
                    const size_t base = (((size_t)st * nt + t) * 2) * 64 * 8;
                    const float rest = v - f16_to_f32(hi);
                    if (!(rest == 0.0f)) exact = false;
                    planes[base + (size_t)lane * 8 + jj] = hi;
                    planes[base + 64 * 8 + (size_t)lane * 8 + jj] = f32_to_f16(rest);
                }
    if (lo_zero) *lo_zero = exact;
    return planes;
}

// the compact planes of two-term products: [k step][column tile][64 lanes][8 halves], w16_planes' layout without the lo half
std::vector<uint16_t> w16_compact(const std::vector<uint16_t> &planes) {
    std::vector<uint16_t> out(planes.size() / 2);
    for (size_t blk = 0; blk < planes.size() / (2 * 64 * 8); blk++)
        memcpy(&out[blk * 64 * 8], &planes[blk * 2 * 64 * 8], 64 * 8 * sizeof(uint16_t));
    return out;
}

// A full convolution's [kh][kw][cin][cout] weights as the implicit GEMM's K x ld rows: the channels of every tap padded to whole
// 32-deep steps (K = kh kw align_up(cin, 32)), the columns to ld; zero in the padding
std::vector<float> conv_gemm_rows(const float *W, const bh::ConvParams &p, int ld) {
    const size_t cpad = align_up((size_t)p.cin, 32), taps = (size_t)p.kh * p.kw;
    std::vector<float> w(taps * cpad * ld, 0.0f);
    for (size_t t = 0; t < taps; t++)
        for (size_t ch = 0; ch < (size_t)p.cin; ch++)
            memcpy(&w[(t * cpad + ch) * ld], W + (t * p.cin + ch) * p.cout, p.cout * sizeof(float));
    return w;
}

// A grouped convolution's compact [kh][kw][cin / G][cout] weights as the matrix Wt [K][16 n_tiles] of kernels_gconv.hip: column o
// of column tile t is dense over k = tap * span + (c - c0), [c0, c0 + span) the tile's span of input channels (gconv_tile_span),
// zero where channel c is not in o's group; K = the largest tile's kh kw span, padded ONCE at the end to whole 32-deep steps
std::vector<float> gconv_matrix(const float *W, const bh::ConvParams &p, int G, int *K_out) {
    const int nt = (p.cout + 15) / 16, gi = p.cin / G, go = p.cout / G, taps = p.kh * p.kw;
    size_t kmax = 0;
    for (int t = 0; t < nt; t++) {
        int c0, span;
        bh::gconv_tile_span(p.cin, p.cout, G, t, c0, span);
        kmax = std::max(kmax, (size_t)taps * span);
    }
    const size_t K = align_up(kmax, 32), ld = (size_t)nt * 16;
    std::vector<float> wt(K * ld, 0.0f);
    for (int o = 0; o < p.cout; o++) {
        int c0, span;
        bh::gconv_tile_span(p.cin, p.cout, G, o / 16, c0, span);
        const int first = (o / go) * gi - c0;      // the group's first channel within the span
        for (int tap = 0; tap < taps; tap++)
            for (int c = 0; c < gi; c++)
                wt[((size_t)tap * span + first + c) * ld + o] = W[((size_t)tap * gi + c) * p.cout + o];
    }
    *K_out = (int)K;
    return wt;
}
// ... and its f32 MFMA fragments [K / 16][n_tiles][64 lanes][4]: element (g, t, lane, c) = Wt[16g + 4 (lane >> 4) + c][16t + (lane & 15)]
std::vector<float> gconv_fragments(const std::vector<float> &wt, int K, int nt) {
    std::vector<float> f((size_t)K * nt * 16);
    const size_t ld = (size_t)nt * 16;
    for (int g = 0; g < K / 16; g++)
        for (int t = 0; t < nt; t++)
            for (int lane = 0; lane < 64; lane++)
                for (int c = 0; c < 4; c++)
                    f[(((size_t)g * nt + t) * 64 + lane) * 4 + c] = wt[((size_t)16 * g + 4 * (lane >> 4) + c) * ld + 16 * t + (lane & 15)];
    return f;
}

// A pointwise / dense layer's [K][N] weights with the rows padded to ld = align_up(N, 4) (the f32 GEMM's 16-B loads); zero in the padding
std::vector<float> pw_gemm_rows(const float *W, size_t K, size_t N, size_t ld) {
    std::vector<float> w(K * ld, 0.0f);
    for (size_t k = 0; k < K; k++) memcpy(&w[k * ld], W + k * N, N * sizeof(float));
    return w;
}

// The weights of one planned fused block as the kernel reads them (kernels.hpp MbDesc): the per-chunk fragment blocks of the picked
// tile configuration, and everything the f16 modes hang on them -- the plane exponents se / sp, e_fold with the scaled GELU
// coefficients, the 2x GELU factors, the hi / lo planes, the stem's run-packed im2col order, the folded depthwise taps, bp scaled to
// the project accumulators' exponent.  Fills d.e_unscale / p_scale / p_unscale / e_fold / gelu.  We, be, Wd, bd, Wp, bp in the
// loaders' layouts ([Cin][Cexp], [tap][Cexp], [Cexp][Cout]); We / be are not read for a no-expand block.  Host only: plan_fusion
// uploads the result at create, bh_debug_mbconv_block for one block alone.
void mb_prepare_weights(bh::MbDesc &d, const float *We, const float *be, const float *Wd, const float *bd, const float *Wp, const float *bp,
                        MbHostWeights &out) {
    // per-chunk weight blocks (kernels.hpp MbDesc)
    const int CE = d.CE, NTE = CE / 16, KG = d.KG, NTOP = d.NTOP, nch = d.nchunks, KK = d.KS * d.KS;
    const bool h16 = d.prec != 0;
    // f16 operand planes hold We * 2^se and Wp * 2^sp (kernels.hpp f16_scale_exponent); be / bp are multiplied alike
    int se = 0, sp = 0;
    if (h16) {
        float me = 0.0f, mp = 0.0f;
        for (size_t q = 0; !d.noexp && q < (size_t)d.Cin * d.Cexp; q++) me = std::max(me, std::fabs(We[q]));
        for (size_t q = 0; q < (size_t)d.Cexp * d.Cout; q++) mp = std::max(mp, std::fabs(Wp[q]));
        se = bh::f16_scale_exponent(me);
        sp = bh::f16_scale_exponent(mp);
    }
    // GELU blocks of the f16 modes: the expand GELU runs on the SCALED accumulator with coefficients c_k 2^(-k se) and the 2^-se
    // moves into the depthwise taps (kernels.hpp gelu_erf_fast4_scaled).  c_5 2^(-5 se) must stay a normal f32 on both sides:
    // |se| <= 21 (weights 2^7 away from the usual He-normal sizes still land within 2^-8 of the top of the f16 range).
    d.e_fold = 0;
    d.gelu = bh::GeluScaled{0.f, 0.f, 0.f, 0.f, 0.f};
    if (d.noexp) se = 0;
    if (h16 && d.act_e == bh::ACT_GELU_ERF && !d.noexp) {
        se = std::max(-21, std::min(21, se));
        d.e_fold = 1;
        float gc[5];
        for (int k = 1; k <= 5; k++) gc[k - 1] = std::ldexp(bh::kGeluCoef[k - 1], -k * se);
        d.gelu = bh::GeluScaled{gc[0], gc[1], gc[2], gc[3], gc[4]};
    }
    const int spa = sp;   // the project accumulators hold 2^spa times the output
    d.e_unscale = std::ldexp(1.0f, -se); d.p_scale = std::ldexp(1.0f, spa); d.p_unscale = std::ldexp(1.0f, -spa);
    const size_t frag = h16 ? 512 : 256, psteps = h16 ? (CE + 31) / 32 : NTE;
    const bool p16 = h16 && CE == 16;   // project GEMM as one 16-deep step: [column tile]{hi, lo}[64 lanes][4 halves]
    const size_t we_fl = (size_t)KG * NTE * frag + CE, wp_fl = p16 ? (size_t)NTOP * 256 : psteps * NTOP * frag, wd_fl = (size_t)KK * CE + CE;
    std::vector<float> &wef = out.we, &wpf = out.wp, &wdf = out.wd;
    wef.assign(nch * we_fl, 0.0f); wpf.assign(nch * wp_fl, 0.0f); wdf.assign(nch * wd_fl, 0.0f);
    // (stem block in the f16 modes: the kernel gathers its im2col columns by memory runs, kernels_mbconv.hip -- position
    //  8 kq + 3 q + dx of the one 32-deep step is tap (dy, dx) of channel ch with run 2 kq + q = 3 ch + dy)
    auto we_at = [&](int k, int n) {
        if (d.stem && h16) {
            const int g = k >> 5, kq = (k & 31) >> 3, jj = k & 7, r = 8 * g + 2 * kq + jj / 3, dx = jj % 3;
            if (jj >= 6 || r >= 3 * d.stem_c) return 0.0f;
            const int ch = r / 3, dy = r - 3 * ch;
            k = (dy * 3 + dx) * d.stem_c + ch;
        }
        return (!d.noexp && k < d.Cin && n < d.Cexp) ? std::ldexp(We[(size_t)k * d.Cexp + n], se) : 0.0f;
    };
    auto wp_at = [&](int k, int n) { return (k < d.Cexp && n < d.Cout) ? std::ldexp(Wp[(size_t)k * d.Cout + n], sp) : 0.0f; };
    // f16: element jj of lane's 8-half fragment = k = 32 g + 8 (lane >> 4) + jj; hi plane then lo plane
    auto put16 = [&](std::vector<float> &dst, size_t base_fl, int plane, int lane, int jj, float v) {
        uint16_t *h = reinterpret_cast<uint16_t *>(dst.data() + base_fl) + ((size_t)plane * 64 + lane) * 8 + jj;
        const uint16_t hi = f32_to_f16(v);
        *h = plane == 0 ? hi : f32_to_f16(v - f16_to_f32(hi));
    };
    for (int ch = 0; ch < nch; ch++) {
        for (int g = 0; g < KG; g++)
            for (int j = 0; j < NTE; j++)
                for (int lane = 0; lane < 64; lane++) {
                    const int n = ch * CE + 16 * j + (lane & 15);
                    if (h16) {
                        for (int jj = 0; jj < 8; jj++) {
                            const float v = we_at(32 * g + 8 * (lane >> 4) + jj, n);
                            const size_t base = ch * we_fl + ((size_t)g * NTE + j) * 512;
                            put16(wef, base, 0, lane, jj, v);
                            put16(wef, base, 1, lane, jj, v);
                        }
                    } else {
                        for (int cc = 0; cc < 4; cc++)
                            wef[ch * we_fl + (((size_t)g * NTE + j) * 64 + lane) * 4 + cc] = we_at(16 * g + 4 * (lane >> 4) + cc, n);
                    }
                }
        for (int n = 0; n < CE; n++) wef[ch * we_fl + (size_t)KG * NTE * frag + n] = (!d.noexp && ch * CE + n < d.Cexp) ? std::ldexp(be[ch * CE + n], se) : 0.0f;
        if (p16) {
            for (int j = 0; j < NTOP; j++)
                for (int lane = 0; lane < 64; lane++)
                    for (int jj = 0; jj < 4; jj++) {
                        const float v = wp_at(ch * CE + 4 * (lane >> 4) + jj, 16 * j + (lane & 15));
                        uint16_t *h = reinterpret_cast<uint16_t *>(wpf.data() + ch * wp_fl + (size_t)j * 256);
                        const uint16_t hi = f32_to_f16(v);
                        h[(size_t)lane * 4 + jj] = hi;
                        h[(size_t)(64 + lane) * 4 + jj] = f32_to_f16(v - f16_to_f32(hi));
                    }
        }
        for (int g = 0; g < (int)psteps && !p16; g++)
            for (int j = 0; j < NTOP; j++)
                for (int lane = 0; lane < 64; lane++) {
                    const int n = 16 * j + (lane & 15);
                    if (h16) {
                        for (int jj = 0; jj < 8; jj++) {
                            const int kk = 32 * g + 8 * (lane >> 4) + jj;          // k inside the chunk (zero padding past CE)
                            const float v = kk < CE ? wp_at(ch * CE + kk, n) : 0.0f;
                            const size_t base = ch * wp_fl + ((size_t)g * NTOP + j) * 512;
                            put16(wpf, base, 0, lane, jj, v);
                            put16(wpf, base, 1, lane, jj, v);
                        }
                    } else {
                        for (int cc = 0; cc < 4; cc++)
                            wpf[ch * wp_fl + (((size_t)g * NTOP + j) * 64 + lane) * 4 + cc] = wp_at(ch * CE + 16 * g + 4 * (lane >> 4) + cc, n);
                    }
                }
        for (int tap = 0; tap < KK; tap++)
            for (int n = 0; n < CE; n++)
                wdf[ch * wd_fl + (size_t)tap * CE + n] = ch * CE + n < d.Cexp ? std::ldexp(Wd[(size_t)tap * d.Cexp + ch * CE + n], d.e_fold ? -se : 0) : 0.0f;
        for (int n = 0; n < CE; n++) wdf[ch * wd_fl + (size_t)KK * CE + n] = ch * CE + n < d.Cexp ? bd[ch * CE + n] : 0.0f;
    }
    out.spa = spa;
    out.bp.clear();
    if (spa != 0) {   // bp * 2^spa: the project accumulators start there
        out.bp.resize(d.Cout);
        for (int n = 0; n < d.Cout; n++) out.bp[n] = std::ldexp(bp[n], spa);
    }
}

// Prepares a fused launch for every block describe_fused_block accepts (weights re-laid fragment-major for the picked tile config).
// It reads the model and d_blob alone, so create runs it before the layers: whether a layer takes planes depends on its result.
int plan_fusion(bh_classifier *c) {
    const auto &m = c->model;
    const size_t nl = m.layers.size();
    const char *fuse_env = getenv("BIRDA_HIP_FUSE");
    if (fuse_env && fuse_env[0] == '0') return BH_OK;
    const char *cfg_env = getenv("BIRDA_HIP_MB_CFG");
    const int force_cfg = cfg_env ? atoi(cfg_env) : -1;
    const std::vector<int> readers = tensor_readers(m);
    for (size_t i = 0; i + 2 < nl; i++) {
        bh::MbDesc d{};
        if (!describe_fused_block(m, readers, i, c->precision, force_cfg, d)) continue;
        // (a no-expand block is layers i = depthwise, i + 1 = project; E then only lends the code below a valid layer to name)
        bh_classifier::SeInfo S;
        if (d.se) { bool ne = false; if (!match_se_block(m, readers, i, S, ne)) continue; }
        const auto &E = m.layers[i], &D = m.layers[d.noexp ? i : i + 1], &P = m.layers[d.se ? S.iP : d.noexp ? i + 1 : i + 2];
        MbHostWeights hw;
        mb_prepare_weights(d, m.blob.data() + E.w_off, m.blob.data() + E.b_off, m.blob.data() + D.w_off, m.blob.data() + D.b_off,
                           m.blob.data() + P.w_off, m.blob.data() + P.b_off, hw);
        auto own = [&](const std::vector<float> &v, const float **dst) { return upload_owned(c->d_owned, v.data(), v.size() * sizeof(float), dst); };
        d.bp = c->d_blob + P.b_off;
        int rc = own(hw.we, &d.We);
        if (rc == BH_OK) rc = own(hw.wp, &d.Wp);
        if (rc == BH_OK) rc = own(hw.wd, &d.Wd);
        if (rc == BH_OK && hw.spa != 0) rc = own(hw.bp, &d.bp);   // bp * 2^spa (mb_prepare_weights)
        if (rc != BH_OK) return rc;
        c->layer[i].fused_at = (int)c->mb.size();
        c->mb.push_back(d);
        {
            bh::MbDesc tw{};
            tw.cfg = -1;
            // (squeeze-excite blocks keep ONE tiling -- the pooled sums are added tile by tile, and a segment's logits must not depend
            //  on the size of the launch it ran in -- except where the one-segment twin adds them in the very same order:
            //  mb_twin_sums_match, the 4x16 stages' whole-image tiles)
            if (force_cfg < 0 && bh::mb_plan_twin(d, tw) && (!d.se || bh::mb_twin_sums_match(d, tw))) c->mb_small.push_back(tw);
            else { tw.cfg = -1; c->mb_small.push_back(tw); }
            bh::MbDesc nw{};
            nw.cfg = -1;
            if (!(force_cfg < 0 && !d.se && bh::mb_plan_narrow(d, nw))) nw.cfg = -1;
            c->mb_narrow.push_back(nw);
            // (squeeze-excite: the slot of the per-tile channel sums holds whichever of the three tilings has the most tiles)
            size_t tiles = (size_t)d.tiles_x * d.tiles_y;
            if (c->mb_small.back().cfg >= 0) tiles = std::max(tiles, (size_t)c->mb_small.back().tiles_x * c->mb_small.back().tiles_y);
            if (nw.cfg >= 0) tiles = std::max(tiles, (size_t)nw.tiles_x * nw.tiles_y);
            S.part_floats = d.se ? tiles * (size_t)d.Cexp : 0;
            c->se.push_back(d.se ? S : bh_classifier::SeInfo{});
        }
        i = fused_block_last(i, d);
    }
    return BH_OK;
}

}  // namespace bhi
