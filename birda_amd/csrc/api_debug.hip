// The classifier-free kernel diagnostics of the C ABI (include/birda_hip_*_debug.h): one kernel family each, alone on operands of
// the caller's, with create's weight preparation and the launcher a forward pass takes.  Tests hold the kernels to float64 through
// them.  Each reads as its argument checks, its weight preparation, the one launch and DebugLaunch::finish.
#include "api_internal.hpp"
#include <deque>
#include "../../include/birda_hip_layer_debug.h"
#include "../../include/birda_hip_pool_debug.h"
#include "../../include/birda_hip_concat_debug.h"
#include "../../include/birda_hip_gate_debug.h"
#include "../../include/birda_hip_resact_debug.h"
#include "../../include/birda_hip_gconv_debug.h"
#include "../../include/birda_hip_block_debug.h"
#include "../../include/birda_hip_resample_debug.h"
#include "../../include/birda_hip_custom_debug.h"
#include "../../include/birda_hip_gated_debug.h"
#include "../../include/birda_hip_dilated_debug.h"
#include "../../include/birda_hip_lnorm_debug.h"
#include "../../include/birda_hip_reduce_debug.h"
#include "../../include/birda_hip_bnact_debug.h"

using namespace bhi;

namespace {

// A device buffer inside 64 KiB guard bands.  The input guards hold a quiet NaN, so a read past an operand shows up as NaN in the
// output (the guards lie inside the allocation: such a read cannot fault); an output buffer, guards and body alike, holds a second
// NaN payload before the launch, so an element the kernel never wrote keeps it and a write past it is found by comparing the
// guards afterwards.
constexpr uint32_t kGuardNaN = 0x7fc00000u, kUnwrittenNaN = 0x7fc0beefu;
struct Guarded {
    static constexpr size_t G = 64 * 1024;
    char *base = nullptr;
    size_t bytes = 0;
    ~Guarded() { if (base) (void)hipFree(base); }
    float *p() const { return (float *)(base + G); }
    // body = src (bytes of it), or the fill pattern too when src is null
    bool put(const void *src, size_t n, uint32_t fill) {
        bytes = (n + 3) & ~(size_t)3;
        std::vector<uint32_t> h((2 * G + bytes) / 4, fill);
        if (src) memcpy((char *)h.data() + G, src, n);
        if (hipMalloc((void **)&base, h.size() * 4) != hipSuccess) { base = nullptr; return false; }
        return hipMemcpy(base, h.data(), h.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
};

// The buffers of one diagnostic call and the launch's end.  A failed allocation or copy is remembered (ok): the entry point asks
// once, before it launches.
struct DebugLaunch {
    const char *who;
    bool ok = true;
    std::deque<Guarded> bufs;
    struct Out { const Guarded *g; const char *label; float *host; size_t floats; };
    std::vector<Out> outs;
    // an operand on the device; null for an operand the caller left out
    const float *in(const void *src, size_t bytes) {
        if (!src) return nullptr;
        bufs.emplace_back();
        ok = ok && bufs.back().put(src, bytes, kGuardNaN);
        return bufs.back().p();
    }
    // an output or scratch buffer the kernel writes, `label` in the message about a broken guard; finish copies it to host (may be null)
    float *out(size_t floats, const char *label, float *host) {
        bufs.emplace_back();
        ok = ok && bufs.back().put(nullptr, floats * 4, kUnwrittenNaN);
        outs.push_back({&bufs.back(), label, host, floats});
        return bufs.back().p();
    }
    int no_memory() const { return fail(BH_ERR_HIP, "%s: device memory", who); }
    int sync() const { HIPCHK(hipGetLastError()); HIPCHK(hipDeviceSynchronize()); return BH_OK; }
    // wait, check the guards of every output, copy the outputs and the kernel's name out
    int finish(const char *name, char *kernel, size_t kernel_cap) const {
        const int rc = sync();
        if (rc != BH_OK) return rc;
        std::vector<uint32_t> h(Guarded::G / 4);
        for (const Out &o : outs)
            for (const char *g : {o.g->base, o.g->base + Guarded::G + o.g->bytes}) {
                HIPCHK(hipMemcpy(h.data(), g, Guarded::G, hipMemcpyDeviceToHost));
                for (uint32_t v : h)
                    if (v != kUnwrittenNaN) return fail(BH_ERR_INTERNAL, "%s: %s wrote outside %s", who, name ? name : "the kernel", o.label);
            }
        for (const Out &o : outs)
            if (o.host) HIPCHK(hipMemcpy(o.host, o.g->p(), o.floats * 4, hipMemcpyDeviceToHost));
        if (kernel && kernel_cap) snprintf(kernel, kernel_cap, "%s", name ? name : "");
        return BH_OK;
    }
};

const char *act_name(int act) {
    static const char *const names[] = {"none", "relu", "relu6", "swish", "gelu", "gelu_tanh", "sigmoid", "hswish", "hsigmoid"};
    return act >= 0 && act <= bh::ACT_LAST ? names[act] : "?";
}

// A shape array's in_h, in_w, out_h, out_w, channels, kh, kw, sh, sw, pad_t, pad_l as the launchers' ConvParams.  The GEMM and
// grouped convolutions carry cin, cout at [4], [5]; pool and plain layers (`one`) carry one channel count at [4], and the direct
// convolution its input channels at [11] (cin_at).
bh::ConvParams shape_params(const int32_t *s, bool one, int cin_at, int in_layout, int act, int after) {
    const int32_t *k = s + (one ? 5 : 6);
    return bh::ConvParams{s[0], s[1], s[2], s[3], s[cin_at], k[-1], k[0], k[1], k[2], k[3], k[4], k[5], in_layout, act, after};
}

// the planes a debug entry point uploads for `terms`: full for 1 and 3; compact for 2, which is refused (false) when W is not made
// of f16 values
bool debug_planes(const float *W, int K, int N, int terms, float *unscale, std::vector<uint16_t> &planes) {
    bool lo_zero = false;
    planes = w16_planes(W, K, N, unscale, &lo_zero);
    if (terms != 2) return true;
    if (!lo_zero) return false;
    planes = w16_compact(planes);
    return true;
}

// The block a shape array describes (birda_hip_block_debug.h), not yet planned; false: arguments no block can have.
bool mb_desc_of_shape(const int32_t *sh, bh::MbDesc &d) {
    d = bh::MbDesc{};
    d.H = sh[0]; d.W = sh[1]; d.Cin = sh[2]; d.Cexp = sh[3]; d.Cout = sh[4]; d.Ho = sh[5]; d.Wo = sh[6]; d.pad_t = sh[7]; d.pad_l = sh[8];
    d.KS = sh[9]; d.ST = sh[10];
    d.act_e = d.act_d = sh[11]; d.act_p = bh::ACT_NONE;
    d.prec = sh[12]; d.noexp = sh[13] != 0; d.se = sh[14] != 0; d.dblk = sh[15] != 0;
    d.stem_c = sh[16]; d.stem_h = sh[17]; d.stem_w = sh[18]; d.stem_k = sh[19]; d.stem_s = sh[20]; d.stem_pt = sh[21]; d.stem_pl = sh[22];
    d.stem = d.stem_c > 0;
    if (d.H < 1 || d.W < 1 || d.Cin < 1 || d.Cexp < 1 || d.Cout < 1 || d.Ho < 1 || d.Wo < 1 || d.pad_t < 0 || d.pad_l < 0 || d.KS < 1 || d.ST < 1) return false;
    if (d.H > 32767 || d.W > 32767 || d.Cin > 65536 || d.Cexp > 65536 || d.Cout > 65536 || d.Ho > d.H + d.pad_t || d.Wo > d.W + d.pad_l) return false;
    if (d.prec != 0 && d.prec != 1 && d.prec != 3) return false;
    if (d.noexp && (d.stem || d.Cexp != d.Cin)) return false;
    if (d.stem && (d.stem_c < 0 || d.stem_h < 1 || d.stem_w < 3 || d.stem_k < 1 || d.stem_s < 1 || d.stem_pt < 0 || d.stem_pl < 0 ||
                   d.stem_h > 32767 || d.stem_w > 32767 || d.Cin != d.stem_k * d.stem_k * d.stem_c)) return false;
    if (d.dblk && (!d.se || d.Cexp % 16 || (d.Ho * d.Wo) % 16)) return false;
    return true;
}

// mb_plan for the shape, then the variant a forward pass would swap in (0: the planned entry, 1: its one-segment twin, 2: its
// narrow-tile twin), and the record of what that is.  BH_ERR_UNSUPPORTED with the planner's words when there is none.
int mb_debug_plan(const int32_t *shape, int force_cfg, int variant, bh::MbDesc &d, int32_t *rec, char *name, size_t name_cap) {
    if (rec) std::fill(rec, rec + 24, 0);
    if (rec) rec[0] = -1;
    if (name && name_cap) name[0] = 0;
    if (!shape || variant < 0 || variant > 2) return fail(BH_ERR_INVALID, "debug_mbconv: bad arguments");
    const int nfam = bh::mb_config_families(), nbase = bh::mb_config_count() / nfam;   // (the activation copies of one list: kernels_mbconv.hip)
    for (int k = 0; rec && force_cfg >= 0 && force_cfg < nbase && k < nfam; k++) {   // the row's own facts, whatever becomes of the shape
        int th = 0, has_se = 0, act = -1;
        if (bh::mb_config_row(force_cfg + k * nbase, &th, &has_se, &act) && act == shape[11]) { rec[6] = has_se; rec[7] = th; }
    }
    if (!mb_desc_of_shape(shape, d)) return fail(BH_ERR_INVALID, "debug_mbconv: not a block's shape");
    bh::MbDesc planned = d;
    if (!bh::mb_plan(planned, force_cfg)) {
        char why[512];
        bh::mb_plan_refusal(d, force_cfg, why, sizeof why);
        return fail(BH_ERR_UNSUPPORTED, "debug_mbconv: %s", why);
    }
    bh::MbDesc tw{}, nw{};
    const bool has_twin = bh::mb_plan_twin(planned, tw), has_narrow = bh::mb_plan_narrow(planned, nw);
    const bool sums = has_twin && bh::mb_twin_sums_match(planned, tw);
    if (variant == 1 && !has_twin) return fail(BH_ERR_UNSUPPORTED, "debug_mbconv: the planned entry has no one-segment twin");
    if (variant == 2 && !has_narrow) return fail(BH_ERR_UNSUPPORTED, "debug_mbconv: the planned entry has no narrow-tile twin");
    d = variant == 1 ? tw : variant == 2 ? nw : planned;
    if (rec) {
        int th = 0, has_se = 0;
        bh::mb_config_row(d.cfg, &th, &has_se, nullptr);
        rec[20] = 0;   // (the PERSIST template argument: always 0, the record keeps its place)
        rec[0] = d.cfg; rec[1] = d.TH; rec[2] = d.tiles_y; rec[3] = d.tiles_x; rec[4] = d.nchunks; rec[5] = d.KG; rec[6] = has_se; rec[7] = th;
        rec[8] = d.S; rec[9] = d.CE; rec[10] = d.NTOP; rec[11] = (int32_t)d.lds_bytes; rec[12] = mb_ksplit_of(d); rec[13] = has_twin;
        rec[14] = has_narrow; rec[15] = sums; rec[16] = d.IH; rec[17] = d.IW; rec[18] = d.mpad_max;
        rec[19] = d.prec != 0 && bh::pw_gemm16_gated_wants_blocked(d.Cexp, d.Cout, d.Ho * d.Wo);
    }
    if (name && name_cap) {
        char nm[128];
        bh::mb_config_name(d.cfg, nm, sizeof nm);
        snprintf(name, name_cap, "mbconv<%s,%d>", nm, d.se ? 1 : 0);
    }
    return BH_OK;
}

// what the last bh_debug_gated_gemm launched (its signature is the debug header's and carries no name buffer)
std::atomic<const char *> g_last_gated_kernel{nullptr};

}  // namespace

extern "C" {

// host only: would create run a [K][N] weight matrix on two terms?  (w16_planes' own answer: the lo plane after the pre-scale)
int bh_debug_w16_two_terms(const float *W, size_t K, size_t N) try {
    if (!W || !K || !N || K > (1u << 24) || N > (1u << 24)) return fail(BH_ERR_INVALID, "debug_w16_two_terms: bad arguments");
    float unscale = 1.0f;
    bool lo_zero = false;
    (void)w16_planes(W, (int)K, (int)N, &unscale, &lo_zero);
    return lo_zero ? 1 : 0;
} catch (...) { return on_exception(); }

int bh_debug_last_gated_kernel(char *out, size_t cap) { return copy_name(g_last_gated_kernel.load(std::memory_order_relaxed), out, cap); }

// The gated project GEMM of a squeeze-excite block on operands of the caller's (tests: any shape, both layouts of D, every kernel
// behind launch_pw_gemm16_gated, without a model around it): C = (A x gate[row / rows_per_seg]) W + bias (+ R).
int bh_debug_gated_gemm(int device, const float *A, const float *gate, const float *W, const float *bias, const float *R, float *C,
                        size_t M, size_t K, size_t N, size_t rows_per_seg, int terms, int blocked) try {
    if (!A || !gate || !W || !bias || !C || !M || !K || !N || !rows_per_seg || M % rows_per_seg || K % 4 || (terms != 1 && terms != 2 && terms != 3))
        return fail(BH_ERR_INVALID, "debug_gated_gemm: bad arguments");
    if (blocked && (K % 16 || M % 16)) return fail(BH_ERR_INVALID, "debug_gated_gemm: blocked rows need K % 16 == 0 and M % 16 == 0");
    HIPCHK(hipSetDevice(device));
    float unscale = 1.0f;
    std::vector<uint16_t> planes;
    if (!debug_planes(W, (int)K, (int)N, terms, &unscale, planes))
        return fail(BH_ERR_UNSUPPORTED, "debug_gated_gemm: terms 2 needs a W made of f16 values (after the power-of-two pre-scale)");
    std::vector<float> Ab;
    if (blocked) {     // kernels.hpp MbDesc::dblk: [row tile of 16][K / 16][16 rows][16 channels]
        Ab.resize(M * K);
        for (size_t r = 0; r < M; r++)
            for (size_t k = 0; k < K; k++) Ab[((r >> 4) * (K / 16) + (k >> 4)) * 256 + (r & 15) * 16 + (k & 15)] = A[r * K + k];
    }
    DebugLaunch h{"debug_gated_gemm"};
    const float *da = h.in(blocked ? Ab.data() : A, M * K * 4), *dg = h.in(gate, M / rows_per_seg * K * 4), *dw = h.in(planes.data(), planes.size() * 2),
                *db = h.in(bias, N * 4), *dr = h.in(R, M * N * 4);
    float *dc = h.out(M * N, "C", C);
    if (!h.ok) return h.no_memory();
    const char *name = bh::launch_pw_gemm16_gated(da, dg, (int)rows_per_seg, dw, db, dr, dc, (int)M, (int)K, (int)N, terms, unscale, blocked, nullptr);
    g_last_gated_kernel.store(name, std::memory_order_relaxed);
    return h.finish(name, nullptr, 0);
} catch (...) { return on_exception(); }

// The same block's project GEMM on the f32 MFMA (a precision="f32" classifier's, and the one BH_FLAG_AUTO re-runs rows on), with
// create's row padding of W, through the call SliceRun::fused_se makes (include/birda_hip_gated_debug.h).
int bh_debug_gated_gemm_f32(int device, const float *A, const float *gate, const float *W, const float *bias, const float *R, float *C,
                            size_t M, size_t K, size_t N, size_t rows_per_seg, int act, char *kernel, size_t kernel_cap) try {
    if (!A || !gate || !W || !bias || !C || !M || !K || !N || !rows_per_seg || M % rows_per_seg || act < 0 || act > bh::ACT_LAST)
        return fail(BH_ERR_INVALID, "debug_gated_gemm_f32: bad arguments");
    if (M * K > (size_t)INT32_MAX || M * N > (size_t)INT32_MAX || K * N > (size_t)INT32_MAX || rows_per_seg > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_gated_gemm_f32: operands past 2^31 elements");
    if (K % 4) return fail(BH_ERR_UNSUPPORTED, "debug_gated_gemm_f32: K %zu is not a multiple of 4", K);
    HIPCHK(hipSetDevice(device));
    const size_t ld = align_up(N, 4);
    const std::vector<float> w = pw_gemm_rows(W, K, N, ld);
    DebugLaunch h{"debug_gated_gemm_f32"};
    const float *da = h.in(A, M * K * 4), *dg = h.in(gate, M / rows_per_seg * K * 4), *dw = h.in(w.data(), w.size() * 4), *db = h.in(bias, N * 4),
                *dr = h.in(R, M * N * 4);
    float *dc = h.out(M * N, "C", C);
    if (!h.ok) return h.no_memory();
    const char *name = bh::launch_pw_gemm_gated(da, dg, (int)rows_per_seg, dw, db, dr, dc, (int)M, (int)K, (int)N, (int)ld, act, nullptr, 0);
    if (!name) return fail(BH_ERR_INTERNAL, "debug_gated_gemm_f32: the launcher has no instantiation for N %zu", N);
    return h.finish(name, kernel, kernel_cap);
} catch (...) { return on_exception(); }

// One full convolution on the implicit-GEMM kernels, on operands of the caller's, with the weight preparation create does
// (conv_gemm_rows, w16_planes) -- tests drive every shape, precision and epilogue instantiation without a model around it.
// (after != 0: bh_debug_conv_gemm_after, include/birda_hip_resact_debug.h -- the activation after the residual add)
// (dil_h, dil_w: bh_debug_dilated_layer, include/birda_hip_dilated_debug.h -- the taps' pitch; 1, 1 from the other two entry points)
static int debug_conv_gemm(int device, const float *X, const float *W, const float *bias, const float *R, float *C, size_t n_seg,
                           const int32_t *shape, int act, int terms, char *kernel, size_t kernel_cap, int after, int dil_h = 1, int dil_w = 1) {
    if (!X || !W || !bias || !C || !shape || !n_seg || (terms != 0 && terms != 1 && terms != 2 && terms != 3) || act < 0 || act > bh::ACT_LAST)
        return fail(BH_ERR_INVALID, "debug_conv_gemm: bad arguments");
    if (after && !R) return fail(BH_ERR_INVALID, "debug_conv_gemm_after: the residual R is required");
    bh::ConvParams p = shape_params(shape, false, 4, 0, act, after ? 1 : 0);
    p.dil_h = dil_h; p.dil_w = dil_w;
    if (p.in_h < 1 || p.in_w < 1 || p.out_h < 1 || p.out_w < 1)
        return fail(BH_ERR_INVALID, "debug_conv_gemm: image %dx%d -> %dx%d", p.in_h, p.in_w, p.out_h, p.out_w);
    if ((p.kh == 1 && p.dil_h != 1) || (p.kw == 1 && p.dil_w != 1))   // (validate_model: one spelling of the undilated axis)
        return fail(BH_ERR_UNSUPPORTED, "debug_conv_gemm: dilation %dx%d on a %dx%d kernel: an axis with one tap is dilation 1", p.dil_h, p.dil_w, p.kh, p.kw);
    if (after ? (terms ? !bh::conv_gemm16_after_supports(p) : (!bh::conv_gemm_supports(p) || act == bh::ACT_NONE))
              : (terms ? !bh::conv_gemm16_supports(p) : !bh::conv_gemm_supports(p)))
        return fail(BH_ERR_UNSUPPORTED, "debug_conv_gemm%s: %dx%d stride %dx%d pad %d,%d dilation %dx%d, %d -> %d channels, %s not built for terms %d",
                    after ? "_after" : "", p.kh, p.kw, p.sh, p.sw, p.pad_t, p.pad_l, p.dil_h, p.dil_w, p.cin, p.cout, act_name(act), terms);
    const size_t M = n_seg * (size_t)p.out_h * p.out_w, x_floats = n_seg * (size_t)p.in_h * p.in_w * p.cin;
    if (M * (size_t)p.cout > (size_t)INT32_MAX || x_floats > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_conv_gemm: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    const size_t K = (size_t)p.kh * p.kw * align_up((size_t)p.cin, 32);
    const int ld = terms ? p.cout : (int)align_up((size_t)p.cout, 4);
    const std::vector<float> w = conv_gemm_rows(W, p, ld);
    float unscale = 1.0f;
    std::vector<uint16_t> planes;
    if (terms && !debug_planes(w.data(), (int)K, p.cout, terms, &unscale, planes))
        return fail(BH_ERR_UNSUPPORTED, "debug_conv_gemm: terms 2 needs a W made of f16 values (after the power-of-two pre-scale)");
    DebugLaunch h{"debug_conv_gemm"};
    const float *dx = h.in(X, x_floats * 4), *dw = terms ? h.in(planes.data(), planes.size() * 2) : h.in(w.data(), w.size() * 4),
                *db = h.in(bias, (size_t)p.cout * 4), *dr = h.in(R, M * p.cout * 4);
    float *dc = h.out(M * p.cout, "C", C);
    if (!h.ok) return h.no_memory();
    return h.finish(terms ? bh::launch_conv_gemm16(dx, dw, db, dr, dc, p, (int)n_seg, terms, unscale, nullptr)
                          : bh::launch_conv_gemm(dx, dw, db, dr, dc, p, (int)n_seg, ld, nullptr), kernel, kernel_cap);
}
int bh_debug_conv_gemm(int device, const float *X, const float *W, const float *bias, const float *R, float *C, size_t n_seg,
                       const int32_t *shape, int act, int terms, char *kernel, size_t kernel_cap) try {
    return debug_conv_gemm(device, X, W, bias, R, C, n_seg, shape, act, terms, kernel, kernel_cap, 0);
} catch (...) { return on_exception(); }
int bh_debug_conv_gemm_after(int device, const float *X, const float *W, const float *bias, const float *R, float *C, size_t n_seg,
                             const int32_t *shape, int act, int terms, char *kernel, size_t kernel_cap) try {
    return debug_conv_gemm(device, X, W, bias, R, C, n_seg, shape, act, terms, kernel, kernel_cap, 1);
} catch (...) { return on_exception(); }

// One dilated layer alone (include/birda_hip_dilated_debug.h): a full convolution through debug_conv_gemm with the taps' pitch, or a
// depthwise one through launch_dwconv, refusing what validate_model and create refuse.
int bh_debug_dilated_layer(int device, int op, const float *X, const float *W, const float *bias, const float *R, float *C, size_t n_seg,
                           const int32_t *shape, int act, int terms, int after, char *kernel, size_t kernel_cap) try {
    if (!shape || (op != bh::OP_CONV && op != bh::OP_DWCONV)) return fail(BH_ERR_INVALID, "debug_dilated_layer: op %d is neither a full nor a depthwise convolution", op);
    const int dil_h = shape[12], dil_w = shape[13];
    if (op == bh::OP_CONV) return debug_conv_gemm(device, X, W, bias, R, C, n_seg, shape, act, terms, kernel, kernel_cap, after ? 1 : 0, dil_h, dil_w);
    if (!X || !W || !bias || !C || !n_seg || n_seg > (size_t)INT32_MAX || act < 0 || act > bh::ACT_LAST || R || terms || after)
        return fail(BH_ERR_INVALID, "debug_dilated_layer: a depthwise layer takes X, W, bias and C, no residual, terms 0");
    bh::ConvParams p = shape_params(shape, false, 4, 0, act, 0);
    p.dil_h = dil_h; p.dil_w = dil_w;
    // (validate_model's ranges)
    if (p.in_h < 1 || p.in_w < 1 || p.out_h < 1 || p.out_w < 1 || p.in_h > 65536 || p.in_w > 65536 || p.out_h > 65536 || p.out_w > 65536 || p.cout < 1 ||
        p.cout > (1 << 24) || p.cin != p.cout || p.kh < 1 || p.kw < 1 || p.kh > 64 || p.kw > 64 || p.sh < 1 || p.sw < 1 || p.sh > 16 || p.sw > 16 ||
        p.pad_t < 0 || p.pad_l < 0 || p.pad_t > 64 || p.pad_l > 64)
        return fail(BH_ERR_INVALID, "debug_dilated_layer: layer dimensions out of range");
    if (p.dil_h < 1 || p.dil_w < 1 || p.dil_h > (int)bh::MAX_DILATION || p.dil_w > (int)bh::MAX_DILATION)
        return fail(BH_ERR_UNSUPPORTED, "debug_dilated_layer: dilation %dx%d (1 .. 16 are supported)", p.dil_h, p.dil_w);
    if (!bh::dwconv_supports(p))
        return fail(BH_ERR_UNSUPPORTED, "debug_dilated_layer: depthwise %dx%d stride %dx%d dilation %dx%d channels %d not built (square 3x3 / 5x5 / 7x7 windows, one "
                    "stride of 1 or 2, channels a multiple of 4)", p.kh, p.kw, p.sh, p.sw, p.dil_h, p.dil_w, p.cout);
    const size_t x_seg = (size_t)p.in_h * p.in_w * p.cout, y_seg = (size_t)p.out_h * p.out_w * p.cout;
    if (x_seg > (size_t)INT32_MAX || y_seg > (size_t)INT32_MAX || n_seg * x_seg > (size_t)INT32_MAX || n_seg * y_seg > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_dilated_layer: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    DebugLaunch h{"debug_dilated_layer"};
    const float *dx = h.in(X, n_seg * x_seg * 4), *dwt = h.in(W, (size_t)p.kh * p.kw * p.cout * 4), *db = h.in(bias, (size_t)p.cout * 4);
    float *dy = h.out(n_seg * y_seg, "C", C);
    if (!h.ok) return h.no_memory();
    const char *name = bh::launch_dwconv(dx, dwt, db, dy, p, (int)n_seg, nullptr);
    if (!name) return fail(BH_ERR_INTERNAL, "debug_dilated_layer: the launcher has no instantiation for a shape dwconv_supports accepts");
    return h.finish(name, kernel, kernel_cap);
} catch (...) { return on_exception(); }

// One channel LayerNorm launch alone on operands of the caller's, through the launcher a forward pass takes
// (include/birda_hip_lnorm_debug.h).
int bh_debug_lnorm(int device, const float *X, const float *gamma, const float *beta, float eps, float *out, size_t n_pixels_total, size_t C,
                   char *name, size_t name_len) try {
    if (!X || !gamma || !beta || !out || !n_pixels_total || !C) return fail(BH_ERR_INVALID, "debug_lnorm: bad arguments");
    if (!std::isfinite(eps) || !(eps > 0.0f)) return fail(BH_ERR_INVALID, "debug_lnorm: eps %g is not finite and > 0", (double)eps);
    if (C > (size_t)INT32_MAX || !bh::lnorm_supports((int)C))
        return fail(BH_ERR_UNSUPPORTED, "debug_lnorm: layer norm over %zu channels not built (a multiple of 4, 4 .. 2048)", C);
    if (n_pixels_total > (size_t)INT32_MAX || n_pixels_total * C > (size_t)INT32_MAX) return fail(BH_ERR_INVALID, "debug_lnorm: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    DebugLaunch h{"debug_lnorm"};
    const float *dx = h.in(X, n_pixels_total * C * 4), *dg = h.in(gamma, C * 4), *db = h.in(beta, C * 4);
    float *dy = h.out(n_pixels_total * C, "out", out);
    if (!h.ok) return h.no_memory();
    const char *kn = bh::launch_lnorm(dx, dg, db, dy, (unsigned long long)n_pixels_total, (int)C, eps, nullptr);
    if (!kn) return fail(BH_ERR_INTERNAL, "debug_lnorm: the launcher has no instantiation for a width lnorm_supports accepts");
    return h.finish(kn, name, name_len);
} catch (...) { return on_exception(); }

// One norm + activation launch alone on operands of the caller's, through the launcher a forward pass takes
// (include/birda_hip_bnact_debug.h).
int bh_debug_bnact(int device, const float *X, const float *scale, const float *shift, int act, float *out, size_t n_pixels_total, size_t C,
                   char *name, size_t name_len) try {
    if (!X || !scale || !shift || !out || !n_pixels_total || !C) return fail(BH_ERR_INVALID, "debug_bnact: bad arguments");
    if (C > (size_t)(1 << 16) || C % 4)
        return fail(BH_ERR_UNSUPPORTED, "debug_bnact: norm + activation over %zu channels not built (a multiple of 4, 4 .. 65 536)", C);
    if (!bh::bnact_supports((int)C, act))
        return fail(BH_ERR_INVALID, "debug_bnact: activation %d (RELU, RELU6, SWISH, GELU_ERF, GELU_TANH or HSWISH: 1 .. 5, 7)", act);
    if (n_pixels_total > (size_t)INT32_MAX || n_pixels_total * C > (size_t)INT32_MAX) return fail(BH_ERR_INVALID, "debug_bnact: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    DebugLaunch h{"debug_bnact"};
    const float *dx = h.in(X, n_pixels_total * C * 4), *da = h.in(scale, C * 4), *db = h.in(shift, C * 4);
    float *dy = h.out(n_pixels_total * C, "out", out);
    if (!h.ok) return h.no_memory();
    const char *kn = bh::launch_bnact(dx, da, db, dy, (unsigned long long)n_pixels_total, (int)C, act, nullptr);
    if (!kn) return fail(BH_ERR_INTERNAL, "debug_bnact: the launcher has no instantiation for a width and an activation bnact_supports accepts");
    return h.finish(kn, name, name_len);
} catch (...) { return on_exception(); }

// The same launch on DEVICE buffers of the caller's, for the timing tool (include/birda_hip_bnact_debug.h): no copies, no guard bands.
int bh_debug_bnact_on_device(int device, const float *dX, const float *dScale, const float *dShift, int act, float *dOut, size_t n_seg, size_t pixels,
                             size_t C, char *name, size_t name_len) try {
    if (!dX || !dScale || !dShift || !dOut || !n_seg || !pixels || !C) return fail(BH_ERR_INVALID, "debug_bnact_on_device: bad arguments");
    if (C > (size_t)(1 << 16) || C % 4) return fail(BH_ERR_UNSUPPORTED, "debug_bnact_on_device: %zu channels not built (a multiple of 4, 4 .. 65 536)", C);
    if (n_seg > (size_t)INT32_MAX || pixels > (size_t)INT32_MAX || n_seg * pixels > ((size_t)1 << 40) / C)
        return fail(BH_ERR_INVALID, "debug_bnact_on_device: tensors past 2^40 elements");
    if (!bh::bnact_supports((int)C, act)) return fail(BH_ERR_INVALID, "debug_bnact_on_device: activation %d (RELU, RELU6, SWISH, GELU_ERF, GELU_TANH or HSWISH: 1 .. 5, 7)", act);
    HIPCHK(hipSetDevice(device));
    const char *kn = bh::launch_bnact(dX, dScale, dShift, dOut, (unsigned long long)n_seg * pixels, (int)C, act, nullptr);
    if (!kn) return fail(BH_ERR_INTERNAL, "debug_bnact_on_device: the launcher has no instantiation for this shape");
    HIPCHK(hipGetLastError());
    if (name && name_len) snprintf(name, name_len, "%s", kn);
    return BH_OK;
} catch (...) { return on_exception(); }

// The timing tool's yardstick, an entry of its own: scale_kernel (launch_scale, the squeeze-excite layer's x times a [n_seg][C] gate), the nearest
// existing kernel, over the same tensor on DEVICE buffers of the caller's (include/birda_hip_bnact_debug.h).
int bh_debug_scale_on_device(int device, const float *dX, const float *dGate, float *dOut, size_t n_seg, size_t pixels, size_t C, char *name,
                             size_t name_len) try {
    if (!dX || !dGate || !dOut || !n_seg || !pixels || !C) return fail(BH_ERR_INVALID, "debug_scale_on_device: bad arguments");
    if (C > (size_t)(1 << 16) || C % 4) return fail(BH_ERR_UNSUPPORTED, "debug_scale_on_device: %zu channels not built (a multiple of 4, 4 .. 65 536)", C);
    if (n_seg > (size_t)INT32_MAX || pixels > (size_t)INT32_MAX || pixels * (C / 4) > (size_t)INT32_MAX || n_seg * pixels > ((size_t)1 << 40) / C)
        return fail(BH_ERR_INVALID, "debug_scale_on_device: tensors past 2^40 elements (or a segment past 2^31 float4s)");
    HIPCHK(hipSetDevice(device));
    const char *kn = bh::launch_scale(dX, dGate, dOut, (int)n_seg, (int)pixels, (int)C, nullptr);
    HIPCHK(hipGetLastError());
    if (name && name_len) snprintf(name, name_len, "%s", kn);
    return BH_OK;
} catch (...) { return on_exception(); }

// One grouped convolution alone on operands of the caller's, with create's weight preparation (gconv_matrix, gconv_fragments,
// w16_planes), through the launchers a forward pass takes (include/birda_hip_gconv_debug.h).
int bh_debug_gconv(int device, const float *X, const float *W, const float *bias, float *C, size_t n_seg, const int32_t *shape, int act,
                   int terms, char *kernel, size_t kernel_cap) try {
    if (!X || !W || !bias || !C || !shape || !n_seg || terms < 0 || terms > 3 || act < 0 || act > bh::ACT_LAST)
        return fail(BH_ERR_INVALID, "debug_gconv: bad arguments");
    const bh::ConvParams p = shape_params(shape, false, 4, 0, act, 0);
    const int G = shape[12];
    if (p.in_h < 1 || p.in_w < 1 || p.out_h < 1 || p.out_w < 1 || p.in_h > 65536 || p.in_w > 65536 || p.out_h > 65536 || p.out_w > 65536 ||
        p.cin > 65536 || p.cout > (1 << 24))
        return fail(BH_ERR_INVALID, "debug_gconv: image %dx%d -> %dx%d, %d -> %d channels", p.in_h, p.in_w, p.out_h, p.out_w, p.cin, p.cout);
    if (terms == 2 || !bh::gconv_supports(p, G))
        return fail(BH_ERR_UNSUPPORTED, "debug_gconv: %dx%d stride %dx%d pad %d,%d, %d -> %d channels in %d groups, %s not built for terms %d",
                    p.kh, p.kw, p.sh, p.sw, p.pad_t, p.pad_l, p.cin, p.cout, G, act_name(act), terms);
    const size_t M = n_seg * (size_t)p.out_h * p.out_w, x_floats = n_seg * (size_t)p.in_h * p.in_w * p.cin;
    if (M * (size_t)p.cout > (size_t)INT32_MAX || x_floats > (size_t)INT32_MAX || n_seg > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_gconv: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    int K = 0;
    const int nt = (p.cout + 15) / 16;
    const std::vector<float> wt = gconv_matrix(W, p, G, &K);
    float unscale = 1.0f;
    std::vector<uint16_t> planes;
    std::vector<float> frags;
    if (terms) planes = w16_planes(wt.data(), K, nt * 16, &unscale);
    else frags = gconv_fragments(wt, K, nt);
    DebugLaunch h{"debug_gconv"};
    const float *dx = h.in(X, x_floats * 4), *dw = terms ? h.in(planes.data(), planes.size() * 2) : h.in(frags.data(), frags.size() * 4),
                *db = h.in(bias, (size_t)p.cout * 4);
    float *dc = h.out(M * p.cout, "C", C);
    if (!h.ok) return h.no_memory();
    const char *name = terms ? bh::launch_gconv16(dx, dw, db, dc, p, G, (int)n_seg, terms, unscale, nullptr)
                             : bh::launch_gconv(dx, dw, db, dc, p, G, (int)n_seg, nullptr);
    if (!name) return fail(BH_ERR_UNSUPPORTED, "debug_gconv: a launch of %zu rows is beyond the grid", M);
    return h.finish(name, kernel, kernel_cap);
} catch (...) { return on_exception(); }

// A pointwise / dense layer (pool_rows == 0) or the fused head convolution + pool (pool_rows = pixels per segment) on operands of
// the caller's, with create's weight preparation (pw_gemm_rows, w16_planes), through the launchers a forward pass calls.
// (after != 0: bh_debug_layer_gemm_after, include/birda_hip_resact_debug.h)
static int debug_layer_gemm(int device, const float *A, const float *W, const float *bias, const float *R, float *C, size_t M, size_t K,
                            size_t N, size_t pool_rows, int act, int terms, char *kernel, size_t kernel_cap, int after) {
    if (after && (!R || pool_rows)) return fail(BH_ERR_INVALID, "debug_layer_gemm_after: the residual R is required, and no head pool");
    if (!A || !W || !bias || !C || !M || !K || !N || (terms != 0 && terms != 1 && terms != 2 && terms != 3) || act < 0 || act > bh::ACT_LAST)
        return fail(BH_ERR_INVALID, "debug_layer_gemm: bad arguments");
    if (M * K > (size_t)INT32_MAX || M * N > (size_t)INT32_MAX || K * N > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_layer_gemm: operands past 2^31 elements");
    if (pool_rows) {
        if (R || !terms || M % pool_rows)
            return fail(BH_ERR_INVALID, "debug_layer_gemm: the head pool takes no residual, split-f16 terms and whole segments");
        if (!bh::head_gap16_supports((int)pool_rows, (int)K, (int)N, act))
            return fail(BH_ERR_UNSUPPORTED, "debug_layer_gemm: head pool of %zu pixels, K %zu, N %zu, %s not built", pool_rows, K, N, act_name(act));
    } else if (after ? (terms ? !bh::pw_gemm16_after_supports((int)K, act) : (K % 4 != 0 || act == bh::ACT_NONE))
                     : (terms ? !bh::pw_gemm16_supports((int)K, act) : K % 4 != 0)) {
        return fail(BH_ERR_UNSUPPORTED, "debug_layer_gemm%s: K %zu, %s not built for terms %d", after ? "_after" : "", K, act_name(act), terms);
    }
    HIPCHK(hipSetDevice(device));
    const size_t ld = align_up(N, 4), out_rows = pool_rows ? M / pool_rows : M;
    float unscale = 1.0f;
    std::vector<uint16_t> planes;
    std::vector<float> w;
    if (terms) {
        if (!debug_planes(W, (int)K, (int)N, terms, &unscale, planes))
            return fail(BH_ERR_UNSUPPORTED, "debug_layer_gemm: terms 2 needs a W made of f16 values (after the power-of-two pre-scale)");
    } else w = pw_gemm_rows(W, K, N, ld);
    DebugLaunch h{"debug_layer_gemm"};
    const float *da = h.in(A, M * K * 4), *dw = terms ? h.in(planes.data(), planes.size() * 2) : h.in(w.data(), w.size() * 4),
                *db = h.in(bias, N * 4), *dr = h.in(R, M * N * 4);
    float *dc = h.out(out_rows * N, "C", C);
    if (!h.ok) return h.no_memory();
    return h.finish(pool_rows ? bh::launch_head_gap16(da, dw, db, dc, (int)out_rows, (int)pool_rows, (int)K, (int)N, act, terms, unscale, nullptr)
                    : terms   ? bh::launch_pw_gemm16(da, dw, db, dr, dc, (int)M, (int)K, (int)N, act, terms, unscale, nullptr, after)
                              : bh::launch_pw_gemm(da, dw, db, dr, dc, (int)M, (int)K, (int)N, (int)ld, act, nullptr, after), kernel, kernel_cap);
}
int bh_debug_layer_gemm(int device, const float *A, const float *W, const float *bias, const float *R, float *C, size_t M, size_t K,
                        size_t N, size_t pool_rows, int act, int terms, char *kernel, size_t kernel_cap) try {
    return debug_layer_gemm(device, A, W, bias, R, C, M, K, N, pool_rows, act, terms, kernel, kernel_cap, 0);
} catch (...) { return on_exception(); }
int bh_debug_layer_gemm_after(int device, const float *A, const float *W, const float *bias, const float *R, float *C, size_t M, size_t K,
                              size_t N, size_t pool_rows, int act, int terms, char *kernel, size_t kernel_cap) try {
    return debug_layer_gemm(device, A, W, bias, R, C, M, K, N, pool_rows, act, terms, kernel, kernel_cap, 1);
} catch (...) { return on_exception(); }

// One pool layer alone on operands of the caller's, through the launcher a forward pass takes (include/birda_hip_pool_debug.h).
int bh_debug_pool(int device, const float *X, float *Y, size_t n_seg, const int32_t *shape, int mode, char *kernel, size_t kernel_cap) try {
    if (!X || !Y || !shape || !n_seg) return fail(BH_ERR_INVALID, "debug_pool: bad arguments");
    const bh::ConvParams p = shape_params(shape, true, 4, 0, 0, 0);
    if (!bh::pool_supports(p, mode))
        return fail(BH_ERR_UNSUPPORTED, "debug_pool: %dx%d -> %dx%d, %d channels, window %dx%d stride %dx%d pad %d,%d, mode %d: not a pool the model "
                    "validator accepts (channels a multiple of 4, mode 0..2, every window holding a pixel of the image)",
                    p.in_h, p.in_w, p.out_h, p.out_w, p.cout, p.kh, p.kw, p.sh, p.sw, p.pad_t, p.pad_l, mode);
    const size_t x_floats = n_seg * (size_t)p.in_h * p.in_w * p.cout, y_floats = n_seg * (size_t)p.out_h * p.out_w * p.cout;
    if (x_floats > (size_t)INT32_MAX || y_floats > (size_t)INT32_MAX || n_seg > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_pool: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    DebugLaunch h{"debug_pool"};
    const float *dx = h.in(X, x_floats * 4);
    float *dy = h.out(y_floats, "Y", Y);
    if (!h.ok) return h.no_memory();
    return h.finish(bh::launch_pool(dx, dy, p, mode, (int)n_seg, nullptr), kernel, kernel_cap);
} catch (...) { return on_exception(); }

// One reduce layer alone on operands of the caller's, through the launcher a forward pass takes (include/birda_hip_reduce_debug.h).
int bh_debug_reduce(int device, const float *X, float *Y, size_t n_seg, const int32_t *shape, int mode, int split, char *kernel, size_t kernel_cap) try {
    if (!X || !Y || !shape || !n_seg) return fail(BH_ERR_INVALID, "debug_reduce: bad arguments");
    const bh::ConvParams p{shape[0], shape[1], shape[2], shape[3], shape[4], shape[4], shape[5], shape[6], 1, 1, 0, 0, 0, 0};
    if (!bh::reduce_supports(p, mode))
        return fail(BH_ERR_UNSUPPORTED, "debug_reduce: %dx%d -> %dx%d, %d channels, window %dx%d, mode %d: not a reduce the model validator accepts (not built: "
                    "channels a multiple of 4, mode 0..2, a window of the whole axis or 1 along each axis and not 1x1, at most 65 536 taps, the mean over "
                    "both axes is the global pool's)", p.in_h, p.in_w, p.out_h, p.out_w, p.cout, p.kh, p.kw, mode);
    if (split != 0 && split != 1 && split != 8) return fail(BH_ERR_INVALID, "debug_reduce: split %d (0: the launcher's choice; 1 or 8)", split);
    const size_t x_floats = n_seg * (size_t)p.in_h * p.in_w * p.cout, y_floats = n_seg * (size_t)p.out_h * p.out_w * p.cout;
    if (x_floats > (size_t)INT32_MAX || y_floats > (size_t)INT32_MAX || n_seg > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_reduce: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    DebugLaunch h{"debug_reduce"};
    const float *dx = h.in(X, x_floats * 4);
    float *dy = h.out(y_floats, "Y", Y);
    if (!h.ok) return h.no_memory();
    const char *kn = bh::launch_reduce(dx, dy, p, mode, (int)n_seg, nullptr, split);
    if (!kn) return fail(BH_ERR_INTERNAL, "debug_reduce: the launcher has no instantiation for a shape reduce_supports accepts");
    return h.finish(kn, kernel, kernel_cap);
} catch (...) { return on_exception(); }

// The same launch on DEVICE buffers of the caller's, for the timing tool (include/birda_hip_reduce_debug.h): no copies, no guard bands.
int bh_debug_reduce_on_device(int device, const float *dX, float *dY, size_t n_seg, const int32_t *shape, int mode, int split, char *kernel,
                              size_t kernel_cap) try {
    if (!dX || !dY || !shape || !n_seg || n_seg > (size_t)INT32_MAX) return fail(BH_ERR_INVALID, "debug_reduce_on_device: bad arguments");
    const bh::ConvParams p{shape[0], shape[1], shape[2], shape[3], shape[4], shape[4], shape[5], shape[6], 1, 1, 0, 0, 0, 0};
    const bool gap = mode == 3;     // the yardstick: gap_kernel, the mean over the whole image
    if (!bh::reduce_supports(p, gap ? 0 : mode) || (gap && (p.kh != p.in_h || p.kw != p.in_w)))
        return fail(BH_ERR_UNSUPPORTED, "debug_reduce_on_device: %dx%d, %d channels, window %dx%d, mode %d not built", p.in_h, p.in_w, p.cout, p.kh, p.kw, mode);
    if (split != 0 && split != 1 && split != 8) return fail(BH_ERR_INVALID, "debug_reduce_on_device: split %d (0, 1 or 8)", split);
    HIPCHK(hipSetDevice(device));
    const char *kn = gap ? bh::launch_gap(dX, dY, (int)n_seg, p.in_h * p.in_w, p.cout, nullptr) : bh::launch_reduce(dX, dY, p, mode, (int)n_seg, nullptr, split);
    if (!kn) return fail(BH_ERR_INTERNAL, "debug_reduce_on_device: the launcher has no instantiation for this shape");
    HIPCHK(hipGetLastError());
    if (kernel && kernel_cap) snprintf(kernel, kernel_cap, "%s", kn);
    return BH_OK;
} catch (...) { return on_exception(); }

// The gate of one squeeze-excite block alone on operands of the caller's, in the form a forward pass takes for its widths
// (se_gate_form) or a forced one, with create's row padding of W1 and W2 and scratch buffers of the forward's sizes
// (include/birda_hip_gate_debug.h).
int bh_debug_se_gate(int device, const float *part, size_t n_seg, size_t tiles, size_t P, size_t C, size_t Cr, const float *W1, const float *b1,
                     int act1, const float *W2, const float *b2, int act2, int form, float *gate, char *kernel, size_t kernel_cap) try {
    if (!part || !W1 || !b1 || !W2 || !b2 || !gate || !n_seg || !tiles || !P || !C || !Cr || form < -1 || form > 2 || act1 < 0 ||
        act1 > bh::ACT_LAST || act2 < 0 || act2 > bh::ACT_LAST)
        return fail(BH_ERR_INVALID, "debug_se_gate: bad arguments");
    if (C > (1u << 24) || Cr > (1u << 24) || tiles > (1u << 24) || P > (size_t)INT32_MAX || n_seg > (size_t)INT32_MAX ||
        tiles * C > (size_t)INT32_MAX || n_seg * (tiles * C) > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_se_gate: operands past 2^31 elements");
    const int c = (int)C, cr = (int)Cr;
    if (form < 0 && (form = se_gate_form(c, cr)) < 0)
        return fail(BH_ERR_UNSUPPORTED, "debug_se_gate: no form of the gate takes %d -> %d -> %d channels", c, cr, c);
    if (form == 0 && !bh::se_gate_supports(c, cr))
        return fail(BH_ERR_UNSUPPORTED, "debug_se_gate: the one-launch gate keeps C + 256 + Cr floats in 64 KiB of LDS and at most 256 hidden channels: %d, %d", c, cr);
    if (form == 1 && !bh::se_gate16_supports(c, cr))
        return fail(BH_ERR_UNSUPPORTED, "debug_se_gate: the partial hidden sums of %d -> %d channels do not fit n_seg x C floats (or Cr > 256)", c, cr);
    if (form == 2 && (C % 4 || Cr % 4))
        return fail(BH_ERR_UNSUPPORTED, "debug_se_gate: the GEMM form needs C and Cr multiples of 4: %d, %d", c, cr);
    HIPCHK(hipSetDevice(device));
    const size_t ld1 = align_up(Cr, 4), ld2 = align_up(C, 4);
    const std::vector<float> w1 = pw_gemm_rows(W1, C, Cr, ld1), w2 = pw_gemm_rows(W2, Cr, C, ld2);
    DebugLaunch h{"debug_se_gate"};
    const float *dp = h.in(part, n_seg * tiles * C * 4), *d1 = h.in(w1.data(), w1.size() * 4), *db1 = h.in(b1, Cr * 4),
                *d2 = h.in(w2.data(), w2.size() * 4), *db2 = h.in(b2, C * 4);
    float *pooled = form != 0 ? h.out(n_seg * C, "the pooled / partial-sum scratch", nullptr) : nullptr;
    float *hidden = form == 2 ? h.out(n_seg * Cr, "the hidden scratch", nullptr) : nullptr;
    float *dg = h.out(n_seg * C, "gate", gate);
    if (!h.ok) return h.no_memory();
    const char *name =
        form == 1 ? bh::launch_se_gate16(dp, (int)tiles, (int)P, pooled, d1, db1, (int)ld1, act1, d2, db2, (int)ld2, act2, dg, (int)n_seg, c, cr, nullptr)
      : form == 2 ? bh::launch_se_gate_gemm(dp, (int)tiles, (int)P, pooled, hidden, d1, db1, (int)ld1, act1, d2, db2, (int)ld2, act2, dg, (int)n_seg, c, cr, nullptr)
                  : bh::launch_se_gate(dp, (int)tiles, (int)P, d1, db1, (int)ld1, act1, d2, db2, (int)ld2, act2, dg, (int)n_seg, c, cr, nullptr);
    if (!name) {   // (the launches of the form before that GEMM are under way: wait for them, then refuse)
        const int rc = h.sync();
        return rc != BH_OK ? rc : fail(BH_ERR_INTERNAL, "debug_se_gate: a GEMM of the three-launch form had no instantiation");
    }
    return h.finish(name, kernel, kernel_cap);
} catch (...) { return on_exception(); }

// One plain f32 layer (depthwise, the NCHW stem's direct convolution, global average pool, gate multiply) alone on operands of the
// caller's, through the launcher SliceRun::layer takes, refusing what create refuses for the op (include/birda_hip_gate_debug.h).
int bh_debug_plain_layer(int device, int op, const float *X, const float *W, const float *bias, const float *gate, float *Y, size_t n_seg,
                         const int32_t *shape, int act, char *kernel, size_t kernel_cap) try {
    if (!X || !Y || !shape || !n_seg || n_seg > (size_t)INT32_MAX || act < 0 || act > bh::ACT_LAST)
        return fail(BH_ERR_INVALID, "debug_plain_layer: bad arguments");
    const bool conv = op == bh::OP_CONV, dw = op == bh::OP_DWCONV, gap = op == bh::OP_GAP, scale = op == bh::OP_SCALE;
    if (!conv && !dw && !gap && !scale) return fail(BH_ERR_INVALID, "debug_plain_layer: op %d is not one of the plain layers", op);
    if (((conv || dw) && (!W || !bias)) || (scale && !gate)) return fail(BH_ERR_INVALID, "debug_plain_layer: null operand");
    const bh::ConvParams p = shape_params(shape, true, conv ? 11 : 4, conv ? 1 : 0, act, 0);
    // (validate_model's ranges)
    if (p.in_h < 1 || p.in_w < 1 || p.out_h < 1 || p.out_w < 1 || p.in_h > 65536 || p.in_w > 65536 || p.out_h > 65536 || p.out_w > 65536 || p.cin < 1 ||
        p.cin > 65536 || p.cout < 1 || p.cout > (1 << 24) || p.kh < 1 || p.kw < 1 || p.kh > 64 || p.kw > 64 || p.sh < 1 || p.sw < 1 || p.sh > 16 ||
        p.sw > 16 || p.pad_t < 0 || p.pad_l < 0 || p.pad_t > 64 || p.pad_l > 64)
        return fail(BH_ERR_INVALID, "debug_plain_layer: layer dimensions out of range");
    if (gap && (p.out_h != 1 || p.out_w != 1)) return fail(BH_ERR_INVALID, "debug_plain_layer: a global pool leaves one pixel");
    if (scale && (p.out_h != p.in_h || p.out_w != p.in_w)) return fail(BH_ERR_INVALID, "debug_plain_layer: a gate multiply keeps the image");
    // (this entry keeps the windows it always took -- tests/test_gate_layers_gpu.py holds it to refusing every other one --; the 7x7
    //  window, dilated or not, runs through bh_debug_dilated_layer, whose dilation 1 is the plain layer's launch)
    if (dw && (!bh::dwconv_supports(p) || p.kh == 7))
        return fail(BH_ERR_UNSUPPORTED, "debug_plain_layer: depthwise %dx%d stride %dx%d channels %d not built here (this entry takes square 3x3 / 5x5 windows, one stride of "
                    "1 or 2, channels a multiple of 4; a 7x7 window runs through bh_debug_dilated_layer)", p.kh, p.kw, p.sh, p.sw, p.cout);
    if (conv && !bh::conv_direct_supports(p))
        return fail(BH_ERR_UNSUPPORTED, "debug_plain_layer: direct conv shape not built (output channels a multiple of 4, %dx%dx%dx%d weights within 64 KiB of LDS)",
                    p.kh, p.kw, p.cin, p.cout);
    if ((gap || scale) && p.cout % 4) return fail(BH_ERR_UNSUPPORTED, "debug_plain_layer: channels %d not a multiple of 4", p.cout);
    // (n_seg < 2^31 and a segment <= 2^16 x 2^16 x 2^24 is checked per segment first: none of these products wraps)
    const size_t x_seg = (size_t)p.in_h * p.in_w, y_seg = (size_t)p.out_h * p.out_w;
    if (x_seg * (conv ? p.cin : p.cout) > (size_t)INT32_MAX || y_seg * p.cout > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_plain_layer: tensors past 2^31 elements");
    const size_t x_floats = n_seg * (x_seg * (conv ? p.cin : p.cout)), y_floats = n_seg * (y_seg * p.cout);
    const size_t w_floats = conv ? (size_t)p.kh * p.kw * p.cin * p.cout : (size_t)p.kh * p.kw * p.cout;
    if (x_floats > (size_t)INT32_MAX || y_floats > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_plain_layer: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    DebugLaunch h{"debug_plain_layer"};
    const float *dx = h.in(X, x_floats * 4), *dwt = h.in(conv || dw ? W : nullptr, w_floats * 4), *db = h.in(conv || dw ? bias : nullptr, (size_t)p.cout * 4),
                *dg = h.in(scale ? gate : nullptr, n_seg * p.cout * 4);
    float *dy = h.out(y_floats, "Y", Y);
    if (!h.ok) return h.no_memory();
    const char *name = dw   ? bh::launch_dwconv(dx, dwt, db, dy, p, (int)n_seg, nullptr)
                     : conv ? bh::launch_conv_direct(dx, dwt, db, dy, p, (int)n_seg, nullptr)
                     : gap  ? bh::launch_gap(dx, dy, (int)n_seg, p.in_h * p.in_w, p.cout, nullptr)
                            : bh::launch_scale(dx, dg, dy, (int)n_seg, p.out_h * p.out_w, p.cout, nullptr);
    if (!name) return fail(BH_ERR_INTERNAL, "debug_plain_layer: the launcher has no instantiation for a shape the validator accepts");
    return h.finish(name, kernel, kernel_cap);
} catch (...) { return on_exception(); }

// One concat / window / shuffle launch alone on operands of the caller's, through the launcher a forward pass takes
// (include/birda_hip_concat_debug.h).
int bh_debug_concat(int device, const float *const *X, int n_src, float *Y, size_t n_seg, const int32_t *shape, char *kernel, size_t kernel_cap) try {
    if (!X || !Y || !shape || !n_seg || n_src < 1 || n_src > 4) return fail(BH_ERR_INVALID, "debug_concat: bad arguments");
    for (int k = 0; k < n_src; k++) if (!X[k]) return fail(BH_ERR_INVALID, "debug_concat: source %d is null", k);
    const int h = shape[0], w = shape[1], groups = shape[2];
    bh::ConcatSource src[4] = {};
    long long C = 0;
    for (int k = 0; k < n_src; k++) {
        const int32_t *q = shape + 3 + 3 * k;
        if (q[0] % 4 || q[0] < 4) return fail(BH_ERR_UNSUPPORTED, "debug_concat: source %d has %d channels (a multiple of 4 is needed)", k, q[0]);
        src[k] = bh::ConcatSource{nullptr, q[0] / 4, q[1], q[2]};
        C += q[2];
    }
    if (!bh::concat_supports(h, w, src, n_src, groups))
        return fail(BH_ERR_UNSUPPORTED, "debug_concat: %dx%d image, %d sources, %lld channels, %d groups: not a concat the model validator accepts (offsets and "
                    "lengths multiples of 4, windows inside their sources, groups dividing the channels)", h, w, n_src, C, groups);
    const size_t px = n_seg * (size_t)h * w, y_floats = px * (size_t)C;
    if (y_floats > (size_t)INT32_MAX || n_seg > (size_t)INT32_MAX) return fail(BH_ERR_INVALID, "debug_concat: tensors past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    DebugLaunch dl{"debug_concat"};
    for (int k = 0; k < n_src; k++) {
        const size_t x_floats = px * 4 * (size_t)src[k].total4;
        if (x_floats > (size_t)INT32_MAX) return fail(BH_ERR_INVALID, "debug_concat: tensors past 2^31 elements");
        src[k].p = dl.in(X[k], x_floats * 4);
    }
    float *dy = dl.out(y_floats, "Y", Y);
    if (!dl.ok) return dl.no_memory();
    return dl.finish(bh::launch_concat(src, n_src, dy, h, w, groups, (int)n_seg, nullptr), kernel, kernel_cap);
} catch (...) { return on_exception(); }

int bh_debug_mbconv_plan(const int32_t *shape, int force_cfg, int variant, int32_t *record, char *name, size_t name_cap) try {
    bh::MbDesc d{};
    return mb_debug_plan(shape, force_cfg, variant, d, record, name, name_cap);
} catch (...) { return on_exception(); }

// One fused block alone on operands of the caller's: mb_plan's choice (or the forced entry), plan_fusion's weight preparation
// (mb_prepare_weights), the launch a forward pass makes -- tests hold every output element of every instantiation to float64.
int bh_debug_mbconv_block(int device, const int32_t *shape, size_t n_seg, const float *X, const float *We, const float *be, const float *Wd,
                          const float *bd, const float *Wp, const float *bp, const float *R, const float *gate, int force_cfg, int variant,
                          int ksplit, float *Y, float *D, float *pool_part, int32_t *record, char *name, size_t name_cap) try {
    bh::MbDesc d{};
    int rc = mb_debug_plan(shape, force_cfg, variant, d, record, name, name_cap);
    if (rc != BH_OK) return rc;
    if (!n_seg || !X || !Wd || !bd || !Wp || !bp || (!d.noexp && (!We || !be)) || (d.se ? !pool_part : !Y))
        return fail(BH_ERR_INVALID, "debug_mbconv_block: null operand");
    if (d.se && (R || gate || ksplit)) return fail(BH_ERR_INVALID, "debug_mbconv_block: pass A takes no residual, gate or channel split");
    if (gate && !d.noexp && !d.stem) return fail(BH_ERR_INVALID, "debug_mbconv_block: the gated one-launch form is the no-expand and stem blocks'");
    if (gate && ksplit) return fail(BH_ERR_INVALID, "debug_mbconv_block: no channel split with a gate");
    const size_t P = (size_t)d.Ho * d.Wo, tiles = (size_t)d.tiles_x * d.tiles_y;
    const size_t x_fl = n_seg * (d.stem ? (size_t)d.stem_c * d.stem_h * d.stem_w : (size_t)d.H * d.W * d.Cin);
    const size_t y_fl = n_seg * P * d.Cout, d_fl = n_seg * P * d.Cexp, pp_fl = n_seg * tiles * d.Cexp;
    if (x_fl > (size_t)INT32_MAX || y_fl > (size_t)INT32_MAX || d_fl > (size_t)INT32_MAX)
        return fail(BH_ERR_INVALID, "debug_mbconv_block: tensors past 2^31 elements");
    if (d.dblk && (n_seg * P) % 16) return fail(BH_ERR_INVALID, "debug_mbconv_block: blocked D needs whole row tiles");
    const int ksp = ksplit ? mb_ksplit_of(d) : 1;
    if (record) record[12] = ksp;
    HIPCHK(hipSetDevice(device));
    MbHostWeights hw;
    mb_prepare_weights(d, We, be, Wd, bd, Wp, bp, hw);
    DebugLaunch h{"debug_mbconv_block"};
    d.X = h.in(X, x_fl * 4); d.We = h.in(hw.we.data(), hw.we.size() * 4); d.Wp = h.in(hw.wp.data(), hw.wp.size() * 4);
    d.Wd = h.in(hw.wd.data(), hw.wd.size() * 4); d.bp = h.in(hw.spa ? hw.bp.data() : bp, (size_t)d.Cout * 4);
    d.R = h.in(R, y_fl * 4); d.gate = h.in(gate, n_seg * d.Cexp * 4);
    d.Y = d.se ? nullptr : h.out(y_fl, "Y", Y);
    d.Dout = d.se && D ? h.out(d_fl, "D", D) : nullptr;
    d.pool_part = d.se ? h.out(pp_fl, "pool_part", pool_part) : nullptr;
    d.ksplit = ksp > 1 ? ksp : 0; d.partial = ksp > 1 ? h.out((size_t)ksp * y_fl, "partial", nullptr) : nullptr;
    if (!h.ok) return h.no_memory();
    bh::launch_mbconv(d, (int)n_seg, nullptr);
    if (ksp > 1) bh::launch_mb_reduce_partials(d.partial, d.Y, ksp, y_fl, d.prec != 0 ? d.p_unscale : 1.0f, nullptr);
    return h.finish(name && name_cap ? name : "mbconv", nullptr, 0);   // (the name is in `name` already: mb_debug_plan)
} catch (...) { return on_exception(); }

// The plan of a rate pair as it lies on the device (include/birda_hip_resample_debug.h): the layouts are not undone here.
int bh_debug_resample_plan(int device, uint32_t from_rate, uint32_t to_rate, int32_t *params, float *op, size_t op_cap, uint16_t *op16,
                           size_t op16_cap) try {
    if (!params || from_rate == 0 || to_rate == 0 || from_rate == to_rate) return fail(BH_ERR_INVALID, "debug_resample_plan: bad arguments");
    HIPCHK(hipSetDevice(device));
    const char *err = nullptr;
    const bh::ResamplePlan *pl = bh::resample_plan(from_rate, to_rate, &err);
    if (!pl) return fail(BH_ERR_UNSUPPORTED, "%s (%u -> %u Hz)", err ? err : "resampler", from_rate, to_rate);
    const int32_t p[8] = {pl->hop, pl->N, pl->nblk, pl->K, pl->dmin, pl->block_form, bh::resample_frame_tiles(*pl), pl->op16_exp};
    memcpy(params, p, sizeof p);
    const size_t n_op = (size_t)pl->nblk * pl->K * 160, n_op16 = 2 * n_op;
    if ((op && op_cap < n_op) || (op16 && op16_cap < n_op16))
        return fail(BH_ERR_INVALID, "debug_resample_plan: the operator is %zu floats and %zu halves", n_op, n_op16);
    if (op) HIPCHK(hipMemcpy(op, pl->d_op, n_op * sizeof(float), hipMemcpyDeviceToHost));
    if (op16) HIPCHK(hipMemcpy(op16, pl->d_op16, n_op16 * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return BH_OK;
} catch (...) { return on_exception(); }

// One launch_resample on operands of the caller's, no classifier (include/birda_hip_resample_debug.h).
int bh_debug_resample(int device, const float *in, size_t n_seg, size_t in_stride, size_t src_len, uint32_t from_rate, uint32_t to_rate,
                      float *out, size_t out_stride, size_t out_len, int split_f16, char *kernel, size_t kernel_cap) try {
    if (!in || !out || !n_seg || !out_len || from_rate == 0 || to_rate == 0 || from_rate == to_rate || src_len > in_stride ||
        out_len > out_stride || (split_f16 != 0 && split_f16 != 1))
        return fail(BH_ERR_INVALID, "debug_resample: bad arguments");
    int rc = resample_ranges("debug_resample", src_len, out_len, n_seg);
    if (rc != BH_OK) return rc;
    if (in_stride > (size_t)INT32_MAX / n_seg || out_stride > (size_t)INT32_MAX / n_seg)
        return fail(BH_ERR_INVALID, "debug_resample: buffers past 2^31 elements");
    HIPCHK(hipSetDevice(device));
    const char *err = nullptr;
    const bh::ResamplePlan *pl = bh::resample_plan(from_rate, to_rate, &err);
    if (!pl) return fail(BH_ERR_UNSUPPORTED, "%s (%u -> %u Hz)", err ? err : "resampler", from_rate, to_rate);
    DebugLaunch h{"debug_resample"};
    const float *dx = h.in(in, n_seg * in_stride * 4);
    float *dy = h.out(n_seg * out_stride, "out", out);
    if (!h.ok) return h.no_memory();
    return h.finish(bh::launch_resample(*pl, dx, in_stride, (int)src_len, dy, out_stride, (int)out_len, (int)n_seg, split_f16 != 0, nullptr),
                    kernel, kernel_cap);
} catch (...) { return on_exception(); }

// The dense stack of a custom classifier alone: host rows through cc_upload_rows and cc_run as bh_custom_classifier_predict_batch
// takes them, the last layer's activated output back, no ranking (include/birda_hip_custom_debug.h).
int bh_debug_custom_logits(bh_custom_classifier *cc, const float *rows, size_t n, float *out, char *kernel, size_t kernel_cap) try {
    if (!cc || !rows || !out || !n) return fail(BH_ERR_INVALID, "debug_custom_logits: bad arguments");
    if (n > (size_t)INT32_MAX / std::max<size_t>(cc->max_width, 1)) return fail(BH_ERR_INVALID, "debug_custom_logits: buffers past 2^31 elements");
    std::lock_guard<std::mutex> g(cc->mu);
    HIPCHK(hipSetDevice(cc->device));
    int rc = cc_upload_rows(cc, rows, n);
    if (rc != BH_OK) return rc;
    const char *name = nullptr;
    rc = cc_run(cc, cc->d_in, cc->k0, n, cc->stream, nullptr, out, &name);
    if (rc != BH_OK) return rc;
    if (!name) return fail(BH_ERR_INTERNAL, "debug_custom_logits: no GEMM was launched");
    if (kernel && kernel_cap) snprintf(kernel, kernel_cap, "%s", name);
    return BH_OK;
} catch (...) { return on_exception(); }

}  // extern "C"
