// Grouped convolutions (model.hpp OP_GCONV: ResNeXt, RegNet, ShuffleNet-style grouped 1x1) for gfx950, NHWC f32.
//
//     C[m][o] = act(sum over (tap, c in o's group) X[m's window pixel at tap][c] W[tap][c][o] + bias[o]),  m = (segment, oy, ox)
//
// An implicit GEMM in which every 16-wide COLUMN TILE has a K range of its own.  Tile t holds output channels 16t .. 16t + 15; the
// groups those belong to read one contiguous run of input channels, the tile's SPAN [c0, c0 + span) (gconv_tile_span, kernels.hpp).
// The host re-lays the compact [kh][kw][cin / G][cout] weights once at create (gconv_matrix): column o of the tile's block is dense
// over k = tap * span + (c - c0), with zeros where channel c is not in o's group, and K = kh kw span is padded to a whole MFMA
// step ONCE, at the end -- never per tap (a 16-channel span padded per tap to 32 would double the f16 work).  One layout takes
// every case: a tile inside one group (width >= 16), a tile of several groups (widths 4, 8), a tile that straddles two groups
// (width 24) and a last partial tile.  The MFMAs a tile spends on the zeros are at most those of the groups it touches, not of all G.
//
// Two kernels, three instantiations: gconv_kernel (v_mfma_f32_16x16x4_f32: BH_FLAG_F32, BIRDA_HIP_KEEP_TENSORS contexts, the
// BH_FLAG_AUTO re-run) and gconv16_kernel<TERMS> (v_mfma_f32_16x16x32_f16; TERMS 3: hi / lo split operands, f32-grade; 1: plain
// f16; planes pre-scaled by a power of two, undone in the epilogue's FMA, as launch_conv_gemm16's).  The activation is a run-time
// argument of both.  Block = 4 waves stacked along M, a wave = 32 rows x one column tile; blocks run column tile fastest, so the
// blocks that gather the same rows of X are neighbours and the re-reads come from L2.  A rows are gathered from NHWC with float4
// loads (widths are multiples of 4, so four consecutive k are four consecutive channels of one tap) one step ahead of their use;
// the tile's weight block streams from L2 in fragment order, one 16-byte load per lane and step (it is read once per 128 rows: an
// LDS copy would save nothing).  Per output element the k order is fixed and there is no split-K, so a segment's bits do not
// depend on the launch it runs in.  Offsets into X and C are 64-bit.
//
// NON-FINITE CONTRACT.  A NaN or inf input value is never lost: every output whose window and group read it is non-finite in front
// of the activation, and the activation keeps it (the comparison forms of act_apply_pos: a NaN stays a NaN, +inf stays +inf; ReLU
// of -inf is 0, as it is everywhere).  Because zero weights meet the value inside the MFMA (0 x inf = NaN), it may also reach the
// OTHER output channels of the same column tile at those pixels.  It reaches no other pixel -- taps outside the image, the padding
// of K and rows past M read as zero or are never stored, never as whatever lies there -- and no other column tile.
#include "kernels.hpp"

#include <algorithm>

namespace bh {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

// n / d for n d < 2^32 as one multiply-high (gconv_supports holds K span below that); d >= 2
__device__ __forceinline__ unsigned gconv_rcp(unsigned d) { return (unsigned)(0x100000000ull / d) + 1u; }

struct GconvTile {       // what a workgroup's column tile reads: wave-uniform
    int c0, span, K;     // first input channel, channels, kh kw span
    unsigned rcp_span, rcp_kw;
};
__device__ __forceinline__ GconvTile gconv_tile(const ConvKernelParams &p, int groups, int t) {
    GconvTile g;
    gconv_tile_span(p.cin, p.cout, groups, t, g.c0, g.span);
    g.K = p.kh * p.kw * g.span;
    g.rcp_span = gconv_rcp((unsigned)g.span);
    g.rcp_kw = p.kw > 1 ? gconv_rcp((unsigned)p.kw) : 0u;
    return g;
}
struct GconvRow {        // one output row's gather origin: its segment's image and the top-left input pixel of its window
    const float *x;
    int iy0, ix0;
};
__device__ __forceinline__ GconvRow gconv_row(const float *X, const ConvKernelParams &p, int m) {
    const int opix = p.out_h * p.out_w;
    const int seg = m / opix, r = m - seg * opix;
    const int oy = r / p.out_w, ox = r - oy * p.out_w;
    return GconvRow{X + (size_t)seg * p.in_h * p.in_w * p.cin, oy * p.sh - p.pad_t, ox * p.sw - p.pad_l};
}
// k .. k + 3 of the tile's flattened (tap, channel in span) index, k % 4 == 0: four channels of one tap.  Zero past K (the padding
// of the last step) and outside the image.
__device__ __forceinline__ float4 gconv_gather4(const GconvRow &r, const ConvKernelParams &p, const GconvTile &g, int k) {
    if (k >= g.K) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int tap = (int)__umulhi((unsigned)k, g.rcp_span), ch = k - tap * g.span;
    const int dy = p.kw > 1 ? (int)__umulhi((unsigned)tap, g.rcp_kw) : tap, dx = tap - dy * p.kw;
    const int iy = r.iy0 + dy, ix = r.ix0 + dx;
    if ((unsigned)iy >= (unsigned)p.in_h || (unsigned)ix >= (unsigned)p.in_w) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *reinterpret_cast<const float4 *>(r.x + ((size_t)iy * p.in_w + ix) * p.cin + g.c0 + ch);
}

constexpr int GC_MT = 2;             // row tiles of 16 a wave
constexpr int GC_BM = 4 * 16 * GC_MT;   // rows a workgroup

}  // namespace

// f32 MFMA.  Wf: fragments [K16 / 16][n_tiles][64 lanes][4], element (g, t, lane, c) = Wt[k = 16g + 4(lane >> 4) + c][16t + (lane & 15)]
// of gconv_matrix's Wt: MFMA step c of lane quad q takes k = 16g + 4q + c, so a lane's four A operands are one float4 gather.
__global__ __launch_bounds__(256) void gconv_kernel(const float *__restrict__ X, const float4 *__restrict__ Wf, const float *__restrict__ bias,
                                                     float *__restrict__ C, ConvKernelParams p, int groups, int M, int n_tiles) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int t = (int)(blockIdx.x % (unsigned)n_tiles), yb = (int)(blockIdx.x / (unsigned)n_tiles);
    const int m0 = yb * GC_BM + wave * 16 * GC_MT;
    const GconvTile g = gconv_tile(p, groups, t);
    const int ngroups = (g.K + 15) >> 4;

    GconvRow rows[GC_MT];
#pragma unroll
    for (int i = 0; i < GC_MT; i++) rows[i] = gconv_row(X, p, min(m0 + i * 16 + li, M - 1));   // rows past M: clamped, never stored

    f32x4 acc[GC_MT];
#pragma unroll
    for (int i = 0; i < GC_MT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    float4 a[GC_MT], an[GC_MT] = {}, b, bn = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load = [&](int gi, float4 (&ra)[GC_MT], float4 &rb) {
#pragma unroll
        for (int i = 0; i < GC_MT; i++) ra[i] = gconv_gather4(rows[i], p, g, 16 * gi + 4 * kq);
        rb = Wf[((size_t)gi * n_tiles + t) * 64 + lane];
    };
    load(0, a, b);
    for (int gi = 0; gi < ngroups; gi++) {
        if (gi + 1 < ngroups) load(gi + 1, an, bn);
#pragma unroll
        for (int i = 0; i < GC_MT; i++) {
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b.x, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b.y, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b.z, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b.w, acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < GC_MT; i++) a[i] = an[i];
        b = bn;
    }

    const int col = t * 16 + li;
    if (col >= p.cout) return;
    const float bv = bias[col];
#pragma unroll
    for (int i = 0; i < GC_MT; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = m0 + i * 16 + kq * 4 + r;
            if (row < M) C[(size_t)row * p.cout + col] = act_apply_pos(bh_add_unpacked(acc[i][r], bv), p.act, true);
        }
}

// f16 MFMA.  Wf: w16_planes' layout over gconv_matrix's Wt, [K32 / 32][n_tiles]{hi, lo}[64 lanes][8 halves]: lane (n & 15, k group)
// holds k = 32 step + 8 (lane >> 4) + 0 .. 7 of column n, times 1 / w_unscale.  A lane's eight A values are two float4 gathers
// (each inside one tap; the two may lie in different taps), split into hi / lo halves in registers.
template <int TERMS>
__global__ __launch_bounds__(256) void gconv16_kernel(const float *__restrict__ X, const f16x8 *__restrict__ Wf, const float *__restrict__ bias,
                                                       float *__restrict__ C, ConvKernelParams p, int groups, int M, int n_tiles, float w_unscale) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int t = (int)(blockIdx.x % (unsigned)n_tiles), yb = (int)(blockIdx.x / (unsigned)n_tiles);
    const int m0 = yb * GC_BM + wave * 16 * GC_MT;
    const GconvTile g = gconv_tile(p, groups, t);
    const int steps = (g.K + 31) >> 5;

    GconvRow rows[GC_MT];
#pragma unroll
    for (int i = 0; i < GC_MT; i++) rows[i] = gconv_row(X, p, min(m0 + i * 16 + li, M - 1));   // rows past M: clamped, never stored

    f32x4 acc[GC_MT];
#pragma unroll
    for (int i = 0; i < GC_MT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    float4 a[GC_MT][2], an[GC_MT][2] = {};
    f16x8 bh = {}, bl = {}, bhn = {}, bln = {};
    auto load = [&](int st, float4 (&ra)[GC_MT][2], f16x8 &rbh, f16x8 &rbl) {
#pragma unroll
        for (int i = 0; i < GC_MT; i++) {
            ra[i][0] = gconv_gather4(rows[i], p, g, 32 * st + 8 * kq);
            ra[i][1] = gconv_gather4(rows[i], p, g, 32 * st + 8 * kq + 4);
        }
        rbh = Wf[(((size_t)st * n_tiles + t) * 2 + 0) * 64 + lane];
        if (TERMS == 3) rbl = Wf[(((size_t)st * n_tiles + t) * 2 + 1) * 64 + lane];
    };
    load(0, a, bh, bl);
    for (int st = 0; st < steps; st++) {
        if (st + 1 < steps) load(st + 1, an, bhn, bln);
        f16x8 ah[GC_MT], al[GC_MT];
#pragma unroll
        for (int i = 0; i < GC_MT; i++) {
            const float v[8] = {a[i][0].x, a[i][0].y, a[i][0].z, a[i][0].w, a[i][1].x, a[i][1].y, a[i][1].z, a[i][1].w};
            bh_split8(v, ah[i], al[i]);
        }
        __builtin_amdgcn_sched_barrier(0);   // no VALU split between the MFMAs (see mel_kernel)
#pragma unroll
        for (int i = 0; i < GC_MT; i++) {
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc[i], 0, 0, 0);
            if (TERMS == 3) {
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc[i], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < GC_MT; i++) { a[i][0] = an[i][0]; a[i][1] = an[i][1]; }
        bh = bhn; bl = bln;
    }

    const int col = t * 16 + li;
    if (col >= p.cout) return;
    const float bv = bias[col];
#pragma unroll
    for (int i = 0; i < GC_MT; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = m0 + i * 16 + kq * 4 + r;
            if (row < M) C[(size_t)row * p.cout + col] = act_apply_pos(__builtin_fmaf(acc[i][r], w_unscale, bv), p.act, true);   // the planes hold W / w_unscale
        }
}

bool gconv_supports(const ConvParams &p, int groups) {
    if (p.in_layout != 0 || groups < 2 || p.cin <= 0 || p.cout <= 0 || p.cin % groups || p.cout % groups) return false;
    const int gi = p.cin / groups, go = p.cout / groups;
    if (gi % 4 || go % 4 || p.kh < 1 || p.kh > 7 || p.kw < 1 || p.kw > 7 || (p.sh != 1 && p.sh != 2) || (p.sw != 1 && p.sw != 2) ||
        p.pad_t < 0 || p.pad_l < 0 || p.act < 0 || p.act > ACT_LAST || p.res_after) return false;
    // the multiply-high divisions of the gather are exact while (K + a step) x span stays below 2^32
    const uint64_t span = (uint64_t)gi * (uint64_t)std::min(groups, 15 / go + 2);
    return ((uint64_t)p.kh * p.kw * span + 32) * span < (1ull << 32);
}

static bool gconv_grid(const ConvParams &p, int n_seg, int &M, int &n_tiles, unsigned &blocks) {
    const long long m = (long long)n_seg * p.out_h * p.out_w;
    n_tiles = (p.cout + 15) / 16;
    const long long b = (m + GC_BM - 1) / GC_BM * n_tiles;
    if (m <= 0 || m > INT32_MAX || b > INT32_MAX) return false;
    M = (int)m;
    blocks = (unsigned)b;
    return true;
}

const char *launch_gconv(const float *in, const float *Wf, const float *b, float *out, const ConvParams &p, int groups, int n_seg, hipStream_t s) {
    int M, n_tiles;
    unsigned blocks;
    if (!gconv_supports(p, groups) || !gconv_grid(p, n_seg, M, n_tiles, blocks)) return nullptr;
    hipLaunchKernelGGL(gconv_kernel, dim3(blocks), dim3(256), 0, s, in, (const float4 *)Wf, b, out, conv_kernel_arg<false>(p), groups, M, n_tiles);
    return "gconv_kernel";
}

const char *launch_gconv16(const float *in, const void *Wf, const float *b, float *out, const ConvParams &p, int groups, int n_seg, int terms,
                           float w_unscale, hipStream_t s) {
    int M, n_tiles;
    unsigned blocks;
    if (!gconv_supports(p, groups) || (terms != 1 && terms != 3) || !gconv_grid(p, n_seg, M, n_tiles, blocks)) return nullptr;
    if (terms == 3) {
        hipLaunchKernelGGL(gconv16_kernel<3>, dim3(blocks), dim3(256), 0, s, in, (const f16x8 *)Wf, b, out, conv_kernel_arg<false>(p), groups, M, n_tiles, w_unscale);
        return "gconv16_kernel<3>";
    }
    hipLaunchKernelGGL(gconv16_kernel<1>, dim3(blocks), dim3(256), 0, s, in, (const f16x8 *)Wf, b, out, conv_kernel_arg<false>(p), groups, M, n_tiles, w_unscale);
    return "gconv16_kernel<1>";
}

}  // namespace bh
