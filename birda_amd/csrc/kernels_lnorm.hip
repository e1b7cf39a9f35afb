// kernels_lnorm.hip -- LayerNorm over the channels of an NHWC f32 tensor, pixel by pixel (model.hpp OP_LNORM; ConvNeXt's norm):
//   y[p][c] = (x[p][c] - mean_p) / sqrt(var_p + eps) * gamma[c] + beta[c],   var_p the biased variance over the C channels.
//
// HBM-bound: a launch reads its input once and writes its output once.  A group of G lanes of a wave owns one pixel, G in
// {8, 16, 32, 64}; lane l of the group holds the pixel's float4s l, l + G, l + 2 G ... -- NV of them, NV <= 8 at C = 2048 -- in
// registers, so every load and store of a group is a run of 16-byte pieces along C, and the groups of a wave take consecutive
// pixels: consecutive memory.  (G, NV) is chosen on the host from C / 4 alone (lnorm_form): the pair that leaves the fewest idle
// float4 slots, the wider group on a tie.  Grid-stride over the pixels; every element offset is 64 bits wide.
//
// Arithmetic, the same in every precision mode and at every launch size.  A lane adds its own values in slot order; the G partial
// sums meet in a __shfl_xor butterfly (G / 2, G / 4 ... 1), which leaves every lane of the group with the same bits.  A pixel's
// result therefore depends on C alone: not on the grid, on n_seg, or on the pixels that share its wave.
//   mean = sum(x) / C                         accumulated in float64: the summands are O(sigma) where the sum is not, and a float32 sum
//                                             leaves the mean off by ~u sigma / sqrt(C) -- an ABSOLUTE error in every x - mean, which an
//                                             element next to the mean (x - mean ~ 0, beta ~ 0) has no tolerance for
//   d    = (x - mh) - ml                      mh + ml = mean as two floats: the error of d is that of one subtraction, relative to |d|
//   var  = sum(d d) / C,  rs = 1 / sqrt(var + eps)      (two-pass: the deviations are never formed as E[x^2] - mean^2; positive
//                                             float32 summands, correctly rounded division and square root)
//   y    = fma(d rs, gamma, beta)
// float64 additions run at half the float32 rate and there is one per element: nothing against the 8 bytes each element moves.
// A constant pixel yields beta exactly: C <= 2048 copies of a 24-bit value add up exactly in float64, (C x) / C = x, so mh = x, ml = 0,
// d = 0, var = 0 and y = fma(0, gamma, beta).
// Non-finite: a NaN or an inf in a pixel makes the mean NaN or inf, d of that element NaN (inf - inf) and of the others NaN or
// -+inf, var NaN or inf and rs NaN or 0 -- every channel of THAT pixel is NaN (inf * 0; gamma = 0 included: NaN * 0), no other pixel is
// touched.  Nothing is clamped: fmaxf would drop the NaN that BH_FLAG_AUTO and BH_ERR_NONFINITE rely on.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace bh {

namespace {

template <int G, typename V>
__device__ __forceinline__ V group_sum(V v) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int G, int NV>
__global__ __launch_bounds__(256) void lnorm_kernel(const float4 *__restrict__ in, const float4 *__restrict__ gamma, const float4 *__restrict__ beta,
                                                     float4 *__restrict__ out, const unsigned long long n_pix, const int c4n, const float eps) {
    constexpr unsigned PPB = 256 / G;                       // pixels a workgroup takes per trip
    const int l = (int)(threadIdx.x % G);
    const float fc = (float)(4 * c4n);
    const double dc = (double)(4 * c4n);
    float4 ga[NV], be[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int j = l + k * G;
        ga[k] = j < c4n ? gamma[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        be[k] = j < c4n ? beta[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // (the trip count is the same for every lane of the workgroup: every lane of a wave reaches the shuffles)
    const unsigned long long step = (unsigned long long)gridDim.x * PPB;
    for (unsigned long long base = (unsigned long long)blockIdx.x * PPB; base < n_pix; base += step) {
        const unsigned long long pix = base + threadIdx.x / G;
        const bool live = pix < n_pix;
        const float4 *src = in + pix * (unsigned long long)c4n;
        float4 x[NV];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int j = l + k * G;
            x[k] = (live && j < c4n) ? src[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            s += (double)x[k].x; s += (double)x[k].y; s += (double)x[k].z; s += (double)x[k].w;
        }
        const double mean = group_sum<G, double>(s) / dc;
        const float mh = (float)mean, ml = (float)(mean - (double)mh);
        float q = 0.0f;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            // (an idle slot stays zero: it is no channel of the pixel)
            if (l + k * G < c4n) x[k] = make_float4((x[k].x - mh) - ml, (x[k].y - mh) - ml, (x[k].z - mh) - ml, (x[k].w - mh) - ml);
            q = __fmaf_rn(x[k].x, x[k].x, q); q = __fmaf_rn(x[k].y, x[k].y, q); q = __fmaf_rn(x[k].z, x[k].z, q); q = __fmaf_rn(x[k].w, x[k].w, q);
        }
        const float var = __fdiv_rn(group_sum<G, float>(q), fc);
        const float rs = __fdiv_rn(1.0f, __fsqrt_rn(var + eps));
        if (!live) continue;
        float4 *dst = out + pix * (unsigned long long)c4n;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int j = l + k * G;
            if (j < c4n)
                dst[j] = make_float4(__fmaf_rn(x[k].x * rs, ga[k].x, be[k].x), __fmaf_rn(x[k].y * rs, ga[k].y, be[k].y),
                                     __fmaf_rn(x[k].z * rs, ga[k].z, be[k].z), __fmaf_rn(x[k].w * rs, ga[k].w, be[k].w));
        }
    }
}

// the group width and the float4s a lane holds for c4n = C / 4 float4s a pixel: the fewest idle slots, the wider group on a tie
void lnorm_form(int c4n, int &G, int &NV) {
    int best = 1 << 30;
    G = 64; NV = 8;
    for (int g = 8; g <= 64; g *= 2) {
        const int nv = (c4n + g - 1) / g;
        if (nv > 8) continue;
        const int idle = g * nv - c4n;
        if (idle <= best) { best = idle; G = g; NV = nv; }
    }
}

}  // namespace

bool lnorm_supports(int C) { return C >= 4 && C % 4 == 0 && C <= 2048; }

const char *launch_lnorm(const float *in, const float *gamma, const float *beta, float *out, unsigned long long n_pix, int C, float eps, hipStream_t s) {
    if (!lnorm_supports(C)) return nullptr;
    if (!n_pix) return "";
    const int c4n = C / 4;
    int G, NV;
    lnorm_form(c4n, G, NV);
    const unsigned long long ppb = 256 / G;
    // at most eight workgroups a CU's worth of a 256-CU chip, as launch_pool: the rest of a large launch is the grid-stride loop's
    const unsigned blocks = (unsigned)std::min<unsigned long long>((n_pix + ppb - 1) / ppb, 256ull * 8);
#define BH_LN(GV, NVV)                                                                                                               \
    if (G == GV && NV == NVV) {                                                                                                      \
        hipLaunchKernelGGL((lnorm_kernel<GV, NVV>), dim3(blocks), dim3(256), 0, s, (const float4 *)in, (const float4 *)gamma,        \
                           (const float4 *)beta, (float4 *)out, n_pix, c4n, eps);                                                    \
        return "lnorm_kernel<" #GV "," #NVV ">";                                                                                     \
    }
#define BH_LN_G(GV) BH_LN(GV, 1) BH_LN(GV, 2) BH_LN(GV, 3) BH_LN(GV, 4) BH_LN(GV, 5) BH_LN(GV, 6) BH_LN(GV, 7) BH_LN(GV, 8)
    BH_LN_G(8) BH_LN_G(16) BH_LN_G(32) BH_LN_G(64)
#undef BH_LN_G
#undef BH_LN
    return nullptr;
}

}  // namespace bh
