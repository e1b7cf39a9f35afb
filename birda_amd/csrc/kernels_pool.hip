// kernels_pool.hip -- windowed pooling (ONNX MaxPool / AveragePool in floor mode; model.hpp OP_POOL), NHWC f32 in and out.
//
// HBM-bound: a launch moves its input and its output once (overlapping windows re-read rows that hit L2).  A thread owns one
// float4 of channels of one output pixel; consecutive threads take consecutive channel groups, then the next pixel, so every tap
// is a run of 16-byte loads coalesced along C.  Grid-stride over [n_seg][out_h][out_w][c / 4]; every element offset is 64 bits
// wide (the input of one launch may pass 2^32 bytes).
//
// Arithmetic, the same in every precision mode and at every launch size: taps are visited ky outer, kx inner; a tap outside the
// image is skipped and never read.
//   max      m = -inf; m = (v > m || v != v) ? v : m -- a NaN tap makes the output NaN and stays (fmaxf would drop it:
//            BH_FLAG_AUTO and BH_ERR_NONFINITE rely on a non-finite activation reaching the logits); +-inf and -0 follow `>`
//   average  f32 sum of the in-image taps in that order, then ONE correctly rounded division by (float)count, count = the
//            in-image taps (mode 1, count_include_pad = 0) or kh * kw (mode 2)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.hpp"

namespace bh {

namespace {

struct PoolGeom {
    int in_h, in_w, out_h, out_w, c4n, kh, kw, sh, sw, pad_t, pad_l;
    unsigned out_seg4;              // float4s of one segment's output: out_h * out_w * c4n (< 2^29)
    unsigned long long in_seg4;     // float4s of one segment's input
};

template <int MODE>
__device__ __forceinline__ void pool_tap(float4 &acc, const float4 v) {
    if (MODE == 0) {
        acc.x = (v.x > acc.x || v.x != v.x) ? v.x : acc.x;
        acc.y = (v.y > acc.y || v.y != v.y) ? v.y : acc.y;
        acc.z = (v.z > acc.z || v.z != v.z) ? v.z : acc.z;
        acc.w = (v.w > acc.w || v.w != v.w) ? v.w : acc.w;
    } else {
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void pool_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, const PoolGeom g,
                                                    const unsigned long long total4) {
    const unsigned long long step = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < total4; i += step) {
        // (one 64-bit division a thread and element only when the launch is that large)
        const unsigned long long seg = (i >> 32) ? i / g.out_seg4 : (unsigned long long)((unsigned)i / g.out_seg4);
        const unsigned r = (unsigned)(i - seg * g.out_seg4);
        const unsigned pix = r / (unsigned)g.c4n, c4 = r - pix * (unsigned)g.c4n;
        const int oy = (int)(pix / (unsigned)g.out_w), ox = (int)(pix - (unsigned)oy * (unsigned)g.out_w);
        const int y0 = oy * g.sh - g.pad_t, x0 = ox * g.sw - g.pad_l;
        // the in-image part of the window (never empty: pool_supports)
        const int ky0 = max(0, -y0), ky1 = min(g.kh, g.in_h - y0), kx0 = max(0, -x0), kx1 = min(g.kw, g.in_w - x0);
        const float4 *src = in + seg * g.in_seg4 + c4;
        const float init = MODE == 0 ? -INFINITY : 0.0f;
        float4 acc = make_float4(init, init, init, init);
        for (int ky = ky0; ky < ky1; ky++) {
            // (signed: x0 is negative in a window that starts in the left pad; y0 + ky and x0 + kx are in the image)
            const long long row = (long long)(y0 + ky) * g.in_w + x0;
            for (int kx = kx0; kx < kx1; kx++) pool_tap<MODE>(acc, src[(unsigned long long)(row + kx) * g.c4n]);
        }
        if (MODE != 0) {
            const float count = MODE == 1 ? (float)((ky1 - ky0) * (kx1 - kx0)) : (float)(g.kh * g.kw);
            acc = make_float4(__fdiv_rn(acc.x, count), __fdiv_rn(acc.y, count), __fdiv_rn(acc.z, count), __fdiv_rn(acc.w, count));
        }
        out[i] = acc;
    }
}

}  // namespace

// what model.hpp validate_model accepts of an OP_POOL record, plus the kernels' channel granularity
bool pool_supports(const ConvParams &p, int mode) {
    if (mode < 0 || mode > 2 || p.cout < 4 || p.cout % 4 || p.cout > (1 << 24)) return false;
    if (p.in_h < 1 || p.in_w < 1 || p.out_h < 1 || p.out_w < 1 || p.in_h > (1 << 16) || p.in_w > (1 << 16) || p.out_h > (1 << 16) || p.out_w > (1 << 16)) return false;
    if (p.kh < 1 || p.kw < 1 || p.kh > 64 || p.kw > 64 || p.sh < 1 || p.sw < 1 || p.sh > 16 || p.sw > 16 || p.pad_t < 0 || p.pad_l < 0) return false;
    if ((long long)p.in_h * p.in_w * p.cout > (1ll << 31) || (long long)p.out_h * p.out_w * p.cout > (1ll << 31)) return false;
    // every window holds a pixel of the image
    return p.pad_t < p.kh && p.pad_l < p.kw && (long long)(p.out_h - 1) * p.sh - p.pad_t < p.in_h && (long long)(p.out_w - 1) * p.sw - p.pad_l < p.in_w;
}

const char *launch_pool(const float *in, float *out, const ConvParams &p, int mode, int n_seg, hipStream_t s) {
    PoolGeom g{p.in_h, p.in_w, p.out_h, p.out_w, p.cout / 4, p.kh, p.kw, p.sh, p.sw, p.pad_t, p.pad_l, 0, 0};
    g.out_seg4 = (unsigned)((size_t)p.out_h * p.out_w * g.c4n);
    g.in_seg4 = (unsigned long long)p.in_h * p.in_w * g.c4n;
    const unsigned long long total4 = (unsigned long long)n_seg * g.out_seg4;
    if (!total4) return "";
    // at most eight workgroups a CU's worth of a 256-CU chip: the rest of a large launch is the grid-stride loop's
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total4 + 255) / 256, 256ull * 8);
#define BH_POOL(M, NAME)                                                                                                  \
    do {                                                                                                                  \
        hipLaunchKernelGGL((pool_kernel<M>), dim3(blocks), dim3(256), 0, s, (const float4 *)in, (float4 *)out, g, total4); \
        return NAME;                                                                                                      \
    } while (0)
    if (mode == 0) BH_POOL(0, "pool_kernel<MAX>");
    if (mode == 1) BH_POOL(1, "pool_kernel<AVG>");
    BH_POOL(2, "pool_kernel<AVG_PAD>");
#undef BH_POOL
}

}  // namespace bh
