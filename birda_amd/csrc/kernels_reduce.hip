// kernels_reduce.hip -- max, mean and max + mean over one image axis or both of an NHWC f32 tensor (model.hpp OP_REDUCE: ONNX ReduceMax /
// ReduceMean over H or W, GlobalMaxPool, and the max + mean head of the PANNs audio CNNs).  The mean over both axes stays gap_kernel.
//
// HBM-bound: a launch reads its input once and writes its output once.  A work item is one float4 of channels of one kept pixel; it
// walks the R taps of the reduced extent at a pitch of C (over W, or over both axes: the taps are neighbours in memory) or W C (over
// H).  Consecutive lanes take consecutive channel groups, then the next kept pixel: every tap is a run of 16-byte loads coalesced
// along C.  Every element offset is 64 bits wide.
//
// Splitting.  With few kept pixels and a long reduced extent (a global max; a time axis of hundreds of frames at 64 channels) one
// lane an item leaves most of the chip idle behind a serial chain of loads, so G lanes of a wave share an item: lane `sub` takes taps
// sub, sub + G, sub + 2 G ... and the G partial results meet in a fixed __shfl_xor butterfly.  The G lanes of an item sit 64 / G
// lanes apart, so that the neighbours of a lane still read neighbouring channel groups.  G is 1 or 8, chosen on the host from the layer's
// shape alone (reduce_split: R and the kept float4s of one segment), never from the segment count or the grid: an item's bits are the
// same at every launch size.
//
// Arithmetic, the same in every precision mode:
//   max       m = -inf; m = (v > m || v != v) ? v : m, tap by tap and lane by lane -- a NaN tap makes the output NaN and stays (fmaxf
//             would drop it: BH_FLAG_AUTO and BH_ERR_NONFINITE rely on a non-finite activation reaching the logits); +-inf, +-0,
//             subnormals and 1e30 follow `>`: the result is a value of the window, exactly
//   mean      one f32 sum: each lane adds its taps in tap order, the butterfly adds the G partial sums (a + b is commutative: every
//             lane of the item holds the same bits), then ONE correctly rounded division by (float)R.  A NaN or an inf tap reaches
//             the outputs whose window holds it and no other: items share nothing but the wave
//   max+mean  both accumulators over ONE read of the window, then max + mean, one addition
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.hpp"

namespace bh {

namespace {

struct ReduceGeom {
    unsigned c4n, R, kept4;               // float4s a pixel; taps a window; float4s of one segment's output (out_h * out_w * c4n)
    unsigned long long in_seg4;           // float4s of one segment's input
    unsigned long long start4, pitch4;    // first tap of kept pixel q: q * start4 (+ the channel group); tap to tap: pitch4
};

__device__ __forceinline__ float nan_max(const float m, const float v) { return (v > m || v != v) ? v : m; }

template <int MODE, int G>
__global__ __launch_bounds__(256) void reduce_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, const ReduceGeom g,
                                                      const unsigned long long total4) {
    constexpr unsigned IPW = 64 / G;                        // items a wave
    const unsigned lane = threadIdx.x & 63u, sub = lane / IPW, li = lane % IPW;
    const unsigned long long nwaves = (unsigned long long)gridDim.x * 4ull;
    // (the trip count is the same for every lane of a wave: every lane reaches the shuffles)
    for (unsigned long long base = ((unsigned long long)blockIdx.x * 4ull + (threadIdx.x >> 6)) * IPW; base < total4; base += nwaves * IPW) {
        const unsigned long long i = base + li;
        const bool live = i < total4;
        float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), sm = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live && sub < g.R) {
            const unsigned long long seg = (i >> 32) ? i / g.kept4 : (unsigned long long)((unsigned)i / g.kept4);
            const unsigned r = (unsigned)(i - seg * g.kept4);
            const unsigned q = r / g.c4n, c4 = r - q * g.c4n;
            const float4 *src = in + seg * g.in_seg4 + (unsigned long long)q * g.start4 + c4 + (unsigned long long)sub * g.pitch4;
            const unsigned long long hop = (unsigned long long)G * g.pitch4;
#pragma unroll 4
            for (unsigned t = sub; t < g.R; t += G, src += hop) {
                const float4 v = *src;
                if (MODE != 1) { mx.x = nan_max(mx.x, v.x); mx.y = nan_max(mx.y, v.y); mx.z = nan_max(mx.z, v.z); mx.w = nan_max(mx.w, v.w); }
                if (MODE != 0) { sm.x += v.x; sm.y += v.y; sm.z += v.z; sm.w += v.w; }
            }
        }
#pragma unroll
        for (unsigned off = 32; off >= IPW && G > 1; off >>= 1) {
            if (MODE != 1) {
                mx.x = nan_max(mx.x, __shfl_xor(mx.x, off, 64)); mx.y = nan_max(mx.y, __shfl_xor(mx.y, off, 64));
                mx.z = nan_max(mx.z, __shfl_xor(mx.z, off, 64)); mx.w = nan_max(mx.w, __shfl_xor(mx.w, off, 64));
            }
            if (MODE != 0) {
                sm.x += __shfl_xor(sm.x, off, 64); sm.y += __shfl_xor(sm.y, off, 64);
                sm.z += __shfl_xor(sm.z, off, 64); sm.w += __shfl_xor(sm.w, off, 64);
            }
        }
        if (!live || sub != 0) continue;
        if (MODE != 0) {
            const float count = (float)g.R;
            sm = make_float4(__fdiv_rn(sm.x, count), __fdiv_rn(sm.y, count), __fdiv_rn(sm.z, count), __fdiv_rn(sm.w, count));
        }
        out[i] = MODE == 0 ? mx : MODE == 1 ? sm : make_float4(mx.x + sm.x, mx.y + sm.y, mx.z + sm.z, mx.w + sm.w);
    }
}

}  // namespace

// what model.hpp validate_model accepts of an OP_REDUCE record
bool reduce_supports(const ConvParams &p, int mode) {
    if (mode < 0 || mode > 2 || p.cout < 4 || p.cout % 4 || p.cout > (1 << 24)) return false;
    if (p.in_h < 1 || p.in_w < 1 || p.in_h > (1 << 16) || p.in_w > (1 << 16) || (long long)p.in_h * p.in_w * p.cout > (1ll << 31)) return false;
    if ((p.kh != 1 && p.kh != p.in_h) || (p.kw != 1 && p.kw != p.in_w) || (p.kh == 1 && p.kw == 1)) return false;
    if ((long long)p.kh * p.kw > (1 << 16) || p.out_h != p.in_h / p.kh || p.out_w != p.in_w / p.kw) return false;
    if (p.sh != 1 || p.sw != 1 || p.pad_t != 0 || p.pad_l != 0) return false;
    return !(mode == 1 && p.kh == p.in_h && p.kw == p.in_w && p.kh > 1 && p.kw > 1);     // (OP_GAP's)
}

// the lanes that share an item, from the layer's shape alone: 8 from kReduceSplitMin taps on where one segment has fewer than
// kReduceKeptMax items, else 1.  Measured (profiles/reduce_layers.txt): at 1 000 segments the two forms are within 3 % of each other on
// every shape; at 16 segments 8 lanes take 0.36 of one lane's time on 64x500x64 over W (1 024 items a segment) and 0.35 on 8x32x512 over
// both (128 items), and 1.12 on 64x500x64 over H (8 000 items).  A 64-lane form was built and dropped: a wave then holds one item, its
// lanes read 64 different rows 16 bytes each, and it took 3 to 4.5 times the 8-lane form's time at 1 000 segments and won nowhere.
int reduce_split(const ConvParams &p) {
    const long long R = (long long)p.kh * p.kw, kept4 = (long long)p.out_h * p.out_w * (p.cout / 4);
    return R >= kReduceSplitMin && kept4 < kReduceKeptMax ? 8 : 1;
}

const char *launch_reduce(const float *in, float *out, const ConvParams &p, int mode, int n_seg, hipStream_t s, int split) {
    if (!reduce_supports(p, mode)) return nullptr;
    const int G = split ? split : reduce_split(p);
    ReduceGeom g{};
    g.c4n = (unsigned)(p.cout / 4);
    g.R = (unsigned)(p.kh * p.kw);
    g.kept4 = (unsigned)((size_t)p.out_h * p.out_w * g.c4n);
    g.in_seg4 = (unsigned long long)p.in_h * p.in_w * g.c4n;
    // over H alone: kept pixel q is column q, the taps a row apart; over W, or over both: kept pixel q is row q (or the image), taps neighbours
    const bool over_h = p.kw == 1 && p.in_w > 1;
    g.start4 = over_h ? g.c4n : (unsigned long long)g.R * g.c4n;
    g.pitch4 = over_h ? (unsigned long long)p.in_w * g.c4n : g.c4n;
    const unsigned long long total4 = (unsigned long long)n_seg * g.kept4;
    if (!total4) return "";
    // at most eight workgroups a CU's worth of a 256-CU chip, as launch_pool: the rest of a large launch is the grid-stride loop's
    const unsigned long long ipb = 256ull / (unsigned)G;
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total4 + ipb - 1) / ipb, 256ull * 8);
#define BH_RED(M, GV, NAME)                                                                                                        \
    if (mode == M && G == GV) {                                                                                                    \
        hipLaunchKernelGGL((reduce_kernel<M, GV>), dim3(blocks), dim3(256), 0, s, (const float4 *)in, (float4 *)out, g, total4);   \
        return "reduce_kernel<" NAME "," #GV ">";                                                                                  \
    }
#define BH_RED_G(GV) BH_RED(0, GV, "MAX") BH_RED(1, GV, "MEAN") BH_RED(2, GV, "MAXMEAN")
    BH_RED_G(1) BH_RED_G(8)
#undef BH_RED_G
#undef BH_RED
    return nullptr;
}

}  // namespace bh
