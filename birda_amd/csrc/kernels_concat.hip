// kernels_concat.hip -- channel concatenation, channel windows (Split / Slice) and the channel shuffle (model.hpp OP_CONCAT), NHWC
// f32 in and out.  The sibling of kernels_pool.hip: HBM-bound, a launch reads every output element's source once and writes it once.
//
// Up to four sources, each an NHWC tensor [n][h][w][total] of which the window [off, off + len) of the channels is read; the output
// [n][h][w][C], C = the sum of the lengths, holds the windows one after the other.  A thread owns one 16-byte group of output
// channels of one pixel; consecutive threads take consecutive channel groups, then the next pixel.  Grid-stride over
// [n h w][C / 4]; every element offset is 64 bits wide.  A source's channels outside its window are never read.
//
//   SHUFFLE = 0   offsets and lengths are multiples of 4, so an output group lies in one window: one 16-byte load, one 16-byte store
//   SHUFFLE = 1   out[p][c] = cat[p][(c % g) * (C / g) + c / g] (Reshape [g, C / g] -> Transpose -> Reshape): the four values of a
//                 group are gathered with 4-byte loads straight from global memory -- the neighbouring lanes and this lane's later
//                 loads reuse the lines from L1 / L2 --, then stored as one 16-byte group
//
// No arithmetic touches the values: they travel as 32-bit integers, so NaN payloads, -0, subnormals and infinities come out as they
// went in, and a non-finite activation in front of a concat still reaches the logits (BH_FLAG_AUTO, BH_ERR_NONFINITE).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace bh {

namespace {

struct ConcatGeom {
    const unsigned *p[4];       // the sources
    unsigned total[4];          // channels of source k (a multiple of 4)
    unsigned off[4];            // first channel read from it
    unsigned start[4];          // where its window starts in the output; 0xffffffff for a source that is not there
    unsigned c4n;               // C / 4
    unsigned g, cg;             // shuffle groups and C / g (SHUFFLE = 1)
};

// the source that holds channel c of the concatenation, and where: element offset of (pixel, c) within it
__device__ __forceinline__ const unsigned *concat_at(const ConcatGeom &q, const unsigned long long pix, const unsigned c) {
    const unsigned *base = q.p[0];
    unsigned total = q.total[0], ch = q.off[0] + c;
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (c >= q.start[k]) { base = q.p[k]; total = q.total[k]; ch = q.off[k] + (c - q.start[k]); }
    return base + pix * total + ch;
}

template <int SHUFFLE>
__global__ __launch_bounds__(256) void concat_kernel(uint4 *__restrict__ out, const ConcatGeom q, const unsigned long long total4) {
    const unsigned long long step = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < total4; i += step) {
        // (one 64-bit division a thread and element only when the launch is that large)
        const unsigned long long pix = (i >> 32) ? i / q.c4n : (unsigned long long)((unsigned)i / q.c4n);
        const unsigned c = 4u * (unsigned)(i - pix * q.c4n);
        uint4 v;
        if (SHUFFLE == 0) {
            v = *reinterpret_cast<const uint4 *>(concat_at(q, pix, c));
        } else {
            // c / g and c % g of four consecutive channels
            unsigned d = c / q.g, r = c - d * q.g, w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                w[j] = *concat_at(q, pix, r * q.cg + d);
                if (++r == q.g) { r = 0; d++; }
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        out[i] = v;
    }
}

}  // namespace

// what model.hpp validate_model accepts of an OP_CONCAT record (one or two sources), and the same of three and four
bool concat_supports(int h, int w, const ConcatSource *src, int n_src, int groups) {
    if (!src || n_src < 1 || n_src > 4 || h < 1 || w < 1 || h > (1 << 16) || w > (1 << 16) || groups < 0) return false;
    long long C = 0;
    for (int k = 0; k < n_src; k++) {
        const ConcatSource &s = src[k];
        if (s.total4 < 1 || s.total4 > (1 << 22) || s.off < 0 || s.len < 4 || s.off % 4 || s.len % 4) return false;
        if ((long long)s.off + s.len > 4ll * s.total4) return false;
        if ((long long)h * w * 4 * s.total4 > (1ll << 31)) return false;
        C += s.len;
    }
    if (C > (1 << 24) || (long long)h * w * C > (1ll << 31)) return false;
    return groups <= 1 || (groups <= C && C % groups == 0);
}

const char *launch_concat(const ConcatSource *src, int n_src, float *out, int h, int w, int groups, int n_seg, hipStream_t s) {
    ConcatGeom q{};
    unsigned C = 0;
    for (int k = 0; k < 4; k++) {
        const bool there = k < n_src;
        q.p[k] = there ? (const unsigned *)src[k].p : nullptr;
        q.total[k] = there ? 4u * (unsigned)src[k].total4 : 0;
        q.off[k] = there ? (unsigned)src[k].off : 0;
        q.start[k] = there ? C : 0xffffffffu;
        if (there) C += (unsigned)src[k].len;
    }
    q.c4n = C / 4;
    q.g = groups > 1 ? (unsigned)groups : 1;
    q.cg = C / q.g;
    const unsigned long long total4 = (unsigned long long)n_seg * h * w * q.c4n;
    if (!total4) return "";
    // at most eight workgroups a CU's worth of a 256-CU chip, as launch_pool: the rest of a large launch is the grid-stride loop's
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total4 + 255) / 256, (unsigned long long)kConcatMaxWorkgroups);
    if (groups > 1) {
        hipLaunchKernelGGL((concat_kernel<1>), dim3(blocks), dim3(256), 0, s, (uint4 *)out, q, total4);
        return "concat_kernel<SHUFFLE>";
    }
    hipLaunchKernelGGL((concat_kernel<0>), dim3(blocks), dim3(256), 0, s, (uint4 *)out, q, total4);
    return "concat_kernel<PLAIN>";
}

}  // namespace bh
