// kernels_bnact.hip -- a folded BatchNormalization + activation on an NHWC f32 tensor (model.hpp OP_BNACT): out[p][c] = act(fma(x[p][c],
// scale[c], shift[c])).  The relu(bn(cat(..))) that opens every DenseNet layer and transition and the relu(bn(sum)) that opens a
// pre-activation ResNet block: a norm no convolution in front of it can take.
//
// HBM-bound: one read and one write of the tensor.  A work item is one float4 of channels of one pixel; consecutive lanes take
// consecutive items, so every load and store is 16 bytes a lane, 1 KiB a wave, coalesced along C and across pixels.  Every element
// offset is 64 bits wide.  scale / shift are read as float4 through the cache, item by item: C is uncapped (the container's 65 536), so
// they are not held in registers, and the 2 x 4 C bytes of them stay in the L1 / L2 under a stream that is never read twice.  The
// channel group of an item is one 64-bit remainder a launch and a 32-bit add-and-wrap a trip: the grid's stride modulo C / 4 is the
// same for every trip.
//
// Arithmetic, the same in every precision mode and at every launch size (an item shares nothing with its neighbours): ONE __fmaf_rn, then
// the activation in its NaN-keeping run-time form, act_apply_pos(v, act, true) -- comparisons where fmaxf / v_med3_f32 would return
// the other operand, and the two limits act(+inf) = +inf, act(-inf) = 0 selected where the fast forms end in inf * 0.  The input is
// a residual stream or a concat: an f16 operand overflow in front of it must still reach the logits as inf / NaN for BH_FLAG_AUTO's
// re-run and BH_ERR_NONFINITE.  A NaN or inf element reaches its own output element and no other.
//
// Code size: the activation is a run-time argument of ONE instantiation.  A second one for ReLU alone (every DenseNet and v2 ResNet; a
// loop without exp / tanh / erf code) was built and measured: 1.312 against 1.349 ms and 1.149 against 1.177 ms for the switch running
// swish on densenet_audio's two largest tensors at 1 000 segments, under 3 % of a layer kind that is a seventh of that model's step.
// Dropped; what the one kernel reaches: profiles/bnact_layers.txt.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace bh {

namespace {

__global__ __launch_bounds__(256) void bnact_kernel(const float4 *__restrict__ in, const float4 *__restrict__ scale, const float4 *__restrict__ shift,
                                                     float4 *__restrict__ out, const unsigned long long total4, const unsigned c4n, const int act) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    unsigned c4 = (unsigned)(i % c4n);                      // (i < 2^19 at the grid's cap: the compiler's 64-bit path is taken once)
    const unsigned hop = (unsigned)(stride % c4n);          // c4 + hop < 2 c4n <= 2^15: one conditional subtraction a trip
    for (; i < total4; i += stride) {
        const float4 x = in[i], a = scale[c4], b = shift[c4];
        float4 y;
        y.x = __fmaf_rn(x.x, a.x, b.x); y.y = __fmaf_rn(x.y, a.y, b.y); y.z = __fmaf_rn(x.z, a.z, b.z); y.w = __fmaf_rn(x.w, a.w, b.w);
        y.x = act_apply_pos(y.x, act, true); y.y = act_apply_pos(y.y, act, true);
        y.z = act_apply_pos(y.z, act, true); y.w = act_apply_pos(y.w, act, true);
        out[i] = y;
        c4 += hop;
        c4 = c4 >= c4n ? c4 - c4n : c4;
    }
}

}  // namespace

// what model.hpp validate_model accepts of an OP_BNACT record: the channel count and the activation
bool bnact_supports(int C, int act) {
    return C >= 4 && C % 4 == 0 && C <= (1 << 16) &&
           (act == ACT_RELU || act == ACT_RELU6 || act == ACT_SWISH || act == ACT_GELU_ERF || act == ACT_GELU_TANH || act == ACT_HSWISH);
}

const char *launch_bnact(const float *in, const float *scale, const float *shift, float *out, unsigned long long n_pix, int C, int act, hipStream_t s) {
    if (!bnact_supports(C, act)) return nullptr;
    if (!n_pix) return "";
    const unsigned c4n = (unsigned)(C / 4);
    const unsigned long long total4 = n_pix * c4n;
    // at most eight workgroups a CU's worth of a 256-CU chip, as launch_pool: the rest of a large launch is the grid-stride loop's
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total4 + 255) / 256, 256ull * 8);
    hipLaunchKernelGGL(bnact_kernel, dim3(blocks), dim3(256), 0, s, (const float4 *)in, (const float4 *)scale, (const float4 *)shift, (float4 *)out,
                       total4, c4n, act);
    return "bnact_kernel";
}

}  // namespace bh
