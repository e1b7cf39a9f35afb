// BHM1 model container reader (format: birda_amd/modelfile.py).  Host only.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace bh {

enum Op : uint32_t { OP_CONV = 1, OP_DWCONV = 2, OP_PWCONV = 3, OP_GAP = 4, OP_DENSE = 5, OP_SCALE = 6, OP_POOL = 7, OP_GCONV = 8, OP_CONCAT = 10, OP_LNORM = 12, OP_REDUCE = 13, OP_BNACT = 14 };   // OP_SCALE: x * gate[n][c] (squeeze-excite; gate = res_tensor)
// OP_POOL (ONNX MaxPool / AveragePool, floor mode): the record's `reserved` word is the mode.  No weights, no bias, no activation.
enum PoolMode : uint32_t { POOL_MAX = 0, POOL_AVG = 1, POOL_AVG_PAD = 2 };   // AVG: over the in-image taps (count_include_pad = 0); AVG_PAD: over kh * kw
// OP_CONV (NHWC), OP_PWCONV, OP_DENSE: the record's `reserved` word is where `act` stands relative to the residual.  0: act(conv + b) + R
// (the only meaning of every file written before the flag existed); RES_ACT_AFTER: act(conv + b + R), the end of a ResNet block.
constexpr uint32_t RES_ACT_AFTER = 1;
// OP_GCONV (a grouped convolution, NHWC): the record's `reserved` word is the group count G, 1 < G; cin and cout are the totals, the
// weights compact [kh][kw][cin / G][cout] -- output channel o reads input channels (o / (cout / G)) * (cin / G) + 0 .. cin / G - 1 --,
// bias [cout].  G = 1 stays OP_CONV and one input channel per group with cout == cin stays OP_DWCONV: one spelling each.  No residual.
// OP_CONCAT = 10 (ONNX Concat / Split / Slice over the channels, and the Reshape -> Transpose -> Reshape channel shuffle): a copy, NHWC
// f32, no weights, bias or activation.  Code 9 is never used: it stays the "unknown layer op" that tests/test_gconv.py demands.
// in_tensor = source A, w_off = the first channel read from A, cin = how many; res_tensor = source B -- a SECOND INPUT, not a
// residual -- or NO_TENSOR (a window and / or a shuffle of A alone), b_off = the first channel read from B, which gives cout - cin
// channels; a source's channel count is its tensor's floats / (in_h in_w).  `reserved` = the shuffle's group count g (0, 1: none):
// out[p][c] = cat[p][(c % g) * (cout / g) + c / g], cat = A's window then B's.  Offsets and lengths are multiples of 4.
// OP_LNORM = 12 (ONNX LayerNormalization over the last axis of an [N, H, W, C] view, ConvNeXt's norm): a LayerNorm over the channels of
// an NHWC f32 tensor, pixel by pixel -- y[p][c] = (x[p][c] - mean_p) / sqrt(var_p + eps) * gamma[c] + beta[c], var_p the biased variance
// over the C channels of pixel p.  cin == cout == C (a multiple of 4), kernel / stride 1, pads 0, out image == in image, in_layout 0,
// never on tensor 0; w_off -> gamma[C], b_off -> beta[C]; no activation, no residual, no dilation; `reserved` = the bit pattern of eps
// as an f32, finite and > 0 (a constant pixel would otherwise be 0 * inf).  Code 11 is never used, like 9: both stay "unknown layer op".
// OP_REDUCE = 13 (ONNX ReduceMax / ReduceMean over H, over W or over both, GlobalMaxPool, and Add(ReduceMax, ReduceMean) of one window --
// the head of the PANNs audio CNNs): a reduction of an NHWC f32 tensor over a window that spans the whole image along each reduced
// axis.  Spelled like OP_GAP: cin == cout == C (a multiple of 4), kh = in_h or 1 and kw = in_w or 1 the window, stride 1, pads 0,
// out_h = in_h / kh, out_w = in_w / kw, in_layout 0, never on tensor 0; no weights, bias, activation, residual or dilation; at most
// 65 536 taps.  `reserved` is the mode; REDUCE_MAXMEAN is max + mean of the same window as one value.  One spelling each: the mean
// over both axes stays OP_GAP, and a 1x1 window is no reduction.
enum ReduceMode : uint32_t { REDUCE_MAX = 0, REDUCE_MEAN = 1, REDUCE_MAXMEAN = 2 };
// OP_BNACT = 14 (ONNX BatchNormalization + an activation on a tensor no convolution can take the BN into: the relu(bn(cat(..))) that opens
// every DenseNet layer and transition, the relu(bn(sum)) that opens a pre-activation ResNet block): y[p][c] = act(fma(x[p][c], scale[c],
// shift[c])) on an NHWC f32 tensor, f32 in every precision mode.  cin == cout == C (a multiple of 4), kernel / stride 1, pads 0, out
// image == in image, in_layout 0, never on tensor 0; w_off -> scale[C], b_off -> shift[C] (gamma / sqrt(var + eps) and beta - mean scale,
// folded by the writer), both at offsets that are multiples of 4; no residual, no dilation, `reserved` 0; `act` is RELU, RELU6, SWISH, GELU_ERF, GELU_TANH or HSWISH -- a norm
// without an activation folds into a convolution or is refused, and the gate activations are no layer's.  A code-14 record with a
// window other than 1x1 is no norm + activation layer at all: it stays "unknown layer op", as does code 15.
constexpr uint32_t NO_TENSOR = 0xFFFFFFFFu;
// Dilation (OP_CONV on an NHWC tensor, OP_DWCONV): the record's words at bytes 88 .. 95, skip_h and skip_w, are the rows and the columns
// SKIPPED between neighbouring taps, dilation - 1 per axis -- tap (dy, dx) reads pixel (oy sh - pad_t + dy (skip_h + 1),
// ox sw - pad_l + dx (skip_w + 1)).  Zero, the tail of every file written before the words existed, is the undilated layer: one
// spelling of it.  At most MAX_DILATION per axis, zero on an axis with one tap, zero on every other op.
constexpr uint32_t MAX_DILATION = 16;

#pragma pack(push, 1)
struct HeaderRec {
    char magic[4];
    uint32_t version, family, sample_rate, sample_count;
    float segment_duration;
    uint32_t n_classes, embedding_dim, n_branches, n_layers, output_activation, embedding_tensor;
    uint64_t blob_offset, blob_floats;
    uint32_t spec_h, spec_w;
    float norm_eps;
};
struct BranchRec {
    uint32_t frame_length, frame_step, fft_length, n_bins, n_mels, n_frames;
    float fmin, fmax, mag_scale, out_scale, out_shift;
    uint32_t flags;
    uint64_t mel_w_off;
};
struct LayerRec {
    uint32_t op, act, in_tensor, res_tensor, cin, cout, kh, kw, sh, sw, pad_t, pad_l;
    uint32_t in_h, in_w, out_h, out_w, in_layout, reserved;
    uint64_t w_off, b_off;
    uint32_t skip_h, skip_w;   // dilation - 1 per axis (above); the rest of the 128-byte record is not read
};
#pragma pack(pop)
static_assert(sizeof(LayerRec) == 96, "the layer record's read part: 96 of its 128 bytes");

struct Model {
    HeaderRec h{};
    std::vector<BranchRec> branches;
    std::vector<LayerRec> layers;
    std::vector<float> blob;
    std::vector<uint64_t> tensor_floats;  // per-segment floats of tensor i (0 = spectrogram)
    bool file_f16 = false;                // the file's convolution / dense weights were float16 tensors (an .onnx file; not in the container)

    uint64_t macs_per_segment() const {
        uint64_t t = 0;
        for (const auto &L : layers) {
            const uint64_t px = (uint64_t)L.out_h * L.out_w;
            if (L.op == OP_CONV) t += px * L.kh * L.kw * L.cin * L.cout;
            else if (L.op == OP_DWCONV) t += px * L.kh * L.kw * L.cout;
            else if (L.op == OP_GCONV && L.reserved) t += px * L.kh * L.kw * (L.cin / L.reserved) * L.cout;
            else if (L.op == OP_PWCONV || L.op == OP_DENSE) t += px * L.cin * L.cout;
        }
        return t;
    }
};

// The checks every model goes through, whichever file it came from (a BHM1 container, or an ONNX graph read by onnx_conv.hpp):
// every dimension is bounded (so that no size product below can wrap), every layer must read exactly the tensor its producer
// wrote, and every weight must lie inside the blob.  Fills tensor_floats.
inline bool validate_model(Model &m, std::string &err) {
    if (m.h.n_branches == 0 || m.h.n_branches > 16 || m.h.n_layers == 0 || m.h.n_layers > 4096 || m.branches.size() != m.h.n_branches ||
        m.layers.size() != m.h.n_layers || m.blob.size() != m.h.blob_floats) { err = "bad counts"; return false; }
    if (m.h.sample_count == 0 || m.h.sample_count > (1u << 24) || m.h.sample_rate == 0 || m.h.n_classes == 0 || m.h.n_classes > (1u << 24) ||
        m.h.spec_h == 0 || m.h.spec_w == 0 || m.h.spec_h > (1u << 14) || m.h.spec_w > (1u << 16)) { err = "bad model dimensions"; return false; }
    // the front-end's branches (round 6, tools/fuzz_create.py: a mutated mel_w_off -- 4.5e18 -- passed every check here and the operator
    // build read the blob there: SIGBUS.  None of these fields was checked against the blob, the segment or the spectrogram before.)
    for (const auto &b : m.branches) {
        if (b.frame_length < 4 || b.frame_length > (1u << 16) || (b.frame_length & 1) || b.fft_length != b.frame_length || b.n_bins != b.frame_length / 2 + 1 ||
            b.frame_step == 0 || b.frame_step > (1u << 16) || b.n_mels == 0 || b.n_mels != m.h.spec_h || b.n_frames == 0 || b.n_frames != m.h.spec_w) {
            err = "front-end branch geometry out of range (frame length / step / bins / mels / frames against the spectrogram)"; return false;
        }
        if ((uint64_t)(b.n_frames - 1) * b.frame_step + b.frame_length > m.h.sample_count) { err = "front-end frames run past the segment"; return false; }
        if (b.mel_w_off > m.h.blob_floats || (uint64_t)b.n_bins * b.n_mels > m.h.blob_floats - b.mel_w_off) { err = "mel matrix outside blob"; return false; }
        if (!std::isfinite(b.mag_scale) || !std::isfinite(b.out_scale) || !std::isfinite(b.out_shift)) { err = "front-end constants are not finite"; return false; }
    }
    if (!std::isfinite(m.h.norm_eps) || m.h.norm_eps < 0) { err = "normalisation epsilon out of range"; return false; }
    m.tensor_floats.assign(m.h.n_layers + 1, 0);
    m.tensor_floats[0] = (uint64_t)m.h.n_branches * m.h.spec_h * m.h.spec_w;
    for (uint32_t i = 0; i < m.h.n_layers; i++) {
        const auto &L = m.layers[i];
        // (a global pool's "kernel" is its whole input image -- the squeeze of a squeeze-excite gate in an early block pools 64 x 249)
        const uint32_t kmax = L.op == OP_GAP || L.op == OP_REDUCE ? (1u << 16) : 64;
        if ((L.cin == 0 && L.op != OP_CONCAT) || L.cout == 0 || L.cin > (1u << 16) || L.cout > (1u << 24) || L.kh == 0 || L.kw == 0 || L.kh > kmax || L.kw > kmax ||
            L.sh == 0 || L.sw == 0 || L.sh > 16 || L.sw > 16 || L.pad_t > 64 || L.pad_l > 64 || L.in_h == 0 || L.in_w == 0 || L.out_h == 0 ||
            L.out_w == 0 || L.in_h > (1u << 16) || L.in_w > (1u << 16) || L.out_h > (1u << 16) || L.out_w > (1u << 16) ||
            (uint64_t)L.out_h * L.out_w * L.cout > (1ull << 31) || (uint64_t)L.in_h * L.in_w * L.cin > (1ull << 31)) {
            err = "layer dimensions out of range"; return false;
        }
        m.tensor_floats[i + 1] = (uint64_t)L.out_h * L.out_w * L.cout;
        if (L.in_tensor > i || (L.res_tensor != NO_TENSOR && L.res_tensor > i)) { err = "layer reads a later tensor"; return false; }
        // what the layer reads must be what its input tensor holds (a pool reads in_h x in_w x cout, a dense layer cin values)
        const uint64_t in_floats = L.op == OP_GAP || L.op == OP_DWCONV || L.op == OP_SCALE || L.op == OP_POOL || L.op == OP_REDUCE || L.op == OP_BNACT ? (uint64_t)L.in_h * L.in_w * L.cout
                                 : L.op == OP_DENSE ? (uint64_t)L.cin
                                 : L.op == OP_CONCAT ? m.tensor_floats[L.in_tensor]   // (a window of its source: held below)
                                 : (uint64_t)L.in_h * L.in_w * L.cin;
        if (in_floats != m.tensor_floats[L.in_tensor]) { err = "layer input shape does not match its tensor"; return false; }
        if (L.res_tensor != NO_TENSOR && L.op != OP_SCALE && L.op != OP_CONCAT && m.tensor_floats[L.res_tensor] != m.tensor_floats[i + 1]) {
            err = "residual shape does not match the layer output"; return false;
        }
        if (L.op < OP_CONV || L.op > OP_BNACT || L.op == 9 || L.op == 11) { err = "unknown layer op"; return false; }
        // (a norm + activation layer has no window: a code-14 record with one is not this op, and is refused first and in the words of an
        //  unknown code, whatever else the record says)
        if (L.op == OP_BNACT && (L.kh != 1 || L.kw != 1)) { err = "unknown layer op: a norm + activation layer with a window other than 1x1"; return false; }
        if (L.op == OP_GCONV) {
            const uint32_t G = L.reserved;
            if (G < 2) { err = "grouped convolution with fewer than two groups (one group is a full convolution)"; return false; }
            if (L.cin % G || L.cout % G) { err = "grouped convolution whose group count does not divide its channels"; return false; }
            if ((L.cin / G) % 4 || (L.cout / G) % 4) { err = "grouped convolution with a group width that is not a multiple of 4"; return false; }
            if (L.res_tensor != NO_TENSOR) { err = "grouped convolution with a residual"; return false; }
            if (L.in_layout != 0 || L.in_tensor == 0) { err = "grouped convolution on the planar spectrogram (tensor 0)"; return false; }
            if (L.kh > 7 || L.kw > 7) { err = "grouped convolution with a kernel outside 1 .. 7"; return false; }
            if (L.sh > 2 || L.sw > 2) { err = "grouped convolution with a stride outside 1 .. 2"; return false; }
        }
        const uint64_t wn = L.op == OP_CONV ? (uint64_t)L.kh * L.kw * L.cin * L.cout
                          : L.op == OP_GCONV ? (uint64_t)L.kh * L.kw * (L.cin / L.reserved) * L.cout
                          : L.op == OP_DWCONV ? (uint64_t)L.kh * L.kw * L.cout
                          : (L.op == OP_PWCONV || L.op == OP_DENSE) ? (uint64_t)L.cin * L.cout : 0;
        if (L.op == OP_SCALE && (L.res_tensor == NO_TENSOR || m.tensor_floats[L.res_tensor] != L.cout || L.cin != L.cout)) { err = "scale layer without a [C] gate"; return false; }
        if (L.op == OP_POOL) {
            if (L.reserved > POOL_AVG_PAD) { err = "pool layer with an unknown mode"; return false; }
            if (L.cin != L.cout) { err = "pool layer that changes the channel count"; return false; }
            if (L.act != 0) { err = "pool layer with an activation"; return false; }
            if (L.res_tensor != NO_TENSOR) { err = "pool layer with a residual"; return false; }
            if (L.in_layout != 0 || L.in_tensor == 0) { err = "pool layer on the planar spectrogram (tensor 0)"; return false; }
            // every window holds at least one pixel of the image: max never comes from nothing, the in-image mean never divides by zero
            if (L.pad_t >= L.kh || L.pad_l >= L.kw || (uint64_t)(L.out_h - 1) * L.sh >= (uint64_t)L.in_h + L.pad_t ||
                (uint64_t)(L.out_w - 1) * L.sw >= (uint64_t)L.in_w + L.pad_l) { err = "pool layer with a window outside the image"; return false; }
        }
        if (L.op == OP_CONCAT) {
            const bool two = L.res_tensor != NO_TENSOR;
            const uint64_t img = (uint64_t)L.in_h * L.in_w;
            if (L.act != 0) { err = "concat layer with an activation"; return false; }
            if (L.kh != 1 || L.kw != 1 || L.sh != 1 || L.sw != 1 || L.pad_t != 0 || L.pad_l != 0) { err = "concat layer with a kernel, stride or padding other than 1 / 1 / 0"; return false; }
            if (L.in_h != L.out_h || L.in_w != L.out_w) { err = "concat layer whose output image is not its input image"; return false; }
            if (L.in_layout != 0 || L.in_tensor == 0 || L.res_tensor == 0) { err = "concat layer on the planar spectrogram (tensor 0)"; return false; }
            if (L.cin == 0 || L.cin > L.cout || (two ? L.cout == L.cin : L.cout != L.cin)) { err = "concat layer whose output channels are not the sum of its windows"; return false; }
            if (L.w_off % 4 || L.cin % 4 || L.cout % 4 || (two && L.b_off % 4)) { err = "concat layer with an offset or a length that is not a multiple of 4"; return false; }
            if (m.tensor_floats[L.in_tensor] % img || (two && m.tensor_floats[L.res_tensor] % img)) { err = "concat layer with a source that does not hold whole images of its size"; return false; }
            const uint64_t ca = m.tensor_floats[L.in_tensor] / img, cb = two ? m.tensor_floats[L.res_tensor] / img : 0;
            if (L.w_off > ca || L.cin > ca - L.w_off || (two && (L.b_off > cb || L.cout - L.cin > cb - L.b_off))) { err = "concat layer with a window past its source's channels"; return false; }
            if (L.reserved > 1 && (L.reserved > L.cout || L.cout % L.reserved)) { err = "concat layer with a shuffle group count that does not divide its channels"; return false; }
        }
        if (L.op == OP_LNORM) {
            float eps;
            memcpy(&eps, &L.reserved, sizeof eps);
            if (L.act != 0) { err = "layer norm with an activation"; return false; }
            if (L.res_tensor != NO_TENSOR) { err = "layer norm with a residual"; return false; }
            if (L.kh != 1 || L.kw != 1 || L.sh != 1 || L.sw != 1 || L.pad_t != 0 || L.pad_l != 0) { err = "layer norm with a kernel, stride or padding other than 1 / 1 / 0"; return false; }
            if (L.in_h != L.out_h || L.in_w != L.out_w) { err = "layer norm whose output image is not its input image"; return false; }
            if (L.cin != L.cout) { err = "layer norm that changes the channel count"; return false; }
            if (L.in_layout != 0 || L.in_tensor == 0) { err = "layer norm on the planar spectrogram (tensor 0)"; return false; }
            if (L.cout % 4) { err = "layer norm over a channel count that is not a multiple of 4"; return false; }
            if (!std::isfinite(eps) || !(eps > 0.0f)) { err = "layer norm with an epsilon that is not finite and > 0"; return false; }
            if (L.w_off > m.h.blob_floats || L.b_off > m.h.blob_floats || L.cout > m.h.blob_floats - L.w_off || L.cout > m.h.blob_floats - L.b_off) {
                err = "layer norm gamma / beta outside the blob"; return false;
            }
        }
        if (L.op == OP_REDUCE) {
            // (the mode word selects the operation -- three of them share the code --, so a mode outside the table is an operation the
            //  table does not hold: refused first and in the words of an unknown code, whatever else the record says)
            if (L.reserved > REDUCE_MAXMEAN) { err = "unknown layer op: a reduce layer with an unknown mode"; return false; }
            if (L.cin != L.cout) { err = "reduce layer that changes the channel count"; return false; }
            if (L.cout % 4) { err = "reduce layer over a channel count that is not a multiple of 4"; return false; }
            if (L.act != 0) { err = "reduce layer with an activation"; return false; }
            if (L.res_tensor != NO_TENSOR) { err = "reduce layer with a residual"; return false; }
            if (L.in_layout != 0 || L.in_tensor == 0) { err = "reduce layer on the planar spectrogram (tensor 0)"; return false; }
            if (L.sh != 1 || L.sw != 1 || L.pad_t != 0 || L.pad_l != 0) { err = "reduce layer with a stride or padding other than 1 / 0"; return false; }
            if ((L.kh != 1 && L.kh != L.in_h) || (L.kw != 1 && L.kw != L.in_w)) { err = "reduce layer with a window that is neither the whole axis nor 1"; return false; }
            if (L.kh == 1 && L.kw == 1) { err = "reduce layer with a 1x1 window (no reduction)"; return false; }
            if (L.out_h != L.in_h / L.kh || L.out_w != L.in_w / L.kw) { err = "reduce layer whose output image is not its input image over its window"; return false; }
            if ((uint64_t)L.kh * L.kw > (1u << 16)) { err = "reduce layer over more than 65 536 taps"; return false; }
            if (L.reserved == REDUCE_MEAN && L.kh == L.in_h && L.kw == L.in_w && L.kh > 1 && L.kw > 1) {
                err = "reduce layer that is the mean over both axes (OP_GAP is its one spelling)"; return false;
            }
        }
        if (L.op == OP_BNACT) {
            if (L.sh != 1 || L.sw != 1 || L.pad_t != 0 || L.pad_l != 0) { err = "norm + activation layer with a stride or padding other than 1 / 0"; return false; }
            if (L.in_h != L.out_h || L.in_w != L.out_w) { err = "norm + activation layer whose output image is not its input image"; return false; }
            if (L.cin != L.cout) { err = "norm + activation layer that changes the channel count"; return false; }
            if (L.cout % 4) { err = "norm + activation layer over a channel count that is not a multiple of 4"; return false; }
            if (L.in_layout != 0 || L.in_tensor == 0) { err = "norm + activation layer on the planar spectrogram (tensor 0)"; return false; }
            if (L.res_tensor != NO_TENSOR) { err = "norm + activation layer with a residual"; return false; }
            if (L.reserved != 0) { err = "norm + activation layer with a reserved word that is not 0"; return false; }
            if (L.act == 0) { err = "norm + activation layer without an activation"; return false; }
            if (L.act == 6 || L.act == 8) { err = "norm + activation layer with a gate activation (sigmoid / hard sigmoid)"; return false; }
            if (L.act > 8) { err = "norm + activation layer with an unknown activation"; return false; }
            if (L.w_off > m.h.blob_floats || L.b_off > m.h.blob_floats || L.cout > m.h.blob_floats - L.w_off || L.cout > m.h.blob_floats - L.b_off) {
                err = "norm + activation layer scale / shift outside the blob"; return false;
            }
            // (the kernel reads both as float4: every writer puts them on 16-float boundaries, and a file is untrusted input)
            if (L.w_off % 4 || L.b_off % 4) { err = "norm + activation layer scale / shift at an offset that is not a multiple of 4"; return false; }
        }
        if (L.op == OP_CONV && L.in_layout != 0) {
            if (L.reserved == RES_ACT_AFTER) { err = "activation after the residual on the NCHW stem convolution"; return false; }
        } else if (L.op == OP_CONV || L.op == OP_PWCONV || L.op == OP_DENSE) {
            if (L.reserved > RES_ACT_AFTER) { err = "layer with an unknown activation position"; return false; }
            if (L.reserved == RES_ACT_AFTER && L.res_tensor == NO_TENSOR) { err = "activation after the residual on a layer without a residual"; return false; }
            if (L.reserved == RES_ACT_AFTER && L.act == 0) { err = "activation after the residual without an activation (a plain residual is position 0)"; return false; }
        }
        if (L.skip_h || L.skip_w) {
            static const char *const names[] = {"?", "stem convolution", "depthwise", "pointwise", "global pool", "dense", "scale", "pool", "grouped convolution", "?", "concat", "?", "layer norm", "reduce", "norm + activation"};
            if (!(L.op == OP_DWCONV || (L.op == OP_CONV && L.in_layout == 0))) {
                err = std::string("dilation on a ") + names[L.op] + " layer"; return false;
            }
            if (L.skip_h >= MAX_DILATION || L.skip_w >= MAX_DILATION) { err = "dilation above 16"; return false; }
            if ((L.kh == 1 && L.skip_h) || (L.kw == 1 && L.skip_w)) { err = "dilation on an axis with one tap (dilation 1 is its one spelling)"; return false; }
        }
        if (L.op != OP_GAP && L.op != OP_SCALE && L.op != OP_POOL && L.op != OP_CONCAT && L.op != OP_LNORM && L.op != OP_REDUCE && L.op != OP_BNACT && (L.w_off > m.h.blob_floats || L.b_off > m.h.blob_floats || L.w_off + wn > m.h.blob_floats ||
                                                   L.b_off + L.cout > m.h.blob_floats)) {
            err = "layer weights outside blob"; return false;
        }
    }
    if (m.h.embedding_tensor > m.h.n_layers) { err = "bad embedding tensor"; return false; }
    return true;
}

inline bool load_model(const char *path, Model &m, std::string &err) {
    FILE *f = fopen(path, "rb");
    if (!f) { err = std::string("cannot open model file ") + path; return false; }
    auto bad = [&](const char *why) { err = std::string(path) + ": " + why; fclose(f); return false; };
    unsigned char hdr[256];
    if (fread(hdr, 1, 256, f) != 256) return bad("truncated header");
    memcpy(&m.h, hdr, sizeof m.h);
    if (memcmp(m.h.magic, "BHM1", 4) != 0 || m.h.version != 1) return bad("not a BHM1 v1 model");
    if (m.h.n_branches == 0 || m.h.n_branches > 16 || m.h.n_layers == 0 || m.h.n_layers > 4096) return bad("bad counts");
    m.branches.resize(m.h.n_branches);
    m.layers.resize(m.h.n_layers);
    for (auto &b : m.branches) {
        unsigned char rec[64];
        if (fread(rec, 1, 64, f) != 64) return bad("truncated branch table");
        memcpy(&b, rec, sizeof b);
    }
    for (auto &L : m.layers) {
        unsigned char rec[128];
        if (fread(rec, 1, 128, f) != 128) return bad("truncated layer table");
        memcpy(&L, rec, sizeof L);
    }
    // the file is untrusted input: sizes are checked against the file before anything is allocated from them, every dimension is
    // bounded (so that no product below can wrap), and every layer must read exactly the tensor its producer wrote
    if (fseek(f, 0, SEEK_END) != 0) return bad("cannot seek");
    const long fsize = ftell(f);
    if (fsize < 0 || m.h.blob_floats > (1ull << 31) || m.h.blob_offset > (uint64_t)fsize ||
        m.h.blob_floats * sizeof(float) > (uint64_t)fsize - m.h.blob_offset)
        return bad("weights outside the file");
    if (m.h.sample_count == 0 || m.h.sample_count > (1u << 24) || m.h.sample_rate == 0 || m.h.n_classes == 0 || m.h.n_classes > (1u << 24) ||
        m.h.spec_h == 0 || m.h.spec_w == 0 || m.h.spec_h > (1u << 14) || m.h.spec_w > (1u << 16))
        return bad("bad model dimensions");
    m.blob.resize(m.h.blob_floats);
    if (fseek(f, (long)m.h.blob_offset, SEEK_SET) != 0) return bad("bad blob offset");
    if (fread(m.blob.data(), sizeof(float), m.h.blob_floats, f) != m.h.blob_floats) return bad("truncated weights");
    fclose(f);
    return validate_model(m, err);
}

// BHC1: a custom classifier on embeddings (birda_amd/modelfile.py write_custom_classifier): dense layers + output activation
#pragma pack(push, 1)
struct CustomHeaderRec {
    char magic[4];
    uint32_t version, input_dim, n_layers, n_classes, output_activation;
    uint64_t blob_offset, blob_floats;
};
struct CustomLayerRec {
    uint32_t in_dim, out_dim, act, reserved;
    uint64_t w_off, b_off;   // W [in][out] row-major, b [out]
};
#pragma pack(pop)

struct CustomModel {
    CustomHeaderRec h{};
    std::vector<CustomLayerRec> layers;
    std::vector<float> blob;
};

inline bool load_custom_model(const char *path, CustomModel &m, std::string &err) {
    FILE *f = fopen(path, "rb");
    if (!f) { err = std::string("cannot open custom classifier file ") + path; return false; }
    auto bad = [&](const char *why) { err = std::string(path) + ": " + why; fclose(f); return false; };
    unsigned char hdr[64];
    if (fread(hdr, 1, 64, f) != 64) return bad("truncated header");
    memcpy(&m.h, hdr, sizeof m.h);
    if (memcmp(m.h.magic, "BHC1", 4) != 0 || m.h.version != 1) return bad("not a BHC1 v1 custom classifier");
    if (m.h.n_layers == 0 || m.h.n_layers > 64 || m.h.input_dim == 0 || m.h.n_classes == 0) return bad("bad counts");
    m.layers.resize(m.h.n_layers);
    for (auto &L : m.layers) {
        unsigned char rec[32];
        if (fread(rec, 1, 32, f) != 32) return bad("truncated layer table");
        memcpy(&L, rec, sizeof L);
    }
    if (fseek(f, 0, SEEK_END) != 0) return bad("cannot seek");
    const long fsize = ftell(f);
    if (fsize < 0 || m.h.blob_floats > (1ull << 31) || m.h.blob_offset > (uint64_t)fsize ||
        m.h.blob_floats * sizeof(float) > (uint64_t)fsize - m.h.blob_offset)
        return bad("weights outside the file");
    if (m.h.input_dim > (1u << 20) || m.h.n_classes > (1u << 24)) return bad("bad dimensions");
    m.blob.resize(m.h.blob_floats);
    if (fseek(f, (long)m.h.blob_offset, SEEK_SET) != 0) return bad("bad blob offset");
    if (fread(m.blob.data(), sizeof(float), m.h.blob_floats, f) != m.h.blob_floats) return bad("truncated weights");
    fclose(f);
    uint32_t dim = m.h.input_dim;
    for (const auto &L : m.layers) {
        if (L.in_dim != dim || L.out_dim == 0 || L.out_dim > (1u << 24)) { err = "custom classifier: layer widths do not chain"; return false; }
        if (L.w_off > m.h.blob_floats || L.b_off > m.h.blob_floats || L.w_off + (uint64_t)L.in_dim * L.out_dim > m.h.blob_floats || L.b_off + L.out_dim > m.h.blob_floats) { err = "custom classifier: weights outside blob"; return false; }
        dim = L.out_dim;
    }
    if (dim != m.h.n_classes) { err = "custom classifier: last layer width != n_classes"; return false; }
    return true;
}

}  // namespace bh
