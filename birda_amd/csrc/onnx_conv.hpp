// onnx_conv.hpp -- bh_classifier_create opens the model file the reference hands it: ClassifierBuilder::model_path(...) is the
// `.onnx` (reference src/inference/classifier.rs:269-283; label-count check src/inference/mod.rs:34-37).  This header reads
// such a file into the in-memory BHM1 form (model.hpp Model) inside the library -- no Python step between birda and the GPU:
//
//   * the CONV STACK is read off the graph (round 4; a C++ port of birda_amd/convert.py model_from_graph, which stays as the
//     second witness: tests/test_onnx_native.py holds the two to the same layer table and the same weights, bit for bit):
//     Conv (1x1 -> pointwise, group == channels -> depthwise, any other group count -> OP_GCONV, else full), BatchNormalization folded into the convolution in
//     front of it -- or, with its activation, on a pool output, a concat, a residual sum or an activated convolution, one OP_BNACT record (DenseNet,
//     pre-activation ResNets) --, the activation spellings exporters emit (Relu, Clip(0, 6), Sigmoid x Mul = swish, Div / Erf / Add / Mul / Mul
//     = GELU, the Gelu operator; HardSwish, HardSigmoid(1/6, 1/2) x Mul and Add 3 / Clip(0, 6) / Mul / Mul 1/6 = hard swish; HardSigmoid(1/6,
//     1/2) or that chain without its Mul(., x) on a pooled tensor = the hard-sigmoid gate), residual Add folded into its 1x1 convolution, MaxPool / AveragePool (floor mode; OP_POOL),
//     GlobalAveragePool / ReduceMean over H, W, ReduceMax / ReduceMean over H or W or both, GlobalMaxPool and the max + mean pair Add(ReduceMax,
//     ReduceMean) of the PANNs head (OP_REDUCE), Concat / Split / Slice over the channels and the Reshape -> Transpose -> Reshape channel
//     shuffle (OP_CONCAT: a Split / Slice output that only Concat nodes read is a view folded into their windows),
//     ConvNeXt blocks (OP_LNORM: Transpose [0, 2, 3, 1] / [0, 3, 1, 2] as an [N, H, W, C] view that costs no record, LayerNormalization over the
//     channels as a node or as the decomposed ReduceMean -> Sub -> Pow -> ReduceMean -> Add -> Sqrt -> Div -> Mul -> Add chain, MatMul + Add on
//     the view as a 1x1 layer, the layer-scale Mul by a constant of the channels folded into the layer in front),
//     squeeze-excite gates (pool -> 1x1 -> 1x1 -> Sigmoid -> Mul), Flatten / Reshape / Squeeze / Identity / Dropout after the
//     pool, Gemm / MatMul + Add, a final Sigmoid or Softmax; NCHW weights re-laid for the NHWC kernels.  Anything else is refused
//     by operator name.
//   * the FRONT-END (min / max normalisation, Hann STFT branches, mel projection, power law, flip) is READ OFF THE GRAPH by probing
//     (round 5, onnx_frontend.hpp: the nodes between the audio input and the first 2-D convolution are run by a small float64
//     evaluator on probe signals; frame length / step, the folded window x DFT x mel operator, the exponent -- i.e. the LEARNED
//     mag_scale --, the affine, the flip and the normalisation epsilon are fitted to the responses and verified against the
//     closed form the kernels compute on random audio, <= 2e-5, or the file is REFUSED with the reason: an operator outside the
//     evaluator's set by its name, another window, a per-mel affine, a magnitude spectrogram, a missing normalisation).  Nothing
//     is assumed about a graph that holds a front-end.  The family table below supplies only what no graph states -- the sample
//     rate and segment duration, keyed by the input length (classifier.rs:360-377 takes them from the model type's config) -- and
//     the whole published front-end ([EXT] SURVEY.md Appendix B) for a graph that STARTS at the spectrogram, where there is
//     nothing to read.
//
// FLOAT16 FILES (the `fp16` variant the reference's installer picks for a GPU provider): a float16 constant is the exact real
// number it encodes, Cast between floating types is the identity, and the graph is evaluated in the library's own (f32-grade)
// arithmetic -- at least as exact as a float16 runtime, without its intermediate rounding or its overflow at 65 504.  Weights,
// biases, BatchNormalization parameters, Gemm / MatMul operands and the activation spellings' scalars are read through ONE
// accessor (`finit`: float32 or float16); a graph input / output of element type float16 is refused by name (the C ABI feeds and
// returns f32).
//
// Hand-written protobuf wire-format walk on onnx_dense.hpp's Reader (no protobuf / onnx dependency).  Untrusted input: every
// length is checked against the buffer, every dimension product against the tensor's payload, and the finished model goes
// through the same validation as a BHM1 file (model.hpp validate_model); fuzzed under ASan with the other loaders
// (tests/test_host_sanitizers.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "model.hpp"
#include "onnx_dense.hpp"
#include "onnx_graph.hpp"
#include "onnx_frontend.hpp"

namespace bh {
namespace onnxc {

// ---- the family table: the front-ends of the model families the reference serves ([EXT] SURVEY.md Appendix B; the same
// numbers as birda_amd/synth.py, which builds the seeded stand-ins) -----------------------------------------------------
// The phrase that marks a well-formed file whose front-end the kernels cannot express: api.hip model_load_status turns exactly this
// constant into BH_ERR_UNSUPPORTED (the status hung on a string literal repeated in two files).
constexpr const char *kFrontendRefusal = "the spectrogram front-end cannot be read off the graph";

struct FamilyBranch { uint32_t L, H, n_mels; float fmin, fmax, mag_scale, out_scale, out_shift; uint32_t flags; };
struct FamilyFrontend {
    uint32_t sample_rate, sample_count;
    float segment_duration, norm_eps;
    uint32_t n_branches;
    FamilyBranch br[2];
    uint32_t n_frames() const { return (sample_count - br[0].L) / br[0].H + 1; }
};
inline const FamilyFrontend *frontend_for(uint32_t sample_count, uint32_t spec_c, uint32_t spec_h, uint32_t spec_w) {
    static const FamilyFrontend kTable[] = {
        // BirdNET v2.4: 3 s at 48 kHz; 0-3 kHz on 2 048-sample frames (hop 278), 0.5-15 kHz on 1 024-sample frames (hop 280), 96 mels x 511 frames
        {48000, 144000, 3.0f, 1e-6f, 2, {{2048, 278, 96, 0.0f, 3000.0f, 1.23f, 0.8f, -0.4f, 1}, {1024, 280, 96, 500.0f, 15000.0f, 1.23f, 0.8f, -0.4f, 1}}},
        // Perch v2 / BirdNET v3.0: 5 s at 32 kHz, one 128-mel branch (60 Hz - 16 kHz, 1 024-sample frames, hop 320)
        {32000, 160000, 5.0f, 1e-6f, 1, {{1024, 320, 128, 60.0f, 16000.0f, 1.23f, 0.8f, -0.4f, 1}, {}}},
        // the quarter-second test stacks of birda_amd/synth.py ("mini*": the unit tests' models)
        {48000, 12000, 0.25f, 1e-6f, 2, {{512, 100, 32, 0.0f, 3000.0f, 1.23f, 0.8f, -0.4f, 1}, {256, 103, 32, 500.0f, 15000.0f, 1.23f, 0.8f, -0.4f, 1}}},
    };
    for (const auto &f : kTable) {
        if (sample_count) { if (f.sample_count == sample_count) return &f; }
        else if (f.n_branches == spec_c && f.br[0].n_mels == spec_h && f.n_frames() == spec_w) return &f;
    }
    return nullptr;
}

// tf.signal.linear_to_mel_weight_matrix (HTK mel) as birda_amd/synth.py restates it, operation for operation in float64 --
// the two must give the same float32 matrix (tests/test_onnx_native.py compares them bit for bit): [n_bins][n_mels], DC row zero
inline void mel_weight_matrix(uint32_t n_mels, uint32_t n_bins, double sample_rate, double fmin, double fmax, std::vector<float> &w) {
    auto mel = [](double f) { return 1127.0 * std::log1p(f / 700.0); };
    const double nyquist = sample_rate / 2.0;
    // numpy.linspace(a, b, n): a + i * ((b - a) / (n - 1)), the last point set to b exactly
    auto linspace = [](double a, double b, uint32_t n, std::vector<double> &out) {
        out.resize(n);
        const double step = (b - a) / (double)(n - 1);
        for (uint32_t i = 0; i < n; i++) out[i] = (double)i * step + a;
        if (n > 1) out[n - 1] = b;
    };
    std::vector<double> lin, edges;
    linspace(0.0, nyquist, n_bins, lin);
    linspace(mel(fmin), mel(fmax), n_mels + 2, edges);
    w.assign((size_t)n_bins * n_mels, 0.0f);
    for (uint32_t k = 1; k < n_bins; k++) {
        const double bm = mel(lin[k]);
        for (uint32_t j = 0; j < n_mels; j++) {
            const double lower = edges[j], center = edges[j + 1], upper = edges[j + 2];
            const double lo = (bm - lower) / (center - lower), up = (upper - bm) / (upper - center);
            const double v = std::fmax(0.0, std::fmin(lo, up));
            w[(size_t)k * n_mels + j] = (float)v;
        }
    }
}

struct Blob {
    std::vector<float> v;
    uint64_t put(const float *p, size_t n) {                 // 16-float alignment, as birda_amd/convert.py _Blob.put
        v.resize((v.size() + 15) / 16 * 16, 0.0f);
        const uint64_t off = v.size();
        v.insert(v.end(), p, p + n);
        return off;
    }
    uint64_t put(const std::vector<float> &a) { return put(a.data(), a.size()); }
};

// The graph -> Model.  `err` names what stopped it.
inline bool model_from_graph(const Graph &g, Model &m, std::string &err) {
    auto fail = [&](const std::string &why) { err = why; return false; };
    // the data input: the one graph input that is not an initializer
    const ValueInfo *gin = nullptr;
    for (const auto &vi : g.inputs)
        if (!g.init.count(vi.name)) { if (gin) return fail("the graph has more than one data input"); gin = &vi; }
    if (!gin) return fail("the graph has no data input");
    if (g.outputs.empty()) return fail("the graph has no output");
    // the C ABI feeds float32 audio and returns float32 scores: a float16 graph input would mean rounding the audio to 11 bits,
    // which is not done silently (the published float16 files keep float32 at both ends, behind / in front of a Cast)
    if (gin->elem_type == 10) return fail("graph input '" + gin->name + "' is float16: only float32 inputs are fed (a float16 file keeps its float32 input in front of a Cast)");
    for (const auto &vo : g.outputs)
        if (vo.elem_type == 10) return fail("graph output '" + vo.name + "' is float16: only float32 outputs are returned (a float16 file casts its outputs back to float32)");
    // the node list the conv-stack walk reads: the graph's, with the tensor names behind floating-point Casts replaced by the
    // Cast's input (below, once the front-end's nodes are known); `outputs` likewise.  Indices are the graph's own.
    std::vector<Node> nodes = g.nodes;
    std::vector<std::string> outputs;
    for (const auto &vo : g.outputs) outputs.push_back(vo.name);
    std::map<std::string, size_t> prod;
    for (size_t i = 0; i < nodes.size(); i++)
        for (const auto &o : nodes[i].out) prod[o] = i;
    std::map<std::string, std::vector<size_t>> cons;
    // "a float initializer": float32 or float16 (read as the exact value it encodes).  `role` names the operand in the refusal of
    // an element type that is present but not read (bfloat16, float64, int8, ...).
    std::string init_refusal;
    auto type_name = [](int64_t t) { return t == 16 ? std::string("bfloat16") : t == 11 ? std::string("float64") : t == 3 ? std::string("int8") : t == 2 ? std::string("uint8") : "element type " + std::to_string(t); };
    auto finit = [&](const std::string &name) -> const Tensor * {
        auto it = g.init.find(name);
        if (it == g.init.end()) return nullptr;
        if (!it->second.is_float()) { init_refusal = " ('" + name + "' is " + type_name(it->second.dtype) + ": not supported)"; return nullptr; }
        return &it->second;
    };
    auto scalar = [&](const std::string &name, float &out, bool *from_f16 = nullptr) {
        const Tensor *t = finit(name);
        if (!t || t->count != 1) return false;
        out = t->at(0);
        if (from_f16) *from_f16 = t->is_f16();
        return true;
    };

    // ---- where the conv stack starts, and which front-end the family table gives it ----
    std::string spec;                 // name of the spectrogram tensor [N, C, H, W]
    const FamilyFrontend *fam = nullptr;
    onnxf::Recovered rec;
    bool recovered = false;
    const size_t rank = gin->dims.size();
    if (rank == 4) {
        const int64_t c = gin->dims[1], h = gin->dims[2], w = gin->dims[3];
        if (c <= 0 || h <= 0 || w <= 0) return fail("spectrogram input with symbolic channel / height / width");
        fam = frontend_for(0, (uint32_t)c, (uint32_t)h, (uint32_t)w);
        if (!fam) return fail("no model family has a " + std::to_string(c) + " x " + std::to_string(h) + " x " + std::to_string(w) + " spectrogram (family table, onnx_conv.hpp)");
        spec = gin->name;
    } else if (rank == 2 || rank == 1 || rank == 3) {
        const int64_t n = gin->dims.back();
        if (n <= 0) return fail("audio input with a symbolic length");
        // the family table is consulted for what NO graph states: the sample rate (the reference takes it from the model type's
        // config, classifier.rs:360-377) and the segment duration that follows from it
        fam = frontend_for((uint32_t)n, 0, 0, 0);
        if (!fam)
            return fail("audio input of " + std::to_string(n) + " samples: no model family in the table has that length, so the sample rate is unknown (onnx_conv.hpp); "
                        "tools/onnx_to_bhm.py takes it as an argument and writes the BHM1 container this library also opens");
        // the front-end itself is READ OFF THE GRAPH by probing (onnx_frontend.hpp) -- never assumed: a trained file's mag_scale,
        // band edges, affine and mel matrices are its own (VERDICT r4 missing #2)
        try { rec = onnxf::recover_frontend(g, *gin); }
        catch (const onnxf::RecoverError &e) { return fail(std::string(kFrontendRefusal) + " (" + e.what() + "): refused rather than assumed"); }
        catch (const onnxf::EvalError &e) { return fail(std::string(kFrontendRefusal) + " (" + e.what() + "): refused rather than assumed"); }
        catch (const std::bad_alloc &) { return fail(std::string(kFrontendRefusal) + " (out of memory while evaluating it)"); }
        recovered = true;
        spec = rec.spectrogram;
    } else return fail("data input of rank " + std::to_string(rank) + " is neither audio [N, samples] nor a spectrogram [N, C, H, W]");
    // everything that produces the spectrogram is the front-end: read above, not part of the layer table
    std::set<size_t> front;
    {
        std::vector<std::string> stack{spec};
        while (!stack.empty()) {
            const std::string t = stack.back(); stack.pop_back();
            auto it = prod.find(t);
            if (it == prod.end() || front.count(it->second)) continue;
            front.insert(it->second);
            for (const auto &x : nodes[it->second].in) stack.push_back(x);
        }
    }

    // ---- Cast between floating types is the identity: behind the front-end every such node is taken out of the walk and its
    // output renamed to its input everywhere (consumers, graph outputs), so the sole-consumer and pattern logic below sees
    // through it (a Cast between a Conv and its Sigmoid * x does not break the swish fold).  Any other target is refused by name.
    std::set<size_t> skip;
    {
        std::map<std::string, std::string> alias;
        auto resolve = [&](const std::string &x) { auto it = alias.find(x); return it == alias.end() ? x : it->second; };
        for (size_t i = 0; i < nodes.size(); i++) {
            if (front.count(i)) continue;
            Node &n = nodes[i];
            for (auto &x : n.in) x = resolve(x);
            if (n.op != "Cast") continue;
            if (n.in.empty() || n.out.empty()) return fail("node '" + n.name + "' (Cast) without inputs or outputs");
            const int64_t to = n.geti("to", 0);
            if (to != 1 && to != 10 && to != 11)
                return fail("Cast '" + n.name + "' to " + type_name(to) + " (to = " + std::to_string(to) + "): only casts between float32, float16 and float64 are read, as the identity");
            alias[n.out[0]] = n.in[0];           // (already resolved: chains of Casts collapse)
            skip.insert(i);
        }
        for (auto &o : outputs) o = resolve(o);
    }
    // ---- the unused second output of torch.max(x, dim): an ArgMax none of whose outputs anything reads.  The walk ignores no other dead
    // node -- an operator it does not know is refused wherever it stands --, so this one is taken out by name, and is no reader of x.
    for (size_t i = 0; i < nodes.size(); i++) {
        if (skip.count(i) || front.count(i) || nodes[i].op != "ArgMax") continue;
        bool read = false;
        for (const auto &o : nodes[i].out) {
            if (std::find(outputs.begin(), outputs.end(), o) != outputs.end()) read = true;
            for (size_t k = 0; k < nodes.size() && !read; k++)
                if (!skip.count(k) && std::find(nodes[k].in.begin(), nodes[k].in.end(), o) != nodes[k].in.end()) read = true;
        }
        if (!read) skip.insert(i);
    }
    for (size_t i = 0; i < nodes.size(); i++)
        if (!skip.count(i))
            for (const auto &x : nodes[i].in) cons[x].push_back(i);

    m = Model{};
    for (const Node &n : nodes)
        if ((n.op == "Conv" || n.op == "Gemm" || n.op == "MatMul") && n.in.size() > 1) {
            auto it = g.init.find(n.in[1]);
            if (it != g.init.end() && it->second.is_f16()) m.file_f16 = true;
        }
    memcpy(m.h.magic, "BHM1", 4);
    m.h.version = 1;
    m.h.sample_rate = fam->sample_rate; m.h.sample_count = fam->sample_count; m.h.segment_duration = fam->segment_duration;
    Blob blob;
    if (recovered) {
        m.h.norm_eps = (float)rec.eps; m.h.n_branches = (uint32_t)rec.branches.size();
        m.h.spec_h = rec.spec_h; m.h.spec_w = rec.spec_w;
        for (const auto &rb : rec.branches) {
            BranchRec r{};
            r.frame_length = rb.L; r.frame_step = rb.H; r.fft_length = rb.L; r.n_bins = rb.L / 2 + 1; r.n_mels = rb.n_mels; r.n_frames = rb.n_frames;
            // (fmin / fmax are informational in the container: the band the fitted matrix covers)
            r.fmin = rb.fmin * (float)fam->sample_rate / (float)rb.L; r.fmax = rb.fmax * (float)fam->sample_rate / (float)rb.L;
            r.mag_scale = (float)std::log(1.0 / rb.expo - 1.0); r.out_scale = (float)rb.scale; r.out_shift = (float)rb.shift; r.flags = rb.flip;
            r.mel_w_off = blob.put(rb.mel_w);
            m.branches.push_back(r);
        }
    } else {
        // a graph that STARTS at the spectrogram holds no front-end to read: the family table states the published one
        m.h.norm_eps = fam->norm_eps; m.h.n_branches = fam->n_branches;
        m.h.spec_h = fam->br[0].n_mels; m.h.spec_w = fam->n_frames();
        for (uint32_t b = 0; b < fam->n_branches; b++) {
            const FamilyBranch &fb = fam->br[b];
            BranchRec r{};
            r.frame_length = fb.L; r.frame_step = fb.H; r.fft_length = fb.L; r.n_bins = fb.L / 2 + 1; r.n_mels = fb.n_mels;
            r.n_frames = (fam->sample_count - fb.L) / fb.H + 1;
            if (r.n_frames != m.h.spec_w) return fail("family table: branches with different frame counts");
            r.fmin = fb.fmin; r.fmax = fb.fmax; r.mag_scale = fb.mag_scale; r.out_scale = fb.out_scale; r.out_shift = fb.out_shift; r.flags = fb.flags;
            std::vector<float> w;
            mel_weight_matrix(fb.n_mels, r.n_bins, (double)fam->sample_rate, fb.fmin, fb.fmax, w);
            r.mel_w_off = blob.put(w);
            m.branches.push_back(r);
        }
    }

    // ---- multi-node activation spellings (convert.py _collapse_activations) ----
    struct Pattern { std::string out; uint32_t act; std::vector<size_t> nodes; };               // (nodes: the pattern's own, the readers it may have of its input)
    std::map<std::string, std::vector<Pattern>> first_of_pattern;                            // pattern input -> (pattern output, act)
    auto sole_consumer = [&](const std::string &name, const char *op, size_t &k) {
        auto it = cons.find(name);
        if (it == cons.end() || it->second.size() != 1 || nodes[it->second[0]].op != op) return false;
        k = it->second[0];
        return true;
    };
    // From a float32 tensor the constant is held to sqrt 2 at 1e-4.  From a float16 tensor it must BE the float16 rounding of the
    // expected value (sqrt 2 -> 1.4140625, 1 / sqrt 2 -> 0.70703125; no wider window), and the exact GELU runs: DESIGN section 5.
    const double SQRT2 = 1.4142135623730951;
    const float SQRT2_F16 = 1.4140625f, RSQRT2_F16 = 0.70703125f;
    // The hard sigmoid the kernels compute is PyTorch's, min(max(x / 6 + 1/2, 0), 1): alpha within 1e-6 of 1/6 and beta = 0.5.  (The
    // ONNX defaults, alpha = 0.2 and beta = 0.5, are Keras's hard sigmoid: another function, refused by name in the walk.)  The
    // decomposed spelling's 1/6 follows the rule above: held to 1e-6 from float32, the float16 rounding of 1/6 itself from float16.
    const float SIXTH_F16 = 0.1666259765625f;
    // a float32 / float16 scalar initializer, WITHOUT finit()'s note for the next refusal (init_refusal): the hard-swish chain below
    // probes the operands of every Add, and an int64 constant it passes over must not turn up in an unrelated message later
    auto probe_scalar = [&](const std::string &name, float &out, bool *from_f16 = nullptr) {
        auto it = g.init.find(name);
        if (it == g.init.end() || !it->second.is_float() || it->second.count != 1) return false;
        out = it->second.at(0);
        if (from_f16) *from_f16 = it->second.is_f16();
        return true;
    };
    auto hsig_is_torch = [](const Node &n) { return std::fabs((double)n.getf("alpha", 0.2f) - 1.0 / 6.0) <= 1e-6 && n.getf("beta", 0.5f) == 0.5f; };
    auto is_output = [&](const std::string &name) { return std::find(outputs.begin(), outputs.end(), name) != outputs.end(); };
    auto clip_is_relu6 = [&](const Node &n) {
        float lo = 0.f, hi = 0.f;
        const bool has_lo = n.in.size() > 1 && !n.in[1].empty() ? probe_scalar(n.in[1], lo) : (n.a.count("min") ? (lo = n.getf("min", 0.f), true) : false);
        const bool has_hi = n.in.size() > 2 && !n.in[2].empty() ? probe_scalar(n.in[2], hi) : (n.a.count("max") ? (hi = n.getf("max", 0.f), true) : false);
        return has_lo && has_hi && lo == 0.0f && hi == 6.0f;
    };
    for (size_t i = 0; i < nodes.size(); i++) {
        const Node &n = nodes[i];
        if (n.op == "Erf" && !n.in.empty() && !n.out.empty()) {
            auto pj = prod.find(n.in[0]);
            if (pj == prod.end()) continue;
            const size_t j = pj->second;
            const Node &pre = nodes[j];
            if ((pre.op != "Div" && pre.op != "Mul") || pre.in.size() != 2) continue;
            std::string x;
            for (int side = 0; side < 2; side++) {
                float c;
                bool c16 = false;
                if (!scalar(pre.in[side ? 0 : 1], c, &c16)) continue;
                const bool is_sqrt2 = c16 ? c == SQRT2_F16 : std::fabs((double)c - SQRT2) < 1e-4;
                const bool is_rsqrt2 = c16 ? c == RSQRT2_F16 : std::fabs((double)c - 1.0 / SQRT2) < 1e-4;
                if ((pre.op == "Div" && side == 0 && is_sqrt2) || (pre.op == "Mul" && is_rsqrt2))
                    x = pre.in[side ? 1 : 0];
            }
            size_t k, m1, m2;
            if (x.empty() || !sole_consumer(n.out[0], "Add", k)) continue;
            bool one = false;
            for (const auto &a : nodes[k].in) { float c; if (scalar(a, c) && std::fabs(c - 1.0f) < 1e-6f) one = true; }
            if (!one || nodes[k].out.empty() || !sole_consumer(nodes[k].out[0], "Mul", m1) || nodes[m1].out.empty() ||
                !sole_consumer(nodes[m1].out[0], "Mul", m2) || nodes[m2].out.empty()) continue;
            bool has_x = false, has_half = false;
            for (const auto &a : nodes[m1].in) if (a != nodes[k].out[0]) { float c; if (a == x) has_x = true; if (scalar(a, c) && std::fabs(c - 0.5f) < 1e-6f) has_half = true; }
            for (const auto &a : nodes[m2].in) if (a != nodes[m1].out[0]) { float c; if (a == x) has_x = true; if (scalar(a, c) && std::fabs(c - 0.5f) < 1e-6f) has_half = true; }
            if (has_x && has_half) {
                skip.insert({j, i, k, m1, m2});
                first_of_pattern[x].push_back(Pattern{nodes[m2].out[0], A_GELU_ERF, {j, i, k, m1, m2}});
            }
        } else if (n.op == "Sigmoid" && !n.in.empty() && !n.out.empty()) {
            size_t k;
            if (sole_consumer(n.out[0], "Mul", k)) {
                bool takes_x = false;
                for (const auto &a : nodes[k].in) if (a == n.in[0]) takes_x = true;
                if (takes_x && !nodes[k].out.empty()) {
                    skip.insert({i, k});
                    first_of_pattern[n.in[0]].push_back(Pattern{nodes[k].out[0], A_SWISH, {i, k}});
                }
            }
        } else if (n.op == "HardSigmoid" && !n.in.empty() && !n.out.empty() && !front.count(i) && hsig_is_torch(n)) {
            // HardSigmoid(x) * x, PyTorch's hard swish below opset 14: folded like Sigmoid * x.  (Without that Mul the node stays in the
            // walk: a squeeze-excite gate or a refusal; any other alpha / beta is refused there by name.)
            size_t k;
            if (sole_consumer(n.out[0], "Mul", k) && !is_output(n.out[0])) {
                bool takes_x = false;
                for (const auto &a : nodes[k].in) if (a == n.in[0]) takes_x = true;
                if (takes_x && !nodes[k].out.empty()) {
                    skip.insert({i, k});
                    first_of_pattern[n.in[0]].push_back(Pattern{nodes[k].out[0], A_HSWISH, {i, k}});
                }
            }
        } else if (n.op == "Add" && n.in.size() == 2 && !n.out.empty() && !skip.count(i) && !front.count(i)) {
            // The decomposed hard swish of tf2onnx and older exporters: Add(x, 3) -> Clip(0, 6) -> Mul(., x) and Mul(., 1/6) or
            // Div(., 6), the last two in either order; without the Mul(., x) it is the hard sigmoid (legal on a pooled tensor only:
            // set_act).  Every inner tensor has exactly one reader and is no graph output.  A chain that matches only in part is left
            // alone: its nodes meet the walk's own rules (Clip alone is ReLU6, a bare Add a residual).
            std::string x;
            for (int side = 0; side < 2; side++) {
                float c;
                if (probe_scalar(n.in[side], c) && c == 3.0f && g.init.find(n.in[1 - side]) == g.init.end()) x = n.in[1 - side];
            }
            size_t k;
            if (x.empty() || is_output(n.out[0]) || !sole_consumer(n.out[0], "Clip", k) || nodes[k].out.empty() || !clip_is_relu6(nodes[k])) continue;
            std::vector<size_t> own{i, k};
            std::string cur = nodes[k].out[0];
            bool has_scale = false, has_x = false;
            for (int step = 0; step < 2; step++) {
                auto it = cons.find(cur);
                if (is_output(cur) || it == cons.end() || it->second.size() != 1) break;
                const size_t q = it->second[0];
                const Node &nq = nodes[q];
                if ((nq.op != "Mul" && nq.op != "Div") || nq.in.size() != 2 || nq.out.empty() || skip.count(q)) break;
                const std::string &other = nq.in[0] == cur ? nq.in[1] : nq.in[0];
                float c;
                bool c16 = false;
                const bool is_const = probe_scalar(other, c, &c16);
                if (!has_scale && is_const && ((nq.op == "Mul" && (c16 ? c == SIXTH_F16 : std::fabs((double)c - 1.0 / 6.0) <= 1e-6)) ||
                                               (nq.op == "Div" && nq.in[0] == cur && c == 6.0f))) has_scale = true;
                else if (!has_x && nq.op == "Mul" && other == x) has_x = true;
                else break;
                own.push_back(q);
                cur = nq.out[0];
            }
            if (!has_scale) continue;
            for (size_t q : own) skip.insert(q);
            first_of_pattern[x].push_back(Pattern{cur, has_x ? A_HSWISH : A_HSIGMOID, own});
        }
    }

    // ---- the decomposed LayerNorm torch.onnx emits below opset 17 (convert.py _find_layer_norms): ReduceMean -> Sub -> Pow(2) ->
    // ReduceMean -> Add(eps) -> Sqrt -> Div -> Mul(gamma) -> Add(beta) over the last axis of an [N, H, W, C] view or axis 1 of an NCHW
    // map.  A ReduceMean over ONE axis (-1, 3 or 1) starts it; a chain that deviates is refused by naming the node where it does.
    struct LnChain { std::string out, gamma, beta, name; float eps; int64_t axis; };
    std::map<std::string, std::vector<LnChain>> ln_of_pattern;                               // chain input -> the chains
    // A ReduceMean over the last axis (-1, 3) with no Sub(x, mean) behind it is no chain: a reduction over W of an NCHW map (OP_REDUCE; the
    // walk).  On an [N, H, W, C] view it stays refused as the chain it is not -- node -> that refusal, raised by the walk.
    std::map<size_t, std::string> ln_deferred;
    {
        std::map<std::string, std::vector<size_t>> rd;                                       // readers outside the patterns found so far
        for (size_t i = 0; i < nodes.size(); i++)
            if (!skip.count(i))
                for (const auto &x : nodes[i].in) rd[x].push_back(i);
        const std::string chain = "ReduceMean -> Sub -> Pow(2) -> ReduceMean -> Add(eps) -> Sqrt -> Div -> Mul(gamma) -> Add(beta)";
        auto dev = [&](const Node &n, const std::string &why) { return fail(n.op + " '" + n.name + "': not the LayerNorm chain " + chain + ": " + why); };
        auto reduce_axes = [&](const Node &n, std::vector<int64_t> &axes) {
            axes.clear();
            if (const auto *ax = n.ints("axes")) { axes = *ax; return true; }
            if (n.in.size() > 1 && !n.in[1].empty()) { auto it = g.init.find(n.in[1]); if (it != g.init.end() && (it->second.dtype == 7 || it->second.dtype == 6) && it->second.il.size() <= 64) { axes = it->second.il; return true; } }
            return false;
        };
        // the one reader of src's output, which must be an `op` node -> k; false: refused (err is set)
        auto only_reader = [&](const Node &src, const char *op, size_t &k) {
            const std::string &name = src.out[0];
            auto it = rd.find(name);
            const size_t nr = it == rd.end() ? 0 : it->second.size();
            if (is_output(name) || nr != 1)
                return dev(src, "its output has " + std::to_string(nr) + " readers" + (is_output(name) ? " and is a graph output" : "") + " (a second reader of an inner tensor)");
            k = it->second[0];
            if (nodes[k].op != op || nodes[k].out.empty()) return dev(nodes[k], std::string(op) + " expected behind " + src.op + " '" + src.name + "'");
            return true;
        };
        auto other = [&](const Node &n, const std::string &name, std::string &o) {
            if (n.in.size() != 2 || (n.in[0] != name && n.in[1] != name)) return dev(n, "two operands expected");
            o = n.in[0] == name ? n.in[1] : n.in[0];
            return true;
        };
        for (size_t i = 0; i < nodes.size(); i++) {
            const Node &n = nodes[i];
            if (n.op != "ReduceMean" || skip.count(i) || front.count(i) || n.in.empty() || n.out.empty()) continue;
            std::vector<int64_t> axes, axes2;
            if (!reduce_axes(n, axes) || axes.size() != 1 || (axes[0] != -1 && axes[0] != 3 && axes[0] != 1)) continue;   // (H, W: the global pool; anything else keeps the walk's refusal)
            const std::string &x = n.in[0];
            size_t j_sub, j_pow, j_div, j_m2, j_add, j_sqrt, j_mul, j_add2, k;
            if (axes[0] != 1) {
                bool has_sub = false;
                auto rn = rd.find(n.out[0]);
                if (rn != rd.end())
                    for (size_t q : rn->second)
                        if (nodes[q].op == "Sub" && std::find(nodes[q].in.begin(), nodes[q].in.end(), x) != nodes[q].in.end()) has_sub = true;
                if (!has_sub) {
                    if (n.geti("keepdims", 1) != 1) dev(n, "keepdims = 0");
                    else if (only_reader(n, "Sub", j_sub)) dev(nodes[j_sub], "Sub(x, mean) expected");
                    ln_deferred[i] = err;
                    err.clear();
                    continue;
                }
            }
            if (n.geti("keepdims", 1) != 1) return dev(n, "keepdims = 0");
            if (!only_reader(n, "Sub", j_sub)) return false;
            const Node &sub = nodes[j_sub];
            if (sub.in.size() != 2 || sub.in[0] != x || sub.in[1] != n.out[0]) return dev(sub, "Sub(x, mean) expected");
            auto rs = rd.find(sub.out[0]);
            if (is_output(sub.out[0]) || rs == rd.end() || rs->second.size() != 2 ||
                !((nodes[rs->second[0]].op == "Pow" && nodes[rs->second[1]].op == "Div") || (nodes[rs->second[0]].op == "Div" && nodes[rs->second[1]].op == "Pow")))
                return dev(sub, "its output must be read by the Pow and the Div alone (a second reader of an inner tensor)");
            j_pow = nodes[rs->second[0]].op == "Pow" ? rs->second[0] : rs->second[1];
            j_div = nodes[rs->second[0]].op == "Pow" ? rs->second[1] : rs->second[0];
            const Node &pw = nodes[j_pow], &div = nodes[j_div];
            float two = 0.0f;
            if (pw.in.size() != 2 || pw.out.empty() || pw.in[0] != sub.out[0] || !probe_scalar(pw.in[1], two) || two != 2.0f) return dev(pw, "an exponent other than 2");
            if (!only_reader(pw, "ReduceMean", j_m2)) return false;
            const Node &m2 = nodes[j_m2];
            if (!reduce_axes(m2, axes2) || axes2 != axes || m2.geti("keepdims", 1) != 1) return dev(m2, "not over the first mean's axis " + std::to_string(axes[0]) + " (another axis)");
            { auto c = rd.find(m2.out[0]); if (c != rd.end() && c->second.size() == 1 && nodes[c->second[0]].op == "Sqrt") return dev(nodes[c->second[0]], "a missing eps (Add(variance, eps) expected in front of the Sqrt)"); }
            if (!only_reader(m2, "Add", j_add)) return false;
            const Node &add = nodes[j_add];
            std::string eps_name, gamma, beta;
            float eps = 0.0f;
            if (!other(add, m2.out[0], eps_name)) return false;
            if (!probe_scalar(eps_name, eps)) return dev(add, "a missing eps (a float32 or float16 scalar constant expected)");
            if (!only_reader(add, "Sqrt", j_sqrt)) return false;
            const Node &sq = nodes[j_sqrt];
            if (!only_reader(sq, "Div", k)) return false;
            if (k != j_div || div.in.size() != 2 || div.out.empty() || div.in[0] != sub.out[0] || div.in[1] != sq.out[0]) return dev(div, "Div(x - mean, sqrt) expected");
            if (!only_reader(div, "Mul", j_mul)) return false;
            const Node &mul = nodes[j_mul];
            if (!other(mul, div.out[0], gamma)) return false;
            if (!only_reader(mul, "Add", j_add2)) return false;
            const Node &add2 = nodes[j_add2];
            if (!other(add2, mul.out[0], beta)) return false;
            { auto it = g.init.find(gamma); if (it == g.init.end() || !it->second.is_float()) return dev(mul, "gamma must be a float32 or float16 initializer"); }
            { auto it = g.init.find(beta); if (it == g.init.end() || !it->second.is_float()) return dev(add2, "beta must be a float32 or float16 initializer"); }
            for (size_t q : {i, j_sub, j_pow, j_m2, j_add, j_sqrt, j_div, j_mul, j_add2}) skip.insert(q);
            ln_of_pattern[x].push_back(LnChain{add2.out[0], gamma, beta, n.name, eps, axes[0]});
        }
    }

    // ---- the walk (convert.py model_from_graph) ----
    // tensor index, channels, height, width (1 x 1 once pooled).  view: the output of a Split / Slice that only Concat nodes read --
    // channels off .. off + c - 1 of tensor idx, folded into those records' windows; no other node ever looks one up
    // nhwc: the name is an [N, H, W, C] view of its tensor (behind Transpose [0, 2, 3, 1]) -- the library keeps activations NHWC, so the
    // view costs nothing; only LayerNormalization, MatMul, the activations, Mul by a [C] constant and the Transpose back read one
    // r3: the name is a rank-3 tensor behind a reduction with keepdims = 0 -- 1: [N, C, H] (W is gone), 2: [N, C, W] (H is gone)
    struct T { uint32_t idx, c, h, w, off = 0; bool view = false; bool nhwc = false; uint32_t r3 = 0; };
    std::map<std::string, T> tmap;
    tmap[spec] = T{0, m.h.n_branches, m.h.spec_h, m.h.spec_w};
    std::vector<LayerRec> &layers = m.layers;
    uint32_t out_act = O_NONE, emb_tensor = 0, emb_dim = 0;
    std::set<std::string> graph_out;
    for (const auto &o : outputs) graph_out.insert(o);
    auto find = [&](const std::string &name, T &t) { auto it = tmap.find(name); if (it == tmap.end()) return false; t = it->second; return true; };
    std::set<std::string> sums;   // the outputs of the residual Adds folded into a layer
    std::vector<std::pair<std::vector<T>, T>> cat_lists;   // (the resolved input list of a Concat, its output tensor), in graph order: prefix reuse
    // ---- the channel shuffle (convert.py _find_shuffles): Reshape [N, g, C / g, H, W] -> Transpose (0, 2, 1, 3, 4) -> Reshape
    // [N, C, H, W], each with one reader, the shapes constants.  Found here, where the activation spellings are; the walk makes an
    // OP_CONCAT record (or the `reserved` word of the Concat in front) of the first Reshape and skips the other two nodes.
    auto const_ints = [&](const std::string &name) -> const std::vector<int64_t> * {
        auto it = g.init.find(name);
        return it != g.init.end() && (it->second.dtype == 7 || it->second.dtype == 6) && it->second.il.size() <= 64 ? &it->second.il : nullptr;
    };
    struct Shuffle { std::string out; std::vector<int64_t> s1, s2; };
    std::map<size_t, Shuffle> shuffle_at;          // the first Reshape's node -> the pattern
    std::set<size_t> shuffle_computed;             // ... whose shapes are not constants: refused by name at the walk
    for (size_t i = 0; i < nodes.size(); i++) {
        const Node &n = nodes[i];
        size_t t, r2;
        if (n.op != "Reshape" || skip.count(i) || front.count(i) || n.in.size() < 2 || n.out.empty() || !sole_consumer(n.out[0], "Transpose", t) ||
            nodes[t].out.empty() || skip.count(t)) continue;
        const auto *perm = nodes[t].ints("perm");
        if (!perm || *perm != std::vector<int64_t>{0, 2, 1, 3, 4}) continue;
        if (!sole_consumer(nodes[t].out[0], "Reshape", r2) || nodes[r2].in.size() < 2 || nodes[r2].out.empty() || skip.count(r2)) continue;
        const auto *s1 = const_ints(n.in[1]), *s2 = const_ints(nodes[r2].in[1]);
        if (!s1 || !s2) { shuffle_computed.insert(i); continue; }
        shuffle_at[i] = Shuffle{nodes[r2].out[0], *s1, *s2};
        skip.insert(t); skip.insert(r2);
    }
    // a Reshape's target with its 0 (copy the input's dimension) and -1 (whatever is left) entries resolved, the batch dimension
    // aside: `in` and the result hold the dimensions behind it.  false: not a shape of `total` elements.
    auto resolve_shape = [](const std::vector<int64_t> &shape, const std::vector<int64_t> &in, int64_t total, std::vector<int64_t> &out) {
        out.clear();
        int64_t known = 1;
        int infer = -1;
        for (size_t k = 1; k < shape.size(); k++) {
            int64_t v = shape[k];
            if (v == 0) { if (k - 1 >= in.size()) return false; v = in[k - 1]; }
            if (v == -1) { if (infer >= 0 || shape[0] == -1) return false; infer = (int)out.size(); v = 1; }
            else if (v <= 0 || v > (1 << 24) || known > (1ll << 40)) return false;
            else known *= v;
            out.push_back(v);
        }
        if (infer >= 0) { if (total % known) return false; out[(size_t)infer] = total / known; known = total; }
        return known == total;
    };
    // one OP_CONCAT record: the window of a (and of b behind it), shuffled in g groups
    const std::string quad = "a channel count or offset that is not a multiple of 4 is not supported (ShuffleNetV2 x1.0's 58-channel halves, for one)";
    auto has_other_reader = [&](const std::string &name) {     // than Concat nodes
        if (graph_out.count(name)) return true;
        auto it = cons.find(name);
        if (it != cons.end()) for (size_t k : it->second) if (nodes[k].op != "Concat") return true;
        return false;
    };
    // tensor of a norm + activation record (OP_BNACT) that has no activation yet -> the refusal its BatchNormalization gets without one
    std::map<uint32_t, std::string> bn_pending;
    // (own: the nodes of the activation itself -- one, or a multi-node spelling's)
    auto set_act = [&](const std::string &name_in, const std::string &name_out, uint32_t act, const std::vector<size_t> &own) {
        T t;
        if (!find(name_in, t)) return fail("activation on unknown tensor '" + name_in + "'");
        if (t.idx != 0 && layers[t.idx - 1].op == OP_BNACT) {
            // the activation that completes a tentative norm + activation record (the BatchNormalization branch below); anything but one of
            // the record's activations as the ONLY reader of the norm's output leaves the norm where it was: refused, in the words stored
            auto pit = bn_pending.find(t.idx);
            if (pit == bn_pending.end()) return fail("activation after '" + name_in + "' cannot be folded into its producer");
            bool other = graph_out.count(name_in) != 0;
            auto cit = cons.find(name_in);
            if (cit != cons.end()) for (size_t k : cit->second) if (std::find(own.begin(), own.end(), k) == own.end()) other = true;
            if (other || !(act == A_RELU || act == A_RELU6 || act == A_SWISH || act == A_GELU_ERF || act == A_GELU_TANH || act == A_HSWISH)) return fail(pit->second);
            bn_pending.erase(pit);
            layers[t.idx - 1].act = act;
            tmap[name_out] = t;
            return true;
        }
        // (the hard sigmoid stands where the Sigmoid inside the graph may: on a pooled [N, C, 1, 1] tensor -- the gate's second 1x1, a dense layer)
        if (act == A_HSIGMOID && (uint64_t)t.h * t.w != 1) return fail("HardSigmoid inside the graph that is neither HardSigmoid * x nor a squeeze-excite gate");
        if (t.idx != 0 && layers[t.idx - 1].op == OP_POOL)
            return fail("activation after '" + name_in + "' cannot be folded into its producer: directly after a MaxPool / AveragePool (a pool layer carries no activation)");
        if (t.idx != 0 && layers[t.idx - 1].op == OP_CONCAT)
            return fail("activation after '" + name_in + "' cannot be folded into its producer: directly after a Concat, Split, Slice or channel shuffle (the record carries no activation)");
        if (t.idx != 0 && layers[t.idx - 1].op == OP_LNORM)
            return fail("activation after '" + name_in + "' cannot be folded into its producer: directly after a LayerNormalization (the record carries no activation)");
        if (t.idx != 0 && layers[t.idx - 1].op == OP_REDUCE)
            return fail("activation after '" + name_in + "' cannot be folded into its producer: directly after a ReduceMax / ReduceMean / GlobalMaxPool (a reduce layer carries no activation)");
        if (t.idx != 0 && sums.count(name_in) && layers[t.idx - 1].res_tensor != NO_TENSOR && layers[t.idx - 1].reserved != RES_ACT_AFTER) {
            // act(conv + x), the end of a ResNet block: the layer keeps its one activation code and records its position
            LayerRec &L = layers[t.idx - 1];
            if (L.act != A_NONE)
                return fail("activation after '" + name_in + "' cannot be folded into its producer: an activation on both sides of a residual Add (act2(act1(conv) + x))");
            bool other = graph_out.count(name_in) != 0;
            auto cit = cons.find(name_in);
            if (cit != cons.end()) for (size_t k : cit->second) if (std::find(own.begin(), own.end(), k) == own.end()) other = true;
            if (other)
                return fail("activation after '" + name_in + "' cannot be folded into its producer: the sum has another reader or is a graph output (it would be handed the activated tensor)");
            L.act = act;
            L.reserved = RES_ACT_AFTER;
            tmap[name_out] = t;
            return true;
        }
        if (t.idx == 0 || layers[t.idx - 1].act != A_NONE || layers[t.idx - 1].res_tensor != NO_TENSOR)
            return fail("activation after '" + name_in + "' cannot be folded into its producer");
        layers[t.idx - 1].act = act;
        tmap[name_out] = t;
        return true;
    };
    std::function<bool(const std::string &)> flush_ln;     // (the decomposed LayerNorm chains that start at a tensor: below, behind new_layer)
    auto flush_patterns = [&](const std::string &x) {
        auto it = first_of_pattern.find(x);
        if (it != first_of_pattern.end()) {
            const auto list = it->second;
            first_of_pattern.erase(it);
            for (const auto &pa : list)
                if (!set_act(x, pa.out, pa.act, pa.nodes)) return false;
        }
        return flush_ln(x);
    };
    auto new_layer = [&](uint32_t op, uint32_t in_t, uint32_t res_t, uint32_t cin, uint32_t cout, uint32_t kh, uint32_t kw, uint32_t sh, uint32_t sw,
                         uint32_t pt, uint32_t pl, uint32_t ih, uint32_t iw, uint32_t oh, uint32_t ow, uint32_t in_layout, uint64_t w_off, uint64_t b_off) {
        LayerRec L{};
        L.op = op; L.act = A_NONE; L.in_tensor = in_t; L.res_tensor = res_t; L.cin = cin; L.cout = cout; L.kh = kh; L.kw = kw; L.sh = sh; L.sw = sw;
        L.pad_t = pt; L.pad_l = pl; L.in_h = ih; L.in_w = iw; L.out_h = oh; L.out_w = ow; L.in_layout = in_layout; L.w_off = w_off; L.b_off = b_off;
        layers.push_back(L);
        return (uint32_t)layers.size();
    };
    constexpr int64_t DIM_MAX = 1 << 16;
    std::vector<float> tmp, tmpb;
    // one OP_LNORM record over the channels of x (an [N, H, W, C] view, or an NCHW map the caller has held to the channel axis) -> `out`,
    // a view when x is one; directly behind the global pool it becomes the embedding (pool -> norm -> dense: the dense head reads the norm)
    auto lnorm_rec = [&](const std::string &who, const T &x, const std::string &out, const Tensor *gamma, const Tensor *beta, float eps) {
        if (x.idx == 0) return fail(who + "a LayerNorm of the spectrogram (tensor 0) is not supported");
        if (!gamma || !gamma->is_float() || gamma->count != x.c || (beta && (!beta->is_float() || beta->count != x.c)))
            return fail(who + "gamma / beta must be float32 or float16 initializers of the " + std::to_string(x.c) + " channels");
        if (x.c % 4) return fail(who + std::to_string(x.c) + " channels: a channel count that is not a multiple of 4 is not supported");
        if (!std::isfinite(eps) || !(eps > 0.0f)) { char v[48]; snprintf(v, sizeof v, "%g", (double)eps); return fail(who + "epsilon " + v + " is not finite and > 0"); }
        tmp.resize(x.c); tmpb.assign(x.c, 0.0f);
        for (uint32_t c = 0; c < x.c; c++) { tmp[c] = gamma->at(c); if (beta) tmpb[c] = beta->at(c); }
        const uint64_t wo = blob.put(tmp), bo = blob.put(tmpb);
        const uint32_t li = new_layer(OP_LNORM, x.idx, NO_TENSOR, x.c, x.c, 1, 1, 1, 1, 0, 0, x.h, x.w, x.h, x.w, 0, wo, bo);
        memcpy(&layers[li - 1].reserved, &eps, sizeof eps);
        if ((layers[x.idx - 1].op == OP_GAP || layers[x.idx - 1].op == OP_REDUCE) && emb_tensor == x.idx) emb_tensor = li;
        T y{li, x.c, x.h, x.w};
        y.nhwc = x.nhwc;
        tmap[out] = y;
        return true;
    };
    flush_ln = [&](const std::string &x) {
        auto it = ln_of_pattern.find(x);
        if (it == ln_of_pattern.end()) return true;
        const auto list = it->second;
        ln_of_pattern.erase(it);
        for (const auto &ch : list) {
            const std::string who = "ReduceMean '" + ch.name + "' (LayerNorm chain): ";
            T t;
            if (!find(x, t)) return fail(who + "input not on the path");
            const Tensor &ga = g.init.find(ch.gamma)->second, &be = g.init.find(ch.beta)->second;
            auto shaped = [&](const Tensor &a) {
                const int64_t C = t.c;
                if (t.nhwc) return a.dims == std::vector<int64_t>{C};
                return a.dims == std::vector<int64_t>{C, 1, 1} || a.dims == std::vector<int64_t>{1, C, 1, 1};
            };
            if (t.nhwc && ch.axis != -1 && ch.axis != 3)
                return fail(who + "axis " + std::to_string(ch.axis) + " of an [N, H, W, C] view: only the last axis, the channels, is normalised (another axis)");
            if (!t.nhwc && ch.axis != 1)
                return fail(who + "axis " + std::to_string(ch.axis) + " of an NCHW tensor: only axis 1, the channels, is normalised (another axis)");
            if (!shaped(ga) || !shaped(be)) return fail(who + "gamma / beta do not have the shape that scales the " + std::to_string(t.c) + " channels");
            if (!lnorm_rec(who, t, ch.out, &ga, &be, ch.eps) || !flush_patterns(ch.out)) return false;
        }
        return true;
    };
    // the layer scale of a ConvNeXt block (convert.py fold_layer_scale): Mul of a convolution's / MatMul layer's output by a constant of its
    // C channels ([C] on an [N, H, W, C] view, [C, 1, 1] or [1, C, 1, 1] on an NCHW map), folded into the layer's weight columns and bias
    // where BatchNormalization is -- one float32 product each.  The layer has no activation and no residual yet, the Mul is its only
    // reader and the tensor no graph output.  folded = false: not that Mul (today's rules apply).  (Every record's weights are a
    // slot of their own in this blob -- both readers put them per node --, so the fold never touches another layer's.)
    auto fold_layer_scale = [&](const Node &n, bool &folded) {
        folded = false;
        if (n.in.size() != 2 || n.out.empty()) return true;
        for (int side = 0; side < 2; side++) {
            const std::string &xn = n.in[side], &sn = n.in[1 - side];
            auto it = g.init.find(sn);
            T t;
            if (it == g.init.end() || !it->second.is_float() || !find(xn, t) || t.idx == 0) continue;
            const Tensor &S = it->second;
            LayerRec &L = layers[t.idx - 1];
            const int64_t C = t.c;
            const bool shape_ok = t.nhwc ? S.dims == std::vector<int64_t>{C} : (S.dims == std::vector<int64_t>{C, 1, 1} || S.dims == std::vector<int64_t>{1, C, 1, 1});
            auto cit = cons.find(xn);
            if (!shape_ok || (L.op != OP_CONV && L.op != OP_DWCONV && L.op != OP_PWCONV && L.op != OP_GCONV) || L.act != A_NONE || L.res_tensor != NO_TENSOR ||
                graph_out.count(xn) || cit == cons.end() || cit->second.size() != 1) continue;
            const uint64_t nw = L.op == OP_CONV ? (uint64_t)L.kh * L.kw * L.cin * L.cout : L.op == OP_GCONV ? (uint64_t)L.kh * L.kw * (L.cin / L.reserved) * L.cout : L.op == OP_DWCONV ? (uint64_t)L.kh * L.kw * L.cout : (uint64_t)L.cin * L.cout;
            for (uint32_t c = 0; c < L.cout; c++) {
                const float sf = S.at(c);
                for (uint64_t q = c; q < nw; q += L.cout) blob.v[L.w_off + q] = blob.v[L.w_off + q] * sf;    // (cout is the last axis in every layout)
                blob.v[L.b_off + c] = blob.v[L.b_off + c] * sf;
            }
            tmap[n.out[0]] = t;
            folded = true;
            return flush_patterns(n.out[0]);
        }
        for (const auto &xn : n.in) {
            T t;
            if (find(xn, t) && t.nhwc)
                return fail("Mul '" + n.name + "': input '" + xn + "' is an [N, H, W, C] view (behind a Transpose): only a Mul by a [C] constant directly behind a MatMul layer without an activation, its only reader, is folded (layer scale)");
        }
        return true;
    };
    // one OP_CONCAT record: the window of a, then that of b (null: a alone), shuffled in g groups (0: not); -> its output, whole
    auto concat_rec = [&](const T &a, const T *b, uint32_t g) {
        const uint32_t cout = a.c + (b ? b->c : 0);
        const uint32_t li = new_layer(OP_CONCAT, a.idx, b ? b->idx : NO_TENSOR, a.c, cout, 1, 1, 1, 1, 0, 0, a.h, a.w, a.h, a.w, 0, a.off, b ? b->off : 0);
        layers[li - 1].reserved = g;
        return T{li, cout, a.h, a.w};
    };
    // the outputs of a Split / Slice: a view where only Concat nodes read it, else a record of its own that materialises it
    auto publish_view = [&](const std::string &name, const T &x, uint32_t off, uint32_t c) {
        T v{x.idx, c, x.h, x.w, x.off + off, true};
        tmap[name] = has_other_reader(name) ? concat_rec(v, nullptr, 0) : v;
    };
    for (size_t i = 0; i < nodes.size(); i++) {
        if (skip.count(i) || front.count(i)) continue;
        const Node &n = nodes[i];
        const std::string &op = n.op;
        if (n.out.empty() || n.in.empty()) return fail("node '" + n.name + "' (" + op + ") without inputs or outputs");
        if (layers.size() > 4000) return fail("more than 4 000 layers");
        // an [N, H, W, C] view among the inputs: only these operators read one
        const std::string *view_in = nullptr;
        for (const auto &xn : n.in) { T t; if (!view_in && find(xn, t) && t.nhwc) view_in = &xn; }
        if (view_in) { auto d = ln_deferred.find(i); if (d != ln_deferred.end()) return fail(d->second); }
        if (view_in && op != "Transpose" && op != "LayerNormalization" && op != "MatMul" && op != "Mul" && op != "Relu" && op != "Gelu" && op != "Clip" && op != "HardSwish")
            return fail(op + " '" + n.name + "': input '" + *view_in + "' is an [N, H, W, C] view (behind a Transpose): only LayerNormalization, MatMul (+ Add of a bias), "
                        "the activations, Mul by a [C] constant and the Transpose back read one");
        // a rank-3 tensor [N, C, T] among the inputs (behind a reduction with keepdims = 0): only these operators read one
        for (const auto &xn : n.in) {
            T t;
            if (find(xn, t) && t.r3 && op != "ReduceMean" && op != "ReduceMax" && op != "Add" && op != "Squeeze" && op != "Unsqueeze" && op != "Flatten" && op != "Reshape")
                return fail(op + " '" + n.name + "': input '" + xn + "' is a rank-3 tensor [N, C, T] (behind a reduction with keepdims = 0): only further reductions, the max + mean "
                            "Add, and Squeeze / Unsqueeze / Flatten / Reshape once one pixel is left read one (1-D convolutions and pools are not supported)");
        }
        // a norm + activation record without its activation yet among the inputs: only an activation reads one (set_act completes it)
        if (!bn_pending.empty())
            for (const auto &xn : n.in) {
                T t;
                if (!find(xn, t)) continue;
                auto pit = bn_pending.find(t.idx);
                if (pit == bn_pending.end()) continue;
                bool relu6 = false;
                if (op == "Clip") {
                    float lo = 0.f, hi = 0.f;
                    const bool has_lo = n.in.size() > 1 && !n.in[1].empty() ? scalar(n.in[1], lo) : (n.a.count("min") ? (lo = n.getf("min", 0.f), true) : false);
                    const bool has_hi = n.in.size() > 2 && !n.in[2].empty() ? scalar(n.in[2], hi) : (n.a.count("max") ? (hi = n.getf("max", 0.f), true) : false);
                    relu6 = has_lo && has_hi && lo == 0.0f && hi == 6.0f;
                }
                if (!(op == "Relu" || op == "Gelu" || op == "HardSwish" || relu6)) return fail(pit->second);
            }
        bool folded = false;
        if (op == "Mul" && !fold_layer_scale(n, folded)) return false;
        if (folded) continue;
        if (op == "Transpose") {
            // the library keeps activations NHWC: [0, 2, 3, 1] marks the result an [N, H, W, C] view of the same tensor, [0, 3, 1, 2] ends it
            const std::string who = "Transpose '" + n.name + "': ";
            T t;
            if (!find(n.in[0], t)) return fail(who + "input '" + n.in[0] + "' is not on the path from '" + spec + "'");
            std::vector<int64_t> perm;
            if (const auto *pp = n.ints("perm")) perm = *pp;
            if (perm == std::vector<int64_t>{0, 2, 3, 1} && !view_in) {
                if (t.idx == 0) return fail(who + "an [N, H, W, C] view of the spectrogram (tensor 0) is not supported");
                if (t.view) return fail(who + "an [N, H, W, C] view of a Split / Slice output that only Concat nodes read is not supported");
                t.nhwc = true;
            } else if (perm == std::vector<int64_t>{0, 3, 1, 2} && view_in) {
                t.nhwc = false;
            } else {
                std::string ps;
                for (size_t q = 0; q < perm.size() && q < 8; q++) ps += (q ? ", " : "") + std::to_string(perm[q]);
                return fail(who + "perm [" + ps + "] on " + (view_in ? "an [N, H, W, C] view" : "an NCHW feature map") + ": only [0, 2, 3, 1] on a feature map and [0, 3, 1, 2] on the view it makes are read");
            }
            tmap[n.out[0]] = t;
            if (!flush_patterns(n.out[0])) return false;
        } else if (op == "LayerNormalization") {
            const std::string who = "LayerNormalization '" + n.name + "': ";
            T t;
            if (!find(n.in[0], t)) return fail(who + "input '" + n.in[0] + "' is not on the path from '" + spec + "'");
            const int64_t axis = n.geti("axis", -1);
            if (view_in) {
                if (axis != -1 && axis != 3) return fail(who + "axis " + std::to_string(axis) + " of an [N, H, W, C] view: only the last axis, the channels, is normalised");
            } else if (axis != 1 || (uint64_t)t.h * t.w != 1) {
                return fail(who + "axis " + std::to_string(axis) + " of an NCHW tensor with a " + std::to_string(t.h) + "x" + std::to_string(t.w) + " image: it would normalise over more than the "
                            "channels (only axis 1 of an [N, C, 1, 1] tensor, or the last axis of an [N, H, W, C] view)");
            }
            for (size_t k = 1; k <= 2; k++)
                if (n.out.size() > k && !n.out[k].empty() && (graph_out.count(n.out[k]) || cons.count(n.out[k])))
                    return fail(who + "the output " + (k == 1 ? "Mean" : "InvStdDev") + " is read: only the normalised tensor is computed");
            init_refusal.clear();
            const Tensor *ga = n.in.size() > 1 ? finit(n.in[1]) : nullptr;
            const bool has_beta = n.in.size() > 2 && !n.in[2].empty();
            const Tensor *be = has_beta ? finit(n.in[2]) : nullptr;
            if (!ga || (has_beta && !be)) return fail(who + "gamma / beta must be float32 or float16 initializers of the " + std::to_string(t.c) + " channels" + init_refusal);
            if (!lnorm_rec(who, t, n.out[0], ga, be, n.getf("epsilon", 1e-5f)) || !flush_patterns(n.out[0])) return false;
        } else if (op == "MatMul" && view_in) {
            // a pointwise layer on the [N, H, W, C] view (a PyTorch Linear between two Transposes), with its Add of a bias
            const std::string who = "MatMul '" + n.name + "': ";
            if (*view_in != n.in[0]) return fail(who + "the [N, H, W, C] view '" + *view_in + "' as the second operand");
            T t;
            find(n.in[0], t);
            init_refusal.clear();
            const Tensor *W = n.in.size() > 1 ? finit(n.in[1]) : nullptr;
            if (!W || W->dims.size() != 2) return fail(who + "needs a 2-d float32 or float16 weight initializer" + init_refusal);
            const int64_t cin = W->dims[0], cout = W->dims[1];
            if (cin <= 0 || cout <= 0 || cin > DIM_MAX || cout > DIM_MAX) return fail(who + "bad weight shape");
            if ((uint64_t)cin != t.c) return fail(who + std::to_string(cin) + " input features, activation has " + std::to_string(t.c));
            const Tensor *B = nullptr;
            std::string out = n.out[0];
            size_t k;
            if (sole_consumer(out, "Add", k) && nodes[k].in.size() == 2 && !nodes[k].out.empty() && !graph_out.count(out)) {
                const std::string &o2 = nodes[k].in[0] == out ? nodes[k].in[1] : nodes[k].in[0];
                auto it = g.init.find(o2);
                if (it != g.init.end() && it->second.is_float() && it->second.count == (uint64_t)cout) { B = &it->second; out = nodes[k].out[0]; skip.insert(k); }
            }
            tmp.resize((size_t)cin * cout);
            for (size_t q = 0; q < tmp.size(); q++) tmp[q] = W->at(q);
            tmpb.assign((size_t)cout, 0.0f);
            if (B) for (int64_t o = 0; o < cout; o++) tmpb[(size_t)o] = B->at((uint64_t)o);
            const uint64_t wo = blob.put(tmp), bo = blob.put(tmpb);
            const uint32_t li = new_layer(OP_PWCONV, t.idx, NO_TENSOR, (uint32_t)cin, (uint32_t)cout, 1, 1, 1, 1, 0, 0, t.h, t.w, t.h, t.w, 0, wo, bo);
            T y{li, (uint32_t)cout, t.h, t.w};
            y.nhwc = true;
            tmap[out] = y;
            if (!flush_patterns(out)) return false;
        } else if (op == "Conv") {
            T x;
            if (!find(n.in[0], x)) return fail("Conv '" + n.name + "': input '" + n.in[0] + "' is not on the path from '" + spec + "'");
            init_refusal.clear();
            const Tensor *W = n.in.size() > 1 ? finit(n.in[1]) : nullptr;
            if (!W || W->dims.size() != 4) return fail("Conv '" + n.name + "': weights must be a 4-d float32 or float16 initializer" + init_refusal);
            const int64_t cout = W->dims[0], cin_g = W->dims[1], kh = W->dims[2], kw = W->dims[3], group = n.geti("group", 1);
            if (cout <= 0 || cin_g <= 0 || kh <= 0 || kw <= 0 || group <= 0 || cout > DIM_MAX || cin_g > DIM_MAX || kh > 64 || kw > 64 || group > DIM_MAX)
                return fail("Conv '" + n.name + "': bad weight shape");
            const Tensor *B = n.in.size() > 2 && !n.in[2].empty() ? finit(n.in[2]) : nullptr;
            if (n.in.size() > 2 && !n.in[2].empty() && (!B || B->count != (uint64_t)cout)) return fail("Conv '" + n.name + "': bias must be a float32 or float16 initializer of the output width" + init_refusal);
            int64_t sh = 1, sw = 1;
            if (const auto *st = n.ints("strides")) { if (st->size() != 2) return fail("Conv '" + n.name + "': strides"); sh = (*st)[0]; sw = (*st)[1]; }
            if (sh <= 0 || sw <= 0 || sh > 16 || sw > 16) return fail("Conv '" + n.name + "': strides");
            const int64_t h = x.h, w = x.w, cin = x.c;
            // dilation (convert.py has the same branch, refusal for refusal): a group-1 convolution of an NHWC activation or a depthwise
            // one, 1 .. 16 per axis; an axis with one tap is dilation 1 whatever the file says (one spelling of the record)
            int64_t dh = 1, dw = 1;
            if (const auto *dl = n.ints("dilations")) {
                bool any = false;
                for (int64_t d : *dl) any = any || d != 1;
                if (any && dl->size() != 2) return fail("Conv '" + n.name + "': dilations must be two values");
                if (any) { dh = (*dl)[0]; dw = (*dl)[1]; }
            }
            if (dh < 1 || dw < 1 || dh > 16 || dw > 16)
                return fail("Conv '" + n.name + "': dilation " + std::to_string(dh) + "x" + std::to_string(dw) + " (1 .. 16 are supported)");
            if (kh == 1) dh = 1;
            if (kw == 1) dw = 1;
            if (dh != 1 || dw != 1) {
                if (x.idx == 0) return fail("Conv '" + n.name + "': dilation on the stem convolution (the spectrogram, tensor 0) is not supported");
                if (group != 1 && !(group == cin && cin_g == 1 && cout == cin))
                    return fail("Conv '" + n.name + "': dilation on a grouped convolution is not supported");
            }
            const int64_t ekh = (kh - 1) * dh + 1, ekw = (kw - 1) * dw + 1;   // the window's extent over the image
            int64_t oh = (h + sh - 1) / sh, ow = (w + sw - 1) / sw, pt = 0, pl = 0;
            const std::string autop = n.gets("auto_pad", "NOTSET");
            if (autop == "SAME_UPPER" || autop == "SAME_LOWER") {
                const int64_t th = std::max<int64_t>((oh - 1) * sh + ekh - h, 0), tw = std::max<int64_t>((ow - 1) * sw + ekw - w, 0);
                if (autop == "SAME_UPPER") { pt = th / 2; pl = tw / 2; } else { pt = th - th / 2; pl = tw - tw / 2; }
            } else {
                int64_t pads[4] = {0, 0, 0, 0};
                if (const auto *pd = n.ints("pads")) { if (pd->size() != 4) return fail("Conv '" + n.name + "': pads"); for (int q = 0; q < 4; q++) pads[q] = (*pd)[q]; }
                for (int64_t p : pads) if (p < 0 || p > 64) return fail("Conv '" + n.name + "': pads");
                pt = pads[0]; pl = pads[1];
                if (h + pads[0] + pads[2] < ekh || w + pads[1] + pads[3] < ekw) return fail("Conv '" + n.name + "': kernel larger than the padded input");
                oh = (h + pads[0] + pads[2] - ekh) / sh + 1; ow = (w + pads[1] + pads[3] - ekw) / sw + 1;
            }
            tmpb.assign((size_t)cout, 0.0f);
            if (B) for (int64_t o = 0; o < cout; o++) tmpb[(size_t)o] = B->at((uint64_t)o);
            uint32_t li;
            if (group == 1 && kh == 1 && kw == 1 && sh == 1 && sw == 1) {
                if (cin_g != cin) return fail("Conv '" + n.name + "': " + std::to_string(cin_g) + " input channels, activation has " + std::to_string(cin));
                tmp.resize((size_t)cin * cout);                                   // W[cout][cin][1][1] -> [cin][cout]
                for (int64_t o = 0; o < cout; o++)
                    for (int64_t c = 0; c < cin; c++) tmp[(size_t)c * cout + o] = W->at((uint64_t)(o * cin + c));
                const uint64_t wo = blob.put(tmp), bo = blob.put(tmpb);
                li = new_layer(OP_PWCONV, x.idx, NO_TENSOR, (uint32_t)cin, (uint32_t)cout, 1, 1, 1, 1, 0, 0, (uint32_t)h, (uint32_t)w, (uint32_t)h, (uint32_t)w, 0, wo, bo);
            } else if (group == cin && cin_g == 1 && cout == cin) {
                tmp.resize((size_t)kh * kw * cout);                               // W[c][1][kh][kw] -> [kh][kw][c]
                for (int64_t c = 0; c < cout; c++)
                    for (int64_t y = 0; y < kh; y++)
                        for (int64_t z = 0; z < kw; z++) tmp[(size_t)((y * kw + z) * cout + c)] = W->at((uint64_t)((c * kh + y) * kw + z));
                const uint64_t wo = blob.put(tmp), bo = blob.put(tmpb);
                li = new_layer(OP_DWCONV, x.idx, NO_TENSOR, (uint32_t)cin, (uint32_t)cout, (uint32_t)kh, (uint32_t)kw, (uint32_t)sh, (uint32_t)sw, (uint32_t)pt, (uint32_t)pl,
                               (uint32_t)h, (uint32_t)w, (uint32_t)oh, (uint32_t)ow, 0, wo, bo);
                layers[li - 1].skip_h = (uint32_t)(dh - 1); layers[li - 1].skip_w = (uint32_t)(dw - 1);
            } else if (group == 1) {
                if (cin_g != cin) return fail("Conv '" + n.name + "': " + std::to_string(cin_g) + " input channels, activation has " + std::to_string(cin));
                tmp.resize((size_t)kh * kw * cin * cout);                         // W[cout][cin][kh][kw] -> [kh][kw][cin][cout]
                for (int64_t o = 0; o < cout; o++)
                    for (int64_t c = 0; c < cin; c++)
                        for (int64_t y = 0; y < kh; y++)
                            for (int64_t z = 0; z < kw; z++)
                                tmp[(size_t)(((y * kw + z) * cin + c) * cout + o)] = W->at((uint64_t)(((o * cin + c) * kh + y) * kw + z));
                const uint64_t wo = blob.put(tmp), bo = blob.put(tmpb);
                li = new_layer(OP_CONV, x.idx, NO_TENSOR, (uint32_t)cin, (uint32_t)cout, (uint32_t)kh, (uint32_t)kw, (uint32_t)sh, (uint32_t)sw, (uint32_t)pt, (uint32_t)pl,
                               (uint32_t)h, (uint32_t)w, (uint32_t)oh, (uint32_t)ow, x.idx == 0 ? 1u : 0u, wo, bo);
                layers[li - 1].skip_h = (uint32_t)(dh - 1); layers[li - 1].skip_w = (uint32_t)(dw - 1);
            } else {
                // a grouped convolution -> OP_GCONV (convert.py has the same branch, refusal for refusal): compact weights
                // W[cout][cin / G][kh][kw] -> [kh][kw][cin / G][cout], the group count in the record's reserved word
                const std::string who = "Conv '" + n.name + "': group " + std::to_string(group) + " with " + std::to_string(cin) + " -> " + std::to_string(cout) + " channels";
                if (x.idx == 0) return fail(who + ": a grouped convolution on the spectrogram (tensor 0) is not supported");
                if (cin % group || cout % group || cin_g * group != cin)
                    return fail(who + ": the group count does not divide them (the weights hold " + std::to_string(cin_g) + " input channels a group)");
                if (cin_g % 4 || (cout / group) % 4)
                    return fail(who + ": a group width (" + std::to_string(cin_g) + " -> " + std::to_string(cout / group) + ") that is not a multiple of 4 is not supported");
                if (kh > 7 || kw > 7) return fail(who + ": a grouped kernel of " + std::to_string(kh) + "x" + std::to_string(kw) + " (1 .. 7 are supported)");
                if (sh > 2 || sw > 2) return fail(who + ": grouped strides of " + std::to_string(sh) + "x" + std::to_string(sw) + " (1 .. 2 are supported)");
                tmp.resize((size_t)kh * kw * cin_g * cout);
                for (int64_t o = 0; o < cout; o++)
                    for (int64_t c = 0; c < cin_g; c++)
                        for (int64_t y = 0; y < kh; y++)
                            for (int64_t z = 0; z < kw; z++)
                                tmp[(size_t)(((y * kw + z) * cin_g + c) * cout + o)] = W->at((uint64_t)(((o * cin_g + c) * kh + y) * kw + z));
                const uint64_t wo = blob.put(tmp), bo = blob.put(tmpb);
                li = new_layer(OP_GCONV, x.idx, NO_TENSOR, (uint32_t)cin, (uint32_t)cout, (uint32_t)kh, (uint32_t)kw, (uint32_t)sh, (uint32_t)sw, (uint32_t)pt, (uint32_t)pl,
                               (uint32_t)h, (uint32_t)w, (uint32_t)oh, (uint32_t)ow, 0, wo, bo);
                layers[li - 1].reserved = (uint32_t)group;
            }
            if (oh <= 0 || ow <= 0 || oh > DIM_MAX || ow > DIM_MAX) return fail("Conv '" + n.name + "': empty or oversized output");
            tmap[n.out[0]] = T{li, (uint32_t)cout, layers[li - 1].out_h, layers[li - 1].out_w};
            if (!flush_patterns(n.out[0])) return false;
        } else if (op == "BatchNormalization") {
            T t;
            if (!find(n.in[0], t) || t.idx == 0) return fail("BatchNormalization that does not follow a convolution directly");
            LayerRec &L = layers[t.idx - 1];
            const bool conv_type = L.op == OP_CONV || L.op == OP_DWCONV || L.op == OP_PWCONV || L.op == OP_GCONV;
            // the refusal this norm has had so far, by its producer; it stands unless the norm becomes a record of its own (below)
            std::string refusal;
            if (L.op == OP_CONCAT)
                refusal = "BatchNormalization '" + n.name + "' directly after a Concat, Split, Slice or channel shuffle cannot be folded (the record carries neither a scale nor an activation)";
            else if (!conv_type || L.act != A_NONE || n.in.size() < 5)
                refusal = "BatchNormalization that does not follow a convolution directly";
            // folding rewrites the convolution's weights, so the BN must be the ONLY reader of the convolution's
            // output (a skip taken before the BN would see scaled values), and a residual already folded into the layer means the BN
            // normalises conv + residual, which no rescaling of the conv's weights expresses
            else if (L.res_tensor != NO_TENSOR) refusal = "BatchNormalization after a residual Add (BN(conv + x)) cannot be folded into the convolution";
            if (!refusal.empty()) {
                // act(bn(x)) on a tensor no convolution can take the norm into -- a pool's, a concat's, an activated convolution's, a sum's,
                // another such record's -- is one OP_BNACT record (DenseNet, pre-activation ResNets; convert.py has the same branch, the two
                // are held to the same records).  The record is tentative, without an activation, until set_act completes it.
                const bool ok = n.in.size() >= 5 && t.h > 0 && t.w > 0 && t.c % 4 == 0 && !t.nhwc && !t.r3 && !t.view &&
                                (L.op == OP_POOL || L.op == OP_CONCAT || (L.op == OP_BNACT && !bn_pending.count(t.idx)) ||
                                 (conv_type && (L.res_tensor == NO_TENSOR || sums.count(n.in[0]))));
                if (!ok) return fail(refusal);
                const Tensor *p[4];
                init_refusal.clear();
                for (int q = 0; q < 4; q++) { p[q] = finit(n.in[1 + q]); if (!p[q] || p[q]->count != t.c) return fail("BatchNormalization '" + n.name + "': scale, B, mean and var must be float32 or float16 initializers of the " + std::to_string(t.c) + " channels" + init_refusal); }
                const double eps = (double)n.getf("epsilon", 1e-5f);
                tmp.resize(t.c); tmpb.resize(t.c);
                for (uint32_t c = 0; c < t.c; c++) {
                    const double gamma = p[0]->at(c), beta = p[1]->at(c), mean = p[2]->at(c), var = p[3]->at(c);
                    const double scale = gamma / std::sqrt(var + eps);
                    tmp[c] = (float)scale;
                    tmpb[c] = (float)(beta - mean * scale);
                }
                const uint64_t wo = blob.put(tmp), bo = blob.put(tmpb);
                const uint32_t li = new_layer(OP_BNACT, t.idx, NO_TENSOR, t.c, t.c, 1, 1, 1, 1, 0, 0, t.h, t.w, t.h, t.w, 0, wo, bo);
                bn_pending[li] = refusal;
                tmap[n.out[0]] = T{li, t.c, t.h, t.w};
                if (!flush_patterns(n.out[0])) return false;
                continue;
            }
            { auto cit = cons.find(n.in[0]); if ((cit != cons.end() && cit->second.size() != 1) || graph_out.count(n.in[0])) return fail("BatchNormalization of a convolution output that has other readers cannot be folded"); }
            const Tensor *p[4];
            init_refusal.clear();
            for (int q = 0; q < 4; q++) { p[q] = finit(n.in[1 + q]); if (!p[q] || p[q]->count != L.cout) return fail("BatchNormalization: parameters must be float32 or float16 initializers of the channel count" + init_refusal); }
            const double eps = (double)n.getf("epsilon", 1e-5f);
            const uint64_t nw = L.op == OP_CONV ? (uint64_t)L.kh * L.kw * L.cin * L.cout : L.op == OP_GCONV ? (uint64_t)L.kh * L.kw * (L.cin / L.reserved) * L.cout : L.op == OP_DWCONV ? (uint64_t)L.kh * L.kw * L.cout : (uint64_t)L.cin * L.cout;
            for (uint32_t c = 0; c < L.cout; c++) {
                const double gamma = p[0]->at(c), beta = p[1]->at(c), mean = p[2]->at(c), var = p[3]->at(c);
                const double scale = gamma / std::sqrt(var + eps);
                const float sf = (float)scale;
                for (uint64_t q = c; q < nw; q += L.cout) blob.v[L.w_off + q] = blob.v[L.w_off + q] * sf;    // (cout is the last axis in all three layouts)
                blob.v[L.b_off + c] = (float)(((double)blob.v[L.b_off + c] - mean) * scale + beta);
            }
            tmap[n.out[0]] = t;
            if (!flush_patterns(n.out[0])) return false;
        } else if (op == "Relu" || op == "Gelu" || op == "Clip") {
            uint32_t act = op == "Relu" ? A_RELU : op == "Gelu" ? A_GELU_ERF : A_RELU6;
            if (op == "Clip") {
                float lo = 0.f, hi = 0.f;
                const bool has_lo = n.in.size() > 1 && !n.in[1].empty() ? scalar(n.in[1], lo) : (n.a.count("min") ? (lo = n.getf("min", 0.f), true) : false);
                const bool has_hi = n.in.size() > 2 && !n.in[2].empty() ? scalar(n.in[2], hi) : (n.a.count("max") ? (hi = n.getf("max", 0.f), true) : false);
                if (!has_lo || !has_hi || lo != 0.0f || hi != 6.0f) return fail("Clip that is not ReLU6 (0, 6)");
            }
            if (op == "Gelu") { const std::string ap = n.gets("approximate", "none"); if (ap != "none") act = A_GELU_TANH; }
            if (!set_act(n.in[0], n.out[0], act, {i})) return false;
        } else if (op == "HardSwish") {
            if (!set_act(n.in[0], n.out[0], A_HSWISH, {i})) return false;
        } else if (op == "HardSigmoid") {
            // (HardSigmoid * x was folded above; what arrives here is a gate -- set_act holds it to a pooled tensor -- or a refusal)
            if (!hsig_is_torch(n)) {
                char v[96];
                snprintf(v, sizeof v, "alpha = %g, beta = %g", (double)n.getf("alpha", 0.2f), (double)n.getf("beta", 0.5f));
                return fail("HardSigmoid '" + n.name + "' with " + v + ": only alpha = 1/6, beta = 0.5 (PyTorch's hard sigmoid) is supported; the ONNX default alpha = 0.2 is Keras's hard sigmoid, a different function that no kernel here computes");
            }
            if (!set_act(n.in[0], n.out[0], A_HSIGMOID, {i})) return false;
        } else if (op == "Add") {
            T a, b;
            if (n.in.size() != 2 || !find(n.in[0], a) || !find(n.in[1], b)) return fail("Add of '" + n.in[0] + "': operands are not both activations on the path");
            bool done = false;
            for (int side = 0; side < 2 && !done; side++) {
                const T &y = side ? b : a, &r = side ? a : b;
                if (y.idx == 0) continue;
                LayerRec &L = layers[y.idx - 1];
                // (a 1x1 or a full NHWC convolution: Add(act(conv(x)), x), the Fused-MBConv residual; never the NCHW stem)
                const bool conv = L.op == OP_PWCONV || (L.op == OP_CONV && L.in_layout == 0);
                if (conv && L.res_tensor == NO_TENSOR && r.idx < y.idx && r.c == y.c && r.h == y.h && r.w == y.w) {
                    L.res_tensor = r.idx;
                    tmap[n.out[0]] = y;
                    sums.insert(n.out[0]);
                    done = true;
                }
            }
            if (!done) return fail("Add of '" + n.in[0] + "', '" + n.in[1] + "': no convolution to fold the residual into");
            if (!flush_patterns(n.out[0])) return false;   // (a multi-node activation behind the sum: act(conv + x))
        } else if (op == "ReduceMean" || op == "ReduceMax" || op == "GlobalMaxPool") {
            // max / mean over H, over W or over both -> OP_REDUCE, and Add(ReduceMax(x, a), ReduceMean(x, a)) -> one MAXMEAN record (convert.py
            // has the same branch; the two are held to the same records).  The mean over both axes of an NCHW map stays OP_GAP.
            const std::string who = op + " '" + n.name + "': ";
            T t;
            if (!find(n.in[0], t)) return fail(who + "input '" + n.in[0] + "' is not on the path from '" + spec + "'");
            // the image axes a node reduces, against its input's rank: (over H, over W); false: refused (err is set)
            auto image_axes = [&](const Node &q, const T &x, bool &rh, bool &rw) {
                const std::string w2 = q.op + " '" + q.name + "': ";
                std::vector<int64_t> axes;
                if (q.op == "GlobalMaxPool") axes = {2, 3};
                else if (const auto *ax = q.ints("axes")) axes = *ax;
                else if (q.in.size() > 1 && !q.in[1].empty()) { const auto *ax2 = const_ints(q.in[1]); if (!ax2) return fail(w2 + "axes '" + q.in[1] + "' that are not a constant"); axes = *ax2; }
                if (axes.empty() || axes.size() > 2) return fail(w2 + std::to_string(axes.size()) + " axes: only the image axes, H (2) or W (3) or both, are reduced");
                const int64_t rank = x.r3 ? 3 : 4;
                rh = rw = false;
                for (int64_t a : axes) {
                    const int64_t b = a < 0 ? a + rank : a;
                    if (b < 2 || b >= rank) return fail(w2 + "axis " + std::to_string(a) + " of a rank-" + std::to_string(rank) + " tensor: only the image axes are reduced (never the batch or the channels)");
                    const bool is_h = x.r3 ? x.r3 == 1 : b == 2;
                    if (is_h ? rh : rw) return fail(w2 + "axis " + std::to_string(a) + " named twice");
                    (is_h ? rh : rw) = true;
                }
                return true;
            };
            if (op == "GlobalMaxPool" && t.r3) return fail(who + "a rank-3 input");
            if (op == "GlobalMaxPool" && n.out.size() > 1) return fail(who + "more than one output");
            bool rh = false, rw = false;
            if (!image_axes(n, t, rh, rw)) return false;
            const int64_t keep = op == "GlobalMaxPool" ? 1 : n.geti("keepdims", 1);
            if (keep != 0 && keep != 1) return fail(who + "keepdims must be 0 or 1");
            uint32_t mode = op == "ReduceMean" ? REDUCE_MEAN : REDUCE_MAX;
            std::string out = n.out[0];
            // the max + mean pair: an Add reads this reduce and another one
            if (op != "GlobalMaxPool") {
                auto cit = cons.find(n.out[0]);
                if (cit != cons.end())
                    for (size_t k : cit->second) {
                        const Node &add = nodes[k];
                        if (add.op != "Add" || add.in.size() != 2 || add.out.empty() || skip.count(k)) continue;
                        const std::string &o2 = add.in[0] == n.out[0] ? add.in[1] : add.in[0];
                        auto pj = prod.find(o2);
                        if (pj == prod.end() || pj->second == i || skip.count(pj->second) || (nodes[pj->second].op != "ReduceMean" && nodes[pj->second].op != "ReduceMax")) continue;
                        const size_t j = pj->second;
                        const Node &q = nodes[j];
                        const std::string wa = "Add '" + add.name + "' (max + mean pair): ";
                        if (q.op == op) return fail(wa + "two " + op + " nodes: one ReduceMax and one ReduceMean of the same tensor are expected");
                        if (q.in.empty() || q.out.empty() || q.in[0] != n.in[0]) return fail(wa + "'" + n.name + "' and '" + q.name + "' reduce different tensors");
                        auto c2 = cons.find(q.out[0]);
                        if (cit->second.size() != 1 || c2 == cons.end() || c2->second.size() != 1 || graph_out.count(n.out[0]) || graph_out.count(q.out[0]))
                            return fail(wa + "a reduce that another node reads too, or that is a graph output (each is read by the Add alone)");
                        bool qh = false, qw = false;
                        if (!image_axes(q, t, qh, qw)) return false;
                        if (qh != rh || qw != rw) return fail(wa + "'" + n.name + "' and '" + q.name + "' reduce different axes");
                        if (q.geti("keepdims", 1) != keep) return fail(wa + "'" + n.name + "' and '" + q.name + "' differ in keepdims");
                        mode = REDUCE_MAXMEAN;
                        out = add.out[0];
                        skip.insert(j); skip.insert(k);
                        break;
                    }
            }
            if (mode == REDUCE_MEAN && rh && rw && !t.r3) {
                // the global average pool: OP_GAP, as ever
                const uint32_t li = new_layer(OP_GAP, t.idx, NO_TENSOR, t.c, t.c, t.h, t.w, 1, 1, 0, 0, t.h, t.w, 1, 1, 0, 0, 0);
                tmap[out] = T{li, t.c, 1, 1};
                emb_tensor = li; emb_dim = t.c;
                if (!flush_patterns(out)) return false;
                continue;
            }
            if (t.idx == 0) return fail(who + "a reduction of the spectrogram (tensor 0) is not supported");
            if (t.view) return fail(who + "a reduction of a Split / Slice output that only Concat nodes read is not supported");
            if (t.c % 4) return fail(who + std::to_string(t.c) + " channels: a channel count that is not a multiple of 4 is not supported");
            const uint32_t kh = rh ? t.h : 1, kw = rw ? t.w : 1;
            if ((uint64_t)kh * kw == 1) return fail(who + "a window of one pixel (the reduced axes have extent 1): nothing to reduce");
            if ((uint64_t)kh * kw > (1u << 16)) return fail(who + "a window of more than 65 536 pixels");
            const uint32_t oh = t.h / kh, ow = t.w / kw;
            const uint32_t li = new_layer(OP_REDUCE, t.idx, NO_TENSOR, t.c, t.c, kh, kw, 1, 1, 0, 0, t.h, t.w, oh, ow, 0, 0, 0);
            layers[li - 1].reserved = mode;
            T y{li, t.c, oh, ow};
            // (the pair over both axes, or one that finishes the image, is [N, C, 1, 1]: no rank-3 tensor of one pixel is kept)
            if (keep == 0 && !t.r3 && !(rh && rw) && !(mode == REDUCE_MAXMEAN && (uint64_t)oh * ow == 1)) y.r3 = rh ? 2 : 1;
            if (keep == 1 && t.r3 && !(mode == REDUCE_MAXMEAN && (uint64_t)oh * ow == 1)) y.r3 = t.r3;
            tmap[out] = y;
            if ((uint64_t)oh * ow == 1) { emb_tensor = li; emb_dim = t.c; }
            if (!flush_patterns(out)) return false;
        } else if (op == "GlobalAveragePool") {
            T t;
            if (!find(n.in[0], t)) return fail(op + ": input not on the path");
            const uint32_t li = new_layer(OP_GAP, t.idx, NO_TENSOR, t.c, t.c, t.h, t.w, 1, 1, 0, 0, t.h, t.w, 1, 1, 0, 0, 0);
            tmap[n.out[0]] = T{li, t.c, 1, 1};
            emb_tensor = li; emb_dim = t.c;
            if (!flush_patterns(n.out[0])) return false;      // (a decomposed LayerNorm behind the pool)
        } else if (op == "MaxPool" || op == "AveragePool") {
            // windowed pooling in floor mode -> OP_POOL (convert.py has the same branch; the two are held to the same records)
            const std::string who = op + " '" + n.name + "': ";
            T x;
            if (!find(n.in[0], x)) return fail(who + "input '" + n.in[0] + "' is not on the path from '" + spec + "'");
            if (x.idx == 0) return fail(who + "pooling on the planar spectrogram (tensor 0) is not supported");
            if (n.out.size() > 1 && !n.out[1].empty()) return fail(who + "the second output (Indices) is not supported");
            const auto *ks = n.ints("kernel_shape");
            if (!ks || ks->size() != 2 || (*ks)[0] < 1 || (*ks)[1] < 1 || (*ks)[0] > 64 || (*ks)[1] > 64) return fail(who + "kernel_shape must be two values, each 1 .. 64");
            const int64_t kh = (*ks)[0], kw = (*ks)[1];
            int64_t sh = 1, sw = 1;
            if (const auto *st = n.ints("strides")) { if (st->size() != 2) return fail(who + "strides"); sh = (*st)[0]; sw = (*st)[1]; }
            if (sh <= 0 || sw <= 0 || sh > 16 || sw > 16) return fail(who + "strides must be 1 .. 16");
            if (const auto *dl = n.ints("dilations")) for (int64_t d : *dl) if (d != 1) return fail(who + "a dilation other than 1 is not supported");
            if (n.geti("storage_order", 0) != 0) return fail(who + "storage_order = 1 (column-major indices) is not supported");
            const int64_t cip = n.geti("count_include_pad", 0), ceil_mode = n.geti("ceil_mode", 0);
            if ((cip != 0 && cip != 1) || (ceil_mode != 0 && ceil_mode != 1)) return fail(who + "count_include_pad / ceil_mode must be 0 or 1");
            const int64_t h = x.h, w = x.w;
            int64_t oh, ow, pt = 0, pl = 0;
            const std::string autop = n.gets("auto_pad", "NOTSET");
            if (autop == "SAME_UPPER" || autop == "SAME_LOWER") {
                oh = (h + sh - 1) / sh; ow = (w + sw - 1) / sw;
                const int64_t th = std::max<int64_t>((oh - 1) * sh + kh - h, 0), tw = std::max<int64_t>((ow - 1) * sw + kw - w, 0);
                if (autop == "SAME_UPPER") { pt = th / 2; pl = tw / 2; } else { pt = th - th / 2; pl = tw - tw / 2; }
            } else if (autop == "NOTSET" || autop == "VALID") {
                int64_t pads[4] = {0, 0, 0, 0};
                if (autop == "NOTSET")
                    if (const auto *pd = n.ints("pads")) { if (pd->size() != 4) return fail(who + "pads must be four values"); for (int q = 0; q < 4; q++) pads[q] = (*pd)[q]; }
                for (int64_t p : pads) if (p < 0 || p > 64) return fail(who + "pads must be 0 .. 64");
                pt = pads[0]; pl = pads[1];
                const int64_t eh = h + pads[0] + pads[2] - kh, ew = w + pads[1] + pads[3] - kw;
                if (eh < 0 || ew < 0) return fail(who + "kernel larger than the padded input");
                oh = eh / sh + 1; ow = ew / sw + 1;
                if (ceil_mode) {   // ONNX: round up, but the last window must start inside the image or its top / left padding
                    int64_t ch = (eh + sh - 1) / sh + 1, cw = (ew + sw - 1) / sw + 1;
                    if ((ch - 1) * sh >= h + pads[0]) ch--;
                    if ((cw - 1) * sw >= w + pads[1]) cw--;
                    if (ch != oh || cw != ow)
                        return fail(who + "ceil_mode = 1 changes the output size (" + std::to_string(oh) + "x" + std::to_string(ow) + " -> " + std::to_string(ch) + "x" + std::to_string(cw) + "): only floor-mode windows are supported");
                }
            } else return fail(who + "auto_pad '" + autop + "'");
            if (oh <= 0 || ow <= 0 || oh > DIM_MAX || ow > DIM_MAX) return fail(who + "empty or oversized output");
            if (pt >= kh || pl >= kw || (oh - 1) * sh - pt >= h || (ow - 1) * sw - pl >= w) return fail(who + "a window without an in-image tap (it lies in the padding alone)");
            const uint32_t li = new_layer(OP_POOL, x.idx, NO_TENSOR, x.c, x.c, (uint32_t)kh, (uint32_t)kw, (uint32_t)sh, (uint32_t)sw, (uint32_t)pt, (uint32_t)pl,
                                          (uint32_t)h, (uint32_t)w, (uint32_t)oh, (uint32_t)ow, 0, 0, 0);
            layers[li - 1].reserved = op == "MaxPool" ? POOL_MAX : cip ? POOL_AVG_PAD : POOL_AVG;
            tmap[n.out[0]] = T{li, x.c, (uint32_t)oh, (uint32_t)ow};
        } else if (op == "Concat") {
            // over the channels -> OP_CONCAT: two inputs one record, more a left-to-right chain, each record reading the one before
            // as its first source (convert.py has the same branch; the two are held to the same records)
            const std::string who = "Concat '" + n.name + "': ";
            if (n.in.size() > 64) return fail(who + std::to_string(n.in.size()) + " inputs (1 .. 64 are read)");
            const int64_t axis = n.geti("axis", 0);
            if (axis != 1 && axis != -3) return fail(who + "axis " + std::to_string(axis) + ": only the channel axis (1, or -3) is concatenated");
            std::vector<T> src;
            int64_t sum = 0;
            for (const auto &name : n.in) {
                T x;
                if (g.init.count(name)) return fail(who + "input '" + name + "' is a constant: only activations are concatenated");
                if (!find(name, x)) return fail(who + "input '" + name + "' is not on the path from '" + spec + "'");
                if (x.idx == 0) return fail(who + "the spectrogram (tensor 0) as an input is not supported");
                if (!src.empty() && (x.h != src[0].h || x.w != src[0].w))
                    return fail(who + "inputs of different images (" + std::to_string(src[0].h) + "x" + std::to_string(src[0].w) + " and " + std::to_string(x.h) + "x" + std::to_string(x.w) + ")");
                if (x.c % 4 || x.off % 4) return fail(who + "input '" + name + "' is " + std::to_string(x.c) + " channels from channel " + std::to_string(x.off) + ": " + quad);
                sum += x.c;
                src.push_back(x);
            }
            if (sum > DIM_MAX) return fail(who + "more than 65 536 channels");
            // prefix reuse (a DenseNet layer's Concat over the whole list of earlier features): where the leading j >= 2 inputs are, in order,
            // the complete input list of an earlier Concat whose output is still a plain whole tensor, the chain starts from that output
            // (the longest such prefix; j < the inputs, so that a Concat always is a record of its own)
            size_t start = 0;
            T y{};
            for (const auto &cl : cat_lists) {
                const size_t j = cl.first.size();
                if (j < 2 || j >= src.size() || j <= start || layers[cl.second.idx - 1].reserved > 1) continue;
                bool same = true;
                for (size_t k = 0; k < j && same; k++)
                    same = cl.first[k].idx == src[k].idx && cl.first[k].c == src[k].c && cl.first[k].off == src[k].off;
                if (same) { start = j; y = cl.second; }
            }
            if (!start) { y = concat_rec(src[0], src.size() > 1 ? &src[1] : nullptr, 0); start = 2; }
            for (size_t k = start; k < src.size(); k++) y = concat_rec(y, &src[k], 0);
            cat_lists.emplace_back(src, y);
            tmap[n.out[0]] = y;
            if (!flush_patterns(n.out[0])) return false;
        } else if (op == "Split" || op == "Slice") {
            // over the channels: every output is a view of the input (publish_view)
            const std::string who = op + " '" + n.name + "': ";
            T x;
            if (!find(n.in[0], x)) return fail(who + "input '" + n.in[0] + "' is not on the path from '" + spec + "'");
            if (x.idx == 0) return fail(who + "the spectrogram (tensor 0) as the input is not supported");
            std::vector<int64_t> starts, sizes;
            if (op == "Split") {
                const int64_t axis = n.geti("axis", 0);
                if (axis != 1 && axis != -3) return fail(who + "axis " + std::to_string(axis) + ": only the channel axis (1) is split");
                const int64_t parts = (int64_t)n.out.size();
                if (parts > 64) return fail(who + std::to_string(parts) + " outputs (1 .. 64 are read)");
                if (const auto *sp = n.ints("split")) sizes = *sp;
                else if (n.in.size() > 1 && !n.in[1].empty()) {
                    const auto *sp2 = const_ints(n.in[1]);
                    if (!sp2) return fail(who + "sizes '" + n.in[1] + "' that are not a constant");
                    sizes = *sp2;
                } else {
                    if (n.geti("num_outputs", parts) != parts || x.c % parts) return fail(who + std::to_string(x.c) + " channels in " + std::to_string(parts) + " equal parts");
                    sizes.assign((size_t)parts, x.c / parts);
                }
                int64_t at = 0;
                if ((int64_t)sizes.size() != parts) return fail(who + std::to_string(sizes.size()) + " sizes for " + std::to_string(parts) + " outputs");
                for (int64_t s : sizes) { if (s <= 0 || s > DIM_MAX) return fail(who + "a part of " + std::to_string(s) + " channels"); starts.push_back(at); at += s; }
                if (at != x.c) return fail(who + "sizes that add up to " + std::to_string(at) + ", the input has " + std::to_string(x.c) + " channels");
            } else {
                const std::vector<int64_t> *lst[4] = {nullptr, nullptr, nullptr, nullptr};   // starts, ends, axes, steps
                for (size_t q = 0; q < 4; q++)
                    if (n.in.size() > q + 1 && !n.in[q + 1].empty()) {
                        lst[q] = const_ints(n.in[q + 1]);
                        if (!lst[q]) return fail(who + "'" + n.in[q + 1] + "' is not a constant (starts, ends, axes and steps are read from constant inputs)");
                    }
                if (!lst[0] || !lst[1] || !lst[2] || lst[0]->size() != 1 || lst[1]->size() != 1 || lst[2]->size() != 1 || (lst[3] && lst[3]->size() != 1))
                    return fail(who + "only a slice along one stated axis, the channels, is read");
                if ((*lst[2])[0] != 1 && (*lst[2])[0] != -3) return fail(who + "axis " + std::to_string((*lst[2])[0]) + ": only the channel axis (1) is sliced");
                if (lst[3] && (*lst[3])[0] != 1) return fail(who + "step " + std::to_string((*lst[3])[0]) + ": only step 1 is read");
                const int64_t C = x.c;
                int64_t s = (*lst[0])[0], e = (*lst[1])[0];
                if (s < 0) s = s < -C ? 0 : s + C;
                if (e < 0) e = e < -C ? 0 : e + C;
                s = std::min(s, C); e = std::min(e, C);
                if (e <= s) return fail(who + "an empty slice");
                starts.push_back(s); sizes.push_back(e - s);
            }
            for (size_t k = 0; k < sizes.size(); k++)
                if (sizes[k] % 4 || starts[k] % 4)
                    return fail(who + "output " + std::to_string(k) + " is " + std::to_string(sizes[k]) + " channels from channel " + std::to_string(starts[k]) + ": " + quad);
            for (size_t k = 0; k < sizes.size(); k++) {
                if (n.out[k].empty()) continue;
                publish_view(n.out[k], x, (uint32_t)starts[k], (uint32_t)sizes[k]);
                if (!flush_patterns(n.out[k])) return false;
            }
        } else if (op == "Reshape" && shuffle_at.count(i)) {
            // the channel shuffle: the `reserved` word of the Concat record in front when this is its only reader, else a record of its own
            const Shuffle &sh = shuffle_at[i];
            const std::string who = "Reshape '" + n.name + "' (channel shuffle): ";
            T x;
            if (!find(n.in[0], x)) return fail(who + "input '" + n.in[0] + "' is not on the path from '" + spec + "'");
            if (x.idx == 0) return fail(who + "the spectrogram (tensor 0) as the input is not supported");
            std::vector<int64_t> d5, d4;
            const int64_t total = (int64_t)x.c * x.h * x.w;
            if (sh.s1.size() != 5 || sh.s2.size() != 4 || !resolve_shape(sh.s1, {x.c, x.h, x.w}, total, d5) || d5[0] * d5[1] != x.c || d5[2] != x.h || d5[3] != x.w ||
                !resolve_shape(sh.s2, {d5[1], d5[0], x.h, x.w}, total, d4) || d4[0] != x.c || d4[1] != x.h || d4[2] != x.w)
                return fail(who + "the shapes are not [N, g, C / g, H, W] and [N, C, H, W] of its " + std::to_string(x.c) + " x " + std::to_string(x.h) + " x " + std::to_string(x.w) + " input");
            if (x.c % 4 || x.off % 4) return fail(who + std::to_string(x.c) + " channels: " + quad);
            const uint32_t groups = (uint32_t)d5[0];
            auto cit = cons.find(n.in[0]);
            LayerRec &P = layers[x.idx - 1];
            if (!x.view && P.op == OP_CONCAT && P.reserved <= 1 && !graph_out.count(n.in[0]) && cit != cons.end() && cit->second.size() == 1) {
                P.reserved = groups;
                tmap[sh.out] = x;
            } else tmap[sh.out] = concat_rec(x, nullptr, groups);
            if (!flush_patterns(sh.out)) return false;
        } else if (op == "Reshape" && shuffle_computed.count(i)) {
            return fail("Reshape '" + n.name + "': a channel shuffle whose shape is computed (Shape -> Gather -> Concat) is not read: the shapes must be constants");
        } else if (op == "Flatten" || op == "Reshape" || op == "Squeeze" || op == "Unsqueeze" || op == "Identity" || op == "Dropout") {
            T t;
            if (!find(n.in[0], t)) return fail(op + ": input not on the path");
            if ((uint64_t)t.h * t.w != 1) return fail(op + " of a " + std::to_string(t.h) + "x" + std::to_string(t.w) + " map (only after the global pool)");
            t.r3 = 0;
            tmap[n.out[0]] = t;
        } else if (op == "Gemm" || op == "MatMul") {
            T t;
            init_refusal.clear();
            const Tensor *W = n.in.size() > 1 ? finit(n.in[1]) : nullptr;
            if (!find(n.in[0], t) || !W || W->dims.size() != 2) return fail(op + ": needs an activation on the path and a 2-d float32 or float16 weight initializer" + init_refusal);
            const bool gemm = op == "Gemm", tb = gemm && n.geti("transB", 0) != 0;
            if (gemm && (n.getf("alpha", 1.0f) != 1.0f || n.getf("beta", 1.0f) != 1.0f || n.geti("transA", 0) != 0)) return fail("Gemm with alpha / beta / transA");
            const int64_t cin = tb ? W->dims[1] : W->dims[0], cout = tb ? W->dims[0] : W->dims[1];
            if (cin <= 0 || cout <= 0 || cin > (1 << 20) || cout > (1 << 24)) return fail(op + ": bad weight shape");
            if ((uint64_t)cin != (uint64_t)t.c * t.h * t.w || (uint64_t)t.h * t.w != 1) return fail(op + ": " + std::to_string(cin) + " input features, activation has " + std::to_string(t.c));
            const Tensor *B = gemm && n.in.size() > 2 && !n.in[2].empty() ? finit(n.in[2]) : nullptr;
            std::string out = n.out[0];
            if (!B) {   // MatMul followed by Add(bias)
                size_t k;
                if (sole_consumer(out, "Add", k) && nodes[k].in.size() == 2 && !nodes[k].out.empty()) {
                    const std::string &other = nodes[k].in[0] == out ? nodes[k].in[1] : nodes[k].in[0];
                    const Tensor *ob = finit(other);
                    if (ob && ob->count == (uint64_t)cout) { B = ob; out = nodes[k].out[0]; skip.insert(k); }
                }
            }
            if (B && B->count != (uint64_t)cout) return fail(op + ": bias width");
            tmp.resize((size_t)cin * cout);
            for (int64_t c = 0; c < cin; c++)
                for (int64_t o = 0; o < cout; o++) tmp[(size_t)c * cout + o] = tb ? W->at((uint64_t)(o * cin + c)) : W->at((uint64_t)(c * cout + o));
            tmpb.assign((size_t)cout, 0.0f);
            if (B) for (int64_t o = 0; o < cout; o++) tmpb[(size_t)o] = B->at((uint64_t)o);
            const uint64_t wo = blob.put(tmp), bo = blob.put(tmpb);
            const uint32_t li = new_layer(OP_DENSE, t.idx, NO_TENSOR, (uint32_t)cin, (uint32_t)cout, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0, wo, bo);
            tmap[out] = T{li, (uint32_t)cout, 1, 1};
            if (!flush_patterns(out)) return false;
        } else if (op == "Sigmoid" && !graph_out.count(n.out[0])) {
            // the gate of a squeeze-excite block: Sigmoid on a pooled [N, C, 1, 1] tensor, consumed by a Mul with the feature map
            T t;
            if (!find(n.in[0], t) || (uint64_t)t.h * t.w != 1) return fail("Sigmoid inside the graph that is neither Sigmoid * x nor a squeeze-excite gate");
            if (!set_act(n.in[0], n.out[0], A_SIGMOID, {i})) return false;
        } else if (op == "Mul") {
            T a, b;
            if (n.in.size() != 2 || !find(n.in[0], a) || !find(n.in[1], b)) return fail("Mul of '" + n.in[0] + "': operands are not both activations on the path");
            bool done = false;
            for (int side = 0; side < 2 && !done; side++) {
                const T &fm = side ? b : a, &gate = side ? a : b;
                if ((uint64_t)fm.h * fm.w > 1 && (uint64_t)gate.h * gate.w == 1 && gate.c == fm.c) {
                    const uint32_t li = new_layer(OP_SCALE, fm.idx, gate.idx, fm.c, fm.c, 1, 1, 1, 1, 0, 0, fm.h, fm.w, fm.h, fm.w, 0, 0, 0);
                    tmap[n.out[0]] = T{li, fm.c, fm.h, fm.w};
                    done = true;
                }
            }
            if (!done) return fail("Mul of '" + n.in[0] + "', '" + n.in[1] + "': not a feature map times a [N, C, 1, 1] gate");
        } else if (op == "Sigmoid" || op == "Softmax") {
            if (!graph_out.count(n.out[0])) return fail(op + " inside the graph (only the output activation is supported, or Sigmoid * x)");
            T t;
            if (!find(n.in[0], t)) return fail(op + ": input not on the path");
            out_act = op == "Sigmoid" ? O_SIGMOID : O_SOFTMAX;
            tmap[n.out[0]] = t;
        } else {
            return fail("unsupported operator " + op + " ('" + n.name + "')");
        }
    }
    if (!bn_pending.empty()) return fail(bn_pending.begin()->second);
    if (!first_of_pattern.empty()) return fail("activation pattern on a tensor that was never produced: '" + first_of_pattern.begin()->first + "'");
    if (!ln_of_pattern.empty()) return fail("activation pattern on a tensor that was never produced: '" + ln_of_pattern.begin()->first + "'");
    if (layers.empty() || layers.back().op != OP_DENSE) return fail("the graph does not end in a dense layer");
    T fin;
    if (!find(outputs[0], fin) || fin.idx != layers.size()) return fail("the graph output is not the last layer's output");
    m.h.n_layers = (uint32_t)layers.size();
    m.h.n_classes = layers.back().cout;
    m.h.embedding_dim = emb_dim;
    m.h.embedding_tensor = emb_tensor;
    m.h.output_activation = out_act;
    // Perch v2 and BirdNET v3.0 share an input length: told apart by what the graph ends in (classifier.rs:360-377 reads the model
    // type from the crate's detection; manifests: Perch softmax over 14 795 classes, v3.0 a sigmoid inside the graph)
    m.h.family = fam->sample_count == 160000 ? (out_act == O_SOFTMAX ? 1u : 2u) : 0u;
    m.blob = std::move(blob.v);
    m.h.blob_floats = m.blob.size();
    m.h.blob_offset = 0;
    return validate_model(m, err);
}

inline bool read_file(const char *path, std::vector<uint8_t> &buf, std::string &err) {
    FILE *f = fopen(path, "rb");
    if (!f) { err = std::string("cannot open model file ") + path; return false; }
    bool ok = false;
    if (fseek(f, 0, SEEK_END) == 0) {
        const long sz = ftell(f);
        if (sz > 0 && sz < (3l << 30)) { buf.resize((size_t)sz); rewind(f); ok = fread(buf.data(), 1, buf.size(), f) == buf.size(); }
    }
    fclose(f);
    if (!ok) { buf.clear(); err = std::string(path) + ": empty, unreadable or larger than 3 GiB"; }
    return ok;
}

inline bool load_onnx_model(const char *path, Model &m, std::string &err) {
    std::vector<uint8_t> buf;
    if (!read_file(path, buf, err)) return false;
    Graph g;
    if (!parse_graph(Span{buf.data(), buf.size()}, g, err) || !model_from_graph(g, m, err)) { err = std::string(path) + ": " + err; return false; }
    return true;
}

// the container birda_amd/modelfile.py writes (header 256 B, branch records 64 B, layer records 128 B, blob at a multiple of 256 B)
inline bool write_bhm(const char *path, const Model &m, std::string &err) {
    FILE *f = fopen(path, "wb");
    if (!f) { err = std::string("cannot write ") + path; return false; }
    HeaderRec h = m.h;
    h.n_branches = (uint32_t)m.branches.size(); h.n_layers = (uint32_t)m.layers.size();
    uint64_t off = 256 + 64ull * m.branches.size() + 128ull * m.layers.size();
    off = (off + 255) / 256 * 256;
    h.blob_offset = off; h.blob_floats = m.blob.size();
    std::vector<unsigned char> head((size_t)off, 0);
    memcpy(head.data(), &h, sizeof h);
    size_t p = 256;
    for (const auto &b : m.branches) { memcpy(head.data() + p, &b, sizeof b); p += 64; }
    for (const auto &L : m.layers) { memcpy(head.data() + p, &L, sizeof L); p += 128; }
    const bool ok = fwrite(head.data(), 1, head.size(), f) == head.size() && fwrite(m.blob.data(), sizeof(float), m.blob.size(), f) == m.blob.size();
    if (fclose(f) != 0 || !ok) { err = std::string("short write to ") + path; return false; }
    return true;
}

}  // namespace onnxc
}  // namespace bh
