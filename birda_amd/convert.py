"""ONNX conv stack  <->  BHM1 layer table.

`model_from_graph` turns the classifier part of an ONNX graph -- from the spectrogram tensor
[N, C, H, W] to the logits -- into the layer table `modelfile.py` describes: Conv (group 1 / depthwise
/ 1x1 / any other group count: OP_GCONV) with BatchNormalization folded (or, with its activation, on a pool output, a concat, a residual sum or an activated convolution, one OP_BNACT record: DenseNet, pre-activation ResNets), the activation that follows folded into the producing layer
(Relu, Clip 0..6, Sigmoid*x, the Div-Erf-Add-Mul-Mul spelling of exact GELU, a fused `Gelu`; MobileNetV3's hard swish as `HardSwish`,
as HardSigmoid(1/6, 1/2)*x or as the Add 3 - Clip 0..6 - Mul x - Mul 1/6 chain, its hard-sigmoid gate as HardSigmoid(1/6, 1/2) or that
chain without the Mul x),
residual Add folded into the project conv -- with the activation that follows the Add, if any, as that layer's (Layer.reserved =
RES_ACT_AFTER: act(conv + x), the end of a ResNet block) --, squeeze-excite blocks (GlobalAveragePool -> 1x1 Conv -> activation -> 1x1 Conv ->
Sigmoid -> Mul with the feature map) as pool / 1x1 / 1x1 / OP_SCALE layers, MaxPool / AveragePool in floor mode (OP_POOL: any
window, stride and padding; count_include_pad either way), Concat / Split / Slice over the channels and the Reshape -> Transpose ->
Reshape channel shuffle (OP_CONCAT; a Split / Slice output that only Concat nodes read is a view folded into their windows),
ConvNeXt blocks (OP_LNORM: Transpose [0, 2, 3, 1] / [0, 3, 1, 2] as an [N, H, W, C] view that costs no record, LayerNormalization over the
channels as a node or as the decomposed ReduceMean -> Sub -> Pow -> ReduceMean -> Add -> Sqrt -> Div -> Mul -> Add chain -- over axis 1 of
an NCHW map too --, MatMul + Add on the view as a 1x1 layer, the layer-scale Mul by a constant of the channels folded into the layer in front),
GlobalAveragePool / ReduceMean, ReduceMax / ReduceMean over H or W or both, GlobalMaxPool and the max + mean pair Add(ReduceMax, ReduceMean)
of the PANNs head (OP_REDUCE), Flatten, Gemm / MatMul + Add,
final Sigmoid / Softmax as the output activation.  Weights move from ONNX's [Cout, Cin/g, kh, kw] to
the NHWC-friendly layouts of the kernels.

The STFT / mel front-end: either the model family's manifest values through `frontend`, with the
graph entered at the spectrogram tensor named by `spectrogram_input` (default: the graph's first input) -- or, with
`frontend=None` and a sample rate, read off the graph itself by probing (`frontend_recover.py`: how the published BirdNET and
Perch ONNX files spell that part -- STFT op, DFT-as-Conv1d, ... -- is not knowable offline, so no spelling is matched; the nodes
in front of the first 2-D convolution are evaluated on probe signals and the container's parameters fitted to the responses).
The reference loads the same file through `birdnet_onnx::ClassifierBuilder::model_path` (src/inference/classifier.rs:269-283).

`graph_from_model` is the inverse for the synthetic models; it exists so that the converter can be
tested (tests/test_convert.py: model -> ONNX bytes -> model, identical layer tables, weights and oracle
logits).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import modelfile as mf
from . import onnx_io as ox

SQRT2 = math.sqrt(2.0)
# the float16 roundings of sqrt 2 and 1 / sqrt 2: what the erf-GELU spelling of a float16 file carries
SQRT2_F16, RSQRT2_F16 = float(np.float16(SQRT2)), float(np.float16(1.0 / SQRT2))
FLOAT_CASTS = (ox.FLOAT, ox.FLOAT16, ox.DOUBLE)


class ConvertError(ValueError):
    pass


# ---------------------------------------------------------------------------------------
# model -> ONNX  (test fixture generator)
# ---------------------------------------------------------------------------------------
def frontend_nodes(g: ox.Graph, m: mf.Model, spelling: str) -> None:
    """Appends the spectrogram front-end of `m` to `g` as nodes from `audio` [N, S] to `spectrogram`
    [N, C, n_mels, n_frames], in one of several spellings an exporter might choose.  Fixture generator for
    tests/test_frontend_recover.py: the recovery must not care which one it gets.
      'conv1d'  DFT as a strided Conv (real rows only) -> MatMul mel -> Mul(t, t) -> Pow(const) -> Mul, Add -> Transpose -> Slice(-1)
      'stft'    opset-17 STFT node -> Gather real part -> MatMul mel -> Pow(t, 2) -> Pow(1 / (1 + Exp(mag_scale))) ->
                BatchNormalization-free affine as Sub / Div -> Gather with reversed indices
      'complex' Conv with cos AND -sin rows -> Slice of the real rows -> 1x1 Conv as the mel projection; the normalisation
                written as (x - min) * (2 / (range + eps)) - 1
      'fused'   window, DFT, mel matrix AND the mel flip folded into the Conv weights: [n_mels, 1, L] rows, nothing else linear"""
    def const(name, arr, dtype=np.float32):
        g.initializers[name] = np.asarray(arr, dtype)
        return name

    def node(op, ins, out, **attrs):
        g.nodes.append(ox.Node(op, list(ins), [out], attrs, name=out))
        return out

    ax1 = const("fe_ax1", [1], np.int64)
    mn = node("ReduceMin", ["audio"], "fe_min", axes=[1], keepdims=1)
    mx = node("ReduceMax", ["audio"], "fe_max", axes=[1], keepdims=1)
    rng_ = node("Sub", [mx, mn], "fe_range")
    den = node("Add", [rng_, const("fe_eps", np.float32(m.norm_eps))], "fe_den")
    if spelling == "complex":
        sc = node("Div", [const("fe_two", 2.0), den], "fe_sc")
        xn = node("Sub", [node("Mul", [node("Sub", ["audio", mn], "fe_c"), sc], "fe_cs"), const("fe_one", 1.0)], "fe_xn")
    else:
        x01 = node("Div", [node("Sub", ["audio", mn], "fe_c"), den], "fe_x01")
        xn = node("Mul", [node("Sub", [x01, const("fe_half", 0.5)], "fe_xh"), const("fe_two", 2.0)], "fe_xn")
    chans = []
    for b, br in enumerate(m.branches):
        t = f"fe{b}"
        L, H, bins = br.frame_length, br.frame_step, br.n_bins
        n = np.arange(L)
        hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / L)
        ang = 2.0 * np.pi * ((n[:, None] * np.arange(bins)[None, :]) % L) / L
        wcos, wsin = hann[:, None] * np.cos(ang), -hann[:, None] * np.sin(ang)          # [L, bins]
        mel = m.weight(br.mel_w_off, bins * br.n_mels).reshape(bins, br.n_mels).astype(np.float64)
        expo = 1.0 / (1.0 + math.exp(br.mag_scale))
        flip = bool(br.flags & 1)
        if spelling == "stft":
            sig = node("Unsqueeze", [xn, const("fe_ax2", [2], np.int64)], t + "_sig")
            st = node("STFT", [sig, const(t + "_step", H, np.int64), const(t + "_win", hann), const(t + "_len", L, np.int64)],
                      t + "_stft", onesided=1)                                                 # [N, frames, bins, 2]
            re = node("Gather", [st, const(t + "_zero", 0, np.int64)], t + "_re", axis=3)
            lin = node("MatMul", [re, const(t + "_mel", mel)], t + "_lin")                      # [N, frames, mels]
            layout = "tm"
        else:
            sig = node("Unsqueeze", [xn, ax1], t + "_sig")                                      # [N, 1, S]
            if spelling == "conv1d":
                cv = node("Conv", [sig, const(t + "_dft", wcos.T[:, None, :])], t + "_cv", strides=[H], kernel_shape=[L])
                tr = node("Transpose", [cv], t + "_tr", perm=[0, 2, 1])
                lin = node("MatMul", [tr, const(t + "_mel", mel)], t + "_lin")
                layout = "tm"
            elif spelling == "complex":
                w = np.concatenate([wcos.T, wsin.T], axis=0)[:, None, :]                       # [2 bins, 1, L]
                cv = node("Conv", [sig, const(t + "_dft", w)], t + "_cv", strides=[H], kernel_shape=[L])
                re = node("Slice", [cv, const(t + "_s0", [0], np.int64), const(t + "_s1", [bins], np.int64), ax1], t + "_re")
                lin = node("Conv", [re, const(t + "_mel", mel.T[:, :, None])], t + "_lin", kernel_shape=[1])   # [N, mels, frames]
                layout = "mt"
            elif spelling == "fused":
                G = wcos @ mel                                                                  # [L, mels]
                if flip:
                    G = G[:, ::-1]
                lin = node("Conv", [sig, const(t + "_op", np.ascontiguousarray(G.T)[:, None, :])], t + "_lin", strides=[H], kernel_shape=[L])
                layout, flip = "mt", False
            else:
                raise ConvertError(f"front-end spelling {spelling!r}")
        if spelling == "stft":
            sq = node("Pow", [lin, const(t + "_p2", 2.0)], t + "_sq")
            e1 = node("Exp", [const(t + "_mag", np.float32(br.mag_scale))], t + "_e1")
            ex = node("Div", [const(t + "_n1", 1.0), node("Add", [e1, const(t + "_o1", 1.0)], t + "_e2")], t + "_ex")
            pw = node("Pow", [sq, ex], t + "_pw")
            # an affine spelled as a normalisation: (v - mean) / std
            af = node("Div", [node("Sub", [pw, const(t + "_mean", np.float32(-br.out_shift / br.out_scale))], t + "_ctr"),
                              const(t + "_std", np.float32(1.0 / br.out_scale))], t + "_af")
        else:
            sq = node("Mul", [lin, lin], t + "_sq")
            pw = node("Pow", [sq, const(t + "_ex", np.float32(expo))], t + "_pw")
            af = node("Add", [node("Mul", [pw, const(t + "_sc", np.float32(br.out_scale))], t + "_scd"),
                              const(t + "_sh", np.float32(br.out_shift))], t + "_af")
        if layout == "tm":
            af = node("Transpose", [af], t + "_mt", perm=[0, 2, 1])                            # [N, mels, frames]
        if flip and spelling == "stft":
            af = node("Gather", [af, const(t + "_rev", np.arange(br.n_mels - 1, -1, -1), np.int64)], t + "_fl", axis=1)
        elif flip:
            af = node("Slice", [af, const(t + "_f0", [-1], np.int64), const(t + "_f1", [-(2 ** 62)], np.int64), ax1,
                                const(t + "_fs", [-1], np.int64)], t + "_fl")
        chans.append(node("Unsqueeze", [af, ax1], t + "_ch"))
    node("Concat", chans, "spectrogram", axis=1)


HSWISH_SPELLINGS = ("op", "hsigmoid", "decomposed")


REDUCE_SPELLING_OPTIONS = {"keep", "input", "neg", "gmp", "swap", "argmax"}


def graph_from_model(m: mf.Model, spell_gelu: str = "erf", frontend_spelling: Optional[str] = None, spell_hswish: str = "op",
                     spell_lnorm: str = "node", spell_reduce: str = "", spell_concat: str = "pair") -> ox.Graph:
    """The conv stack of a BHM1 model as an ONNX graph over `spectrogram` [N, C, H, W] -- or, with `frontend_spelling`
    (see `frontend_nodes`), the whole model over `audio` [N, S].
    spell_gelu: 'erf' = Div, Erf, Add, Mul, Mul (what exporters emit below opset 20); 'gelu' = one Gelu node.
    spell_hswish: how ACT_HSWISH / ACT_HSIGMOID are written -- 'op' = HardSwish (opset 14) / HardSigmoid(alpha 1/6, beta 0.5);
    'hsigmoid' = HardSigmoid * x (PyTorch below opset 14) / HardSigmoid; 'decomposed' = Add(x, 3) -> Clip(0, 6) -> Mul(., x) ->
    Mul(., 1/6) (tf2onnx; the gate without the Mul(., x)).  Options follow 'decomposed' after a colon, comma-separated: 'div' (Div(., 6)
    for the last Mul), 'scale_first' (the scaling in front of the Mul(., x)), 'swap' (every binary node's operands exchanged where the
    operator commutes), 'f16' (float16 constants), 'cast' (a Cast to float32 inside the fold; 'hsigmoid' takes 'swap' and 'cast' too).
    spell_lnorm: how an OP_LNORM record is written between its two Transposes -- 'node' = LayerNormalization(axis = -1, epsilon) (opset
    17); 'chain' = ReduceMean -> Sub -> Pow(2) -> ReduceMean -> Add(eps) -> Sqrt -> Div -> Mul -> Add (what torch.onnx emits below it).
    spell_reduce: how an OP_REDUCE record is written, comma-separated options over PyTorch's default spelling -- x.mean(dim) / torch.max(x,
    dim) as ReduceMean / ReduceMax(axes = [2] or [3], keepdims = 0) with the axes as an attribute, the pair as Add(max, mean) --: 'keep'
    (keepdims = 1), 'input' (the axes as the opset-18 input), 'neg' (negative axes), 'gmp' (a max over both axes as GlobalMaxPool), 'swap'
    (Add(mean, max)), 'argmax' (the ArgMax that torch.max leaves behind, read by nothing).
    spell_concat: 'pair' = an OP_CONCAT record as a Concat of its own one or two sources; 'list' = a dense block's concats as the growing
    list -- a plain two-source record whose first source is the whole output of an earlier such record lists that record's inputs in its
    place, Concat([f0, f1, ..., fk]) over every earlier feature (what torchvision and timm export of a DenseNet layer).
    An OP_BNACT record is written as BatchNormalization(scale = scale, B = shift, mean = 0, var = 1, epsilon = 0) and the activation's
    spelling: either reader folds that back to the same bits (scale / sqrt(1 + 0), shift - 0 scale)."""
    if spell_lnorm not in ("node", "chain"):
        raise ConvertError(f"unknown LayerNorm spelling {spell_lnorm!r}")
    if spell_concat not in ("pair", "list"):
        raise ConvertError(f"unknown concat spelling {spell_concat!r}")
    cat_parts: Dict[int, List[str]] = {}   # tensor of a plain two-source concat record -> the names its Concat node lists ('list')
    red_opts = set(filter(None, spell_reduce.split(",")))
    if not red_opts <= REDUCE_SPELLING_OPTIONS:
        raise ConvertError(f"unknown reduce spelling {spell_reduce!r}")
    rank = {}   # tensor -> 3 or 2 where a reduction with keepdims = 0 left fewer than four axes
    hs_kind, _, hs_opts = spell_hswish.partition(":")
    hs_opts = set(filter(None, hs_opts.split(",")))
    if hs_kind not in HSWISH_SPELLINGS or not hs_opts <= {"div", "scale_first", "swap", "f16", "cast"}:
        raise ConvertError(f"unknown hard-swish spelling {spell_hswish!r}")
    g = ox.Graph(name="birda_conv_stack", producer="birda_amd.convert")
    if frontend_spelling is None:
        g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", len(m.branches), m.spec_h, m.spec_w]))
    else:
        g.inputs.append(ox.ValueInfo("audio", ox.FLOAT, ["N", m.sample_count]))
        frontend_nodes(g, m, frontend_spelling)
    names = {0: "spectrogram"}
    flat = set()   # tensors that are [N, C] (after Flatten)

    def const(name: str, arr) -> str:
        g.initializers[name] = np.asarray(arr, np.float32)
        return name

    def activation(x: str, act: int, tag: str) -> str:
        if act == mf.ACT_NONE:
            return x
        if act == mf.ACT_RELU:
            g.nodes.append(ox.Node("Relu", [x], [tag + "_relu"]))
            return tag + "_relu"
        if act == mf.ACT_RELU6:
            g.nodes.append(ox.Node("Clip", [x, const(tag + "_min", 0.0), const(tag + "_max", 6.0)], [tag + "_relu6"]))
            return tag + "_relu6"
        if act == mf.ACT_SWISH:
            g.nodes.append(ox.Node("Sigmoid", [x], [tag + "_sig"]))
            g.nodes.append(ox.Node("Mul", [x, tag + "_sig"], [tag + "_swish"]))
            return tag + "_swish"
        if act == mf.ACT_SIGMOID:
            g.nodes.append(ox.Node("Sigmoid", [x], [tag + "_gate"]))
            return tag + "_gate"
        if act == mf.ACT_GELU_ERF:
            if spell_gelu == "gelu":
                g.nodes.append(ox.Node("Gelu", [x], [tag + "_gelu"], {"approximate": "none"}))
                return tag + "_gelu"
            g.nodes.append(ox.Node("Div", [x, const(tag + "_sqrt2", np.float32(SQRT2))], [tag + "_d"]))
            g.nodes.append(ox.Node("Erf", [tag + "_d"], [tag + "_e"]))
            g.nodes.append(ox.Node("Add", [tag + "_e", const(tag + "_one", 1.0)], [tag + "_a"]))
            g.nodes.append(ox.Node("Mul", [x, tag + "_a"], [tag + "_m"]))
            g.nodes.append(ox.Node("Mul", [tag + "_m", const(tag + "_half", 0.5)], [tag + "_gelu"]))
            return tag + "_gelu"
        if act in (mf.ACT_HSWISH, mf.ACT_HSIGMOID):
            return hard_activation(x, act == mf.ACT_HSWISH, tag)
        if act == mf.ACT_GELU_TANH:      # (opset 20's node is its one spelling either reader knows)
            g.nodes.append(ox.Node("Gelu", [x], [tag + "_gelu"], {"approximate": "tanh"}))
            return tag + "_gelu"
        raise ConvertError(f"activation {act} has no ONNX spelling here")

    def hard_activation(x: str, swish: bool, tag: str) -> str:
        def binary(op, a, b, out):
            g.nodes.append(ox.Node(op, [b, a] if "swap" in hs_opts and op != "Div" else [a, b], [out]))
            return out

        def hconst(name, v):
            g.initializers[name] = np.asarray(v, np.float16 if "f16" in hs_opts else np.float32)
            return name

        def cast(y):
            if "cast" not in hs_opts:
                return y
            g.nodes.append(ox.Node("Cast", [y], [y + "_c"], {"to": ox.FLOAT}))
            return y + "_c"
        sixth = {"alpha": float(np.float32(1.0 / 6.0)), "beta": 0.5}
        if hs_kind == "op" and swish:
            g.nodes.append(ox.Node("HardSwish", [x], [tag + "_hswish"]))
            return tag + "_hswish"
        if hs_kind in ("op", "hsigmoid"):
            g.nodes.append(ox.Node("HardSigmoid", [x], [tag + "_hsig"], dict(sixth)))
            return binary("Mul", x, cast(tag + "_hsig"), tag + "_hswish") if swish else tag + "_hsig"
        y = binary("Add", x, hconst(tag + "_three", 3.0), tag + "_p3")
        g.nodes.append(ox.Node("Clip", [y, hconst(tag + "_min", 0.0), hconst(tag + "_max", 6.0)], [tag + "_r6"]))
        y = cast(tag + "_r6")

        def scale(y, out):
            if "div" in hs_opts:
                return binary("Div", y, hconst(tag + "_six", 6.0), out)
            return binary("Mul", y, hconst(tag + "_sixth", 1.0 / 6.0), out)
        if not swish:
            return scale(y, tag + "_hsig")
        if "scale_first" in hs_opts:
            return binary("Mul", x, scale(y, tag + "_hs6"), tag + "_hswish")
        return scale(binary("Mul", x, y, tag + "_hsx"), tag + "_hswish")

    for i, L in enumerate(m.layers):
        tag, x = f"l{i}", names[L.in_tensor]
        if L.op in (mf.OP_CONV, mf.OP_DWCONV, mf.OP_PWCONV, mf.OP_GCONV):
            if L.op == mf.OP_GCONV:      # compact [kh][kw][cin / G][cout] -> ONNX [cout][cin / G][kh][kw]
                gi = L.cin // L.reserved
                w = m.weight(L.w_off, L.kh * L.kw * gi * L.cout).reshape(L.kh, L.kw, gi, L.cout).transpose(3, 2, 0, 1)
                group = L.reserved
            elif L.op == mf.OP_CONV:
                w = m.weight(L.w_off, L.kh * L.kw * L.cin * L.cout).reshape(L.kh, L.kw, L.cin, L.cout).transpose(3, 2, 0, 1)
                group = 1
            elif L.op == mf.OP_DWCONV:
                w = m.weight(L.w_off, L.kh * L.kw * L.cout).reshape(L.kh, L.kw, L.cout).transpose(2, 0, 1)[:, None]
                group = L.cout
            else:
                w = m.weight(L.w_off, L.cin * L.cout).reshape(L.cin, L.cout).T[:, :, None, None]
                group = 1
            # (a dilated layer -- OP_CONV on an NHWC tensor, OP_DWCONV -- spans (k - 1) dil + 1 pixels; either reader reads the attribute back)
            pad_b = max((L.out_h - 1) * L.sh + (L.kh - 1) * L.dil_h + 1 - L.in_h - L.pad_t, 0)
            pad_r = max((L.out_w - 1) * L.sw + (L.kw - 1) * L.dil_w + 1 - L.in_w - L.pad_l, 0)
            g.nodes.append(ox.Node("Conv", [x, const(tag + "_w", w), const(tag + "_b", m.weight(L.b_off, L.cout))], [tag + "_conv"],
                                   {"group": group, "kernel_shape": [L.kh, L.kw], "strides": [L.sh, L.sw],
                                    "pads": [L.pad_t, L.pad_l, pad_b, pad_r], "dilations": [L.dil_h, L.dil_w]}, name=tag))
            y = tag + "_conv"
            if L.res_tensor != mf.NO_TENSOR and L.reserved == mf.RES_ACT_AFTER and L.op != mf.OP_DWCONV:
                # act(conv + residual), the end of a ResNet block: Conv -> Add -> activation
                g.nodes.append(ox.Node("Add", [y, names[L.res_tensor]], [tag + "_res"]))
                y = activation(tag + "_res", L.act, tag)
            elif L.res_tensor != mf.NO_TENSOR:   # our executor: act(conv) + residual
                y = activation(y, L.act, tag)
                g.nodes.append(ox.Node("Add", [y, names[L.res_tensor]], [tag + "_res"]))
                y = tag + "_res"
            else:
                y = activation(y, L.act, tag)
        elif L.op == mf.OP_GAP:
            g.nodes.append(ox.Node("GlobalAveragePool", [x], [tag + "_gap"]))
            feeds_conv = any(M.in_tensor == i + 1 and M.op in (mf.OP_PWCONV, mf.OP_LNORM) for M in m.layers)
            if feeds_conv:       # squeeze-excite: the pooled [N, C, 1, 1] map goes on through 1x1 convolutions (ConvNeXt's head: through a LayerNorm)
                y = tag + "_gap"
            else:
                g.nodes.append(ox.Node("Flatten", [tag + "_gap"], [tag + "_flat"], {"axis": 1}))
                y = tag + "_flat"
                flat.add(i + 1)
        elif L.op == mf.OP_SCALE:
            g.nodes.append(ox.Node("Mul", [x, names[L.res_tensor]], [tag + "_se"]))
            y = tag + "_se"
        elif L.op == mf.OP_POOL:
            # explicit pads: the bottom / right ones are the smallest that give out_h, out_w in floor mode
            pad_b = max((L.out_h - 1) * L.sh + L.kh - L.in_h - L.pad_t, 0)
            pad_r = max((L.out_w - 1) * L.sw + L.kw - L.in_w - L.pad_l, 0)
            if ((L.in_h + L.pad_t + pad_b - L.kh) // L.sh + 1, (L.in_w + L.pad_l + pad_r - L.kw) // L.sw + 1) != (L.out_h, L.out_w):
                raise ConvertError(f"layer {i}: a pool whose output is cropped has no ONNX spelling")
            attrs = {"kernel_shape": [L.kh, L.kw], "strides": [L.sh, L.sw], "pads": [L.pad_t, L.pad_l, pad_b, pad_r]}
            if L.reserved != mf.POOL_MAX:
                attrs["count_include_pad"] = 1 if L.reserved == mf.POOL_AVG_PAD else 0
            g.nodes.append(ox.Node("MaxPool" if L.reserved == mf.POOL_MAX else "AveragePool", [x], [tag + "_pool"], attrs, name=tag))
            y = tag + "_pool"
        elif L.op == mf.OP_CONCAT:
            # Slice (a window that is not its whole source) + Concat (two sources, or one that is neither sliced nor shuffled) + the
            # three nodes of the channel shuffle: what either reader turns back into this record
            parts = []
            for side, t_src, off, n_ch in (("a", L.in_tensor, L.w_off, L.cin), ("b", L.res_tensor, L.b_off, L.cout - L.cin)):
                if t_src == mf.NO_TENSOR:
                    continue
                if t_src == 0:
                    raise ConvertError(f"layer {i}: a concat of the spectrogram has no ONNX spelling here")
                if off == 0 and n_ch == m.layers[t_src - 1].cout:
                    parts.append(names[t_src])
                    continue
                cut = f"{tag}_{side}"
                for suffix, v in (("starts", off), ("ends", off + n_ch), ("axes", 1)):
                    g.initializers[f"{cut}_{suffix}"] = np.asarray([v], np.int64)
                g.nodes.append(ox.Node("Slice", [names[t_src], cut + "_starts", cut + "_ends", cut + "_axes"], [cut], name=cut))
                parts.append(cut)
            y = parts[0]
            # (a lone Slice that only concats read would be folded into their windows: a one-input Concat keeps it a record)
            only_concats = all(M.op == mf.OP_CONCAT for M in m.layers if i + 1 in (M.in_tensor, M.res_tensor))
            if len(parts) == 2 or (L.reserved <= 1 and (y == names[L.in_tensor] or only_concats)):
                if spell_concat == "list" and len(parts) == 2 and L.reserved <= 1:
                    if parts[0] == names[L.in_tensor] and L.in_tensor in cat_parts:
                        parts = cat_parts[L.in_tensor] + parts[1:]
                    cat_parts[i + 1] = list(parts)
                g.nodes.append(ox.Node("Concat", parts, [tag + "_cat"], {"axis": 1}, name=tag))
                y = tag + "_cat"
            if L.reserved > 1:
                g.initializers[tag + "_s5"] = np.asarray([0, L.reserved, L.cout // L.reserved, L.out_h, L.out_w], np.int64)
                g.initializers[tag + "_s4"] = np.asarray([0, L.cout, L.out_h, L.out_w], np.int64)
                g.nodes.append(ox.Node("Reshape", [y, tag + "_s5"], [tag + "_r5"], name=tag + "_shuffle"))
                g.nodes.append(ox.Node("Transpose", [tag + "_r5"], [tag + "_tr"], {"perm": [0, 2, 1, 3, 4]}))
                g.nodes.append(ox.Node("Reshape", [tag + "_tr", tag + "_s4"], [tag + "_shuffled"]))
                y = tag + "_shuffled"
        elif L.op == mf.OP_LNORM:
            # the channel LayerNorm as PyTorch exports it from opset 17: on the [N, H, W, C] view between two Transposes (a 1 x 1 image too)
            if L.in_tensor == 0:
                raise ConvertError(f"layer {i}: a LayerNorm of the spectrogram has no ONNX spelling here")
            g.nodes.append(ox.Node("Transpose", [x], [tag + "_nhwc"], {"perm": [0, 2, 3, 1]}))
            ga, be = const(tag + "_gamma", m.weight(L.w_off, L.cout)), const(tag + "_beta", m.weight(L.b_off, L.cout))
            if spell_lnorm == "node":
                g.nodes.append(ox.Node("LayerNormalization", [tag + "_nhwc", ga, be], [tag + "_ln"], {"axis": -1, "epsilon": mf.lnorm_eps(L.reserved)}, name=tag))
            else:
                v = tag + "_nhwc"
                for o, ins, out, attrs in (("ReduceMean", [v], "_mu", {"axes": [-1], "keepdims": 1}), ("Sub", [v, tag + "_mu"], "_d", {}),
                                           ("Pow", [tag + "_d", const(tag + "_two", 2.0)], "_d2", {}), ("ReduceMean", [tag + "_d2"], "_var", {"axes": [-1], "keepdims": 1}),
                                           ("Add", [tag + "_var", const(tag + "_eps", np.float32(mf.lnorm_eps(L.reserved)))], "_ve", {}), ("Sqrt", [tag + "_ve"], "_sd", {}),
                                           ("Div", [tag + "_d", tag + "_sd"], "_xh", {}), ("Mul", [tag + "_xh", ga], "_xg", {}), ("Add", [tag + "_xg", be], "_ln", {})):
                    g.nodes.append(ox.Node(o, ins, [tag + out], attrs, name=tag + out))
            g.nodes.append(ox.Node("Transpose", [tag + "_ln"], [tag + "_nchw"], {"perm": [0, 3, 1, 2]}))
            y = tag + "_nchw"
            if L.in_h * L.in_w == 1 and any(M.in_tensor == i + 1 and M.op == mf.OP_DENSE for M in m.layers):
                g.nodes.append(ox.Node("Flatten", [y], [tag + "_flat"], {"axis": 1}))
                y = tag + "_flat"
                flat.add(i + 1)
        elif L.op == mf.OP_BNACT:
            if L.in_tensor == 0:
                raise ConvertError(f"layer {i}: a norm + activation layer on the spectrogram has no ONNX spelling here")
            g.nodes.append(ox.Node("BatchNormalization", [x, const(tag + "_scale", m.weight(L.w_off, L.cout)), const(tag + "_shift", m.weight(L.b_off, L.cout)),
                                                          const(tag + "_mean", np.zeros(L.cout, np.float32)), const(tag + "_var", np.ones(L.cout, np.float32))],
                                   [tag + "_bn"], {"epsilon": 0.0}, name=tag))
            y = activation(tag + "_bn", L.act, tag)
        elif L.op == mf.OP_REDUCE:
            if L.in_tensor == 0:
                raise ConvertError(f"layer {i}: a reduction of the spectrogram has no ONNX spelling here")
            rk = rank.get(L.in_tensor, 4)
            rh, rw = L.kh > 1, L.kw > 1
            if rk == 4:
                axes = ([2] if rh else []) + ([3] if rw else [])
            elif rk == 3 and not (rh and rw):
                axes = [2]
            else:
                raise ConvertError(f"layer {i}: a reduction of a rank-{rk} tensor over {L.kh}x{L.kw} has no ONNX spelling")
            if "neg" in red_opts:
                axes = [a - rk for a in axes]
            keep = 1 if "keep" in red_opts else 0

            def reduce_node(op, out):
                if op == "ReduceMax" and "gmp" in red_opts and rk == 4 and rh and rw and L.reserved == mf.REDUCE_MAX:
                    g.nodes.append(ox.Node("GlobalMaxPool", [x], [out], name=out))
                    return 1
                if op == "ReduceMax" and "argmax" in red_opts:
                    g.nodes.append(ox.Node("ArgMax", [x], [out + "_idx"], {"axis": axes[0], "keepdims": keep}, name=out + "_idx"))
                if "input" in red_opts:
                    g.initializers[out + "_axes"] = np.asarray(axes, np.int64)
                    g.nodes.append(ox.Node(op, [x, out + "_axes"], [out], {"keepdims": keep}, name=out))
                else:
                    g.nodes.append(ox.Node(op, [x], [out], {"axes": list(axes), "keepdims": keep}, name=out))
                return keep
            if L.reserved == mf.REDUCE_MAXMEAN:
                reduce_node("ReduceMax", tag + "_max")
                kept = reduce_node("ReduceMean", tag + "_mean")
                g.nodes.append(ox.Node("Add", [tag + "_mean", tag + "_max"] if "swap" in red_opts else [tag + "_max", tag + "_mean"], [tag + "_red"], name=tag))
                y = tag + "_red"
            else:
                y = tag + "_red"
                kept = reduce_node("ReduceMax" if L.reserved == mf.REDUCE_MAX else "ReduceMean", y)
            rk_out = rk if kept else rk - len(axes)
            if rk_out != 4:
                rank[i + 1] = rk_out
            if L.out_h * L.out_w == 1:
                feeds_conv = any(M.in_tensor == i + 1 and M.op in (mf.OP_PWCONV, mf.OP_LNORM) for M in m.layers)
                if feeds_conv and rk_out != 4:
                    raise ConvertError(f"layer {i}: a rank-{rk_out} tensor in front of a 1x1 convolution or a LayerNorm has no ONNX spelling here")
                if not feeds_conv and rk_out != 2:
                    g.nodes.append(ox.Node("Flatten", [y], [tag + "_flat"], {"axis": 1}))
                    y = tag + "_flat"
                if not feeds_conv:
                    flat.add(i + 1)
        elif L.op == mf.OP_DENSE:
            w = m.weight(L.w_off, L.cin * L.cout).reshape(L.cin, L.cout)
            g.nodes.append(ox.Node("Gemm", [x, const(tag + "_w", w), const(tag + "_b", m.weight(L.b_off, L.cout))], [tag + "_fc"],
                                   {"alpha": 1.0, "beta": 1.0, "transB": 0}))
            y = activation(tag + "_fc", L.act, tag)
            flat.add(i + 1)
        else:
            raise ConvertError(f"layer {i}: op {L.op}")
        names[i + 1] = y
    out = names[len(m.layers)]
    if m.output_activation == mf.OUT_SIGMOID:
        g.nodes.append(ox.Node("Sigmoid", [out], ["probabilities"]))
        out = "probabilities"
    elif m.output_activation == mf.OUT_SOFTMAX:
        g.nodes.append(ox.Node("Softmax", [out], ["probabilities"], {"axis": -1}))
        out = "probabilities"
    g.outputs.append(ox.ValueInfo(out, ox.FLOAT, ["N", m.n_classes]))
    return g


def model_to_onnx(m: mf.Model, spell_gelu: str = "erf", frontend_spelling: Optional[str] = None, spell_hswish: str = "op",
                  spell_lnorm: str = "node", spell_reduce: str = "", spell_concat: str = "pair") -> bytes:
    """`graph_from_model` serialised: the bytes of the `.onnx` file `bh_classifier_create` opens."""
    return ox.dump(graph_from_model(m, spell_gelu, frontend_spelling, spell_hswish, spell_lnorm, spell_reduce, spell_concat))


# ---------------------------------------------------------------------------------------
# ONNX -> model
# ---------------------------------------------------------------------------------------
class _Blob:
    def __init__(self, seed: Optional[np.ndarray] = None):
        self.chunks: List[np.ndarray] = [] if seed is None or seed.size == 0 else [np.asarray(seed, np.float32).ravel()]
        self.off = sum(c.size for c in self.chunks)

    def put(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a, np.float32).ravel()
        pad = (-self.off) % 16      # 64-B alignment: 16-B vector loads on the device
        if pad:
            self.chunks.append(np.zeros(pad, np.float32))
            self.off += pad
        off = self.off
        self.chunks.append(a)
        self.off += a.size
        return off

    def array(self) -> np.ndarray:
        return np.concatenate(self.chunks) if self.chunks else np.zeros(0, np.float32)


def _scalar(g: ox.Graph, name: str) -> Optional[float]:
    a = g.initializers.get(name)
    return float(a.reshape(-1)[0]) if a is not None and a.size == 1 else None


def _scalar_is_f16(g: ox.Graph, name: str) -> bool:
    a = g.initializers.get(name)
    return a is not None and a.dtype == np.float16


def _see_through_casts(g: ox.Graph, front_nodes: set) -> ox.Graph:
    """Cast between floating types is the identity (a float16 constant is the exact real number it encodes; the graph is evaluated
    in the library's own arithmetic): behind the front-end every such node is dropped and its output renamed to its input everywhere
    -- consumers and graph outputs -- so the sole-consumer / pattern logic sees through it.  Any other target is refused by name.
    The csrc/onnx_conv.hpp walk does the same.  Returns a new graph (nodes copied, initializers shared); front-end nodes untouched."""
    alias: Dict[str, str] = {}
    nodes = []
    for i, n in enumerate(g.nodes):
        if i in front_nodes:
            nodes.append(n)
            continue
        ins = [alias.get(x, x) for x in n.inputs]
        if n.op_type == "Cast":
            to = int(n.attrs.get("to", 0))
            if to not in FLOAT_CASTS:
                raise ConvertError(f"Cast {n.name!r} to {ox._TYPE_NAMES.get(to, 'element type ' + str(to))} (to = {to}): only casts between "
                                   "float32, float16 and float64 are read, as the identity")
            alias[n.outputs[0]] = ins[0]
            continue
        nodes.append(ox.Node(n.op_type, ins, list(n.outputs), n.attrs, n.name))
    outs = [ox.ValueInfo(alias.get(o.name, o.name), o.elem_type, o.shape) for o in g.outputs]
    return ox.Graph(nodes, g.initializers, g.inputs, outs, g.name, g.opset, g.producer)


# The hard sigmoid the kernels compute is PyTorch's, min(max(x / 6 + 1/2, 0), 1): alpha within 1e-6 of 1/6 and beta = 0.5 (the ONNX
# defaults, alpha = 0.2 and beta = 0.5, are Keras's: another function, refused by name).  The decomposed spelling's 1/6 is held to
# 1e-6 from a float32 constant and must BE the float16 rounding of 1/6 from a float16 one.
SIXTH_F16 = float(np.float16(1.0 / 6.0))


def _hsig_params(n: ox.Node) -> Tuple[float, float]:
    return float(np.float32(n.attrs.get("alpha", 0.2))), float(np.float32(n.attrs.get("beta", 0.5)))


def _hsig_is_torch(n: ox.Node) -> bool:
    alpha, beta = _hsig_params(n)
    return abs(alpha - 1.0 / 6.0) <= 1e-6 and beta == 0.5


def _fscalar(g: ox.Graph, name: str) -> Optional[float]:
    """_scalar for a float32 or float16 initializer only (what csrc/onnx_conv.hpp's scalar() reads)"""
    a = g.initializers.get(name)
    return float(a.reshape(-1)[0]) if a is not None and a.size == 1 and a.dtype in (np.float32, np.float16) else None


def _clip_is_relu6(g: ox.Graph, n: ox.Node) -> bool:
    lo = _fscalar(g, n.inputs[1]) if len(n.inputs) > 1 and n.inputs[1] else n.attrs.get("min")
    hi = _fscalar(g, n.inputs[2]) if len(n.inputs) > 2 and n.inputs[2] else n.attrs.get("max")
    return lo is not None and hi is not None and float(lo) == 0.0 and float(hi) == 6.0


def _collapse_activations(g: ox.Graph, front_nodes=frozenset()):
    """Find the multi-node activation spellings.  Returns (skip: set of node indices,
    act_of: {final output name: (input name, ACT, the pattern's own node indices)})."""
    graph_out = {o.name for o in g.outputs}
    prod = {o: i for i, n in enumerate(g.nodes) for o in n.outputs}
    cons: Dict[str, List[int]] = {}
    for i, n in enumerate(g.nodes):
        for x in n.inputs:
            cons.setdefault(x, []).append(i)
    skip, act_of = set(), {}

    def sole_consumer(name: str, op: str) -> Optional[int]:
        c = cons.get(name, [])
        return c[0] if len(c) == 1 and g.nodes[c[0]].op_type == op else None

    for i, n in enumerate(g.nodes):
        if n.op_type == "Erf":
            # x / sqrt2 (or x * (1/sqrt2)) -> Erf -> + 1 -> * x, * 0.5 (either order)
            j = prod.get(n.inputs[0])
            if j is None or g.nodes[j].op_type not in ("Div", "Mul"):
                continue
            pre = g.nodes[j]
            cst = [(_scalar(g, a), _scalar_is_f16(g, a), b, side) for side, (a, b) in enumerate(((pre.inputs[1], pre.inputs[0]), (pre.inputs[0], pre.inputs[1])))]
            x = None
            for c, c16, other, _ in cst:
                if c is None:
                    continue
                # a float32 constant is held to sqrt 2 at 1e-4; a float16 one must BE the float16 rounding of the expected value
                is_sqrt2 = c == SQRT2_F16 if c16 else abs(c - SQRT2) < 1e-4
                is_rsqrt2 = c == RSQRT2_F16 if c16 else abs(c - 1 / SQRT2) < 1e-4
                if (pre.op_type == "Div" and is_sqrt2) or (pre.op_type == "Mul" and is_rsqrt2):
                    x = other
            k = sole_consumer(n.outputs[0], "Add")
            if x is None or k is None:
                continue
            add = g.nodes[k]
            if not any(abs((_scalar(g, a) or 0.0) - 1.0) < 1e-6 for a in add.inputs):
                continue
            m1 = sole_consumer(add.outputs[0], "Mul")
            if m1 is None:
                continue
            m2 = sole_consumer(g.nodes[m1].outputs[0], "Mul")
            if m2 is None:
                continue
            others = [a for a in g.nodes[m1].inputs if a != add.outputs[0]] + [a for a in g.nodes[m2].inputs if a != g.nodes[m1].outputs[0]]
            has_x = x in others
            has_half = any(abs((_scalar(g, a) or 0.0) - 0.5) < 1e-6 for a in others)
            if has_x and has_half:
                skip |= {j, i, k, m1, m2}
                act_of[g.nodes[m2].outputs[0]] = (x, mf.ACT_GELU_ERF, (j, i, k, m1, m2))
        elif n.op_type == "Sigmoid":
            k = sole_consumer(n.outputs[0], "Mul")
            if k is not None and n.inputs[0] in g.nodes[k].inputs:
                skip |= {i, k}
                act_of[g.nodes[k].outputs[0]] = (n.inputs[0], mf.ACT_SWISH, (i, k))
        elif n.op_type == "HardSigmoid" and i not in front_nodes and n.inputs and n.outputs and _hsig_is_torch(n):
            # HardSigmoid(x) * x, PyTorch's hard swish below opset 14: folded like Sigmoid * x.  (Without that Mul the node stays in
            # the walk: a squeeze-excite gate or a refusal; any other alpha / beta is refused there by name.)
            k = sole_consumer(n.outputs[0], "Mul")
            if k is not None and n.outputs[0] not in graph_out and n.inputs[0] in g.nodes[k].inputs and g.nodes[k].outputs:
                skip |= {i, k}
                act_of[g.nodes[k].outputs[0]] = (n.inputs[0], mf.ACT_HSWISH, (i, k))
        elif n.op_type == "Add" and len(n.inputs) == 2 and n.outputs and i not in skip and i not in front_nodes:
            # The decomposed hard swish of tf2onnx and older exporters: Add(x, 3) -> Clip(0, 6) -> Mul(., x) and Mul(., 1/6) or
            # Div(., 6), the last two in either order; without the Mul(., x) it is the hard sigmoid (legal on a pooled tensor only:
            # set_act).  Every inner tensor has exactly one reader and is no graph output.  A chain that matches only in part is left
            # alone: its nodes meet the walk's own rules (Clip alone is ReLU6, a bare Add a residual).
            x = None
            for side in range(2):
                if _fscalar(g, n.inputs[side]) == 3.0 and n.inputs[1 - side] not in g.initializers:
                    x = n.inputs[1 - side]
            k = sole_consumer(n.outputs[0], "Clip")
            if x is None or n.outputs[0] in graph_out or k is None or not g.nodes[k].outputs or not _clip_is_relu6(g, g.nodes[k]):
                continue
            own, cur, has_scale, has_x = [i, k], g.nodes[k].outputs[0], False, False
            for _ in range(2):
                c = cons.get(cur, [])
                if cur in graph_out or len(c) != 1:
                    break
                q = c[0]
                nq = g.nodes[q]
                if nq.op_type not in ("Mul", "Div") or len(nq.inputs) != 2 or not nq.outputs or q in skip:
                    break
                other = nq.inputs[1] if nq.inputs[0] == cur else nq.inputs[0]
                cv = _fscalar(g, other)
                if not has_scale and cv is not None and (
                        (nq.op_type == "Mul" and (cv == SIXTH_F16 if _scalar_is_f16(g, other) else abs(cv - 1.0 / 6.0) <= 1e-6)) or
                        (nq.op_type == "Div" and nq.inputs[0] == cur and cv == 6.0)):
                    has_scale = True
                elif not has_x and nq.op_type == "Mul" and other == x:
                    has_x = True
                else:
                    break
                own.append(q)
                cur = nq.outputs[0]
            if not has_scale:
                continue
            skip |= set(own)
            act_of[cur] = (x, mf.ACT_HSWISH if has_x else mf.ACT_HSIGMOID, tuple(own))
    return skip, act_of


LN_CHAIN = "ReduceMean -> Sub -> Pow(2) -> ReduceMean -> Add(eps) -> Sqrt -> Div -> Mul(gamma) -> Add(beta)"


def _reduce_axes(g: ox.Graph, n: ox.Node) -> Optional[List[int]]:
    axes = n.attrs.get("axes")
    if axes is None and len(n.inputs) > 1 and n.inputs[1]:
        axes = _const_ints(g, n.inputs[1])
    return None if axes is None else [int(a) for a in axes]


def _find_layer_norms(g: ox.Graph, skip: set, front_nodes: set, deferred: Optional[Dict[int, str]] = None) -> Dict[str, list]:
    """The decomposed LayerNorm torch.onnx emits below opset 17 (LN_CHAIN), over the last axis of an [N, H, W, C] view or over axis 1
    of an NCHW map: a ReduceMean over ONE axis (-1, 3 or 1) starts it, and a chain that deviates is refused by naming the node where
    it does (another exponent, another axis, a missing eps, a second reader of an inner tensor).  csrc/onnx_conv.hpp finds it the same
    way.  Returns {the chain's input: [(output name, gamma name, beta name, eps, axis, the ReduceMean's name)]}; the chain's nodes join
    `skip`.  A ReduceMean over the last axis (-1, 3) with no Sub(x, mean) behind it is no chain -- a reduction over W of an NCHW map, the
    walk's OP_REDUCE --; `deferred` receives node -> the refusal it stays on an [N, H, W, C] view, which the walk raises."""
    graph_out = {o.name for o in g.outputs}
    deferred = {} if deferred is None else deferred
    cons: Dict[str, List[int]] = {}
    for i, n in enumerate(g.nodes):
        if i in skip:
            continue
        for x in n.inputs:
            cons.setdefault(x, []).append(i)

    def dev(n: ox.Node, why: str):
        raise ConvertError(f"{n.op_type} {n.name!r}: not the LayerNorm chain {LN_CHAIN}: {why}")

    def only_reader(src: ox.Node, op: str) -> int:
        """the one reader of src's output, which must be an `op` node"""
        name = src.outputs[0]
        c = cons.get(name, [])
        if name in graph_out or len(c) != 1:
            dev(src, f"its output has {len(c)} readers{' and is a graph output' if name in graph_out else ''} (a second reader of an inner tensor)")
        if g.nodes[c[0]].op_type != op or not g.nodes[c[0]].outputs:
            dev(g.nodes[c[0]], f"{op} expected behind {src.op_type} {src.name!r}")
        return c[0]

    def other(n: ox.Node, name: str) -> str:
        if len(n.inputs) != 2 or name not in n.inputs:
            dev(n, "two operands expected")
        return n.inputs[1] if n.inputs[0] == name else n.inputs[0]

    found: Dict[str, list] = {}
    for i, n in enumerate(g.nodes):
        if n.op_type != "ReduceMean" or i in skip or i in front_nodes or not n.inputs or not n.outputs:
            continue
        axes = _reduce_axes(g, n)
        if axes is None or len(axes) != 1 or axes[0] not in (-1, 3, 1):
            continue                                           # (H, W: the global pool; anything else keeps the walk's refusal)
        x = n.inputs[0]
        if axes[0] != 1 and not any(g.nodes[q].op_type == "Sub" and x in g.nodes[q].inputs for q in cons.get(n.outputs[0], [])):
            try:
                if int(n.attrs.get("keepdims", 1)) != 1:
                    dev(n, "keepdims = 0")
                dev(g.nodes[only_reader(n, "Sub")], "Sub(x, mean) expected")
            except ConvertError as e:
                deferred[i] = str(e)
            continue
        if int(n.attrs.get("keepdims", 1)) != 1:
            dev(n, "keepdims = 0")
        j_sub = only_reader(n, "Sub")
        sub = g.nodes[j_sub]
        if list(sub.inputs) != [x, n.outputs[0]]:
            dev(sub, "Sub(x, mean) expected")
        rd = cons.get(sub.outputs[0], [])
        if sub.outputs[0] in graph_out or len(rd) != 2 or sorted(g.nodes[k].op_type for k in rd) != ["Div", "Pow"]:
            dev(sub, "its output must be read by the Pow and the Div alone (a second reader of an inner tensor)")
        j_pow, j_div = (rd if g.nodes[rd[0]].op_type == "Pow" else rd[::-1])
        pw, div = g.nodes[j_pow], g.nodes[j_div]
        if len(pw.inputs) != 2 or pw.inputs[0] != sub.outputs[0] or _fscalar(g, pw.inputs[1]) != 2.0:
            dev(pw, f"exponent {_fscalar(g, pw.inputs[1]) if len(pw.inputs) == 2 else None} (2 expected)")
        j_m2 = only_reader(pw, "ReduceMean")
        m2 = g.nodes[j_m2]
        if _reduce_axes(g, m2) != axes or int(m2.attrs.get("keepdims", 1)) != 1:
            dev(m2, f"axes {_reduce_axes(g, m2)} (the first mean is over {axes}: another axis)")
        c = cons.get(m2.outputs[0], [])
        if len(c) == 1 and g.nodes[c[0]].op_type == "Sqrt":
            dev(g.nodes[c[0]], "a missing eps (Add(variance, eps) expected in front of the Sqrt)")
        j_add = only_reader(m2, "Add")
        add = g.nodes[j_add]
        eps = _fscalar(g, other(add, m2.outputs[0]))
        if eps is None:
            dev(add, "a missing eps (a float32 or float16 scalar constant expected)")
        j_sqrt = only_reader(add, "Sqrt")
        sq = g.nodes[j_sqrt]
        if only_reader(sq, "Div") != j_div or list(div.inputs) != [sub.outputs[0], sq.outputs[0]]:
            dev(div, "Div(x - mean, sqrt) expected")
        j_mul = only_reader(div, "Mul")
        mul = g.nodes[j_mul]
        gamma = other(mul, div.outputs[0])
        j_add2 = only_reader(mul, "Add")
        add2 = g.nodes[j_add2]
        beta = other(add2, mul.outputs[0])
        for role, name, q in (("gamma", gamma, mul), ("beta", beta, add2)):
            a = g.initializers.get(name)
            if a is None or a.dtype not in (np.float32, np.float16):
                dev(q, f"{role} must be a float32 or float16 initializer")
        skip |= {i, j_sub, j_pow, j_m2, j_add, j_sqrt, j_div, j_mul, j_add2}
        found.setdefault(x, []).append((add2.outputs[0], gamma, beta, float(eps), axes[0], n.name))
    return found


def _const_ints(g: ox.Graph, name: str) -> Optional[List[int]]:
    """The integer list a node input names -- an initializer or a Constant node's value -- or None (at most 64 entries are read)"""
    a = g.initializers.get(name)
    if a is None:
        for n in g.nodes:
            if n.op_type == "Constant" and n.outputs and n.outputs[0] == name:
                v = n.attrs.get("value", n.attrs.get("value_ints", [n.attrs["value_int"]] if "value_int" in n.attrs else None))
                a = None if v is None else np.asarray(v)
    if a is None or a.dtype.kind not in "iu" or a.size > 64:
        return None
    return [int(v) for v in np.asarray(a).reshape(-1)]


def _find_shuffles(g: ox.Graph, skip: set, front_nodes: set):
    """The channel shuffle: Reshape [N, g, C / g, H, W] -> Transpose (0, 2, 1, 3, 4) -> Reshape [N, C, H, W], each with one reader,
    the shapes constants (csrc/onnx_conv.hpp finds it the same way).  Returns ({first Reshape's node index: (output name, shape 1,
    shape 2)}, the first Reshapes of patterns whose shapes are computed); the other two nodes of a found pattern join `skip`."""
    cons: Dict[str, List[int]] = {}
    for i, n in enumerate(g.nodes):
        for x in n.inputs:
            cons.setdefault(x, []).append(i)

    def sole_consumer(name: str, op: str) -> Optional[int]:
        c = cons.get(name, [])
        return c[0] if len(c) == 1 and g.nodes[c[0]].op_type == op else None

    found, computed = {}, set()
    for i, n in enumerate(g.nodes):
        if n.op_type != "Reshape" or i in skip or i in front_nodes or len(n.inputs) < 2 or not n.outputs:
            continue
        t = sole_consumer(n.outputs[0], "Transpose")
        if t is None or not g.nodes[t].outputs or t in skip or list(g.nodes[t].attrs.get("perm") or []) != [0, 2, 1, 3, 4]:
            continue
        r2 = sole_consumer(g.nodes[t].outputs[0], "Reshape")
        if r2 is None or len(g.nodes[r2].inputs) < 2 or not g.nodes[r2].outputs or r2 in skip:
            continue
        s1, s2 = _const_ints(g, n.inputs[1]), _const_ints(g, g.nodes[r2].inputs[1])
        if s1 is None or s2 is None:
            computed.add(i)
            continue
        found[i] = (g.nodes[r2].outputs[0], s1, s2)
        skip |= {t, r2}
    return found, computed


def _resolve_shape(shape: List[int], dims: List[int], total: int) -> Optional[List[int]]:
    """A Reshape's target with its 0 (copy the input's dimension) and -1 (whatever is left) entries resolved, the batch dimension
    aside: `dims` and the result hold the dimensions behind it.  None: not a shape of `total` elements."""
    out, known, infer = [], 1, -1
    for k in range(1, len(shape)):
        v = shape[k]
        if v == 0:
            if k - 1 >= len(dims):
                return None
            v = dims[k - 1]
        if v == -1:
            if infer >= 0 or shape[0] == -1:
                return None
            infer, v = len(out), 1
        elif v <= 0 or v > (1 << 24) or known > (1 << 40):
            return None
        else:
            known *= v
        out.append(v)
    if infer >= 0:
        if total % known:
            return None
        out[infer], known = total // known, total
    return out if known == total else None


_QUAD = "a channel count or offset that is not a multiple of 4 is not supported (ShuffleNetV2 x1.0's 58-channel halves, for one)"


def model_from_graph(g: ox.Graph, frontend: Optional[mf.Model] = None, spectrogram_input: Optional[str] = None,
                     sample_rate: Optional[int] = None, family: int = 0) -> mf.Model:
    """`frontend` supplies everything the conv stack does not say: family, sample rate / count, segment
    duration, normalisation eps, the STFT / mel branches and their mel weight matrices (its blob is kept as
    the start of the new blob, so `mel_w_off` stays valid).  Without one, the graph must start at the AUDIO input and the
    front-end is read off it by probing (`frontend_recover.recover_frontend`; `sample_rate` is then required: the graph does
    not state it, the reference takes it from the model type's config, src/inference/classifier.rs:360-377)."""
    for vi in list(g.inputs) + list(g.outputs):
        if vi.elem_type == ox.FLOAT16:
            raise ConvertError(f"graph {'input' if vi in g.inputs else 'output'} {vi.name!r} is float16: only float32 inputs are fed and "
                               "float32 outputs returned (a float16 file keeps float32 at both ends, behind / in front of a Cast)")
    if frontend is None:
        from .frontend_recover import RecoverError, recover_frontend
        if sample_rate is None:
            raise ConvertError("no front-end manifest: the sample rate must be given to read the front-end off the graph")
        try:
            rec = recover_frontend(g, sample_rate, family)
        except RecoverError as e:
            raise ConvertError(f"front-end not recoverable from the graph ({e}); pass a front-end manifest") from None
        frontend, spectrogram_input = rec.frontend, rec.spectrogram
    spec = spectrogram_input or (g.inputs[0].name if g.inputs else None)
    if spec is None:
        raise ConvertError("graph has no input")
    # nodes that produce the spectrogram (a graph that starts at the audio input) are the front-end, not layers
    def producers_of(gr: ox.Graph, tensor: str) -> set:
        prod = {o: i for i, n in enumerate(gr.nodes) for o in n.outputs}
        found, stack = set(), [tensor]
        while stack:
            i = prod.get(stack.pop())
            if i is None or i in found:
                continue
            found.add(i)
            stack.extend(gr.nodes[i].inputs)
        return found
    g = _see_through_casts(g, producers_of(g, spec))
    # the unused second output of torch.max(x, dim): an ArgMax none of whose outputs anything reads.  The walk ignores no other dead node
    # -- an operator it does not know is refused wherever it stands --, so this one is taken out by name, and is no reader of x.
    spec_nodes, read_names = producers_of(g, spec), {x for q in g.nodes for x in q.inputs} | {o.name for o in g.outputs}
    g.nodes[:] = [n for i, n in enumerate(g.nodes) if i in spec_nodes or n.op_type != "ArgMax" or any(o in read_names for o in n.outputs)]
    front_nodes = producers_of(g, spec)
    blob = _Blob(frontend.blob[: max((b.mel_w_off + b.n_bins * b.n_mels for b in frontend.branches), default=0)])
    layers: List[mf.Layer] = []
    # name -> (tensor index, C, H, W) ; H = W = 0 for flattened [N, C]
    tmap: Dict[str, Tuple[int, int, int, int]] = {spec: (0, len(frontend.branches), frontend.spec_h, frontend.spec_w)}
    skip, act_of = _collapse_activations(g, front_nodes)
    out_act, emb_tensor, emb_dim = mf.OUT_NONE, 0, 0
    graph_out = {o.name for o in g.outputs}

    sums = set()   # the outputs of the residual Adds folded into a layer
    r3: Dict[str, int] = {}   # the names that are rank-3 tensors behind a reduction with keepdims = 0 -- 1: [N, C, H] (W is gone), 2: [N, C, W]
    nhwc = set()   # the names that are [N, H, W, C] views of their tensor (behind Transpose [0, 2, 3, 1]): the library keeps activations NHWC
    NHWC_READERS = ("Transpose", "LayerNormalization", "MatMul", "Mul", "Relu", "Gelu", "Clip", "HardSwish")

    def set_act(name_in: str, name_out: str, act: int, own):
        """own: the node indices of the activation itself -- one, or a multi-node spelling's"""
        t = tmap.get(name_in)
        if t is None:
            raise ConvertError(f"activation on unknown tensor {name_in!r}")
        # (the hard sigmoid stands where the Sigmoid inside the graph may: on a pooled [N, C, 1, 1] tensor -- the gate's second 1x1, a dense layer)
        if act == mf.ACT_HSIGMOID and t[2] * t[3] != 1:
            raise ConvertError("HardSigmoid inside the graph that is neither HardSigmoid * x nor a squeeze-excite gate")
        L = layers[t[0] - 1] if t[0] > 0 else None
        if L is not None and L.op == mf.OP_POOL:
            raise ConvertError(f"activation after {name_in!r} cannot be folded into its producer: directly after a MaxPool / AveragePool "
                               "(a pool layer carries no activation)")
        if L is not None and L.op == mf.OP_CONCAT:
            raise ConvertError(f"activation after {name_in!r} cannot be folded into its producer: directly after a Concat, Split, Slice "
                               "or channel shuffle (the record carries no activation)")
        if L is not None and L.op == mf.OP_LNORM:
            raise ConvertError(f"activation after {name_in!r} cannot be folded into its producer: directly after a LayerNormalization "
                               "(the record carries no activation)")
        if L is not None and L.op == mf.OP_REDUCE:
            raise ConvertError(f"activation after {name_in!r} cannot be folded into its producer: directly after a ReduceMax / ReduceMean / "
                               "GlobalMaxPool (a reduce layer carries no activation)")
        if L is not None and L.op == mf.OP_BNACT:
            # the activation that completes a tentative norm + activation record (the BatchNormalization branch below); anything but one of
            # the record's activations as the ONLY reader of the norm's output leaves the norm where it was: refused, in the words stored
            if t[0] not in bn_pending:
                raise ConvertError(f"activation after {name_in!r} cannot be folded into its producer")
            if act not in mf.BNACT_ACTS or name_in in graph_out or any(name_in in q.inputs for k, q in enumerate(g.nodes) if k not in own):
                raise ConvertError(bn_pending[t[0]])
            del bn_pending[t[0]]
            L.act = act
            tmap[name_out] = t
            return
        if name_in in nhwc:
            nhwc.add(name_out)
        if L is not None and name_in in sums and L.res_tensor != mf.NO_TENSOR and L.reserved != mf.RES_ACT_AFTER:
            # act(conv + x), the end of a ResNet block: the layer keeps its one activation code and records its position
            if L.act != mf.ACT_NONE:
                raise ConvertError(f"activation after {name_in!r} cannot be folded into its producer: an activation on both sides of a "
                                   "residual Add (act2(act1(conv) + x))")
            if name_in in graph_out or any(name_in in q.inputs for k, q in enumerate(g.nodes) if k not in own):
                raise ConvertError(f"activation after {name_in!r} cannot be folded into its producer: the sum has another reader or is "
                                   "a graph output (it would be handed the activated tensor)")
            L.act, L.reserved = act, mf.RES_ACT_AFTER
            tmap[name_out] = t
            return
        if L is None or L.act != mf.ACT_NONE or L.res_tensor != mf.NO_TENSOR:
            raise ConvertError(f"activation after {name_in!r} cannot be folded into its producer")
        L.act = act
        tmap[name_out] = t

    bn_pending: Dict[int, str] = {}   # tensor of a norm + activation record that has no activation yet -> the refusal its BatchNormalization gets without one
    cat_lists: List[Tuple[tuple, tuple]] = []   # (the resolved input list of a Concat, its output tensor), in graph order: prefix reuse
    first_of_pattern = {}   # applied when the walk reaches the pattern's input (below)
    for out_name, (x, act, own) in act_of.items():
        first_of_pattern.setdefault(x, []).append((out_name, act, own))
    ln_deferred: Dict[int, str] = {}
    ln_of_pattern = _find_layer_norms(g, skip, front_nodes, ln_deferred)      # the decomposed LayerNorm chains, by their input

    def lnorm_rec(who: str, x_name: str, out_name: str, gamma, beta, eps: float):
        """one OP_LNORM record over the channels of tensor x_name (an [N, H, W, C] view, or an NCHW map the caller has held to the
        channel axis) -> out_name, a view when x_name is one; directly behind the global pool it becomes the embedding"""
        nonlocal emb_tensor
        t = tmap[x_name]
        if t[0] == 0:
            raise ConvertError(who + "a LayerNorm of the spectrogram (tensor 0) is not supported")
        C = t[1]
        if gamma.dtype not in (np.float32, np.float16) or gamma.size != C or (beta is not None and (beta.dtype not in (np.float32, np.float16) or beta.size != C)):
            raise ConvertError(who + f"gamma / beta must be float32 or float16 initializers of the {C} channels")
        if C % 4:
            raise ConvertError(who + f"{C} channels: a channel count that is not a multiple of 4 is not supported")
        e32 = np.float32(eps)
        if not np.isfinite(e32) or not e32 > 0:
            raise ConvertError(who + f"epsilon {eps!r} is not finite and > 0")
        bz = np.zeros(C, np.float32) if beta is None else beta.reshape(-1)
        layers.append(mf.Layer(mf.OP_LNORM, mf.ACT_NONE, t[0], mf.NO_TENSOR, C, C, 1, 1, 1, 1, 0, 0, t[2], t[3], t[2], t[3], 0,
                               blob.put(gamma.reshape(-1)), blob.put(bz), reserved=mf.lnorm_eps_bits(float(e32))))
        if layers[t[0] - 1].op in (mf.OP_GAP, mf.OP_REDUCE) and emb_tensor == t[0]:
            emb_tensor = len(layers)          # pool -> norm -> dense: the dense head reads the norm
        tmap[out_name] = (len(layers), C, t[2], t[3])
        if x_name in nhwc:
            nhwc.add(out_name)

    def flush_patterns(x: str):
        for out_name, act, own in first_of_pattern.pop(x, []):
            set_act(x, out_name, act, own)
        for out_name, gamma, beta, eps, axis, name in ln_of_pattern.pop(x, []):
            who = f"ReduceMean {name!r} (LayerNorm chain): "
            ga, be = g.initializers[gamma], g.initializers[beta]
            C = tmap[x][1]
            if x in nhwc:
                if axis not in (-1, 3):
                    raise ConvertError(who + f"axis {axis} of an [N, H, W, C] view: only the last axis, the channels, is normalised (another axis)")
                ok = ga.shape == (C,) and be.shape == (C,)
            else:
                if axis != 1:
                    raise ConvertError(who + f"axis {axis} of an NCHW tensor: only axis 1, the channels, is normalised (another axis)")
                ok = ga.shape in ((C, 1, 1), (1, C, 1, 1)) and be.shape in ((C, 1, 1), (1, C, 1, 1))
            if not ok:
                raise ConvertError(who + f"gamma / beta of shape {list(ga.shape)} / {list(be.shape)} do not scale the {C} channels")
            lnorm_rec(who, x, out_name, ga, be, eps)
            flush_patterns(out_name)

    shuffle_at, shuffle_computed = _find_shuffles(g, skip, front_nodes)
    prod_idx = {o: k for k, q in enumerate(g.nodes) for o in q.outputs}
    cons_idx: Dict[str, List[int]] = {}
    for k, q in enumerate(g.nodes):
        for x in q.inputs:
            cons_idx.setdefault(x, []).append(k)
    vmap: Dict[str, Tuple[int, int, int, int, int]] = {}   # the views: name -> (tensor, C, H, W, first channel); only Concat looks here
    readers: Dict[str, List[str]] = {}
    for q in g.nodes:
        for x in q.inputs:
            readers.setdefault(x, []).append(q.op_type)

    def concat_rec(a, b, groups: int):
        """one OP_CONCAT record: the window a = (tensor, C, H, W, first channel), then b's (None: a alone) -> its output, whole"""
        cout = a[1] + (b[1] if b else 0)
        layers.append(mf.Layer(mf.OP_CONCAT, mf.ACT_NONE, a[0], b[0] if b else mf.NO_TENSOR, a[1], cout, 1, 1, 1, 1, 0, 0, a[2], a[3], a[2], a[3],
                               0, a[4], b[4] if b else 0, reserved=groups))
        return (len(layers), cout, a[2], a[3])

    def publish_view(name: str, x, off: int, c: int):
        """an output of a Split / Slice: a view where only Concat nodes read it, else a record of its own that materialises it"""
        v = (x[0], c, x[2], x[3], off)
        if name in graph_out or any(o != "Concat" for o in readers.get(name, [])):
            tmap[name] = concat_rec(v, None, 0)
        else:
            vmap[name] = v

    def fold_layer_scale(n: ox.Node, view_in) -> bool:
        """Mul of a convolution's / MatMul layer's output by a constant of its C channels ([C] on an [N, H, W, C] view, [C, 1, 1] or
        [1, C, 1, 1] on an NCHW map): ConvNeXt's layer scale, folded into the layer's weight columns and bias where BatchNormalization
        is -- one float32 product each.  The layer has no activation and no residual yet, the Mul is its only reader and the tensor
        no graph output.  False: not that Mul (today's rules apply)."""
        if len(n.inputs) != 2 or not n.outputs:
            return False
        for x_name, s_name in ((n.inputs[0], n.inputs[1]), (n.inputs[1], n.inputs[0])):
            S, t = g.initializers.get(s_name), tmap.get(x_name)
            if S is None or t is None or t[0] == 0 or S.dtype not in (np.float32, np.float16):
                continue
            L, C = layers[t[0] - 1], t[1]
            shapes = ((C,),) if x_name in nhwc else ((C, 1, 1), (1, C, 1, 1))
            if S.shape not in shapes or L.op not in (mf.OP_CONV, mf.OP_DWCONV, mf.OP_PWCONV, mf.OP_GCONV) or L.act != mf.ACT_NONE or \
                    L.res_tensor != mf.NO_TENSOR or x_name in graph_out or sum(x_name in q.inputs for q in g.nodes) != 1:
                continue
            nw = {mf.OP_CONV: L.kh * L.kw * L.cin * L.cout, mf.OP_DWCONV: L.kh * L.kw * L.cout, mf.OP_PWCONV: L.cin * L.cout,
                  mf.OP_GCONV: L.kh * L.kw * (L.cin // max(L.reserved, 1)) * L.cout}[L.op]
            scale = S.reshape(-1).astype(np.float32)
            arr = blob.array()
            arr[L.w_off: L.w_off + nw] = (arr[L.w_off: L.w_off + nw].reshape(-1, L.cout) * scale).reshape(-1)   # cout is the last axis in every layout
            arr[L.b_off: L.b_off + L.cout] = arr[L.b_off: L.b_off + L.cout] * scale
            blob.chunks, blob.off = [arr], arr.size
            tmap[n.outputs[0]] = t
            if x_name in nhwc:
                nhwc.add(n.outputs[0])
            flush_patterns(n.outputs[0])
            return True
        if view_in is not None:
            raise ConvertError(f"Mul {n.name!r}: input {view_in!r} is an [N, H, W, C] view (behind a Transpose): only a Mul by a [C] constant "
                               "directly behind a MatMul layer without an activation, its only reader, is folded (layer scale)")
        return False

    for i, n in enumerate(g.nodes):
        if i in skip or i in front_nodes:
            continue
        op = n.op_type
        if op == "Constant":      # (the library's parser turns these into initializers; _const_ints reads them where they are)
            continue
        for x in n.inputs if bn_pending else ():
            if x in tmap and tmap[x][0] in bn_pending:
                relu6 = op == "Clip" and (_scalar(g, n.inputs[1]) if len(n.inputs) > 1 else n.attrs.get("min")) == 0.0 and \
                    (_scalar(g, n.inputs[2]) if len(n.inputs) > 2 else n.attrs.get("max")) == 6.0
                if not (op in ("Relu", "Gelu", "HardSwish") or relu6):
                    raise ConvertError(bn_pending[tmap[x][0]])
        view_in = next((x for x in n.inputs if x in nhwc), None)
        if view_in is not None and i in ln_deferred:
            raise ConvertError(ln_deferred[i])
        if view_in is not None and op not in NHWC_READERS:
            raise ConvertError(f"{op} {n.name!r}: input {view_in!r} is an [N, H, W, C] view (behind a Transpose): only LayerNormalization, "
                               "MatMul (+ Add of a bias), the activations, Mul by a [C] constant and the Transpose back read one")
        for x in n.inputs:
            if x in r3 and x in tmap and op not in ("ReduceMean", "ReduceMax", "Add", "Squeeze", "Unsqueeze", "Flatten", "Reshape"):
                raise ConvertError(f"{op} {n.name!r}: input {x!r} is a rank-3 tensor [N, C, T] (behind a reduction with keepdims = 0): only further "
                                   "reductions, the max + mean Add, and Squeeze / Unsqueeze / Flatten / Reshape once one pixel is left read one "
                                   "(1-D convolutions and pools are not supported)")
        if op == "Transpose":
            # the library keeps activations NHWC: [0, 2, 3, 1] marks the result an [N, H, W, C] view of the same tensor, [0, 3, 1, 2] ends it
            who = f"Transpose {n.name!r}: "
            perm = [int(v) for v in (n.attrs.get("perm") or [])]
            t = tmap.get(n.inputs[0])
            if t is None:
                raise ConvertError(who + f"input {n.inputs[0]!r} is not on the path from {spec!r}")
            if perm == [0, 2, 3, 1] and view_in is None:
                if t[0] == 0:
                    raise ConvertError(who + "an [N, H, W, C] view of the spectrogram (tensor 0) is not supported")
                nhwc.add(n.outputs[0])
            elif not (perm == [0, 3, 1, 2] and view_in is not None):
                raise ConvertError(who + f"perm {perm} on {'an [N, H, W, C] view' if view_in is not None else 'an NCHW feature map'}: only "
                                   "[0, 2, 3, 1] on a feature map and [0, 3, 1, 2] on the view it makes are read")
            tmap[n.outputs[0]] = t
            flush_patterns(n.outputs[0])
        elif op == "LayerNormalization":
            who = f"LayerNormalization {n.name!r}: "
            t = tmap.get(n.inputs[0])
            if t is None:
                raise ConvertError(who + f"input {n.inputs[0]!r} is not on the path from {spec!r}")
            axis = int(n.attrs.get("axis", -1))
            if view_in is not None:
                if axis not in (-1, 3):
                    raise ConvertError(who + f"axis {axis} of an [N, H, W, C] view: only the last axis, the channels, is normalised")
            elif axis != 1 or t[2] * t[3] != 1:
                raise ConvertError(who + f"axis {axis} of an NCHW tensor with a {t[2]}x{t[3]} image: it would normalise over more than the "
                                   "channels (only axis 1 of an [N, C, 1, 1] tensor, or the last axis of an [N, H, W, C] view)")
            for k, what in ((1, "Mean"), (2, "InvStdDev")):
                if len(n.outputs) > k and n.outputs[k] and (n.outputs[k] in graph_out or readers.get(n.outputs[k])):
                    raise ConvertError(who + f"the output {what} is read: only the normalised tensor is computed")
            ga = g.initializers.get(n.inputs[1]) if len(n.inputs) > 1 else None
            be = g.initializers.get(n.inputs[2]) if len(n.inputs) > 2 and n.inputs[2] else None
            if ga is None or (len(n.inputs) > 2 and n.inputs[2] and be is None):
                raise ConvertError(who + f"gamma / beta must be float32 or float16 initializers of the {t[1]} channels")
            lnorm_rec(who, n.inputs[0], n.outputs[0], ga, be, float(np.float32(n.attrs.get("epsilon", 1e-5))))
            flush_patterns(n.outputs[0])
        elif op == "MatMul" and view_in is not None:
            # a pointwise layer on the [N, H, W, C] view (a PyTorch Linear between two Transposes), with its Add of a bias
            who = f"MatMul {n.name!r}: "
            if view_in != n.inputs[0]:
                raise ConvertError(who + f"the [N, H, W, C] view {view_in!r} as the second operand")
            t = tmap[n.inputs[0]]
            W = g.initializers.get(n.inputs[1])
            if W is None or W.ndim != 2 or W.dtype not in (np.float32, np.float16):
                raise ConvertError(who + "needs a 2-d float32 or float16 weight initializer")
            cin, cout = W.shape
            if cin != t[1]:
                raise ConvertError(who + f"{cin} input features, activation has {t[1]}")
            B, out = None, n.outputs[0]
            nxt = [k for k, nn in enumerate(g.nodes) if out in nn.inputs]
            if len(nxt) == 1 and g.nodes[nxt[0]].op_type == "Add" and len(g.nodes[nxt[0]].inputs) == 2 and out not in graph_out:
                o2 = [a for a in g.nodes[nxt[0]].inputs if a != out]
                ob = g.initializers.get(o2[0]) if o2 else None
                if ob is not None and ob.dtype in (np.float32, np.float16) and ob.size == cout:
                    B, out = ob, g.nodes[nxt[0]].outputs[0]
                    skip.add(nxt[0])
            layers.append(mf.Layer(mf.OP_PWCONV, mf.ACT_NONE, t[0], mf.NO_TENSOR, cin, cout, 1, 1, 1, 1, 0, 0, t[2], t[3], t[2], t[3], 0,
                                   blob.put(W), blob.put(np.zeros(cout, np.float32) if B is None else B.reshape(-1))))
            tmap[out] = (len(layers), cout, t[2], t[3])
            nhwc.add(out)
            flush_patterns(out)
        elif op == "Mul" and fold_layer_scale(n, view_in):
            pass
        elif op == "Concat":
            who = f"Concat {n.name!r}: "
            if len(n.inputs) > 64:
                raise ConvertError(who + f"{len(n.inputs)} inputs (1 .. 64 are read)")
            axis = int(n.attrs.get("axis", 0))
            if axis not in (1, -3):
                raise ConvertError(who + f"axis {axis}: only the channel axis (1, or -3) is concatenated")
            src = []
            for name in n.inputs:
                if name in g.initializers or any(q.op_type == "Constant" and name in q.outputs for q in g.nodes):
                    raise ConvertError(who + f"input {name!r} is a constant: only activations are concatenated")
                x = vmap.get(name) or (tmap[name] + (0,) if name in tmap else None)
                if x is None:
                    raise ConvertError(who + f"input {name!r} is not on the path from {spec!r}")
                if x[0] == 0:
                    raise ConvertError(who + "the spectrogram (tensor 0) as an input is not supported")
                if src and x[2:4] != src[0][2:4]:
                    raise ConvertError(who + f"inputs of different images ({src[0][2]}x{src[0][3]} and {x[2]}x{x[3]})")
                if x[1] % 4 or x[4] % 4:
                    raise ConvertError(who + f"input {name!r} is {x[1]} channels from channel {x[4]}: " + _QUAD)
                src.append(x)
            if sum(x[1] for x in src) > 65536:
                raise ConvertError(who + "more than 65 536 channels")
            # prefix reuse (a DenseNet layer's Concat over the whole list of earlier features): where the leading j >= 2 inputs are, in order,
            # the complete input list of an earlier Concat whose output is still a plain whole tensor, the chain starts from that output
            # (the longest such prefix; j < the inputs, so that a Concat always is a record of its own)
            start, y = 0, None
            for lst, out_t in cat_lists:
                j = len(lst)
                if 2 <= j < len(src) and j > start and tuple(src[:j]) == lst and layers[out_t[0] - 1].reserved <= 1:
                    start, y = j, out_t
            if y is None:
                y = concat_rec(src[0], src[1] if len(src) > 1 else None, 0)
                start = 2
            for x in src[start:]:
                y = concat_rec(y + (0,), x, 0)
            cat_lists.append((tuple(src), y))
            tmap[n.outputs[0]] = y
            flush_patterns(n.outputs[0])
        elif op in ("Split", "Slice"):
            who = f"{op} {n.name!r}: "
            x = tmap.get(n.inputs[0])
            if x is None:
                raise ConvertError(who + f"input {n.inputs[0]!r} is not on the path from {spec!r}")
            if x[0] == 0:
                raise ConvertError(who + "the spectrogram (tensor 0) as the input is not supported")
            C = x[1]
            if op == "Split":
                axis = int(n.attrs.get("axis", 0))
                if axis not in (1, -3):
                    raise ConvertError(who + f"axis {axis}: only the channel axis (1) is split")
                parts = len(n.outputs)
                if parts > 64:
                    raise ConvertError(who + f"{parts} outputs (1 .. 64 are read)")
                if n.attrs.get("split"):
                    sizes = [int(v) for v in n.attrs["split"]]
                elif len(n.inputs) > 1 and n.inputs[1]:
                    sizes = _const_ints(g, n.inputs[1])
                    if sizes is None:
                        raise ConvertError(who + f"sizes {n.inputs[1]!r} that are not a constant")
                else:
                    if int(n.attrs.get("num_outputs", parts)) != parts or C % parts:
                        raise ConvertError(who + f"{C} channels in {parts} equal parts")
                    sizes = [C // parts] * parts
                if len(sizes) != parts:
                    raise ConvertError(who + f"{len(sizes)} sizes for {parts} outputs")
                starts, at = [], 0
                for s in sizes:
                    if s <= 0 or s > 65536:
                        raise ConvertError(who + f"a part of {s} channels")
                    starts.append(at)
                    at += s
                if at != C:
                    raise ConvertError(who + f"sizes that add up to {at}, the input has {C} channels")
            else:
                lst = [None] * 4   # starts, ends, axes, steps
                for q in range(4):
                    if len(n.inputs) > q + 1 and n.inputs[q + 1]:
                        lst[q] = _const_ints(g, n.inputs[q + 1])
                        if lst[q] is None:
                            raise ConvertError(who + f"{n.inputs[q + 1]!r} is not a constant (starts, ends, axes and steps are read from constant inputs)")
                if lst[0] is None or lst[1] is None or lst[2] is None or any(v is not None and len(v) != 1 for v in lst):
                    raise ConvertError(who + "only a slice along one stated axis, the channels, is read")
                if lst[2][0] not in (1, -3):
                    raise ConvertError(who + f"axis {lst[2][0]}: only the channel axis (1) is sliced")
                if lst[3] is not None and lst[3][0] != 1:
                    raise ConvertError(who + f"step {lst[3][0]}: only step 1 is read")
                s, e = lst[0][0], lst[1][0]
                s = (0 if s < -C else s + C) if s < 0 else s
                e = (0 if e < -C else e + C) if e < 0 else e
                s, e = min(s, C), min(e, C)
                if e <= s:
                    raise ConvertError(who + "an empty slice")
                starts, sizes = [s], [e - s]
            for k, (st, sz) in enumerate(zip(starts, sizes)):
                if sz % 4 or st % 4:
                    raise ConvertError(who + f"output {k} is {sz} channels from channel {st}: " + _QUAD)
            for name, st, sz in zip(n.outputs, starts, sizes):
                if not name:
                    continue
                publish_view(name, x, st, sz)
                flush_patterns(name)
        elif op == "Reshape" and i in shuffle_at:
            out_name, s1, s2 = shuffle_at[i]
            who = f"Reshape {n.name!r} (channel shuffle): "
            x = tmap.get(n.inputs[0])
            if x is None:
                raise ConvertError(who + f"input {n.inputs[0]!r} is not on the path from {spec!r}")
            if x[0] == 0:
                raise ConvertError(who + "the spectrogram (tensor 0) as the input is not supported")
            _, C, h, w = x
            d5 = _resolve_shape(s1, [C, h, w], C * h * w) if len(s1) == 5 and len(s2) == 4 else None
            d4 = _resolve_shape(s2, [d5[1], d5[0], h, w], C * h * w) if d5 is not None and (d5[0] * d5[1], d5[2], d5[3]) == (C, h, w) else None
            if d4 != [C, h, w]:
                raise ConvertError(who + f"the shapes are not [N, g, C / g, H, W] and [N, C, H, W] of its {C} x {h} x {w} input")
            if C % 4:
                raise ConvertError(who + f"{C} channels: " + _QUAD)
            P = layers[x[0] - 1]
            if P.op == mf.OP_CONCAT and P.reserved <= 1 and n.inputs[0] not in graph_out and len(readers.get(n.inputs[0], [])) == 1:
                P.reserved = d5[0]
                tmap[out_name] = x
            else:
                tmap[out_name] = concat_rec(x + (0,), None, d5[0])
            flush_patterns(out_name)
        elif op == "Reshape" and i in shuffle_computed:
            raise ConvertError(f"Reshape {n.name!r}: a channel shuffle whose shape is computed (Shape -> Gather -> Concat) is not read: the shapes must be constants")
        elif op == "Conv":
            x = tmap.get(n.inputs[0])
            if x is None:
                raise ConvertError(f"Conv {n.name!r}: input {n.inputs[0]!r} is not on the path from {spec!r}")
            t_in, cin, h, w = x
            W = g.initializers.get(n.inputs[1])
            if W is None or W.ndim != 4:
                raise ConvertError(f"Conv {n.name!r}: weights must be a 4-d initializer")
            cout, cin_g, kh, kw = W.shape
            B = g.initializers.get(n.inputs[2]) if len(n.inputs) > 2 else np.zeros(cout, np.float32)
            group = int(n.attrs.get("group", 1))
            sh, sw = (n.attrs.get("strides") or [1, 1])
            # dilation (csrc/onnx_conv.hpp has the same branch, refusal for refusal): a group-1 convolution of an NHWC activation or a
            # depthwise one, 1 .. 16 per axis; an axis with one tap is dilation 1 whatever the file says (one spelling of the record)
            dil = [int(d) for d in (n.attrs.get("dilations") or [1, 1])]
            if any(d != 1 for d in dil) and len(dil) != 2:
                raise ConvertError(f"Conv {n.name!r}: dilations must be two values")
            dh, dw = dil if len(dil) == 2 else (1, 1)
            if not (1 <= dh <= mf.MAX_DILATION and 1 <= dw <= mf.MAX_DILATION):
                raise ConvertError(f"Conv {n.name!r}: dilation {dh}x{dw} (1 .. 16 are supported)")
            dh, dw = (1 if kh == 1 else dh), (1 if kw == 1 else dw)
            if (dh, dw) != (1, 1):
                if t_in == 0:
                    raise ConvertError(f"Conv {n.name!r}: dilation on the stem convolution (the spectrogram, tensor 0) is not supported")
                if group != 1 and not (group == cin and cin_g == 1 and cout == cin):
                    raise ConvertError(f"Conv {n.name!r}: dilation on a grouped convolution is not supported")
            ekh, ekw = (kh - 1) * dh + 1, (kw - 1) * dw + 1        # the window's extent over the image
            oh, ow = -(-h // sh), -(-w // sw)
            auto = n.attrs.get("auto_pad", "NOTSET")
            if auto in ("SAME_UPPER", "SAME_LOWER"):
                th, tw = max((oh - 1) * sh + ekh - h, 0), max((ow - 1) * sw + ekw - w, 0)
                pt, pl = (th // 2, tw // 2) if auto == "SAME_UPPER" else (th - th // 2, tw - tw // 2)
            else:
                pads = n.attrs.get("pads") or [0, 0, 0, 0]
                pt, pl = pads[0], pads[1]
                if h + pads[0] + pads[2] < ekh or w + pads[1] + pads[3] < ekw:
                    raise ConvertError(f"Conv {n.name!r}: kernel larger than the padded input")
                oh, ow = (h + pads[0] + pads[2] - ekh) // sh + 1, (w + pads[1] + pads[3] - ekw) // sw + 1
            if group == 1 and kh == 1 and kw == 1 and sh == 1 and sw == 1:
                L = mf.Layer(mf.OP_PWCONV, mf.ACT_NONE, t_in, mf.NO_TENSOR, cin, cout, 1, 1, 1, 1, 0, 0, h, w, h, w, 0,
                             blob.put(W[:, :, 0, 0].T), blob.put(B))
            elif group == cin and cin_g == 1 and cout == cin:
                L = mf.Layer(mf.OP_DWCONV, mf.ACT_NONE, t_in, mf.NO_TENSOR, cin, cout, kh, kw, sh, sw, pt, pl, h, w, oh, ow, 0,
                             blob.put(W[:, 0].transpose(1, 2, 0)), blob.put(B), dil_h=dh, dil_w=dw)
            elif group == 1:
                L = mf.Layer(mf.OP_CONV, mf.ACT_NONE, t_in, mf.NO_TENSOR, cin, cout, kh, kw, sh, sw, pt, pl, h, w, oh, ow,
                             1 if t_in == 0 else 0, blob.put(W.transpose(2, 3, 1, 0)), blob.put(B), dil_h=dh, dil_w=dw)
            else:
                # a grouped convolution -> OP_GCONV (csrc/onnx_conv.hpp has the same branch, refusal for refusal)
                who = f"Conv {n.name!r}: group {group} with {cin} -> {cout} channels"
                if t_in == 0:
                    raise ConvertError(who + ": a grouped convolution on the spectrogram (tensor 0) is not supported")
                if group < 1 or cin % group or cout % group or cin_g * group != cin:
                    raise ConvertError(who + f": the group count does not divide them (the weights hold {cin_g} input channels a group)")
                if cin_g % 4 or (cout // group) % 4:
                    raise ConvertError(who + f": a group width ({cin_g} -> {cout // group}) that is not a multiple of 4 is not supported")
                if kh > 7 or kw > 7:
                    raise ConvertError(who + f": a grouped kernel of {kh}x{kw} (1 .. 7 are supported)")
                if sh > 2 or sw > 2:
                    raise ConvertError(who + f": grouped strides of {sh}x{sw} (1 .. 2 are supported)")
                L = mf.Layer(mf.OP_GCONV, mf.ACT_NONE, t_in, mf.NO_TENSOR, cin, cout, kh, kw, sh, sw, pt, pl, h, w, oh, ow, 0,
                             blob.put(W.transpose(2, 3, 1, 0)), blob.put(B), reserved=group)
            layers.append(L)
            tmap[n.outputs[0]] = (len(layers), cout, L.out_h, L.out_w)
            flush_patterns(n.outputs[0])
        elif op == "BatchNormalization":
            t = tmap.get(n.inputs[0])
            L = layers[t[0] - 1] if t and t[0] > 0 else None
            conv_type = L is not None and L.op in (mf.OP_CONV, mf.OP_DWCONV, mf.OP_PWCONV, mf.OP_GCONV)
            # the refusal this norm has had so far, by its producer; it stands unless the norm becomes a record of its own (below)
            refusal = None
            if L is not None and L.op == mf.OP_CONCAT:
                refusal = (f"BatchNormalization {n.name!r} directly after a Concat, Split, Slice or channel shuffle cannot be folded "
                           "(the record carries neither a scale nor an activation)")
            elif not conv_type or L.act != mf.ACT_NONE:
                refusal = "BatchNormalization that does not follow a convolution directly"
            # folding rewrites the convolution's weights: a residual already folded into the layer (BN(conv + x)) or another
            # reader of the convolution's output (a skip taken before the BN) would silently see the wrong values
            elif L.res_tensor != mf.NO_TENSOR:
                refusal = "BatchNormalization after a residual Add (BN(conv + x)) cannot be folded into the convolution"
            if refusal is not None:
                # act(bn(x)) on a tensor no convolution can take the norm into -- a pool's, a concat's, an activated convolution's, a sum's,
                # another such record's -- is one OP_BNACT record (DenseNet, pre-activation ResNets; csrc/onnx_conv.hpp has the same branch).
                # The record is tentative, without an activation, until set_act completes it.
                ok = L is not None and t[2] > 0 and t[3] > 0 and t[1] % 4 == 0 and n.inputs[0] not in nhwc and n.inputs[0] not in r3 and \
                    (L.op in (mf.OP_POOL, mf.OP_CONCAT) or (L.op == mf.OP_BNACT and t[0] not in bn_pending) or
                     (conv_type and (L.res_tensor == mf.NO_TENSOR or n.inputs[0] in sums)))
                if not ok:
                    raise ConvertError(refusal)
                C = t[1]
                par = [g.initializers.get(a) for a in n.inputs[1:5]]
                if len(par) != 4 or any(a is None or a.dtype not in (np.float32, np.float16) or a.size != C for a in par):
                    raise ConvertError(f"BatchNormalization {n.name!r}: scale, B, mean and var must be float32 or float16 initializers of the {C} channels")
                gamma, beta, mean, var = (a.reshape(-1).astype(np.float64) for a in par)
                scale = gamma / np.sqrt(var + float(np.float32(n.attrs.get("epsilon", 1e-5))))      # (the attribute is an f32: its default too)
                shift = beta - mean * scale
                layers.append(mf.Layer(mf.OP_BNACT, mf.ACT_NONE, t[0], mf.NO_TENSOR, C, C, 1, 1, 1, 1, 0, 0, t[2], t[3], t[2], t[3], 0,
                                       blob.put(scale.astype(np.float32)), blob.put(shift.astype(np.float32))))
                bn_pending[len(layers)] = refusal
                tmap[n.outputs[0]] = (len(layers), C, t[2], t[3])
                flush_patterns(n.outputs[0])
                continue
            if sum(n.inputs[0] in q.inputs for q in g.nodes) != 1 or n.inputs[0] in graph_out:
                raise ConvertError("BatchNormalization of a convolution output that has other readers cannot be folded")
            gamma, beta, mean, var = (g.initializers[a].astype(np.float64) for a in n.inputs[1:5])
            scale = gamma / np.sqrt(var + float(n.attrs.get("epsilon", 1e-5)))
            nw = {mf.OP_CONV: L.kh * L.kw * L.cin * L.cout, mf.OP_DWCONV: L.kh * L.kw * L.cout, mf.OP_PWCONV: L.cin * L.cout,
                  mf.OP_GCONV: L.kh * L.kw * (L.cin // max(L.reserved, 1)) * L.cout}[L.op]
            arr = blob.array()
            wv = arr[L.w_off: L.w_off + nw].reshape(-1, L.cout) * scale.astype(np.float32)     # cout is the last axis in all three layouts
            bv = ((arr[L.b_off: L.b_off + L.cout] - mean) * scale + beta).astype(np.float32)
            arr[L.w_off: L.w_off + nw] = wv.reshape(-1)
            arr[L.b_off: L.b_off + L.cout] = bv
            blob.chunks, blob.off = [arr], arr.size
            tmap[n.outputs[0]] = t
            flush_patterns(n.outputs[0])
        elif op in ("Relu", "Gelu", "Clip"):
            if op == "Clip":
                lo = _scalar(g, n.inputs[1]) if len(n.inputs) > 1 else n.attrs.get("min")
                hi = _scalar(g, n.inputs[2]) if len(n.inputs) > 2 else n.attrs.get("max")
                if lo != 0.0 or hi != 6.0:
                    raise ConvertError(f"Clip({lo}, {hi}) is not ReLU6")
            if op == "Gelu" and n.attrs.get("approximate", "none") not in ("none", b"none"):
                act = mf.ACT_GELU_TANH
            else:
                act = {"Relu": mf.ACT_RELU, "Gelu": mf.ACT_GELU_ERF, "Clip": mf.ACT_RELU6}[op]
            set_act(n.inputs[0], n.outputs[0], act, (i,))
        elif op == "HardSwish":
            set_act(n.inputs[0], n.outputs[0], mf.ACT_HSWISH, (i,))
        elif op == "HardSigmoid":
            # (HardSigmoid * x was folded above; what arrives here is a gate -- set_act holds it to a pooled tensor -- or a refusal)
            if not _hsig_is_torch(n):
                raise ConvertError("HardSigmoid %r with alpha = %g, beta = %g: only alpha = 1/6, beta = 0.5 (PyTorch's hard sigmoid) is "
                                   "supported; the ONNX default alpha = 0.2 is Keras's hard sigmoid, a different function that no kernel "
                                   "here computes" % ((n.name,) + _hsig_params(n)))
            set_act(n.inputs[0], n.outputs[0], mf.ACT_HSIGMOID, (i,))
        elif op == "Add":
            a, b = (tmap.get(x) for x in n.inputs)
            if a is None or b is None:
                # MatMul + Add(bias): handled with the MatMul below
                raise ConvertError(f"Add of {n.inputs}: operands are not both activations on the path")
            # residual: one operand is a 1x1 or a full NHWC conv's output (latest layer, no residual yet; a full convolution is
            # the Fused-MBConv residual Add(act(conv(x)), x), never the NCHW stem), the other an older tensor
            for y, r in ((a, b), (b, a)):
                L = layers[y[0] - 1] if y[0] > 0 else None
                conv = L is not None and (L.op == mf.OP_PWCONV or (L.op == mf.OP_CONV and L.in_layout == 0))
                if conv and L.res_tensor == mf.NO_TENSOR and r[0] < y[0] and r[1:] == y[1:]:
                    L.res_tensor = r[0]
                    tmap[n.outputs[0]] = y
                    sums.add(n.outputs[0])
                    break
            else:
                raise ConvertError(f"Add of {n.inputs}: no convolution to fold the residual into")
            flush_patterns(n.outputs[0])   # (a multi-node activation behind the sum: act(conv + x))
        elif op in ("ReduceMean", "ReduceMax", "GlobalMaxPool"):
            # max / mean over H, over W or over both -> OP_REDUCE, and Add(ReduceMax(x, a), ReduceMean(x, a)) -> one MAXMEAN record
            # (csrc/onnx_conv.hpp has the same branch; the two are held to the same records).  The mean over both axes of an NCHW map stays OP_GAP.
            who = f"{op} {n.name!r}: "
            t = tmap.get(n.inputs[0])
            if t is None:
                raise ConvertError(who + f"input {n.inputs[0]!r} is not on the path from {spec!r}")
            x_r3 = r3.get(n.inputs[0], 0)

            def image_axes(q: ox.Node):
                """the image axes a node reduces, against its input's rank: (over H, over W)"""
                w2 = f"{q.op_type} {q.name!r}: "
                if q.op_type == "GlobalMaxPool":
                    axes = [2, 3]
                else:
                    axes = _reduce_axes(g, q)
                    if axes is None and len(q.inputs) > 1 and q.inputs[1]:
                        raise ConvertError(w2 + f"axes {q.inputs[1]!r} that are not a constant")
                    axes = axes or []
                if not 1 <= len(axes) <= 2:
                    raise ConvertError(w2 + f"{len(axes)} axes: only the image axes, H (2) or W (3) or both, are reduced")
                rank, qh, qw = (3 if x_r3 else 4), False, False
                for a in axes:
                    b = a + rank if a < 0 else a
                    if b < 2 or b >= rank:
                        raise ConvertError(w2 + f"axis {a} of a rank-{rank} tensor: only the image axes are reduced (never the batch or the channels)")
                    is_h = (x_r3 == 1) if x_r3 else b == 2
                    if qh if is_h else qw:
                        raise ConvertError(w2 + f"axis {a} named twice")
                    qh, qw = (True, qw) if is_h else (qh, True)
                return qh, qw

            if op == "GlobalMaxPool" and x_r3:
                raise ConvertError(who + "a rank-3 input")
            if op == "GlobalMaxPool" and len(n.outputs) > 1:
                raise ConvertError(who + "more than one output")
            rh, rw = image_axes(n)
            keep = 1 if op == "GlobalMaxPool" else int(n.attrs.get("keepdims", 1))
            if keep not in (0, 1):
                raise ConvertError(who + "keepdims must be 0 or 1")
            mode, out = (mf.REDUCE_MEAN if op == "ReduceMean" else mf.REDUCE_MAX), n.outputs[0]
            # the max + mean pair: an Add reads this reduce and another one
            for k in (cons_idx.get(n.outputs[0], []) if op != "GlobalMaxPool" else []):
                add = g.nodes[k]
                if add.op_type != "Add" or len(add.inputs) != 2 or not add.outputs or k in skip:
                    continue
                o2 = add.inputs[1] if add.inputs[0] == n.outputs[0] else add.inputs[0]
                j = prod_idx.get(o2)
                if j is None or j == i or j in skip or g.nodes[j].op_type not in ("ReduceMean", "ReduceMax"):
                    continue
                q = g.nodes[j]
                wa = f"Add {add.name!r} (max + mean pair): "
                if q.op_type == op:
                    raise ConvertError(wa + f"two {op} nodes: one ReduceMax and one ReduceMean of the same tensor are expected")
                if not q.inputs or not q.outputs or q.inputs[0] != n.inputs[0]:
                    raise ConvertError(wa + f"{n.name!r} and {q.name!r} reduce different tensors")
                if len(cons_idx.get(n.outputs[0], [])) != 1 or len(cons_idx.get(q.outputs[0], [])) != 1 or n.outputs[0] in graph_out or q.outputs[0] in graph_out:
                    raise ConvertError(wa + "a reduce that another node reads too, or that is a graph output (each is read by the Add alone)")
                if image_axes(q) != (rh, rw):
                    raise ConvertError(wa + f"{n.name!r} and {q.name!r} reduce different axes")
                if int(q.attrs.get("keepdims", 1)) != keep:
                    raise ConvertError(wa + f"{n.name!r} and {q.name!r} differ in keepdims")
                mode, out = mf.REDUCE_MAXMEAN, add.outputs[0]
                skip |= {j, k}
                break
            t_in, C, h, w = t
            if mode == mf.REDUCE_MEAN and rh and rw and not x_r3:
                # the global average pool: OP_GAP, as ever
                layers.append(mf.Layer(mf.OP_GAP, mf.ACT_NONE, t_in, mf.NO_TENSOR, C, C, h, w, 1, 1, 0, 0, h, w, 1, 1))
                tmap[out] = (len(layers), C, 1, 1)
                emb_tensor, emb_dim = len(layers), C
                flush_patterns(out)
                continue
            if t_in == 0:
                raise ConvertError(who + "a reduction of the spectrogram (tensor 0) is not supported")
            if C % 4:
                raise ConvertError(who + f"{C} channels: a channel count that is not a multiple of 4 is not supported")
            kh, kw = (h if rh else 1), (w if rw else 1)
            if kh * kw == 1:
                raise ConvertError(who + "a window of one pixel (the reduced axes have extent 1): nothing to reduce")
            if kh * kw > 65536:
                raise ConvertError(who + "a window of more than 65 536 pixels")
            oh, ow = h // kh, w // kw
            layers.append(mf.Layer(mf.OP_REDUCE, mf.ACT_NONE, t_in, mf.NO_TENSOR, C, C, kh, kw, 1, 1, 0, 0, h, w, oh, ow, reserved=mode))
            tmap[out] = (len(layers), C, oh, ow)
            # (the pair over both axes, or one that finishes the image, is [N, C, 1, 1]: no rank-3 tensor of one pixel is kept)
            whole = mode == mf.REDUCE_MAXMEAN and oh * ow == 1
            if keep == 0 and not x_r3 and not (rh and rw) and not whole:
                r3[out] = 2 if rh else 1
            if keep == 1 and x_r3 and not whole:
                r3[out] = x_r3
            if oh * ow == 1:
                emb_tensor, emb_dim = len(layers), C
            flush_patterns(out)
        elif op == "GlobalAveragePool":
            t = tmap.get(n.inputs[0])
            if t is None:
                raise ConvertError(f"{op}: input not on the path")
            layers.append(mf.Layer(mf.OP_GAP, mf.ACT_NONE, t[0], mf.NO_TENSOR, t[1], t[1], t[2], t[3], 1, 1, 0, 0, t[2], t[3], 1, 1))
            tmap[n.outputs[0]] = (len(layers), t[1], 1, 1)
            emb_tensor, emb_dim = len(layers), t[1]
            flush_patterns(n.outputs[0])      # (a decomposed LayerNorm behind the pool)
        elif op in ("MaxPool", "AveragePool"):
            # windowed pooling in floor mode -> OP_POOL (csrc/onnx_conv.hpp has the same branch)
            who = f"{op} {n.name!r}: "
            x = tmap.get(n.inputs[0])
            if x is None:
                raise ConvertError(who + f"input {n.inputs[0]!r} is not on the path from {spec!r}")
            t_in, c, h, w = x
            if t_in == 0:
                raise ConvertError(who + "pooling on the planar spectrogram (tensor 0) is not supported")
            if len(n.outputs) > 1 and n.outputs[1]:
                raise ConvertError(who + "the second output (Indices) is not supported")
            ks = n.attrs.get("kernel_shape")
            if ks is None or len(ks) != 2 or not all(1 <= int(k) <= 64 for k in ks):
                raise ConvertError(who + "kernel_shape must be two values, each 1 .. 64")
            kh, kw = int(ks[0]), int(ks[1])
            st = n.attrs.get("strides") or [1, 1]
            if len(st) != 2 or not all(1 <= int(v) <= 16 for v in st):
                raise ConvertError(who + "strides must be 1 .. 16")
            sh, sw = int(st[0]), int(st[1])
            if any(d != 1 for d in (n.attrs.get("dilations") or [1, 1])):
                raise ConvertError(who + "a dilation other than 1 is not supported")
            if int(n.attrs.get("storage_order", 0)) != 0:
                raise ConvertError(who + "storage_order = 1 (column-major indices) is not supported")
            cip, ceil_mode = int(n.attrs.get("count_include_pad", 0)), int(n.attrs.get("ceil_mode", 0))
            if cip not in (0, 1) or ceil_mode not in (0, 1):
                raise ConvertError(who + "count_include_pad / ceil_mode must be 0 or 1")
            auto = n.attrs.get("auto_pad", "NOTSET")
            auto = auto.decode() if isinstance(auto, bytes) else auto
            if auto in ("SAME_UPPER", "SAME_LOWER"):
                oh, ow = -(-h // sh), -(-w // sw)
                th, tw = max((oh - 1) * sh + kh - h, 0), max((ow - 1) * sw + kw - w, 0)
                pt, pl = (th // 2, tw // 2) if auto == "SAME_UPPER" else (th - th // 2, tw - tw // 2)
            elif auto in ("NOTSET", "VALID"):
                pads = [int(p) for p in ((n.attrs.get("pads") if auto == "NOTSET" else None) or [0, 0, 0, 0])]
                if len(pads) != 4:
                    raise ConvertError(who + "pads must be four values")
                if not all(0 <= p <= 64 for p in pads):
                    raise ConvertError(who + "pads must be 0 .. 64")
                pt, pl = pads[0], pads[1]
                eh, ew = h + pads[0] + pads[2] - kh, w + pads[1] + pads[3] - kw
                if eh < 0 or ew < 0:
                    raise ConvertError(who + "kernel larger than the padded input")
                oh, ow = eh // sh + 1, ew // sw + 1
                if ceil_mode:   # ONNX: round up, but the last window must start inside the image or its top / left padding
                    ch, cw = -(-eh // sh) + 1, -(-ew // sw) + 1
                    ch -= (ch - 1) * sh >= h + pads[0]
                    cw -= (cw - 1) * sw >= w + pads[1]
                    if (ch, cw) != (oh, ow):
                        raise ConvertError(who + f"ceil_mode = 1 changes the output size ({oh}x{ow} -> {ch}x{cw}): only floor-mode windows are supported")
            else:
                raise ConvertError(who + f"auto_pad {auto!r}")
            if oh <= 0 or ow <= 0 or oh > 65536 or ow > 65536:
                raise ConvertError(who + "empty or oversized output")
            if pt >= kh or pl >= kw or (oh - 1) * sh - pt >= h or (ow - 1) * sw - pl >= w:
                raise ConvertError(who + "a window without an in-image tap (it lies in the padding alone)")
            mode = mf.POOL_MAX if op == "MaxPool" else (mf.POOL_AVG_PAD if cip else mf.POOL_AVG)
            layers.append(mf.Layer(mf.OP_POOL, mf.ACT_NONE, t_in, mf.NO_TENSOR, c, c, kh, kw, sh, sw, pt, pl, h, w, oh, ow, reserved=mode))
            tmap[n.outputs[0]] = (len(layers), c, oh, ow)
        elif op in ("Flatten", "Reshape", "Squeeze", "Unsqueeze", "Identity", "Dropout"):
            t = tmap.get(n.inputs[0])
            if t is None:
                raise ConvertError(f"{op}: input not on the path")
            if t[2] * t[3] != 1:
                raise ConvertError(f"{op} of a {t[2]}x{t[3]} map (only after the global pool)")
            tmap[n.outputs[0]] = t
        elif op in ("Gemm", "MatMul"):
            t = tmap.get(n.inputs[0])
            W = g.initializers.get(n.inputs[1])
            if t is None or W is None or W.ndim != 2:
                raise ConvertError(f"{op}: needs an activation on the path and a 2-d weight initializer")
            if op == "Gemm" and int(n.attrs.get("transB", 0)):
                W = W.T
            if op == "Gemm" and (float(n.attrs.get("alpha", 1.0)) != 1.0 or float(n.attrs.get("beta", 1.0)) != 1.0 or int(n.attrs.get("transA", 0))):
                raise ConvertError("Gemm with alpha / beta / transA")
            cin, cout = W.shape
            if cin != t[1]:
                raise ConvertError(f"{op}: {cin} input features, activation has {t[1]}")
            B = g.initializers.get(n.inputs[2]) if op == "Gemm" and len(n.inputs) > 2 else None
            out = n.outputs[0]
            if B is None:   # MatMul followed by Add(bias)
                nxt = [k for k, nn in enumerate(g.nodes) if nn.op_type == "Add" and out in nn.inputs]
                if len(nxt) == 1:
                    other = [a for a in g.nodes[nxt[0]].inputs if a != out][0]
                    if other in g.initializers and g.initializers[other].size == cout:
                        B, out = g.initializers[other], g.nodes[nxt[0]].outputs[0]
                        skip.add(nxt[0])
            if B is None:
                B = np.zeros(cout, np.float32)
            layers.append(mf.Layer(mf.OP_DENSE, mf.ACT_NONE, t[0], mf.NO_TENSOR, cin, cout, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0,
                                   blob.put(W), blob.put(B.reshape(-1))))
            tmap[out] = (len(layers), cout, 1, 1)
            flush_patterns(out)
        elif op == "Sigmoid" and n.outputs[0] not in graph_out:
            # the gate of a squeeze-excite block: Sigmoid on a pooled [N, C, 1, 1] tensor, consumed by a Mul with the feature map
            t = tmap.get(n.inputs[0])
            if t is None or t[2] * t[3] != 1:
                raise ConvertError("Sigmoid inside the graph that is neither Sigmoid * x nor a squeeze-excite gate")
            set_act(n.inputs[0], n.outputs[0], mf.ACT_SIGMOID, (i,))
        elif op == "Mul":
            a, b = (tmap.get(x) for x in n.inputs)
            if a is None or b is None:
                raise ConvertError(f"Mul of {n.inputs}: operands are not both activations on the path")
            for fm, gate in ((a, b), (b, a)):
                if fm[2] * fm[3] > 1 and gate[2] * gate[3] == 1 and gate[1] == fm[1]:
                    layers.append(mf.Layer(mf.OP_SCALE, mf.ACT_NONE, fm[0], gate[0], fm[1], fm[1], 1, 1, 1, 1, 0, 0, fm[2], fm[3], fm[2], fm[3]))
                    tmap[n.outputs[0]] = (len(layers), fm[1], fm[2], fm[3])
                    break
            else:
                raise ConvertError(f"Mul of {n.inputs}: not a feature map times a [N, C, 1, 1] gate")
        elif op in ("Sigmoid", "Softmax"):
            if n.outputs[0] not in graph_out:
                raise ConvertError(f"{op} inside the graph (only the output activation is supported, or Sigmoid * x)")
            out_act = mf.OUT_SIGMOID if op == "Sigmoid" else mf.OUT_SOFTMAX
            tmap[n.outputs[0]] = tmap[n.inputs[0]]
        else:
            raise ConvertError(f"unsupported operator {op} ({n.name!r})")
    if bn_pending:
        raise ConvertError(bn_pending[min(bn_pending)])
    if first_of_pattern or ln_of_pattern:
        raise ConvertError(f"activation patterns on tensors that were never produced: {sorted(set(first_of_pattern) | set(ln_of_pattern))}")
    if not layers or layers[-1].op != mf.OP_DENSE:
        raise ConvertError("the graph does not end in a dense layer")
    final = [tmap.get(o.name) for o in g.outputs]
    if not final or final[0] is None or final[0][0] != len(layers):
        raise ConvertError("the graph output is not the last layer's output")
    return mf.Model(frontend.family, frontend.sample_rate, frontend.sample_count, frontend.segment_duration,
                    layers[-1].cout, emb_dim, out_act, emb_tensor, frontend.spec_h, frontend.spec_w, frontend.norm_eps,
                    [mf.Branch(**{k: getattr(b, k) for k in ("frame_length", "frame_step", "n_mels", "n_frames", "fmin", "fmax",
                                                             "mag_scale", "out_scale", "out_shift", "flags", "mel_w_off")})
                     for b in frontend.branches], layers, blob.array())


def graph_to_float16(g: ox.Graph, frontend: str = "f16", spectrogram: str = "spectrogram") -> ox.Graph:
    """`g` (a graph from `graph_from_model`) rewritten the way the published float16 export is described: the float32 graph input
    and outputs kept, a Cast(to=float16) behind the input, a Cast(to=float32) in front of each output, every float32 initializer
    converted to float16 (round to nearest even; a magnitude above 65 504 becomes inf, as numpy does it).  frontend='f32': the nodes
    that produce `spectrogram` and the constants only they read stay float32, between a pair of Casts (float16 -> float32 in front
    of them, float32 -> float16 behind the spectrogram).  Test and tool infrastructure: nothing in the product path calls it."""
    if frontend not in ("f16", "f32"):
        raise ConvertError(f"frontend {frontend!r}: 'f16' or 'f32'")
    nodes = [ox.Node(n.op_type, list(n.inputs), list(n.outputs), dict(n.attrs), n.name) for n in g.nodes]
    prod = {o: i for i, n in enumerate(nodes) for o in n.outputs}
    front, stack = set(), [spectrogram]
    while stack:
        i = prod.get(stack.pop())
        if i is None or i in front:
            continue
        front.add(i)
        stack.extend(nodes[i].inputs)
    keep32 = set()
    if frontend == "f32" and front:
        read_elsewhere = {x for i, n in enumerate(nodes) if i not in front for x in n.inputs}
        keep32 = {x for i in front for x in nodes[i].inputs if x in g.initializers and x not in read_elsewhere}
    init = {k: (a.astype(np.float16) if a.dtype == np.float32 and k not in keep32 else a) for k, a in g.initializers.items()}

    def cast(src: str, dst: str, to: int) -> ox.Node:
        return ox.Node("Cast", [src], [dst], {"to": to}, name=dst)

    def rename_readers(old: str, new: str, among) -> None:
        for i in among:
            nodes[i].inputs = [new if x == old else x for x in nodes[i].inputs]

    head, everyone = [], range(len(nodes))
    for vi in g.inputs:
        if vi.elem_type != ox.FLOAT:
            continue
        h16 = vi.name + "_f16"
        head.append(cast(vi.name, h16, ox.FLOAT16))
        if keep32:
            head.append(cast(h16, vi.name + "_f32", ox.FLOAT))
            rename_readers(vi.name, vi.name + "_f32", everyone)
        else:
            rename_readers(vi.name, h16, everyone)
    body = []
    for i, n in enumerate(nodes):
        body.append(n)
        if keep32 and spectrogram in n.outputs:
            body.append(cast(spectrogram, spectrogram + "_f16", ox.FLOAT16))
            rename_readers(spectrogram, spectrogram + "_f16", [j for j in everyone if j not in front])
    tail = []
    for vo in g.outputs:
        if vo.elem_type != ox.FLOAT:
            continue
        inner = vo.name + "_f16"
        for n in nodes:
            n.outputs = [inner if x == vo.name else x for x in n.outputs]
        rename_readers(vo.name, inner, everyone)
        tail.append(cast(inner, vo.name, ox.FLOAT))
    return ox.Graph(head + body + tail, init, list(g.inputs), list(g.outputs), g.name, g.opset, g.producer)


def convert_file(onnx_path: str, frontend_bhm: Optional[str], out_path: str, spectrogram_input: Optional[str] = None,
                 sample_rate: Optional[int] = None, family: int = 0) -> mf.Model:
    """ONNX file (+ a BHM1 file carrying the family's front-end, or none and a sample rate: the front-end is then read
    off the graph) -> BHM1 model."""
    m = model_from_graph(ox.load(open(onnx_path, "rb").read()), mf.read_model(frontend_bhm) if frontend_bhm else None,
                         spectrogram_input, sample_rate, family)
    mf.write_model(out_path, m)
    return m


def dense_stack_from_graph(g: ox.Graph, fold_final_sigmoid: bool = True) -> mf.CustomClassifierModel:
    """A dense-stack ONNX graph (the BirdNET geomodel's shape: Gemm / MatMul + Add, Relu, a final Sigmoid or Softmax; the
    reference's fixture tests/fixtures/fixture-geomodel.onnx is Gemm(3 -> 5) + Sigmoid) -> BHC1.  The Python twin of
    birda_amd/csrc/onnx_dense.hpp (which reads the .onnx file inside the library): same chain walk, same refusals.  A final
    Sigmoid becomes the last layer's activation, so every class's score leaves the GEMM activated (bh_range_filter_*)."""
    data_inputs = [vi.name for vi in g.inputs]
    if len(data_inputs) != 1 or len(g.outputs) != 1:
        raise ConvertError("a dense stack has one data input and one output")
    cur, out_name = data_inputs[0], g.outputs[0].name
    layers: List[mf.CustomLayer] = []
    out_act = mf.OUT_NONE
    todo = list(g.nodes)
    while cur != out_name:
        node = next((n for n in todo if n.inputs and n.inputs[0] == cur), None)
        if node is None:
            raise ConvertError(f"graph is not a chain from its input to its output (at {cur!r})")
        todo.remove(node)
        if out_act != mf.OUT_NONE:
            raise ConvertError(f"operator {node.op_type!r} after the output activation")
        op = node.op_type
        if op in ("Gemm", "MatMul"):
            w = g.initializers.get(node.inputs[1]) if len(node.inputs) > 1 else None
            if w is None or w.ndim != 2:
                raise ConvertError(f"{op}: weight must be a 2-D initializer")
            w = np.asarray(w, np.float32)
            alpha = np.float32(node.attrs.get("alpha", 1.0)) if op == "Gemm" else np.float32(1.0)
            beta = np.float32(node.attrs.get("beta", 1.0)) if op == "Gemm" else np.float32(1.0)
            if op == "Gemm" and node.attrs.get("transA", 0):
                raise ConvertError("Gemm: transA is not a dense layer")
            if op == "Gemm" and node.attrs.get("transB", 0):
                w = w.T
            w = (alpha * w).astype(np.float32)
            b = np.zeros(w.shape[1], np.float32)
            if op == "Gemm" and len(node.inputs) > 2 and node.inputs[2]:
                bias = np.asarray(g.initializers[node.inputs[2]], np.float32).reshape(-1)
                b = (beta * np.broadcast_to(bias, (w.shape[1],))).astype(np.float32)
            if layers and layers[-1].w.shape[1] != w.shape[0]:
                raise ConvertError(f"{op}: layer widths do not chain")
            layers.append(mf.CustomLayer(w, b, mf.ACT_NONE))
        elif op == "Add":
            bias = g.initializers.get(node.inputs[1]) if len(node.inputs) == 2 else None
            if not layers or layers[-1].act != mf.ACT_NONE or bias is None or bias.size != layers[-1].w.shape[1]:
                raise ConvertError("Add: only a bias right after MatMul / Gemm is a dense layer")
            layers[-1].b = (layers[-1].b + np.asarray(bias, np.float32).reshape(-1)).astype(np.float32)
        elif op in ("Relu", "Sigmoid"):
            if not layers or layers[-1].act != mf.ACT_NONE:
                raise ConvertError(f"{op} without a dense layer in front of it")
            layers[-1].act = mf.ACT_RELU if op == "Relu" else mf.ACT_SIGMOID
        elif op == "Softmax":
            if not layers or layers[-1].act != mf.ACT_NONE:
                raise ConvertError("Softmax without a dense layer in front of it")
            out_act = mf.OUT_SOFTMAX
        elif op in ("Identity", "Flatten", "Dropout"):
            pass
        else:
            raise ConvertError(f"operator {op!r} is not part of a dense stack (Gemm, MatMul + Add, Relu, Sigmoid, Softmax)")
        cur = node.outputs[0]
    if not layers:
        raise ConvertError("no dense layer between input and output")
    if not fold_final_sigmoid and layers[-1].act == mf.ACT_SIGMOID:
        layers[-1].act, out_act = mf.ACT_NONE, mf.OUT_SIGMOID
    return mf.CustomClassifierModel(int(layers[0].w.shape[0]), out_act, layers)


def convert_geomodel_file(onnx_path: str, out_path: str) -> mf.CustomClassifierModel:
    """geomodel .onnx -> BHC1 (bh_range_filter_create takes either file)."""
    m = dense_stack_from_graph(ox.load(open(onnx_path, "rb").read()))
    mf.write_custom_classifier(out_path, m)
    return m
