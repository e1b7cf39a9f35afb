"""ConvNeXt models on the host side: the container's OP_LNORM record (code 12), the [N, H, W, C] view both ONNX readers keep behind a
Transpose, LayerNormalization as a node and as the decomposed chain, MatMul layers on the view, the layer-scale fold, the writer and
the validator.

* the yardstick: lnorm64 is the channel LayerNorm in float64 (biased variance, pixel by pixel); layer64c / forward64 compose a
  model's logits from it -- the plain-C oracle does not know the op and is never fed such a model.  Both are held, tensor by tensor,
  to a torch float64 composition (F.layer_norm, F.conv2d(groups = C), F.gelu, scale * (...) + x) of convnext_plan's UN-FOLDED weights:
  the record's meaning and the layer-scale fold at once;
* torch_graph writes a model the way a PyTorch export spells it -- Transpose / LayerNormalization / MatMul + Add / Gelu or the Erf
  chain / Mul by the layer scale / Transpose, or channels-first with the decomposed chain over axis 1 and 1x1 Conv layers -- and both
  readers turn every spelling into the records and the weights of the synth model, the same layer table and blob, bit for bit;
* every refusal the readers make is held to a word of its message, in both readers; every validate_model refusal of a code-12
  record is hit by changing one field; mutated graphs and containers load or are refused, none crashes.
"""
import copy
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_dilated import layer64d
from test_pool import RECORD, both_readers, same_tables_and_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
def lnorm64(X, gamma, beta, eps):
    """X [..., C] -> (x - mean) / sqrt(var + eps) * gamma + beta over the last axis in float64, var the biased variance; eps is the
    float32 value the record holds"""
    X = np.asarray(X, np.float64)
    mean = X.mean(axis=-1, keepdims=True)
    d = X - mean
    var = (d * d).mean(axis=-1, keepdims=True)
    return d / np.sqrt(var + float(np.float32(eps))) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def lnorm_tol(X, gamma, beta, eps, tau):
    """the first-order bound of the f32 kernel against lnorm64: the mean carries a few ulps of mean|x|, x - mean therefore u (|x| +
    |mean|), 1 / sigma a few ulps -- |got - ref| <= tau (|gamma| (2 |xhat| + (|x| + |mean|) / sigma) + |beta|)"""
    X = np.asarray(X, np.float64)
    mean = X.mean(axis=-1, keepdims=True)
    d = X - mean
    sigma = np.sqrt((d * d).mean(axis=-1, keepdims=True) + float(np.float32(eps)))
    return tau * (np.abs(np.asarray(gamma, np.float64)) * (2 * np.abs(d / sigma) + (np.abs(X) + np.abs(mean)) / sigma) + np.abs(np.asarray(beta, np.float64)))


def layer64c(m, L, X, R):
    """tests/test_dilated.py's layer64d, with the OP_LNORM record computed here"""
    if L.op != mf.OP_LNORM:
        return layer64d(m, L, X, R)
    assert R is None and L.act == mf.ACT_NONE and L.cin == L.cout
    n = np.asarray(X).shape[0]
    Y = lnorm64(np.asarray(X).reshape(n, L.in_h, L.in_w, L.cout), m.blob[L.w_off:L.w_off + L.cout], m.blob[L.b_off:L.b_off + L.cout], mf.lnorm_eps(L.reserved))
    return Y


def forward64(m, segs, tensors=False):
    """-> logits [n][n_classes] in float64 (tensors=True: every tensor, T[0] the spectrogram)"""
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        T.append(layer64c(m, L, T[L.in_tensor], None if L.res_tensor == mf.NO_TENSOR else T[L.res_tensor]))
    return T if tensors else T[-1].reshape(segs.shape[0], -1)


@pytest.fixture(scope="module")
def plan():
    return synth.build_model("convnext_plan", seed=1)


def test_convnext_plan_holds_what_it_promises():
    seen_widths, seen_eps = set(), set()
    for seed in range(6):
        m = synth.build_model("convnext_plan", seed=seed)
        ops = [L.op for L in m.layers]
        stem = m.layers[0]
        assert (stem.op, stem.kh, stem.kw, stem.sh, stem.sw, stem.in_layout) == (mf.OP_CONV, 4, 4, 4, 4, 1) and ops[1] == mf.OP_LNORM
        assert ops[-3:] == [mf.OP_GAP, mf.OP_LNORM, mf.OP_DENSE] and m.embedding_tensor == len(m.layers) - 1        # the head norm is the embedding
        dws = [i for i, L in enumerate(m.layers) if L.op == mf.OP_DWCONV]
        assert dws and all((m.layers[i].kh, m.layers[i].kw, m.layers[i].sh, m.layers[i].act) == (7, 7, 1, mf.ACT_NONE) for i in dws)
        for i in dws:           # dw7x7 -> LN -> pw x4 GELU -> pw (layer scale folded) + x
            D, N, P1, P2 = m.layers[i:i + 4]
            assert (N.op, P1.op, P2.op) == (mf.OP_LNORM, mf.OP_PWCONV, mf.OP_PWCONV) and N.in_tensor == i + 1
            assert P1.cout == 4 * D.cout and P1.act == mf.ACT_GELU_ERF and P2.act == mf.ACT_NONE and P2.res_tensor == D.in_tensor
            assert i + 3 in m.convnext_scales
        downs = [i for i, L in enumerate(m.layers) if L.op == mf.OP_CONV and L.in_layout == 0]
        assert downs and all((m.layers[i].kh, m.layers[i].sh, m.layers[i - 1].op) == (2, 2, mf.OP_LNORM) for i in downs)
        seen_widths |= {L.cout for L in m.layers if L.op == mf.OP_LNORM}
        seen_eps |= {mf.lnorm_eps(L.reserved) for L in m.layers if L.op == mf.OP_LNORM}
        assert m.macs_per_segment() == sum(L.out_h * L.out_w * L.kh * L.kw * (L.cin if L.op != mf.OP_DWCONV else 1) * L.cout
                                           for L in m.layers if L.op in (mf.OP_CONV, mf.OP_DWCONV, mf.OP_PWCONV, mf.OP_DENSE))   # the norm is not counted
    assert {36, 72, 100} <= seen_widths and len(seen_eps) == 2
    big = synth.build_model("convnext_audio", n_classes=40)
    assert [L.cout for L in big.layers if L.op == mf.OP_CONV] == [96, 192, 384, 768] and [L.op for L in big.layers].count(mf.OP_DWCONV) == 18
    assert big.n_classes == 40 and big.embedding_dim == 768


def test_forward64_is_the_torch_float64_composition(plan):
    """convnext_plan composed in torch float64 from its UN-FOLDED weights -- F.layer_norm over the channels, conv2d(groups = C), F.gelu,
    scale * pw(...) + x -- against forward64 of the records, tensor by tensor"""
    import torch
    import torch.nn.functional as F
    m = plan
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=5)
    T = forward64(m, segs, tensors=True)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    Y = [t64(T[0])]                                                                      # NCHW throughout
    worst = 0.0
    for i, L in enumerate(m.layers):
        x = Y[L.in_tensor]
        if L.op == mf.OP_LNORM:
            g, b = t64(m.blob[L.w_off:L.w_off + L.cout]), t64(m.blob[L.b_off:L.b_off + L.cout])
            y = F.layer_norm(x.permute(0, 2, 3, 1), (L.cout,), g, b, eps=float(np.float32(mf.lnorm_eps(L.reserved)))).permute(0, 3, 1, 2)
        elif L.op in (mf.OP_CONV, mf.OP_DWCONV):
            b = t64(m.blob[L.b_off:L.b_off + L.cout])
            if L.op == mf.OP_CONV:
                w, groups = m.blob[L.w_off:L.w_off + L.kh * L.kw * L.cin * L.cout].reshape(L.kh, L.kw, L.cin, L.cout).transpose(3, 2, 0, 1), 1
            else:
                w, groups = m.blob[L.w_off:L.w_off + L.kh * L.kw * L.cout].reshape(L.kh, L.kw, L.cout).transpose(2, 0, 1)[:, None], L.cout
            pad_b = max((L.out_h - 1) * L.sh + L.kh - L.in_h - L.pad_t, 0)
            pad_r = max((L.out_w - 1) * L.sw + L.kw - L.in_w - L.pad_l, 0)
            y = F.conv2d(F.pad(x, (L.pad_l, pad_r, L.pad_t, pad_b)), t64(w), b, stride=(L.sh, L.sw), groups=groups)
            assert L.act == mf.ACT_NONE and L.res_tensor == mf.NO_TENSOR
        elif L.op == mf.OP_PWCONV:
            xv = x.permute(0, 2, 3, 1)
            if i in m.convnext_scales:                                                   # scale * (x W + b) + block input, un-folded
                W, b, ls = m.convnext_scales[i]
                y = (t64(ls) * (xv @ t64(W) + t64(b))).permute(0, 3, 1, 2) + Y[L.res_tensor]
            else:
                W, b = m.blob[L.w_off:L.w_off + L.cin * L.cout].reshape(L.cin, L.cout), m.blob[L.b_off:L.b_off + L.cout]
                assert L.act == mf.ACT_GELU_ERF and L.res_tensor == mf.NO_TENSOR
                y = F.gelu(xv @ t64(W) + t64(b)).permute(0, 3, 1, 2)
        elif L.op == mf.OP_GAP:
            y = x.mean(dim=(2, 3), keepdim=True)
        else:
            assert L.op == mf.OP_DENSE and L.act == mf.ACT_NONE
            y = (x.reshape(x.shape[0], -1) @ t64(m.blob[L.w_off:L.w_off + L.cin * L.cout].reshape(L.cin, L.cout)) + t64(m.blob[L.b_off:L.b_off + L.cout]))[:, :, None, None]
        Y.append(y)
        want = y.numpy().transpose(0, 2, 3, 1)
        got = np.asarray(T[i + 1]).reshape(want.shape)
        assert tuple(want.shape[1:]) == (L.out_h, L.out_w, L.cout), i
        # (the fold rounds W * scale and b * scale to float32 once: 2^-24 relative per product, so 1e-6 of the tensor's scale over the
        #  whole depth is generous; a missed fold or a biased variance is off by percents)
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1.0)
        worst = max(worst, err)
        assert err <= 1e-6, (i, L.op, err)
    print(f"forward64 against torch float64, un-folded layer scale: worst {worst:.2e} of a tensor's scale")
    # the folds matter: the same records with the un-folded second pointwise layers are another function
    twin = copy.deepcopy(m)
    for i, (W, b, ls) in m.convnext_scales.items():
        L = twin.layers[i]
        twin.blob[L.w_off:L.w_off + W.size] = W.ravel()
    other = forward64(twin, segs)
    assert np.abs(other - T[-1].reshape(other.shape)).max() > 1e-3 * np.abs(other).max()


def test_lnorm64_is_the_definition():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((5, 3, 12)) + 100.0
    g, b = rng.standard_normal(12), rng.standard_normal(12)
    Y = lnorm64(X, g, b, 1e-5)
    for p in np.ndindex(5, 3):
        x = X[p]
        mu = sum(x) / 12
        var = sum((v - mu) ** 2 for v in x) / 12                                        # biased
        assert np.allclose(Y[p], [(v - mu) / np.sqrt(var + float(np.float32(1e-5))) * g[c] + b[c] for c, v in enumerate(x)], rtol=1e-12, atol=1e-12)
    assert np.array_equal(lnorm64(np.full((2, 8), 3.25), g[:8], b[:8], 1e-6), np.broadcast_to(b[:8], (2, 8)))       # a constant pixel is beta
    # the bound sees the one-pass variance fail on offset data: E[x^2] - mean^2 in float32 against the tolerance
    X32 = X.astype(np.float32)
    one_pass = (X32 * X32).mean(axis=-1, dtype=np.float32) - X32.mean(axis=-1, dtype=np.float32) ** 2
    bad = (X32 - X32.mean(axis=-1, keepdims=True, dtype=np.float32)) / np.sqrt(np.maximum(one_pass, 0)[..., None] + np.float32(1e-5)) * g.astype(np.float32) + b.astype(np.float32)
    tol = lnorm_tol(X32, g.astype(np.float32), b.astype(np.float32), 1e-5, 4e-7)
    assert (np.abs(bad - lnorm64(X32, g.astype(np.float32), b.astype(np.float32), 1e-5)) > tol).any()


# ---- a model as a PyTorch export spells it ----------------------------------------------------------------------------------------
def n_weights(L):
    return {mf.OP_CONV: L.kh * L.kw * L.cin * L.cout, mf.OP_DWCONV: L.kh * L.kw * L.cout, mf.OP_PWCONV: L.cin * L.cout, mf.OP_DENSE: L.cin * L.cout,
            mf.OP_LNORM: L.cout}.get(L.op, 0)


def torch_graph(m, ln="node", layout="nhwc", scale="folded_no", gelu="gelu", head="view", beta=True, frontend=None):
    """The ConvNeXt model m (synth's records; the un-folded layer scales from m.convnext_scales) the way a PyTorch export spells it:
    layout 'nhwc' -- a block is Conv(group = C) -> Transpose [0, 2, 3, 1] -> LayerNorm -> MatMul + Add -> GELU -> MatMul + Add -> Mul by the
    [C] layer scale -> Transpose [0, 3, 1, 2] -> Add(block input); 'nchw' -- channels-first: the decomposed chain over axis 1 with
    [C, 1, 1] parameters, 1x1 Conv layers, the layer scale [C, 1, 1] or [1, C, 1, 1].
    ln: 'node' (LayerNormalization, opset 17) or 'chain' (ReduceMean -> Sub -> Pow -> ReduceMean -> Add -> Sqrt -> Div -> Mul -> Add).
    head: the norm behind the pool as 'view' (between two Transposes) or 'nchw11' (LayerNormalization(axis = 1) on [N, C, 1, 1]).
    scale: the shape of the layer-scale constant on the NCHW map ('c11' / '1c11'; the view takes [C]).  beta=False: no beta input
    (node form).  gelu: 'gelu' or 'erf' (the five-node chain).  frontend: None = the graph starts at `spectrogram`, else the
    spelling convert.frontend_nodes writes in front."""
    g = ox.Graph(name="convnext_torch_style", producer="tests")
    if frontend is None:
        g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", len(m.branches), m.spec_h, m.spec_w]))
    else:
        g.inputs.append(ox.ValueInfo("audio", ox.FLOAT, ["N", m.sample_count]))
        convert.frontend_nodes(g, m, frontend)
    nchw, nhwc = {0: "spectrogram"}, {}

    def const(name, a, dtype=np.float32):
        g.initializers[name] = np.asarray(a, dtype)
        return name

    def node(op, ins, out, **attrs):
        g.nodes.append(ox.Node(op, list(ins), [out], attrs, name=out))
        return out

    def as_nchw(t):
        if t not in nchw:
            nchw[t] = node("Transpose", [nhwc[t]], f"t{t}_nchw", perm=[0, 3, 1, 2])
        return nchw[t]

    def as_nhwc(t):
        if t not in nhwc:
            nhwc[t] = node("Transpose", [nchw[t]], f"t{t}_nhwc", perm=[0, 2, 3, 1])
        return nhwc[t]

    def act(x, a, tag):
        if a == mf.ACT_NONE:
            return x
        assert a == mf.ACT_GELU_ERF
        if gelu == "gelu":
            return node("Gelu", [x], tag + "_gelu")
        node("Div", [x, const(tag + "_sqrt2", np.float32(np.sqrt(2.0)))], tag + "_d")
        node("Erf", [tag + "_d"], tag + "_e")
        node("Add", [tag + "_e", const(tag + "_one", 1.0)], tag + "_a")
        node("Mul", [x, tag + "_a"], tag + "_m")
        return node("Mul", [tag + "_m", const(tag + "_half", 0.5)], tag + "_gelu")

    def chain(x, tag, axis, ga, be, eps):
        node("ReduceMean", [x], tag + "_mu", axes=[axis], keepdims=1)
        node("Sub", [x, tag + "_mu"], tag + "_dev")
        node("Pow", [tag + "_dev", const(tag + "_two", 2.0)], tag + "_sq")
        node("ReduceMean", [tag + "_sq"], tag + "_var", axes=[axis], keepdims=1)
        node("Add", [tag + "_var", const(tag + "_eps", np.float32(eps))], tag + "_ve")
        node("Sqrt", [tag + "_ve"], tag + "_sd")
        node("Div", [tag + "_dev", tag + "_sd"], tag + "_xh")
        node("Mul", [tag + "_xh", ga], tag + "_xg")
        return node("Add", [tag + "_xg", be], tag + "_ln")

    for i, L in enumerate(m.layers):
        tag, t = f"l{i}", i + 1
        W = m.blob[L.w_off:L.w_off + n_weights(L)]
        bias = m.blob[L.b_off:L.b_off + L.cout]
        if L.op in (mf.OP_CONV, mf.OP_DWCONV):
            w = W.reshape(L.kh, L.kw, L.cin, L.cout).transpose(3, 2, 0, 1) if L.op == mf.OP_CONV else W.reshape(L.kh, L.kw, L.cout).transpose(2, 0, 1)[:, None]
            pad_b = max((L.out_h - 1) * L.sh + L.kh - L.in_h - L.pad_t, 0)
            pad_r = max((L.out_w - 1) * L.sw + L.kw - L.in_w - L.pad_l, 0)
            nchw[t] = node("Conv", [as_nchw(L.in_tensor), const(tag + "_w", w), const(tag + "_b", bias)], tag + "_conv", group=1 if L.op == mf.OP_CONV else L.cout,
                           kernel_shape=[L.kh, L.kw], strides=[L.sh, L.sw], pads=[L.pad_t, L.pad_l, pad_b, pad_r])
        elif L.op == mf.OP_LNORM:
            eps = mf.lnorm_eps(L.reserved)
            pooled = L.in_h * L.in_w == 1 and m.layers[L.in_tensor - 1].op == mf.OP_GAP
            if pooled and head == "nchw11":
                nchw[t] = node("LayerNormalization", [as_nchw(L.in_tensor), const(tag + "_g", W), const(tag + "_be", bias)], tag + "_ln", axis=1, epsilon=eps)
            elif layout == "nchw" and not pooled:
                shp = (L.cout, 1, 1) if scale != "1c11" else (1, L.cout, 1, 1)
                nchw[t] = chain(as_nchw(L.in_tensor), tag, 1, const(tag + "_g", W.reshape(shp)), const(tag + "_be", bias.reshape(shp)), eps)
            elif ln == "node":
                ins = [as_nhwc(L.in_tensor), const(tag + "_g", W)] + ([const(tag + "_be", bias)] if beta else [])
                nhwc[t] = node("LayerNormalization", ins, tag + "_ln", axis=-1, epsilon=eps)
            else:
                nhwc[t] = chain(as_nhwc(L.in_tensor), tag, -1, const(tag + "_g", W), const(tag + "_be", bias), eps)
        elif L.op == mf.OP_PWCONV:
            Wm, b2, ls = m.convnext_scales.get(i, (W.reshape(L.cin, L.cout), bias, None))
            if layout == "nhwc":
                y = node("MatMul", [as_nhwc(L.in_tensor), const(tag + "_w", Wm)], tag + "_mm")
                y = act(node("Add", [y, const(tag + "_b", b2)], tag + "_lin"), L.act, tag)
                if ls is not None:
                    y = node("Mul", [const(tag + "_ls", ls), y], tag + "_scaled")
                nhwc[t] = y
            else:
                y = act(node("Conv", [as_nchw(L.in_tensor), const(tag + "_w", Wm.T[:, :, None, None]), const(tag + "_b", b2)], tag + "_conv", kernel_shape=[1, 1]), L.act, tag)
                if ls is not None:
                    y = node("Mul", [y, const(tag + "_ls", ls.reshape((L.cout, 1, 1) if scale != "1c11" else (1, L.cout, 1, 1)))], tag + "_scaled")
                nchw[t] = y
            if L.res_tensor != mf.NO_TENSOR:
                y = node("Add", [as_nchw(L.res_tensor), as_nchw(t)], tag + "_sum")
                nchw[t] = y
                nhwc.pop(t, None)
        elif L.op == mf.OP_GAP:
            nchw[t] = node("GlobalAveragePool", [as_nchw(L.in_tensor)], tag + "_gap")
        else:
            assert L.op == mf.OP_DENSE
            node("Flatten", [as_nchw(L.in_tensor)], tag + "_flat", axis=1)
            nchw[t] = node("Gemm", [tag + "_flat", const(tag + "_w", W.reshape(L.cin, L.cout)), const(tag + "_b", bias)], tag + "_fc")
    out = node("Sigmoid", [nchw[len(m.layers)]], "probabilities")
    g.outputs.append(ox.ValueInfo(out, ox.FLOAT, ["N", m.n_classes]))
    return g


def same_model(m, got):
    """the records of m (offsets aside) and, layer by layer, its weights"""
    assert len(got.layers) == len(m.layers), ([L.op for L in got.layers], [L.op for L in m.layers])
    for i, (x, y) in enumerate(zip(m.layers, got.layers)):
        for f in RECORD[:-2] + ("dil_h", "dil_w"):
            assert getattr(x, f) == getattr(y, f), (i, f, getattr(x, f), getattr(y, f))
        k = n_weights(x)
        assert m.blob[x.w_off:x.w_off + k].tobytes() == got.blob[y.w_off:y.w_off + k].tobytes(), (i, "weights")
        if k:
            assert m.blob[x.b_off:x.b_off + x.cout].tobytes() == got.blob[y.b_off:y.b_off + y.cout].tobytes(), (i, "bias")
    assert (got.embedding_tensor, got.embedding_dim, got.n_classes) == (m.embedding_tensor, m.embedding_dim, m.n_classes)


SPELLINGS = {
    "node_view": dict(),
    "node_view_erf_gelu": dict(gelu="erf"),
    "chain_view": dict(ln="chain"),
    "chain_channels_first_c11": dict(layout="nchw", scale="c11"),
    "chain_channels_first_1c11": dict(layout="nchw", scale="1c11", gelu="erf"),
    "head_on_nchw11": dict(head="nchw11"),
    "channels_first_head_on_nchw11": dict(layout="nchw", head="nchw11"),
}


@pytest.mark.parametrize("case", sorted(SPELLINGS))
def test_both_readers_give_the_synth_model_s_records(case, plan, tmp_path):
    g = torch_graph(plan, **SPELLINGS[case])
    ops = [n.op_type for n in g.nodes]
    if SPELLINGS[case].get("layout") == "nchw":
        assert ("Transpose" in ops) == (SPELLINGS[case].get("head") != "nchw11") and "MatMul" not in ops and ops.count("ReduceMean") >= 2
    else:
        assert "MatMul" in ops and "Transpose" in ops and ("LayerNormalization" in ops) == (SPELLINGS[case].get("ln", "node") == "node")
    assert any(n.op_type == "Mul" and any(k.endswith("_ls") for k in n.inputs) for n in g.nodes)           # un-folded layer scale
    want, got = both_readers(g, plan, tmp_path)
    same_tables_and_blob(want, got)
    same_model(plan, got)
    same_model(plan, want)


def test_without_beta_the_record_holds_zeros(plan, tmp_path):
    want, got = both_readers(torch_graph(plan, beta=False), plan, tmp_path)
    same_tables_and_blob(want, got)
    zeroed = copy.deepcopy(plan)
    for L in zeroed.layers:
        if L.op == mf.OP_LNORM and not (L.in_h * L.in_w == 1):
            zeroed.blob[L.b_off:L.b_off + L.cout] = 0.0
        elif L.op == mf.OP_LNORM:
            zeroed.blob[L.b_off:L.b_off + L.cout] = 0.0
    same_model(zeroed, got)
    assert any(plan.blob[L.b_off:L.b_off + L.cout].any() for L in plan.layers if L.op == mf.OP_LNORM)


@pytest.mark.parametrize("case", ["node_view", "chain_channels_first_c11"])
def test_both_readers_read_a_float16_file_alike(case, plan, tmp_path):
    """gamma, beta, eps and the layer scale as the exact values their float16 encodings hold"""
    g16 = convert.graph_to_float16(torch_graph(plan, **SPELLINGS[case]))
    assert all(a.dtype == np.float16 for a in g16.initializers.values() if a.dtype.kind == "f")
    want, got = both_readers(g16, plan, tmp_path)
    same_tables_and_blob(want, got)
    i = next(k for k, L in enumerate(plan.layers) if L.op == mf.OP_LNORM)
    L, M = plan.layers[i], got.layers[i]
    assert np.array_equal(got.blob[M.w_off:M.w_off + M.cout], plan.blob[L.w_off:L.w_off + L.cout].astype(np.float16).astype(np.float32))
    assert mf.lnorm_eps(M.reserved) == float(np.float32(np.float16(mf.lnorm_eps(L.reserved)))) or SPELLINGS[case].get("layout") != "nchw"
    j = min(plan.convnext_scales)
    W, b, ls = plan.convnext_scales[j]
    f16 = lambda a: a.astype(np.float16).astype(np.float32)
    P = got.layers[j]
    assert np.array_equal(got.blob[P.w_off:P.w_off + W.size].reshape(W.shape), f16(W) * f16(ls))       # one float32 product of the exact values
    assert np.array_equal(got.blob[P.b_off:P.b_off + b.size], f16(b) * f16(ls))


@pytest.mark.parametrize("spell", ["node", "chain"])
@pytest.mark.parametrize("kind", ["convnext_plan", "convnext_plan_seed0"])
def test_the_round_trip_is_record_exact(kind, spell, tmp_path):
    """.bhm -> .onnx (Transpose -> LayerNormalization(axis = -1, epsilon) -> Transpose, on a 1 x 1 image too) -> .bhm through either reader"""
    m = synth.build_model("convnext_plan", seed=0 if kind.endswith("0") else 3)
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    back = mf.read_model(path)
    assert back.layers == m.layers and np.array_equal(back.blob, m.blob)
    g = convert.graph_from_model(m, spell_lnorm=spell)
    n_ln = sum(L.op == mf.OP_LNORM for L in m.layers)
    assert [n.op_type for n in g.nodes].count("Transpose") == 2 * n_ln
    if spell == "node":
        assert [(n.attrs["axis"], np.float32(n.attrs["epsilon"])) for n in g.nodes if n.op_type == "LayerNormalization"] == \
               [(-1, np.float32(mf.lnorm_eps(L.reserved))) for L in m.layers if L.op == mf.OP_LNORM]
    rt = convert.model_from_graph(ox.load(ox.dump(g)), m)
    same_tables_and_blob(m, rt)
    assert rt.embedding_tensor == m.embedding_tensor
    # the library's reader from the audio input (its blob is laid out in its own order): the same records and weights
    onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m_native.bhm")
    with open(onnx_path, "wb") as f:
        f.write(convert.model_to_onnx(m, frontend_spelling="stft", spell_lnorm=spell))
    lib = _lib.load()
    assert lib.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, lib.bh_last_error()
    same_model(m, mf.read_model(out))


def test_code_12_in_the_file(plan, tmp_path):
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, plan)
    raw = open(path, "rb").read()
    n_b, n_l = struct.unpack_from("<II", raw, 32)
    for i, L in enumerate(plan.layers):
        rec = raw[mf.HEADER_SIZE + n_b * mf.BRANCH_SIZE + i * mf.LAYER_SIZE:][:mf.LAYER_SIZE]
        assert struct.unpack_from("<I", rec, 0)[0] == L.op and rec[88:] == bytes(40)
        if L.op == mf.OP_LNORM:
            assert L.op == 12 and struct.unpack_from("<f", rec, 68)[0] == np.float32(mf.lnorm_eps(L.reserved)) > 0       # `reserved`: the bits of eps
    assert mf.lnorm_eps(mf.lnorm_eps_bits(1e-6)) == float(np.float32(1e-6))


def test_existing_models_keep_their_bytes(tmp_path):
    """a model without the op is written, by either writer, as it always was: no code 12, nothing in the records' tails"""
    for kind in ("mini", "mini_se"):
        m = synth.build_model(kind)
        p = str(tmp_path / f"{kind}.bhm")
        mf.write_model(p, m)
        assert all(L.op != mf.OP_LNORM for L in mf.read_model(p).layers)
        g = convert.graph_from_model(m)
        assert not any(n.op_type in ("Transpose", "LayerNormalization") for n in g.nodes)
        same_tables_and_blob(m, convert.model_from_graph(ox.load(ox.dump(g)), m))


# ---- what both readers refuse ------------------------------------------------------------------------------------------------------
class Case:
    """spectrogram [N, 2, 32, 115] -> Conv 4x4 stride 4 (C channels, an 8 x 29 image) -> `body` -> GlobalAveragePool -> Flatten -> Gemm"""

    def __init__(self, C=8):
        self.rng = np.random.default_rng(7)
        self.g = ox.Graph(name="convnext_case", producer="tests")
        self.g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", 2, 32, 115]))
        self.C = C
        self.k = 0
        self.x = self.node("Conv", ["spectrogram", self.f32(C, 2, 4, 4), self.f32(C)], kernel_shape=[4, 4], strides=[4, 4], name="stem")

    def f32(self, *shape, value=None, dtype=np.float32):
        self.k += 1
        name = f"c{self.k}"
        self.g.initializers[name] = (self.rng.standard_normal(shape) if value is None else np.asarray(value)).astype(dtype).reshape(shape)
        return name

    def node(self, op, ins, name=None, outs=None, **attrs):
        self.k += 1
        outs = outs or [f"v{self.k}"]
        self.g.nodes.append(ox.Node(op, list(ins), list(outs), attrs, name=name or f"{op.lower()}_{self.k}"))
        return outs[0]

    def view(self, x=None):
        return self.node("Transpose", [x or self.x], perm=[0, 2, 3, 1])

    def back(self, x):
        return self.node("Transpose", [x], perm=[0, 3, 1, 2])

    def ln(self, x, C=None, name="the_norm", **attrs):
        C = C or self.C
        return self.node("LayerNormalization", [x, self.f32(C), self.f32(C)], name=name, **dict(dict(axis=-1, epsilon=1e-6), **attrs))

    def chain(self, x, axis=-1, shape=None, exponent=2.0, axis2=None, eps=1e-6, tap=None):
        shape = shape or (self.C,)
        mu = self.node("ReduceMean", [x], name="the_mean", axes=[axis], keepdims=1)
        d = self.node("Sub", [x, mu], name="the_sub")
        sq = self.node("Pow", [d, self.f32(value=exponent)], name="the_pow")
        var = self.node("ReduceMean", [sq], name="the_variance", axes=[axis if axis2 is None else axis2], keepdims=1)
        if tap == "variance":
            self.extra = self.node("Relu", [var], name="a_second_reader")
        sd = self.node("Sqrt", [var if eps is None else self.node("Add", [var, self.f32(value=eps)], name="the_eps")], name="the_sqrt")
        xh = self.node("Div", [d, sd], name="the_div")
        return self.node("Add", [self.node("Mul", [xh, self.f32(*shape)], name="the_gamma"), self.f32(*shape)], name="the_beta")

    def finish(self, x, C=None):
        C = C or self.C
        p = self.node("GlobalAveragePool", [x])
        f = self.node("Flatten", [p], axis=1)
        y = self.node("Gemm", [f, self.f32(C, 10), self.f32(10)], outs=["logits"])
        self.g.outputs.append(ox.ValueInfo("logits", ox.FLOAT, ["N", 10]))
        return self.g


def _refused(kind):
    c = Case(6 if kind == "ln_six_channels" else 8)
    C = c.C
    if kind == "transpose_other_perm":
        return c.finish(c.node("Transpose", [c.x], name="the_transpose", perm=[0, 1, 3, 2]))
    if kind == "transpose_back_on_a_map":
        return c.finish(c.node("Transpose", [c.x], name="the_transpose", perm=[0, 3, 1, 2]))
    if kind == "transpose_twice":
        return c.finish(c.back(c.node("Transpose", [c.view()], name="the_transpose", perm=[0, 2, 3, 1])))
    if kind == "transpose_of_the_spectrogram":
        return c.finish(c.back(c.ln(c.node("Transpose", ["spectrogram"], name="the_transpose", perm=[0, 2, 3, 1]), C=2)), C=2)
    if kind == "conv_on_a_view":
        return c.finish(c.node("Conv", [c.ln(c.view()), c.f32(C, C, 1, 1), c.f32(C)], name="the_conv", kernel_shape=[1, 1]))
    if kind == "residual_add_on_a_view":
        v = c.view()
        return c.finish(c.back(c.node("Add", [c.ln(v), v], name="the_add")))
    if kind == "gemm_on_a_view":
        return c.finish(c.back(c.node("Gemm", [c.ln(c.view()), c.f32(C, C), c.f32(C)], name="the_gemm")))
    if kind == "pool_on_a_view":
        c.node("GlobalAveragePool", [c.ln(c.view())], name="the_pool", outs=["p"])
        return c.finish(c.x)
    if kind == "ln_axis_1_on_a_view":
        return c.finish(c.back(c.ln(c.view(), axis=1)))
    if kind == "ln_on_an_nchw_image":
        return c.finish(c.ln(c.x, axis=1))
    if kind == "ln_last_axis_of_nchw":
        return c.finish(c.ln(c.x, axis=-1))
    if kind == "ln_mean_output_read":
        v = c.view()
        y = c.node("LayerNormalization", [v, c.f32(C), c.f32(C)], name="the_norm", outs=["y", "mean_out"], axis=-1)
        c.g.outputs.append(ox.ValueInfo("mean_out", ox.FLOAT, ["N", 8, 29, 1]))
        g = c.finish(c.back(y))
        g.outputs.reverse()
        return g
    if kind == "ln_gamma_is_no_constant":
        v = c.view()
        return c.finish(c.back(c.node("LayerNormalization", [v, v, c.f32(C)], name="the_norm", axis=-1)))
    if kind == "ln_gamma_of_another_width":
        v = c.view()
        return c.finish(c.back(c.node("LayerNormalization", [v, c.f32(C + 4), c.f32(C)], name="the_norm", axis=-1)))
    if kind == "ln_six_channels":
        return c.finish(c.back(c.ln(c.view())))
    if kind == "ln_eps_zero":
        return c.finish(c.back(c.ln(c.view(), epsilon=0.0)))
    if kind == "activation_behind_the_norm":
        return c.finish(c.back(c.node("Relu", [c.ln(c.view())], name="the_relu")))
    if kind == "chain_exponent_3":
        return c.finish(c.back(c.chain(c.view(), exponent=3.0)))
    if kind == "chain_second_mean_over_another_axis":
        return c.finish(c.back(c.chain(c.view(), axis2=2)))
    if kind == "chain_without_eps":
        return c.finish(c.back(c.chain(c.view(), eps=None)))
    if kind == "chain_variance_read_twice":
        return c.finish(c.back(c.chain(c.view(), tap="variance")))
    if kind == "chain_axis_1_on_a_view":
        return c.finish(c.back(c.chain(c.view(), axis=1)))
    if kind == "chain_last_axis_of_nchw":
        return c.finish(c.chain(c.x, axis=-1, shape=(C, 1, 1)))
    if kind == "chain_gamma_shaped_for_the_view_on_nchw":
        return c.finish(c.chain(c.x, axis=1, shape=(C,)))
    if kind == "matmul_of_another_width":
        return c.finish(c.back(c.node("MatMul", [c.ln(c.view()), c.f32(C + 4, C)], name="the_matmul")), C=C)
    if kind == "scale_behind_an_activation_on_a_view":
        y = c.node("Gelu", [c.node("MatMul", [c.ln(c.view()), c.f32(C, C)], name="the_matmul")])
        return c.finish(c.back(c.node("Mul", [y, c.f32(C)], name="the_scale")))
    if kind == "scale_of_a_tensor_read_twice_on_a_view":
        y = c.node("MatMul", [c.ln(c.view()), c.f32(C, C)], name="the_matmul")
        s = c.node("Mul", [y, c.f32(C)], name="the_scale")
        c.node("Relu", [y], name="another_reader")
        return c.finish(c.back(s))
    if kind == "scale_behind_an_activation_on_nchw":
        y = c.node("Relu", [c.node("Conv", [c.x, c.f32(C, C, 1, 1), c.f32(C)], kernel_shape=[1, 1])])
        return c.finish(c.node("Mul", [y, c.f32(C, 1, 1)], name="the_scale"))
    if kind == "scale_shaped_for_the_view_on_nchw":
        y = c.node("Conv", [c.x, c.f32(C, C, 1, 1), c.f32(C)], kernel_shape=[1, 1])
        return c.finish(c.node("Mul", [y, c.f32(C)], name="the_scale"))
    raise KeyError(kind)


# kind -> the words both refusals hold
REFUSED = {
    "transpose_other_perm": ("Transpose", "perm"),
    "transpose_back_on_a_map": ("Transpose", "perm"),
    "transpose_twice": ("Transpose", "view"),
    "transpose_of_the_spectrogram": ("Transpose", "spectrogram"),
    "conv_on_a_view": ("Conv", "[N, H, W, C] view"),
    "residual_add_on_a_view": ("Add", "[N, H, W, C] view"),
    "gemm_on_a_view": ("Gemm", "[N, H, W, C] view"),
    "pool_on_a_view": ("GlobalAveragePool", "[N, H, W, C] view"),
    "ln_axis_1_on_a_view": ("LayerNormalization", "axis 1"),
    "ln_on_an_nchw_image": ("LayerNormalization", "more than the channels"),
    "ln_last_axis_of_nchw": ("LayerNormalization", "more than the channels"),
    "ln_mean_output_read": ("LayerNormalization", "Mean"),
    "ln_gamma_is_no_constant": ("LayerNormalization", "gamma / beta"),
    "ln_gamma_of_another_width": ("LayerNormalization", "gamma / beta"),
    "ln_six_channels": ("LayerNormalization", "multiple of 4"),
    "ln_eps_zero": ("LayerNormalization", "epsilon"),
    "activation_behind_the_norm": ("activation", "LayerNormalization"),
    "chain_exponent_3": ("the_pow", "exponent"),
    "chain_second_mean_over_another_axis": ("the_variance", "another axis"),
    "chain_without_eps": ("the_sqrt", "missing eps"),
    "chain_variance_read_twice": ("the_variance", "second reader"),
    "chain_axis_1_on_a_view": ("the_mean", "another axis"),
    "chain_last_axis_of_nchw": ("the_mean", "another axis"),
    "chain_gamma_shaped_for_the_view_on_nchw": ("the_mean", "gamma / beta"),
    "matmul_of_another_width": ("MatMul", "input features"),
    "scale_behind_an_activation_on_a_view": ("Mul", "layer scale"),
    "scale_of_a_tensor_read_twice_on_a_view": ("Mul", "layer scale"),
    "scale_behind_an_activation_on_nchw": ("Mul", "not both activations"),          # today's refusal of a Mul by a constant
    "scale_shaped_for_the_view_on_nchw": ("Mul", "not both activations"),
}


@pytest.mark.parametrize("kind", sorted(REFUSED))
def test_both_readers_refuse_by_name(kind, plan, tmp_path):
    g = _refused(kind)
    data = ox.dump(g)
    with pytest.raises(convert.ConvertError) as e:
        convert.model_from_graph(ox.load(data), plan)
    for word in REFUSED[kind]:
        assert word in str(e.value), (kind, word, str(e.value))
    onnx_path = str(tmp_path / "case.onnx")
    with open(onnx_path, "wb") as f:
        f.write(data)
    lib = _lib.load()
    rc = lib.bh_onnx_to_bhm(onnx_path.encode(), str(tmp_path / "case.bhm").encode())
    msg = lib.bh_last_error().decode()
    assert rc != 0, kind
    for word in REFUSED[kind]:
        assert word in msg, (kind, word, msg)


def test_the_refused_graphs_are_one_step_from_accepted_ones(plan, tmp_path):
    """the same builder's well-formed graphs load through both readers (so each refusal above is about its one deviation)"""
    def ok(build):
        c = Case()
        want, got = both_readers(build(c), plan, tmp_path)
        same_tables_and_blob(want, got)
        return got
    got = ok(lambda c: c.finish(c.back(c.ln(c.view()))))
    assert [L.op for L in got.layers] == [mf.OP_CONV, mf.OP_LNORM, mf.OP_GAP, mf.OP_DENSE] and got.embedding_tensor == 3
    got = ok(lambda c: c.finish(c.back(c.chain(c.view()))))
    assert got.layers[1].op == mf.OP_LNORM and mf.lnorm_eps(got.layers[1].reserved) == float(np.float32(1e-6))
    got = ok(lambda c: c.finish(c.chain(c.x, axis=1, shape=(1, c.C, 1, 1))))
    assert got.layers[1].op == mf.OP_LNORM
    got = ok(lambda c: c.finish(c.back(c.node("Mul", [c.node("MatMul", [c.ln(c.view()), c.f32(c.C, c.C)]), c.f32(c.C)]))))
    assert [L.op for L in got.layers] == [mf.OP_CONV, mf.OP_LNORM, mf.OP_PWCONV, mf.OP_GAP, mf.OP_DENSE] and not got.blob[got.layers[2].b_off:][:8].any()
    got = ok(lambda c: c.finish(c.node("Mul", [c.node("Conv", [c.x, c.f32(c.C, c.C, 1, 1), c.f32(c.C)], kernel_shape=[1, 1]), c.f32(c.C, 1, 1)])))
    assert [L.op for L in got.layers] == [mf.OP_CONV, mf.OP_PWCONV, mf.OP_GAP, mf.OP_DENSE]
    # LayerNormalization's extra outputs may be declared as long as nothing reads them; stash_type is ignored
    got = ok(lambda c: c.finish(c.back(c.node("LayerNormalization", [c.view(), c.f32(c.C), c.f32(c.C)], outs=["y", "mu", "isd"], axis=3, stash_type=1))))
    assert got.layers[1].op == mf.OP_LNORM and mf.lnorm_eps(got.layers[1].reserved) == float(np.float32(1e-5))     # the operator's default epsilon


# ---- the validator -----------------------------------------------------------------------------------------------------------------
def _load(path):
    """bh_plan_fused_blocks walks a model file on the host: load_model + validate_model; >= 0 = loaded (the fused blocks' count)"""
    L = _lib.load()
    rc = L.bh_plan_fused_blocks(path.encode(), 0, None, None, 0)
    return rc, L.bh_last_error().decode()


def _first_norm(m, pooled=False):
    return next(i for i, L in enumerate(m.layers) if L.op == mf.OP_LNORM and (L.in_h * L.in_w == 1) == pooled)


_NAN_BITS, _INF_BITS, _NEG_BITS = 0x7fc00000, 0x7f800000, mf.lnorm_eps_bits(-1e-6)
# case -> (the change to the first norm record -- a callable (model, record) or a dict of fields --, the validator's reason)
BAD_RECORDS = {
    "activation": (dict(act=mf.ACT_RELU), "layer norm with an activation"),
    "residual": (lambda m, L: setattr(L, "res_tensor", L.in_tensor), "layer norm with a residual"),
    "kernel": (dict(kh=3), "kernel, stride or padding other than 1 / 1 / 0"),
    "stride": (dict(sw=2), "kernel, stride or padding other than 1 / 1 / 0"),
    "padding": (dict(pad_t=1), "kernel, stride or padding other than 1 / 1 / 0"),
    "changed_image": (lambda m, L: setattr(L, "out_w", L.out_w - 1), "output image is not its input image"),
    "changed_channels": (lambda m, L: setattr(L, "cout", L.cout + 4), "changes the channel count"),
    "planar_layout": (dict(in_layout=1), "planar spectrogram (tensor 0)"),
    "eps_zero": (dict(reserved=0), "epsilon that is not finite and > 0"),
    "eps_negative": (dict(reserved=_NEG_BITS), "epsilon that is not finite and > 0"),
    "eps_nan": (dict(reserved=_NAN_BITS), "epsilon that is not finite and > 0"),
    "eps_inf": (dict(reserved=_INF_BITS), "epsilon that is not finite and > 0"),
    "gamma_outside": (lambda m, L: setattr(L, "w_off", len(m.blob) - L.cout + 1), "gamma / beta outside the blob"),
    "beta_outside": (lambda m, L: setattr(L, "b_off", 1 << 40), "gamma / beta outside the blob"),
    "dilation": (dict(dil_h=2), "dilation on a layer norm layer"),
}


@pytest.mark.parametrize("case", sorted(BAD_RECORDS))
def test_the_validator_refuses_a_bad_norm_record(case, plan, tmp_path):
    change, reason = BAD_RECORDS[case]
    m = copy.deepcopy(plan)
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg                                   # the model loads as it stands
    L = m.layers[_first_norm(m)]
    if callable(change):
        change(m, L)
    else:
        for k, v in change.items():
            setattr(L, k, v)
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and reason in msg, (rc, msg)


def test_the_validator_refuses_tensor_0_six_channels_and_the_unused_codes(tmp_path):
    # a norm that reads the spectrogram: 2 channels are no multiple of 4 either, so the model gets a 4-branch spectrogram's worth of
    # channels from a stem and the record is then pointed at tensor 0 with matching sizes
    m = synth.build_model("convnext_plan", seed=1)
    path = str(tmp_path / "m.bhm")
    i = _first_norm(m)
    L = m.layers[i]
    m2 = copy.deepcopy(m)
    N = m2.layers[i]
    N.in_tensor, N.cin, N.cout, N.in_h, N.in_w, N.out_h, N.out_w = 0, 2, 2, m.spec_h, m.spec_w, m.spec_h, m.spec_w
    mf.write_model(path, m2)
    rc, msg = _load(path)
    assert rc < 0 and "tensor 0" in msg, msg
    # C % 4 != 0: the stem and its norm at 6 channels
    m3 = synth.build_model("convnext_plan", plan=dict(widths=(6,), depths=(0,), eps=1e-6, classes=8), seed=1)
    mf.write_model(path, m3)
    rc, msg = _load(path)
    assert rc < 0 and "not a multiple of 4" in msg, msg
    # 9 and 11 stay unknown; 13 is past the table
    for code in (9, 11, 13):
        m4 = copy.deepcopy(m)
        m4.layers[i].op = code
        mf.write_model(path, m4)
        rc, msg = _load(path)
        assert rc < 0 and "unknown layer op" in msg, (code, msg)
    assert L.op == 12


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def test_no_matcher_takes_a_record_run_with_a_norm(tmp_path):
    """pw -> dw -> LayerNorm is no inverted-residual block, dw -> LayerNorm -> pw no depthwise-project block, and a 7x7 depthwise is
    none the fused tile kernel computes: convnext_plan has no fused block in any precision; the same pw -> dw -> pw run with the norm
    taken out and a 3x3 window is fused"""
    lib = _lib.load()
    base = synth.build_model("mini")
    m = synth.build_model("convnext_plan", seed=1)
    path = str(tmp_path / "m.bhm")
    for flags in (0, 1, 2, 3):          # BH_FLAG_AUTO, _F16X3, _F16, _F32
        mf.write_model(path, m)
        assert lib.bh_plan_fused_blocks(path.encode(), flags, None, None, 0) == 0, (flags, lib.bh_last_error())
    # pw -> dw 3x3 -> LN -> pw: with the norm it runs layer by layer, without it the three convolutions fuse
    def stack(with_norm):
        b = synth._Builder(np.random.default_rng(3))
        br = [copy.deepcopy(x) for x in base.branches]
        for x in br:
            x.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(x.n_mels, x.n_bins, base.sample_rate, x.fmin, x.fmax))
        t, h, w = b.conv(0, 32, 115, 2, 8, 3, 2, mf.ACT_RELU, in_layout=1)
        x0 = t
        t = b.pwconv(t, h, w, 8, 32, mf.ACT_RELU6)
        t, h, w = b.dwconv(t, h, w, 32, 3, 1, mf.ACT_RELU6)
        if with_norm:
            t = b.lnorm(t, h, w, 32)
        t = b.pwconv(t, h, w, 32, 8, mf.ACT_NONE, x0)
        t = emb = b.gap(t, h, w, 8)
        b.dense(t, 8, 10)
        return synth._finish(b, br, base.sample_rate, base.sample_count, 10, 8, emb, mf.OUT_SIGMOID)
    layers = np.zeros(16, np.int32)
    mf.write_model(path, stack(True))
    assert lib.bh_plan_fused_blocks(path.encode(), 1, None, layers.ctypes.data, 16) == 0, lib.bh_last_error()
    mf.write_model(path, stack(False))
    assert lib.bh_plan_fused_blocks(path.encode(), 1, None, layers.ctypes.data, 16) >= 1 and int(layers[0]) == 1


# ---- fails without the feature -----------------------------------------------------------------------------------------------------
def test_a_convnext_file_loads_through_both_routes(plan, tmp_path):
    """before this op existed the .onnx route ended in 'unsupported operator Transpose' and the .bhm route in 'unknown layer op'"""
    lib = _lib.load()
    onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m_native.bhm")
    with open(onnx_path, "wb") as f:
        f.write(ox.dump(torch_graph(plan, frontend="stft")))
    assert lib.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, lib.bh_last_error()
    same_model(plan, mf.read_model(out))
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, plan)
    rc, msg = _load(path)
    assert rc == 0, msg


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------
def test_mutated_convnext_files_are_refused_or_read_never_a_crash():
    """tools/fuzz_onnx_reader.py over ConvNeXt graphs (the node and the decomposed chain, from the audio input and from the
    spectrogram) and containers with code-12 records, in child processes: every mutant loads or is refused"""
    env = dict(os.environ, FUZZ_CONVNEXT="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_onnx_reader.py"), "160", "5"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-600:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("160 mutants, 0 bad batches"), r.stdout[-800:]
    assert "'0':" in last and "'-2':" in last, last
