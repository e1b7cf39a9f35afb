"""ctypes binding of the CPU oracle (oracle/birda_oracle.c).

TEST INFRASTRUCTURE ONLY: import this from tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg -- never from birda_amd/.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
from typing import List, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libbirda_oracle.so")
_lib = None

f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")


def build(force: bool = False) -> str:
    src = os.path.join(_HERE, "birda_oracle.c")
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(src):
        subprocess.run(["make", "-C", _HERE], check=True, capture_output=True)
    return _SO


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        build()
    L = C.CDLL(_SO)
    L.bo_model_load.restype = C.c_void_p
    L.bo_model_load.argtypes = [C.c_char_p]
    L.bo_model_free.argtypes = [C.c_void_p]
    for name in ("bo_sample_rate", "bo_sample_count", "bo_n_classes", "bo_embedding_dim", "bo_n_layers"):
        getattr(L, name).restype = C.c_uint32
        getattr(L, name).argtypes = [C.c_void_p]
    L.bo_segment_duration.restype = C.c_float
    L.bo_segment_duration.argtypes = [C.c_void_p]
    L.bo_tensor_floats.restype = C.c_uint64
    L.bo_tensor_floats.argtypes = [C.c_void_p, C.c_uint32]
    L.bo_frontend.argtypes = [C.c_void_p, f32p, f32p]
    L.bo_forward.restype = C.c_int
    L.bo_forward.argtypes = [C.c_void_p, f32p, C.c_int, f32p, C.c_void_p, C.c_int, C.c_void_p]
    L.bo_topk.restype = C.c_int
    L.bo_topk.argtypes = [f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.bo_fft.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int]
    L.bo_scientific_name_len.restype = C.c_size_t
    L.bo_scientific_name_len.argtypes = [C.c_char_p]
    L.bo_project_scores.restype = C.c_size_t
    L.bo_project_scores.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bo_filter_predictions.restype = C.c_int
    L.bo_filter_predictions.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.bo_species_retain.restype = C.c_int
    L.bo_species_retain.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bo_pcm16_to_mono.argtypes = [C.c_void_p, C.c_size_t, C.c_int, f32p]
    L.bo_pcm32_to_mono.argtypes = [C.c_void_p, C.c_size_t, C.c_int, f32p]
    L.bo_f32_to_mono.argtypes = [f32p, C.c_size_t, C.c_int, f32p]
    L.bo_segmenter_new.restype = C.c_void_p
    L.bo_segmenter_new.argtypes = [f32p, C.c_size_t, C.c_size_t]
    L.bo_segmenter_free.argtypes = [C.c_void_p]
    L.bo_segmenter_next.restype = C.c_int
    L.bo_segmenter_next.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, f32p, C.POINTER(C.c_size_t)]
    L.bo_source_samples.restype = C.c_size_t
    L.bo_source_samples.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32]
    L.bo_duration_to_samples.restype = C.c_size_t
    L.bo_duration_to_samples.argtypes = [C.c_float, C.c_uint32]
    L.bo_estimate_segment_count.restype = C.c_int64
    L.bo_estimate_segment_count.argtypes = [C.c_int, C.c_double, C.c_float, C.c_float]
    L.bo_effective_batch_size.restype = C.c_size_t
    L.bo_effective_batch_size.argtypes = [C.c_size_t, C.c_int64]
    L.bo_chunk_times.argtypes = [C.c_size_t, C.c_uint32, C.c_size_t, C.c_uint32, C.POINTER(C.c_float),
                                 C.POINTER(C.c_float)]
    L.bo_chunk_audio_count.restype = C.c_size_t
    L.bo_chunk_audio_count.argtypes = [C.c_size_t, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_size_t]
    L.bo_resampler_sizes.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.bo_resample_max_len.restype = C.c_size_t
    L.bo_resample_max_len.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32]
    L.bo_resample.restype = C.c_size_t
    L.bo_resample.argtypes = [f32p, C.c_size_t, C.c_uint32, C.c_uint32, f32p]
    L.bo_sort_detections.argtypes = [C.c_void_p, C.c_size_t]
    L.bo_csv_row.restype = C.c_size_t
    L.bo_csv_row.argtypes = [C.c_char_p, C.c_float, C.c_float, C.c_float, C.c_char_p, C.c_char_p]
    L.bo_csv_header.restype = C.c_size_t
    L.bo_csv_header.argtypes = [C.c_int, C.c_char_p]
    L.bo_process_stream.restype = C.c_size_t
    L.bo_process_stream.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), f32p, C.c_size_t, C.c_uint32, C.c_float,
                                    C.c_float, C.c_int, C.c_size_t, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t,
                                    C.c_void_p, C.c_size_t, C.c_void_p]
    _lib = L
    return L


class Detection(C.Structure):
    _fields_ = [("start", C.c_float), ("end", C.c_float), ("conf", C.c_float), ("label", C.c_int)]


class ProcessStats(C.Structure):
    _fields_ = [("n_segments", C.c_size_t), ("n_detections", C.c_size_t), ("effective_batch", C.c_size_t),
                ("n_batches", C.c_size_t), ("n_padded_rows", C.c_size_t)]


class OracleModel:
    """CPU forward of a BHM1 model (restates birdnet_onnx::Classifier for this path)."""

    def __init__(self, path: str):
        self.L = lib()
        self.h = self.L.bo_model_load(path.encode())
        if not self.h:
            raise RuntimeError(f"oracle: cannot load {path}")
        self.sample_rate = self.L.bo_sample_rate(self.h)
        self.sample_count = self.L.bo_sample_count(self.h)
        self.segment_duration = self.L.bo_segment_duration(self.h)
        self.n_classes = self.L.bo_n_classes(self.h)
        self.embedding_dim = self.L.bo_embedding_dim(self.h)
        self.n_layers = self.L.bo_n_layers(self.h)

    def close(self):
        if self.h:
            self.L.bo_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tensor_floats(self, t: int) -> int:
        return int(self.L.bo_tensor_floats(self.h, t))

    def frontend(self, seg: np.ndarray) -> np.ndarray:
        seg = np.ascontiguousarray(seg, np.float32)
        out = np.empty(self.tensor_floats(0), np.float32)
        self.L.bo_frontend(self.h, seg, out)
        return out

    def forward(self, segs: np.ndarray, dump_tensor: int = -1, want_embeddings: bool = False):
        segs = np.ascontiguousarray(segs, np.float32).reshape(-1, self.sample_count)
        n = segs.shape[0]
        logits = np.empty((n, self.n_classes), np.float32)
        emb = np.empty((n, self.embedding_dim), np.float32) if want_embeddings else None
        dump = np.empty((n, self.tensor_floats(dump_tensor)), np.float32) if dump_tensor >= 0 else None
        self.L.bo_forward(self.h, segs, n, logits, emb.ctypes.data if emb is not None else None,
                          dump_tensor, dump.ctypes.data if dump is not None else None)
        res = [logits]
        if want_embeddings:
            res.append(emb)
        if dump_tensor >= 0:
            res.append(dump)
        return res[0] if len(res) == 1 else tuple(res)

    def process_stream(self, labels: List[str], samples: np.ndarray, source_rate: int, overlap: float = 0.0,
                       min_conf: float = 0.1, top_k: int = 5, batch_size: int = 8, bom: bool = True,
                       file_path: str = "audio.wav", want_logits: bool = False):
        samples = np.ascontiguousarray(samples, np.float32)
        arr = (C.c_char_p * len(labels))(*[s.encode("utf-8") for s in labels])
        cap = 1 << 22
        buf = C.create_string_buffer(cap)
        stats = ProcessStats()
        max_rows = int(len(samples) / source_rate / max(self.segment_duration - overlap, 1e-3)) + 8
        logits = np.zeros((max_rows, self.n_classes), np.float32) if want_logits else None
        n = self.L.bo_process_stream(self.h, arr, samples, len(samples), source_rate, overlap, min_conf, top_k,
                                     batch_size, int(bom), file_path.encode(), buf, cap,
                                     logits.ctypes.data if want_logits else None, max_rows, C.byref(stats))
        if n == C.c_size_t(-1).value:
            raise RuntimeError("oracle: process_stream failed")
        out = buf.raw[:n]
        if want_logits:
            return out, stats, logits[:stats.n_segments]
        return out, stats


def topk(logits: np.ndarray, out_act: int, top_k: int, min_conf: float) -> Tuple[np.ndarray, np.ndarray]:
    L = lib()
    logits = np.ascontiguousarray(logits, np.float32)
    idx = np.zeros(top_k, np.int32)
    conf = np.zeros(top_k, np.float32)
    k = L.bo_topk(logits, logits.size, out_act, top_k, min_conf, idx.ctypes.data, conf.ctypes.data)
    return idx[:k].copy(), conf[:k].copy()


def scientific_name(label: str) -> str:
    raw = label.encode("utf-8")
    return raw[:lib().bo_scientific_name_len(raw)].decode("utf-8")


def _cstrs(items):
    raw = [s.encode("utf-8") for s in items]
    return (C.c_char_p * max(1, len(raw)))(*raw), raw


def project_scores(geo_labels, reported, cls_labels) -> Tuple[np.ndarray, int]:
    """reported: [(geomodel species label, score)].  Returns (per-class scores with NaN = no geomodel entry, mapped count)."""
    L = lib()
    g, _g = _cstrs(geo_labels)
    sp, _s = _cstrs([r[0] for r in reported])
    c, _c = _cstrs(cls_labels)
    vals = np.asarray([r[1] for r in reported] or [0.0], np.float32)
    out = np.zeros(max(1, len(cls_labels)), np.float32)
    mapped = L.bo_project_scores(g, len(geo_labels), sp, vals.ctypes.data, len(reported), c, len(cls_labels), out.ctypes.data)
    return out[:len(cls_labels)].copy(), int(mapped)


def filter_predictions(idx, conf, scores, threshold: float, keep_unmatched: bool, rerank: bool):
    L = lib()
    idx = np.ascontiguousarray(idx, np.int32); conf = np.ascontiguousarray(conf, np.float32)
    scores = np.ascontiguousarray(scores, np.float32)
    oi = np.zeros(max(1, idx.size), np.int32); oc = np.zeros(max(1, idx.size), np.float32)
    k = L.bo_filter_predictions(idx.ctypes.data, conf.ctypes.data, idx.size, scores.ctypes.data, threshold,
                                int(keep_unmatched), int(rerank), oi.ctypes.data, oc.ctypes.data)
    return oi[:k].copy(), oc[:k].copy()


def species_retain(idx, conf, keep):
    L = lib()
    idx = np.ascontiguousarray(idx, np.int32); conf = np.ascontiguousarray(conf, np.float32)
    keep = np.ascontiguousarray(keep, np.uint8)
    oi = np.zeros(max(1, idx.size), np.int32); oc = np.zeros(max(1, idx.size), np.float32)
    k = L.bo_species_retain(idx.ctypes.data, conf.ctypes.data, idx.size, keep.ctypes.data, oi.ctypes.data, oc.ctypes.data)
    return oi[:k].copy(), oc[:k].copy()


def fft(x: np.ndarray, sign: int = -1) -> np.ndarray:
    L = lib()
    x = np.asarray(x, np.complex128)
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    ore, oim = np.empty_like(re), np.empty_like(im)
    L.bo_fft(re.ctypes.data, im.ctypes.data, ore.ctypes.data, oim.ctypes.data, x.size, sign)
    return ore + 1j * oim


def resample(x: np.ndarray, from_rate: int, to_rate: int) -> np.ndarray:
    L = lib()
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(max(int(L.bo_resample_max_len(x.size, from_rate, to_rate)), 1), np.float32)
    n = L.bo_resample(x, x.size, from_rate, to_rate, out)
    return out[:n].copy()


def resampler_sizes(from_rate: int, to_rate: int, chunk: int = 1024) -> Tuple[int, int]:
    L = lib()
    a, b = C.c_int(), C.c_int()
    L.bo_resampler_sizes(from_rate, to_rate, chunk, C.byref(a), C.byref(b))
    return a.value, b.value


def segment_stream(samples: np.ndarray, seg: int, ovl: int, packet: int = 1152):
    """[(segment, start_sample)] exactly as StreamingDecoder::next_segment would yield."""
    L = lib()
    samples = np.ascontiguousarray(samples, np.float32)
    keep = samples if samples.size else np.zeros(1, np.float32)
    h = L.bo_segmenter_new(keep, samples.size, packet)
    out = []
    try:
        while True:
            buf = np.empty(max(seg, 1), np.float32)
            start = C.c_size_t()
            rc = L.bo_segmenter_next(h, seg, ovl, buf, C.byref(start))
            if rc < 0:
                raise ValueError("overlap_samples must be less than segment_samples")
            if rc == 0:
                break
            out.append((buf, start.value))
    finally:
        L.bo_segmenter_free(h)
    return out


# --------------------------------------------------------------------------------------------------------
# Two-stage inference and BSG post-processing, numpy restatements.  TEST INFRASTRUCTURE like the rest of
# this package.  [EXT] Both live in birdnet-onnx (CustomClassifier, BsgPostProcessor), not in the reference tree: parity
# unpinned; the forms below are the ones include/birda_hip.h states.
# --------------------------------------------------------------------------------------------------------
def custom_classifier_forward(model, embeddings: np.ndarray) -> np.ndarray:
    """birdnet_onnx::CustomClassifier::predict_batch up to the logits (reference call site src/pipeline/processor.rs:341):
    dense layers x W + b with the layer activation (0 none, 1 ReLU), float32 like ONNX Runtime's Gemm."""
    x = np.asarray(embeddings, np.float32)
    for L in model.layers:
        x = (x.astype(np.float64) @ L.w.astype(np.float64) + L.b.astype(np.float64)).astype(np.float32)
        if L.act == 1:
            x = np.maximum(x, 0.0)
        elif L.act != 0:
            raise ValueError("activation not restated")
    return x


def bsg_postprocess(index: np.ndarray, confidence: np.ndarray, intercept: np.ndarray, slope: np.ndarray,
                    prior: Optional[np.ndarray] = None):
    """BirdClassifier::apply_bsg_postprocessing (reference src/inference/classifier.rs:508-545) on one segment's kept
    predictions: conf' = sigmoid(intercept[c] + slope[c] * logit(conf)) (* prior[c]), stable re-sort descending.
    The confidence is clamped to the FLOAT32 numbers 1e-7f and 1.0f - 1e-7f (= 1 - 2^-23: the largest logit the calibration sees is
    15.942, not the 16.118 of a float64 clamp) as the device does (kernels.hpp, TopkFilter); everything else is float64."""
    idx = [int(i) for i in index if i >= 0]
    out = []
    lo, hi = float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7))
    for c, p in zip(idx, confidence):
        p = min(max(float(p), lo), hi)
        lg = np.log(p / (1.0 - p))
        q = 1.0 / (1.0 + np.exp(-(float(intercept[c]) + float(slope[c]) * lg)))
        if prior is not None:
            q *= float(prior[c])
        out.append((c, q))
    order = sorted(range(len(out)), key=lambda i: -out[i][1])     # sorted() is stable: ties keep their order
    return [out[i][0] for i in order], [out[i][1] for i in order]


# --------------------------------------------------------------------------------------------------------
# The layer GEMMs and full convolutions (kernels_conv.hip) in float64, numpy restatements for tests/test_layer_gemm*.py.
# Activation codes as in the model file (kernels.hpp Act).
# --------------------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SWISH, ACT_GELU_ERF, ACT_GELU_TANH, ACT_SIGMOID = range(7)
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_RELU6: "relu6", ACT_SWISH: "swish", ACT_GELU_ERF: "gelu",
             ACT_GELU_TANH: "gelu_tanh", ACT_SIGMOID: "sigmoid"}
_erf = np.frompyfunc(math.erf, 1, 1)


def _sigmoid64(v: np.ndarray) -> np.ndarray:
    e = np.exp(-np.abs(v))                  # never overflows
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def act64(v, act: int) -> np.ndarray:
    """The activation `act` in float64: GELU through math.erf, the tanh form of GELU as ONNX / PyTorch state it."""
    v = np.asarray(v, np.float64)
    if act == ACT_NONE:
        return v.copy()
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_RELU6:
        return np.minimum(np.maximum(v, 0.0), 6.0)
    if act == ACT_SWISH:
        return v * _sigmoid64(v)
    if act == ACT_SIGMOID:
        return _sigmoid64(v)
    if act == ACT_GELU_ERF:
        return 0.5 * v * (1.0 + np.asarray(_erf(v / math.sqrt(2.0)), np.float64))
    if act == ACT_GELU_TANH:
        with np.errstate(over="ignore"):    # (v^3 past 1e308 for |v| > 5e102: tanh(+-inf) is +-1, the right limit)
            return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v * v * v)))
    raise ValueError(f"activation {act} not restated")


def im2col_nhwc(X: np.ndarray, kh: int, kw: int, sh: int, sw: int, pad_t: int, pad_l: int, out_h: int, out_w: int) -> np.ndarray:
    """X [n][in_h][in_w][cin] -> rows [n * out_h * out_w][kh * kw * cin] in float64, k = (dy, dx, channel), taps outside the image
    zero.  The bottom / right padding is what out_h / out_w imply: (out_h - 1) sh + kh - in_h - pad_t rows, negative = a crop."""
    X = np.asarray(X, np.float64)
    n, in_h, in_w, cin = X.shape
    need_h, need_w = (out_h - 1) * sh + kh, (out_w - 1) * sw + kw
    Xp = np.zeros((n, max(need_h, pad_t + in_h), max(need_w, pad_l + in_w), cin))
    Xp[:, pad_t:pad_t + in_h, pad_l:pad_l + in_w] = X
    cols = np.empty((n, out_h, out_w, kh, kw, cin))
    for dy in range(kh):
        for dx in range(kw):
            cols[:, :, :, dy, dx] = Xp[:, dy:dy + (out_h - 1) * sh + 1:sh, dx:dx + (out_w - 1) * sw + 1:sw]
    return cols.reshape(n * out_h * out_w, kh * kw * cin)


def conv_nhwc64(X, W, bias, sh: int, sw: int, pad_t: int, pad_l: int, out_h: int, out_w: int):
    """conv(X, W) + bias in float64, X NHWC, W [kh][kw][cin][cout]: (pre [n * out_h * out_w][cout], the im2col rows)."""
    kh, kw, cin, cout = W.shape
    A = im2col_nhwc(X, kh, kw, sh, sw, pad_t, pad_l, out_h, out_w)
    return gemm64(A, np.asarray(W).reshape(kh * kw * cin, cout), bias), A


def gemm64(A, W, bias) -> np.ndarray:
    """A W + bias in float64."""
    return np.asarray(A, np.float64) @ np.asarray(W, np.float64) + np.asarray(bias, np.float64)


def gated64(A, gate, W, bias, R, P: int) -> np.ndarray:
    """The gated project GEMM of a squeeze-excite block in float64: (A x gate[row // P]) W + bias (+ R); A [n * P][K], gate [n][K]."""
    Ag = np.asarray(A, np.float64) * np.repeat(np.asarray(gate, np.float64), P, axis=0)
    out = Ag @ np.asarray(W, np.float64) + np.asarray(bias, np.float64)
    return out if R is None else out + np.asarray(R, np.float64)


def gated_bound64(A, gate, W, bias, P: int) -> np.ndarray:
    """|A x gate| |W| + |bias|: what the rounding errors of gated64's GEMM scale with."""
    Ag = np.abs(np.asarray(A, np.float64) * np.repeat(np.asarray(gate, np.float64), P, axis=0))
    return Ag @ np.abs(np.asarray(W, np.float64)) + np.abs(np.asarray(bias, np.float64))


def se_gate64(part, P: int, W1, b1, act1: int, W2, b2, act2: int):
    """The gate of a squeeze-excite block in float64: part [n][tiles][C] (per-tile channel sums), W1 [C][Cr], W2 [Cr][C] ->
    (gate [n][C], pooled [n][C] = sum over tiles / P, preH, H = act1(preH) [n][Cr], preG [n][C]); gate = act2(preG)."""
    pooled = np.asarray(part, np.float64).sum(axis=1) / float(P)
    preH = gemm64(pooled, W1, b1)
    H = act64(preH, act1)
    preG = gemm64(H, W2, b2)
    return act64(preG, act2), pooled, preH, H, preG


def direct_conv64(Xp, W, bias, sh: int, sw: int, pad_t: int, pad_l: int, out_h: int, out_w: int):
    """The NCHW stem convolution in float64: Xp planar [n][cin][h][w], W [kh][kw][cin][cout] -> (pre [n * out_h * out_w][cout] NHWC
    rows, the im2col rows), through conv_nhwc64 on the transposed input."""
    return conv_nhwc64(np.transpose(np.asarray(Xp, np.float64), (0, 2, 3, 1)), W, bias, sh, sw, pad_t, pad_l, out_h, out_w)


def head_pool64(v, P: int) -> np.ndarray:
    """The mean over each run of P rows: [n * P][N] -> [n][N] (the head convolution's global average pool)."""
    v = np.asarray(v, np.float64)
    return v.reshape(-1, P, v.shape[-1]).mean(axis=1)


# --------------------------------------------------------------------------------------------------------
# The fused MBConv block (mbconv_kernel.hpp: expand 1x1 or stem conv -> depthwise -> project 1x1 (+ residual)) in float64,
# for tests/test_mbconv_block*.py.  Weights in the loaders' layouts: We [Cin][Cexp] (stem: rows in [kh][kw][channel] order),
# Wd [KS * KS][Cexp] (tap = dy * KS + dx), Wp [Cexp][Cout].
# --------------------------------------------------------------------------------------------------------
def depthwise64(E, Wd, ks: int, st: int, pad_t: int, pad_l: int, out_h: int, out_w: int) -> np.ndarray:
    """sum over taps of E [n][H][W][C] (zero outside the image) times Wd [ks * ks][C], stride st: [n][out_h][out_w][C], no bias."""
    E = np.asarray(E, np.float64)
    Wd = np.asarray(Wd, np.float64)
    n, H, W, Cc = E.shape
    need_h, need_w = (out_h - 1) * st + ks, (out_w - 1) * st + ks
    Ep = np.zeros((n, max(need_h, pad_t + H), max(need_w, pad_l + W), Cc))
    Ep[:, pad_t:pad_t + H, pad_l:pad_l + W] = E
    out = np.zeros((n, out_h, out_w, Cc))
    for dy in range(ks):
        for dx in range(ks):
            out += Ep[:, dy:dy + (out_h - 1) * st + 1:st, dx:dx + (out_w - 1) * st + 1:st] * Wd[dy * ks + dx]
    return out


def stem_rows64(Xp, k: int, s: int, pad_t: int, pad_l: int, out_h: int, out_w: int) -> np.ndarray:
    """The stem convolution's im2col rows of a planar spectrogram [n][c][h][w]: [n][out_h][out_w][k * k * c], columns in
    (dy, dx, channel) order, taps outside the image zero."""
    X = np.transpose(np.asarray(Xp, np.float64), (0, 2, 3, 1))
    n = X.shape[0]
    return im2col_nhwc(X, k, k, s, s, pad_t, pad_l, out_h, out_w).reshape(n, out_h, out_w, -1)


def mbconv64(X, We, be, Wd, bd, Wp, bp, R, ks: int, st: int, pad_t: int, pad_l: int, out_h: int, out_w: int, act: int,
             noexp: bool = False, gate=None, stem=None):
    """One MBConv block in float64.  X is NHWC [n][H][W][Cin]; with stem = (k, s, pad_t, pad_l, H, W) it is the planar spectrogram
    [n][c][h][w] and the expand convolution is the k x k stride-s stem convolution leaving H x W pixels.  noexp: no expand
    convolution, E = X.  gate [n][Cexp] (or None) multiplies the depthwise output in front of the project convolution.
    Returns a dict: A (the expand GEMM's rows [n][H][W][K]), preE, E, preD, D (ungated), Dg (gated: what the project reads), Y,
    and Dsum [n][Cexp], the per-channel sums of D over the image (pass A of a squeeze-excite block)."""
    f = np.float64
    if stem is not None:
        k, s, spt, spl, H, W = stem
        A = stem_rows64(X, k, s, spt, spl, H, W)
    else:
        A = np.asarray(X, f)
    if noexp:
        preE = E = A
    else:
        preE = A @ np.asarray(We, f) + np.asarray(be, f)
        E = act64(preE, act)
    preD = depthwise64(E, Wd, ks, st, pad_t, pad_l, out_h, out_w) + np.asarray(bd, f)
    D = act64(preD, act)
    Dg = D if gate is None else D * np.asarray(gate, f)[:, None, None, :]
    Y = Dg @ np.asarray(Wp, f) + np.asarray(bp, f)
    if R is not None:
        Y = Y + np.asarray(R, f)
    return {"A": A, "preE": preE, "E": E, "preD": preD, "D": D, "Dg": Dg, "Y": Y, "Dsum": D.sum(axis=(1, 2))}


# --------------------------------------------------------------------------------------------------------
# The spectrogram front end (kernels_frontend.hip, api_plan.hip build_gf) in float64, from the DEFINITION
# and not from the folded operator the device builds, for tests/test_frontend*.py.
# --------------------------------------------------------------------------------------------------------
def frontend_operator64(L: int, W) -> np.ndarray:
    """G[n][m] = hann_periodic[n] sum_k cos(2 pi k n / L) W[k][m], k = 0 .. L/2: window x Re(rFFT) x mel as one dense float64
    operator (frame . G = Re(rfft(frame * hann)) . W).  Used for the magnitude sums the rounding errors scale with; the
    spectrogram itself goes through the FFT."""
    W = np.asarray(W, np.float64)
    n = np.arange(L)
    k = np.arange(W.shape[0])
    cos = np.cos(2.0 * np.pi * ((n[:, None] * k[None, :]) % L) / L)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / L))[:, None] * (cos @ W)


def frontend64(m, segs):
    """The front end of model `m` (birda_amd.modelfile.Model) on segs [n][sample_count] float32, in float64:
    x <- 2((x - min) / (max - min + eps) - 0.5) per segment (float32 samples and float32 norm_eps, float64 arithmetic); frames of
    L at hop H; periodic Hann; real part of the rFFT; . mel_W; square; ^ expo, expo = 1 / (1 + exp(mag_scale)); mel flip;
    [branch][mel][frame]; out_scale, out_shift.

    Returns (spec [n][n_branches][n_mels][n_frames], detail): detail[b] holds, for branch b and in the mel order of the FILE
    (before the flip), v [n][n_frames][n_mels] (the value the power law is applied to), B [n][n_frames][n_mels] =
    sum_j |x_j| |G[j][m]| over the frame's samples, G (frontend_operator64), expo, and xn [n][sample_count], the normalised
    samples."""
    segs = np.ascontiguousarray(segs, np.float32).reshape(-1, m.sample_count)
    x = segs.astype(np.float64)
    mn, mx = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
    xn = 2.0 * ((x - mn) / (mx - mn + float(np.float32(m.norm_eps))) - 0.5)
    n = segs.shape[0]
    spec = np.empty((n, len(m.branches), m.spec_h, m.spec_w))
    detail = []
    for b, br in enumerate(m.branches):
        L, H, nf, nm = br.frame_length, br.frame_step, br.n_frames, br.n_mels
        W = np.asarray(m.blob[br.mel_w_off:br.mel_w_off + br.n_bins * nm], np.float64).reshape(br.n_bins, nm)
        G = frontend_operator64(L, W)
        hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)
        fr = np.lib.stride_tricks.sliding_window_view(xn, L, axis=1)[:, ::H][:, :nf]          # [n][nf][L]
        v = np.fft.rfft(fr * hann, axis=2).real @ W
        B = np.abs(fr) @ np.abs(G)
        expo = 1.0 / (1.0 + math.exp(float(np.float32(br.mag_scale))))
        out = np.power(v * v, expo) * float(np.float32(br.out_scale)) + float(np.float32(br.out_shift))
        if br.flags & 1:
            out = out[:, :, ::-1]
        spec[:, b] = np.transpose(out, (0, 2, 1))
        detail.append({"v": v, "B": B, "G": G, "expo": expo, "xn": xn})
    return spec, detail
