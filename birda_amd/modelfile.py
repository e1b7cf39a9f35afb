"""BHM1 model container: the on-disk model format of the birda HIP hot path.

birda itself loads an ONNX file through `birdnet_onnx::ClassifierBuilder`
(reference `src/inference/classifier.rs:269-283`).  Neither ONNX Runtime nor the
BirdNET weights can exist on the GPU box, so the hot path reads a flat,
mmap-friendly container that states exactly what the ONNX graph would state for
this path: model I/O config (`ModelConfig{sample_rate, segment_duration,
sample_count}`, `classifier.rs:360-377`), the spectrogram front-end parameters
 and the conv stack as a layer table with BN already
folded into weights + bias.

Layout (little endian):
  header   256 B            (HEADER_FMT)
  branches n_branches x 64 B (BRANCH_FMT)   front-end STFT/mel branches
  layers   n_layers  x 128 B (LAYER_FMT)    conv stack, tensor i+1 = output of layer i
  blob     f32[]             at header.blob_offset (256-B aligned)

Tensor 0 is the front-end output [B, n_branches, n_mels, n_frames] (planar);
every other tensor is NHWC [B, out_h, out_w, cout].

The same structs are parsed by `birda_amd/csrc/model.hpp` (product) and by
`oracle/birda_oracle.c` (checker); keep the three in sync.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import List

import numpy as np

MAGIC = b"BHM1"
VERSION = 1

OP_CONV, OP_DWCONV, OP_PWCONV, OP_GAP, OP_DENSE, OP_SCALE = 1, 2, 3, 4, 5, 6   # OP_SCALE: x[n,h,w,c] * gate[n,c] (squeeze-excite), gate = res_tensor
OP_POOL = 7   # windowed MaxPool / AveragePool (floor mode); Layer.reserved is the mode; no weights, bias, activation or residual
OP_GCONV = 8  # grouped convolution (NHWC, no residual); Layer.reserved is the group count G >= 2; cin / cout are the totals, weights
              # compact [kh][kw][cin / G][cout] (output channel o reads input channels (o // (cout // G)) * (cin // G) + 0 .. cin // G - 1)
OP_CONCAT = 10  # channel Concat / Split / Slice / shuffle: a copy, NHWC f32, no weights, bias or activation.  (9 is never used: it stays the
                # "unknown layer op" tests/test_gconv.py demands.)  in_tensor = source A, w_off = first channel read from A, cin = how
                # many; res_tensor = source B (a second INPUT, not a residual) or NO_TENSOR, b_off = first channel read from B, which gives
                # cout - cin channels; Layer.reserved = shuffle groups g (0, 1: none): out[c] = cat[(c % g) * (cout // g) + c // g]
OP_LNORM = 12   # LayerNorm over the channels of an NHWC tensor, pixel by pixel (biased variance): cin == cout == C (a multiple of 4), kernel /
                # stride 1, pads 0, the image kept; w_off -> gamma[C], b_off -> beta[C]; no activation, residual or dilation; Layer.reserved
                # is the bit pattern of eps as an f32 (lnorm_eps_bits / lnorm_eps), finite and > 0.  (11 is never used, like 9.)
OP_REDUCE = 13  # ReduceMax / ReduceMean over H, over W or over both of an NHWC tensor, GlobalMaxPool, and max + mean of one window (the PANNs
                # head): spelled like OP_GAP -- cin == cout == C (a multiple of 4), kh = in_h or 1, kw = in_w or 1, stride 1, pads 0, out = in / window;
                # Layer.reserved is the mode.  The mean over both axes stays OP_GAP and a 1x1 window is refused: one spelling each.
OP_BNACT = 14   # a folded BatchNormalization + activation on a tensor no convolution can take the norm into (relu(bn(cat(..))), DenseNet; relu(bn(sum)),
                # pre-activation ResNets): y = act(fma(x, scale[c], shift[c])), f32 in every mode -- cin == cout == C (a multiple of 4), kernel / stride 1,
                # pads 0, the image kept; w_off -> scale[C], b_off -> shift[C]; no residual or dilation, Layer.reserved 0; Layer.act is one of
                # BNACT_ACTS (never ACT_NONE, never a gate activation).  A code-14 record with a window stays "unknown layer op", as does 15.
REDUCE_MAX, REDUCE_MEAN, REDUCE_MAXMEAN = 0, 1, 2  # MAXMEAN: max + mean of the same window, as one value
POOL_MAX, POOL_AVG, POOL_AVG_PAD = 0, 1, 2  # AVG: mean over the in-image taps (count_include_pad = 0); AVG_PAD: over kh * kw
# OP_CONV (NHWC), OP_PWCONV, OP_DENSE: Layer.reserved is where `act` stands relative to the residual -- 0: act(conv + b) + R (every
# file written before the flag existed); RES_ACT_AFTER: act(conv + b + R), the end of a ResNet block
RES_ACT_AFTER = 1
ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SWISH, ACT_GELU_ERF, ACT_GELU_TANH, ACT_SIGMOID, ACT_HSWISH, ACT_HSIGMOID = range(9)
BNACT_ACTS = (ACT_RELU, ACT_RELU6, ACT_SWISH, ACT_GELU_ERF, ACT_GELU_TANH, ACT_HSWISH)  # what an OP_BNACT record's `act` may be
OUT_NONE, OUT_SIGMOID, OUT_SOFTMAX = 0, 1, 2
NO_TENSOR = 0xFFFFFFFF

HEADER_SIZE, BRANCH_SIZE, LAYER_SIZE = 256, 64, 128
# magic, version, family, sample_rate, sample_count, segment_duration, n_classes,
# embedding_dim, n_branches, n_layers, output_activation, embedding_tensor,
# blob_offset, blob_floats, spec_h, spec_w, norm_eps
HEADER_FMT = "<4sIIIIfIIIIIIQQIIf"
# frame_length, frame_step, fft_length, n_bins, n_mels, n_frames, fmin, fmax,
# mag_scale, out_scale, out_shift, flags, mel_w_off
BRANCH_FMT = "<IIIIIIfffffIQ"
# op, act, in_tensor, res_tensor, cin, cout, kh, kw, sh, sw, pad_t, pad_l,
# in_h, in_w, out_h, out_w, in_layout, reserved, w_off, b_off, skip_h, skip_w
# (skip_h, skip_w at bytes 88 .. 95: the rows / columns skipped between neighbouring taps, Layer.dil_h - 1 and Layer.dil_w - 1 -- zero,
#  the tail of every record written before the words existed, is the undilated layer; the rest of the 128 bytes stays zero)
LAYER_FMT = "<IIIIIIIIIIIIIIIIIIQQII"
MAX_DILATION = 16


def lnorm_eps_bits(eps: float) -> int:
    """the `reserved` word of an OP_LNORM record: eps rounded to f32, as its bit pattern"""
    return struct.unpack("<I", struct.pack("<f", eps))[0]


def lnorm_eps(reserved: int) -> float:
    """the f32 eps an OP_LNORM record's `reserved` word holds"""
    return struct.unpack("<f", struct.pack("<I", reserved))[0]


@dataclass
class Branch:
    frame_length: int
    frame_step: int
    n_mels: int
    n_frames: int
    fmin: float
    fmax: float
    mag_scale: float
    out_scale: float = 1.0
    out_shift: float = 0.0
    flags: int = 1  # bit0: reverse the mel axis
    mel_w_off: int = 0

    @property
    def n_bins(self) -> int:
        return self.frame_length // 2 + 1


@dataclass
class Layer:
    op: int
    act: int
    in_tensor: int
    res_tensor: int
    cin: int
    cout: int
    kh: int = 1
    kw: int = 1
    sh: int = 1
    sw: int = 1
    pad_t: int = 0
    pad_l: int = 0
    in_h: int = 1
    in_w: int = 1
    out_h: int = 1
    out_w: int = 1
    in_layout: int = 0  # 0 NHWC, 1 planar NCHW (front-end output)
    w_off: int = 0
    b_off: int = 0
    # OP_POOL: the pool mode (POOL_MAX / POOL_AVG / POOL_AVG_PAD).  OP_CONV (NHWC), OP_PWCONV, OP_DENSE: the position of `act`
    # relative to the residual -- 0: act(conv + b) + R; RES_ACT_AFTER: act(conv + b + R), which needs a residual and an activation.
    # OP_GCONV: the group count.  OP_CONCAT: the channel shuffle's group count (0, 1: no shuffle).  OP_LNORM: the bits of eps as an
    # f32.  OP_REDUCE: the mode (REDUCE_MAX / REDUCE_MEAN / REDUCE_MAXMEAN).  0 for every other op.
    reserved: int = 0
    # dilation per axis (OP_CONV on an NHWC tensor and OP_DWCONV only, 1 .. MAX_DILATION, 1 on an axis with one tap): tap (dy, dx) reads
    # pixel (oy sh - pad_t + dy dil_h, ox sw - pad_l + dx dil_w).  Written as dil - 1.
    dil_h: int = 1
    dil_w: int = 1


@dataclass
class Model:
    family: int
    sample_rate: int
    sample_count: int
    segment_duration: float
    n_classes: int
    embedding_dim: int
    output_activation: int
    embedding_tensor: int
    spec_h: int
    spec_w: int
    norm_eps: float
    branches: List[Branch] = field(default_factory=list)
    layers: List[Layer] = field(default_factory=list)
    blob: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float32))

    # -- helpers -----------------------------------------------------------
    def weight(self, off: int, n: int) -> np.ndarray:
        return self.blob[off:off + n]

    def macs_per_segment(self) -> int:
        total = 0
        for L in self.layers:
            px = L.out_h * L.out_w
            if L.op == OP_CONV:
                total += px * L.kh * L.kw * L.cin * L.cout
            elif L.op == OP_DWCONV:
                total += px * L.kh * L.kw * L.cout
            elif L.op == OP_GCONV:
                total += px * L.kh * L.kw * (L.cin // L.reserved) * L.cout
            elif L.op in (OP_PWCONV, OP_DENSE):
                total += px * L.cin * L.cout
        return total


def write_model(path: str, m: Model) -> None:
    n_b, n_l = len(m.branches), len(m.layers)
    blob_offset = HEADER_SIZE + n_b * BRANCH_SIZE + n_l * LAYER_SIZE
    blob_offset = (blob_offset + 255) // 256 * 256
    blob = np.ascontiguousarray(m.blob, dtype="<f4")
    hdr = struct.pack(HEADER_FMT, MAGIC, VERSION, m.family, m.sample_rate, m.sample_count,
                      m.segment_duration, m.n_classes, m.embedding_dim, n_b, n_l,
                      m.output_activation, m.embedding_tensor, blob_offset, blob.size,
                      m.spec_h, m.spec_w, m.norm_eps)
    with open(path, "wb") as f:
        f.write(hdr.ljust(HEADER_SIZE, b"\0"))
        for b in m.branches:
            rec = struct.pack(BRANCH_FMT, b.frame_length, b.frame_step, b.frame_length, b.n_bins,
                              b.n_mels, b.n_frames, b.fmin, b.fmax, b.mag_scale, b.out_scale,
                              b.out_shift, b.flags, b.mel_w_off)
            f.write(rec.ljust(BRANCH_SIZE, b"\0"))
        for L in m.layers:
            rec = struct.pack(LAYER_FMT, L.op, L.act, L.in_tensor, L.res_tensor, L.cin, L.cout,
                              L.kh, L.kw, L.sh, L.sw, L.pad_t, L.pad_l, L.in_h, L.in_w,
                              L.out_h, L.out_w, L.in_layout, L.reserved, L.w_off, L.b_off, L.dil_h - 1, L.dil_w - 1)
            f.write(rec.ljust(LAYER_SIZE, b"\0"))
        f.write(b"\0" * (blob_offset - f.tell()))
        f.write(blob.tobytes())


def read_model(path: str) -> Model:
    with open(path, "rb") as f:
        raw = f.read()
    h = struct.unpack_from(HEADER_FMT, raw, 0)
    if h[0] != MAGIC or h[1] != VERSION:
        raise ValueError(f"{path}: not a BHM1 v{VERSION} model")
    (_, _, family, sr, sc, dur, ncls, emb, n_b, n_l, oact, etens, boff, bfl, sh, sw, eps) = h
    m = Model(family, sr, sc, dur, ncls, emb, oact, etens, sh, sw, eps)
    off = HEADER_SIZE
    for _ in range(n_b):
        r = struct.unpack_from(BRANCH_FMT, raw, off)
        m.branches.append(Branch(r[0], r[1], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12]))
        off += BRANCH_SIZE
    for _ in range(n_l):
        r = struct.unpack_from(LAYER_FMT, raw, off)
        m.layers.append(Layer(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10],
                              r[11], r[12], r[13], r[14], r[15], r[16], r[18], r[19], r[17], r[20] + 1, r[21] + 1))
        off += LAYER_SIZE
    m.blob = np.frombuffer(raw, dtype="<f4", count=bfl, offset=boff).copy()
    return m


# --------------------------------------------------------------------------------------------------------
# BHC1: custom classifier on embeddings (reference birdnet_onnx::CustomClassifier, src/lib.rs:883-901)
# header 64 B: magic, version, input_dim, n_layers, n_classes, output_activation, blob_offset, blob_floats
# layers n_layers x 32 B: in_dim, out_dim, act, reserved, w_off, b_off        (W [in][out] row-major, b [out])
# --------------------------------------------------------------------------------------------------------
CUSTOM_MAGIC = b"BHC1"
CUSTOM_HEADER_FMT = "<4sIIIIIQQ"
CUSTOM_LAYER_FMT = "<IIIIQQ"


@dataclass
class CustomLayer:
    w: np.ndarray   # [in, out]
    b: np.ndarray   # [out]
    act: int = ACT_NONE


@dataclass
class CustomClassifierModel:
    input_dim: int
    output_activation: int
    layers: List[CustomLayer] = field(default_factory=list)

    @property
    def n_classes(self) -> int:
        return int(self.layers[-1].w.shape[1])


def write_custom_classifier(path: str, m: CustomClassifierModel) -> None:
    chunks, off, recs = [], 0, []
    for L in m.layers:
        w = np.ascontiguousarray(L.w, np.float32)
        b = np.ascontiguousarray(L.b, np.float32)
        pad = (-off) % 16
        if pad:
            chunks.append(np.zeros(pad, np.float32)); off += pad
        w_off = off; chunks.append(w.ravel()); off += w.size
        pad = (-off) % 16
        if pad:
            chunks.append(np.zeros(pad, np.float32)); off += pad
        b_off = off; chunks.append(b.ravel()); off += b.size
        recs.append(struct.pack(CUSTOM_LAYER_FMT, w.shape[0], w.shape[1], L.act, 0, w_off, b_off))
    blob = np.concatenate(chunks) if chunks else np.zeros(0, np.float32)
    blob_offset = (64 + 32 * len(recs) + 255) // 256 * 256
    hdr = struct.pack(CUSTOM_HEADER_FMT, CUSTOM_MAGIC, 1, m.input_dim, len(recs), m.n_classes, m.output_activation,
                      blob_offset, blob.size)
    with open(path, "wb") as f:
        f.write(hdr.ljust(64, b"\0"))
        for r in recs:
            f.write(r)
        f.write(b"\0" * (blob_offset - 64 - 32 * len(recs)))
        f.write(blob.astype("<f4").tobytes())
