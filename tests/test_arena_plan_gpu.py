"""The activation arena's plan against what the forward pass actually reads and writes.

plan_arena (birda_amd/csrc/api_plan.hip) gives every tensor bytes of one arena by liveness: a tensor is born at its layer's step
and its bytes go to the next tensor once its last reader has run.  Several paths of the forward do not follow that picture -- a
launch that stands for several layers writes tensors earlier, or reads them later, than their layers would.  The library states
what the forward launches once, as a schedule built at create (build_schedule: per step its path, its layers, and the tensors it
reads, writes and borrows); forward_slice (birda_amd/csrc/api.hip) walks that schedule and plan_arena derives every lifetime and
size from it.  A step that names too few tensors is silent: the bytes are shared, a late workgroup reads what an early one wrote
over its input, and the logits come out wrong and finite.  Whether that shows on the GPU depends on how many workgroups are
resident at once, so this file does not run a forward at all: it asks the library for its plan (bh_audit_arena_plan: offsets,
planned sizes, and the path the forward takes at every layer) and replays the launches of the forward, restated here from reading
the launch code -- on purpose NOT read from the library's schedule: this is the independent witness -- over the planned bytes:

  * no launch writes bytes that the same launch reads or writes as another tensor;
  * every read finds its tensor's bytes untouched since the launch that wrote that tensor;
  * every write of a layer's output, and every read of a tensor last written as one, finds that tensor planned at its whole size.

tests/golden/arena_plans.json holds every audited plan as recorded at the commit it names (totals and digests; FAMILY_MODELS' under
a commit of their own); a change that is not meant to move a tensor leaves them equal, one that is records them again with
tools/record_arena_plans.py (test_arena_plan_is_the_recorded_one).

The restatement per path (tensor t = output of layer t-1, tensor 0 = the spectrogram):
  plain layer        reads its input, and its res_tensor where the op's launch takes a second tensor (SliceRun::layer, layer_reads()
                     below: the residual of a full NHWC convolution, a 1x1 convolution and a dense layer; the gate of OP_SCALE; source B
                     of OP_CONCAT), writes its output.  The other ops' launches take one tensor, so a record of theirs that names a
                     second one is refused here, as is an op code without an entry;
  fused block        one launch: reads the block input (+ the project's residual), writes the project's output;
  fused SE block     pass A reads the block input, writes the depthwise output D (not for a block without an expand conv, which
                     computes D again later) and the per-tile channel sums (the OP_SCALE output's slot); the gate launch reads the
                     sums and writes the gate (the second 1x1's slot) and, beyond 576 channels, scratch in the slots of the pool
                     and the first 1x1; the gated project GEMM reads D (or the block input again), the gate and the residual;
  head conv + pool   one launch: reads the conv's input, writes the pooled tensor;
  gate fast path     se_hidden_kernel reads the pool's input and writes partial sums into the pool's slot (i+1), then
                     se_gate16_kernel reads those and writes the gate (i+3);
  concat chain       one launch (SliceRun::concat) gathers the leaves -- source A of the first record, then source B of every record of
                     the chain -- straight into the last record's tensor; the records in between write nothing (their tensors get no
                     bytes).  The chain is the run of inner tags behind its first record, every record of it an OP_CONCAT that reads
                     its predecessor whole and brings a source B of its own (concat_chain_len); at most four leaves;
and the embedding tensor is read back after the forward.  The last layer's output goes to the caller's logits buffer.

Two catalogues are audited.  MODEL_NAMES: the inverted-residual stacks (tests/test_launch_scale_gpu.py runs forwards of some of them).
FAMILY_MODELS: every other graph shape the library runs -- pools, ResNet blocks with the activation after the add, grouped
convolutions, Concat / Split / shuffle with the one-launch chain, hard-swish blocks, dilated layers, ConvNeXt, reduce heads, DenseNet
and pre-activation ResNets, Fused-MBConv stages -- on the mini front end, and long_reach_model, a hand-written graph of long
lifetimes.  test_the_audited_models_reach_every_path_and_every_op holds the union to every path tag and every op code.
tests/test_arena_audit.py tests schedule() and audit() themselves, without a device, on plans with seeded faults.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# include/birda_hip_audit.h
PATH_LAYER, PATH_FUSED, PATH_FUSED_SE, PATH_HEAD_GAP, PATH_SE_GATE, PATH_INNER, PATH_CONCAT = range(7)
PATH_NAMES = {PATH_LAYER: "layer", PATH_FUSED: "fused block", PATH_FUSED_SE: "fused SE block", PATH_HEAD_GAP: "head conv + pool",
              PATH_SE_GATE: "gate fast path", PATH_INNER: "inner", PATH_CONCAT: "concat chain"}

# The mini front-end (12 000 samples, 32 mels, one branch) down to 2 x 8 = 16 pixels, then a 640-channel stage with squeeze-excite
# gates: its blocks run layer by layer, and both gates -- 112 -> 672 (Cr 28) and 640 -> 3 840 (Cr 160, the v3.0-sized block) --
# take the gate fast path (pool -> 1x1 -> 1x1 as se_hidden_kernel + se_gate16_kernel).
WIDE_GATE_PLAN = dict(sr=48000, n=12000, branches=[(512, 100, 32, 0.0, 3000.0)], stem=16, act=3, se=True, head=128, classes=50,
                      stages=[(1, 3, 1, 16, 1), (6, 3, 2, 24, 1), (6, 3, 2, 40, 1), (6, 3, 2, 112, 1), (6, 3, 1, 640, 2)])
# The same front-end down to 4 x 15 = 60 pixels and a 112 -> 672 squeeze-excite block that the planner fuses in every precision:
# its gate is se_gate16 on the fused path (more than 576 expanded channels).
FUSED_WIDE_SE_PLAN = dict(WIDE_GATE_PLAN, stages=[(1, 3, 1, 16, 1), (6, 3, 2, 24, 1), (6, 3, 2, 40, 1), (6, 3, 1, 112, 1), (6, 3, 1, 112, 1)])
RANDOM_SEEDS = range(12)
MODEL_NAMES = ["mini", "mini_b0", "mini_hg", "mini_se", "wide_gate", "fused_wide_se", "tail_gate"] + [f"random{s}" for s in RANDOM_SEEDS]
# The mini front end of one branch under two Fused-MBConv stages (a sixth stage element: a 3x3 full convolution as the expand, or as
# the whole block at expand ratio 1, with the residual on a full NHWC convolution) and two gated MBConv stages.
FUSED_MBCONV_PLAN = dict(WIDE_GATE_PLAN, head=64, stages=[(1, 3, 1, 16, 1, True), (4, 3, 2, 24, 2, True), (4, 3, 2, 40, 2), (6, 3, 2, 80, 1)])
# name -> (synth kind, the plan's generator, its seed): the families behind the inverted-residual stacks, all on the mini front end
FAMILY_PLANS = {**{f"dense_plan{s}": ("dense_plan", "random_dense_plan", s) for s in (0, 1, 2)},
                **{f"branchy_plan{s}": ("branchy_plan", "random_branchy_plan", s) for s in (0, 1, 2, 3)},
                **{f"resnet_plan{s}": ("resnet_plan", "random_resnet_plan", s) for s in (0, 1)},
                **{f"resnext_plan{s}": ("resnext_plan", "random_resnext_plan", s) for s in (0, 1)},     # seed 1: OP_GAP / OP_SCALE gates
                **{f"pool_plan{s}": ("pool_plan", "random_pool_plan", s) for s in (0, 2)},
                **{f"reduce_plan{s}": ("reduce_plan", "random_reduce_plan", s) for s in (0, 1)},
                **{f"mnv3_plan{s}": ("mnv3_plan", "random_mnv3_plan", s) for s in (0, 1)},              # seed 1: hard-sigmoid gates
                "convnext_plan": ("convnext_plan", "convnext_plan", 1)}
FAMILY_MODELS = sorted(FAMILY_PLANS) + ["dilated_plan", "fused_mbconv", "six_way", "long_reach"]
RECORDED_PLANS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arena_plans.json")
BATCHES = (0, 1, 16, 300, 4096)    # 0: the context's own plan (max_batch 16); the others: the plan an n-segment lane gets


def build_models(d):
    """name -> (.bhm path, model): every model this file and tests/test_launch_scale_gpu.py audit."""
    from birda_amd import modelfile as mf, synth
    models = {k: synth.build_model(k) for k in ("mini", "mini_b0", "mini_hg", "mini_se")}
    models["wide_gate"] = synth.build_model("custom", plan=WIDE_GATE_PLAN)
    models["fused_wide_se"] = synth.build_model("custom", plan=FUSED_WIDE_SE_PLAN)
    models["tail_gate"] = tail_gate_model()
    for seed in RANDOM_SEEDS:
        p = synth.random_plan(seed)
        p["se"] = True
        models[f"random{seed}"] = synth.build_model("custom", plan=p)
    out = {}
    for k, m in models.items():
        path = os.path.join(str(d), f"{k}.bhm")
        mf.write_model(path, m)
        out[k] = (path, m)
    return out


def tail_gate_model():
    """A model that ENDS in a gate chain (the last three layers: pool of a 2 x 8 = 16-pixel, 640-channel tensor -> 1x1 640 -> 160,
    swish -> 1x1 160 -> 640, sigmoid; 640 classes): the wide-gate plan cut after its last block, the head replaced by the chain.  The
    gate fast path takes it, and its output is the logits."""
    from birda_amd import modelfile as mf, synth
    m = synth.build_model("custom", plan=WIDE_GATE_PLAN)
    b = synth._Builder(np.random.default_rng(0x7A11))
    b.chunks, b.off, b.layers = [m.blob], int(m.blob.size), list(m.layers[:-3])     # (without head conv, pool, dense)
    last = b.layers[-1]
    t, h, w, c = len(b.layers), last.out_h, last.out_w, last.cout
    assert (h * w, c) == (16, 640)
    g = b.gap(t, h, w, c)
    g = b.pwconv(g, 1, 1, c, 160, mf.ACT_SWISH)
    b.pwconv(g, 1, 1, 160, c, mf.ACT_SIGMOID)
    return mf.Model(m.family, m.sample_rate, m.sample_count, m.segment_duration, c, h * w * c, mf.OUT_NONE, t, m.spec_h, m.spec_w,
                    m.norm_eps, m.branches, b.layers, np.concatenate(b.chunks))


def family_models():
    """name -> model, for FAMILY_MODELS (no file, no device)."""
    from birda_amd import synth
    from test_concat_gpu import six_way_model
    models = {k: synth.build_model(kind, plan=getattr(synth, gen)(seed)) for k, (kind, gen, seed) in FAMILY_PLANS.items()}
    models["dilated_plan"] = synth.build_model("dilated_plan")
    models["fused_mbconv"] = synth.build_model("custom", plan=FUSED_MBCONV_PLAN)
    models["six_way"] = six_way_model()            # a 6-way Concat: more than four leaves, so the chain splits into two steps
    models["long_reach"] = long_reach_model()
    assert sorted(models) == sorted(FAMILY_MODELS)
    return models


def build_family_models(d):
    """name -> (.bhm path, model) for FAMILY_MODELS, as build_models does for MODEL_NAMES."""
    from birda_amd import modelfile as mf
    out = {}
    for k, m in family_models().items():
        path = os.path.join(str(d), f"{k}.bhm")
        mf.write_model(path, m)
        out[k] = (path, m)
    return out


def long_reach_model():
    """Long lifetimes in one graph, nothing random but the weights.  The mini front end of one 32-mel branch, a 3x3 stride-2 stem to
    16 channels (T1, 16 x 58 pixels), then, layer k writing tensor T(k):
       2 1x1 T1 -> 24     3 depthwise 3x3 of T2     4 1x1 T2 -> 8     5 1x1 T3 -> 24 + T2 (T2: three readers, the last a residual)
       6 / 7 / 8 1x1 T5 -> 8 / 12 / 4       9..11 Concat(T4, T6, T7, T8) -> 32: three records, one launch; T6 is read again by
      12 1x1 T11 -> 16   13 1x1 T6 -> 16 + T12
      14 Concat(T13, channels 4..15 of T1) -> 28: T1 is read 13 layers after the stem wrote it, and once more by
      15 the window 8..15 of T1 (a one-source record, the Split spelling)
      16 1x1 T14 -> 24   17 1x1 T15 -> 24 + T16
      18 pool T17   19 1x1 -> 8   20 1x1 -> 24, sigmoid: a gate that waits while   21 1x1 T17 -> 24   runs, then   22 T21 x gate T20
      23 pool T22 -> 24 values   24 1x1 T23 -> 8   25 the window 8..15 of T23
      26 Concat(T25, T24) -> 16: with 25 a chain of two leaves, and T26 is the embedding tensor: its only layer reader is
      27 Concat(T26, channels 0..7 of T23) -> 24, which reads it whole as a chain's next record would -- the chain must end at 26,
         and T26 must keep its bytes to the read-back although no layer behind 27 reads it
      28 1x1 T27 -> 16   29 dense -> 12 classes."""
    from birda_amd import modelfile as mf, synth
    b = synth._Builder(np.random.default_rng(0x10A6))
    sr, n, act = 48000, 12000, mf.ACT_RELU6
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t1, h, w = b.conv(0, br.n_mels, br.n_frames, 1, 16, 3, 2, act, in_layout=1)
    t2 = b.pwconv(t1, h, w, 16, 24, act)
    t3, _, _ = b.dwconv(t2, h, w, 24, 3, 1, act)
    t4 = b.pwconv(t2, h, w, 24, 8, act)
    t5 = b.pwconv(t3, h, w, 24, 24, mf.ACT_NONE, res=t2, gain=0.5)
    t6, t7, t8 = (b.pwconv(t5, h, w, 24, c, act) for c in (8, 12, 4))
    t11, c = b.concat([(t4, 0, 8), (t6, 0, 8), (t7, 0, 12), (t8, 0, 4)], h, w)
    t12 = b.pwconv(t11, h, w, c, 16, act)
    t13 = b.pwconv(t6, h, w, 8, 16, mf.ACT_NONE, res=t12, gain=0.5)
    t14, c = b.concat([(t13, 0, 16), (t1, 4, 12)], h, w)
    t15 = b.slice(t1, h, w, 8, 8)
    t16 = b.pwconv(t14, h, w, c, 24, act)
    t17 = b.pwconv(t15, h, w, 8, 24, mf.ACT_NONE, res=t16, gain=0.5)
    t18 = b.gap(t17, h, w, 24)
    t19 = b.pwconv(t18, 1, 1, 24, 8, mf.ACT_SWISH)
    t20 = b.pwconv(t19, 1, 1, 8, 24, mf.ACT_SIGMOID)
    t21 = b.pwconv(t17, h, w, 24, 24, act)
    t22 = b.scale(t21, t20, h, w, 24)
    t23 = b.gap(t22, h, w, 24)
    t24 = b.pwconv(t23, 1, 1, 24, 8, act)
    t25 = b.slice(t23, 1, 1, 8, 8)
    t26, c = b.concat([(t25, 0, 8), (t24, 0, 8)], 1, 1)
    t27, c = b.concat([(t26, 0, 16), (t23, 0, 8)], 1, 1)
    t28 = b.pwconv(t27, 1, 1, c, 16, act)
    t29 = b.dense(t28, 16, 12, gain=1.5)
    assert (t1, t11, t14, t15, t20, t22, t26, t27, t29) == (1, 11, 14, 15, 20, 22, 26, 27, 29)
    return mf.Model(0, sr, n, n / sr, 12, 16, mf.OUT_SIGMOID, t26, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))


def arena_plan(clf, ctx, n):
    """(offsets, planned sizes) per tensor in floats, and the path tag per layer, of `ctx`'s plan (n == 0) or an n-segment lane's."""
    from birda_amd import _lib
    cap = 4096
    off = (C.c_uint64 * cap)()
    sz = (C.c_uint64 * cap)()
    path = (C.c_uint8 * cap)()
    nt = _lib.load().bh_audit_arena_plan(clf._h, ctx._h, n, off, sz, path, cap)
    _lib.check(0 if nt > 0 else nt)
    return np.array(off[:nt], np.uint64), np.array(sz[:nt], np.uint64), list(path[:nt - 1])


def tensor_floats(m, t):
    if t == 0:
        return len(m.branches) * m.spec_h * m.spec_w
    L = m.layers[t - 1]
    return L.out_h * L.out_w * L.cout


def layer_reads():
    """op code -> what the launch of a layer that runs alone reads besides in_tensor (SliceRun::layer): the name of what res_tensor
    is to that launch, or None where the launcher takes one tensor only."""
    from birda_amd import modelfile as mf
    return {mf.OP_CONV: "residual",        # (launch_conv_gemm / launch_conv_gemm16; the planar stem's direct kernel takes none: below)
            mf.OP_DWCONV: None, mf.OP_PWCONV: "residual", mf.OP_GAP: None, mf.OP_DENSE: "residual",
            mf.OP_SCALE: "gate",           # the [n][C] gate the feature map is multiplied by
            mf.OP_POOL: None, mf.OP_GCONV: None,
            mf.OP_CONCAT: "source B",      # a second input, not a residual (concat_sources)
            mf.OP_LNORM: None, mf.OP_REDUCE: None, mf.OP_BNACT: None}


def schedule(m, path):
    """forward_slice's launches in stream order: (name, tensors read, tensors written, tensors written as a layer's output).
    None stands for the caller's logits buffer."""
    from birda_amd import modelfile as mf
    nl = len(m.layers)
    out = lambda t: None if t == nl else t
    res = lambda L: [] if L.res_tensor == mf.NO_TENSOR else [L.res_tensor]
    second = layer_reads()
    launches = [("front end", [], [0], [0])]
    i = 0
    while i < nl:
        L, tag = m.layers[i], path[i]
        assert tag != PATH_INNER, f"layer {i} starts a launch but is tagged as inside an earlier one"
        if tag == PATH_LAYER:
            assert L.op in second, f"layer {i}: op code {L.op} has no entry in the witness's table of launches"
            takes = None if (L.op == mf.OP_CONV and L.in_layout == 1) else second[L.op]
            assert takes is not None or L.res_tensor == mf.NO_TENSOR, f"layer {i}: op {L.op} names T({L.res_tensor}), which its launch never reads"
            assert L.op != mf.OP_SCALE or L.res_tensor != mf.NO_TENSOR, f"layer {i}: a scale layer without a gate"
            launches.append((f"layer {i}", [L.in_tensor] + res(L), [out(i + 1)], [out(i + 1)]))
            i += 1
        elif tag == PATH_CONCAT:
            assert L.op == mf.OP_CONCAT, f"layer {i}: tagged as the start of a concat chain but its op code is {L.op}"
            k = i + 1
            while k < nl and path[k] == PATH_INNER:
                k += 1
            assert k - i >= 2, f"layer {i}: a concat chain of one record"
            for j in range(i + 1, k):      # every record behind the first reads its predecessor whole and brings a source B
                R, P = m.layers[j], m.layers[j - 1]
                assert R.op == mf.OP_CONCAT and R.in_tensor == j and R.w_off == 0 and R.cin == P.cout, (i, j, R.op, R.in_tensor)
                assert R.res_tensor != mf.NO_TENSOR and P.reserved <= 1, (i, j)
            leaves = [L.in_tensor] + [t for j in range(i, k) for t in res(m.layers[j])]
            assert len(leaves) <= 4, f"concat chain {i}..{k - 1}: {len(leaves)} leaves in one launch"
            assert not set(leaves) & set(range(i + 1, k)), f"concat chain {i}..{k - 1}: a leaf is a tensor the chain never writes"
            launches.append((f"concat chain {i}..{k - 1} ({len(leaves)} leaves)", leaves, [out(k)], [out(k)]))
            i = k
        elif tag == PATH_FUSED:
            ip = i + 1 if L.op == mf.OP_DWCONV else i + 2
            assert m.layers[ip].op == mf.OP_PWCONV and all(m.layers[k].in_tensor == k for k in range(i + 1, ip + 1)), i
            assert all(p == PATH_INNER for p in path[i + 1:ip + 1]), (i, path[i:ip + 1])
            launches.append((f"fused block {i}..{ip}", [L.in_tensor] + res(m.layers[ip]), [out(ip + 1)], [out(ip + 1)]))
            i = ip + 1
        elif tag == PATH_FUSED_SE:
            iD = i if L.op == mf.OP_DWCONV else i + 1
            iGap, iPw1, iPw2, iScale, iP = iD + 1, iD + 2, iD + 3, iD + 4, iD + 5
            ops = [m.layers[k].op for k in (iD, iGap, iPw1, iPw2, iScale, iP)]
            assert ops == [mf.OP_DWCONV, mf.OP_GAP, mf.OP_PWCONV, mf.OP_PWCONV, mf.OP_SCALE, mf.OP_PWCONV], (i, ops)
            assert m.layers[iScale].in_tensor == iD + 1 and m.layers[iScale].res_tensor == iPw2 + 1 and m.layers[iP].in_tensor == iScale + 1
            assert all(p == PATH_INNER for p in path[i + 1:iP + 1]), (i, path[i:iP + 1])
            noexp = iD == i
            C_ = m.layers[iD].cout
            launches.append((f"SE block {i}..{iP}: pass A", [L.in_tensor], ([] if noexp else [iD + 1]) + [iScale + 1], []))
            scratch = [iGap + 1, iPw1 + 1] if C_ > 576 else []
            launches.append((f"SE block {i}..{iP}: gate", [iScale + 1], scratch + [iPw2 + 1], []))
            launches.append((f"SE block {i}..{iP}: gated project", ([L.in_tensor] if noexp else [iD + 1]) + [iPw2 + 1] + res(m.layers[iP]),
                             [out(iP + 1)], [out(iP + 1)]))
            i = iP + 1
        elif tag == PATH_HEAD_GAP:
            G = m.layers[i + 1]
            assert L.op == mf.OP_PWCONV and G.op == mf.OP_GAP and G.in_tensor == i + 1 and path[i + 1] == PATH_INNER, i
            launches.append((f"head conv + pool {i}..{i + 1}", [L.in_tensor], [out(i + 2)], [out(i + 2)]))
            i += 2
        elif tag == PATH_SE_GATE:
            G1, G2 = m.layers[i + 1], m.layers[i + 2]
            assert L.op == mf.OP_GAP and G1.op == mf.OP_PWCONV and G2.op == mf.OP_PWCONV and G1.in_tensor == i + 1 and G2.in_tensor == i + 2, i
            assert path[i + 1] == PATH_INNER and path[i + 2] == PATH_INNER, i
            launches.append((f"gate {i}..{i + 2}: se_hidden_kernel", [L.in_tensor], [i + 1], []))
            launches.append((f"gate {i}..{i + 2}: se_gate16_kernel", [i + 1], [out(i + 3)], [out(i + 3)]))
            i += 3
        else:
            raise AssertionError(f"layer {i}: unknown path tag {tag}")
    if m.embedding_tensor != nl:
        launches.append(("embedding read-back", [m.embedding_tensor], [], []))
    return launches


def audit(m, off, sz, path, n):
    """The problems of one plan, as strings (empty: the plan is sound for these launches)."""
    rng = lambda t: (int(off[t]), int(off[t]) + int(sz[t]))
    overlap = lambda a, b: rng(a)[0] < rng(b)[1] and rng(b)[0] < rng(a)[1]
    problems = []
    written_at, writes, as_output = {}, [], {}
    for k, (name, reads, wr, outputs) in enumerate(schedule(m, path)):
        wr = [t for t in wr if t is not None]
        for t in reads:       # (a slot last written as scratch -- the SE paths' sums and partial sums -- keeps its own size)
            if as_output.get(t) and sz[t] < tensor_floats(m, t) * n:
                problems.append(f"{name}: reads T({t}), a layer's output of {tensor_floats(m, t) * n} floats, the plan gives {sz[t]}")
        for t in set(reads) | set(wr):
            if sz[t] == 0:
                problems.append(f"{name}: touches T({t}), which the plan gives no bytes")
        for t in outputs:
            if t is not None and sz[t] < tensor_floats(m, t) * n:
                problems.append(f"{name}: T({t}) needs {tensor_floats(m, t) * n} floats, the plan gives {sz[t]}")
        for t in reads:
            if t not in written_at:
                problems.append(f"{name}: reads T({t}) before any launch wrote it")
                continue
            for (k2, u) in writes:
                if k2 > written_at[t] and u != t and overlap(t, u):
                    problems.append(f"{name}: reads T({t}) at {rng(t)}, overwritten since by T({u}) at {rng(u)} ({schedule_name(m, path, k2)})")
        touched = set(reads) | set(wr)
        for t in wr:
            for u in touched - {t}:
                if overlap(t, u):
                    problems.append(f"{name}: writes T({t}) at {rng(t)} over T({u}) at {rng(u)}, which the same launch "
                                    f"{'reads' if u in reads else 'writes'}")
        for t in wr:
            written_at[t] = k
            writes.append((k, t))
            as_output[t] = t in outputs
    return problems


def schedule_name(m, path, k):
    return schedule(m, path)[k][0]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return {**build_models(tmp_path_factory.mktemp("arena_models")), **build_family_models(tmp_path_factory.mktemp("arena_families"))}


@pytest.fixture(scope="module")
def perch(tmp_path_factory):
    from birda_amd import modelfile as mf, synth
    m = synth.build_model("perch_v2")
    path = str(tmp_path_factory.mktemp("arena_perch") / "perch_v2.bhm")
    mf.write_model(path, m)
    return path, m


_TAGS = {}      # (model file, precision) -> path tags, kept by _audit_model for the coverage test below


def _audit_model(path, m, precision):
    from birda_amd.classifier import BirdClassifier
    clf = BirdClassifier(path, None, precision=precision)
    ctx = clf.create_batch_context(16)
    tags = None
    try:
        failures = []
        for n in BATCHES:
            off, sz, tags = arena_plan(clf, ctx, n)
            assert len(off) == len(m.layers) + 1
            for p in audit(m, off, sz, tags, n or 16):
                failures.append(f"[{precision}, n={n or '16 (context)'}] {p}")
        _TAGS[(os.path.basename(path), precision)] = tags
        return tags, failures
    finally:
        ctx.close()
        clf.close()


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("name", MODEL_NAMES + FAMILY_MODELS)
def test_arena_plan_keeps_every_launchs_tensors_apart(models, name, precision):
    path, m = models[name]
    tags, failures = _audit_model(path, m, precision)
    used = sorted({PATH_NAMES[t] for t in tags if t != PATH_INNER})
    print(f"{name} [{precision}]: {len(m.layers)} layers, paths {used}, {len(failures)} problem(s)")
    assert not failures, "\n".join(failures[:20])
    if name == "wide_gate":     # the chains this plan exists for: both gates of the 640-channel stage on the fast path
        gated = [m.layers[i].cout for i, t in enumerate(tags) if t == PATH_SE_GATE]
        assert 3840 in gated and 672 in gated, (precision, gated)
    if name == "tail_gate":
        assert tags[len(m.layers) - 3] == PATH_SE_GATE, (precision, tags[-3:])


def test_the_audited_models_reach_every_path_and_every_op(models):
    """Conditions on the catalogue, not measurements: over MODEL_NAMES + FAMILY_MODELS in both precisions every path tag of
    include/birda_hip_audit.h occurs, every op code modelfile defines starts a step that runs the layer alone, concat-chain steps of
    two, three and four leaves occur, and a chain is followed directly by a further concat step that reads its output (the split of
    a chain of more than four leaves, and the record behind long_reach_model's embedding tensor).  The seeds are the issue's own: none
    had to change (the chain of two leaves is long_reach_model's, the split six_way's and long_reach_model's)."""
    from birda_amd import modelfile as mf
    from birda_amd.classifier import BirdClassifier
    ops = {v for k, v in vars(mf).items() if k.startswith("OP_")}
    assert ops == set(layer_reads()), "the witness's table of launches and modelfile's op codes differ"
    tags_seen, alone, leaves_seen, split = set(), set(), set(), []
    for name in MODEL_NAMES + FAMILY_MODELS:
        path, m = models[name]
        for precision in ("f32", "f16x3"):
            tags = _TAGS.get((os.path.basename(path), precision))
            if tags is None:
                clf = BirdClassifier(path, None, precision=precision)
                ctx = clf.create_batch_context(16)
                try:
                    _, _, tags = arena_plan(clf, ctx, 0)
                finally:
                    ctx.close()
                    clf.close()
            tags_seen |= set(tags)
            alone |= {m.layers[i].op for i, t in enumerate(tags) if t == PATH_LAYER}
            for i, t in enumerate(tags):
                if t != PATH_CONCAT:
                    continue
                k = i + 1
                while k < len(tags) and tags[k] == PATH_INNER:
                    k += 1
                leaves_seen.add((1 if m.layers[i].res_tensor == mf.NO_TENSOR else 2) + k - i - 1)
                if k < len(tags) and m.layers[k].op == mf.OP_CONCAT and m.layers[k].in_tensor == k and tags[k] in (PATH_CONCAT, PATH_LAYER):
                    split.append((name, precision, i, k, PATH_NAMES[tags[k]]))
    print(f"path tags {sorted(tags_seen)}, ops that run alone {sorted(alone)}, leaves of the concat chains {sorted(leaves_seen)}, "
          f"chains with a concat step behind them {sorted(set(s[0] for s in split))}")
    assert tags_seen == set(range(7)), sorted(tags_seen)
    assert alone == ops, sorted(ops - alone)
    assert leaves_seen == {2, 3, 4}, sorted(leaves_seen)
    assert split


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_arena_plan_of_the_perch_sized_model(perch, precision):
    path, m = perch
    tags, failures = _audit_model(path, m, precision)
    assert PATH_FUSED_SE in tags, (precision, sorted(set(tags)))
    assert not failures, "\n".join(failures[:20])


def plan_digest(off, sz, tags):
    """What tests/golden/arena_plans.json records of one plan: the arena's floats, and a SHA-256 over the offsets and the planned
    sizes (little-endian uint64) and the path tags (uint8)."""
    h = hashlib.sha256(off.astype("<u8").tobytes() + sz.astype("<u8").tobytes() + np.array(tags, np.uint8).tobytes())
    return {"total": int((off + sz).max()), "sha256": h.hexdigest()}


@pytest.fixture(scope="module")
def recorded_plans():
    with open(RECORDED_PLANS) as f:
        return json.load(f)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("name", MODEL_NAMES + ["perch_v2"] + FAMILY_MODELS)
def test_arena_plan_is_the_recorded_one(models, perch, recorded_plans, name, precision):
    """Every tensor's offset and planned size and every layer's path tag, for every n of BATCHES, are what the library planned at
    the commit the golden file names: equality, no forward.  (A change that means to move a tensor records the file again.)"""
    from birda_amd.classifier import BirdClassifier
    path, _ = perch if name == "perch_v2" else models[name]
    clf = BirdClassifier(path, None, precision=precision)
    ctx = clf.create_batch_context(16)
    try:
        got = {n: plan_digest(*arena_plan(clf, ctx, n)) for n in BATCHES}
    finally:
        ctx.close()
        clf.close()
    want = {n: recorded_plans["plans"][f"{name}/{precision}/{n}"] for n in BATCHES}
    at = recorded_plans["families_recorded_at" if name in FAMILY_MODELS else "recorded_at"]
    assert got == want, (f"recorded at {at}", got, want)
