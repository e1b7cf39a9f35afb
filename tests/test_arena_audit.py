"""The witness of tests/test_arena_plan_gpu.py, tested itself -- without a device.

schedule() restates the forward's launches and audit() replays them over a plan; a green audit on the device means something only if
those two report a plan that is NOT sound.  Here the plans are made in Python, never by the library:

* a sound plan -- every tensor its own bytes at tensor_floats * n rounded up to 64 floats, the inner tensors of a concat chain no
  bytes -- gives no problem for every model of FAMILY_MODELS, with every layer tagged as running alone and, for six_way and long_reach,
  with their concat chains tagged as the one-launch steps the library makes of them (written down by hand below);
* one fault at a time is seeded into such a plan of long_reach_model and of one generated plan where that plan has the shape for it,
  and the report must name the launch and the tensors: (a) a concat's output over its source B, (b) a chain's output over a leaf
  that is not its first source, (c) a mid-graph tensor over T1 between T1's write and its late reads, (d) a tensor over the embedding
  tensor after its last layer reader, (e) an output one 64-float unit short, (f) a tensor that is read given no bytes, (g) a gate
  overwritten before its scale launch (long_reach_model alone keeps a gate waiting across another launch; in the generated gates the
  scale follows the gate directly, so there the gate is planned over the feature map the same scale launch reads);
* a tag list with a concat chain on a record that is no OP_CONCAT, a chain of five leaves, an unknown tag and an unknown op code raise;
* long_reach_model is a valid model: the library's host-only loader accepts its file, it holds the lifetimes its docstring states, and
  its float64 forward (tests/test_concat.py) is finite with every concat tensor the torch.cat / narrow of its sources.
"""
import copy

import numpy as np
import pytest

from birda_amd import modelfile as mf
from test_arena_plan_gpu import (FAMILY_MODELS, PATH_CONCAT, PATH_INNER, PATH_LAYER, audit, family_models, long_reach_model, schedule,
                                 tensor_floats)

N = 16
NONE = mf.NO_TENSOR


@pytest.fixture(scope="module")
def families():
    return family_models()


def chain_tags(m, chains):
    """every layer alone, but the records first .. last (0-based layers) of each chain as one concat step"""
    tags = [PATH_LAYER] * len(m.layers)
    for first, last in chains:
        tags[first:last + 1] = [PATH_CONCAT] + [PATH_INNER] * (last - first)
    return tags


# the steps the library makes of the two hand-written models' chains: six_way's five records (layers 7 .. 11) split after four leaves;
# long_reach's 4-way Concat (layers 8 .. 10) and the window + Concat in front of its embedding tensor (layers 24, 25)
CHAINS = {"six_way": [(7, 9), (10, 11)], "long_reach": [(8, 10), (24, 25)]}


def sound_plan(m, tags, n=N):
    """(off, sz): every tensor its own bytes, a chain's inner tensors none"""
    sz = np.array([-(-tensor_floats(m, t) * n // 64) * 64 for t in range(len(m.layers) + 1)], np.uint64)
    for i, t in enumerate(tags):
        if t == PATH_INNER:
            sz[i] = 0           # tensor i = the output of layer i - 1, the record in front of an inner one
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
    return off, sz


def tag_lists(name, m):
    return [[PATH_LAYER] * len(m.layers)] + ([chain_tags(m, CHAINS[name])] if name in CHAINS else [])


@pytest.mark.parametrize("name", FAMILY_MODELS)
def test_a_sound_plan_has_no_problem(families, name):
    m = families[name]
    for tags in tag_lists(name, m):
        off, sz = sound_plan(m, tags)
        assert audit(m, off, sz, tags, N) == []
    if name in CHAINS:
        chains = [(nm, r) for nm, r, _, _ in schedule(m, chain_tags(m, CHAINS[name])) if nm.startswith("concat chain")]
        assert [len(r) for _, r in chains] == ([4, 3] if name == "six_way" else [4, 2]), chains


def _place(off, t, over):
    off = off.copy()
    off[t] = off[over]
    return off


def _reported(problems, *words):
    hits = [p for p in problems if all(w in p for w in words)]
    assert hits, (words, problems[:6])
    return hits


def _two_source_concat(m, tags):
    return next(i for i, L in enumerate(m.layers) if L.op == mf.OP_CONCAT and L.res_tensor != NONE and tags[i] == PATH_LAYER
                and (i + 1 == len(tags) or tags[i + 1] != PATH_INNER))


def _gate(m):
    return next(i for i, L in enumerate(m.layers) if L.op == mf.OP_SCALE)


@pytest.mark.parametrize("chained", [False, True])
def test_every_seeded_fault_in_long_reach_is_reported_by_name(chained):
    m = long_reach_model()
    tags = chain_tags(m, CHAINS["long_reach"]) if chained else [PATH_LAYER] * len(m.layers)
    off, sz = sound_plan(m, tags)
    assert audit(m, off, sz, tags, N) == []
    # (a) layer 13 = Concat(T13, T1) -> T14
    _reported(audit(m, _place(off, 14, 1), sz, tags, N), "layer 13:", "writes T(14)", "over T(1)", "same launch reads")
    # (b) the 4-way Concat's output T11 over its leaf T7 (the chain launch reads it; layer by layer, record 10 = Concat(T10, T7) does)
    if chained:
        _reported(audit(m, _place(off, 11, 7), sz, tags, N), "concat chain 8..10 (4 leaves):", "writes T(11)", "over T(7)", "same launch reads")
    else:
        _reported(audit(m, _place(off, 10, 7), sz, tags, N), "layer 9:", "writes T(10)", "over T(7)", "same launch reads")
    # (c) T9 -- written by layer 8, or T12 by layer 11 where the chain never writes T9 -- over T1, which layers 13 and 14 still read
    mid = 12 if chained else 9
    got = audit(m, _place(off, mid, 1), sz, tags, N)
    _reported(got, "layer 13:", "reads T(1)", f"overwritten since by T({mid})", f"(layer {mid - 1})")
    _reported(got, "layer 14:", "reads T(1)", f"overwritten since by T({mid})")
    # (d) T28 over the embedding tensor T26, whose last layer reader is layer 26
    _reported(audit(m, _place(off, 28, 26), sz, tags, N), "embedding read-back:", "reads T(26)", "overwritten since by T(28)", "(layer 27)")
    # (e) T14 one unit short: reported where it is written and where it is read
    short = sz.copy()
    short[14] -= 64
    got = audit(m, off, short, tags, N)
    _reported(got, "layer 13:", "T(14) needs", f"the plan gives {short[14]}")
    _reported(got, "layer 15:", "reads T(14)", f"the plan gives {short[14]}")
    # (f) T6, read by the chain and by layer 12, without bytes
    none = sz.copy()
    none[6] = 0
    got = audit(m, off, none, tags, N)
    _reported(got, "layer 12:", "touches T(6)", "no bytes")
    _reported(got, "concat chain 8..10 (4 leaves):" if chained else "layer 8:", "touches T(6)", "no bytes")
    # (g) layer 20's output T21 over the gate T20, which layer 21 = T21 x gate reads after it
    assert _gate(m) == 21 and m.layers[21].res_tensor == 20
    _reported(audit(m, _place(off, 21, 20), sz, tags, N), "layer 21:", "reads T(20)", "overwritten since by T(21)", "(layer 20)")


def test_the_seeded_faults_in_generated_plans_are_reported_by_name(families):
    # (a), (c), (e), (f) on a DenseNet plan: its first two-source concat, the stem output's late reader
    m = families["dense_plan0"]
    tags = [PATH_LAYER] * len(m.layers)
    off, sz = sound_plan(m, tags)
    i = _two_source_concat(m, tags)
    B = m.layers[i].res_tensor
    _reported(audit(m, _place(off, i + 1, B), sz, tags, N), f"layer {i}:", f"writes T({i + 1})", f"over T({B})", "same launch reads")
    # a tensor with a reader at least three layers behind its writer, and a tensor written in between
    t, late = next((t, j) for t in range(1, len(m.layers)) for j in range(len(m.layers) - 1, t + 2, -1)
                   if t in (m.layers[j].in_tensor, m.layers[j].res_tensor))
    _reported(audit(m, _place(off, t + 1, t), sz, tags, N), f"layer {late}:", f"reads T({t})", f"overwritten since by T({t + 1})", f"(layer {t})")
    short = sz.copy()
    short[i + 1] -= 64
    _reported(audit(m, off, short, tags, N), f"layer {i}:", f"T({i + 1}) needs", f"the plan gives {short[i + 1]}")
    none = sz.copy()
    none[B] = 0
    _reported(audit(m, off, none, tags, N), f"layer {i}:", f"touches T({B})", "no bytes")
    # (b) on six_way: the first step's output T10 over its third leaf T3
    m = families["six_way"]
    tags = chain_tags(m, CHAINS["six_way"])
    off, sz = sound_plan(m, tags)
    assert m.layers[8].res_tensor == 4
    _reported(audit(m, _place(off, 10, 4), sz, tags, N), "concat chain 7..9 (4 leaves):", "writes T(10)", "over T(4)", "same launch reads")
    # ... and the second step's output over the first step's, which it reads as its first source, and over its last leaf
    _reported(audit(m, _place(off, 12, 10), sz, tags, N), "concat chain 10..11 (3 leaves):", "writes T(12)", "over T(10)")
    _reported(audit(m, _place(off, 12, 7), sz, tags, N), "concat chain 10..11 (3 leaves):", "writes T(12)", "over T(7)")
    # (d) on the same model: the dense layer's input is the embedding tensor; nothing is written behind it but the logits, so the
    # tensor placed over it is the head convolution's output, and the pool that writes the embedding reads it: the same launch
    assert m.embedding_tensor == 14
    _reported(audit(m, _place(off, 14, 13), sz, tags, N), "layer 13:", "writes T(14)", "over T(13)", "same launch reads")
    # (g) on a ResNeXt plan with gates: the scale follows its gate directly, so the gate is planned over the feature map D that
    # the scale launch reads as well
    m = families["resnext_plan1"]
    tags = [PATH_LAYER] * len(m.layers)
    off, sz = sound_plan(m, tags)
    i = _gate(m)
    D, G = m.layers[i].in_tensor, m.layers[i].res_tensor
    assert G == i and D < G
    _reported(audit(m, _place(off, G, D), sz, tags, N), f"layer {i}:", f"reads T({D})", f"overwritten since by T({G})", f"(layer {G - 1})")


def test_malformed_tag_lists_and_unknown_ops_raise(families):
    m = families["long_reach"]
    good = chain_tags(m, CHAINS["long_reach"])
    assert schedule(m, good)
    bad = list(good)
    bad[11:13] = [PATH_CONCAT, PATH_INNER]                  # layers 11, 12: 1x1 convolutions
    with pytest.raises(AssertionError, match="layer 11: tagged as the start of a concat chain but its op code is 3"):
        schedule(m, bad)
    bad = list(good)
    bad[8] = PATH_LAYER                                     # an inner tag behind a step of one layer
    with pytest.raises(AssertionError, match="layer 9 starts a launch but is tagged as inside an earlier one"):
        schedule(m, bad)
    # the record behind the embedding tensor drawn into the chain in front of it: by its records it is a chain (to refuse it is the
    # library's matcher's business), and the plan that goes with it -- no bytes for T26 -- is reported at the read-back
    bad = list(good)
    bad[26] = PATH_INNER
    assert len(schedule(m, bad)) == len(schedule(m, good)) - 1
    _reported(audit(m, *sound_plan(m, bad), bad, N), "embedding read-back:", "touches T(26)", "no bytes")
    with pytest.raises(AssertionError, match="unknown path tag 7"):
        schedule(m, [7] + good[1:])
    six = families["six_way"]
    with pytest.raises(AssertionError, match="6 leaves in one launch"):
        schedule(six, chain_tags(six, [(7, 11)]))
    with pytest.raises(AssertionError, match="a concat chain of one record"):
        schedule(six, chain_tags(six, [(7, 9), (10, 10)]))
    for code in (9, 11, 15):
        odd = copy.deepcopy(m)
        odd.layers[15].op = code
        with pytest.raises(AssertionError, match=f"layer 15: op code {code} has no entry"):
            schedule(odd, [PATH_LAYER] * len(odd.layers))
    odd = copy.deepcopy(m)
    odd.layers[2].res_tensor = 1                            # a depthwise layer's launch takes no second tensor
    with pytest.raises(AssertionError, match="layer 2: op 2 names T\\(1\\), which its launch never reads"):
        schedule(odd, [PATH_LAYER] * len(odd.layers))


def test_long_reach_model_is_valid_and_holds_what_it_promises(tmp_path):
    import torch
    from birda_amd import synth
    from test_concat import _load, forward64
    m = long_reach_model()
    path = str(tmp_path / "long_reach.bhm")
    mf.write_model(path, m)
    rc, err = _load(path)
    assert rc >= 0, err
    L = m.layers
    readers = lambda t: [j for j, R in enumerate(L) if t in (R.in_tensor, R.res_tensor)]
    assert 20 <= len(L) < 30 and L[0].cout == 16 and len(m.branches) == 1 and m.spec_h == 32
    assert readers(1) == [1, 13, 14] and L[13].op == mf.OP_CONCAT and L[13].res_tensor == 1 and 13 - 0 >= 12      # T1: written by layer 0
    assert L[14].op == mf.OP_CONCAT and L[14].res_tensor == NONE and L[14].w_off == 8                              # the Split spelling
    assert readers(2) == [2, 3, 4] and L[4].res_tensor == 2                                                        # three readers, the last a residual
    assert [L[j].op for j in (8, 9, 10)] == [mf.OP_CONCAT] * 3 and L[9].in_tensor == 9 and L[10].in_tensor == 10
    assert readers(6) == [8, 12]                                                                                   # a leaf read after the chain
    assert m.embedding_tensor == 26 and readers(26) == [26] and L[26].op == mf.OP_CONCAT and L[26].in_tensor == 26 and len(L) == 29
    assert L[21].op == mf.OP_SCALE and L[21].res_tensor == 20 and L[20].op == mf.OP_PWCONV
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=7)
    T = forward64(m, segs, tensors=True)
    assert all(np.isfinite(t).all() for t in T) and np.abs(T[-1]).max() > 0 and T[-1].reshape(2, -1).shape == (2, 12)
    for i, R in enumerate(L):
        if R.op != mf.OP_CONCAT:
            continue
        nchw = lambda t: torch.from_numpy(np.ascontiguousarray(np.asarray(T[t]).reshape(2, R.in_h, R.in_w, -1).transpose(0, 3, 1, 2)))
        parts = [nchw(R.in_tensor).narrow(1, R.w_off, R.cin)]
        if R.res_tensor != NONE:
            parts.append(nchw(R.res_tensor).narrow(1, R.b_off, R.cout - R.cin))
        want = torch.cat(parts, dim=1).numpy().transpose(0, 2, 3, 1)
        assert T[i + 1].shape == want.shape and (T[i + 1] == want).all(), i
    # the 4-way Concat is its four leaves side by side, and the scale is the feature map times its gate
    px = lambda t: np.asarray(T[t]).reshape(2, 16 * 58, -1)
    assert (px(11) == np.concatenate([px(4), px(6), px(7), px(8)], axis=2)).all()
    assert np.abs(px(22) - px(21) * np.asarray(T[20]).reshape(2, 1, 24)).max() <= 1e-12 * np.abs(px(22)).max()
