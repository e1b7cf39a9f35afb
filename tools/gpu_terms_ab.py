"""Two-term against three-term products on float16 model files, in ONE process (run on the GPU box).

For each model (default: birdnet_v30_v2l and birdnet_v24, written as float16 .onnx files by convert.graph_to_float16) two
classifiers of the same file -- the default (two terms on compact planes wherever a layer's weights are f16 values) and
BH_FLAG_FULL_PLANES (three terms on full planes: the parent commit's path) -- run device-resident forwards of 256 and 1 000
segments, plus 1 segment for the dense layer, warmed, ALTERNATING the two classifiers REPS times (default 5).  Printed per launch
size: segments/s of both (median and spread over the repeats), and per GEMM layer outside the fused blocks its kernel, the
HIP-event time of both forms (median, min-max over the repeats) with the same runs' mel stage beside them as the clock reference
(the pool's boxes change clock between runs; the front-end does not depend on the weight planes).  A layer counts as slower only
beyond the spread the alternation itself shows between repeats of one variant.

    python tools/gpu_terms_ab.py [--models a,b] [--reps 5] [--sizes 256,1000,1] [--out profiles/fp16_two_terms.txt]
    python tools/gpu_terms_ab.py --trace [--models a] [--sizes 256]     # plain forwards of both classifiers, no events: the program
                                                                        # for `rocprofv3 --kernel-trace --stats -- python ...`

The three-term path is the parent commit's code.  To show it, build the parent's library beside this one (its csrc in a worktree,
linked as tools/ab/libbirda_hip_parent.so) and alternate, one process each, on the SAME file -- an f32 BHM1 container whose weights
are f16 values, which the parent reads too:

    python tools/gpu_terms_ab.py --container birdnet_v30_v2l --lib tools/ab/libbirda_hip_parent.so     # the parent: three terms
    python tools/gpu_terms_ab.py --container birdnet_v30_v2l --full-planes                              # this build, three terms
    python tools/gpu_terms_ab.py --container birdnet_v30_v2l                                            # this build, two terms

each prints one line (segments/s median / min / max, mel / pointwise / dense stage times, a checksum of the logits); the first
two must agree within the spread of their repeats.
"""
import argparse
import os
import statistics as st
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from birda_amd import convert, modelfile as mf, onnx_io as ox, synth
from birda_amd.classifier import BirdClassifier


def float16_file(kind, d):
    m = synth.build_model(kind)
    p = os.path.join(d, kind + "_fp16.onnx")
    with open(p, "wb") as f:
        f.write(ox.dump(convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="conv1d"))))
    return m, p


def container_leg(a):
    """one process, one library, one f32 container of f16 values: a line of times"""
    from birda_amd import _lib
    if a.lib:      # another build of the library (the parent's): bind what it exports
        import ctypes
        L = ctypes.CDLL(os.path.abspath(a.lib))
        for table in (_lib.SYMBOLS, _lib.HOST_SYMBOLS, _lib.AUDIT_SYMBOLS, _lib.LAYER_DEBUG_SYMBOLS, _lib.BLOCK_DEBUG_SYMBOLS, _lib.TERMS_DEBUG_SYMBOLS):
            table[:] = [e for e in table if hasattr(L, e[0])]
        _lib.LIB_PATH = os.path.abspath(a.lib)
    kind, N = a.container, int(a.sizes.split(",")[0])
    m = synth.build_model(kind)
    m.blob = np.asarray(m.blob, np.float32).astype(np.float16).astype(np.float32)
    path = os.path.join(tempfile.mkdtemp(), kind + "_f16_values.bhm")
    mf.write_model(path, m)
    clf = BirdClassifier(path, None, precision="auto", full_planes=a.full_planes)
    os.remove(path)
    x = torch.from_numpy(np.tile(synth.synth_segments(16, m.sample_count, m.sample_rate), (N // 16 + 1, 1))[:N].copy()).cuda()
    logits = torch.empty((N, m.n_classes), device="cuda")
    idx = torch.empty((N, 5), dtype=torch.int32, device="cuda")
    conf = torch.empty((N, 5), device="cuda")
    ctx = clf.create_batch_context(N)

    def forward():
        clf.forward_device(ctx, x.data_ptr(), N, logits.data_ptr(), idx.data_ptr(), conf.data_ptr())
        ctx.synchronize()
    for _ in range(3):
        forward()
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter()
        forward()
        ts.append(time.perf_counter() - t)
    ctx.set_profiling(True)
    forward()
    stg = ctx.stage_ms()
    two = clf.weight_summary()["two_term_layers"] if hasattr(_lib.load(), "bh_classifier_weight_summary") else 0
    r = sorted(N / t for t in ts)
    print(f"{kind} {'parent library' if a.lib else 'this build'}{', BH_FLAG_FULL_PLANES' if a.full_planes else ''} ({two} two-term layers), {N} segments: "
          f"{st.median(r):9.0f} segments/s (min {r[0]:.0f}, max {r[-1]:.0f}); mel {stg['mel'][0] * 1e3:.1f} us, pointwise {stg['pointwise'][0] * 1e3:.1f} us, "
          f"dense {stg['dense'][0] * 1e3:.1f} us; logits checksum {float(logits.double().sum().item()):.12e}", flush=True)
    ctx.close()
    clf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="birdnet_v30_v2l,birdnet_v24")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="256,1000,1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--container", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--full-planes", action="store_true")
    a = ap.parse_args()
    if a.container:
        return container_leg(a)
    sizes = [int(x) for x in a.sizes.split(",")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    d = tempfile.mkdtemp()
    for kind in a.models.split(","):
        m, path = float16_file(kind, d)
        clfs = {"two": BirdClassifier(path, None, precision="auto"), "full": BirdClassifier(path, None, precision="auto", full_planes=True)}
        os.remove(path)
        ws = {k: c.weight_summary() for k, c in clfs.items()}
        terms = clfs["two"].layer_terms()
        say(f"== {kind} (float16 file): {ws['two']['gemm_layers']} GEMM layers outside fused blocks, {ws['two']['two_term_layers']} on two terms; "
            f"plane bytes {ws['two']['plane_bytes'] / 1e6:.1f} MB against {ws['full']['plane_bytes'] / 1e6:.1f} MB under BH_FLAG_FULL_PLANES")
        base = synth.synth_segments(16, m.sample_count, m.sample_rate)
        for N in sizes:
            x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N].copy()).cuda()
            logits = {k: torch.empty((N, m.n_classes), device="cuda") for k in clfs}
            idx = torch.empty((N, 5), dtype=torch.int32, device="cuda")
            conf = torch.empty((N, 5), device="cuda")
            ctxs = {k: c.create_batch_context(N) for k, c in clfs.items()}

            def forward(k):
                clfs[k].forward_device(ctxs[k], x.data_ptr(), N, logits[k].data_ptr(), idx.data_ptr(), conf.data_ptr())
                ctxs[k].synchronize()
            for k in clfs:
                for _ in range(3):
                    forward(k)
            if a.trace:
                for _ in range(a.reps):
                    for k in ("two", "full"):
                        forward(k)
                for c in ctxs.values():
                    c.close()
                continue
            same = bool((logits["two"] == logits["full"]).all().item())
            wall = {k: [] for k in clfs}
            layer = {k: [] for k in clfs}
            mel = {k: [] for k in clfs}
            for _ in range(a.reps):
                for k in ("two", "full"):
                    ctxs[k].set_profiling(False)
                    t = time.perf_counter()
                    forward(k)
                    wall[k].append(time.perf_counter() - t)
                    ctxs[k].set_profiling(True)
                    forward(k)
                    layer[k].append([v[0] for v in ctxs[k].layer_ms()])
                    mel[k].append(ctxs[k].stage_ms()["mel"][0])
            say(f"-- {N} segments a launch; logits of the two classifiers equal as numbers: {same}")
            for k in ("two", "full"):
                r = sorted(N / w for w in wall[k])
                say(f"   {k:4s}: {st.median(r):9.0f} segments/s (min {r[0]:.0f}, max {r[-1]:.0f}); mel stage {st.median(mel[k]) * 1e3:8.1f} us "
                    f"(min {min(mel[k]) * 1e3:.1f}, max {max(mel[k]) * 1e3:.1f})")
            say("   layer  shape (K -> N, rows/segment)         kernel (two-term classifier)                        two: us med (min-max)      "
                "full: us med (min-max)     two/full   verdict")
            for i, L in enumerate(m.layers):
                if terms[i] == 0:
                    continue
                t2 = sorted(r[i] * 1e3 for r in layer["two"])
                t3 = sorted(r[i] * 1e3 for r in layer["full"])
                if st.median(t3) == 0.0:
                    continue
                K = L.kh * L.kw * L.cin if L.op == mf.OP_CONV else L.cin
                spread = max(t2[-1] - t2[0], t3[-1] - t3[0])
                verdict = "slower" if st.median(t2) - st.median(t3) > spread else ("faster" if st.median(t3) - st.median(t2) > spread else "within spread")
                say(f"   {i:5d}  {K:5d} -> {L.cout:5d}, {L.out_h * L.out_w:5d} rows  T={terms[i]}  {clfs['two'].layer_kernel(i) or '(gated / fused launch)':50s} "
                    f"{st.median(t2):9.1f} ({t2[0]:.1f}-{t2[-1]:.1f})   {st.median(t3):9.1f} ({t3[0]:.1f}-{t3[-1]:.1f})   "
                    f"{st.median(t2) / st.median(t3):6.3f}   {verdict}")
            for c in ctxs.values():
                c.close()
        for c in clfs.values():
            c.close()
    if a.out and not a.trace:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
