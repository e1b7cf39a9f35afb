"""What the fused hard-swish blocks cost: every hard-swish inverted-residual block of synth's `mobilenetv3_audio` and of one gated
`random_mnv3_plan` (seed 1), each timed three ways in ONE process on the launch harness of tools/gpu_layer_times.py (forwards of n
segments in one launch each through forward_device, HIP events around every layer's launch: bh_batch_context_layer_ms; a fused block
is booked on its first layer):

  (1) as built: fused on the hard-swish family (tile index 3 n_base + base);
  (2) the swish twin: the same file with activation code 3 for 7 (and the sigmoid for the hard-sigmoid gate) -- the SAME tile entry
      of family 1 (the table asserts base == base), the code the library had before the family existed;
  (3) layer by layer: the model as built with BIRDA_HIP_FUSE=0 at create.

  python tools/hswish_layer_times.py [n] [table.txt]            (PREC=auto|f16x3|f32|f16; run from anywhere: bench.py, whose
  ClockSampler samples the shader clock during the rounds, is imported from the repository root, the directory above this one)
A block's time is the sum over its layers (expand .. project; for a gated block pass A, the gate and the gated project GEMM) of one
forward; after two warm-up forwards of each model, REPEATS = 5 rounds with the order rotated.  Per block: median and minimum of (1)
and (2), the twin's own run-to-run spread ((max - min) / median over its 5 repeats), the ratio, and the pass line ratio <= 1 +
spread; then (3) and its ratio to (1).  A block over the pass line is reported, not tuned."""
import copy, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from birda_amd import modelfile as mf, synth

WARMUP, REPEATS = 2, 5


def swish_twin(m: mf.Model) -> mf.Model:
    t = copy.deepcopy(m)
    for L in t.layers:
        L.act = {mf.ACT_HSWISH: mf.ACT_SWISH, mf.ACT_HSIGMOID: mf.ACT_SIGMOID}.get(L.act, L.act)
    return t


def blocks_of(m):
    """(first, last) layer of every hard-swish block: [expand 1x1,] depthwise, [pool, 1x1, 1x1, scale,] project 1x1"""
    out = []
    for d, L in enumerate(m.layers):
        if L.op == mf.OP_DWCONV and L.act == mf.ACT_HSWISH:
            E = m.layers[d - 1]
            first = d - 1 if (E.op == mf.OP_PWCONV and E.act == mf.ACT_HSWISH and L.in_tensor == d) else d
            out.append((first, d + 5 if m.layers[d + 1].op == mf.OP_GAP else d + 1))
    return out


def time_model(tag, m, N, prec, lines):
    import torch
    import bench                                            # (ROOT/bench.py: ClockSampler)
    from birda_amd.classifier import BirdClassifier
    models = [("as built", m, None), ("swish twin", swish_twin(m), None), ("layer by layer", m, "0")]
    base = synth.synth_segments(16, m.sample_count, m.sample_rate)
    x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
    logits = [torch.empty((N, m.n_classes), device="cuda") for _ in models]
    runs = []
    with tempfile.TemporaryDirectory() as d:
        for k, (_, model, fuse) in enumerate(models):
            path = os.path.join(d, f"m{k}.bhm"); mf.write_model(path, model)
            os.environ.pop("BIRDA_HIP_FUSE", None)
            if fuse is not None:
                os.environ["BIRDA_HIP_FUSE"] = fuse
            clf = BirdClassifier(path, precision=prec)
            os.environ.pop("BIRDA_HIP_FUSE", None)
            ctx = clf.create_batch_context(N)
            ctx.set_sub_slices(1)
            runs.append((clf, ctx))
    times = [[[] for _ in m.layers] for _ in models]

    def fwd(k, keep):
        clf, ctx = runs[k]
        ctx.set_profiling(True)
        clf.forward_device(ctx, x.data_ptr(), N, logits[k].data_ptr())
        ctx.synchronize()
        if keep:
            for i, (ms, n) in enumerate(ctx.layer_ms()):
                times[k][i].append(ms if n else 0.0)
        ctx.set_profiling(False)

    for k in range(3):
        for _ in range(WARMUP):
            fwd(k, False)
    with bench.ClockSampler(0) as cs:
        for r in range(REPEATS):
            for k in [(r + j) % 3 for j in range(3)]:
                fwd(k, True)
    clk = cs.summary()
    n_base = 0
    buf = __import__("ctypes").create_string_buffer(128)
    while runs[0][0]._L.bh_mb_config_name(n_base, buf, 128) > 0:
        n_base += 1
    n_base //= 3
    fused = [clf.fused_blocks() for clf, _ in runs]
    same = float((logits[0] - logits[2]).abs().max())
    blocks = blocks_of(m)
    lines.append(f"{tag}, {N} segments a forward, precision {prec}, {torch.cuda.get_device_name(0)}; {REPEATS} rotating rounds after {WARMUP} warm-up forwards each; "
                 f"shader clock during the rounds {clk['sclk_mhz']} MHz ({clk['sclk_mhz_min_max']}), {clk['power_w']} W, {clk['samples']} samples")
    lines.append(f"fused blocks: as built {len(fused[0])} (tile indices / n_base: {sorted({c // n_base for c in fused[0]})}), swish twin {len(fused[1])} "
                 f"({sorted({c // n_base for c in fused[1]})}), layer by layer {len(fused[2])}; same base entries: {[c % n_base for c in fused[0]] == [c % n_base for c in fused[1]]}; "
                 f"max |logit(as built) - logit(layer by layer)| = {same:.3e}")
    head = len(lines)
    lines.append("block  layers   shape (Cin -> Cexp -> Cout, k / s, image)      gate  entry  hswish fused ms (median / min)  swish twin ms (median / min)  twin spread  ratio  pass   layer by layer ms  / fused")
    worst, over = 0.0, []
    for bi, (a, z) in enumerate(blocks):
        per = [np.sum([np.asarray(times[k][i]) for i in range(a, z + 1)], axis=0) for k in range(3)]
        hm, tm, lm = (float(np.median(p)) for p in per)
        spread = float((per[1].max() - per[1].min()) / tm)
        worst = max(worst, spread)
        ok = hm / tm <= 1.0 + spread
        if not ok:
            over.append(bi)
        D = next(L for L in m.layers[a:z + 1] if L.op == mf.OP_DWCONV)
        P = m.layers[z]
        entry = fused[0][bi] % n_base if bi < len(fused[0]) else -1
        lines.append(f"{bi:5d}  {a:3d}-{z:3d}  {m.layers[a].cin:4d} -> {D.cout:4d} -> {P.cout:4d}  {D.kh}x{D.kw}/{D.sh}  {D.in_h:3d}x{D.in_w:3d} -> {D.out_h:3d}x{D.out_w:3d}   {'yes' if z - a > 2 else 'no ':3s}  {entry:5d}  "
                     f"{hm:10.4f} / {per[0].min():8.4f}        {tm:10.4f} / {per[1].min():8.4f}        {spread:6.3f}      {hm / tm:5.2f}  {'yes' if ok else 'NO ':3s}  {lm:10.4f}         {lm / hm:5.2f}")
    tot = [float(np.median(np.sum([np.sum([np.asarray(times[k][i]) for i in range(a, z + 1)], axis=0) for a, z in blocks], axis=0))) for k in range(3)]
    lines.insert(head, f"twin's run-to-run spread over the blocks: at most {worst:.3f}; blocks over 1 + spread: {over or 'none'}; all blocks: fused {tot[0]:.3f} ms, swish twin {tot[1]:.3f} ms "
                       f"(ratio {tot[0] / tot[1]:.3f}), layer by layer {tot[2]:.3f} ms ({tot[2] / tot[0]:.2f} x fused)")
    lines.append("")
    for clf, ctx in runs:
        ctx.close(); clf.close()


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    out_path = sys.argv[2] if len(sys.argv) > 2 else "hswish_layers.txt"
    prec = os.environ.get("PREC", "auto")
    lines = []
    time_model("mobilenetv3_audio", synth.build_model("mobilenetv3_audio"), N, prec, lines)
    time_model("mnv3_plan, random_mnv3_plan(1) (gated)", synth.build_model("mnv3_plan", plan=synth.random_mnv3_plan(1)), N, prec, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
