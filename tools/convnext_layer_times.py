"""What the LayerNorm and the 7x7 depthwise layers of a ConvNeXt cost: synth's `convnext_audio` (ConvNeXt-T's layout on the v2.4
front end) at the benchmark's batch, on the launch harness of tools/gpu_layer_times.py (forwards of n segments in one launch each
through forward_device, HIP events around every layer's launch: bh_batch_context_layer_ms).

  python tools/convnext_layer_times.py [n] [table.txt]          (PREC=auto|f16x3|f32; run from anywhere: bench.py, whose ClockSampler
  samples the shader clock during the rounds, is imported from the repository root, the directory above this one)

Two models in ONE process, REPEATS = 5 rounds after two warm-up forwards each, the order swapped every round:
  (1) convnext_audio as built;
  (2) its 5x5 twin: the same records with every depthwise layer 5x5 (pads 2; the first 25 taps of the same weights) -- for scale.
Per LayerNorm layer: lnorm_kernel's median time and the rate of the bytes it moves (input + output), against a device-to-device
copy of the same bytes (torch's copy_ between two buffers of the tensor's size, HIP events, the same rounds) -- the rate an HBM-bound
layer can reach here.  Per depthwise layer: dwconv_kernel<7,1>'s median time, its rate over input + output, and the twin's 5x5.
Last: the share of the model's step (the sum over all layers) that the two ops take together.  Nothing is gated: the table is what
a depthwise + LayerNorm fusion would be argued from."""
import copy, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from birda_amd import modelfile as mf, synth

WARMUP, REPEATS = 2, 5


def twin_5x5(m: mf.Model) -> mf.Model:
    t = copy.deepcopy(m)
    for L in t.layers:
        if L.op == mf.OP_DWCONV:
            L.kh = L.kw = 5
            L.pad_t = L.pad_l = 2
    return t


def main():
    import torch
    import bench                                            # (ROOT/bench.py: ClockSampler)
    from birda_amd.classifier import BirdClassifier
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    out_path = sys.argv[2] if len(sys.argv) > 2 else "convnext_layers.txt"
    prec = os.environ.get("PREC", "auto")
    m = synth.build_model("convnext_audio", n_classes=6522)
    models = [("as built", m), ("5x5 twin", twin_5x5(m))]
    base = synth.synth_segments(16, m.sample_count, m.sample_rate)
    x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
    logits = [torch.empty((N, m.n_classes), device="cuda") for _ in models]
    runs = []
    with tempfile.TemporaryDirectory() as d:
        for k, (_, model) in enumerate(models):
            path = os.path.join(d, f"m{k}.bhm"); mf.write_model(path, model)
            clf = BirdClassifier(path, precision=prec)
            ctx = clf.create_batch_context(N)
            ctx.set_sub_slices(1)
            runs.append((clf, ctx))
    times = [[[] for _ in m.layers] for _ in models]
    norms = [i for i, L in enumerate(m.layers) if L.op == mf.OP_LNORM]
    dws = [i for i, L in enumerate(m.layers) if L.op == mf.OP_DWCONV]
    # one pair of buffers per distinct LayerNorm tensor size, for the copy
    sizes = sorted({N * m.layers[i].out_h * m.layers[i].out_w * m.layers[i].cout for i in norms})
    bufs = {s: (torch.randn(s, device="cuda"), torch.empty(s, device="cuda")) for s in sizes}
    copies = {s: [] for s in sizes}

    def fwd(k, keep):
        clf, ctx = runs[k]
        ctx.set_profiling(True)
        clf.forward_device(ctx, x.data_ptr(), N, logits[k].data_ptr())
        ctx.synchronize()
        if keep:
            for i, (ms, n) in enumerate(ctx.layer_ms()):
                times[k][i].append(ms if n else 0.0)
        ctx.set_profiling(False)

    def copy_round(keep):
        for s, (a, b) in bufs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); b.copy_(a); e1.record(); e1.synchronize()
            if keep:
                copies[s].append(e0.elapsed_time(e1))

    for k in range(2):
        for _ in range(WARMUP):
            fwd(k, False)
    copy_round(False); copy_round(False)
    with bench.ClockSampler(0) as cs:
        for r in range(REPEATS):
            for k in ((0, 1) if r % 2 == 0 else (1, 0)):
                fwd(k, True)
            copy_round(True)
    clk = cs.summary()
    med = lambda v: float(np.median(np.asarray(v)))
    gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9 if ms > 0 else float("nan")
    names = [runs[0][0].layer_kernel(i) for i in range(len(m.layers))]
    lines = [f"convnext_audio (ConvNeXt-T: widths 96 / 192 / 384 / 768, depths 3 / 3 / 9 / 3), {N} segments a forward, precision {prec}, {torch.cuda.get_device_name(0)}; "
             f"{REPEATS} rounds after {WARMUP} warm-up forwards each, the order swapped every round; shader clock during the rounds {clk['sclk_mhz']} MHz "
             f"({clk['sclk_mhz_min_max']}), {clk['power_w']} W, {clk['samples']} samples",
             "", "LayerNorm layers (bytes = input + output; copy = a device-to-device copy of the same bytes in the same rounds)",
             "layer  image      C     kernel               ms (median / min)     GB/s    copy ms (median)  copy GB/s   lnorm / copy"]
    ratios = []
    for i in norms:
        L = m.layers[i]
        s = N * L.out_h * L.out_w * L.cout
        t, c = med(times[0][i]), med(copies[s])
        ratios.append(t / c)
        lines.append(f"{i:5d}  {L.out_h:3d}x{L.out_w:3d}  {L.cout:5d}  {names[i]:<20s} {t:9.4f} / {min(times[0][i]):8.4f}  {gbs(8 * s, t):8.1f}  {c:12.4f}     {gbs(8 * s, c):8.1f}     {t / c:6.2f}")
    lines += ["", "depthwise layers (bytes = input + output; the twin runs dwconv_kernel<5,1> on the same image)",
              "layer  image      C     kernel               7x7 ms (median / min)  GB/s    5x5 twin ms (median)   7x7 / 5x5"]
    dratios = []
    for i in dws:
        L = m.layers[i]
        s = N * L.out_h * L.out_w * L.cout
        t7, t5 = med(times[0][i]), med(times[1][i])
        dratios.append(t7 / t5)
        lines.append(f"{i:5d}  {L.out_h:3d}x{L.out_w:3d}  {L.cout:5d}  {names[i]:<20s} {t7:9.4f} / {min(times[0][i]):8.4f}  {gbs(8 * s, t7):8.1f}  {t5:12.4f}            {t7 / t5:6.2f}")
    step = [float(np.sum([np.asarray(times[0][i])[r] for i in range(len(m.layers))])) for r in range(REPEATS)]
    ln_t = [float(np.sum([np.asarray(times[0][i])[r] for i in norms])) for r in range(REPEATS)]
    dw_t = [float(np.sum([np.asarray(times[0][i])[r] for i in dws])) for r in range(REPEATS)]
    lines += ["", f"all layers of a forward: {med(step):.3f} ms ({N / med(step) * 1e3:.0f} segments/s of layer time); LayerNorm {med(ln_t):.3f} ms ({100 * med(ln_t) / med(step):.1f} %), "
                  f"depthwise 7x7 {med(dw_t):.3f} ms ({100 * med(dw_t) / med(step):.1f} %), together {100 * (med(ln_t) + med(dw_t)) / med(step):.1f} % of the step",
              f"lnorm / copy over the layers: {min(ratios):.2f} .. {max(ratios):.2f} (median {med(ratios):.2f}); depthwise 7x7 / 5x5: {min(dratios):.2f} .. {max(dratios):.2f} (median {med(dratios):.2f})",
              f"a block's depthwise output goes to HBM and comes back for its LayerNorm: {sum(8 * N * m.layers[i].out_h * m.layers[i].out_w * m.layers[i].cout for i in dws) / 1e9:.2f} GB a forward "
              "that one launch for both would not move"]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    for clf, ctx in runs:
        ctx.close(); clf.close()


if __name__ == "__main__":
    main()
