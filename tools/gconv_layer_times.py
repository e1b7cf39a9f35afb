"""The grouped layers of synth's `resnext_audio` beside the only way the library could run them before it had OP_GCONV: the same
layer as a dense OP_CONV with block-diagonal weights (conv_gemm_kernel / conv_gemm16_kernel<3>), which spends G times the MFMAs and
weight bytes on zeros.
  python tools/gconv_layer_times.py [n] [table.txt]            (PREC=auto|f16x3|f32|f16; ACT=relu6: every ReLU read as ReLU6, which puts
  the dense twin on conv_gemm16_kernel<3,RELU6> instead of the f32 conv_gemm_kernel; also the program of a
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gconv_layer_times.py ... run)
Forwards of n segments (default 1 000) in one launch each, the two models taking turns in ONE process: after two warm-up forwards
of each, REPEATS rounds, the order of the pair swapped every round (neither always runs behind the other).  Every forward is
profiled on its own (HIP events around every layer's launch: bh_batch_context_layer_ms), so each layer has REPEATS times per model;
the table gives the median and the minimum of both, the twin's run-to-run spread ((max - min) / median), the layer's input + output
bytes over its median time, and a device-to-device copy of the same bytes timed in the same process."""
import copy, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from birda_amd import modelfile as mf, synth

WARMUP, REPEATS = 2, 8


def dense_twin(m: mf.Model) -> mf.Model:
    """m with every OP_GCONV layer as an OP_CONV layer of block-diagonal weights [kh][kw][cin][cout] (appended to the blob)"""
    t = copy.deepcopy(m)
    chunks, off = [np.asarray(m.blob, np.float32)], int(m.blob.size)
    for L in t.layers:
        if L.op != mf.OP_GCONV:
            continue
        G, gi, go = L.reserved, L.cin // L.reserved, L.cout // L.reserved
        w = m.blob[L.w_off:L.w_off + L.kh * L.kw * gi * L.cout].reshape(L.kh, L.kw, gi, L.cout)
        dense = np.zeros((L.kh, L.kw, L.cin, L.cout), np.float32)
        for g in range(G):
            dense[:, :, g * gi:(g + 1) * gi, g * go:(g + 1) * go] = w[:, :, :, g * go:(g + 1) * go]
        pad = (-off) % 16
        chunks += [np.zeros(pad, np.float32), dense.ravel()]
        L.op, L.reserved, L.w_off = mf.OP_CONV, 0, off + pad
        off += pad + dense.size
    t.blob = np.concatenate(chunks)
    return t


def main():
    import torch
    from birda_amd.classifier import BirdClassifier
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    out_path = sys.argv[2] if len(sys.argv) > 2 else "gconv_layers.txt"
    prec = os.environ.get("PREC", "auto")
    m = synth.build_model("resnext_audio")
    if os.environ.get("ACT") == "relu6":     # the like-for-like pair: ReLU (before an add) is no activation of the split-f16 full-convolution
        for L in m.layers:                   # epilogue, so the dense twin of the model as built runs the f32 conv_gemm_kernel; ReLU6 is one
            if L.act == mf.ACT_RELU:
                L.act = mf.ACT_RELU6
    grouped = [i for i, L in enumerate(m.layers) if L.op == mf.OP_GCONV]
    models = [("grouped", m), ("dense twin", dense_twin(m))]
    base = synth.synth_segments(16, m.sample_count, m.sample_rate)
    x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
    logits = [torch.empty((N, m.n_classes), device="cuda") for _ in models]
    runs = []
    with tempfile.TemporaryDirectory() as d:
        for k, (tag, model) in enumerate(models):
            path = os.path.join(d, f"resnext_audio_{k}.bhm"); mf.write_model(path, model)
            clf = BirdClassifier(path, precision=prec)
            ctx = clf.create_batch_context(N)
            ctx.set_sub_slices(1)
            runs.append((clf, ctx))
    times = [[[] for _ in m.layers] for _ in models]

    def fwd(k, keep):
        clf, ctx = runs[k]
        ctx.set_profiling(True)
        clf.forward_device(ctx, x.data_ptr(), N, logits[k].data_ptr())
        ctx.synchronize()
        for i, (ms, n) in enumerate(ctx.layer_ms()):
            if keep and n:
                times[k][i].append(ms)
        ctx.set_profiling(False)

    for k in range(2):
        for _ in range(WARMUP):
            fwd(k, False)
    for r in range(REPEATS):
        for k in ((0, 1) if r % 2 == 0 else (1, 0)):
            fwd(k, True)
    # the two models compute the same function: the twin's zeros add nothing
    diff = float((logits[0] - logits[1]).abs().max())
    scale = float(logits[0].abs().max())
    lines = [f"resnext_audio ({os.environ.get('ACT', 'relu')}), {N} segments a forward, precision {prec}, {torch.cuda.get_device_name(0)}; {REPEATS} alternating rounds after {WARMUP} warm-up forwards each",
             f"max |logit(grouped) - logit(dense twin)| = {diff:.3e} of {scale:.2f}",
             "layer  shape                              G  kernel              grouped ms (median / min)  dense twin ms (median / min)  twin spread  ratio   in+out MB   TB/s   d2d copy ms  TB/s"]
    for i in grouped:
        L = m.layers[i]
        g, t = np.asarray(times[0][i]), np.asarray(times[1][i])
        nbytes = 4 * N * (L.in_h * L.in_w * L.cin + L.out_h * L.out_w * L.cout)
        src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        copies = []
        for r in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
            if r >= 2:
                copies.append(e0.elapsed_time(e1))
        cp = float(np.median(copies))
        del src, dst
        gm, tm = float(np.median(g)), float(np.median(t))
        lines.append(f"{i:5d}  {L.kh}x{L.kw}/{L.sh} {L.cin:4d}->{L.cout:4d} {L.in_h:3d}x{L.in_w:3d}->{L.out_h:3d}x{L.out_w:3d}  {L.reserved:3d}  {runs[0][0].layer_kernel(i):18s}  "
                     f"{gm:9.3f} / {g.min():9.3f}      {tm:9.3f} / {t.min():9.3f}       {(t.max() - t.min()) / tm:6.3f}      {tm / gm:6.2f}  {nbytes / 1e6:9.1f}  {nbytes / (gm * 1e-3) / 1e12:5.2f}  {cp:9.3f}   {nbytes / (cp * 1e-3) / 1e12:5.2f}")
    lines.append("dense twin kernels: " + ", ".join(sorted({runs[1][0].layer_kernel(i) or "conv_gemm_kernel (f32)" for i in grouped})))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    for clf, ctx in runs:
        ctx.close(); clf.close()


if __name__ == "__main__":
    main()
