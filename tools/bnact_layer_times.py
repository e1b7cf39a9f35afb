"""What the norm + activation layers (OP_BNACT: a folded BatchNormalization and its activation) and the concats of a DenseNet cost.

  python tools/bnact_layer_times.py [n] [table.txt]          (table.txt: profiles/bnact_layers.txt of the repository by default; PREC=auto|f16x3|f32; run from anywhere: bench.py, whose ClockSampler
  samples the shader clock during the rounds, is imported from the repository root, the directory above this one)

Two parts, one process:
  (1) synth's `densenet_audio` (DenseNet-121 on the v2.4 front end) at n segments a forward on the launch harness of
      tools/gpu_layer_times.py (forward_device, HIP events around every layer's launch: bh_batch_context_layer_ms), REPEATS rounds after
      two warm-up forwards: the layer time of a step by op, the share of the norm + activation layers and of the concats.  Twice: the
      records both readers make of the model's .onnx file with its concats spelled as the growing list (prefix reuse: one two-source
      record a dense layer), and the records the same file gave WITHOUT prefix reuse (every Concat a left-to-right chain over its whole
      list), rebuilt here from the model.
  (2) bnact_kernel alone on device buffers (bh_debug_bnact_on_device, and bh_debug_scale_on_device for the yardstick, between two events on the null stream) on the model's two largest
      norm + activation tensors at n segments, with ReLU and with swish, against a device-to-device copy of
      the same bytes (torch's copy_) and against scale_kernel, the nearest existing kernel (launch_scale: x times a [n][C] gate), on the
      same tensor: ROUNDS rounds, the four launches taking turns inside every round.
Nothing is gated: the table states the ratios."""
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from birda_amd import _lib, modelfile as mf, synth

WARMUP, REPEATS, ROUNDS = 2, 5, 9
OPS = {mf.OP_CONV: "conv", mf.OP_DWCONV: "dwconv", mf.OP_PWCONV: "1x1", mf.OP_GAP: "global pool", mf.OP_DENSE: "dense", mf.OP_POOL: "pool",
       mf.OP_CONCAT: "concat", mf.OP_BNACT: "norm + activation"}


def without_prefix_reuse(m):
    """densenet_audio's records as a reader without prefix reuse makes them of the list-spelled file: every dense layer's Concat a
    left-to-right chain over the whole list of earlier features"""
    import copy
    out, new_of, parts = [], {0: 0}, {}
    for i, L in enumerate(m.layers):
        L = copy.copy(L)
        if L.op == mf.OP_CONCAT and L.res_tensor != mf.NO_TENSOR and L.reserved <= 1:
            lst = parts.get(L.in_tensor, [(L.in_tensor, L.cin)]) + [(L.res_tensor, L.cout - L.cin)]
            parts[i + 1] = lst
            (t, c) = lst[0]
            t = new_of[t]
            for tb, cb in lst[1:]:
                out.append(mf.Layer(mf.OP_CONCAT, mf.ACT_NONE, t, new_of[tb], c, c + cb, 1, 1, 1, 1, 0, 0, L.in_h, L.in_w, L.in_h, L.in_w, 0, 0, 0, 0))
                t, c = len(out), c + cb
            new_of[i + 1] = len(out)
            continue
        L.in_tensor = new_of[L.in_tensor]
        if L.res_tensor != mf.NO_TENSOR:
            L.res_tensor = new_of[L.res_tensor]
        out.append(L)
        new_of[i + 1] = len(out)
    m2 = copy.copy(m)
    m2.layers, m2.embedding_tensor = out, new_of[m.embedding_tensor]
    return m2


def main():
    import torch
    import bench                                            # (ROOT/bench.py: ClockSampler)
    from birda_amd.classifier import BirdClassifier
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bnact_layers.txt")
    prec = os.environ.get("PREC", "auto")
    lib = _lib.load()
    med = lambda v: float(np.median(np.asarray(v)))
    gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9 if ms > 0 else float("nan")

    # ---- (1) the model ----
    m = synth.build_model("densenet_audio", n_classes=6522)
    base = synth.synth_segments(16, m.sample_count, m.sample_rate)
    x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
    logits = torch.empty((N, m.n_classes), device="cuda")
    lines = []
    for label, model in (("prefix reuse (one two-source concat a dense layer)", m), ("no prefix reuse (every Concat a chain over its list)", without_prefix_reuse(m))):
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.bhm"); mf.write_model(path, model)
            clf = BirdClassifier(path, precision=prec)
        ctx = clf.create_batch_context(N)
        ctx.set_sub_slices(1)
        times = [[] for _ in model.layers]

        def fwd(keep):
            ctx.set_profiling(True)
            clf.forward_device(ctx, x.data_ptr(), N, logits.data_ptr())
            ctx.synchronize()
            if keep:
                for i, (ms, n) in enumerate(ctx.layer_ms()):
                    times[i].append(ms if n else 0.0)
            ctx.set_profiling(False)

        for _ in range(WARMUP):
            fwd(False)
        with bench.ClockSampler(0) as cs:
            for _ in range(REPEATS):
                fwd(True)
        clk = cs.summary()
        step = [float(np.sum([times[i][r] for i in range(len(model.layers))])) for r in range(REPEATS)]
        lines += [f"densenet_audio, {label}: {len(model.layers)} layers, {N} segments a forward, precision {prec}, {torch.cuda.get_device_name(0)}; {REPEATS} rounds "
                  f"after {WARMUP} warm-up forwards; shader clock during the rounds {clk['sclk_mhz']} MHz ({clk['sclk_mhz_min_max']}), {clk['power_w']} W, {clk['samples']} samples",
                  "op                  layers   ms a step (median)   share of the step   bytes moved GB/s"]
        for op, name in OPS.items():
            idx = [i for i, L in enumerate(model.layers) if L.op == op]
            if not idx:
                continue
            t = med([float(np.sum([times[i][r] for i in idx])) for r in range(REPEATS)])
            moved = sum(4 * N * (model.layers[i].in_h * model.layers[i].in_w + model.layers[i].out_h * model.layers[i].out_w) * model.layers[i].cout for i in idx)
            rate = f"{gbs(moved, t):8.1f}" if op in (mf.OP_CONCAT, mf.OP_BNACT) else "       -"
            lines.append(f"{name:<18s}  {len(idx):6d}   {t:10.3f}           {100 * t / med(step):6.2f} %          {rate}")
        lines += [f"all layers of a forward: {med(step):.3f} ms ({N / med(step) * 1e3:.0f} segments/s of layer time)", ""]
        if model is m:
            names = {clf.layer_kernel(i) for i, L in enumerate(m.layers) if L.op == mf.OP_BNACT}
            lines.insert(len(lines) - 1, f"norm + activation kernels: {sorted(names)}")
        ctx.close(); clf.close()
        torch.cuda.empty_cache()
    del x, logits

    # ---- (2) the kernel alone ----
    recs = sorted((L for L in m.layers if L.op == mf.OP_BNACT), key=lambda L: -(L.in_h * L.in_w * L.cout))
    shapes = []
    for L in recs:
        if (L.in_h, L.in_w, L.cout) not in shapes:
            shapes.append((L.in_h, L.in_w, L.cout))
        if len(shapes) == 2:
            break
    lines += [f"bnact_kernel alone on device buffers, {N} segments, {ROUNDS} rounds after {WARMUP}, the launches taking turns inside every round (copy = a device-to-device copy "
              "of the same bytes; scale_kernel = launch_scale, x times a [n][C] gate, on the same tensor)",
              "tensor             launch                 ms (median / min)   GB/s read + written   time / copy's   rate / copy's"]
    for h, w, c in shapes:
        n_pix = N * h * w
        X = torch.randn(n_pix * c, device="cuda")
        Y = torch.empty_like(X)
        sc, sh = torch.randn(c, device="cuda"), torch.randn(c, device="cuda")
        gate = torch.rand(N * c, device="cuda")
        name = C.create_string_buffer(128)

        def bn(act):
            def launch():
                rc = lib.bh_debug_bnact_on_device(0, C.c_void_p(X.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(sh.data_ptr()), act,
                                                  C.c_void_p(Y.data_ptr()), N, h * w, c, name, 128)
                assert rc == 0, lib.bh_last_error()
            return launch

        def scale():
            rc = lib.bh_debug_scale_on_device(0, C.c_void_p(X.data_ptr()), C.c_void_p(gate.data_ptr()), C.c_void_p(Y.data_ptr()), N, h * w, c, name, 128)
            assert rc == 0, lib.bh_last_error()
        runs = [("copy", lambda: Y.copy_(X)), ("bnact ReLU", bn(mf.ACT_RELU)), ("bnact swish", bn(mf.ACT_SWISH)), ("scale_kernel", scale)]
        t = {k: [] for k, _ in runs}
        kn = {}
        for r in range(WARMUP + ROUNDS):
            for k, fn in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); e1.synchronize()
                kn[k] = {"copy": "copy_", "bnact ReLU": name.value.decode() + ", ReLU", "bnact swish": name.value.decode() + ", swish"}.get(k, name.value.decode())
                if r >= WARMUP:
                    t[k].append(e0.elapsed_time(e1))
        for k, _ in runs:
            lines.append(f"{h:3d}x{w:<3d}x{c:<5d}     {kn[k]:<22s} {med(t[k]):8.4f} / {min(t[k]):8.4f}   {gbs(8 * X.numel(), med(t[k])):10.1f}          "
                         f"{med(t[k]) / med(t['copy']):6.2f}         {med(t['copy']) / med(t[k]):6.2f}")
        del X, Y, gate
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
