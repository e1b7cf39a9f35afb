"""What the reduce layers (OP_REDUCE: max / mean / max + mean over one image axis or both) cost.

  python tools/reduce_layer_times.py [n] [table.txt]          (PREC=auto|f16x3|f32; run from anywhere: bench.py, whose ClockSampler
  samples the shader clock during the rounds, is imported from the repository root, the directory above this one)

Two parts, one process:
  (1) synth's `cnn14_audio` (the cnn_pool body under the PANNs head) at n segments a forward on the launch harness of
      tools/gpu_layer_times.py (forward_device, HIP events around every layer's launch: bh_batch_context_layer_ms), REPEATS rounds after
      two warm-up forwards: its two reduce layers' times, the step, and their share of it.
  (2) reduce_kernel alone on device buffers (bh_debug_reduce_on_device between two events on the null stream), REPEATS timed launches
      after two warm-up ones: the two layers of cnn14_audio and three larger shapes -- 64x500x64 over H, 64x500x64 over W, 8x32x512 over
      both -- in every mode the shape has, at n segments and at 16: the launcher's own form and the one it did not choose (1 or 8 lanes
      an output value), each against a device-to-device copy of the same INPUT bytes (torch's copy_, the same events, the same
      run), and the both-axes MAX against gap_kernel -- the global average pool's kernel -- on the same tensor.
Nothing is gated: the table states the ratios."""
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from birda_amd import _lib, modelfile as mf, synth

WARMUP, REPEATS = 2, 7
MODES = ("MAX", "MEAN", "MAXMEAN", "gap_kernel")
# name -> (in_h, in_w, out_h, out_w, c, kh, kw)
SHAPES = (("cnn14_audio freq mean   3x16x512 over H", (3, 16, 1, 16, 512, 3, 1), (1,)),
          ("cnn14_audio time pair   1x16x512 over W", (1, 16, 1, 1, 512, 1, 16), (2,)),
          ("64x500x64 over H", (64, 500, 1, 500, 64, 64, 1), (0, 1, 2)),
          ("64x500x64 over W", (64, 500, 64, 1, 64, 1, 500), (0, 1, 2)),
          ("8x32x512 over both", (8, 32, 1, 1, 512, 8, 32), (0, 2, 3)))


def main():
    import torch
    import bench                                            # (ROOT/bench.py: ClockSampler)
    from birda_amd.classifier import BirdClassifier
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    out_path = sys.argv[2] if len(sys.argv) > 2 else "reduce_layers.txt"
    prec = os.environ.get("PREC", "auto")
    lib = _lib.load()
    med = lambda v: float(np.median(np.asarray(v)))
    gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9 if ms > 0 else float("nan")

    # ---- (1) the model ----
    m = synth.build_model("cnn14_audio", n_classes=6522)
    base = synth.synth_segments(16, m.sample_count, m.sample_rate)
    x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
    logits = torch.empty((N, m.n_classes), device="cuda")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.bhm"); mf.write_model(path, m)
        clf = BirdClassifier(path, precision=prec)
    ctx = clf.create_batch_context(N)
    ctx.set_sub_slices(1)
    times = [[] for _ in m.layers]

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
    reduces = [i for i, L in enumerate(m.layers) if L.op == mf.OP_REDUCE]
    names = [clf.layer_kernel(i) for i in range(len(m.layers))]
    step = [float(np.sum([times[i][r] for i in range(len(m.layers))])) for r in range(REPEATS)]
    red_t = [float(np.sum([times[i][r] for i in reduces])) for r in range(REPEATS)]
    lines = [f"cnn14_audio (the cnn_pool body under the PANNs head), {N} segments a forward, precision {prec}, {torch.cuda.get_device_name(0)}; {REPEATS} rounds after "
             f"{WARMUP} warm-up forwards; shader clock during the rounds {clk['sclk_mhz']} MHz ({clk['sclk_mhz_min_max']}), {clk['power_w']} W, {clk['samples']} samples",
             "", "layer  window of image      C     kernel                        ms (median / min)   input GB/s"]
    for i in reduces:
        L = m.layers[i]
        lines.append(f"{i:5d}  {L.kh:3d}x{L.kw:<3d} of {L.in_h:3d}x{L.in_w:<3d}  {L.cout:5d}  {names[i]:<28s} {med(times[i]):8.4f} / {min(times[i]):8.4f}   "
                     f"{gbs(4 * N * L.in_h * L.in_w * L.cout, med(times[i])):8.1f}")
    lines += [f"all layers of a forward: {med(step):.3f} ms ({N / med(step) * 1e3:.0f} segments/s of layer time); the two reduce layers {med(red_t):.4f} ms, "
              f"{100 * med(red_t) / med(step):.2f} % of the step", ""]
    ctx.close(); clf.close()
    del x, logits

    # ---- (2) the kernel alone ----
    def timed(fn):
        for _ in range(WARMUP):
            fn()
        out = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    lines += ["reduce_kernel alone on device buffers (copy = a device-to-device copy of the same input bytes in the same run; chosen = the form every forward takes)",
              "shape                                    n      mode        kernel                        ms (median / min)   input GB/s   copy ms   kernel / copy   rate / copy's"]
    notes = []
    for label, geom, modes in SHAPES:
        in_h, in_w, out_h, out_w, c, kh, kw = geom
        for n in (N, 16):
            X = torch.randn(n * in_h * in_w * c, device="cuda")
            X2 = torch.empty_like(X)
            Y = torch.empty(n * out_h * out_w * c, device="cuda")
            shp = np.asarray(geom, np.int32)
            t_copy = med(timed(lambda: X2.copy_(X)))
            # (a copy reads and writes the bytes: its rate is 2 x bytes / time, the kernel's -- one read, a small write -- bytes / time)
            for mode in modes:
                own = None
                for split in (0, 1, 8):
                    if mode == 3 and split:
                        continue
                    name = C.create_string_buffer(128)

                    def launch():
                        rc = lib.bh_debug_reduce_on_device(0, C.c_void_p(X.data_ptr()), C.c_void_p(Y.data_ptr()), n, shp.ctypes.data_as(C.c_void_p), mode, split, name, 128)
                        assert rc == 0, lib.bh_last_error()
                    t = timed(launch)
                    kn = name.value.decode()
                    if split == 0:
                        own = kn
                    elif kn == own:
                        continue
                    tag = "chosen" if split == 0 else "forced"
                    lines.append(f"{label:<40s} {n:5d}  {MODES[mode]:<10s}  {kn:<28s}  {med(t):8.4f} / {min(t):8.4f}   {gbs(4 * X.numel(), med(t)):8.1f}   {t_copy:8.4f}   "
                                 f"{med(t) / t_copy:8.2f}        {t_copy / (2 * med(t)):6.2f}   {tag}")
            del X, X2, Y
            torch.cuda.empty_cache()
    text = "\n".join(lines + notes)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
