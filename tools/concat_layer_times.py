"""The concat layers of synth's `shufflenet_audio` and of one 4-way Inception module beside a device-to-device copy of the same bytes:
python tools/concat_layer_times.py [n] [--dry]
Per-layer device events of forwards of n segments (default 1 000; bh_batch_context_layer_ms), and in the same process, between the
forwards, a device-to-device copy that moves each layer's bytes (what it reads + what it writes: half of them copied, read once and
written once), timed with device events.  Four alternations; every figure of every alternation is printed, so the copy's own
run-to-run spread stands beside the kernel's.  --dry: the models and the bytes only (no device).  profiles/concat_layers.txt is this
program's output."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from birda_amd import modelfile as mf, synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 1000
DRY = "--dry" in sys.argv
ALTERNATIONS, FORWARDS, COPIES = 4, 3, 5


def inception_model():
    """the v2.4 front-end, a 3x3 stride-2 stem to 32 channels, MaxPool 2x2 stride 2 (a 24 x 128 image), one 4-branch Inception module
    -- 1x1, 1x1 -> 3x3, 1x1 -> 1x7 -> 7x1, avg-pool -> 1x1; 32 channels each, a 4-way Concat = a chain of three records --, a 1x1
    head, the global pool and a dense layer"""
    b = synth._Builder(np.random.default_rng(7))
    sr, n = 48000, 144000
    branches = [mf.Branch(2048, 278, 96, 511, 0.0, 3000.0, 1.23), mf.Branch(1024, 280, 96, 511, 500.0, 15000.0, 1.23)]
    for br in branches:
        br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
        br.out_scale, br.out_shift = 0.8, -0.4
    A = mf.ACT_RELU
    x, h, w = b.conv(0, 96, 511, 2, 32, 3, 2, A, in_layout=1)
    x, h, w = b.pool(x, h, w, 32, 2, 2, 2, 2, mf.POOL_MAX, "valid")
    b1 = b.pwconv(x, h, w, 32, 32, A)
    b3, _, _ = b.conv(b.pwconv(x, h, w, 32, 16, A), h, w, 16, 32, 3, 1, A)
    b7, _, _ = b.conv(b.pwconv(x, h, w, 32, 16, A), h, w, 16, 16, 1, 1, A, kw=7)
    b7, _, _ = b.conv(b7, h, w, 16, 32, 7, 1, A, kw=1)
    bp, _, _ = b.pool(x, h, w, 32, 3, 3, 1, 1, mf.POOL_AVG, "same")
    bp = b.pwconv(bp, h, w, 32, 32, A)
    t, c = b.concat([(b1, 0, 32), (b3, 0, 32), (b7, 0, 32), (bp, 0, 32)], h, w)
    t = b.pwconv(t, h, w, c, 256, A)
    t = emb = b.gap(t, h, w, 256)
    b.dense(t, 256, 50, gain=1.5)
    return synth._finish(b, branches, sr, n, 50, 256, emb, mf.OUT_SIGMOID)


def concat_bytes(L):
    return 2 * 4 * N * L.out_h * L.out_w * L.cout          # every output element read once and written once


def describe(m, L):
    """(of a chain step: its last record)"""
    src = f"{L.cin} of {m.layers[L.in_tensor - 1].cout} from {L.w_off}"
    if L.res_tensor != mf.NO_TENSOR:
        src += f" + {L.cout - L.cin} of {m.layers[L.res_tensor - 1].cout} from {L.b_off}"
    return f"{'shuffle g=' + str(L.reserved) if L.reserved > 1 else 'plain':11s} {src:34s} {L.out_h:3d}x{L.out_w:<3d} x {L.cout:4d}"


def measure(name, m, by_record=False):
    """by_record: in a BIRDA_HIP_KEEP_TENSORS context, whose schedule runs a chain of concat records launch by launch"""
    concats = [i for i, L in enumerate(m.layers) if L.op == mf.OP_CONCAT]
    print(f"== {name}: {len(concats)} concat records, {N} segments a launch" + (", record by record (a keep-tensors context)" if by_record else ""))
    if DRY:
        for i in concats:
            print(f"layer {i:3d}  {describe(m, m.layers[i])}  {concat_bytes(m.layers[i]) / 1e6:9.1f} MB")
        return
    import torch
    from birda_amd.classifier import BirdClassifier
    path = f"/tmp/{name}.bhm"
    mf.write_model(path, m)
    clf = BirdClassifier(path, precision="auto")
    if by_record:
        os.environ["BIRDA_HIP_KEEP_TENSORS"] = "1"
    ctx = clf.create_batch_context(N)
    os.environ.pop("BIRDA_HIP_KEEP_TENSORS", None)
    base = synth.synth_segments(16, m.sample_count, m.sample_rate)
    x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
    logits = torch.empty((N, m.n_classes), device="cuda")
    fwd = lambda: clf.forward_device(ctx, x.data_ptr(), N, logits.data_ptr())
    for _ in range(3):
        fwd()
    ctx.synchronize()
    # a chain of records that runs as one launch is booked on its first record: the step moves the LAST record's bytes
    ctx.set_profiling(True); fwd(); ctx.synchronize(); launched = ctx.layer_ms(); ctx.set_profiling(False)
    steps, last_of = [i for i in concats if launched[i][1]], {}
    for i in steps:
        k = i
        while k + 1 in concats and not launched[k + 1][1]:
            k += 1
        last_of[i] = k
    step_bytes = lambda i: concat_bytes(m.layers[last_of[i]])
    concats = steps
    sizes = sorted({step_bytes(i) for i in concats})
    bufs = {}
    for nb in sizes:
        src = torch.empty(nb // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        src.fill_(1)
        for _ in range(3):
            dst.copy_(src)
        bufs[nb] = (src, dst)
    torch.cuda.synchronize()
    kernel_us = {i: [] for i in concats}
    copy_us = {nb: [] for nb in sizes}
    for _ in range(ALTERNATIONS):
        ctx.set_profiling(True)
        for _ in range(FORWARDS):
            fwd()
        ctx.synchronize()
        ly = ctx.layer_ms()
        ctx.set_profiling(False)
        for i in concats:
            assert ly[i][1] == FORWARDS, (i, ly[i])
            kernel_us[i].append(ly[i][0] / FORWARDS * 1e3)
        for nb in sizes:
            src, dst = bufs[nb]
            times = []
            for _ in range(COPIES):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); dst.copy_(src); b.record(); b.synchronize()
                times.append(a.elapsed_time(b) * 1e3)
            copy_us[nb].append(float(np.median(times)))
    fmt = lambda v: " ".join(f"{t:8.1f}" for t in v)
    print("layer  kind        sources                            image x C      MB moved   kernel us, one per alternation        TB/s (median)   "
          "copy us, one per alternation         TB/s (slowest .. fastest)   kernel rate / slowest copy")
    plain, shuffled = [], []
    for i in concats:
        L = m.layers[last_of[i]]
        nb = step_bytes(i)
        k, c = kernel_us[i], copy_us[nb]
        rate = nb / (float(np.median(k)) * 1e-6) / 1e12
        slow, fast = nb / (max(c) * 1e-6) / 1e12, nb / (min(c) * 1e-6) / 1e12
        (shuffled if L.reserved > 1 else plain).append(rate / slow)
        print(f"{i:5d}  {describe(m, L)}  {nb / 1e6:9.1f}   {fmt(k)}   {rate:6.2f}          {fmt(c)}   {slow:5.2f} .. {fast:5.2f}              {rate / slow:5.2f}   {clf.layer_kernel(i)}" + (f"   records {i} .. {last_of[i]} in one launch, {last_of[i] - i + 2} leaves" if last_of[i] != i else ""))
    for what, v in (("plain", plain), ("shuffle", shuffled)):
        if v:
            print(f"{what}: kernel rate / slowest copy of the same bytes over {len(v)} layers: min {min(v):.2f}, median {float(np.median(v)):.2f}, max {max(v):.2f}")
    total = sum(float(np.median(kernel_us[i])) for i in concats)
    print(f"all concat launches: {total:.1f} us of a forward of {N} segments, {sum(step_bytes(i) for i in concats) / 1e6:.1f} MB moved")
    ctx.close(); clf.close()


if not DRY:
    import torch
    print(f"{torch.cuda.get_device_name(0)}; {ALTERNATIONS} alternations of {FORWARDS} profiled forwards (device events per layer) and {COPIES} copies per size (median)")
measure("shufflenet_audio", synth.build_model("shufflenet_audio"))
m = inception_model()
measure("inception_module", m)
measure("inception_module", m, by_record=True)
chain = [L for L in m.layers if L.op == mf.OP_CONCAT]
print(f"the 4-way Concat record by record moves {sum(concat_bytes(L) for L in chain) / 1e6:.1f} MB in {len(chain)} launches; gathered in one launch it moves "
      f"{concat_bytes(chain[-1]) / 1e6:.1f} MB")
