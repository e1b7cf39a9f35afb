"""Per-launch times of one forward (HIP events per layer; fused blocks are booked on their first layer): python tools/gpu_layer_times.py [kind] [n] [precision]
(kind: any model of synth.build_model -- perch_v2, cnn_pool, resnet18_audio, resnext_audio, ...)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from birda_amd import modelfile as mf, synth
from birda_amd.classifier import BirdClassifier
kind = sys.argv[1] if len(sys.argv) > 1 else "perch_v2"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
prec = sys.argv[3] if len(sys.argv) > 3 else "f16x3"
m = synth.build_model(kind)
path = f"/tmp/{kind}.bhm"; mf.write_model(path, m)
clf = BirdClassifier(path, precision=prec, low_latency=os.environ.get("LL") == "1")
ctx = clf.create_batch_context(N)
base = synth.synth_segments(16, m.sample_count, m.sample_rate)
x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
logits = torch.empty((N, m.n_classes), device="cuda"); idx = torch.empty((N, 5), dtype=torch.int32, device="cuda"); conf = torch.empty((N, 5), device="cuda")
for _ in range(3):
    clf.forward_device(ctx, x.data_ptr(), N, logits.data_ptr(), idx.data_ptr(), conf.data_ptr())
ctx.synchronize()
ctx.set_profiling(True)
for _ in range(5):
    clf.forward_device(ctx, x.data_ptr(), N, logits.data_ptr(), idx.data_ptr(), conf.data_ptr())
ctx.synchronize()
st = ctx.stage_ms(); ly = ctx.layer_ms()
print({k: round(v[0] / 5 * 1e3 / N, 3) for k, v in st.items()}, "us/segment")
names = {1: "conv", 2: "dw", 3: "pw", 4: "gap", 5: "dense", 6: "scale", 7: "pool", 8: "gconv", 10: "cat"}
for i, (ms, n) in enumerate(ly):
    if n:
        L = m.layers[i]
        line = f"layer {i:3d} {names[L.op]:5s} {L.cin:5d}->{L.cout:5d} {L.in_h}x{L.in_w} k{L.kh} s{L.sh}  {ms / 5 * 1e3:9.1f} us per {N}"
        if L.op in (mf.OP_CONV, mf.OP_PWCONV, mf.OP_DENSE) and L.reserved == mf.RES_ACT_AFTER:
            line += "  act after the residual add"
        if L.op == mf.OP_GCONV:  # near the HBM / MFMA ridge: the kernel it ran, the bytes it moves (input + output) and the rate
            nbytes = 4 * N * (L.in_h * L.in_w * L.cin + L.out_h * L.out_w * L.cout)
            line += f"  {L.reserved} groups of {L.cin // L.reserved}->{L.cout // L.reserved}  {clf.layer_kernel(i)}  {nbytes / 1e6:9.1f} MB  {nbytes / (ms / 5 * 1e-3) / 1e12:5.2f} TB/s"
        if L.op == mf.OP_POOL:   # HBM-bound: the bytes it moves (input + output) and the rate
            nbytes = 4 * N * L.cout * (L.in_h * L.in_w + L.out_h * L.out_w)
            line += f"  {('max', 'avg', 'avg_pad')[L.reserved]} {L.kh}x{L.kw}/{L.sh}x{L.sw}  {nbytes / 1e6:9.1f} MB  {nbytes / (ms / 5 * 1e-3) / 1e12:5.2f} TB/s"
        if L.op == mf.OP_CONCAT:  # HBM-bound: a copy of the output's bytes (res_tensor is the second input, not a residual)
            nbytes = 2 * 4 * N * L.out_h * L.out_w * L.cout
            line += f"  {L.cin}+{L.cout - L.cin} channels{' shuffle g=' + str(L.reserved) if L.reserved > 1 else ''}  {clf.layer_kernel(i)}  {nbytes / 1e6:9.1f} MB  {nbytes / (ms / 5 * 1e-3) / 1e12:5.2f} TB/s"
        print(line)
