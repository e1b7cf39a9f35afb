"""The program of a `rocprofv3 --kernel-trace --stats` run over the pool layers of synth's `cnn_pool` model, and the copy they are
held against:  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/pool_layer_times.py [n] [copy.json]
Forwards of n segments (default 1 000), kept going until a shader-clock query started beside them has answered (so the clock is
the loaded chip's; the table reads the last ten forwards); then, in the same process, for every pool layer
a device-to-device copy that moves the layer's bytes (input + output: half of them copied, read once and written once), timed
with device events.  tools/pool_trace_table.py joins the trace and the JSON written here into the table of profiles/pool_layers.txt."""
import json, os, re, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from birda_amd import modelfile as mf, synth
from birda_amd.classifier import BirdClassifier

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
out_json = sys.argv[2] if len(sys.argv) > 2 else "pool_copy.json"
FORWARDS, COPIES = 10, 20
m = synth.build_model("cnn_pool")
path = "/tmp/cnn_pool.bhm"; mf.write_model(path, m)
clf = BirdClassifier(path, precision=os.environ.get("PREC", "auto"))
ctx = clf.create_batch_context(N)
base = synth.synth_segments(16, m.sample_count, m.sample_rate)
x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
logits = torch.empty((N, m.n_classes), device="cuda")
fwd = lambda: clf.forward_device(ctx, x.data_ptr(), N, logits.data_ptr())
for _ in range(3):
    fwd()
ctx.synchronize()
query = subprocess.Popen(["rocm-smi", "--showclocks"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
done = 0
while done < FORWARDS or (query.poll() is None and done < 50 * FORWARDS):      # the query answers while forwards run
    fwd(); ctx.synchronize(); done += 1
smi = query.communicate()[0]
sclk = sorted({int(v) for v in re.findall(r"sclk clock level: \d+: \((\d+)Mhz\)", smi)})
layers = []
for i, L in enumerate(m.layers):
    if L.op != mf.OP_POOL:
        continue
    nbytes = 4 * N * L.cout * (L.in_h * L.in_w + L.out_h * L.out_w)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    src.fill_(1)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    times = []
    for _ in range(COPIES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); dst.copy_(src); b.record(); b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    layers.append({"layer": i, "mode": ("max", "avg", "avg_pad")[L.reserved], "channels": L.cout, "in": [L.in_h, L.in_w], "out": [L.out_h, L.out_w],
                   "window": [L.kh, L.kw], "stride": [L.sh, L.sw], "bytes": nbytes, "copy_us_median": float(np.median(times)), "copy_us_min": float(min(times))})
    del src, dst
json.dump({"segments": N, "forwards": FORWARDS, "forwards_run": done, "precision": os.environ.get("PREC", "auto"), "sclk_mhz_during_forwards": sclk, "sclk_lines": [l.strip() for l in smi.splitlines() if "sclk" in l],
           "device": torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName, "layers": layers}, open(out_json, "w"), indent=1)
print(json.dumps({"sclk_mhz": sclk, "layers": len(layers)}))
