"""The program of a `rocprofv3 --kernel-trace --stats` run over synth's `resnet18_audio` and its twin with the position flags
cleared (the same shapes with the activation BEFORE the residual add: act(conv + b) + R, what the library ran before the flag):
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/resnet_layer_times.py [n] [layers.json]
Two pairs of models.  "relu": the model as synth builds it.  Its twin's layers above 64 channels run ANOTHER kernel (ReLU before
the add is not an activation of the split-f16 epilogues: the f32 conv_gemm_kernel), so that pair prices the epilogue only on the
f32 kernel.  "relu6": the same weights with every ReLU read as ReLU6, which both positions have on the split-f16 epilogues -- the
like-for-like pair for conv_gemm16_kernel<3,RELU6,AFTER> against conv_gemm16_kernel<3,RELU6>.
Forwards of n segments (default 1 000) in one launch each; after two warm-up forwards of every model, REPEATS rounds over the four
models, the order of a pair's two models swapped every round (neither always runs behind the other).  Every layer of these models
is one launch, so the k-th layer kernel of a forward in the trace is layer k; tools/resnet_trace_table.py joins the trace and the
JSON written here into the table of profiles/resnet_layers.txt."""
import copy, json, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from birda_amd import modelfile as mf, synth
from birda_amd.classifier import BirdClassifier

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
out_json = sys.argv[2] if len(sys.argv) > 2 else "resnet_layers.json"
WARMUP, REPEATS = 2, 8
prec = os.environ.get("PREC", "auto")
m = synth.build_model("resnet18_audio")
flagged = [i for i, L in enumerate(m.layers) if L.op in (mf.OP_CONV, mf.OP_PWCONV, mf.OP_DENSE) and L.reserved == mf.RES_ACT_AFTER]


def variant(relu6, clear):
    v = copy.deepcopy(m)
    for i, L in enumerate(v.layers):
        if relu6 and L.act == mf.ACT_RELU:
            L.act = mf.ACT_RELU6
        if clear and i in flagged:
            L.reserved = 0
    return v


models = [("relu/after", variant(False, False)), ("relu/twin", variant(False, True)), ("relu6/after", variant(True, False)), ("relu6/twin", variant(True, True))]
base = synth.synth_segments(16, m.sample_count, m.sample_rate)
x = torch.from_numpy(np.tile(base, (N // 16 + 1, 1))[:N]).cuda()
logits = torch.empty((N, m.n_classes), device="cuda")
runs = []
with tempfile.TemporaryDirectory() as d:
    for k, (tag, model) in enumerate(models):
        path = os.path.join(d, f"resnet18_audio_{k}.bhm"); mf.write_model(path, model)
        clf = BirdClassifier(path, precision=prec)
        ctx = clf.create_batch_context(N)
        ctx.set_sub_slices(1)
        runs.append((clf, ctx))
fwd = lambda k: (runs[k][0].forward_device(runs[k][1], x.data_ptr(), N, logits.data_ptr()), runs[k][1].synchronize())
order = []                                   # the model of every forward, in launch order
for k in range(len(models)):
    for _ in range(WARMUP):
        fwd(k); order.append(k)
for r in range(REPEATS):
    for k in ((0, 1, 2, 3) if r % 2 == 0 else (1, 0, 3, 2)):
        fwd(k); order.append(k)
kernels = [[clf.layer_kernel(i) for i in range(len(m.layers))] for clf, _ in runs]
json.dump({"segments": N, "warmup": WARMUP, "repeats": REPEATS, "precision": prec, "flagged": flagged, "models": [t for t, _ in models], "order": order,
           "device": torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName,
           "layers": [{"layer": i, "op": L.op, "cin": L.cin, "cout": L.cout, "k": [L.kh, L.kw], "stride": [L.sh, L.sw], "in": [L.in_h, L.in_w],
                       "out": [L.out_h, L.out_w], "residual": L.res_tensor != mf.NO_TENSOR, "split_f16": [kernels[k][i] for k in range(len(models))]}
                      for i, L in enumerate(m.layers)]}, open(out_json, "w"), indent=1)
print(json.dumps({"layers": len(m.layers), "flagged": flagged, "forwards": len(order)}))
