"""rocprofv3 kernel trace of tools/resnet_layer_times.py + its JSON -> the table of profiles/resnet_layers.txt:
python tools/resnet_trace_table.py TRACE_DIR layers.json.  Per pair of models ("relu", "relu6") and per layer whose activation
follows the residual add: its kernel and time (median / min over the repeats), the same layer of the twin model (flags cleared: the
activation before the add), the ratio of the medians, and the twin's run-to-run spread (max - min over the repeats, of its median)
-- the yardstick the ratio is read against; a layer whose ratio differs from 1 by more than that spread is marked."""
import csv, glob, json, re, statistics as st, sys
root, J = sys.argv[1], json.load(open(sys.argv[2]))
LAYER_KERNELS = re.compile(r"conv_direct_kernel|pool_kernel|conv_gemm_kernel|conv_gemm16_kernel|gap_kernel|pw_gemm")
rows = sorted((r for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True) for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
rows = [r for r in rows if LAYER_KERNELS.search(r["Kernel_Name"])]
nl, W, R, order = len(J["layers"]), J["warmup"], J["repeats"], J["order"]
assert len(rows) == nl * len(order), (len(rows), nl, len(order))          # every layer is one launch
timed = {k: [] for k in range(len(J["models"]))}                          # model -> its timed forwards
for f, k in enumerate(order):
    if f >= W * len(J["models"]):
        timed[k].append(rows[f * nl:(f + 1) * nl])
us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
short = lambda r: re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void bh::", "")
print(f"resnet18_audio, {J['segments']} segments a launch, precision {J['precision']}, {J['device']}; {R} forwards of each model, a pair's order swapped every round, rocprofv3 --kernel-trace")
print("`after`: act(conv + b + R), Layer.reserved = RES_ACT_AFTER; `twin`: the same layer with the flag cleared, act(conv + b) + R")
for pair in range(len(J["models"]) // 2):
    ka, kt = 2 * pair, 2 * pair + 1
    print(f"\n== {J['models'][ka].split('/')[0]}")
    print("layer  conv        Cin -> Cout  image       after: kernel, us (median / min)                          twin: kernel, us (median / min)                     after / twin   twin spread")
    worst = 0.0
    for i in J["flagged"]:
        L = J["layers"][i]
        a, t = [f[i] for f in timed[ka]], [f[i] for f in timed[kt]]
        na, nt = {short(r) for r in a}, {short(r) for r in t}
        assert len(na) == 1 and len(nt) == 1, (na, nt)
        # (a split-f16 launch: the name its launcher reports, bh_debug_layer_kernel -- the trace prints the newest instantiations mangled)
        na, nt = L["split_f16"][ka] or na.pop(), L["split_f16"][kt] or nt.pop()
        ua, ut = [us(r) for r in a], [us(r) for r in t]
        spread = (max(ut) - min(ut)) / st.median(ut)
        ratio = st.median(ua) / st.median(ut)
        worst = max(worst, spread)
        print(f"{i:5d}  {L['k'][0]}x{L['k'][1]}/{L['stride'][0]}      {L['cin']:4d} -> {L['cout']:4d}  {L['out'][0]:3d}x{L['out'][1]:<3d}    "
              f"{na[:46]:46s} {st.median(ua):9.1f} / {min(ua):9.1f}   {nt[:40]:40s} {st.median(ut):9.1f} / {min(ut):9.1f}   {ratio:6.3f}   {100 * spread:5.1f} %"
              + ("" if abs(ratio - 1.0) <= spread else "   outside the spread"))
    tot = lambda fs: [sum(us(r) for r in f) for f in fs]
    ta, tt = tot(timed[ka]), tot(timed[kt])
    print(f"all {nl} layer kernels of a forward: after {st.median(ta) / 1e3:.2f} ms, twin {st.median(tt) / 1e3:.2f} ms (median of {R}); "
          f"twin spread {100 * (max(tt) - min(tt)) / st.median(tt):.1f} %; largest per-layer twin spread {100 * worst:.1f} %")
