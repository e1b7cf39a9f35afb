"""rocprofv3 kernel trace of tools/pool_layer_times.py + its JSON -> the table of profiles/pool_layers.txt:
python tools/pool_trace_table.py TRACE_DIR copy.json.  Per pool layer: kernel time (median / min over the timed forwards' launches,
in dispatch order: the k-th pool launch of a forward is the k-th pool layer), bytes moved (input + output), TB/s, and the
device-to-device copy moving the same bytes in the same process."""
import csv, glob, json, re, statistics as st, sys
root, J = sys.argv[1], json.load(open(sys.argv[2]))
rows = sorted((r for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True) for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
pools = [r for r in rows if "pool_kernel" in r["Kernel_Name"]]
nl = len(J["layers"])
assert pools and len(pools) % nl == 0, (len(pools), nl)
pools = pools[-nl * J["forwards"]:]           # the timed forwards (the warm-up's launches run first)
print(f"cnn_pool, {J['segments']} segments a launch, precision {J['precision']}, {J['device']}; shader clock while the forwards ran: "
      f"{J['sclk_mhz_during_forwards']} MHz; {J['forwards']} forwards, rocprofv3 --kernel-trace")
print("layer  pool                 image -> image x C          MB moved   kernel us (median / min)   TB/s    copy of the same bytes us (median / min)   TB/s   pool / copy")
for k, L in enumerate(J["layers"]):
    mine = pools[k::nl]
    names = {re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")).replace("void bh::", "") for r in mine}
    assert len(names) == 1, names
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine]
    med, mn, B = st.median(us), min(us), L["bytes"]
    print(f"{L['layer']:5d}  {L['mode']:3s} {L['window'][0]}x{L['window'][1]}/{L['stride'][0]}x{L['stride'][1]} {names.pop():18s} "
          f"{L['in'][0]:3d}x{L['in'][1]:<3d} -> {L['out'][0]:3d}x{L['out'][1]:<3d} x {L['channels']:3d}   {B / 1e6:8.1f}   {med:9.1f} / {mn:9.1f}   {B / med / 1e6:5.2f}   "
          f"{L['copy_us_median']:9.1f} / {L['copy_us_min']:9.1f}   {B / L['copy_us_median'] / 1e6:5.2f}   {L['copy_us_median'] / med:5.2f}")
