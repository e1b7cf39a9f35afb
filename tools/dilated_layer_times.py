"""Per-layer times of the dilated layers, from the library's own layer events (BatchInferenceContext.set_profiling / layer_ms: one event
pair a layer, every layer of these models one launch), with the shader clock sampled during the timed rounds as bench.py does.

  python tools/dilated_layer_times.py twin [n] [out.json]
      synth's dilated_resnet_audio against its UNDILATED TWIN -- the same records with dilation 1 and the pads of a 3x3 SAME layer,
      so every shape, K and MFMA is the same and only the gather's lines differ -- in ONE process: two warm-up forwards of each,
      then ROUNDS rounds, the order of the two swapped every round.  Prints, per dilated layer, the median time of both, their
      ratio, and the twin's own run-to-run spread (max - min over the median) to read the ratio against.
  python tools/dilated_layer_times.py layers [n] out.json [model] [library]
      one process, one model (default resnet18_audio), one build of the library (default: the one in place; else a file such as
      tools/ab/libbirda_hip_<tag>.so, the builds `tools/ab.sh libs` alternates): the per-layer times of ROUNDS forwards.  Run it with
      two builds taking turns and hand the files to `join`.
  python tools/dilated_layer_times.py join TAG=file.json TAG=file.json ...
      the table of those runs: per layer the median per tag, the ratio of the last tag to the first, and the first tag's own spread
      over its runs (max - min of its per-run medians over their median).
PREC (auto) selects the precision.  n: segments a forward (default 1 000)."""
import copy, json, os, statistics, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ROUNDS = 2, 8
PREC = os.environ.get("PREC", "auto")


def describe(L):
    return f"{L.kh}x{L.kw} s{L.sh} {L.in_h}x{L.in_w} {L.cin:>3}->{L.cout:<3}"


def undilated_twin(m):
    from birda_amd import synth
    t = copy.deepcopy(m)
    for L in t.layers:
        if (L.dil_h, L.dil_w) != (1, 1):
            assert (L.out_h, L.out_w) == (-(-L.in_h // L.sh), -(-L.in_w // L.sw))      # a SAME layer: the twin is the SAME layer of the plain kernel
            (_, L.pad_t), (_, L.pad_l) = synth._same_pad(L.in_h, L.kh, L.sh), synth._same_pad(L.in_w, L.kw, L.sw)
            L.dil_h = L.dil_w = 1
    return t


def time_models(models, n):
    """models: [(tag, Model)] -> (per tag a list over rounds of per-layer ms, per tag the kernels' names, the clock summary)"""
    import numpy as np, torch
    from bench import ClockSampler
    from birda_amd import modelfile as mf, synth
    from birda_amd.classifier import BirdClassifier
    m0 = models[0][1]
    base = synth.synth_segments(16, m0.sample_count, m0.sample_rate)
    x = torch.from_numpy(np.tile(base, (n // 16 + 1, 1))[:n]).cuda()
    logits = torch.empty((n, m0.n_classes), device="cuda")
    runs = []
    with tempfile.TemporaryDirectory() as d:
        for k, (tag, model) in enumerate(models):
            path = os.path.join(d, f"m{k}.bhm")
            mf.write_model(path, model)
            clf = BirdClassifier(path, precision=PREC)
            ctx = clf.create_batch_context(n)
            ctx.set_sub_slices(1)
            runs.append((clf, ctx))

    def fwd(k, timed):
        clf, ctx = runs[k]
        ctx.set_profiling(timed)
        clf.forward_device(ctx, x.data_ptr(), n, logits.data_ptr())
        ctx.synchronize()
        return [ms for ms, _ in ctx.layer_ms()] if timed else None

    for k in range(len(models)):
        for _ in range(WARMUP):
            fwd(k, False)
    times = [[] for _ in models]
    with ClockSampler(0) as clock:
        for r in range(ROUNDS):
            order = list(range(len(models)))
            for k in (order if r % 2 == 0 else order[::-1]):
                times[k].append(fwd(k, True))
    kernels = [[clf.layer_kernel(i) for i in range(len(model.layers))] for (clf, _), (_, model) in zip(runs, models)]
    device = torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName
    for clf, ctx in runs:
        ctx.close(); clf.close()
    return times, kernels, dict(clock.summary(), device=device)


def med(v):
    return statistics.median(v)


def spread(v):
    return (max(v) - min(v)) / med(v) if med(v) > 0 else 0.0


def cmd_twin(n, out_json):
    from birda_amd import synth
    m = synth.build_model("dilated_resnet_audio")
    twin = undilated_twin(m)
    times, kernels, clock = time_models([("dilated", m), ("twin", twin)], n)
    print(f"dilated_resnet_audio against its undilated twin, {n} segments a forward, precision {PREC}, {ROUNDS} rounds (order swapped every round)")
    print(f"{clock['device']}: shader clock median {clock['sclk_mhz']} MHz, min / max {clock['sclk_mhz_min_max']}, {clock['clock_source']}")
    khead = 'kernel ("": the f32 kernel)'
    print(f"{'layer':>5}  {'shape':<26} {'dil':>3}  {khead:<34} {'dilated ms':>10} {'twin ms':>9} {'ratio':>6} {'twin spread':>11}")
    rows = []
    for i, L in enumerate(m.layers):
        if (L.dil_h, L.dil_w) == (1, 1):
            continue
        a, b = [t[i] for t in times[0]], [t[i] for t in times[1]]
        rows.append({"layer": i, "shape": describe(L), "dil": L.dil_h, "kernel": kernels[0][i], "dilated_ms": med(a), "twin_ms": med(b), "ratio": med(a) / med(b), "twin_spread": spread(b)})
        print(f"{i:>5}  {describe(L):<26} {L.dil_h:>3}  {kernels[0][i]:<34} {med(a):>10.4f} {med(b):>9.4f} {med(a) / med(b):>6.3f} {100 * spread(b):>10.1f}%")
    ta, tb = [sum(t) for t in times[0]], [sum(t) for t in times[1]]
    print(f"all layers of a forward: dilated {med(ta):.3f} ms, twin {med(tb):.3f} ms, ratio {med(ta) / med(tb):.3f} (twin spread {100 * spread(tb):.1f}%)")
    json.dump({"segments": n, "precision": PREC, "rounds": ROUNDS, "clock": clock, "rows": rows}, open(out_json, "w"), indent=1)


def cmd_layers(n, out_json, kind, lib=None):
    from birda_amd import _lib, synth
    if lib:
        _lib.LIB_PATH = os.path.abspath(lib)
    m = synth.build_model(kind)
    times, kernels, clock = time_models([(kind, m)], n)
    json.dump({"model": kind, "segments": n, "precision": PREC, "rounds": ROUNDS, "clock": clock, "kernels": kernels[0],
               "shapes": [describe(L) for L in m.layers], "ops": [L.op for L in m.layers],
               "layer_ms": [med([t[i] for t in times[0]]) for i in range(len(m.layers))]}, open(out_json, "w"), indent=1)
    print(json.dumps({"model": kind, "layers": len(m.layers), "forward_ms": med([sum(t) for t in times[0]]), "sclk_mhz": clock["sclk_mhz"]}))


def cmd_join(args):
    runs = {}
    for a in args:
        tag, path = a.split("=", 1)
        runs.setdefault(tag, []).append(json.load(open(path)))
    tags = list(runs)
    first = runs[tags[0]][0]
    print(f"{first['model']}, {first['segments']} segments a forward, precision {first['precision']}: per-layer medians of {first['rounds']} forwards a run, "
          f"the libraries taking turns ({', '.join(f'{len(runs[t])} runs of {t}' for t in tags)})")
    for t in tags:
        print(f"  {t}: shader clock medians {[r['clock']['sclk_mhz'] for r in runs[t]]} MHz ({runs[t][0]['clock']['device']})")
    print(f"{'layer':>5}  {'shape':<26} {'kernel':<34} " + " ".join(f"{t + ' ms':>10}" for t in tags) + f" {tags[-1] + '/' + tags[0]:>9} {tags[0] + ' spread':>11}  inside")
    outside = 0
    for i, shape in enumerate(first["shapes"]):
        if first["ops"][i] not in (1, 2, 3):        # the convolutions
            continue
        per = {t: [r["layer_ms"][i] for r in runs[t]] for t in tags}
        ratio, sp = med(per[tags[-1]]) / med(per[tags[0]]), spread(per[tags[0]])
        inside = min(per[tags[0]]) <= med(per[tags[-1]]) <= max(per[tags[0]]) or abs(ratio - 1.0) <= sp
        outside += not inside
        print(f"{i:>5}  {shape:<26} {first['kernels'][i]:<34} " + " ".join(f"{med(per[t]):>10.4f}" for t in tags) + f" {ratio:>9.3f} {100 * sp:>10.1f}%  {'yes' if inside else 'NO'}")
    tot = {t: [sum(r["layer_ms"]) for r in runs[t]] for t in tags}
    print("all layers of a forward: " + ", ".join(f"{t} {med(tot[t]):.3f} ms" for t in tags) + f"; ratio {med(tot[tags[-1]]) / med(tot[tags[0]]):.3f}, {tags[0]} spread {100 * spread(tot[tags[0]]):.1f}%; "
          f"{outside} layers outside {tags[0]}'s own spread")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "twin"
    if mode == "twin":
        cmd_twin(int(sys.argv[2]) if len(sys.argv) > 2 else 1000, sys.argv[3] if len(sys.argv) > 3 else "dilated_twin.json")
    elif mode == "layers":
        cmd_layers(int(sys.argv[2]) if len(sys.argv) > 2 else 1000, sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else "resnet18_audio",
                   sys.argv[5] if len(sys.argv) > 5 else None)
    elif mode == "join":
        cmd_join(sys.argv[2:])
    else:
        sys.exit(__doc__)
