#!/usr/bin/env python3
"""Prints tests/golden/arena_plans.json for the catalogue of tests/test_arena_plan_gpu.py: per model / precision / n the arena's total
floats and the digest of bh_audit_arena_plan's answer (plan_digest).  Needs a device (a plan is asked of a context); writes nothing.

    python tools/record_arena_plans.py "<commit> (<subject>)" > tests/golden/arena_plans.json

--families records FAMILY_MODELS alone and keeps every other entry, and its commit, as the file has them."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NOTE = ("bh_audit_arena_plan per model / precision / n of tests/test_arena_plan_gpu.py: the arena's total floats and a SHA-256 over "
        "off | sz (little-endian uint64) | path (uint8). Recorded results, compared for equality by test_arena_plan_is_the_recorded_one; "
        "a change that means to change the plan records them again.")


def main():
    import test_arena_plan_gpu as T
    from birda_amd import modelfile as mf, synth
    from birda_amd.classifier import BirdClassifier
    args = [a for a in sys.argv[1:] if a != "--families"]
    families_only = len(args) != len(sys.argv) - 1
    if len(args) != 1:
        sys.exit(__doc__)
    with open(T.RECORDED_PLANS) as f:
        doc = json.load(f)
    with tempfile.TemporaryDirectory() as d:
        models = T.build_family_models(d)
        if not families_only:
            models.update(T.build_models(d))
            models["perch_v2"] = (os.path.join(d, "perch_v2.bhm"), synth.build_model("perch_v2"))
            mf.write_model(*models["perch_v2"])
            doc = {"note": NOTE, "plans": {}, "recorded_at": args[0]}
        doc["families_recorded_at"] = args[0]
        for name, (path, _) in sorted(models.items()):
            for precision in ("f32", "f16x3"):
                clf = BirdClassifier(path, None, precision=precision)
                ctx = clf.create_batch_context(16)
                try:
                    for n in T.BATCHES:
                        doc["plans"][f"{name}/{precision}/{n}"] = T.plan_digest(*T.arena_plan(clf, ctx, n))
                finally:
                    ctx.close()
                    clf.close()
    json.dump(doc, sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
