"""A refused create is free: bh_classifier, bh_batch_context and bh_custom_classifier release what they hold in their destructors,
and create keeps the new object in a unique_ptr until its last phase is through (birda_amd/csrc/api_create.hip, api_custom.hip).

The model here is one model.hpp's loader accepts -- it checks a residual's SHAPE only -- and bh_classifier_create refuses after the
whole blob, the front-end operators, every fused block's weights and every layer's re-laid weights are on the device: a residual on a
depthwise layer (api_create.hip prepare_layers, the last check of the last device phase).

Free device memory is read through HIP's memory-info call.  The conditions assume that nothing else allocates on the device during
the few seconds the module runs.
"""
import numpy as np
import pytest

from birda_amd import modelfile as mf, synth

pytestmark = pytest.mark.gpu

N_REFUSALS = 16
MIN_BLOB_BYTES = 8 << 20
BH_ERR_UNSUPPORTED = -6


def free_bytes() -> int:
    import torch
    return int(torch.cuda.mem_get_info(0)[0])


def write_models(d):
    """(good model path, refused model path, index of the layer that is refused, blob bytes): the short-segment B0 stack, and the same
    file with its first stride-1 depthwise layer given its own input -- a tensor of its output's shape -- as a residual"""
    m = synth.build_model("mini_b0")
    good = str(d / "good.bhm")
    mf.write_model(good, m)
    i = next(i for i, L in enumerate(m.layers) if L.op == mf.OP_DWCONV and L.sh == 1 and L.sw == 1)
    m.layers[i].res_tensor = m.layers[i].in_tensor
    refused = str(d / "refused.bhm")
    mf.write_model(refused, m)
    return good, refused, i, int(m.blob.nbytes)


def write_custom(d):
    """(refused custom classifier path, blob bytes): a hidden width that is no multiple of 4, which cc_build (api_custom.hip) meets at
    the SECOND layer -- after the blob and the first layer's padded rows are on the device"""
    cm = synth.build_custom_classifier(input_dim=1024, n_classes=1000, hidden=(2050,))
    path = str(d / "refused.bhc")
    mf.write_custom_classifier(path, cm)
    return path, sum(int(L.w.nbytes + L.b.nbytes) for L in cm.layers)


def refusal_drop(create, n=N_REFUSALS):
    """free memory before - after n calls of create(), each of which must raise; the errors raised"""
    from birda_amd._lib import BirdaHipError
    before = free_bytes()
    errors = []
    for _ in range(n):
        with pytest.raises(BirdaHipError) as e:
            create()
        errors.append(e.value)
    return before - free_bytes(), errors


def round_trip(path, segs, readings=None):
    """create, context, forward of the segments, destroy; the logits.  readings: free memory after every step"""
    from birda_amd.classifier import BirdClassifier
    note = (lambda: readings.append(free_bytes())) if readings is not None else (lambda: None)
    note()
    clf = BirdClassifier(path, None, precision="auto")
    note()
    ctx = clf.create_batch_context(4)
    note()
    logits = clf.predict_logits(ctx, segs)
    note()
    ctx.close()      # (parked with its classifier, which frees it)
    clf.close()
    note()
    return logits


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    good, refused, layer, blob = write_models(tmp_path_factory.mktemp("ownership"))
    assert blob >= MIN_BLOB_BYTES, blob      # (far above any allocation granule)
    m = mf.read_model(good)
    round_trip(good, synth.synth_segments(1, m.sample_count, m.sample_rate))   # one-time runtime allocations are paid here
    return good, refused, layer, blob


def test_refused_classifier_create_leaves_nothing_on_the_device(models):
    """16 refusals of a model whose blob is 12 184 968 bytes: free memory drops by less than ONE blob.
    (Before the destructors, measured with this test on the MI355X: a drop of 471 859 200 bytes, 38.7 blobs -- every refusal left
    the 16 stream-set streams, the blob, the operators, the fused blocks' and the layers' re-laid weights behind.  With them: 0.)"""
    from birda_amd.classifier import BirdClassifier
    _, refused, layer, blob = models
    drop, errors = refusal_drop(lambda: BirdClassifier(refused, None, precision="auto"))
    print(f"\n{N_REFUSALS} refused creates: free memory dropped by {drop} bytes = {drop / blob:.2f} blobs of {blob} bytes")
    for e in errors:
        assert e.code == BH_ERR_UNSUPPORTED and f"layer {layer}:" in str(e) and "residual on a depthwise layer" in str(e), str(e)
    assert drop < blob, (drop, blob)


def test_refused_custom_classifier_create_leaves_nothing_on_the_device(tmp_path):
    """The same for bh_custom_classifier_create, whose one refusal after its blob upload is a hidden width that is no multiple of 4.
    (This create already held its object in a unique_ptr whose deleter was the destroy function: measured before the destructors,
    the drop was 0 bytes as well.  What changed is where the release code lives.)"""
    from birda_amd.classifier import CustomClassifier
    path, blob = write_custom(tmp_path)
    assert blob >= MIN_BLOB_BYTES, blob
    with pytest.raises(Exception):
        CustomClassifier(path)            # (the runtime's one-time allocations for this path, if any)
    drop, errors = refusal_drop(lambda: CustomClassifier(path))
    print(f"\n{N_REFUSALS} refused custom creates: free memory dropped by {drop} bytes = {drop / blob:.2f} blobs of {blob} bytes")
    for e in errors:
        assert e.code == BH_ERR_UNSUPPORTED and "hidden width 2050 not a multiple of 4" in str(e), str(e)
    assert drop < blob, (drop, blob)


def test_a_good_classifier_after_refusals_works_and_gives_its_memory_back(models):
    """After refusals: create, context, forward of 3 segments, destroy -- twice.  The logits of the two rounds are bit-identical, and
    free memory after each round is what it was before the first, within one allocation granule: the smallest step free memory
    took between two readings of the first round (free memory moves in whole granules).
    (One such round goes before the two that count, as one successful create goes before the refusals: the HIP runtime keeps what
    the first forward of these kernels on a hardware queue makes it allocate -- measured, 142 606 336 bytes that stay after
    everything of the library's is destroyed, before and after the destructors alike -- and the streams of the next classifier
    land on the same queues.)"""
    from birda_amd.classifier import BirdClassifier
    good, refused, _, _ = models
    m = mf.read_model(good)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate)
    refusal_drop(lambda: BirdClassifier(refused, None, precision="auto"), 2)
    round_trip(good, segs)
    readings = []
    first = round_trip(good, segs, readings)
    steps = [abs(a - b) for a, b in zip(readings, readings[1:]) if a != b]
    assert steps, readings               # (a classifier of 16 MB of weights moved no reading: the memory-info call tells nothing)
    granule = min(steps)
    second = round_trip(good, segs)
    after = free_bytes()
    print(f"\nreadings of round 1 {readings}, granule {granule}, after round 2 {after}")
    assert np.isfinite(first).all() and first.tobytes() == second.tobytes()
    assert abs(readings[-1] - readings[0]) <= granule, (readings, granule)
    assert abs(after - readings[0]) <= granule, (after, readings, granule)
