"""The frame stream (irm_amd/stream.py), the part that needs no GPU: every argument error before any GPU call, the
order in which errors surface, the grouping as a pure function, and the host-side builder of the cached noise field."""
import numpy as np
import pytest
import torch

from irm_amd import _hip, deblurganv2, harness, stream, utils

CPU = torch.device("cpu")


class Never(torch.nn.Module):
    def forward(self, t):
        raise AssertionError("the model must not run")


def upscaling():
    sr = Never()
    sr.upscale = 2
    return sr


U8 = np.zeros((8, 12, 3), np.uint8)
Y, UV, U = np.zeros((4, 6), np.uint8), np.zeros((2, 3, 2), np.uint8), np.zeros((2, 3), np.uint8)


def run(model, frames, **kw):
    return list(utils.run_model_inference_stream(model, frames, CPU, patch_size=32, **kw))


def test_utils_reexports_the_stream():
    assert utils.run_model_inference_stream is stream.run_model_inference_stream
    assert utils.group_frames is stream.group_frames
    assert stream.run_model_inference_stream.__module__ == stream.__name__


@pytest.mark.parametrize("k", [0, -1, 2.5, "3", None, True])
def test_bad_frames_per_step(k):
    with pytest.raises(ValueError, match="frames_per_step"):
        run(Never(), [U8], frames_per_step=k)
    with pytest.raises(ValueError, match="frames_per_step"):
        stream.group_frames([1, 1], k)


def test_argument_errors_before_any_gpu_call():
    m = Never()
    with pytest.raises(ValueError, match="out must be"):
        run(m, [U8], out="uint4")
    with pytest.raises(ValueError, match="model"):
        run(None, [U8])
    # the value kinds the batch call refuses: an integer result of another type, unit_range or not
    for kw in (dict(out="uint16", unit_range=True), dict(out="uint16"), dict(out="uint8", unit_range=True)):
        frame = np.zeros((8, 12, 3), np.uint16) if kw["out"] == "uint8" else U8
        with pytest.raises(ValueError, match="integer result"):
            run(m, [frame], **kw)
        with pytest.raises(ValueError, match="integer result"):
            utils.tiled_forward_device_batch(m, [utils.to_device(frame, CPU)], 32, 8, False, **kw)
    with pytest.raises(ValueError, match="integer result"):
        run(m, [U8.astype(np.float32)], out="uint8")              # a float32 frame needs unit_range=True for it
    # DeblurGANv2: raw integer values, an integer result, no YUV
    dg = deblurganv2.FPNMobileNet()
    with pytest.raises(ValueError, match="deblurganv2"):
        run(dg, [U8.astype(np.float32)])
    with pytest.raises(ValueError, match="deblurganv2"):
        run(dg, [U8], out="float32")
    with pytest.raises(ValueError, match="DeblurGANv2"):
        run(dg, [(Y, UV)], fmt="nv12")
    with pytest.raises(ValueError, match="DeblurGANv2"):
        run(dg, [np.zeros((8, 12, 3), np.uint16)])
    # up-scaling models
    with pytest.raises(ValueError, match="luma_only"):
        run(upscaling(), [(Y, UV)], fmt="nv12", luma_only=True)
    with pytest.raises(ValueError, match="need_degradation"):
        run(upscaling(), [U8], need_degradation=True, noise_level=15)
    with pytest.raises(ValueError, match="need_degradation"):
        run(upscaling(), [(Y, UV)], fmt="nv12", need_degradation=True, noise_level=15)
    # frames that are not [H, W, C]
    for bad in (np.zeros((8, 12), np.uint8), np.zeros((1, 8, 12, 3), np.uint8), np.zeros((8, 12, 3), np.float64),
                np.zeros((8, 12, 3), np.int32), [[1, 2], [3, 4]], None, torch.zeros(8, 12, 3, dtype=torch.uint8),
                np.zeros((0, 12, 3), np.uint8)):
        with pytest.raises(ValueError, match="frame"):
            run(m, [bad])
    # YUV: names, planes, and the arguments that describe [H, W, C] frames only
    for kw in (dict(fmt="yv12"), dict(fmt="nv12", matrix="bt2020"), dict(fmt="nv12", siting="top")):
        with pytest.raises(ValueError, match="must be"):
            run(m, [(Y, UV)], **kw)
    for planes, fmt in (((Y, U), "nv12"), ((Y, UV), "i420"), ((Y, U, U), "nv12"), ((Y, UV), "p010"), (Y, "nv12"),
                        ((Y[:, :, None], UV), "nv12"), ((Y.astype(np.float32), UV.astype(np.float32)), "nv12"),
                        ((np.zeros((3, 6), np.uint8), np.zeros((1, 3, 2), np.uint8)), "nv12"),
                        ((Y, U, np.zeros((2, 4), np.uint8)), "i420")):
        with pytest.raises(ValueError):
            run(m, [planes], fmt=fmt)
        with pytest.raises(ValueError):
            utils.run_model_inference_yuv(m, planes, CPU, fmt=fmt, patch_size=32)
    with pytest.raises(ValueError, match="fmt"):
        run(m, [(Y, UV)], fmt="nv12", out="float32")
    with pytest.raises(ValueError, match="fmt"):
        run(m, [(Y, UV)], fmt="nv12", unit_range=True)


def test_arguments_are_checked_when_the_function_is_called():
    """Not at the first next(): a bad argument never leaves a generator behind that fails later."""
    with pytest.raises(ValueError, match="frames_per_step"):
        utils.run_model_inference_stream(Never(), [U8], CPU, frames_per_step=0)
    with pytest.raises(ValueError, match="out must be"):
        utils.run_model_inference_stream(Never(), [U8], CPU, out="int8")


def test_no_cpu_fallback_and_the_empty_stream():
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        run(Never(), [U8])
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        run(Never(), [(Y, U, U)], fmt="i420")
    assert run(Never(), []) == [] and run(Never(), iter(()), fmt="nv12") == []


def test_an_error_surfaces_at_the_offending_frame():
    """The iterable is read one frame at a time: a bad frame raises when it is handed over and nothing after it is
    taken; a valid frame before it is dealt with first (here: refused for the device, as nothing runs on a CPU)."""
    taken = []

    def frames(seq):
        for i, f in enumerate(seq):
            taken.append(i)
            yield f
    bad = np.zeros((8, 12), np.uint8)
    with pytest.raises(ValueError, match="frame"):
        run(Never(), frames([bad, U8, U8]))
    assert taken == [0]
    del taken[:]
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        run(Never(), frames([U8, bad, U8]), frames_per_step=4)
    assert taken == [0, 1], "the second frame closed the group of the first, the third was never taken"
    # the grouping itself hands the frames before the offending one out first, then the error
    seen = []

    def prepare(x):
        if x < 0:
            raise ValueError("negative")
        return ("key", x)
    with pytest.raises(ValueError, match="negative"):
        for g in stream._grouped([1, 2, 3, -1, 5], prepare, 2):
            seen.append([x for _, x in g])
    assert seen == [[1, 2], [3]]

    def broken():
        yield 1
        raise KeyError("the loader broke")
    del seen[:]
    with pytest.raises(KeyError):
        for g in stream._grouped(broken(), prepare, 4):
            seen.append([x for _, x in g])
    assert seen == [[1]]


def test_group_frames():
    a, b = ((40, 56, 1), np.dtype(np.uint8)), ((56, 40, 1), np.dtype(np.uint8))
    assert stream.group_frames([a] * 7, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert stream.group_frames([a, a, b, a], 2) == [[0, 1], [2], [3]]
    assert stream.group_frames([a, a, a, b, b, a, a, a, a, a], 4) == [[0, 1, 2], [3, 4], [5, 6, 7, 8], [9]]
    assert stream.group_frames([a, ((40, 56, 1), np.dtype(np.uint16)), a], 4) == [[0], [1], [2]]       # the dtype counts
    assert stream.group_frames([a] * 5, 1) == [[0], [1], [2], [3], [4]]
    assert stream.group_frames([], 3) == [] and stream.group_frames(iter([a, a]), 8) == [[0, 1]]
    flat = [i for g in stream.group_frames([a, b] * 5 + [a] * 5, 3) for i in g]
    assert flat == list(range(15)), "order is preserved"


@pytest.mark.parametrize("sigma", [15, 25, 50])
def test_noise_field_is_the_reference_draw(sigma):
    shape = (24, 40, 3)
    np.random.seed(seed=0)
    want = np.random.normal(0, sigma / 255., shape)
    np.random.seed(seed=12345)
    state = np.random.get_state()[1].copy()
    got = utils.noise_field(sigma, shape)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(np.random.get_state()[1], state), "the process-wide generator is left alone"
    img = np.full(shape, 0.5, np.float32)
    assert np.array_equal(utils.add_gaussian_noise(img.copy(), sigma), np.clip(img + want, 0, 1).astype(np.float32))


def test_model_hooks_follow_the_model_class():
    from irm_amd import dncnn, restormer
    assert utils._model_hooks(deblurganv2.FPNMobileNet()) == ("deblurganv2", True)
    assert utils._model_hooks(restormer.Restormer(LayerNorm_type="BiasFree")) == (None, True)
    assert utils._model_hooks(dncnn.DnCNN(1, 1, 64, 4, "R")) == (None, False)
    assert utils._model_hooks(Never()) == (None, False)


def test_evaluate_stream_argument_errors():
    kw = dict(task="denoising", subtask="gaussian", dataset="synthetic", model_name="DnCNN")
    cfg = dict(patch_size=32, patch_overlap=8)
    pair = (U8, U8, "a.png")
    with pytest.raises(ValueError, match="metrics"):
        harness.evaluate_stream(Never(), [pair], CPU, cfg, metrics="gpu", **kw)
    with pytest.raises(ValueError, match="frames_per_step"):
        harness.evaluate_stream(Never(), [pair], CPU, cfg, frames_per_step=0, **kw)
    with pytest.raises(ValueError, match="target"):
        harness.evaluate_stream(Never(), [(U8, U8.astype(np.float32), "a.png")], CPU, cfg, **kw)
    with pytest.raises(ValueError, match="target"):
        harness.evaluate_stream(Never(), [(U8, U8[:4], "a.png")], CPU, cfg, **kw)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        harness.evaluate_stream(Never(), [pair], CPU, cfg, **kw)
    row = harness.evaluate_stream(Never(), [], CPU, cfg, **kw)
    assert row["Failed"] == [] and np.isnan(row["PSNR"]) and row["Model"] == "DnCNN"


def test_no_cyclic_gc_during_a_capture():
    """graphed_forward captures with the cyclic collector off (a dead cycle that holds another model's graph or
    pinned memory must not be freed inside a capture) and leaves the collector as it found it."""
    import gc
    import inspect
    assert gc.isenabled()
    with utils._no_cyclic_gc():
        assert not gc.isenabled()
    assert gc.isenabled()
    with pytest.raises(KeyError):
        with utils._no_cyclic_gc():
            raise KeyError("inside")
    assert gc.isenabled()
    gc.disable()
    try:
        with utils._no_cyclic_gc():
            assert not gc.isenabled()
        assert not gc.isenabled(), "a collector that was off stays off"
    finally:
        gc.enable()
    src = inspect.getsource(utils.graphed_forward)
    assert "with _no_cyclic_gc(), torch.cuda.graph(g):" in src


def test_plan_release_empties_the_plan():
    plan = stream._Plan.__new__(stream._Plan)
    plan.pin_in, plan.np_in, plan.up, plan.count, plan.seen = [object()], [[object()]], [object()], 3, {2}
    plan.release()
    assert plan.pin_in == [] and plan.np_in == [] and plan.up == [] and plan.count == 3 and plan.seen == {2}
