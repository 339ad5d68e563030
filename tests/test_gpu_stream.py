"""The frame stream on the GPU (irm_amd/stream.py): utils.run_model_inference_stream and harness.evaluate_stream.

The yardstick is never the stream itself: it is tiled_forward_device_batch on the same groups, run synchronously
BEFORE the stream and downloaded (for YUV frames the public converter -> batch call -> converter composition).  Every
comparison of frames is np.array_equal; synthetic weights, frames from synth.synth_image_pair with distinct indices.
No test times anything."""
import functools

import numpy as np
import pytest
import torch

from irm_amd import deblurganv2, dncnn, harness, restormer, stream, synth, utils, yuv

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def frames_u8(n, h, w, c, first=0):
    """n distinct uint8 frames, made once; no test writes them."""
    out = tuple(synth.synth_image_pair(first + i, h, w, c, seed_base=4200, blur=3)[0] for i in range(n))
    assert all(not np.array_equal(out[0], f) for f in out[1:])
    return out


def max_batch(model):
    return getattr(model, "max_tiles_per_batch", 8)


def yardstick(model, frames, dev, k, patch, overlap, pad8=False, **kw):
    """tiled_forward_device_batch on the groups the stream forms, synchronously, downloaded."""
    groups = stream.group_frames([(f.shape, f.dtype) for f in frames], k)
    want = []
    with torch.no_grad():
        for g in groups:
            res = utils.tiled_forward_device_batch(model, [utils.to_device(frames[i], dev) for i in g], patch, overlap, pad8,
                                                   max_batch=max_batch(model), **kw)
            want += [utils.to_host(o) for o, _ in res]
    torch.cuda.synchronize()
    return want, [len(g) for g in groups]


def same(got, want):
    assert len(got) == len(want)
    for i, (g, t) in enumerate(zip(got, want)):
        assert g.dtype == t.dtype and g.shape == t.shape, (i, g.dtype, t.dtype, g.shape, t.shape)
        assert np.array_equal(g, t), f"frame {i}: {int((g != t).sum())} of {t.size} values differ"


def run_stream(model, frames, dev, **kw):
    got = list(utils.run_model_inference_stream(model, iter(frames), dev, **kw))
    assert all(ms >= 0 for _, ms in got)
    return [p for p, _ in got]


@pytest.fixture(scope="module")
def gray(dev):
    return dncnn.DnCNN(1, 1, 64, 4, "R").load_synthetic(42).eval().to(dev)


@pytest.fixture(scope="module")
def colour(dev):
    return dncnn.DnCNN(3, 3, 64, 4, "R").load_synthetic(42).eval().to(dev)


# --------------------------------------------------------------------------- 1: order and equality
def test_order_and_equality(dev, gray):
    """7 gray frames at 3 per step (groups 3, 3, 1): the batch call's frames in input order, which for this model are
    the one-frame call's too."""
    frames = frames_u8(7, 40, 56, 1)
    want, sizes = yardstick(gray, frames, dev, 3, 32, 8)
    assert sizes == [3, 3, 1]
    single = [utils.run_model_inference(gray, f, dev, patch_size=32, patch_overlap=8)[0] for f in frames]
    got = run_stream(gray, frames, dev, patch_size=32, patch_overlap=8, frames_per_step=3)
    same(got, want)
    same(got, single)
    assert all(not np.array_equal(g, f) for g, f in zip(got, frames)), "the model ran"


# --------------------------------------------------------------------------- 2: slot reuse
def test_slot_reuse_at_a_size_where_copies_take_time(dev, colour):
    """9 frames of 1280 x 720 at 2 per step: 5 groups on 2 slots.  Every yielded array is kept and compared only after
    the stream has ended: a view of a pinned slot, or a slot rewritten too early, shows here."""
    frames = frames_u8(9, 720, 1280, 3)
    cfg = utils.get_patch_config("denoising", "gaussian", "DnCNN")
    want, sizes = yardstick(colour, frames, dev, 2, cfg["patch_size"], cfg["patch_overlap"])
    assert sizes == [2, 2, 2, 2, 1]
    kept = []
    for pred, _ in utils.run_model_inference_stream(colour, iter(frames), dev, frames_per_step=2, **cfg):
        kept.append(pred)
    same(kept, want)
    assert all(a.flags.owndata for a in kept), "the yielded arrays are the caller's own copies"


# --------------------------------------------------------------------------- 3: Restormer, uint16, pad to 8
def test_restormer_uint16_pad8(dev):
    model = restormer.Restormer(LayerNorm_type="WithBias").load_synthetic(42).eval().to(dev)
    frames = [(f.astype(np.uint16) * 257 + i) for i, f in enumerate(frames_u8(3, 40, 56, 3))]
    want, sizes = yardstick(model, frames, dev, 2, 32, 8, pad8=True)
    assert sizes == [2, 1]
    got = run_stream(model, frames, dev, patch_size=32, patch_overlap=8, frames_per_step=2)
    assert all(g.dtype == np.uint16 for g in got)
    same(got, want)


# --------------------------------------------------------------------------- 4: float32 frames
def test_float32_frames(dev, colour):
    base = frames_u8(5, 40, 56, 3)
    # the frame's own min / max, reduced on the device: maxima that differ and exceed 1
    frames = [f.astype(np.float32) * np.float32((i + 3) / 255.0) + np.float32(0.01 * i) for i, f in enumerate(base)]
    assert len({float(f.max()) for f in frames}) == 5 and min(float(f.max()) for f in frames) > 1
    want, _ = yardstick(colour, frames, dev, 2, 32, 8)
    got = run_stream(colour, frames, dev, patch_size=32, patch_overlap=8, frames_per_step=2)
    assert all(g.dtype == np.float32 for g in got)
    same(got, want)
    # in [0, 1] by contract, requantised
    unit = [f.astype(np.float32) / np.float32(255.0) for f in base]
    want, _ = yardstick(colour, unit, dev, 2, 32, 8, unit_range=True, out="uint8")
    got = run_stream(colour, unit, dev, patch_size=32, patch_overlap=8, frames_per_step=2, unit_range=True, out="uint8")
    assert all(g.dtype == np.uint8 for g in got)
    same(got, want)
    # an integer frame as float32
    want, _ = yardstick(colour, base, dev, 2, 32, 8, out="float32")
    same(run_stream(colour, base, dev, patch_size=32, patch_overlap=8, frames_per_step=2, out="float32"), want)


# --------------------------------------------------------------------------- 5: YUV
def random_planes(rng, fmt, h, w):
    top, shift, dt = (1024, 6, np.uint16) if fmt == "p010" else (256, 0, np.uint8)
    y = (rng.integers(0, top, (h, w)) << shift).astype(dt)
    if fmt == "i420":
        return (y, (rng.integers(0, top, (h // 2, w // 2)) << shift).astype(dt),
                (rng.integers(0, top, (h // 2, w // 2)) << shift).astype(dt))
    return y, (rng.integers(0, top, (h // 2, w // 2, 2)) << shift).astype(dt)


def yuv_yardstick(model, frames, dev, fmt, k, patch, overlap, **opts):
    """Per group: the public converter per frame, the batch call, the public converter back; downloaded."""
    luma_only = opts.get("luma_only", False)
    want = []
    with torch.no_grad():
        for g in stream.group_frames([p[0].shape for p in frames], k):
            ups = [tuple(utils.to_device(p, dev) for p in frames[i]) for i in g]
            rgb = [yuv.yuv420_to_rgb_device(up[:1] if luma_only else up, fmt, **opts) for up in ups]
            res = utils.tiled_forward_device_batch(model, rgb, patch, overlap, False, max_batch=max_batch(model),
                                                   unit_range=True, out="float32")
            for (frame, _), up in zip(res, ups):
                back = yuv.rgb_to_yuv420_device(frame, fmt, out=up if luma_only else None, **opts)
                want.append(tuple(utils.to_host(p) for p in back))
    torch.cuda.synchronize()
    return want


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_yuv_colour(dev, colour, fmt):
    rng = np.random.default_rng(51)
    frames = [random_planes(rng, fmt, 32, 48) for _ in range(5)]
    opts = dict(matrix="bt601", full_range=True, siting="center") if fmt == "p010" else {}
    want = yuv_yardstick(colour, frames, dev, fmt, 2, 32, 8, **opts)
    got = run_stream(colour, frames, dev, fmt=fmt, patch_size=32, patch_overlap=8, frames_per_step=2, **opts)
    assert len(got) == 5
    for g, t, f in zip(got, want, frames):
        assert isinstance(g, tuple) and len(g) == 2
        same(list(g), list(t))
        assert not np.array_equal(g[0], f[0]), "the model ran"


def test_yuv_i420_luma_only(dev, gray):
    rng = np.random.default_rng(52)
    frames = [random_planes(rng, "i420", 32, 48) for _ in range(5)]
    before = [tuple(p.copy() for p in f) for f in frames]
    want = yuv_yardstick(gray, frames, dev, "i420", 2, 32, 8, luma_only=True)
    got = run_stream(gray, frames, dev, fmt="i420", luma_only=True, patch_size=32, patch_overlap=8, frames_per_step=2)
    for g, t, f, b in zip(got, want, frames, before):
        assert len(g) == 3 and np.array_equal(g[0], t[0]) and not np.array_equal(g[0], b[0])
        assert np.array_equal(g[1], b[1]) and np.array_equal(g[2], b[2]), "the chroma planes come back untouched"
        assert all(np.array_equal(p, q) for p, q in zip(f, b)), "the caller's planes are not written"


# --------------------------------------------------------------------------- 6: degradation
def test_need_degradation(dev, colour):
    frames = frames_u8(5, 40, 56, 3)
    want, _ = yardstick(colour, frames, dev, 2, 32, 8, noise_sigma=25)
    single = [utils.run_model_inference(colour, f, dev, patch_size=32, patch_overlap=8, need_degradation=True,
                                        noise_level=25)[0] for f in frames]
    clean, _ = yardstick(colour, frames, dev, 2, 32, 8)
    got = run_stream(colour, frames, dev, patch_size=32, patch_overlap=8, frames_per_step=2, need_degradation=True,
                     noise_level=25)
    same(got, want)
    same(got, single)
    assert all(not np.array_equal(g, c) for g, c in zip(got, clean)), "the noise was added"
    # without a level nothing is added, as in the one-frame call
    same(run_stream(colour, frames, dev, patch_size=32, patch_overlap=8, frames_per_step=2, need_degradation=True), clean)


# --------------------------------------------------------------------------- 7: DeblurGANv2 hooks
def test_deblurganv2_hooks(dev):
    model = deblurganv2.FPNMobileNet().load_synthetic(42).to(dev)
    frames = frames_u8(3, 64, 96, 3)
    want, sizes = yardstick(model, frames, dev, 2, None, 32, pad8=True, hooks="deblurganv2")
    assert sizes == [2, 1]
    same(run_stream(model, frames, dev, patch_size=None, frames_per_step=2), want)
    with pytest.raises(ValueError, match="deblurganv2"):
        run_stream(model, [frames[0], frames[1].astype(np.float32)], dev, frames_per_step=2)


# --------------------------------------------------------------------------- 8: two shapes
def test_two_shapes_in_one_stream(dev, gray):
    a, b = frames_u8(3, 40, 56, 1), frames_u8(1, 56, 40, 1, first=10)
    frames = [a[0], a[1], b[0], a[2]]
    want, sizes = yardstick(gray, frames, dev, 2, 32, 8)
    assert sizes == [2, 1, 1]
    got = run_stream(gray, frames, dev, patch_size=32, patch_overlap=8, frames_per_step=2)
    assert [g.shape for g in got] == [(40, 56, 1), (40, 56, 1), (56, 40, 1), (40, 56, 1)]
    same(got, want)
    # more shapes than plans are kept: the least recently used one is made again
    many = [frames_u8(1, 40 + 8 * i, 56, 1, first=20 + i)[0] for i in range(stream.MAX_PLANS + 1)]
    order = many + many[:2]
    want, _ = yardstick(gray, order, dev, 2, 32, 8)
    same(run_stream(gray, order, dev, patch_size=32, patch_overlap=8, frames_per_step=2), want)


# --------------------------------------------------------------------------- 9: early exit and errors
class ThirdForwardRaises(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls = inner, 0

    def forward(self, x):
        self.calls += 1
        if self.calls == 3:
            raise RuntimeError("the third forward")
        return self.inner(x)


def test_early_exit_and_errors(dev, gray):
    frames = frames_u8(6, 40, 56, 1)
    kw = dict(patch_size=32, patch_overlap=8, frames_per_step=2)
    want, _ = yardstick(gray, frames, dev, 2, 32, 8)
    # the consumer breaks after the first frame
    gen = utils.run_model_inference_stream(gray, iter(frames), dev, **kw)
    for pred, _ in gen:
        first = pred
        break
    gen.close()
    same([first], want[:1])
    same([utils.run_model_inference(gray, frames[3], dev, patch_size=32, patch_overlap=8)[0]], want[3:4])
    same(run_stream(gray, frames, dev, **kw), want)
    # an exception in the consumer, thrown into the generator
    gen = utils.run_model_inference_stream(gray, iter(frames), dev, **kw)
    next(gen)
    with pytest.raises(KeyError):
        gen.throw(KeyError("the consumer"))
    same(run_stream(gray, frames, dev, **kw), want)
    # the model raises from Python in its third forward: one forward per group here (2 frames x 4 tiles)
    model = ThirdForwardRaises(gray)
    got = []
    with pytest.raises(RuntimeError, match="third forward"):
        for pred, _ in utils.run_model_inference_stream(model, iter(frames), dev, **kw):
            got.append(pred)
    assert model.calls == 3
    same(got, want[:4])
    same(run_stream(gray, frames, dev, **kw), want)
    # a bad frame in the middle: the frames before it first
    got = []
    with pytest.raises(ValueError, match="frame"):
        for pred, _ in utils.run_model_inference_stream(gray, iter(list(frames[:3]) + [frames[3][:, :, 0]] + [frames[4]]),
                                                        dev, **kw):
            got.append(pred)
    same(got, want[:2] + [utils.run_model_inference(gray, frames[2], dev, patch_size=32, patch_overlap=8)[0]])
    # an iterable that raises
    def loader():
        yield from frames[:3]
        raise OSError("the decoder broke")
    got = []
    with pytest.raises(OSError, match="decoder"):
        for pred, _ in utils.run_model_inference_stream(gray, loader(), dev, **kw):
            got.append(pred)
    assert len(got) == 3
    same(got[:2], want[:2])
    same(run_stream(gray, frames, dev, **kw), want)


# --------------------------------------------------------------------------- 10: the harness
def test_evaluate_stream_against_evaluate(dev, colour):
    pairs = list(harness.synthetic_loader(5, h=40, w=56, c=3, seed_base=77, blur=3))
    cfg = dict(patch_size=32, patch_overlap=8)
    kw = dict(task="denoising", subtask="gaussian", dataset="synthetic", model_name="DnCNN")
    ref = harness.evaluate(colour, iter(pairs), dev, cfg, metrics="device", **kw)
    for metrics in ("device", "host"):
        row = harness.evaluate_stream(colour, iter(pairs), dev, cfg, frames_per_step=2, metrics=metrics, **kw)
        for col in ("PSNR", "SSIM", "Std_PSNR", "Std_SSIM"):
            assert np.isfinite(row[col]) and abs(row[col] - ref[col]) <= 1e-9, (metrics, col, row[col], ref[col])
        assert not row.get("Failed") and row["Avg_Time_ms"] > 0 and list(row)[:len(harness.COLUMNS)] == list(ref)[:len(harness.COLUMNS)]
        assert row["Model_Params"] == ref["Model_Params"]
    noisy = harness.evaluate(colour, iter(pairs), dev, cfg, metrics="device", need_degradation=True, noise_level=25, **kw)
    row = harness.evaluate_stream(colour, iter(pairs), dev, cfg, frames_per_step=4, need_degradation=True, noise_level=25, **kw)
    assert abs(row["PSNR"] - noisy["PSNR"]) <= 1e-9 and abs(row["SSIM"] - noisy["SSIM"]) <= 1e-9
    assert abs(noisy["PSNR"] - ref["PSNR"]) > 1e-3
    with pytest.raises(ValueError, match="frame"):                  # no skip_failed: the exception propagates
        harness.evaluate_stream(colour, iter(pairs[:2] + [(pairs[0][0][:, :, 0], pairs[0][1], "bad")]), dev, cfg, **kw)
