"""YUV 4:2:0 frames on the GPU: irm_yuv420_to_rgb_f32 and irm_rgb_f32_to_yuv420 (include/irm_hip_yuv.h) bit-exact
against the float32 model of tests/yuv_model.py between guard bands, the clips of out-of-gamut input, and
utils.run_model_inference_yuv against the composition of its parts.

Every comparison is exact: the kernels restate the model's float32 operation order."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import yuv_model
from irm_amd import _hip, dncnn, mair, utils, yuv

from guards import PAD, int_fill, intact, sentinel, sentinel_out, two_fills

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FORMATS, SITINGS = ("i420", "nv12", "p010"), ("left", "center")

#: (H, W, luma pitch, planar chroma pitch) in samples, None = dense; an interleaved UV row holds two samples per chroma
#: column, so its pitch is twice the planar one
SHAPES = [(2, 2, None, None), (2, 4, None, None), (4, 2, None, None),      # the smallest frames, every pixel an edge
          (6, 10, None, None),
          (16, 64, None, None),                                            # the 16-byte path
          (34, 258, None, None),                                           # W % 4 = 2: the element path, several workgroups
          (18, 34, 40, 24)]                                                # pitched planes
#: (shape, fmt, siting, matrix, full_range, luma_only)
CASES = [(s, f, c, "bt709", False, False) for s in SHAPES for f in FORMATS for c in SITINGS]
CASES += [(s, f, c, m, r, False) for s in (SHAPES[3], SHAPES[5]) for f in FORMATS for c in SITINGS
          for m, r in (("bt601", False), ("bt601", True), ("bt709", True))]
CASES += [(s, f, "left", "bt709", False, True) for s in (SHAPES[0], SHAPES[5]) for f in FORMATS]
IDS = ["%dx%d%s-%s-%s-%s-%s%s" % (s[0], s[1], "p" if s[2] else "", f, c, m, "full" if r else "lim", "-luma" if lo else "")
       for s, f, c, m, r, lo in CASES]


def random_planes(rng, fmt, h, w):
    top, shift, dt = (1024, 6, np.uint16) if fmt == "p010" else (256, 0, np.uint8)
    y = (rng.integers(0, top, (h, w)) << shift).astype(dt)
    if fmt == "i420":
        return (y, (rng.integers(0, top, (h // 2, w // 2)) << shift).astype(dt),
                (rng.integers(0, top, (h // 2, w // 2)) << shift).astype(dt))
    return y, (rng.integers(0, top, (h // 2, w // 2, 2)) << shift).astype(dt)


def pitched(shape, pitch, dtype, dev, fill):
    """(buf, view): a plane of `shape` ([rows][cols] or [rows][cols][2]) with row pitch `pitch` (None: dense) in the
    middle of a buffer that holds `fill` everywhere, the pitch padding included."""
    row = int(np.prod(shape[1:]))
    pitch = row if pitch is None else pitch
    assert pitch >= row
    n = (shape[0] - 1) * pitch + row
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    strides = (pitch, 1) if len(shape) == 2 else (pitch, 2, 1)
    return buf, buf.as_strided(shape, strides, PAD)


def plane_pitches(fmt, pitch_y, pitch_c):
    return [pitch_y] + ([pitch_c, pitch_c] if fmt == "i420" else [None if pitch_c is None else 2 * pitch_c])


def bits(a: np.ndarray) -> torch.Tensor:
    """A host plane as the tensor the device holds: uint16 as its int16 bit pattern."""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def operands(views, fmt, luma_only):
    """(y, u, v, chroma_step, pitch_y, pitch_c) of device plane views, as the entry points take them."""
    y = views[0]
    if luma_only:
        return _hip.ptr(y), None, None, 1, y.stride(0), 0
    if fmt == "i420":
        return _hip.ptr(y), _hip.ptr(views[1]), _hip.ptr(views[2]), 1, y.stride(0), views[1].stride(0)
    uv = views[1]
    return _hip.ptr(y), _hip.ptr(uv[:, :, 0]), _hip.ptr(uv[:, :, 1]), 2, y.stride(0), uv.stride(0)


def options(fmt, matrix, full, siting, luma_only):
    return (yuv_model.DEPTH[fmt], int(fmt == "p010"), int(matrix == "bt709"), int(full), int(siting == "center"),
            int(luma_only))


@functools.lru_cache(maxsize=None)
def reference(shape, fmt, siting, matrix, full, luma_only):
    """Seeded inputs of a case and the float32 model's results, made once: (planes, rgb of the planes, frame, planes
    of the frame).  The frame reaches beyond [0, 1] on both sides."""
    h, w = shape[:2]
    rng = np.random.default_rng(1000 + 7 * h + w)
    planes = random_planes(rng, fmt, h, w)
    rgb = yuv_model.to_rgb(planes, fmt, matrix, full, siting, luma_only)
    frame = rng.uniform(-0.1, 1.1, (h, w, 1 if luma_only else 3)).astype(np.float32)
    back = yuv_model.to_yuv(frame, fmt, matrix, full, siting, luma_only)
    return planes, rgb, frame, back


@pytest.mark.parametrize("shape,fmt,siting,matrix,full,luma_only", CASES, ids=IDS)
def test_guard_bands_yuv420_to_rgb(dev, shape, fmt, siting, matrix, full, luma_only):
    """Planes between bands of zeros and then of ones (the pitch padding included): the frame must not depend on them;
    the float frame between sentinels, all intact; the frame itself equal to the float32 model bit for bit."""
    h, w, py, pc = shape
    planes, want, _, _ = reference(shape, fmt, siting, matrix, full, luma_only)
    used = planes[:1] if luma_only else planes

    def run(fill):
        views = []
        for p, pitch in zip(used, plane_pitches(fmt, py, pc)):
            t = bits(p)
            _, view = pitched(tuple(t.shape), pitch, t.dtype, dev, int_fill(t.dtype, fill))
            view.copy_(t)
            views.append(view)
        buf, out = sentinel_out((h, w, 1 if luma_only else 3), dev)
        _hip.call("irm_yuv420_to_rgb_f32", *operands(views, fmt, luma_only), *options(fmt, matrix, full, siting, luma_only),
                  h, w, _hip.ptr(out))
        torch.cuda.synchronize()
        assert intact(buf, out), "a store outside the float frame"
        return (out.cpu(),)
    got = two_fills(run)[0].numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{int((got != want).sum())} of {want.size} values differ from the float32 model"
    # the public call on the same (pitched) planes
    views = []
    for p, pitch in zip(used, plane_pitches(fmt, py, pc)):
        t = bits(p)
        _, view = pitched(tuple(t.shape), pitch, t.dtype, dev, 0)
        view.copy_(t)
        views.append(view)
    pub = yuv.yuv420_to_rgb_device(tuple(views), fmt, matrix, full, siting, luma_only)
    assert pub.is_contiguous() and np.array_equal(pub.cpu().numpy(), want)


@pytest.mark.parametrize("shape,fmt,siting,matrix,full,luma_only", CASES, ids=IDS)
def test_guard_bands_rgb_to_yuv420(dev, shape, fmt, siting, matrix, full, luma_only):
    """The float frame between bands of NaN, every output plane between sentinels that also fill its pitch padding: all
    intact afterwards, the planes equal to the float32 model's byte for byte.  With luma_only the chroma planes are
    operands too and must stay untouched."""
    h, w, py, pc = shape
    _, _, frame, want = reference(shape, fmt, siting, matrix, full, luma_only)
    n = PAD + frame.size + PAD
    src = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    src[PAD:PAD + frame.size] = torch.from_numpy(frame).reshape(-1).to(dev)
    dt = torch.int16 if fmt == "p010" else torch.uint8
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)] if fmt == "i420" else [(h, w), (h // 2, w // 2, 2)]
    placed = [pitched(s, pitch, dt, dev, sentinel(dt)) for s, pitch in zip(shapes, plane_pitches(fmt, py, pc))]
    views = [v for _, v in placed]
    _hip.call("irm_rgb_f32_to_yuv420", _hip.ptr(src[PAD:]), *operands(views, fmt, luma_only),
              *options(fmt, matrix, full, siting, luma_only), h, w)
    torch.cuda.synchronize()
    for i, (buf, view) in enumerate(placed):
        assert intact(buf, view), f"a store outside plane {i} (bands or pitch padding)"
        if luma_only and i > 0:
            assert bool((view == sentinel(dt)).all()), "luma_only must not write chroma"
    for i, t in enumerate(want):
        got = utils.to_host(views[i].contiguous())
        assert got.dtype == t.dtype and np.array_equal(got, t), \
            f"plane {i}: {int((got != t).sum())} of {t.size} codes differ from the float32 model"
    # the public call: dense new planes, or the caller's (pitched) planes through out=
    rgb = torch.from_numpy(frame).to(dev)
    if not luma_only:
        for got, t in zip(yuv.rgb_to_yuv420_device(rgb, fmt, matrix, full, siting), want):
            assert got.is_contiguous() and np.array_equal(utils.to_host(got), t)
    placed = [pitched(s, pitch, dt, dev, sentinel(dt)) for s, pitch in zip(shapes, plane_pitches(fmt, py, pc))]
    out = yuv.rgb_to_yuv420_device(rgb, fmt, matrix, full, siting, luma_only, out=tuple(v for _, v in placed))
    assert all(intact(buf, view) for buf, view in placed)
    assert np.array_equal(utils.to_host(out[0].contiguous()), want[0])
    if luma_only:
        assert all(bool((o == sentinel(dt)).all()) for o in out[1:]), "the chroma planes come back as they are"


# --------------------------------------------------------------------------- out of gamut
@pytest.mark.parametrize("fmt", FORMATS)
def test_out_of_gamut_codes_are_clipped_to_the_unit_range(dev, fmt):
    """Limited-range codes can encode RGB outside [0, 1]: Y = 235 with Cr = 240 is white plus half the red excursion,
    Y = 16 with Cb = Cr = 16 lies below black in red and blue.  The frame is clipped, as the unit range needs."""
    k = 4 if fmt == "p010" else 1
    h, w = 4, 8
    y = np.full((h, w), 235 * k, np.int64)
    u = np.full((h // 2, w // 2), 128 * k, np.int64)
    v = np.full((h // 2, w // 2), 240 * k, np.int64)
    y[:, 4:], u[:, 2:], v[:, 2:] = 16 * k, 16 * k, 16 * k
    planes = yuv_model.planes_of(y, u, v, fmt)
    want = yuv_model.to_rgb(planes, fmt, "bt709", False, "left")
    assert want.max() == 1.0 and want.min() == 0.0
    assert 1.0 + 2 * (1 - 0.2126) * 0.5 > 1.7               # R of (235, 128, 240) before the clip
    got = yuv.yuv420_to_rgb_device(tuple(bits(p).to(dev) for p in planes), fmt).cpu().numpy()
    assert np.array_equal(got, want) and got[0, 0, 0] == 1.0 and got[0, 7, 0] == 0.0 and got[0, 7, 2] == 0.0


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
def test_values_outside_the_unit_range_clip_the_codes(dev, fmt, full):
    """-0.25 and 1.5 lie beyond the codes of either range: the codes are clipped to 0 .. 2^d - 1, not wrapped."""
    h, w = 4, 8
    top = 1023 if fmt == "p010" else 255
    frame = np.full((h, w, 3), 1.5, np.float32)
    frame[:, 4:] = -0.25
    frame[2:, :4, 0], frame[2:, 4:, 2] = -0.25, 1.5          # saturated chroma on both sides as well
    want = yuv_model.to_yuv(frame, fmt, "bt601", full, "center")
    yc, uc, vc = yuv_model.codes_of(want, fmt)
    assert yc.max() == top and yc.min() == 0 and max(uc.max(), vc.max()) == top and min(uc.min(), vc.min()) == 0
    got = yuv.rgb_to_yuv420_device(torch.from_numpy(frame).to(dev), fmt, "bt601", full, "center")
    for g, t in zip(got, want):
        assert np.array_equal(utils.to_host(g), t)


# --------------------------------------------------------------------------- the whole call
def composition(model, planes, dev, fmt, patch, overlap, pad8=False, **opts):
    """What run_model_inference_yuv is made of: the device conversion, the device pipeline on the float32 frame, and
    the numpy twin of the way back on the downloaded frame."""
    luma_only = opts.get("luma_only", False)
    up = tuple(bits(p).to(dev) for p in (planes[:1] if luma_only else planes))
    frame = yuv.yuv420_to_rgb_device(up, fmt, **opts)
    out, _ = utils.tiled_forward_device(model, frame, patch, overlap, pad8, unit_range=True, out="float32",
                                        max_batch=getattr(model, "max_tiles_per_batch", 8))
    keep = tuple(p.copy() for p in planes) if luma_only else None
    return yuv.rgb_to_yuv420_host(out.cpu().numpy(), fmt, out=keep, **opts)


def test_whole_call_nv12_colour_dncnn(dev):
    model = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    planes = random_planes(np.random.default_rng(31), "nv12", 48, 80)
    got, ms = utils.run_model_inference_yuv(model, planes, dev, fmt="nv12", patch_size=32, patch_overlap=8)
    want = composition(model, planes, dev, "nv12", 32, 8)
    assert ms > 0 and len(got) == 2
    for g, t in zip(got, want):
        assert g.dtype == np.uint8 and g.shape == t.shape and np.array_equal(g, t)
    assert not np.array_equal(got[0], planes[0]), "the model ran"


def test_whole_call_luma_only_gray_dncnn(dev):
    model = dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(42).eval().to(dev)
    planes = random_planes(np.random.default_rng(32), "nv12", 48, 80)
    before = tuple(p.copy() for p in planes)
    got, _ = utils.run_model_inference_yuv(model, planes, dev, fmt="nv12", luma_only=True, patch_size=32, patch_overlap=8,
                                           matrix="bt601", siting="center")
    want = composition(model, planes, dev, "nv12", 32, 8, luma_only=True, matrix="bt601", siting="center")
    assert len(got) == 2 and np.array_equal(got[1], before[1]) and np.array_equal(planes[1], before[1])
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0]) and not np.array_equal(got[0], before[0])
    assert np.array_equal(planes[0], before[0]), "the caller's Y plane is not written"


def test_whole_call_p010(dev):
    model = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    planes = random_planes(np.random.default_rng(33), "p010", 16, 24)
    got, _ = utils.run_model_inference_yuv(model, planes, dev, fmt="p010", full_range=True, patch_size=32, patch_overlap=8)
    want = composition(model, planes, dev, "p010", 32, 8, full_range=True)
    for g, t in zip(got, want):
        assert g.dtype == np.uint16 and np.array_equal(g, t) and int((g & 63).max()) == 0


def test_whole_call_super_resolution(dev):
    with open(os.path.join(GOLDEN, "mair_sr.json")) as f:
        cfg = json.load(f)["configs"]["light_x2"]
    model = mair.MaIR(**cfg).load_synthetic(42).eval().to(dev)
    planes = random_planes(np.random.default_rng(34), "i420", 16, 24)
    got, _ = utils.run_model_inference_yuv(model, planes, dev, fmt="i420", patch_size=32, patch_overlap=8)
    assert [g.shape for g in got] == [(32, 48), (16, 24), (16, 24)] and all(g.dtype == np.uint8 for g in got)
    want = composition(model, planes, dev, "i420", 32, 8, pad8=True)
    for g, t in zip(got, want):
        assert np.array_equal(g, t)
    with pytest.raises(ValueError, match="luma_only"):
        utils.run_model_inference_yuv(model, planes, dev, fmt="i420", luma_only=True)
