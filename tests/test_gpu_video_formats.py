"""The whole grid of YUV formats on the GPU: irm_yuv_to_rgb_f32, irm_rgb_f32_to_yuv and irm_yuv_metrics
(include/irm_hip_video.h) between guard bands - the conversions bit-exact against the float32 model of
tests/yuv_formats_model.py, the scores against the host twin -, the old entry points against the new ones byte for byte,
and the whole call, the stream and the harness on the new names against the composition of their parts."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import yuv_formats_model as fm
from irm_amd import _hip, dncnn, harness, mair, utils, y4m, yuv

from guards import PAD, int_fill, intact, sentinel, sentinel_out, two_fills

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#: the SSIM distance DESIGN.md section 20 records between irm_yuv420_metrics and the host twin
BOUND = 1.5e-13

#: (H, W) per sampling structure: the smallest frame, the element path (odd where the structure allows it), one whole
#: vector group, the vector path plus the 16-byte frame path, a last group that is not full
SHAPES = {"444": [(1, 1), (3, 5), (2, 8), (5, 36), (5, 38)],
          "422": [(1, 2), (3, 6), (2, 16), (5, 32), (5, 34)],
          "420": [(2, 2), (6, 34)]}
#: variants of a vector shape: pitched planes (luma pitch, planar chroma pitch: multiples of 8 keep the vector path, the
#: others leave it) and a frame pointer offset by 4 bytes (the element path of the float frame)
DENSE, PITCH_VEC, PITCH_ODD, OFFSET = "dense", "pitch-vec", "pitch-odd", "offset"


def _cases():
    """(fmt, (H, W), variant, siting, matrix, full_range, luma_only): every row of the grid, both sitings, both matrices,
    both ranges and luma_only per sampling structure, every shape of a structure and every variant of its vector shapes:
    a few dozen, not the product."""
    grid = {"444": ["i444", "nv24", "i444p10", "p410", "i444p12", "p412"],
            "422": ["i422", "nv16", "i422p10", "p210", "i422p12", "p212"],
            "420": ["i420p12", "p012", "i420p10"]}
    options = [("left", "bt709", False, False), ("center", "bt601", True, False), ("center", "bt709", False, False),
               ("left", "bt601", False, False), ("left", "bt709", True, True), ("center", "bt601", False, False)]
    cases = []
    for sub, fmts in grid.items():
        shapes = SHAPES[sub]
        for i, fmt in enumerate(fmts):
            cases.append((fmt, shapes[i % len(shapes)], DENSE) + options[i % len(options)])
            cases.append((fmt, shapes[-2], DENSE) + options[(i + 1) % len(options)])
            cases.append((fmt, shapes[-1], (PITCH_VEC, PITCH_ODD, OFFSET)[i % 3]) + options[(i + 2) % len(options)])
        for j, shape in enumerate(shapes):                   # every shape, whatever the number of formats
            cases.append((fmts[(j + 1) % len(fmts)], shape, DENSE) + options[j % 2])
        if sub != "420":
            for j, variant in enumerate((PITCH_VEC, PITCH_ODD, OFFSET)):
                cases.append((fmts[j], shapes[2], variant) + options[j])
                cases.append((fmts[3 + j], shapes[3], variant) + options[3 + j])
    return sorted(set(cases))


CASES = _cases()
IDS = ["%s-%dx%d-%s-%s-%s-%s%s" % (f, s[0], s[1], v, c, m, "full" if r else "lim", "-luma" if lo else "")
       for f, s, v, c, m, r, lo in CASES]


def test_the_cases_cover_what_they_must():
    assert 30 <= len(CASES) <= 90
    assert {c[0] for c in CASES} >= set(fm.LAYOUTS) - {"i420", "nv12", "p010"}
    for sub, shapes in SHAPES.items():
        mine = [c for c in CASES if fm.LAYOUTS[c[0]][:2] == {"444": (1, 1), "422": (2, 1), "420": (2, 2)}[sub]]
        assert {c[1] for c in mine} == set(shapes)
        assert {c[3] for c in mine} == {"left", "center"} and {c[4] for c in mine} == {"bt601", "bt709"}
        assert {c[5] for c in mine} == {False, True} and {c[6] for c in mine} == {False, True}
        if sub != "420":
            assert {c[2] for c in mine} == {DENSE, PITCH_VEC, PITCH_ODD, OFFSET}


def bits(a: np.ndarray) -> torch.Tensor:
    """A host plane as the tensor the device holds: uint16 as its int16 bit pattern."""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


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


def plane_pitches(fmt, w, variant):
    """The row pitches, in samples, of the planes of a frame `w` wide."""
    sw, _, n = fm.LAYOUTS[fmt][:3]
    if variant not in (PITCH_VEC, PITCH_ODD):
        return [None] * n
    up8 = lambda v: -(-v // 8) * 8                                                          # noqa: E731
    py, pc = (up8(w) + 16, up8(w // sw) + 8) if variant == PITCH_VEC else (w + 6, w // sw + 3)
    return [py] + ([pc, pc] if n == 3 else [2 * pc])


def operands(views, fmt, luma_only):
    """(y, u, v, chroma_step, pitch_y, pitch_c) of device plane views, as the entry points take them."""
    y = views[0]
    if luma_only:
        return _hip.ptr(y), None, None, 1, y.stride(0), 0
    if fm.LAYOUTS[fmt][2] == 3:
        return _hip.ptr(y), _hip.ptr(views[1]), _hip.ptr(views[2]), 1, y.stride(0), views[1].stride(0)
    uv = views[1]
    return _hip.ptr(y), _hip.ptr(uv[:, :, 0]), _hip.ptr(uv[:, :, 1]), 2, y.stride(0), uv.stride(0)


def options(fmt, matrix, full, siting, luma_only):
    sw, sh, _, depth, upper = fm.LAYOUTS[fmt]
    return sw, sh, depth, upper, int(matrix == "bt709"), int(full), int(siting == "center"), int(luma_only)


@functools.lru_cache(maxsize=None)
def reference(fmt, shape, siting, matrix, full, luma_only):
    """Seeded inputs of a case and the float32 model's results, made once and never written: (planes, rgb of the
    planes, frame, planes of the frame).  The frame reaches beyond [0, 1] on both sides."""
    h, w = shape
    rng = np.random.default_rng(2000 + 7 * h + w)
    planes = fm.random_planes(rng, fmt, h, w)
    rgb = fm.to_rgb(planes, fmt, matrix, full, siting, luma_only)
    frame = rng.uniform(-0.1, 1.1, (h, w, 1 if luma_only else 3)).astype(np.float32)
    back = fm.to_yuv(frame, fmt, matrix, full, siting, luma_only)
    return planes, rgb, frame, back


@pytest.mark.parametrize("fmt,shape,variant,siting,matrix,full,luma_only", CASES, ids=IDS)
def test_guard_bands_yuv_to_rgb(dev, fmt, shape, variant, siting, matrix, full, luma_only):
    """Planes between bands of zeros and then of ones (the pitch padding included): the frame must not depend on them;
    the float frame between sentinels, all intact; the frame itself equal to the float32 model bit for bit."""
    h, w = shape
    planes, want, _, _ = reference(fmt, shape, siting, matrix, full, luma_only)
    used = planes[:1] if luma_only else planes
    c = 1 if luma_only else 3

    def place(fill):
        views = []
        for p, pitch in zip(used, plane_pitches(fmt, w, variant)):
            t = bits(p)
            _, view = pitched(tuple(t.shape), pitch, t.dtype, dev, int_fill(t.dtype, fill))
            view.copy_(t)
            views.append(view)
        return views

    def run(fill):
        views = place(fill)
        if variant == OFFSET:                                 # the frame one float into a 16-byte aligned buffer
            buf, wide = sentinel_out((h * w * c + 1,), dev)
            out = wide[1:].view(h, w, c)
        else:
            buf, out = sentinel_out((h, w, c), dev)
        _hip.call("irm_yuv_to_rgb_f32", *operands(views, fmt, luma_only), *options(fmt, matrix, full, siting, luma_only),
                  h, w, _hip.ptr(out))
        torch.cuda.synchronize()
        assert intact(buf, out), "a store outside the float frame"
        return (out.cpu(),)
    got = two_fills(run)[0].numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{int((got != want).sum())} of {want.size} values differ from the float32 model"
    pub = yuv.yuv_to_rgb_device(tuple(place(0)), fmt, matrix, full, siting, luma_only)
    assert pub.is_contiguous() and np.array_equal(pub.cpu().numpy(), want)


@pytest.mark.parametrize("fmt,shape,variant,siting,matrix,full,luma_only", CASES, ids=IDS)
def test_guard_bands_rgb_to_yuv(dev, fmt, shape, variant, siting, matrix, full, luma_only):
    """The float frame between bands of NaN, every output plane between sentinels that also fill its pitch padding: all
    intact afterwards, the planes equal to the float32 model's byte for byte.  With luma_only the chroma planes are
    operands too and must stay untouched."""
    h, w = shape
    _, _, frame, want = reference(fmt, shape, siting, matrix, full, luma_only)
    off = PAD + (1 if variant == OFFSET else 0)
    src = torch.full((off + frame.size + PAD,), float("nan"), dtype=torch.float32, device=dev)
    src[off:off + frame.size] = torch.from_numpy(frame).reshape(-1).to(dev)
    dt = torch.uint8 if fm.LAYOUTS[fmt][3] == 8 else torch.int16
    shapes = fm.plane_shapes(h, w, fmt)
    placed = [pitched(s, pitch, dt, dev, sentinel(dt)) for s, pitch in zip(shapes, plane_pitches(fmt, w, variant))]
    views = [v for _, v in placed]
    _hip.call("irm_rgb_f32_to_yuv", _hip.ptr(src[off:]), *operands(views, fmt, luma_only),
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
    rgb = torch.from_numpy(frame).to(dev)
    if not luma_only:
        for got, t in zip(yuv.rgb_to_yuv_device(rgb, fmt, matrix, full, siting), want):
            assert got.is_contiguous() and np.array_equal(utils.to_host(got), t)
    placed = [pitched(s, pitch, dt, dev, sentinel(dt)) for s, pitch in zip(shapes, plane_pitches(fmt, w, variant))]
    out = yuv.rgb_to_yuv_device(rgb, fmt, matrix, full, siting, luma_only, out=tuple(v for _, v in placed))
    assert all(intact(buf, view) for buf, view in placed)
    assert np.array_equal(utils.to_host(out[0].contiguous()), want[0])


# --------------------------------------------------------------------------- old entry points against the new ones
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_old_and_new_entry_points_agree_byte_for_byte(dev, fmt):
    h, w = 6, 34
    depth, upper = (10, 1) if fmt == "p010" else (8, 0)
    rng = np.random.default_rng(77)
    planes = tuple(bits(p).to(dev) for p in fm.random_planes(rng, fmt, h, w))
    frame = torch.from_numpy(rng.uniform(-0.1, 1.1, (h, w, 3)).astype(np.float32)).to(dev)
    for siting, matrix, full in ((0, 1, 0), (1, 0, 1)):
        a, b = torch.empty_like(frame), torch.empty_like(frame)
        ops = operands(planes, fmt, False)
        _hip.call("irm_yuv420_to_rgb_f32", *ops, depth, upper, matrix, full, siting, 0, h, w, _hip.ptr(a))
        _hip.call("irm_yuv_to_rgb_f32", *ops, 2, 2, depth, upper, matrix, full, siting, 0, h, w, _hip.ptr(b))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        old, new = (tuple(torch.zeros_like(p) for p in planes) for _ in range(2))
        _hip.call("irm_rgb_f32_to_yuv420", _hip.ptr(frame), *operands(old, fmt, False), depth, upper, matrix, full,
                  siting, 0, h, w)
        _hip.call("irm_rgb_f32_to_yuv", _hip.ptr(frame), *operands(new, fmt, False), 2, 2, depth, upper, matrix, full,
                  siting, 0, h, w)
        assert all(torch.equal(o, n) for o, n in zip(old, new)) and bool((old[0] != 0).any())
    # the general functions and the 4:2:0 ones on the three old names
    assert torch.equal(yuv.yuv_to_rgb_device(planes, fmt), yuv.yuv420_to_rgb_device(planes, fmt))
    for o, n in zip(yuv.rgb_to_yuv420_device(frame, fmt), yuv.rgb_to_yuv_device(frame, fmt)):
        assert torch.equal(o, n)


# --------------------------------------------------------------------------- metrics
#: (fmt, H, W, (luma, planar chroma) pitch extras in samples, luma_only)
METRIC_CASES = [("i444", 7, 7, (0, 0), False), ("nv24", 23, 205, (0, 0), False), ("i444p12", 23, 205, (0, 0), False),
                ("p410", 7, 7, (10, 6), False), ("i422", 7, 14, (0, 0), False), ("nv16", 23, 404, (0, 0), False),
                ("p212", 23, 404, (8, 8), False), ("i422p10", 7, 14, (3, 5), False), ("i420p12", 14, 14, (0, 0), False),
                ("p012", 16, 30, (10, 6), False), ("i422p12", 23, 404, (0, 0), True), ("i444", 7, 7, (0, 0), True)]


@functools.lru_cache(maxsize=None)
def metric_pair(fmt, h, w):
    """(prediction planes, target planes, prediction codes, target codes), seeded by the case, never written: the
    target is the prediction plus noise of a few codes, clipped."""
    rng = np.random.default_rng(3000 + 11 * h + w)
    top = (1 << fm.LAYOUTS[fmt][3]) - 1
    pred = fm.random_planes(rng, fmt, h, w)
    pc = fm.codes_of(pred, fmt)
    tc = tuple(np.clip(c + rng.integers(-(top // 16), top // 16 + 1, c.shape), 0, top) for c in pc)
    return pred, fm.planes_of(*tc, fmt), pc, tc


@pytest.mark.parametrize("fmt,h,w,extras,luma_only", METRIC_CASES,
                         ids=["%s-%dx%d%s%s" % (f, h, w, "p" if e[0] else "", "-luma" if lo else "") for f, h, w, e, lo in METRIC_CASES])
def test_guard_bands_yuv_metrics(dev, fmt, h, w, extras, luma_only):
    """The planes between bands of zeros and then of ones (the pitch padding included): the result must not depend on
    them.  The outputs and the workspace, at exactly the header's minimum, between sentinels: all intact.  sse equals the
    integer sum, SSIM the host twin's within BOUND; identical planes give exactly 0 / 1.0; two calls are bitwise equal."""
    sw, sh, n, depth, upper = fm.LAYOUTS[fmt]
    pp, tp, pc, tc = metric_pair(fmt, h, w)
    tiles = lambda a, b: -(-(a - 6) // 16) * -(-(b - 6) // 192)                            # noqa: E731
    words = 2 * (tiles(h, w) + (0 if luma_only else 2 * tiles(h // sh, w // sw)))

    def place(planes, ex, fill):
        views = []
        for i, p in enumerate(planes[:1] if luma_only else planes):
            t = bits(p)
            row = int(np.prod(t.shape[1:]))
            extra = ex[0] if i == 0 else ex[1] * (2 if n == 2 else 1)
            _, view = pitched(tuple(t.shape), row + extra, t.dtype, dev, int_fill(t.dtype, fill))
            view.copy_(t)
            views.append(view)
        return views

    def run(fill, target=tp):
        vp, vt = place(pp, extras, fill), place(target, (extras[0] // 2, extras[1]), fill)
        outs = [sentinel_out((3,), dev, torch.int64), sentinel_out((3,), dev, torch.float64),
                sentinel_out((words,), dev, torch.float64)]
        (_, sse), (_, ssim), (_, ws) = outs
        _hip.call("irm_yuv_metrics", *operands(vp, fmt, luma_only), *operands(vt, fmt, luma_only), sw, sh, depth, upper,
                  int(luma_only), h, w, _hip.ptr(sse), _hip.ptr(ssim), _hip.ptr(ws), words)
        torch.cuda.synchronize()
        assert all(intact(buf, view) for buf, view in outs), "a store outside an output or the workspace"
        if luma_only:
            assert [int(v) for v in sse[1:]] == [sentinel(torch.int64)] * 2 and bool((ssim[1:] == sentinel(torch.float64)).all())
        return sse.cpu(), ssim.cpu()

    sse, ssim = two_fills(run)
    want = yuv.calculate_metrics_yuv(pp, tp, fmt, luma_only)
    for i in range(1 if luma_only else 3):
        assert int(sse[i]) == int(((pc[i] - tc[i]) ** 2).sum())
        print(f"{fmt} {h}x{w} component {i}: ssim device {float(ssim[i]):.17g} host {want[2 * i + 1]:.17g}")
        assert abs(float(ssim[i]) - want[2 * i + 1]) <= BOUND
    same_sse, same_ssim = run(0, target=pp)
    for i in range(1 if luma_only else 3):
        assert int(same_sse[i]) == 0 and float(same_ssim[i]) == 1.0
    # the public calls: twice, bitwise equal; PSNR from the exact error
    p_dev = tuple(bits(p).to(dev) for p in pp)
    t_dev = tuple(bits(p).to(dev) for p in tp)
    a, b = (yuv.frame_metrics_yuv_device(p_dev, t_dev, fmt, luma_only) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    m = yuv.calculate_metrics_yuv_device(p_dev, t_dev, fmt, luma_only)
    for i in range(1 if luma_only else 3):
        assert abs(m[2 * i] - want[2 * i]) <= 1e-9 and abs(m[2 * i + 1] - want[2 * i + 1]) <= BOUND
    same = yuv.calculate_metrics_yuv_device(p_dev, p_dev, fmt, luma_only)
    assert same[:2] == (float("inf"), 1.0) and (luma_only or same == (float("inf"), 1.0) * 3)


# --------------------------------------------------------------------------- the whole call
def composition(model, planes, dev, fmt, patch, overlap, pad8=False, **opts):
    """What run_model_inference_yuv is made of: the device conversion, the device pipeline on the float32 frame, and
    the numpy twin of the way back on the downloaded frame."""
    luma_only = opts.get("luma_only", False)
    up = tuple(bits(p).to(dev) for p in (planes[:1] if luma_only else planes))
    frame = yuv.yuv_to_rgb_device(up, fmt, **opts)
    out, _ = utils.tiled_forward_device(model, frame, patch, overlap, pad8, unit_range=True, out="float32",
                                        max_batch=getattr(model, "max_tiles_per_batch", 8))
    keep = tuple(p.copy() for p in planes) if luma_only else None
    return yuv.rgb_to_yuv_host(out.cpu().numpy(), fmt, out=keep, **opts)


@pytest.fixture(scope="module")
def colour(dev):
    return dncnn.DnCNN(3, 3, 64, 4, "R").load_synthetic(42).eval().to(dev)


@pytest.mark.parametrize("fmt,opts", [("p210", dict(full_range=True)), ("i444p12", dict(matrix="bt601", siting="center"))])
def test_whole_call_colour_dncnn(dev, fmt, opts):
    model = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    planes = fm.random_planes(np.random.default_rng(35), fmt, 32, 48)
    got, ms = utils.run_model_inference_yuv(model, planes, dev, fmt=fmt, patch_size=32, patch_overlap=8, **opts)
    want = composition(model, planes, dev, fmt, 32, 8, **opts)
    assert ms > 0 and len(got) == len(planes)
    low = (1 << fm.shift_of(fmt)) - 1
    for g, t, p in zip(got, want, planes):
        assert g.dtype == np.uint16 and g.shape == p.shape and np.array_equal(g, t) and int((g & low).max()) == 0
    assert not np.array_equal(got[0], planes[0]), "the model ran"


def test_whole_call_nv16_luma_only_gray_dncnn(dev):
    model = dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(42).eval().to(dev)
    planes = fm.random_planes(np.random.default_rng(36), "nv16", 32, 48)
    before = tuple(p.copy() for p in planes)
    got, _ = utils.run_model_inference_yuv(model, planes, dev, fmt="nv16", luma_only=True, patch_size=32, patch_overlap=8)
    want = composition(model, planes, dev, "nv16", 32, 8, luma_only=True)
    assert len(got) == 2 and got[1].shape == (32, 24, 2) and np.array_equal(got[1], before[1])
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0]) and not np.array_equal(got[0], before[0])
    assert np.array_equal(planes[0], before[0]), "the caller's Y plane is not written"


def test_whole_call_i422_super_resolution(dev):
    with open(os.path.join(GOLDEN, "mair_sr.json")) as f:
        cfg = json.load(f)["configs"]["light_x2"]
    model = mair.MaIR(**cfg).load_synthetic(42).eval().to(dev)
    planes = fm.random_planes(np.random.default_rng(37), "i422", 16, 24)
    got, _ = utils.run_model_inference_yuv(model, planes, dev, fmt="i422", patch_size=32, patch_overlap=8)
    assert [g.shape for g in got] == [(32, 48), (32, 24), (32, 24)] and all(g.dtype == np.uint8 for g in got)
    for g, t in zip(got, composition(model, planes, dev, "i422", 32, 8, pad8=True)):
        assert np.array_equal(g, t)


# --------------------------------------------------------------------------- stream and harness
CFG = dict(patch_size=32, patch_overlap=8)
KW = dict(task="denoising", subtask="gaussian", dataset="synthetic", model_name="DnCNN")


def test_stream_i422p10_equals_the_one_frame_calls(dev, colour):
    rng = np.random.default_rng(53)
    frames = [fm.random_planes(rng, "i422p10", 32, 48) for _ in range(5)]
    opts = dict(fmt="i422p10", matrix="bt601", siting="center")
    got = list(utils.run_model_inference_stream(colour, iter(frames), dev, frames_per_step=2, **opts, **CFG))
    assert len(got) == 5 and all(ms >= 0 for _, ms in got)
    for (g, _), f in zip(got, frames):
        want = utils.run_model_inference_yuv(colour, f, dev, **opts, **CFG)[0]
        assert isinstance(g, tuple) and len(g) == 3
        for a, b in zip(g, want):
            assert a.dtype == np.uint16 and a.shape == b.shape and np.array_equal(a, b)
        assert not np.array_equal(g[0], f[0]), "the model ran"


def test_harness_evaluate_yuv_i444(dev, colour):
    frames = [metric_pair("i444", 32, 40 + i)[:2] + (f"v{i}.yuv",) for i in range(3)]
    host = harness.evaluate_yuv(colour, iter(frames), dev, CFG, fmt="i444", metrics="host", **KW)
    devm = harness.evaluate_yuv(colour, iter(frames), dev, CFG, fmt="i444", **KW)
    assert devm["Failed"] == [] and host["Failed"] == []
    for key in harness.COLUMNS_YUV[6:10] + harness.COLUMNS_YUV[12:]:
        print(f"evaluate_yuv i444 {key}: device {devm[key]:.15f} host {host[key]:.15f}")
        assert math.isfinite(devm[key]) and abs(devm[key] - host[key]) <= 1e-9, key


def test_y4m_file_streamed_and_scored(dev, colour, tmp_path):
    """A Y4M file written, read back, streamed and scored through harness.y4m_pairs."""
    rng = np.random.default_rng(54)
    pairs = []
    for _ in range(3):
        clean_codes = [rng.integers(64, 940, s) for s in ((32, 48), (32, 24), (32, 24))]
        noisy_codes = [np.clip(c + rng.integers(-40, 41, c.shape), 0, 1023) for c in clean_codes]
        pairs.append((fm.planes_of(*noisy_codes, "i422p10"), fm.planes_of(*clean_codes, "i422p10")))
    noisy, clean = str(tmp_path / "noisy.y4m"), str(tmp_path / "clean.y4m")
    assert y4m.write_y4m(noisy, [p for p, _ in pairs], "i422p10", 25) == 3
    assert y4m.write_y4m(clean, [t for _, t in pairs], "i422p10", 25) == 3
    loader = harness.y4m_pairs(noisy, clean)
    assert (loader.fmt, loader.siting, loader.frames) == ("i422p10", "left", 3)
    for (a, b, name), (p, t) in zip(loader, pairs):
        assert all(np.array_equal(x, y) for x, y in zip(a, p)) and all(np.array_equal(x, y) for x, y in zip(b, t))
    streamed = list(utils.run_model_inference_stream(colour, iter(y4m.read_y4m(noisy)), dev, fmt=loader.fmt,
                                                     siting=loader.siting, frames_per_step=2, **CFG))
    row = harness.evaluate_yuv(colour, loader, dev, CFG, fmt=loader.fmt, siting=loader.siting, **KW)
    assert row["Failed"] == [] and math.isfinite(row["PSNR"]) and math.isfinite(row["SSIM_V"])
    scores = [yuv.calculate_metrics_yuv(g, t, "i422p10") for (g, _), (_, t) in zip(streamed, pairs)]
    assert abs(row["PSNR"] - np.mean([m.psnr_y for m in scores])) <= 1e-9
    assert abs(row["SSIM_U"] - np.mean([m.ssim_u for m in scores])) <= 1e-9
