"""PSNR / SSIM of float32 frames and of YUV 4:2:0 planes on the GPU (irm_frame_metrics_f32, irm_yuv420_metrics of
include/irm_hip_metrics.h, through utils.frame_metrics_f32_device / calculate_metrics_f32_device and
yuv.frame_metrics_yuv_device / calculate_metrics_yuv_device, and the harness rows built on them) against the float64
host statements utils.calculate_metrics and yuv.calculate_metrics_yuv.

The bound is the project's standing tolerance for device-against-host metrics, 1e-9 on SSIM and on PSNR
(frame_checks.metric_parity); squared errors of integer codes are compared as integers.  The SSIM tile is 16 rows x 192
values: the shapes are the smallest that reach one window, a ragged tile and a second tile on each axis, plus one 720p
frame."""
import functools
import math

import numpy as np
import pytest
import torch

import yuv_model
from irm_amd import _hip, dncnn, harness, utils, yuv

from guards import PAD, Guards, clean, int_fill, intact, sentinel, sentinel_out, two_fills

pytestmark = pytest.mark.gpu

BOUND = 1e-9
SEED = 41


def close(a, b):
    return (a == b) or abs(a - b) <= BOUND


# =========================================================================== float32 frames
F32_SHAPES = [(7, 7, 1), (7, 7, 3), (7, 300, 1), (13, 1001, 3), (40, 210, 3), (40, 210), (720, 1280, 3)]
F32_CONTENTS = ("noise", "near", "wide", "signed")


@functools.lru_cache(maxsize=None)
def f32_pair(shape, content):
    """(prediction, target, data_range or None) of a case, seeded by its shape, made once and never written."""
    rng = np.random.default_rng(SEED + 13 * shape[0] + shape[1] + F32_CONTENTS.index(content))
    if content == "noise":                                  # uniform noise in [0, 1], the two frames unrelated
        pred, tgt, dr = rng.random(shape), rng.random(shape), None
    elif content == "near":                                 # target + N(0, 0.02), clipped
        tgt = rng.random(shape)
        pred, dr = np.clip(tgt + rng.normal(0, 0.02, shape), 0, 1), None
    elif content == "wide":                                 # values in [0, 7.5] with data_range 7.5
        tgt = rng.random(shape) * 7.5
        pred, dr = np.clip(tgt + rng.normal(0, 0.15, shape), 0, 7.5), 7.5
    else:                                                   # values in [-0.25, 0.9] with the default range
        tgt = rng.uniform(-0.25, 0.9, shape)
        pred, dr = np.clip(tgt + rng.normal(0, 0.05, shape), -0.25, 0.9), None
    return pred.astype(np.float32), tgt.astype(np.float32), dr


def f32_parity(pred, tgt, dr, dev, what):
    ph, sh = utils.calculate_metrics(pred, tgt, dr)
    pd, sd = utils.calculate_metrics_f32_device(torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev), dr)
    print(f"{what}: |dSSIM| {abs(sd - sh):.3e}, |dPSNR| {0.0 if pd == ph else abs(pd - ph):.3e} (SSIM {sd:.12f}, PSNR {pd:.9f})")
    assert math.isfinite(sd) and abs(sd - sh) <= BOUND, (what, sd, sh)
    assert close(pd, ph), (what, pd, ph)
    return pd, sd


@pytest.mark.parametrize("content", F32_CONTENTS)
@pytest.mark.parametrize("shape", F32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_f32_parity_with_the_host(dev, shape, content):
    pred, tgt, dr = f32_pair(shape, content)
    pd, sd = f32_parity(pred, tgt, dr, dev, f"f32 {shape} {content}")
    assert math.isfinite(pd) and -1.0 <= sd < 1.0


@pytest.mark.parametrize("shape", [(7, 7, 1), (13, 1001, 3), (40, 210, 3), (40, 212), (64, 256, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_f32_identical_frames_are_exact(dev, shape):
    """SSE == 0.0, SSIM == 1.0 exactly and PSNR inf for identical frames: random, wide-range, flat and black ones."""
    rng = np.random.default_rng(SEED + shape[1])
    frames = [(rng.random(shape).astype(np.float32), None), ((rng.random(shape) * 7.5).astype(np.float32), 7.5),
              (rng.uniform(-0.25, 0.9, shape).astype(np.float32), None), (np.full(shape, 0.37, np.float32), None),
              (np.zeros(shape, np.float32), None), (np.full(shape, 1.0, np.float32), 1e-3)]
    for a, dr in frames:
        x, y = torch.from_numpy(a).to(dev), torch.from_numpy(a.copy()).to(dev)
        sse, ssim = utils.frame_metrics_f32_device([x], [y], 1.0 if dr is None else dr)
        assert sse.dtype == ssim.dtype == torch.float64 and sse.shape == ssim.shape == (1,)
        assert float(sse[0]) == 0.0 and float(ssim[0]) == 1.0, (shape, dr, float(sse[0]), float(ssim[0]))
        assert utils.calculate_metrics_f32_device(x, y, dr) == (float("inf"), 1.0)


@pytest.mark.parametrize("shape", [(13, 23, 3), (40, 210)], ids=lambda s: "x".join(map(str, s)))
def test_f32_degenerate_frames_stay_finite_and_close(dev, shape):
    """Two different constants, all-zero against tiny noise, a ramp against the ramp + 2^-20."""
    rng = np.random.default_rng(SEED)
    ramp = np.broadcast_to(np.linspace(0, 1, shape[1], dtype=np.float32).reshape((1, -1) + (1,) * (len(shape) - 2)), shape).copy()
    pairs = {"constants": (np.full(shape, 0.25, np.float32), np.full(shape, 0.75, np.float32)),
             "zero-vs-tiny": (np.zeros(shape, np.float32), (rng.random(shape) * 1e-6).astype(np.float32)),
             "ramp": (ramp, ramp + np.float32(2.0 ** -20))}
    for name, (pred, tgt) in pairs.items():
        pd, sd = f32_parity(pred, tgt, None, dev, f"f32 {shape} {name}")
        assert math.isfinite(pd) and math.isfinite(sd)


def test_f32_results_do_not_depend_on_k_or_on_the_call(dev):
    """K = 3 frames in one call equal three single calls bit for bit, and a repeated call repeats; HW1 is HW; a
    non-contiguous frame is made contiguous."""
    preds = [torch.from_numpy(f32_pair((40, 210, 3), c)[0]).to(dev) for c in ("noise", "near", "signed")]
    tgts = [torch.from_numpy(f32_pair((40, 210, 3), c)[1]).to(dev) for c in ("noise", "near", "signed")]
    sse, ssim = utils.frame_metrics_f32_device(preds, tgts)
    again = utils.frame_metrics_f32_device(preds, tgts)
    assert torch.equal(sse.view(torch.int64), again[0].view(torch.int64))
    assert torch.equal(ssim.view(torch.int64), again[1].view(torch.int64))
    for k in range(3):
        s1, q1 = utils.frame_metrics_f32_device(preds[k:k + 1], tgts[k:k + 1])
        assert torch.equal(s1.view(torch.int64), sse[k:k + 1].view(torch.int64)), k
        assert torch.equal(q1.view(torch.int64), ssim[k:k + 1].view(torch.int64)), k
    grey_p, grey_t = preds[0][:, :, 0], tgts[0][:, :, 0]                   # strided views
    a = utils.frame_metrics_f32_device([grey_p], [grey_t])
    b = utils.frame_metrics_f32_device([grey_p.contiguous()[:, :, None]], [grey_t.contiguous()[:, :, None]])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ph, sh = utils.calculate_metrics(grey_p.cpu().numpy(), grey_t.cpu().numpy())
    assert abs(float(a[1][0]) - sh) <= BOUND


@pytest.mark.parametrize("H,W,C", [(7, 7, 1), (13, 23, 3), (13, 72, 3)])
def test_guard_bands_frame_metrics_f32(dev, H, W, C):
    """The frames between bands of NaN, the outputs and the workspace between sentinels, the workspace at exactly the
    header's minimum; K = 2.  13 x 72 x 3 moves in 16-byte pieces (two tiles, the last piece of a tile row reaches past
    the values the tile needs), the two others element by element."""
    K = 2
    rng = np.random.default_rng(SEED + W)
    tgt = rng.random((K, H, W, C)).astype(np.float32)
    pred = np.clip(tgt + rng.normal(0, 0.05, tgt.shape), 0, 1).astype(np.float32)
    words = 2 * K * -(-(H - 6) // 16) * -(-(W - 6) // (192 // C))
    g = Guards(dev)
    sse, ssim, ws = g.out("sse", (K,), torch.float64), g.out("ssim", (K,), torch.float64), g.out("ws", (words,), torch.float64)
    _hip.call("irm_frame_metrics_f32", _hip.ptr(g.inp(torch.from_numpy(pred))), _hip.ptr(g.inp(torch.from_numpy(tgt))),
              K, H, W, C, 1.0, _hip.ptr(sse), _hip.ptr(ssim), _hip.ptr(ws), words)
    g.check()
    sse, ssim = clean(sse), clean(ssim)
    for k in range(K):
        p, t = (a[k] if C == 3 else a[k, :, :, 0] for a in (pred, tgt))
        want = float(((p.astype(np.float64) - t.astype(np.float64)) ** 2).sum())
        assert abs(float(sse[k]) - want) <= 1e-12 * want
        assert abs(float(ssim[k]) - utils.calculate_metrics(p, t)[1]) <= BOUND


# =========================================================================== YUV 4:2:0 planes
FORMATS = ("i420", "nv12", "p010")


def bits(a: np.ndarray) -> torch.Tensor:
    """A host plane as the tensor the device holds: uint16 as its int16 bit pattern."""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def pitched(shape, extra, dtype, dev, fill):
    """(buf, view): a plane of `shape` ([rows][cols] or [rows][cols][2]) whose rows lie `extra` samples further apart
    than they are long, in the middle of a buffer that holds `fill` everywhere, the pitch padding included."""
    row = int(np.prod(shape[1:]))
    pitch = row + extra
    n = (shape[0] - 1) * pitch + row
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    strides = (pitch, 1) if len(shape) == 2 else (pitch, 2, 1)
    return buf, buf.as_strided(shape, strides, PAD)


def place(planes, extras, dev, fill=-1):
    """Host planes as pitched device views (extras: samples added to the luma and to the chroma pitch) of buffers whose
    filler has every bit set: 0xFF / 0xFFFF, so that a read outside [H][W] changes the result."""
    views = []
    for i, p in enumerate(planes):
        t = bits(p)
        _, view = pitched(tuple(t.shape), extras[min(i, 1)], t.dtype, dev, int_fill(t.dtype, fill))
        view.copy_(t)
        views.append(view)
    return tuple(views)


@functools.lru_cache(maxsize=None)
def yuv_pair(fmt, h, w, low_bits=False):
    """(prediction planes, target planes, the integer codes of both) of a case, made once: the prediction is the target
    plus noise of a few codes.  low_bits: random low six bits in every P010 word."""
    rng = np.random.default_rng(SEED + 5 * h + w)
    top = 1023 if fmt == "p010" else 255
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    tgt = [rng.integers(0, top + 1, s) for s in shapes]
    pred = [np.clip(t + rng.integers(-12, 13, t.shape) * (top // 255), 0, top) for t in tgt]
    pp, tp = yuv_model.planes_of(*pred, fmt), yuv_model.planes_of(*tgt, fmt)
    if low_bits:
        pp = tuple(p | rng.integers(0, 64, p.shape).astype(np.uint16) for p in pp)
        tp = tuple(p | rng.integers(0, 64, p.shape).astype(np.uint16) for p in tp)
    return pp, tp, pred, tgt


def yuv_parity(pred_dev, tgt_dev, pred_host, tgt_host, codes, fmt, what, luma_only=False):
    """Squared errors equal as integers, SSIM and PSNR within the bound of the numpy twin; returns the device tensors."""
    want = yuv.calculate_metrics_yuv(pred_host, tgt_host, fmt, luma_only)
    sse, ssim = yuv.frame_metrics_yuv_device(pred_dev, tgt_dev, fmt, luma_only)
    assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and sse.shape == ssim.shape == (3,)
    got = yuv.calculate_metrics_yuv_device(pred_dev, tgt_dev, fmt, luma_only)
    assert isinstance(got, yuv.YuvMetrics)
    for i, (p, t) in enumerate(zip(*codes)):
        if luma_only and i:
            assert math.isnan(got[2 * i]) and math.isnan(got[2 * i + 1]) and math.isnan(want[2 * i])
            continue
        assert int(sse[i]) == int(((p.astype(np.int64) - t.astype(np.int64)) ** 2).sum()), (what, i)
        assert float(ssim[i]) == got[2 * i + 1]
        print(f"{what} {'YUV'[i]}: |dSSIM| {abs(got[2 * i + 1] - want[2 * i + 1]):.3e}, PSNR {got[2 * i]:.9f} vs {want[2 * i]:.9f}")
        assert abs(got[2 * i + 1] - want[2 * i + 1]) <= BOUND, (what, i, got, want)
        assert close(got[2 * i], want[2 * i]), (what, i, got, want)
    return sse, ssim


@pytest.mark.parametrize("h,w", [(14, 14), (16, 30), (46, 400)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_yuv_parity_with_the_host(dev, fmt, h, w):
    """Dense planes, then row-pitched views (Y pitch W + 10, chroma pitch + 6; the prediction's W + 4 and + 2) of
    buffers filled with 0xFF / 0xFFFF: the same result bit for bit.  P010 with random low bits gives the result of
    the cleared words; luma_only leaves the chroma fields NaN and gives the Y of the full call bit for bit."""
    pp, tp, pc, tc = yuv_pair(fmt, h, w)
    dense = yuv_parity(tuple(bits(p).to(dev) for p in pp), tuple(bits(p).to(dev) for p in tp), pp, tp, (pc, tc), fmt,
                       f"{fmt} {h}x{w}")
    views_p, views_t = place(pp, (4, 2), dev), place(tp, (10, 6), dev)
    assert views_p[0].stride(0) == w + 4 and views_t[0].stride(0) == w + 10 and not views_t[1].is_contiguous()
    pit = yuv_parity(views_p, views_t, pp, tp, (pc, tc), fmt, f"{fmt} {h}x{w} pitched")
    assert torch.equal(dense[0], pit[0]) and torch.equal(dense[1].view(torch.int64), pit[1].view(torch.int64))
    lo = yuv_parity(views_p[:1], views_t, pp, tp, (pc, tc), fmt, f"{fmt} {h}x{w} luma", luma_only=True)
    assert int(lo[0][0]) == int(dense[0][0]) and torch.equal(lo[1][:1].view(torch.int64), dense[1][:1].view(torch.int64))
    assert int(lo[0][1]) == int(lo[0][2]) == 0 and bool(torch.isnan(lo[1][1:]).all())
    if fmt == "p010":
        np_, nt, _, _ = yuv_pair(fmt, h, w, True)
        assert any((a != b).any() for a, b in zip(np_, pp))
        noisy = yuv_parity(place(np_, (10, 6), dev), place(nt, (4, 2), dev), np_, nt, (pc, tc), fmt, f"{fmt} {h}x{w} low bits")
        assert torch.equal(dense[0], noisy[0]) and torch.equal(dense[1].view(torch.int64), noisy[1].view(torch.int64))
        as_u16 = yuv.frame_metrics_yuv_device(tuple(torch.from_numpy(p).to(dev) for p in pp),
                                              tuple(torch.from_numpy(p).to(dev) for p in tp), fmt)
        assert as_u16[0].dtype == torch.int64 and torch.equal(dense[0], as_u16[0])
        assert torch.equal(dense[1].view(torch.int64), as_u16[1].view(torch.int64)), "uint16 tensors and their int16 bits"


def test_yuv_parity_720p_nv12(dev):
    pp, tp, pc, tc = yuv_pair("nv12", 720, 1280)
    yuv_parity(tuple(bits(p).to(dev) for p in pp), tuple(bits(p).to(dev) for p in tp), pp, tp, (pc, tc), "nv12", "nv12 720p")


@pytest.mark.parametrize("h,w", [(16, 30), (46, 400), (48, 416)])
def test_yuv_nv12_and_i420_of_the_same_samples_agree_bit_for_bit(dev, h, w):
    """(48 x 416: the planar chroma planes of 24 x 208 move in 16-byte pieces, the interleaved ones sample by sample.)"""
    _, _, pc, tc = yuv_pair("i420", h, w)
    res = []
    for fmt in ("i420", "nv12"):
        pp, tp = yuv_model.planes_of(*pc, fmt), yuv_model.planes_of(*tc, fmt)
        res.append(yuv_parity(tuple(bits(p).to(dev) for p in pp), tuple(bits(p).to(dev) for p in tp), pp, tp, (pc, tc),
                              fmt, f"{fmt} {h}x{w}"))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1].view(torch.int64), res[1][1].view(torch.int64))


@pytest.mark.parametrize("fmt,h,w", [("p010", 14, 14), ("p010", 46, 400), ("nv12", 14, 14), ("i420", 46, 400)])
def test_yuv_bound_reaching_frames(dev, fmt, h, w):
    """Every code at its maximum against all-zero planes and against itself (P010: (49 x 1023)^2 does not fit 32 bits,
    so this is where a 32-bit window moment overflows), and random codes near the maximum.  Identical frames give SSIM
    exactly 1.0, a squared error of 0 and PSNR inf."""
    top = 1023 if fmt == "p010" else 255
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    full, zero = [np.full(s, top) for s in shapes], [np.zeros(s, np.int64) for s in shapes]
    rng = np.random.default_rng(SEED + h)
    high = [rng.integers(top - top // 8, top + 1, s) for s in shapes]
    up = lambda codes: tuple(bits(p).to(dev) for p in yuv_model.planes_of(*codes, fmt))      # noqa: E731
    for name, a, b in (("max-vs-zero", full, zero), ("zero-vs-max", zero, full), ("high-vs-max", high, full)):
        sse, _ = yuv_parity(up(a), up(b), yuv_model.planes_of(*a, fmt), yuv_model.planes_of(*b, fmt), (a, b), fmt,
                            f"{fmt} {h}x{w} {name}")
        if name != "high-vs-max":
            assert [int(v) for v in sse] == [top * top * s[0] * s[1] for s in shapes]
    for a in (full, zero, high):
        sse, ssim = yuv.frame_metrics_yuv_device(up(a), up(a), fmt)
        assert [int(v) for v in sse] == [0, 0, 0] and [float(v) for v in ssim] == [1.0, 1.0, 1.0]
        m = yuv.calculate_metrics_yuv_device(up(a), up(a), fmt)
        assert m == (float("inf"), 1.0) * 3


def test_yuv_luma_agrees_with_the_integer_frame_metric(dev):
    """The Y result of a contiguous 8-bit frame: the squared error of calculate_metrics_device's kernel on that plane
    as an HW frame, and an SSIM within the bound of it."""
    pp, tp, _, _ = yuv_pair("nv12", 46, 400)
    p_dev, t_dev = tuple(bits(p).to(dev) for p in pp), tuple(bits(p).to(dev) for p in tp)
    sse, ssim = yuv.frame_metrics_yuv_device(p_dev, t_dev, "nv12")
    sse_f, ssim_f = utils.frame_metrics_device([p_dev[0]], [t_dev[0]])
    assert int(sse[0]) == int(sse_f[0]) and abs(float(ssim[0]) - float(ssim_f[0])) <= BOUND
    got = yuv.calculate_metrics_yuv_device(p_dev, t_dev, "nv12")
    pf, sf = utils.calculate_metrics_device(p_dev[0], t_dev[0])
    assert close(got.psnr_y, pf) and abs(got.ssim_y - sf) <= BOUND


def test_yuv_device_refusals(dev):
    pp, tp, _, _ = yuv_pair("nv12", 16, 30)
    p_dev = tuple(bits(p).to(dev) for p in pp)
    with pytest.raises(ValueError, match="device"):
        yuv.frame_metrics_yuv_device(p_dev, tuple(bits(p) for p in tp), "nv12")
    with pytest.raises(ValueError, match="another"):
        yuv.frame_metrics_yuv_device(p_dev, tuple(bits(p).to(dev) for p in yuv_pair("nv12", 14, 14)[1]), "nv12")
    small = tuple(torch.zeros(s, dtype=torch.uint8, device=dev) for s in ((12, 30), (6, 15, 2)))
    with pytest.raises(ValueError, match="at least 14"):
        yuv.frame_metrics_yuv_device(small, small, "nv12")


@pytest.mark.parametrize("luma_only", [False, True], ids=["yuv", "luma"])
@pytest.mark.parametrize("h,w,extras", [(14, 14, (0, 0)), (16, 30, (10, 6)), (32, 64, (0, 0))], ids=["14x14", "16x30p", "32x64"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_guard_bands_yuv420_metrics(dev, fmt, h, w, extras, luma_only):
    """The planes between bands of zeros and then of ones (the pitch padding included): the result must not depend on
    them.  The outputs and the workspace, at exactly the header's minimum, between sentinels: all intact, and with
    luma_only entries 1 and 2 of the outputs are not written.  (32 x 64 dense: every plane of "i420" moves in 16-byte
    pieces.)"""
    pp, tp, pc, tc = yuv_pair(fmt, h, w)
    tiles = lambda a, b: -(-(a - 6) // 16) * -(-(b - 6) // 192)                            # noqa: E731
    words = 2 * (tiles(h, w) + (0 if luma_only else 2 * tiles(h // 2, w // 2)))

    def operands(views):
        y = views[0]
        if luma_only:
            return _hip.ptr(y), None, None, 1, y.stride(0), 0
        if fmt == "i420":
            return _hip.ptr(y), _hip.ptr(views[1]), _hip.ptr(views[2]), 1, y.stride(0), views[1].stride(0)
        uv = views[1]
        return _hip.ptr(y), _hip.ptr(uv[:, :, 0]), _hip.ptr(uv[:, :, 1]), 2, y.stride(0), uv.stride(0)

    def run(fill):
        vp, vt = place(pp, extras, dev, fill), place(tp, (extras[0] // 2, extras[1]), dev, fill)
        outs = [sentinel_out((3,), dev, torch.int64), sentinel_out((3,), dev, torch.float64),
                sentinel_out((words,), dev, torch.float64)]
        (_, sse), (_, ssim), (_, ws) = outs
        _hip.call("irm_yuv420_metrics", *operands(vp), *operands(vt), yuv_model.DEPTH[fmt], int(fmt == "p010"),
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
        assert abs(float(ssim[i]) - want[2 * i + 1]) <= BOUND


# =========================================================================== harness
CFG = dict(patch_size=32, patch_overlap=8)
KW = dict(task="denoising", subtask="gaussian", dataset="synthetic", model_name="DnCNN")


@pytest.fixture(scope="module")
def colour(dev):
    return dncnn.DnCNN(3, 3, 64, 4, "R").load_synthetic(42).eval().to(dev)


def test_harness_evaluate_scores_float32_frames_on_the_device(dev, colour, monkeypatch):
    rng = np.random.default_rng(SEED)
    pairs = []
    for i in range(3):
        tgt = rng.random((48, 64, 3)).astype(np.float32)
        pairs.append((np.clip(tgt + rng.normal(0, 0.05, tgt.shape), 0, 1).astype(np.float32), tgt, f"f{i}.npy"))
    seen = []
    inner = harness.calculate_metrics_f32_device

    def spy(pred_dev, target_dev, data_range=None):
        seen.append(pred_dev.cpu().numpy())
        assert pred_dev.dtype == torch.float32 and data_range is None
        return inner(pred_dev, target_dev, data_range)
    monkeypatch.setattr(harness, "calculate_metrics_f32_device", spy)
    host = harness.evaluate(colour, iter(pairs), dev, CFG, **KW)
    assert not seen
    devm = harness.evaluate(colour, iter(pairs), dev, CFG, metrics="device", **KW)
    assert len(seen) == 3 and devm["Failed"] == [] and host["Failed"] == []
    for key in ("PSNR", "SSIM", "Std_PSNR", "Std_SSIM"):
        print(f"evaluate float32 {key}: device {devm[key]:.12f} host {host[key]:.12f}")
        assert math.isfinite(devm[key]) and abs(devm[key] - host[key]) <= BOUND, key
    for (inp, _, _), got in zip(pairs, seen):
        want = utils.get_model_prediction(colour, inp, dev, **CFG)[0]
        assert want.dtype == np.float32 and np.array_equal(got, want)
    # mixed pairs keep raising: reported per frame, or propagated with skip_failed off
    mixed = [(pairs[0][0], (pairs[0][1] * 255).astype(np.uint8), "mixed.npy")]
    row = harness.evaluate(colour, iter(mixed), dev, CFG, metrics="device", **KW)
    assert [n for n, _ in row["Failed"]] == ["mixed.npy"]
    with pytest.raises(ValueError):
        harness.evaluate(colour, iter([((pairs[0][0] * 255).astype(np.uint8), pairs[0][1], "m2")]), dev, CFG,
                         metrics="device", skip_failed=False, **KW)


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_harness_evaluate_yuv(dev, colour, fmt, monkeypatch):
    frames = []
    for i in range(3):
        pp, tp, _, _ = yuv_pair(fmt, 48, 64 + 2 * i)
        frames.append((pp, tp, f"v{i}.yuv"))
    seen = []
    inner = yuv.calculate_metrics_yuv_device

    def spy(pred_dev, target_dev, f, luma_only=False):
        seen.append(tuple(utils.to_host(p.contiguous()) for p in pred_dev))
        return inner(pred_dev, target_dev, f, luma_only)
    monkeypatch.setattr(yuv, "calculate_metrics_yuv_device", spy)
    opts = dict(fmt=fmt, matrix="bt601", full_range=True)
    host = harness.evaluate_yuv(colour, iter(frames), dev, CFG, metrics="host", **opts, **KW)
    assert not seen
    devm = harness.evaluate_yuv(colour, iter(frames), dev, CFG, **opts, **KW)
    assert len(seen) == 3 and devm["Failed"] == [] and set(harness.COLUMNS_YUV) <= set(devm)
    for key in harness.COLUMNS_YUV[6:10] + harness.COLUMNS_YUV[12:]:
        print(f"evaluate_yuv {fmt} {key}: device {devm[key]:.12f} host {host[key]:.12f}")
        assert math.isfinite(devm[key]) and abs(devm[key] - host[key]) <= BOUND, key
    assert devm["Avg_Time_ms"] > 0 and devm["Model_Params"] == host["Model_Params"] > 0
    for (pp, _, _), got in zip(frames, seen):
        want = utils.run_model_inference_yuv(colour, pp, dev, **opts, **CFG)[0]
        assert len(got) == len(want) == 2
        for g, t in zip(got, want):
            assert g.dtype == t.dtype and np.array_equal(g, t)
        assert not np.array_equal(want[0], pp[0]), "the model ran"
    # a frame that raises is reported and the rest are kept
    odd = (yuv_pair(fmt, 48, 64)[0], yuv_pair(fmt, 48, 66)[1], "odd.yuv")
    part = harness.evaluate_yuv(colour, iter([frames[0], odd, frames[1]]), dev, CFG, **opts, **KW)
    assert [n for n, _ in part["Failed"]] == ["odd.yuv"] and math.isfinite(part["PSNR"])
    two = harness.evaluate_yuv(colour, iter(frames[:2]), dev, CFG, **opts, **KW)
    assert part["PSNR"] == two["PSNR"] and part["SSIM_V"] == two["SSIM_V"]
    with pytest.raises(ValueError):
        harness.evaluate_yuv(colour, iter([odd]), dev, CFG, skip_failed=False, **opts, **KW)
