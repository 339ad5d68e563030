"""The resize to any size on the GPU (csrc/resize_any.hip: irm_resize_taps, irm_unit_quantise) against the float64
statement utils.resize_host: float and quantised outputs for every kernel, frame type and channel count, bit identity
with irm_imresize_bicubic at its six factors, reproducibility and independence of K and of the tile width, overshoot,
guard bands and poison, the Resize stage of utils.run_model_chain, and the two full-size conversions."""
import numpy as np
import pytest
import torch

import guards
from guards import Guards, has_nan, two_fills
from irm_amd import _hip, dncnn, resize, synth, utils
from purity import check_uninitialised
from resize_checks import (Recorder, as_dtype, check_float, check_quantised_near_ties, checker, down, fp32_bound, up)

pytestmark = pytest.mark.gpu

KERNELS = ("bicubic", "lanczos3", "bilinear")
#: (72, 90) and (96, 60) shrink, (144, 180) enlarges, (40, 200) shrinks H and enlarges W, (13, 17) is a strong shrink
TARGETS = [dict(size=(72, 90)), dict(size=(144, 180)), dict(size=(40, 200)), dict(size=(96, 60)), dict(size=(13, 17)),
           dict(scale=0.75), dict(scale=1.5), dict(scale=0.3)]
#: from the 61 x 83 slice only: P = 37 / 33 bicubic, 55 / 48 lanczos3
SMALLEST = dict(size=(7, 11))


def source(golden, name):
    g = golden("sr_protocol")
    base, _, cut = name.partition("_")
    img = g[f"hr_{base}"]
    return np.ascontiguousarray(img[:61, :83]) if cut else img


# --------------------------------------------------------------------------- 1. against the host statement
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["random", "synth", "random_cut", "synth_cut"])
def test_float_and_quantised_vs_host(dev, golden, name, kernel):
    """hr_random (96 x 120), hr_synth (97 x 131) and their [:61, :83] slices; u8, u16 and f32; C = 3 and 1."""
    u8 = source(golden, name)
    targets = TARGETS + ([SMALLEST] if name.endswith("_cut") else [])
    worst = 0.0
    for tgt in targets:
        kw = dict(tgt, kernel=kernel)
        e = fp32_bound(u8.shape[0], u8.shape[1], kw)
        for kind in ("u8", "u16", "f32"):
            full = as_dtype(u8, kind)
            for frame in (full, np.ascontiguousarray(full[:, :, 1])):
                what = f"{name} {kernel} {tgt} {kind} C{1 if frame.ndim == 2 else 3}"
                want = utils.resize_host(frame, **kw)
                got = utils.resize_device(up(frame, dev), out="float", **kw)
                assert got.dim() == frame.ndim
                worst = max(worst, check_float(got.cpu().numpy(), want, e, what) / e)
                unit = utils.resize_device(up(frame, dev), out="unit", **kw).cpu().numpy()
                assert np.array_equal(unit, np.clip(got.cpu().numpy(), np.float32(0), np.float32(1))), what
                same = utils.resize_device(up(frame, dev), **kw)                  # out="same" is the default
                if kind == "f32":
                    assert same.dtype == torch.float32 and torch.equal(same, got), what
                else:
                    assert same.dtype == (torch.uint8 if kind == "u8" else torch.int16)
                    check_quantised_near_ties(down(same), want, e, what + " quantised")
    print(f"{name} {kernel}: worst error / bound {worst:.3f}")


def test_uint16_tensors_and_float_to_integer(dev, golden):
    u8 = source(golden, "synth_cut")
    u16 = as_dtype(u8, "u16")
    kw = dict(size=(40, 100), kernel="lanczos3")
    q = utils.resize_device(up(u16, dev), **kw)
    if hasattr(torch, "uint16"):
        q16 = utils.resize_device(up(u16, dev).view(torch.uint16), **kw)
        assert q16.dtype == torch.uint16 and np.array_equal(down(q16), down(q))
    # a float32 frame may ask for an integer type: the unit result under the store rule, the bits of the fused path
    f32 = as_dtype(u8, "f32")
    unit = utils.resize_device(up(f32, dev), out="unit", **kw).cpu().numpy()
    for out, peak, dt in (("uint8", 255.0, np.uint8), ("uint16", 65535.0, np.uint16)):
        got = down(utils.resize_device(up(f32, dev), out=out, **kw), dt)
        assert got.dtype == dt and np.array_equal(got, np.rint(unit * np.float32(peak)).astype(dt))
    from_u8 = utils.resize_device(up(u8, dev), out="unit", **kw)
    assert np.array_equal(down(utils.resize_device(from_u8, size=(40, 100), out="uint8")),
                          np.rint(utils.resize_device(from_u8, size=(40, 100), out="unit").cpu().numpy() * np.float32(255.0)))
    with pytest.raises(ValueError, match="float32 frames"):
        utils.resize_device(up(u8, dev), out="uint16", **kw)
    with pytest.raises(ValueError, match="shorter"):
        utils.resize_device(up(u8, dev), size=(6, 11), kernel="lanczos3")
    with pytest.raises(ValueError, match="share shape"):
        utils.resize_device([up(f32, dev), up(u8, dev)], scale=0.5)
    with pytest.raises(ValueError, match="more than the 128"):           # 1/40 with lanczos3: 242 taps
        utils.resize_device(torch.zeros(2000, 40, 3, dtype=torch.uint8, device=dev), size=(50, 40), kernel="lanczos3")


# --------------------------------------------------------------------------- 2. the old entry's bits
@pytest.mark.parametrize("scale", [0.5, 1.0 / 3.0, 0.25, 2, 3, 4])
def test_bit_identity_with_imresize_device(dev, golden, scale):
    hr = golden("sr_protocol")["hr_synth"]
    if scale > 1:
        hr = np.ascontiguousarray(hr[:40, :52])
    for kind in ("u8", "u16"):
        full = as_dtype(hr, kind)
        for frame in (full, np.ascontiguousarray(full[:, :, 1])):
            for out in ("float", "same"):
                old = utils.imresize_device(up(frame, dev), scale, out=out)
                new = utils.resize_device(up(frame, dev), scale=scale, out=out)
                assert old.dtype == new.dtype and old.shape == new.shape
                assert torch.equal(old, new), (scale, kind, frame.ndim, out, int((old != new).sum()))


# --------------------------------------------------------------------------- 3. reproducibility and independence
@pytest.mark.parametrize("kw", [dict(scale=0.3, kernel="lanczos3"), dict(size=(40, 200)), dict(scale=1.5, kernel="bilinear")])
def test_bitwise_alone_in_a_list_and_in_a_stack(dev, golden, kw):
    g = golden("sr_protocol")
    frames = [g["hr_random"], g["deg_random"], g["hr_random"][::-1].copy(), g["hr_random"][:, ::-1].copy()]
    for kind in ("u8", "f32"):
        devf = [up(as_dtype(f, kind), dev) for f in frames]
        for out in ("float", "same", "unit"):
            alone = [utils.resize_device(devf[1], out=out, **kw).cpu().numpy() for _ in range(2)]
            batch = [utils.resize_device(devf, out=out, **kw) for _ in range(2)]
            stack = [utils.resize_device(torch.stack(devf), out=out, **kw) for _ in range(2)]
            assert isinstance(batch[0], list) and len(batch[0]) == 4 and stack[0].shape[0] == 4
            for b in (alone[1], batch[0][1].cpu().numpy(), batch[1][1].cpu().numpy(), stack[0][1].cpu().numpy(),
                      stack[1][1].cpu().numpy()):
                assert np.array_equal(alone[0], b)
            assert not np.array_equal(alone[0], batch[0][0].cpu().numpy())


@pytest.mark.parametrize("ow", [1, 31, 32, 33, 129])
def test_tile_width_does_not_reach_the_values(dev, golden, monkeypatch, ow):
    """1 column (a frame narrower than any tile), 31 / 32 / 33 (a partial, a full and a started second tile of 32),
    129 (the widest tile plus one); the same bits when a smaller window makes the host pick a narrower tile."""
    u8 = source(golden, "synth_cut")
    kw = dict(size=(40, ow), kernel="bicubic", antialias=ow > 1)          # (83 -> 1 with antialiasing has more taps than columns)
    e = fp32_bound(61, 83, kw)
    wide = {}
    for kind in ("u8", "f32"):
        frame = as_dtype(u8, kind)
        for out in ("float", "same"):
            wide[kind, out] = utils.resize_device(up(frame, dev), out=out, **kw).cpu().numpy()
        check_float(wide[kind, "float"], utils.resize_host(frame, **kw), e, f"OW {ow} {kind}")
    _, iw = utils.resize_taps(83, ow, ow / 83, "bicubic", ow > 1)
    spans = {tow: resize.tile_span(iw, tow) for tow in resize.RESIZE_TOWS}
    tows = {resize._pick_tow(spans, 3)[0]}
    for budget in (8 * spans[32] * 12, 8 * spans[8] * 12):
        monkeypatch.setattr(resize, "RESIZE_WINDOW_BYTES", budget)
        tows.add(resize._pick_tow(spans, 3)[0])
        for (kind, out), want in wide.items():
            got = utils.resize_device(up(as_dtype(u8, kind), dev), out=out, **kw).cpu().numpy()
            assert np.array_equal(got, want), (ow, budget, kind, out)
    assert tows == ({128} if ow == 1 else {128, 32, 8} if ow == 129 else {128, 8}), tows


# --------------------------------------------------------------------------- 4. overshoot
def test_overshoot_is_clamped(dev):
    img = checker()
    kw = dict(scale=1.5, kernel="lanczos3")
    f = utils.resize_device(up(img, dev), out="float", **kw).cpu().numpy()
    assert f.shape == (45, 54, 3) and f.min() < -0.05 and f.max() > 1.05
    e = fp32_bound(30, 36, kw)
    check_float(f, utils.resize_host(img, **kw), e, "checker x1.5 lanczos3")
    u = utils.resize_device(up(img, dev), out="unit", **kw).cpu().numpy()
    assert u.min() == 0.0 and u.max() == 1.0 and np.array_equal(u, np.clip(f, np.float32(0), np.float32(1)))
    q = down(utils.resize_device(up(img, dev), **kw))
    assert q.min() == 0 and q.max() == 255
    check_quantised_near_ties(q, utils.resize_host(img, **kw), e, "checker x1.5 lanczos3 quantised")


# --------------------------------------------------------------------------- 5. guard bands and poison
def _tables(h, w, kw):
    oh, ow, sh, sw = utils.resize_plan(h, w, kw.get("size"), kw.get("scale"), kw["kernel"], True)
    wh, ih = utils.resize_taps(h, oh, sh, kw["kernel"])
    ww, iw = utils.resize_taps(w, ow, sw, kw["kernel"])
    spans = {tow: resize.tile_span(iw, tow) for tow in resize.RESIZE_TOWS}
    return oh, ow, wh, ih, ww, iw, spans


@pytest.mark.parametrize("kind,C", [("u8", 3), ("u16", 1), ("f32", 3), ("f32", 1)])
@pytest.mark.parametrize("kw,H,W", [(dict(size=(9, 70), kernel="bicubic"), 14, 19), (dict(size=(37, 8), kernel="lanczos3"), 20, 44),
                                    (dict(scale=1.5, kernel="bilinear"), 4, 5)])
def test_guard_bands_resize_taps(dev, kind, C, kw, H, W):
    """Frames, the four tables and the output between bands: "irm_resize_taps" called by name on K = 2 frames whose
    sides are near the tap counts (14 rows for 9 taps; 44 columns for 35; 4 x 5 for bilinear's 4 taps), with a partial
    last tile on both axes.  Integer frames and the index tables: two fills; float32 frames and the weights: NaN."""
    K = 2
    rng = np.random.default_rng(23)
    u8 = rng.integers(0, 256, size=(K, H, W, C)).astype(np.uint8)
    frames = as_dtype(u8, kind)
    oh, ow, wh, ih, ww, iw, spans = _tables(H, W, kw)
    tow, ncol = resize._pick_tow(spans, C)
    in_kind = {"u8": 0, "u16": 1, "f32": 2}[kind]
    qdt = {"u8": torch.uint8, "u16": torch.int16}.get(kind)

    def run(fill):
        res = []
        for out_kind in (1, 2, 0) if qdt else (1, 2):
            g = Guards(dev)
            out = g.out("out", (K, oh, ow, C), torch.float32 if out_kind else qdt)
            src = g.inp(up(frames, "cpu"), fill=None if kind == "f32" else fill)
            _hip.call("irm_resize_taps", _hip.ptr(src), in_kind, _hip.ptr(out), out_kind,
                      _hip.ptr(g.inp(torch.from_numpy(wh.astype(np.float32)))),
                      _hip.ptr(g.inp(torch.from_numpy(ih.astype(np.int32)), fill=fill)),
                      _hip.ptr(g.inp(torch.from_numpy(ww.astype(np.float32)))),
                      _hip.ptr(g.inp(torch.from_numpy(iw.astype(np.int32)), fill=fill)), K, H, W, C, oh, ow,
                      wh.shape[1], ww.shape[1], tow, ncol)
            g.check()
            res.append(out.cpu())
        return tuple(res)

    res = two_fills(run)
    assert not has_nan(res[0]) and not has_nan(res[1])
    assert not bool((res[0] == guards.SENTINEL).any()), "an output value was never written"
    e = fp32_bound(H, W, kw)
    want = np.stack([utils.resize_host(f, **kw) for f in frames])
    check_float(res[0].numpy(), want, e, f"guarded {kw} {kind} C{C}")
    assert np.array_equal(res[1].numpy(), np.clip(res[0].numpy(), np.float32(0), np.float32(1)))
    if qdt:
        check_quantised_near_ties(down(res[2]), want, e, f"guarded {kw} {kind} C{C} quantised")


@pytest.mark.parametrize("is_u16", [0, 1])
def test_guard_bands_unit_quantise(dev, is_u16):
    """n = 1000 = three full workgroups and a partial one; values below 0, above 1, exact ties and NaN-free."""
    n, peak = 1000, 65535.0 if is_u16 else 255.0
    x = np.random.default_rng(29).uniform(-0.25, 1.25, n).astype(np.float32)
    x[:4] = (np.float32(0.5) / np.float32(peak), np.float32(1.5) / np.float32(peak), 0.0, 1.0)
    g = Guards(dev)
    out = g.out("out", (n,), torch.int16 if is_u16 else torch.uint8)
    _hip.call("irm_unit_quantise", _hip.ptr(g.inp(torch.from_numpy(x))), _hip.ptr(out), is_u16, n)
    g.check()
    dt = np.uint16 if is_u16 else np.uint8
    want = np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(peak)).astype(dt)
    assert np.array_equal(down(out.cpu(), dt), want)


@pytest.mark.parametrize("kind,C", [("u8", 3), ("u16", 1), ("f32", 3)])
def test_resize_under_poison(dev, kind, C):
    u8 = np.random.default_rng(31).integers(0, 256, size=(2, 33, 47, C)).astype(np.uint8)
    stack = up(as_dtype(u8, kind), dev)
    for kw in (dict(size=(20, 70), kernel="lanczos3"), dict(scale=1.5)):
        for out in ("same", "float", "unit") + (("uint8", "uint16") if kind == "f32" else ()):
            check_uninitialised(None, lambda: utils.resize_device(stack, out=out, **kw).cpu(), f"resize {kw} {kind} {out}")


# --------------------------------------------------------------------------- 6. the chain
@pytest.fixture(scope="module")
def den(dev):
    return dncnn.DnCNN(3, 3, 64, 5, "R").load_synthetic(42).eval().to(dev)


CFG = {"patch_size": 32, "patch_overlap": 8}


def _model(den, frame, out, cfg=CFG):
    r = utils.model_route(den)
    return utils.tiled_forward_device(den, frame, cfg["patch_size"], cfg["patch_overlap"], r.pad8, None,
                                      max_batch=r.max_batch, unit_range=True, out=out)[0]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_chain_equals_the_composition(dev, den, dtype):
    rng = np.random.default_rng(37)
    img = rng.integers(0, 256, size=(40, 56, 3)).astype(np.uint8)
    if dtype == np.uint16:
        img = as_dtype(img, "u16")
    name = np.dtype(dtype).name
    frame = up(img, dev)
    # model, then to a size
    last = utils.Resize(size=(60, 84))
    got, ms = utils.run_model_chain([(den, CFG), last], img, dev)
    want = utils.resize_device(_model(den, frame, "float32"), size=(60, 84), out=name)
    assert got.dtype == dtype and got.shape == (60, 84, 3) and ms > 0 and np.array_equal(got, down(want, dtype))
    gotf, _ = utils.run_model_chain([(den, CFG), last], img, dev, out="float32")
    wantf = utils.resize_device(_model(den, frame, "float32"), size=(60, 84), out="unit")
    assert gotf.dtype == np.float32 and np.array_equal(gotf, wantf.cpu().numpy())
    # to a size, then the model
    got, _ = utils.run_model_chain([utils.Resize(scale=0.75), (den, CFG)], img, dev)
    want = _model(den, utils.resize_device(frame, scale=0.75, out="unit"), name)
    assert got.dtype == dtype and got.shape == (30, 42, 3) and np.array_equal(got, down(want, dtype))
    # a Resize between two models
    mid = utils.Resize(scale=1.5, kernel="lanczos3")
    got, _ = utils.run_model_chain([(den, CFG), mid, (den, CFG)], img, dev)
    f1 = utils.resize_device(_model(den, frame, "float32"), scale=1.5, kernel="lanczos3", out="unit")
    want = _model(den, f1, name)
    assert got.shape == (60, 84, 3) and np.array_equal(got, down(want, dtype))
    gotf, _ = utils.run_model_chain([(den, CFG), mid, (den, CFG)], img, dev, out="float32")
    assert np.array_equal(gotf, _model(den, f1, "float32").cpu().numpy())


def test_chain_of_resizes_alone(dev, golden):
    u8 = source(golden, "synth_cut")
    for img in (u8, as_dtype(u8, "u16"), as_dtype(u8, "f32"), np.ascontiguousarray(u8[:, :, :1])):
        kw = dict(size=(40, 100), kernel="lanczos3")
        got, _ = utils.run_model_chain([utils.Resize(**kw)], img, dev)
        want = utils.resize_device(up(img, dev), out="unit" if img.dtype == np.float32 else "same", **kw)
        assert got.dtype == img.dtype and np.array_equal(got, down(want, img.dtype))
        gotf, _ = utils.run_model_chain([utils.Resize(**kw)], img, dev, out="float32")
        assert gotf.dtype == np.float32
        assert np.array_equal(gotf, utils.resize_device(up(img, dev), out="unit", **kw).cpu().numpy())
    two, _ = utils.run_model_chain([utils.Resize(scale=0.5), utils.Resize(size=(61, 83), kernel="bilinear")], u8, dev)
    half = utils.resize_device(up(u8, dev), scale=0.5, out="unit")
    assert np.array_equal(two, down(utils.resize_device(half, size=(61, 83), kernel="bilinear", out="uint8")))


def test_middle_frame_is_float32_clamped_and_unrounded(dev):
    """The checker overshoots under lanczos3: the model after the Resize sees the float32 frame clamped to [0, 1], with
    values between the 255 levels, and the Resize after a model reads that model's unrounded frame."""
    img = checker()
    cfg = {"patch_size": 64, "patch_overlap": 16}                      # one tile: the frame itself
    rec = Recorder(0.5)
    rs = utils.Resize(scale=1.5, kernel="lanczos3")
    got, _ = utils.run_model_chain([rs, (rec, cfg), utils.Resize(size=(30, 36), kernel="bilinear")], img, dev)
    unit = utils.resize_device(up(img, dev), scale=1.5, kernel="lanczos3", out="unit").cpu()
    seen, = rec.seen
    assert seen.dtype == torch.float32 and torch.equal(seen[0], unit.permute(2, 0, 1))
    assert float(seen.min()) == 0.0 and float(seen.max()) == 1.0
    on_grid = (seen * 255.0 - torch.round(seen * 255.0)).abs() < 1e-4
    assert float(on_grid.float().mean()) < 0.9, "the frame between the stages was rounded to 255 levels"
    halved = _model(Recorder(0.5), unit.to(dev), "float32", cfg)        # the model stage on its own
    assert float(halved.max()) <= 0.5 + 1e-6
    want = utils.resize_device(halved, size=(30, 36), kernel="bilinear", out="uint8")
    assert got.dtype == np.uint8 and np.array_equal(got, down(want))


# --------------------------------------------------------------------------- 7. full size
@pytest.mark.parametrize("h,w,size,kernel", [(720, 1280, (1080, 1920), "bicubic"), (1080, 1920, (720, 1280), "lanczos3")])
def test_full_size_to_a_target(dev, h, w, size, kernel):
    _, img = synth.synth_image_pair(0, h, w, 3)
    kw = dict(size=size, kernel=kernel)
    e = fp32_bound(h, w, kw)
    want = utils.resize_host(img, **kw)
    got = utils.resize_device(up(img, dev), out="float", **kw)
    assert tuple(got.shape) == size + (3,)
    check_float(got.cpu().numpy(), want, e, f"{w}x{h} -> {size[1]}x{size[0]} {kernel}")
    check_quantised_near_ties(down(utils.resize_device(up(img, dev), **kw)), want, e, f"{kernel} full size quantised")
