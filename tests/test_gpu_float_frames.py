"""Float32 frames and model chains on the device pipeline: irm_frame_minmax_f32, irm_tile_extract_f32 and
irm_window_blend_f32 (include/irm_hip_frames.h) bit-exact against the numpy oracle of the reference's loop
(oracle/tiler_ref.py), the float path against the uint8 path, the public calls and utils.run_model_chain.

Every comparison is exact: the kernels restate the reference's float32 operation order, and min / max do not depend
on the order of a reduction."""
import json
import os

import numpy as np
import pytest
import torch

from irm_amd import _hip, deblurganv2, dncnn, mair, utils
from oracle import tiler_ref

from guards import banded, has_nan, intact, sentinel_out

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

#: (h, w, c, ps, ov, pad8, sigma)
CASES = [
    (100, 136, 3, 64, 16, True, None),
    (75, 61, 3, 50, 10, True, 25),            # tiles 50x50 -> padded 56x56, noise path
    (150, 210, 1, 64, 16, False, 15),
    (40, 90, 3, 64, 16, True, None),          # image shorter than the patch
    (64, 64, 3, None, 32, False, None),
    (90, 70, 6, 64, 16, True, None),          # six channels in, three out
]
#: max below 1 (the result is still multiplied by it), max above 1 (the frame is divided by it), a negative lower bound
RANGES = [(0.0, 0.8), (0.0, 7.5), (-0.25, 0.9)]


class Replay(torch.nn.Module):
    """Stands in for a model on either side: records the tiles it is given and returns canned predictions, plus
    `mix` times the first channels of its input (0 or a power of two: the product is exact, the sum is one IEEE
    addition, so the CPU oracle and the GPU agree to the bit)."""

    def __init__(self, preds, mix=0.0):
        super().__init__()
        self.preds, self.mix, self.seen, self.i = preds, mix, [], 0

    def forward(self, t):
        self.seen.append(t.detach().cpu().clone())
        n = t.shape[0]
        out = self.preds[self.i:self.i + n].to(t.device)
        self.i += n
        if self.mix:
            out = out + self.mix * t[:, :out.shape[1], :out.shape[2], :out.shape[3]]
        return out


def geometry(h, w, c, ps, ov, pad8):
    """(number of tiles, padded tile height, padded tile width) of the reference's loop."""
    ps_eff = min(ps, max(h, w)) if ps else max(h, w)
    th, tw = min(ps_eff, h), min(ps_eff, w)
    ph = (th // 8 + 1) * 8 if (pad8 and th % 8) else th
    pw = (tw // 8 + 1) * 8 if (pad8 and tw % 8) else tw
    nt = len(tiler_ref.tile_origins(h, ps_eff, ov)) * len(tiler_ref.tile_origins(w, ps_eff, ov)) if ps else 1
    return nt, ph, pw


def canned(rng, h, w, c, ps, ov, pad8):
    nt, ph, pw = geometry(h, w, c, ps, ov, pad8)
    return torch.from_numpy(rng.uniform(-0.2, 1.2, size=(nt, min(3, c), ph, pw)).astype(np.float32))


def oracle_run(preds, img, ps, ov, pad8, sigma, mix=0.0):
    """(result, tiles) of oracle/tiler_ref.py with a Replay on the CPU."""
    rep = Replay(preds, mix)
    ref = tiler_ref.tiled_inference(rep, img, patch_size=ps, patch_overlap=ov, need_degradation=sigma is not None,
                                    noise_level=sigma, pad=tiler_ref.reflect_pad8 if pad8 else None)
    return ref, torch.cat(rep.seen)


def float_frame(rng, shape, lo, hi):
    img = rng.uniform(lo, hi, size=shape).astype(np.float32)
    img.flat[0], img.flat[-1] = lo, hi
    return img


def u8_frame(rng, shape):
    img = rng.integers(0, 256, size=shape).astype(np.uint8)
    img.flat[0], img.flat[-1] = 0, 255
    return img


# --------------------------------------------------------------------------- 1. tiler vs the oracle
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("h,w,c,ps,ov,pad8,sigma", CASES)
def test_float_tiler_bit_exact_vs_oracle(dev, h, w, c, ps, ov, pad8, sigma, lo, hi):
    rng = np.random.default_rng(5)
    img = float_frame(rng, (h, w, c), lo, hi)
    preds = canned(rng, h, w, c, ps, ov, pad8)
    ref, tiles_ref = oracle_run(preds, img, ps, ov, pad8, sigma)
    assert ref.dtype == np.float32
    rep = Replay(preds)
    out, sse = utils.tiled_forward_device(rep, torch.from_numpy(img.copy()).to(dev), ps, ov, pad8, sigma, max_batch=4)
    assert sse is None and out.dtype == torch.float32 and tuple(out.shape) == (h, w, min(3, c))
    got = out.cpu().numpy()
    assert torch.equal(torch.cat(rep.seen), tiles_ref), "tile extraction (normalise / noise / reflect pad) must be bit-exact"
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} output values differ"
    assert got.min() >= np.float32(lo) and got.max() <= np.float32(hi)


# --------------------------------------------------------------------------- 2. float frames vs the uint8 pipeline
@pytest.mark.parametrize("h,w,c,ps,ov,pad8,sigma", CASES[:5])
def test_unit_range_float_matches_uint8_pipeline(dev, h, w, c, ps, ov, pad8, sigma):
    """float32(img) / 255 with unit_range=True sees the tiles of the uint8 call, and its result x 255, clipped and
    rounded, is the uint8 call's bytes: one multiplication by 255 either side of a clip whose bounds are exact."""
    rng = np.random.default_rng(6)
    img = u8_frame(rng, (h, w, c))
    preds = canned(rng, h, w, c, ps, ov, pad8)
    rep8, repf = Replay(preds), Replay(preds)
    out8, _ = utils.tiled_forward_device(rep8, torch.from_numpy(img).to(dev), ps, ov, pad8, sigma, max_batch=4)
    f = torch.from_numpy(img.astype(np.float32) / np.float32(255.0)).to(dev)
    outf, _ = utils.tiled_forward_device(repf, f, ps, ov, pad8, sigma, max_batch=4, unit_range=True)
    assert torch.equal(torch.cat(repf.seen), torch.cat(rep8.seen))
    gotf = outf.cpu().numpy()
    assert gotf.dtype == np.float32 and gotf.min() == 0.0 and gotf.max() == 1.0
    assert np.array_equal(np.rint(np.clip(gotf * np.float32(255.0), 0, 255)).astype(np.uint8), out8.cpu().numpy())
    # out="float32" from the uint8 frame is the same float frame
    outm, _ = utils.tiled_forward_device(Replay(preds), torch.from_numpy(img).to(dev), ps, ov, pad8, sigma, max_batch=4,
                                         out="float32")
    assert torch.equal(outm, outf)


def test_unit_range_float_matches_uint8_pipeline_dncnn(dev):
    model = dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(42).eval().to(dev)
    img = u8_frame(np.random.default_rng(7), (75, 101, 1))
    k8, kf = [], []
    out8, _ = utils.tiled_forward_device(model, torch.from_numpy(img).to(dev), 64, 16, False, keep_tiles=k8)
    f = torch.from_numpy(img.astype(np.float32) / np.float32(255.0)).to(dev)
    outf, _ = utils.tiled_forward_device(model, f, 64, 16, False, keep_tiles=kf, unit_range=True)
    assert torch.equal(k8[0], kf[0]), "the same tiles give the same predictions"
    gotf = outf.cpu().numpy()
    assert np.array_equal(np.rint(np.clip(gotf * np.float32(255.0), 0, 255)).astype(np.uint8), out8.cpu().numpy())


# --------------------------------------------------------------------------- 3. the reduction
def _minmax(t, ws_floats=2048):
    rng = torch.full((3,), float("nan"), device=t.device)
    ws = torch.empty(ws_floats, device=t.device)
    _hip.call("irm_frame_minmax_f32", _hip.ptr(t), t.numel(), _hip.ptr(rng), _hip.ptr(ws), ws_floats)
    return rng.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 257, 4099, 300 * 300 * 3])
def test_frame_minmax_bitwise(dev, n):
    a = np.random.default_rng(n).normal(0.0, 3.0, size=n + 1).astype(np.float32)
    t = torch.from_numpy(a).to(dev)
    for view, host in ((t[:n], a[:n]), (t[1:], a[1:])):            # 16-byte aligned, and 4 bytes past it
        want = np.array([host.min(), host.max(), host.max()], np.float32)
        got = _minmax(view)
        assert got.tobytes() == want.tobytes(), (got, want)
        assert _minmax(view).tobytes() == got.tobytes()
        assert _minmax(view, ws_floats=6).tobytes() == got.tobytes()     # a short workspace: fewer workgroups


# --------------------------------------------------------------------------- 4. scaled blend
class Nearest(torch.nn.Module):
    """Nearest-neighbour enlargement by `upscale`: a super-resolving stand-in that is exact on any device."""

    def __init__(self, s):
        super().__init__()
        self.upscale = s

    def forward(self, t):
        return t.repeat_interleave(self.upscale, 2).repeat_interleave(self.upscale, 3)


@pytest.mark.parametrize("s", [2, 3])
def test_scaled_float_blend_matches_host_loop(dev, s):
    img = float_frame(np.random.default_rng(8), (45, 37, 3), 0.0, 3.0)
    model = Nearest(s)
    want = utils._run_tiles_on_host(model, img, dev, utils.normalize, 13, 3, False, None, None, None)
    out, _ = utils.tiled_forward_device(model, torch.from_numpy(img.copy()).to(dev), 13, 3, False)
    assert tuple(out.shape) == (45 * s, 37 * s, 3) and want.dtype == np.float32
    assert np.array_equal(out.cpu().numpy(), want)


# --------------------------------------------------------------------------- 5. guard bands
G_H, G_W, G_PS, G_OV, G_PAD = 37, 45, 32, 8, 40


def _origins():
    return [(y0, x0) for y0 in tiler_ref.tile_origins(G_H, G_PS, G_OV) for x0 in tiler_ref.tile_origins(G_W, G_PS, G_OV)]


def test_guard_bands_minmax(dev):
    """An element read from outside the frame would show as the band's value (+-1e30; NaN would be dropped by min / max);
    range and the workspace lie between sentinels."""
    a = np.random.default_rng(9).normal(0.0, 1.0, size=G_H * G_W).astype(np.float32)
    for fill in (1e30, -1e30):
        buf, view = banded(torch.from_numpy(a), dev, fill=fill)
        rbuf, rng = sentinel_out((3,), dev)
        wbuf, ws = sentinel_out((2048,), dev)
        _hip.call("irm_frame_minmax_f32", _hip.ptr(view), a.size, _hip.ptr(rng), _hip.ptr(ws), 2048)
        torch.cuda.synchronize()
        assert intact(rbuf, rng) and intact(wbuf, ws)
        assert rng.cpu().numpy().tobytes() == np.array([a.min(), a.max(), a.max()], np.float32).tobytes()


@pytest.mark.parametrize("sigma", [None, 25])
def test_guard_bands_tile_extract_f32(dev, sigma):
    rng = np.random.default_rng(10)
    img = float_frame(rng, (G_H, G_W, 1), 0.0, 7.5)
    origins, extra = _origins(), G_PAD - G_PS
    seen = []

    def fake(t):
        seen.append(t.clone())
        return t[:, :, :G_PS, :G_PS]
    tiler_ref.tiled_inference(fake, img, patch_size=G_PS, patch_overlap=G_OV, need_degradation=sigma is not None,
                              noise_level=sigma,
                              pad=lambda t: torch.nn.functional.pad(t, (0, extra, 0, extra), mode="reflect"))
    want = torch.cat(seen)
    noise = None
    if sigma is not None:
        np.random.seed(seed=0)
        noise = banded(torch.from_numpy(np.random.normal(0, sigma / 255., (G_PS, G_PS, 1))), dev)
    keep = [banded(torch.from_numpy(img), dev), banded(torch.tensor([0.0, 7.5, 7.5], dtype=torch.float32), dev),
            banded(torch.tensor(origins, dtype=torch.int32), dev, fill=-1)]
    tbuf, tiles = sentinel_out((len(origins), 1, G_PAD, G_PAD), dev)
    _hip.call("irm_tile_extract_f32", _hip.ptr(keep[0][1]), _hip.ptr(keep[1][1]), _hip.ptr(keep[2][1]),
              _hip.ptr(None if noise is None else noise[1]), _hip.ptr(tiles), G_H, G_W, 1, G_PS, G_PS, G_PAD, G_PAD,
              len(origins), 0)
    torch.cuda.synchronize()
    assert intact(tbuf, tiles)
    got = tiles.cpu()
    assert not has_nan(got) and torch.equal(got, want)


@pytest.mark.parametrize("s", [1, 3])
def test_guard_bands_window_blend_f32(dev, s):
    """pred with Cp = 2 > Co = 1 and ph = 40 > th = 32, NaN in the unused channel and in the padding; the float32 frame
    between sentinels, every element of it written."""
    rng = np.random.default_rng(11)
    origins = _origins()
    T = len(origins)
    can = torch.from_numpy(rng.uniform(-0.5, 1.2, size=(T, 1, s * G_PS, s * G_PS)).astype(np.float32))
    pred = torch.full((T, 2, s * G_PAD, s * G_PAD), float("nan"))
    pred[:, :1, :s * G_PS, :s * G_PS] = can
    lo, hi = np.float32(-0.25), np.float32(0.9)
    shape_img = np.full((s * G_H, s * G_W, 1), lo, np.float32)
    shape_img.flat[-1] = hi
    ref, _ = oracle_run(can, shape_img, s * G_PS, s * G_OV, False, None)
    window = torch.from_numpy(utils.get_gaussian_weights(s * G_PS, s * G_PS, 1)[:, :, 0].copy())
    keep = [banded(pred, dev), banded(torch.tensor(origins, dtype=torch.int32), dev, fill=-1), banded(window, dev),
            banded(torch.tensor([float(lo), float(hi), float(hi)], dtype=torch.float32), dev)]
    obuf, out = sentinel_out((s * G_H, s * G_W, 1), dev)
    _hip.call("irm_window_blend_f32", _hip.ptr(keep[0][1]), _hip.ptr(keep[1][1]), _hip.ptr(keep[2][1]), _hip.ptr(out),
              _hip.ptr(keep[3][1]), G_H, G_W, 1, 2, G_PS, G_PS, G_PAD, G_PAD, G_PS, T, s)
    torch.cuda.synchronize()
    assert intact(obuf, out)
    got = out.cpu()
    assert not has_nan(got)
    assert np.array_equal(got.numpy(), ref), f"{int((got.numpy() != ref).sum())} of {ref.size} output values differ"


# --------------------------------------------------------------------------- 6. public call
def test_run_model_inference_float_frames(dev):
    model = dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(42).eval().to(dev)
    img = float_frame(np.random.default_rng(12), (70, 90, 1), 0.0, 1.0)
    pred, ms, out_dev = utils._run_model_inference(model, img, dev, patch_size=64, patch_overlap=16)
    assert out_dev is not None and out_dev.dtype == torch.float32 and pred.dtype == np.float32
    assert pred.shape == img.shape and np.array_equal(out_dev.cpu().numpy(), pred)
    pred2, _ = utils.run_model_inference(model, img, dev, patch_size=64, patch_overlap=16)
    assert np.array_equal(pred2, pred)
    p64, _, out64 = utils._run_model_inference(model, img.astype(np.float64), dev, patch_size=64, patch_overlap=16)
    assert out64 is None and p64.dtype == np.float64
    with pytest.raises((IndexError, ValueError)):
        utils._run_model_inference(model, img[:, :, 0], dev, patch_size=64, patch_overlap=16)


# --------------------------------------------------------------------------- 7. chains
def test_two_stage_chain_equals_the_oracle_run_twice(dev):
    h, w, ps, ov = 100, 136, 64, 16
    rng = np.random.default_rng(13)
    img = u8_frame(rng, (h, w, 3))
    pa, pb = canned(rng, h, w, 3, ps, ov, False), canned(rng, h, w, 3, ps, ov, False) - 0.25
    f1, _ = oracle_run(pa, img.astype(np.float32) / np.float32(255.0), ps, ov, False, None, mix=0.25)
    assert f1.dtype == np.float32 and f1.min() == 0.0 and f1.max() == 1.0        # its own range is the unit range
    f2, tiles2 = oracle_run(pb, f1, ps, ov, False, None, mix=0.5)
    want = np.rint(np.clip(f2 * np.float32(255.0), 0, 255)).astype(np.uint8)
    cfg = {"patch_size": ps, "patch_overlap": ov}
    a, b = Replay(pa, 0.25), Replay(pb, 0.5)
    got, ms = utils.run_model_chain([(a, cfg), (b, cfg)], img, dev)
    assert got.dtype == np.uint8 and ms > 0
    assert torch.equal(torch.cat(b.seen), tiles2), "the second stage sees the unrounded float32 frame"
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
    gotf, _ = utils.run_model_chain([(Replay(pa, 0.25), cfg), (Replay(pb, 0.5), cfg)], img, dev, out="float32")
    assert gotf.dtype == np.float32 and np.array_equal(gotf, f2)
    # the composition through a uint8 frame rounds between the stages and ends elsewhere
    g1, _ = oracle_run(pa, img, ps, ov, False, None, mix=0.25)
    g2, _ = oracle_run(pb, g1, ps, ov, False, None, mix=0.5)
    assert g1.dtype == np.uint8 and g2.dtype == np.uint8
    share = float((g2 != want).mean())
    print(f"chain vs uint8 round trip: {share:.3%} of the bytes differ")
    assert share > 0


def test_chain_float_input_is_unit_range(dev):
    """A float32 input is taken as in [0, 1]: max = 0.8 is not multiplied back, and float32 comes out."""
    h, w, ps, ov = 40, 90, 64, 16
    rng = np.random.default_rng(14)
    img = float_frame(rng, (h, w, 3), 0.0, 0.8)
    pa = canned(rng, h, w, 3, ps, ov, False)
    got, _ = utils.run_model_chain([(Replay(pa), {"patch_size": ps, "patch_overlap": ov})], img, dev)
    out, _ = utils.tiled_forward_device(Replay(pa), torch.from_numpy(img).to(dev), ps, ov, False, unit_range=True)
    assert got.dtype == np.float32 and np.array_equal(got, out.cpu().numpy()) and got.max() == 1.0


def test_one_stage_chain_is_get_model_prediction(dev):
    model = dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(42).eval().to(dev)
    img = u8_frame(np.random.default_rng(15), (75, 101, 1))
    cfg = {"patch_size": 64, "patch_overlap": 16}
    for kw in (dict(), dict(need_degradation=True, noise_level=25)):
        want, _ = utils.get_model_prediction(model, img, dev, **cfg, **kw)
        got, _ = utils.run_model_chain([(model, cfg)], img, dev, **kw)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    img16 = img.astype(np.uint16) * 257
    want, _ = utils.get_model_prediction(model, img16, dev, **cfg)
    got, _ = utils.run_model_chain([(model, cfg)], img16, dev)
    assert got.dtype == np.uint16 and np.array_equal(got, want)


def test_chain_denoise_then_super_resolve(dev):
    with open(os.path.join(GOLDEN, "mair_sr.json")) as f:
        sr_cfg = json.load(f)["configs"]["light_x2"]
    den = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    sr = mair.MaIR(**sr_cfg).load_synthetic(42).eval().to(dev)
    h, w = 40, 56
    img = u8_frame(np.random.default_rng(16), (h, w, 3))
    got, _ = utils.run_model_chain([(den, {"patch_size": 32, "patch_overlap": 8}),
                                    (sr, {"patch_size": 32, "patch_overlap": 8})], img, dev)
    assert got.shape == (2 * h, 2 * w, 3) and got.dtype == np.uint8


# --------------------------------------------------------------------------- 8. refusals
def test_refusals(dev):
    rng = np.random.default_rng(17)
    cfg = {"patch_size": 64, "patch_overlap": 16}
    img = u8_frame(rng, (64, 64, 3))
    f = torch.from_numpy(img.astype(np.float32) / np.float32(255.0)).to(dev)
    rep = Replay(canned(rng, 64, 64, 3, 64, 16, False))
    with pytest.raises(ValueError, match="DeblurGANv2"):
        utils.run_model_chain([(rep, cfg), (deblurganv2.FPNMobileNet(), cfg)], img, dev)
    with pytest.raises(ValueError, match="targets_dev"):
        utils.tiled_forward_device(rep, f, 64, 16, False, target_dev=torch.from_numpy(img).to(dev))
    with pytest.raises(ValueError, match="targets_dev"):
        utils.tiled_forward_device(rep, torch.from_numpy(img).to(dev), 64, 16, False,
                                   target_dev=torch.from_numpy(img).to(dev), out="float32")
    with pytest.raises(ValueError, match="deblurganv2"):
        utils.tiled_forward_device(rep, f, 64, 16, False, hooks="deblurganv2")
    assert rep.seen == [], "refused before any tile was cut"
