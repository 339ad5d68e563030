"""MaIR super resolution on the GPU: the selective scan at MaIR's (d_state, dt_rank) pairs, the SR-head conv epilogues
(LeakyReLU, PixelShuffle(r)) on both 3x3 conv kernels, the blend at output scale, the SR configurations against the
reference goldens (tools/gen_golden_mair_sr.py), the loader and the tiled call."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from irm_amd import _hip, harness, mair, ops, synth, utils
from oracle import mair_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(555, name, shape, lo, hi)


@pytest.fixture(scope="module")
def sr_meta():
    with open(os.path.join(GOLDEN, "mair_sr.json")) as f:
        return json.load(f)


# --------------------------------------------------------------------------- 1. selective scan
@pytest.mark.parametrize("N,R", [(1, 4), (16, 4)])
@pytest.mark.parametrize("D", [66, 90, 128])
@pytest.mark.parametrize("B,H,W,chunk", [(1, 12, 20, 56), (2, 9, 11, 32)])
def test_selective_scan_mair_pairs_vs_float64(dev, N, R, D, B, H, W, chunk):
    """Several chunks per direction, the last one ragged (240 = 4 x 56 + 16; 99 = 3 x 32 + 3).  D = 66 / 90 run the
    (direction, channel) lane mapping, D = 128 (whole 64-channel blocks) the wave-per-direction one."""
    L, J = H * W, R + 2 * N
    ids, inv = mair_ref.scan_ids(H, W, 4)
    tag = f"{N}_{R}_{D}_{B}"
    x = rnd(f"u{tag}", (B, D, L))
    proj = rnd(f"p{tag}", (B, 4, J, L))
    dtw = rnd(f"w{tag}", (4, D, R), -0.5, 0.5)
    dtb = rnd(f"b{tag}", (4, D), -4, -2)
    A = -torch.exp(rnd(f"a{tag}", (4 * D, N), 0, 1.5))
    Ds = rnd(f"d{tag}", (4 * D,), 0.5, 1.5)
    xs = torch.stack([x.index_select(-1, ids[k]) for k in range(4)], 1).double()
    pg = torch.stack([proj[:, k].index_select(-1, ids[k]) for k in range(4)], 1).double()
    dts = torch.einsum("bkrl,kdr->bkdl", pg[:, :, :R], dtw.double())
    y = mair_ref.selective_scan(xs.reshape(B, -1, L), dts.reshape(B, -1, L), A.double(), pg[:, :, R:R + N],
                                pg[:, :, R + N:], Ds.double(), delta_bias=dtb.double().reshape(-1),
                                delta_softplus=True).view(B, 4, D, L)
    assert y.dtype == torch.float64
    y_img = torch.stack([y[:, k].index_select(-1, inv[k]) for k in range(4)], 1)
    xT = x.transpose(1, 2).contiguous().to(dev)
    pT = proj.reshape(B, 4 * J, L).transpose(1, 2).contiguous().to(dev)
    nchunk, DB = -(-L // chunk), -(-D // 64)
    assert nchunk >= 3 and L % chunk
    yT = torch.full((B, 4, L, D), float("nan"), device=dev)
    state = torch.empty(2 * B * 4 * DB * nchunk * N * 64, device=dev)
    sdt = torch.empty(B * 4 * DB * nchunk * 64, device=dev)
    ysum = torch.empty(B * 4 * DB * nchunk * 64, device=dev)
    ops.selective_scan(xT, pT, ids.int().to(dev), dtw.to(dev), dtb.to(dev), A.to(dev), Ds.to(dev), yT, state, sdt, ysum,
                       B, L, D, N, R, chunk)
    got = yT.cpu().permute(0, 1, 3, 2).double()
    ymax = float(y_img.abs().max())
    err = float((got - y_img).abs().max())
    print(f"scan N{N} R{R} D{D} L{L} chunk{chunk}: max-abs vs float64 {err:.3e} (|y| max {ymax:.2f})")
    assert err <= 2e-4 * max(1.0, ymax)
    s = ysum.cpu().view(B, 4, DB, nchunk, 64).sum(3).reshape(B, 4, DB * 64)[:, :, :D].double()
    assert (s / L - y_img.mean(-1)).abs().max() <= 1e-4 * max(1.0, ymax)


def test_selective_scan_other_pairs_still_rejected(dev):
    B, L, D, N, R = 1, 16, 64, 2, 4
    t = torch.zeros(4096, device=dev)
    ids = torch.zeros(4 * L, dtype=torch.int32, device=dev)
    for n, r in ((2, 4), (1, 3), (16, 6), (8, 4)):
        with pytest.raises(_hip.HipLibraryError, match="invalid arguments"):
            _hip.call("irm_selective_scan_f32", *[_hip.ptr(t)] * 2, _hip.ptr(ids), *[_hip.ptr(t)] * 8, B, L, D, n, r, 16)


# --------------------------------------------------------------------------- 2. conv epilogues
def _conv_ref(x, w, b, leaky, r):
    y = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    if leaky is not None:
        y = F.leaky_relu(y, leaky)
    return F.pixel_shuffle(y, r) if r else y


_CONV_CASES = [
    (60, 12, 2, None, 12, 20), (60, 27, 3, None, 12, 20), (60, 48, 4, None, 16, 16),      # UpsampleOneStep (3 r^2)
    (60, 12, 2, None, 9, 13), (60, 27, 3, None, 11, 7), (60, 48, 4, None, 5, 18),         # W % 4 != 0: exact only
    (64, 256, 2, None, 8, 24), (64, 576, 3, None, 8, 12),                                 # Upsample
    (180, 64, 0, 0.01, 12, 20), (60, 64, 0, 0.01, 7, 9), (64, 64, 0, 0.2, 16, 32)]        # conv_before_upsample


# the emulated kernel needs W % 4 == 0 (ops.conv3x3 takes the exact one there)
@pytest.mark.parametrize("kernel,ci,co,r,leaky,H,W", [(k,) + c for k in ("split", "exact") for c in _CONV_CASES
                                                      if k == "exact" or c[-1] % 4 == 0])
def test_conv3x3_sr_epilogues_vs_float64(dev, kernel, ci, co, r, leaky, H, W):
    B = 2
    tag = f"{ci}_{co}_{r}_{H}_{W}"
    x = rnd(f"cx{tag}", (B, ci, H, W))
    w = rnd(f"cw{tag}", (co, ci, 3, 3), -0.1, 0.1)
    b = rnd(f"cb{tag}", (co,), -0.5, 0.5)
    ref = _conv_ref(x, w, b, leaky, r)
    cw = _hip.pack_conv3x3(w.to(dev))
    wp = (cw.split, cw.inv_scale) if kernel == "split" else cw.exact
    y = torch.full(tuple(ref.shape), float("nan"), device=dev)
    kw = dict(store_mode=2, shuffle=r) if r else dict(leaky=leaky)
    ops.conv3x3(wp, x.to(dev), y, ci, co, bias=b.to(dev), **kw)
    err = float((y.cpu().double() - ref).abs().max())
    bound = 1e-4 * max(1.0, float(ref.abs().max()))
    print(f"conv3x3 {kernel} ci{ci} co{co} r{r} leaky{leaky} {H}x{W}: max-abs vs float64 {err:.3e}")
    assert err <= bound
    # the dispatch of ops.conv3x3 (ConvWeight: emulated where aligned, exact otherwise) gives the same result class
    y2 = torch.full(tuple(ref.shape), float("nan"), device=dev)
    ops.conv3x3(cw, x.to(dev), y2, ci, co, bias=b.to(dev), **kw)
    assert float((y2.cpu().double() - ref).abs().max()) <= bound


def test_conv3x3_ep_rejects_bad_epilogues(dev):
    x = torch.zeros(1, 16, 8, 8, device=dev)
    y = torch.zeros(1, 1, 40, 40, device=dev)
    wp = _hip.pack_conv3x3_weight(torch.zeros(27, 16, 3, 3, device=dev))
    for act, shuffle, co in ((0, 5, 27), (3, 3, 27), (0, 3, 26), (0, 4, 27)):
        with pytest.raises(_hip.HipLibraryError, match="invalid arguments"):
            _hip.call("irm_conv3x3_ep_f32", _hip.ptr(wp), _hip.ptr(x), 1024, _hip.ptr(y), 1600, None, 0, None, 1, 16, co,
                      8, 8, act, 0.0, 0, 0, 2, shuffle, 1, 1)


# --------------------------------------------------------------------------- 3. blend at output scale
def _numpy_blend_scaled(pred, origins, h, w, th, tw, ps, s, c, peak):
    """Float32 restatement of irm_window_blend_scaled (the reference blend's operation order, utils.py:433-440)."""
    win = utils.get_gaussian_weights(s * ps, s * ps, 1)[:, :, 0]
    acc = np.zeros((c, s * h, s * w), np.float32)
    wsum = np.zeros((c, s * h, s * w), np.float32)
    for i, (y0, x0) in enumerate(origins):
        ys, xs = slice(s * y0, s * (y0 + th)), slice(s * x0, s * (x0 + tw))
        wt = win[:s * th, :s * tw]
        acc[:, ys, xs] = acc[:, ys, xs] + pred[i, :c, :s * th, :s * tw] * wt
        wsum[:, ys, xs] = wsum[:, ys, xs] + wt
    v = acc / np.maximum(wsum, np.float32(1e-8))
    v = np.rint(np.clip(v * np.float32(peak), np.float32(0), np.float32(peak)))
    return np.ascontiguousarray(v.transpose(1, 2, 0).astype(np.uint16 if peak > 255 else np.uint8))


@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_window_blend_scaled_bit_exact(dev, s, u16):
    """Padded prediction tiles (ph, pw > th, tw) so that the s*ph row stride and the crop to s*th x s*tw are checked."""
    h, w, ps, ov, c = 45, 70, 32, 8, 3
    ys, xs = utils.tile_origins(h, ps, ov), utils.tile_origins(w, ps, ov)
    origins = [(y0, x0) for y0 in ys for x0 in xs]
    T, th, tw, ph, pw = len(origins), ps, ps - 4, 40, 36
    pred = rnd(f"blend{s}", (T, 4, s * ph, s * pw), -0.05, 1.05).numpy()
    peak = 65535 if u16 else 255
    want = _numpy_blend_scaled(pred, origins, h, w, th, tw, ps, s, c, peak)
    out = torch.empty(s * h, s * w, c, dtype=torch.int16 if u16 else torch.uint8, device=dev)
    org = torch.tensor(origins, dtype=torch.int32, device=dev)
    win = torch.from_numpy(utils.get_gaussian_weights(s * ps, s * ps, 1)[:, :, 0].copy()).to(dev)
    tgt = torch.from_numpy(want.view(np.int16) if u16 else want).to(dev)
    sse = torch.zeros(1, dtype=torch.int64, device=dev)
    _hip.call("irm_window_blend_scaled", _hip.ptr(torch.from_numpy(pred).to(dev)), _hip.ptr(org), _hip.ptr(win),
              _hip.ptr(out), int(u16), _hip.ptr(tgt), _hip.ptr(sse), h, w, c, 4, th, tw, ph, pw, ps, T, s, 1.0, 0.0)
    got = out.cpu().numpy()
    got = got.view(np.uint16) if u16 else got
    assert np.array_equal(got, want)
    assert int(sse.item()) == 0


# --------------------------------------------------------------------------- 4. SR configurations vs reference goldens
@pytest.mark.parametrize("name", ["light_x2", "light_x3", "light_x4", "default_x2", "classic_x2", "classic_x3",
                                  "classic_x4"])
def test_mair_sr_vs_golden(dev, golden, sr_meta, name):
    cfg = sr_meta["configs"][name]
    model = mair.MaIR(**cfg).load_synthetic(42).eval().to(dev)
    for h, w in sr_meta["inputs"]:
        x = synth.uniform(7, f"mair_sr_in_{h}x{w}", (1, 3, h, w), 0.0, 1.0)
        y = model(x.to(dev)).cpu().numpy()
        g = golden("mair_sr")[f"{name}_{h}x{w}"]
        assert y.shape == g.shape
        err = float(np.abs(y - g).max())
        print(f"mair sr {name} {h}x{w}: max-abs vs reference golden {err:.3e} (|y| max {float(np.abs(g).max()):.2f})")
        assert err <= 1e-3


# --------------------------------------------------------------------------- 5. loader round trip
def test_get_model_sr_round_trip(dev, tmp_path, golden, sr_meta):
    import yaml
    cfg = dict(sr_meta["configs"]["classic_x3"])
    src = mair.MaIR(**cfg).load_synthetic(42)
    wpath = tmp_path / "MaIR_classicSR_x3.pth"
    torch.save({"params": {"module." + k: v for k, v in src.state_dict().items()}}, wpath)
    yml = tmp_path / "test_MaIR_classicSR_x3.yml"
    yml.write_text(yaml.safe_dump({"name": "x3", "num_gpu": 1, "network_g": dict(type="MaIR", **cfg),
                                   "path": {"pretrain_network_g": str(wpath), "strict_load_g": True}}))
    model = mair.get_model(str(yml))
    assert next(model.parameters()).is_cuda and model.upscale == 3
    x = synth.uniform(7, "mair_sr_in_12x20", (1, 3, 12, 20), 0.0, 1.0).to(dev)
    y = model(x).cpu().numpy()
    assert float(np.abs(y - golden("mair_sr")["classic_x3_12x20"]).max()) <= 1e-3


# --------------------------------------------------------------------------- 6. tiled call at output scale
def _host_blend(tiles, origins, h, w, th, tw, ps, s):
    acc = np.zeros((s * h, s * w, 3), np.float32)
    wsum = np.zeros_like(acc)
    win = utils.get_gaussian_weights(s * ps, s * ps, 3)
    for i, (y0, x0) in enumerate(origins):
        p = tiles[i].transpose(1, 2, 0)
        acc[s * y0:s * (y0 + th), s * x0:s * (x0 + tw)] += p * win[:s * th, :s * tw]
        wsum[s * y0:s * (y0 + th), s * x0:s * (x0 + tw)] += win[:s * th, :s * tw]
    acc /= np.maximum(wsum, 1e-8)
    return np.clip(acc * 255.0, 0, 255).round().astype(np.uint8)


@pytest.mark.parametrize("s,ps", [(2, 64), (4, 64), (2, 128)])
def test_get_model_prediction_sr_tiled(dev, sr_meta, s, ps):
    """Patch 64: 2 x 3 tiles of 64 x 64.  Patch 128: 1 x 2 tiles of 100 x 128, reflect-padded to 104 x 128 (the crop
    of an s*104-row prediction to s*100 rows)."""
    cfg = dict(sr_meta["configs"][f"light_x{s}"])
    model = mair.MaIR(**cfg).load_synthetic(42).eval().to(dev)
    h, w, ov = 100, 140, 16
    lr = (synth.uniform(9, "mair_sr_lr_frame", (h, w, 3), 0.0, 1.0).numpy() * 255).astype(np.uint8)
    pred, ms = utils.get_model_prediction(model, lr, dev, ps, ov)
    assert pred.shape == (s * h, s * w, 3) and pred.dtype == np.uint8
    keep = []
    out, _ = utils.tiled_forward_device(model, torch.from_numpy(lr).to(dev), ps, ov, pad8=True, keep_tiles=keep)
    ys, xs = utils.tile_origins(h, ps, ov), utils.tile_origins(w, ps, ov)
    assert tuple(keep[0].shape[2:]) == (s * min(ps, h), s * min(ps, w))
    host = _host_blend(keep[0].cpu().numpy(), [(a, b) for a in ys for b in xs], h, w, min(ps, h), min(ps, w),
                       min(ps, max(h, w)), s)
    for got in (pred, out.cpu().numpy()):
        diff = np.abs(got.astype(np.int32) - host.astype(np.int32))
        print(f"tiled SR x{s}: {h}x{w} -> {got.shape}, max diff {int(diff.max())}, share {float((diff > 0).mean()):.2e}")
        assert int(diff.max()) <= 1 and float((diff > 0).mean()) < 1e-2
    # uint16 frames take the same path
    lr16 = lr.astype(np.uint16) * 257
    p16, _ = utils.get_model_prediction(model, lr16, dev, ps, ov)
    assert p16.dtype == np.uint16 and p16.shape == (s * h, s * w, 3)
    assert int(np.abs(p16.astype(np.int64) // 257 - pred.astype(np.int64)).max()) <= 1


# --------------------------------------------------------------------------- 7. harness with (LR, HR) pairs
@pytest.mark.parametrize("metrics", ["host", "device"])
def test_harness_evaluate_sr_pairs(dev, sr_meta, metrics):
    """(LR, HR) pairs: the row's PSNR / SSIM are the means of calculate_metrics on each returned x2 prediction against
    its HR target (two different frames, so a metric of the wrong region or frame would not match)."""
    model = mair.MaIR(**sr_meta["configs"]["light_x2"]).load_synthetic(42).eval().to(dev)
    pairs, want = [], []
    for i in range(2):
        lr = (synth.uniform(9, f"mair_sr_lr_h{i}", (40, 56, 3), 0.0, 1.0).numpy() * 255).astype(np.uint8)
        hr = np.repeat(np.repeat(lr, 2, 0), 2, 1)
        pred, _ = utils.get_model_prediction(model, lr, dev, 32, 8)
        assert pred.shape == hr.shape
        want.append(utils.calculate_metrics(pred, hr))
        pairs.append((lr, hr, f"{i}.png"))
    row = harness.evaluate(model, pairs, dev, {"patch_size": 32, "patch_overlap": 8}, task="super-resolution",
                           subtask="x2", dataset="synthetic", model_name="MaIR", metrics=metrics, skip_failed=False)
    assert row["Failed"] == []
    assert abs(want[0][0] - want[1][0]) > 1e-3                    # the two frames score differently
    assert abs(row["PSNR"] - np.mean([p for p, _ in want])) <= 1e-6
    assert abs(row["SSIM"] - np.mean([q for _, q in want])) <= 1e-6
