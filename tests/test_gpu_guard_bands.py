"""Guard-band tests of every kernel family outside the TransformerBlock kernels that
tests/test_gpu_ops.py::test_no_write_outside_the_output covers (tests/guards.py has the method).

Every case: inputs between bands of NaN (integer inputs: run twice, bands of zeros and of ones, results bitwise
equal), outputs and workspaces between sentinels and, where include/irm_hip.h states a minimum size, at exactly that
size; a non-zero batch slack wherever the header has a batch stride.  Asserted: the sentinels survive, no NaN reaches
a result, and the result meets the bar of the family's own test against the same float64 / host reference.  All
guards lie inside the test's own buffers.  Shapes are the smallest that still run a kernel's tail code (a partial
64-channel block, a ragged last chunk, an odd side, a partial pixel tile)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from irm_amd import _hip, ensemble, ops, resize, synth, utils
from oracle import mair_ref, tiler_ref

import block_model as bm
from frame_checks import check_against_host, check_quantised, down, merge_float64, packed_blocks, up
from guards import SLACK, Guards, clean, guarded_fold, has_nan, two_fills
from scan_model import check_scan_f64, scan_inputs, ysum_floor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(909, name, shape, lo, hi)


# --------------------------------------------------------------------------- mamba.hip
def test_transpose(dev):
    """B = 2, R = 37, C = 50: both extents leave a partial 32 x 32 tile; in_bs and out_bs with slack.  Bit exact."""
    B, R, C = 2, 37, 50
    g = Guards(dev)
    x = rnd("tr", (B, R, C))
    xv, out = g.inp(x, SLACK), g.out("out", (B, C, R), slack=SLACK)
    ops.transpose(xv, out, R, C)
    g.check()
    assert torch.equal(clean(out), x.transpose(1, 2).contiguous())


@pytest.mark.parametrize("D,N,R", [(96, 4, 3), (66, 1, 4), (90, 16, 4)])
def test_selective_scan_and_combine(dev, D, N, R):
    """Block path (4, 3) with D = 96 = one full + one partial 64-channel block; flat path (1, 4) with D = 66 and
    (16, 4) with D = 90 (4 D is no multiple of 64).  B = 2, 5 x 7 pixels, chunk 32: the last chunk has 3 steps.
    state, sdt, ysum at exactly the header's sizes; gate at exactly [B][4][D]; z and out with batch slack.
    Bars: SCAN_K / SCAN_F / ysum_floor (scan_model.check_scan_f64) and test_losh_combine_production_vs_float64."""
    B, H, W, chunk = 2, 5, 7, 32
    L, J = H * W, R + 2 * N
    nchunk, DB = -(-L // chunk), -(-D // 64)
    assert ops.scan_is_flat(D, N, R) == (D != 96)
    ids, inv = mair_ref.scan_ids(H, W, 4)
    x, proj, dtw, dtb, A, Ds = scan_inputs(f"gb{D}", "synthetic", B, D, N, R, L)
    xT = x.transpose(1, 2).contiguous()
    pT = proj.reshape(B, 4 * J, L).transpose(1, 2).contiguous()
    gw, gb = rnd(f"cgw{D}", (4 * D, 4), -2, 2), rnd(f"cgb{D}", (4 * D,))
    nw, nb = rnd(f"cnw{D}", (D,), 0.5, 1.5), rnd(f"cnb{D}", (D,), -0.2, 0.2)
    z = rnd(f"cz{D}", (B, D, H, W))

    def run(fill):
        g = Guards(dev)
        yT = g.out("yT", (B, 4, L, D))
        state = g.out("state", (2 * B * 4 * DB * nchunk * N * 64,))
        sdt = g.out("sdt", (B * 4 * DB * nchunk * 64,))
        ysum = g.out("ysum", (B * 4 * DB * nchunk * 64,))
        ops.selective_scan(g.inp(xT), g.inp(pT), g.inp(ids.int(), fill=fill), g.inp(dtw), g.inp(dtb), g.inp(A), g.inp(Ds),
                           yT, state, sdt, ysum, B, L, D, N, R, chunk)
        g.check()
        y_host, ysum_host = yT.cpu(), ysum.cpu().view(B, 4, DB, nchunk, 64)
        gate, out = g.out("gate", (B, 4, D)), g.out("out", (B, D, H, W), slack=SLACK)
        ops.losh_combine(ysum, g.inp(gw), g.inp(gb), gate, yT, g.inp(nw), g.inp(nb), g.inp(z, SLACK), out, B, L, D, nchunk)
        g.check()
        return y_host, ysum_host, gate.cpu(), out.cpu()

    y, ysum, gate, out = two_fills(run)
    for t in (y, gate, out):
        assert not has_nan(t)
    check_scan_f64(f"guarded D{D} N{N}", x, proj, dtw, dtb, A, Ds, ids, inv, y.permute(0, 1, 3, 2), ysum, B, L, D, N, R, chunk)
    yd = y.double()                                                                  # (B, 4, L, D)
    m = yd.mean(2)
    gref = torch.sigmoid(torch.einsum("dqk,bkd->bqd", gw.double().view(D, 4, 4), m) + gb.double().view(D, 4).t())
    v = (yd * gref.unsqueeze(2)).sum(1)                                              # (B, L, D)
    ref = F.layer_norm(v, (D,), nw.double(), nb.double(), 1e-5).transpose(1, 2) * F.silu(z.double().reshape(B, D, L))
    tol_g = 2 * ysum_floor(chunk, nchunk, float(yd.abs().mean(2).max())) + 2.0 ** -22
    assert float((gate.double() - gref).abs().max()) <= tol_g
    assert float((out.double().reshape(B, D, L) - ref).abs().max()) <= 4e-6 * max(1.0, float(ref.abs().max()))


# --------------------------------------------------------------------------- ensemble.hip
#: the smallest frame that plan_axis chops on both axes (CHOP_SIZE = 200) and whose transposed variants have another
#: grid: 200 // 200 + 1 = 2 rows, 400 // 200 + 1 = 3 columns (3 x 2 after the transpose); 400 % 3 != 0 reflect-pads
ENS_H, ENS_W = 200, 400


def test_dihedral_chop(dev):
    """dst_pixels exactly geo.total_pixels; bit exact against ensemble.chop_torch."""
    B, C = 2, 2
    geo = ensemble.geometry(B, ENS_H, ENS_W, True)
    assert all(ensemble.plan(ENS_H, ENS_W, v).grid == ((3, 2) if v >= 4 else (2, 3)) for v in range(8))
    x = rnd("chop", (B, C, ENS_H, ENS_W))

    def run(fill):
        g = Guards(dev)
        packed = g.out("dst", (geo.total_pixels * C,))
        ensemble.dihedral_chop(g.inp(x), g.inp(torch.from_numpy(geo.table), fill=fill), packed, geo)
        g.check()
        return (packed.cpu(),)

    packed, = two_fills(run)
    assert not has_nan(packed)
    blocks = packed_blocks(packed, geo, B, C)
    for v in range(8):
        want = ensemble.chop_torch(x, v, True)
        assert len(want) == len(blocks[v])
        for i, (a, b) in enumerate(zip(blocks[v], want)):
            assert a.shape == b.shape and torch.equal(a, b), (v, i)


@pytest.mark.parametrize("s,B,Co", [(1, 2, 2), (3, 2, 1)])
def test_ensemble_merge(dev, s, B, Co):
    """pred_pixels exactly geo.total_pixels; bar of test_merge_kernel_vs_float64 (2^-21 max|v|)."""
    geo = ensemble.geometry(B, ENS_H, ENS_W, True)
    pred = rnd(f"merge{s}", (geo.total_pixels * Co * s * s,), -3.0, 3.0)
    want = merge_float64([[b.double().numpy() for b in bl] for bl in packed_blocks(pred, geo, B, Co, s)], ENS_H, ENS_W, s, True)

    def run(fill):
        g = Guards(dev)
        out = g.out("out", (B, Co, s * ENS_H, s * ENS_W))
        ensemble.ensemble_merge(g.inp(pred), g.inp(torch.from_numpy(geo.table), fill=fill), out, geo, s)
        g.check()
        return (out.cpu(),)

    out, = two_fills(run)
    assert not has_nan(out)
    assert float(np.abs(out.double().numpy() - want).max()) <= 2.0 ** -21 * float(pred.abs().max())


# --------------------------------------------------------------------------- fpn.hip
def _check_stats(st, x, hi):
    got = clean(st).double()
    mean, rstd = bm.ln_stats(x.double().flatten(2), dim=-1)      # per plane
    assert float((got[..., 0] - mean).abs().max()) < 1e-5 * max(1.0, abs(hi))
    assert float(((got[..., 1] - rstd).abs() / rstd).max()) < 1e-4


@pytest.mark.parametrize("B,C,H,W,nsplit", [(2, 5, 37, 51, 1), (1, 3, 96, 128, 3)])
def test_chan_stats(dev, B, C, H, W, nsplit):
    """Single workgroup (odd plane, unaligned) and split planes (96 x 128 over B C = 3 planes: nsplit = 3).  ws exactly
    3 B C ceil(1024 / (B C)) floats and NaN inside: a slice that is read but never written would reach the result."""
    x = rnd(f"cs{C}{H}", (B, C, H, W), -2.0, 3.0)
    need = 3 * B * C * -(-1024 // (B * C))
    g = Guards(dev)
    xv = g.inp(x, SLACK)
    st, ws = g.out("stats", (B, C, 2)), g.out("ws", (need,))
    ws.fill_(float("nan"))
    _hip.call("irm_chan_stats_ws_f32", _hip.ptr(xv), xv.stride(0), _hip.ptr(st), _hip.ptr(ws), need, B, C, H * W, 1e-5)
    g.check()
    _check_stats(st, x, 3.0)
    split_ran = bool((~torch.isnan(ws)).any())
    assert split_ran == (nsplit > 1), "the case must take the path it is named for"
    st2 = g.out("stats (no workspace)", (B, C, 2))
    _hip.call("irm_chan_stats_f32", _hip.ptr(xv), xv.stride(0), _hip.ptr(st2), B, C, H * W, 1e-5)
    g.check()
    _check_stats(st2, x, 3.0)


def test_chan_norm_act_in_place_with_residual(dev):
    B, C, H, W = 2, 5, 23, 41
    x, r = rnd("cn", (B, C, H, W), -2, 3), rnd("cnr", (B, C, H, W))
    w, b = rnd("cnw", (C,), 0.5, 1.5), rnd("cnb", (C,))
    mean, rstd = bm.ln_stats(x.double().flatten(2), dim=-1)      # per plane
    ref = F.relu(F.instance_norm(x.double(), None, None, w.double(), b.double(), True, 0.1, 1e-5)) + r.double()
    g = Guards(dev)
    y = g.out("y", (B, C, H, W), slack=SLACK)
    y.copy_(x)
    ops.chan_norm_act(y, g.inp(torch.stack([mean, rstd], -1).float()), y, weight=g.inp(w), bias=g.inp(b), res=g.inp(r, SLACK),
                      act=_hip.ACT_RELU)
    g.check()
    assert float((clean(y).double() - ref).abs().max()) < 2e-4


def test_stride2_convs(dev):
    """23 x 41: both extents odd, the last output row and column read the zero border."""
    B, H, W = 2, 23, 41
    g = Guards(dev)
    x, w = rnd("s2x", (B, 3, H, W)), rnd("s2w", (32, 3, 3, 3), -0.3, 0.3)
    ref = F.conv2d(x.double(), w.double(), None, 2, 1)
    y = g.out("conv3x3_s2", tuple(ref.shape), slack=SLACK)
    ops.conv3x3_s2(g.inp(x, SLACK), g.inp(w), y, 3, 32)
    C = 70
    xd, wd = rnd("s2d", (B, C, H, W)), rnd("s2dw", (C, 1, 3, 3))
    refd = F.conv2d(xd.double(), wd.double(), None, 2, 1, groups=C)
    yd = g.out("dwconv3x3_s2", tuple(refd.shape), slack=SLACK)
    ops.dwconv3x3_s2(g.inp(xd, SLACK), g.inp(wd.reshape(C, 9)), yd)
    g.check()
    assert float((clean(y).double() - ref).abs().max()) < 2e-4
    assert float((clean(yd).double() - refd).abs().max()) < 2e-4


def test_upsample_add(dev):
    src, add = rnd("ua", (2, 3, 5, 7)), rnd("ub", (2, 3, 10, 14))
    g = Guards(dev)
    out = g.out("out", (2, 3, 10, 14), slack=SLACK)
    ops.upsample_add(g.inp(src, SLACK), out, 2, add=g.inp(add, SLACK))
    g.check()
    assert torch.equal(clean(out), add + F.interpolate(src, scale_factor=2, mode="nearest"))


# --------------------------------------------------------------------------- tiler.hip
#: 37 x 51 x 3 with 32-pixel tiles (overlap 8) padded to 40: 2 x 2 tiles, the last ones flush with the edges
T_H, T_W, T_C, T_PS, T_OV, T_PAD = 37, 51, 3, 32, 8, 40


def _frame(rng, shape, dtype):
    return rng.integers(0, (255 if dtype == np.uint8 else 65535) + 1, size=shape).astype(dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("pad_zero", [0, 1])
@pytest.mark.parametrize("sigma", [None, 25])
def test_tile_extract(dev, dtype, pad_zero, sigma):
    """Bit exact against the oracle tiler, as test_device_tiler_bit_exact_vs_oracle is."""
    rng = np.random.default_rng(11)
    img = _frame(rng, (T_H, T_W, T_C), dtype)
    origins = [(y0, x0) for y0 in tiler_ref.tile_origins(T_H, T_PS, T_OV) for x0 in tiler_ref.tile_origins(T_W, T_PS, T_OV)]
    T, extra = len(origins), T_PAD - T_PS
    seen = []

    def fake(t):
        seen.append(t.clone())
        return t[:, :, :T_PS, :T_PS]
    tiler_ref.tiled_inference(fake, img, patch_size=T_PS, patch_overlap=T_OV, need_degradation=sigma is not None,
                              noise_level=sigma, pad=lambda t: F.pad(t, (0, extra, 0, extra), mode="constant" if pad_zero else "reflect"))
    want = torch.cat(seen)
    noise = None
    if sigma is not None:
        np.random.seed(seed=0)
        noise = torch.from_numpy(np.random.normal(0, sigma / 255., (T_PS, T_PS, T_C)))

    def run(fill):
        g = Guards(dev)
        tiles = g.out("tiles", (T, T_C, T_PAD, T_PAD))
        _hip.call("irm_tile_extract", _hip.ptr(g.inp(up(img, "cpu"), fill=fill)), int(dtype == np.uint16),
                  _hip.ptr(g.inp(torch.tensor(origins, dtype=torch.int32), fill=fill)), _hip.ptr(g.inp(noise)), _hip.ptr(tiles),
                  T_H, T_W, T_C, T_PS, T_PS, T_PAD, T_PAD, T, 0.0, 1.0, pad_zero)
        g.check()
        return (tiles.cpu(),)

    tiles, = two_fills(run)
    assert not has_nan(tiles) and torch.equal(tiles, want)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("s", [1, 3])
def test_window_blend(dev, dtype, s):
    """irm_window_blend (s = 1) and irm_window_blend_scaled (s = 3): pred with Cp = 4 > Co = 3 and ph = 40 > th = 32, NaN in
    the unused channel and in the padding; the requantised frame between byte sentinels; the integer squared error."""
    rng = np.random.default_rng(13)
    Co, Cp = T_C, T_C + 1
    origins = [(y0, x0) for y0 in tiler_ref.tile_origins(T_H, T_PS, T_OV) for x0 in tiler_ref.tile_origins(T_W, T_PS, T_OV)]
    T = len(origins)
    canned = torch.from_numpy(rng.uniform(-0.2, 1.2, size=(T, Co, s * T_PS, s * T_PS)).astype(np.float32))
    pred = torch.full((T, Cp, s * T_PAD, s * T_PAD), float("nan"))
    pred[:, :Co, :s * T_PS, :s * T_PS] = canned
    target = _frame(rng, (s * T_H, s * T_W, Co), dtype)
    k = [0]

    def fake(t):
        k[0] += 1
        return canned[k[0] - 1:k[0]]
    ref = tiler_ref.tiled_inference(fake, np.zeros((s * T_H, s * T_W, Co), dtype), patch_size=s * T_PS, patch_overlap=s * T_OV)
    window = torch.from_numpy(utils.get_gaussian_weights(s * T_PS, s * T_PS, 1)[:, :, 0].copy())
    tdt = torch.uint8 if dtype == np.uint8 else torch.int16

    def run(fill):
        g = Guards(dev)
        out, sse = g.out("out", (s * T_H, s * T_W, Co), tdt), g.out("sse", (1,), torch.int64)
        sse.zero_()
        args = (_hip.ptr(g.inp(pred)), _hip.ptr(g.inp(torch.tensor(origins, dtype=torch.int32), fill=fill)), _hip.ptr(g.inp(window)),
                _hip.ptr(out), int(dtype == np.uint16), _hip.ptr(g.inp(up(target, "cpu"), fill=fill)), _hip.ptr(sse), T_H, T_W, Co, Cp,
                T_PS, T_PS, T_PAD, T_PAD, T_PS, T)
        if s == 1:
            _hip.call("irm_window_blend", *args, 1.0, 0.0)
        else:
            _hip.call("irm_window_blend_scaled", *args, s, 1.0, 0.0)
        g.check()
        return out.cpu(), sse.cpu()

    out, sse = two_fills(run)
    got = down(out, dtype)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} output values differ"
    assert int(sse[0]) == int(((ref.astype(np.int64) - target.astype(np.int64)) ** 2).sum())


# --------------------------------------------------------------------------- resize.hip, metrics*.hip, niqe.hip
FRAME_KINDS = [(np.uint8, 3), (np.uint8, 1), (np.uint16, 3), (np.uint16, 1)]


@pytest.mark.parametrize("dtype,C", FRAME_KINDS)
@pytest.mark.parametrize("scale,H,W", [(2, 6, 7), (0.5, 10, 11), (0.25, 18, 19)])
def test_imresize_bicubic(dev, dtype, C, scale, H, W):
    """The shortest legal sides (H = P taps: 6 enlarging, 4 s + 2 shrinking) and an odd W = P + 1; K = 2.  The tap tables
    between NaN (weights) and two fills (indices).  Bars of frame_checks.check_resize."""
    K = 2
    rng = np.random.default_rng(17)
    frames = _frame(rng, (K, H, W, C), dtype)
    s, shrink = resize._resize_factor(scale)
    (wh, ih), (ww, iw) = utils.resize_table(H, scale), utils.resize_table(W, scale)
    assert wh.shape[1] == H                                     # the side equals the tap count
    OH, OW = wh.shape[0], ww.shape[0]
    tdt = torch.uint8 if dtype == np.uint8 else torch.int16

    def run(fill):
        res = []
        for out_float in (1, 0):
            g = Guards(dev)
            out = g.out("out", (K, OH, OW, C), torch.float32 if out_float else tdt)
            _hip.call("irm_imresize_bicubic", _hip.ptr(g.inp(up(frames, "cpu"), fill=fill)), int(dtype == np.uint16), _hip.ptr(out),
                      out_float, _hip.ptr(g.inp(torch.from_numpy(wh.astype(np.float32)))),
                      _hip.ptr(g.inp(torch.from_numpy(ih.astype(np.int32)), fill=fill)),
                      _hip.ptr(g.inp(torch.from_numpy(ww.astype(np.float32)))),
                      _hip.ptr(g.inp(torch.from_numpy(iw.astype(np.int32)), fill=fill)), K, H, W, C, s, int(shrink))
            g.check()
            res.append(out.cpu())
        return tuple(res)

    f32, q = two_fills(run)
    assert not has_nan(f32)
    want = np.stack([utils.imresize_host(f, scale) for f in frames])
    assert float(np.abs(f32.numpy().astype(np.float64) - want).max()) <= 1e-6
    check_quantised(down(q, dtype), np.stack([utils.imresize_host(f, scale, out="same") for f in frames]),
                    f"guarded resize {scale} {dtype.__name__} C{C}")


@pytest.mark.parametrize("dtype,C", FRAME_KINDS)
@pytest.mark.parametrize("H,W", [(7, 7), (13, 23)])
def test_frame_metrics(dev, dtype, C, H, W):
    """7 x 7 (one interior pixel) and 13 x 23 (odd sides); K = 2; ws_words exactly the header's minimum.  The squared
    error is exact, SSIM within 1e-9 of the host (frame_checks.metric_parity)."""
    K = 2
    rng = np.random.default_rng(19)
    tgt = _frame(rng, (K, H, W, C), dtype)
    peak = 255 if dtype == np.uint8 else 65535
    pred = np.clip(tgt.astype(np.int64) + rng.integers(-40, 41, size=tgt.shape) * (peak // 255), 0, peak).astype(dtype)
    words = 2 * K * -(-(H - 6) // 16) * -(-(W - 6) // (192 // C))

    def run(fill):
        g = Guards(dev)
        sse, ssim, ws = g.out("sse", (K,), torch.int64), g.out("ssim", (K,), torch.float64), g.out("ws", (words,), torch.float64)
        _hip.call("irm_frame_metrics", _hip.ptr(g.inp(up(pred, "cpu"), fill=fill)), _hip.ptr(g.inp(up(tgt, "cpu"), fill=fill)),
                  int(dtype == np.uint16), K, H, W, C, float(peak), _hip.ptr(sse), _hip.ptr(ssim), _hip.ptr(ws), words)
        g.check()
        return sse.cpu(), ssim.cpu()

    sse, ssim = two_fills(run)
    for k in range(K):
        assert int(sse[k]) == int(((pred[k].astype(np.int64) - tgt[k].astype(np.int64)) ** 2).sum())
        host = utils.calculate_metrics(pred[k] if C == 3 else pred[k, :, :, 0], tgt[k] if C == 3 else tgt[k, :, :, 0])[1]
        assert abs(float(ssim[k]) - host) <= 1e-9, (k, float(ssim[k]), host)


@pytest.mark.parametrize("dtype,C", FRAME_KINDS)
@pytest.mark.parametrize("H,W,crop,y", [(15, 15, 2, 0), (15, 20, 2, 1), (11, 24, 0, 0)])
def test_frame_metrics_basicsr(dev, dtype, C, H, W, crop, y):
    """Cropped sides of 11 (one valid SSIM pixel) and one larger; K = 2; ws_words exactly the header's minimum with
    Ce = test_y_channel ? 1 : C.  PSNR and SSIM within 1e-9 of the host (test_gpu_sr_protocol)."""
    K = 2
    rng = np.random.default_rng(23)
    tgt = _frame(rng, (K, H, W, C), dtype)
    peak = 255 if dtype == np.uint8 else 65535
    pred = np.clip(tgt.astype(np.int64) + rng.integers(-40, 41, size=tgt.shape) * (peak // 255), 0, peak).astype(dtype)
    ce = 1 if y else C
    words = 2 * K * -(-(H - 2 * crop - 10) // 16) * -(-(W - 2 * crop - 10) // (192 // ce))

    def run(fill):
        g = Guards(dev)
        sse = g.out("sse", (K,), torch.float64 if y else torch.int64)
        ssim, ws = g.out("ssim", (K,), torch.float64), g.out("ws", (words,), torch.float64)
        _hip.call("irm_frame_metrics_basicsr", _hip.ptr(g.inp(up(pred, "cpu"), fill=fill)), _hip.ptr(g.inp(up(tgt, "cpu"), fill=fill)),
                  int(dtype == np.uint16), K, H, W, C, crop, y, 0, _hip.ptr(sse), _hip.ptr(ssim), _hip.ptr(ws), words)
        g.check()
        return sse.cpu(), ssim.cpu()

    sse, ssim = two_fills(run)
    n = (H - 2 * crop) * (W - 2 * crop) * ce
    for k in range(K):
        hp, hs = utils.calculate_metrics_basicsr(pred[k], tgt[k], crop, bool(y), "rgb")
        p = float("inf") if float(sse[k]) == 0 else float(10 * np.log10(float(peak) ** 2 / (float(sse[k]) / n)))
        assert abs(p - hp) <= 1e-9 and abs(float(ssim[k]) - hs) <= 1e-9, (k, p, hp, float(ssim[k]), hs)


@pytest.mark.parametrize("dtype,C", FRAME_KINDS)
def test_niqe_features(dev, dtype, C):
    """The smallest frame with two blocks, 1 x 2 of them, plus the crop and 5 spare columns (an odd width); K = 2;
    feat_words exactly 36 K nbh nbw; window and table between NaN.  Bound: niqe.json device_vs_host x MARGIN."""
    K, crop = 2, 2
    H, W = 96 + 2 * crop, 2 * 96 + 2 * crop + 5
    with open(os.path.join(GOLDEN, "niqe.json")) as f:
        meta = json.load(f)
    params = utils.load_niqe_params(os.path.join(GOLDEN, "niqe_pris_params.npz"))
    rng = np.random.default_rng(29)
    frames = _frame(rng, (K, H, W, C), dtype)
    gam, r_gam = utils.niqe_gamma_table()
    window = torch.from_numpy(np.ascontiguousarray(params["gaussian_window"][::-1, ::-1]))
    table = torch.from_numpy(np.stack([r_gam, gam])).contiguous()
    nblk = 2

    def run(fill):
        g = Guards(dev)
        feat = g.out("feat", (K, nblk, 36), torch.float64)
        _hip.call("irm_niqe_features", _hip.ptr(g.inp(up(frames, "cpu"), fill=fill)), int(dtype == np.uint16), K, H, W, C, crop, 1,
                  _hip.ptr(g.inp(window)), _hip.ptr(g.inp(table)), _hip.ptr(feat), 36 * K * nblk)
        g.check()
        return (feat.cpu(),)

    feat, = two_fills(run)
    for k in range(K):
        check_against_host(feat[k].numpy(), frames[k] if C == 3 else frames[k, :, :, 0], crop, params, meta,
                           f"guarded niqe {dtype.__name__} C{C} frame {k}")


# --------------------------------------------------------------------------- conv3x3 family
def _conv_ref(x, w, b, act1, slope, r, res_mode, shuffle):
    ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=1)
    ref = F.relu(ref) if act1 == 1 else F.leaky_relu(ref, slope) if act1 == 2 else ref
    if res_mode == 1:
        ref = ref + r.double()
    elif res_mode == 3:
        ref = torch.clamp(torch.tanh(ref) + r.double(), -1, 1)
    return F.pixel_shuffle(ref, shuffle) if shuffle else ref


@pytest.mark.parametrize("res_mode", [1, 3])
@pytest.mark.parametrize("ci,co", [(3, 48), (64, 1), (6, 2)])
def test_conv3x3_thin(dev, ci, co, res_mode):
    """H = 5, W = 8 (two float4 per row, an odd height), B = 2; x, res and y with batch slack.  Bar of test_conv3x3_thin."""
    B, H, W = 2, 5, 8
    tag = f"th{ci}_{co}"
    w, x = rnd(tag + "w", (co, ci, 3, 3), -0.3, 0.3), rnd(tag + "x", (B, ci, H, W), -1.5, 2.0)
    bv, r = rnd(tag + "b", (co,)), rnd(tag + "r", (B, co, H, W))
    ref = _conv_ref(x, w, bv, 0, 0.0, r, res_mode, 0)
    g = Guards(dev)
    y = g.out("y", (B, co, H, W), slack=SLACK)
    cw = _hip.ConvWeight(None, raw=g.inp(w))
    timer, ops.TIMER = ops.TIMER, ops.KernelTimer()
    try:
        ops.conv3x3(cw, g.inp(x, SLACK), y, ci, co, bias=g.inp(bv), res=g.inp(r, SLACK), res_mode=res_mode)
        assert list(ops.TIMER.summary()) == ["conv3x3_thin"]
    finally:
        ops.TIMER = timer
    g.check()
    assert float((clean(y).double() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("kernel", ["exact", "split"])
@pytest.mark.parametrize("co,shuffle,leaky", [(27, 3, None), (48, 4, None), (40, 0, 0.1)])
def test_conv3x3_sr_epilogues(dev, kernel, co, shuffle, leaky):
    """irm_conv3x3_ep_f32 / irm_conv3x3_f16x3_ep_f32: PixelShuffle 3 and 4, LeakyReLU; Co = 27, 48, 40 with ct = 2 (no
    multiple of 32 output channels: a ragged last pass), W = 12 (a partial 32-pixel tile), H = 5; x and y with batch
    slack.  Bar of test_conv3x3_sr_epilogues_vs_float64."""
    B, ci, H, W = 2, 20, 5, 12
    tag = f"ep{co}_{shuffle}"
    x, w, b = rnd(tag + "x", (B, ci, H, W)), rnd(tag + "w", (co, ci, 3, 3), -0.1, 0.1), rnd(tag + "b", (co,), -0.5, 0.5)
    ref = _conv_ref(x, w, b, 2 if leaky is not None else 0, leaky, None, 0, shuffle)
    g = Guards(dev)
    if kernel == "exact":
        wp = g.inp(_hip.pack_conv3x3_weight(w))
    else:
        split, inv = _hip.pack_conv3x3_weight_split(w)
        wp = (g.inp(split), inv)
    y = g.out("y", tuple(ref.shape), slack=SLACK)
    kw = dict(store_mode=2, shuffle=shuffle) if shuffle else dict(leaky=leaky)
    ops.conv3x3(wp, g.inp(x, SLACK), y, ci, co, bias=g.inp(b), ct=2, **kw)
    g.check()
    assert float((clean(y).double() - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("kernel", ["exact", "split"])
def test_conv3x3_plain_entry_points(dev, kernel):
    """irm_conv3x3_f32 / irm_conv3x3_f16x3_f32 (the entry points without the SR epilogue arguments) with a residual:
    x, res and y with batch slack.  Bar of test_conv3x3 (2e-4)."""
    B, ci, co, H, W = 2, 20, 40, 5, 12
    x, w, b = rnd("px", (B, ci, H, W)), rnd("pw", (co, ci, 3, 3), -0.1, 0.1), rnd("pb", (co,), -0.5, 0.5)
    r = rnd("pr", (B, co, H, W))
    ref = _conv_ref(x, w, b, 1, 0.0, r, 1, 0)
    g = Guards(dev)
    xv, rv, y = g.inp(x, SLACK), g.inp(r, SLACK), g.out("y", (B, co, H, W), slack=SLACK)
    tail = (_hip.ptr(xv), xv.stride(0), _hip.ptr(y), y.stride(0), _hip.ptr(rv), rv.stride(0), _hip.ptr(g.inp(b)), B, ci, co, H, W,
            1, 1, 0, 0, 2, 1)
    if kernel == "exact":
        _hip.call("irm_conv3x3_f32", _hip.ptr(g.inp(_hip.pack_conv3x3_weight(w))), *tail)
    else:
        split, inv = _hip.pack_conv3x3_weight_split(w)
        _hip.call("irm_conv3x3_f16x3_f32", _hip.ptr(g.inp(split)), float(inv), *tail)
    g.check()
    assert float((clean(y).double() - ref).abs().max()) <= 2e-4


# --------------------------------------------------------------------------- dwgemm.hip
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("M,K,H,W", [(40, 6, 5, 4), (96, 96, 21, 40)])
def test_dwgemm(dev, M, K, H, W, gate, split):
    """5 x 4 (less than one 8 x 32 tile, one float4 per row) and 21 x 40 (partial tiles on both axes); M = 40 leaves a
    partial output tile, K = 6 a partial stage.  In place on the residual, with the statistics of the result.
    Bars of test_dwgemm."""
    B = 2
    assert ops.can_fuse_dw(M, W)
    kin = 2 * K if gate else K
    tag = f"dg{M}{K}{H}{int(gate)}"
    x, w9, dwb = rnd(tag + "x", (B, kin, H, W), -1.5, 1.5), rnd(tag + "w9", (kin, 9), -0.5, 0.5), rnd(tag + "db", (kin,), -0.2, 0.2)
    wt, pb, r = rnd(tag + "w", (M, K), -0.2, 0.2), rnd(tag + "b", (M,), -0.3, 0.3), rnd(tag + "r", (B, M, H, W))
    d = F.conv2d(x.double(), w9.double().view(kin, 1, 3, 3), dwb.double(), padding=1, groups=kin)
    gd = F.gelu(d[:, :K]) * d[:, K:] if gate else d
    ref = torch.einsum("mk,bkhw->bmhw", wt.double(), gd) + pb.double().view(1, M, 1, 1) + r.double()
    g = Guards(dev)
    packed = g.inp((_hip.pack_gemm_weight_split if split else _hip.pack_gemm_weight)(wt))
    y, st = g.out("y", (B, M, H, W), slack=SLACK), g.out("stats", (B, 2, H * W))
    y.copy_(r)
    ops.dwgemm(packed, g.inp(_hip.pack_dw_table(w9, dwb, K, gate)), g.inp(x, SLACK), y, M, K, gate=gate, res=y, bias=g.inp(pb),
               stats_out=st, split=split)
    g.check()
    assert float((clean(y).double() - ref).abs().max()) < 2e-4
    sc = clean(st).double()
    rstd = 1.0 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5).reshape(B, -1)
    assert float((sc[:, 0] - ref.mean(1).reshape(B, -1)).abs().max()) < 1e-4
    assert float(((sc[:, 1] - rstd).abs() / rstd).max()) < 1e-4


# --------------------------------------------------------------------------- gemm_ps.hip, fused_tail.hip (C = 192)
def _ps_operands(tag, M, K, ln):
    w, lnw = rnd(tag + "w", (M, K), -0.3, 0.3), rnd(tag + "lw", (K,), 0.5, 1.5)
    lnb = rnd(tag + "lb", (K,), -0.2, 0.2) if ln == 1 else None
    return w, lnw, lnb, rnd(tag + "b", (M,), -0.3, 0.3)


@pytest.mark.parametrize("ln", [1, 2])
def test_presplit_gemms(dev, ln):
    """K = 192 at N = 16, the smallest can_presplit admits (one pixel tile per image, B = 2), M = 40 (a partial output
    tile): irm_ln_split_f16 + irm_gemm_presplit_f16x3_f32 with xs at exactly B K N floats, and the one-launch
    irm_ln_gemm_presplit_f16x3_f32.  Bar of test_gemm_presplit / test_ln_gemm_presplit_fused (2e-5)."""
    B, M, K, H, W = 2, 40, 192, 4, 4
    N = H * W
    assert ops.can_presplit(K, N)
    w, lnw, lnb, bv = _ps_operands(f"ps{ln}", M, K, ln)
    x = rnd(f"psx{ln}", (B, K, H, W), -2, 3)
    ref = torch.einsum("mk,bkhw->bmhw", w.double(), bm.layer_norm(x.double(), lnw, lnb, ln)) + bv.double().view(1, M, 1, 1)
    frag, s_w = _hip.pack_gemm_weight_presplit(w)
    s_x = _hip.ln_split_scale(lnw, lnb, K, ln == 1)
    g = Guards(dev)
    xv, fv, lw, lb, bg = g.inp(x, SLACK), g.inp(frag), g.inp(lnw), g.inp(lnb), g.inp(bv)
    xs, y = g.out("xs", (B * K * N,)), g.out("y pair", (B, M, H, W), slack=SLACK)
    ops.ln_split(xv, xs, lw, lb, ln, s_x)
    ops.gemm_presplit(fv, xs, y, M, K, out_scale=1.0 / (s_w * s_x), bias=bg)
    assert _hip.plan_presplit((M + 15) // 16, B * N // 16, K)[1] == 1          # ln_gemm_presplit takes the one-launch kernel
    y1 = g.out("y fused", (B, M, H, W), slack=SLACK)
    ops.ln_gemm_presplit(fv, xv, y1, M, K, lw, lb, ln, s_x, out_scale=1.0 / (s_w * s_x), bias=bg)
    g.check()
    assert not has_nan(xs.cpu())
    assert float((clean(y).double() - ref).abs().max()) < 2e-5
    assert float((clean(y1).double() - ref).abs().max()) < 2e-5


@pytest.mark.parametrize("ln", [1, 2])
def test_gdfn_tail_c192(dev, ln):
    """irm_ln_gemm_presplit_cl_f16x3_f32 + irm_gdfn_tail_f16x3_f32 on one 8 x 32 tile per image, the smallest
    can_gdfn_tail admits; hid = 100 (a partial 16-channel stage) padded to 128; h_cl at exactly B 2 hid_pad N floats; x in
    place with batch slack.  Bar of test_gdfn_tail_c192."""
    B, C, hid, hp, H, W = 2, 192, 100, 128, 8, 32
    assert ops.can_gdfn_tail(C, H, W)
    tag = f"gt{ln}"
    x = rnd(tag + "x", (B, C, H, W), -1.5, 2.0)
    lnw, lnb, pin_w, pin_b, dw_w, dw_b, pout_w, pout_b = bm.gdfn_operands(rnd, tag, C, hid, ln, ws=0.2)
    ref = bm.gdfn(x.double(), lnw, lnb, ln, pin_w, pin_b, dw_w, dw_b, pout_w, pout_b)
    frag, s_w, bp = _hip.pack_pin_padded(pin_w, pin_b, hp)
    s_x = _hip.ln_split_scale(lnw, lnb, C, ln == 1)
    rec, w2, inv_s2 = _hip.pack_gdfn_tail(dw_w, dw_b, pout_w)
    g = Guards(dev)
    xv, h_cl = g.out("x", (B, C, H, W), slack=SLACK), g.out("h_cl", (B * 2 * hp * H * W,))
    xv.copy_(x)
    ops.ln_gemm_presplit_cl(g.inp(frag), xv, h_cl, 2 * hp, C, g.inp(lnw), g.inp(lnb), ln, s_x, out_scale=1.0 / (s_w * s_x),
                            bias=g.inp(bp))
    ops.gdfn_tail((g.inp(rec), g.inp(w2), inv_s2), h_cl, xv, C, hid, hp, bias=g.inp(pout_b))
    g.check()
    assert not has_nan(h_cl.cpu())
    assert float((clean(xv).double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))


# --------------------------------------------------------------------------- fused_block.hip, fused_qkv_cm.hip (C = 48 / 96)
def test_attn_gdfn_fused(dev):
    """C = 48, hid = 127, 9 x 36 (a partial 8 x 32 tile on both axes, W % 4 == 0: the smallest family can_fuse_gdfn
    admits with more than one tile); x, v and y with batch slack.  Bar of test_attn_gdfn_fused."""
    B, C, hid, H, W, ln = 2, 48, 127, 9, 36, 1
    assert ops.can_fuse_gdfn(C, W)
    tag = "ag"
    x, v, mf = rnd(tag + "x", (B, C, H, W), -1.5, 2.0), rnd(tag + "v", (B, C, H, W), -2.0, 2.0), rnd(tag + "m", (B, C, C), -0.2, 0.2)
    lnw, lnb, pin_w, pin_b, dw_w, dw_b, pout_w, pout_b = bm.gdfn_operands(rnd, tag, C, hid, ln)
    bo = rnd(tag + "bo", (C,), -0.3, 0.3)
    x1 = x.double() + torch.einsum("bij,bjhw->bihw", mf.double(), v.double()) + bo.double()[None, :, None, None]
    ref = bm.gdfn(x1, lnw, lnb, ln, pin_w, pin_b, dw_w, dw_b, pout_w, pout_b)
    rec, w2, inv_s1, inv_s2 = _hip.pack_gdfn_fused(pin_w, pin_b, dw_w, dw_b, pout_w, lnw, lnb, kperm=True)
    g = Guards(dev)
    y = g.out("y", (B, C, H, W), slack=SLACK)
    ops.attn_gdfn_fused((g.inp(rec), g.inp(w2), inv_s1, inv_s2), g.inp(x, SLACK), g.inp(v, SLACK), g.inp(_hip.pack_mfold_frag(mf)), y,
                        C, hid, ln_mode=ln, bias_o=g.inp(bo), bias=g.inp(pout_b))
    g.check()
    assert float((clean(y).double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))


def _qkv_operands(tag, C):
    M = 3 * C
    lnw, lnb = rnd(tag + "lw", (C,), 0.5, 1.5), rnd(tag + "lb", (C,), -0.2, 0.2)
    w, dw_w = rnd(tag + "w", (M, C), -0.3, 0.3), rnd(tag + "dw", (M, 9), -0.4, 0.4)
    gs = _hip.gram_scales(w.view(M, C, 1, 1), None, dw_w.view(M, 1, 3, 3), None, lnw, lnb, True)
    return lnw, lnb, w, dw_w, gs



@pytest.mark.parametrize("C", [48, 96])
def test_qkv_tile_major_and_gram_tm(dev, C):
    """qkv_dw_fused(tm=True) - irm_qkv_dw_cm_f16x3_f32 at C = 48, irm_qkv_dw_fused_tm_f16x3_f32 at C = 96 - on one 8 x 32
    tile per image (N = 256: the smallest can_qk_tile_major admits), x and y with batch slack; then both tile-major Gram
    passes (f16x3 with operand scales, f32 ring) and the fragment finalize, workspaces at their record sizes.
    Bars: test_qkv_dw_fused (2e-5) for q, k, v; test_mdta_fold (2e-5 on the attention matrix, 1e-6 on the fragments)."""
    B, heads, H, W = 2, 1, 8, 32
    M, N = 3 * C, H * W
    assert ops.can_qk_tile_major(C, heads, H, W) and ops._use_qkv_cm(C) == (C == 48)
    tag = f"tm{C}"
    lnw, lnb, w, dw_w, gs = _qkv_operands(tag, C)
    x = rnd(tag + "x", (B, C, H, W), -1.5, 2.0)
    temp, wout = rnd(tag + "t", (heads,), 2.0, 6.0), rnd(tag + "wo", (C, C), -0.3, 0.3)
    ref = bm.qkv(x.double(), lnw, lnb, 1, w, None, dw_w, None)
    rec, inv_s1 = _hip.pack_qkv_fused(w, None, dw_w, None, lnw, lnb)
    g = Guards(dev)
    qkv = g.out("qkv", (B, M, H, W), slack=SLACK)
    ops.qkv_dw_fused((g.inp(rec), inv_s1), g.inp(x, SLACK), qkv, C, M, ln_mode=1, tm=True)
    g.check()
    got = clean(qkv)
    planar = torch.cat([bm.qk_from_tm(got[:, :2 * C]), got[:, 2 * C:]], 1)
    assert float((planar.double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    aref = bm.attention_qk(ref[:, :2 * C], temp, heads)
    tg, wg = g.inp(temp), g.inp(wout)
    for scale in (g.inp(gs), None):
        attn, _ = guarded_fold(g, qkv, B, C, heads, N, tg, wg, gram_scale=scale, tm=True)
        g.check()
        assert float((clean(attn).double() - aref).abs().max()) < 2e-5
    attn, mfrag = guarded_fold(g, qkv, B, C, heads, N, tg, wg, gram_scale=g.inp(gs), tm=True, frag=True)
    g.check()
    a = clean(attn).double()
    mref = torch.stack([wout.double() @ torch.block_diag(*a[i]) for i in range(B)])
    assert float((_hip.unpack_mfold_frag(clean(mfrag), B, C).double() - mref).abs().max()) < 1e-6 * max(1.0, float(mref.abs().max()))


def test_qkv_gram_cm(dev):
    """irm_qkv_gram_cm_f16x3_f32 at 32 x 32, the smallest can_qkv_gram admits (4 tiles = one record per image), B = 2;
    part at exactly B nchunk 2400 floats; q, k are never written (their part of y keeps the sentinel), v against float64
    (bar of test_qkv_dw_fused), the attention matrix of the records against float64 (bar of test_mdta_fold)."""
    B, C, heads, H, W = 2, 48, 1, 32, 32
    M, N = 3 * C, H * W
    assert ops.can_qkv_gram(C, heads, H, W)
    lnw, lnb, w, dw_w, gs = _qkv_operands("qg", C)
    x = rnd("qgx", (B, C, H, W), -1.5, 2.0)
    temp, wout = rnd("qgt", (heads,), 2.0, 6.0), rnd("qgwo", (C, C), -0.3, 0.3)
    ref = bm.qkv(x.double(), lnw, lnb, 1, w, None, dw_w, None)
    rec, inv_s1 = _hip.pack_qkv_fused(w, None, dw_w, None, lnw, lnb)
    nchunk = (H // 8) * (W // 32) // ops.QKV_GRAM_NCH
    g = Guards(dev)
    qkv, part = g.out("qkv", (B, M, H, W), slack=SLACK), g.out("part", (B * nchunk * (C * C + 2 * C),))
    gsc = g.inp(gs)
    assert ops.qkv_gram_cm((g.inp(rec), inv_s1), g.inp(x, SLACK), qkv, gsc, part, C, ln_mode=1) == nchunk
    g.check()
    assert bool((qkv[:, :2 * C] == 12345.0).all()), "q, k must not be written"
    v = clean(qkv[:, 2 * C:])
    assert float((v.double() - ref[:, 2 * C:]).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    attn, _ = guarded_fold(g, qkv, B, C, heads, N, g.inp(temp), g.inp(wout), part=part, nready=nchunk, gram_scale=gsc, tm=True)
    g.check()
    assert float((clean(attn).double() - bm.attention_qk(ref[:, :2 * C], temp, heads)).abs().max()) < 2e-5
