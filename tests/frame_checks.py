"""Checkers of the frame-level device paths against their host restatements, shared by each family's own GPU test and
tests/test_gpu_guard_bands.py: the bicubic resize and its quantised output, the NIQE features, PSNR / SSIM parity, and
the packed buffers of the x8 self-ensemble with the float64 restatement of its merge."""
import numpy as np
import torch

from irm_amd import ensemble, utils

#: margin on the distances recorded in tests/golden/niqe.json (host_vs_reference by the generator, device_vs_host by its
#: --device-bound run on an MI355X)
NIQE_MARGIN = 4.0


def up(a: np.ndarray, dev) -> torch.Tensor:
    """A uint8 / uint16 host frame on the GPU (uint16 as its int16 bit pattern)."""
    return torch.from_numpy(np.ascontiguousarray(a.view(np.int16) if a.dtype == np.uint16 else a)).to(dev)


def down(t: torch.Tensor, dtype=None) -> np.ndarray:
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


# --------------------------------------------------------------------------- resize
def quantise_ref(x32):
    """tensor2img on the reference's fp32 result: clamp, x 255 in fp32, round half to even."""
    return (np.clip(x32, np.float32(0), np.float32(1)) * 255.0).round().astype(np.uint8)


def check_quantised(got, ref, what):
    """Every value within 1 of the reference's, differing values at most 1e-3 of the frame for bytes.  Where that share
    comes from: two results that agree to 1e-6 before rounding (the float bound below) round differently only when
    one lies within 1e-6 of a rounding boundary, i.e. for at most 2 x 1e-6 x R of uniformly placed values: 5.1e-4
    for R = 255, under the 1e-3 of the byte rule.  uint16 steps are 257 times finer, so the same reasoning gives
    2 x 1e-6 x 65535 = 0.131 there (the values still within 1)."""
    diff = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    share = float((diff > 0).mean())
    limit = 1e-3 if got.dtype == np.uint8 else 2 * 1e-6 * 65535
    print(f"{what}: max difference {int(diff.max())}, differing share {share:.2e} ({int((diff > 0).sum())} of {diff.size})")
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert int(diff.max()) <= 1 and share <= limit


def check_resize(src, scale, dev, what):
    """Device float output within 1e-6 of imresize_host (an fp32 chain of at most 18 taps on values in [0, 1]), the
    quantised output by the byte rule; returns the device float result."""
    want = utils.imresize_host(src, scale)
    got = utils.imresize_device(up(src, dev), scale, out="float")
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: {src.shape} {src.dtype} -> {got.shape}, device fp32 vs float64 host max-abs {err:.3e}")
    assert err <= 1e-6
    q = utils.imresize_device(up(src, dev), scale, out="same")
    check_quantised(down(q, src.dtype), utils.imresize_host(src, scale, out="same"), what + " quantised")
    return got


# --------------------------------------------------------------------------- NIQE
def check_against_host(dev_feat, frame, crop, params, meta, what, order="bgr"):
    """alpha: equal, or one grid step apart in at most one entry of the frame; the other features and the score within
    4 x the distance measured on an MI355X (niqe.json, device_vs_host).  Returns (host score, device score)."""
    bound = meta["device_vs_host"]
    host = utils.niqe_features(utils.niqe_plane(frame, crop, "HWC", order), params)
    differing, steps, rel = utils.niqe_feature_distance(dev_feat, host)
    hs, ds = utils.niqe_score(host, params), utils.niqe_score(dev_feat, params)
    srel = abs(ds - hs) / abs(hs)
    print(f"{what}: alpha differing {differing} (max {steps:.3g} steps), features {rel:.3e}, score {ds:.12f} vs host "
          f"{hs:.12f} ({srel:.3e})")
    assert dev_feat.shape == host.shape
    assert differing <= 1 and steps <= 1.0 + 1e-6
    assert rel <= NIQE_MARGIN * bound["features_rel"]
    assert srel <= NIQE_MARGIN * bound["score_rel"]
    return hs, ds


# --------------------------------------------------------------------------- PSNR / SSIM
def up16(x: np.ndarray, dev) -> torch.Tensor:
    """numpy uint8 / uint16 frame -> device tensor (uint16 through its int16 bits, then viewed back)."""
    return up(x, dev).view(torch.uint16) if x.dtype == np.uint16 else up(x, dev)


def metric_parity(pred: np.ndarray, tgt: np.ndarray, dev, data_range=None):
    """utils.calculate_metrics_device within 1e-9 of the float64 host restatement; returns the device (PSNR, SSIM)."""
    ph, sh = utils.calculate_metrics(pred, tgt, data_range)
    pd, sd = utils.calculate_metrics_device(up16(pred, dev), up16(tgt, dev), data_range)
    assert abs(sd - sh) <= 1e-9, (pred.shape, sd, sh)
    assert (pd == ph == float("inf")) or abs(pd - ph) <= 1e-9, (pred.shape, pd, ph)
    return pd, sd


# --------------------------------------------------------------------------- x8 self-ensemble
def packed_blocks(buf, geo, B, C, s=1):
    """packed buffer -> blocks[variant][partition] = [B, C, s ph, s pw] views, grid order."""
    out = [[] for _ in range(8)]
    for row in geo.table[8:]:
        e, _, _, ph, pw, off = (int(v) for v in row[:6])
        out[e].append(buf[off * C * s * s:(off + B * ph * pw) * C * s * s].view(B, C, s * ph, s * pw))
    return out


def merge_float64(blocks, H, W, s, chop):
    """numpy float64 restatement of one_img_test's stitch (:65-77, x s), the crop (:103) and gather (:107-117)."""
    total = 0.0
    for v in range(8):
        p = ensemble.plan(H, W, v, chop)
        (ha, wa), (nh, nw) = p.size, p.grid
        B, Co = blocks[v][0].shape[:2]
        img = np.zeros((B, Co, s * (ha + p.pad[0]), s * (wa + p.pad[1])))
        for i in range(nh):
            for j in range(nw):
                top, left = (0 if i == 0 else p.shave[0] * s), (0 if j == 0 else p.shave[1] * s)
                img[:, :, i * p.split[0] * s:(i + 1) * p.split[0] * s, j * p.split[1] * s:(j + 1) * p.split[1] * s] = \
                    blocks[v][i * nw + j][:, :, top:top + p.split[0] * s, left:left + p.split[1] * s]
        img = img[:, :, :s * ha, :s * wa]
        if v >= 4:
            img = img.transpose(0, 1, 3, 2)
        if v & 2:
            img = img[:, :, :, ::-1]
        if v & 1:
            img = img[:, :, ::-1, :]
        total = total + img
    return total / 8.0
