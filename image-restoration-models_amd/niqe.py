"""No-reference quality: NIQE (basicsr/metrics/niqe.py), restated in float64 on the host, the
block features on the GPU (irm_niqe_features)."""
from __future__ import annotations

import numpy as np
import torch

from . import _hip
from .frames import check_order_and_crop, device_constant, device_frames, frame_bits

_NIQE_BLOCK = 96
_NIQE_SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
_NIQE_KEYS = {"mu_pris_param": (1, 36), "cov_pris_param": (36, 36), "gaussian_window": (7, 7)}


def load_niqe_params(path) -> dict:
    """The pristine model NIQE scores against, from an .npz with the reference's three keys (its
    niqe_pris_params.npz): mu_pris_param 1x36, cov_pris_param 36x36, gaussian_window 7x7, as float64.  The package
    ships no copy: the caller names the file, as for weights.  ValueError for a missing key or another shape."""
    with np.load(path) as z:
        missing = [k for k in _NIQE_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: no {', '.join(missing)} (keys: {', '.join(z.files)})")
        params = {k: np.array(z[k], dtype=np.float64) for k in _NIQE_KEYS}
    _check_niqe_params(params)
    return params


def _check_niqe_params(params) -> None:
    if not isinstance(params, dict):
        raise ValueError("params must be what load_niqe_params returns")
    for k, shape in _NIQE_KEYS.items():
        if k not in params:
            raise ValueError(f"NIQE parameters: no {k}")
        if tuple(np.shape(params[k])) != shape:
            raise ValueError(f"NIQE parameters: {k} has shape {tuple(np.shape(params[k]))}, not {shape}")


def niqe_gamma_table() -> tuple:
    """(gam, r_gam) of the AGGD fit, float64, 9801 entries each: the grid arange(0.2, 10.001, 0.001) and
    gamma(2 / a)^2 / (gamma(1 / a) gamma(3 / a)) on it, as estimate_aggd_param builds them on every call."""
    from scipy.special import gamma
    gam = np.arange(0.2, 10.001, 0.001)
    rec = np.reciprocal(gam)
    return gam, np.square(gamma(rec * 2)) / (gamma(rec) * gamma(rec * 3))


def _aggd_fit(block: np.ndarray, gam: np.ndarray, r_gam: np.ndarray) -> tuple:
    """(alpha, beta_l, beta_r) of niqe.py:10-37; an empty side gives NaN quietly."""
    from scipy.special import gamma
    b = block.ravel()
    with np.errstate(invalid="ignore", divide="ignore"):
        neg, pos = b[b < 0], b[b > 0]
        left_std = np.sqrt(np.sum(neg ** 2) / neg.size) if neg.size else np.float64("nan")
        right_std = np.sqrt(np.sum(pos ** 2) / pos.size) if pos.size else np.float64("nan")
        gammahat = left_std / right_std
        rhat = np.mean(np.abs(b)) ** 2 / np.mean(b ** 2)
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
        alpha = gam[np.argmin((r_gam - rhatnorm) ** 2)]           # the first minimum; index 0 when all are NaN
        root = np.sqrt(gamma(1 / alpha) / gamma(3 / alpha))
    return alpha, left_std * root, right_std * root


def _niqe_block_features(block: np.ndarray, gam, r_gam) -> list:
    """The 18 features of niqe.py:40-64; np.roll wraps inside the block."""
    from scipy.special import gamma
    alpha, bl, br = _aggd_fit(block, gam, r_gam)
    feat = [alpha, (bl + br) / 2]
    for shift in _NIQE_SHIFTS:
        alpha, bl, br = _aggd_fit(block * np.roll(block, shift, axis=(0, 1)), gam, r_gam)
        feat.extend([alpha, (br - bl) * (gamma(2 / alpha) / gamma(1 / alpha)), bl, br])
    return feat


def niqe_features(y_plane: np.ndarray, params) -> np.ndarray:
    """The [n_blocks][36] NIQE feature matrix of a 2-D plane in the 0..255 range (niqe.py:101-140), in float64: the
    plane is cropped to whole 96x96 blocks; for scale 1 and 2 the 7x7-window mean and sqrt|E[x^2] - mu^2| (border
    mode `nearest`), the MSCN image, and per block - columns of blocks outer, rows inner - the AGGD fits of the block
    and of its four circularly rolled products.  Between the scales the plane is halved by the 2x2 mean (what the
    reference's bilinear resize to exactly half of even extents computes).  Fewer than two blocks: ValueError."""
    from scipy.ndimage import convolve
    _check_niqe_params(params)
    img = np.asarray(y_plane, dtype=np.float64)
    if img.ndim != 2:
        raise ValueError(f"niqe_features takes a 2-D plane, not shape {img.shape}")
    nbh, nbw = img.shape[0] // _NIQE_BLOCK, img.shape[1] // _NIQE_BLOCK
    if nbh * nbw < 2:
        raise ValueError(f"NIQE needs at least two 96x96 blocks; a {img.shape[0]}x{img.shape[1]} plane has {nbh * nbw}")
    img = img[:nbh * _NIQE_BLOCK, :nbw * _NIQE_BLOCK]
    window = params["gaussian_window"]
    gam, r_gam = niqe_gamma_table()
    per_scale = []
    for scale in (1, 2):
        mu = convolve(img, window, mode="nearest")
        sigma = np.sqrt(np.abs(convolve(np.square(img), window, mode="nearest") - np.square(mu)))
        mscn = (img - mu) / (sigma + 1)
        b = _NIQE_BLOCK // scale
        per_scale.append(np.array([_niqe_block_features(mscn[ih * b:(ih + 1) * b, iw * b:(iw + 1) * b], gam, r_gam)
                                   for iw in range(nbw) for ih in range(nbh)]))
        if scale == 1:
            img = (((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2]) * 0.25
    return np.concatenate(per_scale, axis=1)


def niqe_score(features: np.ndarray, params) -> float:
    """The NIQE value of a feature matrix (niqe.py:142-155), float64: nanmean over the blocks, the covariance of the
    NaN-free rows, pinv of the mean of the two covariances, the square root of the quadratic form."""
    _check_niqe_params(params)
    feats = np.asarray(features, dtype=np.float64)
    mu = np.nanmean(feats, axis=0)
    cov = np.cov(feats[~np.isnan(feats).any(axis=1)], rowvar=False)
    inv = np.linalg.pinv((params["cov_pris_param"] + cov) / 2)
    d = params["mu_pris_param"] - mu
    return float(np.sqrt(np.matmul(np.matmul(d, inv), d.T)).item())


def niqe_feature_distance(features: np.ndarray, reference: np.ndarray) -> tuple:
    """How far a [n_blocks][36] feature matrix is from a reference one, as the NIQE fixtures and tests measure it:
    (alpha_differing, alpha_max_steps, rel).  Columns 0, 2, 6, 10, 14 of each scale's 18 are grid values (alpha):
    the number of entries that differ and their largest distance in grid steps of 0.001.  For the other columns
    rel = max |a - b| / max(|b|, 0.01) (the floor keeps the near-zero `mean` features from dominating).  NaNs must sit
    in the same places, else rel is inf."""
    a, b = np.asarray(features, np.float64), np.asarray(reference, np.float64)
    if a.shape != b.shape or (np.isnan(a) != np.isnan(b)).any():
        return 0, 0.0, float("inf")
    is_alpha = np.zeros(36, bool)
    is_alpha[[0, 2, 6, 10, 14, 18, 20, 24, 28, 32]] = True
    da = np.abs(a[:, is_alpha] - b[:, is_alpha]) / 0.001
    ok = ~np.isnan(b[:, ~is_alpha])
    rel = np.abs(a[:, ~is_alpha] - b[:, ~is_alpha])[ok] / np.maximum(np.abs(b[:, ~is_alpha][ok]), 0.01)
    return int((da > 1e-6).sum()), float(da.max()), float(rel.max()) if rel.size else 0.0


def _check_niqe_args(crop_border, convert_to, channel_order) -> int:
    if convert_to == "gray":
        raise NotImplementedError("convert_to='gray' is OpenCV's grey conversion, which this package does not restate")
    if convert_to != "y":
        raise ValueError(f"convert_to must be 'y', not {convert_to!r}")
    return check_order_and_crop(channel_order, crop_border)


def _check_niqe_blocks(h: int, w: int, crop: int) -> tuple:
    hc, wc = h - 2 * crop, w - 2 * crop
    nbh, nbw = max(hc, 0) // _NIQE_BLOCK, max(wc, 0) // _NIQE_BLOCK
    if nbh * nbw < 2:
        raise ValueError(f"NIQE needs at least two 96x96 blocks: a {h}x{w} frame cropped by {crop} has {nbh * nbw} "
                         "(the covariance needs two rows; the reference yields NaN)")
    return nbh, nbw


def niqe_plane(img: np.ndarray, crop_border: int = 0, input_order: str = "HWC", channel_order: str = "bgr") -> np.ndarray:
    """The float64 plane calculate_niqe scores: HW / HWC / CHW frame -> BT.601 Y for 3 channels (to_y_channel on a
    float frame, unrounded: ((b / 255 x 24.966 + g / 255 x 128.553) + r / 255 x 65.481) + 16), the values themselves
    for one; cropped by crop_border.  Values are taken in the 0..255 range; uint16 frames are divided by 257 first."""
    if not isinstance(img, np.ndarray):
        raise ValueError("calculate_niqe takes numpy arrays (calculate_niqe_device takes GPU tensors)")
    if input_order not in ("HW", "HWC", "CHW"):
        raise ValueError(f"input_order must be 'HW', 'HWC' or 'CHW', not {input_order!r}")
    x = img.astype(np.float64) / 257.0 if img.dtype == np.uint16 else img.astype(np.float64)
    if x.ndim == 2:
        x = x[..., None]
    elif input_order == "CHW":
        x = x.transpose(1, 2, 0)
    if x.ndim != 3 or x.shape[2] not in (1, 3):
        raise ValueError(f"calculate_niqe takes frames with 1 or 3 channels, not shape {img.shape}")
    if x.shape[2] == 3:
        b, r = (x[..., 0], x[..., 2]) if channel_order == "bgr" else (x[..., 2], x[..., 0])
        y = (((b / 255.0) * 24.966 + (x[..., 1] / 255.0) * 128.553) + (r / 255.0) * 65.481) + 16.0
    else:
        y = x[..., 0]
    return y[crop_border:y.shape[0] - crop_border, crop_border:y.shape[1] - crop_border]


def calculate_niqe(img: np.ndarray, crop_border: int, params, input_order: str = "HWC", convert_to: str = "y",
                   channel_order: str = "bgr") -> float:
    """NIQE of one frame without a target (basicsr's calculate_niqe restated in float64; lower is better).  `img`:
    values in the 0..255 range, any real dtype (uint16 frames are divided by 257), HW / HWC / CHW; 3 channels are read
    in `channel_order` (the reference reads BGR) and converted to the Y channel.  `params` comes from
    load_niqe_params.  A frame with fewer than two 96x96 blocks after the crops raises ValueError;
    convert_to='gray' raises NotImplementedError."""
    crop = _check_niqe_args(crop_border, convert_to, channel_order)
    _check_niqe_params(params)
    plane = niqe_plane(img, crop, input_order, channel_order)
    _check_niqe_blocks(plane.shape[0] + 2 * crop, plane.shape[1] + 2 * crop, crop)
    return niqe_score(niqe_features(plane, params), params)


def _niqe_tables_on(device, window: np.ndarray) -> tuple:
    """(window, table) on the device: the 49 weights flipped for the kernel's correlation (scipy's convolve flips
    them) and [r_gam, gam] as one [2][9801] float64 tensor, built once on the host in float64 and cached per device
    like the resize tables."""
    def build():
        gam, r_gam = niqe_gamma_table()
        return (torch.from_numpy(np.ascontiguousarray(window[::-1, ::-1])).to(device),
                torch.from_numpy(np.stack([r_gam, gam])).contiguous().to(device))
    return device_constant(("niqe", str(device), window.tobytes()), build)


def niqe_features_device(frames, crop_border: int, params, channel_order: str = "rgb") -> torch.Tensor:
    """NIQE block features on the GPU (irm_niqe_features): `frames` is one uint8 / uint16 (or int16 = uint16 bit
    pattern) HW / HWC GPU tensor, a [K][H][W][C] stack, or a list of K frames of one shape.  Returns the
    [K][n_blocks][36] float64 device tensor of niqe_features' rows (fp64 arithmetic throughout), without
    synchronising; a frame's features are bitwise the same on every call and for any K.  CPU tensors raise
    HipLibraryError: there is no CPU fallback (niqe_features takes host planes)."""
    crop = _check_niqe_args(crop_border, "y", channel_order)
    _check_niqe_params(params)
    items, k, h, w, c, stacked = device_frames(frames, "the device NIQE", "calculate_niqe takes numpy arrays", "NIQE")
    nbh, nbw = _check_niqe_blocks(h, w, crop)
    f0 = items[0]
    if not f0.is_cuda:
        raise _hip.HipLibraryError("the device NIQE needs GPU tensors; there is no CPU fallback (calculate_niqe takes "
                                   "host arrays)")
    dev = f0.device
    with torch.cuda.device(dev):
        src = frame_bits(items, stacked)
        window, table = _niqe_tables_on(dev, params["gaussian_window"])
        feat = torch.empty((k, nbh * nbw, 36), dtype=torch.float64, device=dev)
        _hip.call("irm_niqe_features", _hip.ptr(src), int(f0.dtype != torch.uint8), k, h, w, c, crop,
                  int(channel_order == "bgr"), _hip.ptr(window), _hip.ptr(table), _hip.ptr(feat), feat.numel())
    return feat


def calculate_niqe_device(frame_dev, crop_border: int, params, convert_to: str = "y", channel_order: str = "rgb"):
    """Device twin of calculate_niqe for uint8 / uint16 GPU frames: a float for one frame; for a list or a
    [K][H][W][C] stack, K floats after one synchronisation.  The GPU computes the block features; the 36-element mean,
    the covariance and the 36x36 pinv stay on the host in float64 (niqe_score) after one download of
    K x n_blocks x 36 doubles."""
    _check_niqe_args(crop_border, convert_to, channel_order)
    feats = niqe_features_device(frame_dev, crop_border, params, channel_order).cpu().numpy()   # the one synchronisation
    scores = [niqe_score(f, params) for f in feats]
    many = isinstance(frame_dev, (list, tuple)) or frame_dev.dim() == 4
    return scores if many else scores[0]
