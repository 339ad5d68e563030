"""PSNR and SSIM: the reference's calculate_metrics (src/utils.py:134-156; skimage is restated) and
the super-resolution protocol's Y-channel / cropped pair (basicsr), each on the host in float64
and on the GPU (irm_frame_metrics, irm_frame_metrics_basicsr; irm_frame_metrics_f32 for float32 frames, DESIGN.md
section 20)."""
from __future__ import annotations

import numpy as np
import torch

from . import _hip
from .frames import check_order_and_crop, frame_bits, frame_shape, pair_frames, psnr_from_error


def psnr(target: np.ndarray, pred: np.ndarray, data_range) -> float:
    err = np.mean((np.asarray(target, dtype=np.float64) - np.asarray(pred, dtype=np.float64)) ** 2)
    return psnr_from_error(data_range, err)


def ssim(target: np.ndarray, pred: np.ndarray, data_range, channel_axis=None) -> float:
    """structural_similarity with skimage's defaults (7x7 uniform window, K1=.01,
    K2=.03, sample covariance, border crop).  Restated from the published
    algorithm: parity with skimage is unpinned (skimage is not installed here)."""
    from scipy.ndimage import uniform_filter
    if channel_axis is not None:
        vals = [ssim(np.take(target, i, axis=channel_axis), np.take(pred, i, axis=channel_axis), data_range)
                for i in range(target.shape[channel_axis])]
        return float(np.mean(vals))
    x, y = target.astype(np.float64), pred.astype(np.float64)
    win, npx = 7, 49
    cov_norm = npx / (npx - 1)
    ux, uy = uniform_filter(x, win), uniform_filter(y, win)
    uxx, uyy, uxy = uniform_filter(x * x, win), uniform_filter(y * y, win), uniform_filter(x * y, win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    p = (win - 1) // 2
    return float(s[p:-p, p:-p].mean())


def calculate_metrics(pred: np.ndarray, target: np.ndarray, data_range=None):
    """PSNR and SSIM between prediction and target (src/utils.py:134-156)."""
    if data_range is None:
        data_range = 255 if pred.dtype == np.uint8 else 65535 if pred.dtype == np.uint16 else 1.0
    psnr_value = psnr(target, pred, data_range)
    if pred.ndim == 3 and pred.shape[2] == 3:
        ssim_value = ssim(target, pred, data_range, channel_axis=2)
    elif pred.ndim == 3 and pred.shape[2] == 1:
        ssim_value = ssim(target[:, :, 0], pred[:, :, 0], data_range)
    else:
        ssim_value = ssim(target, pred, data_range)
    return psnr_value, ssim_value


#: output tile of irm_frame_metrics (csrc/metrics.hip; the geometry is SsimTile of csrc/irm_frame.h): 16 rows x 192 values
#: (pixels x channels), one partial each
_METRICS_TILE_ROWS, _METRICS_TILE_VALUES = 16, 192


def _pairs_on_gpu(preds, targets) -> None:
    for p, t in zip(preds, targets):
        if not p.is_cuda or not t.is_cuda:
            raise ValueError("device metrics need GPU tensors; there is no CPU fallback")
        if p.device != preds[0].device or t.device != preds[0].device:
            raise ValueError("the frames of one call must share a device")


def _launch(symbol: str, preds, targets, h, w, c, lost: int, ce: int, sse_dtype, *args) -> tuple:
    """One launch of a frame-metrics entry point over K pairs: (sse [K], ssim [K]) device tensors, not synchronised.
    The SSIM map is `lost` pixels smaller than the frame on each axis and has `ce` channels; each of its output tiles
    leaves two float64 partials in the workspace."""
    k, dev = len(preds), preds[0].device
    tiles = -(-(h - lost) // _METRICS_TILE_ROWS) * -(-(w - lost) // (_METRICS_TILE_VALUES // ce))
    with torch.cuda.device(dev):
        p, t = frame_bits(preds), frame_bits(targets)
        ws = torch.empty(2 * k * tiles, dtype=torch.float64, device=dev)
        sse = torch.empty(k, dtype=sse_dtype, device=dev)
        ssim_dev = torch.empty(k, dtype=torch.float64, device=dev)
        _hip.call(symbol, _hip.ptr(p), _hip.ptr(t), int(preds[0].dtype != torch.uint8), k, h, w, c, *args,
                  _hip.ptr(sse), _hip.ptr(ssim_dev), _hip.ptr(ws), ws.numel())
    return sse, ssim_dev


def frame_metrics_device(preds, targets, data_range=None):
    """Device SSE and SSIM of K prediction / target frames of one shape (irm_frame_metrics): lists of uint8 or uint16
    HW / HWC (C = 1 or 3) GPU tensors, e.g. the tiler's outputs.  Returns device tensors (sse [K] int64, exact;
    ssim [K] float64, the values of `ssim` above: channel mean for C = 3) without synchronising with the host.  Same
    data_range rule as calculate_metrics.  A frame's values are bitwise the same whatever K and on every call."""
    preds, targets = pair_frames(preds, targets, "calculate_metrics")
    h, w, c = frame_shape(preds[0].shape, "frame_metrics_device")
    if min(h, w) < 7:
        raise ValueError(f"frame {h}x{w}: both sides must be at least 7, the SSIM window (skimage refuses it too)")
    _pairs_on_gpu(preds, targets)
    if data_range is None:
        data_range = 255 if preds[0].dtype == torch.uint8 else 65535
    if not (np.isfinite(data_range) and data_range > 0):
        raise ValueError(f"data_range must be positive and finite, not {data_range}")
    return _launch("irm_frame_metrics", preds, targets, h, w, c, 6, c, torch.int64, float(data_range))


def calculate_metrics_device(pred_dev: torch.Tensor, target_dev: torch.Tensor, data_range=None):
    """Device twin of calculate_metrics for uint8 / uint16 GPU frames (HWC with 3 channels: channel-mean SSIM; HW1 and
    HW: grey): (psnr, ssim) as Python floats after one synchronising copy.  PSNR is inf for identical frames."""
    sse, ssim_dev = frame_metrics_device([pred_dev], [target_dev], data_range)
    h, w, c = frame_shape(pred_dev.shape)
    if data_range is None:
        data_range = 255 if pred_dev.dtype == torch.uint8 else 65535
    host = torch.stack([sse, ssim_dev.view(torch.int64)]).cpu()       # the one host synchronisation
    sse_v, ssim_v = int(host[0, 0]), float(host[1].view(torch.float64)[0])
    return psnr_from_error(data_range, sse_v / (h * w * c)), ssim_v


def frame_metrics_f32_device(preds, targets, data_range=1.0):
    """Device squared error and SSIM of K float32 prediction / target frames of one shape (irm_frame_metrics_f32): lists
    of float32 HW / HW1 / HW3 GPU tensors, e.g. the pipeline's out="float32" frames.  Returns device tensors
    (sse [K] float64, the fp64 sum of the squared differences; ssim [K] float64, the values of `ssim` above) without
    synchronising with the host.  A non-contiguous tensor is made contiguous.  A frame's values are bitwise the same
    whatever K and on every call.  Non-finite values are outside the contract."""
    preds, targets = list(preds), list(targets)
    if not preds or len(preds) != len(targets):
        raise ValueError(f"{len(preds)} predictions and {len(targets)} targets: need the same number, at least one")
    for p, t in zip(preds, targets):
        if not isinstance(p, torch.Tensor) or not isinstance(t, torch.Tensor):
            raise ValueError("device metrics take torch tensors (use calculate_metrics for numpy arrays)")
        if p.shape != t.shape or p.dtype != t.dtype:
            raise ValueError(f"prediction {tuple(p.shape)} {p.dtype} and target {tuple(t.shape)} {t.dtype} differ in "
                             "shape or dtype")
        if p.dtype != torch.float32:
            raise ValueError(f"frame_metrics_f32_device takes float32 frames, not {p.dtype} (frame_metrics_device "
                             "takes uint8 and uint16)")
        if p.shape != preds[0].shape:
            raise ValueError("the frames of one call must share shape and dtype")
    h, w, c = frame_shape(preds[0].shape, "frame_metrics_f32_device")
    if min(h, w) < 7:
        raise ValueError(f"frame {h}x{w}: both sides must be at least 7, the SSIM window (skimage refuses it too)")
    _pairs_on_gpu(preds, targets)
    if not (np.isfinite(data_range) and data_range > 0):
        raise ValueError(f"data_range must be positive and finite, not {data_range}")
    k, dev = len(preds), preds[0].device
    tiles = -(-(h - 6) // _METRICS_TILE_ROWS) * -(-(w - 6) // (_METRICS_TILE_VALUES // c))
    with torch.cuda.device(dev):
        p, t = frame_bits(preds), frame_bits(targets)
        ws = torch.empty(2 * k * tiles, dtype=torch.float64, device=dev)
        sse = torch.empty(k, dtype=torch.float64, device=dev)
        ssim_dev = torch.empty(k, dtype=torch.float64, device=dev)
        _hip.call("irm_frame_metrics_f32", _hip.ptr(p), _hip.ptr(t), k, h, w, c, float(data_range), _hip.ptr(sse),
                  _hip.ptr(ssim_dev), _hip.ptr(ws), ws.numel())
    return sse, ssim_dev


def calculate_metrics_f32_device(pred_dev: torch.Tensor, target_dev: torch.Tensor, data_range=None):
    """Device twin of calculate_metrics for float32 GPU frames (HW3: channel-mean SSIM; HW1 and HW: grey): (psnr, ssim)
    as Python floats after one synchronising copy.  data_range=None means 1.0, the reference's rule for a non-integer
    dtype (src/utils.py:137-143).  PSNR is inf for identical frames."""
    if data_range is None:
        data_range = 1.0
    sse, ssim_dev = frame_metrics_f32_device([pred_dev], [target_dev], data_range)
    h, w, c = frame_shape(pred_dev.shape)
    host = torch.stack([sse, ssim_dev]).cpu()                         # the one host synchronisation
    return psnr_from_error(data_range, float(host[0, 0]) / (h * w * c)), float(host[1, 0])


_Y_COEF = {"rgb": (65.481, 128.553, 24.966), "bgr": (24.966, 128.553, 65.481)}


def _gauss11() -> np.ndarray:
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def _basicsr_values(img: np.ndarray, crop_border: int, test_y_channel: bool, channel_order: str) -> np.ndarray:
    """The HxWxCe float64 values the reference's metrics see (psnr_ssim.py:32-41, metric_util.to_y_channel)."""
    peak = np.float32(255.0 if img.dtype == np.uint8 else 65535.0)
    if img.ndim == 2:
        img = img[..., None]
    if crop_border:
        img = img[crop_border:-crop_border, crop_border:-crop_border]
    if not test_y_channel:
        return img.astype(np.float64)
    v = img.astype(np.float32) / peak                                         # fp32
    if img.shape[2] == 3:
        k = _Y_COEF[channel_order]
        v64 = v.astype(np.float64)
        y = ((v64[..., 0] * k[0] + v64[..., 1] * k[1]) + v64[..., 2] * k[2]) + 16.0      # fp64
        v = (y / 255.0).astype(np.float32)[..., None]
    return (v * peak).astype(np.float64)                                      # the product is fp32


def _check_basicsr_args(shape, crop_border, channel_order):
    check_order_and_crop(channel_order, crop_border)
    h, w, c = frame_shape(shape, "the basicsr metrics")
    if min(h, w) - 2 * crop_border < 11:
        raise ValueError(f"frame {h}x{w} cropped by {crop_border}: both sides must keep at least 11 pixels, the SSIM window")
    return h, w, c


def calculate_metrics_basicsr(pred: np.ndarray, target: np.ndarray, crop_border: int, test_y_channel: bool,
                              channel_order: str = "rgb"):
    """(psnr, ssim) of the super-resolution protocol for uint8 / uint16 HW or HWC frames: basicsr's calculate_psnr /
    calculate_ssim restated (crop, optional BT.601 Y channel with the reference's fp32 / fp64 steps, 11x11 Gaussian
    window of sigma 1.5 applied separably over the valid region, channel mean).  The Y-channel squared error is
    summed in float64 (the reference takes that mean in fp32)."""
    if not isinstance(pred, np.ndarray) or not isinstance(target, np.ndarray):
        raise ValueError("calculate_metrics_basicsr takes numpy arrays (calculate_metrics_basicsr_device takes GPU tensors)")
    if pred.shape != target.shape or pred.dtype != target.dtype:
        raise ValueError(f"prediction {pred.shape} {pred.dtype} and target {target.shape} {target.dtype} differ")
    if pred.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"the basicsr metrics take uint8 or uint16 frames, not {pred.dtype}")
    _check_basicsr_args(pred.shape, crop_border, channel_order)
    peak = 255.0 if pred.dtype == np.uint8 else 65535.0
    x = _basicsr_values(pred, int(crop_border), bool(test_y_channel), channel_order)
    y = _basicsr_values(target, int(crop_border), bool(test_y_channel), channel_order)
    psnr_value = psnr_from_error(peak, np.mean((x - y) ** 2))
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    g = _gauss11()

    def blur(a):                                                              # valid region, rows then columns
        n0, n1 = a.shape[0] - 10, a.shape[1] - 10
        v = sum(g[d] * a[d:d + n0] for d in range(11))
        return sum(g[d] * v[:, d:d + n1] for d in range(11))
    vals = []
    for ch in range(x.shape[2]):
        a, b = x[..., ch], y[..., ch]
        m1, m2 = blur(a), blur(b)
        v1, v2, v12 = blur(a * a) - m1 * m1, blur(b * b) - m2 * m2, blur(a * b) - m1 * m2
        vals.append((((2 * (m1 * m2) + c1) * (2 * v12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (v1 + v2 + c2))).mean())
    return psnr_value, float(np.mean(vals))


def frame_metrics_basicsr_device(preds, targets, crop_border: int, test_y_channel: bool, channel_order: str = "rgb"):
    """Device squared-error sums and SSIMs of K prediction / target frames of one shape (irm_frame_metrics_basicsr):
    returns (sse [K] - int64, exact, with test_y_channel off; float64 with it on - and ssim [K] float64) as device
    tensors, without synchronising.  A frame's values are bitwise the same whatever K and on every call."""
    preds, targets = pair_frames(preds, targets, "calculate_metrics_basicsr")
    h, w, c = _check_basicsr_args(preds[0].shape, crop_border, channel_order)
    _pairs_on_gpu(preds, targets)
    crop_border, test_y = int(crop_border), bool(test_y_channel)
    return _launch("irm_frame_metrics_basicsr", preds, targets, h, w, c, 2 * crop_border + 10, 1 if test_y else c,
                   torch.float64 if test_y else torch.int64, crop_border, int(test_y), int(channel_order == "bgr"))


def calculate_metrics_basicsr_device(pred_dev: torch.Tensor, target_dev: torch.Tensor, crop_border: int,
                                     test_y_channel: bool, channel_order: str = "rgb"):
    """Device twin of calculate_metrics_basicsr: (psnr, ssim) as Python floats after one synchronising copy."""
    sse, ssim_dev = frame_metrics_basicsr_device([pred_dev], [target_dev], crop_border, test_y_channel, channel_order)
    h, w, c = frame_shape(pred_dev.shape)
    host = torch.stack([sse.view(torch.int64), ssim_dev.view(torch.int64)]).cpu()     # the one host synchronisation
    sse_v = float(host[0].view(torch.float64)[0]) if test_y_channel else int(host[0, 0])
    ssim_v = float(host[1].view(torch.float64)[0])
    peak = 255.0 if pred_dev.dtype == torch.uint8 else 65535.0
    n = (h - 2 * int(crop_border)) * (w - 2 * int(crop_border)) * (1 if test_y_channel else c)
    return psnr_from_error(peak, sse_v / n), ssim_v
