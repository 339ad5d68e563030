"""Glue API with the reference's call surface (src/utils.py): model factory,
patch-config lookup, the tiled-patch inference loop and the metrics.

The hot loop (reference: src/utils.py:353-454, one synchronous forward + D2H +
numpy blend per tile) runs here as ONE device pipeline per image:
``irm_tile_extract`` (normalise / seeded noise / reflect pad) -> batched model
forward over all tiles -> ``irm_window_blend`` (Gaussian blend, /weight,
requantise) -> one D2H of the uint8 result.  Results equal the reference loop's
given equal per-tile predictions (same float32 operation order).
"""
from __future__ import annotations

import os
import time
from typing import Callable, Literal

import numpy as np
import torch
from torch.nn import Module

from . import _hip, deblurganv2, dncnn, mair, ops, rednet, restormer
from .convnet_common import check_precision
from .configs import PATCH_CONFIG, ROOT_RESULTS_DIR, ROOT_WEIGHTS_DIR
from .dncnn import DnCNN
from .rednet import REDNet
from .restormer import Restormer
from .mair import MaIR, MaIRPlus, MaIRUNet
from .deblurganv2 import FPNMobileNet

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))

#: model classes whose forward is the HIP path (isinstance dispatch as in utils.py:280/292)
_PAD8_MODELS = (Restormer, MaIR, MaIRUNet, MaIRPlus)


def get_model_total_parameters(model: Module) -> int:
    return sum(p.numel() for p in model.parameters())


def add_gaussian_noise(img: np.ndarray, sigma: int | float = 15):
    """src/utils.py:29-36 (seed 0 on every call, float64 noise added into a float32 array)."""
    if img.dtype != np.float32 and img.dtype != np.float64:
        img = img.astype(np.float32) / 255.
    np.random.seed(seed=0)
    img += np.random.normal(0, sigma / 255., img.shape)
    return np.clip(img, 0, 1).astype(np.float32)


def normalize(img: np.ndarray):
    """src/utils.py:159-171."""
    if img.dtype == np.uint16:
        out = img.astype(np.float32) / 65535.0
    elif img.dtype == np.uint8:
        out = img.astype(np.float32) / 255.0
    else:
        peak = np.max(img)
        out = img.astype(np.float32) / peak if peak > 1.0 else img.astype(np.float32)
    return out.astype(np.float32)


def pad(x: torch.Tensor, downscale_factor: int = 8):
    """src/utils.py:174-181: reflect-pad right/bottom to the next multiple of the factor."""
    h, w = x.shape[-2:]
    padh = (h // downscale_factor + 1) * downscale_factor - h if h % downscale_factor else 0
    padw = (w // downscale_factor + 1) * downscale_factor - w if w % downscale_factor else 0
    return torch.nn.functional.pad(x, (0, padw, 0, padh), 'reflect')


def get_gaussian_weights(height: int, width: int, n_channels=3, sigma_scale=0.125):
    """src/utils.py:314-350: Gaussian blending window, float64 maths, centre at size/2."""
    yy = (np.arange(height) - height / 2.0) ** 2 / (2 * (height * sigma_scale) ** 2)
    xx = (np.arange(width) - width / 2.0) ** 2 / (2 * (width * sigma_scale) ** 2)
    g = np.exp(-(yy[:, None] + xx[None, :]))
    return np.repeat(g[:, :, np.newaxis], n_channels, axis=2).astype(np.float32)


def get_patch_config(task, subtask, model_name) -> dict | None:
    """src/utils.py:184-213."""
    model_key = model_name.split(' ')[0]
    if model_key == 'MaIR+':                      # the same network under the x8 self-ensemble: the same tiles
        model_key = 'MaIR'
    config = PATCH_CONFIG.get(model_key, None)
    if isinstance(config, list):
        if model_key == 'DeblurGANv2':
            config = config[0] if 'Inception' in model_name else config[1]
        elif model_key == 'MaIR':
            config = config[0] if subtask.lower() == 'gaussian' else config[1]
        elif model_key == 'Restormer':
            config = config[0] if task.lower() == 'denoising' else config[1]
        else:
            config = config[0]
    return config


def _restormer_opt(name: str) -> str:
    return os.path.join(_PKG_DIR, 'restormer', 'options', name + '.yml')


#: the model families that have the reduced-precision mode (get_model_instance(..., precision="fp16"))
HALF_PRECISION_FAMILIES = ('DnCNN', 'REDNet')


def get_model_instance(task, subtask, model_name, device: torch.device, gray=False,
                       sigma: int | float | None = None, precision: str = "fp32") -> torch.nn.Module:
    """src/utils.py:216-267: same (task, subtask, model, gray, sigma) -> weights table.  precision="fp16" (DnCNN and
    REDNet only, not reference-parity) selects their native-fp16 kernels."""
    model_key = model_name.split(' ')[0]
    check_precision(precision, "get_model_instance")
    if precision == "fp16" and model_key not in HALF_PRECISION_FAMILIES:
        raise ValueError(f"precision='fp16' is available for {' and '.join(HALF_PRECISION_FAMILIES)} only, "
                         f"not for {model_key}")
    if model_key == 'REDNet':
        if task == 'denoising' and subtask == 'gaussian' and sigma is not None:
            return rednet.get_model(f'{ROOT_WEIGHTS_DIR}/REDNet/{sigma}.pt', device, precision=precision)
    elif model_key == 'DnCNN':
        if task == 'denoising' and subtask == 'gaussian':
            if gray:
                if sigma is not None:
                    return dncnn.get_model(f'{ROOT_WEIGHTS_DIR}/DnCNN/dncnn_{sigma}.pth', 1, 17, device,
                                           precision=precision)
                return dncnn.get_model(f'{ROOT_WEIGHTS_DIR}/DnCNN/dncnn_gray_blind.pth', 1, 20, device,
                                       precision=precision)
            if sigma is None:
                return dncnn.get_model(f'{ROOT_WEIGHTS_DIR}/DnCNN/dncnn_color_blind.pth', 3, 20, device,
                                       precision=precision)
    elif model_key == 'Restormer':
        kind = 'Gray' if gray else 'Color'
        if task == 'denoising':
            if subtask == 'gaussian':
                suffix = f'Sigma{sigma}' if sigma is not None else ''
                return restormer.get_model(_restormer_opt(f'Gaussian{kind}Denoising_Restormer{suffix}'), device)
            if subtask == 'real':
                return restormer.get_model(_restormer_opt('RealDenoising_Restormer'), device)
        if task == 'deblurring':
            if subtask == 'defocus':
                if 'Dual-pixel' in model_name:
                    return restormer.get_model(_restormer_opt('DefocusDeblur_DualPixel_16bit_Restormer'), device)
                return restormer.get_model(_restormer_opt('DefocusDeblur_Single_8bit_Restormer'), device)
            if subtask == 'motion':
                return restormer.get_model(_restormer_opt('Deblurring_Restormer'), device)
    elif model_key in ('MaIR', 'MaIR+'):
        opt_dir = os.path.join(_PKG_DIR, 'mair', 'options')
        plus = model_key == 'MaIR+'               # the same option files (model_type: MaIRPlusModel), wrapped
        if task == 'denoising':
            if subtask == 'gaussian' and not gray and sigma is not None:
                return mair.get_model(os.path.join(opt_dir, f'test_MaIR_CDN_s{sigma}.yml'), plus=plus)
            if subtask == 'real':
                return mair.get_model(os.path.join(opt_dir, 'test_MaIR_RealDN.yml'), plus=plus)
        if task == 'deblurring' and subtask == 'motion':
            return mair.get_model(os.path.join(opt_dir, 'test_MaIR_MotionDeblur.yml'), plus=plus)
    elif model_key == 'DeblurGANv2':
        if task == 'deblurring' and subtask == 'motion':
            if 'Inception' in model_name:
                return deblurganv2.get_model(f'{ROOT_WEIGHTS_DIR}/DeblurGANv2/fpn_inception.h5', device)
            if 'MobileNet' in model_name:
                return deblurganv2.get_model(f'{ROOT_WEIGHTS_DIR}/DeblurGANv2/fpn_mobilenet.h5', device)
    raise ValueError('No model instance found for current configuration.')


# ---------------------------------------------------------------------------
# metrics (src/utils.py:134-156; skimage is restated)
# ---------------------------------------------------------------------------

def psnr(target: np.ndarray, pred: np.ndarray, data_range) -> float:
    err = np.mean((np.asarray(target, dtype=np.float64) - np.asarray(pred, dtype=np.float64)) ** 2)
    return float('inf') if err == 0 else float(10 * np.log10((data_range ** 2) / err))


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


#: output tile of irm_frame_metrics (csrc/metrics.hip): 16 rows x 192 values (pixels x channels), one partial each
_METRICS_TILE_ROWS, _METRICS_TILE_VALUES = 16, 192
#: int16 is read as the uint16 bit pattern, as the tiler does (its uint16 frames travel as int16 tensors)
_METRICS_DTYPES = (torch.uint8, torch.uint16, torch.int16)


def _metrics_frame_shape(pred, target) -> tuple:
    """(H, W, C) of a prediction / target pair for the device metrics; ValueError before any GPU call otherwise."""
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise ValueError("device metrics take torch tensors (use calculate_metrics for numpy arrays)")
    if tuple(pred.shape) != tuple(target.shape) or pred.dtype != target.dtype:
        raise ValueError(f"prediction {tuple(pred.shape)} {pred.dtype} and target {tuple(target.shape)} "
                         f"{target.dtype} differ in shape or dtype")
    if pred.dtype not in _METRICS_DTYPES:
        raise ValueError(f"device metrics take uint8 or uint16 frames, not {pred.dtype}")
    if pred.dim() == 2:
        (h, w), c = pred.shape, 1
    elif pred.dim() == 3:
        h, w, c = pred.shape
    else:
        raise ValueError(f"device metrics take HW or HWC frames, not shape {tuple(pred.shape)}")
    if c not in (1, 3):
        raise ValueError(f"device metrics take 1 or 3 channels, not {c}")
    if min(h, w) < 7:
        raise ValueError(f"frame {h}x{w}: both sides must be at least 7, the SSIM window (skimage refuses it too)")
    if not pred.is_cuda or not target.is_cuda:
        raise ValueError("device metrics need GPU tensors; there is no CPU fallback (calculate_metrics takes host arrays)")
    if pred.device != target.device:
        raise ValueError(f"prediction on {pred.device}, target on {target.device}")
    return h, w, c


def frame_metrics_device(preds, targets, data_range=None):
    """Device SSE and SSIM of K prediction / target frames of one shape (irm_frame_metrics): lists of uint8 or uint16
    HW / HWC (C = 1 or 3) GPU tensors, e.g. the tiler's outputs.  Returns device tensors (sse [K] int64, exact;
    ssim [K] float64, the values of `ssim` above: channel mean for C = 3) without synchronising with the host.  Same
    data_range rule as calculate_metrics.  A frame's values are bitwise the same whatever K and on every call."""
    preds, targets = list(preds), list(targets)
    if not preds or len(preds) != len(targets):
        raise ValueError(f"{len(preds)} predictions and {len(targets)} targets: need the same number, at least one")
    h, w, c = _metrics_frame_shape(preds[0], targets[0])
    for p, t in zip(preds, targets):
        if (_metrics_frame_shape(p, t) != (h, w, c) or p.shape != preds[0].shape or p.dtype != preds[0].dtype
                or p.device != preds[0].device):
            raise ValueError("the frames of one call must share shape, dtype and device")
    is_u16 = preds[0].dtype != torch.uint8
    if data_range is None:
        data_range = 65535 if is_u16 else 255
    if not (np.isfinite(data_range) and data_range > 0):
        raise ValueError(f"data_range must be positive and finite, not {data_range}")
    # uint16 as its int16 bit pattern: the copies below need no uint16 kernels
    as_bits = (lambda x: x.view(torch.int16)) if preds[0].dtype == torch.uint16 else (lambda x: x)
    k, dev = len(preds), preds[0].device
    with torch.cuda.device(dev):
        if k == 1:
            p, t = as_bits(preds[0]).contiguous(), as_bits(targets[0]).contiguous()
        else:
            p, t = torch.stack([as_bits(x) for x in preds]), torch.stack([as_bits(x) for x in targets])
        tiles = -(-(h - 6) // _METRICS_TILE_ROWS) * -(-(w - 6) // (_METRICS_TILE_VALUES // c))
        ws = torch.empty(2 * k * tiles, dtype=torch.float64, device=dev)
        sse = torch.empty(k, dtype=torch.int64, device=dev)
        ssim_dev = torch.empty(k, dtype=torch.float64, device=dev)
        _hip.call("irm_frame_metrics", _hip.ptr(p), _hip.ptr(t), int(is_u16), k, h, w, c, float(data_range),
                  _hip.ptr(sse), _hip.ptr(ssim_dev), _hip.ptr(ws), ws.numel())
    return sse, ssim_dev


def calculate_metrics_device(pred_dev: torch.Tensor, target_dev: torch.Tensor, data_range=None):
    """Device twin of calculate_metrics for uint8 / uint16 GPU frames (HWC with 3 channels: channel-mean SSIM; HW1 and
    HW: grey): (psnr, ssim) as Python floats after one synchronising copy.  PSNR is inf for identical frames."""
    h, w, c = _metrics_frame_shape(pred_dev, target_dev)
    if data_range is None:
        data_range = 255 if pred_dev.dtype == torch.uint8 else 65535
    sse, ssim_dev = frame_metrics_device([pred_dev], [target_dev], data_range)
    host = torch.stack([sse, ssim_dev.view(torch.int64)]).cpu()       # the one host synchronisation
    sse_v, ssim_v = int(host[0, 0]), float(host[1].view(torch.float64)[0])
    err = sse_v / (h * w * c)
    return (float('inf') if sse_v == 0 else float(10 * np.log10((data_range ** 2) / err))), ssim_v


# ---------------------------------------------------------------------------
# super-resolution protocol: MATLAB bicubic resize, Y-channel / cropped metrics (basicsr)
# ---------------------------------------------------------------------------

_RESIZE_SCALES = (2, 3, 4)


def mod_crop(img, scale: int):
    """Drop the bottom rows / right columns beyond a multiple of `scale` (HW or HWC array or tensor; a view)."""
    scale = int(scale)
    if scale < 1:
        raise ValueError(f"mod_crop: scale must be a positive integer, not {scale}")
    if len(img.shape) not in (2, 3):
        raise ValueError(f"mod_crop takes HW or HWC frames, not shape {tuple(img.shape)}")
    h, w = img.shape[:2]
    return img[:h - h % scale, :w - w % scale]


def _resize_factor(scale) -> tuple:
    """scale -> (s, shrink) for s or 1 / s with s in {2, 3, 4}; ValueError otherwise."""
    for s in _RESIZE_SCALES:
        if scale == s:
            return s, False
        if isinstance(scale, float) and abs(scale * s - 1.0) < 1e-12:
            return s, True
    raise ValueError(f"resize factor must be s or 1/s with s in {_RESIZE_SCALES}, not {scale!r}")


def _cubic(x: np.ndarray) -> np.ndarray:
    a = np.abs(x)
    return np.where(a <= 1, (1.5 * a - 2.5) * a * a + 1, np.where(a <= 2, ((-0.5 * a + 2.5) * a - 4) * a + 2, 0.0))


def resize_table(in_length: int, scale) -> tuple:
    """Taps of MATLAB's bicubic imresize along one axis, in float64: (weights [out][P], indices [out][P] int64,
    0-based and reflected into [0, in_length)), out = ceil(in_length * scale).  u = x / scale + 0.5 (1 - 1 / scale) for
    the 1-based output coordinate x; kernel width 4, or 4 / scale when shrinking (antialiasing); P = ceil(width) + 2 taps
    from floor(u - width / 2); the cubic kernel at scale * distance times scale when shrinking; rows normalised to sum 1.
    Zero-weight edge taps stay in the table."""
    s, shrink = _resize_factor(scale)
    scale = 1.0 / s if shrink else float(s)
    width = 4 * s if shrink else 4
    p = width + 2
    if in_length < p:
        raise ValueError(f"resize by {scale:g}: a side of {in_length} is shorter than the {p} taps")
    out_length = -(-in_length // s) if shrink else in_length * s
    x = np.arange(1, out_length + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - width / 2)
    idx = left[:, None] + np.arange(p, dtype=np.float64)[None, :]           # 1-based
    dist = u[:, None] - idx
    w = scale * _cubic(dist * scale) if shrink else _cubic(dist)
    w = w / w.sum(1, keepdims=True)
    i0 = idx.astype(np.int64) - 1
    i0 = np.where(i0 < 0, -i0 - 1, np.where(i0 >= in_length, 2 * in_length - 1 - i0, i0))
    assert i0.min() >= 0 and i0.max() < in_length
    return w, i0


def _check_resize_frame(shape, what="imresize") -> tuple:
    if len(shape) == 2:
        return shape[0], shape[1], 1
    if len(shape) == 3 and shape[2] in (1, 3):
        return tuple(shape)
    raise ValueError(f"{what} takes HW or HWC frames with 1 or 3 channels, not shape {tuple(shape)}")


def imresize_host(img: np.ndarray, scale, out: str = "float") -> np.ndarray:
    """MATLAB bicubic imresize (antialiased when shrinking) of a uint8 / uint16 HW or HWC frame, restated in float64:
    the frame / 255 (65535), the H pass, then the W pass.  out="float": float64 in [0, 1] nominal, unrounded;
    out="same": clipped to [0, 1], x 255 (65535), rounded half to even, in the frame's dtype (tensor2img)."""
    if out not in ("float", "same"):
        raise ValueError(f"out must be 'float' or 'same', not {out!r}")
    if not isinstance(img, np.ndarray) or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("imresize_host takes uint8 or uint16 numpy frames")
    h, w, _ = _check_resize_frame(img.shape, "imresize_host")
    wh, ih = resize_table(h, scale)
    ww, iw = resize_table(w, scale)
    peak = 255.0 if img.dtype == np.uint8 else 65535.0
    x = img.astype(np.float64) / peak
    mid = np.zeros((wh.shape[0],) + x.shape[1:], np.float64)
    for p in range(wh.shape[1]):                                              # ascending tap order
        mid += wh[:, p].reshape((-1,) + (1,) * (x.ndim - 1)) * x[ih[:, p]]
    res = np.zeros((mid.shape[0], ww.shape[0]) + mid.shape[2:], np.float64)
    for p in range(ww.shape[1]):
        res += ww[:, p].reshape((1, -1) + (1,) * (x.ndim - 2)) * mid[:, iw[:, p]]
    if out == "float":
        return res
    return np.round(np.clip(res, 0.0, 1.0) * peak).astype(img.dtype)


_RESIZE_TABLES: dict = {}


def _resize_table_on(device, in_length: int, s: int, shrink: bool) -> tuple:
    """The axis table on the device (fp32 weights, int32 indices), cached per (device, length, factor) like
    mairunet_arch.scan_ids: a repeated or captured call enqueues kernels only."""
    key = (str(device), in_length, s, shrink)
    if key not in _RESIZE_TABLES:
        w, i = resize_table(in_length, 1.0 / s if shrink else s)
        _RESIZE_TABLES[key] = (torch.from_numpy(w.astype(np.float32)).contiguous().to(device),
                               torch.from_numpy(i.astype(np.int32)).contiguous().to(device))
    return _RESIZE_TABLES[key]


def imresize_device(frames, scale, out: str = "same"):
    """MATLAB bicubic imresize on the GPU (irm_imresize_bicubic): `frames` is one uint8 / uint16 (or int16 = uint16 bit
    pattern) HW / HWC GPU tensor, a [K][H][W][C] stack, or a list of frames of one shape; scale is s or 1/s, s in
    {2, 3, 4}.  out="same": quantised to the input's dtype (how LR files are made); out="float": float32 in [0, 1]
    nominal, unrounded.  Returns the same arrangement (tensor -> tensor, list -> list) without synchronising."""
    if out not in ("float", "same"):
        raise ValueError(f"out must be 'float' or 'same', not {out!r}")
    s, shrink = _resize_factor(scale)
    as_list = isinstance(frames, (list, tuple))
    items = list(frames) if as_list else [frames]
    if not items:
        raise ValueError("imresize_device: no frames")
    for f in items:
        if not isinstance(f, torch.Tensor):
            raise ValueError("imresize_device takes torch tensors (imresize_host takes numpy arrays)")
        if f.dtype not in _METRICS_DTYPES:
            raise ValueError(f"imresize_device takes uint8 or uint16 frames, not {f.dtype}")
        if f.shape != items[0].shape or f.dtype != items[0].dtype or f.device != items[0].device:
            raise ValueError("the frames of one call must share shape, dtype and device")
        if not f.is_cuda:
            raise ValueError("imresize_device needs GPU tensors; there is no CPU fallback (imresize_host takes host arrays)")
    f0 = items[0]
    stacked = not as_list and f0.dim() == 4
    if stacked:
        k, (h, w, c) = f0.shape[0], _check_resize_frame(f0.shape[1:], "imresize_device")
        if k < 1:
            raise ValueError("imresize_device: empty stack")
    else:
        k, (h, w, c) = len(items), _check_resize_frame(f0.shape, "imresize_device")
    p = 4 * s + 2 if shrink else 6
    if min(h, w) < p:
        raise ValueError(f"resize by {scale:g}: a {h}x{w} frame has a side shorter than the {p} taps")
    oh, ow = (-(-h // s), -(-w // s)) if shrink else (h * s, w * s)
    as_bits = (lambda x: x.view(torch.int16)) if f0.dtype == torch.uint16 else (lambda x: x)
    dev = f0.device
    with torch.cuda.device(dev):
        src = as_bits(f0).contiguous() if (stacked or k == 1) else torch.stack([as_bits(x) for x in items])
        wh, ih = _resize_table_on(dev, h, s, shrink)
        ww, iw = _resize_table_on(dev, w, s, shrink)
        res = torch.empty((k, oh, ow, c), dtype=torch.float32 if out == "float" else src.dtype, device=dev)
        _hip.call("irm_imresize_bicubic", _hip.ptr(src), int(f0.dtype != torch.uint8), _hip.ptr(res), int(out == "float"),
                  _hip.ptr(wh), _hip.ptr(ih), _hip.ptr(ww), _hip.ptr(iw), k, h, w, c, s, int(shrink))
    if out == "same" and f0.dtype == torch.uint16:
        res = res.view(torch.uint16)
    tail = (oh, ow) if (f0.dim() - int(stacked)) == 2 else (oh, ow, c)
    if stacked:
        return res.view((k,) + tail)
    return [r.view(tail) for r in res] if as_list else res[0].view(tail)


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
    if channel_order not in _Y_COEF:
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', not {channel_order!r}")
    if int(crop_border) != crop_border or crop_border < 0:
        raise ValueError(f"crop_border must be a non-negative integer, not {crop_border!r}")
    h, w, c = _check_resize_frame(shape, "the basicsr metrics")
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
    mse = np.mean((x - y) ** 2)
    psnr_value = float('inf') if mse == 0 else float(10 * np.log10(peak ** 2 / mse))
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
    preds, targets = list(preds), list(targets)
    if not preds or len(preds) != len(targets):
        raise ValueError(f"{len(preds)} predictions and {len(targets)} targets: need the same number, at least one")
    for p_, t_ in zip(preds, targets):
        if not isinstance(p_, torch.Tensor) or not isinstance(t_, torch.Tensor):
            raise ValueError("device metrics take torch tensors (use calculate_metrics_basicsr for numpy arrays)")
        if p_.shape != t_.shape or p_.dtype != t_.dtype or p_.shape != preds[0].shape or p_.dtype != preds[0].dtype:
            raise ValueError("the frames of one call must share shape and dtype")
        if p_.dtype not in _METRICS_DTYPES:
            raise ValueError(f"device metrics take uint8 or uint16 frames, not {p_.dtype}")
    h, w, c = _check_basicsr_args(preds[0].shape, crop_border, channel_order)
    for p_, t_ in zip(preds, targets):
        if not p_.is_cuda or not t_.is_cuda:
            raise ValueError("device metrics need GPU tensors; there is no CPU fallback")
        if p_.device != preds[0].device or t_.device != preds[0].device:
            raise ValueError("the frames of one call must share a device")
    crop_border, test_y = int(crop_border), bool(test_y_channel)
    as_bits = (lambda x: x.view(torch.int16)) if preds[0].dtype == torch.uint16 else (lambda x: x)
    k, dev = len(preds), preds[0].device
    ce = 1 if test_y else c
    with torch.cuda.device(dev):
        if k == 1:
            p, t = as_bits(preds[0]).contiguous(), as_bits(targets[0]).contiguous()
        else:
            p, t = torch.stack([as_bits(x) for x in preds]), torch.stack([as_bits(x) for x in targets])
        tiles = (-(-(h - 2 * crop_border - 10) // _METRICS_TILE_ROWS)
                 * -(-(w - 2 * crop_border - 10) // (_METRICS_TILE_VALUES // ce)))
        ws = torch.empty(2 * k * tiles, dtype=torch.float64, device=dev)
        sse = torch.empty(k, dtype=torch.float64 if test_y else torch.int64, device=dev)
        ssim_dev = torch.empty(k, dtype=torch.float64, device=dev)
        _hip.call("irm_frame_metrics_basicsr", _hip.ptr(p), _hip.ptr(t), int(preds[0].dtype != torch.uint8), k, h, w, c,
                  crop_border, int(test_y), int(channel_order == "bgr"), _hip.ptr(sse), _hip.ptr(ssim_dev), _hip.ptr(ws),
                  ws.numel())
    return sse, ssim_dev


def calculate_metrics_basicsr_device(pred_dev: torch.Tensor, target_dev: torch.Tensor, crop_border: int,
                                     test_y_channel: bool, channel_order: str = "rgb"):
    """Device twin of calculate_metrics_basicsr: (psnr, ssim) as Python floats after one synchronising copy."""
    sse, ssim_dev = frame_metrics_basicsr_device([pred_dev], [target_dev], crop_border, test_y_channel, channel_order)
    h, w, c = _check_resize_frame(pred_dev.shape)
    host = torch.stack([sse.view(torch.int64), ssim_dev.view(torch.int64)]).cpu()     # the one host synchronisation
    sse_v = float(host[0].view(torch.float64)[0]) if test_y_channel else int(host[0, 0])
    ssim_v = float(host[1].view(torch.float64)[0])
    peak = 255.0 if pred_dev.dtype == torch.uint8 else 65535.0
    n = (h - 2 * int(crop_border)) * (w - 2 * int(crop_border)) * (1 if test_y_channel else c)
    return (float('inf') if sse_v == 0 else float(10 * np.log10(peak ** 2 / (sse_v / n)))), ssim_v


# ---------------------------------------------------------------------------
# no-reference quality: NIQE (basicsr/metrics/niqe.py)
# ---------------------------------------------------------------------------

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
    if channel_order not in _Y_COEF:
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', not {channel_order!r}")
    if int(crop_border) != crop_border or crop_border < 0:
        raise ValueError(f"crop_border must be a non-negative integer, not {crop_border!r}")
    return int(crop_border)


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


_NIQE_TABLES: dict = {}


def _niqe_tables_on(device, window: np.ndarray) -> tuple:
    """(window, table) on the device: the 49 weights flipped for the kernel's correlation (scipy's convolve flips
    them) and [r_gam, gam] as one [2][9801] float64 tensor, built once on the host in float64 and cached per device
    like `_resize_table_on`."""
    key = (str(device), window.tobytes())
    if key not in _NIQE_TABLES:
        gam, r_gam = niqe_gamma_table()
        _NIQE_TABLES[key] = (torch.from_numpy(np.ascontiguousarray(window[::-1, ::-1])).to(device),
                             torch.from_numpy(np.stack([r_gam, gam])).contiguous().to(device))
    return _NIQE_TABLES[key]


def _niqe_frames(frames) -> tuple:
    """frames -> (list of frame tensors or one stack, K, H, W, C, stacked); the checks that need no GPU."""
    as_list = isinstance(frames, (list, tuple))
    items = list(frames) if as_list else [frames]
    if not items:
        raise ValueError("NIQE: no frames")
    for f in items:
        if not isinstance(f, torch.Tensor):
            raise ValueError("the device NIQE takes torch tensors (calculate_niqe takes numpy arrays)")
        if f.dtype not in _METRICS_DTYPES:
            raise ValueError(f"the device NIQE takes uint8 or uint16 frames, not {f.dtype}")
        if f.shape != items[0].shape or f.dtype != items[0].dtype or f.device != items[0].device:
            raise ValueError("the frames of one call must share shape, dtype and device")
    f0 = items[0]
    stacked = not as_list and f0.dim() == 4
    if stacked:
        k, (h, w, c) = f0.shape[0], _check_resize_frame(f0.shape[1:], "the device NIQE")
        if k < 1:
            raise ValueError("NIQE: empty stack")
    else:
        k, (h, w, c) = len(items), _check_resize_frame(f0.shape, "the device NIQE")
    return items, k, h, w, c, stacked


def niqe_features_device(frames, crop_border: int, params, channel_order: str = "rgb") -> torch.Tensor:
    """NIQE block features on the GPU (irm_niqe_features): `frames` is one uint8 / uint16 (or int16 = uint16 bit
    pattern) HW / HWC GPU tensor, a [K][H][W][C] stack, or a list of K frames of one shape.  Returns the
    [K][n_blocks][36] float64 device tensor of niqe_features' rows (fp64 arithmetic throughout), without
    synchronising; a frame's features are bitwise the same on every call and for any K.  CPU tensors raise
    HipLibraryError: there is no CPU fallback (niqe_features takes host planes)."""
    crop = _check_niqe_args(crop_border, "y", channel_order)
    _check_niqe_params(params)
    items, k, h, w, c, stacked = _niqe_frames(frames)
    nbh, nbw = _check_niqe_blocks(h, w, crop)
    f0 = items[0]
    if not f0.is_cuda:
        raise _hip.HipLibraryError("the device NIQE needs GPU tensors; there is no CPU fallback (calculate_niqe takes "
                                   "host arrays)")
    as_bits = (lambda x: x.view(torch.int16)) if f0.dtype == torch.uint16 else (lambda x: x)
    dev = f0.device
    with torch.cuda.device(dev):
        src = as_bits(f0).contiguous() if (stacked or k == 1) else torch.stack([as_bits(x) for x in items])
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


# ---------------------------------------------------------------------------
# tiled-patch inference
# ---------------------------------------------------------------------------

def tile_origins(extent: int, patch: int, overlap: int) -> list:
    """src/utils.py:385-388."""
    stride = max(patch - overlap, 1)
    return list(range(0, extent - patch, stride)) + [max(extent - patch, 0)]


_WINDOW_CACHE: dict = {}
_SIDE_STREAMS: dict = {}


def _side_stream(device, index: int):
    key = (str(device), index)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


def _window_on(device, ps: int) -> torch.Tensor:
    key = (str(device), ps)
    if key not in _WINDOW_CACHE:
        _WINDOW_CACHE[key] = torch.from_numpy(get_gaussian_weights(ps, ps, 1)[:, :, 0].copy()).to(device)
    return _WINDOW_CACHE[key]


_UNIT_RANGE_CACHE: dict = {}
#: floats of workspace irm_frame_minmax_f32 never needs more than (include/irm_hip_frames.h)
_MINMAX_WS_FLOATS = 2048


def _unit_range_on(device) -> torch.Tensor:
    """The constant value range (lo, hi, mul) = (0, 1, 1) of a frame that is in [0, 1] by contract, as the three-float
    device buffer the float32 tiler kernels read: no division on the way in, clip(v, 0, 1) on the way out."""
    key = str(device)
    if key not in _UNIT_RANGE_CACHE:
        _UNIT_RANGE_CACHE[key] = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float32).to(device)
    return _UNIT_RANGE_CACHE[key]


def _frame_range_on(img_dev: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """(min, max, max) of a float32 device frame, the reference's value range for a float image (utils.py:159-171,
    450-454), as a three-float device buffer; enqueued, never read by the host.  Non-finite values are outside the
    contract."""
    rng = torch.empty(3, dtype=torch.float32, device=img_dev.device)
    _hip.call("irm_frame_minmax_f32", _hip.ptr(img_dev), img_dev.numel(), _hip.ptr(rng), _hip.ptr(ws), ws.numel())
    return rng


#: bound of the per-model graph cache: entries, and bytes of graph-owned memory (static buffers + workspaces)
_GRAPH_MAX_ENTRIES, _GRAPH_MAX_BYTES = 8, 96 << 30


def _weights_version(model: Module):
    return _hip.param_key(model)


def _release_workspace(model: Module):
    rel = getattr(model, "release_workspace", None)
    if callable(rel):
        rel()


def graphed_forward(model: Module, x: torch.Tensor) -> torch.Tensor:
    """model(x) replayed from a HIP graph where that pays: the conv stacks and MaIR at small images are bound by
    the host's launch rate (hundreds of kernels of 10-60 us per image), not by the GPU.

    Opt-in per model (`model.hip_graph = True`, the default of the built-in model classes); off while a KernelTimer
    is installed (per-launch events need eager launches) and with IRM_NO_GRAPH=1.  The first call for an (input
    shape, stream, weights version) runs eagerly once (weight packing, LDS attributes), then captures the forward on
    torch's capture stream - every kernel of libirm_hip.so is enqueued on torch's current stream and allocates
    nothing, so the capture holds plain kernel nodes; later calls copy the input into the graph's static buffer and
    replay.  The returned tensor is the graph's static output: consume it (on the same stream) before the next call,
    as the tiler does.

    Ownership: a graph's kernels hold raw pointers, so every buffer they touch must live exactly as long as the
    graph.  The model's workspace is therefore dropped before the capture (`release_workspace()`), re-allocated
    INSIDE it - from the graph's private memory pool - and dropped again afterwards: the pool keeps those blocks for
    the graph alone, and no later eager call, other input shape or other graph can be handed the same memory
    (DnCNN's eagerly allocated layer buffers were freed on a shape change while an older graph still wrote
    to them).  The graphs live on the model object (`model._irm_graphs`), so they die with it; entries of other
    weight versions are dropped, the rest is bounded (least recently used)."""
    if (ops.TIMER is not None or not getattr(model, "hip_graph", False) or os.environ.get("IRM_NO_GRAPH")
            or not x.is_cuda or torch.cuda.is_current_stream_capturing()):
        return model(x)
    graphs = model.__dict__.get("_irm_graphs")
    if graphs is None:
        graphs = model.__dict__["_irm_graphs"] = {}
    version = _weights_version(model)
    key = (tuple(x.shape), x.device.index, torch.cuda.current_stream().cuda_stream, version)
    ent = graphs.pop(key, None)
    if ent is None:
        for k in [k for k in graphs if k[3] != version]:
            del graphs[k]                            # stale weights
        model(x)                                     # eager warm-up (packs weights, sets kernel attributes)
        _release_workspace(model)
        static_in = x.clone()
        g = torch.cuda.CUDAGraph()
        before = torch.cuda.memory_reserved(x.device)
        with torch.cuda.graph(g):
            static_out = model(static_in)
        _release_workspace(model)                    # the buffers stay reserved in g's private pool
        ent = (g, static_in, static_out, max(torch.cuda.memory_reserved(x.device) - before, 0))
        while graphs and (len(graphs) >= _GRAPH_MAX_ENTRIES
                          or sum(e[3] for e in graphs.values()) + ent[3] > _GRAPH_MAX_BYTES):
            del graphs[next(iter(graphs))]           # least recently used first (dict order = recency, see below)
    graphs[key] = ent                                # (re-)insert at the end: most recently used
    g, static_in, static_out, _ = ent
    static_in.copy_(x)
    g.replay()
    return static_out


def tiled_forward_device(model: Module, img_dev: torch.Tensor, patch_size, patch_overlap, pad8: bool,
                         noise_sigma=None, target_dev: torch.Tensor | None = None, max_batch: int = 8,
                         keep_tiles: list | None = None, hooks: str | None = None, unit_range: bool = False,
                         out: str = "same"):
    """Device pipeline for one uint8/uint16/float32 HWC image already on the GPU.

    Returns (out HWC device tensor, sse device tensor or None): uint8/uint16 like the input, float32 for a float32
    input or with out="float32" (tiled_forward_device_batch has the rules for float frames).
    Nothing here synchronises with the host.  hooks="deblurganv2" selects that model's normalize / pad /
    postprocess (src/deblurganv2/__init__.py:11-28) instead of /255 and the reflect pad to 8.
    """
    outs = tiled_forward_device_batch(model, [img_dev], patch_size, patch_overlap, pad8, noise_sigma,
                                      None if target_dev is None else [target_dev], max_batch, keep_tiles, hooks,
                                      unit_range, out)
    return outs[0]


def tiled_forward_device_batch(model: Module, imgs_dev: list, patch_size, patch_overlap, pad8: bool,
                               noise_sigma=None, targets_dev: list | None = None, max_batch: int = 8,
                               keep_tiles: list | None = None, hooks: str | None = None, unit_range: bool = False,
                               out: str = "same") -> list:
    """The device pipeline for SEVERAL images of one shape at once (throughput serving; the reference's loop,
    src/utils.py:353-454, is one image and one tile at a time): the tiles of all images form one batch axis, so the
    low-resolution levels of the network fill the GPU and every kernel's tail is paid once per batch instead of once per
    image (Restormer, 1280x720: 53.8 ms for one frame, 52.3 ms per frame for two, tools/bench_batch.py).  Each image is
    extracted, blended, requantised and scored exactly as in the single-image call - a tile's result does not depend on
    its batch (tests/test_gpu_fullsize.py) - and the list of (out, sse) pairs is returned in order.

    Float frames.  A float32 [H, W, C] frame gives a float32 [s H, s W, min(3, C)] frame.  unit_range=False is the
    reference's rule for a float image (utils.py:159-171, 450-454): the frame's own min / max are reduced on the device
    (irm_frame_minmax_f32), the frame is divided by max where max > 1, and the result is clip(v * max, min, max) - a max
    below 1 multiplies too, as it does there.  unit_range=True takes the frame as in [0, 1] by contract: no reduction,
    no division, the result is clip(v, 0, 1).  out="float32" returns the float32 frame for a uint8 / uint16 input as
    well: extracted as always (/255, /65535), blended with the unit range and not rounded; out="uint8" / "uint16" (the
    bit pattern in an int16 tensor, as on the way in) requantises a float32 frame that is in [0, 1] (unit_range=True) as
    an integer frame is: rint(clip(v * peak, 0, peak)).  A float32 result has no
    integer squared error (targets_dev raises ValueError), and hooks="deblurganv2" is defined on raw integer values
    with an integer result (a float32 input or out="float32" raises ValueError).  Non-finite values in a float frame
    are outside the contract."""
    if out not in ("same", "float32", "uint8", "uint16"):
        raise ValueError(f"out must be 'same', 'float32', 'uint8' or 'uint16', not {out!r}")
    norm_mean, norm_inv_std, post_scale, post_shift = 0.0, 1.0, 1.0, 0.0
    pad_mode = "reflect8" if pad8 else "none"
    if hooks == "deblurganv2":
        norm_mean = float(np.float32(0.5) * np.float32(255.0))
        norm_inv_std = float(np.float32(1.0) / (np.float32(0.5) * np.float32(255.0)))
        post_scale, post_shift, pad_mode = 0.5, 1.0, "zero32"
    s = int(getattr(model, "upscale", 1) or 1)             # super-resolving model: outputs s x the tile
    if s > 1 and noise_sigma is not None:
        raise ValueError("need_degradation with a super-resolution model: the reference defines no SR degradation")
    img0 = imgs_dev[0]
    h, w, c = img0.shape
    if any(tuple(im.shape) != (h, w, c) or im.dtype != img0.dtype for im in imgs_dev):
        raise ValueError("tiled_forward_device_batch: the images of a batch must share shape and dtype")
    is_u16 = img0.dtype in (torch.uint16, torch.int16)
    is_f32 = img0.dtype == torch.float32
    if img0.dtype.is_floating_point and not is_f32:
        raise ValueError(f"the device pipeline takes uint8, uint16 and float32 frames, not {img0.dtype}")
    own = "float32" if is_f32 else "uint16" if is_u16 else "uint8"
    kind = own if out == "same" else out
    f32_out = kind == "float32"
    if not f32_out and kind != own and not (is_f32 and unit_range):
        raise ValueError(f"out={out!r} for a {own} frame: an integer result comes from a frame of that type, or from a "
                         "float32 frame with unit_range=True")
    out_dtype = img0.dtype if kind == own else torch.uint8 if kind == "uint8" else torch.int16
    out_u16 = kind == "uint16"
    if (is_f32 or f32_out) and hooks == "deblurganv2":
        raise ValueError("hooks='deblurganv2' normalises raw integer values and requantises: no float32 frames")
    if f32_out and targets_dev is not None:
        raise ValueError("targets_dev needs an integer result: a float32 frame has no integer squared error")
    dev = img0.device
    if patch_size:
        ps = min(patch_size, max(h, w))
        ys, xs = tile_origins(h, ps, patch_overlap), tile_origins(w, ps, patch_overlap)
    else:
        ps, ys, xs = max(h, w), [0], [0]
    th, tw = min(ps, h), min(ps, w)
    if pad_mode == "reflect8":
        ph = (th // 8 + 1) * 8 if th % 8 else th
        pw = (tw // 8 + 1) * 8 if tw % 8 else tw
    elif pad_mode == "zero32":
        ph, pw = (th // 32 + 1) * 32, (tw // 32 + 1) * 32
    else:
        ph, pw = th, tw
    origins = [(y0, x0) for y0 in ys for x0 in xs]
    T = len(origins)
    K = len(imgs_dev)
    org = torch.tensor(origins, dtype=torch.int32).to(dev, non_blocking=True)
    noise = None
    if noise_sigma is not None:
        np.random.seed(seed=0)                       # utils.py:33: same field for every tile
        noise = torch.from_numpy(np.random.normal(0, noise_sigma / 255., (th, tw, c))).to(dev)
    tiles = torch.empty(K * T, c, ph, pw, dtype=torch.float32, device=dev)
    ranges = [_unit_range_on(dev)] * K if (is_f32 or f32_out) else None
    if is_f32 and not unit_range:
        ws = torch.empty(_MINMAX_WS_FLOATS, dtype=torch.float32, device=dev)      # (one stream: the frames take turns)
        ranges = [_frame_range_on(im, ws) for im in imgs_dev]
    for k, im in enumerate(imgs_dev):
        if is_f32:
            _hip.call("irm_tile_extract_f32", _hip.ptr(im), _hip.ptr(ranges[k]), _hip.ptr(org), _hip.ptr(noise),
                      _hip.ptr(tiles[k * T:]), h, w, c, th, tw, ph, pw, T, int(pad_mode == "zero32"))
            continue
        _hip.call("irm_tile_extract", _hip.ptr(im), int(is_u16), _hip.ptr(org), _hip.ptr(noise),
                  _hip.ptr(tiles[k * T:]), h, w, c, th, tw, ph, pw, T, float(norm_mean), float(norm_inv_std),
                  int(pad_mode == "zero32"))
    c_out = min(3, c)
    pred = None
    if ops.TIMER is not None:
        ops.TIMER.break_chain()                    # the tile extraction above is not a timed launch
    NT = K * T
    nstreams = min(int(getattr(model, "num_streams", 1)), NT)
    if nstreams > 1 and not os.environ.get("IRM_EXPERIMENTAL_STREAMS"):
        # EXPERIMENTAL, off in the product: on some GPUs of the pool overlapping forwards were not bit-reproducible
        # (rare stale read of an in-place updated buffer, cause not established: DESIGN.md section 6)
        raise ValueError("model.num_streams > 1 is experimental (not bit-reproducible on every GPU, DESIGN.md section 6); "
                         "set IRM_EXPERIMENTAL_STREAMS=1 to run it")
    if nstreams > 1:
        # independent tile groups on separate HIP streams: one group's HBM-bound kernels overlap the
        # other's MFMA-bound GEMMs; the groups join before the blend
        main = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(main)
        per = -(-NT // nstreams)
        done, outs = [], []
        for gi, i in enumerate(range(0, NT, per)):
            st = _side_stream(dev, gi)
            st.wait_event(ready)
            with torch.cuda.stream(st):
                o = model(tiles[i:i + per])              # (side streams: eager)
                outs.append((i, o))
                ev = torch.cuda.Event()
                ev.record(st)
                done.append(ev)
        for ev in done:
            main.wait_event(ev)
        pred = torch.empty(NT, *outs[0][1].shape[1:], dtype=torch.float32, device=dev)
        for i, o in outs:
            pred[i:i + o.shape[0]] = o
            o.record_stream(main)
    else:
        for i in range(0, NT, max_batch):
            o = graphed_forward(model, tiles[i:i + max_batch]) if callable(getattr(model, "forward", None)) else model(tiles[i:i + max_batch])
            if pred is None:
                pred = o if o.shape[0] == NT else torch.empty(NT, *o.shape[1:], dtype=torch.float32, device=dev)
            if pred is not o:
                pred[i:i + o.shape[0]] = o
    if s > 1 and tuple(pred.shape[2:]) != (s * ph, s * pw):
        raise ValueError(f"model.upscale = {s}: expected {s * ph}x{s * pw} predictions for {ph}x{pw} tiles, "
                         f"got {tuple(pred.shape[2:])}")
    if keep_tiles is not None:
        keep_tiles.append(pred[:, :c_out, :s * th, :s * tw].clone())
    results = []
    for k in range(K):
        if f32_out:
            # extents in input pixels, predictions and window at output scale (irm_hip_frames.h)
            frame = torch.empty(s * h, s * w, c_out, dtype=torch.float32, device=dev)
            _hip.call("irm_window_blend_f32", _hip.ptr(pred[k * T:]), _hip.ptr(org), _hip.ptr(_window_on(dev, s * ps)),
                      _hip.ptr(frame), _hip.ptr(ranges[k]), h, w, c_out, pred.shape[1], th, tw, pred.shape[2] // s,
                      pred.shape[3] // s, ps, T, s)
            results.append((frame, None))
            continue
        frame = torch.empty(s * h, s * w, c_out, dtype=out_dtype, device=dev)
        sse, tgt = None, None
        if targets_dev is not None and targets_dev[k] is not None:
            sse, tgt = torch.zeros(1, dtype=torch.int64, device=dev), targets_dev[k]
        if s > 1:
            # tiles cut at input scale, blended at output scale: origins x s, window of s * ps (irm_hip.h)
            _hip.call("irm_window_blend_scaled", _hip.ptr(pred[k * T:]), _hip.ptr(org), _hip.ptr(_window_on(dev, s * ps)),
                      _hip.ptr(frame), int(out_u16), _hip.ptr(tgt), _hip.ptr(sse), h, w, c_out, pred.shape[1], th, tw, ph, pw,
                      ps, T, s, post_scale, post_shift)
        else:
            _hip.call("irm_window_blend", _hip.ptr(pred[k * T:]), _hip.ptr(org), _hip.ptr(_window_on(dev, ps)), _hip.ptr(frame),
                      int(out_u16), _hip.ptr(tgt), _hip.ptr(sse), h, w, c_out, pred.shape[1], th, tw,
                      pred.shape[2], pred.shape[3], ps, T, post_scale, post_shift)
        results.append((frame, sse))
    return results


def run_model_inference(model: Module, input_img: np.ndarray, device: torch.device,
                        normalize: Callable = normalize, patch_size: int | None = None, patch_overlap: int = 32,
                        need_degradation=False, noise_level=None, pad: Callable | None = None,
                        postprocess: Callable | None = None, progress_bar=None):
    """Run inference; returns (prediction, inference_time_ms) like src/utils.py:353-454.

    uint8/uint16 and float32 HWC images with the stock normalize/pad hooks take
    the device pipeline (a float32 image by the reference's rule for float
    images: divided by its max where that exceeds 1, clipped to its own min /
    max, float32 out); anything else (float64 / float16 images, custom hooks,
    DeblurGANv2 on a float image) takes a per-tile loop with the reference's
    host-side blend - the model forward is the HIP path in both."""
    output_img, ms, _ = _run_model_inference(model, input_img, device, normalize, patch_size, patch_overlap,
                                             need_degradation, noise_level, pad, postprocess)
    return output_img, ms


def _run_model_inference(model, input_img, device, normalize=normalize, patch_size=None, patch_overlap=32,
                         need_degradation=False, noise_level=None, pad=None, postprocess=None):
    """run_model_inference that also hands back the device pipeline's output tensor (uint8, uint16 as int16 bits, or
    float32; None after the per-tile host loop): (prediction, inference_time_ms, out_dev).  The time covers the same work as
    run_model_inference's, input upload through output download."""
    start_time = time.time()
    out = None
    if need_degradation and int(getattr(model, "upscale", 1) or 1) > 1:
        raise ValueError("need_degradation with a super-resolution model: the reference defines no SR degradation")
    dg = (normalize is deblurganv2.normalize and pad is deblurganv2.pad and postprocess is deblurganv2.postprocess
          and input_img.dtype == np.uint8)
    stock = dg or (normalize is globals()['normalize'] and (pad is None or pad is globals()['pad'])
                   and postprocess is None
                   and (input_img.dtype in (np.uint8, np.uint16)
                        or (input_img.dtype == np.float32 and input_img.ndim == 3)))
    with torch.no_grad():
        if stock:
            dev = torch.device(device)
            src = input_img.view(np.int16) if input_img.dtype == np.uint16 else input_img
            img_dev = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
            sigma = noise_level if (need_degradation and noise_level is not None) else None
            out, _ = tiled_forward_device(model, img_dev, patch_size, patch_overlap, pad is not None, sigma,
                                          max_batch=getattr(model, 'max_tiles_per_batch', 8),
                                          hooks="deblurganv2" if dg else None)
            output_img = out.cpu().numpy()
            if input_img.dtype == np.uint16:
                output_img = output_img.view(np.uint16)
        else:
            output_img = _run_tiles_on_host(model, input_img, device, normalize, patch_size, patch_overlap,
                                            need_degradation, noise_level, pad, postprocess)
    return output_img, (time.time() - start_time) * 1000, out


def _run_tiles_on_host(model, input_img, device, normalize_fn, patch_size, patch_overlap, need_degradation,
                       noise_level, pad_fn, postprocess):
    """Per-tile loop with arbitrary hooks (reference order of operations, utils.py:379-450)."""
    img = normalize_fn(input_img)
    h, w = img.shape[:2]
    if patch_size:
        ps = min(patch_size, max(h, w))
        ys, xs = tile_origins(h, ps, patch_overlap), tile_origins(w, ps, patch_overlap)
    else:
        ps, ys, xs = max(h, w), [0], [0]
    c_out = min(3, img.shape[2])
    s = int(getattr(model, "upscale", 1) or 1)        # super resolution: blend at output scale
    acc = np.zeros((s * h, s * w, c_out), np.float32)
    wsum = np.zeros((s * h, s * w, c_out), np.float32)
    win = get_gaussian_weights(s * ps, s * ps, c_out)
    for y0 in ys:
        for x0 in xs:
            tile = img[y0:y0 + ps, x0:x0 + ps, :].copy()
            if need_degradation and noise_level is not None:
                tile = add_gaussian_noise(tile, noise_level)
            t = torch.from_numpy(tile.transpose(2, 0, 1)).unsqueeze(0).to(device)
            if pad_fn is not None:
                hp, wp = t.shape[-2:]
                o = model(pad_fn(t))[:, :, :s * hp, :s * wp]
            else:
                o = model(t)
            if postprocess is not None:
                o = postprocess(o)
            p = o.squeeze(0).cpu().numpy().transpose(1, 2, 0)
            ch, cw = p.shape[:2]
            acc[s * y0:s * y0 + ch, s * x0:s * x0 + cw, :] += p * win[:ch, :cw]
            wsum[s * y0:s * y0 + ch, s * x0:s * x0 + cw, :] += win[:ch, :cw]
    acc /= np.maximum(wsum, 1e-8)
    if input_img.dtype == np.uint16:
        return np.clip(acc * 65535.0, 0, 65535).round().astype(np.uint16)
    if input_img.dtype == np.uint8:
        return np.clip(acc * 255.0, 0, 255).round().astype(np.uint8)
    lo, hi = np.min(input_img), np.max(input_img)
    return np.clip(acc * hi, lo, hi).astype(input_img.dtype)


def get_model_prediction(model: Module, input_image: np.ndarray, device: torch.device, patch_size: int,
                         patch_overlap: int, need_degradation=False, noise_level=None, progress_bar=None):
    """src/utils.py:270-311: dispatch on the model class (reflect-pad-to-8 models vs plain)."""
    pred, ms, _ = _get_model_prediction(model, input_image, device, patch_size, patch_overlap, need_degradation,
                                        noise_level)
    return pred, ms


def _get_model_prediction(model, input_image, device, patch_size, patch_overlap, need_degradation=False,
                          noise_level=None):
    """get_model_prediction through _run_model_inference: (prediction, inference_time_ms, out_dev or None)."""
    kw = dict(patch_size=patch_size, patch_overlap=patch_overlap, need_degradation=need_degradation,
              noise_level=noise_level)
    if isinstance(model, (FPNMobileNet,)):                      # utils.py:280-291
        return _run_model_inference(model, input_image, device, normalize=deblurganv2.normalize, pad=deblurganv2.pad,
                                    postprocess=deblurganv2.postprocess, **kw)
    if isinstance(model, _PAD8_MODELS):
        return _run_model_inference(model, input_image, device, pad=pad, **kw)
    return _run_model_inference(model, input_image, device, **kw)


def _chain_hooks(model) -> bool:
    """pad8 of a chain stage, by the model class as _get_model_prediction dispatches; DeblurGANv2 is refused."""
    if isinstance(model, FPNMobileNet) or type(model).__module__.startswith(deblurganv2.__name__ + "."):
        raise ValueError("run_model_chain: DeblurGANv2 normalises raw integer values and has no float32 frames; "
                         "run it on its own with get_model_prediction")
    return isinstance(model, _PAD8_MODELS)


def run_model_chain(stages, input_img: np.ndarray, device: torch.device, need_degradation=False, noise_level=None,
                    out: str = "same"):
    """Run several restoration models one after another on one frame: denoise then deblur, denoise then
    super-resolve.  Returns (image, inference_time_ms), the time from input upload through output download.

    `stages` is a sequence of (model, patch_config) with patch_config = {'patch_size': .., 'patch_overlap': ..} as
    get_patch_config returns it.  Every stage is the device pipeline of run_model_inference with the hooks
    get_model_prediction picks for the model class (reflect pad to 8 for Restormer / MaIR); a DeblurGANv2 model
    raises ValueError.  The frame is uploaded once and downloaded once.

    The reference has no chain; these semantics are this package's own:
      1. the first stage reads the input as run_model_inference does (uint8 / 255, uint16 / 65535); a float32 input is
         taken as in [0, 1] already (unit_range=True of tiled_forward_device: no division by its max);
      2. every frame between two stages is float32, clipped to [0, 1] and never rounded to 255 levels - the next model
         does not see a quantisation step as new noise - and stays on the device;
      3. need_degradation / noise_level apply to the first stage only;
      4. the last stage requantises to the input's dtype as run_model_inference does, or returns the float32 frame in
         [0, 1] for a float32 input or with out="float32".
    Super-resolving stages enlarge the frame for the stages after them; a 6-channel first stage yields 3 channels.  A
    one-stage chain on a uint8 / uint16 frame returns exactly what get_model_prediction returns."""
    try:
        stages = [(m, dict(cfg)) for m, cfg in stages]
    except (TypeError, ValueError):
        raise ValueError("run_model_chain: stages is a sequence of (model, patch_config) pairs") from None
    if not stages:
        raise ValueError("run_model_chain: at least one stage")
    for m, cfg in stages:
        if not callable(m) or set(cfg) != {"patch_size", "patch_overlap"}:
            raise ValueError("run_model_chain: a stage is (model, {'patch_size': .., 'patch_overlap': ..})")
    pad8 = [_chain_hooks(m) for m, _ in stages]
    if out not in ("same", "float32"):
        raise ValueError(f"out must be 'same' or 'float32', not {out!r}")
    if (not isinstance(input_img, np.ndarray) or input_img.ndim != 3
            or input_img.dtype not in (np.uint8, np.uint16, np.float32)):
        raise ValueError("run_model_chain: a uint8, uint16 or float32 [H, W, C] array")
    if need_degradation and int(getattr(stages[0][0], "upscale", 1) or 1) > 1:
        raise ValueError("need_degradation with a super-resolution model: the reference defines no SR degradation")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _hip.HipLibraryError("run_model_chain runs on the GPU only (no CPU fallback); pass a 'cuda' device")
    start_time = time.time()
    with torch.no_grad():
        src = input_img.view(np.int16) if input_img.dtype == np.uint16 else input_img
        frame = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
        sigma = noise_level if (need_degradation and noise_level is not None) else None
        last = len(stages) - 1
        final = "float32" if out == "float32" else str(input_img.dtype)      # the last stage requantises
        for i, ((m, cfg), p8) in enumerate(zip(stages, pad8)):
            kind = final if i == last else "float32"
            frame, _ = tiled_forward_device(m, frame, cfg["patch_size"], cfg["patch_overlap"], p8,
                                            sigma if i == 0 else None,
                                            max_batch=getattr(m, 'max_tiles_per_batch', 8), unit_range=True, out=kind)
        output_img = frame.cpu().numpy()
    if output_img.dtype == np.int16:
        output_img = output_img.view(np.uint16)
    return output_img, (time.time() - start_time) * 1000
