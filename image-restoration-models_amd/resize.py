"""The super-resolution protocol's resize: MATLAB's bicubic imresize, antialiased when
shrinking, restated in float64 on the host and run on the GPU (irm_imresize_bicubic)."""
from __future__ import annotations

import numpy as np
import torch

from . import _hip
from .frames import FRAME_DTYPES, device_constant, device_frames, frame_bits, frame_shape

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


def imresize_host(img: np.ndarray, scale, out: str = "float") -> np.ndarray:
    """MATLAB bicubic imresize (antialiased when shrinking) of a uint8 / uint16 HW or HWC frame, restated in float64:
    the frame / 255 (65535), the H pass, then the W pass.  out="float": float64 in [0, 1] nominal, unrounded;
    out="same": clipped to [0, 1], x 255 (65535), rounded half to even, in the frame's dtype (tensor2img)."""
    if out not in ("float", "same"):
        raise ValueError(f"out must be 'float' or 'same', not {out!r}")
    if not isinstance(img, np.ndarray) or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("imresize_host takes uint8 or uint16 numpy frames")
    h, w, _ = frame_shape(img.shape, "imresize_host")
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


def _resize_table_on(device, in_length: int, s: int, shrink: bool) -> tuple:
    """The axis table on the device (fp32 weights, int32 indices), cached per (device, length, factor) like
    mairunet_arch.scan_ids: a repeated or captured call enqueues kernels only."""
    def build():
        w, i = resize_table(in_length, 1.0 / s if shrink else s)
        return (torch.from_numpy(w.astype(np.float32)).contiguous().to(device),
                torch.from_numpy(i.astype(np.int32)).contiguous().to(device))
    return device_constant(("resize", str(device), in_length, s, shrink), build)


def imresize_device(frames, scale, out: str = "same"):
    """MATLAB bicubic imresize on the GPU (irm_imresize_bicubic): `frames` is one uint8 / uint16 (or int16 = uint16 bit
    pattern) HW / HWC GPU tensor, a [K][H][W][C] stack, or a list of frames of one shape; scale is s or 1/s, s in
    {2, 3, 4}.  out="same": quantised to the input's dtype (how LR files are made); out="float": float32 in [0, 1]
    nominal, unrounded.  Returns the same arrangement (tensor -> tensor, list -> list) without synchronising."""
    if out not in ("float", "same"):
        raise ValueError(f"out must be 'float' or 'same', not {out!r}")
    s, shrink = _resize_factor(scale)
    as_list = isinstance(frames, (list, tuple))
    first = frames[0] if as_list and frames else frames
    if isinstance(first, torch.Tensor) and first.dtype in FRAME_DTYPES and not first.is_cuda:
        # as before the split: a CPU frame is refused ahead of the shape, stack and tap checks (device_frames below)
        raise ValueError("imresize_device needs GPU tensors; there is no CPU fallback (imresize_host takes host arrays)")
    items, k, h, w, c, stacked = device_frames(frames, "imresize_device", "imresize_host takes numpy arrays")
    p = 4 * s + 2 if shrink else 6
    if min(h, w) < p:
        raise ValueError(f"resize by {scale:g}: a {h}x{w} frame has a side shorter than the {p} taps")
    oh, ow = (-(-h // s), -(-w // s)) if shrink else (h * s, w * s)
    f0 = items[0]
    dev = f0.device
    with torch.cuda.device(dev):
        src = frame_bits(items, stacked)
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
