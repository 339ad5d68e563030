"""What the frame front ends (metrics, resize, NIQE, the tiled pipeline) share: the checks that need no GPU, the int16
view of uint16 frames, upload / download of a host frame, one cache of per-device constants, PSNR from an error."""
from __future__ import annotations

import numpy as np
import torch

#: int16 is read as the uint16 bit pattern, as the tiler does (its uint16 frames travel as int16 tensors)
FRAME_DTYPES = (torch.uint8, torch.uint16, torch.int16)


def frame_shape(shape, what="imresize") -> tuple:
    """(H, W, C) of an HW or HWC shape with 1 or 3 channels."""
    if len(shape) == 2:
        return shape[0], shape[1], 1
    if len(shape) == 3 and shape[2] in (1, 3):
        return tuple(shape)
    raise ValueError(f"{what} takes HW or HWC frames with 1 or 3 channels, not shape {tuple(shape)}")


def device_frames(frames, what: str, host: str, label: str | None = None, float32: bool = False) -> tuple:
    """tensor | list of tensors of one shape | [K][H][W][C] stack -> (items, K, H, W, C, stacked): the checks that
    need no GPU; a 4-D tensor is always read as a stack.  `what` ("the device NIQE") and `host` (what to say about the
    numpy twin) word the messages; `label` opens the two about an empty call; `float32`: float32 frames are taken too."""
    as_list = isinstance(frames, (list, tuple))
    items = list(frames) if as_list else [frames]
    if not items:
        raise ValueError(f"{label or what}: no frames")
    f0 = items[0]
    for f in items:
        if not isinstance(f, torch.Tensor):
            raise ValueError(f"{what} takes torch tensors ({host})")
        if f.dtype not in FRAME_DTYPES and not (float32 and f.dtype == torch.float32):
            raise ValueError(f"{what} takes uint8{', uint16 or float32' if float32 else ' or uint16'} frames, not {f.dtype}")
        if f.shape != f0.shape or f.dtype != f0.dtype or f.device != f0.device:
            raise ValueError("the frames of one call must share shape, dtype and device")
    stacked = not as_list and f0.dim() == 4
    h, w, c = frame_shape(f0.shape[1:] if stacked else f0.shape, what)
    k = f0.shape[0] if stacked else len(items)
    if k < 1:
        raise ValueError(f"{label or what}: empty stack")
    return items, k, h, w, c, stacked


def pair_frames(preds, targets, host: str) -> tuple:
    """The K prediction / target pairs of a device metric as two lists, with the checks that need no GPU: per pair
    torch tensors of one shape and dtype (asked before the dtype itself, so "differ" wins for a float32 prediction
    with a uint8 target), uint8 / uint16, and like the first pair.  No stack: a pair is two frames."""
    preds, targets = list(preds), list(targets)
    if not preds or len(preds) != len(targets):
        raise ValueError(f"{len(preds)} predictions and {len(targets)} targets: need the same number, at least one")
    for p, t in zip(preds, targets):
        if not isinstance(p, torch.Tensor) or not isinstance(t, torch.Tensor):
            raise ValueError(f"device metrics take torch tensors (use {host} for numpy arrays)")
        if p.shape != t.shape or p.dtype != t.dtype:
            raise ValueError(f"prediction {tuple(p.shape)} {p.dtype} and target {tuple(t.shape)} {t.dtype} differ in "
                             "shape or dtype")
        if p.dtype not in FRAME_DTYPES:
            raise ValueError(f"device metrics take uint8 or uint16 frames, not {p.dtype}")
        if p.shape != preds[0].shape or p.dtype != preds[0].dtype:
            raise ValueError("the frames of one call must share shape and dtype")
    return preds, targets


def frame_bits(items, stacked: bool = False) -> torch.Tensor:
    """The contiguous tensor the kernels read: uint16 as its int16 bit pattern (the copies need no uint16 kernels),
    the frame itself for K = 1 or a stack, else a torch.stack."""
    bits = [x.view(torch.int16) if x.dtype == torch.uint16 else x for x in items]
    return bits[0].contiguous() if (stacked or len(bits) == 1) else torch.stack(bits)


def to_device(img: np.ndarray, device) -> torch.Tensor:
    """A host frame on the device (uint16 as its int16 bit pattern, as the tiler takes it)."""
    src = img.view(np.int16) if img.dtype == np.uint16 else img
    return torch.from_numpy(np.ascontiguousarray(src)).to(device)


def to_host(t: torch.Tensor) -> np.ndarray:
    """The device frame as a host array; the uint16 bit pattern (an int16 or uint16 tensor) comes back as uint16."""
    a = t.view(torch.int16).cpu().numpy() if t.dtype == torch.uint16 else t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def plane_slots(shapes, dtype, k: int, device, pinned: bool) -> tuple:
    """One buffer for k frames whose planes (`shapes`) lie behind one another, pinned host memory or on `device`:
    (buffer, per frame the views of its planes, elements of a frame).  The views of a pinned buffer are numpy's."""
    sizes = [int(np.prod(s)) for s in shapes]
    per = sum(sizes)
    buf = torch.empty(k * per, dtype=dtype, pin_memory=True) if pinned else torch.empty(k * per, dtype=dtype, device=device)
    flat = buf.numpy() if pinned else buf
    if pinned and dtype == torch.int16:
        flat = flat.view(np.uint16)                                          # the uint16 bit pattern, as to_host reads it
    views, off = [], 0
    for _ in range(k):
        frame = []
        for n, s in zip(sizes, shapes):
            frame.append(flat[off:off + n].reshape(s))
            off += n
        views.append(frame)
    return buf, views, per


_DEVICE_CONSTANTS: dict = {}


def device_constant(key: tuple, build):
    """build() once per key (which names the device): the per-device tables, windows and streams, so a repeated or
    captured call enqueues kernels only."""
    if key not in _DEVICE_CONSTANTS:
        _DEVICE_CONSTANTS[key] = build()
    return _DEVICE_CONSTANTS[key]


def check_order_and_crop(channel_order, crop_border) -> int:
    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', not {channel_order!r}")
    if int(crop_border) != crop_border or crop_border < 0:
        raise ValueError(f"crop_border must be a non-negative integer, not {crop_border!r}")
    return int(crop_border)


def psnr_from_error(peak, err) -> float:
    """PSNR of a mean squared error at the given peak; inf for none."""
    return float('inf') if err == 0 else float(10 * np.log10(peak ** 2 / err))
