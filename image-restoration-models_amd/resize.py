"""The super-resolution protocol's resize: MATLAB's bicubic imresize, antialiased when
shrinking, restated in float64 on the host and run on the GPU (irm_imresize_bicubic).  Below it the resize to any size
(DESIGN.md section 25): the same `contributions` formula for any scale, three kernels and both axes on their own
(resize_taps, resize_host), run on the GPU from the tap tables (irm_resize_taps: resize_device), and the Resize stage of
run_model_chain."""
from __future__ import annotations

import dataclasses
import math

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


# --------------------------------------------------------------------------- any size, three kernels
def _lanczos3(x: np.ndarray) -> np.ndarray:
    return np.where(np.abs(x) < 3, np.sinc(x) * np.sinc(x / 3.0), 0.0)


def _triangle(x: np.ndarray) -> np.ndarray:
    return np.maximum(0.0, 1.0 - np.abs(x))


#: name -> (kernel function, kernel width kw)
RESIZE_KERNELS = {"bicubic": (_cubic, 4.0), "lanczos3": (_lanczos3, 6.0), "bilinear": (_triangle, 2.0)}
#: taps per output coordinate the device entry takes (1/16 with lanczos3 has 98)
RESIZE_MAX_TAPS = 128
#: output columns per workgroup, widest first, and the LDS window a workgroup's intermediate may fill
#: (8 rows x source columns x C floats; both as irm_resize_taps states them)
RESIZE_TOWS = (128, 64, 32, 16, 8)
RESIZE_WINDOW_BYTES = 32768
#: the window the host stays under where some tile does: at 1/4 bicubic the 32-column tile of irm_imresize_bicubic
#: (13.4 KiB).  The 64-column tile (26 KiB) halves the workgroups of a 320 x 180 output to 115 on 256 CUs and measured
#: 1.79 x the time (profiles/bench_resize.jsonl)
RESIZE_WINDOW_PREFERRED = 16384
_OUT_KINDS = {"same": 0, "float": 1, "unit": 2}


def _check_kernel(kernel) -> tuple:
    if not isinstance(kernel, str) or kernel not in RESIZE_KERNELS:
        raise ValueError(f"resize kernel must be one of {sorted(RESIZE_KERNELS)}, not {kernel!r}")
    return RESIZE_KERNELS[kernel]


def _tap_count(scale: float, kernel: str, antialias: bool) -> tuple:
    """(width, P) of MATLAB's contributions: the kernel width, stretched by 1 / scale when shrinking with
    antialiasing, and P = ceil(width) + 2 taps."""
    kw = _check_kernel(kernel)[1]
    width = kw / scale if (scale < 1 and antialias) else kw
    return width, int(math.ceil(width)) + 2


def resize_taps(in_length: int, out_length: int, scale, kernel: str = "bicubic", antialias: bool = True) -> tuple:
    """Taps of MATLAB's imresize (`contributions`) along one axis for any scale, in float64, spelled as resize_table
    spells them: (weights [out_length][P], indices [out_length][P] int64, 0-based and reflected into [0, in_length)).
    u = x / scale + 0.5 (1 - 1 / scale) for the 1-based output coordinate x; kernel width kw (4 bicubic, 6 lanczos3,
    2 bilinear), or kw / scale when shrinking with antialiasing; P = ceil(width) + 2 taps from floor(u - width / 2);
    weights k(d), or scale k(scale d) when shrinking with antialiasing; rows normalised to sum 1.  Zero-weight edge taps
    stay in the table.  At the factors of resize_table and the bicubic kernel the fp32 weights and the indices are
    resize_table's."""
    fn = _check_kernel(kernel)[0]
    in_length, out_length = int(in_length), int(out_length)
    if not isinstance(scale, (int, float, np.integer, np.floating)) or not (scale > 0) or not math.isfinite(scale):
        raise ValueError(f"resize scale must be a positive number, not {scale!r}")
    if out_length < 1:
        raise ValueError(f"resize: the output length must be at least 1, not {out_length}")
    scale = float(scale)
    stretch = scale < 1 and bool(antialias)
    width, p = _tap_count(scale, kernel, antialias)
    if in_length < p:
        raise ValueError(f"resize by {scale:g} ({kernel}): a side of {in_length} is shorter than the {p} taps")
    x = np.arange(1, out_length + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - width / 2)
    idx = left[:, None] + np.arange(p, dtype=np.float64)[None, :]           # 1-based
    dist = u[:, None] - idx
    w = scale * fn(dist * scale) if stretch else fn(dist)
    w = w / w.sum(1, keepdims=True)
    i0 = idx.astype(np.int64) - 1
    i0 = np.where(i0 < 0, -i0 - 1, np.where(i0 >= in_length, 2 * in_length - 1 - i0, i0))
    assert i0.min() >= 0 and i0.max() < in_length
    return w, i0


def resize_plan(h: int, w: int, size=None, scale=None, kernel: str = "bicubic", antialias: bool = True) -> tuple:
    """(oh, ow, scale_h, scale_w) of a resize of an h x w frame, with every check that needs no frame.  scale=s is
    MATLAB's scalar form: out = ceil(in * s) on both axes and that s in both tables; size=(oh, ow) is the vector form:
    the scale of an axis is out / in.  Exactly one of the two; a side shorter than its taps raises ("shorter")."""
    _check_kernel(kernel)
    if (size is None) == (scale is None):
        raise ValueError("resize takes exactly one of size=(oh, ow) and scale=s")
    if scale is not None:
        if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) \
                or not (scale > 0) or not math.isfinite(scale):
            raise ValueError(f"resize scale must be a positive number, not {scale!r}")
        sh = sw = float(scale)
        oh, ow = int(math.ceil(h * sh)), int(math.ceil(w * sw))
    else:
        try:
            oh, ow = size
            ok = int(oh) == oh and int(ow) == ow and oh >= 1 and ow >= 1
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"resize size must be (oh, ow), two positive integers, not {size!r}")
        oh, ow = int(oh), int(ow)
        sh, sw = oh / h, ow / w
    for n, s in ((h, sh), (w, sw)):
        p = _tap_count(s, kernel, antialias)[1]
        if n < p:
            raise ValueError(f"resize by {s:g} ({kernel}): a {h}x{w} frame has a side shorter than the {p} taps")
    return oh, ow, sh, sw


def resize_host(img: np.ndarray, size=None, scale=None, kernel: str = "bicubic", antialias: bool = True,
                out: str = "float") -> np.ndarray:
    """Resize a uint8 / uint16 / float32 HW or HWC frame to any size with MATLAB's imresize arithmetic, in float64: the
    statement irm_resize_taps is held to.  Integer frames are divided by 255 / 65535, a float32 frame is taken as it
    is; the H pass runs first, then the W pass, taps in ascending order - the order of imresize_host and of basicsr,
    not MATLAB's rule of resizing the axis with the smaller scale first.  size / scale as resize_plan reads them.
    out="float": the unrounded float64 result; out="unit": that clipped to [0, 1]; out="same": integer frames clipped
    to [0, 1], x 255 (65535) and rounded half to even in the frame's dtype, a float32 frame as float32 (unclipped)."""
    if out not in _OUT_KINDS:
        raise ValueError(f"out must be 'float', 'same' or 'unit', not {out!r}")
    if not isinstance(img, np.ndarray) or img.dtype not in (np.uint8, np.uint16, np.float32):
        raise ValueError("resize_host takes uint8, uint16 or float32 numpy frames")
    h, w, _ = frame_shape(img.shape, "resize_host")
    oh, ow, sh, sw = resize_plan(h, w, size, scale, kernel, antialias)
    wh, ih = resize_taps(h, oh, sh, kernel, antialias)
    ww, iw = resize_taps(w, ow, sw, kernel, antialias)
    peak = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0}.get(img.dtype)
    x = img.astype(np.float64) / peak if peak else img.astype(np.float64)
    mid = np.zeros((oh,) + x.shape[1:], np.float64)
    for p in range(wh.shape[1]):                                              # ascending tap order
        mid += wh[:, p].reshape((-1,) + (1,) * (x.ndim - 1)) * x[ih[:, p]]
    res = np.zeros((oh, ow) + mid.shape[2:], np.float64)
    for p in range(ww.shape[1]):
        res += ww[:, p].reshape((1, -1) + (1,) * (x.ndim - 2)) * mid[:, iw[:, p]]
    if out == "float":
        return res
    if out == "unit":
        return np.clip(res, 0.0, 1.0)
    if peak is None:
        return res.astype(np.float32)
    return np.round(np.clip(res, 0.0, 1.0) * peak).astype(img.dtype)


def tile_span(indices: np.ndarray, tow: int) -> int:
    """The largest number of source columns the taps of any aligned run of `tow` output columns touch (reflection
    keeps the set of a run contiguous): what sizes the LDS window of irm_resize_taps."""
    lo, hi = indices.min(1), indices.max(1)
    starts = np.arange(0, len(lo), tow)
    return int((np.maximum.reduceat(hi, starts) - np.minimum.reduceat(lo, starts)).max()) + 1


def _taps_on(device, in_length: int, out_length: int, scale: float, kernel: str, antialias: bool) -> tuple:
    """The axis table on the device, cached like _resize_table_on: (fp32 weights, int32 indices, P, {tow: tile_span})."""
    def build():
        w, i = resize_taps(in_length, out_length, scale, kernel, antialias)
        return (torch.from_numpy(w.astype(np.float32)).contiguous().to(device),
                torch.from_numpy(i.astype(np.int32)).contiguous().to(device), w.shape[1],
                {tow: tile_span(i, tow) for tow in RESIZE_TOWS})
    return device_constant(("resize_taps", str(device), in_length, out_length, float(scale), kernel, bool(antialias)), build)


def _pick_tow(spans: dict, c: int) -> tuple:
    """(tow, ncol_max): the widest tile whose window of 8 x ncol_max x C floats fits RESIZE_WINDOW_PREFERRED, or, where
    none does (1/16 with lanczos3), the widest that fits RESIZE_WINDOW_BYTES."""
    for budget in (min(RESIZE_WINDOW_PREFERRED, RESIZE_WINDOW_BYTES), RESIZE_WINDOW_BYTES):
        for tow in RESIZE_TOWS:
            if 8 * spans[tow] * c * 4 <= budget:
                return tow, spans[tow]
    raise ValueError(f"resize: even {RESIZE_TOWS[-1]} output columns touch {spans[RESIZE_TOWS[-1]]} source columns, more "
                     f"than the {RESIZE_WINDOW_BYTES}-byte window holds; shrink in two steps")


def resize_device(frames, size=None, scale=None, kernel: str = "bicubic", antialias: bool = True, out: str = "same"):
    """resize_host on the GPU (irm_resize_taps): `frames` is one uint8 / uint16 (or int16 = uint16 bit pattern) or
    float32 HW / HWC GPU tensor, a [K][H][W][C] stack, or a list of frames of one shape; size / scale, kernel and
    antialias as resize_host takes them.  out="same": integer frames quantised to their dtype (clamp, x peak, round
    half to even), float32 frames float32 as computed; out="float": float32, unrounded and unclamped; out="unit":
    float32 clamped to [0, 1].  A float32 frame may also ask for out="uint8" / "uint16": the unit result under the same
    quantising rule (irm_unit_quantise; uint16 as its int16 bit pattern, as the tiler returns it).  The tap tables are
    cached per device; returns the same arrangement (tensor -> tensor, list -> list) without synchronising.  H pass
    first, then W pass, as basicsr does - not MATLAB's smaller-scale-first rule."""
    if out not in _OUT_KINDS and out not in ("uint8", "uint16"):
        raise ValueError(f"out must be 'same', 'float', 'unit' (or 'uint8' / 'uint16' for float32 frames), not {out!r}")
    as_list = isinstance(frames, (list, tuple))
    first = frames[0] if as_list and frames else frames
    is_f32 = isinstance(first, torch.Tensor) and first.dtype == torch.float32
    if isinstance(first, torch.Tensor) and (is_f32 or first.dtype in FRAME_DTYPES) and not first.is_cuda:
        raise ValueError("resize_device needs GPU tensors; there is no CPU fallback (resize_host takes host arrays)")
    items, k, h, w, c, stacked = device_frames(frames, "resize_device", "resize_host takes numpy arrays", float32=True)
    if out in ("uint8", "uint16") and not is_f32:
        raise ValueError(f"out={out!r} is for float32 frames; an integer frame keeps its type with out='same'")
    oh, ow, sh, sw = resize_plan(h, w, size, scale, kernel, antialias)
    taps = max(_tap_count(sh, kernel, antialias)[1], _tap_count(sw, kernel, antialias)[1])
    if taps > RESIZE_MAX_TAPS:
        raise ValueError(f"resize: {taps} taps per output value, more than the {RESIZE_MAX_TAPS} the kernel takes; "
                         "shrink in two steps")
    f0 = items[0]
    dev = f0.device
    with torch.cuda.device(dev):
        src = frame_bits(items, stacked)
        wh, ih, ph, _ = _taps_on(dev, h, oh, sh, kernel, antialias)
        ww, iw, pw, spans = _taps_on(dev, w, ow, sw, kernel, antialias)
        tow, ncol = _pick_tow(spans, c)
        to_int = out in ("uint8", "uint16")
        kind = 2 if to_int else 1 if (is_f32 and out == "same") else _OUT_KINDS[out]
        res = torch.empty((k, oh, ow, c), dtype=src.dtype if kind == 0 else torch.float32, device=dev)
        _hip.call("irm_resize_taps", _hip.ptr(src), 2 if is_f32 else int(f0.dtype != torch.uint8), _hip.ptr(res), kind,
                  _hip.ptr(wh), _hip.ptr(ih), _hip.ptr(ww), _hip.ptr(iw), k, h, w, c, oh, ow, ph, pw, tow, ncol)
        if to_int:
            q = torch.empty(res.shape, dtype=torch.uint8 if out == "uint8" else torch.int16, device=dev)
            _hip.call("irm_unit_quantise", _hip.ptr(res), _hip.ptr(q), int(out == "uint16"), res.numel())
            res = q
    if kind == 0 and f0.dtype == torch.uint16:
        res = res.view(torch.uint16)
    tail = (oh, ow) if (f0.dim() - int(stacked)) == 2 else (oh, ow, c)
    if stacked:
        return res.view((k,) + tail)
    return [r.view(tail) for r in res] if as_list else res[0].view(tail)


@dataclasses.dataclass(frozen=True)
class Resize:
    """A resize stage of run_model_chain, in place of a (model, patch_config) pair: exactly one of size=(oh, ow) and
    scale=s, a kernel of RESIZE_KERNELS and the antialiasing, as resize_device takes them."""
    size: tuple | None = None
    scale: float | None = None
    kernel: str = "bicubic"
    antialias: bool = True

    def __post_init__(self):
        if self.size is not None and not isinstance(self.size, tuple):
            try:
                object.__setattr__(self, "size", tuple(self.size))
            except TypeError:
                pass                                                          # resize_plan words the refusal
        resize_plan(1 << 20, 1 << 20, self.size, self.scale, self.kernel, self.antialias)

    def plan(self, h: int, w: int) -> tuple:
        """(oh, ow) of this stage on an h x w frame; ValueError where a side is shorter than its taps."""
        return resize_plan(h, w, self.size, self.scale, self.kernel, self.antialias)[:2]
