"""YUV video frames (DESIGN.md sections 16 and 23): planes to the float32 RGB frame in [0, 1] of the device pipeline and
back, on the GPU (irm_yuv_to_rgb_f32, irm_rgb_f32_to_yuv) and restated in numpy float32 on the host with the same
operation order, for the whole grid of YUV_LAYOUTS: 4:2:0, 4:2:2 and 4:4:4 at 8, 10 and 12 bit, planar and semi-planar.
The reference has no YUV path; tests/yuv_model.py and tests/yuv_formats_model.py state the arithmetic.  Their PSNR /
SSIM per component, on the host in float64 and on the GPU (irm_yuv_metrics, irm_yuv420_metrics).

The yuv420_* functions are the general ones behind a check of their three names, "i420", "nv12" and "p010"."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _hip
from .frames import psnr_from_error
from .metrics import psnr, ssim

#: format -> (sub_w, sub_h, planes, bit depth, upper_bits): chroma planes are [H / sub_h][W / sub_w]; 3 planes are
#: (y, u, v), 2 are (y, uv [CH][CW][2]); 8-bit samples are uint8, the others uint16 with the code in the low bits, or,
#: with upper_bits, stored as code << (16 - depth)
YUV_LAYOUTS = {
    "i420": (2, 2, 3, 8, 0), "nv12": (2, 2, 2, 8, 0), "i420p10": (2, 2, 3, 10, 0), "p010": (2, 2, 2, 10, 1),
    "i420p12": (2, 2, 3, 12, 0), "p012": (2, 2, 2, 12, 1),
    "i422": (2, 1, 3, 8, 0), "nv16": (2, 1, 2, 8, 0), "i422p10": (2, 1, 3, 10, 0), "p210": (2, 1, 2, 10, 1),
    "i422p12": (2, 1, 3, 12, 0), "p212": (2, 1, 2, 12, 1),
    "i444": (1, 1, 3, 8, 0), "nv24": (1, 1, 2, 8, 0), "i444p10": (1, 1, 3, 10, 0), "p410": (1, 1, 2, 10, 1),
    "i444p12": (1, 1, 3, 12, 0), "p412": (1, 1, 2, 12, 1),
}
#: the three names of the yuv420_* functions -> (planes, bit depth)
YUV_FORMATS = {fmt: YUV_LAYOUTS[fmt][2:4] for fmt in ("i420", "nv12", "p010")}
_SAMPLING = {(2, 2): "4:2:0", (2, 1): "4:2:2", (1, 1): "4:4:4"}
#: matrix -> (Kr, Kb)
YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
YUV_SITINGS = ("left", "center")


def _check_options(fmt, matrix, siting) -> None:
    if fmt not in YUV_FORMATS:
        raise ValueError(f"fmt must be one of {sorted(YUV_FORMATS)}, not {fmt!r}")
    if matrix not in YUV_MATRICES:
        raise ValueError(f"matrix must be one of {sorted(YUV_MATRICES)}, not {matrix!r}")
    if siting not in YUV_SITINGS:
        raise ValueError(f"siting must be 'left' or 'center', not {siting!r}")


def _check_layout_options(fmt, matrix, siting) -> None:
    """_check_options over the whole grid of YUV_LAYOUTS."""
    if fmt not in YUV_LAYOUTS:
        raise ValueError(f"fmt must be one of {sorted(YUV_LAYOUTS)}, not {fmt!r}")
    _check_options("i420", matrix, siting)


def plane_shapes(h: int, w: int, fmt, luma_only: bool = False) -> list:
    """The plane shapes of an h x w frame in `fmt`: Y, then U and V or the interleaved UV; Y alone with luma_only."""
    sw, sh, n = YUV_LAYOUTS[fmt][:3]
    chroma = [(h // sh, w // sw)] * 2 if n == 3 else [(h // sh, w // sw, 2)]
    return [(h, w)] + ([] if luma_only else chroma)


def _np_dtype(fmt):
    return np.uint8 if YUV_LAYOUTS[fmt][3] == 8 else np.uint16


def _shift(fmt) -> int:
    """A stored word is its code shifted left by this."""
    _, _, _, depth, upper = YUV_LAYOUTS[fmt]
    return 16 - depth if upper else 0


def _check_size(h: int, w: int, fmt) -> None:
    sw, sh = YUV_LAYOUTS[fmt][:2]
    if h <= 0 or w <= 0 or h % sh or w % sw:
        need = {(2, 2): "even, positive H and W", (2, 1): "an even W and positive H, W",
                (1, 1): "positive H and W"}[sw, sh]
        raise ValueError(f"{_SAMPLING[sw, sh]} frames have {need}, not {h} x {w}")


def _check_planes(planes, fmt, luma_only: bool, kind, dtypes) -> tuple:
    """(H, W) of the planes of one frame: their number, type (`kind`: np.ndarray or torch.Tensor), dtype and shapes.
    With luma_only the chroma planes are not looked at and may be missing."""
    sw, sh, n = YUV_LAYOUTS[fmt][:3]
    what = "(y, u, v)" if n == 3 else "(y, uv)"
    if not isinstance(planes, (tuple, list)) or not (len(planes) == n or (luma_only and len(planes) == 1)):
        raise ValueError(f"{fmt!r} planes are {what}, not {type(planes).__name__}"
                         + (f" of {len(planes)}" if isinstance(planes, (tuple, list)) else ""))
    used = planes[:1] if luma_only else planes
    for p in used:
        if not isinstance(p, kind):
            raise ValueError(f"{fmt!r} planes must be {kind.__name__}s, not {type(p).__name__}")
        if p.dtype not in dtypes:
            raise ValueError(f"{fmt!r} planes are {' or '.join(str(d) for d in dtypes)}, not {p.dtype}")
    if len(planes[0].shape) != 2:
        raise ValueError(f"the Y plane is [H][W], not shape {tuple(planes[0].shape)}")
    h, w = (int(s) for s in planes[0].shape)
    _check_size(h, w, fmt)
    want = (h // sh, w // sw) if n == 3 else (h // sh, w // sw, 2)
    for p in used[1:]:
        if tuple(p.shape) != want:
            raise ValueError(f"a chroma plane of a {h} x {w} {fmt!r} frame is {list(want)}, not {list(p.shape)}")
    return h, w


def _check_rgb(rgb, luma_only: bool, kind, fmt="i420") -> tuple:
    c = 1 if luma_only else 3
    if not isinstance(rgb, kind) or len(rgb.shape) != 3 or rgb.shape[2] != c or str(rgb.dtype).split(".")[-1] != "float32":
        raise ValueError(f"the frame is a float32 [H][W][{c}] {kind.__name__}" + (" with luma_only" if luma_only else ""))
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    _check_size(h, w, fmt)
    return h, w


def _constants(matrix, full_range, depth) -> dict:
    """The float32 constants of both directions: the float32 roundings of the float64 expressions."""
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    s, top = float(2 ** (depth - 8)), float(2 ** depth - 1)
    f = np.float32
    return dict(y0=f(0.0 if full_range else 16.0 * s), yr=f(top if full_range else 219.0 * s), c0=f(128.0 * s),
                cr=f(top if full_range else 224.0 * s), kr=f(kr), kg=f(kg), kb=f(kb), r_cr=f(2.0 * (1.0 - kr)),
                b_cb=f(2.0 * (1.0 - kb)), g_cb=f(2.0 * kb * (1.0 - kb) / kg), g_cr=f(2.0 * kr * (1.0 - kr) / kg),
                top=f(top))


# ---------------------------------------------------------------------------
# the numpy float32 twins

def _split_planes(planes, fmt, luma_only):
    """Integer codes (y, u, v) as int64 arrays; u, v None with luma_only."""
    shift = _shift(fmt)
    y = planes[0].astype(np.int64) >> shift
    if luma_only:
        return y, None, None
    if YUV_LAYOUTS[fmt][2] == 3:
        return y, planes[1].astype(np.int64) >> shift, planes[2].astype(np.int64) >> shift
    return y, planes[1][:, :, 0].astype(np.int64) >> shift, planes[1][:, :, 1].astype(np.int64) >> shift


def _upsample16_of(c: np.ndarray, fmt, siting: str) -> np.ndarray:
    """Sixteen times the linearly up-sampled chroma codes of a `fmt` frame, [H / sub_h][W / sub_w] -> [H][W], edges
    clamped, in two integer stages of a factor four each: down the columns if sub_h == 2, along the rows if sub_w == 2."""
    sub_w, sub_h = YUV_LAYOUTS[fmt][:2]
    t = 4 * c
    if sub_h == 2:
        p = np.pad(c, ((1, 1), (0, 0)), mode="edge")
        t = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
        t[0::2] = 3 * p[1:-1] + p[:-2]                  # a quarter above the sample
        t[1::2] = 3 * p[1:-1] + p[2:]                   # a quarter below
    if sub_w == 1:
        return 4 * t
    p = np.pad(t, ((0, 0), (1, 1)), mode="edge")
    left, mid, right = p[:, :-2], p[:, 1:-1], p[:, 2:]
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int64)
    if siting == "center":
        out[:, 0::2] = 3 * mid + left
        out[:, 1::2] = 3 * mid + right
    else:
        out[:, 0::2] = 4 * mid                          # on the sample
        out[:, 1::2] = 2 * mid + 2 * right              # midway between two
    return out


def yuv420_to_rgb_host(planes, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False) -> np.ndarray:
    """The planes of one 4:2:0 frame -> float32 [H][W][3] RGB in [0, 1] ([H][W][1], the luma, with luma_only): the
    numpy twin of yuv420_to_rgb_device, bit for bit.  `planes` is (y, u, v) for "i420" and (y, uv) for "nv12" /
    "p010" (uint16, the code in the upper ten bits)."""
    _check_options(fmt, matrix, siting)
    return yuv_to_rgb_host(planes, fmt, matrix, full_range, siting, luma_only)


def yuv_to_rgb_host(planes, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False) -> np.ndarray:
    """yuv420_to_rgb_host for every format of YUV_LAYOUTS: the numpy twin of yuv_to_rgb_device, bit for bit.  4:2:2
    chroma is up-sampled along the row alone, 4:4:4 chroma not at all (`siting` is then checked and ignored)."""
    _check_layout_options(fmt, matrix, siting)
    depth = YUV_LAYOUTS[fmt][3]
    _check_planes(planes, fmt, luma_only, np.ndarray, (_np_dtype(fmt),))
    k = _constants(matrix, full_range, depth)
    f = np.float32
    y, u, v = _split_planes(planes, fmt, luma_only)
    yp = (y.astype(f) - k["y0"]) / k["yr"]
    if luma_only:
        return np.clip(yp, f(0), f(1))[:, :, None]
    cb = (_upsample16_of(u, fmt, siting).astype(f) * f(0.0625) - k["c0"]) / k["cr"]
    cr = (_upsample16_of(v, fmt, siting).astype(f) * f(0.0625) - k["c0"]) / k["cr"]
    rgb = np.empty(y.shape + (3,), f)
    rgb[:, :, 0] = yp + k["r_cr"] * cr
    rgb[:, :, 1] = (yp - k["g_cb"] * cb) - k["g_cr"] * cr
    rgb[:, :, 2] = yp + k["b_cb"] * cb
    return np.clip(rgb, f(0), f(1), out=rgb)


def _filter_chroma(c: np.ndarray, siting: str) -> np.ndarray:
    """Per-pixel chroma [H][W] -> [H/2][W/2] at the chroma site; the order of the additions is the kernel's."""
    f = np.float32
    if siting == "center":
        return ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * f(0.25)
    m, r = c[:, 0::2], c[:, 1::2]
    left = np.concatenate([m[:, :1], r[:, :-1]], axis=1)            # the column before the even one, clamped
    h = ((left + (m + m)) + r) * f(0.25)
    return (h[0::2] + h[1::2]) * f(0.5)


def _filter_chroma_row(c: np.ndarray, siting: str) -> np.ndarray:
    """Per-pixel chroma [H][W] -> [H][W/2] (4:2:2): the row filter of _filter_chroma without the vertical mean."""
    f = np.float32
    m, r = c[:, 0::2], c[:, 1::2]
    if siting == "center":
        return (m + r) * f(0.5)
    left = np.concatenate([m[:, :1], r[:, :-1]], axis=1)
    return ((left + (m + m)) + r) * f(0.25)


def _filter_chroma_of(c: np.ndarray, fmt, siting: str) -> np.ndarray:
    sub = YUV_LAYOUTS[fmt][:2]
    return _filter_chroma(c, siting) if sub == (2, 2) else _filter_chroma_row(c, siting) if sub == (2, 1) else c


def _codes(off, rng, v, top) -> np.ndarray:
    return np.rint(np.clip(off + rng * v, np.float32(0), top)).astype(np.int64)


def _out_planes(out, luma_only: bool, h: int, w: int, fmt, empty) -> tuple:
    """The planes an rgb_to_yuv_* call writes: `out`, required with luma_only, or new ones from empty(shape)."""
    if out is None and luma_only:
        raise ValueError("luma_only writes the Y plane alone: pass the frame's planes as out, their chroma is kept")
    return tuple(empty(s) for s in plane_shapes(h, w, fmt)) if out is None else out


def rgb_to_yuv420_host(rgb, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, out=None) -> tuple:
    """float32 [H][W][3] RGB -> the planes of a 4:2:0 frame in `fmt`, the numpy twin of rgb_to_yuv420_device, bit for
    bit; values outside [0, 1] are legal (the codes are clipped).  With luma_only the frame is [H][W][1] and only Y is
    made: `out`, the planes of the frame it belongs to, is required, its Y plane is overwritten and its chroma planes
    come back as they are.  Without luma_only `out` is optional (planes to write into)."""
    _check_options(fmt, matrix, siting)
    return rgb_to_yuv_host(rgb, fmt, matrix, full_range, siting, luma_only, out)


def rgb_to_yuv_host(rgb, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, out=None) -> tuple:
    """rgb_to_yuv420_host for every format of YUV_LAYOUTS: the numpy twin of rgb_to_yuv_device, bit for bit.  4:2:2
    chroma is filtered along the row alone, 4:4:4 chroma not at all."""
    _check_layout_options(fmt, matrix, siting)
    n, depth = YUV_LAYOUTS[fmt][2:4]
    h, w = _check_rgb(rgb, luma_only, np.ndarray, fmt)
    dt = _np_dtype(fmt)
    out = _out_planes(out, luma_only, h, w, fmt, lambda s: np.empty(s, dt))
    if _check_planes(out, fmt, False, np.ndarray, (dt,)) != (h, w):
        raise ValueError(f"out holds the planes of another frame size than {h} x {w}")
    k = _constants(matrix, full_range, depth)
    shift = _shift(fmt)
    if luma_only:
        out[0][...] = _codes(k["y0"], k["yr"], rgb[:, :, 0], k["top"]) << shift
        return tuple(out)
    r, g, b = rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]
    yp = (k["kr"] * r + k["kg"] * g) + k["kb"] * b
    cb = _filter_chroma_of((b - yp) / k["b_cb"], fmt, siting)
    cr = _filter_chroma_of((r - yp) / k["r_cr"], fmt, siting)
    out[0][...] = _codes(k["y0"], k["yr"], yp, k["top"]) << shift
    u, v = (out[1], out[2]) if n == 3 else (out[1][:, :, 0], out[1][:, :, 1])
    u[...] = _codes(k["c0"], k["cr"], cb, k["top"]) << shift
    v[...] = _codes(k["c0"], k["cr"], cr, k["top"]) << shift
    return tuple(out)


# ---------------------------------------------------------------------------
# the device calls

def _device_planes(planes, fmt, luma_only) -> tuple:
    """The checks of device planes that need no GPU call and the operands the kernels take: (h, w, y, u, v, step,
    pitch_y, pitch_c) with u, v views of the chroma plane(s), None with luma_only."""
    sw, _, n, depth, _ = YUV_LAYOUTS[fmt]
    dtypes = (torch.uint8,) if depth == 8 else (torch.uint16, torch.int16)
    h, w = _check_planes(planes, fmt, luma_only, torch.Tensor, dtypes)
    used = planes[:1] if luma_only else planes
    if any(p.device != planes[0].device or p.dtype != planes[0].dtype for p in used):
        raise ValueError("the planes of one frame must share device and dtype")
    y = planes[0]
    if y.stride(1) != 1 or y.stride(0) < w:
        raise ValueError(f"the Y plane needs unit stride inside a row and a row stride of at least {w}, not {y.stride()}")
    if luma_only:
        return h, w, y, None, None, 1, y.stride(0), 0
    if n == 3:
        for p in planes[1:]:
            if p.stride(1) != 1 or p.stride(0) < w // sw:
                raise ValueError(f"a planar chroma plane needs unit stride inside a row and a row stride of at least "
                                 f"{w // sw}, not {p.stride()}")
        if planes[1].stride(0) != planes[2].stride(0):
            raise ValueError("the U and the V plane must share their row stride")
        return h, w, y, planes[1], planes[2], 1, y.stride(0), planes[1].stride(0)
    uv = planes[1]
    if uv.stride(2) != 1 or uv.stride(1) != 2 or uv.stride(0) < 2 * (w // sw):
        raise ValueError(f"the UV plane needs strides (row >= {2 * (w // sw)}, 2, 1), not {uv.stride()}")
    return h, w, y, uv[:, :, 0], uv[:, :, 1], 2, y.stride(0), uv.stride(0)


def _kernel_options(fmt, matrix, full_range, siting, luma_only) -> tuple:
    depth, upper = YUV_LAYOUTS[fmt][3:]
    return (depth, upper, int(matrix == "bt709"), int(bool(full_range)), int(siting == "center"), int(bool(luma_only)))


def yuv420_to_rgb_device(planes, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False) -> torch.Tensor:
    """Device planes of one 4:2:0 frame -> a contiguous float32 [H][W][3] RGB frame in [0, 1] on the same device
    ([H][W][1], the luma, with luma_only; the chroma planes are then not read and may be left out).  `planes` is
    (y, u, v) for "i420" and (y, uv) for "nv12" / "p010": uint8 tensors, for "p010" uint16 or its int16 bit pattern.
    They may be row-pitched views: unit stride inside a row (2 inside UV), any row stride of at least the width.
    Enqueued on the current stream; ValueError before any GPU call for everything else."""
    _check_options(fmt, matrix, siting)
    return yuv_to_rgb_device(planes, fmt, matrix, full_range, siting, luma_only)


def yuv_to_rgb_device(planes, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False) -> torch.Tensor:
    """yuv420_to_rgb_device for every format of YUV_LAYOUTS (irm_yuv_to_rgb_f32): 8-bit planes are uint8 tensors, all
    others uint16 or its int16 bit pattern; chroma planes are [H / sub_h][W / sub_w] (a UV plane [..][..][2]) and may
    be row-pitched views like the Y plane."""
    _check_layout_options(fmt, matrix, siting)
    h, w, y, u, v, step, pitch_y, pitch_c = _device_planes(planes, fmt, luma_only)
    rgb = torch.empty(h, w, 1 if luma_only else 3, dtype=torch.float32, device=y.device)
    _hip.call("irm_yuv_to_rgb_f32", _hip.ptr(y), _hip.ptr(u), _hip.ptr(v), step, pitch_y, pitch_c, *YUV_LAYOUTS[fmt][:2],
              *_kernel_options(fmt, matrix, full_range, siting, luma_only), h, w, _hip.ptr(rgb))
    return rgb


def rgb_to_yuv420_device(rgb, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, out=None) -> tuple:
    """A float32 [H][W][3] device frame -> the planes of a 4:2:0 frame in `fmt` on the same device: contiguous new
    tensors (uint8; for "p010" the uint16 bit pattern in int16 tensors), or `out`, planes as yuv420_to_rgb_device
    takes them (row-pitched views included: nothing outside [H][W] of a plane is written).  Values outside [0, 1] are
    legal.  With luma_only the frame is [H][W][1] and only the Y plane of `out` - required - is written; its chroma
    planes come back as they are."""
    _check_options(fmt, matrix, siting)
    return rgb_to_yuv_device(rgb, fmt, matrix, full_range, siting, luma_only, out)


def rgb_to_yuv_device(rgb, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, out=None) -> tuple:
    """rgb_to_yuv420_device for every format of YUV_LAYOUTS (irm_rgb_f32_to_yuv): new planes are uint8 tensors at
    8 bit and the uint16 bit pattern in int16 tensors otherwise."""
    _check_layout_options(fmt, matrix, siting)
    depth = YUV_LAYOUTS[fmt][3]
    h, w = _check_rgb(rgb, luma_only, torch.Tensor, fmt)
    dt = torch.uint8 if depth == 8 else torch.int16
    out = _out_planes(out, luma_only, h, w, fmt, lambda s: torch.empty(s, dtype=dt, device=rgb.device))
    oh, ow, y, u, v, step, pitch_y, pitch_c = _device_planes(out, fmt, luma_only)
    if (oh, ow) != (h, w) or y.device != rgb.device:
        raise ValueError(f"out holds the planes of another device or frame size than {h} x {w}")
    rgb = rgb.contiguous()
    _hip.call("irm_rgb_f32_to_yuv", _hip.ptr(rgb), _hip.ptr(y), _hip.ptr(u), _hip.ptr(v), step, pitch_y, pitch_c,
              *YUV_LAYOUTS[fmt][:2], *_kernel_options(fmt, matrix, full_range, siting, luma_only), h, w)
    return tuple(out)


# ---------------------------------------------------------------------------
# PSNR / SSIM per component (DESIGN.md sections 20 and 23): on the integer codes of Y (H x W) and of U and V
# (H / sub_h x W / sub_w), with skimage's SSIM defaults and data_range 255 (8 bit), 1023 (10 bit) or 4095 (12 bit).  The
# code of an upper-bits format is its word shifted right by 16 - depth (P010: six).

class YuvMetrics(NamedTuple):
    """Python floats; with luma_only the four chroma fields are NaN."""
    psnr_y: float
    ssim_y: float
    psnr_u: float
    ssim_u: float
    psnr_v: float
    ssim_v: float


def _check_metric_size(h: int, w: int, luma_only: bool, fmt="i420") -> None:
    sw, sh = YUV_LAYOUTS[fmt][:2]
    if (sw, sh) == (2, 2):
        least = 8 if luma_only else 14
        if min(h, w) < least:
            raise ValueError(f"frame {h} x {w}: both sides must be at least {least}"
                             + (", the 7 x 7 SSIM window" if luma_only else ", so that a chroma plane holds one 7 x 7 SSIM window"))
    elif h < 7 or w < (7 if luma_only else 7 * sw):
        raise ValueError(f"frame {h} x {w}: a {_SAMPLING[sw, sh]} frame must be at least 7 x {7 if luma_only else 7 * sw}"
                         + (", the 7 x 7 SSIM window" if luma_only else ", so that a chroma plane holds one 7 x 7 SSIM window"))


def _metric_tiles(h: int, w: int) -> int:
    """Output tiles of an h x w plane in irm_yuv420_metrics (csrc/metrics_video.hip): 16 rows x 192 values each."""
    return -(-(h - 6) // 16) * -(-(w - 6) // 192)


def _peak(fmt) -> int:
    return 2 ** YUV_LAYOUTS[fmt][3] - 1


def calculate_metrics_yuv(pred_planes, target_planes, fmt, luma_only=False) -> YuvMetrics:
    """PSNR and SSIM of the planes of one frame (any format of YUV_LAYOUTS) against the target's, per component:
    metrics.psnr / metrics.ssim in float64 on the integer codes.  The numpy twin of calculate_metrics_yuv_device;
    `planes` as yuv_to_rgb_host takes them."""
    _check_layout_options(fmt, "bt709", "left")
    dtypes = (_np_dtype(fmt),)
    size = _check_planes(pred_planes, fmt, luma_only, np.ndarray, dtypes)
    if _check_planes(target_planes, fmt, luma_only, np.ndarray, dtypes) != size:
        raise ValueError(f"the target holds the planes of another frame size than {size[0]} x {size[1]}")
    _check_metric_size(*size, luma_only, fmt)
    peak = _peak(fmt)
    vals = []
    for p, t in zip(_split_planes(pred_planes, fmt, luma_only), _split_planes(target_planes, fmt, luma_only)):
        vals += [float("nan")] * 2 if p is None else [psnr(t, p, peak), ssim(t, p, peak)]
    return YuvMetrics(*vals)


def frame_metrics_yuv_device(pred_planes, target_planes, fmt, luma_only=False) -> tuple:
    """Device squared errors and SSIMs of the planes of one frame (any format of YUV_LAYOUTS) against the target's
    (irm_yuv420_metrics for the three names of YUV_FORMATS, irm_yuv_metrics for the others):
    (sse [3] int64, exact; ssim [3] float64) for Y, U, V as device tensors, without synchronising.  The planes are as
    yuv420_to_rgb_device takes them: row-pitched views and the int16 bit pattern of "p010" included, and the two sides
    may be pitched differently.  With luma_only the chroma planes are not read; entries 1 and 2 are then 0 and NaN."""
    _check_layout_options(fmt, "bt709", "left")
    h, w, y, u, v, step, pitch_y, pitch_c = _device_planes(pred_planes, fmt, luma_only)
    th, tw, ty, tu, tv, tstep, tpitch_y, tpitch_c = _device_planes(target_planes, fmt, luma_only)
    if (th, tw) != (h, w) or ty.device != y.device:
        raise ValueError(f"the target holds the planes of another device or frame size than {h} x {w}")
    _check_metric_size(h, w, luma_only, fmt)
    if not y.is_cuda:
        raise ValueError("device metrics need GPU tensors; there is no CPU fallback")
    dev = y.device
    sw, sh, _, depth, upper = YUV_LAYOUTS[fmt]
    words = 2 * (_metric_tiles(h, w) + (0 if luma_only else 2 * _metric_tiles(h // sh, w // sw)))
    with torch.cuda.device(dev):
        ws = torch.empty(words, dtype=torch.float64, device=dev)
        if luma_only:
            sse = torch.zeros(3, dtype=torch.int64, device=dev)
            ssim_dev = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
        else:
            sse = torch.empty(3, dtype=torch.int64, device=dev)
            ssim_dev = torch.empty(3, dtype=torch.float64, device=dev)
        sides = (_hip.ptr(y), _hip.ptr(u), _hip.ptr(v), step, pitch_y, pitch_c,
                 _hip.ptr(ty), _hip.ptr(tu), _hip.ptr(tv), tstep, tpitch_y, tpitch_c)
        rest = (int(bool(luma_only)), h, w, _hip.ptr(sse), _hip.ptr(ssim_dev), _hip.ptr(ws), ws.numel())
        if fmt in YUV_FORMATS:
            _hip.call("irm_yuv420_metrics", *sides, depth, upper, *rest)
        else:
            _hip.call("irm_yuv_metrics", *sides, sw, sh, depth, upper, *rest)
    return sse, ssim_dev


def calculate_metrics_yuv_device(pred_planes, target_planes, fmt, luma_only=False) -> YuvMetrics:
    """Device twin of calculate_metrics_yuv: a YuvMetrics of Python floats after one synchronising copy.  PSNR is inf
    for identical planes."""
    sse, ssim_dev = frame_metrics_yuv_device(pred_planes, target_planes, fmt, luma_only)
    h, w = (int(s) for s in pred_planes[0].shape)
    host = torch.stack([sse, ssim_dev.view(torch.int64)]).cpu()       # the one host synchronisation
    ssim_v = host[1].view(torch.float64)
    vals = []
    sw, sh = YUV_LAYOUTS[fmt][:2]
    for i, n in enumerate((h * w, (h // sh) * (w // sw), (h // sh) * (w // sw))):
        if luma_only and i:
            vals += [float("nan")] * 2
        else:
            vals += [psnr_from_error(_peak(fmt), int(host[0, i]) / n), float(ssim_v[i])]
    return YuvMetrics(*vals)
