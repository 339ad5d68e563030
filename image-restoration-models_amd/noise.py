"""The noise level of a frame from its diagonal Haar detail band: Donoho's robust estimate
sigma = median(|HH|) / 0.6745 on the integer codes of a uint8 / uint16 frame or of the Y plane of a YUV 4:2:0 frame.
The GPU produces four integers per (frame, channel) (irm_noise_hh_stats); `noise_stats` is their exact numpy twin and
`noise_sigma_from_stats` turns them into a sigma on the 0..255 scale of every other `sigma` argument of this package.
The reference has no estimator: its benchmark adds the noise itself and so knows the level."""
from __future__ import annotations

import numpy as np
import torch

from . import _hip, yuv
from .frames import device_frames, frame_bits, frame_shape

#: the 0.75 quantile of the standard normal distribution: median(|x|) = MAD_SCALE sigma for x ~ N(0, sigma)
MAD_SCALE = 0.6744897501960817
#: 8-byte workspace words per (frame, channel) of irm_noise_hh_stats (include/irm_hip_noise.h)
_WS_WORDS = 4098


def _saturation(peak: int, sat, exclude_saturated: bool) -> tuple:
    """(sat_lo, sat_hi): a block is left out when its minimum is <= sat_lo or its maximum >= sat_hi."""
    if not exclude_saturated:
        return -1, 2 * peak + 1
    if sat is None:
        return 0, peak
    lo, hi = (int(v) for v in sat)
    if lo < -1 or hi <= lo:
        raise ValueError(f"sat is (sat_lo, sat_hi) with -1 <= sat_lo < sat_hi, not {sat!r}")
    return lo, hi


def _check_shift(shift, bits: int) -> int:
    if int(shift) != shift or not 0 <= shift < bits:
        raise ValueError(f"shift must be an integer in [0, {bits}), not {shift!r}")
    return int(shift)


def _check_size(h: int, w: int) -> None:
    if min(h, w) < 2:
        raise ValueError(f"frame {h}x{w}: both sides must be at least 2, one 2x2 block")


def noise_stats(img: np.ndarray, shift: int = 0, sat=None, exclude_saturated: bool = True) -> np.ndarray:
    """The numpy twin of irm_noise_hh_stats for one uint8 / uint16 [H, W] or [H, W, C] frame (C = 1 or 3): an int64
    [C, 4] array of (n, m, below, at) per channel.  With v = img >> shift, every non-overlapping 2 x 2 block (a trailing
    odd row or column is ignored) gives d = |a - b - c + e|; a block is left out when one of its samples is <= sat_lo or
    >= sat_hi (`sat`, default (0, peak of the dtype); exclude_saturated=False counts every block).  n is the number of
    counted blocks, m the lower median of their d (0-based index (n - 1) // 2), below and at the numbers of d < m and
    d == m; n == 0 gives (0, 0, 0, 0)."""
    if not isinstance(img, np.ndarray):
        raise ValueError("noise_stats takes a numpy array (noise_stats_device takes GPU tensors)")
    if img.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"noise_stats takes uint8 or uint16 frames, not {img.dtype}")
    h, w, c = frame_shape(img.shape, "noise_stats")
    _check_size(h, w)
    bits = 8 * img.dtype.itemsize
    shift = _check_shift(shift, bits)
    sat_lo, sat_hi = _saturation(2 ** bits - 1, sat, exclude_saturated)
    v = img.reshape(h, w, c)[:h // 2 * 2, :w // 2 * 2].astype(np.int64) >> shift
    a, b, cc, e = v[0::2, 0::2], v[0::2, 1::2], v[1::2, 0::2], v[1::2, 1::2]
    d = np.abs(a - b - cc + e)
    lo, hi = np.minimum(np.minimum(a, b), np.minimum(cc, e)), np.maximum(np.maximum(a, b), np.maximum(cc, e))
    keep = (lo > sat_lo) & (hi < sat_hi)
    out = np.zeros((c, 4), np.int64)
    for ch in range(c):
        vals = np.sort(d[..., ch][keep[..., ch]])
        n = vals.size
        if n:
            m = vals[(n - 1) // 2]
            out[ch] = n, m, np.count_nonzero(vals < m), np.count_nonzero(vals == m)
    return out


def noise_sigma_from_stats(stats, span) -> np.ndarray:
    """float64 [..., C] sigmas on the 0..255 scale from [..., C, 4] integers (n, m, below, at) of samples that span
    `span` codes (255, 65535, 1023 for full-range data, 219 << (bits - 8) for limited-range Y).  n == 0 gives NaN, m == 0
    gives 0.0; otherwise the grouped median m_g = m - 0.5 + (n / 2 - below) / at stands for the integer m (the d are
    integers: the median of the underlying continuous value is interpolated inside the bin of m) and
    sigma = m_g / 2 / 0.6744897501960817 * 255 / span - d has twice the noise's standard deviation."""
    s = np.asarray(stats.cpu() if isinstance(stats, torch.Tensor) else stats).astype(np.int64)
    if s.ndim < 1 or s.shape[-1] != 4:
        raise ValueError(f"stats is [..., 4] (n, m, below, at), not shape {s.shape}")
    if not (np.isfinite(span) and span > 0):
        raise ValueError(f"span must be positive and finite, not {span}")
    n, m, below, at = (s[..., i].astype(np.float64) for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        m_g = m - 0.5 + (n / 2 - below) / at
        sigma = m_g / 2 / MAD_SCALE * 255 / float(span)
    sigma = np.where(m == 0, 0.0, sigma)
    return np.where(n == 0, np.nan, sigma)


def _frame_sigma(channel_sigmas) -> float:
    """The mean of the finite channel sigmas, NaN if there is none."""
    s = np.asarray(channel_sigmas, np.float64)
    s = s[np.isfinite(s)]
    return float(s.mean()) if s.size else float("nan")


def estimate_noise_sigma(img: np.ndarray) -> float:
    """The noise sigma of a uint8 / uint16 frame on the 0..255 scale, on the host: the mean over the channels of
    noise_sigma_from_stats(noise_stats(img), peak).  NaN for a frame without an unsaturated block."""
    stats = noise_stats(img)
    return _frame_sigma(noise_sigma_from_stats(stats, 2 ** (8 * img.dtype.itemsize) - 1))


def _launch(bits, is_u16: bool, k, h, w, c, pitch, frame_stride, shift, sat_lo, sat_hi) -> torch.Tensor:
    dev = bits.device
    with torch.cuda.device(dev):
        ws = torch.empty(_WS_WORDS * k * c, dtype=torch.int64, device=dev)
        stats = torch.empty(k, c, 4, dtype=torch.int64, device=dev)
        _hip.call("irm_noise_hh_stats", _hip.ptr(bits), int(is_u16), k, h, w, c, pitch, frame_stride, shift, sat_lo,
                  sat_hi, _hip.ptr(stats), _hip.ptr(ws), ws.numel())
    return stats


def noise_stats_device(frames, shift: int = 0, sat=None, exclude_saturated: bool = True) -> torch.Tensor:
    """Device twin of noise_stats (irm_noise_hh_stats): one uint8 / uint16 HW or HWC (C = 1 or 3) GPU frame, or a list
    of K frames of one shape - uint16 frames as this package carries them on the device, uint16 or its int16 bit
    pattern.  One call of the entry point for all K frames; returns an int64 [K, C, 4] device tensor of
    (n, m, below, at) without synchronising with the host.  The integers are those of noise_stats, whatever K and on
    every call."""
    as_list = isinstance(frames, (list, tuple))
    for f in (frames if as_list else [frames]):
        if isinstance(f, np.ndarray):
            raise ValueError("noise_stats_device needs GPU tensors (noise_stats takes numpy arrays); there is no CPU "
                             "fallback")
        if isinstance(f, torch.Tensor) and f.dtype.is_floating_point:
            raise ValueError(f"noise_stats_device takes uint8 or uint16 frames, not {f.dtype}: a float frame has no "
                             "integer codes")
    items = list(frames) if as_list else [frames]
    items, k, h, w, c, _ = device_frames(items, "noise_stats_device", "noise_stats takes numpy arrays")
    _check_size(h, w)
    is_u16 = items[0].dtype != torch.uint8
    bits_n = 16 if is_u16 else 8
    shift = _check_shift(shift, bits_n)
    sat_lo, sat_hi = _saturation(2 ** bits_n - 1, sat, exclude_saturated)
    if not items[0].is_cuda:
        raise ValueError("noise_stats_device needs GPU tensors; there is no CPU fallback")
    bits = frame_bits(items)
    return _launch(bits, is_u16, k, h, w, c, w * c, h * w * c, shift, sat_lo, sat_hi)


def estimate_noise_sigma_device(frames):
    """The noise sigma of device frames on the 0..255 scale: a float for one frame, a list of floats for a list of
    frames.  noise_stats_device and one synchronising copy of its K x C x 4 integers - the only place that waits for the
    GPU; the float64 arithmetic is estimate_noise_sigma's, so the two agree exactly."""
    as_list = isinstance(frames, (list, tuple))
    stats = noise_stats_device(frames)
    first = frames[0] if as_list else frames
    peak = 255 if first.dtype == torch.uint8 else 65535
    sig = noise_sigma_from_stats(stats.cpu().numpy(), peak)           # the one host synchronisation
    vals = [_frame_sigma(s) for s in sig]
    return vals if as_list else vals[0]


def _yuv_span(fmt, full_range: bool) -> tuple:
    """(shift, sat_lo, sat_hi, span) of the Y plane of `fmt`."""
    depth = yuv.YUV_FORMATS[fmt][1]
    shift = yuv._shift(fmt)
    if full_range:
        peak = 2 ** depth - 1
        return shift, 0, peak, peak
    return shift, 16 << (depth - 8), 235 << (depth - 8), 219 << (depth - 8)


def estimate_noise_sigma_yuv(planes, fmt, full_range: bool = False) -> float:
    """The noise sigma of the Y plane of one YUV 4:2:0 frame, on the host: `planes` as yuv420_to_rgb_host takes them
    (the chroma planes are not looked at and may be left out).  The codes of a "p010" plane are its words shifted right by
    six; blocks that touch the ends of the range (16 and 235 << (bits - 8) for limited range, 0 and the peak for full
    range) are left out, and the result is scaled by 255 / span with span = 219 << (bits - 8) or the peak.

    This is the sigma of the Y plane itself.  Y is a weighted sum of R, G, B, so independent noise of equal sigma in the
    three channels reaches it as sqrt(sum w^2) times that sigma - 0.75 for BT.709, 0.67 for BT.601 - and that is what a
    luma_only model sees."""
    yuv._check_options(fmt, "bt709", "left")
    dtypes = (np.uint16,) if yuv.YUV_FORMATS[fmt][1] == 10 else (np.uint8,)
    h, w = yuv._check_planes(planes, fmt, True, np.ndarray, dtypes)
    _check_size(h, w)
    shift, sat_lo, sat_hi, span = _yuv_span(fmt, full_range)
    stats = noise_stats(np.ascontiguousarray(planes[0]), shift=shift, sat=(sat_lo, sat_hi))
    return _frame_sigma(noise_sigma_from_stats(stats, span))


def noise_stats_yuv_device(planes, fmt, full_range: bool = False) -> torch.Tensor:
    """int64 [1, 1, 4] device tensor of (n, m, below, at) of the Y plane of device planes, as yuv420_to_rgb_device takes
    them; a row-pitched plane is read in place.  Not synchronised."""
    yuv._check_options(fmt, "bt709", "left")
    h, w, y, _, _, _, pitch_y, _ = yuv._device_planes(planes, fmt, True)
    _check_size(h, w)
    if not y.is_cuda:
        raise ValueError("estimate_noise_sigma_yuv_device needs GPU tensors; there is no CPU fallback")
    shift, sat_lo, sat_hi, _ = _yuv_span(fmt, full_range)
    bits = y.view(torch.int16) if y.dtype == torch.uint16 else y
    return _launch(bits, fmt == "p010", 1, h, w, 1, int(pitch_y), (h - 1) * int(pitch_y) + w, shift, sat_lo, sat_hi)


def estimate_noise_sigma_yuv_device(planes, fmt, full_range: bool = False) -> float:
    """Device twin of estimate_noise_sigma_yuv: the Y plane of device planes (row-pitched views included), a float
    after one synchronising copy.  The same value as the host's, and the same reading: the sigma of the Y plane itself,
    sqrt(sum w^2) (0.75 for BT.709) times the sigma of independent RGB noise."""
    stats = noise_stats_yuv_device(planes, fmt, full_range)
    span = _yuv_span(fmt, full_range)[3]
    return _frame_sigma(noise_sigma_from_stats(stats.cpu().numpy(), span)[0])     # the one host synchronisation
