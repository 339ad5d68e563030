"""Aligned scoring of beam-splitter pairs (RealBlur_J / RealBlur_R): the protocol of the evaluation script published
with the dataset, which every RealBlur table in the literature uses - one gain, a homography by the ECC iteration, a
bicubic warp of the prediction onto the target, PSNR and Gaussian-window SSIM under the validity mask of that warp.
`calculate_metrics_aligned` is the float64 numpy statement of the contract below (the host twin and the yardstick),
the *_device functions run it on the GPU (irm_align_prepare, irm_ecc_iterate, irm_aligned_metrics of csrc/align.hip).

The contract is this package's own: cv2 and skimage are absent, parity with them is UNPINNED (as for metrics.ssim).  It
follows the published script and OpenCV's documented algorithm (findTransformECC with MOTION_HOMOGRAPHY, Gaussian filter
size 5, exactly `iterations` rounds, epsilon 0; warpPerspective, bicubic) with two deliberate deviations, (D1) and (D2).
Inputs are a prediction z8 and a target x8, uint8 or uint16 [H, W, 3] of one shape, both sides at least 11;
z = z8 / peak, x = x8 / peak.

1. Gain.  g = sum(x z) / sum(z z) over all samples, taken as sum(x8 z8) / sum(z8 z8): sums of integers in float64,
   exact below 2^53.  sum(z z) == 0: failed.  zs = g z.
2. Grey.  (0.299 R + 0.587 G) + 0.114 B of x (the template T) and of zs (the image I).
3. Pre-filter.  Both planes through the separable 5-tap Gaussian, sigma 0.3 ((5 - 1) / 2 - 1) + 0.8 = 1.1, taps
   normalised to 1, along x first and then along y, borders reflected without repeating the edge sample (dcb|abcd|cba),
   rounded to float32.  Gx, Gy = 0.5 (I[x + 1] - I[x - 1]) along each axis of the float32 I, same border, float32.
4. Iteration, exactly `iterations` times.  The map M is 3 x 3 float64 (D2: OpenCV's is float32), starts as the identity,
   M[2][2] stays 1.  For every target pixel (x, y): den = (M20 x + M21 y) + 1, position
   (px, py) = ((M00 x + M01 y) + M02, (M10 x + M11 y) + M12) / den.  I, Gx, Gy are sampled there bilinearly at the
   EXACT position (D1: OpenCV samples on a 1/32-pixel grid, which turns the iteration into a limit cycle; DESIGN.md
   section 24 has the evidence); taps outside the frame read 0.  The mask m is 1 where the position rounded to nearest
   lies inside the frame.  Under the mask: zero-mean I and T, their norms, the correlation rho; with a = Gx / den,
   b = Gy / den, t = -(px a + py b) the Jacobian row [a x, b x, t x, a y, b y, t y, a, b]; the Hessian J^T J, the
   projections, lambda = lambda_n / lambda_d and dp = H^-1 J^T (lambda T_zm - I_zm) (Evangelidis & Psarakis, forward
   additive ECC); dp is added to M00, M10, M20, M01, M11, M21, M02, M12 in that order.  All of it from ONE pass: the 66
   sums n, sum I, sum T, sum I^2, sum T^2, sum I T, the upper triangle of J^T J and J^T I, J^T T, J^T 1 - the zero-mean
   quantities follow algebraically (`ecc_update`).  lambda_d <= 0, an empty mask or a Hessian that is not positive
   definite (Cholesky): failed, the map stays as it was.  rho is the correlation at the map before the last update.
5. Final warp.  One pass, quantised like OpenCV's remap: position as above (float64, no contraction), cr = 1 where
   the unquantised position rounded to nearest (half to even) lies inside the frame; q = rint(32 position), integer
   part q >> 5, phase q & 31; each channel of zs sampled with the 4 x 4 bicubic kernel, A = -0.75, weights from a
   32-phase table (three taps by interpolateCubic's formulas, the fourth 1 - c0 - c1 - c2), along x first, borders
   reflected with the edge sample repeated (cba|abcd|dcb).  zr = sample cr, xr = x cr.  Identical frames give a map equal
   to the identity, every phase 0 and zr == x exactly.
6. Scores.  coverage = sum(cr) / (H W), 0: failed.  PSNR = 10 log10(1 / (sum((xr - zr)^2) / (3 sum(cr)))), inf for no
   error.  SSIM per channel: the map of (xr, zr) with the 11-tap Gaussian of sigma 1.5 over the valid region (the
   script's reflected border is cropped by 5, so only the valid region counts; the window of metrics_basicsr.hip),
   data_range 1, population covariance, K1 = 0.01, K2 = 0.03; the map times cr, summed, over the sum of cr on that
   region; the channel mean.

Out of the contract: other motion models, input masks, pyramids, grey or float32 frames."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _hip
from .frames import FRAME_DTYPES, frame_bits

#: the accumulate tile of irm_ecc_iterate, the chunk of the gain sums and the output tile of irm_aligned_metrics
_ECC_TILE_H, _ECC_TILE_W, _GAIN_CHUNK, _METRIC_TILE_H, _METRIC_TILE_W = 16, 64, 4096, 16, 32
N_SUMS = 66
_IU = [(i, j) for i in range(8) for j in range(i, 8)]


class AlignedMetrics(NamedTuple):
    psnr: float
    ssim: float
    rho: float
    coverage: float
    gain: float
    ok: bool
    map: np.ndarray          # [3, 3] float64


def _taps(n: int, sigma: float) -> list:
    """Normalised Gaussian taps; math.exp is the C library's exp, the one the launcher calls."""
    c = (n - 1) // 2
    g = [math.exp(-float((i - c) * (i - c)) / (2.0 * sigma * sigma)) for i in range(n)]
    s = 0.0
    for v in g:
        s += v
    return [v / s for v in g]


def _cubic_table() -> np.ndarray:
    a = -0.75
    tab = np.empty((32, 4))
    for i in range(32):
        x = i / 32.0
        x1, x2 = x + 1.0, 1.0 - x
        tab[i, 0] = ((a * x1 - 5.0 * a) * x1 + 8.0 * a) * x1 - 4.0 * a
        tab[i, 1] = (((a + 2.0) * x - (a + 3.0)) * x) * x + 1.0
        tab[i, 2] = (((a + 2.0) * x2 - (a + 3.0)) * x2) * x2 + 1.0
        tab[i, 3] = ((1.0 - tab[i, 0]) - tab[i, 1]) - tab[i, 2]
    return tab


def _check_host_pair(pred, target, what: str) -> float:
    if not isinstance(pred, np.ndarray) or not isinstance(target, np.ndarray):
        raise ValueError(f"{what} takes numpy arrays (the *_device functions take GPU tensors)")
    if pred.shape != target.shape or pred.dtype != target.dtype:
        raise ValueError(f"prediction {pred.shape} {pred.dtype} and target {target.shape} {target.dtype} differ")
    if pred.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"{what} takes uint8 or uint16 frames, not {pred.dtype}")
    _check_shape(pred.shape, what)
    return 255.0 if pred.dtype == np.uint8 else 65535.0


def _check_shape(shape, what: str) -> tuple:
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"{what} takes HWC frames with 3 channels, not shape {tuple(shape)}")
    if min(shape[0], shape[1]) < 11:
        raise ValueError(f"frame {shape[0]}x{shape[1]}: both sides must be at least 11, the SSIM window")
    if shape[0] * shape[1] * 3 > 0x7fffffff:
        raise ValueError(f"frame {shape[0]}x{shape[1]} is too large")
    return int(shape[0]), int(shape[1])


def _check_iterations(iterations) -> int:
    if int(iterations) != iterations or not 1 <= iterations <= 10000:
        raise ValueError(f"iterations must be an integer in 1 .. 10000, not {iterations!r}")
    return int(iterations)


# --------------------------------------------------------------------------- the statement, steps 1 to 3
def gain_of(pred: np.ndarray, target: np.ndarray):
    """(g, ok): step 1."""
    z, x = pred.astype(np.float64), target.astype(np.float64)
    szz = float((z * z).sum())
    if not szz > 0.0:
        return 0.0, False
    return float((x * z).sum()) / szz, True


def _blur5(a: np.ndarray) -> np.ndarray:
    g = _taps(5, 1.1)
    h, w = a.shape
    p = np.pad(a, ((0, 0), (2, 2)), mode="reflect")
    r = 0.0
    for d in range(5):
        r = r + g[d] * p[:, d:d + w]
    p = np.pad(r, ((2, 2), (0, 0)), mode="reflect")
    r = 0.0
    for d in range(5):
        r = r + g[d] * p[d:d + h]
    return r


def planes_of(pred: np.ndarray, target: np.ndarray, gain: float) -> tuple:
    """(T, I, Gx, Gy) float32 [H, W]: steps 2 and 3."""
    peak = 255.0 if pred.dtype == np.uint8 else 65535.0
    x = target.astype(np.float64) / peak
    zs = gain * (pred.astype(np.float64) / peak)
    grey = lambda v: (0.299 * v[..., 0] + 0.587 * v[..., 1]) + 0.114 * v[..., 2]      # noqa: E731
    t = _blur5(grey(x)).astype(np.float32)
    i = _blur5(grey(zs)).astype(np.float32)
    i64 = i.astype(np.float64)
    px = np.pad(i64, ((0, 0), (1, 1)), mode="reflect")
    py = np.pad(i64, ((1, 1), (0, 0)), mode="reflect")
    gx = (0.5 * (px[:, 2:] - px[:, :-2])).astype(np.float32)
    gy = (0.5 * (py[2:] - py[:-2])).astype(np.float32)
    return t, i, gx, gy


# --------------------------------------------------------------------------- step 4
def positions(m: np.ndarray, h: int, w: int) -> tuple:
    """(den, px, py, inside) of every target pixel: multiply, add and divide as separate operations in this order."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        den = (m[2, 0] * x + m[2, 1] * y) + 1.0
        px = ((m[0, 0] * x + m[0, 1] * y) + m[0, 2]) / den
        py = ((m[1, 0] * x + m[1, 1] * y) + m[1, 2]) / den
        rx, ry = np.rint(px), np.rint(py)
        inside = (rx >= 0.0) & (rx <= w - 1.0) & (ry >= 0.0) & (ry <= h - 1.0)
    return den, px, py, inside


def _bilinear(plane: np.ndarray, px, py) -> np.ndarray:
    """Bilinear samples at positions that round to inside the frame; taps outside read 0."""
    h, w = plane.shape
    fx0, fy0 = np.floor(px), np.floor(py)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    fx, fy = px - fx0, py - fy0
    wx0, wy0 = 1.0 - fx, 1.0 - fy
    p = np.zeros((h + 2, w + 2))
    p[1:-1, 1:-1] = plane
    v00, v01, v10, v11 = p[y0 + 1, x0 + 1], p[y0 + 1, x0 + 2], p[y0 + 2, x0 + 1], p[y0 + 2, x0 + 2]
    return (v00 * wx0 + v01 * fx) * wy0 + (v10 * wx0 + v11 * fx) * fy


def ecc_terms(planes, m: np.ndarray) -> np.ndarray:
    """[n_masked, 66]: the terms of the 66 sums of one round at map m, one row per pixel under the mask."""
    t, i, gx, gy = planes
    h, w = t.shape
    den, px, py, inside = positions(m, h, w)
    yy, xx = np.nonzero(inside)
    den, px, py = den[inside], px[inside], py[inside]
    xd, yd = xx.astype(np.float64), yy.astype(np.float64)
    vi, vgx, vgy = _bilinear(i, px, py), _bilinear(gx, px, py), _bilinear(gy, px, py)
    tv = t[inside].astype(np.float64)
    a, b = vgx / den, vgy / den
    tt = -(px * a + py * b)
    jac = [a * xd, b * xd, tt * xd, a * yd, b * yd, tt * yd, a, b]
    cols = [np.ones_like(vi), vi, tv, vi * vi, tv * tv, vi * tv]
    cols += [jac[p] * jac[q] for p, q in _IU]
    cols += [j * vi for j in jac] + [j * tv for j in jac] + jac
    return np.stack(cols, axis=1) if len(vi) else np.zeros((0, N_SUMS))


def ecc_sums(planes, m: np.ndarray) -> np.ndarray:
    return ecc_terms(planes, m).sum(axis=0)


def hessian_of(s: np.ndarray) -> np.ndarray:
    hm = np.zeros((8, 8))
    for k, (i, j) in enumerate(_IU):
        hm[i, j] = hm[j, i] = s[6 + k]
    return hm


def _cholesky(hm: np.ndarray):
    low = np.zeros((8, 8))
    for j in range(8):
        d = hm[j, j]
        for q in range(j):
            d = d - low[j, q] * low[j, q]
        if not (d > 0.0) or not (d < 1.7e308):
            return None
        dj = math.sqrt(d)
        low[j, j] = dj
        for i in range(j + 1, 8):
            v = hm[i, j]
            for q in range(j):
                v = v - low[i, q] * low[j, q]
            low[i, j] = v / dj
    return low


def _chol_solve(low: np.ndarray, rhs) -> np.ndarray:
    yv, out = np.zeros(8), np.zeros(8)
    for i in range(8):
        v = rhs[i]
        for q in range(i):
            v = v - low[i, q] * yv[q]
        yv[i] = v / low[i, i]
    for i in range(7, -1, -1):
        v = yv[i]
        for q in range(i + 1, 8):
            v = v - low[q, i] * out[q]
        out[i] = v / low[i, i]
    return out


def ecc_update(s: np.ndarray):
    """(dp [8] or None, rho or None) of one round from its 66 sums; dp None: the round failed."""
    n = float(s[0])
    if not n > 0.0:
        return None, None
    mi, mt = s[1] / n, s[2] / n
    ni2, nt2, corr = s[3] - mi * s[1], s[4] - mt * s[2], s[5] - mi * s[2]
    bi = np.array([s[42 + k] - mi * s[58 + k] for k in range(8)])
    bt = np.array([s[50 + k] - mt * s[58 + k] for k in range(8)])
    with np.errstate(all="ignore"):
        rho = float(corr / (np.sqrt(ni2) * np.sqrt(nt2)))
    rho = None if rho != rho else rho
    low = _cholesky(hessian_of(s))
    if low is None:
        return None, rho
    hi = _chol_solve(low, bi)
    ln, ld = ni2, corr
    for k in range(8):
        ln = ln - bi[k] * hi[k]
        ld = ld - bt[k] * hi[k]
    if not ld > 0.0:
        return None, rho
    lam = ln / ld
    dp = _chol_solve(low, [lam * bt[k] - bi[k] for k in range(8)])
    if not all(abs(v) < 1.7e308 for v in dp):
        return None, rho
    return dp, rho


#: where dp[k] goes in the map
_DP_AT = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (0, 2), (1, 2)]


def ecc_iterate(planes, iterations: int = 100, m=None, sums_hook=None):
    """(map, rho, ok): step 4 from map m (the identity by default).  sums_hook(s, round) -> s stands between the sums
    and the update: the tests measure with it how far a rounding-level change of the sums moves the result."""
    m = np.eye(3) if m is None else np.array(m, dtype=np.float64)
    rho = -1.0
    for it in range(iterations):
        s = ecc_sums(planes, m)
        if sums_hook is not None:
            s = sums_hook(s, it)
        dp, r = ecc_update(s)
        if r is not None:
            rho = r
        if dp is None:
            return m, rho, False
        for k, (i, j) in enumerate(_DP_AT):
            m[i, j] += dp[k]
    return m, rho, True


# --------------------------------------------------------------------------- steps 5 and 6
def warp_to_target(pred: np.ndarray, gain: float, m: np.ndarray) -> tuple:
    """(zr float64 [H, W, 3], cr bool [H, W]): step 5."""
    peak = 255.0 if pred.dtype == np.uint8 else 65535.0
    h, w = pred.shape[:2]
    zs = gain * (pred.astype(np.float64) / peak)
    _, px, py, cr = positions(np.asarray(m, dtype=np.float64), h, w)
    zr = np.zeros((h, w, 3))
    if not cr.any():
        return zr, cr
    tab = _cubic_table()
    qx, qy = np.rint(32.0 * px[cr]).astype(np.int64), np.rint(32.0 * py[cr]).astype(np.int64)
    ix, iy = (qx >> 5) - 1, (qy >> 5) - 1
    wx, wy = tab[qx & 31], tab[qy & 31]

    def reflect(i, n):
        return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    xs = [reflect(ix + j, w) for j in range(4)]
    out = np.zeros((len(qx), 3))
    for r in range(4):
        row = reflect(iy + r, h)
        hsum = np.zeros((len(qx), 3))
        for j in range(4):
            hsum = hsum + wx[:, j:j + 1] * zs[row, xs[j]]
        out = out + wy[:, r:r + 1] * hsum
    zr[cr] = out
    return zr, cr


def masked_sums(target: np.ndarray, zr: np.ndarray, cr: np.ndarray, terms: bool = False):
    """The nine numbers of step 6 as irm_aligned_metrics writes them: sse, sum cr, three SSIM numerators, three
    denominators, coverage.  terms=True: also sum |terms| of the first five (the tests' error bound)."""
    peak = 255.0 if target.dtype == np.uint8 else 65535.0
    h, w = cr.shape
    xr = (target.astype(np.float64) / peak) * cr[..., None]
    d = xr - zr
    g = _taps(11, 1.5)
    c1, c2 = 0.01 * 0.01, 0.03 * 0.03

    def blur(a):                                                              # valid region, rows then columns
        v = sum(g[k] * a[k:k + h - 10] for k in range(11))
        return sum(g[k] * v[:, k:k + w - 10] for k in range(11))
    centre = cr[5:h - 5, 5:w - 5]
    nums, mags = [], []
    for ch in range(3):
        a, b = xr[..., ch], zr[..., ch]
        m1, m2 = blur(a), blur(b)
        m11, m22, m12 = m1 * m1, m2 * m2, m1 * m2
        v1, v2, v12 = blur(a * a) - m11, blur(b * b) - m22, blur(a * b) - m12
        smap = ((2.0 * m12 + c1) * (2.0 * v12 + c2)) / ((m11 + m22 + c1) * (v1 + v2 + c2))
        nums.append(float(smap[centre].sum()))
        mags.append(float(np.abs(smap[centre]).sum()))
    n, nv = float(cr.sum()), float(centre.sum())
    out = np.array([float((d * d).sum()), n] + nums + [nv] * 3 + [n / (h * w)])
    return (out, np.array([out[0], n] + mags)) if terms else out


def scores_of(out, gain: float, rho: float, ok: bool, m) -> AlignedMetrics:
    """AlignedMetrics from the nine numbers of step 6."""
    sse, n, cov = float(out[0]), float(out[1]), float(out[8])
    m = np.array(m, dtype=np.float64).reshape(3, 3)
    if not n > 0.0:
        return AlignedMetrics(float("nan"), float("nan"), float(rho), cov, float(gain), False, m)
    psnr = float("inf") if sse == 0.0 else float(10.0 * np.log10(1.0 / (sse / (3.0 * n))))
    with np.errstate(all="ignore"):
        ssim = float(np.mean([out[2 + c] / out[5 + c] for c in range(3)]))
    return AlignedMetrics(psnr, ssim, float(rho), cov, float(gain), bool(ok), m)


def align_to_target(pred: np.ndarray, target: np.ndarray, iterations: int = 100, m=None) -> tuple:
    """(zr float32 [H, W, 3], cr uint8 [H, W], AlignedMetrics): the whole statement; with a map `m` the iteration is
    skipped and the frames are warped and scored under it (rho is NaN)."""
    _check_host_pair(pred, target, "align_to_target")
    iterations = _check_iterations(iterations)
    gain, ok = gain_of(pred, target)
    rho = float("nan")
    if m is None:
        m = np.eye(3)
        if ok:
            m, rho, ok = ecc_iterate(planes_of(pred, target, gain), iterations)
    zr, cr = warp_to_target(pred, gain, m)
    res = scores_of(masked_sums(target, zr, cr), gain, rho, ok, m)
    return zr.astype(np.float32), cr.astype(np.uint8), res


def calculate_metrics_aligned(pred: np.ndarray, target: np.ndarray, iterations: int = 100) -> AlignedMetrics:
    """The float64 numpy statement of the aligned protocol: AlignedMetrics(psnr, ssim, rho, coverage, gain, ok, map).
    A pair that cannot be aligned (flat frames, no overlap) has ok False; nothing is raised for it."""
    return align_to_target(pred, target, iterations)[2]


# --------------------------------------------------------------------------- the device
def _check_device_pair(pred_dev, target_dev, what: str) -> tuple:
    if not isinstance(pred_dev, torch.Tensor) or not isinstance(target_dev, torch.Tensor):
        raise ValueError(f"{what} takes torch tensors (use calculate_metrics_aligned for numpy arrays)")
    if pred_dev.shape != target_dev.shape or pred_dev.dtype != target_dev.dtype:
        raise ValueError(f"prediction {tuple(pred_dev.shape)} {pred_dev.dtype} and target {tuple(target_dev.shape)} "
                         f"{target_dev.dtype} differ in shape or dtype")
    if pred_dev.dtype not in FRAME_DTYPES:
        raise ValueError(f"{what} takes uint8 or uint16 frames, not {pred_dev.dtype}")
    h, w = _check_shape(pred_dev.shape, what)
    if not pred_dev.is_cuda or not target_dev.is_cuda:
        raise ValueError("device metrics need GPU tensors; there is no CPU fallback")
    if pred_dev.device != target_dev.device:
        raise ValueError("the frames of one call must share a device")
    return h, w


def prepare_words(h: int, w: int) -> int:
    return 2 * -(-(3 * h * w) // _GAIN_CHUNK)


def iterate_words(h: int, w: int) -> int:
    return N_SUMS * -(-h // _ECC_TILE_H) * -(-w // _ECC_TILE_W)


def metrics_words(h: int, w: int) -> int:
    return 6 * -(-(h - 10) // _METRIC_TILE_H) * -(-(w - 10) // _METRIC_TILE_W)


class _Run:
    """The device state of one pair: frames as the kernels read them, gain, map, rho, status and one workspace."""

    def __init__(self, pred_dev, target_dev, what):
        self.h, self.w = _check_device_pair(pred_dev, target_dev, what)
        self.dev = pred_dev.device
        h, w = self.h, self.w
        with torch.cuda.device(self.dev):
            self.p, self.t = frame_bits([pred_dev]), frame_bits([target_dev])
            self.u16 = int(pred_dev.dtype != torch.uint8)
            self.f64 = torch.zeros(20, dtype=torch.float64, device=self.dev)      # gain, rho, map [9], out [9]
            self.f64[2:11] = torch.eye(3, dtype=torch.float64, device=self.dev).reshape(-1)
            self.f64[1] = -1.0
            self.gain, self.rho, self.map, self.out = self.f64[0:1], self.f64[1:2], self.f64[2:11], self.f64[11:20]
            self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self.ws = torch.empty(max(prepare_words(h, w), iterate_words(h, w), metrics_words(h, w)),
                                  dtype=torch.float64, device=self.dev)

    def prepare_and_iterate(self, iterations):
        h, w = self.h, self.w
        with torch.cuda.device(self.dev):
            planes = torch.empty(4, h, w, dtype=torch.float32, device=self.dev)
            _hip.call("irm_align_prepare", _hip.ptr(self.p), _hip.ptr(self.t), self.u16, h, w, _hip.ptr(self.gain),
                      _hip.ptr(self.status), *(_hip.ptr(planes[k]) for k in range(4)), _hip.ptr(self.ws), self.ws.numel())
            _hip.call("irm_ecc_iterate", *(_hip.ptr(planes[k]) for k in range(4)), h, w, iterations, _hip.ptr(self.map),
                      _hip.ptr(self.rho), _hip.ptr(self.status), _hip.ptr(self.ws), self.ws.numel())

    def score(self, frames: bool):
        h, w = self.h, self.w
        with torch.cuda.device(self.dev):
            zr = torch.empty(h, w, 3, dtype=torch.float32, device=self.dev) if frames else None
            cr = torch.empty(h, w, dtype=torch.uint8, device=self.dev) if frames else None
            _hip.call("irm_aligned_metrics", _hip.ptr(self.p), _hip.ptr(self.t), self.u16, h, w, _hip.ptr(self.gain),
                      _hip.ptr(self.map), _hip.ptr(self.out), _hip.ptr(self.status), _hip.ptr(zr), _hip.ptr(cr),
                      _hip.ptr(self.ws), self.ws.numel())
        return zr, cr

    def result(self) -> AlignedMetrics:
        host = torch.cat([self.f64, self.status.to(torch.float64)]).cpu().numpy()      # the one host synchronisation
        return scores_of(host[11:20], host[0], host[1], host[20] == 0.0, host[2:11])


def ecc_homography_device(pred_dev: torch.Tensor, target_dev: torch.Tensor, iterations: int = 100) -> tuple:
    """Steps 1 to 4 on the GPU for a uint8 / uint16 [H, W, 3] pair: (map [3, 3] float64 device tensor, status int32
    device tensor [1]: 0 fine, 1 failed - the map is then the last good one), not synchronised with the host."""
    iterations = _check_iterations(iterations)
    run = _Run(pred_dev, target_dev, "ecc_homography_device")
    run.prepare_and_iterate(iterations)
    return run.map.reshape(3, 3).clone(), run.status


def align_to_target_device(pred_dev: torch.Tensor, target_dev: torch.Tensor, iterations: int = 100) -> tuple:
    """The whole protocol on the GPU: (zr float32 [H, W, 3] and cr uint8 [H, W] device tensors, AlignedMetrics) after one
    synchronising copy.  Bitwise the same on every call."""
    iterations = _check_iterations(iterations)
    run = _Run(pred_dev, target_dev, "align_to_target_device")
    run.prepare_and_iterate(iterations)
    zr, cr = run.score(True)
    return zr, cr, run.result()


def calculate_metrics_aligned_device(pred_dev: torch.Tensor, target_dev: torch.Tensor, iterations: int = 100) -> AlignedMetrics:
    """Device twin of calculate_metrics_aligned for uint8 / uint16 [H, W, 3] GPU frames: 2 x iterations + 6 launches on
    the current stream, one synchronising copy at the end.  No CPU fallback."""
    iterations = _check_iterations(iterations)
    run = _Run(pred_dev, target_dev, "calculate_metrics_aligned_device")
    run.prepare_and_iterate(iterations)
    run.score(False)
    return run.result()
