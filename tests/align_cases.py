"""Frames for the tests of the aligned protocol (irm_amd/align.py): an analytic image - per channel a sum of 24
low-frequency sinusoids - sampled EXACTLY under a known homography, so that no interpolation enters the truth.

The target is the image at the pixel centres, the prediction is GAIN times the image at the inverse-mapped pixel
centres: a target pixel p shows what the prediction shows at TRUE_MAP p.  Both are rounded to uint8.  The map is a
rotation by 0.4 degrees and scales 1.004 / 0.997 about the frame centre, a shift of (1.7, -0.9) pixels and a perspective
row (2e-5, -1e-5)."""
import math

import numpy as np

CASES = {"A": (96, 128), "B": (61, 83)}
GAIN = 0.93
SEED = 24

#: corner displacement (corner_displacement below, pixels) of the statement's map from the true one after 100 rounds,
#: measured with the statement: A 0.12487, B 0.06352 (what the uint8 rounding of both frames and the zero taps at the
#: border leave).  The bound is 1.5 times that; the identity is 1.88 (A) and 1.91 (B) off.
RECOVERY_BOUND = {"A": 1.5 * 0.12487, "B": 1.5 * 0.06352}

#: how far a rounding-level change of the sums moves the statement's result: each of the 66 sums of each of the 100
#: rounds multiplied by 1 + 1e-12 u, u uniform in [-1, 1] (numpy default_rng(1000 + draw)), the largest change over 8
#: draws - corner displacement from the unperturbed map 2.352e-10 (A) and 2.946e-10 (B) pixels, rho 2.030e-10 and
#: 1.917e-10, PSNR and SSIM 0 (no mask bit and no 1/32 phase moves).  The tolerances are 4 times that.
CORNER_TOL = {"A": 4 * 2.352e-10, "B": 4 * 2.946e-10}
RHO_TOL = {"A": 4 * 2.030e-10, "B": 4 * 1.917e-10}
_MADE = {}


def true_map(h: int, w: int) -> np.ndarray:
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    a = math.radians(0.4)
    lin = np.array([[1.004 * math.cos(a), -0.997 * math.sin(a)], [1.004 * math.sin(a), 0.997 * math.cos(a)]])
    m = np.eye(3)
    m[:2, :2] = lin
    m[:2, 2] = np.array([cx, cy]) - lin @ np.array([cx, cy]) + np.array([1.7, -0.9])
    m[2, :2] = (2e-5, -1e-5)
    return m


def apply_map(m: np.ndarray, x, y) -> tuple:
    den = m[2, 0] * x + m[2, 1] * y + m[2, 2]
    return (m[0, 0] * x + m[0, 1] * y + m[0, 2]) / den, (m[1, 0] * x + m[1, 1] * y + m[1, 2]) / den


def corner_displacement(ma, mb, h: int, w: int) -> float:
    """Mean distance, in pixels, between the images of the four frame corners under two maps."""
    d = []
    for x, y in ((0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0)):
        ax, ay = apply_map(np.asarray(ma, dtype=np.float64).reshape(3, 3), x, y)
        bx, by = apply_map(np.asarray(mb, dtype=np.float64).reshape(3, 3), x, y)
        d.append(math.hypot(ax - bx, ay - by))
    return float(np.mean(d))


def image(x, y) -> np.ndarray:
    """The analytic image at real positions: [..., 3] in (0.05, 0.95)."""
    rng = np.random.default_rng(SEED)
    out = []
    for _ in range(3):
        f = rng.uniform(-0.06, 0.06, (24, 2))              # cycles per pixel: wavelengths of 12 pixels and more
        ph = rng.uniform(0.0, 2.0 * math.pi, 24)
        amp = rng.uniform(0.5, 1.0, 24)
        amp *= 0.45 / amp.sum()
        v = 0.5
        for k in range(24):
            v = v + amp[k] * np.sin(2.0 * math.pi * (f[k, 0] * x + f[k, 1] * y) + ph[k])
        out.append(v)
    return np.stack(out, axis=-1)


def pair(name: str) -> tuple:
    """(prediction, target, true map) of case A or B, uint8 [H, W, 3]; made once, shared, never written to."""
    if name not in _MADE:
        h, w = CASES[name]
        m = true_map(h, w)
        y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        target = np.rint(255.0 * image(x, y)).astype(np.uint8)
        ux, uy = apply_map(np.linalg.inv(m), x, y)
        pred = np.rint(255.0 * GAIN * image(ux, uy)).astype(np.uint8)
        for a in (pred, target, m):
            a.setflags(write=False)
        _MADE[name] = (pred, target, m)
    return _MADE[name]


def shift_map(dx: int, dy: int) -> np.ndarray:
    m = np.eye(3)
    m[0, 2], m[1, 2] = dx, dy
    return m


def outside_map(h: int, w: int) -> np.ndarray:
    """Pushes the right third of the frame outside: a shift by w / 3 with a little rotation and perspective."""
    m = true_map(h, w)
    m[0, 2] += w / 3.0
    return m
