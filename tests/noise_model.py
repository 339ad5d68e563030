"""The noise statistic stated by brute force, and the frames the noise tests share.  No test functions here:
tests/test_noise_cpu.py and tests/test_gpu_noise.py import this module.

The statistic (include/irm_hip_noise.h): with v = sample >> shift, every non-overlapping 2 x 2
block gives d = |a - b - c + e|; blocks with a sample <= sat_lo or >= sat_hi are left out; the result per channel is
(n, m, below, at) with m the element of index (n - 1) // 2 of the sorted d."""
import numpy as np

MAD_SCALE = 0.6744897501960817


def brute_stats(img, shift=0, sat_lo=None, sat_hi=None):
    """[C][4] Python ints, one block at a time, sorted() on a list."""
    img = np.asarray(img)
    peak = 255 if img.dtype == np.uint8 else 65535
    sat_lo = 0 if sat_lo is None else sat_lo
    sat_hi = peak if sat_hi is None else sat_hi
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, ch = img.shape
    out = []
    for k in range(ch):
        vals = []
        for i in range(h // 2):
            for j in range(w // 2):
                a, b = int(img[2 * i, 2 * j, k]) >> shift, int(img[2 * i, 2 * j + 1, k]) >> shift
                c, e = int(img[2 * i + 1, 2 * j, k]) >> shift, int(img[2 * i + 1, 2 * j + 1, k]) >> shift
                if min(a, b, c, e) <= sat_lo or max(a, b, c, e) >= sat_hi:
                    continue
                vals.append(abs(a - b - c + e))
        vals = sorted(vals)
        n = len(vals)
        if n == 0:
            out.append([0, 0, 0, 0])
            continue
        m = vals[(n - 1) // 2]
        out.append([n, m, sum(1 for v in vals if v < m), sum(1 for v in vals if v == m)])
    return out


def sigma_of(stats4, span):
    """The sigma of one (n, m, below, at), in Python floats."""
    n, m, below, at = (int(v) for v in stats4)
    if n == 0:
        return float("nan")
    if m == 0:
        return 0.0
    return (m - 0.5 + (n / 2 - below) / at) / 2 / MAD_SCALE * 255 / span


def noisy_frame(h, w, c, sigma, dtype=np.uint8):
    """A smooth frame plus N(0, sigma) noise (sigma on the 0..255 scale), rounded and clipped to the dtype's range."""
    peak = 255 if dtype == np.uint8 else 65535
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 0.5 + 0.25 * np.sin(x / 17) * np.cos(y / 23)
    img = np.repeat(base[:, :, None], c, axis=2) * peak
    img = img + np.random.RandomState(100 + sigma).normal(0, sigma / 255 * peak, (h, w, c))
    return np.clip(np.rint(img), 0, peak).astype(dtype)


def degenerate_frames(dtype=np.uint8):
    """name -> (frame, kwargs of noise_stats, expected [C][4]) for the frames whose integers can be written down."""
    peak = 255 if dtype == np.uint8 else 65535
    one = np.full((6, 8), peak // 2, dtype)
    one[:, :] = 0                                    # saturated everywhere ...
    one[2:4, 4:6] = [[1, 2], [3, 5]]                 # ... but for one block: d = |1 - 2 - 3 + 5| = 1
    checker = np.zeros((6, 8), dtype)
    checker[0::2, 0::2] = peak
    checker[1::2, 1::2] = peak                       # a = e = peak, b = c = 0: d = 2 peak
    return {"flat": (np.full((7, 9, 3), peak // 3, dtype), {}, [[12, 0, 0, 12]] * 3),
            "black": (np.zeros((6, 8), dtype), {}, [[0, 0, 0, 0]]),
            "peak": (np.full((6, 8, 3), peak, dtype), {}, [[0, 0, 0, 0]] * 3),
            "one_block": (one, {}, [[1, 1, 0, 1]]),
            "checkerboard": (checker, {"exclude_saturated": False}, [[12, 2 * peak, 0, 12]]),
            "checkerboard_excluded": (checker, {}, [[0, 0, 0, 0]])}
