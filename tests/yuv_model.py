"""CPU model of the YUV 4:2:0 conversions (csrc/yuv.hip, irm_amd/yuv.py): the statement of their arithmetic.

Two models from one text.  `ft=np.float32` is the kernels' arithmetic, operation by operation: every multiply, add,
subtract and divide below is one correctly rounded float32 operation on float32 operands, the coefficients are the
float32 roundings of their float64 expressions, and the order of the operations is the order written here.
`ft=np.float64` evaluates the same formulas with the float64 coefficients and no float32 rounding: the independent
yardstick the float32 model is held to.

Formats (4:2:0, H and W even): "i420" = (y [H][W], u [H/2][W/2], v [H/2][W/2]) uint8; "nv12" = (y, uv [H/2][W/2][2],
U first) uint8; "p010" = (y, uv) uint16 with the 10-bit code in the upper bits (code = word >> 6).
d = bit depth, k = 2^(d-8); limited range y0 = 16 k, yr = 219 k, c0 = 128 k, cr = 224 k; full range y0 = 0,
yr = cr = 2^d - 1, c0 = 128 k.  matrix "bt601": Kr 0.299, Kb 0.114; "bt709": Kr 0.2126, Kb 0.0722; Kg = 1 - Kr - Kb.

Chroma sites.  "center": the sample lies in the middle of its 2 x 2 luma block.  "left": it lies on the even luma column,
midway between the two rows.  Up-sampling is linear between the sites on the integer codes with clamped coordinates;
all weights are sixteenths, so sixteen times the value is an integer below 2^15 and the product with 1/16 is exact.
"""
import numpy as np

DEPTH = {"i420": 8, "nv12": 8, "p010": 10}
K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def constants(matrix, full_range, depth, ft):
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    k, top = 2.0 ** (depth - 8), 2.0 ** depth - 1.0
    c = {"y0": 0.0 if full_range else 16.0 * k, "yr": top if full_range else 219.0 * k, "c0": 128.0 * k,
         "cr": top if full_range else 224.0 * k, "kr": kr, "kg": kg, "kb": kb, "top": top,
         "r_cr": 2.0 * (1.0 - kr), "b_cb": 2.0 * (1.0 - kb),
         "g_cb": 2.0 * kb * (1.0 - kb) / kg, "g_cr": 2.0 * kr * (1.0 - kr) / kg}
    return {name: ft(v) for name, v in c.items()}


def check(fmt, matrix, siting, h, w):
    if fmt not in DEPTH or matrix not in K or siting not in ("left", "center"):
        raise ValueError((fmt, matrix, siting))
    if h <= 0 or w <= 0 or h % 2 or w % 2:
        raise ValueError(f"odd frame {h} x {w}")


def codes_of(planes, fmt):
    """(y, u, v) integer codes of a frame's planes (u, v None if only Y was given)."""
    shift = 6 if fmt == "p010" else 0
    y = planes[0].astype(np.int64) >> shift
    if len(planes) == 1:
        return y, None, None
    if fmt == "i420":
        return y, planes[1].astype(np.int64), planes[2].astype(np.int64)
    return y, planes[1][..., 0].astype(np.int64) >> shift, planes[1][..., 1].astype(np.int64) >> shift


def planes_of(y, u, v, fmt):
    """Integer codes -> the planes of `fmt`."""
    dt, shift = (np.uint16, 6) if fmt == "p010" else (np.uint8, 0)
    if fmt == "i420":
        return (y << shift).astype(dt), (u << shift).astype(dt), (v << shift).astype(dt)
    return (y << shift).astype(dt), (np.stack([u, v], axis=-1) << shift).astype(dt)


def upsample_weights(siting):
    """Per output parity: (offset of the second sample, weight of the own sample, weight of the second), in quarters.
    Vertically both sitings place the sample midway between its two rows."""
    vertical = {0: (-1, 3, 1), 1: (+1, 3, 1)}
    horizontal = vertical if siting == "center" else {0: (0, 4, 0), 1: (+1, 2, 2)}
    return vertical, horizontal


def upsample16(c, siting):
    """Sixteen times the up-sampled codes: [H/2][W/2] integers -> [H][W] integers."""
    ch, cw = c.shape
    vertical, horizontal = upsample_weights(siting)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    rows, cols = np.arange(ch), np.arange(cw)
    for py, (dy, wy0, wy1) in vertical.items():
        r1 = np.clip(rows + dy, 0, ch - 1)
        for px, (dx, wx0, wx1) in horizontal.items():
            c1 = np.clip(cols + dx, 0, cw - 1)
            out[py::2, px::2] = (wy0 * wx0 * c + wy0 * wx1 * c[:, c1] + wy1 * wx0 * c[r1, :]
                                 + wy1 * wx1 * c[np.ix_(r1, c1)])
    return out


def to_rgb(planes, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, ft=np.float32):
    """Planes -> ft [H][W][3] in [0, 1] ([H][W][1] = clip(Y') with luma_only)."""
    h, w = planes[0].shape
    check(fmt, matrix, siting, h, w)
    k = constants(matrix, full_range, DEPTH[fmt], ft)
    y, u, v = codes_of(planes[:1] if luma_only else planes, fmt)
    yp = (y.astype(ft) - k["y0"]) / k["yr"]
    if luma_only:
        return np.clip(yp, ft(0), ft(1))[:, :, None]
    cb = (upsample16(u, siting).astype(ft) * ft(1 / 16) - k["c0"]) / k["cr"]
    cr = (upsample16(v, siting).astype(ft) * ft(1 / 16) - k["c0"]) / k["cr"]
    r = yp + k["r_cr"] * cr
    g = (yp - k["g_cb"] * cb) - k["g_cr"] * cr
    b = yp + k["b_cb"] * cb
    return np.clip(np.stack([r, g, b], axis=-1), ft(0), ft(1))


def filter_chroma(c, siting, ft):
    """Per-pixel chroma [H][W] -> the value at the chroma site [H/2][W/2]; this fixes the order of the additions."""
    if siting == "center":
        a, b, cc, d = c[0::2, 0::2], c[0::2, 1::2], c[1::2, 0::2], c[1::2, 1::2]
        return ((a + b) + (cc + d)) * ft(0.25)
    w = c.shape[1]
    even = np.arange(0, w, 2)
    l, m, r = c[:, np.maximum(even - 1, 0)], c[:, even], c[:, even + 1]
    rows = ((l + (m + m)) + r) * ft(0.25)
    return (rows[0::2] + rows[1::2]) * ft(0.5)


def to_yuv_values(rgb, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, ft=np.float32):
    """The clipped code values before rounding: (y [H][W], u, v [H/2][W/2]) in ft (u, v None with luma_only)."""
    h, w = rgb.shape[:2]
    check(fmt, matrix, siting, h, w)
    k = constants(matrix, full_range, DEPTH[fmt], ft)
    rgb = rgb.astype(ft)
    if luma_only:
        return np.clip(k["y0"] + k["yr"] * rgb[:, :, 0], ft(0), k["top"]), None, None
    r, g, b = rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]
    yp = (k["kr"] * r + k["kg"] * g) + k["kb"] * b
    cb = filter_chroma((b - yp) / k["b_cb"], siting, ft)
    cr = filter_chroma((r - yp) / k["r_cr"], siting, ft)
    return (np.clip(k["y0"] + k["yr"] * yp, ft(0), k["top"]), np.clip(k["c0"] + k["cr"] * cb, ft(0), k["top"]),
            np.clip(k["c0"] + k["cr"] * cr, ft(0), k["top"]))


def to_yuv(rgb, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, ft=np.float32, chroma=None):
    """float [H][W][3] -> the planes of `fmt`, codes rounded half to even.  With luma_only the frame is [H][W][1] and
    `chroma`, the frame's other planes, is returned behind the new Y plane as it is."""
    y, u, v = (None if t is None else np.rint(t).astype(np.int64)
               for t in to_yuv_values(rgb, fmt, matrix, full_range, siting, luma_only, ft))
    if luma_only:
        dt, shift = (np.uint16, 6) if fmt == "p010" else (np.uint8, 0)
        return ((y << shift).astype(dt),) + tuple(chroma or ())
    return planes_of(y, u, v, fmt)
