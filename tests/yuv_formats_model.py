"""CPU model of the YUV conversions over the whole grid of formats (csrc/yuv.hip, irm_amd/yuv.py):
4:2:0, 4:2:2 and 4:4:4 at 8, 10 and 12 bit, planar and semi-planar.  It extends tests/yuv_model.py, whose text states
the 4:2:0 arithmetic, and equals it bit for bit on its three names.

Two models from one text, as there: `ft=np.float32` is the kernels' arithmetic, every multiply, add, subtract and divide
one correctly rounded float32 operation in the order written; `ft=np.float64` is the same formulas with float64
coefficients, the yardstick.

LAYOUTS: name -> (sub_w, sub_h, planes, depth, upper_bits).  Chroma planes are [H / sub_h][W / sub_w]; planar is
(y, u, v), semi-planar (y, uv [CH][CW][2], U first); 8-bit samples are uint8, all others uint16 with the code in the low
bits or, with upper_bits, stored as code << (16 - depth).

Up-sampling (to RGB), linear on the integer codes with clamped edges, in sixteenths:
  4:2:0   yuv_model.upsample16;
  4:2:2   horizontally only.  "left": 16 c[i] on column 2 i, 8 c[i] + 8 c[i + 1] on column 2 i + 1.
          "center": 12 c[i] + 4 c[i - 1] on column 2 i, 12 c[i] + 4 c[i + 1] on column 2 i + 1;
  4:4:4   16 c.
Sixteen times a code is an integer below 2^16: its product with 1/16 is exact in float32.
Filtering (to YUV) of the per-pixel chroma c:
  4:2:0   yuv_model.filter_chroma;
  4:2:2   "center": (c[2i] + c[2i+1]) * 0.5;  "left": ((c[2i-1] + (c[2i] + c[2i])) + c[2i+1]) * 0.25, c[-1] = c[0];
  4:4:4   c.
"""
import numpy as np

import yuv_model

LAYOUTS = {}
for _sub, _tag, _semi in (((2, 2), "420", ("nv12", "p010", "p012")), ((2, 1), "422", ("nv16", "p210", "p212")),
                          ((1, 1), "444", ("nv24", "p410", "p412"))):
    for _depth, _name in zip((8, 10, 12), _semi):
        LAYOUTS[f"i{_tag}" + ("" if _depth == 8 else f"p{_depth}")] = _sub + (3, _depth, 0)
        LAYOUTS[_name] = _sub + (2, _depth, int(_depth > 8))
PLANAR = sorted(n for n, v in LAYOUTS.items() if v[2] == 3)


def shift_of(fmt):
    _, _, _, depth, upper = LAYOUTS[fmt]
    return 16 - depth if upper else 0


def dtype_of(fmt):
    return np.uint8 if LAYOUTS[fmt][3] == 8 else np.uint16


def plane_shapes(h, w, fmt):
    sw, sh, n = LAYOUTS[fmt][:3]
    return [(h, w)] + ([(h // sh, w // sw)] * 2 if n == 3 else [(h // sh, w // sw, 2)])


def check(fmt, matrix, siting, h, w):
    if fmt not in LAYOUTS or matrix not in yuv_model.K or siting not in ("left", "center"):
        raise ValueError((fmt, matrix, siting))
    sw, sh = LAYOUTS[fmt][:2]
    if h <= 0 or w <= 0 or h % sh or w % sw:
        raise ValueError(f"frame {h} x {w} in {fmt}")


def codes_of(planes, fmt):
    """(y, u, v) integer codes of a frame's planes (u, v None if only Y was given)."""
    s = shift_of(fmt)
    y = planes[0].astype(np.int64) >> s
    if len(planes) == 1:
        return y, None, None
    if LAYOUTS[fmt][2] == 3:
        return y, planes[1].astype(np.int64) >> s, planes[2].astype(np.int64) >> s
    return y, planes[1][..., 0].astype(np.int64) >> s, planes[1][..., 1].astype(np.int64) >> s


def planes_of(y, u, v, fmt):
    """Integer codes -> the planes of `fmt`."""
    dt, s = dtype_of(fmt), shift_of(fmt)
    if LAYOUTS[fmt][2] == 3:
        return (y << s).astype(dt), (u << s).astype(dt), (v << s).astype(dt)
    return (y << s).astype(dt), (np.stack([u, v], axis=-1) << s).astype(dt)


def random_planes(rng, fmt, h, w):
    top = 1 << LAYOUTS[fmt][3]
    return tuple((rng.integers(0, top, s) << shift_of(fmt)).astype(dtype_of(fmt)) for s in plane_shapes(h, w, fmt))


def upsample16(c, fmt, siting):
    """Sixteen times the up-sampled codes: [CH][CW] integers -> [H][W] integers."""
    sub = LAYOUTS[fmt][:2]
    if sub == (2, 2):
        return yuv_model.upsample16(c, siting)
    if sub == (1, 1):
        return 16 * c
    cw = c.shape[1]
    cols = np.arange(cw)
    out = np.zeros((c.shape[0], 2 * cw), np.int64)
    if siting == "center":
        out[:, 0::2] = 12 * c + 4 * c[:, np.clip(cols - 1, 0, cw - 1)]
        out[:, 1::2] = 12 * c + 4 * c[:, np.clip(cols + 1, 0, cw - 1)]
    else:
        out[:, 0::2] = 16 * c
        out[:, 1::2] = 8 * c + 8 * c[:, np.clip(cols + 1, 0, cw - 1)]
    return out


def to_rgb(planes, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, ft=np.float32):
    """Planes -> ft [H][W][3] in [0, 1] ([H][W][1] = clip(Y') with luma_only)."""
    h, w = planes[0].shape
    check(fmt, matrix, siting, h, w)
    k = yuv_model.constants(matrix, full_range, LAYOUTS[fmt][3], ft)
    y, u, v = codes_of(planes[:1] if luma_only else planes, fmt)
    yp = (y.astype(ft) - k["y0"]) / k["yr"]
    if luma_only:
        return np.clip(yp, ft(0), ft(1))[:, :, None]
    cb = (upsample16(u, fmt, siting).astype(ft) * ft(1 / 16) - k["c0"]) / k["cr"]
    cr = (upsample16(v, fmt, siting).astype(ft) * ft(1 / 16) - k["c0"]) / k["cr"]
    r = yp + k["r_cr"] * cr
    g = (yp - k["g_cb"] * cb) - k["g_cr"] * cr
    b = yp + k["b_cb"] * cb
    return np.clip(np.stack([r, g, b], axis=-1), ft(0), ft(1))


def filter_chroma(c, fmt, siting, ft):
    """Per-pixel chroma [H][W] -> the value at the chroma site [CH][CW]; this fixes the order of the additions."""
    sub = LAYOUTS[fmt][:2]
    if sub == (2, 2):
        return yuv_model.filter_chroma(c, siting, ft)
    if sub == (1, 1):
        return c
    even = np.arange(0, c.shape[1], 2)
    l, m, r = c[:, np.maximum(even - 1, 0)], c[:, even], c[:, even + 1]
    if siting == "center":
        return (m + r) * ft(0.5)
    return ((l + (m + m)) + r) * ft(0.25)


def to_yuv_values(rgb, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, ft=np.float32):
    """The clipped code values before rounding: (y [H][W], u, v [CH][CW]) in ft (u, v None with luma_only)."""
    h, w = rgb.shape[:2]
    check(fmt, matrix, siting, h, w)
    k = yuv_model.constants(matrix, full_range, LAYOUTS[fmt][3], ft)
    rgb = rgb.astype(ft)
    if luma_only:
        return np.clip(k["y0"] + k["yr"] * rgb[:, :, 0], ft(0), k["top"]), None, None
    r, g, b = rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]
    yp = (k["kr"] * r + k["kg"] * g) + k["kb"] * b
    cb = filter_chroma((b - yp) / k["b_cb"], fmt, siting, ft)
    cr = filter_chroma((r - yp) / k["r_cr"], fmt, siting, ft)
    return (np.clip(k["y0"] + k["yr"] * yp, ft(0), k["top"]), np.clip(k["c0"] + k["cr"] * cb, ft(0), k["top"]),
            np.clip(k["c0"] + k["cr"] * cr, ft(0), k["top"]))


def to_yuv(rgb, fmt, matrix="bt709", full_range=False, siting="left", luma_only=False, ft=np.float32, chroma=None):
    """float [H][W][3] -> the planes of `fmt`, codes rounded half to even.  With luma_only the frame is [H][W][1] and
    `chroma`, the frame's other planes, is returned behind the new Y plane as it is."""
    y, u, v = (None if t is None else np.rint(t).astype(np.int64)
               for t in to_yuv_values(rgb, fmt, matrix, full_range, siting, luma_only, ft))
    if luma_only:
        return ((y << shift_of(fmt)).astype(dtype_of(fmt)),) + tuple(chroma or ())
    return planes_of(y, u, v, fmt)
