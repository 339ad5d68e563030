"""The whole grid of YUV formats (4:2:0, 4:2:2, 4:4:4 at 8, 10 and 12 bit), the part that needs no GPU: the model of
tests/yuv_formats_model.py against tests/yuv_model.py and against its float64 twin, the C ABI of
include/irm_hip_video.h against _hip.SIGNATURES_VIDEO, the library's argument refusals before any launch, hand-made
anchors, the up-sampling weights, the numpy twins of irm_amd/yuv.py against the model bit for bit, the metrics twin, and
the callers that learn the new names."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import yuv_formats_model as fm
import yuv_model
from irm_amd import _hip, harness, metrics, stream, utils, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_yuv_to_rgb_f32", "irm_rgb_f32_to_yuv", "irm_yuv_metrics"]
MATRICES, SITINGS = ("bt601", "bt709"), ("left", "center")
CPU = torch.device("cpu")
SEED = 20
GRID = sorted(fm.LAYOUTS)


def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip.load()


# --------------------------------------------------------------------------- the grid and the model
def test_the_grid_is_the_issue_s_table():
    assert yuv.YUV_FORMATS == {"i420": (3, 8), "nv12": (2, 8), "p010": (2, 10)}
    assert yuv.YUV_LAYOUTS == fm.LAYOUTS and len(GRID) == 18
    assert yuv.YUV_LAYOUTS["p210"] == (2, 1, 2, 10, 1) and yuv.YUV_LAYOUTS["i444p12"] == (1, 1, 3, 12, 0)
    assert yuv.YUV_LAYOUTS["i420p10"] == (2, 2, 3, 10, 0) and yuv.YUV_LAYOUTS["nv24"] == (1, 1, 2, 8, 0)
    for name, (planes, depth) in yuv.YUV_FORMATS.items():
        assert yuv.YUV_LAYOUTS[name][:4] == (2, 2, planes, depth)
    assert yuv.plane_shapes(5, 6, "i422") == [(5, 6), (5, 3), (5, 3)]
    assert yuv.plane_shapes(5, 7, "p412") == [(5, 7), (5, 7, 2)]
    assert yuv.plane_shapes(4, 6, "nv12") == [(4, 6), (2, 3, 2)] and yuv.plane_shapes(4, 6, "p210", True) == [(4, 6)]


@pytest.mark.parametrize("fmt", ["i420", "nv12", "p010"])
def test_model_equals_the_420_model_on_its_three_names(fmt):
    rng = np.random.default_rng(SEED)
    for matrix, full, siting in itertools.product(MATRICES, (False, True), SITINGS):
        planes = fm.random_planes(rng, fmt, 6, 10)
        rgb = rng.uniform(-0.1, 1.1, (6, 10, 3)).astype(np.float32)
        for ft in (np.float32, np.float64):
            for luma_only in (False, True):
                a = fm.to_rgb(planes, fmt, matrix, full, siting, luma_only, ft=ft)
                b = yuv_model.to_rgb(planes, fmt, matrix, full, siting, luma_only, ft=ft)
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
                frame = rgb[:, :, :1] if luma_only else rgb
                for g, t in zip(fm.to_yuv(frame, fmt, matrix, full, siting, luma_only, ft=ft, chroma=planes[1:]),
                                yuv_model.to_yuv(frame, fmt, matrix, full, siting, luma_only, ft=ft, chroma=planes[1:])):
                    assert g.dtype == t.dtype and np.array_equal(g, t)


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_symbols():
    """include/irm_hip_video.h, included by irm_hip.h inside its extern "C" block after irm_hip_lpips.h, and
    _hip.SIGNATURES_VIDEO, disjoint from the other nine tables, match one to one; the library exports the symbols,
    load() binds them, and all-zero arguments return IRM_EINVAL before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_lpips.h"') < main.index('#include "irm_hip_video.h"') \
        < main.rindex("#ifdef __cplusplus")
    assert main.index('extern "C" {') < main.index('#include "irm_hip_video.h"')
    text = open(os.path.join(ROOT, "include", "irm_hip_video.h")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    assert "ws_words >=" in text, "the header states the workspace minimum"
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_VIDEO)
    others = (_hip.SIGNATURES, _hip.SIGNATURES_HALF, _hip.SIGNATURES_FRAMES, _hip.SIGNATURES_GRAM, _hip.SIGNATURES_YUV,
              _hip.SIGNATURES_INCEPTION, _hip.SIGNATURES_METRICS, _hip.SIGNATURES_NOISE, _hip.SIGNATURES_LPIPS)
    assert not set(_hip.SIGNATURES_VIDEO) & set().union(*others)
    for hdr, table in (("irm_hip_yuv.h", _hip.SIGNATURES_YUV), ("irm_hip_metrics.h", _hip.SIGNATURES_METRICS)):
        old = open(os.path.join(ROOT, "include", hdr)).read()
        assert len(re.findall(r"^\s*int\s+(irm_\w+)\s*\(", old, flags=re.M)) == len(table) == 2
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b"}
    _lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_VIDEO[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_every_video_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_VIDEO: each
    symbol is called by name in a test_guard_bands_* function of tests/test_gpu_video_formats.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_video_formats.py")) as f:
        text = f.read()
    reached = set()
    for body in re.split(r"^def ", text, flags=re.M):
        if body.startswith("test_guard_bands_"):
            reached |= set(re.findall(r'"(irm_\w+)"', body))
    missing = sorted(set(_hip.SIGNATURES_VIDEO) - reached)
    assert not missing, f"video entry points without a guard-band case: {missing}"


def test_conversions_refuse_bad_arguments_before_any_launch():
    """Each class of bad argument on its own, everything else valid.  The pointers are never followed: nothing is
    launched without a device, and a launch would return IRM_ELAUNCH, not IRM_EINVAL."""
    lib = _lib()
    good = dict(y=4096, u=8192, v=8194, step=2, pitch_y=16, pitch_c=16, sw=2, sh=1, depth=10, upper=1, matrix=1, full=0,
                siting=0, luma=0, H=7, W=16, rgb=1 << 20)
    bad = [dict(sw=1, sh=2), dict(sw=3, sh=1), dict(sw=0, sh=0), dict(sw=2, sh=3),        # unknown (sub_w, sub_h)
           dict(depth=9), dict(depth=14), dict(depth=16), dict(depth=8, upper=1),
           dict(W=15), dict(sh=2, H=7),                                                   # odd W at 4:2:2, odd H at 4:2:0
           dict(pitch_c=15), dict(sw=1, sh=1, pitch_c=31), dict(step=1, pitch_c=7),       # one below the minimum
           dict(pitch_y=15), dict(y=4097), dict(u=8193, v=8195), dict(depth=12, v=8193),  # misaligned 16-bit pointers
           dict(y=0), dict(u=0), dict(v=0), dict(rgb=0), dict(rgb=(1 << 20) + 2), dict(step=0), dict(step=3),
           dict(upper=2), dict(matrix=2), dict(full=2), dict(siting=-1), dict(siting=2), dict(luma=2), dict(H=0),
           dict(W=-2), dict(H=(1 << 20) + 1)]
    for change in bad:
        a = dict(good, **change)
        planes = (a["y"], a["u"], a["v"], a["step"], a["pitch_y"], a["pitch_c"], a["sw"], a["sh"], a["depth"],
                  a["upper"], a["matrix"], a["full"], a["siting"], a["luma"], a["H"], a["W"])
        assert lib.irm_yuv_to_rgb_f32(*planes, a["rgb"], None) == -1, change
        assert lib.irm_rgb_f32_to_yuv(a["rgb"], *planes, None) == -1, change
    # the five old entry points keep refusing depth 12
    p420 = (4096, 8192, 8194, 2, 16, 16, 12, 1, 1, 0, 0, 0, 8, 16)
    assert lib.irm_yuv420_to_rgb_f32(*p420, 1 << 20, None) == -1
    assert lib.irm_rgb_f32_to_yuv420(1 << 20, *p420, None) == -1


def test_metrics_entry_refuses_bad_arguments_before_any_launch():
    f = _lib().irm_yuv_metrics
    good = dict(y=4096, u=8192, v=8194, step=2, pitch_y=32, pitch_c=32, ty=12288, tu=16384, tv=16386, tstep=2,
                tpitch_y=32, tpitch_c=32, sw=2, sh=1, depth=10, upper=1, luma=0, H=7, W=32, sse=1 << 20, ssim=1 << 21,
                ws=1 << 22, words=None)

    def rc(**change):
        a = dict(good, **change)
        if a["words"] is None:
            t = lambda h, w: -(-(h - 6) // 16) * -(-(w - 6) // 192)        # noqa: E731
            ch, cw = a["H"] // max(a["sh"], 1), a["W"] // max(a["sw"], 1)
            a["words"] = 2 * (t(a["H"], a["W"]) + (0 if a["luma"] else 2 * t(ch, cw))) + a.get("short", 0)
        return f(a["y"], a["u"], a["v"], a["step"], a["pitch_y"], a["pitch_c"], a["ty"], a["tu"], a["tv"], a["tstep"],
                 a["tpitch_y"], a["tpitch_c"], a["sw"], a["sh"], a["depth"], a["upper"], a["luma"], a["H"], a["W"],
                 a["sse"], a["ssim"], a["ws"], a["words"], None)

    bad = [dict(sw=1, sh=2), dict(sw=4, sh=1), dict(depth=9), dict(depth=8, upper=1), dict(upper=2), dict(W=31),
           dict(sh=2, H=15), dict(pitch_c=31), dict(tpitch_c=31), dict(sw=1, pitch_c=63, tpitch_c=64),
           dict(y=4097), dict(tu=16385, tv=16387), dict(depth=12, v=8193),
           dict(W=12), dict(H=6), dict(sh=2, H=12),                        # a chroma plane below 7 x 7
           dict(sw=1, sh=1, H=6, W=7, pitch_c=14, tpitch_c=14), dict(sw=1, sh=1, H=7, W=6, pitch_c=14, tpitch_c=14),
           dict(luma=1, H=6), dict(luma=1, W=6), dict(short=-1), dict(tstep=1), dict(step=3, tstep=3), dict(luma=2),
           dict(y=0), dict(u=0), dict(tv=0), dict(sse=0), dict(ssim=0), dict(ws=0), dict(sse=(1 << 20) + 4), dict(H=0)]
    for change in bad:
        assert rc(**change) == -1, change
    # the old entry keeps refusing depth 12
    old = _hip.load().irm_yuv420_metrics
    assert old(4096, 8192, 8194, 2, 32, 32, 12288, 16384, 16386, 2, 32, 32, 12, 0, 0, 14, 32, 1 << 20, 1 << 21, 1 << 22,
               6, None) == -1


# --------------------------------------------------------------------------- anchors worked out by hand
#: 12-bit limited range: y0 = 256, yr = 3504, c0 = 2048, cr = 3584.  White Y = 256 + 3504 = 3760, black 256, both with
#: neutral chroma 2048.  BT.601 red: Y = 256 + 3504 x 0.299 = 1303.70 -> 1304; Cb = -0.299 / 1.772,
#: U = 2048 - 3584 x 0.299 / 1.772 = 1443.25 -> 1443; Cr = 0.701 / 1.402 = 1/2, V = 2048 + 1792 = 3840.
ANCHORS12 = {(1, 1, 1): (3760, 2048, 2048), (0, 0, 0): (256, 2048, 2048), (1, 0, 0): (1304, 1443, 3840)}


@pytest.mark.parametrize("fn", [fm.to_yuv, yuv.rgb_to_yuv_host], ids=["model", "host"])
@pytest.mark.parametrize("fmt,h,w", [("i444p12", 1, 1), ("p412", 1, 1), ("i422p12", 3, 6), ("p212", 3, 6)])
def test_known_12_bit_codes(fmt, h, w, fn):
    for siting in SITINGS:
        for colour, want in ANCHORS12.items():
            rgb = np.broadcast_to(np.array(colour, np.float32), (h, w, 3)).copy()
            planes = fn(rgb, fmt, "bt601", False, siting)
            for got, code in zip(fm.codes_of(planes, fmt), want):
                assert (got == code).all(), (fmt, colour, got, code)
            assert all(p.dtype == np.uint16 for p in planes)
            if fmt.startswith("p"):
                assert all(int((p & 15).max()) == 0 for p in planes), "stored << 4"
            else:
                assert all(int(p.max()) <= 4095 for p in planes), "the code is the word"


@pytest.mark.parametrize("fn", [fm.to_rgb, yuv.yuv_to_rgb_host], ids=["model", "host"])
@pytest.mark.parametrize("fmt", GRID)
def test_white_and_black_decode_exactly(fmt, fn):
    sw, sh, _, depth, _ = fm.LAYOUTS[fmt]
    k = 1 << (depth - 8)
    h, w = 2 * sh, 3 * sw
    for matrix, siting in itertools.product(MATRICES, SITINGS):
        for codes, value in (((235, 128, 128), 1.0), ((16, 128, 128), 0.0)):
            y, u, v = (np.full(s[:2], c * k, np.int64) for s, c in zip(((h, w), (h // sh, w // sw), (h // sh, w // sw)), codes))
            planes = fm.planes_of(y, u, v, fmt)
            rgb = fn(planes, fmt, matrix, False, siting)
            assert rgb.dtype == np.float32 and rgb.shape == (h, w, 3) and (rgb == np.float32(value)).all()
            luma = fn(planes, fmt, matrix, False, siting, True)
            assert luma.shape == (h, w, 1) and (luma == np.float32(value)).all()


# --------------------------------------------------------------------------- up-sampling weights
@pytest.mark.parametrize("fn", ["model", "host"])
def test_422_upsampling_weights_of_an_impulse(fn):
    """A row of three chroma samples under six luma columns, in sixteenths.  "left": sample i lies on column 2 i - the
    sample itself there, half of it on the odd columns beside it; the last odd column takes its right neighbour from the
    clamped edge and so is the last sample whole.  "center": sample i lies midway between columns 2 i and 2 i + 1 -
    3/4 on those two, 1/4 on the next column outwards; at the edges the quarter from outside comes from the edge sample."""
    up = (lambda c, s: fm.upsample16(c, "i422", s)) if fn == "model" else (lambda c, s: yuv._upsample16_of(c, "i422", s))
    want = {"left": ([16, 8, 0, 0, 0, 0], [0, 8, 16, 8, 0, 0], [0, 0, 0, 8, 16, 16]),
            "center": ([16, 12, 4, 0, 0, 0], [0, 4, 12, 12, 4, 0], [0, 0, 0, 4, 12, 16])}
    for siting, rows in want.items():
        for i, row in enumerate(rows):
            c = np.zeros((2, 3), np.int64)
            c[1, i] = 1
            got = up(c, siting)
            assert got.shape == (2, 6) and got[0].tolist() == [0] * 6 and got[1].tolist() == row, (siting, i, got)
        assert sum(np.array(r) for r in rows).tolist() == [16] * 6          # the weights of a column sum to one


@pytest.mark.parametrize("fmt", ["i444", "nv24", "i444p10", "p410", "i444p12", "p412"])
def test_444_is_the_identity_on_in_gamut_codes(fmt):
    """Codes made from RGB in [0.05, 0.95] come back unchanged from codes -> RGB -> codes: no resampling, and the
    float32 error (2^-19 of a range of at most 4095) is far below half a code."""
    rng = np.random.default_rng(SEED)
    rgb = rng.uniform(0.05, 0.95, (5, 7, 3)).astype(np.float32)
    for matrix, full in itertools.product(MATRICES, (False, True)):
        planes = yuv.rgb_to_yuv_host(rgb, fmt, matrix, full, "center")
        back = yuv.rgb_to_yuv_host(yuv.yuv_to_rgb_host(planes, fmt, matrix, full, "left"), fmt, matrix, full, "left")
        for a, b in zip(planes, back):
            assert np.array_equal(a, b), (fmt, matrix, full)
    assert np.array_equal(fm.upsample16(np.arange(6).reshape(2, 3), fmt, "left"), 16 * np.arange(6).reshape(2, 3))


# --------------------------------------------------------------------------- float32 model vs float64 model
def test_float32_model_against_float64_to_rgb():
    """About eight float32 operations on magnitudes below 2.2, each off by at most 2^-24 of its result: 2^-19."""
    rng = np.random.default_rng(SEED)
    for fmt, matrix, full, siting in itertools.product(GRID, MATRICES, (False, True), SITINGS):
        planes = fm.random_planes(rng, fmt, 6, 10)
        for luma_only in (False, True):
            a = fm.to_rgb(planes, fmt, matrix, full, siting, luma_only)
            b = fm.to_rgb(planes, fmt, matrix, full, siting, luma_only, ft=np.float64)
            assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape
            err = float(np.abs(a.astype(np.float64) - b).max())
            assert err <= 2.0 ** -19, (fmt, matrix, full, siting, luma_only, err)
            assert a.min() >= 0.0 and a.max() <= 1.0


def test_float32_model_against_float64_to_yuv():
    """Codes are equal wherever the float64 value before rounding is further than the band from a half-integer, at most
    1 apart inside it; the band is 2^-10 code units at depths 8 and 10 and 2^-9 at depth 12 (the float32 error of a
    value of at most 4095 after about eight operations: 8 x 2^-13 x 2^-... = 2^-9 at most; the largest distance seen at
    12 bit is 5.0e-4), and may hold at most 1 % of the samples (64 x 96 uniform samples in [-0.1, 1.1], seed SEED: 0.30
    to 0.50 %)."""
    for fmt, sitings in (("i444", ("left",)), ("i444p10", ("left",)), ("i444p12", ("left",)), ("p412", ("left",)),
                         ("i422", SITINGS), ("p210", SITINGS), ("i422p12", SITINGS), ("i420p12", ("left",)),
                         ("i420p10", ("left",)), ("p012", ("left",))):
        band_w = 2.0 ** -9 if fm.LAYOUTS[fmt][3] == 12 else 2.0 ** -10
        rng = np.random.default_rng(SEED)
        in_band = total = 0
        for matrix, full, siting in itertools.product(MATRICES, (False, True), sitings):
            rgb = rng.uniform(-0.1, 1.1, (64, 96, 3)).astype(np.float32)
            for luma_only in (False, True):
                frame = rgb[:, :, :1] if luma_only else rgb
                v64 = fm.to_yuv_values(frame, fmt, matrix, full, siting, luma_only, ft=np.float64)
                p32 = fm.to_yuv(frame, fmt, matrix, full, siting, luma_only)
                p64 = fm.to_yuv(frame, fmt, matrix, full, siting, luma_only, ft=np.float64)
                for v, c32, c64 in zip(v64, fm.codes_of(p32, fmt), fm.codes_of(p64, fmt)):
                    if v is None:
                        continue
                    band = np.abs(v - np.floor(v) - 0.5) <= band_w
                    assert np.array_equal(c32[~band], c64[~band]), (fmt, matrix, full, siting, luma_only)
                    assert int(np.abs(c32 - c64).max()) <= 1
                    in_band += int(band.sum())
                    total += band.size
        assert in_band <= 0.01 * total, (fmt, in_band, total)


# --------------------------------------------------------------------------- the numpy twins of the package
@pytest.mark.parametrize("fmt", GRID)
def test_host_twins_equal_the_float32_model(fmt):
    sw, sh = fm.LAYOUTS[fmt][:2]
    rng = np.random.default_rng(SEED + 1)
    for (h, w), matrix, full, siting in itertools.product(((sh, sw), (3 * sh, 5 * sw), (17 * sh, 35 * sw)), MATRICES,
                                                          (False, True), SITINGS):
        planes = fm.random_planes(rng, fmt, h, w)
        rgb = rng.uniform(-0.25, 1.5, (h, w, 3)).astype(np.float32)
        for luma_only in (False, True):
            a = yuv.yuv_to_rgb_host(planes, fmt, matrix, full, siting, luma_only)
            b = fm.to_rgb(planes, fmt, matrix, full, siting, luma_only)
            assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            frame = np.ascontiguousarray(rgb[:, :, :1]) if luma_only else rgb
            keep = tuple(p.copy() for p in planes)
            got = yuv.rgb_to_yuv_host(frame, fmt, matrix, full, siting, luma_only, out=keep if luma_only else None)
            want = fm.to_yuv(frame, fmt, matrix, full, siting, luma_only, chroma=planes[1:])
            assert len(got) == len(want) == len(planes)
            for g, t in zip(got, want):
                assert g.dtype == t.dtype and g.shape == t.shape and np.array_equal(g, t), (fmt, matrix, full, siting)
    for name in ("yuv_to_rgb_host", "rgb_to_yuv_host", "yuv_to_rgb_device", "rgb_to_yuv_device", "YUV_LAYOUTS"):
        assert getattr(utils, name) is getattr(yuv, name)
    src = open(yuv.__file__).read()
    assert "yuv_formats_model" not in src.replace("tests/yuv_formats_model.py", "") and "import tests" not in src


def test_the_420_functions_keep_their_three_names():
    rgb = np.zeros((4, 4, 3), np.float32)
    for fmt in ("i420p10", "p012", "i422", "i444"):
        planes = tuple(np.zeros(s, fm.dtype_of(fmt)) for s in fm.plane_shapes(4, 4, fmt))
        with pytest.raises(ValueError, match="must be"):
            yuv.yuv420_to_rgb_host(planes, fmt)
        with pytest.raises(ValueError, match="must be"):
            yuv.rgb_to_yuv420_host(rgb, fmt)
        with pytest.raises(ValueError, match="must be"):
            yuv.yuv420_to_rgb_device(tuple(torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p) for p in planes), fmt)
        with pytest.raises(ValueError, match="must be"):
            yuv.rgb_to_yuv420_device(torch.from_numpy(rgb), fmt)


# --------------------------------------------------------------------------- the metrics twin
def test_metrics_twin_on_hand_computable_planes():
    """The target is the prediction plus one code in U only: the mean squared error of U is 1, PSNR-U is
    10 log10(peak^2); Y and V are identical: inf and 1.0.  Every SSIM is metrics.ssim of the codes."""
    rng = np.random.default_rng(SEED + 2)
    for fmt, h, w in (("i422", 9, 16), ("p210", 7, 14), ("i444p12", 7, 9), ("nv24", 8, 7), ("p412", 9, 8)):
        sw, sh, _, depth, _ = fm.LAYOUTS[fmt]
        peak = 2 ** depth - 1
        y = rng.integers(0, peak + 1, (h, w))
        u, v = (rng.integers(0, peak, (h // sh, w // sw)) for _ in range(2))
        pred, target = fm.planes_of(y, u, v, fmt), fm.planes_of(y, u + 1, v, fmt)
        m = yuv.calculate_metrics_yuv(pred, target, fmt)
        assert abs(m.psnr_u - 10 * math.log10(float(peak) ** 2)) <= 1e-12
        assert m.psnr_y == m.psnr_v == float("inf") and m.ssim_y == m.ssim_v == 1.0
        assert abs(m.ssim_u - metrics.ssim(u + 1, u, peak)) <= 1e-12 and 0.9 < m.ssim_u < 1.0
        same = yuv.calculate_metrics_yuv(pred, pred, fmt)
        assert same == (float("inf"), 1.0) * 3
        lo = yuv.calculate_metrics_yuv(pred, target, fmt, luma_only=True)
        assert lo[:2] == m[:2] and all(math.isnan(x) for x in lo[2:])
    # upper-bits formats ignore the low bits of their words
    pred = fm.random_planes(rng, "p212", 8, 16)
    noisy = tuple(p | rng.integers(0, 16, p.shape).astype(np.uint16) for p in pred)
    target = fm.random_planes(rng, "p212", 8, 16)
    assert yuv.calculate_metrics_yuv(noisy, target, "p212") == yuv.calculate_metrics_yuv(pred, target, "p212")


def test_metric_sizes_before_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library must not be called")
    monkeypatch.setattr(_hip, "call", boom)
    z = lambda fmt, h, w: tuple(np.zeros(s, fm.dtype_of(fmt)) for s in fm.plane_shapes(h, w, fmt))    # noqa: E731
    for fmt, h, w in (("i422", 6, 14), ("i422", 7, 12), ("i444", 6, 7), ("i444", 7, 6), ("nv16", 7, 12)):
        with pytest.raises(ValueError, match="at least 7"):
            yuv.calculate_metrics_yuv(z(fmt, h, w), z(fmt, h, w), fmt)
        t = tuple(torch.from_numpy(p) for p in z(fmt, h, w))
        with pytest.raises(ValueError, match="at least 7"):
            yuv.frame_metrics_yuv_device(t, t, fmt)
    with pytest.raises(ValueError, match="at least 14"):
        yuv.calculate_metrics_yuv(z("i420p12", 12, 20), z("i420p12", 12, 20), "i420p12")
    t = tuple(torch.from_numpy(p) for p in z("i444", 7, 7))
    with pytest.raises(ValueError, match="GPU"):
        yuv.frame_metrics_yuv_device(t, t, "i444")                  # valid CPU tensors: there is no CPU fallback


# --------------------------------------------------------------------------- the callers
class Never(torch.nn.Module):
    def forward(self, t):
        raise AssertionError("the model must not run")


def test_whole_call_takes_the_new_names_without_the_feature_it_raises_value_error():
    """utils.run_model_inference_yuv(..., fmt="p210") raised ValueError before the grid: with it the arguments are
    valid and, without a GPU, the call reaches the 'no CPU fallback' error."""
    m = Never()
    for fmt, h, w in (("p210", 5, 6), ("i444p10", 5, 7), ("i420p12", 4, 6), ("nv16", 3, 2)):
        planes = tuple(np.zeros(s, fm.dtype_of(fmt)) for s in fm.plane_shapes(h, w, fmt))
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            utils.run_model_inference_yuv(m, planes, CPU, fmt=fmt, patch_size=32)
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            list(stream.run_model_inference_stream(m, [planes], CPU, fmt=fmt, patch_size=32, patch_overlap=8))
    # the refusals of the new names: sizes that do not divide, wrong dtype, wrong chroma shape
    y = np.zeros((4, 5), np.uint16)
    with pytest.raises(ValueError, match="even"):
        utils.run_model_inference_yuv(m, (y, np.zeros((4, 2, 2), np.uint16)), CPU, fmt="p210", patch_size=32)
    with pytest.raises(ValueError, match="even"):
        utils.run_model_inference_yuv(m, (np.zeros((3, 4), np.uint16),) * 3, CPU, fmt="i420p12", patch_size=32)
    with pytest.raises(ValueError):
        utils.run_model_inference_yuv(m, (y.astype(np.uint8), np.zeros((4, 5, 2), np.uint8)), CPU, fmt="p410", patch_size=32)
    with pytest.raises(ValueError):
        utils.run_model_inference_yuv(m, (y, np.zeros((2, 5, 2), np.uint16)), CPU, fmt="p410", patch_size=32)
    for bad in ("yv12", "nv21", "i440", "p016"):
        with pytest.raises(ValueError, match="must be"):
            utils.run_model_inference_yuv(m, (y, y, y), CPU, fmt=bad, patch_size=32)
    with pytest.raises(ValueError, match="must be"):
        utils.run_model_inference_yuv(m, (y, y, y), CPU, fmt="i444p10", matrix="bt2020", patch_size=32)
    sr = Never()
    sr.upscale = 2
    with pytest.raises(ValueError, match="luma_only"):
        utils.run_model_inference_yuv(sr, (y, y, y), CPU, fmt="i444p10", luma_only=True)
    kw = dict(task="denoising", subtask="gaussian", dataset="d", model_name="m")
    row = harness.evaluate_yuv(m, iter([]), CPU, dict(patch_size=32, patch_overlap=8), fmt="i422p10", **kw)
    assert math.isnan(row["PSNR"]) and row["Failed"] == []
