"""YUV 4:2:0 frames, the part that needs no GPU: the C ABI of include/irm_hip_yuv.h against _hip.SIGNATURES_YUV, known
code triples of the two matrices, the float32 model of tests/yuv_model.py against its float64 twin, the numpy functions
of irm_amd/yuv.py against the float32 model bit for bit, the up-sampling weights, and argument validation before any
GPU call."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import yuv_model
from irm_amd import _hip, deblurganv2, utils, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_yuv420_to_rgb_f32", "irm_rgb_f32_to_yuv420"]
FORMATS, MATRICES, SITINGS = ("i420", "nv12", "p010"), ("bt601", "bt709"), ("left", "center")
CPU = torch.device("cpu")
#: the seed of every random frame below
SEED = 20


def random_planes(rng, fmt, h, w):
    top, shift, dt = (1024, 6, np.uint16) if fmt == "p010" else (256, 0, np.uint8)
    y = (rng.integers(0, top, (h, w)) << shift).astype(dt)
    if fmt == "i420":
        return (y, (rng.integers(0, top, (h // 2, w // 2)) << shift).astype(dt),
                (rng.integers(0, top, (h // 2, w // 2)) << shift).astype(dt))
    return y, (rng.integers(0, top, (h // 2, w // 2, 2)) << shift).astype(dt)


def flat_planes(fmt, h, w, yuv_codes):
    y, u, v = (np.full(s, c, np.int64) for s, c in zip(((h, w), (h // 2, w // 2), (h // 2, w // 2)), yuv_codes))
    return yuv_model.planes_of(y, u, v, fmt)


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_two_symbols():
    """The YUV entry points have a header of their own, include/irm_hip_yuv.h, which irm_hip.h includes inside its
    extern "C" block after irm_hip_gram.h, and a table of their own, _hip.SIGNATURES_YUV, disjoint from the other four:
    header and table match one to one, the library exports each symbol, load() binds it, and each one returns
    IRM_EINVAL for null pointers and zero sizes before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_gram.h"') < main.index('#include "irm_hip_yuv.h"') < main.rindex("#ifdef __cplusplus")
    text = open(os.path.join(ROOT, "include", "irm_hip_yuv.h")).read()
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_YUV)
    assert not set(_hip.SIGNATURES_YUV) & (set(_hip.SIGNATURES) | set(_hip.SIGNATURES_HALF) | set(_hip.SIGNATURES_FRAMES)
                                           | set(_hip.SIGNATURES_GRAM))
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b"}
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_YUV[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """Each class of bad argument on its own, everything else valid (the pointers are never followed: nothing is
    launched without a device, and a launch would return IRM_ELAUNCH, not IRM_EINVAL)."""
    lib = _hip.load()
    # y, u, v, step, pitch_y, pitch_c, depth, upper, matrix, full, siting, luma_only, H, W, rgb
    good = dict(y=4096, u=8192, v=8193, step=2, pitch_y=16, pitch_c=16, depth=8, upper=0, matrix=1, full=0, siting=0,
                luma=0, H=8, W=16, rgb=1 << 20)
    bad = [dict(y=0), dict(u=0), dict(v=0), dict(rgb=0), dict(rgb=(1 << 20) + 2), dict(step=0), dict(step=3),
           dict(pitch_y=15), dict(pitch_c=15), dict(depth=12), dict(depth=8, upper=1), dict(upper=2), dict(matrix=2),
           dict(full=2), dict(siting=-1), dict(luma=2), dict(H=7), dict(W=15), dict(H=0), dict(W=-2),
           dict(depth=10, y=4097), dict(depth=10, u=8191, v=8193)]
    for change in bad:
        a = dict(good, **change)
        planes = (a["y"], a["u"], a["v"], a["step"], a["pitch_y"], a["pitch_c"], a["depth"], a["upper"], a["matrix"],
                  a["full"], a["siting"], a["luma"], a["H"], a["W"])
        assert lib.irm_yuv420_to_rgb_f32(*planes, a["rgb"], None) == -1, change
        assert lib.irm_rgb_f32_to_yuv420(a["rgb"], *planes, None) == -1, change


def test_every_yuv_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_YUV: each
    symbol is called by name in a test_guard_bands_* function of tests/test_gpu_yuv.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_yuv.py")) as f:
        text = f.read()
    reached = set()
    for body in re.split(r"^def ", text, flags=re.M):
        if body.startswith("test_guard_bands_"):
            reached |= set(re.findall(r'"(irm_\w+)"', body))
    missing = sorted(set(_hip.SIGNATURES_YUV) - reached)
    assert not missing, f"YUV entry points without a guard-band case: {missing}"


def test_kernel_source_keeps_the_repository_rules():
    """No preprocessor conditional in the new kernel file and header, the arithmetic spelled with the correctly rounded
    intrinsics (a contracted multiply-add would break the bit-exact match with the float32 model), no LDS, no atomics."""
    src = open(os.path.join(os.path.dirname(_hip.LIB_PATH), "csrc", "yuv.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "irm_hip_yuv.h")).read()
    for text in (src, hdr):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    for word in ("__fdiv_rn(__fsub_rn(", "__fadd_rn(yp[j], __fmul_rn(k.r_cr, cr))",
                 "__fsub_rn(__fsub_rn(yp[j], __fmul_rn(k.g_cb, cb)), __fmul_rn(k.g_cr, cr))",
                 "__fadd_rn(__fadd_rn(__fmul_rn(k.kr, R), __fmul_rn(k.kg, G)), __fmul_rn(k.kb, B))",
                 "__fadd_rn(off, __fmul_rn(range, v))"):
        assert word in src, word
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code.lower() and "__shared__" not in code


# --------------------------------------------------------------------------- anchors from the standards
#: limited-range codes of the primaries, worked out by hand from Kr, Kb and the ranges, not taken from the code:
#: (matrix, colour) -> (8-bit codes, 10-bit codes).  The 10-bit ranges are the 8-bit ones times four, so a code that
#: is exact at 8 bits (white, black, the 240 of a saturated chroma) is four times that; the others are rounded at 10-bit
#: precision (red under BT.601: 64 + 876 x 0.299 = 325.92 -> 326, not 4 x 81) and lie within 2 of four times the 8-bit
#: code.
ANCHORS = {("bt601", (1, 0, 0)): ((81, 90, 240), (326, 361, 960)),
           ("bt601", (0, 1, 0)): ((145, 54, 34), (578, 215, 137)),
           ("bt601", (0, 0, 1)): ((41, 240, 110), (164, 960, 439)),
           ("bt709", (1, 0, 0)): ((63, 102, 240), (250, 409, 960)),
           ("bt601", (1, 1, 1)): ((235, 128, 128), (940, 512, 512)), ("bt709", (1, 1, 1)): ((235, 128, 128), (940, 512, 512)),
           ("bt601", (0, 0, 0)): ((16, 128, 128), (64, 512, 512)), ("bt709", (0, 0, 0)): ((16, 128, 128), (64, 512, 512))}


@pytest.mark.parametrize("fn", [yuv_model.to_yuv, yuv.rgb_to_yuv420_host], ids=["model", "host"])
@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_known_codes_of_flat_frames(fmt, siting, fn):
    for (matrix, colour), (want8, want10) in ANCHORS.items():
        assert all(abs(t - 4 * e) <= 2 for e, t in zip(want8, want10))
        if sum(colour) in (0, 3):
            assert want10 == tuple(4 * e for e in want8)      # white and black: the same codes times four
        rgb = np.broadcast_to(np.array(colour, np.float32), (4, 4, 3)).copy()
        planes = fn(rgb, fmt, matrix, False, siting)
        for got, code in zip(yuv_model.codes_of(planes, fmt), want10 if fmt == "p010" else want8):
            assert (got == code).all(), (matrix, colour, got, code)
        if fmt == "p010":
            assert all(p.dtype == np.uint16 and int((p & 63).max()) == 0 for p in planes), "stored << 6"


@pytest.mark.parametrize("fn", [yuv_model.to_rgb, yuv.yuv420_to_rgb_host], ids=["model", "host"])
@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_white_and_black_decode_exactly(fmt, matrix, siting, fn):
    scale = 4 if fmt == "p010" else 1
    for codes, value in (((235, 128, 128), 1.0), ((16, 128, 128), 0.0)):
        rgb = fn(flat_planes(fmt, 4, 4, [c * scale for c in codes]), fmt, matrix, False, siting)
        assert rgb.dtype == np.float32 and rgb.shape == (4, 4, 3) and (rgb == np.float32(value)).all()
        luma = fn(flat_planes(fmt, 4, 4, [c * scale for c in codes]), fmt, matrix, False, siting, True)
        assert luma.shape == (4, 4, 1) and (luma == np.float32(value)).all()


# --------------------------------------------------------------------------- float32 model vs float64 model
EVERY = list(itertools.product(FORMATS, MATRICES, (False, True), SITINGS))


@pytest.mark.parametrize("h,w", [(6, 10), (34, 70)])
def test_float32_model_against_float64_to_rgb(h, w):
    """About eight float32 operations on magnitudes below 2.2, each off by at most 2^-24 of its result: 2^-19."""
    rng = np.random.default_rng(SEED)
    for fmt, matrix, full, siting in EVERY:
        planes = random_planes(rng, fmt, h, w)
        for luma_only in (False, True):
            a = yuv_model.to_rgb(planes, fmt, matrix, full, siting, luma_only)
            b = yuv_model.to_rgb(planes, fmt, matrix, full, siting, luma_only, ft=np.float64)
            assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape
            err = float(np.abs(a.astype(np.float64) - b).max())
            assert err <= 2.0 ** -19, (fmt, matrix, full, siting, luma_only, err)
            assert a.min() >= 0.0 and a.max() <= 1.0


@pytest.mark.parametrize("h,w", [(6, 10), (34, 70)])
def test_float32_model_against_float64_to_yuv(h, w):
    """Codes are equal wherever the float64 value before rounding is further than 2^-10 code units from a half-integer
    (wider than the float32 error of a value of at most 1023 after about eight operations: 8 x 2^-15), differ by at most
    1 elsewhere, and that band may hold at most 1 % of the samples (uniform inputs, seed SEED: about 0.2 %)."""
    rng = np.random.default_rng(SEED)
    in_band = total = 0
    for fmt, matrix, full, siting in EVERY:
        rgb = rng.random((h, w, 3), dtype=np.float32)
        for luma_only in (False, True):
            frame = rgb[:, :, :1] if luma_only else rgb
            v64 = yuv_model.to_yuv_values(frame, fmt, matrix, full, siting, luma_only, ft=np.float64)
            p32 = yuv_model.to_yuv(frame, fmt, matrix, full, siting, luma_only)
            p64 = yuv_model.to_yuv(frame, fmt, matrix, full, siting, luma_only, ft=np.float64)
            for v, c32, c64 in zip(v64, yuv_model.codes_of(p32, fmt), yuv_model.codes_of(p64, fmt)):
                if v is None:
                    continue
                band = np.abs(v - np.floor(v) - 0.5) <= 2.0 ** -10
                assert np.array_equal(c32[~band], c64[~band]), (fmt, matrix, full, siting, luma_only)
                assert int(np.abs(c32 - c64).max()) <= 1
                in_band += int(band.sum())
                total += band.size
    assert in_band <= 0.01 * total, (in_band, total)


# --------------------------------------------------------------------------- the numpy twins of the package
@pytest.mark.parametrize("h,w", [(2, 2), (6, 10), (34, 70)])
def test_host_twins_equal_the_float32_model(h, w):
    rng = np.random.default_rng(SEED + 1)
    for fmt, matrix, full, siting in EVERY:
        planes = random_planes(rng, fmt, h, w)
        rgb = rng.uniform(-0.25, 1.5, (h, w, 3)).astype(np.float32)
        for luma_only in (False, True):
            a = yuv.yuv420_to_rgb_host(planes, fmt, matrix, full, siting, luma_only)
            b = yuv_model.to_rgb(planes, fmt, matrix, full, siting, luma_only)
            assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            frame = np.ascontiguousarray(rgb[:, :, :1]) if luma_only else rgb
            keep = tuple(p.copy() for p in planes)
            got = yuv.rgb_to_yuv420_host(frame, fmt, matrix, full, siting, luma_only, out=keep if luma_only else None)
            want = yuv_model.to_yuv(frame, fmt, matrix, full, siting, luma_only, chroma=planes[1:])
            assert len(got) == len(want) == len(planes)
            for g, t in zip(got, want):
                assert g.dtype == t.dtype and np.array_equal(g, t), (fmt, matrix, full, siting, luma_only)
    assert utils.yuv420_to_rgb_host is yuv.yuv420_to_rgb_host and utils.rgb_to_yuv420_host is yuv.rgb_to_yuv420_host
    assert utils.yuv420_to_rgb_device is yuv.yuv420_to_rgb_device and utils.rgb_to_yuv420_device is yuv.rgb_to_yuv420_device
    src = open(yuv.__file__).read()
    assert "yuv_model" not in src.replace("tests/yuv_model.py", "") and "import tests" not in src


# --------------------------------------------------------------------------- up-sampling weights
#: an axis of two chroma samples under four luma positions: the weight, in quarters, of sample 0 and of sample 1 at
#: each position.  Midway ("center", and the vertical axis of both sitings): positions 0 and 3 would take a quarter
#: from outside the frame and take it from the edge sample instead.  Co-sited ("left", horizontal): position 0 is
#: sample 0, 1 the mean of the two, 2 is sample 1, 3 the mean of sample 1 and the clamped one past it.
MIDWAY = ([4, 3, 1, 0], [0, 1, 3, 4])
COSITED = ([4, 2, 0, 0], [0, 2, 4, 4])


@pytest.mark.parametrize("fn", ["model", "host"])
@pytest.mark.parametrize("siting", SITINGS)
def test_upsampling_weights_of_an_impulse(siting, fn):
    """A 4 x 4 frame has 2 x 2 chroma samples, every one at an edge.  A one in one of them spreads, in sixteenths, with
    the outer product of the per-axis weights above."""
    up = yuv_model.upsample16 if fn == "model" else (lambda c, s: yuv._upsample16_of(c, "i420", s))
    horizontal = MIDWAY if siting == "center" else COSITED
    for cy in range(2):
        for cx in range(2):
            c = np.zeros((2, 2), np.int64)
            c[cy, cx] = 1
            want = np.outer(MIDWAY[cy], horizontal[cx])
            assert np.array_equal(up(c, siting), want), (siting, cy, cx)
    # spelled out once: left siting, the sample at chroma (0, 0)
    if siting == "left":
        c = np.zeros((2, 2), np.int64)
        c[0, 0] = 1
        assert up(c, "left").tolist() == [[16, 8, 0, 0], [12, 6, 0, 0], [4, 2, 0, 0], [0, 0, 0, 0]]
    else:
        c = np.zeros((2, 2), np.int64)
        c[0, 0] = 1
        assert up(c, "center").tolist() == [[16, 12, 4, 0], [12, 9, 3, 0], [4, 3, 1, 0], [0, 0, 0, 0]]


# --------------------------------------------------------------------------- argument errors before any GPU call
class Never(torch.nn.Module):
    def forward(self, t):
        raise AssertionError("the model must not run")


def test_argument_errors_before_any_gpu_call():
    y, uv = np.zeros((4, 6), np.uint8), np.zeros((2, 3, 2), np.uint8)
    u = np.zeros((2, 3), np.uint8)
    rgb = np.zeros((4, 6, 3), np.float32)
    ty, tuv, tu, trgb = (torch.from_numpy(a) for a in (y, uv, u, rgb))
    m = Never()

    def every(planes, fmt, frame=None, **kw):
        """The same bad call through the host twin, the device call and the whole call."""
        torch_planes = tuple(torch.from_numpy(p) if isinstance(p, np.ndarray) else p for p in planes) \
            if isinstance(planes, tuple) else planes
        with pytest.raises(ValueError):
            yuv.yuv420_to_rgb_host(planes, fmt, **kw)
        with pytest.raises(ValueError):
            yuv.yuv420_to_rgb_device(torch_planes, fmt, **kw)
        with pytest.raises(ValueError):
            utils.run_model_inference_yuv(m, planes, CPU, fmt=fmt, patch_size=32, **kw)
    # odd sizes
    every((np.zeros((3, 6), np.uint8), np.zeros((1, 3, 2), np.uint8)), "nv12")
    every((np.zeros((4, 5), np.uint8), np.zeros((2, 2, 2), np.uint8)), "nv12")
    for bad in (np.zeros((3, 6, 3), np.float32), np.zeros((4, 5, 3), np.float32)):
        with pytest.raises(ValueError, match="even"):
            yuv.rgb_to_yuv420_host(bad, "nv12")
        with pytest.raises(ValueError, match="even"):
            yuv.rgb_to_yuv420_device(torch.from_numpy(bad), "nv12")
    # wrong plane shapes, counts and dtypes
    every((y, u), "nv12")
    every((y, uv), "i420")
    every((y, u, u), "nv12")
    every((y, u, np.zeros((2, 4), np.uint8)), "i420")
    every((y[:, :, None], uv), "nv12")
    every((y, uv), "p010")
    every((y.astype(np.uint16), uv.astype(np.uint16)), "nv12")
    every((y.astype(np.float32), uv.astype(np.float32)), "nv12")
    every(y, "nv12")
    every(([[0]], uv), "nv12")
    # unknown names
    every((y, uv), "yv12")
    every((y, uv), "nv12", matrix="bt2020")
    every((y, uv), "nv12", siting="top")
    for fn, frame in ((yuv.rgb_to_yuv420_host, rgb), (yuv.rgb_to_yuv420_device, trgb)):
        for kw in (dict(fmt="nv21"), dict(fmt="nv12", matrix="bt2020"), dict(fmt="nv12", siting="top")):
            with pytest.raises(ValueError, match="must be"):
                fn(frame, **kw)
        with pytest.raises(ValueError, match="float32"):
            fn(frame.astype(np.float64) if isinstance(frame, np.ndarray) else frame.double(), "nv12")
        with pytest.raises(ValueError, match="float32"):
            fn(frame[:, :, :1], "nv12")                                   # three channels unless luma_only
        with pytest.raises(ValueError, match="luma_only"):
            fn(frame[:, :, :1], "nv12", luma_only=True)                   # Y alone needs the frame's planes
    with pytest.raises(ValueError, match="another"):
        yuv.rgb_to_yuv420_host(rgb, "nv12", out=(np.zeros((4, 8), np.uint8), np.zeros((2, 4, 2), np.uint8)))
    # device planes: strides
    wide = torch.zeros(4, 12, dtype=torch.uint8)
    with pytest.raises(ValueError, match="stride"):
        yuv.yuv420_to_rgb_device((wide[:, ::2], tuv), "nv12")
    with pytest.raises(ValueError, match="stride"):
        yuv.yuv420_to_rgb_device((ty, torch.zeros(2, 3, 4, dtype=torch.uint8)[:, :, ::2]), "nv12")
    with pytest.raises(ValueError, match="stride"):
        yuv.yuv420_to_rgb_device((ty, tu, torch.zeros(2, 6, dtype=torch.uint8)[:, ::2]), "i420")
    with pytest.raises(ValueError, match="share"):
        yuv.yuv420_to_rgb_device((ty, tu, torch.zeros(2, 8, dtype=torch.uint8)[:, :3]), "i420")
    # the whole call: the model
    with pytest.raises(ValueError, match="model"):
        utils.run_model_inference_yuv(None, (y, uv), CPU, fmt="nv12")
    with pytest.raises(ValueError, match="DeblurGANv2"):
        utils.run_model_inference_yuv(deblurganv2.FPNMobileNet(), (y, uv), CPU, fmt="nv12")
    sr = Never()
    sr.upscale = 2
    with pytest.raises(ValueError, match="luma_only"):
        utils.run_model_inference_yuv(sr, (y, uv), CPU, fmt="nv12", luma_only=True)
    with pytest.raises(ValueError, match="need_degradation"):
        utils.run_model_inference_yuv(sr, (y, uv), CPU, fmt="nv12", need_degradation=True, noise_level=15)
    # valid arguments, no GPU: there is no CPU fallback
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        utils.run_model_inference_yuv(m, (y, uv), CPU, fmt="nv12", patch_size=32)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        utils.run_model_inference_yuv(sr, (y, u, u), CPU, fmt="i420")
