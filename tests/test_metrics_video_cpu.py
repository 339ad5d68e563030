"""PSNR / SSIM of float32 frames and of YUV 4:2:0 planes, the part that needs no GPU: the C ABI of
include/irm_hip_metrics.h against _hip.SIGNATURES_METRICS, the library's own argument checks (which return before any
HIP call), the Python checks (which raise before the library is touched), the numpy twin calculate_metrics_yuv on planes
whose scores can be worked out by hand, and harness.evaluate_yuv without a frame."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import yuv_model
from irm_amd import _hip, harness, metrics, utils, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_frame_metrics_f32", "irm_yuv420_metrics"]
CPU = torch.device("cpu")
SEED = 23


def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip.load()


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_two_symbols():
    """The entry points have a header of their own, include/irm_hip_metrics.h, which irm_hip.h includes inside its
    extern "C" block after irm_hip_inception.h, and a table of their own, _hip.SIGNATURES_METRICS, disjoint from the
    other six: header and table match one to one, the library exports each symbol, load() binds it, and each one
    returns IRM_EINVAL for null pointers and zero sizes before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_inception.h"') < main.index('#include "irm_hip_metrics.h"') \
        < main.rindex("#ifdef __cplusplus")
    assert main.index('extern "C" {') < main.index('#include "irm_hip_metrics.h"')
    text = open(os.path.join(ROOT, "include", "irm_hip_metrics.h")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    assert "ws_words >=" in text, "the header states the workspace minimum"
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_METRICS)
    others = (_hip.SIGNATURES, _hip.SIGNATURES_HALF, _hip.SIGNATURES_FRAMES, _hip.SIGNATURES_GRAM, _hip.SIGNATURES_YUV,
              _hip.SIGNATURES_INCEPTION)
    assert not set(_hip.SIGNATURES_METRICS) & set().union(*others)
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b", ctypes.c_double: r"^double\b"}
    _lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_METRICS[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_f32_entry_refuses_bad_arguments_before_any_launch():
    """Non-null placeholder pointers that are never followed: every check below fails before a launch (a launch without
    a device would return IRM_ELAUNCH, not IRM_EINVAL)."""
    f = _lib().irm_frame_metrics_f32
    fake = 4096

    def rc(k=1, h=720, w=1280, c=3, data_range=1.0, ws_words=None, pred=fake, target=fake, sse=fake, ssim=fake, ws=fake):
        if ws_words is None:
            ws_words = 2 * k * -(-(h - 6) // 16) * -(-(w - 6) // (192 // max(c, 1)))
        return f(pred, target, k, h, w, c, data_range, sse, ssim, ws, ws_words, None)

    assert rc(ws_words=2 * 45 * 20 - 1) == -1          # 720p RGB needs 2 x 45 x 20 words: one word short
    assert rc(k=3, ws_words=3 * 2 * 45 * 20 - 1) == -1
    assert rc(c=2) == -1 and rc(c=4) == -1
    assert rc(h=6) == -1 and rc(w=6) == -1
    assert rc(k=0) == -1 and rc(k=65536) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(data_range=bad) == -1, bad
    assert rc(h=40000, w=40000) == -1                  # more than 2^31 values in a frame
    for name in ("pred", "target", "sse", "ssim", "ws"):
        assert rc(**{name: 0}) == -1, name
    assert rc(pred=fake + 2) == -1 and rc(sse=fake + 4) == -1


def test_yuv_entry_refuses_bad_arguments_before_any_launch():
    f = _lib().irm_yuv420_metrics
    good = dict(y=4096, u=8192, v=8193, step=2, pitch_y=32, pitch_c=32, ty=12288, tu=16384, tv=16385, tstep=2,
                tpitch_y=32, tpitch_c=32, depth=8, p010=0, luma=0, H=14, W=32, sse=1 << 20, ssim=1 << 21, ws=1 << 22,
                words=None)

    def rc(**change):
        a = dict(good, **change)
        if a["words"] is None:
            t = lambda h, w: -(-(h - 6) // 16) * -(-(w - 6) // 192)        # noqa: E731
            a["words"] = 2 * (t(a["H"], a["W"]) + (0 if a["luma"] else 2 * t(a["H"] // 2, a["W"] // 2))) + a.get("short", 0)
        return f(a["y"], a["u"], a["v"], a["step"], a["pitch_y"], a["pitch_c"], a["ty"], a["tu"], a["tv"], a["tstep"],
                 a["tpitch_y"], a["tpitch_c"], a["depth"], a["p010"], a["luma"], a["H"], a["W"], a["sse"], a["ssim"],
                 a["ws"], a["words"], None)

    bad = [dict(H=15), dict(W=31), dict(H=12, W=14), dict(H=14, W=12), dict(depth=9), dict(depth=12), dict(p010=1),
           dict(p010=2), dict(depth=10, p010=0, y=4097), dict(step=3, tstep=3), dict(step=0, tstep=0), dict(tstep=1),
           dict(pitch_y=31), dict(tpitch_y=31), dict(pitch_c=31), dict(tpitch_c=31), dict(short=-1), dict(luma=2),
           dict(luma=1, H=6, W=8), dict(luma=1, H=8, W=6), dict(y=0), dict(u=0), dict(tv=0), dict(ty=0), dict(sse=0),
           dict(ssim=0), dict(ws=0), dict(H=0), dict(W=-2), dict(H=(1 << 20) + 2),
           # 46 x 400: 3 x 3 luma tiles and 2 x 2 tiles in each chroma plane, 34 words
           dict(H=46, W=400, pitch_y=400, tpitch_y=400, pitch_c=400, tpitch_c=400, words=2 * (9 + 2 * 4) - 1)]
    for change in bad:
        assert rc(**change) == -1, change
    assert rc(luma=1, H=8, W=8, short=-1) == -1         # the luma-only minimum: one tile, two words


# --------------------------------------------------------------------------- Python checks before the library
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library must not be called")
    monkeypatch.setattr(_hip, "call", boom)
    monkeypatch.setattr(_hip, "load", boom)


def test_f32_refusals_raise_before_the_library(no_library):
    a = torch.zeros(16, 16, 3)
    for fn in (lambda p, t, **kw: utils.frame_metrics_f32_device([p], [t], **kw), utils.calculate_metrics_f32_device):
        with pytest.raises(ValueError, match="GPU"):
            fn(a, a.clone())
        with pytest.raises(ValueError, match="torch tensors"):
            fn(a.numpy(), a.numpy())
        with pytest.raises(ValueError, match="differ"):
            fn(a, torch.zeros(16, 17, 3))
        with pytest.raises(ValueError, match="differ"):
            fn(a, a.double())
        with pytest.raises(ValueError, match="float32"):
            fn(a.to(torch.uint8), a.to(torch.uint8))
        with pytest.raises(ValueError, match="float32"):
            fn(a.double(), a.double())
        with pytest.raises(ValueError, match="channels"):
            fn(torch.zeros(16, 16, 2), torch.zeros(16, 16, 2))
        with pytest.raises(ValueError, match="channels"):
            fn(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16, 3))
        for shape in ((6, 40, 3), (40, 6, 1), (6, 6)):
            with pytest.raises(ValueError, match="at least 7"):
                fn(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError, match="same number"):
        utils.frame_metrics_f32_device([a, a], [a])
    with pytest.raises(ValueError, match="same number"):
        utils.frame_metrics_f32_device([], [])
    with pytest.raises(ValueError, match="share"):
        utils.frame_metrics_f32_device([a, a[:8]], [a, a[:8]])
    assert utils.frame_metrics_f32_device is metrics.frame_metrics_f32_device
    assert utils.calculate_metrics_f32_device is metrics.calculate_metrics_f32_device


def test_existing_refusals_are_kept(no_library):
    """The integer entry points still refuse float32 frames, with the words they had."""
    a = torch.zeros(16, 16, 3)
    with pytest.raises(ValueError, match="uint8 or uint16"):
        utils.calculate_metrics_device(a, a.clone())
    with pytest.raises(ValueError, match="uint8 or uint16"):
        utils.frame_metrics_device([a], [a.clone()])


def planes_of(fmt, h, w, rng=None, value=0):
    top, shift, dt = (1024, 6, np.uint16) if fmt == "p010" else (256, 0, np.uint8)
    shapes = yuv.plane_shapes(h, w, fmt)
    if rng is None:
        return tuple(np.full(s, value << shift, dt) for s in shapes)
    return tuple((rng.integers(0, top, s) << shift).astype(dt) for s in shapes)


def test_yuv_refusals_raise_before_the_library(no_library):
    good = planes_of("nv12", 16, 20)
    tgood = tuple(torch.from_numpy(p) for p in good)

    def every(pred, target, fmt, **kw):
        as_t = lambda ps: tuple(torch.from_numpy(p) if isinstance(p, np.ndarray) else p for p in ps) \
            if isinstance(ps, tuple) else ps                                # noqa: E731
        with pytest.raises(ValueError):
            yuv.calculate_metrics_yuv(pred, target, fmt, **kw)
        with pytest.raises(ValueError):
            yuv.frame_metrics_yuv_device(as_t(pred), as_t(target), fmt, **kw)
        with pytest.raises(ValueError):
            yuv.calculate_metrics_yuv_device(as_t(pred), as_t(target), fmt, **kw)
    every(good, good, "yv12")                                               # unknown fmt
    every(good, good, "i420")                                               # wrong plane count
    every(good, good[:1], "nv12")
    every(good, good, "p010")                                               # wrong dtype
    every(good, (good[0], good[1][:, :, 0]), "nv12")                        # wrong chroma shape
    every(good, planes_of("nv12", 16, 22), "nv12")                          # another frame size
    every(good, planes_of("nv12", 18, 20), "nv12")
    every(planes_of("nv12", 12, 20), planes_of("nv12", 12, 20), "nv12")     # below 14 x 14
    every(planes_of("nv12", 20, 12), planes_of("nv12", 20, 12), "nv12")
    every(planes_of("i420", 6, 20), planes_of("i420", 6, 20), "i420", luma_only=True)      # below 8 x 8 with luma_only
    every(good[0], good[0], "nv12")                                         # not a tuple
    with pytest.raises(ValueError, match="at least 14"):
        yuv.calculate_metrics_yuv(planes_of("nv12", 12, 20), planes_of("nv12", 12, 20), "nv12")
    with pytest.raises(ValueError, match="at least 8"):
        yuv.calculate_metrics_yuv(planes_of("nv12", 6, 20), planes_of("nv12", 6, 20), "nv12", luma_only=True)
    # numpy planes to the device call, tensors to the host twin
    with pytest.raises(ValueError):
        yuv.frame_metrics_yuv_device(good, good, "nv12")
    with pytest.raises(ValueError):
        yuv.calculate_metrics_yuv(tgood, tgood, "nv12")
    # valid CPU tensors: there is no CPU fallback
    with pytest.raises(ValueError, match="GPU"):
        yuv.frame_metrics_yuv_device(tgood, tgood, "nv12")
    # a 12 x 20 frame is enough for luma_only on the host
    m = yuv.calculate_metrics_yuv(planes_of("nv12", 12, 20), planes_of("nv12", 12, 20), "nv12", luma_only=True)
    assert m.psnr_y == float("inf") and m.ssim_y == 1.0 and all(math.isnan(v) for v in m[2:])
    for name in ("YuvMetrics", "calculate_metrics_yuv", "frame_metrics_yuv_device", "calculate_metrics_yuv_device"):
        assert getattr(utils, name) is getattr(yuv, name)


# --------------------------------------------------------------------------- the numpy twin
def test_yuv_twin_on_hand_computable_planes():
    """The target is the prediction plus one in Y only: the mean squared error of Y is 1, so PSNR-Y = 10 log10(255^2);
    U and V are identical, PSNR inf and SSIM 1; every SSIM is metrics.ssim of those planes."""
    rng = np.random.default_rng(SEED)
    y = rng.integers(0, 255, (20, 26)).astype(np.uint8)
    u, v = (rng.integers(0, 256, (10, 13)).astype(np.uint8) for _ in range(2))
    m = yuv.calculate_metrics_yuv((y, u, v), (y + 1, u, v), "i420")
    assert isinstance(m, yuv.YuvMetrics) and m._fields == ("psnr_y", "ssim_y", "psnr_u", "ssim_u", "psnr_v", "ssim_v")
    assert abs(m.psnr_y - 10 * math.log10(255.0 ** 2)) <= 1e-12
    assert m.psnr_u == m.psnr_v == float("inf")
    for got, (t, p) in zip((m.ssim_y, m.ssim_u, m.ssim_v), ((y + 1, y), (u, u), (v, v))):
        assert abs(got - metrics.ssim(t.astype(np.int64), p.astype(np.int64), 255)) <= 1e-12
    assert m.ssim_u == m.ssim_v == 1.0 and 0.9 < m.ssim_y < 1.0
    lo = yuv.calculate_metrics_yuv((y, u, v), (y + 1, u, v), "i420", luma_only=True)
    assert lo[:2] == m[:2] and all(math.isnan(x) for x in lo[2:])
    assert yuv.calculate_metrics_yuv((y,), (y + 1,), "i420", luma_only=True)[:2] == m[:2]


def test_yuv_twin_ignores_the_low_bits_of_p010():
    rng = np.random.default_rng(SEED + 1)
    pred, target = planes_of("p010", 16, 18, rng), planes_of("p010", 16, 18, rng)
    noisy = tuple(p | rng.integers(0, 64, p.shape).astype(np.uint16) for p in pred)
    noisy_t = tuple(p | rng.integers(0, 64, p.shape).astype(np.uint16) for p in target)
    assert any((a != b).any() for a, b in zip(noisy, pred))
    assert yuv.calculate_metrics_yuv(noisy, noisy_t, "p010") == yuv.calculate_metrics_yuv(pred, target, "p010")
    # 10-bit peak: a difference of one code in Y
    one = (pred[0] + np.uint16(64) * (pred[0] < (1023 << 6)) - np.uint16(64) * (pred[0] == (1023 << 6)),) + pred[1:]
    assert abs(yuv.calculate_metrics_yuv(pred, one, "p010").psnr_y - 10 * math.log10(1023.0 ** 2)) <= 1e-12


def test_yuv_twin_nv12_and_i420_of_the_same_samples_agree():
    rng = np.random.default_rng(SEED + 2)
    codes = [rng.integers(0, 256, s) for s in ((18, 22), (9, 11), (9, 11))]
    other = [rng.integers(0, 256, s) for s in ((18, 22), (9, 11), (9, 11))]
    a = yuv.calculate_metrics_yuv(yuv_model.planes_of(*codes, "i420"), yuv_model.planes_of(*other, "i420"), "i420")
    b = yuv.calculate_metrics_yuv(yuv_model.planes_of(*codes, "nv12"), yuv_model.planes_of(*other, "nv12"), "nv12")
    assert a == b and all(np.isfinite(a))


# --------------------------------------------------------------------------- coverage rule
def test_every_metrics_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_METRICS: each
    symbol is called by name in a test_guard_bands_* function of tests/test_gpu_metrics_video.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_metrics_video.py")) as f:
        text = f.read()
    reached = set()
    for body in re.split(r"^def ", text, flags=re.M):
        if body.startswith("test_guard_bands_"):
            reached |= set(re.findall(r'"(irm_\w+)"', body))
    missing = sorted(set(_hip.SIGNATURES_METRICS) - reached)
    assert not missing, f"metrics entry points without a guard-band case: {missing}"


def test_kernel_file_keeps_the_repository_rules():
    """No preprocessor conditional and no atomics in the kernel file, numerator and denominator written with the
    rounded intrinsics, and the file built without contraction in both Makefile rules."""
    csrc = os.path.join(os.path.dirname(_hip.LIB_PATH), "csrc")
    src = open(os.path.join(csrc, "metrics_video.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", src, flags=re.M)
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code.lower()
    assert "__dmul_rn(__dadd_rn(" in code and "ssim_reduce_kernel<true>" in code
    make = open(os.path.join(csrc, "Makefile")).read()
    listed = re.search(r"^NO_CONTRACT := (.*)$", make, flags=re.M).group(1).split()
    assert "yuv" in listed and "metrics_video" in listed
    assert "$(if $(filter $(NO_CONTRACT),$(basename $(notdir $1))),-ffp-contract=off)" in make
    assert "$(HIPCC) $(strip $(CXXFLAGS) $(call extra,$<)) -c" in make
    assert "$(HIPCC) $(strip $(ASAN_FLAGS) $(call extra,$<)) -c" in make


# --------------------------------------------------------------------------- harness
class Never(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(5))

    def forward(self, t):
        raise AssertionError("the model must not run")


KW = dict(task="denoising", subtask="gaussian", dataset="d", model_name="m")
CFG = dict(patch_size=32, patch_overlap=8)


def test_evaluate_yuv_argument_errors():
    m = Never()
    with pytest.raises(ValueError, match="metrics"):
        harness.evaluate_yuv(m, iter([]), CPU, CFG, fmt="nv12", metrics="gpu", **KW)
    with pytest.raises(ValueError, match="fmt"):
        harness.evaluate_yuv(m, iter([]), CPU, CFG, fmt="nv21", **KW)
    with pytest.raises(ValueError, match="matrix"):
        harness.evaluate_yuv(m, iter([]), CPU, CFG, fmt="nv12", matrix="bt2020", **KW)
    with pytest.raises(ValueError, match="siting"):
        harness.evaluate_yuv(m, iter([]), CPU, CFG, fmt="nv12", siting="top", **KW)
    with pytest.raises(ValueError, match="patch_config"):
        harness.evaluate_yuv(m, iter([]), CPU, dict(patch_size=32), fmt="nv12", **KW)
    with pytest.raises(TypeError):
        harness.evaluate_yuv(m, iter([]), CPU, CFG, **KW)                   # fmt is required
    # a frame that raises propagates with skip_failed off, and is reported with it on
    bad = [((np.zeros((15, 20), np.uint8), np.zeros((7, 10, 2), np.uint8)),) * 2 + ("odd.yuv",)]
    with pytest.raises(ValueError, match="even"):
        harness.evaluate_yuv(m, iter(bad), CPU, CFG, fmt="nv12", skip_failed=False, **KW)
    row = harness.evaluate_yuv(m, iter(bad), CPU, CFG, fmt="nv12", **KW)
    assert [n for n, _ in row["Failed"]] == ["odd.yuv"] and math.isnan(row["PSNR"])


@pytest.mark.parametrize("metrics_mode", ["device", "host"])
def test_evaluate_yuv_empty_loader_gives_a_nan_row(metrics_mode, tmp_path):
    row = harness.evaluate_yuv(Never(), iter([]), CPU, CFG, fmt="p010", metrics=metrics_mode, **KW)
    assert list(row)[:len(harness.COLUMNS)] == harness.COLUMNS and set(harness.COLUMNS_YUV) <= set(row)
    assert harness.COLUMNS_YUV[:len(harness.COLUMNS)] == harness.COLUMNS
    assert harness.COLUMNS_YUV[len(harness.COLUMNS):] == ["PSNR_U", "PSNR_V", "SSIM_U", "SSIM_V", "Std_PSNR_U",
                                                          "Std_PSNR_V", "Std_SSIM_U", "Std_SSIM_V"]
    for col in harness.COLUMNS_YUV[6:]:
        assert math.isnan(row[col]), col
    assert row["Failed"] == [] and row["Model_Params"] == 5 and row["Task"] == "Denoising"
    import csv
    with open(harness.save_results([row], out_dir=str(tmp_path), columns=harness.COLUMNS_YUV)) as f:
        assert list(csv.DictReader(f).fieldnames) == harness.COLUMNS_YUV


def test_evaluate_keeps_its_refusals_for_mixed_frames(no_library):
    """metrics="device": a float target for an integer prediction, or the reverse, keeps raising."""
    u8, f32 = np.zeros((16, 16, 3), np.uint8), np.zeros((16, 16, 3), np.float32)
    with pytest.raises(ValueError, match="uint8 or uint16 target"):
        harness._device_metrics(u8, torch.zeros(16, 16, 3, dtype=torch.uint8), f32, CPU, u8)
    with pytest.raises(ValueError, match="differ"):
        harness._device_metrics(f32, torch.zeros(16, 16, 3), u8, CPU, f32)
    with pytest.raises(ValueError, match="uint8 or uint16 target"):
        harness._device_metrics(f32, torch.zeros(16, 16, 3), f32[:8], CPU, f32)       # not the prediction's shape
    with pytest.raises(ValueError, match="GPU"):
        harness._device_metrics(f32, torch.zeros(16, 16, 3), f32, CPU, f32)           # the float route, no GPU
