"""Noise estimation and the sigma-routed call, the part that needs no GPU: the numpy twin against a brute-force
statement and on frames whose integers can be worked out by hand, its accuracy on frames of known noise, SigmaBank and
get_model_bank, the C ABI of include/irm_hip_noise.h against _hip.SIGNATURES_NOISE, the library's own argument checks
(which return before any HIP call) and the Python refusals (which raise before the library is touched)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import noise_model as nm
from irm_amd import _hip, dncnn, harness, noise, rednet, utils, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_noise_hh_stats"]
CPU = torch.device("cpu")


def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip.load()


# --------------------------------------------------------------------------- hand-computed frames
def test_one_block_by_hand():
    img = np.array([[1, 2], [3, 5]], np.uint8)
    stats = utils.noise_stats(img)
    assert stats.dtype == np.int64 and stats.shape == (1, 4) and stats.tolist() == [[1, 1, 0, 1]]
    # m_g = 1 - 0.5 + (0.5 - 0) / 1 = 1
    sigma = utils.noise_sigma_from_stats(stats, 255)
    assert sigma.dtype == np.float64 and sigma.shape == (1,)
    assert sigma[0] == 1 / (2 * 0.6744897501960817) == utils.estimate_noise_sigma(img)
    assert utils.noise_sigma_from_stats(stats, 65535)[0] == 1 / 2 / 0.6744897501960817 * 255 / 65535
    assert utils.noise_stats(img[:, :, None]).tolist() == [[1, 1, 0, 1]]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_degenerate_frames_by_hand(dtype):
    peak = 255 if dtype == np.uint8 else 65535
    frames = nm.degenerate_frames(dtype)
    assert set(frames) == {"flat", "black", "peak", "one_block", "checkerboard", "checkerboard_excluded"}
    for name, (img, kw, want) in frames.items():
        assert utils.noise_stats(img, **kw).tolist() == want, name
        sat = dict(sat_lo=-1, sat_hi=2 * peak + 1) if kw else {}
        assert nm.brute_stats(img, **sat) == want, name
    assert utils.estimate_noise_sigma(frames["flat"][0]) == 0.0
    assert math.isnan(utils.estimate_noise_sigma(frames["black"][0]))
    assert math.isnan(utils.estimate_noise_sigma(frames["peak"][0]))
    assert utils.estimate_noise_sigma(frames["one_block"][0]) == 1 / (2 * nm.MAD_SCALE) * 255 / peak
    checker = utils.noise_stats(frames["checkerboard"][0], exclude_saturated=False)
    assert checker[0, 1] == (510 if dtype == np.uint8 else 131070)
    # the frame's sigma is the mean of its finite channels
    mixed = np.stack([frames["black"][0], frames["one_block"][0], frames["one_block"][0]], axis=2)
    assert utils.estimate_noise_sigma(mixed) == 1 / (2 * nm.MAD_SCALE) * 255 / peak


def test_sigma_from_stats_grouped_median():
    stats = np.array([[[10, 4, 3, 4], [0, 0, 0, 0]], [[9, 0, 0, 6], [7, 2, 3, 1]]], np.int64)
    s = utils.noise_sigma_from_stats(stats, 255)
    assert s.shape == (2, 2)
    assert s[0, 0] == (4 - 0.5 + (5 - 3) / 4) / 2 / nm.MAD_SCALE and math.isnan(s[0, 1])
    assert s[1, 0] == 0.0 and s[1, 1] == (2 - 0.5 + (3.5 - 3) / 1) / 2 / nm.MAD_SCALE
    for st, want in zip(stats.reshape(-1, 4), s.reshape(-1)):
        got = nm.sigma_of(st, 255)
        assert got == want or (math.isnan(got) and math.isnan(want))
    assert utils.noise_sigma_from_stats(torch.from_numpy(stats), 219 << 2)[0, 0] == s[0, 0] * 255 / 876
    with pytest.raises(ValueError):
        utils.noise_sigma_from_stats(np.zeros((3, 3), np.int64), 255)
    with pytest.raises(ValueError):
        utils.noise_sigma_from_stats(stats, 0)


# --------------------------------------------------------------------------- twin against brute force
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("shape", [(6, 10), (7, 11), (6, 9), (9, 6), (2, 2), (3, 3)])
def test_twin_equals_brute_force(dtype, c, shape):
    """Even and odd H, W; 6 x 10 has 15 blocks (odd n), 6 x 9 and 9 x 6 have 12 (even n).  Values in a narrow band so that
    equal d occur (`at` > 1), with some saturated samples."""
    rng = np.random.default_rng([np.dtype(dtype).itemsize, c, *shape])
    peak = 255 if dtype == np.uint8 else 65535
    h, w = shape
    for trial in range(3):
        img = rng.integers(max(peak // 2 - 6, 0), peak // 2 + 6, (h, w, c)).astype(dtype)
        if trial == 1 and h * w > 4:
            img[rng.integers(0, h), rng.integers(0, w)] = 0
            img[rng.integers(0, h), rng.integers(0, w)] = peak
        if trial == 2:
            img = rng.integers(0, peak + 1, (h, w, c)).astype(dtype)
        frame = img[:, :, 0] if c == 1 and trial == 0 else img
        assert utils.noise_stats(frame).tolist() == nm.brute_stats(frame), (trial, shape)
        assert utils.noise_stats(frame, exclude_saturated=False).tolist() == nm.brute_stats(frame, 0, -1, 2 * peak + 1)
        assert utils.noise_stats(frame, sat=(peak // 2 - 5, peak // 2 + 4)).tolist() == \
            nm.brute_stats(frame, 0, peak // 2 - 5, peak // 2 + 4)


@pytest.mark.parametrize("shape", [(6, 10), (7, 12)])
def test_twin_equals_brute_force_with_shift(shape):
    rng = np.random.default_rng(5)
    img = (rng.integers(60, 1000, shape) << 6 | rng.integers(0, 64, shape)).astype(np.uint16)
    got = utils.noise_stats(img, shift=6, sat=(64, 940))
    assert got.tolist() == nm.brute_stats(img, 6, 64, 940) and got[0, 0] > 0
    assert got.tolist() == utils.noise_stats((img >> 6).astype(np.uint16), sat=(64, 940)).tolist()
    # the Y plane of a P010 frame: limited and full range
    h, w = shape[0] // 2 * 2, shape[1]
    planes = (img[:h], np.zeros((h // 2, w // 2, 2), np.uint16))
    lim = nm.sigma_of(nm.brute_stats(img[:h], 6, 64, 940)[0], 876)
    full = nm.sigma_of(nm.brute_stats(img[:h], 6, 0, 1023)[0], 1023)
    assert utils.estimate_noise_sigma_yuv(planes, "p010") == lim
    assert utils.estimate_noise_sigma_yuv(planes, "p010", full_range=True) == full
    assert utils.estimate_noise_sigma_yuv(planes[:1], "p010") == lim              # the chroma may be left out
    y8 = (img[:h] >> 8).astype(np.uint8)
    for fmt, rest in (("nv12", (np.zeros((h // 2, w // 2, 2), np.uint8),)), ("i420", (np.zeros((h // 2, w // 2), np.uint8),) * 2)):
        assert utils.estimate_noise_sigma_yuv((y8,) + rest, fmt) == nm.sigma_of(nm.brute_stats(y8, 0, 16, 235)[0], 219)
        assert utils.estimate_noise_sigma_yuv((y8,) + rest, fmt, True) == nm.sigma_of(nm.brute_stats(y8, 0, 0, 255)[0], 255)


# --------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_twin_accuracy_on_known_noise(dtype):
    """64 x 96 x 3 frames of the generator.  The bounds are the issue's: 10 % at sigma 5, 15, 25 (3.4 % per channel was
    seen), [-15 %, +5 %] at sigma 50 where clipping removes part of the noise, below 1.0 without noise."""
    for sigma in (5, 15, 25):
        est = utils.estimate_noise_sigma(nm.noisy_frame(64, 96, 3, sigma, dtype))
        print(f"{np.dtype(dtype).name} sigma {sigma}: estimate {est:.3f} ({100 * (est / sigma - 1):+.1f} %)")
        assert abs(est - sigma) <= 0.10 * sigma, (sigma, est)
    est = utils.estimate_noise_sigma(nm.noisy_frame(64, 96, 3, 50, dtype))
    print(f"{np.dtype(dtype).name} sigma 50: estimate {est:.3f} ({100 * (est / 50 - 1):+.1f} %)")
    assert -0.15 * 50 <= est - 50 <= 0.05 * 50, est
    est = utils.estimate_noise_sigma(nm.noisy_frame(64, 96, 3, 0, dtype))
    print(f"{np.dtype(dtype).name} sigma 0: estimate {est:.3f}")
    assert 0.0 <= est < 1.0, est


# --------------------------------------------------------------------------- the bank
class Named(torch.nn.Module):
    def __init__(self, name):
        super().__init__()
        self.name = name


def test_sigma_bank_pick():
    models = {50: Named("c"), 15: Named("a"), 25: Named("b")}
    bank = utils.SigmaBank(models)
    assert bank.levels == [15, 25, 50] and bank.models == models
    lo, hi = math.sqrt(15 * 25), math.sqrt(25 * 50)
    assert abs(lo - 19.36) < 0.01 and abs(hi - 35.36) < 0.01
    for est, want in ((0.0, 15), (-3.0, 15), (1e-9, 15), (14.0, 15), (19.3, 15), (19.4, 25), (25.0, 25), (35.3, 25),
                      (35.4, 50), (50.0, 50), (300.0, 50), (float("inf"), 50)):
        level, model = bank.pick(est)
        assert level == want and model is models[want], est
    # a tie goes to the lower level: 20 is the geometric mean of 10 and 40, exactly
    assert utils.SigmaBank({10: Named("x"), 40: Named("y")}).pick(20.0)[0] == 10
    assert utils.SigmaBank({10: Named("x"), 40: Named("y")}).pick(np.nextafter(20.0, 21.0))[0] == 40
    with pytest.raises(ValueError, match="NaN"):
        bank.pick(float("nan"))
    single = utils.SigmaBank({25: models[25]})
    assert single.levels == [25]
    for est in (0.0, 3.0, 25.0, 1000.0):
        assert single.pick(est) == (25, models[25])
    with pytest.raises(ValueError, match="NaN"):
        single.pick(float("nan"))
    for bad in ({}, {0: models[15]}, {-5: models[15]}, {"a": models[15]}, {15: None}):
        with pytest.raises(ValueError):
            utils.SigmaBank(bad)


def test_get_model_bank_loads_one_checkpoint_per_sigma(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("weights/DnCNN")
    os.makedirs("weights/REDNet")
    for i, s in enumerate((15, 25, 50)):
        torch.save(dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(10 + i).state_dict(), f"weights/DnCNN/dncnn_{s}.pth")
        torch.save(rednet.REDNet().load_synthetic(20 + i).state_dict(), f"weights/REDNet/{s}.pt")
    bank = utils.get_model_bank("denoising", "gaussian", "DnCNN", CPU, gray=True)
    assert isinstance(bank, utils.SigmaBank) and bank.levels == [15, 25, 50]
    assert all(m.nb == 17 and m.precision == "fp32" for m in bank.models.values())
    for i, s in enumerate((15, 25, 50)):
        want = dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(10 + i).state_dict()
        got = bank.models[s].state_dict()
        assert all(torch.equal(got[k], want[k]) for k in want), s
    red = utils.get_model_bank("denoising", "gaussian", "REDNet", CPU, sigmas=(50, 15), precision="fp16")
    assert red.levels == [15, 50] and all(m.precision == "fp16" for m in red.models.values())
    assert red.pick(27.0)[0] == 15 and red.pick(28.0)[0] == 50             # sqrt(15 x 50) = 27.39
    with pytest.raises(ValueError):
        utils.get_model_bank("denoising", "gaussian", "DnCNN", CPU, gray=True, sigmas=())
    with pytest.raises(FileNotFoundError):
        utils.get_model_bank("denoising", "gaussian", "DnCNN", CPU, gray=True, sigmas=(15, 35))


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_symbol():
    """The entry point has a header of its own, include/irm_hip_noise.h, which irm_hip.h includes inside its extern "C"
    block after irm_hip_metrics.h, and a table of its own, _hip.SIGNATURES_NOISE, disjoint from the other seven: header
    and table match one to one, the library exports the symbol, load() binds it, and it returns IRM_EINVAL for null
    pointers and zero sizes before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_metrics.h"') < main.index('#include "irm_hip_noise.h"') \
        < main.rindex("#ifdef __cplusplus")
    assert main.index('extern "C" {') < main.index('#include "irm_hip_noise.h"')
    text = open(os.path.join(ROOT, "include", "irm_hip_noise.h")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    assert "ws_words >=" in text, "the header states the workspace minimum"
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_NOISE)
    others = (_hip.SIGNATURES, _hip.SIGNATURES_HALF, _hip.SIGNATURES_FRAMES, _hip.SIGNATURES_GRAM, _hip.SIGNATURES_YUV,
              _hip.SIGNATURES_INCEPTION, _hip.SIGNATURES_METRICS)
    assert not set(_hip.SIGNATURES_NOISE) & set().union(*others)
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b"}
    _lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_NOISE[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_entry_refuses_bad_arguments_before_any_launch():
    """Non-null placeholder pointers that are never followed: every check below fails before a launch (a launch without
    a device would return IRM_ELAUNCH, not IRM_EINVAL)."""
    f = _lib().irm_noise_hh_stats
    fake = 4096

    def rc(frames=fake, u16=0, k=1, h=720, w=1280, c=3, pitch=None, stride=None, shift=0, lo=0, hi=255, stats=fake,
           ws=fake, words=None):
        pitch = w * c if pitch is None else pitch
        stride = (h - 1) * pitch + w * c if stride is None else stride
        words = 4098 * k * c if words is None else words
        return f(frames, u16, k, h, w, c, pitch, stride, shift, lo, hi, stats, ws, words, None)

    assert rc(words=4098 * 3 - 1) == -1 and rc(k=4, words=4 * 4098 * 3 - 1) == -1 and rc(c=1, words=4097) == -1
    assert rc(c=2) == -1 and rc(c=4) == -1 and rc(c=0) == -1
    assert rc(h=1) == -1 and rc(w=1) == -1 and rc(h=0) == -1 and rc(w=-2) == -1
    assert rc(k=0) == -1 and rc(k=65536) == -1
    assert rc(u16=2) == -1 and rc(u16=-1) == -1
    assert rc(h=40000, w=40000) == -1                  # more than 2^31 values in a frame
    assert rc(pitch=1280 * 3 - 1) == -1                # rows would overlap
    assert rc(k=2, stride=720 * 1280 * 3 - 1) == -1    # frames would overlap
    assert rc(c=1, pitch=1408, stride=719 * 1408 + 1279) == -1
    assert rc(shift=-1) == -1 and rc(shift=8) == -1 and rc(u16=1, shift=16) == -1
    assert rc(lo=-2) == -1 and rc(lo=255, hi=255) == -1 and rc(lo=10, hi=3) == -1
    for name in ("frames", "stats", "ws"):
        assert rc(**{name: 0}) == -1, name
    assert rc(u16=1, frames=fake + 1) == -1            # a 16-bit word on an odd address
    assert rc(stats=fake + 4) == -1 and rc(ws=fake + 4) == -1


def test_kernel_file_keeps_the_repository_rules():
    """No preprocessor conditional, integer counts only (no float atomics), and the Makefile needs no rule of its own."""
    csrc = os.path.join(os.path.dirname(_hip.LIB_PATH), "csrc")
    src = open(os.path.join(csrc, "noise.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", src, flags=re.M)
    code = re.sub(r"//.*", "", src)
    assert re.findall(r'#include [<"]([\w.]+)[>"]', code) == ["irm_frame.h"]
    assert not re.search(r"\b(float|double)\b", code), "every count is an integer"
    assert "noise" not in open(os.path.join(csrc, "Makefile")).read()


def test_every_noise_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_NOISE: each symbol
    is called by name in a test_guard_bands_* function of tests/test_gpu_noise.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_noise.py")) as f:
        text = f.read()
    reached = set()
    for body in re.split(r"^def ", text, flags=re.M):
        if body.startswith("test_guard_bands_"):
            reached |= set(re.findall(r'"(irm_\w+)"', body))
    missing = sorted(set(_hip.SIGNATURES_NOISE) - reached)
    assert not missing, f"noise entry points without a guard-band case: {missing}"


# --------------------------------------------------------------------------- Python checks before the library
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library must not be called")
    monkeypatch.setattr(_hip, "call", boom)
    monkeypatch.setattr(_hip, "load", boom)


def test_refusals_raise_before_the_library(no_library):
    a = torch.zeros(16, 16, 3, dtype=torch.uint8)
    for fn in (utils.noise_stats_device, utils.estimate_noise_sigma_device):
        with pytest.raises(ValueError, match="GPU"):
            fn(a.numpy())                                                  # a host array
        with pytest.raises(ValueError, match="GPU"):
            fn([a.numpy(), a.numpy()])
        with pytest.raises(ValueError, match="GPU"):
            fn(a)                                                          # a CPU tensor: no CPU fallback
        with pytest.raises(ValueError, match="GPU"):
            fn([a, a.clone()])
        with pytest.raises(ValueError, match="uint8 or uint16"):
            fn(a.float())
        with pytest.raises(ValueError, match="uint8 or uint16"):
            fn(a.double())
        with pytest.raises(ValueError, match="uint8 or uint16"):
            fn(a.to(torch.int32))
        for shape in ((1, 16, 3), (16, 1), (1, 1, 1)):
            with pytest.raises(ValueError, match="at least 2"):
                fn(torch.zeros(shape, dtype=torch.uint8))
        for ch in (2, 4):
            with pytest.raises(ValueError, match="channels"):
                fn(torch.zeros(16, 16, ch, dtype=torch.uint8))
        with pytest.raises(ValueError, match="share"):
            fn([a, a[:8]])
        with pytest.raises(ValueError, match="share"):
            fn([a, a.to(torch.int16)])
        with pytest.raises(ValueError, match="no frames"):
            fn([])
    with pytest.raises(ValueError, match="shift"):
        utils.noise_stats_device(a, shift=8)
    with pytest.raises(ValueError, match="sat"):
        utils.noise_stats_device(a, sat=(9, 3))
    # the numpy twin
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="numpy"):
        utils.noise_stats(a)
    with pytest.raises(ValueError, match="uint8 or uint16"):
        utils.noise_stats(img.astype(np.float32))
    with pytest.raises(ValueError, match="uint8 or uint16"):
        utils.estimate_noise_sigma(img.astype(np.float64))
    with pytest.raises(ValueError, match="at least 2"):
        utils.noise_stats(img[:1])
    with pytest.raises(ValueError, match="channels"):
        utils.noise_stats(img[:, :, :2])
    with pytest.raises(ValueError, match="channels"):
        utils.noise_stats(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(ValueError, match="shift"):
        utils.noise_stats(img, shift=-1)
    with pytest.raises(ValueError, match="shift"):
        utils.noise_stats(img.astype(np.uint16), shift=16)
    with pytest.raises(ValueError, match="sat"):
        utils.noise_stats(img, sat=(4, 4))


def test_yuv_refusals_raise_before_the_library(no_library):
    y, uv = np.zeros((16, 20), np.uint8), np.zeros((8, 10, 2), np.uint8)
    ty, tuv = torch.from_numpy(y), torch.from_numpy(uv)
    for host, device in (((y, uv), (ty, tuv)),):
        with pytest.raises(ValueError):
            utils.estimate_noise_sigma_yuv(host, "yv12")
        with pytest.raises(ValueError):
            utils.estimate_noise_sigma_yuv_device(device, "yv12")
        with pytest.raises(ValueError):
            utils.estimate_noise_sigma_yuv(host, "p010")                    # wrong dtype
        with pytest.raises(ValueError):
            utils.estimate_noise_sigma_yuv_device(device, "p010")
        with pytest.raises(ValueError):
            utils.estimate_noise_sigma_yuv(device, "nv12")                  # tensors to the host twin
        with pytest.raises(ValueError):
            utils.estimate_noise_sigma_yuv_device(host, "nv12")             # arrays to the device call
        with pytest.raises(ValueError):
            utils.estimate_noise_sigma_yuv(y, "nv12")                       # not a tuple
        with pytest.raises(ValueError, match="even"):
            utils.estimate_noise_sigma_yuv((y[:15], uv), "nv12")
        with pytest.raises(ValueError, match="GPU"):
            utils.estimate_noise_sigma_yuv_device(device, "nv12")           # valid CPU tensors: no CPU fallback
        with pytest.raises(ValueError, match="stride"):
            utils.estimate_noise_sigma_yuv_device((ty[:, ::2], tuv), "nv12")
    assert "0.75" in noise.estimate_noise_sigma_yuv.__doc__ and "0.75" in noise.estimate_noise_sigma_yuv_device.__doc__


def test_routed_call_refusals(no_library):
    bank = utils.SigmaBank({25: Named("b")})
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="SigmaBank"):
        utils.run_model_inference_auto({25: Named("b")}, img, CPU)
    with pytest.raises(ValueError, match="uint8 or uint16"):
        utils.run_model_inference_auto(bank, img.astype(np.float32), CPU)
    with pytest.raises(ValueError, match="uint8 or uint16"):
        utils.run_model_inference_auto(bank, torch.zeros(16, 16, 3, dtype=torch.uint8), CPU)
    with pytest.raises(_hip.HipLibraryError, match="GPU"):
        utils.run_model_inference_auto(bank, img, CPU)
    import inspect
    assert list(inspect.signature(utils.run_model_inference_auto).parameters) == ["bank", "input_img", "device", "patch_size",
                                                                                  "patch_overlap"]


def test_utils_re_exports_the_objects_of_noise():
    names = ["noise_stats", "noise_sigma_from_stats", "estimate_noise_sigma", "noise_stats_device",
             "estimate_noise_sigma_device", "estimate_noise_sigma_yuv", "estimate_noise_sigma_yuv_device"]
    for n in names:
        assert getattr(utils, n) is getattr(noise, n), n
        assert getattr(noise, n).__module__ == noise.__name__, n
    for n in ("SigmaBank", "get_model_bank", "run_model_inference_auto"):
        assert getattr(utils, n).__module__ == utils.__name__, n
    assert noise.MAD_SCALE == nm.MAD_SCALE == 0.6744897501960817
    assert yuv.YUV_FORMATS["p010"] == (2, 10)


# --------------------------------------------------------------------------- harness
KW = dict(task="denoising", subtask="gaussian", dataset="d", model_name="m")
CFG = dict(patch_size=32, patch_overlap=8)


def test_evaluate_auto_sigma_without_a_frame(tmp_path):
    bank = utils.SigmaBank({15: torch.nn.Linear(2, 2), 25: torch.nn.Linear(2, 2)})
    assert harness.COLUMNS_AUTO == harness.COLUMNS + ["Sigma_Est", "Std_Sigma_Est", "Sigma_Used"]
    row = harness.evaluate_auto_sigma(bank, iter([]), CPU, CFG, **KW)
    assert list(row)[:len(harness.COLUMNS)] == harness.COLUMNS and set(harness.COLUMNS_AUTO) <= set(row)
    assert math.isnan(row["PSNR"]) and math.isnan(row["Sigma_Est"]) and math.isnan(row["Std_Sigma_Est"])
    assert row["Sigma_Used"] == {} and row["Failed"] == [] and row["Model_Params"] == 6 and row["Sigma"] == "auto"
    with pytest.raises(ValueError, match="metrics"):
        harness.evaluate_auto_sigma(bank, iter([]), CPU, CFG, metrics="gpu", **KW)
    with pytest.raises(ValueError, match="SigmaBank"):
        harness.evaluate_auto_sigma(torch.nn.Linear(2, 2), iter([]), CPU, CFG, **KW)
    with pytest.raises(ValueError, match="patch_config"):
        harness.evaluate_auto_sigma(bank, iter([]), CPU, dict(patch_size=32), **KW)
    # a frame that raises is reported with skip_failed on and propagates with it off
    bad = [(np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.uint8), "float.png")]
    row = harness.evaluate_auto_sigma(bank, iter(bad), CPU, CFG, **KW)
    assert [n for n, _ in row["Failed"]] == ["float.png"] and row["Sigma_Used"] == {}
    with pytest.raises(ValueError, match="uint8 or uint16"):
        harness.evaluate_auto_sigma(bank, iter(bad), CPU, CFG, skip_failed=False, **KW)
    import csv
    with open(harness.save_results([row], out_dir=str(tmp_path), columns=harness.COLUMNS_AUTO)) as f:
        assert list(csv.DictReader(f).fieldnames) == harness.COLUMNS_AUTO
