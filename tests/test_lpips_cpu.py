"""LPIPS, the part that needs no GPU: the float64 host twin against the written-out model, its exact cases, the head
formula by hand, the space-to-depth re-layout of the first conv, the loader, the Python refusals (which raise before the
library is touched), the C ABI of include/irm_hip_lpips.h against _hip.SIGNATURES_LPIPS, the library's own argument
checks (which return before any HIP call) and the harness row."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_model as lm
from irm_amd import _hip, harness, perceptual, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_lpips_pack", "irm_lpips_head"]


def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip.load()


@pytest.fixture(scope="module")
def states():
    return lm.synth_states()


@pytest.fixture(scope="module")
def params(states):
    return utils.lpips_params_from_state(*states)


# --------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("dtype", lm.DTYPES)
@pytest.mark.parametrize("h,w", [(31, 31), (34, 139), (64, 96)])
def test_twin_equals_the_model(states, params, dtype, h, w):
    a, b = lm.random_frame(h, w, dtype, 1), lm.random_frame(h, w, dtype, 2)
    taps, total = lm.lpips(a, b, *states)
    got_taps = utils.lpips_taps(a, b, params)
    got = utils.calculate_lpips(a, b, params)
    assert isinstance(got, float) and total > 0
    assert abs(got - total) <= 1e-12 * total
    for g, want in zip(got_taps, taps):
        assert abs(g - want) <= 1e-12 * want


@pytest.mark.parametrize("dtype", lm.DTYPES)
def test_exact_cases(params, dtype):
    a, b = lm.random_frame(40, 53, dtype, 3), lm.random_frame(40, 53, dtype, 4)
    assert utils.calculate_lpips(a, a.copy(), params) == 0.0
    assert utils.calculate_lpips(a, b, params) == utils.calculate_lpips(b, a, params) > 0.0


def test_head_formula_by_hand():
    c, h, w = 5, 3, 4
    lin = torch.tensor([0.5, 0.25, 2.0, 1.0, 0.125], dtype=torch.float64)
    f, g = torch.zeros(c, h, w, dtype=torch.float64), torch.zeros(c, h, w, dtype=torch.float64)
    f[1], g[2] = 1.0, 1.0                                             # e_1 against e_2 at every pixel
    assert abs(perceptual.lpips_head_host(f, g, lin) - float(lin[1] + lin[2])) <= 1e-9
    assert abs(lm.head(f, g, lin) - float(lin[1] + lin[2])) <= 1e-9
    g = torch.rand(c, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) + 0.1
    ng = g.pow(2).sum(0).sqrt()
    want = float((lin.view(-1, 1, 1) * g ** 2 / (ng + 1e-10) ** 2).sum(0).mean())
    got = perceptual.lpips_head_host(torch.zeros_like(g), g, lin)
    assert not math.isnan(got) and abs(got - want) <= 1e-12 * want
    assert perceptual.lpips_head_host(torch.zeros_like(g), torch.zeros_like(g), lin) == 0.0


@pytest.mark.parametrize("h", [31, 32, 33, 34])
@pytest.mark.parametrize("w", [31, 67, 139])
def test_space_to_depth_relayout(states, params, h, w):
    """The 3 x 3 stride-1 pad-0 conv with params.w3 over the space-to-depth frame is the 11 x 11 stride-4 pad-2 conv."""
    alex = states[0]
    u = lm.scaled(lm.random_frame(h, w, np.float32, h * 1000 + w))
    want = F.conv2d(u, alex["features.0.weight"].double(), alex["features.0.bias"].double(), stride=4, padding=2)
    z = torch.from_numpy(lm.space_to_depth(u[0].numpy()))[None]
    assert params.w3.shape == (64, 48, 3, 3)
    got = F.conv2d(z, params.w3.double(), alex["features.0.bias"].double())
    assert got.shape == want.shape == (1, 64, lm.out_size(h), lm.out_size(w))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# --------------------------------------------------------------------------- the loader
def test_loader_reads_both_layouts(tmp_path, states, params):
    alex, lin = states
    a, b = lm.random_frame(33, 35, np.uint8, 5), lm.random_frame(33, 35, np.uint8, 6)
    want = utils.calculate_lpips(a, b, params)
    plain = dict(alex, **{"classifier.1.weight": torch.zeros(8, 8), "classifier.1.bias": torch.zeros(8)})
    torch.save(plain, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    torch.save({"module." + k: v for k, v in plain.items()}, tmp_path / "alexnet_dp.pth")
    torch.save({"module." + k: v for k, v in lin.items()}, tmp_path / "alex_dp.pth")
    for pa, pl in (("alexnet.pth", "alex.pth"), ("alexnet_dp.pth", "alex_dp.pth")):
        p = utils.load_lpips_params(tmp_path / pa, tmp_path / pl)
        assert isinstance(p, utils.LpipsParams) and utils.calculate_lpips(a, b, p) == want
    bad = dict(alex)
    bad["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match="shape"):
        utils.lpips_params_from_state(bad, lin)
    with pytest.raises(ValueError, match="features.8.bias"):
        utils.lpips_params_from_state({k: v for k, v in alex.items() if k != "features.8.bias"}, lin)
    with pytest.raises(ValueError, match="lin4"):
        utils.lpips_params_from_state(alex, {k: v for k, v in lin.items() if not k.startswith("lin4")})
    with pytest.raises(ValueError, match="tensor"):
        utils.lpips_params_from_state(dict(alex, **{"features.0.bias": [0.0] * 64}), lin)
    with pytest.raises(ValueError, match="shape"):
        utils.lpips_params_from_state(alex, dict(lin, **{"lin2.model.1.weight": torch.zeros(384)}))
    with pytest.raises(ValueError, match="state dict"):
        utils.lpips_params_from_state([1, 2], lin)


# --------------------------------------------------------------------------- Python checks before the library
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library must not be called")
    monkeypatch.setattr(_hip, "call", boom)
    monkeypatch.setattr(_hip, "load", boom)


def test_refusals_raise_before_the_library(no_library, params):
    ok = np.zeros((40, 40, 3), np.uint8)
    cases = [(np.zeros((30, 64, 3), np.uint8), None, ">= 31"), (np.zeros((64, 30, 3), np.uint8), None, ">= 31"),
             (np.zeros((40, 40, 1), np.uint8), None, "3 channels"), (np.zeros((40, 40, 4), np.uint8), None, "3 channels"),
             (np.zeros((40, 40), np.uint8), None, "3 channels"),
             (np.zeros((40, 40, 3), np.float64), None, "float32"), (np.zeros((40, 40, 3), np.float16), None, "float32"),
             (ok, np.zeros((40, 41, 3), np.uint8), "differ"), (ok, np.zeros((40, 40, 3), np.uint16), "differ")]
    for a, b, msg in cases:
        b = a.copy() if b is None else b
        with pytest.raises(ValueError, match=msg):
            utils.calculate_lpips(a, b, params)
        ta, tb = torch.from_numpy(a), torch.from_numpy(b)
        for fn in (utils.calculate_lpips_device, utils.frame_lpips_device):
            with pytest.raises(ValueError, match=msg):
                fn(ta, tb, params)
    t = torch.from_numpy(ok)
    for fn in (utils.calculate_lpips_device, utils.frame_lpips_device):
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(ok, ok, params)                                        # host arrays
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            fn(t, t.clone(), params)                                  # CPU tensors
        with pytest.raises(ValueError, match="params"):
            fn(t, t, {"lin": 1})
    with pytest.raises(ValueError, match="same number"):
        utils.frame_lpips_device([t, t], [t], params)
    with pytest.raises(ValueError, match="share"):
        utils.frame_lpips_device([t, torch.zeros(48, 40, 3, dtype=torch.uint8)],
                                 [t, torch.zeros(48, 40, 3, dtype=torch.uint8)], params)
    with pytest.raises(ValueError, match="numpy"):
        utils.calculate_lpips(t, t, params)
    with pytest.raises(ValueError, match="metrics"):
        harness.evaluate_perceptual(None, [], torch.device("cpu"), {}, lpips_params=params, metrics="gpu")


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_symbols():
    """include/irm_hip_lpips.h, included by irm_hip.h inside its extern "C" block after irm_hip_noise.h, and
    _hip.SIGNATURES_LPIPS, disjoint from the other eight tables, match one to one; the library exports the symbols,
    load() binds them, and all-zero arguments return IRM_EINVAL before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_noise.h"') < main.index('#include "irm_hip_lpips.h"') \
        < main.rindex("#ifdef __cplusplus")
    assert main.index('extern "C" {') < main.index('#include "irm_hip_lpips.h"')
    text = open(os.path.join(ROOT, "include", "irm_hip_lpips.h")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    assert "ws_words >=" in text, "the header states the workspace minimum"
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_LPIPS)
    others = (_hip.SIGNATURES, _hip.SIGNATURES_HALF, _hip.SIGNATURES_FRAMES, _hip.SIGNATURES_GRAM, _hip.SIGNATURES_YUV,
              _hip.SIGNATURES_INCEPTION, _hip.SIGNATURES_METRICS, _hip.SIGNATURES_NOISE)
    assert not set(_hip.SIGNATURES_LPIPS) & set().union(*others)
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b", ctypes.c_float: r"^float\b"}
    _lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_LPIPS[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_entries_refuse_bad_arguments_before_any_launch():
    """Non-null placeholder pointers that are never followed: every check below fails before a launch (a launch without
    a device would return IRM_ELAUNCH, not IRM_EINVAL)."""
    lib = _lib()
    fake = 4096

    def pack(frames=fake, kind=0, k=1, h=720, w=1280, pitch=None, stride=None, z=fake, z_bs=None):
        pitch = 3 * w if pitch is None else pitch
        stride = (h - 1) * pitch + 3 * w if stride is None else stride
        z_bs = 48 * (lm.out_size(h) + 2) * (lm.out_size(w) + 2) if z_bs is None else z_bs
        return lib.irm_lpips_pack(frames, kind, k, h, w, pitch, stride, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, z, z_bs, None)

    assert pack(frames=0) == -1 and pack(z=0) == -1
    assert pack(kind=-1) == -1 and pack(kind=3) == -1
    assert pack(k=0) == -1 and pack(k=-1) == -1 and pack(k=65536) == -1
    assert pack(h=6) == -1 and pack(w=6) == -1 and pack(h=0) == -1 and pack(w=-3) == -1
    assert pack(h=40000, w=40000) == -1                 # more than 2^31 samples in a frame
    assert pack(pitch=3 * 1280 - 1) == -1              # rows would overlap
    assert pack(k=2, stride=720 * 3 * 1280 - 1) == -1  # frames would overlap
    assert pack(pitch=4096, stride=719 * 4096 + 3 * 1280 - 1) == -1
    assert pack(z_bs=48 * 181 * 321 - 1) == -1         # the blocks of two frames would overlap
    assert pack(kind=1, frames=fake + 1) == -1 and pack(kind=2, frames=fake + 2) == -1
    assert pack(z=fake + 2) == -1

    def head(f=fake, f_bs=None, lin=fake, k=1, c=64, h=179, w=319, out=fake, stride=6, ws=fake, words=None):
        f_bs = c * h * w if f_bs is None else f_bs
        words = k * -(-h * w // 64) if words is None else words
        return lib.irm_lpips_head(f, f_bs, lin, k, c, h, w, out, stride, ws, words, None)

    for name in ("f", "lin", "out", "ws"):
        assert head(**{name: 0}) == -1, name
    assert head(k=0) == -1 and head(k=65536) == -1
    assert head(c=0) == -1 and head(c=-1) == -1 and head(c=4097) == -1
    assert head(h=0) == -1 and head(w=0) == -1 and head(h=-5) == -1
    assert head(c=4096, h=1024, w=1024) == -1           # more than 2^31 values in a map
    assert head(f_bs=64 * 179 * 319 - 1) == -1         # maps would overlap
    assert head(stride=0) == -1 and head(stride=-6) == -1
    assert head(words=-(-179 * 319 // 64) - 1) == -1 and head(k=3, words=3 * -(-179 * 319 // 64) - 1) == -1
    assert head(f=fake + 2) == -1 and head(lin=fake + 1) == -1
    assert head(out=fake + 4) == -1 and head(ws=fake + 4) == -1


def test_kernel_file_keeps_the_repository_rules():
    """No preprocessor conditional, no float atomics, and the Makefile needs no rule of its own: the affine is an
    explicit fma and every rounding of the head is spelled out."""
    csrc = os.path.join(os.path.dirname(_hip.LIB_PATH), "csrc")
    src = open(os.path.join(csrc, "lpips.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", src, flags=re.M)
    code = re.sub(r"//.*", "", src)
    assert re.findall(r'#include [<"]([\w.]+)[>"]', code) == ["irm_frame.h"]
    assert "atomic" not in code
    assert "__fmaf_rn" in code
    assert "lpips" not in open(os.path.join(csrc, "Makefile")).read()


def test_every_lpips_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_LPIPS: each
    symbol is called by name in a test_guard_bands_* function of tests/test_gpu_lpips.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_lpips.py")) as f:
        text = f.read()
    reached = set()
    for body in re.split(r"^def ", text, flags=re.M):
        if body.startswith("test_guard_bands_"):
            reached |= set(re.findall(r'"(irm_\w+)"', body))
    missing = sorted(set(_hip.SIGNATURES_LPIPS) - reached)
    assert not missing, f"LPIPS entry points without a guard-band case: {missing}"


# --------------------------------------------------------------------------- harness
def test_evaluate_perceptual_host_row(tmp_path, params):
    from irm_amd.metrics import calculate_metrics
    frames = [lm.pairs(48, 56, np.uint8, seed=s)["blurred"] for s in range(3)]
    loader = [(a, b, f"f{i}") for i, (a, b) in enumerate(frames)]
    row = harness.evaluate_perceptual(None, loader, torch.device("cpu"), {}, lpips_params=params, metrics="host",
                                      dataset="unit")
    vals = [utils.calculate_lpips(a, b, params) for a, b in frames]
    ps = [calculate_metrics(a, b) for a, b in frames]
    assert row["LPIPS"] == np.mean(vals) and row["Std_LPIPS"] == np.std(vals) and row["LPIPS"] > 0
    assert row["PSNR"] == np.mean([p for p, _ in ps]) and row["SSIM"] == np.mean([s for _, s in ps])
    assert row["Avg_Time_ms"] == 0.0 and row["Model"] == "Input" and row["Model_Params"] == 0 and row["Failed"] == []
    assert harness.COLUMNS_PERCEPTUAL == harness.COLUMNS + ["LPIPS", "Std_LPIPS"]
    path = harness.save_results([row], str(tmp_path), "p.csv", columns=harness.COLUMNS_PERCEPTUAL)
    with open(path) as f:
        header, line = f.read().strip().split("\n")
    assert header.split(",") == harness.COLUMNS_PERCEPTUAL and float(line.split(",")[-2]) == row["LPIPS"]
    empty = harness.evaluate_perceptual(None, [], torch.device("cpu"), {}, lpips_params=params, metrics="host")
    assert all(math.isnan(empty[k]) for k in ("PSNR", "SSIM", "LPIPS", "Std_LPIPS", "Avg_Time_ms"))
    # a frame that cannot be scored is reported, not fatal
    small = (np.zeros((20, 20, 3), np.uint8),) * 2 + ("small",)
    row2 = harness.evaluate_perceptual(None, loader + [small], torch.device("cpu"), {}, lpips_params=params,
                                       metrics="host")
    assert row2["LPIPS"] == row["LPIPS"] and [n for n, _ in row2["Failed"]] == ["small"]
