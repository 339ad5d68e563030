"""The super-resolution benchmark protocol on the host: the float64 restatement of MATLAB's bicubic imresize and of
basicsr's cropped / Y-channel PSNR and SSIM against the reference goldens (tools/gen_golden_sr_protocol.py), the tap
tables, mod_crop, the C ABI declarations and the argument errors."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from frame_checks import check_quantised, quantise_ref
from irm_amd import _hip, harness, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("random", "synth")
#: max-abs bounds of a float64 restatement against the reference's fp32 imresize: measured 1.7e-7 (shrinking) and
#: 2.1e-7 (x2, x4); 1.3e-5 at x3, where the reference builds its weights with an fp32 linspace
RESIZE_BOUND = {"down2": 1e-6, "down3": 1e-6, "down4": 1e-6, "up2": 1e-6, "up3": 1e-4, "up4": 1e-6}
SCALE = {"down2": 0.5, "down3": 1.0 / 3.0, "down4": 0.25, "up2": 2, "up3": 3, "up4": 4}


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "sr_protocol.json")) as f:
        return json.load(f)


def source_of(g, key, name):
    """The uint8 frame a golden resize was made from: the HR frame when shrinking, the reference's LR (1/4) frame."""
    return g[f"hr_{name}"] if key.startswith("down") else g[f"lr4_{name}"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("key", list(RESIZE_BOUND))
def test_imresize_host_vs_reference(golden, key, name):
    g = golden("sr_protocol")
    ref, src = g[f"{key}_{name}"], source_of(g, key, name)
    got = utils.imresize_host(src, SCALE[key])
    assert got.dtype == np.float64 and got.shape == ref.shape
    err = float(np.abs(got - ref.astype(np.float64)).max())
    print(f"imresize_host {key} {name} {src.shape} -> {got.shape}: max-abs vs reference {err:.3e}")
    assert err <= RESIZE_BOUND[key]
    check_quantised(utils.imresize_host(src, SCALE[key], out="same"), quantise_ref(ref), f"quantised {key} {name}")


def test_imresize_host_grey_and_uint16(golden):
    """A grey frame resizes as one channel of a colour frame does; a uint16 frame of 257 x the bytes gives the same
    float result (v * 257 / 65535 = v / 255) and 257 x the quantised bytes up to rounding."""
    hr = golden("sr_protocol")["hr_synth"]
    for scale in (0.25, 3):
        full = utils.imresize_host(hr, scale)
        grey = utils.imresize_host(hr[:, :, 1].copy(), scale)
        assert grey.shape == full.shape[:2] and np.array_equal(grey, full[:, :, 1])
        assert np.array_equal(utils.imresize_host(hr[:, :, 1:2].copy(), scale)[:, :, 0], grey)
        f16 = utils.imresize_host(hr.astype(np.uint16) * 257, scale)
        assert float(np.abs(f16 - full).max()) <= 1e-12
        q16 = utils.imresize_host(hr.astype(np.uint16) * 257, scale, out="same")
        assert q16.dtype == np.uint16
        assert np.array_equal(q16, np.round(np.clip(f16, 0, 1) * 65535).astype(np.uint16))


@pytest.mark.parametrize("n", [18, 25, 96, 97, 131, 720, 1280])
@pytest.mark.parametrize("scale", [0.5, 1.0 / 3.0, 0.25, 2, 3, 4])
def test_resize_table_properties(n, scale):
    w, i = utils.resize_table(n, scale)
    s = round(1 / scale) if scale < 1 else scale
    p = 4 * s + 2 if scale < 1 else 6
    out = -(-n // s) if scale < 1 else n * s
    assert w.shape == i.shape == (out, p) and w.dtype == np.float64
    assert float(np.abs(w.sum(1) - 1.0).max()) <= 1e-14
    assert float(np.abs(w.astype(np.float32).astype(np.float64).sum(1) - 1.0).max()) <= 1e-6     # what the device sums
    assert int(i.min()) >= 0 and int(i.max()) < n
    # the reflected source indices of a row cover a contiguous range (what the kernel's LDS window relies on)
    for row in i[[0, 1, out // 2, out - 2, out - 1]]:
        u = np.unique(row)
        assert u[-1] - u[0] + 1 == len(u)


def test_resize_table_rejects_short_sides_and_other_factors():
    for scale, n in ((0.25, 17), (1.0 / 3.0, 13), (0.5, 9), (2, 5), (4, 5)):
        with pytest.raises(ValueError, match="shorter"):
            utils.resize_table(n, scale)
    for scale in (1, 5, 1.5, 0.2, 0, -2, 0.3):
        with pytest.raises(ValueError, match="resize factor"):
            utils.resize_table(64, scale)


def _metric_args(g, key):
    name, kind, crop, y = key.split("/")
    a, b = g[f"deg_{name}"], g[f"hr_{name}"]
    if kind == "grey":
        a, b = a[:, :, 1].copy(), b[:, :, 1].copy()
    return a, b, int(crop[4:]), bool(int(y[1:]))


def test_calculate_metrics_basicsr_vs_reference(golden, meta):
    """The reference reads colour frames as BGR.  Allowed: twice the distance the generator measured for this host
    restatement (the reference takes its Y-channel mean in fp32, so PSNR does not agree to 1e-9)."""
    g = golden("sr_protocol")
    tol_p, tol_s = 2 * meta["metrics_host_vs_reference"]["psnr_db"], 2 * meta["metrics_host_vs_reference"]["ssim"]
    assert len(meta["metrics"]) == 16 and 0 < tol_p < 1e-4 and 0 < tol_s < 1e-12
    for key, want in meta["metrics"].items():
        a, b, crop, y = _metric_args(g, key)
        p, s = utils.calculate_metrics_basicsr(a, b, crop, y, channel_order="bgr")
        print(f"{key}: PSNR {p:.9f} (reference {want['psnr']:.9f}, off {abs(p - want['psnr']):.2e}), "
              f"SSIM {s:.12f} (off {abs(s - want['ssim']):.2e})")
        assert abs(p - want["psnr"]) <= tol_p and abs(s - want["ssim"]) <= tol_s


def test_calculate_metrics_basicsr_properties(golden):
    g = golden("sr_protocol")
    a, b = g["deg_synth"], g["hr_synth"]
    assert utils.calculate_metrics_basicsr(b, b, 4, True) == (float("inf"), 1.0)
    assert utils.calculate_metrics_basicsr(b, b, 0, False) == (float("inf"), 1.0)
    # the channel order matters on the Y channel only, and swapping the channels swaps the order back
    rgb, bgr = utils.calculate_metrics_basicsr(a, b, 4, True, "rgb"), utils.calculate_metrics_basicsr(a, b, 4, True, "bgr")
    assert rgb != bgr
    assert utils.calculate_metrics_basicsr(a[:, :, ::-1].copy(), b[:, :, ::-1].copy(), 4, True, "bgr") == rgb
    assert (utils.calculate_metrics_basicsr(a, b, 4, False, "rgb") == utils.calculate_metrics_basicsr(a, b, 4, False, "bgr"))
    # the crop is a crop
    assert (utils.calculate_metrics_basicsr(a, b, 4, True)
            == utils.calculate_metrics_basicsr(a[4:-4, 4:-4].copy(), b[4:-4, 4:-4].copy(), 0, True))
    # without the Y channel, PSNR is the project's PSNR
    assert abs(utils.calculate_metrics_basicsr(a, b, 0, False)[0] - utils.psnr(b, a, 255)) <= 1e-12
    # uint16 frames of 257 x the bytes: the same SSIM and PSNR without the Y channel (both scale with the range)
    p8, s8 = utils.calculate_metrics_basicsr(a, b, 2, False)
    p16, s16 = utils.calculate_metrics_basicsr(a.astype(np.uint16) * 257, b.astype(np.uint16) * 257, 2, False)
    assert abs(p8 - p16) <= 1e-9 and abs(s8 - s16) <= 1e-9


def test_mod_crop():
    x = np.arange(97 * 131 * 3).reshape(97, 131, 3)
    for s, shape in ((2, (96, 130, 3)), (3, (96, 129, 3)), (4, (96, 128, 3)), (1, (97, 131, 3))):
        y = utils.mod_crop(x, s)
        assert y.shape == shape and np.array_equal(y, x[:shape[0], :shape[1]])
    assert utils.mod_crop(x[:, :, 0], 4).shape == (96, 128)
    assert tuple(utils.mod_crop(torch.zeros(10, 11, 3), 4).shape) == (8, 8, 3)
    assert utils.mod_crop(x[:96, :128], 4).shape == (96, 128, 3)
    with pytest.raises(ValueError):
        utils.mod_crop(x, 0)
    with pytest.raises(ValueError):
        utils.mod_crop(np.zeros((2, 3, 4, 5)), 2)


def test_header_signatures_and_library_agree():
    text = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M))
    for name, nargs in (("irm_imresize_bicubic", 15), ("irm_frame_metrics_basicsr", 15)):
        assert name in declared and name in _hip.SIGNATURES
        body = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", text, flags=re.M | re.S).group(1)
        assert len(body.split(",")) == nargs == len(_hip.SIGNATURES[name])
        # pointer parameters are c_void_p, long is c_long, double c_double, the rest int
        for decl, ct in zip(body.split(","), _hip.SIGNATURES[name]):
            decl = decl.strip()
            want = (ctypes.c_void_p if ("*" in decl or "irm_stream_t" in decl) else ctypes.c_long if decl.startswith("long")
                    else ctypes.c_double if decl.startswith("double") else ctypes.c_int)
            assert ct is want, (name, decl)
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _hip.load()
    for name in ("irm_imresize_bicubic", "irm_frame_metrics_basicsr"):
        fn = getattr(lib, name)
        assert fn(*[t(0) for t in _hip.SIGNATURES[name]]) == -1          # IRM_EINVAL before any HIP call


def test_no_new_environment_variable():
    for f in ("utils.py", "harness.py", "frames.py", "metrics.py", "resize.py", "niqe.py"):
        with open(os.path.join(os.path.dirname(os.path.abspath(utils.__file__)), f)) as fh:
            names = set(re.findall(r"IRM_[A-Z_]+", fh.read()))
        assert names <= {"IRM_NO_GRAPH", "IRM_EXPERIMENTAL_STREAMS"}, names


def test_value_errors_before_any_gpu_call():
    """Every one of these is refused on a machine with no GPU: the checks come before the first HIP call."""
    u8 = torch.zeros(32, 40, 3, dtype=torch.uint8)
    for frames, scale, kw in ((u8, 2, {}),                                    # a CPU tensor
                              (u8.float(), 2, {}),                             # dtype
                              (np.zeros((32, 40, 3), np.uint8), 2, {}),        # numpy
                              (u8, 5, {}), (u8, 1.5, {}),                      # factor
                              (u8, 2, {"out": "uint8"}),                       # flag
                              (torch.zeros(32, 40, 2, dtype=torch.uint8), 2, {}),
                              (torch.zeros(2, 2, 32, 40, 3, dtype=torch.uint8), 2, {}),
                              ([u8, torch.zeros(32, 41, 3, dtype=torch.uint8)], 2, {}),
                              ([], 2, {}),
                              (torch.zeros(17, 40, 3, dtype=torch.uint8), 0.25, {})):
        with pytest.raises(ValueError):
            utils.imresize_device(frames, scale, **kw)
    a = np.zeros((32, 40, 3), np.uint8)
    for bad in (dict(out="same8"), ):
        with pytest.raises(ValueError):
            utils.imresize_host(a, 2, **bad)
    with pytest.raises(ValueError):
        utils.imresize_host(a.astype(np.float32), 2)
    with pytest.raises(ValueError):
        utils.imresize_host(np.zeros((32, 40, 4), np.uint8), 2)
    for args in ((a, a[:-1], 0, True), (a, a.astype(np.uint16), 0, True), (a.astype(np.float32), a.astype(np.float32), 0, True),
                 (a, a, -1, True), (a, a, 11, True), (a, a, 0.5, True), (a, a, 0, True, "gbr"),
                 (torch.zeros(32, 40, 3), torch.zeros(32, 40, 3), 0, True)):
        with pytest.raises(ValueError):
            utils.calculate_metrics_basicsr(*args)
    for args in ((u8, u8, 0, True),                                            # CPU tensors
                 (a, a, 0, True),                                              # numpy
                 (u8, u8[:-1], 0, True), (u8, u8, 11, True), (u8, u8, -1, False), (u8, u8, 0, True, "xyz"),
                 (u8.float(), u8.float(), 0, True)):
        with pytest.raises(ValueError):
            utils.calculate_metrics_basicsr_device(*args)
    with pytest.raises(ValueError):
        list(harness.sr_pairs([(a, "a.png")], 5, "cpu"))
    with pytest.raises(ValueError):
        list(harness.sr_pairs([(a.astype(np.float32), "a.png")], 2, "cpu"))
    for kw in (dict(scale=5), dict(scale=2, metrics="gpu"), dict(scale=2, crop_border=-1), dict(scale=2, channel_order="x")):
        with pytest.raises(ValueError):
            harness.evaluate_sr(None, [(a, "a.png")], "cpu", {}, **kw)


def test_evaluate_keeps_its_signature_and_columns():
    import inspect
    assert list(inspect.signature(harness.evaluate).parameters) == [
        "model", "loader", "device", "patch_config", "task", "subtask", "dataset", "model_name", "sigma",
        "need_degradation", "noise_level", "with_ssim", "skip_failed", "metrics"]
    assert harness.COLUMNS == ['Task', 'Type', 'Dataset', 'Sigma', 'Model', 'Model_Params', 'PSNR', 'SSIM', 'Std_PSNR',
                               'Std_SSIM', 'Avg_Time_ms', 'Std_Time_ms']
    sig = inspect.signature(harness.evaluate_sr).parameters
    assert list(sig)[:5] == ["model", "hr_loader", "device", "patch_config", "scale"]
    assert sig["crop_border"].default is None and sig["test_y_channel"].default is True
