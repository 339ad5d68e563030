#!/usr/bin/env python3
"""Golden fixtures of the super-resolution benchmark protocol: tests/golden/sr_protocol.npz and sr_protocol.json.

Runs where the reference tree is available (CPU).  It loads the reference's own basicsr files by path -
utils/matlab_functions.py (imresize, bgr2ycbcr), metrics/metric_util.py and metrics/psnr_ssim.py (calculate_psnr,
calculate_ssim) - under their package names, with two stand-ins in sys.modules:
  * `cv2` (not installed here): getGaussianKernel(ksize, sigma) as the normalised float64 exp(-(i - c)^2 / (2 sigma^2))
    column OpenCV builds for ksize > 7, and filter2D(img, -1, window) as scipy.ndimage.correlate(mode='mirror')
    (OpenCV's default BORDER_REFLECT_101; the reference keeps only the valid region [5:-5, 5:-5], where the border
    mode plays no part);
  * `mair.basicsr.utils.registry`: a METRIC_REGISTRY whose register() leaves the function as it is.
Both are recorded in the JSON.

Stored: two uint8 HR frames (96x120 random, 97x131 `synth` image) and a degraded frame of each; the reference's
imresize at 1/2, 1/3, 1/4 of each HR frame (float32, on frame / 255 in float32); the 1/4 result quantised as the
reference's tensor2img does (clamp, x 255, round half to even) and the reference's imresize at 2, 3, 4 of that LR frame;
the reference's PSNR / SSIM for crop in {0, 4} x Y in {off, on} x {colour read as BGR, grey}; and the measured distance
of utils.imresize_host / utils.calculate_metrics_basicsr from the reference.

Usage: python tools/gen_golden_sr_protocol.py
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden  # noqa: E402
from irm_amd import synth, utils  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FRAMES = {"random": (96, 120), "synth": (97, 131)}
SHRINK = {2: 0.5, 3: 1.0 / 3.0, 4: 0.25}


def _cv2_stand_in():
    from scipy.ndimage import correlate
    cv2 = types.ModuleType("cv2")

    def getGaussianKernel(ksize, sigma):
        i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
        g = np.exp(-(i * i) / (2.0 * sigma * sigma))
        return (g / g.sum()).reshape(ksize, 1)

    def filter2D(img, ddepth, window):
        assert ddepth == -1
        return correlate(np.asarray(img, dtype=np.float64), np.asarray(window, dtype=np.float64), mode="mirror")
    cv2.getGaussianKernel, cv2.filter2D = getGaussianKernel, filter2D
    return cv2


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    """(matlab_functions, psnr_ssim) of the reference, loaded by file path."""
    base = os.path.join(gen_golden.REF_SRC, "mair", "basicsr")
    sys.modules["cv2"] = _cv2_stand_in()
    for pkg in ("mair", "mair.basicsr", "mair.basicsr.utils", "mair.basicsr.metrics"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
    reg = types.ModuleType("mair.basicsr.utils.registry")

    class _Registry:
        def register(self):
            return lambda fn: fn
    reg.METRIC_REGISTRY = _Registry()
    sys.modules["mair.basicsr.utils.registry"] = reg
    mf = _load("mair.basicsr.utils.matlab_functions", os.path.join(base, "utils", "matlab_functions.py"))
    _load("mair.basicsr.metrics.metric_util", os.path.join(base, "metrics", "metric_util.py"))
    ps = _load("mair.basicsr.metrics.psnr_ssim", os.path.join(base, "metrics", "psnr_ssim.py"))
    return mf, ps


def frames():
    """name -> (hr uint8 HWC, degraded uint8 HWC of the same shape)."""
    out = {}
    h, w = FRAMES["random"]
    rng = np.random.default_rng(20240)
    hr = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    noisy = np.clip(np.rint(hr.astype(np.float64) + rng.normal(0.0, 12.0, hr.shape)), 0, 255).astype(np.uint8)
    out["random"] = (hr, noisy)
    h, w = FRAMES["synth"]
    inp, tgt = synth.synth_image_pair(3, h, w, 3, seed_base=7000, blur=5)
    out["synth"] = (tgt, inp)
    return out


def quantise_ref(x32: np.ndarray) -> np.ndarray:
    """tensor2img's steps on an fp32 image in [0, 1] nominal: clamp, x 255.0 in fp32, round half to even, uint8."""
    return (np.clip(x32, np.float32(0), np.float32(1)) * 255.0).round().astype(np.uint8)


def main():
    mf, ps = import_reference()
    out, meta = {}, {
        "generated_by": "tools/gen_golden_sr_protocol.py (reference basicsr imresize / calculate_psnr / calculate_ssim, "
                        "loaded by file path, numpy / torch CPU)",
        "stand_ins": {"cv2": "getGaussianKernel and filter2D through numpy / scipy.ndimage.correlate(mode='mirror'): "
                             "cv2 is not installed where the fixtures are generated",
                      "mair.basicsr.utils.registry": "METRIC_REGISTRY.register() as the identity decorator"},
        "frames": {k: list(v) for k, v in FRAMES.items()}, "resize_host_vs_reference": {}, "metrics": {},
        "resize_quantised_host_vs_reference": {}}
    d_psnr = d_ssim = 0.0
    for name, (hr, deg) in frames().items():
        out[f"hr_{name}"], out[f"deg_{name}"] = hr, deg
        x32 = hr.astype(np.float32) / np.float32(255.0)

        def record(key, ref, src_u8, scale):
            host = utils.imresize_host(src_u8, scale)
            d = float(np.abs(host - ref.astype(np.float64)).max())
            meta["resize_host_vs_reference"][key] = d
            q_ref, q_host = quantise_ref(ref), utils.imresize_host(src_u8, scale, out="same")
            diff = np.abs(q_ref.astype(np.int32) - q_host.astype(np.int32))
            meta["resize_quantised_host_vs_reference"][key] = {"max": int(diff.max()), "differing": int((diff > 0).sum()),
                                                               "of": int(diff.size)}
            print(f"{key}: {ref.shape} host float64 vs reference {d:.3e}; quantised: {int((diff > 0).sum())} of {diff.size} differ")

        for s, scale in SHRINK.items():
            ref = mf.imresize(x32, scale)
            assert ref.dtype == np.float32
            out[f"down{s}_{name}"] = ref
            record(f"down{s}_{name}", ref, hr, scale)
        lr = quantise_ref(out[f"down4_{name}"])
        out[f"lr4_{name}"] = lr
        l32 = lr.astype(np.float32) / np.float32(255.0)
        for s in (2, 3, 4):
            ref = mf.imresize(l32, s)
            out[f"up{s}_{name}"] = ref
            record(f"up{s}_{name}", ref, lr, s)
        # metrics: the degraded frame against the HR frame; the reference reads colour frames as BGR
        for kind, (a, b) in {"bgr": (deg, hr), "grey": (deg[:, :, 1].copy(), hr[:, :, 1].copy())}.items():
            for crop in (0, 4):
                for y in (False, True):
                    p_ref = float(ps.calculate_psnr(a, b, crop, test_y_channel=y))
                    s_ref = float(ps.calculate_ssim(a, b, crop, test_y_channel=y))
                    p_h, s_h = utils.calculate_metrics_basicsr(a, b, crop, y, channel_order="bgr")
                    key = f"{name}/{kind}/crop{crop}/y{int(y)}"
                    meta["metrics"][key] = {"psnr": p_ref, "ssim": s_ref}
                    d_psnr, d_ssim = max(d_psnr, abs(p_h - p_ref)), max(d_ssim, abs(s_h - s_ref))
                    print(f"{key}: reference PSNR {p_ref:.9f} SSIM {s_ref:.12f}; host restatement off by "
                          f"{abs(p_h - p_ref):.3e} dB, {abs(s_h - s_ref):.3e}")
    meta["metrics_host_vs_reference"] = {"psnr_db": d_psnr, "ssim": d_ssim,
                                         "note": "max over all cases of |calculate_metrics_basicsr - reference|; the "
                                                 "reference takes its Y-channel mean squared error in fp32"}
    os.makedirs(GOLD, exist_ok=True)
    npz = os.path.join(GOLD, "sr_protocol.npz")
    np.savez_compressed(npz, **out)
    with open(os.path.join(GOLD, "sr_protocol.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", npz, os.path.getsize(npz), "bytes")
    assert os.path.getsize(npz) < (1 << 20)


if __name__ == "__main__":
    main()
