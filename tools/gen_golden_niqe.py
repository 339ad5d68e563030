#!/usr/bin/env python3
"""Golden fixtures of the no-reference metric: tests/golden/niqe.npz and niqe.json.

Default mode (CPU, where the reference tree is available).  It loads the reference's own realDenoising basicsr files
by path - utils/matlab_functions.py (bgr2ycbcr), metrics/metric_util.py and metrics/niqe.py - under their package
names, with stand-ins in sys.modules, both recorded in the JSON:
  * `cv2` (not installed here): resize(img, (w, h), interpolation=INTER_LINEAR) to exactly half of even extents as
    the 2 x 2 mean, which is what bilinear interpolation computes there;
  * the packages `mair.realDenoising.basicsr[.utils|.metrics]` as empty modules, so that metric_util's import of
    `...utils.matlab_functions` finds the reference's own file without the packages' __init__ (they import cv2, lmdb).
Reference code is imported, never copied.  The reference reads its parameter file relative to the working directory;
the generator changes into the reference's realDenoising directory for the calls.

Stored per fixture case: the frame, the reference's per-block features (captured around compute_feature, scale 1
then scale 2, joined to [n_blocks][36]) and its score, and the measured distance of utils.niqe_features /
calculate_niqe from them (utils.niqe_feature_distance).  The generator fails if the host restatement differs from the
reference in any alpha entry.

--device-bound (on a GPU, no reference needed): measures utils.niqe_features_device / calculate_niqe_device against
the host restatement on the stored frames, a stack of three, a frame with a black block and the harness test's frames, and writes the maxima under `device_vs_host`.

Usage: python tools/gen_golden_niqe.py [--device-bound] [--out JSON]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from irm_amd import synth, utils  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PARAMS = os.path.join(GOLD, "niqe_pris_params.npz")
#: case -> (frame key, crop_border)
CASES = {"synth_crop0": ("synth", 0), "synth_crop4": ("synth", 4), "noise": ("noise", 0), "grey": ("grey", 0),
         "u16": ("u16", 0)}


def frames() -> dict:
    """The fixture frames, the smallest that reach every path: 200x300 colour (2 x 3 blocks, extents no multiple of
    96), 192x288 colour with sigma-20 noise, 96x192 grey (two blocks, the minimum), 192x192 uint16 colour."""
    rng = np.random.default_rng(9600)
    out = {"synth": synth.synth_image_pair(1, 200, 300, 3, seed_base=9600, blur=0)[1]}
    clean = synth.synth_image_pair(2, 192, 288, 3, seed_base=9600, blur=0)[1]
    out["noise"] = np.clip(np.rint(clean.astype(np.float64) + rng.normal(0.0, 20.0, clean.shape)), 0, 255).astype(np.uint8)
    out["grey"] = synth.synth_image_pair(3, 96, 192, 1, seed_base=9600, blur=3)[0][:, :, 0].copy()
    base = synth.synth_image_pair(4, 192, 192, 3, seed_base=9600, blur=0)[1].astype(np.float64)
    out["u16"] = np.clip(np.rint(base * 257.0 + rng.normal(0.0, 300.0, base.shape)), 0, 65535).astype(np.uint16)
    return out


def stack3(frame: np.ndarray) -> np.ndarray:
    """The K = 3 case of the device tests: the frame, upside down, and mirrored."""
    return np.ascontiguousarray(np.stack([frame, frame[::-1], frame[:, ::-1]]))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    """(niqe module, the reference's realDenoising directory), loaded by file path."""
    from oracle import gen_golden
    rd = os.path.join(gen_golden.REF_SRC, "mair", "realDenoising")
    base = os.path.join(rd, "basicsr")
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1

    def resize(img, dsize, interpolation=None):
        h, w = img.shape
        assert interpolation == cv2.INTER_LINEAR and h % 2 == 0 and w % 2 == 0 and dsize == (w // 2, h // 2)
        return (((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2]) * img.dtype.type(0.25)
    cv2.resize = resize
    sys.modules["cv2"] = cv2
    for pkg in ("mair", "mair.realDenoising", "mair.realDenoising.basicsr", "mair.realDenoising.basicsr.utils",
                "mair.realDenoising.basicsr.metrics"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
    _load("mair.realDenoising.basicsr.utils.matlab_functions", os.path.join(base, "utils", "matlab_functions.py"))
    _load("mair.realDenoising.basicsr.metrics.metric_util", os.path.join(base, "metrics", "metric_util.py"))
    return _load("mair.realDenoising.basicsr.metrics.niqe", os.path.join(base, "metrics", "niqe.py")), rd


def reference_niqe(niqe_mod, rd, frame, crop):
    """(features [n_blocks][36], score) of the reference for one frame; uint16 goes in as float values / 257."""
    img = frame.astype(np.float64) / 257.0 if frame.dtype == np.uint16 else frame
    rows, inner = [], niqe_mod.compute_feature

    def capture(block):
        feat = inner(block)
        rows.append([float(v) for v in feat])
        return feat
    cwd = os.getcwd()
    niqe_mod.compute_feature = capture
    try:
        os.chdir(rd)
        with np.errstate(all="ignore"):
            score = float(np.asarray(niqe_mod.calculate_niqe(img, crop, input_order="HWC", convert_to="y")).item())
    finally:
        os.chdir(cwd)
        niqe_mod.compute_feature = inner
    n = len(rows) // 2
    return np.concatenate([np.array(rows[:n]), np.array(rows[n:])], axis=1), score


def generate(out_json):
    niqe_mod, rd = import_reference()
    ref_params = os.path.join(rd, "basicsr", "metrics", "niqe_pris_params.npz")
    assert open(ref_params, "rb").read() == open(PARAMS, "rb").read(), "tests/golden/niqe_pris_params.npz is not the reference's file"
    params = utils.load_niqe_params(PARAMS)
    old = json.load(open(out_json)) if os.path.exists(out_json) else {}
    fr = frames()
    out = {f"frame_{k}": v for k, v in fr.items()}
    meta = {"generated_by": "tools/gen_golden_niqe.py (reference realDenoising basicsr calculate_niqe, loaded by file "
                            "path, numpy / scipy CPU)",
            "stand_ins": {"cv2": "resize(img, (w // 2, h // 2), INTER_LINEAR) of even extents as the 2 x 2 mean "
                                 "((a + b) + c + d) x 0.25 in the array's dtype: cv2 is not installed where the fixtures "
                                 "are generated, so this step of the reference is not pinned",
                          "mair.realDenoising.basicsr.utils.matlab_functions": "the reference's own file, loaded by path "
                          "under empty stand-in packages (their __init__ import cv2 and lmdb)"},
            "uint16": "the reference takes values in 0..255; a uint16 frame goes in as float64 values / 257",
            "distance": "utils.niqe_feature_distance: alpha entries in grid steps, other features |a - b| / max(|b|, 0.01)",
            "cases": {}}
    feat_rel = score_rel = 0.0
    for case, (key, crop) in CASES.items():
        frame = fr[key]
        ref_feat, ref_score = reference_niqe(niqe_mod, rd, frame, crop)
        plane = utils.niqe_plane(frame, crop, "HWC", "bgr")
        host_feat = utils.niqe_features(plane, params)
        host_score = utils.calculate_niqe(frame, crop, params, channel_order="bgr")
        differing, steps, rel = utils.niqe_feature_distance(host_feat, ref_feat)
        srel = abs(host_score - ref_score) / abs(ref_score)
        assert differing == 0, f"{case}: the host restatement differs from the reference in {differing} alpha entries"
        assert np.isfinite(rel) and np.isfinite(ref_score)
        out[f"features_{case}"] = ref_feat
        meta["cases"][case] = {"frame": key, "crop_border": crop, "shape": list(frame.shape), "dtype": str(frame.dtype),
                               "blocks": int(ref_feat.shape[0]), "score": ref_score,
                               "host_vs_reference": {"alpha_differing": differing, "features_rel": rel, "score_rel": srel}}
        feat_rel, score_rel = max(feat_rel, rel), max(score_rel, srel)
        print(f"{case}: {ref_feat.shape[0]} blocks, reference NIQE {ref_score:.9f}; host restatement: alpha equal, "
              f"features {rel:.3e}, score {srel:.3e}")
    meta["host_vs_reference"] = {"features_rel": feat_rel, "score_rel": score_rel,
                                 "note": "maxima over the cases; the reference computes the plane in float32"}
    if "device_vs_host" in old:
        meta["device_vs_host"] = old["device_vs_host"]
    npz = os.path.join(GOLD, "niqe.npz")
    np.savez_compressed(npz, **out)
    with open(out_json, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", npz, os.path.getsize(npz), "bytes")
    assert os.path.getsize(npz) < (1 << 20)


def device_bound(out_json):
    import torch
    from irm_amd import harness
    from irm_amd.frames import to_device
    params = utils.load_niqe_params(PARAMS)
    meta = json.load(open(os.path.join(GOLD, "niqe.json")))
    z = np.load(os.path.join(GOLD, "niqe.npz"))
    worst = {"alpha_differing_per_frame": 0, "alpha_max_steps": 0.0, "features_rel": 0.0, "score_rel": 0.0}

    def measure(label, frames, crop, order="bgr"):
        """`frames`: one frame, or a list of frames of one shape (one call with K = len)."""
        many = isinstance(frames, list)
        stack = frames if many else [frames]
        up = [to_device(np.ascontiguousarray(f), "cuda:0") for f in stack]
        dev = utils.niqe_features_device(up if many else up[0], crop, params, channel_order=order).cpu().numpy()
        for i, f in enumerate(stack):
            host = utils.niqe_features(utils.niqe_plane(f, crop, "HWC", order), params)
            differing, steps, rel = utils.niqe_feature_distance(dev[i], host)
            hs, ds = utils.niqe_score(host, params), utils.niqe_score(dev[i], params)
            srel = abs(ds - hs) / abs(hs)
            print(f"{label}[{i}]: alpha differing {differing} (max {steps:.3g} steps), features {rel:.3e}, score {srel:.3e}")
            worst["alpha_differing_per_frame"] = max(worst["alpha_differing_per_frame"], differing)
            worst["alpha_max_steps"] = max(worst["alpha_max_steps"], steps)
            worst["features_rel"] = max(worst["features_rel"], rel)
            worst["score_rel"] = max(worst["score_rel"], srel)
    for case, (key, crop) in CASES.items():
        measure(case, z[f"frame_{key}"], crop)
    measure("stack3", list(stack3(z["frame_synth"])), 0)
    black = np.random.default_rng(11).integers(0, 256, size=(96, 384)).astype(np.uint8)     # the NaN-block test's frame
    black[:, :104] = 0
    measure("black_block", black, 0)
    # the frames of the harness test: three synthetic inputs and their DnCNN predictions, crop 2, read as RGB
    from irm_amd import dncnn
    model = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to("cuda:0")
    cfg = utils.get_patch_config("denoising", "gaussian", "DnCNN")
    inputs = [inp for inp, _, _ in harness.synthetic_loader(3, h=200, w=300, c=3, seed_base=4100, blur=3)]
    measure("harness_inputs", inputs, 2, "rgb")
    measure("harness_predictions", [utils.get_model_prediction(model, inp, "cuda:0", **cfg)[0] for inp in inputs], 2, "rgb")
    assert torch.cuda.is_available()
    worst["note"] = ("maxima over the fixture cases, the stack of three, the black-block frame and the harness test's "
                     "frames: device features / score against the float64 host restatement, measured on "
                     f"{torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}")
    meta["device_vs_host"] = worst
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", out_json)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-bound", action="store_true")
    ap.add_argument("--out", default=os.path.join(GOLD, "niqe.json"))
    a = ap.parse_args()
    (device_bound if a.device_bound else generate)(a.out)
