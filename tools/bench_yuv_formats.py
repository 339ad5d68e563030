"""The grid of YUV formats (4:2:0, 4:2:2, 4:4:4 at 8, 10 and 12 bit) on the device, timed: one process, one GPU.

Three groups, one JSON line each (--out FILE appends them: profiles/bench_yuv_formats.jsonl).

  kernels    irm_yuv_to_rgb_f32, irm_rgb_f32_to_yuv and irm_yuv_metrics on one frame (1280 x 720) of every format:
             `--kernel-batch` launches in one HIP graph between two device events, per launch, the median of `--reps`
             replays; the graphs of all formats take turns, round after round.  bytes = the planes plus the float frame
             (12 H W) for a conversion, both sides' planes for the scores; the rate as a share of the 8.0 TB/s HBM peak.
             At this size a frame fits the 256 MiB Infinity Cache: a streaming kernel's rate, not proof of HBM traffic.
  against_parent
             irm_yuv420_to_rgb_f32, irm_rgb_f32_to_yuv420 and irm_yuv420_metrics for "i420", "nv12" and "p010", and
             irm_yuv_to_rgb_f32 and irm_rgb_f32_to_yuv for a planar and a semi-planar format of each sampling structure
             (NEW_FORMATS), from this build against the same symbols of `--parent-lib`, the library built from the parent
             commit, loaded into the same process with ctypes.  Legs `this`, `parent` and `parent_again` alternate;
             `parent_again` against `parent` is the spread that `this` against `parent` is held to
             (`inside_parent_min_max`).  Skipped without --parent-lib.
  whole_call utils.run_model_inference_yuv on "p210" and on "i444p10" planes against utils.get_model_prediction on the
             uint16 RGB frame (Restormer, motion deblurring, patch 512 / overlap 96, synthetic weights), host clocks
             around calls that end in a download, the legs in every order in turn, as tools/bench_yuv.py does for NV12.
"""
import argparse
import ctypes
import itertools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import _hip, restormer, synth, utils, yuv

HBM_PEAK = 8.0e12
OLD = ("irm_yuv420_to_rgb_f32", "irm_rgb_f32_to_yuv420", "irm_yuv420_metrics")
OLD_FORMATS = ("i420", "nv12", "p010")
NEW = ("irm_yuv_to_rgb_f32", "irm_rgb_f32_to_yuv")
#: one planar and one semi-planar format of each sampling structure, both sample types in each
NEW_FORMATS = ("i420", "p010", "i422p10", "nv16", "i444", "p410")


def _graph(fn, batch):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(batch):
            fn()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    return g


def _alternate_graphs(fns, batch, reps):
    """{name: fn} -> {name: [median, min, max] microseconds per launch}: one graph of `batch` launches per leg, replayed
    between two device events; the legs take turns, every round starting one leg further."""
    names = list(fns)
    graphs = {k: _graph(fns[k], batch) for k in names}
    ts = {k: [] for k in names}
    for r in range(reps):
        for i in range(len(names)):
            k = names[(r + i) % len(names)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[k].replay()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / batch)
    return {k: [float(np.median(v)), float(np.min(v)), float(np.max(v))] for k, v in ts.items()}


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _alternate_calls(legs, reps, warmup):
    orders = list(itertools.permutations(legs))
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for r in range(reps):
        for k in orders[r % len(orders)]:
            ts[k].append(_host_ms(legs[k]))
    return {k: [float(np.median(v)), float(np.min(v)), float(np.max(v))] for k, v in ts.items()}


def _planes(rgb_unit, fmt, dev):
    host = yuv.rgb_to_yuv_host(rgb_unit, fmt)
    return host, tuple(utils.to_device(p, dev) for p in host)


def _plane_bytes(planes):
    return sum(p.numel() * p.element_size() for p in planes)


def kernels(a, dev, rgb_unit):
    h, w = rgb_unit.shape[:2]
    fns, nbytes = {}, {}
    keep = []
    for fmt in yuv.YUV_LAYOUTS:
        _, up = _planes(rgb_unit, fmt, dev)
        other = tuple(p.clone() for p in up)
        frame = yuv.yuv_to_rgb_device(up, fmt)
        out = yuv.rgb_to_yuv_device(frame, fmt)
        keep.append((up, other, frame, out))
        fns[f"{fmt}:to_rgb"] = lambda up=up, fmt=fmt: yuv.yuv_to_rgb_device(up, fmt)
        fns[f"{fmt}:to_yuv"] = lambda frame=frame, out=out, fmt=fmt: yuv.rgb_to_yuv_device(frame, fmt, out=out)
        fns[f"{fmt}:metrics"] = lambda up=up, other=other, fmt=fmt: yuv.frame_metrics_yuv_device(up, other, fmt)
        nbytes[f"{fmt}:to_rgb"] = nbytes[f"{fmt}:to_yuv"] = _plane_bytes(up) + 12 * h * w
        nbytes[f"{fmt}:metrics"] = 2 * _plane_bytes(up)
    us = _alternate_graphs(fns, a.kernel_batch, a.reps)
    return {"group": "kernels", "frame": f"{h}x{w}", "kernel_batch": a.kernel_batch, "reps": a.reps,
            "us_median_min_max": us, "bytes": nbytes,
            "share_of_hbm_peak": {k: nbytes[k] / (v[0] * 1e-6) / HBM_PEAK for k, v in us.items()}}


def _bind(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in OLD + NEW:
        fn = getattr(lib, name)
        fn.argtypes = {**_hip.SIGNATURES_YUV, **_hip.SIGNATURES_VIDEO, **_hip.SIGNATURES_METRICS}[name]
        fn.restype = ctypes.c_int
    return lib


def against_parent(a, dev, rgb_unit):
    h, w = rgb_unit.shape[:2]
    this, parent = _hip.load(), _bind(a.parent_lib)
    fns, keep, keys = {}, [], []
    for fmt in dict.fromkeys(OLD_FORMATS + NEW_FORMATS):
        sw, sh = yuv.YUV_LAYOUTS[fmt][:2]
        _, up = _planes(rgb_unit, fmt, dev)
        other = tuple(p.clone() for p in up)
        frame = yuv.yuv_to_rgb_device(up, fmt)
        out = tuple(torch.empty_like(p) for p in up)
        y, u, v, step, py, pc = yuv._device_planes(up, fmt, False)[2:]
        oy, ou, ov = yuv._device_planes(out, fmt, False)[2:5]
        ty, tu, tv = yuv._device_planes(other, fmt, False)[2:5]
        opt = yuv._kernel_options(fmt, "bt709", False, "left", False)
        words = 2 * (yuv._metric_tiles(h, w) + 2 * yuv._metric_tiles(h // sh, w // sw))
        ws = torch.empty(words, dtype=torch.float64, device=dev)
        sse = torch.empty(3, dtype=torch.int64, device=dev)
        ssim = torch.empty(3, dtype=torch.float64, device=dev)
        keep.append((up, other, frame, out, ws, sse, ssim))
        P = _hip.ptr
        args = {"irm_yuv420_to_rgb_f32": (P(y), P(u), P(v), step, py, pc, *opt, h, w, P(frame)),
                "irm_rgb_f32_to_yuv420": (P(frame), P(oy), P(ou), P(ov), step, py, pc, *opt, h, w),
                "irm_yuv420_metrics": (P(y), P(u), P(v), step, py, pc, P(ty), P(tu), P(tv), step, py, pc, opt[0], opt[1],
                                       0, h, w, P(sse), P(ssim), P(ws), words),
                "irm_yuv_to_rgb_f32": (P(y), P(u), P(v), step, py, pc, sw, sh, *opt, h, w, P(frame)),
                "irm_rgb_f32_to_yuv": (P(frame), P(oy), P(ou), P(ov), step, py, pc, sw, sh, *opt, h, w)}
        for name in (OLD if fmt in OLD_FORMATS else ()) + (NEW if fmt in NEW_FORMATS else ()):
            keys.append(f"{fmt}:{name}")
            for leg, lib in (("this", this), ("parent", parent), ("parent_again", parent)):
                def call(fn=getattr(lib, name), args=args[name]):
                    rc = fn(*args, torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, rc
                fns[f"{fmt}:{name}:{leg}"] = call
    us = _alternate_graphs(fns, a.kernel_batch, a.reps)
    rows = {}
    for key in keys:
        t, p, q = (us[f"{key}:{leg}"] for leg in ("this", "parent", "parent_again"))
        rows[key] = {"this": t, "parent": p, "parent_again": q, "this_minus_parent_us": t[0] - p[0],
                     "parent_spread_us": abs(q[0] - p[0]),
                     "inside_parent_min_max": min(p[1], q[1]) <= t[0] <= max(p[2], q[2])}
    return {"group": "against_parent", "frame": f"{h}x{w}", "kernel_batch": a.kernel_batch, "reps": a.reps, "rows": rows}


def whole_call(a, dev, blurred):
    h, w = blurred.shape[:2]
    model = restormer.Restormer(LayerNorm_type="WithBias").load_synthetic(42).eval().to(dev)
    cfg = utils.get_patch_config("deblurring", "motion", "Restormer")
    unit = blurred.astype(np.float32) / np.float32(255.0)
    rgb16 = np.rint(unit * np.float32(65535.0)).astype(np.uint16)
    p210, i444p10 = yuv.rgb_to_yuv_host(unit, "p210"), yuv.rgb_to_yuv_host(unit, "i444p10")
    legs = {"yuv_call_p210": lambda: utils.run_model_inference_yuv(model, p210, dev, fmt="p210", **cfg)[0],
            "yuv_call_i444p10": lambda: utils.run_model_inference_yuv(model, i444p10, dev, fmt="i444p10", **cfg)[0],
            "rgb16_call": lambda: utils.get_model_prediction(model, rgb16, dev, **cfg)[0],
            "rgb16_call_again": lambda: utils.get_model_prediction(model, rgb16, dev, **cfg)[0]}
    ms = _alternate_calls(legs, a.call_reps, a.warmup)
    m = {k: v[0] for k, v in ms.items()}
    return {"group": "whole_call", "frame": f"{h}x{w}", "model": "Restormer deblurring", **cfg, "reps": a.call_reps,
            "ms_median_min_max": ms, "p210_minus_rgb16_ms": m["yuv_call_p210"] - m["rgb16_call"],
            "i444p10_minus_rgb16_ms": m["yuv_call_i444p10"] - m["rgb16_call"],
            "rgb16_spread_ms": abs(m["rgb16_call_again"] - m["rgb16_call"]),
            "bytes_up": {"p210": 4 * h * w, "i444p10": 6 * h * w, "rgb16": 6 * h * w}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--call-reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-batch", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="libirm_hip.so built from the parent commit")
    ap.add_argument("--groups", default="kernels,against_parent,whole_call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv_formats: needs a GPU")
    dev = torch.device("cuda:0")
    blurred, _ = synth.synth_image_pair(0, a.height, a.width, 3, seed_base=1000, blur=15)
    unit = blurred.astype(np.float32) / np.float32(255.0)
    lines = []
    for group in a.groups.split(","):
        if group == "kernels":
            lines.append(kernels(a, dev, unit))
        elif group == "against_parent" and a.parent_lib:
            lines.append(against_parent(a, dev, unit))
        elif group == "whole_call":
            lines.append(whole_call(a, dev, blurred))
    for res in lines:
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for res in lines:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
