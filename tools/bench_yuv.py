"""NV12 video frames on the device pipeline, timed end to end: one process, one GPU.

One 1280 x 720 frame (the synthetic blurred frame of bench.py) through Restormer (motion deblurring, patch 512 /
overlap 96, synthetic weights), four legs that take turns, every round in another order:

  yuv_call       (a) utils.run_model_inference_yuv on the NV12 planes: 1.5 bytes per pixel each way, the two conversion
                 kernels, the float32 frame never rounded to 255 RGB levels
  rgb_call       (b) utils.get_model_prediction on the uint8 RGB frame: what a caller with RGB frames has
  rgb_call_again (b) once more in the same round: the spread of (b) against itself, the yardstick for (a) - (b)
  rgb_call_host  (c) what a caller with video pays without the device path: utils.yuv420_to_rgb_host rounded to uint8,
                 leg (b), utils.rgb_to_yuv420_host of the result / 255

All four are host clocks around a call that ends in a download; median, minimum and maximum in milliseconds.

The two kernels on their own: `--kernel-batch` launches in one HIP graph between two device events, per launch, the
median of `--reps` replays; bytes = the planes (1.5 H W) plus the float frame (12 H W), and the rate as a share of the
8.0 TB/s HBM peak (6.29 TB/s is what a float4 copy reaches).  At 1280 x 720 the 12.4 MB fit the 256 MiB Infinity
Cache, so a warm repetition need not reach HBM: the figure is a streaming kernel's rate, not proof of HBM traffic.

PSNR-Y: the Y plane of the NV12 result against the Y plane of the converted sharp target
(utils.calculate_metrics_device on [H][W] frames), next to the same figure for the RGB call's result converted on the
host.  Prints one JSON line; --out FILE writes it too."""
import argparse
import itertools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import restormer, synth, utils

HBM_PEAK = 8.0e12


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _alternate(legs, reps, warmup):
    """legs: {name: fn} -> {name: [median, min, max]}.  The legs take turns, round r in the r-th permutation of their
    order (24 rounds: every order of four legs once), so every leg follows every other equally often: whatever follows
    the host-conversion leg starts on a GPU that has idled for that leg's numpy part and takes 0.8 - 1.0 ms longer
    (measured: 49.4 against 48.3 ms for yuv_call, 49.2 against 48.4 ms for rgb_call), and in a fixed or merely rotated
    order one leg alone pays for that."""
    orders = list(itertools.permutations(legs))
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for r in range(reps):
        for k in orders[r % len(orders)]:
            ts[k].append(_host_ms(legs[k]))
    return {k: [float(np.median(v)), float(np.min(v)), float(np.max(v))] for k, v in ts.items()}


def _kernel_us(fn, batch, reps):
    """Microseconds per launch: `batch` launches captured into one HIP graph (a chain of kernel nodes: the Python
    binding cannot enqueue as fast as these kernels run), replayed between two device events, the median of `reps`
    replays.  A launch includes the boundary to the next kernel of the chain."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(batch):
            fn()
    for _ in range(2):
        g.replay()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / batch)
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def _unit(u8):
    return u8.astype(np.float32) / np.float32(255.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-batch", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv: needs a GPU")
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    model = restormer.Restormer(LayerNorm_type="WithBias").load_synthetic(42).eval().to(dev)
    cfg = utils.get_patch_config("deblurring", "motion", "Restormer")
    blurred, sharp = synth.synth_image_pair(0, h, w, 3, seed_base=1000, blur=15)
    opts = dict(matrix="bt709", full_range=False, siting="left")
    planes = utils.rgb_to_yuv420_host(_unit(blurred), "nv12", **opts)
    target_y = utils.rgb_to_yuv420_host(_unit(sharp), "nv12", **opts)[0]

    def yuv_call():
        return utils.run_model_inference_yuv(model, planes, dev, fmt="nv12", **opts, **cfg)[0]

    def rgb_call(frame=blurred):
        return utils.get_model_prediction(model, frame, dev, **cfg)[0]

    def rgb_call_host():
        rgb = np.rint(utils.yuv420_to_rgb_host(planes, "nv12", **opts) * np.float32(255.0)).astype(np.uint8)
        return utils.rgb_to_yuv420_host(_unit(rgb_call(rgb)), "nv12", **opts)
    legs = {"yuv_call": yuv_call, "rgb_call": rgb_call, "rgb_call_again": rgb_call, "rgb_call_host": rgb_call_host}
    ms = _alternate(legs, a.reps, a.warmup)
    res = {"group": "yuv", "frame": f"{h}x{w}", "fmt": "nv12", "model": "Restormer deblurring", **cfg, **opts,
           "reps": a.reps, "ms_median_min_max": ms}
    m = {k: v[0] for k, v in ms.items()}
    res["yuv_minus_rgb_ms"] = m["yuv_call"] - m["rgb_call"]
    res["rgb_spread_ms"] = {"again_minus_first": m["rgb_call_again"] - m["rgb_call"],
                            "max_minus_min": max(ms["rgb_call"][2], ms["rgb_call_again"][2])
                            - min(ms["rgb_call"][1], ms["rgb_call_again"][1])}
    res["host_path_over_yuv_call"] = m["rgb_call_host"] / m["yuv_call"]

    # ---- the two kernels on their own
    up = tuple(utils.to_device(p, dev) for p in planes)
    frame = utils.yuv420_to_rgb_device(up, "nv12", **opts)
    out = utils.rgb_to_yuv420_device(frame, "nv12", **opts)
    nbytes = h * w * 3 // 2 + 12 * h * w
    res["kernel_bytes"] = nbytes
    res["kernel_us_median_min_max"] = {
        "irm_yuv420_to_rgb_f32": _kernel_us(lambda: utils.yuv420_to_rgb_device(up, "nv12", **opts), a.kernel_batch, a.reps),
        "irm_rgb_f32_to_yuv420": _kernel_us(lambda: utils.rgb_to_yuv420_device(frame, "nv12", out=out, **opts),
                                            a.kernel_batch, a.reps)}
    res["kernel_bytes_per_s"] = {k: nbytes / (v[0] * 1e-6) for k, v in res["kernel_us_median_min_max"].items()}
    res["kernel_share_of_hbm_peak"] = {k: v / HBM_PEAK for k, v in res["kernel_bytes_per_s"].items()}

    # ---- quality on the luma plane
    ty = torch.from_numpy(target_y).to(dev)
    res["psnr_y"] = {
        "input": utils.calculate_metrics_device(torch.from_numpy(planes[0]).to(dev), ty)[0],
        "yuv_call": utils.calculate_metrics_device(torch.from_numpy(yuv_call()[0]).to(dev), ty)[0],
        "rgb_call_host": utils.calculate_metrics_device(torch.from_numpy(rgb_call_host()[0]).to(dev), ty)[0]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
