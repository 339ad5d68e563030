"""Cost of estimating the noise level of a 1280x720 frame on the GPU (irm_noise_hh_stats), against irm_frame_metrics on
a frame of the same shape as the yardstick, against the numpy twin, and the overhead of the sigma-routed call.

  kernel us      events around a graph replay of R calls (the three or five launches of a call, no host enqueue cost)
  visible ms     estimate_noise_sigma_device / estimate_noise_sigma_yuv_device on operands already on the GPU, wall clock
                 including the one synchronising copy
  host ms        utils.estimate_noise_sigma / estimate_noise_sigma_yuv on the host arrays, wall clock
  us per MB      kernel time per megabyte of operand read (the 16-bit legs read their frame twice)

Legs: a uint8 RGB frame with sigma-25 noise, the same frame noise-free, a flat frame (every block in bin 0: the
contention case), a uint16 RGB frame, the Y plane of an NV12 and of a P010 frame.  They alternate in one process,
--rounds times; every figure is the median with the minimum and the maximum.  Then utils.run_model_inference_auto over a
bank of three colour DnCNN-20 against utils.get_model_prediction with the model it picks.
--kernels-only runs just the device calls (for a `rocprofv3 --kernel-trace --stats` run of its own).
Prints one JSON line at the end and writes it to --out (default profiles/bench_noise.jsonl)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import dncnn, harness, utils, yuv

H, W = 720, 1280


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def _bits(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the legs")
    ap.add_argument("--reps", type=int, default=50, help="device calls per graph replay")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_noise.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise: needs a GPU")
    dev = torch.device("cuda:0")
    _, clean, _ = next(iter(harness.synthetic_loader(1, h=H, w=W, c=3)))
    noise = np.random.RandomState(125).normal(0, 25.0, clean.shape)
    noisy = np.clip(np.rint(clean + noise), 0, 255).astype(np.uint8)
    noisy16 = np.clip(np.rint((clean + noise) * 257.0), 0, 65535).astype(np.uint16)
    flat = np.full_like(clean, 128)
    planes = {fmt: yuv.rgb_to_yuv420_host(noisy.astype(np.float32) / np.float32(255), fmt) for fmt in ("nv12", "p010")}
    host = {"u8_noisy": noisy, "u8_clean": clean, "u8_flat": flat, "u16_noisy": noisy16}
    on_dev = {k: _bits(v).to(dev) for k, v in host.items()}
    y_dev = {fmt: (_bits(planes[fmt][0]).to(dev),) for fmt in planes}
    clean_dev = torch.from_numpy(clean).to(dev)
    mbytes = {"u8_noisy": H * W * 3 / 1e6, "u8_clean": H * W * 3 / 1e6, "u8_flat": H * W * 3 / 1e6,
              "u16_noisy": 2 * H * W * 3 * 2 / 1e6, "nv12_y": H * W / 1e6, "p010_y": 2 * H * W * 2 / 1e6,
              "metrics_u8": 2 * H * W * 3 / 1e6}
    enqueue = {k: (lambda k=k: utils.noise_stats_device(on_dev[k])) for k in host}
    visible = {k: (lambda k=k: utils.estimate_noise_sigma_device(on_dev[k])) for k in host}
    twin = {k: (lambda k=k: utils.estimate_noise_sigma(host[k])) for k in host}
    for fmt in planes:
        enqueue[fmt + "_y"] = lambda fmt=fmt: utils.noise_stats_yuv_device(y_dev[fmt], fmt)
        visible[fmt + "_y"] = lambda fmt=fmt: utils.estimate_noise_sigma_yuv_device(y_dev[fmt], fmt)
        twin[fmt + "_y"] = lambda fmt=fmt: utils.estimate_noise_sigma_yuv(planes[fmt], fmt)
    enqueue["metrics_u8"] = lambda: utils.frame_metrics_device([on_dev["u8_noisy"]], [clean_dev])
    visible["metrics_u8"] = lambda: utils.calculate_metrics_device(on_dev["u8_noisy"], clean_dev)
    twin["metrics_u8"] = lambda: utils.calculate_metrics(noisy, clean)
    legs = list(enqueue)

    if a.kernels_only:
        for _ in range(20):
            for leg in legs:
                enqueue[leg]()
        torch.cuda.synchronize()
        print(f"kernels-only: 20 x ({', '.join(legs)}) calls done")
        return

    graphs = {}
    for leg in legs:
        for _ in range(3):
            enqueue[leg]()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.reps):
                enqueue[leg]()
        g.replay()
        torch.cuda.synchronize()
        graphs[leg] = g
        visible[leg]()
    kernel_us = {leg: [] for leg in legs}
    visible_ms = {leg: [] for leg in legs}
    host_ms = {leg: [] for leg in legs}
    for r in range(a.rounds):
        for leg in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[leg].replay()
            e1.record()
            e1.synchronize()
            kernel_us[leg].append(e0.elapsed_time(e1) * 1e3 / a.reps)
            t0 = time.perf_counter()
            for _ in range(10):
                visible[leg]()
            visible_ms[leg].append((time.perf_counter() - t0) * 1e2)
            if r < 3:
                t0 = time.perf_counter()
                twin[leg]()
                host_ms[leg].append((time.perf_counter() - t0) * 1e3)
    res = {"frame": f"{W}x{H}, synthetic_loader target + N(0, 25), rounded and clipped; nv12 / p010: the Y plane of its "
                    "BT.709 limited-range planes", "rounds": a.rounds, "reps": a.reps}
    for leg in legs:
        res[leg] = {"read_MB": mbytes[leg], "kernel_us": _stats(kernel_us[leg]), "visible_ms": _stats(visible_ms[leg]),
                    "host_ms": _stats(host_ms[leg]), "kernel_us_per_MB": float(np.median(kernel_us[leg])) / mbytes[leg]}
    yard = res["metrics_u8"]["kernel_us_per_MB"]
    for leg in legs[:-1]:
        res[leg]["per_byte_vs_metrics_u8"] = res[leg]["kernel_us_per_MB"] / yard
        res[leg]["sigma_device"], res[leg]["sigma_host"] = visible[leg](), twin[leg]()
    res["flat_over_noisy_kernel_time"] = res["u8_flat"]["kernel_us"]["median"] / res["u8_noisy"]["kernel_us"]["median"]
    res["clean_over_noisy_kernel_time"] = res["u8_clean"]["kernel_us"]["median"] / res["u8_noisy"]["kernel_us"]["median"]

    # the routed call against the plain call with the model it picks
    bank = utils.SigmaBank({s: dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(s).eval().to(dev) for s in (15, 25, 50)})
    cfg = utils.get_patch_config("denoising", "gaussian", "DnCNN")
    pred, _, est, used = utils.run_model_inference_auto(bank, noisy, dev, **cfg)
    want, _ = utils.get_model_prediction(bank.models[used], noisy, dev, **cfg)
    auto_ms, plain_ms = [], []
    for _ in range(a.rounds):
        auto_ms.append(utils.run_model_inference_auto(bank, noisy, dev, **cfg)[1])
        plain_ms.append(utils.get_model_prediction(bank.models[used], noisy, dev, **cfg)[1])
    res["routed"] = {"model": "DnCNN-20 colour x 3", "patch_config": cfg, "sigma_est": est, "sigma_used": used,
                     "byte_identical": bool(np.array_equal(pred, want)), "auto_ms": _stats(auto_ms),
                     "plain_ms": _stats(plain_ms),
                     "overhead_ms": float(np.median(auto_ms) - np.median(plain_ms))}

    for k, v in res.items():
        print(f"{k}: {v}")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
