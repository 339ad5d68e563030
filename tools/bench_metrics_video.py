"""Cost of scoring a 1280x720 frame that never passed through 255 RGB levels: a float32 RGB frame
(irm_frame_metrics_f32) and the planes of an NV12 / P010 frame (irm_yuv420_metrics), against the uint8 RGB frame of
irm_frame_metrics as the yardstick, and against their host twins.

  kernel us      events around a graph replay of R calls (the two launches of a call, no host enqueue cost)
  visible ms     calculate_metrics_f32_device / calculate_metrics_yuv_device / calculate_metrics_device on operands
                 already on the GPU, wall clock including the one synchronising copy
  host ms        utils.calculate_metrics / yuv.calculate_metrics_yuv on the host arrays, wall clock
  us per MB      kernel time per megabyte of operand read (both sides)

The legs alternate in one process, --rounds times; every figure is the median with the minimum and the maximum.
--kernels-only runs just the device calls (for a `rocprofv3 --kernel-trace --stats` run of its own).
Prints one JSON line at the end and writes it to --out (default profiles/bench_metrics_video.jsonl)."""
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
from irm_amd import harness, utils, yuv

H, W = 720, 1280


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def _bits(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def _planes(frame_u8, fmt):
    """The planes of an RGB frame in `fmt` (BT.709, limited range) on the host."""
    return yuv.rgb_to_yuv420_host(frame_u8.astype(np.float32) / np.float32(255), fmt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the legs")
    ap.add_argument("--reps", type=int, default=50, help="device calls per graph replay")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_metrics_video.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics_video: needs a GPU")
    dev = torch.device("cuda:0")
    inp, tgt, _ = next(iter(harness.synthetic_loader(1, h=H, w=W, c=3)))
    host = {"uint8": (inp, tgt), "float32": (inp.astype(np.float32) / np.float32(255), tgt.astype(np.float32) / np.float32(255)),
            "nv12": (_planes(inp, "nv12"), _planes(tgt, "nv12")), "p010": (_planes(inp, "p010"), _planes(tgt, "p010"))}
    on_dev = {"uint8": tuple(torch.from_numpy(x).to(dev) for x in host["uint8"]),
              "float32": tuple(torch.from_numpy(x).to(dev) for x in host["float32"])}
    for fmt in ("nv12", "p010"):
        on_dev[fmt] = tuple(tuple(_bits(p).to(dev) for p in side) for side in host[fmt])
    mbytes = {"uint8": 2 * H * W * 3 / 1e6, "float32": 2 * H * W * 3 * 4 / 1e6, "nv12": 2 * H * W * 1.5 / 1e6,
              "p010": 2 * H * W * 3 / 1e6}
    enqueue = {"uint8": lambda: utils.frame_metrics_device([on_dev["uint8"][0]], [on_dev["uint8"][1]]),
               "float32": lambda: utils.frame_metrics_f32_device([on_dev["float32"][0]], [on_dev["float32"][1]]),
               "nv12": lambda: yuv.frame_metrics_yuv_device(*on_dev["nv12"], "nv12"),
               "p010": lambda: yuv.frame_metrics_yuv_device(*on_dev["p010"], "p010")}
    visible = {"uint8": lambda: utils.calculate_metrics_device(*on_dev["uint8"]),
               "float32": lambda: utils.calculate_metrics_f32_device(*on_dev["float32"]),
               "nv12": lambda: yuv.calculate_metrics_yuv_device(*on_dev["nv12"], "nv12"),
               "p010": lambda: yuv.calculate_metrics_yuv_device(*on_dev["p010"], "p010")}
    twin = {"uint8": lambda: utils.calculate_metrics(*host["uint8"]),
            "float32": lambda: utils.calculate_metrics(*host["float32"]),
            "nv12": lambda: yuv.calculate_metrics_yuv(*host["nv12"], "nv12"),
            "p010": lambda: yuv.calculate_metrics_yuv(*host["p010"], "p010")}
    legs = list(enqueue)

    if a.kernels_only:
        for _ in range(20):
            for leg in legs:
                enqueue[leg]()
        torch.cuda.synchronize()
        print("kernels-only: 20 x (uint8, float32, nv12, p010) calls done")
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
    res = {"frame": f"{W}x{H}, synthetic_loader (degraded input vs target); nv12 / p010: its BT.709 limited-range planes",
           "rounds": a.rounds, "reps": a.reps}
    for leg in legs:
        res[leg] = {"operand_MB": mbytes[leg], "kernel_us": _stats(kernel_us[leg]), "visible_ms": _stats(visible_ms[leg]),
                    "host_ms": _stats(host_ms[leg]),
                    "kernel_us_per_MB": float(np.median(kernel_us[leg])) / mbytes[leg]}
    yard = res["uint8"]["kernel_us_per_MB"]
    for leg in legs[1:]:
        res[leg]["per_byte_vs_uint8"] = res[leg]["kernel_us_per_MB"] / yard
    # the replayed calls computed what the host computes
    ph, sh = twin["float32"]()
    pd, sd = visible["float32"]()
    res["float32_dSSIM_device_minus_host"], res["float32_dPSNR_device_minus_host"] = sd - sh, pd - ph
    for fmt in ("nv12", "p010"):
        hm, dm = twin[fmt](), visible[fmt]()
        res[f"{fmt}_max_abs_d_device_minus_host"] = float(max(abs(x - y) for x, y in zip(dm, hm)))

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
