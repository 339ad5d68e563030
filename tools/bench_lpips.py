"""Cost of LPIPS (AlexNet) on a 1280x720 pair on the GPU (utils.frame_lpips_device), per frame dtype, with synthetic
parameters:

  kernel us      per launch family, HIP events around each launch (ops.KernelTimer): lpips_pack (2 launches per pair),
                 convkxk (2), pool3x3 (2), conv3x3 / conv3x3_f16x3 (3), lpips_head (5); the sum over a call as well
  device ms      events around --reps back-to-back calls of frame_lpips_device, per call (launch gaps included)
  visible ms     calculate_lpips_device on frames already on the GPU, wall clock including the one synchronising copy
  host ms        utils.calculate_lpips, the float64 torch-CPU statement, once
  torch ms       the same network composed from torch's library ops (conv2d, max_pool2d, elementwise head) in float32 on
                 the same GPU, events around --reps calls: a yardstick for time only, its value is printed beside ours

One JSON line per leg (uint8, uint16, float32) to --out (default profiles/bench_lpips.jsonl)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

import irm_amd  # noqa: F401
from irm_amd import harness, ops, perceptual, synth, utils
from irm_amd.frames import to_device

H, W = 720, 1280


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def synthetic_params(seed=7):
    shapes, lin = {}, {}
    for l, (p, co, ci, k, _, _, _) in enumerate(perceptual.TRUNK_ALEX):
        shapes[p + ".weight"], shapes[p + ".bias"] = (co, ci, k, k), (co,)
        lin[f"lin{l}.model.1.weight"] = (1, co, 1, 1)
    lin_state = {k: v.abs() for k, v in synth.synth_state_dict(lin, seed=seed + 1).items()}
    return utils.lpips_params_from_state(synth.synth_state_dict(shapes, seed=seed), lin_state)


def torch_lpips(pred, target, params, dev):
    """The network from torch's library ops, float32 on the GPU; returns a closure and its operands stay on `dev`."""
    peak = {torch.uint8: 255.0, torch.int16: 65535.0, torch.float32: 1.0}[pred.dtype]
    shift = torch.tensor(perceptual.LPIPS_SHIFT, device=dev).view(1, 3, 1, 1)
    scale = torch.tensor(perceptual.LPIPS_SCALE, device=dev).view(1, 3, 1, 1)
    convs = [(w.to(dev), b.to(dev)) for w, b in params.convs]
    lins = [v.to(dev).view(1, -1, 1, 1) for v in params.lin]

    def unit(t):
        x = ((t.int() & 0xFFFF) if t.dtype == torch.int16 else t).float() / peak     # int16: the uint16 bit pattern
        return ((2 * x - 1).permute(2, 0, 1)[None] - shift) / scale

    def run():
        t = torch.cat([unit(pred), unit(target)])
        total = torch.zeros((), device=dev)
        for (_, _, _, _, stride, pad, pool), (w, b), lin in zip(perceptual.TRUNK_ALEX, convs, lins):
            if pool:
                t = F.max_pool2d(t, 3, 2)
            t = F.relu(F.conv2d(t, w, b, stride=stride, padding=pad))
            n = t / (t.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            total = total + (lin * (n[:1] - n[1:]) ** 2).sum(1).mean()
        return total
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="device calls per timed burst")
    ap.add_argument("--no-host", action="store_true", help="skip the float64 host statement (tens of seconds per leg)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_lpips.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: needs a GPU")
    dev = torch.device("cuda:0")
    params = synthetic_params()
    inp, tgt, _ = next(iter(harness.synthetic_loader(1, h=H, w=W, c=3)))
    pairs = {"uint8": (inp, tgt),
             "uint16": (inp.astype(np.uint16) * 257, tgt.astype(np.uint16) * 257),
             "float32": ((inp / 255.0).astype(np.float32), (tgt / 255.0).astype(np.float32))}
    lines = []
    for leg, (p, t) in pairs.items():
        pd, td = to_device(p, dev), to_device(t, dev)
        call = lambda: utils.frame_lpips_device([pd], [td], params)           # noqa: E731
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        value = utils.calculate_lpips_device(pd, td, params)
        ops.TIMER = timer = ops.KernelTimer()
        try:
            for _ in range(a.reps):
                call()
            families = timer.summary()
        finally:
            ops.TIMER = None
        kernel_us = {k: {"launches_per_call": v["launches"] // a.reps, "us_per_launch": v["ms"] * 1e3 / v["launches"],
                         "us_per_call": v["ms"] * 1e3 / a.reps} for k, v in families.items()}
        device_ms, visible_ms = [], []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            e1.synchronize()
            device_ms.append(e0.elapsed_time(e1) / a.reps)
            t0 = time.perf_counter()
            for _ in range(a.reps):
                utils.calculate_lpips_device(pd, td, params)
            visible_ms.append((time.perf_counter() - t0) * 1e3 / a.reps)
        print(f"{leg}: device legs done", flush=True)
        run = torch_lpips(pd, td, params, dev)
        for _ in range(3):
            yard = run()
        torch.cuda.synchronize()
        torch_ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                run()
            e1.record()
            e1.synchronize()
            torch_ms.append(e0.elapsed_time(e1) / a.reps)
        print(f"{leg}: torch yardstick done", flush=True)
        res = {"leg": leg, "frame": f"{W}x{H} pair, synthetic_loader input against its target, synthetic parameters",
               "rounds": a.rounds, "reps": a.reps, "kernel_us": kernel_us,
               "kernel_us_per_call": float(sum(v["us_per_call"] for v in kernel_us.values())),
               "device_ms": _stats(device_ms), "visible_ms": _stats(visible_ms), "torch_ms": _stats(torch_ms),
               "lpips_device": value, "lpips_torch_f32": float(yard)}
        if not a.no_host:
            t0 = time.perf_counter()
            res["lpips_host"] = utils.calculate_lpips(p, t, params)
            res["host_ms"] = (time.perf_counter() - t0) * 1e3
            res["rel_err_device"] = abs(value - res["lpips_host"]) / res["lpips_host"]
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
