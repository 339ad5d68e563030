"""Cost of the aligned scoring protocol (irm_amd/align.py) on one 680 x 773 uint8 pair - the size of a RealBlur frame -
on the GPU, against its float64 numpy statement on the same machine:

  entry ms       HIP events around each of the three entry points on its own, --reps calls back to back:
                 irm_align_prepare (4 launches), irm_ecc_iterate (2 x iterations launches), irm_aligned_metrics (2)
  device ms      events around --reps back-to-back runs of the whole protocol, per run (launch gaps included)
  visible ms     calculate_metrics_aligned_device on frames already on the GPU, wall clock including the allocations
                 and the one synchronising copy
  host ms        calculate_metrics_aligned, the numpy statement, once (--no-host skips it: it takes minutes)

The pair is an analytic image sampled exactly under a known homography (rotation 0.4 degrees, scales 1.004 / 0.997, shift
(1.7, -0.9) pixels, perspective (2e-5, -1e-5) / 8), gain 0.93, rounded to uint8.  One JSON line to --out (default
profiles/bench_aligned.jsonl).  cv2 is not installed: there is no OpenCV leg."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import _hip, align
from irm_amd.frames import to_device

H, W = 680, 773


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def make_pair(h, w, seed=24):
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    a = math.radians(0.4)
    lin = np.array([[1.004 * math.cos(a), -0.997 * math.sin(a)], [1.004 * math.sin(a), 0.997 * math.cos(a)]])
    m = np.eye(3)
    m[:2, :2] = lin
    m[:2, 2] = np.array([cx, cy]) - lin @ np.array([cx, cy]) + np.array([1.7, -0.9])
    m[2, :2] = (2e-5 / 8, -1e-5 / 8)
    rng = np.random.default_rng(seed)
    waves = [(rng.uniform(-0.03, 0.03, (24, 2)), rng.uniform(0, 2 * math.pi, 24), rng.uniform(0.5, 1.0, 24)) for _ in range(3)]

    def image(x, y):
        out = []
        for f, ph, amp in waves:
            amp = amp * (0.45 / amp.sum())
            v = 0.5
            for k in range(24):
                v = v + amp[k] * np.sin(2 * math.pi * (f[k, 0] * x + f[k, 1] * y) + ph[k])
            out.append(v)
        return np.stack(out, axis=-1)

    def apply(mm, x, y):
        den = mm[2, 0] * x + mm[2, 1] * y + mm[2, 2]
        return (mm[0, 0] * x + mm[0, 1] * y + mm[0, 2]) / den, (mm[1, 0] * x + mm[1, 1] * y + mm[1, 2]) / den
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    target = np.rint(255.0 * image(x, y)).astype(np.uint8)
    ux, uy = apply(np.linalg.inv(m), x, y)
    pred = np.rint(255.0 * 0.93 * image(ux, uy)).astype(np.uint8)
    return pred, target, m


def timed(fn, reps, rounds):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return _stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="device calls per timed burst")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy statement (minutes at this size)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_aligned.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_aligned: needs a GPU")
    dev = torch.device("cuda:0")
    pred, target, truth = make_pair(H, W)
    p, t = to_device(pred, dev), to_device(target, dev)
    planes = torch.empty(4, H, W, dtype=torch.float32, device=dev)
    state = torch.zeros(20, dtype=torch.float64, device=dev)          # gain, rho, map [9], out [9]
    eye = torch.eye(3, dtype=torch.float64, device=dev).reshape(-1)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(align.prepare_words(H, W), align.iterate_words(H, W), align.metrics_words(H, W)),
                     dtype=torch.float64, device=dev)
    pp = [_hip.ptr(planes[k]) for k in range(4)]

    def prepare():
        _hip.call("irm_align_prepare", _hip.ptr(p), _hip.ptr(t), 0, H, W, _hip.ptr(state[0:1]), _hip.ptr(status), *pp,
                  _hip.ptr(ws), ws.numel())

    def iterate():
        state[2:11] = eye
        _hip.call("irm_ecc_iterate", *pp, H, W, a.iterations, _hip.ptr(state[2:11]), _hip.ptr(state[1:2]),
                  _hip.ptr(status), _hip.ptr(ws), ws.numel())

    def score():
        _hip.call("irm_aligned_metrics", _hip.ptr(p), _hip.ptr(t), 0, H, W, _hip.ptr(state[0:1]), _hip.ptr(state[2:11]),
                  _hip.ptr(state[11:20]), _hip.ptr(status), None, None, _hip.ptr(ws), ws.numel())

    def whole():
        prepare()
        iterate()
        score()
    for _ in range(2):
        whole()
    torch.cuda.synchronize()
    dev_res = align.calculate_metrics_aligned_device(p, t, a.iterations)
    entry_ms = {"irm_align_prepare": timed(prepare, a.reps, a.rounds), "irm_ecc_iterate": timed(iterate, a.reps, a.rounds),
                "irm_aligned_metrics": timed(score, a.reps, a.rounds)}
    device_ms = timed(whole, a.reps, a.rounds)
    visible = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            align.calculate_metrics_aligned_device(p, t, a.iterations)
        visible.append((time.perf_counter() - t0) * 1e3 / a.reps)
    print("device legs done", flush=True)

    def off(m):
        d = []
        for x, y in ((0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0)):
            v, u = m @ np.array([x, y, 1.0]), truth @ np.array([x, y, 1.0])
            d.append(math.hypot(v[0] / v[2] - u[0] / u[2], v[1] / v[2] - u[1] / u[2]))
        return float(np.mean(d))
    res = {"frame": f"{W}x{H} uint8 pair, analytic image under a known homography", "iterations": a.iterations,
           "rounds": a.rounds, "reps": a.reps, "entry_ms": entry_ms, "iteration_us": entry_ms["irm_ecc_iterate"]["median"] * 1e3 / a.iterations,
           "device_ms": device_ms, "visible_ms": _stats(visible),
           "device": {"psnr": dev_res.psnr, "ssim": dev_res.ssim, "rho": dev_res.rho, "coverage": dev_res.coverage,
                      "gain": dev_res.gain, "ok": dev_res.ok, "corner_px_from_truth": off(dev_res.map)}}
    if not a.no_host:
        t0 = time.perf_counter()
        host = align.calculate_metrics_aligned(pred, target, a.iterations)
        res["host_ms"] = (time.perf_counter() - t0) * 1e3
        res["host"] = {"psnr": host.psnr, "ssim": host.ssim, "rho": host.rho, "coverage": host.coverage,
                       "corner_px_from_truth": off(host.map)}
        res["dpsnr"], res["dssim"] = abs(host.psnr - dev_res.psnr), abs(host.ssim - dev_res.ssim)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
