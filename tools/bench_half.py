"""fp32 mode against fp16 mode of the conv stacks (precision="fp16": csrc/conv3x3_h.hip), one process, one GPU.

Configurations: DnCNN nb 17 / 20 on 8 x 256^2 gray and colour tiles, REDNet on 8 x 256^2 gray tiles.  For each one,
fp32 mode first and fp16 mode second:

  forward_us   the forward replayed from a HIP graph, device events around the replay, median of N replays (the kernels
               of one forward back to back; host launch cost is not in it)
  agreement    eight synthetic 256 x 256 uint8 frames, sigma 25, through utils.tiled_forward_device_batch in both modes:
               share of output bytes that differ, the largest difference, PSNR against the clean frames for both

The weights are synthetic (load_synthetic): the PSNR figures only have to agree, they say nothing about denoising.
Prints one JSON line per configuration; --out FILE writes the lines too."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import dncnn, rednet, synth, utils

CONFIGS = [
    ("dncnn17_gray", lambda p: dncnn.DnCNN(1, 1, 64, 17, "R", precision=p), 1),
    ("dncnn20_gray", lambda p: dncnn.DnCNN(1, 1, 64, 20, "R", precision=p), 1),
    ("dncnn20_colour", lambda p: dncnn.DnCNN(3, 3, 64, 20, "R", precision=p), 3),
    ("rednet_gray", lambda p: rednet.REDNet(precision=p), 1),
]


def _forward_us(model, x, n):
    for _ in range(3):
        model(x)
    torch.cuda.synchronize()
    if hasattr(model, "release_workspace"):
        model.release_workspace()                 # the capture allocates the workspace in the graph's own pool
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        model(x)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def _psnr(a, b):
    err = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if err == 0 else float(10 * np.log10(255.0 ** 2 / err))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30, help="graph replays per timing (median)")
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half: needs a GPU")
    dev = torch.device("cuda:0")
    lines = []
    for name, make, c in CONFIGS:
        if a.only and name not in a.only.split(","):
            continue
        x = synth.uniform(7, f"bench_half_{name}", (a.batch, c, a.size, a.size), 0.0, 1.0).to(dev)
        frames = [synth.synth_image_pair(i, a.size, a.size, c, seed_base=7000, blur=0)[1] for i in range(a.batch)]
        frames_dev = [torch.from_numpy(f).to(dev) for f in frames]
        res = {"config": name, "input": f"{a.batch}x{c}x{a.size}x{a.size}", "reps": a.reps}
        outs = {}
        for prec in ("fp32", "fp16"):
            model = make(prec).load_synthetic(42).eval().to(dev)
            med, lo, hi = _forward_us(model, x, a.reps)
            res[f"{prec}_forward_us"], res[f"{prec}_forward_us_min_max"] = med, [lo, hi]
            pairs = utils.tiled_forward_device_batch(model, frames_dev, a.size, 0, False, noise_sigma=25,
                                                     max_batch=a.batch)
            outs[prec] = np.stack([o.cpu().numpy() for o, _ in pairs])
            del model
        clean = np.stack(frames).reshape(outs["fp32"].shape)
        diff = np.abs(outs["fp32"].astype(int) - outs["fp16"].astype(int))
        res["fp16_over_fp32_time"] = res["fp16_forward_us"] / res["fp32_forward_us"]
        res["bytes_differ_share"] = float((diff > 0).mean())
        res["bytes_max_diff"] = int(diff.max())
        res["psnr_fp32_db"], res["psnr_fp16_db"] = _psnr(clean, outs["fp32"]), _psnr(clean, outs["fp16"])
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
