"""What the frame stream buys: one process, one GPU, 1280 x 720 frames from harness.synthetic_loader.

Per workload three kinds of leg, `--frames` frames each after a warm-up group, taking turns (round r starts with leg
r, as tools/ab_bench.sh alternates its two sides); the figure of a leg is the median over the rounds, ms per frame on
the host clock around work that ends in a synchronise:

  loop      (a) the per-frame loop of utils.get_model_prediction / run_model_inference_yuv: upload from pageable
            memory, forward, download, synchronise, frame by frame
  resident  (b) the ceiling: tiled_forward_device_batch on frames that are on the device already, groups of
            frames_per_step, no copies, one synchronise at the end (NV12: the two converters per frame included)
  stream    (c) utils.run_model_inference_stream at the same frames_per_step: the sum of its `ms`, which is the wall
            time of the stream, its unpipelined first group included

for frames_per_step 1, 2 and 4, and from them resident / stream (the target of the Restormer workload is >= 0.98 at
4) and loop / stream.  `front_end_share` is the share of a resident step that is not the model: (resident step -
the forward alone on tiles of the same shape) / resident step, both graphed where the model is - the tiler and the
converters are launched outside ops.KernelTimer's wrappers, so the timer cannot see them.

Workloads: restormer (motion deblurring, uint8, 512 / 96), dncnn (colour, nb 20, uint8, 256 / 48), dncnn_nv12,
fpn_mobilenet (uint8, 2048 / 384).  One JSON line per workload; --out FILE appends them."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import deblurganv2, dncnn, harness, restormer, utils

STEPS = (1, 2, 4)
YUV = dict(matrix="bt709", full_range=False, siting="left")


def _models(dev):
    return {
        "restormer": (lambda: restormer.Restormer(LayerNorm_type="WithBias").load_synthetic(42).eval().to(dev),
                      utils.get_patch_config("deblurring", "motion", "Restormer"), None),
        "dncnn": (lambda: dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev),
                  utils.get_patch_config("denoising", "gaussian", "DnCNN"), None),
        "dncnn_nv12": (lambda: dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev),
                       utils.get_patch_config("denoising", "gaussian", "DnCNN"), "nv12"),
        "fpn_mobilenet": (lambda: deblurganv2.FPNMobileNet().load_synthetic(42).to(dev),
                          utils.get_patch_config("deblurring", "motion", "DeblurGANv2 (MobileNet)"), None),
    }


def _wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _resident_step(model, group, cfg, fmt, hooks, pad8):
    """One group of device frames through the batch call (NV12: converter, batch call, converter)."""
    mb = getattr(model, "max_tiles_per_batch", 8)
    if fmt is None:
        return utils.tiled_forward_device_batch(model, group, cfg["patch_size"], cfg["patch_overlap"], pad8, max_batch=mb,
                                                hooks=hooks)
    rgb = [utils.yuv420_to_rgb_device(p, fmt, **YUV) for p in group]
    res = utils.tiled_forward_device_batch(model, rgb, cfg["patch_size"], cfg["patch_overlap"], pad8, max_batch=mb,
                                           unit_range=True, out="float32")
    return [utils.rgb_to_yuv420_device(f, fmt, **YUV) for f, _ in res]


def bench(name, dev, frames_u8, n, rounds):
    make, cfg, fmt = _models(dev)[name]
    model = make()
    hooks, pad8 = utils._model_hooks(model)
    h, w = frames_u8[0].shape[:2]
    if fmt is None:
        host = list(frames_u8)
        on_dev = [utils.to_device(f, dev) for f in host]
    else:
        host = [utils.rgb_to_yuv420_host(f.astype(np.float32) / np.float32(255.0), fmt, **YUV) for f in frames_u8]
        on_dev = [tuple(utils.to_device(p, dev) for p in planes) for planes in host]
    kw = dict(cfg, fmt=fmt, **YUV) if fmt else dict(cfg)

    def loop():
        one = ((lambda f: utils.run_model_inference_yuv(model, f, dev, fmt=fmt, **YUV, **cfg)) if fmt
               else (lambda f: utils.get_model_prediction(model, f, dev, **cfg)))
        one(host[0])
        return _wall_ms(lambda: [one(f) for f in host[:n]]) / n

    def resident(k):
        def run():
            _resident_step(model, on_dev[:k], cfg, fmt, hooks, pad8)
            return _wall_ms(lambda: [_resident_step(model, on_dev[i:i + k], cfg, fmt, hooks, pad8) for i in range(0, n, k)]) / n
        return run

    def stream(k):
        def run():
            list(utils.run_model_inference_stream(model, iter(host[:k]), dev, frames_per_step=k, **kw))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms = [m for _, m in utils.run_model_inference_stream(model, iter(host[:n]), dev, frames_per_step=k, **kw)]
            wall = (time.perf_counter() - t0) * 1e3
            walls.append((sum(ms) / n, wall / n))
            return sum(ms) / n
        return run

    walls = []                                      # (sum of ms, host wall time) per frame of every stream leg: they agree
    legs = {"loop": loop}
    for k in STEPS:
        legs[f"resident_{k}"], legs[f"stream_{k}"] = resident(k), stream(k)
    names = list(legs)
    with torch.no_grad():
        ts = {k: [] for k in legs}
        for r in range(rounds):
            for i in range(len(names)):
                leg = names[(i + r) % len(names)]
                ts[leg].append(legs[leg]())
        ms = {k: float(np.median(v)) for k, v in ts.items()}
        share = _front_end_share(model, dev, on_dev, cfg, fmt, hooks, pad8, h, w, max(STEPS), n)
    res = {"group": "stream", "workload": name, "frame": f"{h}x{w}", "fmt": fmt or "uint8", **cfg, "frames": n,
           "rounds": rounds, "ms_per_frame": ms, "ms_per_frame_all_rounds": ts,
           "resident_over_stream": {k: ms[f"resident_{k}"] / ms[f"stream_{k}"] for k in STEPS},
           "loop_over_stream": {k: ms["loop"] / ms[f"stream_{k}"] for k in STEPS},
           "front_end_share": share,
           "stream_ms_sum_vs_wall_max_rel": max(abs(a - b) / b for a, b in walls)}
    del model, on_dev
    torch.cuda.empty_cache()
    return res


def _front_end_share(model, dev, on_dev, cfg, fmt, hooks, pad8, h, w, k, n):
    """(resident step - forward alone) / resident step at frames_per_step k: the tiler and the converters' share."""
    pad_mode = "zero32" if hooks == "deblurganv2" else "reflect8" if pad8 else "none"
    _, origins, _, _, ph, pw = utils.tile_plan(h, w, cfg["patch_size"], cfg["patch_overlap"], pad_mode)
    tiles = torch.rand(k * len(origins), 3, ph, pw, device=dev)
    mb = getattr(model, "max_tiles_per_batch", 8)
    reps = max(n // k, 1)
    utils._forward_tiles(model, tiles, mb)
    _resident_step(model, on_dev[:k], cfg, fmt, hooks, pad8)
    step, fwd = [], []
    for _ in range(3):
        fwd.append(_wall_ms(lambda: [utils._forward_tiles(model, tiles, mb) for _ in range(reps)]) / reps)
        step.append(_wall_ms(lambda: [_resident_step(model, on_dev[:k], cfg, fmt, hooks, pad8) for _ in range(reps)]) / reps)
    step_ms, fwd_ms = float(np.median(step)), float(np.median(fwd))
    return {"frames_per_step": k, "step_ms": step_ms, "forward_ms": fwd_ms, "share": (step_ms - fwd_ms) / step_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="restormer,dncnn,dncnn_nv12,fpn_mobilenet")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream: needs a GPU")
    if a.frames % max(STEPS):
        raise SystemExit(f"--frames must be a multiple of {max(STEPS)}")
    dev = torch.device("cuda:0")
    frames = [inp for inp, _, _ in harness.synthetic_loader(a.frames, h=a.height, w=a.width)]
    for name in a.workloads.split(","):
        line = json.dumps(bench(name, dev, frames, a.frames, a.rounds))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
