"""Cost of scoring a frame: host calculate_metrics (numpy / scipy float64) vs the device path (irm_frame_metrics) on
synthetic 1280x720 RGB frames (harness.synthetic_loader), and what it does to a harness sweep.

  host ms/frame        utils.calculate_metrics on the host arrays (wall clock)
  device kernel us     events around a graph replay of R calls (the two launches of a call, no host enqueue cost);
                       K=1 and K=4 frames per call
  device visible ms    utils.calculate_metrics_device on frames already on the GPU, wall clock incl. its one sync
  harness frames/s     harness.evaluate over N frames, DnCNN colour (synthetic weights), metrics="host" / "device",
                       wall clock, alternated twice

--kernels-only runs just the device calls (for a `rocprofv3 --kernel-trace --stats` run of its own).
Prints one JSON line at the end; --out FILE writes it too."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import dncnn, harness, utils


def _med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6, help="harness frames per mode")
    ap.add_argument("--reps", type=int, default=50, help="device calls per graph replay")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: needs a GPU")
    dev = torch.device("cuda:0")
    frames = list(harness.synthetic_loader(max(a.frames, 4), h=720, w=1280, c=3))
    preds = [torch.from_numpy(f[0]).to(dev) for f in frames[:4]]
    tgts = [torch.from_numpy(f[1]).to(dev) for f in frames[:4]]
    res = {"frame": "1280x720x3 uint8, synthetic_loader (degraded input vs target)"}

    if a.kernels_only:
        for _ in range(20):
            utils.frame_metrics_device(preds[:1], tgts[:1])
            utils.frame_metrics_device(preds, tgts)
        torch.cuda.synchronize()
        print("kernels-only: 20 x (K=1 call, K=4 call) done")
        return

    # host
    utils.calculate_metrics(frames[0][0], frames[0][1])
    ht = []
    for i in range(3):
        t0 = time.perf_counter()
        utils.calculate_metrics(frames[i][0], frames[i][1])
        ht.append((time.perf_counter() - t0) * 1e3)
    res["host_calculate_metrics_ms_per_frame"] = _med(ht)

    # device kernel time: R calls captured in one graph, events around its replay
    for k in (1, 4):
        for _ in range(3):
            utils.frame_metrics_device(preds[:k], tgts[:k])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.reps):
                utils.frame_metrics_device(preds[:k], tgts[:k])
        g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / (a.reps * k))
        res[f"device_us_per_frame_K{k}_graph_events"] = _med(ts)
        del g
    # check the graph-replayed values against an eager call
    s_e, m_e = utils.frame_metrics_device(preds, tgts)
    ph, sh = utils.calculate_metrics(frames[0][0], frames[0][1])
    res["ssim_frame0_device_minus_host"] = float(m_e[0]) - sh

    # host-visible device metrics (one sync per frame)
    for _ in range(3):
        utils.calculate_metrics_device(preds[0], tgts[0])
    vt = []
    for i in range(30):
        t0 = time.perf_counter()
        utils.calculate_metrics_device(preds[i % 4], tgts[i % 4])
        vt.append((time.perf_counter() - t0) * 1e3)
    res["device_visible_ms_per_frame"] = _med(vt)

    # harness sweep, DnCNN colour blind (synthetic weights), alternated
    model = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    cfg = utils.get_patch_config("denoising", "gaussian", "DnCNN")
    kw = dict(task="denoising", subtask="gaussian", dataset="synthetic", model_name="DnCNN")
    sweep = frames[:a.frames]
    for m in ("host", "device"):
        harness.evaluate(model, iter(sweep[:1]), dev, cfg, metrics=m, **kw)
    fps = {"host": [], "device": []}
    rows = {}
    for _ in range(2):
        for m in ("host", "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows[m] = harness.evaluate(model, iter(sweep), dev, cfg, metrics=m, **kw)
            fps[m].append(len(sweep) / (time.perf_counter() - t0))
    for m in ("host", "device"):
        res[f"harness_frames_per_s_{m}"] = fps[m]
        res[f"harness_avg_time_ms_{m}"] = float(rows[m]["Avg_Time_ms"])
    res["harness_dSSIM_device_minus_host"] = float(rows["device"]["SSIM"] - rows["host"]["SSIM"])
    res["harness_dPSNR_device_minus_host"] = float(rows["device"]["PSNR"] - rows["host"]["PSNR"])

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
