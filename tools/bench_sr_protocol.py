"""Cost of the super-resolution protocol's own steps on a synthetic 1280x720 RGB uint8 frame (synth.synth_image_pair):

  shrink        irm_imresize_bicubic 1280x720 -> 320x180 (quantised output, how LR frames are made)
  enlarge       irm_imresize_bicubic 320x180 -> 1280x720 (quantised output, the bicubic baseline)
  score         irm_frame_metrics_basicsr of a 720p pair, crop 4, Y channel

Device time: HIP events around a graph replay of R calls (kernels only: the tap tables are cached on the device by the
warm-up call), per call.  With it, the share of the 8 TB/s HBM peak that the compulsory bytes (input read once, output
written once) account for.  The host restatements (utils.imresize_host, utils.calculate_metrics_basicsr) are timed in
the same run, wall clock.  Prints one JSON line at the end; --out FILE writes it too."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import synth, utils

HBM_PEAK = 8.0e12


def _graph_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(ts))


def _host_ms(fn, n=3):
    fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="device calls per graph replay")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sr_protocol: needs a GPU")
    dev = torch.device("cuda:0")
    _, hr = synth.synth_image_pair(0, 720, 1280, 3)
    hr_dev = torch.from_numpy(hr).to(dev)
    lr_dev = utils.imresize_device(hr_dev, 0.25)
    lr = lr_dev.cpu().numpy()
    back_dev = utils.imresize_device(lr_dev, 4)
    back = back_dev.cpu().numpy()
    res = {"frame": "1280x720x3 uint8 (synth_image_pair target), LR 320x180x3"}
    steps = {
        "shrink_720p_to_180p": (lambda: utils.imresize_device(hr_dev, 0.25), hr.nbytes + lr.nbytes),
        "enlarge_180p_to_720p": (lambda: utils.imresize_device(lr_dev, 4), lr.nbytes + hr.nbytes),
        "score_720p_crop4_y": (lambda: utils.frame_metrics_basicsr_device([back_dev], [hr_dev], 4, True), 2 * hr.nbytes),
    }
    for name, (fn, nbytes) in steps.items():
        us = _graph_us(fn, a.reps)
        res[f"{name}_device_us"] = us
        res[f"{name}_compulsory_bytes"] = int(nbytes)
        res[f"{name}_share_of_hbm_peak"] = nbytes / (us * 1e-6) / HBM_PEAK
    res["shrink_host_ms"] = _host_ms(lambda: utils.imresize_host(hr, 0.25, out="same"))
    res["enlarge_host_ms"] = _host_ms(lambda: utils.imresize_host(lr, 4, out="same"))
    res["score_host_ms"] = _host_ms(lambda: utils.calculate_metrics_basicsr(back, hr, 4, True))
    vt = []
    for _ in range(20):
        t0 = time.perf_counter()
        p, s = utils.calculate_metrics_basicsr_device(back_dev, hr_dev, 4, True)
        vt.append((time.perf_counter() - t0) * 1e3)
    res["score_device_visible_ms"] = float(np.median(vt))
    hp, hs = utils.calculate_metrics_basicsr(back, hr, 4, True)
    res["bicubic_x4_psnr_y_db"], res["bicubic_x4_ssim_y"] = p, s
    res["score_device_minus_host"] = [p - hp, s - hs]
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
