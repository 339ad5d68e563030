"""Cost of NIQE on a synthetic 1280x720 RGB uint8 frame (synth.synth_image_pair): 7 x 13 = 91 blocks of 96 x 96.

  host          utils.calculate_niqe, the float64 numpy / scipy restatement, wall clock
  device call   utils.calculate_niqe_device on a frame that is already on the GPU, wall clock: the launch, the one
                download of 91 x 36 doubles and the host tail (mean, covariance, 36 x 36 pinv)
  kernel        irm_niqe_features alone: HIP events around a graph replay of R calls, per call
  host tail     utils.niqe_score on the downloaded features, wall clock

--kernels-only runs R plain launches and nothing else, for a separate `rocprofv3 --kernel-trace --stats` run.
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
from irm_amd import synth, utils


def _wall_ms(fn, n):
    fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                     "tests", "golden", "niqe_pris_params.npz"))
    ap.add_argument("--reps", type=int, default=20, help="device calls per graph replay / plain launches")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_niqe: needs a GPU")
    dev = torch.device("cuda:0")
    params = utils.load_niqe_params(a.params)
    _, frame = synth.synth_image_pair(0, 720, 1280, 3)
    frame_dev = torch.from_numpy(frame).to(dev)
    if a.kernels_only:
        for _ in range(a.reps):
            utils.niqe_features_device(frame_dev, 0, params)
        torch.cuda.synchronize()
        print(f"bench_niqe: {a.reps} launches of irm_niqe_features on 1280x720x3 uint8")
        return
    res = {"frame": "1280x720x3 uint8 (synth_image_pair target), 91 blocks"}
    res["device_call_ms"] = _wall_ms(lambda: utils.calculate_niqe_device(frame_dev, 0, params), 20)
    res["kernel_us"] = _graph_us(lambda: utils.niqe_features_device(frame_dev, 0, params), a.reps)
    feats = utils.niqe_features_device(frame_dev, 0, params).cpu().numpy()[0]
    res["host_tail_ms"] = _wall_ms(lambda: utils.niqe_score(feats, params), 20)
    res["host_ms"] = _wall_ms(lambda: utils.calculate_niqe(frame, 0, params, channel_order="rgb"), 3)
    d, h = utils.calculate_niqe_device(frame_dev, 0, params), utils.calculate_niqe(frame, 0, params, channel_order="rgb")
    res["niqe_device"], res["niqe_host"], res["device_minus_host_rel"] = d, h, abs(d - h) / abs(h)
    res["host_over_device_call"] = res["host_ms"] / res["device_call_ms"]
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
