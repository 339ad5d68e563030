"""Float32 frames and model chains on the device pipeline, timed end to end: one process, one GPU.

Frame legs, one 1280 x 720 x 3 frame through Restormer (motion deblurring, patch 512 / overlap 96, synthetic weights):

  float32_call   utils.get_model_prediction on the float32 frame (upload, irm_frame_minmax_f32, irm_tile_extract_f32,
                 batched forwards, irm_window_blend_f32, download)
  host_loop      utils._run_tiles_on_host on the same frame: what a float32 frame took before it had a device path (one
                 tile per forward, a download per tile, the blend in numpy)
  uint8_call     utils.get_model_prediction on the uint8 frame

and the parts the first and the last differ in: `*_device` is utils.tiled_forward_device on a frame that is already on
the GPU (device events: no copies in it), `*_upload` / `*_download` are the two copies on their own (pageable host
memory, as the calls make them).

Chain legs, DnCNN (colour, blind, patch 256 / 48) followed by the same Restormer on one uint8 frame:

  chain          utils.run_model_chain: one upload, a float32 frame between the stages on the device, one download
  two_calls      two utils.get_model_prediction calls: the uint8 frame of the first goes through the host

Every leg is warmed up, then timed --reps times in turn with the others (the legs alternate, so drift hits all alike);
a host clock around a call that ends in a download, the median, the minimum and the maximum in milliseconds.  Prints
one JSON line per group; --out FILE writes the lines too."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import dncnn, restormer, synth, utils


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternate(legs, reps, warmup):
    """legs: {name: (timer, fn)} -> {name: [median, min, max]} with the legs taking turns."""
    for _ in range(warmup):
        for timer, fn in legs.values():
            timer(fn)
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, (timer, fn) in legs.items():
            ts[k].append(timer(fn))
    return {k: [float(np.median(v)), float(np.min(v)), float(np.max(v))] for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3, help="repetitions of the per-tile host loop")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_float_frames: needs a GPU")
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    deblur = restormer.Restormer(LayerNorm_type="WithBias").load_synthetic(42).eval().to(dev)
    denoise = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    cfg_r = utils.get_patch_config("deblurring", "motion", "Restormer")
    cfg_d = utils.get_patch_config("denoising", "gaussian", "DnCNN")
    u8 = synth.synth_image_pair(0, h, w, 3, seed_base=9100, blur=5)[0]
    f32 = u8.astype(np.float32) / np.float32(255.0)
    u8_dev, f32_dev = torch.from_numpy(u8).to(dev), torch.from_numpy(f32).to(dev)
    mb = getattr(deblur, "max_tiles_per_batch", 8)
    lines = []

    # ---- frames
    legs = {
        "float32_call": (_host_ms, lambda: utils.get_model_prediction(deblur, f32, dev, **cfg_r)),
        "uint8_call": (_host_ms, lambda: utils.get_model_prediction(deblur, u8, dev, **cfg_r)),
        "float32_device": (_event_ms, lambda: utils.tiled_forward_device(deblur, f32_dev, cfg_r["patch_size"],
                                                                         cfg_r["patch_overlap"], True, max_batch=mb)),
        "uint8_device": (_event_ms, lambda: utils.tiled_forward_device(deblur, u8_dev, cfg_r["patch_size"],
                                                                       cfg_r["patch_overlap"], True, max_batch=mb)),
        "float32_upload": (_host_ms, lambda: torch.from_numpy(f32).to(dev)),
        "uint8_upload": (_host_ms, lambda: torch.from_numpy(u8).to(dev)),
        "float32_download": (_host_ms, lambda: f32_dev.cpu()),
        "uint8_download": (_host_ms, lambda: u8_dev.cpu()),
    }
    res = {"group": "frames", "frame": f"{h}x{w}x3", "model": "Restormer deblurring", **cfg_r, "reps": a.reps,
           "ms_median_min_max": _alternate(legs, a.reps, a.warmup)}
    host = {"host_loop": (_host_ms, lambda: utils._run_tiles_on_host(deblur, f32, dev, utils.normalize,
                                                                      cfg_r["patch_size"], cfg_r["patch_overlap"], False,
                                                                      None, utils.pad, None))}
    res["ms_median_min_max"].update(_alternate(host, a.host_reps, 1))
    m = {k: v[0] for k, v in res["ms_median_min_max"].items()}
    res["float32_over_uint8_call"] = m["float32_call"] / m["uint8_call"]
    res["host_loop_over_float32_call"] = m["host_loop"] / m["float32_call"]
    res["call_difference_ms"] = m["float32_call"] - m["uint8_call"]
    res["copy_difference_ms"] = (m["float32_upload"] + m["float32_download"]) - (m["uint8_upload"] + m["uint8_download"])
    res["device_difference_ms"] = m["float32_device"] - m["uint8_device"]
    # the device result against the host loop on the same frame (different tile batches: not bit for bit)
    pred = utils.get_model_prediction(deblur, f32, dev, **cfg_r)[0]
    ref = utils._run_tiles_on_host(deblur, f32, dev, utils.normalize, cfg_r["patch_size"], cfg_r["patch_overlap"], False,
                                   None, utils.pad, None)
    res["max_abs_vs_host_loop"] = float(np.abs(pred - ref).max())
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)

    # ---- chain
    def two_calls():
        mid = utils.get_model_prediction(denoise, u8, dev, **cfg_d)[0]
        return utils.get_model_prediction(deblur, mid, dev, **cfg_r)[0]

    def chain():
        return utils.run_model_chain([(denoise, cfg_d), (deblur, cfg_r)], u8, dev)[0]
    legs = {"chain": (_host_ms, chain), "two_calls": (_host_ms, two_calls)}
    res = {"group": "chain", "frame": f"{h}x{w}x3", "stages": ["DnCNN colour blind 256/48", "Restormer deblurring 512/96"],
           "reps": a.reps, "ms_median_min_max": _alternate(legs, a.reps, a.warmup)}
    m = {k: v[0] for k, v in res["ms_median_min_max"].items()}
    res["chain_over_two_calls"] = m["chain"] / m["two_calls"]
    diff = np.abs(chain().astype(int) - two_calls().astype(int))
    res["bytes_differ_share"], res["bytes_max_diff"] = float((diff > 0).mean()), int(diff.max())
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
