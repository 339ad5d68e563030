"""Cost of the resize to any size (irm_resize_taps) on synthetic RGB frames (synth.synth_image_pair), three groups:

  same work     irm_resize_taps against irm_imresize_bicubic at 1280x720 x 1/4 and 320x180 x 4, uint8 in and out (the two
                legs tools/bench_sr_protocol.py times).  Both kernels move the same bytes; the general one may take
                1.25 x the old entry's time ("within_margin").
  target sizes  1280x720 -> 1920x1080 (bicubic, lanczos3) and 3840x2160 -> 1920x1080 (lanczos3), uint8 and float32
                frames, for reporting.
  chain         colour DnCNN followed by Resize(size=(1080, 1920)) as one run_model_chain call, against the same model
                call followed by a download, resize_host and an upload - the round trip the stage removes.

Device time: HIP events around a graph replay of R calls (kernels only: the tap tables are cached on the device by the
warm-up calls), per call.  The two legs of a comparison alternate in one process, --rounds times; median, minimum and
maximum of the rounds are reported, and the compulsory bytes (input read once, output written once) as a share of the
8 TB/s HBM peak.  The chain legs are wall clock around calls that end in the download.  Prints one JSON line at the end;
--out FILE appends it (profiles/bench_resize.jsonl)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import dncnn, synth, utils
from irm_amd.frames import to_device

HBM_PEAK = 8.0e12


def _graph(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _replay_us(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternate_us(legs, reps, rounds):
    """legs: name -> callable.  Each leg captured once, then `rounds` rounds that time every leg in turn."""
    graphs = {name: _graph(fn, reps) for name, fn in legs.items()}
    ts = {name: [] for name in legs}
    for _ in range(rounds):
        for name, g in graphs.items():
            ts[name].append(_replay_us(g, reps))
    return {name: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))} for name, v in ts.items()}


def _wall_ms(fn, n):
    fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="device calls per graph replay")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds per comparison")
    ap.add_argument("--chain-runs", type=int, default=25, help="alternating rounds of the model and the chain call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/bench_resize.py", "reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}

    # ---- the same work through both entries
    _, hr = synth.synth_image_pair(0, 720, 1280, 3)
    hr_dev = torch.from_numpy(hr).to(dev)
    lr_dev = utils.imresize_device(hr_dev, 0.25)
    assert torch.equal(utils.resize_device(hr_dev, scale=0.25), lr_dev)
    assert torch.equal(utils.resize_device(lr_dev, scale=4), utils.imresize_device(lr_dev, 4))
    nbytes = hr.nbytes + lr_dev.numel()
    for name, old, new in (("shrink_720p_to_180p", lambda: utils.imresize_device(hr_dev, 0.25), lambda: utils.resize_device(hr_dev, scale=0.25)),
                           ("enlarge_180p_to_720p", lambda: utils.imresize_device(lr_dev, 4), lambda: utils.resize_device(lr_dev, scale=4))):
        t = alternate_us({"irm_imresize_bicubic": old, "irm_resize_taps": new}, a.reps, a.rounds)
        ratio = t["irm_resize_taps"]["median_us"] / t["irm_imresize_bicubic"]["median_us"]
        res[name] = dict(t, compulsory_bytes=int(nbytes), ratio_new_over_old=ratio, within_margin=bool(ratio <= 1.25),
                         share_of_hbm_peak_new=nbytes / (t["irm_resize_taps"]["median_us"] * 1e-6) / HBM_PEAK)

    # ---- target sizes
    _, uhd = synth.synth_image_pair(1, 2160, 3840, 3)
    sources = {"720p": hr, "2160p": uhd}
    for src, kernel in (("720p", "bicubic"), ("720p", "lanczos3"), ("2160p", "lanczos3")):
        legs, sizes = {}, {}
        for kind in ("uint8", "float32"):
            frame = sources[src] if kind == "uint8" else sources[src].astype(np.float32) / np.float32(255.0)
            fd = torch.from_numpy(frame).to(dev)
            legs[kind] = (lambda fd=fd: utils.resize_device(fd, size=(1080, 1920), kernel=kernel))
            sizes[kind] = frame.nbytes + 1080 * 1920 * 3 * frame.itemsize
        t = alternate_us(legs, a.reps, a.rounds)
        for kind in legs:
            t[kind]["compulsory_bytes"] = int(sizes[kind])
            t[kind]["share_of_hbm_peak"] = sizes[kind] / (t[kind]["median_us"] * 1e-6) / HBM_PEAK
        res[f"{src}_to_1080p_{kernel}"] = t
        del legs

    # ---- the chain against the round trip through the host
    den = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    cfg = utils.get_patch_config("denoising", "gaussian", "DnCNN")
    stage = utils.Resize(size=(1080, 1920))

    def host_leg():
        mid, _ = utils.run_model_chain([(den, cfg)], hr, dev)
        out = utils.resize_host(mid, size=(1080, 1920), out="same")
        return to_device(out, dev)
    legs = {"model": lambda: utils.run_model_chain([(den, cfg)], hr, dev),
            "chain": lambda: utils.run_model_chain([(den, cfg), stage], hr, dev)}
    for fn in legs.values():
        for _ in range(3):
            fn()
    walls = {name: [] for name in legs}
    for _ in range(a.chain_runs):                                          # the two legs in turn
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            walls[name].append((time.perf_counter() - t0) * 1e3)
    model, chain = ({"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
                     "p25_ms": float(np.percentile(v, 25)), "p75_ms": float(np.percentile(v, 75))}
                    for v in (walls["model"], walls["chain"]))
    host = _wall_ms(host_leg, 3)
    mid_dev = utils.tiled_forward_device(den, hr_dev, cfg["patch_size"], cfg["patch_overlap"], False, None, unit_range=True,
                                         out="float32")[0]
    kern = alternate_us({"resize_f32_to_uint8": lambda: utils.resize_device(mid_dev, size=(1080, 1920), out="uint8")}, a.reps, a.rounds)
    spread = model["max_ms"] - model["min_ms"]                         # (the quartiles are in the legs' own records)
    # the chain downloads a 1080p frame where the model call downloads a 720p one: timed on its own and named
    big = utils.resize_device(hr_dev, size=(1080, 1920))
    extra = _wall_ms(lambda: big.cpu(), 9)["median_ms"] - _wall_ms(lambda: hr_dev.cpu(), 9)["median_ms"]
    res["chain_dncnn_720p_then_1080p"] = {
        "model_call": model, "chain_call": chain, "model_then_host_resize_then_upload": host,
        "resize_kernels_us": kern["resize_f32_to_uint8"], "model_run_to_run_spread_ms": spread,
        "larger_download_ms": extra, "chain_minus_model_ms": chain["median_ms"] - model["median_ms"],
        "allowance_ms": kern["resize_f32_to_uint8"]["median_us"] * 1e-3 + spread,
        "allowance_interquartile_ms": kern["resize_f32_to_uint8"]["median_us"] * 1e-3 + model["p75_ms"] - model["p25_ms"],
        "host_leg_minus_chain_ms": host["median_ms"] - chain["median_ms"]}
    for k, v in res.items():
        print(f"{k}: {v}")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
