#!/usr/bin/env python3
"""MaIR+ on the GPU: what the x8 self-ensemble with partitioned forward costs, and what its two kernels cost.

Cases: a 320 x 180 frame through the lightweight x4 MaIR, and a 256 x 256 frame through the colour-denoising MaIR
(synthetic weights).  Per case, with HIP events around warmed-up loops:

  * the whole MaIRPlus call (eager, and replayed by utils.graphed_forward) against 8 x the plain forward;
  * irm_dihedral_chop_f32 and irm_ensemble_merge_f32 alone, their share of the eager call, and their compulsory
    bytes over their time as a fraction of the 8 TB/s HBM peak (chop: 1 read of the image + 1 write of every
    partition; merge: 8 reads + 1 write of the output);
  * the same chop and merge composed from torch ops (ensemble.chop_torch / merge_torch: flips, transposes, reflect
    pad, slice copies, slice writes, stack + mean) on the same buffers - the baseline, since no older path exists.

Usage: python tools/bench_mair_plus.py [--iters 20] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import irm_amd  # noqa: E402,F401
from irm_amd import ensemble, mair, synth, utils  # noqa: E402

HBM_PEAK = 8.0e12
LIGHT_X4 = dict(upscale=4, in_chans=3, img_range=1., embed_dim=60, d_state=1, depths=[6, 6, 6, 6], ssm_ratio=1.1,
                mlp_ratio=1.6, upsampler='pixelshuffledirect', scan_len=4, resi_connection='1conv')


def cdn_config():
    with open(os.path.join(ROOT, "image-restoration-models_amd", "mair", "options", "test_MaIR_CDN_s25.yml")) as f:
        cfg = dict(yaml.safe_load(f)["network_g"])
    cfg.pop("type")
    return cfg


def timed(fn, iters, warmup=3):
    """Mean milliseconds of fn() over `iters` calls between two events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def run_case(name, net, H, W, iters):
    dev = torch.device("cuda:0")
    net = net.load_synthetic(42).eval().to(dev)
    model = mair.MaIRPlus(net)
    s = model.upscale
    x = synth.uniform(7, f"bench_plus_{name}", (1, 3, H, W), 0.0, 1.0).to(dev)
    geo, table = ensemble._geometry_on(dev, 1, H, W, True)
    res = {"input": [H, W], "scale": s, "partitions": geo.P, "groups": [list(g[:3]) for g in geo.groups]}
    y = model(x)
    res["plus_eager_ms"] = timed(lambda: model(x), iters)
    res["plain_forward_ms"] = timed(lambda: net(x), iters)
    res["plus_over_8_plain"] = res["plus_eager_ms"] / (8 * res["plain_forward_ms"])
    if model.hip_graph:
        assert torch.equal(utils.graphed_forward(model, x), y)
        res["plus_graph_ms"] = timed(lambda: utils.graphed_forward(model, x), iters)
        res["plain_graph_ms"] = timed(lambda: utils.graphed_forward(net, x), iters)
    # ---- the two kernels alone, on the buffers of this case
    C = 3
    packed = torch.empty(geo.total_pixels * C, device=dev)
    pred = synth.uniform(7, "bench_plus_pred", (geo.total_pixels * C * s * s,), 0.0, 1.0).to(dev)
    out = torch.empty(1, C, s * H, s * W, device=dev)
    k_iters = max(iters, 50)
    chop_ms = timed(lambda: ensemble.dihedral_chop(x, table, packed, geo), k_iters)
    merge_ms = timed(lambda: ensemble.ensemble_merge(pred, table, out, geo, s), k_iters)
    chop_bytes = 4.0 * C * (H * W + geo.total_pixels)
    merge_bytes = 36.0 * out.numel()
    # ---- the torch-op composition of the same movement
    blocks = [[] for _ in range(8)]
    for row in geo.table[8:]:
        e, _, _, ph, pw, off = (int(v) for v in row[:6])
        blocks[e].append(pred[off * C * s * s:(off + ph * pw) * C * s * s].view(1, C, s * ph, s * pw))

    def chop_torch():
        return [t.contiguous() for v in range(8) for t in ensemble.chop_torch(x, v)]
    torch_chop_ms = timed(chop_torch, k_iters)
    torch_merge_ms = timed(lambda: ensemble.merge_torch(blocks, H, W, s), k_iters)
    assert torch.equal(torch.cat([t.reshape(-1) for t in chop_torch()]).sort().values, packed.sort().values)
    ensemble.ensemble_merge(pred, table, out, geo, s)
    assert float((ensemble.merge_torch(blocks, H, W, s) - out).abs().max()) <= 2.0 ** -21
    res.update(chop_us=1e3 * chop_ms, merge_us=1e3 * merge_ms, torch_chop_us=1e3 * torch_chop_ms,
               torch_merge_us=1e3 * torch_merge_ms, torch_over_kernels=(torch_chop_ms + torch_merge_ms) / (chop_ms + merge_ms),
               kernels_share_of_call=(chop_ms + merge_ms) / res["plus_eager_ms"],
               chop_bytes=chop_bytes, merge_bytes=merge_bytes,
               chop_fraction_of_hbm_peak=chop_bytes / (chop_ms * 1e-3) / HBM_PEAK,
               merge_fraction_of_hbm_peak=merge_bytes / (merge_ms * 1e-3) / HBM_PEAK,
               torch_chop_fraction_of_hbm_peak=chop_bytes / (torch_chop_ms * 1e-3) / HBM_PEAK,
               torch_merge_fraction_of_hbm_peak=merge_bytes / (torch_merge_ms * 1e-3) / HBM_PEAK)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mair_plus.py measures on the GPU; none is present")
    results = {"light_x4_320x180": run_case("light_x4", mair.MaIR(**LIGHT_X4), 180, 320, args.iters),
               "cdn_256x256": run_case("cdn", mair.MaIR(**cdn_config()), 256, 256, args.iters)}
    line = json.dumps(results, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
