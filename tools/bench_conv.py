#!/usr/bin/env python3
"""Isolated timing of irm_conv3x3_ep_f32 (HIP events), with --split also of the emulated irm_conv3x3_f16x3_ep_f32 on the
same shapes.  Usage: python tools/bench_conv.py [reps] [index] [--split]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irm_amd  # noqa
from irm_amd import _hip, ops

SHAPES = [  # ci, co, H, W, B, store_mode
    (96, 192, 256, 256, 6, 2), (192, 384, 128, 128, 6, 2), (64, 64, 256, 256, 16, 0), (128, 128, 128, 128, 16, 0),
    (48, 24, 512, 512, 6, 1), (96, 3, 512, 512, 6, 0), (3, 48, 512, 512, 6, 0),
    (64, 64, 321, 481, 4, 0),     # odd W: the guarded conv3x3_kernel with scalar stores (exact only)
]


def main():
    argv = [a for a in sys.argv[1:] if a != "--split"]
    kinds = ("exact", "split") if "--split" in sys.argv else ("exact",)
    reps = int(argv[0]) if argv else 50
    only = int(argv[1]) if len(argv) > 1 else None
    dev = torch.device("cuda:0")
    for idx, (ci, co, H, W, B, st) in enumerate(SHAPES):
        if only is not None and idx != only:
            continue
        x = torch.randn(B, ci, H, W, device=dev)
        oc, oh, ow = (co, H, W) if st == 0 else (co * 4, H // 2, W // 2) if st == 1 else (co // 4, 2 * H, 2 * W)
        y = torch.empty(B, oc, oh, ow, device=dev)
        wt = torch.randn(co, ci, 3, 3) * 0.05
        bias = torch.zeros(co, device=dev) if st == 0 and ci == co else None
        for kind in kinds:
            if kind == "split" and W % 4:
                continue
            if kind == "exact":
                w = _hip.pack_conv3x3_weight(wt).to(dev)
            else:
                wps, inv_scale = _hip.pack_conv3x3_weight_split(wt)
                w = (wps.to(dev), inv_scale)
            for _ in range(2):
                ops.conv3x3(w, x, y, ci, co, bias=bias, relu1=bias is not None, store_mode=st)
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.conv3x3(w, x, y, ci, co, bias=bias, relu1=bias is not None, store_mode=st)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            t = sorted(ts)[len(ts) // 2] * 1e-3
            fl = 18.0 * B * ci * co * H * W
            by = 4.0 * B * H * W * (ci + co)
            print(f"{kind:5s} ci{ci:4d} co{co:4d} {H}x{W} B{B} st{st}: {t*1e6:8.1f} us  {fl/t/1e12:6.1f} TF  {by/t/1e9:6.0f} GB/s",
                  flush=True)


if __name__ == "__main__":
    main()
