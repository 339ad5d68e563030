#!/usr/bin/env python3
"""Golden fixtures of MaIR super resolution: tests/golden/mair_sr.npz and tests/golden/mair_sr.json.

Runs where the reference tree is available (CPU).  It imports the reference's own mair_arch.MaIR through
oracle.gen_golden.import_reference_mairunet() (mamba_ssm's selective scan replaced by oracle/mair_ref.selective_scan),
loads synthetic weights (synth.synth_state_dict with the MaIR SYNTH_RULES, seed 42) and stores the reference's
train-mode CPU forward (the eval-mode forward binds its scan tables under CUDA only, as in gen_golden.gen_mair) for
every configuration below on a 16x16 and a 12x20 input.  It also records, per configuration, the state_dict shapes
and the distance of a float64 composition of oracle/mair_ref.py pieces plus the SR head (`oracle_sr_forward`) from
the reference output.

Usage: python tools/gen_golden_mair_sr.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden, mair_ref  # noqa: E402
from irm_amd import synth  # noqa: E402
from irm_amd.mair import SYNTH_RULES  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
INPUTS = [(16, 16), (12, 20)]
_BASE = dict(in_chans=3, img_range=1., depths=[2, 2], scan_len=4, resi_connection='1conv', dynamic_ids=False,
             img_size=16, batch_size=1)
_LIGHT = dict(_BASE, embed_dim=60, d_state=1, ssm_ratio=1.1, mlp_ratio=1.6, upsampler='pixelshuffledirect')
_DEFAULT = dict(_BASE, embed_dim=60, d_state=16, ssm_ratio=1.5, mlp_ratio=2.0, upsampler='pixelshuffledirect')
_CLASSIC = dict(_BASE, embed_dim=180, d_state=16, ssm_ratio=2.0, mlp_ratio=2.5, upsampler='pixelshuffle')
#: name -> MaIR constructor keywords (the reference __main__ configurations, mair_arch.py:999-1003, with depths [2, 2])
CONFIGS = {
    "light_x2": dict(_LIGHT, upscale=2), "light_x3": dict(_LIGHT, upscale=3), "light_x4": dict(_LIGHT, upscale=4),
    "default_x2": dict(_DEFAULT, upscale=2),
    "classic_x2": dict(_CLASSIC, upscale=2), "classic_x3": dict(_CLASSIC, upscale=3), "classic_x4": dict(_CLASSIC, upscale=4),
}


def input_for(h, w):
    return synth.uniform(7, f"mair_sr_in_{h}x{w}", (1, 3, h, w), 0.0, 1.0)


def oracle_sr_forward(x, p, cfg):
    """MaIR.forward, SR branches (mair_arch.py:705-718), from oracle/mair_ref.py pieces; float64 in, float64 out."""
    B, C, H, W = x.shape
    hw, sl, r = (H, W), cfg["scan_len"], cfg["img_range"]
    mean = torch.tensor(mair_ref.RGB_MEAN, dtype=x.dtype).view(1, -1, 1, 1)
    tabs = [mair_ref.scan_ids(H, W, sl), mair_ref.scan_ids(H, W, sl, sl // 2)]
    x = (x - mean) * r
    first = F.conv2d(x, p["conv_first.weight"], p["conv_first.bias"], padding=1)
    E = first.shape[1]
    t = F.layer_norm(mair_ref._tok(first), (E,), p["patch_embed.norm.weight"], p["patch_embed.norm.bias"], 1e-5)
    li = 0
    while f"layers.{li}.conv.weight" in p:
        g_in, bi = t, 0
        while f"layers.{li}.residual_group.blocks.{bi}.ln_1.weight" in p:
            t = mair_ref.vss_block(t, p, f"layers.{li}.residual_group.blocks.{bi}.", hw, *tabs[bi % 2], mlp="conv_blk")
            bi += 1
        t = mair_ref._tok(F.conv2d(mair_ref._img(t, hw), p[f"layers.{li}.conv.weight"], p[f"layers.{li}.conv.bias"],
                                   padding=1)) + g_in
        li += 1
    t = F.layer_norm(t, (E,), p["norm.weight"], p["norm.bias"], 1e-5)
    x = F.conv2d(mair_ref._img(t, hw), p["conv_after_body.weight"], p["conv_after_body.bias"], padding=1) + first
    if cfg["upsampler"] == 'pixelshuffle':
        x = F.leaky_relu(F.conv2d(x, p["conv_before_upsample.0.weight"], p["conv_before_upsample.0.bias"], padding=1), 0.01)
        i = 0
        while f"upsample.{i}.weight" in p:
            wt = p[f"upsample.{i}.weight"]
            f = int(round((wt.shape[0] // wt.shape[1]) ** 0.5))
            x = F.pixel_shuffle(F.conv2d(x, wt, p[f"upsample.{i}.bias"], padding=1), f)
            i += 2
        x = F.conv2d(x, p["conv_last.weight"], p["conv_last.bias"], padding=1)
    else:
        x = F.pixel_shuffle(F.conv2d(x, p["upsample.0.weight"], p["upsample.0.bias"], padding=1), cfg["upscale"])
    return x / r + mean


def main():
    torch.set_grad_enabled(False)
    arch = gen_golden.import_reference_mairunet()
    out, meta = {}, {"configs": {}, "param_shapes": {}, "oracle_vs_reference": {}, "inputs": INPUTS,
                     "generated_by": "tools/gen_golden_mair_sr.py (reference mair_arch.MaIR, torch CPU fp32, train mode)",
                     "torch": torch.__version__}
    for name, cfg in CONFIGS.items():
        net = arch.flat.MaIR(**cfg)
        shapes = gen_golden.shapes_of(net)
        sd = synth.synth_state_dict(shapes, seed=42, rules=SYNTH_RULES)
        net.load_state_dict(sd, strict=True)
        net.train()
        meta["configs"][name] = cfg
        meta["param_shapes"][name] = {k: list(v) for k, v in shapes.items()}
        sd64 = {k: v.double() for k, v in sd.items()}
        for (h, w) in INPUTS:
            x = input_for(h, w)
            y = net(x)
            s = cfg["upscale"]
            assert tuple(y.shape) == (1, 3, s * h, s * w), y.shape
            d = gen_golden.maxabs(y, oracle_sr_forward(x.double(), sd64, cfg))
            meta["oracle_vs_reference"][f"{name}/{h}x{w}(float64 oracle, scan op = oracle stand-in)"] = d
            print(f"{name} {h}x{w}: out {tuple(y.shape)} range [{float(y.min()):.3f}, {float(y.max()):.3f}] "
                  f"float64 oracle vs reference {d:.3e}")
            assert d <= 2e-4, d
            out[f"{name}_{h}x{w}"] = y.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, "mair_sr.npz"), **out)
    with open(os.path.join(GOLD, "mair_sr.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(GOLD, "mair_sr.npz"), os.path.getsize(os.path.join(GOLD, "mair_sr.npz")), "bytes")


if __name__ == "__main__":
    main()
