#!/usr/bin/env python3
"""Golden fixtures of MaIR+ (x8 self-ensemble with partitioned forward): tests/golden/mair_plus.npz and .json.

Runs where the reference tree is available (CPU).  It loads the reference's own mairplus_model.py by file path, with
sys.modules stubs for what is absent on the machine (torchvision.transforms.functional: hflip / vflip are flip(-1) /
flip(-2); the SRModel base; the model registry; tqdm), and calls its `augment`, `one_img_test` and `gather` on a plain
namespace that carries `opt={'scale': s}` and `net_g` - the cropping branch of one_img_test.  Stored:

  * geometry: with an identity `net_g` that records every chop's shape, the shapes per variant for six image sizes;
  * chop + ensemble under cheap networks that are not equivariant under flips / transposes (synthetic weights, seed
    42): the reference DnCNN with 5 layers on 3x230x410, and Conv2d(3, 3 s^2, 3, padding=1) + PixelShuffle(s) for
    s = 2, 3 on 3x64x210;
  * MaIR itself under the ensemble, one partition (16x16 and 12x20 inputs): light_x2 and classic_x2 of
    tools/gen_golden_mair_sr.py and the CDN denoising configuration with depths [2, 2]; the reference's train-mode
    CPU forward with the oracle's scan stand-in, as in gen_golden_mair_sr.py.

Usage: python tools/gen_golden_mair_plus.py
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import gen_golden  # noqa: E402
from irm_amd import synth  # noqa: E402
from irm_amd.dncnn import SYNTH_RULES as DN_RULES  # noqa: E402
from irm_amd.mair import SYNTH_RULES as MAIR_RULES  # noqa: E402
import gen_golden_mair_sr as sr  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
GEOMETRY_SIZES = [(199, 200), (200, 200), (230, 410), (64, 210), (401, 33), (720, 1280)]
DNCNN_LAYERS, DNCNN_INPUT = 5, (230, 410)
HEAD_SCALES, HEAD_INPUT = (2, 3), (64, 210)
HEAD_RULES = [[r"weight$", "range", [-0.3, 0.3]], [r"bias$", "range", [-0.1, 0.1]]]      # synth rules of the shuffle head
MAIR_INPUTS = [(16, 16), (12, 20)]
CDN_CFG = dict(upscale=1, in_chans=3, img_range=1., d_state=16, depths=[2, 2], embed_dim=180, ssm_ratio=1.3,
               mlp_ratio=2.0, upsampler=None, resi_connection='1conv', img_size=16, dynamic_ids=False, batch_size=1,
               scan_len=4)             # test_MaIR_CDN_s*.yml network_g with fewer groups / blocks
MAIR_CONFIGS = {"light_x2": sr.CONFIGS["light_x2"], "classic_x2": sr.CONFIGS["classic_x2"], "cdn": CDN_CFG}


def import_mairplus():
    """The reference's MaIRPlusModel class; call after gen_golden.import_reference_mairunet() (it installs `mair`)."""
    def pkg(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Reg:
        def register(self, *a, **k):
            return lambda cls: cls
    tf = pkg("torchvision.transforms.functional", hflip=lambda t: t.flip(-1), vflip=lambda t: t.flip(-2))
    pkg("torchvision.transforms", functional=tf)
    pkg("torchvision", transforms=sys.modules["torchvision.transforms"])
    sys.modules["mair.basicsr.utils.registry"].MODEL_REGISTRY = _Reg()
    pkg("mair.basicsr.models")
    pkg("mair.basicsr.models.sr_model", SRModel=type("SRModel", (), {}))
    if importlib.util.find_spec("tqdm") is None:
        pkg("tqdm", tqdm=lambda it, *a, **k: it)
    spec = importlib.util.spec_from_file_location("mair.basicsr.models.mairplus_model",
                                                  os.path.join(gen_golden.REF_SRC, "mair/basicsr/models/mairplus_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MaIRPlusModel


def run_plus(cls, net, x, scale):
    """MaIRPlusModel.test() without the progress bar: augment -> one_img_test per variant -> gather."""
    me = types.SimpleNamespace(opt={"scale": scale}, net_g=net)
    lqs = cls.augment(me, x)
    return cls.gather(me, [cls.one_img_test(me, lq) for lq in lqs])


class Recorder(nn.Module):
    def __init__(self):
        super().__init__()
        self.shapes = []

    def forward(self, x):
        self.shapes.append([int(x.shape[-2]), int(x.shape[-1])])
        return x


class ShuffleHead(nn.Sequential):
    def __init__(self, s):
        super().__init__(nn.Conv2d(3, 3 * s * s, 3, padding=1), nn.PixelShuffle(s))


def head_state(s):
    shapes = {"0.weight": (3 * s * s, 3, 3, 3), "0.bias": (3 * s * s,)}
    return synth.synth_state_dict(shapes, seed=42, rules=tuple((p, k, tuple(a)) for p, k, a in HEAD_RULES))


def plus_input(name, h, w):
    return synth.uniform(7, f"mair_plus_in_{name}_{h}x{w}", (1, 3, h, w), 0.0, 1.0)


def main():
    torch.set_grad_enabled(False)
    ref = gen_golden.import_reference()
    arch = gen_golden.import_reference_mairunet()
    cls = import_mairplus()
    out = {}
    meta = {"generated_by": "tools/gen_golden_mair_plus.py (reference mairplus_model.MaIRPlusModel augment / one_img_test "
                            "(net_g branch) / gather, torch CPU fp32)",
            "torch": torch.__version__, "chop_shapes": {}, "mair_configs": MAIR_CONFIGS, "mair_inputs": MAIR_INPUTS,
            "dncnn": {"layers": DNCNN_LAYERS, "input": DNCNN_INPUT}, "head": {"scales": HEAD_SCALES, "input": HEAD_INPUT, "rules": HEAD_RULES}}
    # ---- geometry: chop shapes per variant
    for h, w in GEOMETRY_SIZES:
        me = types.SimpleNamespace(opt={"scale": 1})
        x = torch.zeros(1, 1, h, w)
        per_variant = []
        for lq in cls.augment(me, x):
            me.net_g = Recorder()
            y = cls.one_img_test(me, lq)
            assert tuple(y.shape[-2:]) == tuple(lq.shape[-2:])
            per_variant.append(me.net_g.shapes)
        meta["chop_shapes"][f"{h}x{w}"] = per_variant
        print(f"geometry {h}x{w}: {[len(v) for v in per_variant]} chops, variant 0 {per_variant[0][:3]}...")
    # an identity network gives the input back, up to the rounding of torch's mean of 8 equal values
    x = plus_input("identity", 230, 410)
    assert gen_golden.maxabs(run_plus(cls, nn.Identity(), x, 1), x) <= 2.0 ** -22
    # ---- cheap, non-equivariant networks
    net = ref.dncnn.DnCNN(in_nc=3, out_nc=3, nc=64, nb=DNCNN_LAYERS, act_mode="R")
    net.load_state_dict(synth.synth_state_dict(gen_golden.shapes_of(net), seed=42, rules=DN_RULES), strict=True)
    h, w = DNCNN_INPUT
    x = plus_input("dncnn", h, w)
    y = run_plus(cls, net, x, 1)
    single = net.eval()(x)
    meta["dncnn"]["ensemble_vs_single_forward"] = gen_golden.maxabs(y, single)
    print(f"dncnn{DNCNN_LAYERS} {h}x{w}: out {tuple(y.shape)}, ensemble vs plain forward {gen_golden.maxabs(y, single):.3e}")
    assert tuple(y.shape) == (1, 3, h, w) and gen_golden.maxabs(y, single) > 1e-4        # not equivariant
    out[f"dncnn{DNCNN_LAYERS}_{h}x{w}"] = y.numpy().astype(np.float32)
    h, w = HEAD_INPUT
    for s in HEAD_SCALES:
        net = ShuffleHead(s)
        net.load_state_dict(head_state(s), strict=True)
        x = plus_input(f"head_x{s}", h, w)
        y = run_plus(cls, net, x, s)
        d = gen_golden.maxabs(y, net(x))
        print(f"shuffle head x{s} {h}x{w}: out {tuple(y.shape)}, ensemble vs plain forward {d:.3e}")
        assert tuple(y.shape) == (1, 3, s * h, s * w) and d > 1e-4
        out[f"head_x{s}_{h}x{w}"] = y.numpy().astype(np.float32)
    # ---- MaIR under the ensemble (one partition)
    for name, cfg in MAIR_CONFIGS.items():
        net = arch.flat.MaIR(**cfg)
        net.load_state_dict(synth.synth_state_dict(gen_golden.shapes_of(net), seed=42, rules=MAIR_RULES), strict=True)

        class TrainMode(nn.Module):           # one_img_test switches net_g to eval(): keep the train-mode CPU forward
            def forward(self, t):
                return net.train()(t)

            def eval(self):
                return self

            def train(self, mode=True):
                return self
        s = cfg["upscale"]
        for h, w in MAIR_INPUTS:
            x = plus_input(name, h, w)
            y = run_plus(cls, TrainMode(), x, s)
            d = gen_golden.maxabs(y, net.train()(x))
            print(f"mair {name} {h}x{w}: out {tuple(y.shape)}, ensemble vs plain forward {d:.3e}")
            assert tuple(y.shape) == (1, 3, s * h, s * w) and d > 1e-5
            out[f"mair_{name}_{h}x{w}"] = y.numpy().astype(np.float32)
    meta["files"] = save_split(out)
    with open(os.path.join(GOLD, "mair_plus.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


def save_split(out, budget=200_000):
    """A committed file stays below 1 MiB: arrays are cut into row bands `name@first_row` of at most `budget` values
    and the bands spread over mair_plus.npz, mair_plus_1.npz, ... (tests concatenate the bands in row order)."""
    bands = []
    for name, a in out.items():
        rows = max(1, budget // int(np.prod(a.shape[:-2]) * a.shape[-1]))
        bands += [(f"{name}@{r}", a[..., r:r + rows, :]) for r in range(0, a.shape[-2], rows)]
    files, cur, n = [], {}, 0
    for key, a in bands + [(None, None)]:
        if key is None or (cur and n + a.size > budget):
            fname = "mair_plus.npz" if not files else f"mair_plus_{len(files)}.npz"
            path = os.path.join(GOLD, fname)
            np.savez_compressed(path, **cur)
            assert os.path.getsize(path) < 1 << 20, (fname, os.path.getsize(path))
            print("wrote", path, os.path.getsize(path), "bytes")
            files.append(fname)
            cur, n = {}, 0
        if key is not None:
            cur[key] = np.ascontiguousarray(a)
            n += a.size
    return files


if __name__ == "__main__":
    main()
