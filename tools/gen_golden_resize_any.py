#!/usr/bin/env python3
"""Golden fixtures of the resize to any size: tests/golden/resize_any.npz and resize_any.json.

Runs where the reference tree is available (CPU).  It loads the reference's basicsr utils/matlab_functions.py by path,
as tools/gen_golden_sr_protocol.py does, and stores the reference's float32 imresize(x, s) for the scales below - none of
them a factor utils.resize_table takes - with the measured max-abs distance of utils.resize_host(scale=s) from each.

The sources are not stored again: they are the [:61, :83] slices of hr_random and hr_synth of tests/golden/sr_protocol.npz,
as uint8 / 255 in float32.  The fixtures hold arrays and numbers only.

Usage: python tools/gen_golden_resize_any.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_golden_sr_protocol import GOLD, import_reference  # noqa: E402
from irm_amd import utils  # noqa: E402

#: key -> scale; the slice every source is cut to
SCALES = {"s0750": 0.75, "s0667": 2.0 / 3.0, "s0900": 0.9, "s0400": 0.4, "s0300": 0.3, "s1250": 1.25, "s1500": 1.5}
SLICE = (61, 83)
NAMES = ("random", "synth")


def main():
    mf, _ = import_reference()
    src = np.load(os.path.join(GOLD, "sr_protocol.npz"))
    out, meta = {}, {
        "generated_by": "tools/gen_golden_resize_any.py (reference basicsr imresize, loaded by file path, numpy / torch CPU)",
        "sources": "hr_<name>[:61, :83] of sr_protocol.npz, uint8 / 255 in float32",
        "scales": SCALES, "resize_host_vs_reference": {}}
    for name in NAMES:
        u8 = np.ascontiguousarray(src[f"hr_{name}"][:SLICE[0], :SLICE[1]])
        x32 = u8.astype(np.float32) / np.float32(255.0)
        for key, s in SCALES.items():
            ref = mf.imresize(x32, s)
            assert ref.dtype == np.float32
            host = utils.resize_host(u8, scale=s)
            assert host.shape == ref.shape, (key, host.shape, ref.shape)
            d = float(np.abs(host - ref.astype(np.float64)).max())
            out[f"{key}_{name}"] = ref
            meta["resize_host_vs_reference"][f"{key}_{name}"] = d
            print(f"{key}_{name}: x{s:g} -> {ref.shape}, resize_host float64 vs reference {d:.3e}")
    npz = os.path.join(GOLD, "resize_any.npz")
    np.savez_compressed(npz, **out)
    with open(os.path.join(GOLD, "resize_any.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", npz, os.path.getsize(npz), "bytes")
    assert os.path.getsize(npz) < (1 << 20)


if __name__ == "__main__":
    main()
