"""MaIR super-resolution timing on the reference's __main__ configurations (mair_arch.py:999-1003), x4 on a
320x180 -> 1280x720 frame, synthetic weights:

  light    embed 60, depths 6x4, d_state 1, ssm 1.1, mlp 1.6, pixelshuffledirect (UpsampleOneStep)
  classic  embed 180, depths 6x6, d_state 16, ssm 2.0, mlp 2.5, pixelshuffle (conv_before_upsample + Upsample)

Per configuration: whole-frame forward and tiled call (LR patch 128, overlap 32, device blend at output scale), ms per
frame from HIP events; then one whole-frame forward under ops.KernelTimer: time per kernel group, the selective scan's
and the upsampling convs' achieved rate against the MI355X peaks, and the 1x1-GEMM path of every K = 60 / 66 / 90
layer.  The kernel table of record comes from a separate `rocprofv3 --kernel-trace --stats` run of `--once`.

usage: python tools/bench_mair_sr.py [--reps N] [--once] [--only light|classic]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from irm_amd import mair, ops, synth, utils  # noqa: E402

PEAK_F32_TFLOPS = 157.3        # MI355X_MICROARCH.md: f32 vector / f32-input MFMA peak
PEAK_F16_MFMA_TFLOPS = 2500.0  # dense fp16 MFMA peak
PEAK_HBM_GBS = 8000.0          # HBM3E peak

CONFIGS = {
    "light": dict(embed_dim=60, depths=(6, 6, 6, 6), d_state=1, ssm_ratio=1.1, mlp_ratio=1.6, upscale=4,
                  upsampler='pixelshuffledirect'),
    "classic": dict(embed_dim=180, depths=(6, 6, 6, 6, 6, 6), d_state=16, ssm_ratio=2.0, mlp_ratio=2.5, upscale=4,
                    upsampler='pixelshuffle'),
}
H, W, PATCH, OVERLAP = 180, 320, 128, 32


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_table(model, x):
    ops.TIMER = ops.KernelTimer(detail=True)
    try:
        model(x)
        rows = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    total = sum(r["ms"] for r in rows.values())
    groups = {}
    for k, r in rows.items():
        g = groups.setdefault(k.split(" ")[0], dict(ms=0.0, flops=0.0, bytes=0.0, launches=0))
        for f in g:
            g[f] += r[f]
    scan = groups.get("selective_scan", dict(ms=0.0, flops=0.0, bytes=0.0))
    ups = [dict(key=k, **r) for k, r in rows.items() if k.startswith("conv3x3") and (" ps" in k or " st2" in k)]
    bound = []
    for u in ups:
        emu = u["key"].startswith("conv3x3_f16x3")
        tf = (3.0 if emu else 1.0) * u["flops"] / (u["ms"] * 1e-3) / 1e12
        bound.append(dict(kernel=u["key"], ms=u["ms"], tflops=tf, frac_of_peak=tf / (PEAK_F16_MFMA_TFLOPS if emu else PEAK_F32_TFLOPS),
                          gbs=u["bytes"] / (u["ms"] * 1e-3) / 1e9))
    gemm = sorted(k for k in rows if k.startswith("gemm") and any(f"K{c}" in k.split() for c in (60, 66, 90)))
    return dict(
        total_ms=total,
        groups={k: dict(ms=round(v["ms"], 4), share=round(v["ms"] / total, 4), launches=v["launches"])
                for k, v in sorted(groups.items(), key=lambda kv: -kv[1]["ms"])},
        scan=dict(ms=scan["ms"], tflops=scan["flops"] / max(scan["ms"], 1e-9) / 1e9, gbs=scan["bytes"] / max(scan["ms"], 1e-9) / 1e6,
                  frac_f32_peak=scan["flops"] / max(scan["ms"], 1e-9) / 1e9 / PEAK_F32_TFLOPS,
                  frac_hbm_peak=scan["bytes"] / max(scan["ms"], 1e-9) / 1e6 / PEAK_HBM_GBS),
        upsampling_convs=bound,
        gemm_k60_66_90=gemm,
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one whole-frame and one tiled call per config (profiler run)")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lr = (synth.uniform(3, "mair_sr_bench_frame", (H, W, 3), 0.0, 1.0).numpy() * 255).astype(np.uint8)
    lr_dev = torch.from_numpy(lr).to(dev)
    x = torch.from_numpy(lr.transpose(2, 0, 1).astype(np.float32) / 255.0).unsqueeze(0).contiguous().to(dev)
    for name, cfg in CONFIGS.items():
        if a.only and name != a.only:
            continue
        model = mair.MaIR(**cfg).load_synthetic(42).eval().to(dev)
        with torch.no_grad():
            if a.once:
                model(x)
                utils.tiled_forward_device(model, lr_dev, PATCH, OVERLAP, pad8=True,
                                           max_batch=model.max_tiles_per_batch)
                torch.cuda.synchronize()
                print(json.dumps(dict(config=name, once=True)), flush=True)
                continue
            whole = timed(lambda: model(x), a.reps)
            tiled = timed(lambda: utils.tiled_forward_device(model, lr_dev, PATCH, OVERLAP, pad8=True,
                                                             max_batch=model.max_tiles_per_batch), a.reps)
            table = kernel_table(model, x)
        out = dict(config=name, frame=f"{W}x{H} -> {4 * W}x{4 * H}", params=sum(p.numel() for p in model.parameters()),
                   whole_frame_ms=round(whole, 3), tiled_ms=round(tiled, 3), tile=f"LR {PATCH}, overlap {OVERLAP}",
                   kernels=table)
        print(json.dumps(out), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
