"""DeblurGANv2 FPN-Inception on one GPU: the hand-written path against the library-composed forward of the same network.

  frame      a 1280x720 uint8 frame through utils.get_model_prediction with the stock patch entry (768 / 128: two tiles,
             each padded to 736x800), host clock from upload to the downloaded result, median of --frames runs after two
             warm-up runs; the same for FPNMobileNet with its own entry, for context
  tile       one padded tile [1, 3, 736, 800]: the forward replayed from a HIP graph, device events around a replay,
             median of --reps; and the eager forward (host launch cost included)
  composed   the float32 plain-torch statement of the network (tests/inception_model.py) moved to the GPU: the same
             tile through torch's library kernels, device events around a forward, median of --reps after warm-up; the
             largest difference between the two outputs.  If it cannot run, the error is recorded instead
  kernels    one eager forward of the tile under ops.KernelTimer: per kernel its launches, time, algorithmic FLOPs and
             compulsory bytes, and the share of its own bound, max(FLOPs / 155 TFLOP/s, bytes / 6.29 TB/s) over the
             time (the measured exact-f32 matrix rate and the measured HBM copy rate of the MI355X).  Events around
             every launch add to short kernels: the table says where the time goes, the graph replay says how much

The weights are synthetic (load_synthetic).  Prints one JSON line per record; --out FILE writes them too."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import irm_amd  # noqa: F401
from irm_amd import deblurganv2, ops, synth, utils

PEAK_FLOPS, PEAK_BYTES = 155e12, 6.29e12


def _events_ms(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), reps=reps)


def _frame_ms(model, img, dev, name, runs):
    cfg = utils.get_patch_config("deblurring", "motion", name)
    for _ in range(2):
        out, _ = utils.get_model_prediction(model, img, dev, **cfg)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, _ = utils.get_model_prediction(model, img, dev, **cfg)
        ts.append((time.perf_counter() - t0) * 1e3)
    assert out.shape == img.shape and out.dtype == img.dtype
    return dict(record="frame", model=name, frame=f"{img.shape[1]}x{img.shape[0]}", patch=cfg,
                median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tile", default="736x800", help="HxW of the padded tile")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inception: needs a GPU")
    dev = torch.device("cuda:0")
    th, tw = (int(v) for v in a.tile.split("x"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:                                  # line by line: a later stage that fails keeps the earlier records
            with open(a.out, "a") as f:
                f.write(line + "\n")

    model = deblurganv2.FPNInception().load_synthetic(42).to(dev).train(True)
    img, _ = synth.synth_image_pair(0, 720, 1280, 3)
    emit(_frame_ms(model, img, dev, "DeblurGANv2 (Inception)", a.frames))
    mobile = deblurganv2.FPNMobileNet().load_synthetic(42).to(dev).train(True)
    emit(_frame_ms(mobile, img, dev, "DeblurGANv2 (MobileNet)", a.frames))
    del mobile

    # ---- one padded tile: graph replay and eager
    x = synth.uniform(7, "bench_inception_tile", (1, 3, th, tw), -1.0, 1.0).to(dev)
    for _ in range(2):
        ours = utils.graphed_forward(model, x).clone()
    rec = dict(record="tile", input=f"1x3x{th}x{tw}", graph=_events_ms(lambda: utils.graphed_forward(model, x), a.reps))
    model.__dict__.pop("_irm_graphs", None)
    rec["eager"] = _events_ms(lambda: model(x), a.reps)
    emit(rec)

    # ---- per-kernel table
    torch.cuda.synchronize()
    ops.TIMER = ops.KernelTimer(detail=True)
    try:
        model(x)
        detail = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    table = {}
    for k, v in detail.items():                    # by kernel; convkxk by geometry as well ("convkxk 3x3 s2")
        parts = k.split(" ")
        d = table.setdefault(" ".join(parts[:3]) if parts[0] == "convkxk" else parts[0],
                             dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
        for f in d:
            d[f] += v[f]
    total = sum(v["ms"] for v in table.values())
    for k, v in sorted(table.items(), key=lambda kv: -kv[1]["ms"]):
        s = v["ms"] * 1e-3
        bound_f, bound_b = v["flops"] / PEAK_FLOPS, v["bytes"] / PEAK_BYTES
        emit(dict(record="kernel", kernel=k, launches=v["launches"], ms=round(v["ms"], 4), share=round(v["ms"] / total, 4),
                  gflop=round(v["flops"] / 1e9, 3), mbytes=round(v["bytes"] / 1e6, 2),
                  tflops=round(v["flops"] / s / 1e12, 2) if s else None, gbytes_s=round(v["bytes"] / s / 1e9, 1) if s else None,
                  bound="matrix" if bound_f >= bound_b else "hbm",
                  share_of_bound=round(max(bound_f, bound_b) / s, 4) if s else None))
    emit(dict(record="kernels_total", ms=round(total, 3), launches=sum(v["launches"] for v in table.values()),
              gflop=round(sum(v["flops"] for v in table.values()) / 1e9, 2)))

    # ---- the composed forward of the same network
    rec = dict(record="composed", input=f"1x3x{th}x{tw}")
    try:
        import inception_model as im
        net = im.build(torch.float32, {k: v.cpu() for k, v in model.state_dict().items()}).to(dev)
        for _ in range(3):
            theirs = im.forward(net, x)
        torch.cuda.synchronize()
        rec.update(_events_ms(lambda: im.forward(net, x), a.reps))
        rec["max_abs_difference"] = float((theirs - ours).abs().max())
        del net, theirs
    except Exception as exc:                       # recorded, not hidden: the comparison is then absent from the file
        rec["error"] = f"{type(exc).__name__}: {exc}"[:500]
    emit(rec)


if __name__ == "__main__":
    main()
