"""Launch stream and output of every model's forward, for comparing two builds of the host code on one GPU.

  launch_trace.py OUT            every case, each in a fresh process with a time limit; stops at the first failure
  launch_trace.py OUT CASE       one case: OUT/CASE.json (the trace) and OUT/CASE.pt (the outputs)
  launch_trace.py --compare A B  exit status 1 unless every trace of A equals B's and every output passes torch.equal

A case seeds its input, calls load_synthetic(3), and logs every _hip.call of one eager forward (hip_graph off): the
entry point and each argument whose declared ctypes type is not a pointer.  It then saves that output, the output of
one more forward through utils.graphed_forward, and the output of an eager forward under an installed ops.KernelTimer
(which must not change the result)."""
import ctypes
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = sys.path[0]


def _cases():
    from irm_amd import deblurganv2 as dg, dncnn, mair, rednet, restormer
    R, U, M = restormer.Restormer, mair.MaIRUNet, mair.MaIR
    cases = {
        "restormer_256": (R, {}, (2, 3, 256, 256)),          # whole 8x32 tiles in chunks of four at every level
        "restormer_offtile": (R, {}, (1, 3, 40, 24)),        # every level on the generic block
        "restormer_biasfree": (R, dict(LayerNorm_type="BiasFree"), (1, 3, 64, 64)),
        "restormer_bias": (R, dict(bias=True), (1, 3, 64, 64)),
        "restormer_dual": (R, dict(dual_pixel_task=True, inp_channels=6), (1, 6, 64, 64)),
        "mairunet": (U, {}, (1, 3, 64, 64)),
        "mairunet_dual": (U, dict(dual_pixel_task=True), (1, 3, 64, 64)),
        "mair_dn": (M, dict(upsampler=None, upscale=1), (1, 3, 32, 32)),
        "mair_x3_direct": (M, dict(upsampler="pixelshuffledirect", upscale=3), (1, 3, 32, 32)),
        "mair_x4_classic": (M, dict(upsampler="pixelshuffle", upscale=4), (1, 3, 32, 32)),
        "fpn_mobilenet": (dg.FPNMobileNet, {}, (1, 3, 64, 64)),
        "fpn_inception": (dg.FPNInceptionDecoder, {}, (1, 3, 128, 160)),
    }
    for p in ("fp32", "fp16"):
        cases[f"dncnn_{p}"] = (dncnn.DnCNN, dict(act_mode="R", precision=p), (2, 1, 32, 32))
        cases[f"rednet_{p}"] = (rednet.REDNet, dict(precision=p), (2, 1, 32, 32))
    return cases


def run_case(out, name):
    import numpy as np
    import torch
    import irm_amd  # noqa: F401
    from irm_amd import _hip, ops, synth, utils
    cls, kwargs, shape = _cases()[name]
    model = cls(**kwargs).load_synthetic(3).to("cuda")
    model.train(name.startswith("fpn"))                   # the DeblurGANv2 generators run in train mode
    inputs = [synth.uniform(11, "trace_in", shape, 0.0, 1.0).cuda()]
    if name == "fpn_inception":                           # the encoder maps are inputs: sizes as in the decoder's GPU test
        sizes = np.load(os.path.join(ROOT, "tests", "golden", "fpn_inception.npz"))["fi_sizes_128x160"]
        inputs += [synth.uniform(11, f"trace_enc{i}", (1, c, int(s[0]), int(s[1])), -1.0, 1.0).cuda()
                   for i, (c, s) in enumerate(zip((32, 64, 192, 1088, 2080), sizes))]
    sigs = {**_hip.SIGNATURES, **_hip.SIGNATURES_HALF, **_hip.SIGNATURES_FRAMES, **_hip.SIGNATURES_GRAM,
            **_hip.SIGNATURES_YUV, **_hip.SIGNATURES_INCEPTION}
    trace, call = [], _hip.call

    def logged(entry, *args):
        trace.append([entry] + [float(a) if t in (ctypes.c_float, ctypes.c_double) else int(a)
                                for a, t in zip(args, sigs[entry]) if t is not ctypes.c_void_p])
        call(entry, *args)

    graph, model.hip_graph = getattr(model, "hip_graph", False), False
    _hip.call = logged
    outs = {"eager": model(*inputs).clone()}
    _hip.call = call
    model.hip_graph = graph
    # (the decoder with its six inputs is not a graphed_forward model: a second eager forward stands in)
    outs["graphed"] = (utils.graphed_forward(model, inputs[0]) if len(inputs) == 1 else model(*inputs)).clone()
    ops.TIMER = ops.KernelTimer()
    outs["timer"] = model(*inputs).clone()
    ops.TIMER = None
    torch.cuda.synchronize()
    with open(os.path.join(out, name + ".json"), "w") as f:
        json.dump(trace, f)
    torch.save({k: v.cpu() for k, v in outs.items()}, os.path.join(out, name + ".pt"))
    same = torch.equal(outs["eager"], outs["timer"])
    print(f"{name}: {len(trace)} launches, timer output {'equal' if same else 'DIFFERS'}", flush=True)
    return 0 if same else 1


def compare(a, b):
    import torch
    bad = 0
    for f in sorted(os.listdir(a)):
        if f.endswith(".json"):
            ok = json.load(open(os.path.join(a, f))) == json.load(open(os.path.join(b, f)))
        else:
            x, y = (torch.load(os.path.join(d, f)) for d in (a, b))
            ok = x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in x)
        print(f"{f}: {'equal' if ok else 'MISMATCH'}")
        bad += not ok
    return 1 if bad or sorted(os.listdir(a)) != sorted(os.listdir(b)) else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    os.makedirs(sys.argv[1], exist_ok=True)
    if len(sys.argv) > 2:
        sys.exit(run_case(sys.argv[1], sys.argv[2]))
    import irm_amd  # noqa: F401
    for case in _cases():
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), sys.argv[1], case], timeout=240).returncode
        if rc:
            sys.exit(f"{case}: exit status {rc}; nothing further is started")
