"""Float32 frames and model chains, the part that needs no GPU: the C ABI of include/irm_hip_frames.h against
_hip.SIGNATURES_FRAMES, argument validation of the tiler and of utils.run_model_chain (before any GPU call), the
routing of _run_model_inference, and the constant range buffer of unit_range."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from irm_amd import _hip, deblurganv2, dncnn, mair, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_frame_minmax_f32", "irm_tile_extract_f32", "irm_window_blend_f32"]
CFG = {"patch_size": 64, "patch_overlap": 16}
CPU = torch.device("cpu")


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_three_symbols():
    """The float-frame entry points have a header of their own, include/irm_hip_frames.h, which irm_hip.h includes
    inside its extern "C" block, and a table of their own, _hip.SIGNATURES_FRAMES (the coverage rule of
    tests/test_guards_cpu.py reads _hip.SIGNATURES against the older guard-band file; the rule for this table is the
    next test): header and table match one to one, the library exports each symbol, load() binds it, and each one
    returns IRM_EINVAL for null pointers and zero sizes before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_frames.h"') < main.rindex("#ifdef __cplusplus")
    text = open(os.path.join(ROOT, "include", "irm_hip_frames.h")).read()
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_FRAMES)
    assert not set(_hip.SIGNATURES_FRAMES) & (set(_hip.SIGNATURES) | set(_hip.SIGNATURES_HALF))
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b"}
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_FRAMES[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_every_float_frame_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_FRAMES: each
    symbol is called by name in a test_guard_bands_* function of tests/test_gpu_float_frames.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_float_frames.py")) as f:
        text = f.read()
    reached = set()
    for body in re.split(r"^def ", text, flags=re.M):
        if body.startswith("test_guard_bands_"):
            reached |= set(re.findall(r'"(irm_\w+)"', body))
    missing = sorted(set(_hip.SIGNATURES_FRAMES) - reached)
    assert not missing, f"float-frame entry points without a guard-band case: {missing}"


def test_kernel_source_keeps_the_repository_rules():
    """No preprocessor conditional in the kernel file, in the frame-side header it includes (where the tile walk
    lives) and in the C header, and the reference's arithmetic is spelled with the correctly rounded intrinsics (a
    contracted multiply-add would break the bit-exact blend)."""
    csrc = os.path.join(os.path.dirname(_hip.LIB_PATH), "csrc")
    kernels = open(os.path.join(csrc, "tiler_f32.hip")).read()
    included = re.findall(r'^#include "(\w+\.h)"', kernels, flags=re.M)
    assert included == ["irm_frame.h"]
    walk = open(os.path.join(csrc, "irm_frame.h")).read()
    hdr = open(os.path.join(ROOT, "include", "irm_hip_frames.h")).read()
    for text in (kernels, walk, hdr):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    src = kernels + walk
    for word in ("__fdiv_rn(raw, hi)", "__fadd_rn(acc, __fmul_rn(p, w))", "__fdiv_rn(acc, fmaxf(wsum, 1e-8f))",
                 "fminf(fmaxf(__fmul_rn(v, mul), lo), hi)"):
        assert word in src, word
    assert "atomic" not in src.lower().replace("no atomics", "")


# --------------------------------------------------------------------------- the unit range
def test_unit_range_buffer():
    r = utils._unit_range_on(CPU)
    assert r.dtype == torch.float32 and r.tolist() == [0.0, 1.0, 1.0]
    assert utils._unit_range_on(CPU) is r, "one constant buffer per device"


# --------------------------------------------------------------------------- tiler arguments
class Never(torch.nn.Module):
    def forward(self, t):
        raise AssertionError("the model must not run")


def test_tiler_refuses_before_any_gpu_call():
    f = torch.zeros(64, 64, 3)
    u = torch.zeros(64, 64, 3, dtype=torch.uint8)
    m = Never()
    with pytest.raises(ValueError, match="out must be"):
        utils.tiled_forward_device(m, f, 64, 16, False, out="float64")
    with pytest.raises(ValueError, match="float32 frames, not torch.float64"):
        utils.tiled_forward_device(m, f.double(), 64, 16, False)
    with pytest.raises(ValueError, match="float32 frames, not torch.float16"):
        utils.tiled_forward_device(m, f.half(), 64, 16, False)
    with pytest.raises(ValueError, match="targets_dev"):
        utils.tiled_forward_device(m, f, 64, 16, False, target_dev=u)
    with pytest.raises(ValueError, match="targets_dev"):
        utils.tiled_forward_device(m, u, 64, 16, False, target_dev=u, out="float32")
    with pytest.raises(ValueError, match="deblurganv2"):
        utils.tiled_forward_device(m, f, 64, 16, False, hooks="deblurganv2")
    with pytest.raises(ValueError, match="deblurganv2"):
        utils.tiled_forward_device(m, u, 64, 16, False, hooks="deblurganv2", out="float32")
    # an integer result from a float32 frame needs the unit range; another integer type is no conversion
    with pytest.raises(ValueError, match="unit_range=True"):
        utils.tiled_forward_device(m, f, 64, 16, False, out="uint8")
    with pytest.raises(ValueError, match="unit_range=True"):
        utils.tiled_forward_device(m, u, 64, 16, False, out="uint16")


# --------------------------------------------------------------------------- the chain's arguments
def test_run_model_chain_validates_before_any_gpu_call():
    m = Never()
    img = np.zeros((64, 64, 3), np.uint8)
    for stages in ([], None, [m], [(m, CFG, 3)], [(m, {"patch_size": 64})], [("model", CFG)]):
        with pytest.raises(ValueError, match="run_model_chain"):
            utils.run_model_chain(stages, img, CPU)
    with pytest.raises(ValueError, match="DeblurGANv2"):
        utils.run_model_chain([(m, CFG), (deblurganv2.FPNMobileNet(), CFG)], img, CPU)
    with pytest.raises(ValueError, match="out must be"):
        utils.run_model_chain([(m, CFG)], img, CPU, out="uint8")
    for bad in (img.astype(np.float64), img.astype(np.float16), img[:, :, 0], img.astype(np.float32)[:, :, 0], "frame"):
        with pytest.raises(ValueError, match="float32 \\[H, W, C\\]"):
            utils.run_model_chain([(m, CFG)], bad, CPU)
    sr = Never()
    sr.upscale = 2
    with pytest.raises(ValueError, match="need_degradation"):
        utils.run_model_chain([(sr, CFG), (m, CFG)], img, CPU, need_degradation=True, noise_level=15)
    # valid arguments, no GPU: there is no CPU fallback
    for frame in (img, img.astype(np.uint16), img.astype(np.float32)):
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            utils.run_model_chain([(m, CFG), (sr, CFG)], frame, CPU)


def test_chain_hooks_follow_the_model_class():
    def chain_pad8(model):                      # what run_model_chain does per stage: the refusal, then the route
        utils.refuse_deblurgan(model, "run_model_chain", "run it on its own with get_model_prediction")
        return utils.model_route(model).pad8
    assert chain_pad8(dncnn.DnCNN(1, 1, 64, 17, "R")) is False
    assert chain_pad8(utils.Restormer()) is True
    assert all(issubclass(c, torch.nn.Module) for c in utils._PAD8_MODELS) and mair.MaIR in utils._PAD8_MODELS
    with pytest.raises(ValueError, match="DeblurGANv2"):
        chain_pad8(deblurganv2.FPNMobileNet())


def test_chain_stage_kinds(monkeypatch):
    """What each stage of a chain is asked for: float32 between the stages, the input's type (or float32) at the end,
    unit range throughout, noise at the first stage only."""
    calls = []

    def fake(model, frame, ps, ov, pad8, sigma, **kw):
        calls.append((str(frame.dtype), tuple(frame.shape), pad8, sigma, kw["unit_range"], kw["out"]))
        s = int(getattr(model, "upscale", 1))
        dt = {"float32": torch.float32, "uint8": torch.uint8, "uint16": torch.int16}[kw["out"]]
        return torch.zeros(s * frame.shape[0], s * frame.shape[1], min(3, frame.shape[2]), dtype=dt), None
    monkeypatch.setattr(utils, "tiled_forward_device", fake)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)         # (the upload to 'cuda')
    a, b, c = Never(), utils.Restormer(), Never()
    c.upscale = 2
    cuda = torch.device("cuda:0")
    out, ms = utils.run_model_chain([(a, CFG), (b, CFG), (c, CFG)], np.zeros((8, 10, 6), np.uint16), cuda, True, 25)
    assert out.dtype == np.uint16 and out.shape == (16, 20, 3)
    assert calls == [("torch.int16", (8, 10, 6), False, 25, True, "float32"),
                     ("torch.float32", (8, 10, 3), True, None, True, "float32"),
                     ("torch.float32", (8, 10, 3), False, None, True, "uint16")]
    del calls[:]
    out, _ = utils.run_model_chain([(b, CFG), (b, CFG)], np.zeros((8, 10, 3), np.uint8), cuda, out="float32")
    assert out.dtype == np.float32 and [c[-1] for c in calls] == ["float32", "float32"]
    del calls[:]
    out, _ = utils.run_model_chain([(b, CFG)], np.zeros((8, 10, 3), np.float32), cuda)
    assert out.dtype == np.float32 and calls == [("torch.float32", (8, 10, 3), True, None, True, "float32")]
    del calls[:]
    out, _ = utils.run_model_chain([(b, CFG)], np.zeros((8, 10, 3), np.uint8), cuda)
    assert out.dtype == np.uint8 and calls[0][-1] == "uint8"


# --------------------------------------------------------------------------- routing of the public call
def test_run_model_inference_routing(monkeypatch):
    """float32 HWC frames with the stock hooks take the device pipeline; float64 / float16 frames, custom hooks,
    DeblurGANv2 on a float frame and a frame that is not HWC keep the host loop."""
    took = []

    def dev_path(model, img_dev, *a, **kw):
        took.append(("device", str(img_dev.dtype), kw.get("hooks")))
        return torch.zeros(img_dev.shape[0], img_dev.shape[1], min(3, img_dev.shape[2]), dtype=img_dev.dtype), None

    def host_path(model, img, *a):
        took.append(("host", str(img.dtype), None))
        return np.zeros(img.shape, img.dtype)
    monkeypatch.setattr(utils, "tiled_forward_device", dev_path)
    monkeypatch.setattr(utils, "_run_tiles_on_host", host_path)
    m = Never()
    f = np.zeros((16, 24, 3), np.float32)
    pred, ms, out_dev = utils._run_model_inference(m, f, CPU, patch_size=64)
    assert took[-1] == ("device", "torch.float32", None) and out_dev is not None and pred.dtype == np.float32
    utils._run_model_inference(m, f, CPU, patch_size=64, pad=utils.pad)
    assert took[-1][0] == "device"
    for frame, kw in ((f.astype(np.float64), {}), (f.astype(np.float16), {}), (f[:, :, 0], {}),
                      (f, dict(normalize=lambda x: x)), (f, dict(postprocess=lambda x: x)),
                      (f, dict(pad=lambda x: x)),
                      (f, dict(normalize=deblurganv2.normalize, pad=deblurganv2.pad,
                               postprocess=deblurganv2.postprocess))):
        pred, ms, out_dev = utils._run_model_inference(m, frame, CPU, patch_size=64, **kw)
        assert took[-1][0] == "host" and out_dev is None, (frame.dtype, frame.ndim, sorted(kw))
    u8 = np.zeros((16, 24, 3), np.uint8)
    utils._run_model_inference(m, u8, CPU, patch_size=64, normalize=deblurganv2.normalize, pad=deblurganv2.pad,
                               postprocess=deblurganv2.postprocess)
    assert took[-1] == ("device", "torch.uint8", "deblurganv2")
