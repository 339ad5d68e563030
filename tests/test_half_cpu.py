"""CPU tests of the fp16 inference mode of the conv stacks: weight packing, the `precision` keyword through every
layer of the public interface, and the C ABI of the three entry points (no GPU needed)."""
import math
import os
import re

import pytest
import torch

from irm_amd import _hip, dncnn, rednet, synth, utils

import half_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("irm_conv3x3_h_in_f32", "irm_conv3x3_h_f16", "irm_conv3x3_h_out_f32")


@pytest.mark.parametrize("co,ci,gain", [(64, 64, 1.0), (128, 64, 3.0e-4), (64, 128, 700.0), (128, 128, 1.0)])
def test_pack_round_trip_and_scale(co, ci, gain):
    w = synth.uniform(3, f"hw{co}_{ci}", (co, ci, 3, 3), -1.0, 1.0) * gain
    packed, inv = _hip.pack_conv3x3_h(w)
    assert packed.dtype == torch.float16 and packed.numel() == co * ci * 9
    s = 1.0 / inv
    assert math.log2(s) == int(math.log2(s)), "the scale is a power of two"
    top = float(w.abs().max()) * s
    assert 2.0 ** 13 <= top < 2.0 ** 14
    want = (w.double() * s).numpy().astype("float16").astype("float64") / s        # RNE_fp16(W s) / s, one rounding
    got = _hip.unpack_conv3x3_h(packed, inv, co, ci)
    assert torch.equal(got.double(), torch.from_numpy(want))
    assert torch.equal(half_model.quantised_weight(w), got)


def test_pack_fragment_order():
    """The element the kernel's lane (g, m) reads as half j of (stage, tap, mtile, k-step)."""
    co, ci = 128, 128
    w = synth.uniform(4, "hfrag", (co, ci, 3, 3), -1.0, 1.0)
    packed, inv = _hip.pack_conv3x3_h(w)
    p = packed.view(ci // 64, 9, co // 16, 2, 64, 8)
    q = (w * (1.0 / inv)).half()
    for st, tap, mt, ks, lane, j in [(0, 0, 0, 0, 0, 0), (1, 5, 7, 1, 37, 3), (0, 8, 3, 1, 63, 7), (1, 2, 4, 0, 16, 1)]:
        g, m = lane >> 4, lane & 15
        assert p[st, tap, mt, ks, lane, j] == q[16 * mt + m, 64 * st + 32 * ks + 8 * g + j, tap // 3, tap % 3]


def test_pack_all_zero_weights():
    packed, inv = _hip.pack_conv3x3_h(torch.zeros(64, 64, 3, 3))
    assert inv == 1.0 and not bool(packed.any())
    assert not bool(_hip.unpack_conv3x3_h(packed, inv, 64, 64).any())


def test_pack_rejects_other_shapes():
    with pytest.raises(ValueError):
        _hip.pack_conv3x3_h(torch.zeros(64, 3, 3, 3))
    with pytest.raises(ValueError):
        _hip.pack_conv3x3_h(torch.zeros(96, 64, 3, 3))


def test_constructors_take_precision():
    assert dncnn.DnCNN(1, 1, 64, 17, "R").precision == "fp32"
    assert rednet.REDNet().precision == "fp32"
    d = dncnn.DnCNN(3, 3, 64, 20, "R", precision="fp16")
    r = rednet.REDNet(precision="fp16")
    assert d.precision == "fp16" and r.precision == "fp16" and d.hip_graph and r.hip_graph
    for bad in ("bf16", "half", None, 16):
        with pytest.raises(ValueError):
            dncnn.DnCNN(1, 1, 64, 17, "R", precision=bad)
        with pytest.raises(ValueError):
            rednet.REDNet(precision=bad)
    with pytest.raises(ValueError):                      # the fp16 layout has 64 or 128 channels
        dncnn.DnCNN(1, 1, 48, 17, "R", precision="fp16")
    # the same checkpoint loads in either mode
    assert list(d.state_dict()) == list(dncnn.DnCNN(3, 3, 64, 20, "R").state_dict())
    assert list(r.state_dict()) == list(rednet.REDNet().state_dict())
    d.load_state_dict(dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(1).state_dict(), strict=True)
    d.release_workspace(), r.release_workspace()


def test_loaders_forward_precision(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("weights/DnCNN")
    os.makedirs("weights/REDNet")
    torch.save(dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(2).state_dict(), "weights/DnCNN/dncnn_25.pth")
    torch.save(rednet.REDNet().load_synthetic(3).state_dict(), "weights/REDNet/25.pt")
    cpu = torch.device("cpu")
    for prec in ("fp32", "fp16"):
        assert dncnn.get_model("weights/DnCNN/dncnn_25.pth", 1, 17, cpu, precision=prec).precision == prec
        assert rednet.get_model("weights/REDNet/25.pt", cpu, precision=prec).precision == prec
        got = utils.get_model_instance("denoising", "gaussian", "DnCNN", cpu, gray=True, sigma=25, precision=prec)
        assert got.precision == prec and got.nb == 17
        got = utils.get_model_instance("denoising", "gaussian", "REDNet", cpu, sigma=25, precision=prec)
        assert got.precision == prec
    assert utils.get_model_instance("denoising", "gaussian", "REDNet", cpu, sigma=25).precision == "fp32"
    with pytest.raises(ValueError):
        utils.get_model_instance("denoising", "gaussian", "DnCNN", cpu, gray=True, sigma=25, precision="bf16")


@pytest.mark.parametrize("args", [("deblurring", "motion", "Restormer"), ("denoising", "real", "MaIR"),
                                  ("denoising", "real", "MaIR+"), ("deblurring", "motion", "DeblurGANv2 (MobileNet)")])
def test_fp16_is_refused_for_other_families(args):
    with pytest.raises(ValueError, match="DnCNN and REDNet"):
        utils.get_model_instance(*args, torch.device("cpu"), precision="fp16")


def test_header_declares_the_three_symbols():
    """The fp16 entry points have a header of their own, include/irm_hip_half.h, which irm_hip.h includes inside its
    extern "C" block, and a table of their own, _hip.SIGNATURES_HALF: the two match one to one, the library exports
    each symbol, load() binds it, and each one returns IRM_EINVAL for null pointers and zero sizes before any HIP call."""
    import ctypes
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_half.h"') < main.rindex("#ifdef __cplusplus")
    text = open(os.path.join(ROOT, "include", "irm_hip_half.h")).read()
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_HALF)
    assert not set(_hip.SIGNATURES_HALF) & set(_hip.SIGNATURES)
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b", ctypes.c_float: r"^float\b"}
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_HALF[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_every_fp16_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_HALF: each of
    its symbols is reached in tests/test_gpu_half.py, where every kernel case runs between sentinels, through its wrapper
    (ops_half.py, also reachable as ops.conv3x3_h*); a fp16 kernel added later fails here until it gets a case."""
    wrappers = {"ops.conv3x3_h_in(": "irm_conv3x3_h_in_f32", "ops.conv3x3_h(": "irm_conv3x3_h_f16",
                "ops.conv3x3_h_out(": "irm_conv3x3_h_out_f32"}
    with open(os.path.join(ROOT, "tests", "test_gpu_half.py")) as f:
        text = f.read()
    with open(os.path.join(os.path.dirname(_hip.LIB_PATH), "ops_half.py")) as f:
        ops_text = f.read()
    reached = set()
    for call, symbol in wrappers.items():
        body = ops_text[ops_text.index("def " + call[len("ops."):]):]
        body = body[:body.index("\ndef ", 1)] if "\ndef " in body[1:] else body
        assert symbol in body, f"{call} no longer calls {symbol}"
        if call in text:
            reached.add(symbol)
    missing = sorted(set(_hip.SIGNATURES_HALF) - reached)
    assert not missing, f"fp16 entry points without a guard-band case: {missing}"


def test_chain_model_rounding_helpers():
    v = torch.tensor([0.0, 1.0, 1.5, 2047.0, 2048.0, 65504.0, 3.0e-6, -0.3], dtype=torch.float64)
    want = torch.tensor([2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 1.0, 2.0, 32.0, 2.0 ** -24, 2.0 ** -12], dtype=torch.float64)
    assert torch.equal(half_model.ulp16(v), want)
    t = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.9, 65520.0, -1e9, float("nan")], dtype=torch.float64)
    q = half_model.rne16(t)
    assert q[0] == 1.0 and q[1] == 1.0 + 2.0 ** -9 and q[2] == 65504.0 and q[3] == float("inf") and q[4] == -float("inf")
    assert bool(torch.isnan(q[5]))
    # float64 -> fp16 in ONE rounding: just above a tie in float64, on the tie after a float32 step
    assert half_model.rne16(torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -40], dtype=torch.float64))[0] == 1.0 + 2.0 ** -10
