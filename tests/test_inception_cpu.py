"""DeblurGANv2 FPN-Inception, the part that needs no GPU: the plain-torch statement of the network
(tests/inception_model.py) against the two published facts that pin it, the state dict of deblurganv2.FPNInception
against it, the checkpoint loader, the C ABI of include/irm_hip_inception.h against _hip.SIGNATURES_INCEPTION, argument
validation before any HIP call, and the launch planner."""
import ctypes
import os
import re

import pytest
import torch

import inception_model as im
import ledger
from irm_amd import _hip, deblurganv2, ops, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_convkxk_f32", "irm_pool3x3_f32"]
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def net():
    torch.manual_seed(3)
    return im.build(torch.float64)


# --------------------------------------------------------------------------- the network
def test_parameter_counts(net):
    """55 843 464 is the figure of the published model table for inception_resnet_v2 with 1000 classes; the part
    FPN.forward runs (through mixed_7a) has 30 754 272."""
    inc = net.fpn.inception
    assert sum(p.numel() for p in inc.parameters()) == im.PARAMS_FULL == 55_843_464
    used = sum(p.numel() for k, p in inc.named_parameters() if not k.startswith(im.TAIL))
    assert used == im.PARAMS_USED == 30_754_272
    model = deblurganv2.FPNInception()
    assert sum(p.numel() for p in model.fpn.inception.parameters()) == im.PARAMS_USED


def test_map_sizes(net):
    """128x160 gives the sizes the reference's decoder golden was recorded with (ledger.FI_ENC); 256x128 follows the
    side formula 16k-1, 8k-2, 4k-3, 2k-2, k-2 for a side of 32k."""
    got = [tuple(e.shape[1:]) for e in im.encoder_maps(net, torch.zeros(1, 3, 128, 160, dtype=torch.float64))]
    assert tuple(got) == ledger.FI_ENC
    got = [tuple(e.shape[1:]) for e in im.encoder_maps(net, torch.zeros(1, 3, 256, 128, dtype=torch.float64))]
    want = [(c, h, w) for c, h, w in zip((32, 64, 192, 1088, 2080), im.map_sides(256), im.map_sides(128))]
    assert got == want and im.map_sides(256) == (127, 62, 29, 14, 6) and im.map_sides(128) == (63, 30, 13, 6, 2)


def test_state_dict_is_the_helpers_minus_the_tail(net):
    want = {k: tuple(v.shape) for k, v in net.state_dict().items() if not im.is_tail(k)}
    got = {k: tuple(v.shape) for k, v in deblurganv2.FPNInception().state_dict().items()}
    assert got == want
    assert any(im.is_tail(k) for k in net.state_dict()) and not any(im.is_tail(k) for k in got)
    for alias in ("fpn.enc0.conv.weight", "fpn.enc1.1.bn.bias", "fpn.enc2.0.conv.weight", "fpn.enc3.1.9.conv2d.bias",
                  "fpn.enc3.2.branch1.2.conv.weight", "fpn.enc4.0.19.branch1.1.conv.weight", "fpn.enc4.1.branch2.2.bn.weight"):
        assert alias in got, alias
    # the decoder keeps its own keys: the new class adds, it does not rename
    dec = deblurganv2.FPNInceptionDecoder().state_dict()
    assert set(dec) <= set(got) and all(tuple(dec[k].shape) == got[k] for k in dec)


def test_loader_reads_a_reference_shaped_checkpoint(net, tmp_path, capsys):
    full = {k: v.float() for k, v in net.state_dict().items()}
    for prefix in ("", "module."):
        path = os.path.join(tmp_path, f"fpn_inception{len(prefix)}.h5")
        torch.save({"model": {prefix + k: v for k, v in full.items()}}, path)
        model = deblurganv2.get_model_inception(path, CPU)
        assert isinstance(model, deblurganv2.FPNInception) and model.training
        assert "Successfully loaded" in capsys.readouterr().out
        sd = model.state_dict()
        assert all(torch.equal(sd[k], full[k]) for k in sd)
        # an alias and its original are one tensor
        assert model.fpn.enc0.conv.weight is model.fpn.inception.conv2d_1a.conv.weight
    used = {k: v for k, v in full.items() if not im.is_tail(k)}
    torch.save({"model": used}, os.path.join(tmp_path, "notail.h5"))      # the tail may be absent as well
    deblurganv2.get_model_inception(os.path.join(tmp_path, "notail.h5"), CPU)
    missing = {k: v for k, v in full.items() if k != "fpn.inception.repeat_1.7.branch1.1.conv.weight"}
    torch.save({"model": missing}, os.path.join(tmp_path, "missing.h5"))
    with pytest.raises(RuntimeError, match="Missing key"):
        deblurganv2.get_model_inception(os.path.join(tmp_path, "missing.h5"), CPU)
    shaped = dict(full)
    shaped["fpn.inception.mixed_5b.branch1.1.conv.weight"] = torch.zeros(64, 48, 3, 3)
    torch.save({"model": shaped}, os.path.join(tmp_path, "shape.h5"))
    with pytest.raises(RuntimeError, match="size mismatch"):
        deblurganv2.get_model_inception(os.path.join(tmp_path, "shape.h5"), CPU)
    extra = dict(full, **{"fpn.inception.conv2d_9z.conv.weight": torch.zeros(1)})
    torch.save({"model": extra}, os.path.join(tmp_path, "extra.h5"))
    with pytest.raises(RuntimeError, match="Unexpected key"):
        deblurganv2.get_model_inception(os.path.join(tmp_path, "extra.h5"), CPU)


def test_reference_shaped_loaders_name_the_new_one(tmp_path):
    """deblurganv2.get_model keeps refusing the fpn_inception file stem (existing tests pin that); its message now
    says which loader builds the generator."""
    with pytest.raises(NotImplementedError, match="get_model_inception"):
        deblurganv2.get_model(os.path.join(tmp_path, "fpn_inception.h5"), CPU)


def test_refusals_without_a_gpu():
    model = deblurganv2.FPNInception()
    assert model.hip_graph is True and model.max_tiles_per_batch == 2
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        model(torch.zeros(1, 3, 128, 128))
    with pytest.raises(ValueError, match="DeblurGANv2"):
        utils.run_model_chain([(model, dict(patch_size=128, patch_overlap=32))], torch.zeros(4, 4, 3).numpy(), CPU)
    assert utils.get_patch_config("deblurring", "motion", "DeblurGANv2 (Inception)") == dict(patch_size=768, patch_overlap=128)


def test_synthetic_weights_reach_every_used_parameter():
    a, b = deblurganv2.FPNInception().load_synthetic(5), deblurganv2.FPNInception().load_synthetic(5)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    w = sa["fpn.inception.repeat.3.branch0.bn.weight"]
    assert 0.6 <= float(w.min()) and float(w.max()) <= 1.4
    assert torch.equal(sa["fpn.enc3.1.3.branch0.bn.weight"], w)
    fresh = deblurganv2.FPNInception().state_dict()
    changed = [k for k in sa if "running_" not in k and "num_batches" not in k and not torch.equal(sa[k], fresh[k])]
    assert len(changed) == sum(1 for k in sa if "running_" not in k and "num_batches" not in k)


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_two_symbols():
    """include/irm_hip_inception.h is included by irm_hip.h inside its extern "C" block after irm_hip_yuv.h; the table
    _hip.SIGNATURES_INCEPTION is disjoint from the other five; header and table match one to one, the library exports each
    symbol, load() binds it, and each returns IRM_EINVAL for null pointers and zero sizes before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_yuv.h"') < main.index('#include "irm_hip_inception.h"') < main.rindex("#ifdef __cplusplus")
    text = open(os.path.join(ROOT, "include", "irm_hip_inception.h")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_INCEPTION)
    assert not set(_hip.SIGNATURES_INCEPTION) & (set(_hip.SIGNATURES) | set(_hip.SIGNATURES_HALF) | set(_hip.SIGNATURES_FRAMES)
                                                 | set(_hip.SIGNATURES_GRAM) | set(_hip.SIGNATURES_YUV))
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b"}
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_INCEPTION[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """Each class of bad argument on its own, everything else valid (the pointers are never followed: nothing is launched
    without a device, and a launch would return IRM_ELAUNCH, not IRM_EINVAL)."""
    lib = _hip.load()
    good = dict(wp=4096, x=8192, x_bs=3 * 64, y=16384, y_bs=16 * 9, res=0, r_bs=0, bias=0, B=1, Ci=3, Co=16, H=8, W=8,
                kh=3, kw=3, stride=2, pad_h=0, pad_w=0, act1=1, res_mode=0, relu2=0, ct=1, ygroups=1)
    bad = [dict(wp=0), dict(x=0), dict(y=0), dict(B=0), dict(B=70000), dict(Ci=0), dict(Co=-1), dict(H=0), dict(W=-3),
           dict(kh=0), dict(kw=0), dict(stride=0), dict(stride=3), dict(kh=2, kw=2), dict(kh=7, kw=7), dict(kh=1, kw=7, stride=2),
           dict(pad_h=-1), dict(pad_w=3), dict(pad_h=3), dict(act1=2), dict(act1=-1), dict(res_mode=1), dict(res_mode=2, res=64),
           dict(ct=0), dict(ct=3), dict(ct=8), dict(kh=5, kw=5, stride=1, ct=4), dict(H=2), dict(W=2),
           dict(kh=7, kw=1, stride=1, H=6), dict(kh=1, kw=7, stride=1, W=3, pad_w=1)]
    for change in bad:
        a = dict(good, **change)
        assert lib.irm_convkxk_f32(*a.values(), None) == -1, change
    good = dict(x=4096, x_bs=64, y=8192, y_bs=9, B=1, C=1, H=8, W=8, mode=0)
    for change in (dict(x=0), dict(y=0), dict(B=0), dict(C=0), dict(C=70000), dict(B=70000), dict(H=0), dict(W=-1),
                   dict(mode=2), dict(mode=-1), dict(H=2), dict(W=2)):
        a = dict(good, **change)
        assert lib.irm_pool3x3_f32(*a.values(), None) == -1, change


def test_every_inception_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_INCEPTION: each
    symbol is called by name in a test_guard_bands_* function of tests/test_gpu_inception_ops.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_inception_ops.py")) as f:
        text = f.read()
    reached = set()
    for body in re.split(r"^def ", text, flags=re.M):
        if body.startswith("test_guard_bands_"):
            reached |= set(re.findall(r'"(irm_\w+)"', body))
    missing = sorted(set(_hip.SIGNATURES_INCEPTION) - reached)
    assert not missing, f"FPN-Inception entry points without a guard-band case: {missing}"


# --------------------------------------------------------------------------- packing and planning
def test_pack_convkxk_weight_layout():
    w = torch.arange(20 * 5 * 1 * 7, dtype=torch.float32).reshape(20, 5, 1, 7)
    wp = _hip.pack_convkxk_weight(w).view(7, 2, 2, 64)
    for tap, mt, ks, lane in ((0, 0, 0, 0), (3, 1, 0, 3), (6, 0, 1, 17), (2, 1, 1, 5), (5, 1, 0, 63)):
        co, ci = 16 * mt + (lane & 15), 4 * ks + (lane >> 4)
        want = float(w[co, ci, 0, tap]) if co < 20 and ci < 5 else 0.0
        assert float(wp[tap, mt, ks, lane]) == want
    half = _hip.pack_convkxk_weight(w, 0.5)
    assert torch.equal(half, _hip.pack_convkxk_weight(w) * 0.5)


def test_planner_keeps_to_the_built_kernels():
    """ct is one the geometry is built with, never above the number of output tiles, and halves on the small maps of
    the encoder until the grid reaches 256 workgroups or ct is 1; ygroups stays within the passes."""
    for (kh, kw, s), top in ops.CONVKXK_GEOMETRIES.items():
        for co in (16, 20, 80, 192, 384, 1088):
            for (oh, ow) in ((1, 1), (6, 8), (48, 48), (97, 97), (399, 399)):
                for B in (1, 2):
                    ct, yg = ops.plan_convkxk(co, oh, ow, B, kh, kw, s)
                    mt = -(-co // 16)
                    assert ct in (1, 2, 4) and ct <= top and ct <= max(mt, 1)
                    assert 1 <= yg <= -(-mt // ct)
                    blocks = -(-ow // 32) * -(-oh // 8) * B
                    if ct > 1:
                        assert blocks * -(-mt // ct) >= 256
    assert ops.plan_convkxk(160, 48, 48, 1, 1, 7, 1) == (1, 10)           # Block17 on an 800x800 tile: 12 x 10 workgroups
    assert ops.plan_convkxk(32, 399, 399, 1, 3, 3, 2) == (2, 1)           # the stem: 650 pixel tiles
    assert ops.plan_convkxk(64, 13, 17, 1, 5, 5, 1, ct=2, ygroups=1) == (2, 1)
    assert ops.convkxk_out_size(128, 160, 3, 3, 2, (0, 0)) == (63, 79)
    with pytest.raises(ValueError, match="no kernel"):
        ops.convkxk(None, torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), 1, 1, 2, 2)
