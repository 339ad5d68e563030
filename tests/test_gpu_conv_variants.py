"""Every fp32 instantiation behind the dense 3x3-conv entry points, at its edges, against float64.

irm_conv3x3_ep_f32 (csrc/conv3x3.hip), irm_conv3x3_f16x3_ep_f32 (csrc/conv3x3_f16.hip) and irm_conv3x3_thin_f32
(csrc/conv3x3_thin.hip) pick one of 24 kernel instantiations.  tests/variant_model.py lists them (CONV_VARIANTS), restates
the three dispatches and the dealing of the output-channel passes in Python, and holds the cases (CONV_CASES) placed on
each instantiation's edges; this file checks that table and runs every case.

For each case, on the same seeded inputs:
  e    = max|y_gpu - y64|   (y64: F.conv2d + the epilogue in float64 on the CPU)
  e_32 = max|y32 - y64|     (y32: the same in float32 on the CPU)
The exact and the thin kernels pass when e <= K * e_32 + F * max|y64|, the bar of tests/test_gpu_precision.py (cases
with the tanh epilogue: 2e-6 * max(1, max|y64|), the bar of test_conv3x3_thin - device tanhf and host tanh differ by
more than F).  The split kernel passes when e <= 2 * e_exact + 4e-7 * max(1, max|y64|), its own bar
(tests/test_gpu_launch_replay.py), where e_exact is the error of the exact kernel on the same inputs at the planner's
ct, and that exact run must itself pass the K / F bar.  The written slice of the output starts as NaN and the rest of
its buffer as a sentinel: an unwritten element fails, so does a stray write.  Three committed positive controls (one
weight of the last, partial tile of a multi-pass case perturbed by 2^-10 on the ring and on the generic kernel; the lo
halves of a split weight zeroed) must fail the same bars."""
import math

import pytest
import torch
import torch.nn.functional as TF

from block_model import F, K, conv_epilogue
from guards import channel_slice as _slice
from irm_amd import _hip, ops, synth
from variant_model import CONV_CASE_IDS as CASE_IDS
from variant_model import CONV_CASES as CASES
from variant_model import (CONV_VARIANTS, EXACT_CTS, SPLIT_CTS, case_passes, case_plan, case_variant, expected_conv_variant,
                           layout, out_shape, pass_structure, passes_per_group, split, thin_in, thin_out)
from variant_model import conv_generic as generic
from variant_model import conv_ring as ring

SENTINEL = 7.0


# --------------------------------------------------------------------------- CPU tests of the table and the cases
def test_variant_coverage():
    """Each case lands on the variant (and the store path) its path names, and the cases reach all 24 (CPU only: the
    dispatch mirror)."""
    wrong = []
    for cid, c in zip(CASE_IDS, CASES):
        v = case_variant(c)
        ct = c["ct"]
        want = {"ring": lambda: (ring(ct), True), "scalar": lambda: (generic(ct), False),
                "vec": lambda: (generic(ct), True), "split": lambda: (split(ct), True),
                "thin": lambda: ((thin_out(c["co"]) if c["ci"] > 4 else thin_in(c["ci"])), True)}[c["path"]]()
        if v != want:
            wrong.append((cid, want, v))
        if c["kind"] != "thin" and case_plan(c)[0] != ct:
            wrong.append((cid, "ct", case_plan(c)))
    assert not wrong, wrong
    missing = sorted(set(CONV_VARIANTS) - {case_variant(c)[0] for c in CASES})
    assert not missing, missing


def _last_pass(c):
    """(tiles in the last pass, tiles per pass) of a case."""
    mt, ct = (c["co"] + 15) // 16, c["ct"]
    return mt - (-(-mt // ct) - 1) * ct, ct


def test_case_edges():
    """Exact and split: every CT of every kernel has a case in which a workgroup runs two passes or more while the
    groups run unequal pass counts, and (where a pass holds more than one tile) a case whose last pass is ragged and
    whose last tile has Co % 16 != 0; the generic kernel has those on its 16-byte and on its scalar store path."""
    groups = {}
    for c in CASES:
        if c["kind"] != "thin":
            groups.setdefault((c["path"], c["ct"]), []).append(c)
    assert set(groups) == {(p, ct) for p in ("ring", "scalar", "vec") for ct in EXACT_CTS} | {("split", ct) for ct in SPLIT_CTS}
    for (path, ct), cs in groups.items():
        assert any(pass_structure(case_passes(c)) == "uneven" for c in cs), (path, ct, "no uneven multi-pass case")
        assert any(pass_structure(case_passes(c)) == "even" and len(case_passes(c)) == 1 for c in cs), (path, ct)
        assert any(pass_structure(case_passes(c)) == "single" for c in cs), (path, ct)
        assert any(c["co"] % 16 and (ct == 1 or _last_pass(c)[0] < ct) and max(case_passes(c)) > 1 for c in cs), \
            (path, ct, "no ragged last pass with a partial tile")
    for ct in EXACT_CTS:
        assert {case_variant(c)[1] for c in CASES if c["kind"] == "exact" and case_variant(c)[0] == generic(ct)} == {True, False}
    # the clamp of an oversized ygroups
    assert any(c["yg"] == 100 and case_passes(c) == [1] for c in CASES)


def test_expected_conv_variant_spot_checks():
    """A few hand-derived dispatch outcomes (CPU only)."""
    al = dict(x_al=True, y_al=True, r_al=True, wp_al=True)
    dense = dict(x_bs=64 * 64 * 64, y_bs=64 * 64 * 64, r_bs=0)
    assert expected_conv_variant("exact", 64, 64, 64, 4, **dense, **al) == (ring(4), True)
    # a BSD68 image: no 16-byte path at all
    odd = dict(x_bs=64 * 321 * 481, y_bs=64 * 321 * 481, r_bs=0)
    assert expected_conv_variant("exact", 64, 64, 481, 4, **odd, **al) == (generic(4), False)
    # only x off alignment: the generic kernel, but with 16-byte stores
    assert expected_conv_variant("exact", 64, 64, 64, 6, **dense, **dict(al, x_al=False)) == (generic(6), True)
    # a residual with a batch stride that is no multiple of 4 floats: scalar stores
    assert expected_conv_variant("exact", 64, 64, 64, 2, **dict(dense, r_bs=4098), **al) == (generic(2), False)
    assert expected_conv_variant("exact", 64, 64, 64, 5, **dense, **al) is None
    assert expected_conv_variant("exact", 64, 64, 64, 8, **dense, **al) is None
    assert expected_conv_variant("split", 64, 64, 64, 8, **dense, **al) == ("conv3x3_f16x3_kernel<4, 2>", True)
    assert expected_conv_variant("split", 64, 64, 64, 12, **dense, **al) == ("conv3x3_f16x3_kernel<4, 3>", True)
    assert expected_conv_variant("split", 64, 64, 64, 3, **dense, **al) == ("conv3x3_f16x3_kernel<3, 1>", True)
    assert expected_conv_variant("split", 64, 64, 64, 6, **dense, **al) is None
    assert expected_conv_variant("split", 64, 64, 62, 4, **dense, **al) is None
    assert expected_conv_variant("split", 64, 64, 64, 4, **dense, **dict(al, y_al=False)) is None
    assert expected_conv_variant("thin", 96, 3, 64, None, **dense, **al) == (thin_out(3), True)
    assert expected_conv_variant("thin", 3, 48, 64, None, **dense, **al) == (thin_in(3), True)
    assert expected_conv_variant("thin", 2, 2, 64, None, **dense, **al) == (thin_in(2), True)       # both thin: thin_in
    assert expected_conv_variant("thin", 5, 5, 64, None, **dense, **al) is None
    assert expected_conv_variant("thin", 3, 48, 63, None, **dense, **al) is None
    assert passes_per_group(7, 3, 2) == [2, 1] and passes_per_group(7, 3, 100) == [1, 1, 1]
    assert passes_per_group(9, 3, 1) == [3] and passes_per_group(2, 6, 0) == [1]
    assert pass_structure([2, 1]) == "uneven" and pass_structure([3]) == "even" and pass_structure([1, 1]) == "single"


# --------------------------------------------------------------------------- buffers and references
def inputs(c, idx):
    B, ci, co, H, W = c["B"], c["ci"], c["co"], c["H"], c["W"]
    g = f"cv{idx}_{co}_{ci}_{H}x{W}_{B}"
    return dict(x=synth.uniform(37, g + "x", (B, ci, H, W), -1.5, 2.0),
                w=synth.uniform(37, g + "w", (co, ci, 3, 3), -0.2, 0.2),
                bias=synth.uniform(37, g + "b", (co,), -0.5, 0.5),
                r=synth.uniform(37, g + "r", (B, co, H, W), -1.0, 1.0))


def reference(c, t, dt):
    """F.conv2d and the epilogue chain of the kernels (bias, relu1 / leaky, res_mode, relu2, store) in dtype dt."""
    y = TF.conv2d(t["x"].to(dt), t["w"].to(dt), t["bias"].to(dt) if c["bias"] else None, padding=1)
    return conv_epilogue(y, t["r"], c["relu1"], c["res_mode"], c["relu2"], c["store_mode"], c["shuffle"], c["leaky"])


_REFS = {}      # case index -> (y64, e_32, max|y64|): computed once, shared, left unchanged


def refs(c, idx, t):
    if idx not in _REFS:
        y64 = reference(c, t, torch.float64)
        y32 = reference(c, t, torch.float32)
        _REFS[idx] = (y64, float((y32.double() - y64).abs().max()), float(y64.abs().max()))
    return _REFS[idx]


def pack(c, w, dev):
    if c["kind"] == "thin":
        return _hip.pack_conv3x3(w.to(dev))
    if c["kind"] == "split":
        wps, inv = _hip.pack_conv3x3_weight_split(w)
        return wps.to(dev), inv
    return _hip.pack_conv3x3_weight(w).to(dev)


def run_case(c, t, dev, wp=None, planner=False):
    """Launch a case through ops.conv3x3; returns (y slice, whole y allocation, written mask), all on the CPU.
    planner: leave ct and ygroups to ops.plan_conv3x3."""
    B, ci, co, H, W = c["B"], c["ci"], c["co"], c["H"], c["W"]
    lay = layout(c)
    _, xv = _slice(dev, B, ci, 3, 2, H, W, c["x_off"], 0.0)
    xv.copy_(t["x"].to(dev))
    oc, oh, ow = out_shape(c)
    ybuf, yv = _slice(dev, B, oc, 2, 1, oh, ow, c["y_off"], SENTINEL)
    mask = torch.zeros_like(ybuf, dtype=torch.bool)
    mask.as_strided(yv.shape, yv.stride(), yv.storage_offset()).fill_(True)
    yv.fill_(float("nan"))
    res = None
    if c["res_mode"]:
        _, res = _slice(dev, B, co, 3, 1, H, W, c["r_off"], 0.0)
        res.copy_(t["r"].to(dev))
    # the buffers have the layout the dispatch mirror was given
    assert (xv.data_ptr() % 16 == 0) == lay["x_al"] and (yv.data_ptr() % 16 == 0) == lay["y_al"]
    assert xv.stride(0) == lay["x_bs"] and yv.stride(0) == lay["y_bs"]
    assert res is None or ((res.data_ptr() % 16 == 0) == lay["r_al"] and res.stride(0) == lay["r_bs"])
    if wp is None:
        wp = pack(c, t["w"], dev)
    kw = dict(bias=t["bias"].to(dev) if c["bias"] else None, relu1=c["relu1"], res=res, res_mode=c["res_mode"],
              relu2=c["relu2"], store_mode=c["store_mode"], leaky=c["leaky"], shuffle=c["shuffle"])
    if not planner and c["kind"] != "thin":
        kw.update(ct=c["ct"], ygroups=c["yg"])
    timer, ops.TIMER = ops.TIMER, ops.KernelTimer()
    try:
        ops.conv3x3(wp, xv, yv, ci, co, **kw)
        ran = list(ops.TIMER.summary())
    finally:
        ops.TIMER = timer
    want = {"thin": "conv3x3_thin", "split": "conv3x3_f16x3", "exact": "conv3x3"}["exact" if planner else c["kind"]]
    assert ran == [want], (ran, want)                    # the kernel family under test ran, not another one
    return yv.cpu().double(), ybuf.cpu(), mask.cpu()


def exact_bar(c, e32, ymax):
    if c["res_mode"] == 3:
        return 2e-6 * max(1.0, ymax)        # test_conv3x3_thin's bar: device tanhf vs host tanh
    return K * e32 + F * ymax


def split_bar(e_exact, ymax):
    return 2.0 * e_exact + 4e-7 * max(1.0, ymax)


def measure(c, idx, t, dev, wp=None):
    """(e, e_32, max|y64|, bar, e_exact or None) of a case, after the unwritten / stray write checks."""
    got, ybuf, mask = run_case(c, t, dev, wp=wp)
    stray = ybuf[~mask]
    assert torch.all(stray == SENTINEL), f"{int((stray != SENTINEL).sum())} writes outside the output slice"
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} output elements never written"
    y64, e32, ymax = refs(c, idx, t)
    e = float((got - y64).abs().max())
    if c["kind"] != "split":
        return e, e32, ymax, exact_bar(c, e32, ymax), None
    # the yardstick of the split kernel: the exact kernel on the same inputs at the planner's ct, itself held to K / F
    ex, xbuf, xmask = run_case(dict(c, kind="exact"), t, dev, wp=_hip.pack_conv3x3_weight(t["w"]).to(dev), planner=True)
    assert torch.all(xbuf[~xmask] == SENTINEL) and not torch.isnan(ex).any()
    e_exact = float((ex - y64).abs().max())
    assert e_exact <= exact_bar(c, e32, ymax), f"exact kernel above its bar: e {e_exact:.3e} e_32 {e32:.3e}"
    return e, e32, ymax, split_bar(e_exact, ymax), e_exact


_TABLE = {}      # case id -> (e, e_32, bar, e_exact)


@pytest.fixture(scope="module")
def table():
    yield _TABLE
    if _TABLE:
        print(f"\n3x3-conv variants: exact / thin e <= {K} * e_32 + 2^{int(math.log2(F))} * max|y64| (tanh epilogue: 2e-6 "
              "max(1, max|y64|)); split e <= 2 e_exact + 4e-7 max(1, max|y64|)")
        print(f"{'variant':38s} {'case':50s} {'e':>10s} {'e_32':>10s} {'ratio':>7s} {'e_exact':>10s}")
        for cid, (e, e32, bar, ex) in _TABLE.items():
            v, name = cid.split("_|_")
            exs = "" if ex is None else f"{ex:10.3e}"
            print(f"{v:38s} {name[:50]:50s} {e:10.3e} {e32:10.3e} {e / e32 if e32 else float('inf'):7.2f} {exs:>10s}"
                  f"{'' if e <= bar else '  FAIL'}")


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_conv_variant(dev, table, idx):
    c = CASES[idx]
    t = inputs(c, idx)
    e, e32, ymax, bar, e_exact = measure(c, idx, t, dev)
    table[CASE_IDS[idx]] = (e, e32, bar, e_exact)
    print(f"{CASE_IDS[idx]}: e {e:.3e} e_32 {e32:.3e} bar {bar:.3e}" + ("" if e_exact is None else f" e_exact {e_exact:.3e}"))
    assert e <= bar, f"e {e:.3e} above the bar {bar:.3e} (e_32 {e32:.3e}, max|y64| {ymax:.3e}, e_exact {e_exact})"


# --------------------------------------------------------------------------- positive controls
def _find(path, ct, name):
    idx, = [i for i, c in enumerate(CASES) if c["path"] == path and c["ct"] == ct and c["name"] == name]
    return idx


def _perturb_last_tile(c, t):
    """Packed exact weight with one weight of the last, partial output tile scaled by 1 + 2^-10: the largest |w| of
    output row Co - 2, in Wp[tap][mtile][kstep][lane], lane = (k % 4) * 16 + m % 16.  The reference keeps the true one."""
    co, ci = c["co"], c["ci"]
    mt, ks = (co + 15) // 16, 2 * ((ci + 7) // 8)
    m = co - 2
    assert m // 16 == mt - 1 and passes_per_group(mt, c["ct"], c["yg"]) == [2, 1]      # the tail of group 0's 2nd pass
    k, tap = divmod(int(t["w"][m].reshape(ci, 9).abs().argmax()), 9)
    wp = _hip.pack_conv3x3_weight(t["w"]).clone()
    v = wp.view(9, mt, ks, 64)
    lane = (k % 4) * 16 + m % 16
    assert v[tap, m // 16, k // 4, lane] == t["w"][m, k, tap // 3, tap % 3]
    v[tap, m // 16, k // 4, lane] *= 1.0 + 2.0 ** -10
    return wp


def _control_exact(dev, path):
    idx = _find(path, 3, "A uneven-groups ragged-last-pass relu res1 relu2")
    c = CASES[idx]
    t = inputs(c, idx)
    e, e32, ymax, bar, _ = measure(c, idx, t, dev, wp=_perturb_last_tile(c, t).to(dev))
    print(f"control {CASE_IDS[idx]}: e {e:.3e} e_32 {e32:.3e} bar {bar:.3e}")
    return e <= bar


@pytest.mark.gpu
def test_positive_control_ring_last_tile_weight(dev):
    """Case A at CT 3 on the ring with one weight of the last tile (the one-tile second pass of group 0) off by 2^-10
    relative, in the packed tensor only, must fail the bar."""
    assert not _control_exact(dev, "ring")


@pytest.mark.gpu
def test_positive_control_generic_last_tile_weight(dev):
    """The same perturbation on the generic kernel (scalar stores, W = 35) must fail the bar."""
    assert not _control_exact(dev, "scalar")


@pytest.mark.gpu
def test_positive_control_split_lo_zeroed(dev):
    """A split case whose packed weight [mtile][S][tap][hi | lo][64][8] has its fp16 lo halves zeroed must fail the
    split kernel's bar."""
    idx = _find("split", 3, "A uneven-groups ragged-last-pass relu res1 relu2")
    c = CASES[idx]
    t = inputs(c, idx)
    wps, inv = _hip.pack_conv3x3_weight_split(t["w"])
    wps = wps.clone()
    mt, st = (c["co"] + 15) // 16, (c["ci"] + 31) // 32
    h = wps.view(torch.float16).view(mt, st, 9, 2, 64 * 8)
    assert h[:, :, :, 1].abs().max() > 0
    h[:, :, :, 1] = 0
    e, e32, ymax, bar, e_exact = measure(c, idx, t, dev, wp=(wps.to(dev), inv))
    print(f"control {CASE_IDS[idx]}: e {e:.3e} e_32 {e32:.3e} e_exact {e_exact:.3e} bar {bar:.3e}")
    assert not e <= bar
