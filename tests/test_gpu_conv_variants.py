"""Every fp32 instantiation behind the dense 3x3-conv entry points, at its edges, against float64.

irm_conv3x3_ep_f32 (csrc/conv3x3.hip), irm_conv3x3_f16x3_ep_f32 (csrc/conv3x3_f16.hip) and irm_conv3x3_thin_f32
(csrc/conv3x3_thin.hip) pick one of 24 kernel instantiations.  CONV_VARIANTS lists them, expected_conv_variant() restates
the three dispatches in Python, passes_per_group() restates how the output-channel passes are dealt to the workgroup
groups, and CASES places cases on each instantiation's edges: several passes in one workgroup, groups with unequal pass
counts, a ragged last pass, a last tile with Co % 16 != 0, a half-full last input stage, partial row and column tiles,
channel slices of larger buffers, the scalar and the 16-byte store path of the generic kernel, and every epilogue.  The
launch planner shrinks ct on images this small, so every case passes ct and ygroups explicitly (ops.plan_conv3x3 keeps
explicit values).

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

from irm_amd import _hip, ops, synth
from test_gpu_precision import F, K

SENTINEL = 7.0
EXACT_CTS = (1, 2, 3, 4, 6)             # the two ct switches of irm_conv3x3_ep_f32 (conv3x3.hip)
SPLIT_CTS = (1, 2, 3, 4, 8, 12)         # output tiles per pass: the ct switch of irm_conv3x3_f16x3_ep_f32


# --------------------------------------------------------------------------- the variant table and its dispatch mirror
def ring(ct):
    return f"conv3x3_ring_kernel<{ct}, 3>"              # launch_conv_ring (conv3x3.hip): NS = 3


def generic(ct):
    return f"conv3x3_kernel<{ct}>"


def split(ct):
    """ct 1 ... 4: one weight chunk of ct tiles; 8 / 12: 2 / 3 chunks of 4 (the ct switch of irm_conv3x3_f16x3_ep_f32)."""
    return f"conv3x3_f16x3_kernel<{min(ct, 4)}, {max(1, ct // 4)}>"


def thin_in(ci):
    return f"conv3x3_thin_in_kernel<{ci}, 2>"


def thin_out(co):
    return f"conv3x3_thin_out_kernel<{co}, 4>"


CONV_VARIANTS = sorted([ring(ct) for ct in EXACT_CTS] + [generic(ct) for ct in EXACT_CTS]
                       + [split(ct) for ct in SPLIT_CTS]
                       + [thin_in(c) for c in (1, 2, 3, 4)] + [thin_out(c) for c in (1, 2, 3, 4)])
assert len(CONV_VARIANTS) == len(set(CONV_VARIANTS)) == 24


def expected_conv_variant(kind, ci, co, W, ct, x_bs, y_bs, r_bs, x_al, y_al, r_al, wp_al):
    """(instantiation, vec) the entry point of `kind` ("exact", "split", "thin") launches, None = IRM_EINVAL.  *_bs:
    batch strides in floats (0 without a residual), *_al: the pointer is 16-byte aligned (a null residual is).  vec is
    ConvArgs.vec, the 16-byte store path of the generic kernel; the split and the thin kernels always store 16 bytes."""
    all_vec = W % 4 == 0 and x_bs % 4 == 0 and y_bs % 4 == 0 and r_bs % 4 == 0 and x_al and y_al and r_al
    if kind == "exact":                                             # irm_conv3x3_ep_f32 (conv3x3.hip)
        if ct not in EXACT_CTS:
            return None
        vec = W % 4 == 0 and y_bs % 4 == 0 and r_bs % 4 == 0 and y_al and r_al      # a.vec
        fast = vec and x_bs % 4 == 0 and x_al and wp_al                             # fast
        return (ring(ct) if fast else generic(ct)), vec
    if kind == "split":                                             # irm_conv3x3_f16x3_ep_f32: alignment, ct switch
        if not (all_vec and wp_al) or ct not in SPLIT_CTS:
            return None
        return split(ct), True
    if kind == "thin":                                              # irm_conv3x3_thin_f32: checks, Co / Ci dispatch
        if not all_vec or (co > 4 and ci > 4):
            return None
        return (thin_out(co) if co <= 4 and ci > 4 else thin_in(ci)), True
    raise ValueError(kind)


def passes_per_group(mtiles, ct, ygroups):
    """Output-channel passes each workgroup group runs: ygroups is clamped to [1, nchunks] (irm_conv_common,
    conv_epilogue.h) and group y takes passes y, y + ygroups, ... (my_chunks in conv3x3_ring_kernel)."""
    nchunks = -(-mtiles // ct)
    yg = min(max(ygroups, 1), nchunks)
    return [(nchunks - y + yg - 1) // yg for y in range(yg)]


def pass_structure(passes):
    """"single": no workgroup runs a second pass; else "even" or "uneven" pass counts over the groups."""
    return "single" if max(passes) == 1 else "even" if min(passes) == max(passes) else "uneven"


# --------------------------------------------------------------------------- cases
def _case(kind, path, name, co, ci, H, W, *, B=2, ct=None, yg=None, bias=False, relu1=False, res_mode=0, relu2=False,
          store_mode=0, shuffle=2, leaky=None, x_off=0, y_off=0, r_off=0):
    """One launch.  path: "ring" / "scalar" / "vec" (exact), "split", "thin"; *_off: floats the buffer starts past a
    16-byte boundary."""
    return dict(kind=kind, path=path, name=name, co=co, ci=ci, H=H, W=W, B=B, ct=ct, yg=yg, bias=bias, relu1=relu1,
                res_mode=res_mode, relu2=relu2, store_mode=store_mode, shuffle=shuffle, leaky=leaky, x_off=x_off,
                y_off=y_off, r_off=r_off)


def _exact_cases(ct, path):
    """Cases A - D of one exact CT on one path: the ring (all aligned, W = 36), the generic kernel with scalar stores
    (W = 35; once W = 36 with every buffer one float past alignment) or with 16-byte stores (W = 36, only x one float
    past alignment).  The PixelUnshuffle case takes W = 40 instead of 36 (its output planes, 5 x 18 floats at W = 36,
    would put the output slice off 16-byte alignment and the launch on the scalar path) and W = 38 on the scalar path."""
    W = 35 if path == "scalar" else 36
    off = dict(x_off=1) if path == "vec" else {}
    kw = dict(ct=ct, **off)
    cases = [
        _case("exact", path, "A uneven-groups ragged-last-pass relu res1 relu2", 16 * (2 * ct + 1) - 1, 20, 9, W, yg=2,
              bias=True, relu1=True, res_mode=1, relu2=True, **kw),
        _case("exact", path, "B one-pass m%16=1 res2", 16 * (ct - 1) + 1, 5, 5, W, yg=1, res_mode=2, **kw),
        _case("exact", path, "C three-passes one-stage shuffle2", 48 * ct, 3, 5, W, yg=1, store_mode=2, shuffle=2, **kw),
        _case("exact", path, "C three-passes one-stage shuffle4", 48 * ct, 3, 5, W, yg=1, store_mode=2, shuffle=4, **kw),
        _case("exact", path, "D two-passes ragged unshuffle", 16 * ct + 8, 12, 10, 38 if path == "scalar" else 40, yg=1,
              store_mode=1, **kw),
    ]
    if path == "scalar":
        cases.append(_case("exact", path, "A all-buffers-offset", 16 * (2 * ct + 1) - 1, 20, 9, 36, yg=2, bias=True,
                           relu1=True, res_mode=1, relu2=True, ct=ct, x_off=1, y_off=1, r_off=1))
    if ct == 3:
        cases.append(_case("exact", path, "B ygroups-100-clamped", 16 * (ct - 1) + 1, 5, 5, W, yg=100, res_mode=2, **kw))
    return cases


def _exact_epilogue_cases(path):
    """Once per path: the tanh + clamp residual (res_mode 3) and LeakyReLU."""
    W = 35 if path == "scalar" else 36
    off = dict(x_off=1) if path == "vec" else {}
    return [
        _case("exact", path, "E tanh-clamp two-groups", 40, 9, 9, W, ct=2, yg=2, bias=True, res_mode=3, **off),
        _case("exact", path, "F leaky two-passes", 50, 9, 9, W, ct=3, yg=1, bias=True, leaky=0.1, **off),
    ]


def _split_cases(ct):
    """A, C, D with CT = the output tiles per pass, W = 36 and aligned slices (the kernel accepts nothing else), and B
    for the single-pass launch production issues most."""
    return [
        _case("split", "split", "A uneven-groups ragged-last-pass relu res1 relu2", 16 * (2 * ct + 1) - 1, 40, 9, 36,
              ct=ct, yg=2, bias=True, relu1=True, res_mode=1, relu2=True),
        _case("split", "split", "B one-pass m%16=1 res2", 16 * (ct - 1) + 1, 5, 5, 36, ct=ct, yg=1, res_mode=2),
        _case("split", "split", "C three-passes one-stage shuffle2", 48 * ct, 3, 5, 36, ct=ct, yg=1, store_mode=2),
        _case("split", "split", "C three-passes one-stage shuffle4", 48 * ct, 3, 5, 36, ct=ct, yg=1, store_mode=2,
              shuffle=4),
        _case("split", "split", "D two-passes ragged unshuffle", 16 * ct + 8, 70, 10, 40, ct=ct, yg=1, store_mode=1),
    ]


def _thin_cases():
    cases = [
        _case("thin", "thin", "ragged co group 13+13+13+11", 50, 3, 9, 12, B=1, bias=True, relu1=True),
        _case("thin", "thin", "ragged co group 10+9 B3", 19, 2, 5, 8, B=3, res_mode=1, relu2=True),
        _case("thin", "thin", "gray first layer odd H", 17, 1, 7, 8, bias=True, relu1=True),
        _case("thin", "thin", "ci4 ragged co group 9+9+9+6", 33, 4, 9, 12, B=1, bias=True, res_mode=2),
    ]
    for co in (1, 2, 3, 4):     # H = 6: the second 4-row strip holds 2 rows; Ci = 9: the four waves sum 3, 2, 2, 2 channels
        cases.append(_case("thin", "thin", f"co{co} partial strip", co, 9, 6, 12, bias=co % 2 == 1,
                           res_mode=(0, 1, 2, 3)[co - 1], relu1=co == 2, relu2=co == 4))
    return cases


CASES = []
for _ct in EXACT_CTS:
    for _path in ("ring", "scalar", "vec"):
        CASES += _exact_cases(_ct, _path)
for _path in ("ring", "scalar", "vec"):
    CASES += _exact_epilogue_cases(_path)
for _ct in SPLIT_CTS:
    CASES += _split_cases(_ct)
CASES += _thin_cases()


# --------------------------------------------------------------------------- layouts
def out_shape(c):
    """(channels, H, W) of the output tensor."""
    co, H, W, r = c["co"], c["H"], c["W"], c["shuffle"]
    if c["store_mode"] == 1:
        return co * 4, H // 2, W // 2
    if c["store_mode"] == 2:
        return co // (r * r), H * r, W * r
    return co, H, W


def layout(c):
    """Batch strides (floats) and 16-byte alignment of x, y, res of a case: x is channels [2, 2 + Ci) of a Ci + 3
    channel buffer, y channels [1, 1 + C_out) of C_out + 2, res channels [1, 1 + Co) of Co + 3 (allocations are 16-byte
    aligned; *_off floats are skipped in front)."""
    N = c["H"] * c["W"]
    oc, oh, ow = out_shape(c)
    lay = dict(x_bs=(c["ci"] + 3) * N, x_al=(c["x_off"] + 2 * N) % 4 == 0,
               y_bs=(oc + 2) * oh * ow, y_al=(c["y_off"] + oh * ow) % 4 == 0, r_bs=0, r_al=True)
    if c["res_mode"]:
        lay.update(r_bs=(c["co"] + 3) * N, r_al=(c["r_off"] + N) % 4 == 0)
    return lay


def case_plan(c):
    """(ct, ygroups) the launch gets from ops.conv3x3 (the thin kernel has no plan)."""
    if c["kind"] == "thin":
        return None, None
    return ops.plan_conv3x3(c["co"], c["H"], c["W"], c["B"], split=c["kind"] == "split", ct=c["ct"], ygroups=c["yg"])


def case_variant(c):
    ct, _ = case_plan(c)
    return expected_conv_variant(c["kind"], c["ci"], c["co"], c["W"], ct, wp_al=True, **layout(c))


def case_passes(c):
    ct, yg = case_plan(c)
    return passes_per_group((c["co"] + 15) // 16, ct, yg)


def _variant_name(c):
    v = case_variant(c)
    if v is None:
        return "rejected"
    return v[0] + (" vec" if c["path"] == "vec" else " scalar" if c["path"] == "scalar" else "")


CASE_IDS = [f"{_variant_name(c)} | {c['name']}".replace(" ", "_") for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)

#: variant -> the pass structures ("single" / "even" / "uneven") its cases run; tests/test_planner_cpu.py and
#: tests/test_gpu_launch_replay.py hold the planner's and production's launches against it
CASE_STRUCTURES = {}
for _c in CASES:
    _v = case_variant(_c)
    if _v is not None:
        CASE_STRUCTURES.setdefault(_v[0], set()).add("single" if _c["kind"] == "thin" else pass_structure(case_passes(_c)))


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
def _slice(dev, B, C, extra, ch, H, W, off, fill):
    """A [B, C, H, W] channel slice at channel `ch` of a [B, C + extra, H, W] buffer that starts `off` floats into its
    allocation.  Returns (flat allocation, view)."""
    N = H * W
    flat = torch.full((B * (C + extra) * N + 4,), fill, dtype=torch.float32, device=dev)
    view = flat.as_strided((B, C, H, W), ((C + extra) * N, N, W, 1), off + ch * N)
    return flat, view


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
    if c["relu1"]:
        y = torch.relu(y)
    if c["leaky"] is not None:
        y = torch.where(y > 0, y, y * torch.tensor(c["leaky"], dtype=torch.float32).to(dt))
    if c["res_mode"]:
        r = t["r"].to(dt)
        y = y + r if c["res_mode"] == 1 else r - y if c["res_mode"] == 2 else (torch.tanh(y) + r).clamp(-1, 1)
    if c["relu2"]:
        y = torch.relu(y)
    if c["store_mode"] == 1:
        y = TF.pixel_unshuffle(y, 2)
    elif c["store_mode"] == 2:
        y = TF.pixel_shuffle(y, c["shuffle"])
    return y


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
