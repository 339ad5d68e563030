"""Every kernel instantiation behind the two 1x1-GEMM entry points, at its edges, against float64.

irm_gemm1x1_f32 and irm_gemm1x1_f16x3_f32 both go through gemm_entry (csrc/gemm_pw.hip), which picks one of 78
instantiations of gemm_ring_kernel, gemm_pw_kernel and gemm_xres_kernel.  tests/variant_model.py lists them (VARIANTS)
and restates the dispatch in Python (expected_variant); CASES places cases on each variant's edges: M tails, a partly
filled last pass, M <= 48, uneven ygroups, K tails, N not a multiple of 256, channel slices of larger buffers, and every
option the variant accepts.

For each case, on the same seeded inputs:
  e    = max|y_gpu - y64|   (y64: the same op in float64 on the CPU)
  e_32 = max|y32 - y64|     (y32: the same op in float32 on the CPU)
and the case passes when e <= K * e_32 + F * max|y64|, the ledger's bar (block_model.passes).  The written slice of
the output starts as NaN and the rest of its buffer as a sentinel: an unwritten element fails, so does a stray write.
Two committed positive controls (lo halves of the split weight zeroed; one weight of the last, partial output tile
perturbed by 2^-10) must fail the same bar."""
import math

import pytest
import torch

import block_model as bm
from block_model import F, K, passes
from guards import channel_slice as _slice
from irm_amd import _hip, ops, synth
from variant_model import CTS, LN_NONE, LN_WB, VARIANTS, expected_variant, res_depths, xres
from variant_model import gemm_generic as generic
from variant_model import gemm_ring as ring

SENTINEL = 7.0


# --------------------------------------------------------------------------- cases
def _case(variant, name, M, K, H, W, B, *, ct, yg=None, ln=0, res=None, scale=False, bias=False, act=0,
          stats_out=False, w_bs=False, misalign=False):
    """One launch: res None / "sep" (a channel slice of another buffer) / "inplace" (res is y); misalign: x, y start
    one float past a 16-byte boundary.  Split (irm_gemm1x1_f16x3_f32) for the F16 ring and the xres variants."""
    split = variant.startswith("gemm_xres") or (variant.startswith("gemm_ring") and variant.endswith("true>"))
    return dict(variant=variant, name=name, M=M, K=K, H=H, W=W, B=B, ct=ct, yg=yg, ln=ln, res=res, scale=scale,
                bias=bias, act=act, stats_out=stats_out, w_bs=w_bs, misalign=misalign, split=split)


def _ring_res_cases(ct, ns, f16):
    v = ring(2, ct, ns, LN_NONE, True, f16)
    # NS 4 where NS 3 exists: K > 512
    k_lo, k_hi = (530, 601) if ns == 4 and 3 in res_depths(ct, f16) else (37, 90)
    return [
        _case(v, "m%16=1 partial-last-pass inplace scale", 16 * ct + 1, k_lo, 12, 20, 2, ct=ct, yg=1, res="inplace",
              scale=True, bias=True),
        _case(v, "m%16=15 yg2-uneven sep act2", 16 * (2 * ct + 1) - 1, k_hi, 9, 28, 2, ct=ct, yg=2, res="sep", act=2),
        _case(v, "M16 one-tile stats scale", 16, k_lo, 10, 36, 2, ct=ct, res="sep", scale=True, stats_out=True),
        _case(v, "M31 two-tile inplace stats bias", 31, k_hi, 8, 44, 2, ct=ct, res="inplace", bias=True,
              stats_out=True, act=1),
        _case(v, "M44 three-tile inplace scale stats act3", 44, k_lo, 7, 52, 3, ct=ct, res="inplace", scale=True,
              stats_out=True, act=3, bias=True),
        _case(v, "M48 per-batch-w sep", 48, k_hi, 12, 12, 3, ct=ct, res="sep", w_bs=True, scale=True),
    ]


def _ring_plain_cases(pt, ct, ln, f16):
    """No residual.  PT 4 on the exact path needs B * ceil(N / 256) * ygroups >= 512 (gemm_pw.hip:668)."""
    v = ring(pt, ct, 3 if pt == 4 else 4, ln, False, f16)
    # LN on the split path: keep off the input-resident kernel (K 48 = 3 stages, K > 192, stats_out or per-batch weights)
    k_a, k_b = (48, 200) if (f16 and ln) else (37, 90)
    big = pt == 4 and not f16
    cases = []
    # M % 16 == 1, last pass holds one tile; two groups
    m = 16 * ct + 1
    cases.append(_case(v, "m%16=1 partial-last-pass yg2", m, k_a, *((130, 252, 2) if big else (12, 20, 2)), ct=ct, yg=2,
                       ln=ln, bias=True, act=2))
    # M % 16 == 15, three passes over two groups (2 + 1)
    m = 16 * (2 * ct + 1) - 1
    cases.append(_case(v, "m%16=15 yg2-uneven", m, k_b, *((130, 252, 2) if big else (9, 28, 2)), ct=ct, yg=2, ln=ln,
                       act=1))
    # M <= 48: 1, 2, 3 tiles in the only pass
    cases.append(_case(v, "M16 one-tile stats", 16, k_a, *((256, 256, 2) if big else (10, 36, 2)), ct=ct, ln=ln,
                       stats_out=True, act=3))
    cases.append(_case(v, "M31 two-tile per-batch-w", 31, k_b, *((128, 256, 4) if big else (8, 44, 3)), ct=ct, ln=ln,
                       w_bs=True, bias=True))
    cases.append(_case(v, "M44 three-tile stats bias", 44, k_a, *((252, 260, 2) if big else (7, 52, 2)), ct=ct, ln=ln,
                       stats_out=True, bias=True))
    # many passes, four groups taking 2, 2, 1, 1 (strided assignment), N % 256 != 0
    m = 16 * 6 * ct - 5
    cases.append(_case(v, "6-pass yg4-uneven", m, k_a, *((100, 164, 2) if big else (6, 20, 1)), ct=ct, yg=4, ln=ln,
                       bias=True))
    return cases


def _generic_cases(ct, vec):
    v = generic(ct, vec)
    if vec:
        # the generic kernel's aligned path: a residual together with a LayerNorm prologue (gemm_pw.hip:665)
        return [
            _case(v, "m%16=1 res+ln1 yg2", 16 * ct + 1, 37, 12, 20, 2, ct=ct, yg=2, ln=1, res="sep", scale=True,
                  bias=True),
            _case(v, "m%16=15 res+ln2 inplace yg2-uneven", 16 * (2 * ct + 1) - 1, 90, 9, 28, 2, ct=ct, yg=2, ln=2,
                  res="inplace", act=2),
            _case(v, "M16 res+ln1 stats", 16, 40, 10, 36, 2, ct=ct, ln=1, res="sep", stats_out=True),
            _case(v, "M44 res+ln2 stats per-batch-w act3", 44, 51, 7, 52, 3, ct=ct, ln=2, res="inplace",
                  stats_out=True, act=3, w_bs=True, scale=True),
        ]
    return [
        _case(v, "m%16=1 N%4=3 yg2", 16 * ct + 1, 37, 5, 7, 2, ct=ct, yg=2, ln=1, bias=True, act=2),
        _case(v, "m%16=15 N%4=2 res yg2-uneven", 16 * (2 * ct + 1) - 1, 90, 9, 30, 2, ct=ct, yg=2, res="sep",
              scale=True, act=1),
        _case(v, "M16 misaligned stats", 16, 40, 10, 36, 2, ct=ct, ln=2, stats_out=True, misalign=True),
        _case(v, "M31 N%4=1 inplace stats", 31, 25, 3, 11, 3, ct=ct, res="inplace", stats_out=True, bias=True),
        _case(v, "M44 misaligned res per-batch-w act3", 44, 51, 7, 52, 2, ct=ct, res="sep", act=3, w_bs=True,
              misalign=True),
    ]


def _xres_cases(kt, ct):
    v = xres(kt, ct)
    ks = {2: (20, 32), 4: (50, 64), 6: (90, 96), 12: (180, 192)}[kt]       # a K inside the stage count, and a full one
    if ct == 9:
        ms = (137, 144, 288) if kt != 12 else (575, 1152, 1146)            # mtiles 9 / 18 / 36 / 72
    else:
        ms = (145, 44, 31) if kt != 12 else (513, 1009, 767)
    return [
        _case(v, f"M{ms[0]} ln1 bias act2", ms[0], ks[0], 12, 20, 2, ct=ct, ln=1, bias=True, act=2),
        _case(v, f"M{ms[1]} ln2 act1", ms[1], ks[1], 9, 28, 2, ct=ct, ln=2, act=1),
        _case(v, f"M{ms[2]} ln1 act3 N%256", ms[2], ks[0], 6, 100, 3, ct=ct, ln=1, act=3, bias=True),
    ] + ([_case(v, "M16 one-tile ln2", 16, ks[1], 10, 36, 2, ct=ct, ln=2, bias=True)] if ct == 8 and kt != 12 else [])


CASES = []
for _ct in CTS:
    for _f16 in (False, True):
        for _ns in res_depths(_ct, _f16):
            CASES += _ring_res_cases(_ct, _ns, _f16)
    for _ln in (0, 1, 2):
        CASES += _ring_plain_cases(2, _ct, _ln, False) + _ring_plain_cases(4, _ct, _ln, False)
        CASES += _ring_plain_cases(4, _ct, _ln, True)
    CASES += _generic_cases(_ct, False) + _generic_cases(_ct, True)
for _kt in (2, 4, 6, 12):
    for _ct in (8, 9):
        CASES += _xres_cases(_kt, _ct)
CASE_IDS = [f"{c['variant']} | {c['name']}".replace(" ", "_") for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


# --------------------------------------------------------------------------- buffers and references
def _plan(c):
    """(ct, ygroups) the launch gets from ops.gemm1x1."""
    return ops.plan_gemm1x1(c["M"], c["K"], c["H"] * c["W"], c["B"], split=c["split"], res=c["res"] is not None,
                            stats_out=c["stats_out"], ct=c["ct"], ygroups=c["yg"])


def _vec(c):
    N = c["H"] * c["W"]
    # every batch stride below is (channels + 3) * N or (channels + 2) * N
    return N % 4 == 0 and not c["misalign"]


def case_variant(c):
    ct, yg = _plan(c)
    return expected_variant(split=c["split"], M=c["M"], K=c["K"], N=c["H"] * c["W"], B=c["B"], ct=ct, ygroups=yg,
                            ln=c["ln"], res=c["res"] is not None, stats_out=c["stats_out"], w_bs=c["w_bs"], vec=_vec(c))


def reference(c, t, dt):
    """y (and its LayerNorm statistics) of a case in dtype dt on the CPU."""
    B, M, Kc, H, W = c["B"], c["M"], c["K"], c["H"], c["W"]
    x = bm.layer_norm(t["x"].to(dt), t["lnw"], t["lnb"], c["ln"])
    w = t["w"].to(dt)
    y = torch.einsum("bmk,bkhw->bmhw", w, x) if w.dim() == 3 else torch.einsum("mk,bkhw->bmhw", w, x)
    if c["bias"]:
        y = y + t["bias"].to(dt).view(1, M, 1, 1)
    y = bm.act(y, c["act"])
    if c["res"] is not None:
        r = t["r"].to(dt)
        y = y + (r * t["scale"].to(dt).view(1, M, 1, 1) if c["scale"] else r)
    return y, (bm.ln_stats(y) if c["stats_out"] else None)


def inputs(c, idx):
    B, M, Kc, H, W = c["B"], c["M"], c["K"], c["H"], c["W"]
    g = f"gv{idx}_{M}_{Kc}_{H}x{W}_{B}"
    t = dict(x=synth.uniform(31, g + "x", (B, Kc, H, W), -1.5, 2.0),
             w=synth.uniform(31, g + "w", ((B, M, Kc) if c["w_bs"] else (M, Kc)), -0.3, 0.3),
             lnw=synth.uniform(31, g + "lw", (Kc,), 0.5, 1.5), lnb=synth.uniform(31, g + "lb", (Kc,), -0.2, 0.2),
             bias=synth.uniform(31, g + "b", (M,), -0.3, 0.3), r=synth.uniform(31, g + "r", (B, M, H, W), -2.0, 2.0),
             scale=synth.uniform(31, g + "s", (M,), 0.5, 1.5))
    return t


def pack(c, w):
    pk = _hip.pack_gemm_weight_split if c["split"] else _hip.pack_gemm_weight
    if w.dim() == 3:
        return torch.stack([pk(w[b]) for b in range(w.shape[0])])
    return pk(w)


def run_case(c, t, dev, wp=None):
    """Launch a case through ops.gemm1x1; returns (y slice, whole y buffer, written mask, stats_out or None)."""
    B, M, Kc, H, W = c["B"], c["M"], c["K"], c["H"], c["W"]
    N = H * W
    mis = int(c["misalign"])          # x, y, res start one float past a 16-byte boundary
    _, xv = _slice(dev, B, Kc, 3, 2, H, W, mis, 0.0)
    xv.copy_(t["x"].to(dev))
    ybuf, yv = _slice(dev, B, M, 2, 1, H, W, mis, SENTINEL)
    mask = torch.zeros_like(ybuf, dtype=torch.bool)
    mask.as_strided(yv.shape, yv.stride(), yv.storage_offset()).fill_(True)
    yv.fill_(float("nan"))
    res = None
    if c["res"] == "inplace":
        yv.copy_(t["r"].to(dev))
        res = yv
    elif c["res"] == "sep":
        _, res = _slice(dev, B, M, 3, 1, H, W, mis, 0.0)
        res.copy_(t["r"].to(dev))
    stats = None
    if c["ln"]:
        stats = torch.empty(B, 2, N, device=dev)
        ops.ln_stats(xv, stats)
    st_out = torch.full((B, 2, N), float("nan"), device=dev) if c["stats_out"] else None
    if wp is None:
        wp = pack(c, t["w"])
    wp = wp.to(dev)
    ops.gemm1x1(wp, xv, yv, M, Kc, res=res, bias=t["bias"].to(dev) if c["bias"] else None, stats=stats,
                lnw=t["lnw"].to(dev) if c["ln"] else None, lnb=t["lnb"].to(dev) if c["ln"] == LN_WB else None,
                ln_mode=c["ln"], act=c["act"], w_bs=wp.shape[1] if wp.dim() == 2 else 0, ct=c["ct"], ygroups=c["yg"],
                stats_out=st_out, res_scale=t["scale"].to(dev) if c["scale"] else None, split=c["split"])
    torch.cuda.synchronize()
    return yv.cpu().double(), ybuf.cpu(), mask.cpu(), (None if st_out is None else st_out.cpu().double())


def measure(c, t, got, stats_got):
    """[(row, e, e_32, max|y64|)] of a case: the output, and with stats_out its mean and rstd."""
    y64, s64 = reference(c, t, torch.float64)
    y32, s32 = reference(c, t, torch.float32)
    rows = [("y", float((got - y64).abs().max()), float((y32.double() - y64).abs().max()), float(y64.abs().max()))]
    if s64 is not None:
        for i, nm in enumerate(("mean", "rstd")):
            ref = s64[i].reshape(c["B"], -1)
            rows.append((nm, float((stats_got[:, i] - ref).abs().max()),
                         float((s32[i].reshape(c["B"], -1).double() - ref).abs().max()), float(ref.abs().max())))
    return rows


_TABLE = {}      # case id -> rows


@pytest.fixture(scope="module")
def table():
    yield _TABLE
    if _TABLE:
        print(f"\n1x1-GEMM variants: e <= {K} * e_32 + 2^{int(math.log2(F))} * max|y64|")
        print(f"{'variant':52s} {'case':40s} {'row':4s} {'e':>10s} {'e_32':>10s} {'ratio':>7s}")
        for cid, rows in _TABLE.items():
            v, name = cid.split("_|_")
            for row, e, e32, ymax in rows:
                print(f"{v:52s} {name[:40]:40s} {row:4s} {e:10.3e} {e32:10.3e} {e / e32 if e32 else float('inf'):7.2f}"
                      f"{'' if passes(e, e32, ymax) else '  FAIL'}")


def test_variant_coverage():
    """The cases reach every entry of VARIANTS, and each lands on the variant its row names (CPU only: the dispatch
    mirror; on hardware the kernel names in a kernel trace of this file are exactly VARIANTS)."""
    wrong = [(cid, c["variant"], case_variant(c)) for cid, c in zip(CASE_IDS, CASES) if case_variant(c) != c["variant"]]
    assert not wrong, wrong
    missing = sorted(set(VARIANTS) - {c["variant"] for c in CASES})
    assert not missing, missing


def test_expected_variant_spot_checks():
    """A few hand-derived dispatch outcomes (also CPU only)."""
    kw = dict(B=1, ygroups=1, res=False, stats_out=False, w_bs=False, vec=True)
    assert expected_variant(split=True, M=144, K=96, N=1024, ct=9, ln=1, **kw) == xres(6, 9)
    assert expected_variant(split=True, M=144, K=48, N=1024, ct=9, ln=1, **kw) == ring(4, 9, 3, 1, False, True)
    assert expected_variant(split=True, M=144, K=180, N=1024, ct=9, ln=2, **kw) == ring(4, 9, 3, 2, False, True)
    assert expected_variant(split=True, M=576, K=180, N=1024, ct=9, ln=2, **kw) == xres(12, 9)
    assert expected_variant(split=False, M=48, K=96, N=1024, ct=3, ln=0, **kw) == ring(2, 3, 4, 0, False, False)
    assert expected_variant(split=False, M=48, K=96, N=65536, ct=3, ln=0, **dict(kw, B=2)) == ring(4, 3, 3, 0, False, False)
    assert expected_variant(split=False, M=48, K=600, N=1024, ct=3, ln=0, **dict(kw, res=True)) == ring(2, 3, 4, 0, True, False)
    assert expected_variant(split=False, M=48, K=96, N=1023, ct=3, ln=0, **dict(kw, vec=False)) == generic(3, False)
    assert expected_variant(split=True, M=48, K=96, N=1024, ct=3, ln=1, **dict(kw, res=True)) is None
    assert expected_variant(split=False, M=160, K=96, N=1024, ct=9, ln=0, **dict(kw, stats_out=True)) is None


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_gemm_variant(dev, table, idx):
    c = CASES[idx]
    t = inputs(c, idx)
    got, ybuf, mask, st = run_case(c, t, dev)
    stray = ybuf[~mask]
    assert torch.all(stray == SENTINEL), f"{int((stray != SENTINEL).sum())} writes outside the output slice"
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} output elements never written"
    if st is not None:
        assert not torch.isnan(st).any(), "stats_out not fully written"
    rows = measure(c, t, got, st)
    table[CASE_IDS[idx]] = rows
    bad = [(row, e, e32) for row, e, e32, ymax in rows if not passes(e, e32, ymax)]
    assert not bad, f"above {K} * e_32 + F * max|y64|: {bad}"


def _control(dev, c, idx, mutate):
    t = inputs(c, idx)
    wp = mutate(pack(c, t["w"]).clone())
    got, *_ = run_case(c, t, dev, wp=wp)
    rows = measure(c, t, got, None)
    row, e, e32, ymax = rows[0]
    print(f"control {c['variant']} {c['name']}: e {e:.3e} e_32 {e32:.3e} ratio {e / e32:.1f}")
    return passes(e, e32, ymax)


@pytest.mark.gpu
def test_positive_control_split_lo_zeroed(dev):
    """A split case whose packed weight has its fp16 lo halves zeroed must fail the bar."""
    c = _case(ring(4, 3, 3, 0, False, True), "control lo zeroed", 44, 90, 7, 52, 2, ct=3, bias=True)
    assert case_variant(c) == c["variant"]

    def zero_lo(wp):
        mt, st = (c["M"] + 15) // 16, (c["K"] + 15) // 16
        h = wp.view(torch.float16).view(mt, st, 2, 256)          # [mtile][stage][hi | lo][lane x 4 halves]
        h[:, :, 1] = 0
        return wp
    assert not _control(dev, c, 10_000, zero_lo)


@pytest.mark.gpu
def test_positive_control_last_tile_weight(dev):
    """One weight of the last, partial output tile perturbed by 2^-10 relative in the packed tensor only (the reference
    keeps the true weight) must fail the bar: an M <= 48 case with three tiles in its only pass."""
    c = _case(ring(2, 3, 4, 0, False, False), "control last tile", 44, 90, 7, 52, 2, ct=3, bias=True)
    assert case_variant(c) == c["variant"]
    m, k = 41, 57                                               # tile 2 holds rows 32..43

    def perturb(wp):
        ks = 4 * ((c["K"] + 15) // 16)
        v = wp.view((c["M"] + 15) // 16, ks, 4, 16)             # [mtile][k-step][g][r], k = 4 k-step + g
        v[m // 16, k // 4, k % 4, m % 16] *= 1.0 + 2.0 ** -10
        return wp
    assert not _control(dev, c, 10_001, perturb)
