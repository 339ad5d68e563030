"""The normalising kernels on flat, black and bound-reaching inputs, each against float64.

Every other GPU test draws its activations from independent uniform noise, on which a normalising kernel cannot reach its
special cases (no pixel with zero variance over the channels, no zero q / k row, no constant plane).  Here the inputs come
from tests/degenerate.py; shapes and tolerances are those of each kernel's own existing test, the float64 references and the
fixed bars the shared ones of tests/block_model.py and tests/scan_model.py, the tolerance taken over the whole float64 output
where it scales with max|ref|.

One tolerance needed mending.  test_gemm1x1_f16x3, test_gemm_presplit and test_ln_gemm_presplit_fused carry an ABSOLUTE
clause (e < 2e-5) written for outputs of magnitude ~10.  A BiasFree LayerNorm does not remove the mean, so a C(a) or A(a)
pixel gives a / sqrt(eps) * w = 316 a w and GEMM outputs of magnitude 1e3, whose fp32 half-ulp (3e-5 ... 6e-5) is already
above 2e-5: no fp32 result can meet it.  On the C(a) and A(a) pixels of the BiasFree rows, and only there, that clause is
applied as 2e-5 * max(1, |ref|max over the pixels of that pattern) (abs_scale); noise, Z and S pixels of the same rows, and
every pixel of the WithBias rows, keep the 2e-5 verbatim, and the clauses relative to the exact-f32 kernel are unchanged.

The float64 references are the plain ones of the existing tests everywhere.  Two fixed operand ranges of the kernels end
where a flat BiasFree pixel is (open items): the clamp of irm_ln_split_f16 at +-65000 / s_x and the
+-16 x 65000 of the fused GDFN kernels' gate.  The ordinary tests hold every element that does not reach such a limit to the
ordinary bar against plain float64 and ask the ones beyond it to be finite; test_biasfree_clamp_is_pinned and
test_gdfn_gate_limit_is_pinned say where each limit starts: the largest power of two below it meets the ordinary bar against
plain float64, the next one above it is finite and equals the float64 reference limited at the same value.

test_every_listed_entry_point_ran checks at the end that each entry point of the families below was launched; like the
ledger's, it needs the whole module in one process (it skips itself under -k or a split of the module over workers): the run
of the whole file is the one that counts."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_model as bm
import degenerate as dg
import scan_model
from block_model import FPN_TOL, FUSED_TOL, OPS_TOL, qk_from_tm, qk_to_tm, unpack_mfold, unpack_presplit
from block_model import run_mdta_fold as _fold
from irm_amd import _hip, ops, synth
from oracle import mair_ref

pytestmark = pytest.mark.gpu

IMAGES = ("patterned", "all_Z", "all_C1")
SAT = 65000.0                                  # irm_sat_h (irm_common.h)
_REACHED = set()

LISTED = {
    "irm_ln_stats_f32", "irm_gemm1x1_f32", "irm_gemm1x1_f16x3_f32",
    "irm_ln_split_f16", "irm_gemm_presplit_f16x3_f32", "irm_ln_gemm_presplit_f16x3_f32", "irm_ln_gemm_presplit_cl_f16x3_f32",
    "irm_gdfn_fused_f16x3_f32", "irm_attn_gdfn_fused_f16x3_f32", "irm_qkv_dw_fused_f16x3_f32", "irm_qkv_dw_fused_tm_f16x3_f32",
    "irm_qkv_dw_cm_f16x3_f32", "irm_qkv_gram_cm_f16x3_f32",
    "irm_mdta_gram_f32", "irm_mdta_gram_f16x3_f32", "irm_mdta_gram_tm_f32", "irm_mdta_gram_tm_f16x3_f32", "irm_dw_gram_cm_f16x3_f32",
    "irm_mdta_finalize_f32", "irm_mdta_finalize_f16x3_f32", "irm_mdta_finalize_frag_f16x3_f32",
    "irm_chan_stats_f32", "irm_chan_stats_ws_f32", "irm_chan_norm_act_f32",
    "irm_selective_scan_f32", "irm_losh_combine_f32",
}


@pytest.fixture(scope="module", autouse=True)
def _record_entry_points():
    yield from bm.record_calls(_REACHED)


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(977, name, shape, lo, hi)


def image(kind, tag, B, K, H, W, tile, lo=-1.5, hi=2.0):
    """(x [B][K][H][W], labels [H][W]) of one of IMAGES."""
    if kind == "patterned":
        return dg.patterned_image(tag, B, K, H, W, tile, lo, hi)
    name = "Z" if kind == "all_Z" else "C(1)"
    return dg.all_pattern_image(name, B, K, H, W), torch.full((H, W), dg.PATTERNS[name])


def ln64(xd, lnw, lnb, ln, labels=None, clamp=None):
    """The float64 LayerNorm of the existing tests (block_model.layer_norm).  labels: the output at the Z / C(a) pixels REPLACED by
    the bias (WithBias: what the LayerNorm of a pixel without deviations is); clamp: BiasFree output limited to +-clamp."""
    y = bm.layer_norm(xd, lnw, lnb, ln)
    if labels is not None:
        assert ln == 1
        m = dg.flat_mask(labels)
        y = torch.where(m[None, None], lnb.double().view(1, -1, 1, 1).expand_as(y), y)
    if clamp is not None:
        y = y.clamp(-clamp, clamp)
    return y


def in_slice(x, extra, at, tag):
    """x as a channel slice of a larger noise buffer (a batch stride that is not C * H * W), as the existing tests feed it."""
    B, K, H, W = x.shape
    big = rnd(tag + "big", (B, K + extra, H, W), -2.0, 3.0)
    big[:, at:at + K] = x
    return big


# =========================================================================== LN statistics + LN-prologue GEMM
@pytest.mark.parametrize("kind", IMAGES)
def test_ln_stats(dev, kind):
    """test_ln_stats' (2, 96, 12, 20): 240 pixels = three runs of 64 and a partial one; mean abs 1e-5, rstd rel 1e-5."""
    B, C, H, W = 2, 96, 12, 20
    x, lab = image(kind, f"lnst{kind}", B, C, H, W, 64, -2.0, 3.0)
    big = in_slice(x, 5, 2, f"lnst{kind}")
    stats = torch.empty(B, 2, H * W, device=dev)
    ops.ln_stats(big.to(dev)[:, 2:2 + C], stats, 1e-5)
    xr = x.double()
    mean, rstd = (s.reshape(B, -1) for s in bm.ln_stats(xr))
    s = stats.cpu().double()
    e_m, e_r = float((s[:, 0] - mean).abs().max()), float(((s[:, 1] - rstd).abs() / rstd).max())
    print(f"ln_stats {kind}: mean abs {e_m:.3e}  rstd rel {e_r:.3e}")
    assert e_m < 1e-5 and e_r < 1e-5


def _gemm_operands(tag, M, K, B, H, W, res, bias, wlo=0.3):
    w = rnd(tag + "w", (M, K), -wlo, wlo)
    r = rnd(tag + "r", (B, M, H, W)) if res else None
    bv = rnd(tag + "b", (M,), -0.3, 0.3) if bias else None
    lnw, lnb = rnd(tag + "lw", (K,), 0.5, 1.5), rnd(tag + "lb", (K,), -0.2, 0.2)
    return w, r, bv, lnw, lnb


def _gemm_ref(w, xn, bv, r):
    ref = torch.einsum("mk,bkhw->bmhw", w.double(), xn)
    if bv is not None:
        ref = ref + bv.double().view(1, -1, 1, 1)
    return ref if r is None else ref + r.double()


# M, K, H, W, B, ln, res, bias: test_gemm1x1's LayerNorm cases with several runs of 64 pixels - (144, 48, 16, 24) whole runs,
# (96, 48, 9, 15) = 135 pixels: two runs and a partial one on the scalar path (odd N) - each under both LayerNorm flavours
GEMM_LN = [(144, 48, 16, 24, 2, 1, False, False), (144, 48, 16, 24, 2, 2, False, False),
           (96, 48, 9, 15, 1, 1, True, True), (96, 48, 9, 15, 1, 2, True, True)]


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("M,K,H,W,B,ln,res,bias", GEMM_LN)
def test_gemm1x1_ln(dev, M, K, H, W, B, ln, res, bias, kind):
    tag = f"g{M}_{K}_{H}_{ln}{kind}"
    w, r, bv, lnw, lnb = _gemm_operands(tag, M, K, B, H, W, res, bias)
    x, lab = image(kind, tag, B, K, H, W, 64)
    ref = _gemm_ref(w, ln64(x.double(), lnw, lnb, ln), bv, r)
    xg = x.to(dev)
    stats = torch.empty(B, 2, H * W, device=dev)
    ops.ln_stats(xg, stats)
    ybig = torch.full((B, M + 3, H, W), 7.0, device=dev)
    ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), xg, ybig[:, 1:1 + M], M, K, res=r.to(dev) if res else None,
                bias=bv.to(dev) if bias else None, stats=stats, lnw=lnw.to(dev), lnb=lnb.to(dev) if ln == 1 else None, ln_mode=ln)
    got = ybig.cpu().double()
    tol = OPS_TOL * max(1.0, float(ref.abs().max()))
    err = float((got[:, 1:1 + M] - ref).abs().max())
    print(f"gemm1x1 {tag}: {err:.3e} (bar {tol:.3e})")
    assert err < tol
    assert torch.all(got[:, 0] == 7.0) and torch.all(got[:, 1 + M:] == 7.0)
    if ln == 1:
        m = dg.flat_mask(lab)
        ref_b = _gemm_ref(w, ln64(x.double(), lnw, lnb, ln, labels=lab), bv, r)      # W b + bias at the flat pixels
        assert float((got[:, 1:1 + M] - ref_b)[:, :, m].abs().max()) < tol


# M, K, H, W, B, ln, bias, ct: test_gemm1x1_f16x3's two smallest cases, one per LayerNorm flavour (whole runs of 64 pixels:
# the emulated kernel takes N % 4 == 0 only)
F16X3 = [(144, 48, 16, 24, 2, 1, False, 9), (510, 96, 16, 32, 1, 2, True, 8), (144, 48, 16, 24, 2, 2, False, 9),
         (510, 96, 16, 32, 1, 1, True, 8)]


def _abs_clause(ln, ref):
    """The absolute 2e-5 per unit of |ref|max, for a BiasFree image that is one C(a) run in noise (the clamp pin)."""
    return 2e-5 * (max(1.0, float(ref.abs().max())) if ln == 2 else 1.0)


UNBOUNDED = tuple(dg.PATTERNS[n] for n in ("C(1)", "C(-2)", "C(0.5)", "A(1)", "A(-2)", "A(0.5)"))


def abs_scale(ref, lab, ln):
    """[H][W] factor on an absolute clause (module docstring): 1, but max(1, |ref|max over the pattern's pixels) on the C(a) and
    A(a) pixels of a BiasFree row, whose LayerNorm output is 316 a w."""
    sc = torch.ones(lab.shape, dtype=torch.float64)
    if ln == 2:
        for code in UNBOUNDED:
            m = lab == code
            if bool(m.any()):
                sc[m] = max(1.0, float(ref[:, :, m].abs().max()))
    return sc


def pix(err):
    """[B][M][H][W] -> [H][W]: the largest |err| of each pixel."""
    return err.abs().amax((0, 1))


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("M,K,H,W,B,ln,bias,ct", F16X3)
def test_gemm1x1_f16x3_ln(dev, M, K, H, W, B, ln, bias, ct, kind):
    tag = f"s{M}_{K}_{ln}{kind}"
    w, _, bv, lnw, lnb = _gemm_operands(tag, M, K, B, H, W, False, bias)
    x, lab = image(kind, tag, B, K, H, W, 64, -2.0, 3.0)
    ref = _gemm_ref(w, ln64(x.double(), lnw, lnb, ln), bv, None)
    xg = x.to(dev)
    st = torch.empty(B, 2, H * W, device=dev)
    ops.ln_stats(xg, st)
    kw = dict(bias=bv.to(dev) if bias else None, stats=st, lnw=lnw.to(dev), lnb=lnb.to(dev) if ln == 1 else None, ln_mode=ln, ct=ct)
    y16, y32 = torch.empty(B, M, H, W, device=dev), torch.empty(B, M, H, W, device=dev)
    ops.gemm1x1(_hip.pack_gemm_weight_split(w).to(dev), xg, y16, M, K, split=True, **kw)
    ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), xg, y32, M, K, **kw)
    e16 = float((y16.cpu().double() - ref).abs().max())
    e32 = float((y32.cpu().double() - ref).abs().max())
    a16 = float((pix(y16.cpu().double() - ref) / abs_scale(ref, lab, ln)).max())
    print(f"gemm1x1 f16x3 {tag}: f16x3 {e16:.3e} (per unit of its pattern's bar {a16:.3e})  f32 {e32:.3e}  |ref|max {float(ref.abs().max()):.3g}")
    assert a16 < 2e-5 and e16 < 8 * max(e32, 1e-7)
    if ln == 1:
        m = dg.flat_mask(lab)
        ref_b = _gemm_ref(w, ln64(x.double(), lnw, lnb, ln, labels=lab), bv, None)
        assert float((y16.cpu().double() - ref_b)[:, :, m].abs().max()) < 2e-5


@pytest.mark.parametrize("kind", IMAGES)
def test_gemm1x1_output_statistics(dev, kind):
    """The statistics epilogue of irm_gemm1x1_f32 (the LayerNorm statistics of the GEMM's own output) on degenerate OUTPUT pixels:
    an identity weight carries the patterns through unchanged.  test_gemm1x1_fused_output_statistics' (48, 48) at 12 x 20 (three
    runs of 64 pixels and a partial one), its bars."""
    M = K = 48
    B, H, W = 2, 12, 20
    x, _ = image(kind, f"so{kind}", B, K, H, W, 64)
    ref = x.double()
    mean, rstd = (s.reshape(B, -1) for s in bm.ln_stats(ref))
    y = torch.empty(B, M, H, W, device=dev)
    st = torch.full((B, 2, H * W), float("nan"), device=dev)
    assert ops.can_fuse_stats(M)
    ops.gemm1x1(_hip.pack_gemm_weight(torch.eye(M)).to(dev), x.to(dev), y, M, K, stats_out=st)
    s_ = st.cpu().double()
    e_y, e_m, e_r = float((y.cpu().double() - ref).abs().max()), float((s_[:, 0] - mean).abs().max()), float(((s_[:, 1] - rstd).abs() / rstd).max())
    print(f"gemm1x1 stats_out {kind}: y {e_y:.3e}  mean {e_m:.3e}  rstd rel {e_r:.3e}")
    assert e_y < OPS_TOL * max(1.0, float(ref.abs().max()))
    assert e_m < 1e-5 * max(1.0, float(mean.abs().max())) and e_r < 1e-5
    st2 = torch.empty(B, 2, H * W, device=dev)
    ops.ln_stats(y, st2)
    assert float((st2 - st).abs().max()) < 1e-5 * max(1.0, float(rstd.max()))      # (1e-5 of test_..., rstd reaches 316 here)


def flat_frame(kind, B, C, H, W):
    """Planes that are constant (black: zero) or constant up to their border behind a stride-2 stencil (checker)."""
    if kind == "black":
        return torch.zeros(B, C, H, W)
    x = dg.frame("checker", (B, C, H, W), -1.0, 1.0)
    return x * (torch.arange(C, dtype=torch.float32).view(1, C, 1, 1) % 5 - 2.0) * 0.25


@pytest.mark.parametrize("kind", ["black", "checker"])
def test_fpn_convs_on_flat_planes(dev, kind):
    """The convolutions of FPN-MobileNet (stride-2 stem, stride-2 and stride-1 depth-wise, plain 1x1, dense 3x3 with bias) on the
    planes a black or checkered frame gives them, with the shapes, float64 references and TOL of test_stride2_convs, test_dwconv3x3,
    test_gemm1x1 and test_conv3x3; the stride-2 outputs of a checker are constant up to the border, exactly as in float64."""
    TOL = FPN_TOL
    x = flat_frame(kind, 2, 3, 32, 48)
    w = rnd("s2w", (32, 3, 3, 3), -0.3, 0.3)
    ref = F.conv2d(x.double(), w.double(), None, 2, 1)
    y = torch.empty(2, 32, 16, 24, device=dev)
    ops.conv3x3_s2(x.to(dev), w.to(dev), y, 3, 32)
    assert float((y.cpu().double() - ref).abs().max()) < TOL
    inner = y.cpu()[:, :, 1:-1, 1:-1]
    assert torch.equal(inner, inner[:, :, :1, :1].expand_as(inner)), "equal patches must give equal outputs"
    xd = flat_frame(kind, 2, 96, 32, 48)
    wd = rnd("s2dw", (96, 1, 3, 3))
    refd = F.conv2d(xd.double(), wd.double(), None, 2, 1, groups=96)
    yd = torch.empty(2, 96, 16, 24, device=dev)
    ops.dwconv3x3_s2(xd.to(dev), wd.reshape(96, 9).to(dev), yd)
    assert float((yd.cpu().double() - refd).abs().max()) < TOL
    ref1 = F.conv2d(xd.double(), wd.double(), None, 1, 1, groups=96)
    y1 = torch.empty(2, 96, 32, 48, device=dev)
    ops.dwconv3x3(xd.to(dev), wd.reshape(96, 9).to(dev), y1)
    assert float((y1.cpu().double() - ref1).abs().max()) < OPS_TOL
    wp = rnd("fpw", (40, 96), -0.3, 0.3)
    refp = torch.einsum("mk,bkhw->bmhw", wp.double(), xd.double())
    yp = torch.empty(2, 40, 32, 48, device=dev)
    ops.gemm1x1(_hip.pack_gemm_weight(wp).to(dev), xd.to(dev), yp, 40, 96)
    assert float((yp.cpu().double() - refp).abs().max()) < OPS_TOL * max(1.0, float(refp.abs().max()))
    wc, bc = rnd("fcw", (64, 96, 3, 3), -0.2, 0.2), rnd("fcb", (64,))
    refc = F.conv2d(xd.double(), wc.double(), bc.double(), padding=1)
    yc = torch.empty(2, 64, 32, 48, device=dev)
    ops.conv3x3(_hip.pack_conv3x3_weight(wc).to(dev), xd.to(dev), yc, 96, 64, bias=bc.to(dev))
    assert float((yc.cpu().double() - refc).abs().max()) < OPS_TOL * max(1.0, float(refc.abs().max()))


# =========================================================================== LN split + pre-split GEMM
# K, H, W, B, ln: test_ln_split's amp = 1 shapes (and its (384, 16, 8, 1, 2) without the 1e-4 amplitude)
LN_SPLIT = [(192, 16, 16, 2, 1), (192, 16, 32, 1, 2), (384, 8, 16, 3, 1), (384, 16, 8, 1, 2)]


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("K,H,W,B,ln", LN_SPLIT)
def test_ln_split(dev, K, H, W, B, ln, kind):
    """hi + lo of LayerNorm(x) s_x against the plain float64 LayerNorm, gains up to 30 as in test_ln_split.  BiasFree: with
    gains that large some channels of the C(-2) pixel pass the clamp (2 / sqrt(eps) * 30 * s_x > 65000, s_x = 4 at K = 192):
    those elements must be finite and at the limit, every other element meets the ordinary bar (test_biasfree_clamp_is_pinned
    pins where the clamp starts)."""
    N = H * W
    tag = f"ls{K}{H}{ln}{kind}"
    x, lab = image(kind, tag, B, K, H, W, 16, -2.0, 3.0)
    big = in_slice(x, 3, 2, tag)
    lnw = rnd(f"lsw{K}{ln}", (K,), 0.05, 30.0)
    lnb = rnd(f"lsb{K}{ln}", (K,), -2.0, 2.0) if ln == 1 else None
    s_x = _hip.ln_split_scale(lnw, lnb, K, ln == 1)
    xs = torch.full((B * K * N + 64,), float("nan"), device=dev)
    ops.ln_split(big.to(dev)[:, 2:2 + K], xs, lnw.to(dev), lnb.to(dev) if ln == 1 else None, ln, s_x)
    assert torch.isnan(xs[B * K * N:]).all()
    got = unpack_presplit(xs[:B * K * N].cpu(), B * N, K).view(B, N, K).permute(0, 2, 1).reshape(B, K, H, W) / s_x
    ref = ln64(x.double(), lnw, lnb, ln)
    beyond = ref.abs() * s_x > SAT if ln == 2 else torch.zeros_like(ref, dtype=torch.bool)
    assert ln == 2 or not bool(beyond.any())
    d = torch.where(beyond, torch.zeros_like(ref), got - ref)
    err, scale = float(d.abs().max()), float(ref.abs().max())
    at = np.unravel_index(int(d.abs().argmax()), ref.shape)
    if bool(beyond.any()):
        print(f"ln_split {tag}: {int(beyond.sum())} elements beyond the clamp")
        assert float((got[beyond].abs() - SAT / s_x).abs().max()) <= 4e-7 * SAT / s_x
    print(f"ln_split {tag}: s_x {s_x:g}  |ref|max {scale:.3e}  max-abs {err:.3e} at {tuple(int(i) for i in at)} (label "
          f"{int(lab[at[2], at[3]])}, ref {float(ref[at]):.4g}, x {float(x[at]):.4g}, w {float(lnw[at[1]]):.4g})")
    assert torch.isfinite(got).all() and err <= 4e-7 * scale + 1e-9
    if ln == 1:
        m = dg.flat_mask(lab)
        assert float((got - lnb.double().view(1, K, 1, 1))[:, :, m].abs().max()) <= 4e-7 * scale + 1e-9


# M, K, H, W, B, ln, bias, ct, mgroups, wg_shape: test_gemm_presplit's smallest cases with a tail workgroup (144 pixels = 9 runs
# of 16 per image), K = 192 and 384 under both LayerNorm flavours
PRESPLIT = [(576, 192, 12, 12, 3, 1, True, 6, 2, 42), (1020, 192, 12, 12, 3, 2, True, 8, 1, 32),
            (1152, 384, 12, 12, 3, 1, True, 8, 2, 81), (2042, 384, 16, 8, 1, 2, True, 8, 4, 81)]


def _presplit_pair(dev, w, x, lnw, lnb, ln, bv, ct, mgroups, wg_shape):
    B, K, H, W = x.shape
    M, N = w.shape[0], H * W
    frag, s_w = _hip.pack_gemm_weight_presplit(w.to(dev))
    s_x = _hip.ln_split_scale(lnw, lnb, K, ln == 1)
    xs = torch.empty(B * K * N, device=dev)
    xg = x.to(dev)
    ops.ln_split(xg, xs, lnw.to(dev), lnb.to(dev) if ln == 1 else None, ln, s_x)
    ybig = torch.full((B, M + 7, H, W), 777.0, device=dev)
    ops.gemm_presplit(frag, xs, ybig[:, 3:3 + M], M, K, out_scale=1.0 / (s_w * s_x), bias=None if bv is None else bv.to(dev),
                      ct=ct, mgroups=mgroups, wg_shape=wg_shape)
    assert (ybig[:, :3] == 777.0).all() and (ybig[:, 3 + M:] == 777.0).all()
    st = torch.empty(B, 2, N, device=dev)
    ops.ln_stats(xg, st)
    y32 = torch.empty(B, M, H, W, device=dev)
    ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), xg, y32, M, K, bias=None if bv is None else bv.to(dev), stats=st,
                lnw=lnw.to(dev), lnb=lnb.to(dev) if ln == 1 else None, ln_mode=ln)
    return ybig[:, 3:3 + M].cpu().double(), y32.cpu().double(), frag, s_w, s_x


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("M,K,H,W,B,ln,bias,ct,mgroups,wg_shape", PRESPLIT)
def test_gemm_presplit(dev, M, K, H, W, B, ln, bias, ct, mgroups, wg_shape, kind):
    tag = f"p{M}{K}{H}{ln}{kind}"
    x, lab = image(kind, tag, B, K, H, W, 16, -2.0, 3.0)
    w = rnd(tag + "w", (M, K), -0.3, 0.3)
    lnw = rnd(tag + "lw", (K,), 0.5, 1.5)
    lnb = rnd(tag + "lb", (K,), -0.2, 0.2) if ln == 1 else None
    bv = rnd(tag + "b", (M,), -0.3, 0.3) if bias else None
    ref = _gemm_ref(w, ln64(x.double(), lnw, lnb, ln), bv, None)
    y16, y32, _, _, s_x = _presplit_pair(dev, w, x, lnw, lnb, ln, bv, ct, mgroups, wg_shape)
    if ln == 2:      # nothing of this image reaches the clamp (test_biasfree_clamp_is_pinned covers where it starts)
        assert float(ln64(x.double(), lnw, lnb, ln).abs().max()) * s_x < SAT
    e16, e32 = float((y16 - ref).abs().max()), float((y32 - ref).abs().max())
    a16 = float((pix(y16 - ref) / abs_scale(ref, lab, ln)).max())
    print(f"presplit {tag}: f16x3 {e16:.3e} (per unit of its pattern's bar {a16:.3e})  f32 {e32:.3e}  |ref|max {float(ref.abs().max()):.3g}")
    assert a16 < 2e-5 and e16 <= 2.0 * max(e32, 1e-7)
    if ln == 1:
        m = dg.flat_mask(lab)
        ref_b = _gemm_ref(w, ln64(x.double(), lnw, lnb, ln, labels=lab), bv, None)
        assert float((y16 - ref_b)[:, :, m].abs().max()) < 2e-5


def _ln_fused(dev, frag, x, lnw, lnb, ln, s_x, s_w, bv, M):
    B, K, H, W = x.shape
    y = torch.full((B, M + 2, H, W), 9.0, device=dev)
    _hip.call("irm_ln_gemm_presplit_f16x3_f32", _hip.ptr(frag), _hip.ptr(x), x.stride(0), _hip.ptr(lnw), _hip.ptr(lnb), ln,
              float(s_x), 1e-5, _hip.ptr(y[:, 1:1 + M]), y.stride(0), _hip.ptr(bv), float(1.0 / (s_w * s_x)), B, M, K, H * W, 1)
    assert (y[:, 0] == 9.0).all() and (y[:, -1] == 9.0).all()
    return y[:, 1:1 + M].cpu().double()


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("M,H,W,B,ln,bias", [(576, 16, 16, 2, 1, True), (1020, 12, 12, 3, 2, False)])
def test_ln_gemm_presplit_fused(dev, M, H, W, B, ln, bias, kind):
    """The LayerNorm inside the GEMM's operand load (K = 192) against float64 and against the two-launch pair, with
    test_ln_gemm_presplit_fused's three clauses."""
    K = 192
    tag = f"lf{M}{H}{ln}{kind}"
    x, lab = image(kind, tag, B, K, H, W, 16, -2.0, 3.0)
    big = in_slice(x, 2, 1, tag)
    w = rnd(tag + "w", (M, K), -0.3, 0.3)
    lnw = rnd(tag + "lw", (K,), 0.5, 1.5)
    lnb = rnd(tag + "lb", (K,), -0.2, 0.2) if ln == 1 else None
    bv = rnd(tag + "b", (M,), -0.3, 0.3) if bias else None
    ref = _gemm_ref(w, ln64(x.double(), lnw, lnb, ln), bv, None)
    y0, _, frag, s_w, s_x = _presplit_pair(dev, w, x, lnw, lnb, ln, bv, 4, 1, 43)
    y1 = _ln_fused(dev, frag, big.to(dev)[:, 1:1 + K], lnw.to(dev), None if lnb is None else lnb.to(dev), ln, s_x, s_w,
                   None if bv is None else bv.to(dev), M)
    e0, e1, dd = float((y0 - ref).abs().max()), float((y1 - ref).abs().max()), float((y1 - y0).abs().max())
    sc = abs_scale(ref, lab, ln)
    a1, ad = float((pix(y1 - ref) / sc).max()), float((pix(y1 - y0) / sc).max())
    a10 = float(((pix(y1 - ref) - 1.5 * e0) / sc).max())
    print(f"LN-fused presplit {tag}: fused {e1:.3e}  pair {e0:.3e}  fused vs pair {dd:.3e}  |ref|max {float(ref.abs().max()):.3g}; "
          f"per unit of the pattern's bar: fused {a1:.3e}, fused vs pair {ad:.3e}")
    assert a1 < 2e-5 and a10 <= 1e-6 and ad <= 1e-5
    if ln == 1:
        m = dg.flat_mask(lab)
        ref_b = _gemm_ref(w, ln64(x.double(), lnw, lnb, ln, labels=lab), bv, None)
        assert float((y1 - ref_b)[:, :, m].abs().max()) < 2e-5


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("ln", [1, 2])
def test_ln_gemm_presplit_cl(dev, ln, kind):
    """The same LayerNorm + GEMM writing h tile-major channel-last (the C = 192 GDFN's project_in), as test_gdfn_tail_c192
    checks h: 16 x 64 = 2 x 2 tiles, <= TOL max(1, |href|max)."""
    C, hid, hp, H, W, B = 192, 510, 512, 16, 64, 2
    tag = f"cl{ln}{kind}"
    x, lab = image(kind, tag, B, C, H, W, (8, 32))
    big = in_slice(x, 3, 1, tag)
    lnw = rnd(tag + "lw", (C,), 0.5, 1.5)
    lnb = rnd(tag + "lb", (C,), -0.2, 0.2) if ln == 1 else None
    pin_w, pin_b = rnd(tag + "pi", (2 * hid, C), -0.2, 0.2), rnd(tag + "pib", (2 * hid,), -0.3, 0.3)
    frag, s_w, bp = _hip.pack_pin_padded(pin_w.to(dev), pin_b.to(dev), hp)
    s_x = _hip.ln_split_scale(lnw, lnb, C, ln == 1)
    h_cl = torch.full((B * 2 * hp * H * W + 64,), 7.0, device=dev)
    ops.ln_gemm_presplit_cl(frag, big.to(dev)[:, 1:1 + C], h_cl, 2 * hp, C, lnw.to(dev), None if lnb is None else lnb.to(dev), ln,
                            s_x, out_scale=1.0 / (s_w * s_x), bias=bp)
    assert torch.all(h_cl[-64:] == 7.0)
    hc = (h_cl[:-64].cpu().view(B, H // 8, W // 32, 2 * hp // 64, 8, 32, 64).permute(0, 3, 6, 1, 4, 2, 5)
          .reshape(B, 2 * hp, H, W)).double()
    got = torch.cat([hc[:, :hid], hc[:, hp:hp + hid]], 1)

    def href(labels):
        return F.conv2d(ln64(x.double(), lnw, lnb, ln, labels=labels), pin_w.double()[:, :, None, None], pin_b.double())
    ref = href(None)
    tol = FUSED_TOL * max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"LN-fused cl {tag}: {err:.3e} (bar {tol:.3e})")
    assert err <= tol
    assert float(hc[:, hid:hp].abs().max()) == 0.0 and float(hc[:, hp + hid:].abs().max()) == 0.0
    if ln == 1:
        assert float((got - href(lab))[:, :, dg.flat_mask(lab)].abs().max()) <= tol


def clamp_threshold(lnw, K):
    """Largest |a| for which a BiasFree C(a) pixel stays below the clamp of irm_ln_split_f16, from the code: the kernel
    forms fl(fl(a rstd) (w s_x)) with rstd = 1 / sqrt(0 + eps) and limits it at +-65000, so channel k clamps from
    |a| = 65000 sqrt(eps) / (s_x |w_k|) on - first the channel with the largest gain."""
    s_x = _hip.ln_split_scale(lnw, None, K, False)
    return SAT * (1e-5 ** 0.5) / (s_x * float(lnw.abs().max())), s_x


@pytest.mark.parametrize("K,M,H,W,B", [(192, 576, 12, 12, 3), (384, 1152, 12, 12, 3)])
def test_biasfree_clamp_is_pinned(dev, K, M, H, W, B):
    """Where the BiasFree clamp starts (Degenerate inputs): a run of 16 C(a) pixels inside a noise image, a the
    largest power of two below the derived threshold and the next one above it.  Below: the ordinary bars of test_ln_split and
    test_gemm_presplit against the plain float64 LayerNorm.  Above: finite, and the same bars against the float64 reference
    whose LayerNorm output is clamped at +-65000 / s_x (the exact-f32 kernel pair does not clamp: no comparison with it
    there).  K = 192 also through the LN-fused GEMM."""
    tag = f"clamp{K}"
    lnw = rnd(tag + "lw", (K,), 0.5, 1.5)
    thr, s_x = clamp_threshold(lnw, K)
    below = 2.0 ** np.floor(np.log2(thr))
    if below == thr:
        below /= 2.0
    above = 2.0 * below
    assert below < thr < above
    print(f"BiasFree clamp K{K}: s_x {s_x:g}  max|w| {float(lnw.abs().max()):.4f}  threshold |a| {thr:.4f} = "
          f"{thr / 1e-5 ** 0.5:.1f} sqrt(var + eps); below {below:g}  above {above:g}")
    w = rnd(tag + "w", (M, K), -0.3, 0.3)
    bv = rnd(tag + "b", (M,), -0.3, 0.3)
    N = H * W
    for a, clamped in ((below, False), (above, True), (-above, True)):
        x = rnd(tag + "x", (B, K, H, W), -2.0, 3.0)
        x.view(B, K, N)[:, :, 16:32] = a
        lim = SAT / s_x
        plain = ln64(x.double(), lnw, None, 2)
        assert (float(plain.abs().max()) > lim) == clamped
        lnr = plain.clamp(-lim, lim)
        ref = _gemm_ref(w, lnr, bv, None)
        y16, y32, frag, s_w, _ = _presplit_pair(dev, w, x, lnw, None, 2, bv, *((6, 2, 42) if K == 192 else (8, 2, 81)))
        xs = torch.empty(B * K * N, device=dev)
        ops.ln_split(x.to(dev), xs, lnw.to(dev), None, 2, s_x)
        got = unpack_presplit(xs.cpu(), B * N, K).view(B, N, K).permute(0, 2, 1).reshape(B, K, H, W) / s_x
        e_ln, e16, e32 = float((got - lnr).abs().max()), float((y16 - ref).abs().max()), float((y32 - ref).abs().max())
        print(f"  a {a:g}: ln_split {e_ln:.3e} (|ref|max {float(lnr.abs().max()):.4g})  gemm f16x3 {e16:.3e}  f32 pair {e32:.3e}  "
              f"|ref|max {float(ref.abs().max()):.4g}")
        assert torch.isfinite(got).all() and torch.isfinite(y16).all()
        assert e_ln <= 4e-7 * float(lnr.abs().max()) + 1e-9
        assert e16 < _abs_clause(2, ref)
        if not clamped:
            assert e16 <= 2.0 * max(e32, 1e-7)
        if K == 192:
            y1 = _ln_fused(dev, frag, x.to(dev), lnw.to(dev), None, 2, s_x, s_w, bv.to(dev), M)
            e1 = float((y1 - ref).abs().max())
            print(f"  a {a:g}: LN-fused gemm {e1:.3e}")
            assert torch.isfinite(y1).all() and e1 < _abs_clause(2, ref) and e1 <= 1.5 * e16 + 1e-6 * _abs_clause(2, ref) / 2e-5


# =========================================================================== fused branch kernels
GATE_SAT = 16.0 * SAT      # the gated activations are split to fp16 behind a fixed 2^-4 and limited at +-65000 there (irm_gate_split2)


def gdfn_reference(x1, o, ln):
    """(block_model.gdfn as it stands, [B][H][W] mask of the pixels with a gate value beyond the kernels' limit).  WithBias: no
    such pixel.  BiasFree: a C(a) pixel enters project_in as a / sqrt(eps) w = 316 a w, its gate gelu(h1) h2 reaches 1e6 and
    passes |gate| <= 16 x 65000 (test_gate_out_of_range_saturates_instead_of_nan; test_gdfn_gate_limit_is_pinned)."""
    plain = bm.gdfn(x1.double(), o["lnw"], o["lnb"], ln, o["pin_w"], o["pin_b"], o["dw_w"], o["dw_b"], o["pout_w"], o["pout_b"])
    _, beyond = bm.gdfn_from_ln(x1.double(), ln64(x1.double(), o["lnw"], o["lnb"], ln), o["pin_w"], o["pin_b"], o["dw_w"], o["dw_b"],
                       o["pout_w"], o["pout_b"], gate_sat=GATE_SAT)
    assert ln == 2 or not bool(beyond.any())
    return plain, beyond


def held(got, ref, beyond):
    """max |got - ref| over the pixels that do not reach the limit."""
    return float(torch.where(beyond[:, None], torch.zeros_like(ref), got - ref).abs().max())


def _gdfn_operands(tag, C, hid, ln):
    return dict(zip(("lnw", "lnb", "pin_w", "pin_b", "dw_w", "dw_b", "pout_w", "pout_b"), bm.gdfn_operands(rnd, tag, C, hid, ln)))


# C, hid, H, W, B: test_gdfn_fused's (48, 127, 20, 36) = 3 x 2 tiles of 8 x 32, partial in both directions, and (96, 255, 24, 40)
BRANCH = [(48, 127, 20, 36, 1), (96, 255, 24, 40, 2)]


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("ln", [1, 2])
@pytest.mark.parametrize("C,hid,H,W,B", BRANCH)
def test_gdfn_fused(dev, C, hid, H, W, B, ln, kind):
    tag = f"f{C}_{ln}{kind}"
    o = _gdfn_operands(tag, C, hid, ln)
    x, lab = image(kind, tag, B, C, H, W, (8, 32))
    big = in_slice(x, 3, 1, tag)
    ref, beyond = gdfn_reference(x, o, ln)
    pk = _hip.pack_gdfn_fused(o["pin_w"].to(dev), o["pin_b"], o["dw_w"], o["dw_b"], o["pout_w"], o["lnw"], o["lnb"])
    xb = big.to(dev)
    yb = torch.full((B, C + 2, H, W), 7.0, device=dev)
    ops.gdfn_fused(pk, xb[:, 1:1 + C], yb[:, 2:2 + C], C, hid, ln_mode=ln, bias=o["pout_b"].to(dev))
    y = yb.cpu()
    got = y[:, 2:2 + C].double()
    tol = FUSED_TOL * max(1.0, float(ref.abs().max()))
    err = held(got, ref, beyond)
    print(f"gdfn_fused {tag}: {err:.3e} (bar {tol:.3e}){f'  pixels beyond the gate limit, not held: {int(beyond.sum())} of {beyond.numel()}' if bool(beyond.any()) else ''}")
    assert err <= tol and bool(torch.isfinite(got).all())
    assert torch.all(y[:, :2] == 7.0) and torch.equal(xb.cpu(), big)
    if ln == 1:
        m = dg.flat_neighbourhood_mask(lab)
        ref_b, _ = bm.gdfn_from_ln(x.double(), ln64(x.double(), o["lnw"], o["lnb"], 1, labels=lab), o["pin_w"], o["pin_b"], o["dw_w"],
                          o["dw_b"], o["pout_w"], o["pout_b"])
        assert bool(m.any()) and float((got - ref_b)[:, :, m].abs().max()) <= tol


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("ln", [1, 2])
@pytest.mark.parametrize("C,hid,H,W,B", BRANCH)
def test_attn_gdfn_fused(dev, C, hid, H, W, B, ln, kind):
    """x' = x + Mfold[b] v, y = x' + GDFN(x').  The LayerNorm reads x', so the patterns must arrive there exactly: v is 0 at
    the patterned pixels (the folded attention then adds exact zeros) and there is no project_out bias of the attention."""
    tag = f"a{C}_{ln}{kind}"
    o = _gdfn_operands(tag, C, hid, ln)
    x, lab = image(kind, tag, B, C, H, W, (8, 32))
    big = in_slice(x, 3, 1, tag)
    vbig = rnd(tag + "v", (B, 3 * C, H, W), -2.0, 2.0)
    vbig[:, 2 * C:][:, :, lab != 0] = 0.0
    mf = rnd(tag + "m", (B, C, C), -0.2, 0.2)
    x1 = x.double() + torch.einsum("bij,bjhw->bihw", mf.double(), vbig[:, 2 * C:].double())
    assert torch.equal(x1[:, :, lab != 0], x.double()[:, :, lab != 0])
    ref, beyond = gdfn_reference(x1, o, ln)
    pk = _hip.pack_gdfn_fused(o["pin_w"].to(dev), o["pin_b"], o["dw_w"], o["dw_b"], o["pout_w"], o["lnw"], o["lnb"], kperm=True)
    frag = _hip.pack_mfold_frag(mf).to(dev)
    xb, vb = big.to(dev), vbig.to(dev)
    yb = torch.full((B, C + 2, H, W), 7.0, device=dev)
    ops.attn_gdfn_fused(pk, xb[:, 1:1 + C], vb[:, 2 * C:], frag, yb[:, 2:2 + C], C, hid, ln_mode=ln, bias=o["pout_b"].to(dev))
    y = yb.cpu()
    got = y[:, 2:2 + C].double()
    tol = FUSED_TOL * max(1.0, float(ref.abs().max()))
    err = held(got, ref, beyond)
    print(f"attn_gdfn_fused {tag}: {err:.3e} (bar {tol:.3e}){f'  pixels beyond the gate limit, not held: {int(beyond.sum())} of {beyond.numel()}' if bool(beyond.any()) else ''}")
    assert err <= tol and bool(torch.isfinite(got).all())
    assert torch.all(y[:, :2] == 7.0) and torch.equal(xb.cpu(), big) and torch.equal(vb.cpu(), vbig)
    if ln == 1:
        m = dg.flat_neighbourhood_mask(lab)
        ref_b, _ = bm.gdfn_from_ln(x1, ln64(x1, o["lnw"], o["lnb"], 1, labels=lab), o["pin_w"], o["pin_b"], o["dw_w"], o["dw_b"], o["pout_w"],
                          o["pout_b"])
        assert float((got - ref_b)[:, :, m].abs().max()) <= tol


@pytest.mark.parametrize("attn", [False, True])
@pytest.mark.parametrize("C,hid,H,W,B", BRANCH)
def test_gdfn_gate_limit_is_pinned(dev, C, hid, H, W, B, attn):
    """Where the gate limit of the fused GDFN kernels starts for a BiasFree C(a) pixel: one row of tiles
    of C(a) inside a noise image, a the largest power of two for which no gate value of the float64 chain passes 16 x 65000, and
    the next one.  Below: the ordinary bar against the plain float64 block_model.gdfn at every pixel.  Above: finite, and the
    ordinary bar against the float64 chain whose gate is limited at the same value.  The threshold comes from the float64 chain
    and the constants of irm_gate_split2, not from a run of the kernel."""
    tag = f"gate{C}{int(attn)}"
    o = _gdfn_operands(tag, C, hid, 2)
    noise = rnd(tag + "x", (B, C, H, W), -1.5, 2.0)
    vbig = rnd(tag + "v", (B, 3 * C, H, W), -2.0, 2.0)
    vbig[:, 2 * C:, 8:16] = 0.0                                  # the attention adds exact zeros on the flat rows
    mf = rnd(tag + "m", (B, C, C), -0.2, 0.2)

    def chain(a, sat):
        x = noise.clone()
        x[:, :, 8:16] = a
        x1 = x.double() + torch.einsum("bij,bjhw->bihw", mf.double(), vbig[:, 2 * C:].double()) if attn else x.double()
        y, beyond = bm.gdfn_from_ln(x1, ln64(x1, o["lnw"], None, 2), o["pin_w"], o["pin_b"], o["dw_w"], o["dw_b"], o["pout_w"], o["pout_b"],
                           gate_sat=sat)
        return x, x1, y, beyond
    below = max(a for a in (2.0 ** k for k in range(-8, 4)) if not bool(chain(a, GATE_SAT)[3].any()))
    above = 2.0 * below
    assert bool(chain(above, GATE_SAT)[3].any())
    if attn:
        pk = _hip.pack_gdfn_fused(o["pin_w"].to(dev), o["pin_b"], o["dw_w"], o["dw_b"], o["pout_w"], o["lnw"], None, kperm=True)
        frag, vb = _hip.pack_mfold_frag(mf).to(dev), vbig.to(dev)
    else:
        pk = _hip.pack_gdfn_fused(o["pin_w"].to(dev), o["pin_b"], o["dw_w"], o["dw_b"], o["pout_w"], o["lnw"], None)
    for a, limited in ((below, False), (above, True)):
        x, x1, ref, beyond = chain(a, GATE_SAT if limited else None)
        if not limited:
            plain = bm.gdfn(x1, o["lnw"], None, 2, o["pin_w"], o["pin_b"], o["dw_w"], o["dw_b"], o["pout_w"], o["pout_b"])
            assert float((ref - plain).abs().max()) <= 1e-12 * float(plain.abs().max())
            ref = plain
        y = torch.empty(B, C, H, W, device=dev)
        if attn:
            ops.attn_gdfn_fused(pk, x.to(dev), vb[:, 2 * C:], frag, y, C, hid, ln_mode=2, bias=o["pout_b"].to(dev))
        else:
            ops.gdfn_fused(pk, x.to(dev), y, C, hid, ln_mode=2, bias=o["pout_b"].to(dev))
        got = y.cpu().double()
        tol = FUSED_TOL * max(1.0, float(ref.abs().max()))
        err = float((got - ref).abs().max())
        print(f"gate limit {tag}: a {a:g} ({'limited' if limited else 'plain'} reference, {int(beyond.sum())} pixels beyond): {err:.3e} (bar {tol:.3e})")
        assert bool(torch.isfinite(got).all()) and err <= tol and bool(beyond.any()) == limited


def _qkv_operands(tag, C, ln, bias=True):
    M = 3 * C
    return dict(lnw=rnd(tag + "lw", (C,), 0.5, 1.5), lnb=rnd(tag + "lb", (C,), -0.2, 0.2) if ln == 1 else None,
                w=rnd(tag + "w", (M, C), -0.3, 0.3), dw_w=rnd(tag + "dw", (M, 9), -0.4, 0.4),
                wb=rnd(tag + "wb", (M,), -0.3, 0.3) if bias else None, dw_b=rnd(tag + "dwb", (M,), -0.3, 0.3) if bias else None)


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("ln", [1, 2])
@pytest.mark.parametrize("C,H,W,B", [(48, 20, 36, 1), (96, 24, 40, 2)])
def test_qkv_dw_fused(dev, C, H, W, B, ln, kind):
    tag = f"q{C}_{ln}{kind}"
    M = 3 * C
    o = _qkv_operands(tag, C, ln)
    x, lab = image(kind, tag, B, C, H, W, (8, 32))
    big = in_slice(x, 3, 1, tag)
    ref = bm.qkv(x.double(), o["lnw"], o["lnb"], ln, o["w"], o["wb"], o["dw_w"], o["dw_b"])
    pk = _hip.pack_qkv_fused(o["w"].to(dev), o["wb"], o["dw_w"], o["dw_b"], o["lnw"], o["lnb"])
    yb = torch.full((B, M + 2, H, W), 7.0, device=dev)
    ops.qkv_dw_fused(pk, big.to(dev)[:, 1:1 + C], yb[:, 1:1 + M], C, M, ln_mode=ln)
    y = yb.cpu()
    got = y[:, 1:1 + M].double()
    tol = FUSED_TOL * max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"qkv_dw_fused {tag}: {err:.3e} (bar {tol:.3e})")
    assert err <= tol
    assert torch.all(y[:, 0] == 7.0) and torch.all(y[:, M + 1] == 7.0)
    if ln == 1:
        m = dg.flat_neighbourhood_mask(lab)
        ref_b = bm.qkv_from_ln(ln64(x.double(), o["lnw"], o["lnb"], 1, labels=lab), o["w"], o["wb"], o["dw_w"], o["dw_b"])
        assert bool(m.any()) and float((got - ref_b)[:, :, m].abs().max()) <= tol


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("C,heads,ln", [(96, 2, 1), (48, 1, 1), (96, 2, 2), (48, 1, 2)])
def test_qkv_tile_major_chain(dev, C, heads, ln, kind):
    """qkv_dw_fused(tm) at 16 x 64 (2 x 2 whole tiles: test_qk_tile_major_chain's smallest such shape) - the tile-major kernel
    at C = 96, the channel-major one at C = 48: q, k, v against float64 with test_qkv_dw_fused's bar, q, k a bit-exact
    permutation of the planar kernel's and v its bytes, and the tile-major Gram pass (f16x3 under WithBias, f32 ring under
    BiasFree) + finalize against the float64 attention (test_mdta_fold's 2e-5) and the planar chain (2e-6)."""
    H, W, B = 16, 64, 2
    M = 3 * C
    tag = f"tm{C}_{ln}{kind}"
    o = _qkv_operands(tag, C, ln, bias=False)
    x, lab = image(kind, tag, B, C, H, W, (8, 32))
    ref = bm.qkv(x.double(), o["lnw"], o["lnb"], ln, o["w"], None, o["dw_w"], None)
    pk = _hip.pack_qkv_fused(o["w"].to(dev), None, o["dw_w"], None, o["lnw"], o["lnb"])
    gs = _hip.gram_scales(o["w"].view(M, C, 1, 1), None, o["dw_w"].view(M, 1, 3, 3), None, o["lnw"], o["lnb"], ln == 1)
    assert (gs is not None) == (ln == 1)
    gs = None if gs is None else gs.to(dev)
    temp, wout = rnd(tag + "t", (heads,), 2.0, 6.0), rnd(tag + "wo", (C, C), -0.3, 0.3)
    xg = x.to(dev)
    res = []
    for tm in (False, True):
        qkv = torch.full((B, M, H, W), 7.0, device=dev)
        ops.qkv_dw_fused(pk, xg, qkv, C, M, ln_mode=ln, tm=tm)
        a, mfold, _ = _fold(dev, qkv, temp, wout, C, heads, gram_scale=gs, tm=tm)
        res.append((qkv.cpu(), a, mfold))
    (q0, a0, m0), (q1, a1, m1) = res
    assert torch.equal(q0[:, 2 * C:], q1[:, 2 * C:])
    back = qk_from_tm(q1[:, :2 * C])
    assert torch.equal(back, q0[:, :2 * C])
    tol = FUSED_TOL * max(1.0, float(ref.abs().max()))
    err = float((torch.cat([back, q1[:, 2 * C:]], 1).double() - ref).abs().max())
    aref = bm.attention(ref[:, :C], ref[:, C:2 * C], temp, heads)
    ea = float((a1.double() - aref).abs().max())
    print(f"qkv tm chain {tag}: qkv {err:.3e} (bar {tol:.3e})  attn vs float64 {ea:.3e}  tm vs planar {float((a0 - a1).abs().max()):.3e}")
    assert err <= tol and ea < 2e-5
    assert float((a0 - a1).abs().max()) <= 2e-6 and float((m0 - m1).abs().max()) <= 2e-6
    if ln == 1:
        m = dg.flat_neighbourhood_mask(lab)
        ref_b = bm.qkv_from_ln(ln64(x.double(), o["lnw"], o["lnb"], 1, labels=lab), o["w"], None, o["dw_w"], None)
        assert float((q0.double() - ref_b)[:, :, m].abs().max()) <= tol


@pytest.mark.parametrize("kind", IMAGES)
def test_qkv_gram_cm(dev, kind):
    """qkv_gram_cm (C = 48, WithBias) at test_qkv_gram_cm_c48's 16 x 128 (2 x 4 tiles), planar x: v the bytes of qkv_dw_fused, the
    attention and the folded matrix within 2e-6 of the tile-major chain's, and the attention against float64 (2e-5)."""
    C, heads, H, W, B = 48, 1, 16, 128, 2
    M = 3 * C
    tag = f"qg{kind}"
    o = _qkv_operands(tag, C, 1, bias=False)
    x, lab = image(kind, tag, B, C, H, W, (8, 32))
    pk = _hip.pack_qkv_fused(o["w"].to(dev), None, o["dw_w"], None, o["lnw"], o["lnb"])
    gs = _hip.gram_scales(o["w"].view(M, C, 1, 1), None, o["dw_w"].view(M, 1, 3, 3), None, o["lnw"], o["lnb"], True).to(dev)
    temp, wout = rnd(tag + "t", (heads,), 2.0, 6.0), rnd(tag + "wo", (C, C), -0.3, 0.3)
    xg = x.to(dev)
    rec = C * C + 2 * C
    q0 = torch.full((B, M, H, W), 7.0, device=dev)
    ops.qkv_dw_fused(pk, xg, q0, C, M, ln_mode=1, tm=True, v_tm=True)
    a0, m0, _ = _fold(dev, q0, temp, wout, C, heads, gram_scale=gs, tm=True)
    q1 = torch.full((B, M, H, W), 7.0, device=dev)
    nchunk = (H // 8) * (W // 32) // ops.QKV_GRAM_NCH
    part = torch.full((B * nchunk * rec,), float("nan"), device=dev)
    assert ops.qkv_gram_cm(pk, xg, q1, gs, part, C, ln_mode=1, v_tm=True) == nchunk
    assert torch.all(q1[:, :2 * C] == 7.0)
    a1, m1, _ = _fold(dev, q1, temp, wout, C, heads, gram_scale=gs, tm=True, nchunk_ready=nchunk, part=part)
    assert torch.equal(q0[:, 2 * C:], q1[:, 2 * C:])
    ref = bm.qkv(x.double(), o["lnw"], o["lnb"], 1, o["w"], None, o["dw_w"], None)
    ea = float((a1.double() - bm.attention(ref[:, :C], ref[:, C:2 * C], temp, heads)).abs().max())
    da, dm = float((a0 - a1).abs().max()), float((m0 - m1).abs().max())
    print(f"qkv_gram_cm {tag}: attn vs float64 {ea:.3e}  vs chain: attn {da:.3e} mfold {dm:.3e}")
    assert da <= 2e-6 and dm <= 2e-6 and ea < 2e-5


# =========================================================================== MDTA: zero and repeated rows
MDTA_CASES = ("q_head_zero", "k_head_zero", "all_zero", "q_rows_equal", "q_one_pixel")


def mdta_degenerate(case, q, k, heads):
    """q, k [B][C][H][W] (any dtype) edited in place: the five cases of the issue, on head 0 (q) / the last head (k)."""
    B, C, H, W = q.shape
    c = C // heads
    if case == "q_head_zero":
        q[:, :c] = 0
    elif case == "k_head_zero":
        k[:, C - c:] = 0
    elif case == "all_zero":
        q.zero_()
        k.zero_()
    elif case == "q_rows_equal":
        q[:, :c] = q[:, :1].clone()
    elif case == "q_one_pixel":
        keep = q[:, :, H // 2, W // 3].clone()
        q.zero_()
        q[:, :, H // 2, W // 3] = keep
    else:
        raise ValueError(case)


def check_attention(case, a, aref, heads, tol=2e-5):
    """The attention as test_mdta_fold compares it, and the exact properties of the case."""
    c = a.shape[-1]
    err = float((a.double() - aref).abs().max())
    assert err < tol, (case, err)
    uniform = torch.full((c,), 1.0, dtype=torch.float32) / torch.tensor(float(c), dtype=torch.float32)
    if case == "all_zero":
        assert torch.equal(a, uniform.expand_as(a)), "softmax rows of zero logits must be exactly 1 / c"
    elif case == "q_head_zero":
        assert torch.equal(a[:, 0], uniform.expand_as(a[:, 0]))
    elif case == "k_head_zero":
        assert torch.equal(a[:, -1], uniform.expand_as(a[:, -1]))
    elif case == "q_rows_equal":
        assert torch.equal(a[:, 0], a[:, 0, :1].expand_as(a[:, 0])), "equal q rows must give identical rows of A"
    return err


@pytest.mark.parametrize("case", MDTA_CASES)
@pytest.mark.parametrize("B,C,heads,H,W", [(1, 96, 2, 16, 16), (1, 64, 2, 8, 8)])
def test_mdta_fold(dev, B, C, heads, H, W, case):
    """test_mdta_fold's (1, 96, 2, 16, 16) (LDS-DMA ring Gram) and (1, 64, 2, 8, 8) (generic Gram), two heads so that one can
    be degenerate next to an ordinary one: the f32 Gram pass and all three finalize entries."""
    N, c = H * W, C // heads
    tag = f"md{C}{case}"
    qkv = rnd(tag, (B, 3 * C, H, W))
    mdta_degenerate(case, qkv[:, :C], qkv[:, C:2 * C], heads)
    temp, wout = rnd(tag + "t", (heads,), 2.0, 6.0), rnd(tag + "w", (C, C), -0.3, 0.3)
    aref = bm.attention(qkv[:, :C].double(), qkv[:, C:2 * C].double(), temp, heads)
    v = qkv[:, 2 * C:].double().reshape(B, heads, c, N)
    ref = torch.einsum("oc,bcn->bon", wout.double(), (aref @ v).reshape(B, C, N)).reshape(B, C, H, W)
    qg = qkv.to(dev)
    a, mfold, _ = _fold(dev, qg, temp, wout, C, heads)
    err = check_attention(case, a, aref, heads)
    y = torch.empty(B, C, H, W, device=dev)
    ops.gemm1x1(mfold.to(dev), qg[:, 2 * C:], y, C, C, w_bs=ops.mfold_numel(C))
    e_y = float((y.cpu().double() - ref).abs().max())
    print(f"mdta {tag}: attn {err:.3e}  folded + applied {e_y:.3e}")
    assert e_y < OPS_TOL
    a2, mf2, _ = _fold(dev, qg, temp, wout, C, heads, split=True)
    y2 = torch.empty(B, C, H, W, device=dev)
    ops.gemm1x1(mf2.to(dev), qg[:, 2 * C:], y2, C, C, w_bs=ops.mfold_numel(C), split=True)
    assert torch.equal(a2, a) and float((y2.cpu().double() - ref).abs().max()) < OPS_TOL and float((y2 - y).abs().max()) < 2e-5
    part = torch.full((B * heads * ops.mdta_plan(B, C, heads, N)[1] * (c * c + 2 * c),), float("nan"), device=dev)
    gsum = torch.empty(B * heads * (c * c + 2 * c), device=dev)
    mfrag = torch.zeros(B * ops.mfold_frag_numel(C), device=dev)
    a3 = torch.empty(B, heads, c, c, device=dev)
    ops.mdta_fold(qg, part, gsum, temp.to(dev), wout.to(dev), mfrag, C, heads, attn=a3, frag=True)
    assert torch.equal(a3.cpu(), a)
    mref = torch.stack([wout.double() @ torch.block_diag(*a[i].double()) for i in range(B)])
    assert float((_hip.unpack_mfold_frag(mfrag, B, C).double() - mref).abs().max()) < 1e-6 * max(1.0, float(mref.abs().max()))


@pytest.mark.parametrize("case", MDTA_CASES)
@pytest.mark.parametrize("tm", [False, True])
def test_mdta_gram_f16x3(dev, tm, case):
    """The emulated Gram pass (planar and tile-major q, k) next to the f32-input pass with test_mdta_gram_f16x3's clauses, at
    its (1, 96, 2, 16, 16) and at 16 x 64 for the tile-major kernels; operand scales from a per-channel bound as there."""
    B, C, heads = 1, 96, 2
    H, W = (16, 64) if tm else (16, 16)
    N, c = H * W, C // heads
    tag = f"gq{int(tm)}{case}"
    bound = rnd(tag + "b", (2 * C,), 0.5, 40.0)
    qkv = rnd(tag, (B, 3 * C, H, W))
    mdta_degenerate(case, qkv[:, :C], qkv[:, C:2 * C], heads)
    if case == "q_rows_equal":
        bound[:c] = bound[0]           # equal rows stay equal, and inside the bound their operand scale is built from
    qkv[:, :2 * C] *= bound.view(1, 2 * C, 1, 1)
    scale = torch.pow(2.0, torch.floor(torch.log2(2.0 ** 14.8 / bound))).float()
    temp, wout = rnd(tag + "t", (heads,), 2.0, 6.0), rnd(tag + "w", (C, C), -0.3, 0.3)
    q, k = qkv[:, :C].double().reshape(B, heads, c, N), qkv[:, C:2 * C].double().reshape(B, heads, c, N)
    gref = torch.cat([(q @ k.transpose(-1, -2)).reshape(B, heads, c * c), (q * q).sum(-1), (k * k).sum(-1)], -1)
    aref = bm.attention(qkv[:, :C].double(), qkv[:, C:2 * C].double(), temp, heads)
    dev_qkv = qkv.clone()
    if tm:
        dev_qkv[:, :2 * C] = qk_to_tm(qkv[:, :2 * C])
    qg = dev_qkv.to(dev)
    (a32, _, g32), (a16, _, g16) = (_fold(dev, qg, temp, wout, C, heads, gram_scale=sc, tm=tm) for sc in (None, scale.to(dev)))
    mag = max(float(gref.abs().max()), 1e-300)
    e32 = float((g32.double().view(B, heads, -1) - gref).abs().max()) / mag
    e16 = float((g16.double().view(B, heads, -1) - gref).abs().max()) / mag
    d32, d16 = check_attention(case, a32, aref, heads), check_attention(case, a16, aref, heads)
    print(f"gram {tag}: records rel err f32 {e32:.2e} f16x3 {e16:.2e}; attn abs err f32 {d32:.2e} f16x3 {d16:.2e}")
    assert e16 <= 2 * e32 + 2e-7 and d16 <= 2 * d32 + 2e-7


@functools.lru_cache(maxsize=None)
def _dw_gram_operands(case):
    C, heads, H, W, B = 192, 4, 16, 128, 2
    tag = f"dgz{case}"
    raw = rnd(tag + "x", (B, 3 * C, H, W), -3.0, 3.0)
    mdta_degenerate(case, raw[:, :C], raw[:, C:2 * C], heads)
    dw_w = rnd(tag + "dw", (3 * C, 9), -0.4, 0.4)
    if case == "q_rows_equal":
        dw_w[:C // heads] = dw_w[:1].clone()                 # equal raw rows stay equal behind equal taps
    # operand scales from a bound of |dw(q)|, |dw(k)| per channel: the taps' absolute sum times the raw range
    bound = dw_w[:2 * C].abs().sum(1) * 3.0
    gs = torch.pow(2.0, torch.floor(torch.log2(2.0 ** 14.8 / bound))).float()
    temp, wout = rnd(tag + "t", (heads,), 2.0, 6.0), rnd(tag + "wo", (C, C), -0.3, 0.3)
    qk = F.conv2d(raw.double()[:, :2 * C], dw_w.double()[:2 * C].view(2 * C, 1, 3, 3), None, padding=1, groups=2 * C)
    attn = bm.attention(qk[:, :C], qk[:, C:], temp, heads)
    mfold = torch.stack([wout.double() @ torch.block_diag(*attn[i]) for i in range(B)])
    return C, heads, H, W, B, raw, dw_w, gs, temp, wout, attn, mfold


@pytest.mark.parametrize("case", MDTA_CASES)
def test_dw_gram(dev, case):
    """dw_gram (the depth-wise conv of q, k inside the Gram pass, C = 192) at test_dw_gram's 16 x 128 (2 x 4 tiles, interior
    seams), without the depth-wise bias so that a zero raw row stays a zero row: against float64 with test_dw_gram_vs_float64's
    bound (twice the two-kernel path's error) and against the two-kernel path (2e-6)."""
    C, heads, H, W, B, raw, dw_w, gs, temp, wout, attn, mfold = _dw_gram_operands(case)
    assert ops.can_dw_gram(C, heads, H, W)
    rg, wg, gsg = raw.to(dev), dw_w.to(dev), gs.to(dev)
    rec = 48 * 48 + 96
    old = torch.full((B, 3 * C, H, W), 7.0, device=dev)
    ops.dwconv3x3(rg, wg, old)
    a0, m0, _ = _fold(dev, old, temp, wout, C, heads, gram_scale=gsg)
    new = torch.full((B, 3 * C, H, W), 7.0, device=dev)
    nchunk = (H // 8) * (W // 32) // ops.QKV_GRAM_NCH
    part = torch.full((B * heads * nchunk * rec,), float("nan"), device=dev)
    assert ops.dw_gram(rg, wg[:2 * C].contiguous(), gsg, part, C, heads) == nchunk
    a1, m1, _ = _fold(dev, new, temp, wout, C, heads, gram_scale=gsg, nchunk_ready=nchunk, part=part)
    assert not bool(torch.isnan(part).any())
    m0, m1 = unpack_mfold(m0, B, C), unpack_mfold(m1, B, C)
    ea0, ea1 = check_attention(case, a0, attn, heads), check_attention(case, a1, attn, heads)
    em0, em1 = float((m0.double() - mfold).abs().max()), float((m1.double() - mfold).abs().max())
    print(f"dw_gram {case}: attn old {ea0:.3e} new {ea1:.3e}  mfold old {em0:.3e} new {em1:.3e}")
    assert ea1 <= 2.0 * ea0 and em1 <= 2.0 * em0
    assert float((a0 - a1).abs().max()) <= 2e-6 and float((m0 - m1).abs().max()) <= 2e-6


# =========================================================================== InstanceNorm
def plane(kind, tag, B, C, H, W):
    """constant: every plane one dyadic value of its own; hot: the same with one pixel at 100; offset: 1024 + 2^-3 x integer
    noise in [-8, 8] (mean^2 about 6e7 times the variance: a one-pass E[x^2] - mean^2 in fp32 has no bits left); border: constant up
    to a one-pixel border (what a checkered frame leaves behind the stride-2 stem of FPN-MobileNet)."""
    base = (torch.arange(B * C, dtype=torch.float32).view(B, C, 1, 1) % 7 - 3.0) * 0.25
    if kind == "constant":
        return base.expand(B, C, H, W).contiguous()
    if kind == "hot":
        x = base.expand(B, C, H, W).contiguous()
        x[:, :, H // 2, W // 3] = 100.0
        return x
    if kind == "border":
        x = base.expand(B, C, H, W).contiguous()
        x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = x[:, :, 0] + 0.125, x[:, :, -1] - 0.25, x[:, :, :, 0] + 0.5, x[:, :, :, -1] - 0.125
        return x
    return 1024.0 + 0.125 * torch.round(rnd(tag, (B, C, H, W), -8.0, 8.0))


PLANES = ("constant", "hot", "offset", "border")


@pytest.mark.parametrize("kind", PLANES)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("affine", [True, False])
def test_chan_norm(dev, affine, res, kind):
    """test_chan_norm's (1, 24, 23, 41): 943 pixels, an odd count over several passes of a 256-thread workgroup; TOL 2e-4."""
    B, C, H, W = 1, 24, 23, 41
    x = plane(kind, f"cn{kind}", B, C, H, W)
    w, b = rnd("cnw", (C,), 0.5, 1.5), rnd("cnb", (C,))
    r = rnd("cnr", (B, C, H, W))
    ref = F.instance_norm(x.double(), None, None, w.double() if affine else None, b.double() if affine else None, True, 0.1, 1e-5)
    if kind == "constant":
        assert float((ref - (b.double().view(1, C, 1, 1) if affine else 0.0)).abs().max()) <= 1e-12      # output = b[c], or 0
    if res:
        ref = ref + r.double()
    xg = x.to(dev)
    st = torch.empty(B, C, 2, device=dev)
    _hip.call("irm_chan_stats_f32", _hip.ptr(xg), xg.stride(0), _hip.ptr(st), B, C, H * W, 1e-5)
    st2 = torch.empty(B, C, 2, device=dev)
    ops.chan_stats(xg, st2)
    assert torch.equal(st, st2)                              # a plane this small takes the single-workgroup kernel either way
    ops.chan_norm_act(xg, st, xg, weight=w.to(dev) if affine else None, bias=b.to(dev) if affine else None,
                      res=r.to(dev) if res else None)
    err = float((xg.cpu().double() - ref).abs().max())
    print(f"chan_norm {kind} affine{int(affine)} res{int(res)}: {err:.3e}")
    assert err < FPN_TOL


@pytest.mark.parametrize("kind", PLANES)
def test_chan_stats_split_planes(dev, kind):
    """test_chan_stats_split_planes' (1, 8, 96, 128): three slices per plane merged by Chan's formula; its bars (mean abs
    1e-5 max(1, |x|max), rstd rel 1e-4), bit-identical on a second run."""
    B, C, H, W = 1, 8, 96, 128
    x = plane(kind, f"cs{kind}", B, C, H, W)
    xg = x.to(dev)
    st, st2 = torch.empty(B, C, 2, device=dev), torch.empty(B, C, 2, device=dev)
    ops.chan_stats(xg, st)
    ops.chan_stats(xg, st2)
    assert torch.equal(st, st2)
    xd = x.double().reshape(B, C, -1)
    mean, var = xd.mean(-1), xd.var(-1, unbiased=False)
    got = st.cpu().double()
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    e_m, e_r = float((got[..., 0] - mean).abs().max()), float(((got[..., 1] - rstd).abs() / rstd).max())
    print(f"chan_stats split {kind}: mean abs {e_m:.3e}  rstd rel {e_r:.3e}")
    assert e_m < 1e-5 * max(1.0, float(x.abs().max())) and e_r < 1e-4
    if kind == "constant":
        assert torch.equal(st.cpu()[..., 0], x[:, :, 0, 0])


# =========================================================================== selective scan + combine
# B, D, N, R, H, W, chunk: test_selective_scan_vs_oracle's (1, 192, 8, 6, 32, 32) at its one chunk of 1024 and at 32 chunks of 32
# (the 16-group carry walks two chunks per group), its ragged (1, 96, 4, 3, 5, 7, 32), and the flat lane mapping at MaIR's pairs
# (test_selective_scan_mair_pairs_vs_float64: N = 1 with D = 66, N = 16 with D = 90, 240 steps = 4 x 56 + 16)
SCANS = [(1, 192, 8, 6, 32, 32, 1024), (1, 192, 8, 6, 32, 32, 32), (1, 96, 4, 3, 5, 7, 32), (1, 66, 1, 4, 12, 20, 56),
         (1, 90, 16, 4, 12, 20, 56)]
SCAN_CASES = ("u_zero", "proj_zero", "constant", "dt_pm30")


def scan_degenerate(case, tag, B, D, N, R, L):
    """The synthetic regime of scan_model.scan_inputs with one degenerate edit."""
    x, proj, dtw, dtb, A, Ds = scan_model.scan_inputs(tag, "synthetic", B, D, N, R, L)
    if case == "u_zero":
        x = torch.zeros_like(x)
    elif case == "proj_zero":
        proj = torch.zeros_like(proj)
    elif case == "constant":
        x = x[:, :, :1].expand(B, D, L).contiguous()
        proj = proj[:, :, :, :1].expand(B, 4, R + 2 * N, L).contiguous()
    elif case == "dt_pm30":
        # raw dt + bias exactly +30 / -30: both softplus tails, where 1 + exp(-|x|) rounds to 1 (the dd == 0 arm)
        dtw = torch.zeros_like(dtw)
        dtw[:, :, 0] = 1.0
        dtb = torch.zeros_like(dtb)
        proj[:, :, 0] = torch.where(rnd(tag + "sg", (B, 4, L)) > 0, 30.0, -30.0)
    return x, proj, dtw, dtb, A, Ds


@pytest.mark.parametrize("case", SCAN_CASES)
@pytest.mark.parametrize("B,D,N,R,H,W,chunk", SCANS)
def test_selective_scan(dev, B, D, N, R, H, W, chunk, case):
    L = H * W
    assert ops.scan_is_flat(D, N, R) == (D in (66, 90))
    ids, inv = mair_ref.scan_ids(H, W, 4)
    tag = f"dz{D}{N}{case}"
    x, proj, dtw, dtb, A, Ds = scan_degenerate(case, tag, B, D, N, R, L)
    yT, ysum, nchunk = scan_model.run_scan(dev, x, proj, dtw, dtb, A, Ds, ids, B, L, D, N, R, chunk)
    got = yT.cpu().permute(0, 1, 3, 2)                      # (B, 4, D, L) pixel order
    assert torch.isfinite(got).all()
    sums = ysum.cpu().sum(3).reshape(B, 4, -1)[:, :, :D]
    if case == "u_zero":
        assert not bool(got.any()) and not bool(sums.any()), "u == 0 must give y == 0 and ysum == 0 exactly"
    if case == "proj_zero":
        want = Ds.view(1, 4, D, 1) * x.view(B, 1, D, L)
        assert torch.equal(got, want), "a zero projection must give y = D u exactly"
    if case != "u_zero":                                     # (0 = 0 there: the bar's e_32 is 0 too)
        scan_model.check_scan_f64(f"{case} D{D} N{N} L{L} chunk{chunk}", x, proj, dtw, dtb.reshape(4, D), A, Ds, ids, inv, got,
                              ysum.cpu(), B, L, D, N, R, chunk)


def test_losh_combine_zero_y(dev):
    """test_losh_combine's shape with y == 0: the LayerNorm over D sees zeros (var == 0), so out = nb silu(z) and the gate is
    sigmoid(gb); its bars (gate 1e-5, out 2e-4)."""
    B, D, H, W, nchunk = 2, 96, 8, 12, 3
    L = H * W
    zfull = rnd("cz", (B, D + 3, H, W))
    gw, gb = rnd("cgw", (4 * D, 4), -2, 2), rnd("cgb", (4 * D,))
    nw, nb = rnd("cnw", (D,), 0.5, 1.5), rnd("cnb", (D,), -0.2, 0.2)
    g = torch.sigmoid(gb.double().view(D, 4).t()).expand(B, 4, D)
    ref = nb.double().view(1, D, 1) * F.silu(zfull[:, 1:1 + D].double().reshape(B, D, L))
    gate = torch.empty(B, 4, D, device=dev)
    out = torch.empty(B, D, H, W, device=dev)
    ops.losh_combine(torch.zeros(B, 4, 2, nchunk, 64, device=dev), gw.to(dev), gb.to(dev), gate, torch.zeros(B, 4, L, D, device=dev),
                     nw.to(dev), nb.to(dev), zfull.to(dev)[:, 1:1 + D], out, B, L, D, nchunk)
    e_g, e_o = float((gate.cpu().double() - g).abs().max()), float((out.cpu().double().reshape(B, D, L) - ref).abs().max())
    print(f"combine y == 0: gate {e_g:.3e}  out {e_o:.3e}")
    assert e_g < 1e-5 and e_o < 2e-4


def test_every_listed_entry_point_ran(request):
    """Every entry point of the families above was launched by a degenerate case.  Only meaningful when the whole module ran."""
    ran = {it.originalname for it in request.session.items if it.module is request.module}
    if ran != {n for n in vars(request.module) if n.startswith("test_")}:
        pytest.skip("only part of the module was selected")
    assert not sorted(LISTED - _REACHED), f"entry points no degenerate case launched: {sorted(LISTED - _REACHED)}"
