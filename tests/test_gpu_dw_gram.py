"""GPU tests of dw_gram (irm_dw_gram_cm_f16x3_f32, dw_gram.hip): the depth-wise conv of q, k inside the Gram pass at the
levels with 48 channels per head (C = 192, 384), against float64 and against the two-kernel path it replaces
(dwconv3x3 + mdta_gram_f16x3) on the same inputs.

Shapes (every case at B = 2, with and without the depth-wise bias):
  C 192, 4 heads, 32 x 32    4 tiles = one chunk per (image, head); every tile lies on two or three borders
  C 192, 4 heads, 16 x 128   8 tiles = two chunks; interior vertical and horizontal tile seams
  C 384, 8 heads, 32 x 32    the C = 384 level
The inputs of a case (and the float64 reference, and both paths' results) are computed once and shared by its tests."""
import functools

import pytest
import torch
import torch.nn.functional as F

import block_model as bm
from block_model import unpack_mfold
from guards import SLACK, Guards, clean, guarded_fold, has_nan
from irm_amd import _hip, ops, restormer, synth
from oracle import restormer_ref

pytestmark = pytest.mark.gpu

SHAPES = [(192, 4, 32, 32), (192, 4, 16, 128), (384, 8, 32, 32)]
CASES = [(C, heads, H, W, bias) for (C, heads, H, W) in SHAPES for bias in (True, False)]
B = 2
SENTINEL = 7.0


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(321, name, shape, lo, hi)


@functools.lru_cache(maxsize=None)
def inputs(C, heads, H, W, bias):
    """rnd operands as in test_qkv_gram_cm_c48; the raw qkv standing in for the GEMM output is W LN(x) in float64, rounded to
    float32 (it obeys the static bound the operand scales are built from); float64 attention and folded matrix."""
    tag = f"dg{C}_{H}_{W}_{int(bias)}"
    M = 3 * C
    x = rnd(tag + "x", (B, C, H, W), -1.5, 2.0).double()
    lnw, lnb = rnd(tag + "lw", (C,), 0.5, 1.5), rnd(tag + "lb", (C,), -0.2, 0.2)
    w, dw_w = rnd(tag + "w", (M, C), -0.3, 0.3), rnd(tag + "dw", (M, 9), -0.4, 0.4)
    dw_b = rnd(tag + "dwb", (M,), -0.3, 0.3) if bias else None
    temp, wout = rnd(tag + "t", (heads,), 2.0, 6.0), rnd(tag + "wo", (C, C), -0.3, 0.3)
    gs = _hip.gram_scales(w.view(M, C, 1, 1), None, dw_w.view(M, 1, 3, 3), dw_b, lnw, lnb, True)
    xn = restormer_ref.layer_norm_c(x, lnw.double(), lnb.double())
    raw = F.conv2d(xn, w.double()[:, :, None, None]).float()
    qk = F.conv2d(raw.double()[:, :2 * C], dw_w.double()[:2 * C].view(2 * C, 1, 3, 3), None if dw_b is None else dw_b.double()[:2 * C],
                  padding=1, groups=2 * C)
    attn = bm.attention_qk(qk, temp, heads)
    mfold = torch.stack([wout.double() @ torch.block_diag(*attn[i]) for i in range(B)])
    return dict(raw=raw, dw_w=dw_w, dw_b=dw_b, gs=gs, temp=temp, wout=wout, attn=attn, mfold=mfold)


def run(dev, C, heads, H, W, bias, new, nb=B):
    """(attention [nb][heads][48][48], folded matrix [nb][C][C], qkv2, part) of the old or the new path on images [0, nb)."""
    d = inputs(C, heads, H, W, bias)
    N = H * W
    qkv = d["raw"][:nb].to(dev).contiguous()
    dw_w, dw_b, gs = d["dw_w"].to(dev), None if d["dw_b"] is None else d["dw_b"].to(dev), d["gs"].to(dev)
    temp, wout = d["temp"].to(dev), d["wout"].to(dev)
    qkv2 = torch.full((nb, 3 * C, H, W), SENTINEL, device=dev)
    _, nchunk, rec = ops.mdta_plan(nb, C, heads, N)
    nready = None
    if new:
        nchunk = (H // 8) * (W // 32) // ops.QKV_GRAM_NCH
    part = torch.full((nb * heads * nchunk * rec,), float("nan"), device=dev)
    if new:
        nready = ops.dw_gram(qkv, dw_w[:2 * C], gs, part, C, heads, bias=None if dw_b is None else dw_b[:2 * C])
        assert nready == nchunk
        ops.dwconv3x3(qkv[:, 2 * C:], dw_w[2 * C:], qkv2[:, 2 * C:], bias=None if dw_b is None else dw_b[2 * C:])
    else:
        ops.dwconv3x3(qkv, dw_w, qkv2, bias=dw_b)
    gsum = torch.empty(nb * heads * rec, device=dev)
    mfold = torch.zeros(nb * ops.mfold_numel(C), device=dev)
    attn = torch.empty(nb, heads, 48, 48, device=dev)
    ops.mdta_fold(qkv2, part, gsum, temp, wout, mfold, C, heads, attn=attn, gram_scale=gs, nchunk_ready=nready)
    return attn.cpu(), unpack_mfold(mfold.cpu(), nb, C), qkv2.cpu(), part.cpu()


@functools.lru_cache(maxsize=None)
def results(dev, C, heads, H, W, bias):
    return run(dev, C, heads, H, W, bias, False), run(dev, C, heads, H, W, bias, True)


@pytest.mark.parametrize("C,heads,H,W,bias", CASES)
def test_dw_gram_vs_float64(dev, C, heads, H, W, bias):
    """Attention and folded matrix of the new path against float64 (zero-padded depth-wise conv, normalise, softmax with
    temperature, fold with wout).  Bound: twice the error of today's two-kernel path against the same float64 result on the
    same inputs - the new path only changes the fp32 summation order of the same fp16x3 products.
    Measured on the MI355X, max-abs error against float64 (old path = dwconv3x3 + mdta_gram_f16x3, new path = dw_gram):
        C, H x W, bias       attention old / new        folded matrix old / new
        192, 32 x 32, yes    6.791e-09 / 7.958e-09      2.876e-08 / 3.548e-08
        192, 32 x 32, no     7.658e-09 / 8.006e-09      3.370e-08 / 3.370e-08
        192, 16 x 128, yes   1.019e-08 / 9.620e-09      3.191e-08 / 3.191e-08
        192, 16 x 128, no    7.587e-09 / 8.546e-09      2.982e-08 / 2.631e-08
        384, 32 x 32, yes    1.541e-08 / 1.150e-08      3.694e-08 / 3.694e-08
        384, 32 x 32, no     8.685e-09 / 8.452e-09      3.969e-08 / 3.969e-08"""
    assert ops.can_dw_gram(C, heads, H, W)
    d = inputs(C, heads, H, W, bias)
    (a0, m0, _, _), (a1, m1, _, _) = results(dev, C, heads, H, W, bias)
    ea0, ea1 = float((a0.double() - d["attn"]).abs().max()), float((a1.double() - d["attn"]).abs().max())
    em0, em1 = float((m0.double() - d["mfold"]).abs().max()), float((m1.double() - d["mfold"]).abs().max())
    print(f"dw_gram C{C} {H}x{W} bias{int(bias)}: attn old {ea0:.3e} new {ea1:.3e}  mfold old {em0:.3e} new {em1:.3e}")
    assert ea1 <= 2.0 * ea0 and em1 <= 2.0 * em0, (ea0, ea1, em0, em1)


@pytest.mark.parametrize("C,heads,H,W,bias", CASES)
def test_dw_gram_vs_two_kernel_path(dev, C, heads, H, W, bias):
    """The same inputs through dwconv3x3 + mdta_gram_f16x3: the tolerance of test_qkv_gram_cm_c48 (2e-6 on the attention and
    on the folded matrix, same input ranges).  dw(q), dw(k) are never written (their part of qkv2 keeps its pre-fill), v is
    bit-identical to the three-way launch's, and no record element keeps the NaN pre-fill of `part`."""
    (a0, m0, y0, _), (a1, m1, y1, part) = results(dev, C, heads, H, W, bias)
    assert float((a0 - a1).abs().max()) <= 2e-6 and float((m0 - m1).abs().max()) <= 2e-6, \
        (float((a0 - a1).abs().max()), float((m0 - m1).abs().max()))
    assert bool((y1[:, :2 * C] == SENTINEL).all()), "q, k must not be written"
    assert torch.equal(y1[:, 2 * C:], y0[:, 2 * C:]), "v differs from the three-way depth-wise launch"
    assert not bool(torch.isnan(part).any())


@pytest.mark.parametrize("C,heads,H,W,bias", CASES)
def test_dw_gram_batch_independent_and_deterministic(dev, C, heads, H, W, bias):
    _, (a1, m1, _, p1) = results(dev, C, heads, H, W, bias)
    a2, m2, _, p2 = run(dev, C, heads, H, W, bias, True)
    assert torch.equal(a1, a2) and torch.equal(m1, m2) and torch.equal(p1, p2), "two runs differ"
    a3, m3, _, _ = run(dev, C, heads, H, W, bias, True, nb=1)
    assert torch.equal(a3[0], a1[0]) and torch.equal(m3[0], m1[0]), "depends on the batch"


def test_dw_gram_entry_checks(dev):
    C, heads, H, W = 192, 4, 32, 32
    qkv, taps, gs = torch.zeros(1, 3 * C, 32, 128, device=dev), torch.zeros(2 * C, 9, device=dev), torch.ones(2 * C, device=dev)
    part = torch.zeros(heads * 4 * 2400, device=dev)
    fn = _hip.load().irm_dw_gram_cm_f16x3_f32
    stream = torch.cuda.current_stream().cuda_stream

    def rc(C=C, heads=heads, H=H, W=W, part=part):
        return fn(qkv.data_ptr(), 3 * C * H * W, taps.data_ptr(), None, gs.data_ptr(), None if part is None else part.data_ptr(),
                  1, C, heads, H, W, stream)
    assert rc() == 0
    assert rc(heads=2) == -1 and rc(heads=5) == -1          # C / heads != 48
    assert rc(H=36) == -1 and rc(H=28) == -1                # H % 8 != 0
    assert rc(W=48) == -1                                   # W % 32 != 0
    assert rc(H=24) == -1 and rc(H=8, W=96) == -1           # 3 tiles: not a multiple of the chunk
    assert rc(part=None) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("new", [True, False])
def test_transformer_block_c192_with_and_without_dw_gram(dev, monkeypatch, new):
    """One C = 192 TransformerBlock (WithBias LayerNorm: the Gram pass has its operand scales) at 32 x 32 through
    Restormer._block on the product packing, with the new path and with ops.can_dw_gram patched to False, against the float64
    oracle of the block; the tolerance of test_transformer_block_vs_golden (2e-4)."""
    import torch.nn as nn
    c, heads, h, w = 192, 4, 32, 32
    host = restormer.Restormer(LayerNorm_type="WithBias")
    blk = restormer.restormer.TransformerBlock(c, heads, 2.66, False, "WithBias")
    shapes = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
    blk.load_state_dict(synth.synth_state_dict(shapes, seed=11, rules=restormer.restormer.SYNTH_RULES))
    host.encoder_level1 = nn.Sequential(blk)
    host = host.to(dev)
    wt = host._pack()["encoder_level1.0"]
    assert host._split and "gram_s" in wt and "qk_dw" in wt and ops.can_dw_gram(c, heads, h, w)
    ran = []
    real = ops.dw_gram
    monkeypatch.setattr(ops, "dw_gram", lambda *a, **k: (ran.append(1), real(*a, **k))[1])
    if not new:
        monkeypatch.setattr(ops, "can_dw_gram", lambda *a: False)
    x = synth.uniform(7, "dg_tb_in", (2, c, h, w), -1.0, 1.0)
    y = x.to(dev).clone()
    host._block(blk, wt, y)
    assert bool(ran) == new
    with torch.no_grad():
        ref = restormer_ref.transformer_block(x.double(), {k: v.detach().cpu().double() for k, v in blk.state_dict().items()}, "", heads)
    err = float((y.cpu().double() - ref).abs().max())
    print(f"block c192 32x32 dw_gram={new}: max-abs vs float64 oracle {err:.3e}")
    assert err <= 2e-4


def test_dw_gram_guard_bands(dev):
    """irm_dw_gram_cm_f16x3_f32 between guard bands (tests/guards.py), the rule of tests/test_gpu_guard_bands.py: C = 192,
    4 heads, 32 x 32 (4 tiles = one record per image and head: the smallest can_dw_gram admits; every tile on two or three
    borders), B = 2 with batch slack.  qkv holds the q, k planes ONLY, between NaN bands: a halo read one pixel before a
    plane's row, past its end or past the k planes poisons a record.  part at exactly B heads nchunk 2400 floats between
    sentinels.  The attention matrix of the records against float64 (bar of test_mdta_fold, 2e-5)."""
    nb, C, heads, H, W = 2, 192, 4, 32, 32
    assert ops.can_dw_gram(C, heads, H, W)
    raw, dw_w, dw_b = rnd("dgq", (nb, 2 * C, H, W), -1.0, 1.0), rnd("dgw", (2 * C, 9), -0.4, 0.4), rnd("dgb", (2 * C,), -0.3, 0.3)
    gs = torch.full((2 * C,), 4096.0)                    # |dw(raw)| <= 9 * 0.4 + 0.3: far inside the fp16 range at 2^12
    temp, wout = rnd("dgt", (heads,), 2.0, 6.0), rnd("dgwo", (C, C), -0.3, 0.3)
    ref = F.conv2d(raw.double(), dw_w.double().view(2 * C, 1, 3, 3), dw_b.double(), padding=1, groups=2 * C)
    nchunk = (H // 8) * (W // 32) // ops.QKV_GRAM_NCH
    g = Guards(dev)
    qkv, part = g.inp(raw, SLACK), g.out("part", (nb * heads * nchunk * (48 * 48 + 96),))
    gsc = g.inp(gs)
    assert ops.dw_gram(qkv, g.inp(dw_w), gsc, part, C, heads, bias=g.inp(dw_b)) == nchunk
    g.check()
    assert not has_nan(part.cpu())
    attn, _ = guarded_fold(g, qkv, nb, C, heads, H * W, g.inp(temp), g.inp(wout), part=part, nready=nchunk, gram_scale=gsc)
    g.check()
    assert float((clean(attn).double() - bm.attention_qk(ref, temp, heads)).abs().max()) < 2e-5
