"""GPU parity tests of the individual HIP kernels (through the C ABI) against
plain PyTorch fp32/fp64 references of the same op computed on the CPU.

Tolerances: fp32 kernels vs an fp64 reference, absolute 2e-4 on O(1) data
(the path's end-to-end budget is 1e-3 max-abs, BASELINE.json north_star)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_model as bm
import guards
from block_model import OPS_TOL as TOL
from block_model import unpack_gemm, unpack_presplit
from irm_amd import _hip, ops, synth

pytestmark = pytest.mark.gpu


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(123, name, shape, lo, hi)


def test_pack_roundtrip_cpu_side():
    w = rnd("w", (37, 29))
    assert torch.equal(unpack_gemm(_hip.pack_gemm_weight(w), 37, 29), w)


@pytest.mark.parametrize("B,C,H,W", [(1, 48, 8, 16), (2, 96, 12, 20), (3, 7, 4, 4), (1, 384, 8, 8), (2, 48, 5, 7)])
def test_ln_stats(dev, B, C, H, W):
    big = rnd(f"ln{B}{C}", (B, C + 5, H, W), -2, 3)
    xb = big.to(dev)
    x = xb[:, 2:2 + C]                         # channel slice: batch stride != C*H*W
    stats = torch.empty(B, 2, H * W, device=dev)
    ops.ln_stats(x, stats, 1e-5)
    xr = big[:, 2:2 + C].double()
    mean, rstd = (s.reshape(B, -1) for s in bm.ln_stats(xr))
    s = stats.cpu().double()
    assert (s[:, 0] - mean).abs().max() < 1e-5
    assert ((s[:, 1] - rstd).abs() / rstd).max() < 1e-5


GEMM_CASES = [
    # M, K, H, W, B, ln, res, bias, act, ct, yg
    (144, 48, 16, 24, 2, 1, False, False, 0, None, None),
    (144, 48, 16, 24, 1, 2, False, False, 0, 3, 2),
    (48, 48, 8, 8, 2, 0, True, False, 0, None, None),
    (254, 48, 16, 16, 1, 1, False, False, 0, None, None),
    (48, 127, 16, 16, 2, 0, True, False, 0, None, None),
    (96, 255, 8, 24, 1, 0, True, True, 0, None, None),
    (288, 96, 16, 24, 1, 2, False, False, 0, None, 1),
    (510, 96, 8, 16, 2, 1, False, True, 0, 8, 3),
    (192, 384, 8, 8, 2, 0, False, False, 0, None, None),
    (1152, 384, 8, 8, 1, 1, False, False, 0, None, None),
    (2042, 384, 8, 8, 1, 2, False, False, 0, None, None),
    (384, 1021, 8, 8, 2, 0, True, False, 0, None, None),
    (40, 20, 4, 12, 1, 0, False, True, 2, 4, None),
    (33, 50, 4, 12, 1, 0, True, True, 1, 6, None),
    (64, 64, 12, 12, 1, 0, False, True, 3, 9, None),
    (1152, 384, 5, 7, 2, 1, False, False, 0, None, None),     # odd N: scalar path
    (384, 1021, 5, 7, 1, 0, True, False, 0, None, None),
    (96, 48, 9, 15, 1, 2, True, True, 0, None, None),
]


@pytest.mark.parametrize("M,K,H,W,B,ln,res,bias,act,ct,yg", GEMM_CASES)
def test_gemm1x1(dev, M, K, H, W, B, ln, res, bias, act, ct, yg):
    tag = f"g{M}_{K}_{H}_{W}_{B}_{ln}"
    w = rnd(tag + "w", (M, K), -0.3, 0.3)
    x = rnd(tag + "x", (B, K, H, W), -1.5, 2.0)
    r = rnd(tag + "r", (B, M, H, W)) if res else None
    bv = rnd(tag + "b", (M,)) if bias else None
    lnw = rnd(tag + "lw", (K,), 0.5, 1.5)
    lnb = rnd(tag + "lb", (K,), -0.2, 0.2)
    ref = torch.einsum("mk,bkhw->bmhw", w.double(), bm.layer_norm(x.double(), lnw, lnb, ln))
    if bias:
        ref = ref + bv.double().view(1, -1, 1, 1)
    ref = bm.act(ref, act)
    if res:
        ref = ref + r.double()

    xg = x.to(dev)
    stats = None
    if ln:
        stats = torch.empty(B, 2, H * W, device=dev)
        ops.ln_stats(xg, stats)
    ybig = torch.full((B, M + 3, H, W), 7.0, device=dev)     # write into a channel slice
    y = ybig[:, 1:1 + M]
    ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), xg, y, M, K, res=r.to(dev) if res else None,
                bias=bv.to(dev) if bias else None, stats=stats, lnw=lnw.to(dev) if ln else None,
                lnb=lnb.to(dev) if ln == 1 else None, ln_mode=ln, act=act, ct=ct, ygroups=yg)
    got = ybig.cpu().double()
    assert (got[:, 1:1 + M] - ref).abs().max() < TOL * max(1.0, float(ref.abs().max()))
    assert torch.all(got[:, 0] == 7.0) and torch.all(got[:, 1 + M:] == 7.0)     # no stray writes


@pytest.mark.parametrize("M,K,H,W,B,res", [(96, 255, 16, 24, 2, True), (48, 48, 8, 16, 1, True), (144, 96, 16, 16, 1, False),
                                           (96, 96, 5, 7, 2, True), (40, 30, 8, 8, 1, True)])
def test_gemm1x1_fused_output_statistics(dev, M, K, H, W, B, res):
    """stats_out = LayerNorm statistics of the GEMM result (incl. residual) for the next LayerNorm."""
    tag = f"fs{M}_{K}_{H}"
    w = rnd(tag + "w", (M, K), -0.3, 0.3)
    x = rnd(tag + "x", (B, K, H, W), -1.5, 2.0)
    r = rnd(tag + "r", (B, M, H, W), -3, 3) if res else None
    ref = torch.einsum("mk,bkhw->bmhw", w.double(), x.double()) + (r.double() if res else 0)
    mean, rstd = (s.reshape(B, -1) for s in bm.ln_stats(ref))
    y = torch.empty(B, M, H, W, device=dev)
    st = torch.full((B, 2, H * W), float("nan"), device=dev)
    ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), x.to(dev), y, M, K, res=r.to(dev) if res else None, stats_out=st)
    assert (y.cpu().double() - ref).abs().max() < TOL * max(1.0, float(ref.abs().max()))
    s = st.cpu().double()
    assert (s[:, 0] - mean).abs().max() < 1e-5 * max(1.0, float(mean.abs().max()))
    assert ((s[:, 1] - rstd).abs() / rstd).max() < 1e-5
    # and against the standalone statistics kernel on the same tensor
    st2 = torch.empty(B, 2, H * W, device=dev)
    ops.ln_stats(y, st2)
    assert (st2 - st).abs().max() < 1e-5


def test_gemm1x1_inplace_residual_and_per_batch_weights(dev):
    B, C, H, W = 3, 96, 8, 16
    x = rnd("ipx", (B, C, H, W))
    v = rnd("ipv", (B, C, H, W))
    wb = rnd("ipw", (B, C, C), -0.2, 0.2)
    packed = torch.stack([_hip.pack_gemm_weight(wb[b]) for b in range(B)]).to(dev)
    xg = x.to(dev).clone()
    ops.gemm1x1(packed, v.to(dev), xg, C, C, res=xg, w_bs=packed.shape[1])
    ref = x.double() + torch.einsum("bmk,bkhw->bmhw", wb.double(), v.double())
    assert (xg.cpu().double() - ref).abs().max() < TOL * 4


@pytest.mark.parametrize("B,C,H,W,bias,act", [(2, 144, 16, 24, False, 0), (1, 7, 5, 8, True, 3), (1, 48, 64, 64, False, 0),
                                               (2, 30, 9, 12, True, 0), (2, 33, 5, 7, False, 0), (1, 8, 17, 10, True, 3)])
def test_dwconv3x3(dev, B, C, H, W, bias, act):
    x = rnd(f"dw{C}{H}", (B, C, H, W))
    w = rnd(f"dww{C}", (C, 1, 3, 3))
    bv = rnd(f"dwb{C}", (C,)) if bias else None
    ref = F.conv2d(x.double(), w.double(), bv.double() if bias else None, padding=1, groups=C)
    if act == 3:
        ref = F.silu(ref)
    y = torch.empty(B, C, H, W, device=dev)
    ops.dwconv3x3(x.to(dev), w.reshape(C, 9).to(dev), y, bias=bv.to(dev) if bias else None, act=act)
    assert (y.cpu().double() - ref).abs().max() < TOL


@pytest.mark.parametrize("B,hid,H,W", [(2, 127, 16, 24), (1, 255, 8, 8), (1, 5, 3, 4), (2, 1021, 5, 7)])
def test_dwconv3x3_gate(dev, B, hid, H, W):
    x = rnd(f"gt{hid}", (B, 2 * hid, H, W), -2, 2)
    w = rnd(f"gtw{hid}", (2 * hid, 1, 3, 3))
    d = F.conv2d(x.double(), w.double(), None, padding=1, groups=2 * hid)
    ref = F.gelu(d[:, :hid]) * d[:, hid:]
    y = torch.empty(B, hid, H, W, device=dev)
    ops.dwconv3x3_gate(x.to(dev), w.reshape(-1, 9).to(dev), y)
    assert (y.cpu().double() - ref).abs().max() < TOL


@pytest.mark.parametrize("M,K,H,W,B,ln,bias,ct", [(144, 48, 16, 24, 2, 1, False, 9), (510, 96, 16, 32, 1, 2, True, 8),
                                                  (254, 48, 8, 32, 2, 1, False, 8), (96, 255, 16, 16, 1, 0, True, 6),
                                                  (1020, 192, 8, 16, 2, 1, False, 8)])
def test_gemm1x1_f16x3(dev, M, K, H, W, B, ln, bias, ct):
    """fp32 emulation on the fp16 matrix cores (hi/lo split, three MFMAs): against float64 and against the
    exact-fp32 kernel - the emulation must stay at fp32 rounding level (2^-21 per product)."""
    N = H * W
    x = rnd(f"sx{M}{K}", (B, K, H, W), -2, 3)
    w = rnd(f"sw{M}{K}", (M, K), -0.3, 0.3)
    lnw, lnb = rnd(f"slw{K}", (K,), 0.5, 1.5), rnd(f"slb{K}", (K,), -0.2, 0.2)
    bv = rnd(f"sb{M}", (M,), -0.3, 0.3) if bias else None
    ref = torch.einsum("mk,bkhw->bmhw", w.double(), bm.layer_norm(x.double(), lnw, lnb, ln))
    if bias:
        ref = ref + bv.double().view(1, M, 1, 1)
    xg = x.to(dev)
    st = torch.empty(B, 2, N, device=dev)
    if ln:
        ops.ln_stats(xg, st)
    kw = dict(bias=bv.to(dev) if bias else None, stats=st if ln else None, lnw=lnw.to(dev) if ln else None,
              lnb=lnb.to(dev) if ln == 1 else None, ln_mode=ln, ct=ct)
    y16, y32 = torch.empty(B, M, H, W, device=dev), torch.empty(B, M, H, W, device=dev)
    ops.gemm1x1(_hip.pack_gemm_weight_split(w).to(dev), xg, y16, M, K, split=True, **kw)
    ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), xg, y32, M, K, **kw)
    e16 = (y16.cpu().double() - ref).abs().max().item()
    e32 = (y32.cpu().double() - ref).abs().max().item()
    print(f"M{M} K{K}: max-abs vs float64  f16x3 {e16:.3e}   f32 {e32:.3e}")
    assert e16 < 2e-5 and e16 < 8 * max(e32, 1e-7)


@pytest.mark.parametrize("K,H,W,B,ln,amp", [(192, 16, 16, 2, 1, 1.0), (192, 16, 32, 1, 2, 1.0), (384, 8, 16, 3, 1, 1.0),
                                            (384, 16, 8, 1, 2, 1e-4), (192, 16, 16, 1, 1, 3e4)])
def test_ln_split(dev, K, H, W, B, ln, amp):
    """irm_ln_split_f16: hi + lo of LayerNorm(x) * s_x in fragment order against float64, from a channel slice of a
    larger buffer; LayerNorm gains up to 30 (the static scale keeps every value inside fp16)."""
    N = H * W
    big = rnd(f"lsx{K}{H}{ln}", (B, K + 3, H, W), -2, 3) * amp
    lnw = rnd(f"lsw{K}{ln}", (K,), 0.05, 30.0)
    lnb = rnd(f"lsb{K}{ln}", (K,), -2.0, 2.0) if ln == 1 else None
    x = big.to(dev)[:, 2:2 + K]
    s_x = _hip.ln_split_scale(lnw, lnb, K, ln == 1)
    xs = torch.full((B * K * N + 64,), float("nan"), device=dev)
    ops.ln_split(x, xs, lnw.to(dev), lnb.to(dev) if ln == 1 else None, ln, s_x)
    assert torch.isnan(xs[B * K * N:]).all()                                   # nothing written past the image
    got = unpack_presplit(xs[:B * K * N].cpu(), B * N, K).view(B, N, K).permute(0, 2, 1).reshape(B, K, H, W) / s_x
    ref = bm.layer_norm(big[:, 2:2 + K].double(), lnw, lnb, ln)
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    print(f"ln_split K{K} ln{ln} amp{amp:g}: s_x {s_x:g}  |ref|max {scale:.3e}  max-abs {err:.3e}")
    assert torch.isfinite(got).all() and err <= 4e-7 * scale + 1e-9


PS_CASES = [   # M, K, H, W, B, ln, bias, ct, mgroups, wg_shape
    (576, 192, 16, 16, 2, 1, True, 6, 2, 0), (1020, 192, 16, 32, 1, 2, False, 8, 2, 42), (1020, 192, 16, 16, 3, 1, True, 8, 3, 32),
    (1152, 384, 8, 16, 2, 1, False, 6, 4, 0), (2042, 384, 16, 8, 1, 2, True, 8, 4, 81), (2042, 384, 8, 16, 1, 1, False, 8, 3, 0),
    (576, 192, 16, 16, 1, 1, False, 6, 1, 32), (570, 192, 16, 16, 1, 1, True, None, None, 0), (1152, 384, 16, 24, 2, 1, True, None, None, 0),
    # pixel-tile counts that are no multiple of a workgroup's tiles (tail workgroup, workgroups straddling images)
    (576, 192, 12, 12, 3, 1, True, 6, 2, 42), (1020, 192, 12, 12, 3, 2, True, 8, 1, 32), (1020, 192, 12, 20, 5, 1, False, 4, 3, 43),
    (1152, 384, 12, 12, 3, 1, True, 8, 2, 81), (300, 192, 4, 4, 1, 1, True, 4, 1, 43),
]


@pytest.mark.parametrize("M,K,H,W,B,ln,bias,ct,mgroups,wg_shape", PS_CASES)
def test_gemm_presplit(dev, M, K, H, W, B, ln, bias, ct, mgroups, wg_shape):
    """LayerNorm + 1x1 conv with pre-split fp16 operands (irm_ln_split_f16 + irm_gemm_presplit_f16x3_f32) against
    float64 and against the exact-f32 kernel pair (ln_stats + irm_gemm1x1_f32): the emulation must stay at fp32 rounding
    level.  Output written into a channel slice of a sentinel-filled buffer (nothing outside it may change)."""
    N = H * W
    x = rnd(f"px{M}{K}{H}", (B, K, H, W), -2, 3)
    w = rnd(f"pw{M}{K}", (M, K), -0.3, 0.3)
    lnw = rnd(f"plw{K}", (K,), 0.5, 1.5)
    lnb = rnd(f"plb{K}", (K,), -0.2, 0.2) if ln == 1 else None
    bv = rnd(f"pb{M}", (M,), -0.3, 0.3) if bias else None
    ref = torch.einsum("mk,bkhw->bmhw", w.double(), bm.layer_norm(x.double(), lnw, lnb, ln))
    if bias:
        ref = ref + bv.double().view(1, M, 1, 1)
    xg = x.to(dev)
    frag, s_w = _hip.pack_gemm_weight_presplit(w.to(dev))
    assert float((unpack_presplit(frag.cpu(), M, K) / s_w - w.double()).abs().max()) <= 2.0 ** -21 * float(w.abs().max())
    s_x = _hip.ln_split_scale(lnw, lnb, K, ln == 1)
    xs = torch.empty(B * K * N, device=dev)
    ops.ln_split(xg, xs, lnw.to(dev), lnb.to(dev) if ln == 1 else None, ln, s_x)
    ybig = torch.full((B, M + 7, H, W), 777.0, device=dev)
    y16 = ybig[:, 3:3 + M]
    ops.gemm_presplit(frag, xs, y16, M, K, out_scale=1.0 / (s_w * s_x), bias=bv.to(dev) if bias else None, ct=ct,
                      mgroups=mgroups, wg_shape=wg_shape)
    assert (ybig[:, :3] == 777.0).all() and (ybig[:, 3 + M:] == 777.0).all()
    st = torch.empty(B, 2, N, device=dev)
    ops.ln_stats(xg, st)
    y32 = torch.empty(B, M, H, W, device=dev)
    ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), xg, y32, M, K, bias=bv.to(dev) if bias else None, stats=st,
                lnw=lnw.to(dev), lnb=lnb.to(dev) if ln == 1 else None, ln_mode=ln)
    e16 = (y16.cpu().double() - ref).abs().max().item()
    e32 = (y32.cpu().double() - ref).abs().max().item()
    print(f"presplit M{M} K{K} N{N} B{B} ln{ln}: max-abs vs float64  f16x3 {e16:.3e}   f32 {e32:.3e}")
    assert e16 < 2e-5 and e16 <= 2.0 * max(e32, 1e-7)
    # run-to-run bit identity
    y2 = torch.empty(B, M, H, W, device=dev)
    ops.gemm_presplit(frag, xs, y2, M, K, out_scale=1.0 / (s_w * s_x), bias=bv.to(dev) if bias else None, ct=ct,
                      mgroups=mgroups, wg_shape=wg_shape)
    assert torch.equal(y2, y16)


@pytest.mark.parametrize("M,H,W,B,ln,bias", [(576, 16, 16, 2, 1, True), (1020, 12, 12, 3, 2, False), (300, 4, 4, 1, 1, True),
                                             (1020, 32, 32, 6, 1, True)])
def test_ln_gemm_presplit_fused(dev, M, H, W, B, ln, bias):
    """irm_ln_gemm_presplit_f16x3_f32 (LayerNorm + split inside the GEMM's operand load, K = 192) against float64 and against
    the two-launch pair irm_ln_split_f16 + irm_gemm_presplit_f16x3_f32 (same operands and routine, not bit-identical: measured
    1.4e-6 ... 3.8e-6 apart, i.e. a few fp32 ulps of the sums, and equally close to float64 - the assertion is dd <= 1e-5), incl. tail workgroups and a sentinel-padded output."""
    K, N = 192, H * W
    big = rnd(f"lfx{M}{H}", (B, K + 2, H, W), -2, 3)
    x = big.to(dev)[:, 1:1 + K]
    w = rnd(f"lfw{M}", (M, K), -0.3, 0.3)
    lnw_c = rnd(f"lflw{M}", (K,), 0.5, 1.5)
    lnb_c = rnd(f"lflb{M}", (K,), -0.2, 0.2) if ln == 1 else None
    bv_c = rnd(f"lfb{M}", (M,), -0.3, 0.3) if bias else None
    lnw, lnb, bv = lnw_c.to(dev), None if lnb_c is None else lnb_c.to(dev), None if bv_c is None else bv_c.to(dev)
    ref = torch.einsum("mk,bkhw->bmhw", w.double(), bm.layer_norm(big[:, 1:1 + K].double(), lnw_c, lnb_c, ln))
    if bias:
        ref = ref + bv_c.double().view(1, M, 1, 1)
    frag, s_w = _hip.pack_gemm_weight_presplit(w.to(dev))
    s_x = _hip.ln_split_scale(lnw, lnb, K, ln == 1)
    xs = torch.empty(B * K * N, device=dev)
    ops.ln_split(x, xs, lnw, lnb, ln, s_x)
    y0 = torch.empty(B, M, H, W, device=dev)
    ops.gemm_presplit(frag, xs, y0, M, K, out_scale=1.0 / (s_w * s_x), bias=bv, ct=4, mgroups=1, wg_shape=43)
    y1 = torch.full((B, M + 2, H, W), 9.0, device=dev)
    _hip.call("irm_ln_gemm_presplit_f16x3_f32", _hip.ptr(frag), _hip.ptr(x), x.stride(0), _hip.ptr(lnw), _hip.ptr(lnb), ln,
              float(s_x), 1e-5, _hip.ptr(y1[:, 1:1 + M]), y1.stride(0), _hip.ptr(bv), float(1.0 / (s_w * s_x)), B, M, K, N, 1)
    assert (y1[:, 0] == 9.0).all() and (y1[:, -1] == 9.0).all()
    e0 = float((y0.cpu().double() - ref).abs().max())
    e1 = float((y1[:, 1:1 + M].cpu().double() - ref).abs().max())
    dd = float((y1[:, 1:1 + M] - y0).abs().max())
    print(f"LN-fused presplit M{M} N{N} B{B} ln{ln}: vs float64 fused {e1:.3e}, pair {e0:.3e}; fused vs pair {dd:.3e}")
    assert e1 < 2e-5 and e1 <= 1.5 * e0 + 1e-6 and dd <= 1e-5
    y2 = torch.empty(B, M, H, W, device=dev)
    _hip.call("irm_ln_gemm_presplit_f16x3_f32", _hip.ptr(frag), _hip.ptr(x), x.stride(0), _hip.ptr(lnw), _hip.ptr(lnb), ln,
              float(s_x), 1e-5, _hip.ptr(y2), y2.stride(0), _hip.ptr(bv), float(1.0 / (s_w * s_x)), B, M, K, N, 1)
    assert torch.equal(y2, y1[:, 1:1 + M])                        # run-to-run bit identity


def test_gemm_presplit_trained_like(dev):
    """Trained-like statistics: LayerNorm gains up to 30, weights spanning 1e-5 ... 10, activations x 1e-4 / 1 / 1e4 -
    power-of-two scales on both operands keep the emulation within 2x of the exact-f32 kernel pair."""
    M, K, H, W, B = 576, 192, 16, 16, 1
    N = H * W
    for ln in (1, 2):
        for amp in (1e-4, 1.0, 1e4):
            tag = f"pt{ln}{amp}"
            x = rnd(tag + "x", (B, K, H, W), -1.5, 2.0) * amp
            sign = torch.where(rnd(tag + "s", (M, K)) < 0, -1.0, 1.0)
            w = sign * torch.exp(rnd(tag + "w", (M, K), np.log(1e-5), np.log(10.0)))
            lnw = torch.exp(rnd(tag + "lw", (K,), np.log(0.1), np.log(30.0)))
            lnb = rnd(tag + "lb", (K,), -2.0, 2.0) if ln == 1 else None
            ref = torch.einsum("mk,bkhw->bmhw", w.double(), bm.layer_norm(x.double(), lnw, lnb, ln))
            xg = x.to(dev)
            frag, s_w = _hip.pack_gemm_weight_presplit(w.to(dev))
            s_x = _hip.ln_split_scale(lnw, lnb, K, ln == 1)
            xs = torch.empty(B * K * N, device=dev)
            ops.ln_split(xg, xs, lnw.to(dev), lnb.to(dev) if ln == 1 else None, ln, s_x)
            y16 = torch.empty(B, M, H, W, device=dev)
            ops.gemm_presplit(frag, xs, y16, M, K, out_scale=1.0 / (s_w * s_x))
            st = torch.empty(B, 2, N, device=dev)
            ops.ln_stats(xg, st)
            y32 = torch.empty(B, M, H, W, device=dev)
            ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), xg, y32, M, K, stats=st, lnw=lnw.to(dev),
                        lnb=lnb.to(dev) if ln == 1 else None, ln_mode=ln)
            scale = float(ref.abs().max())
            e16, e32 = float((y16.cpu().double() - ref).abs().max()), float((y32.cpu().double() - ref).abs().max())
            print(f"presplit trained-like ln{ln} x{amp:g}: |ref|max {scale:.3e}  f16x3 {e16:.3e}  f32 {e32:.3e}")
            assert torch.isfinite(y16).all() and e16 <= 2.0 * e32 + 4e-7 * scale


@pytest.mark.parametrize("M,K,H,W,B,scale", [(192, 510, 8, 16, 2, 1.0), (384, 1021, 8, 8, 1, 1.0), (96, 255, 16, 16, 1, 3000.0)])
def test_gemm1x1_f16x3_residual(dev, M, K, H, W, B, scale):
    """The emulated GEMM without the LayerNorm prologue (inputs pre-scaled by 2^-4 for the fp16 split) + bias +
    residual, in place; the last case feeds activations of magnitude 3000."""
    x = rnd(f"rx{M}{K}", (B, K, H, W), -2, 3) * scale
    w = rnd(f"rw{M}{K}", (M, K), -0.2, 0.2)
    bv = rnd(f"rb{M}", (M,), -0.3, 0.3)
    r = rnd(f"rr{M}", (B, M, H, W))
    ref = torch.einsum("mk,bkhw->bmhw", w.double(), x.double()) + bv.double().view(1, M, 1, 1) + r.double()
    y = r.clone().to(dev)
    ops.gemm1x1(_hip.pack_gemm_weight_split(w).to(dev), x.to(dev), y, M, K, res=y, bias=bv.to(dev), split=True)
    y32 = r.clone().to(dev)
    ops.gemm1x1(_hip.pack_gemm_weight(w).to(dev), x.to(dev), y32, M, K, res=y32, bias=bv.to(dev))
    e16 = (y.cpu().double() - ref).abs().max().item() / scale
    e32 = (y32.cpu().double() - ref).abs().max().item() / scale
    print(f"M{M} K{K} scale {scale:g}: max-abs/scale vs float64  f16x3 {e16:.3e}   f32 {e32:.3e}")
    assert e16 < 4e-5 and e16 < 8 * max(e32, 1e-7)


DWGEMM_CASES = [
    # M, K, H, W, B, gate, res, bias, stats, per_batch
    (48, 127, 19, 36, 2, True, True, False, True, False),
    (96, 255, 16, 64, 1, True, True, True, True, False),
    (48, 48, 8, 32, 2, False, True, False, True, True),
    (96, 96, 21, 40, 1, False, True, True, False, True),
    (40, 6, 5, 4, 1, True, False, True, False, False),
    (96, 255, 40, 96, 2, True, True, False, True, False),
]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,K,H,W,B,gate,res,bias,stats,per_batch", DWGEMM_CASES)
def test_dwgemm(dev, M, K, H, W, B, gate, res, bias, stats, per_batch, split):
    """Fused depth-wise 3x3 (+ gelu gate) + 1x1 conv (+ residual, + LN statistics of the result); split = the
    1x1 part emulated on the fp16 matrix cores (host weights only)."""
    kin = 2 * K if gate else K
    big = rnd(f"dgx{M}{K}{H}", (B, kin + 3, H, W), -1.5, 1.5)
    x = big.to(dev)[:, 1:1 + kin]
    w9 = rnd(f"dgw9{K}", (kin, 9), -0.5, 0.5)
    dwb = rnd(f"dgdb{K}", (kin,), -0.2, 0.2) if bias else None
    wt = rnd(f"dgw{M}{K}", (B if per_batch else 1, M, K), -0.2, 0.2)
    pb = rnd(f"dgb{M}", (M,), -0.3, 0.3) if bias else None
    r = rnd(f"dgr{M}{H}", (B, M, H, W)) if res else None
    pack = _hip.pack_gemm_weight_split if split else _hip.pack_gemm_weight
    packed = torch.stack([pack(wt[i]) for i in range(wt.shape[0])]).to(dev)
    dwp = _hip.pack_dw_table(w9, dwb, K, gate).to(dev)
    y = r.clone().to(dev) if res else torch.empty(B, M, H, W, device=dev)      # in place on the residual
    st = torch.zeros(B, 2, H * W, device=dev) if stats else None
    ops.dwgemm(packed, dwp, x, y, M, K, gate=gate, res=y if res else None, bias=pb.to(dev) if bias else None,
               w_bs=packed.shape[1] if per_batch else 0, stats_out=st, split=split)
    xr = big[:, 1:1 + kin].double()
    d = F.conv2d(xr, w9.double().view(kin, 1, 3, 3), dwb.double() if bias else None, padding=1, groups=kin)
    g = F.gelu(d[:, :K]) * d[:, K:] if gate else d
    ref = torch.einsum("bmk,bkhw->bmhw", wt.double().expand(B, M, K), g)
    if bias:
        ref = ref + pb.double().view(1, M, 1, 1)
    if res:
        ref = ref + r.double()
    err = (y.cpu().double() - ref).abs().max().item()
    assert err < TOL, err
    if stats:
        mean = ref.mean(1).reshape(B, -1)
        rstd = 1.0 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5).reshape(B, -1)
        sc = st.cpu().double()
        assert (sc[:, 0] - mean).abs().max() < 1e-4
        assert ((sc[:, 1] - rstd).abs() / rstd).max() < 1e-4


@pytest.mark.parametrize("B,C,heads,H,W", [(2, 48, 1, 16, 24), (1, 96, 2, 16, 16), (2, 96, 1, 8, 40), (1, 192, 4, 8, 8),
                                           (1, 384, 8, 8, 8), (1, 64, 2, 8, 8), (1, 32, 2, 8, 8), (1, 48, 1, 64, 80), (2, 384, 8, 5, 7), (1, 96, 1, 9, 15),
                                           (1, 96, 1, 64, 64), (2, 192, 2, 32, 48), (3, 48, 1, 48, 64), (1, 96, 1, 8, 8)])
def test_mdta_fold(dev, B, C, heads, H, W):
    N, c = H * W, C // heads
    qkv = rnd(f"md{C}{heads}{H}", (B, 3 * C, H, W))
    temp = rnd(f"mdt{C}{heads}", (heads,), 2.0, 6.0)
    wout = rnd(f"mdw{C}", (C, C), -0.3, 0.3)
    v = qkv[:, 2 * C:].double().reshape(B, heads, c, N)
    attn = bm.attention_qk(qkv[:, :2 * C].double(), temp, heads)
    ref = torch.einsum("oc,bcn->bon", wout.double(), (attn @ v).reshape(B, C, N)).reshape(B, C, H, W)

    chunk, nchunk, rec = ops.mdta_plan(B, C, heads, N)
    part = torch.full((B * heads * nchunk * rec,), float("nan"), device=dev)
    gsum = torch.empty(B * heads * rec, device=dev)
    mfold = torch.zeros(B * ops.mfold_numel(C), device=dev)
    attn_out = torch.empty(B, heads, c, c, device=dev)
    qg = qkv.to(dev)
    ops.mdta_fold(qg, part, gsum, temp.to(dev), wout.to(dev), mfold, C, heads, attn=attn_out)
    assert (attn_out.cpu().double() - attn).abs().max() < 2e-5
    y = torch.empty(B, C, H, W, device=dev)
    ops.gemm1x1(mfold, qg[:, 2 * C:], y, C, C, w_bs=ops.mfold_numel(C))
    assert (y.cpu().double() - ref).abs().max() < TOL
    if N % 4 == 0:
        # the same fold written in fp16 hi/lo order and applied by the emulated GEMM
        ops.mdta_fold(qg, part, gsum, temp.to(dev), wout.to(dev), mfold, C, heads, split=True)
        y2 = torch.empty(B, C, H, W, device=dev)
        ops.gemm1x1(mfold, qg[:, 2 * C:], y2, C, C, w_bs=ops.mfold_numel(C), split=True)
        assert (y2.cpu().double() - ref).abs().max() < TOL
        assert (y2 - y).abs().max() < 2e-5
    if C % 16 == 0:
        # ... and as fp16 hi/lo MFMA fragments (irm_attn_gdfn_fused_f16x3_f32's operand): the same matrix, hi + lo
        mfrag = torch.zeros(B * ops.mfold_frag_numel(C), device=dev)
        attn2 = torch.empty_like(attn_out)
        ops.mdta_fold(qg, part, gsum, temp.to(dev), wout.to(dev), mfrag, C, heads, attn=attn2, frag=True)
        assert torch.equal(attn2, attn_out)
        mref = torch.stack([wout.double() @ torch.block_diag(*attn_out[i].cpu().double()) for i in range(B)])
        got = _hip.unpack_mfold_frag(mfrag, B, C).double()
        assert (got - mref).abs().max() < 1e-6 * max(1.0, float(mref.abs().max()))


@pytest.mark.parametrize("B,C,heads,H,W,span", [(2, 48, 1, 16, 24, 1.0), (1, 96, 2, 16, 16, 1.0), (2, 96, 1, 8, 40, 1.0),
                                                (1, 192, 4, 8, 8, 1.0), (1, 384, 8, 8, 8, 1.0), (1, 96, 1, 64, 64, 1.0),
                                                (2, 192, 2, 32, 48, 1.0), (3, 48, 1, 48, 64, 1.0),
                                                (1, 96, 1, 32, 32, 2.0 ** -9), (1, 48, 1, 32, 32, 0.999), (1, 96, 1, 8, 8, 1.0)])
def test_mdta_gram_f16x3(dev, B, C, heads, H, W, span):
    """Gram pass emulated on the fp16 matrix cores against float64 and against the f32-input MFMA pass: records
    (Gram + squared norms) and the attention matrix.  scale = 2^14 / (a bound of |q|, |k| per channel); span = how
    much of that bound the data uses (2^-9: typical trained activations, far below the static bound; 0.999: at it)."""
    N, c = H * W, C // heads
    bound = rnd(f"gb{C}{heads}", (2 * C,), 0.5, 40.0)
    qkv = rnd(f"gq{C}{heads}{H}", (B, 3 * C, H, W))
    qkv[:, :2 * C] *= (bound * span).view(1, 2 * C, 1, 1)
    scale = torch.pow(2.0, torch.floor(torch.log2(2.0 ** 14.8 / bound))).float()
    assert float((qkv[:, :2 * C].abs() * scale.view(1, -1, 1, 1)).max()) < 65504
    temp = rnd(f"gt{C}{heads}", (heads,), 2.0, 6.0)
    wout = rnd(f"gw{C}", (C, C), -0.3, 0.3)
    q, k, _ = qkv.double().reshape(B, 3, heads, c, N).unbind(1)
    G = q @ k.transpose(-1, -2)
    attn = bm.attention(q.reshape(B, C, N), k.reshape(B, C, N), temp, heads)
    chunk, nchunk, rec = ops.mdta_plan(B, C, heads, N)
    qg = qkv.to(dev)
    outs = []
    for sc in (None, scale.to(dev)):
        attn_out, _, gsum = bm.run_mdta_fold(dev, qg, temp, wout, C, heads, gram_scale=sc)
        outs.append((gsum.double().view(B, heads, rec), attn_out.double()))
    gref = torch.cat([G.reshape(B, heads, c * c), (q * q).sum(-1), (k * k).sum(-1)], -1)
    mag = gref.abs().max()
    e32, e16 = (outs[0][0] - gref).abs().max() / mag, (outs[1][0] - gref).abs().max() / mag
    a32, a16 = (outs[0][1] - attn).abs().max(), (outs[1][1] - attn).abs().max()
    print(f"gram C{C} h{heads} N{N} span {span:.1e}: records rel err f32 {e32:.2e} f16x3 {e16:.2e}; attn abs err f32 {a32:.2e} f16x3 {a16:.2e}")
    assert e16 <= 2 * e32 + 2e-7 and a16 <= 2 * a32 + 2e-7


CONV_CASES = [
    # ci, co, H, W, B, bias, relu1, res_mode, relu2, store
    (3, 48, 16, 32, 2, False, False, 0, False, 0),
    (48, 24, 16, 32, 1, False, False, 0, False, 1),
    (96, 48, 8, 40, 2, False, False, 0, False, 1),
    (96, 192, 8, 16, 1, False, False, 0, False, 2),
    (384, 768, 8, 8, 1, False, False, 0, False, 2),
    (96, 3, 24, 40, 2, False, False, 1, False, 0),
    (1, 64, 13, 21, 1, True, True, 0, False, 0),
    (64, 64, 13, 21, 2, True, True, 0, False, 0),
    (64, 1, 13, 21, 1, True, False, 2, False, 0),
    (128, 128, 16, 16, 1, True, True, 1, True, 0),
    (6, 48, 9, 33, 1, True, False, 0, False, 0),
    (192, 96, 10, 14, 1, False, False, 0, False, 1),     # unshuffle, W % 4 != 0
    (384, 768, 5, 7, 2, False, False, 0, False, 2),       # shuffle at an odd level-4 size
]


@pytest.mark.parametrize("ci,co,H,W,B,bias,relu1,res_mode,relu2,store", CONV_CASES)
def test_conv3x3(dev, ci, co, H, W, B, bias, relu1, res_mode, relu2, store):
    tag = f"cv{ci}_{co}_{H}_{W}"
    x = rnd(tag + "x", (B, ci, H, W))
    w = rnd(tag + "w", (co, ci, 3, 3), -0.2, 0.2)
    bv = rnd(tag + "b", (co,)) if bias else None
    r = rnd(tag + "r", (B, co, H, W)) if res_mode else None
    ref = bm.conv_epilogue(F.conv2d(x.double(), w.double(), bv.double() if bias else None, padding=1), r, relu1, res_mode, relu2, store)
    ybig = torch.full((B, ref.shape[1] + 2, ref.shape[2], ref.shape[3]), 5.0, device=dev)
    y = ybig[:, 1:1 + ref.shape[1]]
    ops.conv3x3(_hip.pack_conv3x3_weight(w).to(dev), x.to(dev), y, ci, co, bias=bv.to(dev) if bias else None,
                relu1=relu1, res=r.to(dev) if res_mode else None, res_mode=res_mode, relu2=relu2, store_mode=store)
    got = ybig.cpu().double()
    assert (got[:, 1:-1] - ref).abs().max() < TOL * max(1.0, float(ref.abs().max()))
    assert torch.all(got[:, 0] == 5.0) and torch.all(got[:, -1] == 5.0)


def test_deconv_as_conv(dev):
    wt = rnd("dcw", (32, 16, 3, 3), -0.3, 0.3)      # ConvTranspose2d weight [Ci][Co][3][3]
    x = rnd("dcx", (1, 32, 10, 12))
    ref = F.conv_transpose2d(x.double(), wt.double(), None, padding=1)
    y = torch.empty(1, 16, 10, 12, device=dev)
    ops.conv3x3(_hip.pack_conv3x3_weight(_hip.deconv_as_conv_weight(wt)).to(dev), x.to(dev), y, 32, 16)
    assert (y.cpu().double() - ref).abs().max() < TOL


def test_rejects_bad_arguments(dev):
    x = torch.zeros(1, 4, 3, 5, device=dev)
    with pytest.raises(_hip.HipLibraryError):      # act code out of range -> IRM_EINVAL, nothing launched
        ops.dwconv3x3(x, torch.zeros(4, 9, device=dev), torch.empty_like(x), act=9)
    with pytest.raises(_hip.HipLibraryError):      # PixelUnshuffle needs even H, W
        ops.conv3x3(torch.zeros(9 * 64, device=dev), x, torch.empty(1, 16, 1, 2, device=dev), 4, 4, store_mode=1)
    with pytest.raises(ValueError):
        ops.ln_stats(torch.zeros(1, 4, 4, 4), torch.zeros(32))          # CPU tensor


CONV_F16_CASES = [
    # ci, co, H, W, B, bias, relu1, res_mode, relu2, store_mode, ct
    (64, 64, 16, 32, 2, True, True, 0, False, 0, None),
    (3, 48, 24, 40, 1, False, False, 0, False, 0, None),       # patch embed: one padded stage
    (48, 24, 16, 32, 2, False, False, 0, False, 1, None),      # down: PixelUnshuffle
    (96, 192, 8, 32, 1, False, False, 0, False, 2, 3),         # up: PixelShuffle
    (96, 3, 16, 36, 1, True, False, 1, False, 0, None),        # output conv + global residual, partial tile
    (1, 64, 12, 20, 1, True, True, 0, False, 0, None),         # DnCNN first layer (gray)
    (64, 1, 12, 20, 1, True, False, 2, False, 0, None),        # DnCNN last layer: x - conv
    (128, 128, 8, 8, 2, True, False, 1, True, 0, 4),           # REDNet-style: conv + skip + relu
    (70, 50, 20, 44, 1, True, False, 0, False, 0, 2),          # ragged channel counts
    (96, 192, 16, 64, 2, False, False, 0, False, 2, 12),       # up: all 12 output tiles in ONE pass (3 weight chunks of 4)
    (64, 384, 8, 32, 1, True, False, 0, False, 2, 12),         # 24 output tiles: two passes of 12
    (40, 150, 16, 36, 1, True, True, 0, False, 0, 8),          # 10 output tiles: a pass of 8 + a ragged pass, ragged channels
    (192, 384, 8, 32, 2, False, False, 0, False, 2, None),     # the launch plan's own choice (ct 12)
]


@pytest.mark.parametrize("ci,co,H,W,B,bias,relu1,res_mode,relu2,store_mode,ct", CONV_F16_CASES)
def test_conv3x3_f16x3(dev, ci, co, H, W, B, bias, relu1, res_mode, relu2, store_mode, ct):
    """irm_conv3x3_f16x3_f32 (fp32 emulated on the fp16 matrix cores) vs float64, next to the exact-f32 kernel on the
    same inputs: its error must not exceed 2x the exact kernel's (+ fp32 rounding of the output)."""
    tag = f"cf{ci}_{co}_{H}_{W}_{store_mode}"
    w = rnd(tag + "w", (co, ci, 3, 3), -0.2, 0.2)
    x = rnd(tag + "x", (B, ci, H, W), -1.5, 2.0)
    bv = rnd(tag + "b", (co,)) if bias else None
    oc, oh, ow = (co, H, W) if store_mode == 0 else (co * 4, H // 2, W // 2) if store_mode == 1 else (co // 4, 2 * H, 2 * W)
    r = rnd(tag + "r", (B, oc, oh, ow)) if res_mode else None
    ref = bm.conv_epilogue(F.conv2d(x.double(), w.double(), None if bv is None else bv.double(), padding=1), r, relu1, res_mode, relu2,
                           store_mode)
    xd = x.to(dev)
    kw = dict(bias=None if bv is None else bv.to(dev), relu1=relu1, res=None if r is None else r.to(dev), res_mode=res_mode,
              relu2=relu2, store_mode=store_mode)
    y16 = torch.full((B, oc + 1, oh, ow), 7.0, device=dev)
    wps, inv = _hip.pack_conv3x3_weight_split(w)
    ops.conv3x3((wps.to(dev), inv), xd, y16[:, :oc], ci, co, ct=ct, **kw)
    y32 = torch.empty(B, oc, oh, ow, device=dev)
    ops.conv3x3(_hip.pack_conv3x3_weight(w).to(dev), xd, y32, ci, co, **kw)
    e16 = float((y16[:, :oc].cpu().double() - ref).abs().max())
    e32 = float((y32.cpu().double() - ref).abs().max())
    scale = max(1.0, float(ref.abs().max()))
    print(f"conv3x3 f16x3 {tag}: {e16:.3e} (exact f32 kernel {e32:.3e})")
    assert e16 <= TOL * scale and e16 <= 2.0 * e32 + 4e-7 * scale
    assert torch.all(y16[:, oc] == 7.0)


THIN_CASES = [   # ci, co, H, W, B, bias, relu1, res_mode, relu2
    (96, 3, 24, 40, 2, False, False, 1, False),      # Restormer output conv + inp_img
    (3, 48, 24, 40, 1, False, False, 0, False),      # Restormer patch embed
    (64, 1, 13, 20, 1, True, False, 2, False),       # DnCNN last layer: x - conv (odd height)
    (1, 64, 13, 20, 2, True, True, 0, False),        # DnCNN first layer (gray) + ReLU
    (128, 1, 16, 16, 1, True, False, 1, True),       # REDNet-style: + skip, ReLU
    (4, 20, 5, 8, 1, True, False, 0, False),         # ci = 4, ragged co group
    (50, 4, 9, 12, 3, False, True, 0, False),        # co = 4
    (2, 2, 4, 4, 1, True, False, 3, False),          # both thin; tanh + clamp epilogue (DeblurGANv2 final)
    (6, 2, 3, 36, 1, False, False, 0, False),        # fewer input channels than ci groups x 2
]


@pytest.mark.parametrize("ci,co,H,W,B,bias,relu1,res_mode,relu2", THIN_CASES)
def test_conv3x3_thin(dev, ci, co, H, W, B, bias, relu1, res_mode, relu2):
    """irm_conv3x3_thin_f32 (exact fp32 on the vector pipe, convs with <= 4 channels on one side) through ops.conv3x3's
    dispatch on a ConvWeight, into a channel slice of a sentinel-filled buffer, against float64."""
    tag = f"th{ci}_{co}_{H}_{W}"
    w = rnd(tag + "w", (co, ci, 3, 3), -0.3, 0.3)
    x = rnd(tag + "x", (B, ci, H, W), -1.5, 2.0)
    bv = rnd(tag + "b", (co,)) if bias else None
    r = rnd(tag + "r", (B, co, H, W)) if res_mode else None
    ref = bm.conv_epilogue(F.conv2d(x.double(), w.double(), None if bv is None else bv.double(), padding=1), r, relu1, res_mode, relu2)
    cw = _hip.pack_conv3x3(w.to(dev))
    assert cw.raw is not None
    ybig = torch.full((B, co + 2, H, W), 5.0, device=dev)
    timer, ops.TIMER = ops.TIMER, ops.KernelTimer()
    try:
        ops.conv3x3(cw, x.to(dev), ybig[:, 1:1 + co], ci, co, bias=None if bv is None else bv.to(dev), relu1=relu1,
                    res=None if r is None else r.to(dev), res_mode=res_mode, relu2=relu2)
        assert list(ops.TIMER.summary()) == ["conv3x3_thin"]           # the thin kernel ran, not a matrix-core one
    finally:
        ops.TIMER = timer
    got = ybig.cpu().double()
    err = float((got[:, 1:-1] - ref).abs().max())
    print(f"conv3x3 thin {tag}: max-abs vs float64 {err:.3e}")
    assert err <= 2e-6 * max(1.0, float(ref.abs().max()))
    assert torch.all(got[:, 0] == 5.0) and torch.all(got[:, -1] == 5.0)


def test_kernel_timer_only_times_the_selected_group(dev):
    """ops.KernelTimer(only=...): bench.py's timed steps carry events around the roofline kernel only - the other launches run
    plainly (and give the same results), the selected group is timed launch by launch."""
    B, C, H, W = 2, 32, 16, 32
    x = rnd("kt_x", (B, C, H, W)).to(dev)
    w9 = rnd("kt_w", (C, 9), -0.4, 0.4).to(dev)
    stats = torch.empty(B, 2, H * W, device=dev)
    y0, y1 = torch.empty_like(x), torch.empty_like(x)
    ops.dwconv3x3(x, w9, y0)
    timer, ops.TIMER = ops.TIMER, ops.KernelTimer(only={"dwconv3x3"})
    try:
        ops.ln_stats(x, stats)                      # not selected: no record
        ops.dwconv3x3(x, w9, y1)
        ops.ln_stats(x, stats)
        ops.dwconv3x3(x, w9, y1)
        s = ops.TIMER.summary()
    finally:
        ops.TIMER = timer
    assert list(s) == ["dwconv3x3"] and s["dwconv3x3"]["launches"] == 2 and s["dwconv3x3"]["ms"] > 0.0
    assert torch.equal(y0, y1)


# --------------------------------------------------------------------------- no writes outside the output
@pytest.mark.parametrize("C,H,W", [(48, 64, 96), (96, 40, 56), (192, 32, 32), (384, 16, 24), (96, 9, 15)])
def test_no_write_outside_the_output(dev, C, H, W):
    """Every kernel of a TransformerBlock and the dense convs write into the middle of a sentinel-filled buffer: the
    sentinels on both sides must survive (tile / chunk tails, masked lanes, pixel-shuffle stores, odd sizes)."""
    B = 2
    hid = int(C * 2.66)
    X = rnd(f"cx{C}{H}", (B, C, H, W)).to(dev)
    checks = []

    def run(name, shape, fn):
        buf, y = guards.sentinel_out(shape, dev, pad=1 << 14)
        fn(y)
        torch.cuda.synchronize()
        checks.append((name, guards.intact(buf, y)))
    aligned = W % 4 == 0
    run("ln_stats", (B, 2, H, W), lambda y: ops.ln_stats(X, y))
    st = torch.empty(B, 2, H, W, device=dev)
    ops.ln_stats(X, st)
    lnw, lnb = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    for M in (3 * C, 2 * hid):
        for split in ((True, False) if aligned else (False,)):
            w = rnd(f"cw{M}{C}", (M, C), -0.2, 0.2)
            wp = (_hip.pack_gemm_weight_split(w) if split else _hip.pack_gemm_weight(w)).to(dev)
            run(f"gemm LN M{M} split{int(split)}", (B, M, H, W),
                lambda y: ops.gemm1x1(wp, X, y, M, C, stats=st, lnw=lnw, lnb=lnb, ln_mode=1, split=split))
    G = rnd(f"cg{C}{H}", (B, hid, H, W)).to(dev)
    for split in ((True, False) if aligned else (False,)):
        w = rnd(f"cp{C}", (C, hid), -0.2, 0.2)
        wp = (_hip.pack_gemm_weight_split(w) if split else _hip.pack_gemm_weight(w)).to(dev)

        def inplace(y):
            y.copy_(X)
            ops.gemm1x1(wp, G, y, C, hid, res=y, split=split)
        run(f"gemm res in place split{int(split)}", (B, C, H, W), inplace)
    Hh = rnd(f"ch{C}{H}", (B, 2 * hid, H, W)).to(dev)
    run("dwconv3x3_gate", (B, hid, H, W), lambda y: ops.dwconv3x3_gate(Hh, rnd(f"cdg{C}", (2 * hid, 9), -0.4, 0.4).to(dev), y))
    QKV = rnd(f"cq{C}{H}", (B, 3 * C, H, W)).to(dev)
    run("dwconv3x3", (B, 3 * C, H, W), lambda y: ops.dwconv3x3(QKV, rnd(f"cd{C}", (3 * C, 9), -0.4, 0.4).to(dev), y))
    heads = max(1, C // 48)
    temp, wout = torch.ones(heads, device=dev), rnd(f"co{C}", (C, C), -0.3, 0.3).to(dev)
    chunk, nchunk, rec = ops.mdta_plan(B, C, heads, H * W)
    sc = torch.full((2 * C,), 1024.0, device=dev)
    for gs in (None, sc):
        bp, part = guards.sentinel_out((B * heads * nchunk * rec,), dev, pad=1 << 14)
        bg, gsum = guards.sentinel_out((B * heads * rec,), dev, pad=1 << 14)
        bf, mf = guards.sentinel_out((B * ops.mfold_numel(C),), dev, pad=1 << 14)
        mf.zero_()
        ops.mdta_fold(QKV, part, gsum, temp, wout, mf, C, heads, split=aligned, gram_scale=gs)
        torch.cuda.synchronize()
        checks.append((f"mdta f16x3={gs is not None}", guards.intact(bp, part) and guards.intact(bg, gsum)
                       and guards.intact(bf, mf)))
    if C <= 96 and aligned:
        pk = _hip.pack_gdfn_fused(rnd("fa", (2 * hid, C), -.3, .3).to(dev), None, rnd("fb", (2 * hid, 9), -.4, .4), None,
                                  rnd("fc", (C, hid), -.3, .3), rnd("fd", (C,), .5, 1.5), rnd("fe", (C,), -.2, .2))
        run("gdfn_fused", (B, C, H, W), lambda y: ops.gdfn_fused(pk, X, y, C, hid, ln_mode=1))
        pkq = _hip.pack_qkv_fused(rnd("fq", (3 * C, C), -.3, .3).to(dev), None, rnd("fr", (3 * C, 9), -.4, .4), None,
                                  rnd("fd", (C,), .5, 1.5), rnd("fe", (C,), -.2, .2))
        run("qkv_dw_fused", (B, 3 * C, H, W), lambda y: ops.qkv_dw_fused(pkq, X, y, C, 3 * C, ln_mode=1))
    if H % 2 == 0 and W % 2 == 0:
        for co, mode in ((C // 2, 1), (2 * C, 2), (C, 0)):
            wc = rnd(f"cc{C}{co}", (co, C, 3, 3), -0.05, 0.05).to(dev)
            oc, oh, ow = (co * 4, H // 2, W // 2) if mode == 1 else (co // 4, H * 2, W * 2) if mode == 2 else (co, H, W)
            for cw in (_hip.pack_conv3x3(wc), _hip.pack_conv3x3_weight(wc).to(dev)):
                run(f"conv3x3 co{co} mode{mode} {'emulated' if not torch.is_tensor(cw) else 'exact'}", (B, oc, oh, ow),
                    lambda y: ops.conv3x3(cw, X, y, C, co, store_mode=mode))
    bad = [n for n, ok in checks if not ok]
    assert not bad, f"writes outside the output: {bad}"
