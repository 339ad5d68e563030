"""GPU tests of the fp16 inference mode of the conv stacks (csrc/conv3x3_h.hip) against the float64 quantised-chain model
of tests/half_model.py.  Kernel bounds are derived there (half an fp16 ulp for the one rounding of the store plus the
fp32 accumulation chain), never measured on the code under test; every operand lies between guard bands (tests/guards.py).
"""
import functools

import numpy as np
import pytest
import torch

from irm_amd import _hip, dncnn, ops, rednet, synth, utils
from oracle import tiler_ref

import guards
import half_model as hm

pytestmark = pytest.mark.gpu

SIZES = [(24, 40), (9, 33), (1, 5)]     # several tiles, partial in both axes; odd; smaller than a tile and than the halo
SLACK = 64                              # elements between the images of a batch (a batch stride larger than the tensor)


def uni(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(11, name, shape, lo, hi)


def h16(t):
    """Values rounded to fp16, as float32 (exact)."""
    return t.half().float()


def to_cl(t):
    """Planar [B,C,H,W] values that are fp16 numbers -> fp16 channel-last [B,H,W,C]."""
    return t.permute(0, 2, 3, 1).contiguous().half()


def from_cl(t):
    return t.detach().cpu().permute(0, 3, 1, 2).double()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def check(y, v, bound, what):
    err = (y - v).abs()
    ratio = float((err / bound).max())
    print(f"{what}: max |y - v| / bound = {ratio:.3f}, max |y - v| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} outside the bound (x{ratio:.2f})"


def mid_operands(ci, co, H, W, tag, xscale=1.0):
    x = h16(uni(f"mx{tag}", (2, ci, H, W)) * xscale)
    w = uni(f"mw{tag}", (co, ci, 3, 3)) * (3.0 / (9 * ci)) ** 0.5
    bias = uni(f"mb{tag}", (co,), -0.5, 0.5)
    res = h16(uni(f"mr{tag}", (2, co, H, W)))
    return x, w, bias, res


def run_mid(dev, x, w, bias, res, relu1, res_mode, relu2):
    """(y planar float64, bit pattern, guards intact) of one irm_conv3x3_h_f16 launch between guard bands."""
    co, ci = w.shape[:2]
    B, _, H, W = x.shape
    packed, inv = _hip.pack_conv3x3_h(w)
    _, xv = guards.banded(to_cl(x), dev, batch_slack=SLACK)
    rv = guards.banded(to_cl(res), dev, batch_slack=SLACK)[1] if res_mode else None
    ybuf, yv = guards.sentinel_out((B, H, W, co), dev, dtype=torch.float16, batch_slack=SLACK)
    ops.conv3x3_h((packed.to(dev), inv), xv, yv, ci, co, bias=bias.to(dev), relu1=relu1, res=rv, res_mode=res_mode,
                  relu2=relu2)
    torch.cuda.synchronize()
    return from_cl(yv), bits(yv), guards.intact(ybuf, yv)


EPILOGUES = {"bias": (False, 0, False), "relu1": (True, 0, False), "res_relu2": (True, 1, True)}


@pytest.mark.parametrize("ep", list(EPILOGUES))
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("ci,co", [(64, 64), (64, 128), (128, 64), (128, 128)])
def test_mid_kernel_vs_model(dev, ci, co, H, W, ep):
    relu1, res_mode, relu2 = EPILOGUES[ep]
    x, w, bias, res = mid_operands(ci, co, H, W, f"{ci}_{co}_{H}")
    y, b0, ok = run_mid(dev, x, w, bias, res, relu1, res_mode, relu2)
    assert ok, "a store outside the output"
    v, S = hm.layer(x, hm.quantised_weight(w), bias, relu1=relu1, res=res if res_mode else None, res_mode=res_mode,
                    relu2=relu2)
    assert not guards.has_nan(y), "a read outside the input reached the output"
    check(y, v, hm.bound_f16(v, S, ci), "irm_conv3x3_h_f16" + f" {ci}->{co} {H}x{W} {ep}")
    _, b1, _ = run_mid(dev, x, w, bias, res, relu1, res_mode, relu2)
    assert torch.equal(b0, b1), "a repeated launch is not bit-identical"


WIDE = (9, 2017)    # 2 x 64 pixel tiles, partial in both axes; x B = 2: the 256 pixel tiles from which Co = 128 runs CT = 8


@pytest.mark.parametrize("ci", [64, 128])
def test_mid_kernel_eight_tile_workgroup(dev, ci):
    """Co = 128 with at least 256 pixel tiles in the launch: one workgroup owns all eight output-channel tiles
    (conv3x3_h_kernel<8>: two weight pieces per wave, 16 accumulator tiles, the largest LDS footprint at Ci = 128).
    Same bound, guard bands and repeat identity as the small cases; and, launched one image at a time (128 pixel tiles:
    the four-tile workgroups), the same images give the same bits, since the two differ only in who owns which channels."""
    H, W = WIDE
    assert -(-H // 8) * -(-W // 32) * 2 == 256
    relu1, res_mode, relu2 = EPILOGUES["res_relu2"]
    x, w, bias, res = mid_operands(ci, 128, H, W, f"wide{ci}")
    y, b8, ok = run_mid(dev, x, w, bias, res, relu1, res_mode, relu2)
    assert ok, "a store outside the output"
    assert not guards.has_nan(y), "a read outside the input reached the output"
    v, S = hm.layer(x, hm.quantised_weight(w), bias, relu1=relu1, res=res, res_mode=res_mode, relu2=relu2)
    check(y, v, hm.bound_f16(v, S, ci), f"irm_conv3x3_h_f16 {ci}->128 {H}x{W} B 2 (eight-tile workgroup)")
    _, again, _ = run_mid(dev, x, w, bias, res, relu1, res_mode, relu2)
    assert torch.equal(b8, again), "a repeated launch is not bit-identical"
    for b in range(2):
        _, b4, ok4 = run_mid(dev, x[b:b + 1], w, bias, res[b:b + 1], relu1, res_mode, relu2)
        assert ok4 and torch.equal(b4, b8[b:b + 1]), f"image {b}: the four-tile and the eight-tile workgroup differ"


def test_mid_kernel_small_weights_keep_their_bits(dev):
    """BN-merged weights of 1e-4: the power-of-two scale keeps them out of the fp16 subnormals."""
    x, w, bias, res = mid_operands(64, 64, 9, 33, "small")
    w = w * 1.0e-4
    y, _, ok = run_mid(dev, x, w, bias * 1.0e-4, res, False, 0, False)
    v, S = hm.layer(x, hm.quantised_weight(w), bias * 1.0e-4)
    assert ok
    check(y, v, hm.bound_f16(v, S, 64), "mid small weights")
    exact, _ = hm.layer(x, w, bias * 1.0e-4)
    assert float((v - exact).abs().max()) <= 2.0 ** -10 * float(S.max())      # 11-bit weights, not subnormal ones


def test_mid_kernel_overflow_becomes_inf(dev):
    """Inputs scaled so that some outputs exceed 65504: those, and only those, are +-inf."""
    x, w, bias, res = mid_operands(64, 64, 9, 33, "ovf", xscale=6.0e4)
    y, _, ok = run_mid(dev, x, w, bias, res, False, 0, False)
    v, S = hm.layer(x, hm.quantised_weight(w), bias)
    assert ok and not guards.has_nan(y)
    want_inf = torch.isinf(hm.rne16(v))
    unsure = (v.abs() - 65520.0).abs() <= (9 * 64 + 4) * 2.0 ** -24 * S       # the fp32 sum may land on either side
    n_inf, n_fin = int(want_inf.sum()), int((~want_inf).sum())
    print(f"overflow: {n_inf} of {v.numel()} outputs beyond fp16, {int(unsure.sum())} undecided")
    assert n_inf > 50 and n_fin > 50
    assert torch.equal(torch.isinf(y)[~unsure], want_inf[~unsure])
    assert torch.equal(torch.sign(y)[want_inf & ~unsure], torch.sign(v)[want_inf & ~unsure])
    fin = ~want_inf & ~unsure
    check(y[fin], v[fin], hm.bound_f16(v, S, 64)[fin], "mid overflow, finite part")


def test_mid_kernel_nan_stays_local(dev):
    """One NaN input pixel: NaN at exactly the outputs of its 3x3 neighbourhood, through the ReLU too."""
    x, w, bias, res = mid_operands(64, 128, 24, 40, "nan")
    x[1, :, 8, 32] = float("nan")                       # a tile corner: its neighbourhood spans four tiles
    x[0, 5, 0, 0] = float("nan")                        # one channel, image corner
    y, _, ok = run_mid(dev, x, w, bias, res, True, 0, False)
    assert ok
    want = torch.zeros(2, 128, 24, 40, dtype=torch.bool)
    want[1, :, 7:10, 31:34] = True
    want[0, :, 0:2, 0:2] = True
    assert torch.equal(torch.isnan(y), want)
    v, S = hm.layer(x, hm.quantised_weight(w), bias, relu1=True)
    assert torch.equal(torch.isnan(v), want)
    check(y[~want], v[~want], hm.bound_f16(v, S, 64)[~want], "mid nan, the rest")


@pytest.mark.parametrize("relu1", [False, True])
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("co", [64, 128])
@pytest.mark.parametrize("ci", [1, 3])
def test_in_kernel_vs_model(dev, ci, co, H, W, relu1):
    x = uni(f"ix{ci}_{H}", (2, ci, H, W), 0.0, 1.0)
    w = uni(f"iw{ci}_{co}", (co, ci, 3, 3))
    bias = uni(f"ib{co}", (co,), -0.5, 0.5)

    def run():
        _, xv = guards.banded(x, dev, batch_slack=SLACK)
        ybuf, yv = guards.sentinel_out((2, H, W, co), dev, dtype=torch.float16, batch_slack=SLACK)
        ops.conv3x3_h_in(w.to(dev), xv, yv, ci, co, bias=bias.to(dev), relu1=relu1)
        torch.cuda.synchronize()
        return from_cl(yv), bits(yv), guards.intact(ybuf, yv)
    y, b0, ok = run()
    assert ok, "a store outside the output"
    assert not guards.has_nan(y), "a read outside the input reached the output"
    v, S = hm.layer(x, w, bias, relu1=relu1)
    check(y, v, hm.bound_f16(v, S, ci), "irm_conv3x3_h_in_f32" + f" {ci}->{co} {H}x{W}")
    assert torch.equal(b0, run()[1]), "a repeated launch is not bit-identical"


@pytest.mark.parametrize("res_mode", [1, 2])
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("ci", [64, 128])
@pytest.mark.parametrize("co", [1, 3])
def test_out_kernel_vs_model(dev, ci, co, H, W, res_mode):
    x = h16(uni(f"ox{ci}_{H}", (2, ci, H, W)))
    w = uni(f"ow{ci}_{co}", (co, ci, 3, 3)) * (3.0 / (9 * ci)) ** 0.5
    bias = uni(f"ob{co}", (co,), -0.5, 0.5)
    res = uni(f"or{co}_{H}", (2, co, H, W), 0.0, 1.0)

    def run():
        _, xv = guards.banded(to_cl(x), dev, batch_slack=SLACK)
        _, rv = guards.banded(res, dev, batch_slack=SLACK)
        ybuf, yv = guards.sentinel_out((2, co, H, W), dev, batch_slack=SLACK)
        ops.conv3x3_h_out(w.to(dev), xv, yv, ci, co, bias=bias.to(dev), res=rv, res_mode=res_mode)
        torch.cuda.synchronize()
        return yv.cpu().double(), bits(yv), guards.intact(ybuf, yv)
    y, b0, ok = run()
    assert ok, "a store outside the output"
    assert not guards.has_nan(y), "a read outside an input reached the output"
    v, S = hm.layer(x, w, bias, res=res, res_mode=res_mode)
    check(y, v, hm.bound_f32(v, S, ci), "irm_conv3x3_h_out_f32" + f" {ci}->{co} {H}x{W} res_mode {res_mode}")
    assert torch.equal(b0, run()[1]), "a repeated launch is not bit-identical"


def test_wrappers_reject_wrong_operands(dev):
    x = torch.zeros(1, 8, 8, 64, dtype=torch.float16, device=dev)
    wp = (torch.zeros(9 * 64 * 64, dtype=torch.float16, device=dev), 1.0)
    with pytest.raises(ValueError):
        ops.conv3x3_h(wp, x.float(), x, 64, 64)
    with pytest.raises(ValueError):
        ops.conv3x3_h(wp, x, torch.zeros(1, 8, 8, 128, dtype=torch.float16, device=dev), 64, 64)
    with pytest.raises(ValueError):
        ops.conv3x3_h(wp, x, x.clone(), 64, 64, res_mode=1)
    with pytest.raises(ValueError):
        ops.conv3x3_h(wp, x[:, :, :, :32], x.clone(), 64, 64)
    with pytest.raises(ValueError):
        ops.conv3x3_h_in(torch.zeros(64, 5, 3, 3, device=dev), torch.zeros(1, 5, 8, 8, device=dev), x, 5, 64)
    with pytest.raises(ValueError):
        ops.conv3x3_h_out(torch.zeros(3, 64, 3, 3, device=dev), x, torch.zeros(1, 3, 8, 8, device=dev), 64, 3, res_mode=2)


# --------------------------------------------------------------------------- models
MODELS = {
    "dncnn17_gray": (lambda **kw: dncnn.DnCNN(1, 1, 64, 17, "R", **kw), hm.dncnn_spec, 1),
    "dncnn20_colour": (lambda **kw: dncnn.DnCNN(3, 3, 64, 20, "R", **kw), hm.dncnn_spec, 3),
    "rednet": (lambda **kw: rednet.REDNet(**kw), hm.rednet_spec, 1),
}


@functools.lru_cache(maxsize=None)
def chain_reference(tag, H, W):
    """(x, A, d0) on the CPU, once per (model, size): A = the quantised chain with float64 sums, d0 = its distance to
    the same chain with float32 sums (the chain's own sensitivity to the summation order)."""
    make, spec_of, c = MODELS[tag]
    spec = spec_of(make().load_synthetic(42))
    x = synth.uniform(7, f"half_{tag}_{H}", (2, c, H, W), 0.0, 1.0)
    A = hm.run_chain(spec, x, "f64")
    Bm = hm.run_chain(spec, x, "f32")
    return x, A, float((A - Bm).abs().max())


@pytest.mark.parametrize("H,W", [(24, 40), (9, 33)])
@pytest.mark.parametrize("tag", list(MODELS))
def test_model_vs_quantised_chain(dev, tag, H, W):
    x, A, d0 = chain_reference(tag, H, W)
    model = MODELS[tag][0](precision="fp16").load_synthetic(42).eval().to(dev)
    y = model(x.to(dev)).cpu().double()
    dist, bound = float((y - A).abs().max()), 8 * d0 + 2.0 ** -20 * float(A.abs().max())
    print(f"{tag} {H}x{W}: d0 = {d0:.3e}, max |gpu - A| = {dist:.3e}, bound = {bound:.3e}, max |A| = {float(A.abs().max()):.3f}")
    assert y.shape == A.shape and dist <= bound


@pytest.mark.parametrize("tag", list(MODELS))
def test_fp32_mode_is_unchanged_and_graph_replays_fp16(dev, tag):
    make, _, c = MODELS[tag]
    x = synth.uniform(7, f"half_{tag}_24", (2, c, 24, 40), 0.0, 1.0).to(dev)
    plain = make().load_synthetic(42).eval().to(dev)
    named = make(precision="fp32").load_synthetic(42).eval().to(dev)
    assert torch.equal(plain(x), named(x))
    half = make(precision="fp16").load_synthetic(42).eval().to(dev)
    assert list(half.state_dict()) == list(plain.state_dict())
    eager = half(x).clone()
    assert not torch.equal(eager, plain(x)), "the fp16 mode did not run"
    for _ in range(2):
        assert torch.equal(utils.graphed_forward(half, x), eager)
    assert "_irm_graphs" in half.__dict__ and not half._ws.get("key"), "the graph owns the workspace"
    half(x[:1])                                          # another shape: new workspace, same results per image
    assert torch.equal(half(x), eager)
    half.release_workspace()
    assert not half._ws


def test_tiler_psnr_agrees_between_the_modes(dev):
    """A 96 x 128 uint8 synthetic frame, sigma 25, patch 64 / overlap 16, DnCNN (nb 17, gray, synthetic weights) in both
    modes: the PSNR against the clean target agrees within 0.01 dB.  On the CPU the same frame through the reference
    tiler gives 20.775966 dB with the float64 network and 20.775829 dB with the quantised chain (1.4e-4 dB apart, 93 of
    12288 bytes differ by 1; the synthetic weights do not denoise, the figure only has to agree)."""
    model32 = dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(42).eval().to(dev)
    model16 = dncnn.DnCNN(1, 1, 64, 17, "R", precision="fp16").load_synthetic(42).eval().to(dev)
    _, clean = synth.synth_image_pair(1, 96, 128, 1, seed_base=3000, blur=0)
    kw = dict(patch_size=64, patch_overlap=16, need_degradation=True, noise_level=25)
    p32, _ = utils.run_model_inference(model32, clean, dev, **kw)
    p16, _ = utils.run_model_inference(model16, clean, dev, **kw)
    a, b = tiler_ref.psnr(clean, p32), tiler_ref.psnr(clean, p16)
    diff = np.abs(p32.astype(int) - p16.astype(int))
    print(f"tiler: PSNR fp32 {a:.4f} dB, fp16 {b:.4f} dB; {int((diff > 0).sum())} of {diff.size} bytes differ (max {diff.max()})")
    assert abs(a - b) <= 0.01
