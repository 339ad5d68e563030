"""The conditions the inputs of tests/degenerate.py must meet (no GPU): the pixel patterns are exact in fp32 under the
oracle's own LayerNorm, and the CPU oracles are finite, with a non-zero fp32 error, on the frames the GPU ledger
(tests/test_gpu_degenerate_models.py) feeds them.  The GPU file checks the same conditions on every (case, frame) pair
as it goes."""
import pytest
import torch

import degenerate as dg
from irm_amd import synth
from oracle import restormer_ref
from ledger import CASES, cpu_params, f64

KS = (48, 96, 192, 384)


def _ln_params(K, with_bias):
    lnw = synth.uniform(11, f"dg_lnw{K}", (K,), 0.5, 1.5)
    lnb = synth.uniform(11, f"dg_lnb{K}", (K,), -0.2, 0.2) if with_bias else None
    return lnw, lnb


def _ln(x, lnw, lnb, dtype):
    return restormer_ref.layer_norm_c(x.to(dtype).view(1, -1, 1, 1), lnw.to(dtype), None if lnb is None else lnb.to(dtype)).view(-1)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("K", KS)
def test_flat_pixels_are_exact_in_fp32(K, with_bias):
    """Z and C(a): the fp32 LayerNorm equals the float64 one rounded to fp32.  WithBias: bit for bit, and the value is
    the bias (the deviations are exactly 0, so eps, the square root and the division never touch the result).  BiasFree:
    Z bit for bit (0); C(a) gives a / sqrt(0 + eps) * w, where the MEAN and VARIANCE are exact but eps = 1e-5 itself is
    not an fp32 number and the square root, the division and the product round once each - four roundings of 2^-24
    relative against the one of the rounded float64 value, asserted as that: |d| <= 4 * 2^-24 |y64|."""
    lnw, lnb = _ln_params(K, with_bias)
    for name in ("Z", "C(1)", "C(-2)", "C(0.5)"):
        x = dg.pattern(name, K)
        y32, y64 = _ln(x, lnw, lnb, torch.float32), _ln(x, lnw, lnb, torch.float64)
        xd = x.double()
        assert float(xd.mean()) == float(x[0]) and float(xd.var(unbiased=False)) == 0.0
        assert float(x.mean()) == float(x[0]) and float(x.var(unbiased=False)) == 0.0, (name, K)
        if with_bias:
            assert torch.equal(y32, y64.float()), (name, K)
            assert torch.equal(y32, lnb), (name, K)
        elif name == "Z":
            assert torch.equal(y32, y64.float()) and not bool(y32.any())
        else:
            assert bool(((y32.double() - y64).abs() <= 4 * 2.0 ** -24 * y64.abs()).all()), (name, K)


@pytest.mark.parametrize("K", KS)
def test_alternating_pixel_variance_is_exact(K):
    """A(a): fp32 mean exactly a, fp32 variance exactly 2^-24, under both s * fl(1 / K) and s / K, in forward and in
    pairwise summation order."""
    for a in dg.C_VALUES:
        x = dg.pattern(f"A({a:g})", K)
        assert float(x.var(unbiased=False)) == dg.A_VAR and float(x.mean()) == a
        s = torch.zeros((), dtype=torch.float32)
        for v in x:                                  # strictly sequential fp32 sum
            s = s + v
        inv = torch.tensor(1.0 / K, dtype=torch.float32)
        assert float(s * inv) == a and float(s / K) == a, (K, a)
        d = x - a
        q = torch.zeros((), dtype=torch.float32)
        for v in d:
            q = q + v * v
        assert float(q / K) == dg.A_VAR and float(x.double().var(unbiased=False)) == dg.A_VAR
        assert dg.A_VAR < 1e-5 / 100


@pytest.mark.parametrize("K", KS)
def test_one_hot_pixel_reaches_the_bound(K):
    """S: the normalised deviation of channel 0 is sqrt(K - 1) up to eps - the bound of _hip.ln_split_scale."""
    x = dg.pattern("S", K).double()
    d = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-5)
    # var = (K - 1) / K^2, so eps shortens it by 1 / sqrt(1 + eps K^2 / (K - 1)) >= 0.998 at K = 384
    assert 0.998 * (K - 1) ** 0.5 < float(d[0]) <= (K - 1) ** 0.5


def test_patterned_image_places_every_pattern():
    for tile, H, W in (((8, 32), 24, 72), (16, 8, 16), (64, 16, 24)):
        x, lab = dg.patterned_image(f"t{tile}", 2, 48, H, W, tile)
        assert set(lab.unique().tolist()) >= {0, 1, 2, 3, 5, 8}
        assert lab[0, 0] == dg.PATTERNS["Z"] and lab[-1, -1] == dg.PATTERNS["S"]
        for name, code in dg.PATTERNS.items():
            m = lab == code
            if bool(m.any()):
                assert torch.equal(x[1][:, m], dg.pattern(name, 48).view(-1, 1).expand(-1, int(m.sum())))
        if isinstance(tile, tuple):
            th, tw = tile
            assert bool((lab[th + 1:2 * th, tw:2 * tw] == 1).all()) and bool((lab[th + 1:2 * th, 1:tw] == 2).all())
            assert bool(dg.flat_neighbourhood_mask(lab)[th + 2, tw + 2]) and not bool(dg.flat_neighbourhood_mask(lab)[0, 0])


#: the (ledger case, frame) pairs run here: every pair of the GPU file but MaIRUNet's (8 s of CPU per frame; the Restormer
#: variants that share weights and oracle with restormer_wb_64x64_b1 are the same runs)
FOUR = ("black", "flat_hot", "letterbox", "checker")
PAIRS = ([(c, f) for c in ("restormer_wb_64x64_b1", "restormer_bf_64x64_b1") for f in FOUR]
         + [(c, f) for c in ("mair_flat_16x16_b1", "dncnn_color20_29x45_b1", "dncnn_gray17_37x53_b2", "rednet_33x45_b1",
                             "fpn_mobilenet_96x160_b1") for f in dg.FRAMES])


@pytest.mark.parametrize("case,kind", PAIRS)
def test_oracles_are_finite_on_frames(case, kind):
    """Float32 and float64 oracle outputs (Restormer: `out` and the `refinement` tap) are finite and differ, so the bar
    K e_32 + F max|y64| of the GPU ledger has a yardstick on every frame.  The one exception is exact: a bias-free network
    maps a black tile to zeros at every layer, in both precisions."""
    factory, shape, (lo, hi), fn, _ = CASES[case]
    p = cpu_params(factory().load_synthetic(42))
    x = dg.frame(kind, shape, lo, hi)
    t32, t64 = {}, {}
    with torch.no_grad():
        y32 = dict(out=fn(x, p, t32), **t32)
        y64 = dict(out=fn(x.double(), f64(p), t64), **t64)
    assert set(y32) == set(y64) and ("refinement" in y64) == case.startswith("restormer")
    for row in y64:
        assert bool(torch.isfinite(y32[row]).all()) and bool(torch.isfinite(y64[row]).all()), row
        if case == "restormer_bf_64x64_b1" and kind == "black":
            assert not bool(y32[row].any()) and not bool(y64[row].any()), row
        else:
            assert float((y32[row].double() - y64[row]).abs().max()) > 0.0, row
