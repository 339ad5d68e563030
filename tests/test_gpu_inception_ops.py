"""GPU tests of the kernels of FPN-Inception's encoder against float64 torch.nn.functional: irm_convkxk_f32 (every built
geometry, the block closer among them), irm_pool3x3_f32, guard bands around every operand of both, and one Block35 and one
Block17 of the model against the plain-torch helper (tests/inception_model.py).  Tolerance: block_model.FPN_TOL on O(1)
data."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import guards
import inception_model as im
from block_model import FPN_TOL as TOL
from irm_amd import _hip, ops, synth
from irm_amd.deblurganv2.models import fpn_inception as fi

pytestmark = pytest.mark.gpu

SENTINEL = guards.SENTINEL


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(777, name, shape, lo, hi)


def weight(name, co, ci, kh, kw):
    a = (3.0 / (ci * kh * kw)) ** 0.5                # unit-variance outputs from U(-1, 1) inputs
    return rnd(name, (co, ci, kh, kw), -a, a)


#: (kh, kw, stride, (pad_h, pad_w)): the five geometries the stock kernels lack, and the 1x1 of the block closer
GEOMETRIES = [(3, 3, 2, (0, 0)), (3, 3, 1, (0, 0)), (5, 5, 1, (2, 2)), (1, 7, 1, (0, 3)), (7, 1, 1, (3, 0)), (1, 1, 1, (0, 0))]
#: output sizes (OH, OW): widths 1, 3, 33 and 65 - below a tile, one tile plus one column, two tiles plus one column
OUT_SIZES = [(1, 1), (9, 3), (3, 33), (2, 65)]
#: (bias, act1, residual, relu2); "inplace": the residual is the output buffer itself, as the block closer runs it
EPILOGUES = [(False, False, None, False), (True, True, None, False), (True, False, "inplace", True), (True, True, "other", False),
             (False, False, "other", True), (False, True, None, True)]


def in_size(o, k, s, p, even):
    """An input extent that gives `o` outputs; under stride 2 the even extent has a last row / column no window reaches."""
    n = (o - 1) * s + k - 2 * p
    return n + 1 if (s == 2 and even) else n


def conv_reference(x, w, b, s, pad, act1, res, relu2):
    y = F.conv2d(x.double(), w.double(), None if b is None else b.double(), s, pad)
    if act1:
        y = F.relu(y)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu2 else y


@pytest.mark.parametrize("kh,kw,s,pad", GEOMETRIES, ids=lambda v: str(v).replace(" ", ""))
def test_convkxk_geometry(dev, kh, kw, s, pad):
    """Ci in {3, 5, 48} x Co in {16, 20, 80} x the four output sizes (x both parities under stride 2), B = 2, the output a
    channel slice of a larger buffer whose other channels must come back untouched, the epilogues and the built ct values
    in rotation, explicit and planned ygroups; a second run is bit-identical."""
    top = ops.CONVKXK_GEOMETRIES[(kh, kw, s)]
    cts = [c for c in (1, 2, 4) if c <= top]
    B, n, worst, seen = 2, 0, 0.0, set()
    for ci, co in itertools.product((3, 5, 48), (16, 20, 80)):
        w = weight(f"w{kh}{kw}{s}_{ci}_{co}", co, ci, kh, kw)
        wp = _hip.pack_convkxk_weight(w).to(dev)
        bias = rnd(f"b{co}", (co,))
        for (oh, ow), even in itertools.product(OUT_SIZES, (False, True) if s == 2 else (False,)):
            H, W = in_size(oh, kh, s, pad[0], even), in_size(ow, kw, s, pad[1], even)
            use_b, act1, res_kind, relu2 = EPILOGUES[n % len(EPILOGUES)]
            ct = cts[(n // 2) % len(cts)]
            yg = (None, 1, 2)[n % 3]
            n += 1
            seen.add((use_b, act1, res_kind, relu2, ct))
            x = rnd(f"x{ci}_{H}_{W}", (B, ci, H, W))
            r = rnd(f"r{co}_{oh}_{ow}", (B, co, oh, ow)) if res_kind else None
            ref = conv_reference(x, w, bias if use_b else None, s, pad, act1, r, relu2)
            assert tuple(ref.shape) == (B, co, oh, ow)
            # the output: channels 3 .. 3 + co of a [B, co + 5] buffer, 0 or 2 floats into its allocation
            flat, y = guards.channel_slice(dev, B, co, 5, 3, oh, ow, (0, 2)[n % 2], SENTINEL)
            rg = None
            if res_kind == "inplace":
                y.copy_(r)
                rg = y
            elif res_kind == "other":
                rg = r.to(dev)
            args = dict(stride=s, pad=pad, bias=bias.to(dev) if use_b else None, relu1=act1, res=rg, relu2=relu2, ct=ct,
                        ygroups=yg)
            ops.convkxk(wp, x.to(dev), y, ci, co, kh, kw, **args)
            got = y.cpu()
            err = float((got.double() - ref).abs().max())
            worst = max(worst, err)
            assert err < TOL, (ci, co, H, W, args["relu1"], res_kind, relu2, ct, yg, err)
            mask = torch.ones_like(flat, dtype=torch.bool)
            mask.as_strided(y.shape, y.stride(), y.storage_offset()).fill_(False)
            assert bool((flat[mask] == SENTINEL).all()), ("a write outside the channel slice", ci, co, H, W)
            if res_kind == "inplace":
                y.copy_(r)
            ops.convkxk(wp, x.to(dev), y, ci, co, kh, kw, **args)
            assert torch.equal(y.cpu(), got), "second run differs"
    assert {c for *_, c in seen} == set(cts) and {e[:4] for e in seen} == set(EPILOGUES)
    print(f"convkxk {kh}x{kw} s{s}: {n} cases, worst max-abs error {worst:.3e}")


def test_convkxk_stride2_ignores_the_unreached_row_and_column(dev):
    """An even input under 3x3 stride 2: the last row and column reach no window.  Poisoned with NaN, they must not
    change the result, which equals that of the odd input without them bit for bit."""
    ci, co = 5, 20
    w = weight("wpar", co, ci, 3, 3)
    wp = _hip.pack_convkxk_weight(w).to(dev)
    x = rnd("xpar", (2, ci, 11, 67))
    xe = torch.full((2, ci, 12, 68), float("nan"))
    xe[:, :, :11, :67] = x
    ya, yb = torch.empty(2, co, 5, 33, device=dev), torch.empty(2, co, 5, 33, device=dev)
    ops.convkxk(wp, x.to(dev), ya, ci, co, 3, 3, stride=2)
    ops.convkxk(wp, xe.to(dev), yb, ci, co, 3, 3, stride=2)
    assert torch.equal(ya, yb) and not guards.has_nan(yb)


def test_convkxk_block_closer_at_the_models_widths(dev):
    """relu(x + s (W cat + b)) with s folded into the packed weight and bias, at the channel counts of Block35 and
    Block17, planned launch, in place, the concat a channel slice of the block's buffer."""
    for cat_c, c, scale, h, w_ in ((128, 320, 0.17, 9, 13), (384, 1088, 0.10, 6, 8)):
        wt, b = weight(f"cw{c}", c, cat_c, 1, 1), rnd(f"cb{c}", (c,))
        buf = rnd(f"cbuf{c}", (2, cat_c + 64, h, w_)).to(dev)
        x = rnd(f"cx{c}", (2, c, h, w_), -2.0, 2.0)
        ref = F.relu(x.double() + scale * F.conv2d(buf[:, 64:].cpu().double(), wt.double(), b.double()))
        y = x.to(dev)
        ops.convkxk(_hip.pack_convkxk_weight(wt, scale).to(dev), buf[:, 64:], y, cat_c, c, 1, 1,
                    bias=(b.double() * scale).float().to(dev), res=y, relu2=True)
        assert float((y.cpu().double() - ref).abs().max()) < TOL


# --------------------------------------------------------------------------- pooling
def pool_case(dev, mode, B, C, H, W, lo, hi):
    x = rnd(f"p{mode}_{H}_{W}", (B, C, H, W), lo, hi)
    ref = (F.max_pool2d(x.double(), 3, 2) if mode == ops.POOL_MAX_S2
           else F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False))
    oh, ow = ref.shape[2:]
    flat, y = guards.channel_slice(dev, B, C, 4, 2, oh, ow, 2, SENTINEL)
    ops.pool3x3(x.to(dev), y, mode)
    mask = torch.ones_like(flat, dtype=torch.bool)
    mask.as_strided(y.shape, y.stride(), y.storage_offset()).fill_(False)
    assert bool((flat[mask] == SENTINEL).all())
    return y.cpu(), ref


@pytest.mark.parametrize("H,W", [(3, 3), (4, 5), (30, 38)])
def test_max_pool_on_all_negative_data(dev, H, W):
    """MaxPool2d(3, 2): the maximum starts at -inf, so all-negative planes give negative maxima (a start at 0 gives 0);
    4x5 has a row and columns no window reaches."""
    y, ref = pool_case(dev, ops.POOL_MAX_S2, 2, 5, H, W, -3.0, -0.5)
    assert tuple(y.shape[2:]) == ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
    assert torch.equal(y.double(), ref) and float(y.max()) < 0.0


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (13, 17)])
def test_avg_pool_divides_by_the_taps_inside(dev, H, W):
    """AvgPool2d(3, 1, 1, count_include_pad=False): 4 taps at a corner, 6 at an edge, 9 inside (1 for a 1x1 image)."""
    y, ref = pool_case(dev, ops.POOL_AVG_S1, 2, 5, H, W, -1.0, 2.0)
    assert float((y.double() - ref).abs().max()) < 1e-6
    ones = torch.ones(1, 1, H, W, device=dev)
    out = torch.empty_like(ones)
    ops.pool3x3(ones, out, ops.POOL_AVG_S1)
    assert torch.equal(out, ones)                    # the divisor is the number of taps that were summed


# --------------------------------------------------------------------------- guard bands
def test_guard_bands_convkxk(dev):
    """Every operand of "irm_convkxk_f32" between guard bands: inputs, packed weights, bias and residual between NaNs
    (a value read from outside poisons the result), the output between sentinels with slack between its images; partial
    tiles in both directions, Ci and Co no multiples of 4 and 16, each geometry once."""
    for kh, kw, s, pad in GEOMETRIES:
        B, ci, co, oh, ow = 2, 5, 20, 9, 35
        H, W = in_size(oh, kh, s, pad[0], True), in_size(ow, kw, s, pad[1], True)
        g = guards.Guards(dev)
        w = weight(f"gw{kh}{kw}{s}", co, ci, kh, kw)
        x, b, r = rnd("gx", (B, ci, H, W)), rnd("gb", (co,)), rnd("gr", (B, co, oh, ow))
        xg, rg = g.inp(x, guards.SLACK), g.inp(r, guards.SLACK)
        wg, bg = g.inp(_hip.pack_convkxk_weight(w)), g.inp(b)
        y = g.out("y", (B, co, oh, ow), slack=guards.SLACK)
        _hip.call("irm_convkxk_f32", _hip.ptr(wg), _hip.ptr(xg), xg.stride(0), _hip.ptr(y), y.stride(0), _hip.ptr(rg),
                  rg.stride(0), _hip.ptr(bg), B, ci, co, H, W, kh, kw, s, pad[0], pad[1], 1, 1, 1, 2, 2)
        g.check()
        ref = conv_reference(x, w, b, s, pad, True, r, True)
        assert float((guards.clean(y).double() - ref).abs().max()) < TOL, (kh, kw, s)


def test_guard_bands_pool3x3(dev):
    """ "irm_pool3x3_f32" in both modes: the input between NaNs, the output between sentinels, odd and even extents."""
    for mode, (H, W) in itertools.product((0, 1), ((7, 9), (8, 10), (3, 3))):
        B, C = 2, 3
        g = guards.Guards(dev)
        x = rnd(f"gp{H}", (B, C, H, W), -2.0, -1.0)
        xg = g.inp(x, guards.SLACK)
        ref = F.max_pool2d(x.double(), 3, 2) if mode == 0 else F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False)
        y = g.out("y", tuple(ref.shape), slack=guards.SLACK)
        _hip.call("irm_pool3x3_f32", _hip.ptr(xg), xg.stride(0), _hip.ptr(y), y.stride(0), B, C, H, W, mode)
        g.check()
        assert float((guards.clean(y).double() - ref).abs().max()) < 1e-6, (mode, H, W)


# --------------------------------------------------------------------------- whole blocks
def _load(dst, src):
    dst.load_state_dict({k: v.float() for k, v in src.state_dict().items()})
    return dst


@pytest.mark.parametrize("kind,h,w", [("block35", 9, 13), ("block17", 6, 8)])
def test_block_against_the_helper(dev, kind, h, w):
    """One residual block as the model runs it - merged head GEMM, branches into the slices of one buffer, closer with
    the folded scale - against the helper's block in float64; also in place, as every block but the first runs."""
    torch.manual_seed(11)
    ref_blk = (im.Block35() if kind == "block35" else im.Block17()).double()
    for k, p in ref_blk.named_parameters():
        if k.endswith("bn.weight"):
            p.data.copy_(rnd(kind + k, p.shape, 0.6, 1.4))
        elif k.endswith("bn.bias") or k.endswith("conv2d.bias"):
            p.data.copy_(rnd(kind + k, p.shape, -0.3, 0.3))
    c, nbuf = (320, 192) if kind == "block35" else (1088, 512)
    x = rnd(kind + "x", (2, c, h, w), 0.0, 2.0)
    with torch.no_grad():
        ref = ref_blk(x.double())
    blk = _load(fi.Block35() if kind == "block35" else fi.Block17(), ref_blk).to(dev)
    d = fi.pack_block35(blk) if kind == "block35" else fi.pack_block17(blk)
    run = fi.run_block35 if kind == "block35" else fi.run_block17
    xg = x.to(dev)
    buf = torch.empty(2, nbuf, h, w, device=dev)
    out = run(d, xg, buf, torch.empty_like(xg))
    err = float((out.cpu().double() - ref).abs().max())
    print(f"{kind} {h}x{w}: max-abs error {err:.3e} on values up to {float(ref.abs().max()):.2f}")
    assert err < TOL and torch.equal(xg.cpu(), x)
    again = run(d, xg, buf, xg)
    assert again is xg and torch.equal(again, out)
