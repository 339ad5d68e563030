"""CPU model of the fp16 inference mode of the conv stacks (csrc/conv3x3_h.hip), float64.

One layer:  xq = the layer's input values, taken exactly (fp16 hidden activations, fp32 for the first layer);
            wq = RNE_fp16(W s) / s for a hidden layer (what _hip.pack_conv3x3_h stores), W itself for the first and
                 the last layer (they run fp32 FMAs on the plain weight);
            v  = sum wq xq + bias, then the epilogue (relu1, res_mode 1: + res, 2: res - v, relu2), all in float64;
            S  = sum |wq| |xq| + |bias|  (a conv of absolute values);
            ulp16(v) = the fp16 spacing at |v|, with a floor of 2^-24.
A stored fp16 output y obeys |y - v| <= ulp16(v) / 2 + n 2^-24 S with n = 9 Ci + 4 fp32 operations in the
accumulation chain (products of two fp16 values are exact in fp32); the fp32 output of the last layer obeys
|y - v| <= n 2^-24 S + 2^-23 |v|.  Derived, not measured.

A chain (DnCNN, REDNet) is the same layers with every hidden activation rounded to fp16 once (`run_chain`); with
acc="f32" every layer's sum is a float32 torch CPU conv on the same rounded values: the distance between the two is
the chain's own sensitivity to the summation order.
"""
import numpy as np
import torch
import torch.nn.functional as F

from irm_amd import _hip


def rne16(t: torch.Tensor) -> torch.Tensor:
    """Round to the nearest fp16 value (ties to even, beyond +-65504 -> +-inf, NaN kept), returned in t's dtype.
    numpy converts float64 -> float16 in one step; torch goes through float32 (a double rounding)."""
    with np.errstate(over="ignore", invalid="ignore"):
        q = t.detach().cpu().numpy().astype(np.float16).astype(np.float64)
    return torch.from_numpy(q).to(t.dtype)


def ulp16(v: torch.Tensor) -> torch.Tensor:
    """fp16 spacing at |v| (float64): 2^(floor(log2 |v|) - 10), at least 2^-24 (the subnormal spacing)."""
    a = v.double().abs()
    _, e = torch.frexp(a)                                  # a = m 2^e, m in [0.5, 1)
    u = torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 11).double())
    return torch.where(a < 2.0 ** -14, torch.full_like(u, 2.0 ** -24), u)


def quantised_weight(w: torch.Tensor) -> torch.Tensor:
    """RNE_fp16(W s) / s of a hidden layer, through the product's own packing (float32, exact)."""
    packed, inv = _hip.pack_conv3x3_h(w)
    return _hip.unpack_conv3x3_h(packed, inv, w.shape[0], w.shape[1])


def _epilogue(v, relu1, res, res_mode, relu2):
    if relu1:
        v = torch.relu(v)
    if res_mode == 1:
        v = v + res
    elif res_mode == 2:
        v = res - v
    if relu2:
        v = torch.relu(v)
    return v


def layer(x, w, bias=None, *, relu1=False, res=None, res_mode=0, relu2=False):
    """(v, S) of one layer in float64.  x [B,Ci,H,W] planar (the exact input values), w [Co,Ci,3,3] the weights the
    kernel multiplies with, res planar like the output."""
    x, w = x.double(), w.double()
    b = None if bias is None else bias.double()
    v = F.conv2d(x, w, b, padding=1)
    S = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), padding=1)
    return _epilogue(v, relu1, None if res is None else res.double(), res_mode, relu2), S


def bound_f16(v, S, ci):
    """|y - v| allowed for a stored fp16 output."""
    return ulp16(v) / 2 + (9 * ci + 4) * 2.0 ** -24 * S


def bound_f32(v, S, ci):
    """|y - v| allowed for the fp32 output of the last layer."""
    return (9 * ci + 4) * 2.0 ** -24 * S + 2.0 ** -23 * v.abs()


# --------------------------------------------------------------------------- chains
def dncnn_spec(model, quantise=True):
    """Layer list of an irm_amd DnCNN: dicts kind / w / bias / relu1 / res / res_mode / relu2; res names an earlier
    layer's output by index, or "x" (the network input)."""
    convs = [m for m in model.model if isinstance(m, torch.nn.Conv2d)]
    spec = []
    qw = quantised_weight if quantise else (lambda t: t)
    for i, m in enumerate(convs):
        kind = "in" if i == 0 else "out" if i + 1 == len(convs) else "mid"
        w = m.weight.detach().float().cpu()
        spec.append(dict(kind=kind, w=qw(w) if kind == "mid" else w, bias=m.bias.detach().float().cpu(),
                         relu1=kind != "out", res="x" if kind == "out" else None, res_mode=2 if kind == "out" else 0,
                         relu2=False))
    return spec


def rednet_spec(model, quantise=True):
    spec = []
    qw = quantised_weight if quantise else (lambda t: t)
    for i in range(1, 16):                               # c1..c15 -> layers 0..14
        m = getattr(model, f"conv{i}")
        w = m.weight.detach().float().cpu()
        spec.append(dict(kind="in" if i == 1 else "mid", w=w if i == 1 else qw(w),
                         bias=m.bias.detach().float().cpu(), relu1=True, res=None, res_mode=0, relu2=False))
    for i in range(1, 16):                               # deconv1..15
        m = getattr(model, f"deconv{i}")
        w = _hip.deconv_as_conv_weight(m.weight).float().cpu()
        b = m.bias.detach().float().cpu()
        if i == 15:
            spec.append(dict(kind="out", w=w, bias=b, relu1=False, res="x", res_mode=1, relu2=False))
        elif i % 2 == 1:                                 # relu(relu(deconv) + c_{15-i}): layer index 14 - i
            spec.append(dict(kind="mid", w=qw(w), bias=b, relu1=True, res=14 - i, res_mode=1, relu2=True))
        else:
            spec.append(dict(kind="mid", w=qw(w), bias=b, relu1=True, res=None, res_mode=0, relu2=False))
    return spec


def run_chain(spec, x, acc="f64"):
    """The quantised chain on x [B,C,H,W] (fp32 values): every hidden activation is rounded to fp16 once, the last
    layer is not.  acc "f64": float64 sums; "f32": every layer a float32 torch conv.  Returns float64."""
    dt = torch.float64 if acc == "f64" else torch.float32
    x = x.detach().cpu().float().to(dt)
    outs, cur = [], x
    with torch.no_grad():
        for L in spec:
            v = F.conv2d(cur, L["w"].to(dt), L["bias"].to(dt), padding=1)
            res = None if L["res"] is None else x if L["res"] == "x" else outs[L["res"]]
            v = _epilogue(v, L["relu1"], res, L["res_mode"], L["relu2"])
            if L["kind"] != "out":
                v = rne16(v)
            outs.append(v)
            cur = v
    return cur.double()


def full_precision(spec, x):
    """The same network without any rounding of activations, float64; with a spec built with quantise=False it is the
    fp32 mode's target."""
    x = x.detach().cpu().double()
    outs, cur = [], x
    with torch.no_grad():
        for L in spec:
            v = F.conv2d(cur, L["w"].double(), L["bias"].double(), padding=1)
            res = None if L["res"] is None else x if L["res"] == "x" else outs[L["res"]]
            v = _epilogue(v, L["relu1"], res, L["res_mode"], L["relu2"])
            outs.append(v)
            cur = v
    return cur
