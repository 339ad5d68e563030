"""Plain-torch model of the pieces of a Restormer TransformerBlock, the layouts the kernels exchange them in, and the bars
the kernel tests hold them to.

Every function computes in the dtype (and on the device) of the activations it is given and casts its parameters to that
dtype itself: called on x.double() it is the float64 reference of a test, called on x it is the float32 chain behind an
e_32, and the two are the same code.  float32 -> float64 casts are exact, so a parameter may arrive in either.
tests/test_block_model_cpu.py pins layer_norm, gdfn and qkv + attention to oracle/restormer_ref.py, the oracle that
tests/test_cpu.py pins to the recorded reference outputs.

Plain functions, no fixtures and no tests: a kernel test imports this model and does not restate it."""
import torch
import torch.nn.functional as TF

from irm_amd import _hip, ops

# --------------------------------------------------------------------------- bars
#: the precision ledger's bar (tests/test_gpu_precision.py): e_gpu <= K * e_32 + F * max|y64|, ONE pair for every file
K = 4.0
F = 2.0 ** -22
#: fp32 kernels vs float64, absolute on O(1) data (tests/test_gpu_ops.py; the path's budget is 1e-3 max-abs)
OPS_TOL = 2e-4
#: the whole-branch fused kernels vs float64, per unit of max(1, |ref|max) (tests/test_gpu_fused.py)
FUSED_TOL = 2e-5
#: the FPN-MobileNet kernels vs float64 (tests/test_gpu_deblurgan.py)
FPN_TOL = 2e-4


def passes(e, e32, ymax):
    return e <= K * e32 + F * ymax


def record_calls(reached):
    """Generator body of a module's autouse entry-point fixture (`yield from record_calls(_REACHED)`): while it is
    suspended every _hip.call adds the entry point's name to `reached`."""
    real = _hip.call

    def call(name, *args):
        reached.add(name)
        return real(name, *args)
    _hip.call = call
    try:
        yield
    finally:
        _hip.call = real


# --------------------------------------------------------------------------- LayerNorm over the channels
def _chan(p, x, dim):
    shape = [1] * x.dim()
    shape[dim] = -1
    return p.to(x.dtype).view(shape)


def layer_norm(x, lnw, lnb, ln, eps=1e-5, dim=1):
    """ln 0: x itself; 1 (WithBias): (x - mu) / sqrt(var + eps) * w + b; 2 (BiasFree): x / sqrt(var + eps) * w, mu and the
    biased var over `dim`."""
    if not ln:
        return x
    mu, var = x.mean(dim, keepdim=True), x.var(dim, unbiased=False, keepdim=True)
    xn = ((x - mu) if ln == 1 else x) / torch.sqrt(var + eps) * _chan(lnw, x, dim)
    return xn + _chan(lnb, x, dim) if ln == 1 else xn


def ln_stats(x, eps=1e-5, dim=1):
    """(mean, rstd) over `dim`, that axis dropped: what irm_ln_stats_f32 and a stats_out epilogue write (dim -1 over the
    flattened pixels: the InstanceNorm statistics of a plane)."""
    return x.mean(dim), 1.0 / torch.sqrt(x.var(dim, unbiased=False) + eps)


# --------------------------------------------------------------------------- the two branches
def _conv1x1(x, w, b):
    return TF.conv2d(x, w.to(x.dtype)[:, :, None, None], None if b is None else b.to(x.dtype))


def _dw3x3(x, w, b):
    M = w.shape[0]
    return TF.conv2d(x, w.to(x.dtype).view(M, 1, 3, 3), None if b is None else b.to(x.dtype), padding=1, groups=M)


def gdfn_from_ln(x1, xn, pin_w, pin_b, dw_w, dw_b, pout_w, pout_b, gate_sat=None):
    """x1 + project_out(gelu(dw(h)[:hid]) * dw(h)[hid:]), h = project_in(xn), from the LayerNorm output xn on; gate_sat: the
    gate limited to +-gate_sat, where the fused kernels limit it.  Returns (y, [B][H][W] mask of the pixels with a gate value
    beyond the limit)."""
    hid = pout_w.shape[1]
    h = _dw3x3(_conv1x1(xn, pin_w, pin_b), dw_w, dw_b)
    g = TF.gelu(h[:, :hid]) * h[:, hid:]
    beyond = torch.zeros(g.shape[0], g.shape[2], g.shape[3], dtype=torch.bool, device=g.device)
    if gate_sat is not None:
        beyond = (g.abs() > gate_sat).any(1)
        g = g.clamp(-gate_sat, gate_sat)
    return x1 + _conv1x1(g, pout_w, pout_b), beyond


def gdfn(x, lnw, lnb, ln, pin_w, pin_b, dw_w, dw_b, pout_w, pout_b, eps=1e-5):
    """x + GDFN(LN(x)) (restormer.py:25-70, 148)."""
    return gdfn_from_ln(x, layer_norm(x, lnw, lnb, ln, eps), pin_w, pin_b, dw_w, dw_b, pout_w, pout_b)[0]


def gdfn_operands(rnd, tag, C, hid, ln, bias=True, ws=0.3):
    """(lnw, lnb, pin_w, pin_b, dw_w, dw_b, pout_w, pout_b) of a GDFN branch from a test file's own seeded
    rnd(name, shape, lo, hi), in the ranges the fused-branch tests draw: lnb None under BiasFree, the biases None without `bias`."""
    b = (lambda n, m: rnd(tag + n, (m,), -0.3, 0.3)) if bias else (lambda n, m: None)
    return (rnd(tag + "lw", (C,), 0.5, 1.5), rnd(tag + "lb", (C,), -0.2, 0.2) if ln == 1 else None,
            rnd(tag + "pi", (2 * hid, C), -ws, ws), b("pib", 2 * hid), rnd(tag + "dw", (2 * hid, 9), -0.4, 0.4), b("dwb", 2 * hid),
            rnd(tag + "po", (C, hid), -ws, ws), b("pob", C))


def qkv_from_ln(xn, w, b, dw_w, dw_b):
    """dw3x3(conv1x1(xn)): q, k, v stacked on the channel axis."""
    return _dw3x3(_conv1x1(xn, w, b), dw_w, dw_b)


def qkv(x, lnw, lnb, ln, w, b, dw_w, dw_b, eps=1e-5):
    return qkv_from_ln(layer_norm(x, lnw, lnb, ln, eps), w, b, dw_w, dw_b)


def attention(q, k, temp, heads):
    """Attention matrix [B][heads][c][c] of planar q, k [B][C][H][W]: softmax(normalize(q) normalize(k)^T * temp)."""
    B, C = q.shape[:2]
    q, k = q.reshape(B, heads, C // heads, -1), k.reshape(B, heads, C // heads, -1)
    return torch.softmax(TF.normalize(q, dim=-1) @ TF.normalize(k, dim=-1).transpose(-1, -2) * temp.to(q.dtype).view(1, heads, 1, 1), -1)


def attention_qk(qk, temp, heads):
    """attention() of q, k = the two halves of a [B][2C][H][W] tensor."""
    C = qk.shape[1] // 2
    return attention(qk[:, :C], qk[:, C:], temp, heads)


def run_mdta_fold(dev, qkv, temp, wout, C, heads, part=None, **kw):
    """ops.mdta_fold on a device qkv with fresh workspaces (part pre-filled with NaN unless given): the (attention, packed
    folded matrix, summed Gram records) on the host."""
    B, _, H, W = qkv.shape
    _, nchunk, rec = ops.mdta_plan(B, C, heads, H * W)
    if part is None:
        part = torch.full((B * heads * (kw.get("nchunk_ready") or nchunk) * rec,), float("nan"), device=dev)
    gsum = torch.empty(B * heads * rec, device=dev)
    mfold = torch.zeros(B * ops.mfold_numel(C), device=dev)
    attn = torch.empty(B, heads, C // heads, C // heads, device=dev)
    ops.mdta_fold(qkv, part, gsum, temp.to(dev), wout.to(dev), mfold, C, heads, attn=attn, **kw)
    return attn.cpu(), mfold.cpu(), gsum.cpu()


def act(y, code):
    """The activation codes of include/irm_hip.h: 0 none, 1 ReLU, 2 GELU, 3 SiLU."""
    return {0: lambda t: t, 1: torch.relu, 2: TF.gelu, 3: TF.silu}[code](y)


def conv_epilogue(y, r=None, relu1=False, res_mode=0, relu2=False, store_mode=0, shuffle=2, leaky=None):
    """The epilogue chain of the dense 3x3 conv kernels on a conv output y [B][Co][H][W] (bias added), in y's dtype: relu1 or
    LeakyReLU, the residual (1: y + r, 2: r - y, 3: clamp(tanh(y) + r, -1, 1)), relu2, PixelUnshuffle(2) (store 1) or
    PixelShuffle (store 2).  How the conv itself is summed stays each test's own (F.conv2d, or a per-tap einsum)."""
    if relu1:
        y = torch.relu(y)
    if leaky is not None:
        y = torch.where(y > 0, y, y * torch.tensor(leaky, dtype=torch.float32).to(y.dtype))
    if res_mode:
        r = r.to(y.dtype)
        y = y + r if res_mode == 1 else r - y if res_mode == 2 else (torch.tanh(y) + r).clamp(-1, 1)
    if relu2:
        y = torch.relu(y)
    if store_mode:
        y = TF.pixel_unshuffle(y, 2) if store_mode == 1 else TF.pixel_shuffle(y, shuffle)
    return y


# --------------------------------------------------------------------------- layouts
def to_tm(t):
    """[B][C][H][W] planar -> the same container holding the tile-major channel-last order of include/irm_hip.h
    ([tile][8 x 32 pixels][C])."""
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 8, 8, W // 32, 32).permute(0, 2, 4, 3, 5, 1).reshape(B, C, H, W).contiguous()


def from_tm(t):
    B, C, H, W = t.shape
    return t.reshape(B, H // 8, W // 32, 8, 32, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W).contiguous()


def qk_to_tm(t):
    """q, k: planar -> tile-major CHANNEL-MAJOR [tile][channels][8 x 32] (the tile of (ty, tx) holds channel ch of pixel
    (8 ty + r, 32 tx + c) at [ch][32 r + c]) - another order than to_tm's channel-last one."""
    B, C2, H, W = t.shape
    return t.reshape(B, C2, H // 8, 8, W // 32, 32).permute(0, 2, 4, 1, 3, 5).reshape(B, C2, H, W).contiguous()


def qk_from_tm(t):
    B, C2, H, W = t.shape
    return t.reshape(B, H // 8, W // 32, C2, 8, 32).permute(0, 3, 1, 4, 2, 5).reshape(B, C2, H, W)


def unpack_gemm(wp, M, K):
    """_hip.pack_gemm_weight's [mtile][kstep][g][r] -> [M][K]."""
    mt, ks = (M + 15) // 16, 4 * ((K + 15) // 16)
    return wp.view(mt, ks, 4, 16).permute(0, 3, 1, 2).reshape(mt * 16, ks * 4)[:M, :K]


def unpack_presplit(frag, M, K):
    """fp64 value of the hi + lo fragments written by the host packer / irm_ln_split_f16: [rows][K]."""
    h = frag.view(torch.float16).double().view(-1, K // 32, 2, 4, 16, 8)      # [tile][ks][hi|lo][g][m][e]
    v = (h[:, :, 0] + h[:, :, 1]).permute(0, 3, 1, 2, 4).reshape(-1, K)        # [tile][m][ks][g][e]
    return v[:M]


def unpack_mfold(mf, nb, C):
    """packed [mtile][kstep][lane] (lane = 16 g + r holds M[16 mtile + r][4 kstep + g]) -> [nb][C][C]"""
    mt = C // 16
    return mf.view(nb, mt, 4 * mt, 4, 16).permute(0, 1, 4, 2, 3).reshape(nb, C, C)
