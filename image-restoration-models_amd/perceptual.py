"""Perceptual distance: LPIPS v0.1, net='alex', eval mode, restated in float64 on the host and
run on the GPU between two kernels of its own (irm_lpips_pack, irm_lpips_head) and the conv trunk the package has.

The definition, for a prediction p and a target t, two 3-channel frames of one shape:

  1. Input values.  v = 2 x - 1 with x in [0, 1]: x = code / 255 for uint8, code / 65535 for uint16 and the value itself
     for float32 (taken as in [0, 1] by contract).  The scaling layer gives u_c = (v_c - shift_c) / scale_c with
     shift = (-.030, -.088, -.188) and scale = (.458, .448, .450), channels in RGB order.
  2. Trunk.  torchvision's AlexNet `features`, tapped after each of its five ReLUs (TRUNK_ALEX):
       conv 11x11 s4 p2 3->64, ReLU (tap 1); maxpool 3 s2, conv 5x5 p2 64->192, ReLU (tap 2);
       maxpool 3 s2, conv 3x3 p1 192->384, ReLU (tap 3); conv 3x3 p1 384->256, ReLU (tap 4);
       conv 3x3 p1 256->256, ReLU (tap 5).
     Every conv has a bias; the state-dict keys are features.{0,3,6,8,10}.{weight,bias}; classifier.* is dropped.
  3. Head.  Per tap l with maps f, g [C_l, H_l, W_l] and lin_l [C_l] (key lin{l}.model.1.weight, [1, C_l, 1, 1], used as
     given, no sign check), n_f(y, x) = sqrt(sum_c f_c^2):
       d_l = mean_{y,x} sum_c lin_l[c] ( f_c / (n_f + 1e-10) - g_c / (n_g + 1e-10) )^2.
  4. LPIPS = sum_l d_l.

A frame needs H, W >= 31 (below that the second pool has no output).  The package ships no weights: the caller names
the two files, as for every model here.  The reference has no perceptual metric; this is the number the deblurring and
super-resolution literature prints beside PSNR and SSIM."""
from __future__ import annotations

import itertools

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip, ops
from .frames import device_constant

LPIPS_SHIFT = (-.030, -.088, -.188)
LPIPS_SCALE = (.458, .448, .450)
LPIPS_EPS = 1e-10
LPIPS_MIN_SIDE = 31
#: the trunk as a table of layers: (state-dict prefix, C_out, C_in, kernel, stride, pad, max-pool 3 s2 before the conv);
#: every conv is followed by a ReLU and a tap
TRUNK_ALEX = (("features.0", 64, 3, 11, 4, 2, False),
              ("features.3", 192, 64, 5, 1, 2, True),
              ("features.6", 384, 192, 3, 1, 1, True),
              ("features.8", 256, 384, 3, 1, 1, False),
              ("features.10", 256, 256, 3, 1, 1, False))
_PEAK = {"uint8": 255.0, "uint16": 65535.0, "int16": 65535.0, "float32": 1.0}
_tokens = itertools.count()


class LpipsParams:
    """The AlexNet trunk and the five lin vectors on the host: `convs` [(weight, bias)] float32 as loaded, `lin` [C_l]
    float32, `w3` the first conv re-laid for the space-to-depth frame ([64, 48, 3, 3]), and the packed operands of the
    kernels.  Device copies are made once per device (frames.device_constant)."""

    def __init__(self, convs, lin):
        self.convs, self.lin = convs, lin
        self.w3 = space_to_depth_weight(convs[0][0])
        self._token = next(_tokens)
        self._packed = None

    def _host_packed(self):
        if self._packed is None:
            p = [_hip.pack_convkxk_weight(self.w3), _hip.pack_convkxk_weight(self.convs[1][0])]
            p += [_hip.pack_conv3x3(w) for w, _ in self.convs[2:]]
            self._packed = p
        return self._packed

    def on(self, device):
        """(packed weights, biases, lin vectors) on `device`."""
        def build():
            def move(p):
                if isinstance(p, _hip.ConvWeight):
                    return _hip.ConvWeight(p.exact.to(device), None if p.split is None else p.split.to(device),
                                           p.inv_scale)
                return p.to(device)
            return ([move(p) for p in self._host_packed()], [b.to(device) for _, b in self.convs],
                    [v.to(device) for v in self.lin])
        return device_constant(("lpips", str(device), self._token), build)


def space_to_depth_weight(w: torch.Tensor) -> torch.Tensor:
    """The 11 x 11 stride-4 kernel [O, 3, 11, 11] as the 3 x 3 stride-1 kernel over the space-to-depth frame:
    W3[o][c 16 + i 4 + j][a][b] = W12[o][c][4 a + i][4 b + j], W12 the kernel zero extended to 12 x 12."""
    o, c = w.shape[:2]
    w12 = torch.zeros(o, c, 12, 12, dtype=w.dtype)
    w12[:, :, :11, :11] = w
    return w12.view(o, c, 3, 4, 3, 4).permute(0, 1, 3, 5, 2, 4).reshape(o, c * 16, 3, 3).contiguous()


def _strip(state, what):
    if not isinstance(state, dict):
        raise ValueError(f"{what}: a state dict is needed, not {type(state).__name__}")
    return {(k[7:] if isinstance(k, str) and k.startswith("module.") else k): v for k, v in state.items()}


def _tensor(state, key, shape, what):
    if key not in state:
        raise ValueError(f"{what}: no {key}")
    t = state[key]
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {key} is a {type(t).__name__}, not a tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {key} has shape {tuple(t.shape)}, not {tuple(shape)}")
    return t.detach().to("cpu", torch.float32).contiguous()


def lpips_params_from_state(alex_state: dict, lin_state: dict) -> LpipsParams:
    """LpipsParams from the two state dicts (a `module.` prefix is tolerated, classifier.* and any other key ignored).
    ValueError for a missing key, a value that is no tensor or another shape."""
    alex, lin = _strip(alex_state, "AlexNet weights"), _strip(lin_state, "LPIPS lin weights")
    convs = [(_tensor(alex, f"{p}.weight", (co, ci, k, k), "AlexNet weights"),
              _tensor(alex, f"{p}.bias", (co,), "AlexNet weights")) for p, co, ci, k, _, _, _ in TRUNK_ALEX]
    lins = [_tensor(lin, f"lin{l}.model.1.weight", (1, t[1], 1, 1), "LPIPS lin weights").reshape(-1).contiguous()
            for l, t in enumerate(TRUNK_ALEX)]
    return LpipsParams(convs, lins)


def load_lpips_params(alexnet_path, lin_path) -> LpipsParams:
    """The parameters LPIPS scores with, from torchvision's AlexNet checkpoint and the `lpips` package's alex.pth,
    both read with weights_only=True.  The package ships no copy: the caller names the files, as for weights."""
    alex = torch.load(alexnet_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    return lpips_params_from_state(alex, lin)


def _check_params(params) -> None:
    if not isinstance(params, LpipsParams):
        raise ValueError("params must be what load_lpips_params or lpips_params_from_state returns")


def _check_pair(shape_p, dtype_p, shape_t, dtype_t, dtypes) -> tuple:
    if tuple(shape_p) != tuple(shape_t) or dtype_p != dtype_t:
        raise ValueError(f"prediction {tuple(shape_p)} {dtype_p} and target {tuple(shape_t)} {dtype_t} differ in shape "
                         "or dtype")
    if dtype_p not in dtypes:
        raise ValueError(f"LPIPS takes uint8, uint16 or float32 frames, not {dtype_p}")
    if len(shape_p) != 3 or shape_p[2] != 3:
        raise ValueError(f"LPIPS takes HWC frames with 3 channels, not shape {tuple(shape_p)}")
    h, w = int(shape_p[0]), int(shape_p[1])
    if min(h, w) < LPIPS_MIN_SIDE:
        raise ValueError(f"frame {h}x{w}: LPIPS needs both sides >= {LPIPS_MIN_SIDE} (the second pool has no output "
                         "below that)")
    return h, w


# --------------------------------------------------------------------------- the float64 host statement
def _features_host(img: np.ndarray, params: LpipsParams) -> list:
    x = torch.from_numpy(np.ascontiguousarray(img).astype(np.float64)) / _PEAK[img.dtype.name]
    v = 2.0 * x - 1.0
    u = (v - torch.tensor(LPIPS_SHIFT, dtype=torch.float64)) / torch.tensor(LPIPS_SCALE, dtype=torch.float64)
    t = u.permute(2, 0, 1).unsqueeze(0)
    taps = []
    for (_, _, _, _, stride, pad, pool), (w, b) in zip(TRUNK_ALEX, params.convs):
        if pool:
            t = F.max_pool2d(t, 3, 2)
        t = F.relu(F.conv2d(t, w.double(), b.double(), stride=stride, padding=pad))
        taps.append(t[0])
    return taps


def lpips_head_host(f: torch.Tensor, g: torch.Tensor, lin: torch.Tensor) -> float:
    """d_l of two float64 maps [C, H, W] and lin [C], as the definition writes it."""
    f, g, lin = f.double(), g.double(), lin.double()
    nf = torch.sqrt((f * f).sum(0, keepdim=True))
    ng = torch.sqrt((g * g).sum(0, keepdim=True))
    d = (f / (nf + LPIPS_EPS) - g / (ng + LPIPS_EPS)) ** 2
    return float((d * lin.view(-1, 1, 1)).sum(0).mean())


def lpips_taps(pred: np.ndarray, target: np.ndarray, params: LpipsParams) -> list:
    """The five d_l of one pair of numpy frames, float64 on the host."""
    _check_params(params)
    for a in (pred, target):
        if not isinstance(a, np.ndarray):
            raise ValueError("calculate_lpips takes numpy arrays (calculate_lpips_device takes GPU tensors)")
    _check_pair(pred.shape, pred.dtype, target.shape, target.dtype, (np.uint8, np.uint16, np.float32))
    fp, ft = _features_host(pred, params), _features_host(target, params)
    return [lpips_head_host(f, g, lin) for f, g, lin in zip(fp, ft, params.lin)]


def calculate_lpips(pred: np.ndarray, target: np.ndarray, params: LpipsParams) -> float:
    """LPIPS of two uint8 / uint16 / float32 HWC numpy frames: the definition above as a torch-CPU float64 chain with
    the first layer as the 11 x 11 stride-4 conv it is.  Slow, and meant to be: it is the statement the GPU path is
    held to.  Identical frames give exactly 0.0 and the value is symmetric in its two frames."""
    return float(sum(lpips_taps(pred, target, params)))


# --------------------------------------------------------------------------- the device path
_KIND = {torch.uint8: 0, torch.uint16: 1, torch.int16: 1, torch.float32: 2}


def _affine(dtype) -> tuple:
    """(a, b): u_c = fma(raw, a_c, b_c), made in float64 and rounded once to float32."""
    peak = _PEAK[str(dtype).replace("torch.", "")]
    a = [float(np.float32(2.0 / (peak * s))) for s in LPIPS_SCALE]
    b = [float(np.float32((-1.0 - m) / s)) for m, s in zip(LPIPS_SHIFT, LPIPS_SCALE)]
    return a, b


def _frame_layout(t: torch.Tensor) -> tuple:
    """(tensor to read, row pitch in samples): a frame whose rows are dense is read where it lies, anything else is
    copied first."""
    if t.dtype == torch.uint16:
        t = t.view(torch.int16)
    h, w, _ = t.shape
    if t.stride(2) == 1 and t.stride(1) == 3 and (h == 1 or t.stride(0) >= 3 * w):
        return t, int(t.stride(0))
    return t.contiguous(), 3 * w


def lpips_pack(frame: torch.Tensor, z: torch.Tensor, index: int = 0) -> None:
    """Frame [H, W, 3] (uint8, uint16 or its int16 bit pattern, float32; rows may be pitched) -> z[index], z a dense
    [B, 48, OH + 2, OW + 2] float32 tensor (irm_lpips_pack)."""
    src, pitch = _frame_layout(frame)
    h, w, _ = src.shape
    a, b = _affine(frame.dtype)
    n = z[index].numel()
    ops._launch("lpips_pack", 6.0 * h * w, float(src.element_size() * 3 * h * w + 4 * n), "irm_lpips_pack",
                _hip.ptr(src), _KIND[frame.dtype], 1, h, w, pitch, (h - 1) * pitch + 3 * w, *a, *b,
                _hip.ptr(z[index]), n, tag=f"{str(frame.dtype)[6:]} {h}x{w}")


def lpips_head(f: torch.Tensor, lin: torch.Tensor, out: torch.Tensor, column: int, ws: torch.Tensor) -> None:
    """out[k, column] = d_l of the maps f[k] and f[K + k], f a [2K, C, H, W] float32 tensor with a free batch stride,
    out a dense [K, n] float64 tensor, ws a float64 workspace of at least K ceil(H W / 64) elements (irm_lpips_head)."""
    ops._chk(f, "f")
    b2, c, h, w = f.shape
    k = b2 // 2
    ops._launch("lpips_head", 8.0 * b2 * c * h * w, 8.0 * b2 * c * h * w, "irm_lpips_head", _hip.ptr(f), ops._bs(f),
                _hip.ptr(lin), k, c, h, w, _hip.ptr(out) + 8 * column, out.stride(0), _hip.ptr(ws), ws.numel(),
                tag=f"C{c} {h}x{w} K{k}")


def frame_lpips_device(preds, targets, params: LpipsParams) -> torch.Tensor:
    """LPIPS of K pairs of device frames of one shape and dtype (uint8, uint16 or its int16 bit pattern, float32;
    [H, W, 3], rows may be pitched): a [K, 6] float64 device tensor, the five d_l and their sum, without synchronising.
    The 2K frames go through the trunk as one batch, so every layer launches once.  A pair's row does not depend on the
    call it is part of beyond the kernels' choice of tiling, and a repeated call is bitwise the same.  Host arrays and
    CPU tensors are refused: there is no CPU fallback (calculate_lpips takes numpy arrays)."""
    _check_params(params)
    preds = list(preds) if isinstance(preds, (list, tuple)) else [preds]
    targets = list(targets) if isinstance(targets, (list, tuple)) else [targets]
    if not preds or len(preds) != len(targets):
        raise ValueError(f"{len(preds)} predictions and {len(targets)} targets: need the same number, at least one")
    for p, t in zip(preds, targets):
        if not isinstance(p, torch.Tensor) or not isinstance(t, torch.Tensor):
            raise ValueError("the device LPIPS needs GPU tensors (calculate_lpips takes numpy arrays); there is no CPU "
                             "fallback")
        h, w = _check_pair(p.shape, p.dtype, t.shape, t.dtype, tuple(_KIND))
        if p.shape != preds[0].shape or p.dtype != preds[0].dtype or p.device != preds[0].device \
                or t.device != p.device:
            raise ValueError("the frames of one call must share shape, dtype and device")
    dev = preds[0].device
    if dev.type != "cuda":
        raise _hip.HipLibraryError("the device LPIPS needs GPU tensors; there is no CPU fallback (calculate_lpips takes "
                                   "host arrays)")
    k = len(preds)
    with torch.cuda.device(dev):
        packed, biases, lins = params.on(dev)
        oh, ow = (h - 7) // 4 + 1, (w - 7) // 4 + 1
        z = torch.empty((2 * k, 48, oh + 2, ow + 2), dtype=torch.float32, device=dev)
        for i, frame in enumerate(preds + targets):
            lpips_pack(frame, z, i)
        out = torch.empty((k, 6), dtype=torch.float64, device=dev)
        ws = torch.empty(k * -(-oh * ow // 64), dtype=torch.float64, device=dev)
        x, hh, ww = z, oh, ow
        for l, (_, co, ci, ks, _, pad, pool) in enumerate(TRUNK_ALEX):
            if pool:
                hh, ww = (hh - 3) // 2 + 1, (ww - 3) // 2 + 1
                y = torch.empty((2 * k, ci, hh, ww), dtype=torch.float32, device=dev)
                ops.pool3x3(x, y, ops.POOL_MAX_S2)
                x = y
            y = torch.empty((2 * k, co, hh, ww), dtype=torch.float32, device=dev)
            if l == 0:
                ops.convkxk(packed[0], x, y, 48, co, 3, 3, bias=biases[0], relu1=True)
            elif ks == 5:
                ops.convkxk(packed[l], x, y, ci, co, 5, 5, pad=(pad, pad), bias=biases[l], relu1=True)
            else:
                ops.conv3x3(packed[l], x, y, ci, co, bias=biases[l], relu1=True)
            lpips_head(y, lins[l], out, l, ws)
            x = y
        out[:, 5] = ((out[:, 0] + out[:, 1]) + out[:, 2]) + out[:, 3] + out[:, 4]
    return out


def calculate_lpips_device(pred_dev, target_dev, params: LpipsParams) -> float:
    """Device twin of calculate_lpips for one pair of GPU frames: a float after the one synchronising copy of six
    doubles.  Differs from the host's value by the float32 rounding of the trunk only."""
    return float(frame_lpips_device([pred_dev], [target_dev], params)[0, 5].item())
