"""Tensor-level wrappers of the entry points of include/irm_hip_inception.h: the K_h x K_w conv and the 3x3 poolings of
the Inception-ResNet-v2 encoder of DeblurGANv2's FPN-Inception generator (csrc/convkxk.hip, csrc/pool3x3.hip).

Also reachable as ops.convkxk / ops.pool3x3 / ops.plan_convkxk / ops.convkxk_out_size.  They live apart from ops.py
because every entry point ops.py names belongs to the case list of the precision ledger (tests/ledger.py,
tests/test_gpu_precision.py::test_every_entry_point_is_reached); FPN-Inception is held to the ledger's bar, K e_32 + F,
map by map, by a test of its own (tests/test_gpu_inception.py).
"""
from __future__ import annotations

from . import _hip
from .ops import _bs, _chk, _launch, target_blocks

#: (kh, kw, stride) triples irm_convkxk_f32 is built for -> the largest ct of that geometry (convkxk.hip: LDS budget)
CONVKXK_GEOMETRIES = {(1, 1, 1): 4, (3, 3, 1): 4, (3, 3, 2): 4, (5, 5, 1): 2, (1, 7, 1): 4, (7, 1, 1): 4}


def convkxk_out_size(H: int, W: int, kh: int, kw: int, stride: int, pad):
    return (H + 2 * pad[0] - kh) // stride + 1, (W + 2 * pad[1] - kw) // stride + 1


def plan_convkxk(co: int, OH: int, OW: int, B: int, kh: int, kw: int, stride: int, *, ct: int | None = None,
                 ygroups: int | None = None):
    """(ct, ygroups) of an irm_convkxk_f32 launch; explicit values are kept.  The encoder's maps are small (a 768-pixel
    tile plus its pad gives 48 x 48 maps to the 1x7 / 7x1 convs: 12 pixel tiles), so ct starts at the geometry's largest
    and halves until pixel tiles x passes reach 256 workgroups - one per CU - or ct is 1; ygroups then spreads the
    passes of a pixel tile over workgroups up to target_blocks()."""
    mt = (co + 15) // 16
    blocks = -(-OW // 32) * -(-OH // 8) * B
    if ct is None:
        ct = CONVKXK_GEOMETRIES[(kh, kw, stride)]
        while ct > 1 and (ct > mt or blocks * -(-mt // ct) < 256):
            ct //= 2
    if ygroups is None:
        nchunks = -(-mt // ct)
        ygroups = max(1, min(nchunks, -(-target_blocks() // blocks)))
    return ct, ygroups


def convkxk(wp, x, y, ci: int, co: int, kh: int, kw: int, *, stride: int = 1, pad=(0, 0), bias=None, relu1=False,
            res=None, relu2=False, ct: int | None = None, ygroups: int | None = None):
    """y = relu2?(relu1?(conv(x) + bias) + res): dense kh x kw conv with stride and zero padding pad = (pad_h, pad_w) on
    the exact-f32 MFMA (irm_convkxk_f32); wp from _hip.pack_convkxk_weight.  x, y and res may be channel slices of
    larger buffers; res may be y."""
    if (kh, kw, stride) not in CONVKXK_GEOMETRIES:
        raise ValueError(f"convkxk: no kernel for a {kh}x{kw} conv of stride {stride}")
    _chk(x, "x"), _chk(y, "y")
    B, _, H, W = x.shape
    OH, OW = convkxk_out_size(H, W, kh, kw, stride, pad)
    if OH < 1 or OW < 1 or tuple(y.shape[2:]) != (OH, OW) or y.shape[0] != B:
        raise ValueError(f"convkxk: a {H}x{W} input gives a {OH}x{OW} output, not {tuple(y.shape[2:])}")
    assert x.shape[1] >= ci and y.shape[1] >= co
    if res is not None:
        _chk(res, "res")
        assert tuple(res.shape[2:]) == (OH, OW) and res.shape[1] >= co
    ct, ygroups = plan_convkxk(co, OH, OW, B, kh, kw, stride, ct=ct, ygroups=ygroups)
    nbytes = 4.0 * B * (ci * H * W + OH * OW * (co + (co if res is not None else 0)))
    _launch("convkxk", 2.0 * B * ci * co * kh * kw * OH * OW, nbytes, "irm_convkxk_f32", _hip.ptr(wp), _hip.ptr(x),
            _bs(x), _hip.ptr(y), _bs(y), _hip.ptr(res), _bs(res), _hip.ptr(bias), B, ci, co, H, W, kh, kw, int(stride),
            int(pad[0]), int(pad[1]), int(bool(relu1)), int(res is not None), int(bool(relu2)), ct, ygroups,
            tag=f"{kh}x{kw} s{stride} ci{ci} co{co} {H}x{W} B{B} ct{ct} yg{ygroups}")


POOL_MAX_S2, POOL_AVG_S1 = 0, 1


def pool3x3(x, y, mode: int):
    """POOL_MAX_S2: MaxPool2d(3, 2); POOL_AVG_S1: AvgPool2d(3, 1, 1, count_include_pad=False) (irm_pool3x3_f32)."""
    _chk(x, "x"), _chk(y, "y")
    B, C, H, W = x.shape
    want = (H, W) if mode == POOL_AVG_S1 else ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
    if tuple(y.shape[2:]) != want or y.shape[0] != B or y.shape[1] < C:
        raise ValueError(f"pool3x3: a {H}x{W} input gives a {want[0]}x{want[1]} output, not {tuple(y.shape[2:])}")
    _launch("pool3x3", 9.0 * B * C * want[0] * want[1], 4.0 * B * C * (H * W + want[0] * want[1]), "irm_pool3x3_f32",
            _hip.ptr(x), _bs(x), _hip.ptr(y), _bs(y), B, C, H, W, int(mode), tag=f"m{mode} C{C} {H}x{W} B{B}")
