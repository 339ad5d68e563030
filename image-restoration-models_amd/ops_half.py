"""Tensor-level wrappers of the fp16 entry points (include/irm_hip_half.h): the fp16 mode of the conv stacks.

Also reachable as ops.conv3x3_h_in / ops.conv3x3_h / ops.conv3x3_h_out.  They live apart from ops.py because every
kernel ops.py launches belongs to the fp32 precision ledger (error against a float64 oracle relative to an fp32 run),
and this mode rounds every hidden activation to fp16 on purpose: it is held to its own quantised-chain model instead.
"""
from __future__ import annotations

import torch

from . import _hip
from .ops import _bs, _chk, _launch


def _chk_cl(t: torch.Tensor, name: str, c: int):
    """fp16 channel-last activation [B, H, W, C]: dense inner axes, free batch stride (a multiple of 8 elements)."""
    if not (t.is_cuda and t.dtype == torch.float16 and t.dim() == 4):
        raise ValueError(f"{name}: expected a float16 CUDA tensor [B,H,W,C]")
    _, h, w, ch = t.shape
    if ch != c or c not in (64, 128):
        raise ValueError(f"{name}: expected {c} channels in the last axis, 64 or 128 (got shape {tuple(t.shape)})")
    if t.stride(3) != 1 or t.stride(2) != c or (h > 1 and t.stride(1) != w * c):
        raise ValueError(f"{name}: pixel/channel axes must be dense (got strides {t.stride()})")
    if t.stride(0) % 8 or t.data_ptr() % 16:
        raise ValueError(f"{name}: needs a 16-byte aligned base and a batch stride that is a multiple of 8")
    return t


def _chk_thin_w(w: torch.Tensor, co: int, ci: int, name: str):
    if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (co, ci, 3, 3)):
        raise ValueError(f"{name}: expected a contiguous float32 CUDA weight [{co},{ci},3,3]")
    return w


def conv3x3_h_in(w, x, y, ci: int, co: int, *, bias=None, relu1=False):
    """First layer of the fp16 mode (irm_conv3x3_h_in_f32): x fp32 planar [B,ci<=3,H,W] -> y fp16 channel-last
    [B,H,W,co]; w: the plain fp32 weight [co,ci,3,3]."""
    _chk(x, "x"), _chk_cl(y, "y", co), _chk_thin_w(w, co, ci, "w")
    B, cx, H, W = x.shape
    if cx != ci or not 1 <= ci <= 3 or tuple(y.shape[:3]) != (B, H, W):
        raise ValueError(f"conv3x3_h_in: x {tuple(x.shape)} / y {tuple(y.shape)} do not fit ci={ci} <= 3, co={co}")
    _launch("conv3x3_h_in", 18.0 * B * ci * co * H * W, B * H * W * (4.0 * ci + 2.0 * co), "irm_conv3x3_h_in_f32",
            _hip.ptr(w), _hip.ptr(x), _bs(x), _hip.ptr(y), _bs(y), _hip.ptr(bias), B, ci, co, H, W, int(bool(relu1)),
            tag=f"ci{ci} co{co} {H}x{W} B{B}")


def conv3x3_h(wp, x, y, ci: int, co: int, *, bias=None, relu1=False, res=None, res_mode=0, relu2=False):
    """Hidden layer of the fp16 mode (irm_conv3x3_h_f16): x, y, res fp16 channel-last [B,H,W,C], ci, co in {64, 128};
    wp: the pair _hip.pack_conv3x3_h(w).  res_mode 1: + res between relu1 and relu2."""
    wps, inv_scale = wp
    _chk_cl(x, "x", ci), _chk_cl(y, "y", co)
    B, H, W, _ = x.shape
    if tuple(y.shape[:3]) != (B, H, W):
        raise ValueError(f"conv3x3_h: x {tuple(x.shape)} and y {tuple(y.shape)} differ in batch or image size")
    if res_mode not in (0, 1) or (res_mode == 1) != (res is not None):
        raise ValueError("conv3x3_h: res_mode is 0 (no res) or 1 (with res)")
    if res is not None and tuple(_chk_cl(res, "res", co).shape) != tuple(y.shape):
        raise ValueError("conv3x3_h: res must have y's shape")
    if not (wps.is_cuda and wps.dtype == torch.float16 and wps.numel() == 9 * ci * co):
        raise ValueError("conv3x3_h: wp is not pack_conv3x3_h of a [co,ci,3,3] weight on the device")
    _launch("conv3x3_h", 18.0 * B * ci * co * H * W, 2.0 * B * H * W * (ci + co + (co if res is not None else 0)),
            "irm_conv3x3_h_f16", _hip.ptr(wps), float(inv_scale), _hip.ptr(x), _bs(x), _hip.ptr(y), _bs(y), _hip.ptr(res),
            _bs(res), _hip.ptr(bias), B, ci, co, H, W, int(bool(relu1)), int(res_mode), int(bool(relu2)),
            tag=f"ci{ci} co{co} {H}x{W} B{B}")


def conv3x3_h_out(w, x, y, ci: int, co: int, *, bias=None, res=None, res_mode=0):
    """Last layer of the fp16 mode (irm_conv3x3_h_out_f32): x fp16 channel-last [B,H,W,ci] -> y fp32 planar
    [B,co<=3,H,W]; res (fp32 planar like y) with res_mode 1: v + res, 2: res - v; w: the plain fp32 weight [co,ci,3,3]."""
    _chk_cl(x, "x", ci), _chk(y, "y"), _chk_thin_w(w, co, ci, "w")
    B, H, W, _ = x.shape
    if tuple(y.shape) != (B, co, H, W) or not 1 <= co <= 3:
        raise ValueError(f"conv3x3_h_out: x {tuple(x.shape)} / y {tuple(y.shape)} do not fit ci={ci}, co={co} <= 3")
    if res_mode not in (0, 1, 2) or (res_mode != 0) != (res is not None):
        raise ValueError("conv3x3_h_out: res_mode is 0 (no res), 1 (v + res) or 2 (res - v)")
    if res is not None and tuple(_chk(res, "res").shape) != tuple(y.shape):
        raise ValueError("conv3x3_h_out: res must have y's shape")
    _launch("conv3x3_h_out", 18.0 * B * ci * co * H * W, B * H * W * (2.0 * ci + 4.0 * co * (2 if res is not None else 1)),
            "irm_conv3x3_h_out_f32", _hip.ptr(w), _hip.ptr(x), _bs(x), _hip.ptr(y), _bs(y), _hip.ptr(res), _bs(res),
            _hip.ptr(bias), B, ci, co, H, W, int(res_mode), tag=f"ci{ci} co{co} {H}x{W} B{B}")

