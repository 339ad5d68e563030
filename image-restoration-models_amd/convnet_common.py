"""Shared driver for the plain conv3x3 stacks (DnCNN, REDNet) on the HIP conv kernel."""
from __future__ import annotations

import torch

from . import _hip, ops


def conv3x3(wp, x, y, ci, co, bias=None, relu1=False, res=None, res_mode=0, relu2=False):
    """y = epilogue(conv3x3(x)) through irm_conv3x3_f32 (include/irm_hip.h)."""
    ops.conv3x3(wp, x, y, ci, co, bias=bias, relu1=relu1, res=res, res_mode=res_mode, relu2=relu2)


#: the values of a conv stack's `precision` keyword; "fp16" runs the native-fp16 kernels (conv3x3_h.hip) and is NOT
#: reference-parity: every hidden activation is rounded to 11 significant bits
PRECISIONS = ("fp32", "fp16")


def check_precision(precision, what, features=None):
    if precision not in PRECISIONS:
        raise ValueError(f"{what}: precision must be one of {PRECISIONS}, got {precision!r}")
    if precision == "fp16" and features is not None and features not in (64, 128):
        raise ValueError(f"{what}: precision='fp16' needs 64 or 128 hidden channels, got {features}")
    return precision


def thin_weight(w):
    """The plain fp32 weight of a first / last layer of the fp16 mode (ops.conv3x3_h_in / conv3x3_h_out)."""
    return w.detach().float().contiguous()


def half_workspace(ws, key, names, shape, device):
    """fp16 channel-last buffers `names` of `shape` [B, H, W, C], kept in the dict `ws` while `key` is unchanged."""
    if ws.get("key") != key:
        ws.clear()
        ws["key"] = key
        for n in names:
            ws[n] = torch.empty(shape, dtype=torch.float16, device=device)
    return ws


class PackedCache:
    """Rebuilds packed weights when the parameters of `module` change."""

    def __init__(self, module, build):
        self.module, self.build, self.key, self.value = module, build, None, None

    def get(self):
        key = _hip.param_key(self.module)
        if self.value is None or key != self.key:
            self.value, self.key = self.build(), key
        return self.value


def require_cuda(x, what):
    if not x.is_cuda:
        raise _hip.HipLibraryError(f"irm_amd {what} runs on the GPU only (no CPU fallback); "
                                   "move the model and input to 'cuda'")
