"""What the plain conv3x3 stacks (DnCNN, REDNet) share: the `precision` keyword and the fp16 mode's workspace."""
from __future__ import annotations

import torch


#: the values of a conv stack's `precision` keyword; "fp16" runs the native-fp16 kernels (conv3x3_h.hip) and is NOT
#: reference-parity: every hidden activation is rounded to 11 significant bits
PRECISIONS = ("fp32", "fp16")


def check_precision(precision, what, features=None):
    if precision not in PRECISIONS:
        raise ValueError(f"{what}: precision must be one of {PRECISIONS}, got {precision!r}")
    if precision == "fp16" and features is not None and features not in (64, 128):
        raise ValueError(f"{what}: precision='fp16' needs 64 or 128 hidden channels, got {features}")
    return precision


class PrecisionMode:
    """`precision` of a conv stack as a validated attribute that the caches are keyed on.  Mixed in before ModelHost:
    an assignment after construction is checked as the constructor's keyword is, and mode_key() carries the value
    into _hip.param_key, so the packed weights and the HIP graphs of the other mode are never handed to this one.  The
    class names the attribute that holds its hidden width in WIDTH_ATTR and sets it before `precision`."""
    WIDTH_ATTR = None

    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, value):
        self._precision = check_precision(value, type(self).__name__, getattr(self, self.WIDTH_ATTR))

    def mode_key(self):
        return super().mode_key() + (self._precision,)


def half_workspace(ws, key, names, shape, device):
    """fp16 channel-last buffers `names` of `shape` [B, H, W, C], kept in the dict `ws` while `key` is unchanged."""
    if ws.get("key") != key:
        ws.clear()
        ws["key"] = key
        for n in names:
            ws[n] = torch.empty(shape, dtype=torch.float16, device=device)
    return ws
