"""What every model class shares on the host side: the packed-weight cache, the per-stream workspace, synthetic
weights and the GPU-only check.  The sub-modules of a model only hold its parameters under the reference's names;
`forward` drives the kernels of libirm_hip.so through ops.py."""
from __future__ import annotations

import functools
import re

import torch
import torch.nn as nn

from . import _hip, synth

#: asked once per process: _buf runs several times per launch, and the answer does not change
_has_cuda = functools.lru_cache(None)(torch.cuda.is_available)


def f32(t):
    """A parameter as the kernels read it (dense float32, detached); None stays None (a conv without bias)."""
    return None if t is None else t.detach().float().contiguous()


class ModelHost(nn.Module):
    #: synthetic-weight rules of the model family (synth.py); a model class binds its package's table here
    SYNTH_RULES = ()
    #: regex of state_dict keys that load_synthetic leaves alone (buffers and aliases no kernel reads)
    SYNTH_SKIP = None

    def __init__(self):
        super().__init__()
        self._packed, self._packed_key = None, None
        self._ws_by_stream = {}
        self._converted = 0

    # ------------------------------------------------------------------ cache keys
    def mode_key(self):
        """Everything but the parameters that decides what _build() and forward() do, as a hashable value:
        _hip.param_key folds it into the key of the packed weights and of the HIP graphs, for this model and for
        every module that wraps it.  The base part counts the conversions (`.half()`, `.float()`, `.to()`): they
        replace every parameter's storage without touching its version, and the allocator may hand the old
        addresses back; and the calls of _hip.invalidate that reached this model, so that a wrapper's graphs go with
        them.  A model with a mode of its own (the conv stacks' `precision`) appends it."""
        return (self._converted, self.__dict__.get("_irm_inval", 0))

    def _apply(self, fn, *args, **kw):
        out = super()._apply(fn, *args, **kw)
        self._converted += 1
        return out

    # ------------------------------------------------------------------ weights
    def load_synthetic(self, seed=42):
        """Fill every parameter from the deterministic generator (synth.py)."""
        skip = self.SYNTH_SKIP
        shapes = {k: tuple(v.shape) for k, v in self.state_dict().items() if not (skip and re.search(skip, k))}
        self.load_state_dict(synth.synth_state_dict(shapes, seed=seed, rules=self.SYNTH_RULES), strict=skip is None)
        return self

    def _build(self):
        """The packed / flattened device copies of the weights, in whatever shape the model's forward reads."""
        raise NotImplementedError

    def _pack(self):
        """The cached result of _build(), rebuilt when the parameters or the mode change (_hip.param_key)."""
        key = _hip.param_key(self)
        if self._packed is None or key != self._packed_key:
            self._packed, self._packed_key = self._build(), key
        return self._packed

    # ------------------------------------------------------------------ workspace
    def _buf(self, name, numel, device):
        """`numel` float32 of the current stream's workspace under `name`; grown, never shrunk; contents undefined.
        (Per stream: concurrent forwards on different streams must not share buffers.)"""
        ws = self._ws_by_stream.setdefault(torch.cuda.current_stream().cuda_stream if _has_cuda() else 0, {})
        t = ws.get(name)
        if t is None or t.numel() < numel or t.device != device:
            t = torch.empty(int(numel), dtype=torch.float32, device=device)
            ws[name] = t
        return t[:numel]

    def _zeros(self, key, numel, device):
        """A zero-initialised workspace tensor of the current stream, created once per key and device."""
        ws = self._ws_by_stream.setdefault(torch.cuda.current_stream().cuda_stream if _has_cuda() else 0, {})
        t = ws.get(key)
        if t is None or t.device != device:
            t = torch.zeros(numel, dtype=torch.float32, device=device)
            ws[key] = t
        return t

    def release_workspace(self):
        """Drop every buffer (utils.graphed_forward: a graph's buffers must come from the graph's own pool)."""
        self._ws_by_stream.clear()
        ws = self.__dict__.get("_ws")         # the conv stacks' buffers of one (B, H, W, device)
        if ws is not None:
            ws.clear()

    # ------------------------------------------------------------------ forward
    def _require_cuda(self, x):
        if not x.is_cuda:
            raise _hip.HipLibraryError(f"irm_amd {type(self).__name__} runs on the GPU only (no CPU fallback); "
                                       "move the model and input to 'cuda'")
