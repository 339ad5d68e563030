"""DnCNN forward on MI355X (drop-in for src/dncnn/models/network_dncnn.py:40-71).

Same constructor and state_dict keys as the reference (``model.<2i>.weight/bias``:
B.conv with mode 'C'+'R' puts a ReLU module after every conv but the last,
basicblock.py:61-98).  Every layer is one irm_conv3x3_f32 launch with bias+ReLU
in the epilogue; the last layer also folds the residual ``x - n``.

``precision="fp16"`` (opt-in, not reference-parity) keeps the hidden activations as fp16 channel-last tensors and runs
irm_conv3x3_h_in_f32 -> irm_conv3x3_h_f16 x (nb - 2) -> irm_conv3x3_h_out_f32; input, output and state_dict are the same."""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import _hip, ops
from .. import SYNTH_RULES
from ...convnet_common import PrecisionMode, half_workspace
from ...host import ModelHost, f32


class DnCNN(PrecisionMode, ModelHost):
    SYNTH_RULES = SYNTH_RULES
    WIDTH_ATTR = "nc"

    def __init__(self, in_nc=1, out_nc=1, nc=64, nb=17, act_mode='BR', precision="fp32"):
        super().__init__()
        self.nc = nc
        self.precision = precision
        if 'B' in act_mode:
            raise NotImplementedError("inference uses BN-merged weights (act_mode='R', src/dncnn/__init__.py:8)")
        assert 'R' in act_mode, 'only ReLU activation is used by the reference loader'
        self.in_nc, self.out_nc, self.nc, self.nb = in_nc, out_nc, nc, nb
        layers = []
        chans = [in_nc] + [nc] * (nb - 1) + [out_nc]
        for i in range(nb):
            layers.append(nn.Conv2d(chans[i], chans[i + 1], 3, padding=1, bias=True))
            if i + 1 < nb:
                layers.append(nn.ReLU(inplace=True))
        self.model = nn.Sequential(*layers)      # parameter holder: never called
        self.hip_graph = True      # the tiler replays the per-batch forward from a HIP graph (utils.graphed_forward)
        self._ws = {}

    def _convs(self):
        return [m for m in self.model if isinstance(m, nn.Conv2d)]

    def _build(self):
        if self.precision == "fp16":
            return self._build_half()
        return [(_hip.pack_conv3x3(m.weight), f32(m.bias), m.in_channels, m.out_channels) for m in self._convs()]

    def _build_half(self):
        convs = self._convs()
        bias = [f32(m.bias) for m in convs]
        # (first / last layer of the fp16 mode: the plain fp32 weight, ops.conv3x3_h_in / conv3x3_h_out)
        return ([(f32(convs[0].weight), bias[0])]
                + [(_hip.pack_conv3x3_h(m.weight), b) for m, b in zip(convs[1:-1], bias[1:-1])]
                + [(f32(convs[-1].weight), bias[-1])])

    @torch.no_grad()
    def forward(self, x):
        self._require_cuda(x)
        x = x.float().contiguous()
        B, _, H, W = x.shape
        layers = self._pack()
        key = (B, H, W, str(x.device), self.precision)
        if self.precision == "fp16":
            return self._forward_half(x, layers, key)
        if self._ws.get("key") != key:
            self._ws = {"key": key,
                        "a": torch.empty(B, self.nc, H, W, dtype=torch.float32, device=x.device),
                        "b": torch.empty(B, self.nc, H, W, dtype=torch.float32, device=x.device)}
        cur, nxt = x, self._ws["a"]
        out = torch.empty(B, self.out_nc, H, W, dtype=torch.float32, device=x.device)
        for i, (wp, bias, ci, co) in enumerate(layers):
            if i + 1 < len(layers):
                ops.conv3x3(wp, cur, nxt, ci, co, bias=bias, relu1=True)
                cur, nxt = nxt, (self._ws["b"] if nxt is self._ws["a"] else self._ws["a"])
            else:
                ops.conv3x3(wp, cur, out, ci, co, bias=bias, res=x, res_mode=2)    # x - n
        return out

    def _forward_half(self, x, layers, key):
        B, _, H, W = x.shape
        ws = half_workspace(self._ws, key, ("a", "b"), (B, H, W, self.nc), x.device)
        cur, nxt = ws["a"], ws["b"]
        ops.conv3x3_h_in(layers[0][0], x, cur, self.in_nc, self.nc, bias=layers[0][1], relu1=True)
        for wp, bias in layers[1:-1]:
            ops.conv3x3_h(wp, cur, nxt, self.nc, self.nc, bias=bias, relu1=True)
            cur, nxt = nxt, cur
        out = torch.empty(B, self.out_nc, H, W, dtype=torch.float32, device=x.device)
        ops.conv3x3_h_out(layers[-1][0], cur, out, self.nc, self.out_nc, bias=layers[-1][1], res=x, res_mode=2)    # x - n
        return out
