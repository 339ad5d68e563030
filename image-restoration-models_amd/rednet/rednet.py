"""REDNet forward on MI355X (drop-in for src/rednet/rednet.py:15-136).

Same state_dict keys (conv1..15, deconv1..15).  ConvTranspose2d(k=3,s=1,p=1) is
run as a conv3x3 with the weight transposed and flipped at pack time; the
symmetric skips ``relu(relu(deconv) + c)`` and the final ``+ x`` are conv epilogues.

``precision="fp16"`` (opt-in, not reference-parity) keeps the hidden activations and the skip features as fp16
channel-last tensors: irm_conv3x3_h_in_f32 -> irm_conv3x3_h_f16 x 28 -> irm_conv3x3_h_out_f32."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _hip, ops
from . import SYNTH_RULES
from ..convnet_common import PrecisionMode, half_workspace
from ..host import ModelHost, f32


class REDNet(PrecisionMode, ModelHost):
    SYNTH_RULES = SYNTH_RULES
    WIDTH_ATTR = "num_features"

    def __init__(self, num_channels=1, num_features=128, precision="fp32"):
        super().__init__()
        self.num_channels, self.num_features = num_channels, num_features
        self.precision = precision
        for i in range(1, 16):
            setattr(self, f"conv{i}", nn.Conv2d(num_channels if i == 1 else num_features, num_features, 3, padding=1))
        for i in range(1, 16):
            setattr(self, f"deconv{i}", nn.ConvTranspose2d(num_features, num_channels if i == 15 else num_features,
                                                           3, padding=1))
        self.hip_graph = True      # the tiler replays the per-batch forward from a HIP graph (utils.graphed_forward)
        self._ws = {}              # fp16 mode: ping-pong and skip buffers of one (B, H, W, device)

    def _build(self):
        if self.precision == "fp16":
            return self._build_half()
        enc = [(_hip.pack_conv3x3(m.weight), f32(m.bias), m.in_channels, m.out_channels)
               for m in (getattr(self, f"conv{i}") for i in range(1, 16))]
        dec = [(_hip.pack_conv3x3(_hip.deconv_as_conv_weight(m.weight)), f32(m.bias), m.in_channels, m.out_channels)
               for m in (getattr(self, f"deconv{i}") for i in range(1, 16))]
        return enc, dec

    def _build_half(self):
        convs = [getattr(self, f"conv{i}") for i in range(1, 16)]
        deconvs = [getattr(self, f"deconv{i}") for i in range(1, 16)]
        # (first / last layer of the fp16 mode: the plain fp32 weight, ops.conv3x3_h_in / conv3x3_h_out)
        first = (f32(convs[0].weight), f32(convs[0].bias))
        enc = [(_hip.pack_conv3x3_h(m.weight), f32(m.bias)) for m in convs[1:]]
        dec = [(_hip.pack_conv3x3_h(_hip.deconv_as_conv_weight(m.weight)), f32(m.bias)) for m in deconvs[:-1]]
        last = (f32(_hip.deconv_as_conv_weight(deconvs[-1].weight)), f32(deconvs[-1].bias))
        return first, enc, dec, last

    @torch.no_grad()
    def forward(self, x):
        self._require_cuda(x)
        x = x.float().contiguous()
        B, _, H, W = x.shape
        if self.precision == "fp16":
            return self._forward_half(x)
        enc, dec = self._pack()
        F = self.num_features

        def new(c=F):
            return torch.empty(B, c, H, W, dtype=torch.float32, device=x.device)

        feats, cur = [], x
        for (wp, b, ci, co) in enc:                       # c1..c15 (rednet.py:66-80)
            nxt = new()
            ops.conv3x3(wp, cur, nxt, ci, co, bias=b, relu1=True)
            feats.append(nxt)
            cur = nxt
        d = cur
        for i in range(1, 15):                            # deconv1..14 (rednet.py:84-130)
            wp, b, ci, co = dec[i - 1]
            nxt = new()
            if i % 2 == 1:                                # relu(relu(deconv) + c_{15-i})
                ops.conv3x3(wp, d, nxt, ci, co, bias=b, relu1=True, res=feats[14 - i], res_mode=1, relu2=True)
            else:
                ops.conv3x3(wp, d, nxt, ci, co, bias=b, relu1=True)
            d = nxt
        wp, b, ci, co = dec[14]
        out = new(self.num_channels)
        ops.conv3x3(wp, d, out, ci, co, bias=b, res=x, res_mode=1)      # d15 + x (rednet.py:133-136)
        return out

    def _forward_half(self, x):
        B, _, H, W = x.shape
        first, enc, dec, last = self._pack()
        F = self.num_features
        # the features the decoder adds back (c2, c4 ... c14) own a buffer each, everything else ping-pongs
        skips = tuple(f"c{k}" for k in range(2, 15, 2))
        ws = half_workspace(self._ws, (B, H, W, str(x.device), self.precision), ("a", "b") + skips, (B, H, W, F), x.device)

        def other(t):
            return ws["b"] if t is ws["a"] else ws["a"]

        cur = ws["a"]
        ops.conv3x3_h_in(first[0], x, cur, self.num_channels, F, bias=first[1], relu1=True)     # c1
        for k, (wp, b) in enumerate(enc, start=2):                                              # c2..c15
            nxt = ws[f"c{k}"] if k % 2 == 0 and k < 15 else other(cur)
            ops.conv3x3_h(wp, cur, nxt, F, F, bias=b, relu1=True)
            cur = nxt
        for i, (wp, b) in enumerate(dec, start=1):                                              # deconv1..14
            nxt = other(cur)
            if i % 2 == 1:                                # relu(relu(deconv) + c_{15-i})
                ops.conv3x3_h(wp, cur, nxt, F, F, bias=b, relu1=True, res=ws[f"c{15 - i}"], res_mode=1, relu2=True)
            else:
                ops.conv3x3_h(wp, cur, nxt, F, F, bias=b, relu1=True)
            cur = nxt
        out = torch.empty(B, self.num_channels, H, W, dtype=torch.float32, device=x.device)
        ops.conv3x3_h_out(last[0], cur, out, F, self.num_channels, bias=last[1], res=x, res_mode=1)    # d15 + x
        return out
