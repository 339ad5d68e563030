"""Flat MaIR on MI355X - drop-in for src/mair/basicsr/archs/mair_arch.py:493-730 (`resi_connection='1conv'`, all
three reconstruction branches: denoising `upsampler=None`, classical SR `'pixelshuffle'`, lightweight SR
`'pixelshuffledirect'`; same constructor keywords and state_dict keys).  It reuses the VSSBlock driver of
mairunet_arch.py (the reference's RMB is the same block with the MLP called `conv_blk`); odd blocks of a group use
the shifted scan tables (mair_arch.py:455, 379-382).

  (x - mean) * img_range -> conv3x3 conv_first -> LayerNorm (patch_embed.norm) -> groups of RMBs, each closed by
  conv3x3 + residual (RMG, :863-864) -> LayerNorm -> conv_after_body + conv_first output -> head -> / img_range + mean

  head, denoising:          conv_last + input
  head, classical SR:       conv_before_upsample (conv3x3 + LeakyReLU(0.01)) -> Upsample (per factor 2: conv3x3 to
                            4 x 64 channels + PixelShuffle(2); factor 3: 9 x 64 + PixelShuffle(3)) -> conv_last
  head, lightweight SR:     UpsampleOneStep (conv3x3 to 3 r^2 channels + PixelShuffle(r))   (:940-969)
The activation and every PixelShuffle are folded into the conv epilogues (irm_conv3x3_ep_f32 /
irm_conv3x3_f16x3_ep_f32).  `upscale` is the factor of the output (1 for denoising); the tiler reads it.

The two stand-alone LayerNorms run as an identity-weight irm_gemm1x1_f32 with the LN prologue (1 GFLOP per
128x128 tile, no extra kernel); the mean shifts run on irm_chan_norm_act_f32 with constant "statistics".
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _hip, ops
from ..host import f32
from .mairunet_arch import MambaHost, VSSBlock, pack_block, scan_ids

RGB_MEAN = (0.4488, 0.4371, 0.4040)


class _Group(nn.Module):
    """RMG holder: residual_group.blocks.{i}, conv (mair_arch.py:793-864)."""

    def __init__(self, dim, depth, d_state, ssm_ratio, mlp_ratio):
        super().__init__()
        self.residual_group = nn.Module()
        self.residual_group.blocks = nn.ModuleList(
            [VSSBlock(dim, d_state, ssm_ratio, mlp_ratio, mlp_name="conv_blk") for _ in range(depth)])
        self.conv = nn.Conv2d(dim, dim, 3, 1, 1)


class _Norm(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim)


NUM_FEAT = 64               # channels of the classical-SR head (mair_arch.py:547)
LEAKY_SLOPE = 0.01          # nn.LeakyReLU() of conv_before_upsample (:624)


def _upsample_factors(scale: int) -> list:
    """PixelShuffle factors of the reference's Upsample (mair_arch.py:971-988): 2^n -> n x 2, 3 -> [3]."""
    if scale >= 1 and (scale & (scale - 1)) == 0:
        return [2] * (scale.bit_length() - 1)
    if scale == 3:
        return [3]
    raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')


class MaIR(MambaHost):
    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=60, depths=(6, 6, 6, 6), drop_rate=0., d_state=16,
                 ssm_ratio=1.5, drop_path_rate=0.1, norm_layer=nn.LayerNorm, patch_norm=True, use_checkpoint=False, upscale=2,
                 img_range=1., upsampler='pixelshuffledirect', resi_connection='1conv', dynamic_ids=False, scan_len=8,
                 mlp_ratio=2, **kwargs):
        super().__init__()
        if upsampler in (None, '', 'None'):
            upsampler = None
        if resi_connection != '1conv' or patch_size != 1:
            raise NotImplementedError("MaIR with resi_connection='3conv' or patch_size != 1 is not built in the MI355X path")
        if upsampler is None and upscale != 1:
            raise NotImplementedError("the denoising configuration of MaIR (upsampler=None) is built with upscale=1 only")
        if upsampler not in (None, 'pixelshuffle', 'pixelshuffledirect'):
            raise NotImplementedError(f"MaIR upsampler {upsampler!r} is not built in the MI355X path")
        if upsampler == 'pixelshuffledirect' and upscale not in (2, 3, 4):
            raise NotImplementedError("lightweight-SR MaIR (upsampler='pixelshuffledirect') is built for upscale 2, 3 and 4")
        self.in_chans, self.embed_dim, self.img_range, self.scan_len = in_chans, embed_dim, float(img_range), scan_len
        self.upsampler = upsampler
        self.patch_norm = patch_norm
        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = _Norm(embed_dim) if patch_norm else nn.Module()
        self.layers = nn.ModuleList([_Group(embed_dim, d, d_state, ssm_ratio, mlp_ratio) for d in depths])
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1)
        if upsampler == 'pixelshuffle':                      # classical SR (mair_arch.py:621-626)
            self.ps_factors = _upsample_factors(int(upscale))
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, NUM_FEAT, 3, 1, 1), nn.LeakyReLU())
            ups = []
            for r in self.ps_factors:
                ups += [nn.Conv2d(NUM_FEAT, r * r * NUM_FEAT, 3, 1, 1), nn.PixelShuffle(r)]
            self.upsample = nn.Sequential(*ups)
            self.conv_last = nn.Conv2d(NUM_FEAT, in_chans, 3, 1, 1)
        elif upsampler == 'pixelshuffledirect':              # lightweight SR (:627-629, UpsampleOneStep)
            self.ps_factors = [int(upscale)]
            self.upsample = nn.Sequential(nn.Conv2d(embed_dim, upscale * upscale * in_chans, 3, 1, 1),
                                          nn.PixelShuffle(upscale))
        else:                                                # denoising
            self.ps_factors = []
            self.conv_last = nn.Conv2d(embed_dim, in_chans, 3, 1, 1)
        self.upscale = int(upscale) if upsampler is not None else 1
        self.max_tiles_per_batch = 8
        self.hip_graph = True      # the tiler replays the per-batch forward from a HIP graph (utils.graphed_forward)

    def _build(self):
        c3 = lambda conv: (_hip.pack_conv3x3(conv.weight), f32(conv.bias))     # noqa: E731
        dev = self.conv_first.weight.device
        E = self.embed_dim
        pk = {name: pack_block(m) for name, m in self.named_modules() if isinstance(m, VSSBlock)}
        pk["conv_first"], pk["conv_after_body"] = c3(self.conv_first), c3(self.conv_after_body)
        if self.upsampler != 'pixelshuffledirect':
            pk["conv_last"] = c3(self.conv_last)
        if self.upsampler == 'pixelshuffle':
            pk["conv_before_upsample"] = c3(self.conv_before_upsample[0])
        if self.upsampler is not None:
            pk["upsample"] = [c3(self.upsample[2 * i]) for i in range(len(self.ps_factors))]
        for i, g in enumerate(self.layers):
            pk[f"layers.{i}.conv"] = c3(g.conv)
        pk["eye"] = _hip.pack_gemm_weight(torch.eye(E, device=dev))
        if self.patch_norm:
            pk["pn"] = (f32(self.patch_embed.norm.weight), f32(self.patch_embed.norm.bias))
        pk["fn"] = (f32(self.norm.weight), f32(self.norm.bias))
        mean = torch.tensor(RGB_MEAN if self.in_chans == 3 else [0.0] * self.in_chans, dtype=torch.float32, device=dev)
        r = self.img_range
        # chan_norm_act computes (x - m) * s: shift in = (x - mean) * r ; shift out = (y + mean * r) / r
        pk["shift_in"] = torch.stack([mean, torch.full_like(mean, r)], dim=1).contiguous()
        pk["shift_out"] = torch.stack([-mean * r, torch.full_like(mean, 1.0 / r)], dim=1).contiguous()
        return pk

    def _layer_norm(self, x, y, wb, pk):
        B, C, H, W = x.shape
        stats = self._buf("stats", B * 2 * H * W, x.device)
        ops.ln_stats(x, stats)
        ops.gemm1x1(pk["eye"], x, y, C, C, stats=stats, lnw=wb[0], lnb=wb[1], ln_mode=ops.LN_WITHBIAS)

    @torch.no_grad()
    def forward(self, inp: torch.Tensor) -> torch.Tensor:
        self._require_cuda(inp)
        x = inp.float().contiguous()
        B, Cin, H, W = x.shape
        dev, E = x.device, self.embed_dim
        pk = self._pack()
        ids = (scan_ids(H, W, self.scan_len, dev), scan_ids(H, W, self.scan_len, dev, self.scan_len // 2))
        new = lambda c: torch.empty(B, c, H, W, dtype=torch.float32, device=dev)      # noqa: E731
        xin = new(Cin)
        ops.chan_norm_act(x, pk["shift_in"].unsqueeze(0).expand(B, -1, -1).contiguous(), xin)
        first = new(E)
        ops.conv3x3(pk["conv_first"][0], xin, first, Cin, E, bias=pk["conv_first"][1])
        t = new(E)
        if self.patch_norm:
            self._layer_norm(first, t, pk["pn"], pk)
        else:
            t.copy_(first)
        g_in = new(E)
        for li, grp in enumerate(self.layers):
            g_in.copy_(t)
            for bi, blk in enumerate(grp.residual_group.blocks):
                self._block(blk, pk[f"layers.{li}.residual_group.blocks.{bi}"], t, ids[bi % 2])
            nxt = new(E)
            ops.conv3x3(pk[f"layers.{li}.conv"][0], t, nxt, E, E, bias=pk[f"layers.{li}.conv"][1], res=g_in, res_mode=1)
            t = nxt
        tn = new(E)
        self._layer_norm(t, tn, pk["fn"], pk)
        res = new(E)
        ops.conv3x3(pk["conv_after_body"][0], tn, res, E, E, bias=pk["conv_after_body"][1], res=first, res_mode=1)
        if self.upsampler is None:
            out = new(Cin)
            ops.conv3x3(pk["conv_last"][0], res, out, E, Cin, bias=pk["conv_last"][1], res=xin, res_mode=1)
        else:
            out = self._sr_head(res, pk)
        ops.chan_norm_act(out, pk["shift_out"].unsqueeze(0).expand(B, -1, -1).contiguous(), out)
        return out

    def _sr_head(self, res, pk):
        """conv_before_upsample / Upsample / conv_last, or UpsampleOneStep: the output at upscale x the input size."""
        B, E, H, W = res.shape
        dev, Cin = res.device, self.in_chans
        if self.upsampler == 'pixelshuffledirect':
            r = self.ps_factors[0]
            out = torch.empty(B, Cin, r * H, r * W, dtype=torch.float32, device=dev)
            w, b = pk["upsample"][0]
            ops.conv3x3(w, res, out, E, r * r * Cin, bias=b, store_mode=2, shuffle=r)
            return out
        f = torch.empty(B, NUM_FEAT, H, W, dtype=torch.float32, device=dev)
        w, b = pk["conv_before_upsample"]
        ops.conv3x3(w, res, f, E, NUM_FEAT, bias=b, leaky=LEAKY_SLOPE)
        for (w, b), r in zip(pk["upsample"], self.ps_factors):
            h, wd = f.shape[2:]
            g = torch.empty(B, NUM_FEAT, r * h, r * wd, dtype=torch.float32, device=dev)
            ops.conv3x3(w, f, g, NUM_FEAT, r * r * NUM_FEAT, bias=b, store_mode=2, shuffle=r)
            f = g
        h, wd = f.shape[2:]
        out = torch.empty(B, Cin, h, wd, dtype=torch.float32, device=dev)
        ops.conv3x3(pk["conv_last"][0], f, out, NUM_FEAT, Cin, bias=pk["conv_last"][1])
        return out
