"""The four-level U-Net that Restormer and MaIRUNet share (restormer.py:254-285, mairunet_arch.py:690-739): its
packing and its walk.  The models differ in what a stage is; everything between the stages is here.

  conv3x3 (patch embed, down/up-sampling with the pixel (un)shuffle folded into the store, output conv + input
  residual) and the two reduce_chan 1x1 GEMMs.  The concatenations (restormer.py:264-273) are not copies: producers
  write straight into channel slices of the concat buffers.
"""
from __future__ import annotations

import torch

from . import _hip, ops
from .host import f32

RESAMPLE = ("down1_2", "down2_3", "down3_4", "up4_3", "up3_2", "up2_1")


def pack_unet(model) -> dict:
    """Packed weights of the layers between the stages."""
    pk = {name: _hip.pack_conv3x3(getattr(model, name).body[0].weight) for name in RESAMPLE}
    pk["patch_embed"] = _hip.pack_conv3x3(model.patch_embed.proj.weight)
    pk["output"] = _hip.pack_conv3x3(model.output.weight)
    pk["output_b"] = f32(model.output.bias)
    for name in ("reduce_chan_level3", "reduce_chan_level2") + (("skip_conv",) if model.dual_pixel_task else ()):
        pk[name] = _hip.pack_gemm_weight(getattr(model, name).weight)
        pk[name + "_b"] = f32(getattr(model, name).bias)
    return pk


def _reduce_chan(pk, name, cat, dec, c):
    # the fp16-emulated GEMM where the model packed a split weight (Restormer); it needs the 16-byte fast path
    split = name + "_s" in pk and (cat.shape[2] * cat.shape[3]) % 4 == 0
    ops.gemm1x1(pk[name + "_s" if split else name], cat, dec, c, 2 * c, bias=pk[name + "_b"], split=split)


def forward(model, x, pk, run_stage, after_trunk=None):
    """The walk on x (float32 [B][Cin][H][W], H and W multiples of 8) with the packed weights pk.

    run_stage(names, t, level) runs the blocks of the stages `names` in place on t, a tensor of level 0..3 (H >> level);
    how consecutive stages on one tensor are grouped is the model's business.  after_trunk(t), if given, sees the
    trunk output before the `output` conv."""
    B, Cin, H, W = x.shape
    dev = x.device
    d1, d2, d3, d4 = model.dim, model.dim * 2, model.dim * 4, model.dim * 8
    H2, W2, H3, W3, H4, W4 = H // 2, W // 2, H // 4, W // 4, H // 8, W // 8

    def buf(name, ch, h, w):
        return model._buf(name, B * ch * h * w, dev).view(B, ch, h, w)

    cat1 = buf("cat1", 2 * d1, H, W)       # [up2_1 | enc1]   (restormer.py:272)
    cat2 = buf("cat2", 2 * d2, H2, W2)     # [up3_2 | enc2]   (restormer.py:267)
    cat3 = buf("cat3", 2 * d3, H3, W3)     # [up4_3 | enc3]   (restormer.py:262)
    lat = buf("latent", d4, H4, W4)
    dec3 = buf("dec3", d3, H3, W3)
    dec2 = buf("dec2", d2, H2, W2)

    e1 = cat1[:, d1:]
    ops.conv3x3(pk["patch_embed"], x, e1, Cin, d1)
    if model.dual_pixel_task:
        e1_in = buf("enc1_in", d1, H, W)
        e1_in.copy_(e1)
        if ops.TIMER is not None:
            ops.TIMER.break_chain()            # a torch kernel sits between two timed launches
    run_stage(("encoder_level1",), e1, 0)
    e2 = cat2[:, d2:]
    ops.conv3x3(pk["down1_2"], e1, e2, d1, d1 // 2, store_mode=1)
    run_stage(("encoder_level2",), e2, 1)
    e3 = cat3[:, d3:]
    ops.conv3x3(pk["down2_3"], e2, e3, d2, d2 // 2, store_mode=1)
    run_stage(("encoder_level3",), e3, 2)
    ops.conv3x3(pk["down3_4"], e3, lat, d3, d3 // 2, store_mode=1)
    run_stage(("latent",), lat, 3)

    ops.conv3x3(pk["up4_3"], lat, cat3[:, :d3], d4, d4 * 2, store_mode=2)
    _reduce_chan(pk, "reduce_chan_level3", cat3, dec3, d3)
    run_stage(("decoder_level3",), dec3, 2)
    ops.conv3x3(pk["up3_2"], dec3, cat2[:, :d2], d3, d3 * 2, store_mode=2)
    _reduce_chan(pk, "reduce_chan_level2", cat2, dec2, d2)
    run_stage(("decoder_level2",), dec2, 1)
    ops.conv3x3(pk["up2_1"], dec2, cat1[:, :d1], d2, d2 * 2, store_mode=2)
    # (decoder_level1 and refinement work on the same tensor)
    run_stage(("decoder_level1", "refinement"), cat1, 0)
    if after_trunk is not None:
        after_trunk(cat1)

    out = torch.empty(B, model.out_channels, H, W, dtype=torch.float32, device=dev)
    if model.dual_pixel_task:
        ops.gemm1x1(pk["skip_conv"], e1_in, cat1, d2, d1, res=cat1, bias=pk["skip_conv_b"])
        ops.conv3x3(pk["output"], cat1, out, d2, model.out_channels, bias=pk["output_b"])
    else:
        ops.conv3x3(pk["output"], cat1, out, d2, model.out_channels, bias=pk["output_b"], res=x, res_mode=1)
    return out
