"""FPN-Inception generator of DeblurGANv2 on MI355X (src/deblurganv2/models/fpn_inception.py), with the reference's
state_dict keys.

`FPNInceptionDecoder` is the in-tree part of the reference file - lateral 1x1 convs, reflect pads and the top-down path
of `FPN` (:142-170), the four heads, smoothing convs and the tanh/clamp output of `FPNInception.forward` (:65-81); its
`forward` takes the five encoder feature maps as inputs:

    y = decoder(x, enc0, enc1, enc2, enc3, enc4)    # enc_i = fpn.enc_i(...) of the reference, float32 on the GPU

`FPNInception` adds the bottom-up encoder, `timm.create_model('inception_resnet_v2')` in the reference
(fpn_inception.py:94-118).  timm is third-party code that is neither vendored in the reference nor installed here, so
the network is restated from its publication (Szegedy et al., "Inception-v4, Inception-ResNet and the Impact of
Residual Connections on Learning", and the layer table of the published pretrained model): every conv unit is
Conv2d(bias=False) -> BatchNorm2d(eps=1e-3) -> ReLU; the stem, mixed_5b, 10 x Block35 (scale 0.17), mixed_6a,
20 x Block17 (scale 0.10) and mixed_7a are what `FPN.forward` runs.  The tail of the classifier (repeat_2, block8,
conv2d_7b, last_linear) is in the checkpoint but never run, and is not declared here.  Two facts pin the restatement:
the parameter count of the full network (55 843 464, timm's table) and the five map sizes of a 128x160 input, which
equal those the reference's own decoder golden was recorded with (tests/inception_model.py, tests/test_inception_cpu.py).

    y = model(x)                                    # x [B, 3, H, W], H and W multiples of 32 and at least 128

Norm layers run in TRAIN mode like the reference's generators (src/deblurganv2/__init__.py:38), one tile at a time:
BatchNorm2d and InstanceNorm2d both normalise with the statistics of the current tile, here chan_stats +
chan_norm_act per (sample, channel), which keeps batched tiles independent; running statistics are loaded, never read.
Reflect padding of the small lateral maps is tensor plumbing (torch.nn.functional.pad on the device); every conv / norm
/ pool / up-sample runs in libirm_hip.so: 1x1 convs on gemm1x1, 3x3 pad-1 convs on conv3x3, every other geometry and
the block closers relu(x + s (W cat + b)) on convkxk, the poolings on pool3x3.  The 1x1 convs at the head of a
block's branches read the same input and run as ONE GEMM over their concatenated weights with one stats and one norm
launch; every branch writes straight into its channel slice of the block's concat buffer.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import _hip, ops
from ...host import ModelHost, f32
from .fpn_mobilenet import FPNHead, FPNMobileNet

ENC_CHANNELS = (32, 64, 192, 1088, 2080)          # conv2d_1a, maxpool_3a, maxpool_5a, mixed_6a, mixed_7a outputs


class _FPNTop(nn.Module):
    """Holder for the in-tree layers of `FPN` (keys fpn.td1.0.weight, fpn.lateral4.weight, ...)."""

    def __init__(self, norm_layer, num_filters=256):
        super().__init__()
        for name in ("td1", "td2", "td3"):
            setattr(self, name, nn.Sequential(nn.Conv2d(num_filters, num_filters, 3, padding=1), norm_layer(num_filters),
                                              nn.ReLU(inplace=True)))
        self.lateral4 = nn.Conv2d(ENC_CHANNELS[4], num_filters, 1, bias=False)
        self.lateral3 = nn.Conv2d(ENC_CHANNELS[3], num_filters, 1, bias=False)
        self.lateral2 = nn.Conv2d(ENC_CHANNELS[2], num_filters, 1, bias=False)
        self.lateral1 = nn.Conv2d(ENC_CHANNELS[1], num_filters, 1, bias=False)
        self.lateral0 = nn.Conv2d(ENC_CHANNELS[0], num_filters // 2, 1, bias=False)


class FPNInceptionDecoder(ModelHost):
    SYNTH_RULES, SYNTH_SKIP = FPNMobileNet.SYNTH_RULES, FPNMobileNet.SYNTH_SKIP

    def __init__(self, norm_layer=None, output_ch=3, num_filters=128, num_filters_fpn=256):
        super().__init__()
        if norm_layer is None:
            import functools
            norm_layer = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=True)   # networks.py:22
        self.nf, self.nfpn = num_filters, num_filters_fpn
        self.fpn = _FPNTop(norm_layer, num_filters_fpn)
        for i in (1, 2, 3, 4):
            setattr(self, f"head{i}", FPNHead(num_filters_fpn, num_filters, num_filters))
        self.smooth = nn.Sequential(nn.Conv2d(4 * num_filters, num_filters, 3, padding=1), norm_layer(num_filters), nn.ReLU())
        self.smooth2 = nn.Sequential(nn.Conv2d(num_filters, num_filters // 2, 3, padding=1), norm_layer(num_filters // 2),
                                     nn.ReLU())
        self.final = nn.Conv2d(num_filters // 2, output_ch, 3, padding=1)

    def _build(self):
        c3 = lambda conv: (_hip.pack_conv3x3(conv.weight), f32(conv.bias))    # noqa: E731
        pk = {f"lateral{i}": _hip.pack_gemm_weight(getattr(self.fpn, f"lateral{i}").weight) for i in range(5)}
        for n in ("td1", "td2", "td3"):
            pk[n] = c3(getattr(self.fpn, n)[0])
        for i in (1, 2, 3, 4):
            h = getattr(self, f"head{i}")
            pk[f"head{i}"] = (c3(h.block0)[0], c3(h.block1)[0])
        pk["smooth"], pk["smooth2"], pk["final"] = c3(self.smooth[0]), c3(self.smooth2[0]), c3(self.final)
        return pk

    @torch.no_grad()
    def forward(self, x, enc0, enc1, enc2, enc3, enc4):
        self._require_cuda(x)
        x = x.float().contiguous()
        B, _, H, W = x.shape
        dev = x.device
        pk = self._pack()
        Fp, nf = self.nfpn, self.nf
        new = lambda c, h, w: torch.empty(B, c, h, w, dtype=torch.float32, device=dev)     # noqa: E731
        rpad = lambda t, p: torch.nn.functional.pad(t, p, "reflect").contiguous()          # noqa: E731

        def norm(t):
            st = torch.empty(B, t.shape[1], 2, dtype=torch.float32, device=dev)
            ops.chan_stats(t, st)
            ops.chan_norm_act(t, st, t, act=ops.ACT_RELU)
            return t

        def lateral(i, e):
            e = e.float().contiguous()
            co = Fp // 2 if i == 0 else Fp
            t = new(co, e.shape[2], e.shape[3])
            ops.gemm1x1(pk[f"lateral{i}"], e, t, co, e.shape[1])
            return t

        # lateral connections + reflect pads (fpn_inception.py:153-163)
        l4 = rpad(lateral(4, enc4), (1, 1, 1, 1))
        l3 = rpad(lateral(3, enc3), (1, 1, 1, 1))
        l2 = rpad(lateral(2, enc2), (1, 2, 1, 2))
        l1 = rpad(lateral(1, enc1), (1, 1, 1, 1))
        map0 = rpad(lateral(0, enc0), (0, 1, 0, 1))

        def td(lat, top, name):                       # td(lateral + up2(top))   (:166-168)
            s = torch.empty_like(lat)
            ops.upsample_add(top, s, 2, add=lat)
            o = torch.empty_like(lat)
            ops.conv3x3(pk[name][0], s, o, Fp, Fp, bias=pk[name][1])
            return norm(o)
        map4 = l4
        map3 = td(l3, map4, "td1")
        map2 = td(l2, map3, "td2")
        map1 = td(l1, map2, "td3")
        # heads, nearest up-sampling into the concat buffer [map4 | map3 | map2 | map1] (:68-73)
        h4, w4 = map1.shape[2], map1.shape[3]
        cat = new(4 * nf, h4, w4)
        for slot, (m, name, scale) in enumerate(((map4, "head4", 8), (map3, "head3", 4), (map2, "head2", 2), (map1, "head1", 1))):
            a = new(nf, m.shape[2], m.shape[3])
            ops.conv3x3(pk[name][0], m, a, Fp, nf, relu1=True)
            dst = cat[:, slot * nf:(slot + 1) * nf]
            if scale == 1:
                ops.conv3x3(pk[name][1], a, dst, nf, nf, relu1=True)
            else:
                b2 = new(nf, m.shape[2], m.shape[3])
                ops.conv3x3(pk[name][1], a, b2, nf, nf, relu1=True)
                ops.upsample_add(b2, dst, scale)
        sm = new(nf, h4, w4)
        ops.conv3x3(pk["smooth"][0], cat, sm, 4 * nf, nf, bias=pk["smooth"][1])
        norm(sm)
        s2 = new(nf, 2 * h4, 2 * w4)
        ops.upsample_add(sm, s2, 2, add=map0)                                      # (:75-76)
        sm2 = new(nf // 2, 2 * h4, 2 * w4)
        ops.conv3x3(pk["smooth2"][0], s2, sm2, nf, nf // 2, bias=pk["smooth2"][1])
        norm(sm2)
        if (4 * h4, 4 * w4) != (H, W):
            raise ValueError(f"encoder maps of a {4 * h4}x{4 * w4} image do not belong to this {H}x{W} input")
        up = new(nf // 2, H, W)
        ops.upsample_add(sm2, up, 2)
        out = new(x.shape[1], H, W)
        ops.conv3x3(pk["final"][0], up, out, nf // 2, x.shape[1], bias=pk["final"][1], res=x, res_mode=3)   # clamp(tanh(.) + x)
        return out


# --------------------------------------------------------------------------- the Inception-ResNet-v2 encoder
class ConvNormAct(nn.Module):
    """Conv2d(bias=False) -> BatchNorm2d(eps=1e-3) -> ReLU: keys `conv.weight`, `bn.{weight,bias,running_*}`."""

    def __init__(self, cin, cout, k, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=1e-3)


def _seq(*units):
    return nn.Sequential(*units)


class Mixed5b(nn.Module):                 # 192 -> 96 + 64 + 96 + 64 = 320
    def __init__(self):
        super().__init__()
        self.branch0 = ConvNormAct(192, 96, 1)
        self.branch1 = _seq(ConvNormAct(192, 48, 1), ConvNormAct(48, 64, 5, 1, 2))
        self.branch2 = _seq(ConvNormAct(192, 64, 1), ConvNormAct(64, 96, 3, 1, 1), ConvNormAct(96, 96, 3, 1, 1))
        self.branch3 = _seq(nn.AvgPool2d(3, 1, 1, count_include_pad=False), ConvNormAct(192, 64, 1))


class Block35(nn.Module):                 # relu(x + 0.17 conv2d(cat)), 320 channels
    scale = 0.17

    def __init__(self):
        super().__init__()
        self.branch0 = ConvNormAct(320, 32, 1)
        self.branch1 = _seq(ConvNormAct(320, 32, 1), ConvNormAct(32, 32, 3, 1, 1))
        self.branch2 = _seq(ConvNormAct(320, 32, 1), ConvNormAct(32, 48, 3, 1, 1), ConvNormAct(48, 64, 3, 1, 1))
        self.conv2d = nn.Conv2d(128, 320, 1)


class Mixed6a(nn.Module):                 # 320 -> 384 + 384 + 320 = 1088, half size
    def __init__(self):
        super().__init__()
        self.branch0 = ConvNormAct(320, 384, 3, 2)
        self.branch1 = _seq(ConvNormAct(320, 256, 1), ConvNormAct(256, 256, 3, 1, 1), ConvNormAct(256, 384, 3, 2))
        self.branch2 = nn.MaxPool2d(3, 2)


class Block17(nn.Module):                 # relu(x + 0.10 conv2d(cat)), 1088 channels
    scale = 0.10

    def __init__(self):
        super().__init__()
        self.branch0 = ConvNormAct(1088, 192, 1)
        self.branch1 = _seq(ConvNormAct(1088, 128, 1), ConvNormAct(128, 160, (1, 7), 1, (0, 3)),
                            ConvNormAct(160, 192, (7, 1), 1, (3, 0)))
        self.conv2d = nn.Conv2d(384, 1088, 1)


class Mixed7a(nn.Module):                 # 1088 -> 384 + 288 + 320 + 1088 = 2080, half size
    def __init__(self):
        super().__init__()
        self.branch0 = _seq(ConvNormAct(1088, 256, 1), ConvNormAct(256, 384, 3, 2))
        self.branch1 = _seq(ConvNormAct(1088, 256, 1), ConvNormAct(256, 288, 3, 2))
        self.branch2 = _seq(ConvNormAct(1088, 256, 1), ConvNormAct(256, 288, 3, 1, 1), ConvNormAct(288, 320, 3, 2))
        self.branch3 = nn.MaxPool2d(3, 2)


class InceptionResNetV2Trunk(nn.Module):
    """The layers of inception_resnet_v2 that FPN.forward runs, under the published model's names."""

    def __init__(self):
        super().__init__()
        self.conv2d_1a = ConvNormAct(3, 32, 3, 2)
        self.conv2d_2a = ConvNormAct(32, 32, 3, 1)
        self.conv2d_2b = ConvNormAct(32, 64, 3, 1, 1)
        self.maxpool_3a = nn.MaxPool2d(3, 2)
        self.conv2d_3b = ConvNormAct(64, 80, 1)
        self.conv2d_4a = ConvNormAct(80, 192, 3, 1)
        self.maxpool_5a = nn.MaxPool2d(3, 2)
        self.mixed_5b = Mixed5b()
        self.repeat = _seq(*[Block35() for _ in range(10)])
        self.mixed_6a = Mixed6a()
        self.repeat_1 = _seq(*[Block17() for _ in range(20)])
        self.mixed_7a = Mixed7a()


class _FPNFull(_FPNTop):
    """`FPN` with its encoder: fpn.inception.* and the aliases fpn.enc0 .. fpn.enc4 the reference's Sequentials create
    (fpn_inception.py:99-118)."""

    def __init__(self, norm_layer, num_filters=256):
        super().__init__(norm_layer, num_filters)
        self.inception = t = InceptionResNetV2Trunk()
        self.enc0 = t.conv2d_1a
        self.enc1 = nn.Sequential(t.conv2d_2a, t.conv2d_2b, t.maxpool_3a)
        self.enc2 = nn.Sequential(t.conv2d_3b, t.conv2d_4a, t.maxpool_5a)
        self.enc3 = nn.Sequential(t.mixed_5b, t.repeat, t.mixed_6a)
        self.enc4 = nn.Sequential(t.repeat_1, t.mixed_7a)


#: checkpoint keys of the classifier tail, which FPN.forward never runs (get_model_inception drops them)
INCEPTION_TAIL = r"^fpn\.inception\.(repeat_2|block8|conv2d_7b|last_linear)\."

#: smallest H and W: the maps have sides 16k-1, 8k-2, 4k-3, 2k-2, k-2 for a side of 32k, and the decoder reflect-pads the
#: last one by 1, which needs 2 pixels
MIN_SIDE = 128


# ---- packing: a ConvNormAct unit, the merged 1x1 heads of a block, the closer of a residual block
def _pack_unit(m):
    """A ConvNormAct unit: its conv packed for the kernel its geometry runs on, and its norm's affine."""
    c = m.conv
    k, s, p = tuple(c.kernel_size), c.stride[0], tuple(c.padding)
    d = {"ci": c.in_channels, "co": c.out_channels, "k": k, "s": s, "p": p, "bn": (f32(m.bn.weight), f32(m.bn.bias))}
    if k == (1, 1):
        d["kind"], d["w"] = "g", _hip.pack_gemm_weight(c.weight)
    elif k == (3, 3) and s == 1 and p == (1, 1):
        d["kind"], d["w"] = "c3", _hip.pack_conv3x3(c.weight)
    else:
        d["kind"], d["w"] = "k", _hip.pack_convkxk_weight(c.weight)
    return d


def _pack_heads(*ms):
    """The 1x1 convs at the heads of a block's branches as one GEMM: weights and affines concatenated in this order."""
    w = torch.cat([m.conv.weight.detach().float().reshape(m.conv.out_channels, -1) for m in ms])
    return {"ci": ms[0].conv.in_channels, "co": w.shape[0], "w": _hip.pack_gemm_weight(w),
            "bn": (torch.cat([f32(m.bn.weight) for m in ms]), torch.cat([f32(m.bn.bias) for m in ms]))}


def _pack_closer(blk):
    """conv2d of a residual block with the block's scale folded into weight and bias."""
    return {"w": _hip.pack_convkxk_weight(blk.conv2d.weight, blk.scale),
            "b": (blk.conv2d.bias.detach().double() * blk.scale).float().contiguous()}


def pack_block35(b):
    return {"heads": _pack_heads(b.branch2[0], b.branch1[0], b.branch0), "b1": _pack_unit(b.branch1[1]),
            "b2": (_pack_unit(b.branch2[1]), _pack_unit(b.branch2[2])), "close": _pack_closer(b)}


def pack_block17(b):
    return {"heads": _pack_heads(b.branch1[0], b.branch0), "b1": (_pack_unit(b.branch1[1]), _pack_unit(b.branch1[2])),
            "close": _pack_closer(b)}


# ---- launches
def _new(like, c, h, w):
    return torch.empty(like.shape[0], c, h, w, dtype=torch.float32, device=like.device)


def _norm(t, bn, out=None):
    """Train-mode BatchNorm2d(eps=1e-3) on one tile + ReLU, in place or into `out` (a slice of a concat buffer)."""
    st = torch.empty(t.shape[0], t.shape[1], 2, dtype=torch.float32, device=t.device)
    ops.chan_stats(t, st, eps=1e-3)
    ops.chan_norm_act(t, st, t if out is None else out, weight=bn[0], bias=bn[1], act=ops.ACT_RELU)
    return t if out is None else out


def _cna(d, t, out=None):
    """One ConvNormAct unit on t (maybe a channel slice); the result in a new tensor or in `out`."""
    h, w = ops.convkxk_out_size(t.shape[2], t.shape[3], d["k"][0], d["k"][1], d["s"], d["p"])
    y = _new(t, d["co"], h, w)
    if d["kind"] == "g":
        ops.gemm1x1(d["w"], t, y, d["co"], d["ci"])
    elif d["kind"] == "c3":
        ops.conv3x3(d["w"], t, y, d["ci"], d["co"])
    else:
        ops.convkxk(d["w"], t, y, d["ci"], d["co"], d["k"][0], d["k"][1], stride=d["s"], pad=d["p"])
    return _norm(y, d["bn"], out)


def _maxpool(t, out=None):
    if out is None:
        out = _new(t, t.shape[1], (t.shape[2] - 3) // 2 + 1, (t.shape[3] - 3) // 2 + 1)
    ops.pool3x3(t, out, ops.POOL_MAX_S2)
    return out


def _heads(d, t, buf):
    """The merged head GEMM of a block into the first channels of `buf`, normalised in place."""
    y = buf[:, :d["co"]]
    ops.gemm1x1(d["w"], t, y, d["co"], d["ci"])
    return _norm(y, d["bn"])


def _close(d, cat, t, out):
    """out = relu(t + s (W cat + b)) with s folded into W and b; out may be t."""
    ops.convkxk(d["w"], cat, out, cat.shape[1], out.shape[1], 1, 1, bias=d["b"], res=t, relu2=True)
    return out


def run_block35(d, y, buf, out):
    """Block35 on y [B, 320, h, w] into `out` (which may be y).  buf [B, 192, h, w] is laid out
    [head2 32 | head1 32 | branch0 32 | branch1 32 | branch2 64]: the merged GEMM fills the first 96 channels, the
    closer reads the concat [branch0 | branch1 | branch2] as channels 64 .. 192."""
    _heads(d["heads"], y, buf)
    _cna(d["b1"], buf[:, 32:64], buf[:, 96:128])
    _cna(d["b2"][1], _cna(d["b2"][0], buf[:, 0:32]), buf[:, 128:192])
    return _close(d["close"], buf[:, 64:192], y, out)


def run_block17(d, y, buf, out):
    """Block17 on y [B, 1088, h, w] into `out` (which may be y).  buf [B, 512, h, w] is laid out
    [head1 128 | branch0 192 | branch1 192]; the closer reads channels 128 .. 512."""
    _heads(d["heads"], y, buf)
    _cna(d["b1"][1], _cna(d["b1"][0], buf[:, 0:128]), buf[:, 320:512])
    return _close(d["close"], buf[:, 128:512], y, out)


class FPNInception(FPNInceptionDecoder):
    SYNTH_RULES = FPNMobileNet.SYNTH_RULES + ((r"\.bn\.weight$", "range", (0.6, 1.4)), (r"\.bn\.bias$", "range", (-0.3, 0.3)))
    SYNTH_SKIP = r"(running_mean|running_var|num_batches_tracked)$|^fpn\.enc\d"      # norm buffers; aliases of fpn.inception

    def __init__(self, norm_layer=None, output_ch=3, num_filters=128, num_filters_fpn=256):
        if norm_layer is None:
            import functools
            norm_layer = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=True)   # networks.py:22
        super().__init__(norm_layer, output_ch, num_filters, num_filters_fpn)
        self.fpn = _FPNFull(norm_layer, num_filters_fpn)          # the decoder's holder plus the encoder
        # An 800x800 tile (the 768/128 entry of configs.PATCH_CONFIG, padded) keeps about 0.9 GB of float32
        # activations alive at its peak - the decoder's 512 x 200 x 200 concat and 64 x 800 x 800 up-sampled maps
        # dominate, the encoder's largest are the 64 x 397 x 397 stem maps - and a 1280x720 frame is two such tiles:
        # they go in one batch; more tiles per batch only grow the workspace a graph holds (utils.graphed_forward).
        self.max_tiles_per_batch = 2
        self.hip_graph = True

    # ------------------------------------------------------------------ weights
    def _build(self):
        pk = super()._build()
        t = self.fpn.inception
        e = {n: _pack_unit(getattr(t, n)) for n in ("conv2d_1a", "conv2d_2a", "conv2d_2b", "conv2d_3b", "conv2d_4a")}
        m = t.mixed_5b
        e["mixed_5b"] = {"heads": _pack_heads(m.branch2[0], m.branch1[0], m.branch0), "b1": _pack_unit(m.branch1[1]),
                         "b2": (_pack_unit(m.branch2[1]), _pack_unit(m.branch2[2])), "b3": _pack_unit(m.branch3[1])}
        e["repeat"] = [pack_block35(b) for b in t.repeat]
        m = t.mixed_6a
        e["mixed_6a"] = {"b0": _pack_unit(m.branch0), "b1": tuple(_pack_unit(u) for u in m.branch1)}
        e["repeat_1"] = [pack_block17(b) for b in t.repeat_1]
        m = t.mixed_7a
        e["mixed_7a"] = {"heads": _pack_heads(m.branch0[0], m.branch1[0], m.branch2[0]), "b0": _pack_unit(m.branch0[1]),
                         "b1": _pack_unit(m.branch1[1]), "b2": (_pack_unit(m.branch2[1]), _pack_unit(m.branch2[2]))}
        pk["enc"] = e
        return pk

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def encode(self, x):
        """(enc0, .., enc4) of x [B, 3, H, W] on the GPU, the five maps of FPN.forward (fpn_inception.py:145-153): what
        `forward` hands to the decoder."""
        self._require_cuda(x)
        x = x.float().contiguous()
        H, W = x.shape[-2:]
        if H % 32 or W % 32 or H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"FPNInception needs H and W to be multiples of 32 and at least {MIN_SIDE} "
                             f"(deblurganv2.pad; the top map of a smaller tile cannot be reflect-padded), got {H}x{W}")
        e = self._pack()["enc"]
        enc0 = _cna(e["conv2d_1a"], x)
        enc1 = _maxpool(_cna(e["conv2d_2b"], _cna(e["conv2d_2a"], enc0)))
        enc2 = _maxpool(_cna(e["conv2d_4a"], _cna(e["conv2d_3b"], enc1)))
        # mixed_5b: buffer [head2 64 | head1 48 | branch0 96 | branch1 64 | branch2 96 | branch3 64]; the block's output
        # is channels 112 .. 432
        h, w = enc2.shape[2:]
        d = e["mixed_5b"]
        buf = _new(x, 432, h, w)
        _heads(d["heads"], enc2, buf)
        _cna(d["b1"], buf[:, 64:112], buf[:, 208:272])
        _cna(d["b2"][1], _cna(d["b2"][0], buf[:, 0:64]), buf[:, 272:368])
        pooled = _new(x, 192, h, w)
        ops.pool3x3(enc2, pooled, ops.POOL_AVG_S1)
        _cna(d["b3"], pooled, buf[:, 368:432])
        y = buf[:, 112:432]
        # repeat: the first block writes a dense map, the others run in place
        buf = _new(x, 192, h, w)
        for i, d in enumerate(e["repeat"]):
            y = run_block35(d, y, buf, _new(x, 320, h, w) if i == 0 else y)
        # mixed_6a: [branch0 384 | branch1 384 | max pool 320]
        d = e["mixed_6a"]
        h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        enc3 = _new(x, 1088, h, w)
        _cna(d["b0"], y, enc3[:, 0:384])
        _cna(d["b1"][2], _cna(d["b1"][1], _cna(d["b1"][0], y)), enc3[:, 384:768])
        _maxpool(y, enc3[:, 768:1088])
        # repeat_1: the first block leaves enc3 as it is (the decoder reads it), the others run in place
        buf = _new(x, 512, h, w)
        y = enc3
        for i, d in enumerate(e["repeat_1"]):
            y = run_block17(d, y, buf, _new(x, 1088, h, w) if i == 0 else y)
        # mixed_7a: [branch0 384 | branch1 288 | branch2 320 | max pool 1088], the three heads in one GEMM
        d = e["mixed_7a"]
        hb = _new(x, 768, h, w)
        _heads(d["heads"], y, hb)
        h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        enc4 = _new(x, 2080, h, w)
        _cna(d["b0"], hb[:, 0:256], enc4[:, 0:384])
        _cna(d["b1"], hb[:, 256:512], enc4[:, 384:672])
        _cna(d["b2"][1], _cna(d["b2"][0], hb[:, 512:768]), enc4[:, 672:992])
        _maxpool(y, enc4[:, 992:2080])
        return enc0, enc1, enc2, enc3, enc4

    @torch.no_grad()
    def forward(self, x):
        return super().forward(x, *self.encode(x))
