"""Plain torch.nn statement of DeblurGANv2's FPN-Inception generator with its Inception-ResNet-v2 encoder: the model the
GPU path (irm_amd.deblurganv2.FPNInception) is held to.  A test helper, no tests.

The encoder is written from the published architecture (Szegedy et al., "Inception-v4, Inception-ResNet and the Impact
of Residual Connections on Learning", under the layer names of the published pretrained model, which the reference
obtains as timm's `inception_resnet_v2`): every conv unit is Conv2d(bias=False) -> BatchNorm2d(eps=1e-3) -> ReLU.  The
classifier tail (repeat_2, block8, conv2d_7b, last_linear with 1000 classes) is declared so that the parameter count can
be checked against the published one, 55 843 464; FPN.forward never runs it.  The FPN and decoder half is
oracle.deblurgan_ref.fpn_inception_decoder.

The reference returns its generators in TRAIN mode and runs one tile at a time, so every norm uses the statistics of
the current tile; `forward` here normalises per (sample, channel), which is the same for one tile and keeps batched
tiles independent, as the GPU path does.

    net = build(torch.float64)            # or torch.float32
    encs = encoder_maps(net, x)           # (enc0, .., enc4)
    y = forward(net, x)                   # the generator's output
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import deblurgan_ref

PARAMS_FULL = 55_843_464          # inception_resnet_v2 with its 1000-class classifier (the published model table)
PARAMS_USED = 30_754_272          # conv2d_1a .. mixed_7a
TAIL = ("repeat_2.", "block8.", "conv2d_7b.", "last_linear.")


class C(nn.Module):
    def __init__(self, i, o, k, s=1, p=0):
        super().__init__()
        self.conv = nn.Conv2d(i, o, k, stride=s, padding=p, bias=False)
        self.bn = nn.BatchNorm2d(o, eps=1e-3)

    def forward(self, x):
        # train-mode BatchNorm on one tile = instance statistics per (sample, channel), biased variance
        y = self.conv(x)
        return F.relu(F.instance_norm(y, None, None, self.bn.weight, self.bn.bias, True, 0.1, self.bn.eps))


class Mixed5b(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = C(192, 96, 1)
        self.branch1 = nn.Sequential(C(192, 48, 1), C(48, 64, 5, 1, 2))
        self.branch2 = nn.Sequential(C(192, 64, 1), C(64, 96, 3, 1, 1), C(96, 96, 3, 1, 1))
        self.branch3 = nn.Sequential(nn.AvgPool2d(3, 1, 1, count_include_pad=False), C(192, 64, 1))

    def forward(self, x):
        return torch.cat([self.branch0(x), self.branch1(x), self.branch2(x), self.branch3(x)], 1)


class ResBlock(nn.Module):
    """relu(x + scale * conv2d(cat(branches)))"""

    def __init__(self, scale, relu=True):
        super().__init__()
        self.scale, self.relu = scale, relu

    def forward(self, x):
        y = self.conv2d(torch.cat([b(x) for b in self.branches()], 1))
        y = x + self.scale * y
        return F.relu(y) if self.relu else y


class Block35(ResBlock):
    def __init__(self):
        super().__init__(0.17)
        self.branch0 = C(320, 32, 1)
        self.branch1 = nn.Sequential(C(320, 32, 1), C(32, 32, 3, 1, 1))
        self.branch2 = nn.Sequential(C(320, 32, 1), C(32, 48, 3, 1, 1), C(48, 64, 3, 1, 1))
        self.conv2d = nn.Conv2d(128, 320, 1)

    def branches(self):
        return self.branch0, self.branch1, self.branch2


class Mixed6a(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = C(320, 384, 3, 2)
        self.branch1 = nn.Sequential(C(320, 256, 1), C(256, 256, 3, 1, 1), C(256, 384, 3, 2))
        self.branch2 = nn.MaxPool2d(3, 2)

    def forward(self, x):
        return torch.cat([self.branch0(x), self.branch1(x), self.branch2(x)], 1)


class Block17(ResBlock):
    def __init__(self):
        super().__init__(0.10)
        self.branch0 = C(1088, 192, 1)
        self.branch1 = nn.Sequential(C(1088, 128, 1), C(128, 160, (1, 7), 1, (0, 3)), C(160, 192, (7, 1), 1, (3, 0)))
        self.conv2d = nn.Conv2d(384, 1088, 1)

    def branches(self):
        return self.branch0, self.branch1


class Mixed7a(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = nn.Sequential(C(1088, 256, 1), C(256, 384, 3, 2))
        self.branch1 = nn.Sequential(C(1088, 256, 1), C(256, 288, 3, 2))
        self.branch2 = nn.Sequential(C(1088, 256, 1), C(256, 288, 3, 1, 1), C(288, 320, 3, 2))
        self.branch3 = nn.MaxPool2d(3, 2)

    def forward(self, x):
        return torch.cat([self.branch0(x), self.branch1(x), self.branch2(x), self.branch3(x)], 1)


class Block8(ResBlock):
    def __init__(self, relu=True):
        super().__init__(0.20 if relu else 1.0, relu)
        self.branch0 = C(2080, 192, 1)
        self.branch1 = nn.Sequential(C(2080, 192, 1), C(192, 224, (1, 3), 1, (0, 1)), C(224, 256, (3, 1), 1, (1, 0)))
        self.conv2d = nn.Conv2d(448, 2080, 1)

    def branches(self):
        return self.branch0, self.branch1


class InceptionResNetV2(nn.Module):
    def __init__(self, classes=1000):
        super().__init__()
        self.conv2d_1a = C(3, 32, 3, 2)
        self.conv2d_2a = C(32, 32, 3, 1)
        self.conv2d_2b = C(32, 64, 3, 1, 1)
        self.maxpool_3a = nn.MaxPool2d(3, 2)
        self.conv2d_3b = C(64, 80, 1)
        self.conv2d_4a = C(80, 192, 3, 1)
        self.maxpool_5a = nn.MaxPool2d(3, 2)
        self.mixed_5b = Mixed5b()
        self.repeat = nn.Sequential(*[Block35() for _ in range(10)])
        self.mixed_6a = Mixed6a()
        self.repeat_1 = nn.Sequential(*[Block17() for _ in range(20)])
        self.mixed_7a = Mixed7a()
        # the tail: in the checkpoint, never run by FPN.forward
        self.repeat_2 = nn.Sequential(*[Block8() for _ in range(9)])
        self.block8 = Block8(relu=False)
        self.conv2d_7b = C(2080, 1536, 1)
        self.last_linear = nn.Linear(1536, classes)


class FPN(nn.Module):
    def __init__(self, norm_layer, num_filters=256):
        super().__init__()
        self.inception = t = InceptionResNetV2()
        self.enc0 = t.conv2d_1a
        self.enc1 = nn.Sequential(t.conv2d_2a, t.conv2d_2b, t.maxpool_3a)
        self.enc2 = nn.Sequential(t.conv2d_3b, t.conv2d_4a, t.maxpool_5a)
        self.enc3 = nn.Sequential(t.mixed_5b, t.repeat, t.mixed_6a)
        self.enc4 = nn.Sequential(t.repeat_1, t.mixed_7a)
        for name in ("td1", "td2", "td3"):
            setattr(self, name, nn.Sequential(nn.Conv2d(num_filters, num_filters, 3, padding=1), norm_layer(num_filters),
                                              nn.ReLU(inplace=True)))
        for i, c in enumerate((32, 64, 192, 1088, 2080)):
            setattr(self, f"lateral{i}", nn.Conv2d(c, num_filters // 2 if i == 0 else num_filters, 1, bias=False))


class Head(nn.Module):
    def __init__(self, num_in, num_mid, num_out):
        super().__init__()
        self.block0 = nn.Conv2d(num_in, num_mid, 3, padding=1, bias=False)
        self.block1 = nn.Conv2d(num_mid, num_out, 3, padding=1, bias=False)


class FPNInceptionNet(nn.Module):
    """Parameter holder under the checkpoint's names; `forward(net, x)` below runs it."""

    def __init__(self, num_filters=128, num_filters_fpn=256, output_ch=3):
        super().__init__()
        norm = lambda c: nn.InstanceNorm2d(c, affine=False, track_running_stats=True)      # noqa: E731
        self.fpn = FPN(norm, num_filters_fpn)
        for i in (1, 2, 3, 4):
            setattr(self, f"head{i}", Head(num_filters_fpn, num_filters, num_filters))
        self.smooth = nn.Sequential(nn.Conv2d(4 * num_filters, num_filters, 3, padding=1), norm(num_filters), nn.ReLU())
        self.smooth2 = nn.Sequential(nn.Conv2d(num_filters, num_filters // 2, 3, padding=1), norm(num_filters // 2), nn.ReLU())
        self.final = nn.Conv2d(num_filters // 2, output_ch, 3, padding=1)


def build(dtype=torch.float64, state_dict=None):
    """The network in `dtype`, in train mode like the reference's generators; state_dict: weights to load (the tail's
    keys may be missing: they keep their initial values, nothing reads them)."""
    net = FPNInceptionNet()
    if state_dict is not None:
        missing, unexpected = net.load_state_dict(state_dict, strict=False)
        assert not unexpected, unexpected
        assert all(is_tail(k) or k.endswith("num_batches_tracked") or "running_" in k for k in missing), missing
    return net.to(dtype).train(True)


def is_tail(key):
    return key.startswith("fpn.inception.") and key[len("fpn.inception."):].startswith(TAIL)


@torch.no_grad()
def encoder_maps(net, x):
    f = net.fpn
    enc0 = f.enc0(x)
    enc1 = f.enc1(enc0)
    enc2 = f.enc2(enc1)
    enc3 = f.enc3(enc2)
    enc4 = f.enc4(enc3)
    return enc0, enc1, enc2, enc3, enc4


@torch.no_grad()
def forward(net, x, encs=None):
    """The generator's output for x [B, 3, H, W] in the dtype of `net`; encs: maps already computed by encoder_maps."""
    p = {k: v for k, v in net.state_dict().items() if not k.startswith("fpn.inception.") and not k.startswith("fpn.enc")}
    return deblurgan_ref.fpn_inception_decoder(x, encs if encs is not None else encoder_maps(net, x), p)


def map_sides(side):
    """Sides of the five maps of an input side of 32 k: 16k-1, 8k-2, 4k-3, 2k-2, k-2."""
    k = side // 32
    return 16 * k - 1, 8 * k - 2, 4 * k - 3, 2 * k - 2, k - 2
