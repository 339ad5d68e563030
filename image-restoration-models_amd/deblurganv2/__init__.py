"""DeblurGANv2 (FPN-MobileNet and FPN-Inception generators) on MI355X - call surface of
src/deblurganv2/__init__.py:11-41, plus get_model_inception for the FPN-Inception checkpoint."""

#: synthetic-weight rules (synth.py)
SYNTH_RULES = (
    (r"^final\.weight$", "gain", 0.3),
    (r"features\.\d+\.(\d+\.)?(conv\.)?\d+\.weight$", "gain", 1.4),
)

import os as _os
import re as _re

import numpy as _np
import torch as _torch

from .models.fpn_mobilenet import FPNMobileNet  # noqa: E402
from .models.fpn_inception import INCEPTION_TAIL, FPNInception, FPNInceptionDecoder  # noqa: E402

__all__ = ["FPNMobileNet", "FPNInception", "FPNInceptionDecoder", "get_model", "get_model_inception", "normalize", "pad",
           "postprocess", "SYNTH_RULES"]


def normalize(x: _np.ndarray):
    """albumentations Normalize(mean=.5, std=.5) (aug.py:31-39): (x - 127.5) * (1/127.5) in float32.
    Restated from the library's published arithmetic (albumentations is not installed: unpinned)."""
    mean = _np.float32(0.5) * _np.float32(255.0)
    denom = _np.float32(1.0) / (_np.float32(0.5) * _np.float32(255.0))
    return ((x.astype(_np.float32) - mean) * denom).astype(_np.float32)


def pad(x: _torch.Tensor):
    """src/deblurganv2/__init__.py:16-24: zero pad to (h//32+1)*32 - always at least one more block."""
    h, w = x.shape[-2:]
    return _torch.nn.functional.pad(x, (0, (w // 32 + 1) * 32 - w, 0, (h // 32 + 1) * 32 - h), 'constant', 0)


def postprocess(x: _torch.Tensor):
    return (x + 1) / 2.0


def get_model(weights_path: str, device: _torch.device):
    """src/deblurganv2/__init__.py:31-41: generator name = file stem; checkpoint['model'] carries the
    DataParallel 'module.' prefix; the model is returned in TRAIN mode like the reference."""
    name = _os.path.basename(weights_path).split('.')[0]
    if name != 'fpn_mobilenet':
        raise NotImplementedError(f"generator {name!r}: this loader builds fpn_mobilenet only.  The FPN-Inception generator "
                                  "(deblurganv2.FPNInception) is loaded with deblurganv2.get_model_inception(weights_path, "
                                  "device)")
    model = FPNMobileNet()
    sd = _torch.load(weights_path, map_location="cpu", weights_only=True)['model']
    model.load_state_dict({(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()})
    model.to(device)
    model.train(True)
    print(f"Successfully loaded {_np.sum([p.numel() for p in model.parameters()]):,} parameters from {weights_path}")
    return model


def get_model_inception(weights_path: str, device: _torch.device):
    """The FPN-Inception generator from a reference checkpoint ({'model': state_dict}, keys maybe with the DataParallel
    'module.' prefix).  The keys of the classifier tail of inception_resnet_v2 (repeat_2, block8, conv2d_7b,
    last_linear), which FPN.forward never runs, are dropped; everything else loads strictly.  Returned in TRAIN mode
    like the reference's generators (src/deblurganv2/__init__.py:38)."""
    model = FPNInception()
    sd = _torch.load(weights_path, map_location="cpu", weights_only=True)['model']
    sd = {(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()}
    model.load_state_dict({k: v for k, v in sd.items() if not _re.search(INCEPTION_TAIL, k)})
    model.to(device)
    model.train(True)
    print(f"Successfully loaded {_np.sum([p.numel() for p in model.parameters()]):,} parameters from {weights_path}")
    return model
