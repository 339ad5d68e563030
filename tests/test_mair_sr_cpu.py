"""MaIR super resolution, host side: the SR heads' state_dict against the reference class (shapes recorded by
tools/gen_golden_mair_sr.py from the imported reference), the constructor's refusals, the loader, and the tile
geometry of the tiled call at output scale (scaled origins, crop, window) against a numpy restatement."""
import json
import os

import numpy as np
import pytest
import torch

from irm_amd import mair, utils
from irm_amd.mair import mair_arch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sr_meta():
    with open(os.path.join(GOLDEN, "mair_sr.json")) as f:
        return json.load(f)


def test_sr_state_dict_matches_reference(sr_meta):
    assert len(sr_meta["configs"]) == 7
    for name, cfg in sr_meta["configs"].items():
        m = mair.MaIR(**cfg)
        got = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert got == sr_meta["param_shapes"][name], name
        assert m.upscale == cfg["upscale"]


def test_sr_head_keys():
    light = mair.MaIR(embed_dim=60, depths=[1], d_state=1, ssm_ratio=1.1, upscale=3)     # the class defaults' branch
    keys = {k for k in light.state_dict() if not k.startswith(("layers.", "patch_embed.", "norm.", "conv_first.",
                                                               "conv_after_body."))}
    assert keys == {"upsample.0.weight", "upsample.0.bias"}
    assert tuple(light.upsample[0].weight.shape) == (27, 60, 3, 3)
    c8 = mair.MaIR(embed_dim=36, depths=[1], upscale=8, upsampler='pixelshuffle')
    keys = {k for k in c8.state_dict() if k.startswith(("upsample.", "conv_before_upsample.", "conv_last."))}
    assert keys == {f"upsample.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")} | \
        {"conv_before_upsample.0.weight", "conv_before_upsample.0.bias", "conv_last.weight", "conv_last.bias"}
    assert c8.upscale == 8 and c8.ps_factors == [2, 2, 2]
    den = mair.MaIR(embed_dim=36, depths=[1], upscale=1, upsampler=None)
    assert den.upscale == 1 and not hasattr(den, "upsample")


@pytest.mark.parametrize("scale", [5, 6, 7, 12])
def test_classical_sr_rejects_scales_like_the_reference(scale):
    with pytest.raises(ValueError, match="Supported scales: 2\\^n and 3"):
        mair.MaIR(embed_dim=36, depths=[1], upscale=scale, upsampler='pixelshuffle')


def test_sr_refusals():
    with pytest.raises(NotImplementedError):
        mair.MaIR(embed_dim=36, depths=[1], upscale=5)                       # pixelshuffledirect: 2, 3, 4 only
    with pytest.raises(NotImplementedError):
        mair.MaIR(embed_dim=36, depths=[1], upscale=2, resi_connection='3conv')
    with pytest.raises(NotImplementedError):
        mair.MaIR(embed_dim=36, depths=[1], upscale=2, upsampler='pixelshuffle', resi_connection='3conv')
    with pytest.raises(NotImplementedError):
        mair.MaIR(embed_dim=36, depths=[1], upscale=2, patch_size=2)
    with pytest.raises(NotImplementedError):
        mair.MaIR(embed_dim=36, depths=[1], upscale=2, upsampler='nearest+conv')
    for s in (2, 3, 4):
        assert mair.MaIR(embed_dim=36, depths=[1], upscale=s).upscale == s
    for s in (1, 2, 3, 4, 8):
        assert mair.MaIR(embed_dim=36, depths=[1], upscale=s, upsampler='pixelshuffle').upscale == s


def test_sr_need_degradation_raises():
    m = mair.MaIR(embed_dim=36, depths=[1], upscale=2)
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="no SR degradation"):
        utils.get_model_prediction(m, img, torch.device("cpu"), 16, 4, need_degradation=True, noise_level=15)


@pytest.mark.parametrize("prefix", ["", "module."])
def test_get_model_sr_option_file(tmp_path, prefix):
    net_g = dict(type="MaIR", upscale=3, in_chans=3, img_size=64, img_range=1.0, d_state=1, depths=[2, 2], embed_dim=60,
                 ssm_ratio=1.1, mlp_ratio=1.6, upsampler="pixelshuffledirect", resi_connection="1conv", scan_len=4)
    src = mair.MaIR(**{k: v for k, v in net_g.items() if k != "type"}).load_synthetic(5)
    wpath = tmp_path / "MaIR_SR_x3.pth"
    torch.save({"params": {prefix + k: v for k, v in src.state_dict().items()}}, wpath)
    yml = tmp_path / "test_MaIR_SR_x3.yml"
    opt = {"name": "MaIR_SR_x3", "num_gpu": 0, "network_g": net_g,
           "path": {"pretrain_network_g": str(wpath), "strict_load_g": True}}
    import yaml
    yml.write_text(yaml.safe_dump(opt))
    got = mair.get_model(str(yml))
    assert isinstance(got, mair.MaIR) and got.upscale == 3 and not got.training
    sd = got.state_dict()
    assert sd.keys() == src.state_dict().keys()
    assert all(torch.equal(sd[k], v) for k, v in src.state_dict().items())


class _NearestUp(torch.nn.Module):
    """CPU stand-in of an SR model for the tile geometry: nearest upsampling by `upscale` plus a position ramp, so a
    misplaced tile or a wrong crop changes the blend."""

    def __init__(self, s):
        super().__init__()
        self.upscale = s

    def forward(self, x):
        y = x.repeat_interleave(self.upscale, 2).repeat_interleave(self.upscale, 3)
        ramp = torch.arange(y.shape[-1], dtype=y.dtype) / 512.0
        return y * 0.75 + ramp


def _numpy_sr_blend(img_u8, s, ps, ov):
    """Restatement of the tiled call at output scale: tiles cut at input scale (utils.tile_origins), each prediction
    cropped to s*th x s*tw and placed at s*origin, Gaussian window of s*ps, / weight, requantise."""
    x = img_u8.astype(np.float32) / 255.0
    h, w = x.shape[:2]
    ps = min(ps, max(h, w))
    ys, xs = utils.tile_origins(h, ps, ov), utils.tile_origins(w, ps, ov)
    win = utils.get_gaussian_weights(s * ps, s * ps, 3)
    acc = np.zeros((s * h, s * w, 3), np.float32)
    wsum = np.zeros_like(acc)
    for y0 in ys:
        for x0 in xs:
            t = x[y0:y0 + ps, x0:x0 + ps]
            th, tw = t.shape[:2]
            up = np.repeat(np.repeat(t, s, 0), s, 1)
            ramp = (np.arange(up.shape[1], dtype=np.float32) / np.float32(512.0))[None, :, None]
            p = up * np.float32(0.75) + ramp
            assert p.shape[:2] == (s * th, s * tw)
            acc[s * y0:s * (y0 + th), s * x0:s * (x0 + tw)] += p * win[:s * th, :s * tw]
            wsum[s * y0:s * (y0 + th), s * x0:s * (x0 + tw)] += win[:s * th, :s * tw]
    acc /= np.maximum(wsum, 1e-8)
    return np.clip(acc * 255.0, 0, 255).round().astype(np.uint8)


@pytest.mark.parametrize("s,h,w,ps,ov", [(2, 37, 53, 16, 4), (3, 24, 40, 16, 8), (4, 20, 20, 32, 8)])
def test_sr_tile_geometry_vs_numpy(s, h, w, ps, ov):
    rng = np.random.default_rng(s * 100 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    model = _NearestUp(s)
    got = utils._run_tiles_on_host(model, img, torch.device("cpu"), utils.normalize, ps, ov, False, None, None, None)
    want = _numpy_sr_blend(img, s, ps, ov)
    assert got.shape == (s * h, s * w, 3)
    assert np.array_equal(got, want)


def test_sr_tile_geometry_padded_crop():
    """With the reflect pad to 8 (MaIR's path) the prediction of a padded tile is cropped to s * the unpadded size."""
    s, h, w = 2, 21, 30
    img = np.random.default_rng(3).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = utils._run_tiles_on_host(_NearestUp(s), img, torch.device("cpu"), utils.normalize, 13, 3, False, None,
                                   utils.pad, None)
    # nearest upsampling is local: the padded rows/columns never reach the crop, so the result equals the unpadded one
    assert np.array_equal(got, _numpy_sr_blend(img, s, 13, 3))


def test_upsample_factors():
    assert mair_arch._upsample_factors(1) == [] and mair_arch._upsample_factors(2) == [2]
    assert mair_arch._upsample_factors(4) == [2, 2] and mair_arch._upsample_factors(3) == [3]


def test_scan_plan_for_the_direction_channel_lane_mapping():
    from irm_amd import ops
    assert ops.scan_is_flat(66, 1, 4) and ops.scan_is_flat(90, 16, 4)
    assert not ops.scan_is_flat(128, 1, 4) and not ops.scan_is_flat(234, 16, 12) and not ops.scan_is_flat(90, 16, 12)
    for B, L, D in ((1, 57600, 66), (1, 57600, 90), (8, 128 * 128, 66), (1, 240, 66), (3, 99, 90)):
        assert ops.scan_plan(B, L, D) == ops.scan_plan(B, L, D, flat=False)
        chunk, nchunk, DB = ops.scan_plan(B, L, D, flat=True)
        assert DB == -(-D // 64) and chunk % 8 == 0 and chunk >= 32
        assert nchunk == -(-L // chunk) and (nchunk - 1) * chunk < L
        assert nchunk >= ops.scan_plan(B, L, D)[1]              # fewer waves per chunk: at least as many chunks
