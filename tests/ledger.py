"""The machinery of the model-level precision ledger: its cases, the model builds, the CPU oracles and the GPU runs.
tests/test_gpu_precision.py runs the cases on seeded noise, tests/test_gpu_degenerate_models.py on frames, and
tests/test_degenerate_cpu.py checks the oracles on those frames without a GPU.

The cases take every dispatch outcome of restormer.py at least once (fused C = 48 / 96 blocks with and without the Gram
in the qkv kernel and the tile-major chain between them, C = 192 with presplit + GDFN tail / presplit only / neither,
C = 384 presplit / split-only / unsplit, the two branches of ops.mdta_plan, both reduce_chan GEMMs, the dual-pixel
skip_conv, the strictly-f32 IRM_GEMM_EXACT=1 leg), plus the conv nets, both DeblurGANv2 paths and both MaIR models."""
import torch

from block_model import F, K, passes  # noqa: F401  (the ledger's bar, for the files that go through this module)
from irm_amd import _hip, deblurganv2, dncnn, mair, ops, rednet, restormer, synth
from oracle import convnets_ref, deblurgan_ref, mair_ref, restormer_ref

NET_G = dict(inp_channels=3, out_channels=3, dim=48, num_blocks=[4, 6, 6, 8], num_refinement_blocks=4, ssm_ratio=2.0,
             flp_ratio=4.0, mlp_ratio=1.5, bias=False, dual_pixel_task=False, img_size=128, scan_len=4, batch_size=8,
             dynamic_ids=False)
FLAT_CFG = dict(upscale=1, in_chans=3, img_range=1., d_state=16, depths=[2, 2], embed_dim=180, ssm_ratio=1.3, mlp_ratio=2.0,
                upsampler=None, resi_connection='1conv', img_size=16, dynamic_ids=False, batch_size=1, scan_len=4)
FI_ENC = ((32, 63, 79), (64, 30, 38), (192, 13, 17), (1088, 6, 8), (2080, 2, 3))     # FPN-Inception maps of a 128x160 input


def _restormer(ln, cin=3, cout=3, dp=False):
    return lambda: restormer.Restormer(inp_channels=cin, out_channels=cout, LayerNorm_type=ln, dual_pixel_task=dp)


class _Block(torch.nn.Module):
    """One TransformerBlock run through the product path (Restormer._pack + _run_stage), weights seeded as in
    test_gpu_models.test_transformer_block_product_path_vs_golden."""

    def __init__(self, c, heads, ln="WithBias"):
        super().__init__()
        self.host = restormer.Restormer(LayerNorm_type=ln)
        self.host.encoder_level1 = torch.nn.Sequential(restormer.restormer.TransformerBlock(c, heads, 2.66, False, ln))

    def load_synthetic(self, seed=42):
        blk = self.host.encoder_level1[0]
        shapes = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
        blk.load_state_dict(synth.synth_state_dict(shapes, seed=seed, rules=restormer.restormer.SYNTH_RULES))
        return self

    def state_dict(self, *args, **kw):
        return self.host.encoder_level1[0].state_dict(*args, **kw)

    def forward(self, x):
        y = x.clone()
        self.host._run_stage("encoder_level1", self.host._pack(), y)
        return y


# name -> (model factory, input shape, input range, oracle(x, state dict, tap), environment)
CASES = {}
for _ln, _t in (("WithBias", "wb"), ("BiasFree", "bf")):
    for _shape in ((1, 3, 128, 128), (1, 3, 64, 64), (1, 3, 40, 56), (3, 3, 64, 72)):
        CASES[f"restormer_{_t}_{_shape[2]}x{_shape[3]}_b{_shape[0]}"] = (
            _restormer(_ln), _shape, (0.0, 1.0), lambda x, p, tap: restormer_ref.restormer_forward(x, p, tap=tap), {})
CASES["restormer_gray_bf_64x64_b1"] = (_restormer("BiasFree", 1, 1), (1, 1, 64, 64), (0.0, 1.0),
                                       lambda x, p, tap: restormer_ref.restormer_forward(x, p, tap=tap), {})
CASES["restormer_dualpixel_wb_64x64_b1"] = (
    _restormer("WithBias", 6, 3, True), (1, 6, 64, 64), (0.0, 1.0),
    lambda x, p, tap: restormer_ref.restormer_forward(x, p, dual_pixel_task=True, tap=tap), {})
CASES["restormer_wb_128x128_b1_exact"] = (_restormer("WithBias"), (1, 3, 128, 128), (0.0, 1.0),
                                          lambda x, p, tap: restormer_ref.restormer_forward(x, p, tap=tap),
                                          {"IRM_GEMM_EXACT": "1"})
# every level on the per-op kernels (dwgemm_f16x3 at C <= 96), the path of a dim that is not a multiple of 16:
# build patches ops.can_fuse_gdfn to refuse the whole-branch kernels
CASES["restormer_wb_64x64_b1_unfused"] = (_restormer("WithBias"), (1, 3, 64, 64), (0.0, 1.0),
                                          lambda x, p, tap: restormer_ref.restormer_forward(x, p, tap=tap), {})
# a checkpoint whose level-1 project_out weights fall under the split guard (_hip.split_is_safe: max|W| < 2^-6): the
# fused C = 48 blocks keep the folded attention on the exact f32 MFMA and run the plain GDFN kernel (gdfn_fused)
CASES["restormer_wb_64x64_b1_tiny_project_out"] = (_restormer("WithBias"), (1, 3, 64, 64), (0.0, 1.0),
                                                   lambda x, p, tap: restormer_ref.restormer_forward(x, p, tap=tap), {})
# one C = 192 block on enough pixels (B * N = 81920) that the K = 192 pre-split GEMM plans one workgroup per pixel
# block (_hip.plan_presplit): LayerNorm + split inside the GEMM (irm_ln_gemm_presplit_f16x3_f32), as on 512^2 tiles
CASES["restormer_block_c192_h4_64x40_b32"] = (lambda: _Block(192, 4), (32, 192, 64, 40), (-1.0, 1.0),
                                              lambda x, p, tap: restormer_ref.transformer_block(x, p, "", 4), {})
CASES["dncnn_gray17_37x53_b2"] = (lambda: dncnn.DnCNN(1, 1, 64, 17, "R"), (2, 1, 37, 53), (0.0, 1.0),
                                  lambda x, p, tap: convnets_ref.dncnn_forward(x, p), {})
CASES["dncnn_color20_29x45_b1"] = (lambda: dncnn.DnCNN(3, 3, 64, 20, "R"), (1, 3, 29, 45), (0.0, 1.0),
                                   lambda x, p, tap: convnets_ref.dncnn_forward(x, p), {})
CASES["rednet_33x45_b1"] = (lambda: rednet.REDNet(), (1, 1, 33, 45), (0.0, 1.0),
                            lambda x, p, tap: convnets_ref.rednet_forward(x, p), {})
CASES["fpn_mobilenet_96x160_b1"] = (lambda: deblurganv2.FPNMobileNet().train(True), (1, 3, 96, 160), (-1.0, 1.0),
                                    lambda x, p, tap: deblurgan_ref.fpn_mobilenet_forward(x, p), {})
CASES["fpn_inception_decoder_128x160_b1"] = (lambda: deblurganv2.FPNInceptionDecoder().train(True), (1, 3, 128, 160),
                                             (-1.0, 1.0), None, {})
for _shape in ((1, 3, 32, 32), (1, 3, 24, 40), (2, 3, 64, 64)):
    CASES[f"mairunet_{_shape[2]}x{_shape[3]}_b{_shape[0]}"] = (
        lambda: mair.MaIRUNet(**NET_G), _shape, (0.0, 1.0), lambda x, p, tap: mair_ref.mairunet_forward(x, p), {})
for _shape in ((1, 3, 16, 16), (1, 3, 24, 20)):
    CASES[f"mair_flat_{_shape[2]}x{_shape[3]}_b{_shape[0]}"] = (
        lambda: mair.MaIR(**FLAT_CFG), _shape, (0.0, 1.0), lambda x, p, tap: mair_ref.mair_forward(x, p), {})

_ORACLE = {}       # case, or (case, frame) -> {row: (y64, e_32)}: float64 and fp32 oracle runs, once per process


def inputs(case):
    _, shape, (lo, hi), _, _ = CASES[case]
    x = synth.uniform(7, f"ledger_{case}", shape, lo, hi)
    if case.startswith("fpn_inception"):
        encs = [synth.uniform(7, f"ledger_{case}_enc{i}", (shape[0],) + c, -1.0, 1.0) for i, c in enumerate(FI_ENC)]
        return x, encs
    return x, None


def cpu_params(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def f64(p):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}


def oracle(case, p, frame=None, x=None):
    """{row: (y64, e_32)} of a case: 'out', and for Restormer also 'refinement' (the trunk before the output conv,
    whose gain 0.02 attenuates the trunk's error in the output).  frame, x: another input than the case's seeded noise
    (tests/test_gpu_degenerate_models.py), cached under (case, frame)."""
    key = case if frame is None else (case, frame)
    if key not in _ORACLE:
        fn = CASES[case][3]
        x, encs = inputs(case) if frame is None else (x, None)
        res = {}
        with torch.no_grad():
            for dt, pp in ((torch.float32, p), (torch.float64, f64(p))):
                tap = {}
                if encs is not None:
                    y = deblurgan_ref.fpn_inception_decoder(x.to(dt), [e.to(dt) for e in encs], pp)
                else:
                    y = fn(x.to(dt), pp, tap)
                res[dt] = dict(out=y, **tap)
        _ORACLE[key] = {r: (res[torch.float64][r], float((res[torch.float32][r].double() - res[torch.float64][r]).abs().max()))
                         for r in res[torch.float64]}
    return _ORACLE[key]


def run_gpu(case, dev, model, tap, x=None):
    x, encs = inputs(case) if x is None else (x, None)
    if tap:
        model._tap = {}
    with torch.no_grad():
        if encs is not None:
            y = model(x.to(dev), *[e.to(dev) for e in encs])
        else:
            y = model(x.to(dev))
    out = dict(out=y.cpu().double())
    if tap:
        out["refinement"] = model._tap["refinement"].cpu().double()
    return out


def build(case, dev, monkeypatch):
    for k, v in CASES[case][4].items():
        monkeypatch.setenv(k, v)
    if case.endswith("_unfused"):
        monkeypatch.setattr(ops, "can_fuse_gdfn", lambda C, W: False)
    model = CASES[case][0]().load_synthetic(42)
    if case.endswith("_tiny_project_out"):
        with torch.no_grad():
            for blk in model.encoder_level1:
                blk.attn.project_out.weight.mul_(2.0 ** -8)
        assert not _hip.split_is_safe(model.encoder_level1[0].attn.project_out.weight)
    p = cpu_params(model)
    return model.to(dev), p
