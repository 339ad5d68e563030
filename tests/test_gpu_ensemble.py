"""x8 self-ensemble with partitioned forward (MaIR+) on the GPU: the chop kernel bit exact against the torch
composition, the merge kernel against a float64 restatement, SelfEnsemble / MaIRPlus against the reference goldens
(tools/gen_golden_mair_plus.py), batch independence, graph replay, the tiled public surface and admissibility."""
import json
import os

import numpy as np
import pytest
import torch

from frame_checks import merge_float64, packed_blocks
from irm_amd import _hip, dncnn, ensemble, mair, ops, restormer, synth, utils

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(777, name, shape, lo, hi)


@pytest.fixture(scope="module")
def plus_meta():
    with open(os.path.join(GOLDEN, "mair_plus.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plus_golden(plus_meta):
    """name -> array: the row bands `name@first_row` of the mair_plus*.npz files joined in row order."""
    bands = {}
    for fname in plus_meta["files"]:
        with np.load(os.path.join(GOLDEN, fname)) as z:
            for key in z.files:
                name, r = key.split("@")
                bands.setdefault(name, []).append((int(r), z[key]))
    return {name: np.concatenate([a for _, a in sorted(b, key=lambda t: t[0])], axis=-2) for name, b in bands.items()}


class Identity(torch.nn.Module):
    def forward(self, x):
        return x


class ShuffleHead(torch.nn.Module):
    """Conv2d(3, 3 s^2, 3, padding=1) + PixelShuffle(s) as one irm_conv3x3 launch with the shuffle epilogue."""

    def __init__(self, s, rules):
        super().__init__()
        self.upscale = s
        self.conv = torch.nn.Conv2d(3, 3 * s * s, 3, padding=1)
        sd = synth.synth_state_dict({"0.weight": (3 * s * s, 3, 3, 3), "0.bias": (3 * s * s,)}, seed=42,
                                    rules=tuple((p, k, tuple(a)) for p, k, a in rules))
        self.conv.load_state_dict({"weight": sd["0.weight"], "bias": sd["0.bias"]})
        self._packed = None

    @torch.no_grad()
    def forward(self, x):
        if self._packed is None:
            self._packed = (_hip.pack_conv3x3(self.conv.weight), self.conv.bias.detach().float().contiguous())
        B, _, H, W = x.shape
        s = self.upscale
        y = torch.empty(B, 3, s * H, s * W, dtype=torch.float32, device=x.device)
        ops.conv3x3(self._packed[0], x, y, 3, 3 * s * s, bias=self._packed[1], store_mode=2, shuffle=s)
        return y


# --------------------------------------------------------------------------- 1. chop kernel: pure data movement
@pytest.mark.parametrize("B,C,H,W,chop", [(2, 3, 230, 410, True), (1, 1, 199, 200, True), (1, 3, 401, 33, True),
                                          (2, 3, 64, 210, True), (1, 2, 203, 467, True), (2, 3, 37, 53, False),
                                          (1, 3, 12, 20, False), (1, 1, 2, 2, False)])
def test_chop_kernel_bit_exact(dev, B, C, H, W, chop):
    x = rnd(f"chop{B}{C}{H}{W}", (B, C, H, W)).to(dev)
    geo = ensemble.geometry(B, H, W, chop)
    table = torch.from_numpy(geo.table).to(dev)
    packed = torch.full((geo.total_pixels * C,), float("nan"), device=dev)
    ensemble.dihedral_chop(x, table, packed, geo)
    blocks = packed_blocks(packed, geo, B, C)
    for v in range(8):
        want = ensemble.chop_torch(x, v, chop)
        assert len(want) == len(blocks[v])
        for i, (a, b) in enumerate(zip(blocks[v], want)):
            assert a.shape == b.shape and torch.equal(a, b), (v, i)


def test_kernels_reject_bad_arguments(dev):
    t = torch.zeros(64, device=dev)
    tab = torch.zeros(9 * 8, dtype=torch.int32, device=dev)
    for args in ((t, tab, t, 0, 1, 1, 4, 4, 1, 4, 4), (t, tab, t, 16, 1, 1, 4, 4, 0, 4, 4), (t, tab, t, 16, 1, 1, 4, 4, 1, 0, 4),
                 (t, tab, t, 16, 70000, 1, 4, 4, 1, 4, 4)):
        with pytest.raises(_hip.HipLibraryError, match="invalid arguments"):
            _hip.call("irm_dihedral_chop_f32", *[_hip.ptr(a) if torch.is_tensor(a) else a for a in args])
    for args in ((t, tab, t, 16, 1, 1, 4, 4, 1, 5), (t, tab, t, 16, 1, 1, 4, 4, 1, 0), (t, tab, t, 0, 1, 1, 4, 4, 1, 1)):
        with pytest.raises(_hip.HipLibraryError, match="invalid arguments"):
            _hip.call("irm_ensemble_merge_f32", *[_hip.ptr(a) if torch.is_tensor(a) else a for a in args])


# --------------------------------------------------------------------------- 2. merge kernel vs float64
@pytest.mark.parametrize("B,Co,H,W,s,chop", [(2, 3, 230, 410, 1, True), (1, 3, 230, 410, 2, True), (2, 2, 64, 210, 3, True),
                                             (1, 3, 64, 210, 4, True), (1, 1, 401, 33, 2, True), (2, 3, 37, 53, 3, False),
                                             (1, 3, 203, 467, 1, True)])
def test_merge_kernel_vs_float64(dev, B, Co, H, W, s, chop):
    """|err| <= 2^-21 max|v|: seven fp32 additions of partial sums bounded by 8 max|v|, then an exact x 0.125, give
    7 * 2^-24 max|v|; rounded up to 8."""
    geo = ensemble.geometry(B, H, W, chop)
    pred = rnd(f"merge{B}{Co}{H}{W}{s}", (geo.total_pixels * Co * s * s,), -3.0, 3.0)
    want = merge_float64([[b.double().numpy() for b in bl] for bl in packed_blocks(pred, geo, B, Co, s)], H, W, s, chop)
    out = torch.full((B, Co, s * H, s * W), float("nan"), device=dev)
    ensemble.ensemble_merge(pred.to(dev), torch.from_numpy(geo.table).to(dev), out, geo, s)
    got = out.cpu().double().numpy()
    vmax = float(pred.abs().max())
    err = float(np.abs(got - want).max())
    print(f"merge B{B} Co{Co} {H}x{W} x{s} chop={chop}: max-abs vs float64 {err:.3e}, bound {2.0 ** -21 * vmax:.3e}")
    assert err <= 2.0 ** -21 * vmax


@pytest.mark.parametrize("B,C,H,W", [(2, 3, 230, 410), (1, 3, 720, 1280), (1, 1, 199, 200), (3, 2, 12, 20)])
def test_identity_network_returns_the_input_bit_for_bit(dev, B, C, H, W):
    """The mean of 8 equal values is exact in the merge's summation order (2x, 4x, 8x, x 0.125)."""
    x = rnd(f"ident{B}{C}{H}{W}", (B, C, H, W)).to(dev)
    assert torch.equal(ensemble.SelfEnsemble(Identity(), chop=True)(x), x)
    assert torch.equal(ensemble.SelfEnsemble(Identity(), chop=False)(x), x)
    assert torch.equal(mair.MaIRPlus(Identity())(x), x)


# --------------------------------------------------------------------------- 3. end to end vs the reference goldens
def plus_input(name, h, w):
    return synth.uniform(7, f"mair_plus_in_{name}_{h}x{w}", (1, 3, h, w), 0.0, 1.0)


def test_dncnn_in_mairplus_vs_golden(dev, plus_meta, plus_golden):
    """Bound: tests/test_gpu_models.py::test_dncnn_vs_golden (TOL = 1e-3)."""
    nb, (h, w) = plus_meta["dncnn"]["layers"], plus_meta["dncnn"]["input"]
    net = dncnn.DnCNN(3, 3, 64, nb, "R").load_synthetic(42).eval().to(dev)
    y = mair.MaIRPlus(net)(plus_input("dncnn", h, w).to(dev)).cpu().numpy()
    g = plus_golden[f"dncnn{nb}_{h}x{w}"]
    assert y.shape == g.shape
    err = float(np.abs(y - g).max())
    print(f"MaIRPlus(DnCNN{nb}) {h}x{w}: max-abs vs reference golden {err:.3e} (|y| max {float(np.abs(g).max()):.2f})")
    assert err <= 1e-3


@pytest.mark.parametrize("s", [2, 3])
def test_shuffle_head_in_mairplus_vs_golden(dev, plus_meta, plus_golden, s):
    """Bound: tests/test_gpu_mair_sr.py::test_conv3x3_sr_epilogues_vs_float64 (1e-4 max(1, |ref| max))."""
    h, w = plus_meta["head"]["input"]
    net = ShuffleHead(s, plus_meta["head"]["rules"]).to(dev)
    y = mair.MaIRPlus(net)(plus_input(f"head_x{s}", h, w).to(dev)).cpu().numpy()
    g = plus_golden[f"head_x{s}_{h}x{w}"]
    assert y.shape == g.shape == (1, 3, s * h, s * w)
    err = float(np.abs(y - g).max())
    print(f"MaIRPlus(shuffle head x{s}) {h}x{w}: max-abs vs reference golden {err:.3e} (|y| max {float(np.abs(g).max()):.2f})")
    assert err <= 1e-4 * max(1.0, float(np.abs(g).max()))


@pytest.mark.parametrize("name", ["light_x2", "classic_x2", "cdn"])
def test_mair_in_mairplus_vs_golden(dev, plus_meta, plus_golden, name):
    """Bound: tests/test_gpu_mair_sr.py::test_mair_sr_vs_golden and tests/test_gpu_mair.py::test_mair_flat_vs_golden
    (1e-3).  12 x 20: the transposing variants run 20 x 12 forwards."""
    cfg = plus_meta["mair_configs"][name]
    model = mair.MaIRPlus(mair.MaIR(**cfg).load_synthetic(42).eval().to(dev))
    s = model.upscale
    for h, w in plus_meta["mair_inputs"]:
        y = model(plus_input(name, h, w).to(dev)).cpu().numpy()
        g = plus_golden[f"mair_{name}_{h}x{w}"]
        assert y.shape == g.shape == (1, 3, s * h, s * w)
        err = float(np.abs(y - g).max())
        print(f"MaIRPlus(MaIR {name}) {h}x{w}: max-abs vs reference golden {err:.3e} (|y| max {float(np.abs(g).max()):.2f})")
        assert err <= 1e-3


# --------------------------------------------------------------------------- 4. batch, graph, public surface
def test_batch_independence(dev):
    net = dncnn.DnCNN(3, 3, 64, 5, "R").load_synthetic(42).eval().to(dev)
    model = mair.MaIRPlus(net)
    x = rnd("batch", (2, 3, 210, 230), 0.0, 1.0).to(dev)
    y2 = model(x).clone()
    assert torch.equal(model(x[:1]), y2[:1]) and torch.equal(model(x[1:]), y2[1:])
    assert torch.equal(model(x), y2)                                 # and deterministic


@pytest.mark.parametrize("family", ["dncnn", "mair"])
def test_graph_replay_equals_eager(dev, plus_meta, family, monkeypatch):
    monkeypatch.delenv("IRM_NO_GRAPH", raising=False)
    if family == "dncnn":
        net, shape = dncnn.DnCNN(3, 3, 64, 5, "R").load_synthetic(42).eval().to(dev), (1, 3, 210, 230)
    else:
        net, shape = mair.MaIR(**plus_meta["mair_configs"]["light_x2"]).load_synthetic(42).eval().to(dev), (2, 3, 24, 40)
    model = mair.MaIRPlus(net)
    assert model.hip_graph
    x1, x2 = rnd("g1", shape, 0.0, 1.0).to(dev), rnd("g2", shape, 0.0, 1.0).to(dev)
    e1, e2 = model(x1).clone(), model(x2).clone()
    assert not torch.equal(e1, e2)
    assert torch.equal(utils.graphed_forward(model, x1), e1)          # warm-up + capture + first replay
    assert "_irm_graphs" in model.__dict__ and len(model.__dict__["_irm_graphs"]) == 1
    assert torch.equal(utils.graphed_forward(model, x2), e2)          # replay with new input
    assert torch.equal(utils.graphed_forward(model, x1), e1)
    assert torch.equal(model(x2), e2)                                 # eager still works beside the graph


def test_get_model_prediction_through_mairplus(dev, plus_meta):
    """The tiled public call (device tiler, graphs, scaled blend) against the per-tile host loop, both through the
    wrapper: every byte within 1 LSB."""
    model = mair.MaIRPlus(mair.MaIR(**plus_meta["mair_configs"]["light_x2"]).load_synthetic(42).eval().to(dev))
    h, w, ps, ov = 50, 76, 32, 8
    lr = (synth.uniform(9, "mair_plus_lr_frame", (h, w, 3), 0.0, 1.0).numpy() * 255).astype(np.uint8)
    pred, _ = utils.get_model_prediction(model, lr, dev, ps, ov)
    assert pred.shape == (2 * h, 2 * w, 3) and pred.dtype == np.uint8
    with torch.no_grad():
        host = utils._run_tiles_on_host(model, lr, dev, utils.normalize, ps, ov, False, None, utils.pad, None)
    diff = np.abs(pred.astype(np.int32) - host.astype(np.int32))
    print(f"MaIRPlus tiled x2: {h}x{w} -> {pred.shape}, max diff {int(diff.max())}, share {float((diff > 0).mean()):.2e}")
    assert int(diff.max()) <= 1
    plain, _ = utils.get_model_prediction(model.net, lr, dev, ps, ov)
    assert not np.array_equal(plain, pred)                           # the ensemble is not a no-op


def test_admissibility(dev):
    net = restormer.Restormer(LayerNorm_type="WithBias").load_synthetic(42).eval().to(dev)
    with pytest.raises(ValueError, match="multiples of 8"):
        ensemble.SelfEnsemble(net, chop=True)(torch.zeros(1, 3, 232, 232, device=dev))      # partitions of 127
    x = rnd("adm", (1, 3, 64, 72), 0.0, 1.0).to(dev)
    y = ensemble.SelfEnsemble(net, chop=False)(x)
    want = torch.stack([ensemble.deaugment(net(ensemble.augment(x, v).contiguous()), v) for v in range(8)]).mean(0)
    assert y.shape == x.shape and float((y - want).abs().max()) <= 1e-4
    assert float((y - net(x)).abs().max()) > 1e-4
