"""CPU-only tests of the x8 self-ensemble's host side (irm_amd/ensemble.py): the geometry planner against the chop
shapes the reference recorded (tools/gen_golden_mair_plus.py), the exact tiling of the padded output by the partition
interiors, the device table's layout, the 'MaIR+' routing of utils and the C-ABI declarations."""
import json
import os
import re

import numpy as np
import pytest
import torch

from irm_amd import _hip, ensemble, mair, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(199, 200), (200, 200), (230, 410), (64, 210), (401, 33), (720, 1280)]


@pytest.fixture(scope="module")
def plus_meta():
    with open(os.path.join(ROOT, "tests", "golden", "mair_plus.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("h,w", SIZES)
def test_planner_rects_equal_recorded_reference_chops(plus_meta, h, w):
    recorded = plus_meta["chop_shapes"][f"{h}x{w}"]
    assert len(recorded) == 8
    for v in range(8):
        p = ensemble.plan(h, w, v)
        assert [[y1 - y0, x1 - x0] for (y0, y1, x0, x1) in p.rects] == recorded[v], (h, w, v)
        assert len(p.rects) == p.grid[0] * p.grid[1]


def test_planner_hand_checked_case():
    """230 x 410: 2 x 3 sections of 115 x 137 after a pad of (0, 1), shaves 11 and 13; the transposing variants plan
    the swapped extents: 3 x 2 and the pad on the other axis."""
    p = ensemble.plan(230, 410, 0)
    assert (p.grid, p.pad, p.split, p.shave) == ((2, 3), (0, 1), (115, 137), (11, 13))
    assert [y1 - y0 for (y0, y1, _, _) in p.rects[::3]] == [126, 126]
    assert [x1 - x0 for (_, _, x0, x1) in p.rects[:3]] == [150, 163, 150]
    t = ensemble.plan(230, 410, 5)
    assert (t.size, t.grid, t.pad, t.split) == ((410, 230), (3, 2), (1, 0), (137, 115))
    one = ensemble.plan(230, 410, 6, chop=False)
    assert one.grid == (1, 1) and one.pad == (0, 0) and one.rects == ((0, 410, 0, 230),)


@pytest.mark.parametrize("chop", [True, False])
@pytest.mark.parametrize("h,w", SIZES + [(7, 5), (1000, 201)])
def test_interiors_tile_the_padded_output_exactly_once(h, w, chop):
    for v in range(8):
        p = ensemble.plan(h, w, v, chop)
        Hp, Wp = p.size[0] + p.pad[0], p.size[1] + p.pad[1]
        assert Hp % p.grid[0] == 0 and Wp % p.grid[1] == 0
        assert p.pad[0] < p.size[0] and p.pad[1] < p.size[1]          # a reflect pad without edge repeat exists
        cover = np.zeros((Hp, Wp), np.int32)
        for (y0, y1, x0, x1), ((Y0, Y1, X0, X1), (oy, ox)) in zip(p.rects, p.interiors):
            cover[Y0:Y1, X0:X1] += 1
            assert 0 <= y0 < y1 <= Hp and 0 <= x0 < x1 <= Wp
            # the interior lies inside its partition, at the recorded offset
            assert (y0 + oy, x0 + ox) == (Y0, X0) and Y1 <= y1 and X1 <= x1
        assert cover.min() == 1 and cover.max() == 1


@pytest.mark.parametrize("B,h,w,chop", [(1, 230, 410, True), (2, 64, 210, True), (3, 37, 53, False), (1, 48, 48, False)])
def test_geometry_table_packs_equal_shapes_back_to_back(B, h, w, chop):
    g = ensemble.geometry(B, h, w, chop)
    assert g.table.shape == (8 + g.P, 8) and g.table.dtype == np.int32
    seen, end = {}, 0
    for ph, pw, n, off in g.groups:                     # groups are contiguous and in order
        assert off == end and n % B == 0
        end = off + n * ph * pw
        seen[(ph, pw)] = (off, n)
    assert end == g.total_pixels
    blocks = []
    for v in range(8):
        p = ensemble.plan(h, w, v, chop)
        nh, nw, sh, sw, vh, vw, p0 = g.table[v, :7]
        assert (nh, nw) == p.grid and (sh, sw) == p.split and (vh, vw) == p.shave
        for idx, (y0, y1, x0, x1) in enumerate(p.rects):
            e, ty, tx, ph, pw, off = g.table[8 + p0 + idx, :6]
            assert (e, ty, tx, ph, pw) == (v, y0, x0, y1 - y0, x1 - x0)
            goff, n = seen[(ph, pw)]
            assert (off - goff) % (B * ph * pw) == 0 and off + B * ph * pw <= goff + n * ph * pw
            blocks.append((off, off + B * ph * pw))
    blocks.sort()
    assert blocks[0][0] == 0 and all(a[1] == b[0] for a, b in zip(blocks, blocks[1:])) and blocks[-1][1] == g.total_pixels
    # the four plain variants share their shapes, and so do the four transposing ones
    if h != w:
        assert len(g.groups) == 2 * len({(r[1] - r[0], r[3] - r[2]) for r in ensemble.plan(h, w, 0, chop).rects})
    assert (g.max_ph, g.max_pw) == (max(s[0] for s in seen), max(s[1] for s in seen))


def test_torch_composition_round_trips_an_identity_network():
    """chop_torch / merge_torch (the data-movement oracle of the GPU tests) restate augment / one_img_test / gather:
    with an identity network the mean of the 8 stitched results is the input, at x1 and at a replicated x2."""
    x = torch.rand(2, 3, 230, 410, dtype=torch.float64)
    for chop in (True, False):
        preds = [[t.clone() for t in ensemble.chop_torch(x, v, chop)] for v in range(8)]
        assert float((ensemble.merge_torch(preds, 230, 410, 1, chop) - x).abs().max()) <= 1e-15
    up = lambda t: t.repeat_interleave(2, -2).repeat_interleave(2, -1)      # noqa: E731
    preds = [[up(t) for t in ensemble.chop_torch(x, v)] for v in range(8)]
    assert float((ensemble.merge_torch(preds, 230, 410, 2) - up(x)).abs().max()) <= 1e-15


def test_mair_plus_routing():
    for task, sub in (("denoising", "gaussian"), ("denoising", "real"), ("deblurring", "motion")):
        assert utils.get_patch_config(task, sub, "MaIR+") == utils.get_patch_config(task, sub, "MaIR")
    assert utils.get_patch_config("denoising", "gaussian", "MaIR+")["patch_size"] == 128
    assert mair.MaIRPlus in utils._PAD8_MODELS and issubclass(mair.MaIRPlus, ensemble.SelfEnsemble)


def test_mair_plus_factory_wraps_the_same_option_files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                        # no weights here: the MaIR+ route reaches the loader of MaIR
    with pytest.raises(FileNotFoundError):
        utils.get_model_instance("denoising", "gaussian", "MaIR+", torch.device("cpu"), sigma=25)
    with pytest.raises(ValueError, match="No model instance"):
        utils.get_model_instance("denoising", "gaussian", "MaIR+", torch.device("cpu"), gray=True, sigma=25)
    import yaml
    cfg = dict(upscale=2, in_chans=3, img_range=1., depths=[1], embed_dim=60, d_state=1, ssm_ratio=1.1, mlp_ratio=1.6,
               upsampler='pixelshuffledirect', scan_len=4, resi_connection='1conv', dynamic_ids=False, img_size=16,
               batch_size=1)
    net = mair.MaIR(**cfg).load_synthetic(42)
    torch.save({"params": net.state_dict()}, tmp_path / "w.pth")
    (tmp_path / "o.yml").write_text(yaml.safe_dump({"num_gpu": 0, "network_g": dict(type="MaIR", **cfg),
                                                    "path": {"pretrain_network_g": str(tmp_path / "w.pth")}}))
    plain, plus = mair.get_model(str(tmp_path / "o.yml")), mair.get_model(str(tmp_path / "o.yml"), plus=True)
    assert isinstance(plain, mair.MaIR) and isinstance(plus, mair.MaIRPlus) and isinstance(plus.net, mair.MaIR)
    assert plus.chop and not plus.training and plus.upscale == 2
    assert plus.max_tiles_per_batch == plain.max_tiles_per_batch and plus.hip_graph == plain.hip_graph
    with pytest.raises(_hip.HipLibraryError):          # no CPU fallback
        plus(torch.zeros(1, 3, 8, 8))


def test_admissibility_is_checked_on_the_host():
    from irm_amd import restormer
    net = restormer.Restormer(dim=16, num_blocks=(1, 1, 1, 1), num_refinement_blocks=1, heads=(1, 1, 1, 1))
    w = ensemble.SelfEnsemble(net, chop=True)
    with pytest.raises(ValueError, match="multiples of 8"):
        w._check_admissible(ensemble.geometry(1, 232, 232, True))           # 116 + 11 = 127
    ensemble.SelfEnsemble(net, chop=False)._check_admissible(ensemble.geometry(1, 64, 72, False))
    with pytest.raises(ValueError, match="multiples of 8"):
        ensemble.SelfEnsemble(net, chop=False)._check_admissible(ensemble.geometry(1, 64, 70, False))


def test_header_declares_both_symbols():
    text = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    names = set(re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M))
    for sym, nargs in (("irm_dihedral_chop_f32", 12), ("irm_ensemble_merge_f32", 11)):
        assert sym in names and len(_hip.SIGNATURES[sym]) == nargs
