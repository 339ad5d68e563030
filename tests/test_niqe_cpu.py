"""NIQE on the host: the float64 restatement (utils.niqe_features / calculate_niqe) against the reference goldens
(tools/gen_golden_niqe.py), the parameter loader, the argument errors, the wrap of the roll inside a block, and the
C ABI declaration and argument checks of irm_niqe_features."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from irm_amd import _hip, harness, niqe, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PARAMS = os.path.join(GOLDEN, "niqe_pris_params.npz")
CASES = ("synth_crop0", "synth_crop4", "noise", "grey", "u16")
#: the recorded maxima get this margin: the reference sums in float32, in an order that differs across numpy builds
MARGIN = 4.0


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "niqe.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def params():
    return utils.load_niqe_params(PARAMS)


@pytest.mark.parametrize("case", CASES)
def test_host_restatement_vs_reference(golden, meta, params, case):
    """Alpha entries: at most one per frame may differ, by one grid step (the fixtures were chosen so that none does).
    Other features and the score: the distance recorded by the generator, x 4."""
    g, info = golden("niqe"), meta["cases"][case]
    frame, crop = g[f"frame_{info['frame']}"], info["crop_border"]
    assert list(frame.shape) == info["shape"] and str(frame.dtype) == info["dtype"]
    ref = g[f"features_{case}"]
    feat = utils.niqe_features(utils.niqe_plane(frame, crop, "HWC", "bgr"), params)
    assert feat.shape == ref.shape == (info["blocks"], 36) and feat.dtype == np.float64
    differing, steps, rel = utils.niqe_feature_distance(feat, ref)
    score = utils.calculate_niqe(frame, crop, params, channel_order="bgr")
    srel = abs(score - info["score"]) / abs(info["score"])
    print(f"{case}: alpha differing {differing} (max {steps:.3g} steps), features {rel:.3e}, score {score:.9f} "
          f"vs {info['score']:.9f} ({srel:.3e})")
    assert differing <= 1 and steps <= 1.0 + 1e-6
    assert rel <= MARGIN * meta["host_vs_reference"]["features_rel"]
    assert srel <= MARGIN * meta["host_vs_reference"]["score_rel"]


def test_fixture_records_are_complete(meta):
    assert set(meta["cases"]) == set(CASES) and set(meta["stand_ins"]) >= {"cv2"}
    assert all(c["host_vs_reference"]["alpha_differing"] == 0 for c in meta["cases"].values())
    assert 0 < meta["host_vs_reference"]["features_rel"] < 1e-3 and 0 < meta["host_vs_reference"]["score_rel"] < 1e-4
    assert os.path.getsize(PARAMS) == 11850


def test_layouts_and_orders_agree(golden, params):
    """HWC / CHW / HW inputs, RGB against channel-reversed BGR, and uint16 against the same values as floats."""
    frame = golden("niqe")["frame_synth"]
    want = utils.calculate_niqe(frame, 0, params)
    assert utils.calculate_niqe(np.ascontiguousarray(frame.transpose(2, 0, 1)), 0, params, input_order="CHW") == want
    assert utils.calculate_niqe(np.ascontiguousarray(frame[..., ::-1]), 0, params, channel_order="rgb") == want
    assert utils.calculate_niqe(frame.astype(np.float32), 0, params) == want
    grey = golden("niqe")["frame_grey"]
    assert utils.calculate_niqe(grey, 0, params, input_order="HW") == utils.calculate_niqe(grey[..., None], 0, params)
    u16 = golden("niqe")["frame_u16"]
    assert utils.calculate_niqe(u16, 0, params) == utils.calculate_niqe(u16.astype(np.float64) / 257.0, 0, params)


def test_roll_wraps_inside_the_block(params):
    """A plane where the neighbouring block differs wildly gives block 0 the features of block 0 alone: the rolled
    partners come from inside the block.  A one-block plane is refused, so `alone` is taken two ways: on the MSCN level
    (the block's features do not see the image it was cut from), and through niqe_features with two planes that share
    block 0 and the three columns the 7x7 window reaches, and differ wildly beyond (a roll over the whole MSCN image
    would bring the far columns into block 0's products)."""
    rng = np.random.default_rng(5)
    gam, r_gam = utils.niqe_gamma_table()
    block = rng.normal(0.0, 1.0, (96, 96))
    big = rng.normal(0.0, 500.0, (288, 288))
    big[96:192, 96:192] = block
    assert niqe._niqe_block_features(big[96:192, 96:192], gam, r_gam) == niqe._niqe_block_features(block, gam, r_gam)
    # the partners are the wrapped ones: row 0 pairs with row 95, column 0 with column 95, column 95 with column 0
    probe = np.zeros((96, 96))
    probe[0, 0], probe[95, 95], probe[0, 95], probe[95, 0], probe[95, 1] = 2.0, 3.0, 5.0, 7.0, 11.0
    prods = [probe * np.roll(probe, s, axis=(0, 1)) for s in niqe._NIQE_SHIFTS]
    assert [float(p[0, 0]) for p in prods] == [2.0 * 5.0, 2.0 * 7.0, 2.0 * 3.0, 2.0 * 11.0]
    calm = rng.normal(120.0, 10.0, (96, 99))

    def plane(seed, spread):
        wild = np.random.default_rng(seed).normal(128.0, spread, (96, 93))
        return np.concatenate([calm, wild], axis=1)
    a, b = utils.niqe_features(plane(1, 3.0), params), utils.niqe_features(plane(2, 90.0), params)
    assert np.array_equal(a[0, :18], b[0, :18]) and not np.isnan(a).any()
    assert np.abs(a[1, :18] - b[1, :18]).max() > 1e-3


def test_constant_block_gives_nan_features(params):
    """A black block (the window sums to 1 - 1e-16, so only the constant 0 leaves the MSCN identically 0): no negative
    and no positive value, so the fits are NaN (alpha = gam[0]); the score is taken over the other blocks."""
    rng = np.random.default_rng(11)
    plane = rng.normal(128.0, 20.0, (96, 384))
    plane[:, :96] = 0.0
    plane[:, 96:99] = 0.0                                                     # keep the window inside constant values
    feat = utils.niqe_features(plane, params)
    assert feat[0, 0] == 0.2 and np.isnan(feat[0, [1, 3, 4, 5, 7, 8, 9]]).all()
    assert not np.isnan(feat[2:]).any()
    assert np.isfinite(utils.niqe_score(feat, params))


def test_load_niqe_params_validates(tmp_path, params):
    assert params["mu_pris_param"].shape == (1, 36) and params["cov_pris_param"].shape == (36, 36)
    assert params["gaussian_window"].shape == (7, 7) and params["gaussian_window"].dtype == np.float64
    good = {k: v for k, v in params.items()}
    for drop in good:
        p = str(tmp_path / f"no_{drop}.npz")
        np.savez(p, **{k: v for k, v in good.items() if k != drop})
        with pytest.raises(ValueError):
            utils.load_niqe_params(p)
    for key, bad in (("mu_pris_param", np.zeros(36)), ("cov_pris_param", np.zeros((36, 35))),
                     ("gaussian_window", np.zeros((5, 5)))):
        p = str(tmp_path / f"bad_{key}.npz")
        np.savez(p, **dict(good, **{key: bad}))
        with pytest.raises(ValueError):
            utils.load_niqe_params(p)
    with pytest.raises(ValueError):
        utils.calculate_niqe(np.zeros((96, 192), np.uint8), 0, {"mu_pris_param": good["mu_pris_param"]})


def test_calculate_niqe_argument_errors(params):
    one_block = np.zeros((100, 150, 3), np.uint8)
    with pytest.raises(ValueError):
        utils.calculate_niqe(one_block, 0, params)
    with pytest.raises(ValueError):
        utils.calculate_niqe(np.zeros((200, 200, 3), np.uint8), 5, params)    # 190 x 190 after the crop: one block
    with pytest.raises(NotImplementedError):
        utils.calculate_niqe(np.zeros((200, 300, 3), np.uint8), 0, params, convert_to="gray")
    for kw in (dict(convert_to="luma"), dict(channel_order="gbr"), dict(input_order="WHC")):
        with pytest.raises(ValueError):
            utils.calculate_niqe(np.zeros((200, 300, 3), np.uint8), 0, params, **kw)
    for crop in (-1, 1.5):
        with pytest.raises(ValueError):
            utils.calculate_niqe(np.zeros((200, 300, 3), np.uint8), crop, params)
    with pytest.raises(ValueError):
        utils.calculate_niqe(np.zeros((200, 300, 2), np.uint8), 0, params)
    with pytest.raises(ValueError):
        utils.calculate_niqe(torch.zeros(200, 300, 3, dtype=torch.uint8), 0, params)


def test_device_functions_refuse_before_any_gpu_call(params):
    """Without a GPU: CPU tensors raise HipLibraryError, like every other op; the other checks come first."""
    u8 = torch.zeros(200, 300, 3, dtype=torch.uint8)
    with pytest.raises(_hip.HipLibraryError):
        utils.niqe_features_device(u8, 0, params)
    with pytest.raises(_hip.HipLibraryError):
        utils.calculate_niqe_device([u8, u8], 0, params)
    with pytest.raises(NotImplementedError):
        utils.calculate_niqe_device(u8, 0, params, convert_to="gray")
    for frames in (torch.zeros(100, 150, 3, dtype=torch.uint8), u8.float(), np.zeros((200, 300, 3), np.uint8), [],
                   torch.zeros(200, 300, 2, dtype=torch.uint8), [u8, torch.zeros(200, 301, 3, dtype=torch.uint8)]):
        with pytest.raises(ValueError):
            utils.niqe_features_device(frames, 0, params)
    with pytest.raises(ValueError):
        utils.niqe_features_device(u8, -1, params)
    with pytest.raises(ValueError):
        harness.evaluate_blind(None, iter([]), "cpu", {}, niqe_params=params, metrics="gpu")


def test_header_signature_and_library_agree_on_niqe():
    text = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M))
    name = "irm_niqe_features"
    assert name in declared and name in _hip.SIGNATURES
    body = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", text, flags=re.M | re.S).group(1)
    assert len(body.split(",")) == 13 == len(_hip.SIGNATURES[name])
    for decl, ct in zip(body.split(","), _hip.SIGNATURES[name]):
        decl = decl.strip()
        want = (ctypes.c_void_p if ("*" in decl or "irm_stream_t" in decl) else ctypes.c_long if decl.startswith("long")
                else ctypes.c_double if decl.startswith("double") else ctypes.c_int)
        assert ct is want, (name, decl)


def test_library_rejects_bad_niqe_arguments():
    """IRM_EINVAL before any launch: this machine has no GPU, so anything that reached HIP would answer otherwise."""
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    fn = getattr(_hip.load(), "irm_niqe_features")
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    #       frames u16 K  H    W    C  crop bgr window table feat words stream
    good = [p, 0, 1, 200, 300, 3, 0, 0, p, p, p, 6 * 36, None]

    def call(**kw):
        names = ["frames", "u16", "K", "H", "W", "C", "crop", "bgr", "window", "table", "feat", "words", "stream"]
        return fn(*[kw.get(n, v) for n, v in zip(names, good)])
    assert fn(*[t(0) for t in _hip.SIGNATURES["irm_niqe_features"]]) == -1
    for bad in (dict(frames=None), dict(window=None), dict(table=None), dict(feat=None),      # null pointers
                dict(K=0), dict(K=-3), dict(C=2), dict(C=4), dict(crop=-1), dict(u16=2), dict(bgr=5),
                dict(H=100, W=150),                                                            # one block
                dict(H=95, W=400),                                                             # no row of blocks
                dict(crop=5, H=200, W=200),                                                    # one block after the crop
                dict(crop=150),                                                                # nothing left
                dict(words=6 * 36 - 1),                                                        # output too small
                dict(H=0), dict(W=-1), dict(H=50000, W=50000)):
        assert call(**bad) == -1, bad
