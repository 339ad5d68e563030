"""NIQE on the GPU: irm_niqe_features against the float64 host restatement and the reference's golden scores, bit
reproducibility (runs, K, channel order, crop), the NaN block, and harness.evaluate_blind."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from frame_checks import NIQE_MARGIN as MARGIN
from frame_checks import check_against_host, up
from irm_amd import _hip, dncnn, harness, utils

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("synth_crop0", "synth_crop4", "noise", "grey", "u16")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "niqe.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def params():
    return utils.load_niqe_params(os.path.join(GOLDEN, "niqe_pris_params.npz"))


def bits(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("case", CASES)
def test_device_features_vs_host_and_reference(golden, meta, params, dev, case):
    g, info = golden("niqe"), meta["cases"][case]
    frame, crop = g[f"frame_{info['frame']}"], info["crop_border"]
    feat = utils.niqe_features_device(up(frame, dev), crop, params, channel_order="bgr")
    assert feat.shape == (1, info["blocks"], 36) and feat.dtype == torch.float64 and feat.is_cuda
    _, ds = check_against_host(feat[0].cpu().numpy(), frame, crop, params, meta, case)
    score = utils.calculate_niqe_device(up(frame, dev), crop, params, channel_order="bgr")
    assert isinstance(score, float) and score == ds
    # against the reference's golden score: the host restatement's bound plus the device bound
    limit = MARGIN * (meta["host_vs_reference"]["score_rel"] + meta["device_vs_host"]["score_rel"])
    srel = abs(score - info["score"]) / abs(info["score"])
    print(f"{case}: device NIQE {score:.9f}, reference {info['score']:.9f} ({srel:.3e}, limit {limit:.3e})")
    assert srel <= limit


def stack3(frame):
    return np.ascontiguousarray(np.stack([frame, frame[::-1], frame[:, ::-1]]))


def test_stack_of_three_and_bit_identity(golden, meta, params, dev):
    """K = 3 stacked frames against the host; two runs give the same bytes; frame 0 alone equals frame 0 of the K = 3
    call; a list equals the stack; an RGB frame equals its channel-reversed copy read as BGR."""
    frame = golden("niqe")["frame_synth"]
    stack = stack3(frame)
    feat = utils.niqe_features_device(up(stack, dev), 0, params, channel_order="bgr")
    assert feat.shape == (3, 6, 36)
    host_feat = feat.cpu().numpy()
    for i in range(3):
        check_against_host(host_feat[i], stack[i], 0, params, meta, f"stack3[{i}]")
    again = utils.niqe_features_device(up(stack, dev), 0, params, channel_order="bgr")
    assert np.array_equal(bits(feat), bits(again))
    alone = utils.niqe_features_device(up(frame, dev), 0, params, channel_order="bgr")
    assert np.array_equal(bits(alone[0]), bits(feat[0]))
    listed = utils.niqe_features_device([up(f, dev) for f in stack], 0, params, channel_order="bgr")
    assert np.array_equal(bits(listed), bits(feat))
    rgb = utils.niqe_features_device(up(np.ascontiguousarray(frame[..., ::-1]), dev), 0, params, channel_order="rgb")
    assert np.array_equal(bits(rgb[0]), bits(feat[0]))
    scores = utils.calculate_niqe_device(up(stack, dev), 0, params, channel_order="bgr")
    assert isinstance(scores, list) and len(scores) == 3
    assert scores == [utils.niqe_score(f, params) for f in host_feat]


@pytest.mark.parametrize("key", ["synth", "u16", "grey"])
def test_crop_and_nearest_border_are_bitwise(golden, params, dev, key):
    """A frame whose outer 4 pixels are garbage gives, with crop_border 4, bitwise the features of the inner frame
    with crop 0: the border repeated by the window is that of the cropped plane."""
    inner = golden("niqe")[f"frame_{key}"]
    rng = np.random.default_rng(3)
    peak = 255 if inner.dtype == np.uint8 else 65535
    outer = rng.integers(0, peak + 1, size=(inner.shape[0] + 8, inner.shape[1] + 8) + inner.shape[2:]).astype(inner.dtype)
    outer[4:-4, 4:-4] = inner
    a = utils.niqe_features_device(up(outer, dev), 4, params)
    b = utils.niqe_features_device(up(inner, dev), 0, params)
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_roll_wraps_inside_the_block_on_the_device(params, dev):
    """Two grey frames that share block 0 and the three columns its window reaches, and differ wildly beyond, give
    block 0 the same scale-1 features bit for bit: the rolled partners come from inside the block."""
    rng = np.random.default_rng(5)
    calm = rng.integers(60, 200, size=(96, 99))

    def frame(seed, lo, hi):
        wild = np.random.default_rng(seed).integers(lo, hi, size=(96, 93))
        return np.concatenate([calm, wild], axis=1).astype(np.uint8)
    fa, fb = frame(1, 120, 130), frame(2, 0, 256)
    a, b = utils.niqe_features_device(up(fa, dev), 0, params), utils.niqe_features_device(up(fb, dev), 0, params)
    assert np.array_equal(bits(a[0, 0, :18]), bits(b[0, 0, :18]))
    assert not np.array_equal(bits(a[0, 1, :18]), bits(b[0, 1, :18]))
    host = utils.niqe_features(fb.astype(np.float64), params)
    got = b.cpu().numpy()[0][:1, :18]
    differing, _, rel = utils.niqe_feature_distance(np.tile(got, (1, 2)), np.tile(host[:1, :18], (1, 2)))
    assert differing == 0 and rel < 1e-9


def test_black_block_gives_nan_features_and_a_score_over_the_rest(params, meta, dev):
    """A block that is 0 throughout (MSCN identically 0) has no negative and no positive value: its fits are NaN, with
    no fault; the NaNs sit where the host restatement has them and the score is taken over the other blocks."""
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, size=(96, 384)).astype(np.uint8)
    frame[:, :104] = 0                                                        # block 0 and what its windows reach, both scales
    feat = utils.niqe_features_device(up(frame, dev), 0, params).cpu().numpy()[0]
    host = utils.niqe_features(frame.astype(np.float64), params)
    assert feat[0, 0] == 0.2 and np.isnan(feat[0, [1, 3, 4, 5, 7, 8, 9]]).all()
    assert np.array_equal(np.isnan(feat), np.isnan(host)) and not np.isnan(feat[2:]).any()
    hs, ds = check_against_host(feat, frame, 0, params, meta, "black block")
    assert np.isfinite(ds) and utils.calculate_niqe_device(up(frame, dev), 0, params) == ds


def test_evaluate_blind_through_dncnn(params, meta, dev, tmp_path):
    """harness.evaluate_blind on three 200x300 frames: NIQE is the mean of calculate_niqe on the downloaded predictions
    within the device bound, host and device scoring agree, the CSV carries the two new columns, model=None scores the
    inputs, and a loader with targets is read the same way."""
    model = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    cfg = utils.get_patch_config("denoising", "gaussian", "DnCNN")
    frames = [(inp, name) for inp, _, name in harness.synthetic_loader(3, h=200, w=300, c=3, seed_base=4100, blur=3)]
    limit = MARGIN * meta["device_vs_host"]["score_rel"]
    kw = dict(niqe_params=params, crop_border=2, task="denoising", subtask="real", dataset="synthetic", model_name="DnCNN")
    row = harness.evaluate_blind(model, iter(frames), dev, cfg, metrics="device", **kw)
    want = [utils.calculate_niqe(utils.get_model_prediction(model, inp, dev, **cfg)[0], 2, params, channel_order="rgb")
            for inp, _ in frames]
    print(f"evaluate_blind: NIQE {row['NIQE']:.9f}, host mean {np.mean(want):.9f}")
    assert abs(row["NIQE"] - np.mean(want)) <= limit * np.mean(want)
    assert abs(row["Std_NIQE"] - np.std(want)) <= limit * np.mean(want)
    assert np.isnan(row["PSNR"]) and np.isnan(row["SSIM"]) and row["Avg_Time_ms"] > 0 and row["Failed"] == []
    assert row["Model_Params"] == 668227 and row["Task"] == "Denoising"
    host_row = harness.evaluate_blind(model, iter(frames), dev, cfg, metrics="host", **kw)
    assert host_row["NIQE"] == float(np.mean(want))
    assert abs(host_row["NIQE"] - row["NIQE"]) <= limit * row["NIQE"]
    with_targets = harness.evaluate_blind(model, harness.synthetic_loader(3, h=200, w=300, c=3, seed_base=4100, blur=3),
                                          dev, cfg, metrics="device", **kw)
    assert with_targets["NIQE"] == row["NIQE"]
    before = harness.evaluate_blind(None, iter(frames), dev, cfg, metrics="device", **dict(kw, model_name="Input"))
    inputs = [utils.calculate_niqe(inp, 2, params, channel_order="rgb") for inp, _ in frames]
    assert abs(before["NIQE"] - np.mean(inputs)) <= limit * np.mean(inputs) and before["Model_Params"] == 0
    path = harness.save_results([before, row], out_dir=str(tmp_path), columns=harness.COLUMNS_BLIND)
    with open(path) as f:
        rd = list(csv.DictReader(f))
    assert list(rd[0].keys()) == harness.COLUMNS + ["NIQE", "Std_NIQE"] and len(rd) == 2
    assert abs(float(rd[1]["NIQE"]) - row["NIQE"]) < 1e-9 and abs(float(rd[1]["Std_NIQE"]) - row["Std_NIQE"]) < 1e-9
    plain = harness.save_results([row], out_dir=str(tmp_path), file_name="plain.csv")
    with open(plain) as f:
        assert list(csv.DictReader(f).fieldnames) == harness.COLUMNS
    # a frame too small for two blocks is reported, not fatal; skip_failed=False lets it through
    small = [(np.zeros((100, 150, 3), np.uint8), "small.png")] + frames[:1]
    part = harness.evaluate_blind(None, iter(small), dev, cfg, metrics="device", **kw)
    assert [n for n, _ in part["Failed"]] == ["small.png"] and np.isfinite(part["NIQE"])
    with pytest.raises(ValueError):
        harness.evaluate_blind(None, iter(small), dev, cfg, metrics="device", skip_failed=False, **kw)


def test_cpu_tensors_raise_hip_library_error(params, dev):
    u8 = torch.zeros(200, 300, 3, dtype=torch.uint8)
    with pytest.raises(_hip.HipLibraryError):
        utils.niqe_features_device(u8, 0, params)
    with pytest.raises(_hip.HipLibraryError):
        utils.calculate_niqe_device(u8, 0, params)
    with pytest.raises(_hip.HipLibraryError):
        utils.calculate_niqe_device([u8, u8], 0, params)
