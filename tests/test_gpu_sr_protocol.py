"""The super-resolution benchmark protocol on the GPU: irm_imresize_bicubic against the float64 restatement and the
reference goldens, irm_frame_metrics_basicsr against the host restatement and the reference's PSNR / SSIM, bit
reproducibility of both, the full-size frames and harness.evaluate_sr."""
import json
import os

import numpy as np
import pytest
import torch

from frame_checks import check_quantised, check_resize, down, quantise_ref, up
from irm_amd import _hip, harness, mair, synth, utils

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("random", "synth")
#: as in tests/test_sr_protocol_cpu.py: the bounds of a float64 restatement against the reference's fp32 imresize
RESIZE_BOUND = {"down2": 1e-6, "down3": 1e-6, "down4": 1e-6, "up2": 1e-6, "up3": 1e-4, "up4": 1e-6}
SCALE = {"down2": 0.5, "down3": 1.0 / 3.0, "down4": 0.25, "up2": 2, "up3": 3, "up4": 4}


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "sr_protocol.json")) as f:
        return json.load(f)


# --------------------------------------------------------------------------- 1. resize
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("key", list(RESIZE_BOUND))
def test_imresize_device_vs_host_and_reference(dev, golden, key, name):
    g = golden("sr_protocol")
    src = g[f"hr_{name}"] if key.startswith("down") else g[f"lr4_{name}"]
    got = check_resize(src, SCALE[key], dev, f"{key} {name}")
    ref = g[f"{key}_{name}"]
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"{key} {name}: device vs reference max-abs {err:.3e}")
    assert err <= RESIZE_BOUND[key]
    q = utils.imresize_device(up(src, dev), SCALE[key])                      # out="same" is the default
    check_quantised(down(q), quantise_ref(ref), f"{key} {name} quantised vs reference")


@pytest.mark.parametrize("scale", [0.5, 1.0 / 3.0, 0.25, 2, 3, 4])
def test_imresize_device_uint16_and_grey(dev, golden, scale):
    hr = golden("sr_protocol")["hr_synth"]
    if scale > 1:
        hr = hr[:40, :52]
    rng = np.random.default_rng(5)
    u16 = (hr.astype(np.uint16) * 256 + rng.integers(0, 256, hr.shape).astype(np.uint16)).astype(np.uint16)
    check_resize(u16, scale, dev, f"uint16 x{scale:g}")
    grey = np.ascontiguousarray(hr[:, :, 1])
    got = check_resize(grey, scale, dev, f"grey HW x{scale:g}")
    got1 = check_resize(grey[:, :, None].copy(), scale, dev, f"grey HW1 x{scale:g}")
    assert got.ndim == 2 and got1.ndim == 3 and np.array_equal(got, got1[:, :, 0])
    # a grey frame is a channel of the colour frame, bit for bit
    full = utils.imresize_device(up(hr, dev), scale, out="float").cpu().numpy()
    assert np.array_equal(full[:, :, 1], got)
    check_resize(u16[:, :, 0].copy(), scale, dev, f"uint16 grey x{scale:g}")
    if hasattr(torch, "uint16"):
        t16 = up(u16, dev).view(torch.uint16)
        q = utils.imresize_device(t16, scale)
        assert q.dtype == torch.uint16
        assert np.array_equal(q.view(torch.int16).cpu().numpy(), utils.imresize_device(up(u16, dev), scale).cpu().numpy())


def test_imresize_device_clamps_when_quantising(dev):
    """Bicubic overshoot beyond [0, 1] (a black / white checker of 3-pixel squares, enlarged) is clamped."""
    yy, xx = np.mgrid[0:30, 0:36]
    img = ((((yy // 3) + (xx // 3)) % 2) * 255).astype(np.uint8)[:, :, None].repeat(3, 2)
    f = utils.imresize_device(up(img, dev), 4, out="float").cpu().numpy()
    assert f.min() < -0.05 and f.max() > 1.05
    check_resize(img, 4, dev, "checker x4")


def test_imresize_device_rejects_short_sides(dev):
    z = torch.zeros(18, 17, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        utils.imresize_device(z, 0.25)
    t = torch.zeros(4096, device=dev)
    i = torch.zeros(4096, dtype=torch.int32, device=dev)
    out = torch.zeros(4096, device=dev)
    for (h, w, c, s, shrink) in ((18, 17, 3, 4, 1), (5, 6, 3, 2, 0), (18, 18, 2, 4, 1), (18, 18, 3, 5, 1), (18, 18, 3, 1, 0)):
        with pytest.raises(_hip.HipLibraryError, match="invalid arguments"):
            _hip.call("irm_imresize_bicubic", _hip.ptr(z), 0, _hip.ptr(out), 1, _hip.ptr(t), _hip.ptr(i), _hip.ptr(t),
                      _hip.ptr(i), 1, h, w, c, s, shrink)


@pytest.mark.parametrize("scale", [0.25, 1.0 / 3.0, 3])
def test_imresize_device_bitwise_alone_and_in_a_batch(dev, golden, scale):
    g = golden("sr_protocol")
    frames = [g["hr_random"], g["deg_random"], g["hr_random"][::-1].copy(), g["hr_random"][:, ::-1].copy()]
    devf = [up(f, dev) for f in frames]
    for out in ("float", "same"):
        alone = [utils.imresize_device(devf[1], scale, out=out).cpu().numpy() for _ in range(2)]
        batch = [utils.imresize_device(devf, scale, out=out) for _ in range(2)]
        stack = utils.imresize_device(torch.stack(devf), scale, out=out)
        assert isinstance(batch[0], list) and len(batch[0]) == 4 and stack.shape[0] == 4
        for b in (alone[1], batch[0][1].cpu().numpy(), batch[1][1].cpu().numpy(), stack[1].cpu().numpy()):
            assert np.array_equal(alone[0], b)
        assert not np.array_equal(alone[0], batch[0][0].cpu().numpy())


# --------------------------------------------------------------------------- 2. metrics
def _metric_args(g, key):
    name, kind, crop, y = key.split("/")
    a, b = g[f"deg_{name}"], g[f"hr_{name}"]
    if kind == "grey":
        a, b = a[:, :, 1].copy(), b[:, :, 1].copy()
    return a, b, int(crop[4:]), bool(int(y[1:]))


def test_metrics_device_vs_host_and_reference(dev, golden, meta):
    """Against the host restatement: 1e-9 for SSIM and for PSNR in dB, the project's allowance for device metrics.
    Against the reference's own values: twice the distance the generator measured for the host restatement."""
    g = golden("sr_protocol")
    tol_p, tol_s = 2 * meta["metrics_host_vs_reference"]["psnr_db"], 2 * meta["metrics_host_vs_reference"]["ssim"]
    for key, want in meta["metrics"].items():
        a, b, crop, y = _metric_args(g, key)
        p, s = utils.calculate_metrics_basicsr_device(up(a, dev), up(b, dev), crop, y, channel_order="bgr")
        hp, hs = utils.calculate_metrics_basicsr(a, b, crop, y, channel_order="bgr")
        print(f"{key}: device PSNR {p:.9f} SSIM {s:.12f}; vs host {abs(p - hp):.2e} dB, {abs(s - hs):.2e}; "
              f"vs reference {abs(p - want['psnr']):.2e} dB, {abs(s - want['ssim']):.2e}")
        assert abs(p - hp) <= 1e-9 and abs(s - hs) <= 1e-9
        assert abs(p - want["psnr"]) <= tol_p and abs(s - want["ssim"]) <= tol_s


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("y", [False, True])
@pytest.mark.parametrize("shape,crop", [((21, 23, 3), 0), ((21, 23, 3), 5), ((64, 300, 3), 3), ((47, 215, 1), 2), ((33, 222), 0)])
def test_metrics_device_vs_host_shapes_and_uint16(dev, shape, crop, y, order):
    """Several tiles per row and column, ragged last tiles, the smallest valid frame (11 x 13 after the crop), both
    dtypes."""
    rng = np.random.default_rng(abs(hash((shape, crop))) % 1000)
    b = rng.integers(0, 256, shape).astype(np.uint8)
    a = np.clip(b.astype(np.int64) + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)
    for pa, pb in ((a, b), (a.astype(np.uint16) * 257, b.astype(np.uint16) * 256 + 7)):
        p, s = utils.calculate_metrics_basicsr_device(up(pa, dev), up(pb, dev), crop, y, channel_order=order)
        hp, hs = utils.calculate_metrics_basicsr(pa, pb, crop, y, channel_order=order)
        print(f"{shape} crop {crop} y {y} {order} {pa.dtype}: PSNR {p:.6f} SSIM {s:.9f}; vs host {abs(p - hp):.2e}, {abs(s - hs):.2e}")
        assert abs(p - hp) <= 1e-9 and abs(s - hs) <= 1e-9
    if not y:
        sse, _ = utils.frame_metrics_basicsr_device([up(a, dev)], [up(b, dev)], crop, False)
        av, bv = (x.reshape(shape[0], shape[1], -1)[crop:shape[0] - crop, crop:shape[1] - crop] for x in (a, b))
        assert sse.dtype == torch.int64 and int(sse[0]) == int(((av.astype(np.int64) - bv) ** 2).sum())


def test_metrics_device_identical_frames(dev, golden):
    b = golden("sr_protocol")["hr_synth"]
    for frame in (b, b[:, :, 1].copy(), b.astype(np.uint16) * 257):
        for y in (False, True):
            for crop in (0, 4):
                p, s = utils.calculate_metrics_basicsr_device(up(frame, dev), up(frame, dev), crop, y)
                assert p == float("inf") and s == 1.0


def test_metrics_device_rejects_small_crops(dev):
    z = torch.zeros(30, 40, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        utils.calculate_metrics_basicsr_device(z, z, 10, True)
    out = torch.zeros(64, dtype=torch.float64, device=dev)
    for (h, w, c, crop, y, bgr, words) in ((30, 40, 3, 10, 1, 0, 64), (30, 40, 2, 0, 1, 0, 64), (30, 40, 3, -1, 1, 0, 64),
                                           (30, 40, 3, 0, 2, 0, 64), (30, 40, 3, 0, 1, 2, 64), (30, 40, 3, 0, 1, 0, 3)):
        with pytest.raises(_hip.HipLibraryError, match="invalid arguments"):
            _hip.call("irm_frame_metrics_basicsr", _hip.ptr(z), _hip.ptr(z), 0, 1, h, w, c, crop, y, bgr, _hip.ptr(out),
                      _hip.ptr(out), _hip.ptr(out), words)


@pytest.mark.parametrize("y", [False, True])
def test_metrics_device_bitwise_alone_and_in_a_batch(dev, golden, y):
    g = golden("sr_protocol")
    b = g["hr_random"]
    preds = [g["deg_random"], b[::-1].copy(), b[:, ::-1].copy(), np.roll(b, 1, 0)]
    pd, td = [up(x, dev) for x in preds], [up(b, dev)] * 4
    runs = []
    for _ in range(2):
        sse1, ssim1 = utils.frame_metrics_basicsr_device([pd[2]], [td[2]], 4, y)
        sse4, ssim4 = utils.frame_metrics_basicsr_device(pd, td, 4, y)
        runs.append((sse1.view(torch.int64).cpu(), ssim1.view(torch.int64).cpu(), sse4.view(torch.int64).cpu(),
                     ssim4.view(torch.int64).cpu()))
    for r in runs:
        assert int(r[0][0]) == int(r[2][2]) and int(r[1][0]) == int(r[3][2])
        assert all(torch.equal(x, y_) for x, y_ in zip(r, runs[0]))
    assert len({int(v) for v in runs[0][3]}) == 4


# --------------------------------------------------------------------------- 3. full size
def test_full_size_resize_and_score(dev):
    _, hr = synth.synth_image_pair(0, 720, 1280, 3)
    lr_f = check_resize(hr, 0.25, dev, "720p -> 180p")
    assert lr_f.shape == (180, 320, 3)
    lr = down(utils.imresize_device(up(hr, dev), 0.25))
    back_f = check_resize(lr, 4, dev, "180p -> 720p")
    assert back_f.shape == (720, 1280, 3)
    back = utils.imresize_device(up(lr, dev), 4)
    p, s = utils.calculate_metrics_basicsr_device(back, up(hr, dev), 4, True)
    hp, hs = utils.calculate_metrics_basicsr(down(back), hr, 4, True)
    print(f"720p bicubic x4 round trip: PSNR {p:.6f} dB SSIM {s:.9f}; device vs host {abs(p - hp):.2e} dB, {abs(s - hs):.2e}")
    assert np.isfinite(p) and abs(p - hp) <= 1e-9 and abs(s - hs) <= 1e-9


# --------------------------------------------------------------------------- 4. harness
def _hr_loader(n, h=96, w=128):
    for i in range(n):
        _, tgt = synth.synth_image_pair(i, h, w, 3, seed_base=4200, blur=0)
        yield tgt, f"hr_{i}.png"


def test_sr_pairs(dev):
    _, hr = synth.synth_image_pair(1, 97, 131, 3, seed_base=4200, blur=0)
    for s in (2, 3, 4):
        (lr, hrc, name), = list(harness.sr_pairs([(hr, "a.png")], s, dev))
        assert name == "a.png" and np.array_equal(hrc, utils.mod_crop(hr, s))
        assert lr.dtype == np.uint8 and lr.shape == (hrc.shape[0] // s, hrc.shape[1] // s, 3)
        check_quantised(lr, utils.imresize_host(hrc, 1.0 / s, out="same"), f"sr_pairs x{s}")
    (lr16, hr16, _), = list(harness.sr_pairs([(hr, hr.astype(np.uint16) * 257, "b.png")], 4, dev))      # (input, target, name)
    assert lr16.dtype == np.uint16 and hr16.dtype == np.uint16 and lr16.shape == (24, 32, 3)
    check_quantised(lr16, utils.imresize_host(hr16, 0.25, out="same"), "sr_pairs uint16")


def test_evaluate_sr_model_rows(dev):
    """Light x4 MaIR with synthetic weights on two 96x128 HR frames: device and host scoring agree to 1e-9 and equal the
    per-frame protocol done by hand."""
    with open(os.path.join(GOLDEN, "mair_sr.json")) as f:
        cfg = json.load(f)["configs"]["light_x4"]
    model = mair.MaIR(**cfg).load_synthetic(42).eval().to(dev)
    pc = {"patch_size": 32, "patch_overlap": 8}
    rows = {m: harness.evaluate_sr(model, _hr_loader(2), dev, pc, 4, dataset="synthetic", model_name="MaIR light x4",
                                   metrics=m, skip_failed=False) for m in ("device", "host")}
    want = []
    for lr, hr, _ in harness.sr_pairs(_hr_loader(2), 4, dev):
        pred, _ = utils.get_model_prediction(model, lr, dev, **pc)
        want.append(utils.calculate_metrics_basicsr(pred, hr, 4, True))
    for m, row in rows.items():
        print(m, {k: row[k] for k in ("PSNR", "SSIM", "Avg_Time_ms")})
        assert row["Failed"] == [] and row["Type"] == "X4" and row["Model_Params"] == utils.get_model_total_parameters(model)
        assert np.isfinite(row["PSNR"]) and row["Avg_Time_ms"] > 0
        assert abs(row["PSNR"] - np.mean([p for p, _ in want])) <= 1e-9
        assert abs(row["SSIM"] - np.mean([q for _, q in want])) <= 1e-9
    assert abs(want[0][0] - want[1][0]) > 1e-6                     # two frames, two scores
    assert abs(rows["device"]["PSNR"] - rows["host"]["PSNR"]) <= 1e-9
    assert abs(rows["device"]["SSIM"] - rows["host"]["SSIM"]) <= 1e-9
    with pytest.raises(ValueError):
        harness.evaluate_sr(model, _hr_loader(1), dev, pc, 2)


def test_evaluate_sr_bicubic_baseline(dev, tmp_path):
    rows = [harness.evaluate_sr(None, _hr_loader(2), dev, {}, 4, metrics=m, skip_failed=False) for m in ("device", "host")]
    for row in rows:
        assert row["Failed"] == [] and row["Model"] == "Bicubic" and row["Model_Params"] == 0
        assert np.isfinite(row["PSNR"]) and 0 < row["SSIM"] < 1 and row["Avg_Time_ms"] > 0
    assert abs(rows[0]["PSNR"] - rows[1]["PSNR"]) <= 1e-9 and abs(rows[0]["SSIM"] - rows[1]["SSIM"]) <= 1e-9
    # bicubic beats nearest-neighbour upsampling of the same LR frames under the same score
    nn = []
    for lr, hr, _ in harness.sr_pairs(_hr_loader(2), 4, dev):
        nn.append(utils.calculate_metrics_basicsr(np.repeat(np.repeat(lr, 4, 0), 4, 1), hr, 4, True)[0])
    print(f"bicubic baseline PSNR {rows[0]['PSNR']:.3f} dB, nearest neighbour {np.mean(nn):.3f} dB")
    assert rows[0]["PSNR"] > np.mean(nn)
    # crop_border and the Y channel reach the score
    other = harness.evaluate_sr(None, _hr_loader(2), dev, {}, 4, crop_border=0, test_y_channel=False, skip_failed=False)
    assert abs(other["PSNR"] - rows[0]["PSNR"]) > 1e-6
    path = harness.save_results(rows, str(tmp_path))
    with open(path) as f:
        assert f.readline().strip().split(",") == harness.COLUMNS
