"""irm_noise_hh_stats on the GPU against its numpy twin (utils.noise_stats): all four integers equal, on frames, on
pitched and unaligned Y planes, between guard bands; then the sigma-routed call and the harness entry on top of it."""
import math

import numpy as np
import pytest
import torch

import noise_model as nm
from guards import Guards, int_fill, intact, sentinel, sentinel_out, two_fills
from irm_amd import _hip, dncnn, harness, utils

pytestmark = pytest.mark.gpu

#: the tile of nz_hist_kernel (csrc/noise.hip): NZ_ROWS frame rows x NZ_VALS row values (pixels x channels), and the
#: workgroups per frame above which a workgroup walks more than one tile
TILE_ROWS, TILE_VALS, MAX_WG = 8, 768, 256
WS_WORDS = 4098


def two_tiles_each_way(c):
    """Two whole tiles and a partial third in each direction, with a trailing odd row and column."""
    return 2 * TILE_ROWS + 5, 2 * (TILE_VALS // c) + 37


def bits(a: np.ndarray) -> torch.Tensor:
    """A host frame as the tensor the device holds: uint16 as its int16 bit pattern."""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def twin(frames, **kw):
    return torch.from_numpy(np.stack([utils.noise_stats(f, **kw) for f in frames]))


SHAPES = [(2, 2), (3, 5), (17, 23), (64, 96), (65, 97), "tiles"]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_stats_equal_the_twin(dev, dtype, c, shape):
    """K = 3 frames of sigma 5 / 25 / 50 in one launch; HW frames for C = 1 on the even shapes, HW1 on the odd ones."""
    h, w = two_tiles_each_way(c) if shape == "tiles" else shape
    frames = [nm.noisy_frame(h, w, c, s, dtype) for s in (5, 25, 50)]
    if c == 1 and h % 2 == 0:
        frames = [f[:, :, 0] for f in frames]
    want = twin(frames)
    got = utils.noise_stats_device([bits(f).to(dev) for f in frames])
    assert got.dtype == torch.int64 and got.shape == (3, c, 4) and got.is_cuda
    assert torch.equal(got.cpu(), want)
    if min(h, w) >= 17:
        assert int(want[:, :, 0].min()) > 0 and int(want[1, 0, 1]) > 0
    no_sat = utils.noise_stats_device([bits(f).to(dev) for f in frames], exclude_saturated=False)
    assert torch.equal(no_sat.cpu(), twin(frames, exclude_saturated=False))
    # the float sigma is the twin's, bit for bit
    est = utils.estimate_noise_sigma_device([bits(f).to(dev) for f in frames])
    for e, f in zip(est, frames):
        t = utils.estimate_noise_sigma(f)
        assert e == t or (math.isnan(e) and math.isnan(t))
    one = utils.estimate_noise_sigma_device(bits(frames[1]).to(dev))
    assert isinstance(one, float) and one == est[1]


@pytest.mark.parametrize("dtype,c,h,w", [(np.uint8, 3, TILE_ROWS * (MAX_WG // 2 + 2), TILE_VALS // 3 + 2),
                                         (np.uint16, 1, TILE_ROWS * (MAX_WG // 2 + 2), TILE_VALS + 2)])
def test_more_tiles_than_workgroups(dev, dtype, c, h, w):
    """2 x 130 = 260 tiles for 256 workgroups: four of them walk a second tile."""
    assert -(-h // TILE_ROWS) * -(-(w // 2 * 2 * c) // TILE_VALS) > MAX_WG
    f = nm.noisy_frame(h, w, c, 25, dtype)
    assert torch.equal(utils.noise_stats_device(bits(f).to(dev)).cpu(), twin([f]))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_degenerate_frames(dev, dtype):
    for name, (img, kw, want) in nm.degenerate_frames(dtype).items():
        got = utils.noise_stats_device(bits(img).to(dev), **kw).cpu()
        assert got[0].tolist() == want, name
        assert torch.equal(got, twin([img], **kw)), name
    frames = nm.degenerate_frames(dtype)
    assert utils.estimate_noise_sigma_device(bits(frames["flat"][0]).to(dev)) == 0.0
    assert math.isnan(utils.estimate_noise_sigma_device(bits(frames["black"][0]).to(dev)))
    assert math.isnan(utils.estimate_noise_sigma_device(bits(frames["peak"][0]).to(dev)))


def blocks_of(ds, base=1000):
    """A 2-row uint16 frame whose blocks have exactly the values `ds`: a = base + d, b = c = e = base."""
    img = np.full((2, 2 * len(ds)), base, np.uint16)
    img[0, 0::2] = [base + d for d in ds]
    return img


def test_u16_median_at_a_coarse_bin_boundary(dev):
    """The two-level select: the median rank falls on the last value of coarse bin 0 (255), on the first of bin 1 (256),
    and the values around it lie on both sides of the boundary."""
    for ds, want in (([100, 255, 255, 256, 256, 700], [6, 255, 1, 2]),
                     ([100, 255, 256, 256, 257, 700, 60000], [7, 256, 2, 2]),
                     ([256, 255], [2, 255, 0, 1]), ([511, 512, 513], [3, 512, 1, 1]), ([64000], [1, 64000, 0, 1])):
        img = blocks_of(ds)
        got = utils.noise_stats_device(bits(img).to(dev)).cpu()
        assert got[0, 0].tolist() == want and torch.equal(got, twin([img])), ds


def test_u16_top_coarse_bin(dev):
    """A 1 / 65534 checkerboard: nothing is saturated, every d is 131066, the last of the 512 coarse bins."""
    img = np.full((10, 14, 3), 1, np.uint16)
    img[0::2, 0::2] = 65534
    img[1::2, 1::2] = 65534
    got = utils.noise_stats_device(bits(img).to(dev)).cpu()
    assert got[0].tolist() == [[35, 131066, 0, 35]] * 3 and torch.equal(got, twin([img]))
    assert 131066 >> 8 == 511


GUARD_CASES = [(np.uint8, 3, 21, 549, 8),          # an odd pitch: sample by sample
               (np.uint8, 3, 20, 560, 16),         # 16-byte pieces, three tiles a row
               (np.uint16, 1, 21, 1573, 8),        # sample by sample
               (np.uint16, 3, 12, 264, 8),         # 16-byte pieces
               (np.uint8, 1, 2, 2, 4)]


@pytest.mark.parametrize("dtype,c,h,w,slack", GUARD_CASES)
def test_guard_bands_noise_hh_stats(dev, dtype, c, h, w, slack):
    """K = 2 frames with slack between them, between bands of zeros and then of ones: the result does not depend on the
    bands.  stats and the workspace, at exactly the header's minimum, between sentinels: nothing outside them changes,
    and every element of stats is written."""
    K = 2
    frames = np.stack([nm.noisy_frame(h, w, c, s, dtype) for s in (25, 50)])
    peak = 255 if dtype == np.uint8 else 65535

    def run(fill):
        g = Guards(dev)
        x = g.inp(bits(frames), slack=slack, fill=fill)
        outs = [sentinel_out((K, c, 4), dev, torch.int64), sentinel_out((WS_WORDS * K * c,), dev, torch.int64)]
        (_, stats), (_, ws) = outs
        _hip.call("irm_noise_hh_stats", _hip.ptr(x), int(dtype == np.uint16), K, h, w, c, w * c, x.stride(0), 0, 0, peak,
                  _hip.ptr(stats), _hip.ptr(ws), WS_WORDS * K * c)
        torch.cuda.synchronize()
        assert all(intact(buf, view) for buf, view in outs), "a store outside stats or the workspace"
        assert not bool((stats == sentinel(torch.int64)).any()), "an element of stats was not written"
        return (stats.cpu(),)

    (stats,) = two_fills(run)
    assert torch.equal(stats, twin(list(frames)))


# --------------------------------------------------------------------------- Y planes
def y_plane(fmt, h, w, seed):
    """Noisy Y codes of a limited-range frame: 8 bit, or 10 bit in the upper bits of a word whose low six bits are set
    at random."""
    rng = np.random.default_rng(seed)
    top = 1023 if fmt == "p010" else 255
    yy, xx = np.mgrid[0:h, 0:w]
    y = (0.5 + 0.3 * np.sin(xx / 9) * np.cos(yy / 7)) * top + rng.normal(0, 0.08 * top, (h, w))
    y = np.clip(np.rint(y), 0, top).astype(np.uint16)
    if fmt == "p010":
        return (y << 6 | rng.integers(0, 64, (h, w))).astype(np.uint16)
    return y.astype(np.uint8)


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("h,w,pitch,off", [(22, 70, 96, 0), (22, 70, 96, 1), (18, 1600, 1616, 0), (18, 1600, 1619, 3),
                                           (2, 2, 16, 0), (2, 2, 5, 1)])
def test_y_plane_in_place(dev, fmt, h, w, pitch, off):
    """The Y plane as a view into a wider buffer: rows `pitch` samples apart (the 16-byte pieces where pitch and base
    allow them, and a last piece that is cut), or starting at an odd column (sample by sample).  What lies around the
    plane is filled twice, differently; the integers equal the twin's on the contiguous copy, limited and full range."""
    y = y_plane(fmt, h, w, 7 * h + w + off)
    shift, depth = (6, 10) if fmt == "p010" else (0, 8)
    for full in (False, True):
        sat = (0, 2 ** depth - 1) if full else (16 << (depth - 8), 235 << (depth - 8))
        want = torch.from_numpy(utils.noise_stats(y, shift=shift, sat=sat))[None]
        results = []
        for fill in (0, -1):
            flat = torch.full((h * pitch + 64,), int_fill(bits(y).dtype, fill), dtype=bits(y).dtype, device=dev)
            view = flat.as_strided((h, w), (pitch, 1), off)
            view.copy_(bits(y))
            assert view.stride(0) == pitch and (view.data_ptr() - flat.data_ptr()) == off * y.itemsize
            got = utils.noise_stats_yuv_device((view,), fmt, full_range=full)
            results.append(got.cpu())
            sig = utils.estimate_noise_sigma_yuv_device((view,), fmt, full_range=full)
            host = utils.estimate_noise_sigma_yuv((y,), fmt, full_range=full)
            assert sig == host or (math.isnan(sig) and math.isnan(host))
        assert torch.equal(results[0], want) and torch.equal(results[1], want), (fmt, full)
    if h > 2:
        assert int(want[0, 0, 0]) > 0 and int(want[0, 0, 1]) > 0


# --------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_repeatable_and_independent_of_k(dev, dtype):
    h, w = two_tiles_each_way(3)
    frames = [bits(nm.noisy_frame(h, w, 3, s, dtype)).to(dev) for s in (5, 25, 50)]
    a = utils.noise_stats_device(frames)
    b = utils.noise_stats_device(frames)
    assert torch.equal(a, b)
    singles = torch.cat([utils.noise_stats_device(f) for f in frames])
    assert torch.equal(a, singles)
    assert torch.equal(a, utils.noise_stats_device(list(reversed(frames))).flip(0))


# --------------------------------------------------------------------------- the routed call
@pytest.fixture(scope="module")
def bank(dev):
    return utils.SigmaBank({s: dncnn.DnCNN(3, 3, 64, 5, "R").load_synthetic(s).eval().to(dev) for s in (15, 25, 50)})


def test_routed_call_runs_the_model_of_the_frames_sigma(dev, bank):
    for sigma in (15, 25, 50):
        img = nm.noisy_frame(96, 128, 3, sigma)
        pred, ms, est, used = utils.run_model_inference_auto(bank, img, dev, patch_size=64, patch_overlap=16)
        assert used == sigma and est == utils.estimate_noise_sigma(img) and ms > 0
        want, _ = utils.get_model_prediction(bank.models[sigma], img, dev, 64, 16)
        assert pred.dtype == np.uint8 and pred.shape == img.shape and np.array_equal(pred, want)
        other, _ = utils.get_model_prediction(bank.models[15 if sigma != 15 else 25], img, dev, 64, 16)
        assert not np.array_equal(pred, other), "the three models must be told apart by their predictions"
    with pytest.raises(ValueError, match="NaN"):
        utils.run_model_inference_auto(bank, np.zeros((32, 32, 3), np.uint8), dev)


def test_evaluate_auto_sigma(dev, bank):
    clean = nm.noisy_frame(96, 128, 3, 0)
    loader = [(nm.noisy_frame(96, 128, 3, s), clean, f"s{s}.png") for s in (15, 25, 50)]
    rows = {m: harness.evaluate_auto_sigma(bank, iter(loader), dev, dict(patch_size=64, patch_overlap=16), task="denoising",
                                           subtask="gaussian", dataset="generator", model_name="DnCNN-5", metrics=m)
            for m in ("host", "device")}
    for row in rows.values():
        assert row["Sigma_Used"] == {15: 1, 25: 1, 50: 1} and row["Failed"] == []
        assert math.isfinite(row["PSNR"]) and math.isfinite(row["SSIM"]) and row["Sigma"] == "auto"
        ests = [utils.estimate_noise_sigma(f) for f, _, _ in loader]
        assert row["Sigma_Est"] == np.mean(ests) and row["Std_Sigma_Est"] == np.std(ests)
    assert abs(rows["host"]["PSNR"] - rows["device"]["PSNR"]) <= 1e-9
    assert abs(rows["host"]["SSIM"] - rows["device"]["SSIM"]) <= 1e-9
