"""LPIPS on the GPU: irm_lpips_pack against the numpy statement of the space-to-depth frame, irm_lpips_head against the
float64 formula, guard bands around both, the whole device call against the float64 model (tests/lpips_model.py) within
a bound measured on the float32 CPU chain, and the harness row."""
import numpy as np
import pytest
import torch

import lpips_model as lm
from guards import Guards, clean, sentinel
from irm_amd import _hip, dncnn, harness, perceptual, utils
from irm_amd.frames import to_device

pytestmark = pytest.mark.gpu

PACK_SIZES = [(31, 31), (32, 35), (33, 67), (34, 139)]
HEAD_SIZES = [(1, 1), (3, 7), (7, 34), (16, 33)]
HEAD_CHANNELS = [64, 192, 256, 384]
E2E_SIZES = [(31, 31), (47, 141), (64, 96)]


@pytest.fixture(scope="module")
def states():
    return lm.synth_states()


@pytest.fixture(scope="module")
def params(states):
    return utils.lpips_params_from_state(*states)


def z_shape(k, h, w):
    return (k, 48, lm.out_size(h) + 2, lm.out_size(w) + 2)


def pitched(img, dev, extra=5, fill=0):
    """The frame as a row-pitched view into a wider device buffer whose surplus columns hold `fill`."""
    h, w, c = img.shape
    wide = np.full((h, w + extra, c), fill, img.dtype)
    wide[:, :w] = img
    return to_device(wide, dev)[:, :w]


# --------------------------------------------------------------------------- pack
@pytest.mark.parametrize("dtype", lm.DTYPES)
@pytest.mark.parametrize("h,w", PACK_SIZES)
def test_pack_against_the_numpy_statement(dev, dtype, h, w):
    """K = 2, the second frame a row-pitched view: at most 1 float32 ulp from the float64 evaluation of raw a_c + b_c
    (one rounding on the device, the rounding of the comparison), the border and the positions past the frame exactly 0."""
    frames = [lm.random_frame(h, w, dtype, s) for s in (11, 12)]
    z = torch.full(z_shape(2, h, w), float("nan"), dtype=torch.float32, device=dev)
    perceptual.lpips_pack(to_device(frames[0], dev), z, 0)
    perceptual.lpips_pack(pitched(frames[1], dev, fill=1), z, 1)
    got = z.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), "an element of z was not written"
    for k in range(2):
        want = lm.pack_model(frames[k])
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got[k] - want) <= ulp).all()
        u = np.zeros((3, 4 * z.shape[2], 4 * z.shape[3]), bool)
        u[:, 2:2 + min(h, 4 * lm.out_size(h) + 5), 2:2 + min(w, 4 * lm.out_size(w) + 5)] = True
        inside = u.reshape(3, z.shape[2], 4, z.shape[3], 4).transpose(0, 2, 4, 1, 3).reshape(48, z.shape[2], z.shape[3])
        assert (got[k][~inside] == 0.0).all() and not (got[k][inside] == 0.0).any()


@pytest.mark.parametrize("h,w", [(34, 34), (38, 70)])
def test_pack_never_reads_what_the_stride_leaves_out(dev, h, w):
    """h, w are one more than the size the stride reaches: the last row and column, NaN here, do not appear in z."""
    assert (h - 7) % 4 == 3 and (w - 7) % 4 == 3
    img = lm.random_frame(h, w, np.float32, 5)
    img[-1], img[:, -1] = np.nan, np.nan
    z = torch.empty(z_shape(1, h, w), dtype=torch.float32, device=dev)
    perceptual.lpips_pack(to_device(img, dev), z, 0)
    got = clean(z)[0].numpy().astype(np.float64)
    want = lm.pack_model(np.nan_to_num(img, nan=0.5)[:h - 1, :w - 1])
    assert got.shape == want.shape and (np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


@pytest.mark.parametrize("dtype", lm.DTYPES)
def test_guard_bands_lpips_pack(dev, dtype):
    """K = 2 pitched frames with slack between them inside a buffer whose every other sample is poison (NaN for
    float32; for the integers two runs with different fills must agree), z between sentinels with slack between its
    blocks: nothing outside z's blocks is written, every element inside is, and no poison reaches a value."""
    h, w, K = 33, 67, 2
    frames = np.stack([lm.random_frame(h, w, dtype, s) for s in (1, 2)])
    pitch, stride = 3 * w + 8, (h - 1) * (3 * w + 8) + 3 * w + 16
    a, b = lm.affine(dtype)
    zs = z_shape(K, h, w)
    per = zs[1] * zs[2] * zs[3]

    def run(fill):
        g = Guards(dev)
        buf = np.full(4096 + (K - 1) * stride + (h - 1) * pitch + 3 * w + 4096, fill, dtype)
        for k in range(K):
            for r in range(h):
                o = 4096 + k * stride + r * pitch
                buf[o:o + 3 * w] = frames[k, r].reshape(-1)
        x = to_device(buf, dev)
        z = g.out("z", zs, slack=8)
        _hip.call("irm_lpips_pack", x.data_ptr() + 4096 * x.element_size(), lm.DTYPES.index(dtype), K, h, w, pitch,
                  stride, *[float(v) for v in a], *[float(v) for v in b], _hip.ptr(z), per + 8)
        g.check()
        assert not bool((z == sentinel(torch.float32)).any()), "an element of z was not written"
        return clean(z)

    runs = [run(np.nan)] if dtype == np.float32 else [run(0), run(np.iinfo(dtype).max)]
    assert all(torch.equal(r, runs[0]) for r in runs)
    for k in range(K):
        want = lm.pack_model(frames[k])
        assert (np.abs(runs[0][k].numpy() - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


# --------------------------------------------------------------------------- head
def head_maps(c, h, w, k, seed):
    """2k maps like a ReLU's output: about half the values zero, and a few pixels all zero."""
    gen = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(2 * k, c, h, w, generator=gen))
    if h * w > 1:
        f[:, :, 0, 0] = 0.0
    lin = torch.rand(c, generator=gen)
    return f, lin


def run_head(dev, f, lin, g=None):
    """irm_lpips_head on f [2K, C, H, W] as a batch-strided slice of a larger NaN-filled buffer, lin at the front of a
    longer NaN-filled vector; out and the workspace at exactly their sizes between sentinels."""
    g = g or Guards(dev)
    k2, c, h, w = f.shape
    k = k2 // 2
    big = torch.full((k2, c + 3, h, w), float("nan"), device=dev)
    big[:, :c] = f.to(dev)
    lin_big = torch.full((c + 5,), float("nan"), device=dev)
    lin_big[:c] = lin.to(dev)
    out = g.out("out", (k, 6), torch.float64)
    ws = g.out("ws", (k * -(-h * w // 64),), torch.float64)
    perceptual.lpips_head(big[:, :c], lin_big, out, 2, ws)
    g.check()
    col = out[:, 2].cpu()
    rest = torch.cat([out[:, :2], out[:, 3:]], 1).cpu()
    assert bool((rest == sentinel(torch.float64)).all()), "a store to another column of out"
    return col


@pytest.mark.parametrize("c", HEAD_CHANNELS)
@pytest.mark.parametrize("h,w", HEAD_SIZES)
def test_head_against_the_float64_formula(dev, c, h, w):
    f, lin = head_maps(c, h, w, 2, c + 10 * h + w)
    got = run_head(dev, f, lin)
    for k in range(2):
        want = lm.head(f[k].double(), f[2 + k].double(), lin.double())
        assert not torch.isnan(got[k]) and abs(float(got[k]) - want) <= 1e-6 * want, (k, float(got[k]), want)
    assert torch.equal(run_head(dev, f, lin).view(torch.int64), got.view(torch.int64)), "a second run differs"
    same = torch.cat([f[:2], f[:2]])
    assert run_head(dev, same, lin).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("h,w", [(1, 1), (7, 34)])
def test_head_hand_cases(dev, h, w):
    c = 64
    lin = torch.rand(c, generator=torch.Generator().manual_seed(1)) + 0.1
    f = torch.zeros(4, c, h, w)
    f[0, 1], f[2, 2] = 1.0, 1.0                        # pair 0: e_1 against e_2 at every pixel
    f[3] = torch.rand(c, h, w, generator=torch.Generator().manual_seed(2)) + 0.1   # pair 1: all-zero f against g
    got = run_head(dev, f, lin)
    assert abs(float(got[0]) - float(lin[1].double() + lin[2].double())) <= 1e-9
    g64 = f[3].double()
    want = float((lin.double().view(-1, 1, 1) * g64 ** 2 / (g64.pow(2).sum(0).sqrt() + 1e-10) ** 2).sum(0).mean())
    assert abs(float(got[1]) - want) <= 1e-6 * want


def test_guard_bands_lpips_head(dev):
    """The entry point by name: maps with slack between them and NaN around, lin inside NaN, out and the workspace at
    their minimum between sentinels."""
    k, c, h, w = 2, 192, 7, 34
    f, lin = head_maps(c, h, w, k, 3)
    g = Guards(dev)
    x = g.inp(f, slack=8)
    lv = g.inp(lin)
    out = g.out("out", (k, 1), torch.float64)
    ws = g.out("ws", (k * -(-h * w // 64),), torch.float64)
    _hip.call("irm_lpips_head", _hip.ptr(x), x.stride(0), _hip.ptr(lv), k, c, h, w, _hip.ptr(out), 1, _hip.ptr(ws),
              ws.numel())
    g.check()
    got = clean(out)[:, 0]
    for i in range(k):
        want = lm.head(f[i].double(), f[k + i].double(), lin.double())
        assert abs(float(got[i]) - want) <= 1e-6 * want


# --------------------------------------------------------------------------- end to end
def rel(got, want):
    return abs(got - want) / want


@pytest.fixture(scope="module")
def e2e(states):
    """Per case the frames, the float64 model's value and the float32 CPU chain's, computed once."""
    cases = []
    for (h, w) in E2E_SIZES:
        for dtype in lm.DTYPES:
            for name, (a, b) in lm.pairs(h, w, dtype, seed=h).items():
                want = lm.lpips(a, b, *states)[1]
                f32 = lm.lpips(a, b, *states, dtype=torch.float32)[1]
                cases.append((f"{h}x{w} {np.dtype(dtype).name} {name}", a, b, want, f32))
    return cases


def test_device_against_the_float64_model(dev, params, e2e):
    """The largest relative error of the device over the whole set is at most 8 times the largest of the float32 CPU
    chain on the same inputs; identical frames give exactly 0.0; a repeated call is bit-identical."""
    cpu_err, dev_err = 0.0, 0.0
    for name, a, b, want, f32 in e2e:
        got = utils.calculate_lpips_device(to_device(a, dev), to_device(b, dev), params)
        assert got == utils.calculate_lpips_device(to_device(a, dev), to_device(b, dev), params), name
        if name.endswith("same"):
            assert want == 0.0 and f32 == 0.0 and got == 0.0, name
            continue
        cpu_err, dev_err = max(cpu_err, rel(f32, want)), max(dev_err, rel(got, want))
    print(f"\nLPIPS end to end: float32 CPU chain max rel err {cpu_err:.3e}, device max rel err {dev_err:.3e}, "
          f"bound {8 * cpu_err:.3e}")
    assert cpu_err > 0.0
    assert dev_err <= 8 * cpu_err


def test_batch_of_three_equals_single_calls(dev, params, e2e):
    cpu_err = max(rel(f32, want) for n, _, _, want, f32 in e2e if not n.endswith("same"))
    picked = [c for c in e2e if c[0].startswith("47x141 uint8")][:3]
    preds = [to_device(c[1], dev) for c in picked]
    targets = [to_device(c[2], dev) for c in picked]
    rows = utils.frame_lpips_device(preds, targets, params)
    assert rows.shape == (3, 6) and rows.dtype == torch.float64 and rows.is_cuda
    again = utils.frame_lpips_device(preds, targets, params)
    assert torch.equal(rows.view(torch.int64), again.view(torch.int64))
    rows = rows.cpu()
    for i, c in enumerate(picked):
        single = utils.calculate_lpips_device(preds[i], targets[i], params)
        assert abs(float(rows[i, 5]) - single) <= 8 * cpu_err * single, c[0]
        assert bool((rows[i, :5] >= 0).all()) and float(rows[i, 5]) == sum(float(v) for v in rows[i, :5])


def test_pitched_frames_are_read_in_place(dev, params):
    a, b = lm.random_frame(40, 53, np.uint16, 1), lm.random_frame(40, 53, np.uint16, 2)
    want = utils.calculate_lpips_device(to_device(a, dev), to_device(b, dev), params)
    assert utils.calculate_lpips_device(pitched(a, dev, 7, 65535), pitched(b, dev, 7, 65535), params) == want


# --------------------------------------------------------------------------- harness
def test_evaluate_perceptual_device_row(dev, params, e2e):
    cpu_err = max(rel(f32, want) for n, _, _, want, f32 in e2e if not n.endswith("same"))
    model = dncnn.DnCNN(3, 3, 64, 5, "R").load_synthetic(3).eval().to(dev)
    frames = [lm.pairs(64, 96, np.uint8, seed=s)["blurred"] for s in range(3)]
    loader = [(a, b, f"f{i}") for i, (a, b) in enumerate(frames)]
    cfg = utils.get_patch_config("denoising", "gaussian", "DnCNN")
    kw = dict(task="denoising", subtask="gaussian", dataset="unit", model_name="DnCNN")
    row = harness.evaluate_perceptual(model, loader, dev, cfg, lpips_params=params, metrics="device", **kw)
    ref = harness.evaluate(model, loader, dev, cfg, metrics="device", **kw)
    for key in ("PSNR", "SSIM", "Std_PSNR", "Std_SSIM"):
        assert row[key] == ref[key], key
    assert row["Failed"] == [] and ref["Failed"] == []
    vals = []
    for a, b, _ in loader:
        pred = utils.get_model_prediction(model, a, dev, **cfg)[0]
        vals.append(utils.calculate_lpips(pred, b, params))
    print(f"\nLPIPS harness: device {row['LPIPS']!r}, host twin {np.mean(vals)!r}, bound {8 * cpu_err:.3e} relative")
    assert abs(row["LPIPS"] - np.mean(vals)) <= 8 * cpu_err * max(vals)
    assert abs(row["Std_LPIPS"] - np.std(vals)) <= 8 * cpu_err * max(vals)
