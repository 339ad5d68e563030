"""The rows of harness.py, protocol by protocol, without a GPU: the predictors are replaced by deterministic fakes
(harness looks them up as module globals), scoring is the protocol's own host scorer.  Pinned for each of the seven
guarded sweeps: a frame that fails in the middle leaves no trace in any statistic, an empty loader gives a NaN row, the
columns are the documented ones, and nothing a predictor handed back outlives the sweep."""
import csv
import gc
import math
import os
import weakref

import numpy as np
import pytest
import torch

import align_cases as ac
import lpips_model as lm
from irm_amd import harness, utils, yuv
from irm_amd.align import calculate_metrics_aligned
from irm_amd.metrics import calculate_metrics, calculate_metrics_basicsr

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(patch_size=32, patch_overlap=8)
KW = dict(task="denoising", subtask="gaussian", dataset="d", model_name="m")
STATS = ['PSNR', 'SSIM', 'Std_PSNR', 'Std_SSIM', 'Avg_Time_ms', 'Std_Time_ms']

BASE = ['Task', 'Type', 'Dataset', 'Sigma', 'Model', 'Model_Params', 'PSNR', 'SSIM', 'Std_PSNR', 'Std_SSIM',
        'Avg_Time_ms', 'Std_Time_ms']
LITERALS = {
    "COLUMNS": BASE,
    "COLUMNS_BLIND": BASE + ['NIQE', 'Std_NIQE'],
    "COLUMNS_AUTO": BASE + ['Sigma_Est', 'Std_Sigma_Est', 'Sigma_Used'],
    "COLUMNS_PERCEPTUAL": BASE + ['LPIPS', 'Std_LPIPS'],
    "COLUMNS_ALIGNED": BASE + ['Rho', 'Coverage', 'Std_Rho', 'Std_Coverage'],
    "COLUMNS_YUV": BASE + ['PSNR_U', 'PSNR_V', 'SSIM_U', 'SSIM_V', 'Std_PSNR_U', 'Std_PSNR_V', 'Std_SSIM_U',
                           'Std_SSIM_V'],
}


# --------------------------------------------------------------------------- the fakes
def restore(img, grow=1):
    """The fake model: every code rounded down to an even one; `grow` repeats the pixels (a super-resolving model)."""
    if isinstance(img, tuple):
        return tuple(restore(p) for p in img)
    out = img // 2 * 2
    return out if grow == 1 else np.ascontiguousarray(np.repeat(np.repeat(out, grow, 0), grow, 1))


def ms_of(img) -> float:
    """The fake time of a frame: it depends on the frame, so a statistic over the wrong frames shows."""
    return 1.0 + float((img[0] if isinstance(img, tuple) else img).mean())


def sigma_of(img) -> float:
    return float(img[0, 0, 0])


class Kept:
    """What a fake predictor hands back in place of the device output: weak-referenceable, nothing else."""


class Fake:
    """Stands in for the three predictors harness.py calls; `bad(img)` marks the frame that raises."""

    def __init__(self, monkeypatch, bad=lambda img: False, grow=1):
        self.bad, self.grow, self.refs = bad, grow, []
        monkeypatch.setattr(harness, "_get_model_prediction", self.predict)
        monkeypatch.setattr(harness, "_run_model_inference_auto", self.auto)
        monkeypatch.setattr(harness, "_run_model_inference_yuv", self.yuv)

    def _run(self, img):
        if self.bad(img):
            raise RuntimeError("boom")
        kept = Kept()
        self.refs.append(weakref.ref(kept))
        return restore(img, self.grow), ms_of(img), kept

    def predict(self, model, img, device, patch_size, patch_overlap, need_degradation=False, noise_level=None):
        return self._run(img)

    def auto(self, bank, img, device, patch_size=None, patch_overlap=32):
        pred, ms, kept = self._run(img)
        return pred, ms, sigma_of(img), bank.pick(sigma_of(img))[0], kept

    def yuv(self, model, planes, device, *, fmt, patch_size=None, patch_overlap=32, **kw):
        return self._run(planes)

    def all_dead(self) -> bool:
        gc.collect()
        return all(r() is None for r in self.refs)


def fake_sr_pairs(hr_loader, scale, device):
    for item in hr_loader:
        yield np.ascontiguousarray(item[-2][::scale, ::scale]), item[-2], item[-1]


def module(n=2, **attrs):
    m = torch.nn.Linear(n, n)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


# --------------------------------------------------------------------------- the seven protocols
class Protocol:
    """One guarded sweep: `run(loader, **kw)` calls it with metrics="host"; `items` are three good frames and a marked
    one ("bad") in the middle; `want(good items)` is (psnr, ssim, time, {extra column: values}), each per frame,
    straight from the protocol's host scorer; `columns` names the COLUMNS list of its rows."""
    columns = "COLUMNS"
    grow = 1

    def is_bad(self, img):
        return any(img is item[0] for item in self.items if item[-1] == "bad")


def frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]


def with_bad(good, bad):
    return [good[0], bad, good[1], good[2]]


class Plain(Protocol):
    def __init__(self):
        f = frames(8, 24, 32, 1)
        self.items = with_bad([(f[2 * i], f[2 * i + 1], f"g{i}") for i in range(3)], (f[6], f[7], "bad"))

    def run(self, loader, **kw):
        return harness.evaluate(module(), loader, CPU, CFG, metrics="host", **KW, **kw)

    def want(self, good):
        ps = [calculate_metrics(restore(a), b) for a, b, _ in good]
        return [p for p, _ in ps], [s for _, s in ps], [ms_of(a) for a, _, _ in good], {}


class Auto(Plain):
    columns = "COLUMNS_AUTO"

    def __init__(self):
        super().__init__()
        for (a, _, _), sigma in zip(self.items, (60, 30, 12, 55)):       # levels 50, (25, the bad one), 15, 50
            a[0, 0, 0] = sigma
        self.bank = utils.SigmaBank({25: module(3), 50: module(4), 15: module(2)})

    def run(self, loader, **kw):
        return harness.evaluate_auto_sigma(self.bank, loader, CPU, CFG, metrics="host", **KW, **kw)

    def want(self, good):
        return super().want(good)[:3] + ({'Sigma_Est': [sigma_of(a) for a, _, _ in good]},)


class Sr(Protocol):
    grow = 2

    def __init__(self):
        f = frames(4, 48, 48, 2)
        self.items = with_bad([(f[i], f"g{i}") for i in range(3)], (f[3], "bad"))
        for hr, name in self.items:
            hr[0, 0, 0] = 251 if name == "bad" else 7

    def is_bad(self, lr):
        return lr[0, 0, 0] == 251

    def run(self, loader, **kw):
        return harness.evaluate_sr(module(upscale=2), loader, CPU, CFG, 2, metrics="host", **kw)

    def want(self, good):
        lrs = [np.ascontiguousarray(hr[::2, ::2]) for hr, _ in good]
        ps = [calculate_metrics_basicsr(restore(lr, 2), hr, 2, True, "rgb") for lr, (hr, _) in zip(lrs, good)]
        return [p for p, _ in ps], [s for _, s in ps], [ms_of(lr) for lr in lrs], {}


class Yuv(Protocol):
    columns = "COLUMNS_YUV"

    def __init__(self):
        rng = np.random.default_rng(3)

        def planes():
            return tuple(rng.integers(0, 256, s).astype(np.uint8) for s in ((16, 32), (8, 16), (8, 16)))
        self.items = with_bad([(planes(), planes(), f"g{i}") for i in range(3)], (planes(), planes(), "bad"))

    def run(self, loader, **kw):
        return harness.evaluate_yuv(module(), loader, CPU, CFG, fmt="i420", metrics="host", **KW, **kw)

    def want(self, good):
        ms = [yuv.calculate_metrics_yuv(restore(a), b, "i420", False) for a, b, _ in good]
        return ([m.psnr_y for m in ms], [m.ssim_y for m in ms], [ms_of(a) for a, _, _ in good],
                {'PSNR_U': [m.psnr_u for m in ms], 'PSNR_V': [m.psnr_v for m in ms],
                 'SSIM_U': [m.ssim_u for m in ms], 'SSIM_V': [m.ssim_v for m in ms]})


class Blind(Protocol):
    columns = "COLUMNS_BLIND"

    def __init__(self, golden, params):
        g, self.params = golden("niqe"), params
        self.items = [(g["frame_synth"], "g0"), (g["frame_noise"].copy(), "bad"),     # items with and without a target
                      (g["frame_noise"], g["frame_noise"], "g1"), (g["frame_u16"], "g2")]

    def run(self, loader, **kw):
        return harness.evaluate_blind(module(), loader, CPU, CFG, niqe_params=self.params, metrics="host", **kw)

    def want(self, good):
        nan = [float('nan')] * len(good)
        return nan, nan, [ms_of(item[0]) for item in good], {
            'NIQE': [utils.calculate_niqe(restore(item[0]), 0, self.params, channel_order="rgb") for item in good]}


class Perceptual(Protocol):
    columns = "COLUMNS_PERCEPTUAL"

    def __init__(self, params):
        self.params = params
        pairs = [lm.pairs(48, 56, np.uint8, seed=s)["blurred"] for s in range(4)]
        self.items = with_bad([(a, b, f"g{i}") for i, (a, b) in enumerate(pairs[:3])], pairs[3] + ("bad",))

    def run(self, loader, **kw):
        return harness.evaluate_perceptual(module(), loader, CPU, CFG, lpips_params=self.params, metrics="host", **kw)

    def want(self, good):
        ps = [calculate_metrics(restore(a), b) for a, b, _ in good]
        return ([p for p, _ in ps], [s for _, s in ps], [ms_of(a) for a, _, _ in good],
                {'LPIPS': [utils.calculate_lpips(restore(a), b, self.params) for a, b, _ in good]})


class Aligned(Protocol):
    columns = "COLUMNS_ALIGNED"

    def __init__(self):
        (pa, ta, _), (pb, tb, _) = ac.pair("A"), ac.pair("B")
        flip = (np.ascontiguousarray(pb[::-1]), np.ascontiguousarray(tb[::-1]))
        self.items = with_bad([(pb, tb, "g0"), (pa, ta, "g1"), flip + ("g2",)], (pb.copy(), tb, "bad"))

    def run(self, loader, **kw):
        return harness.evaluate_aligned(module(), loader, CPU, CFG, iterations=30, metrics="host", **kw)

    def want(self, good):
        ms = [calculate_metrics_aligned(restore(a), b, 30) for a, b, _ in good]
        assert all(m.ok for m in ms)
        return ([m.psnr for m in ms], [m.ssim for m in ms], [ms_of(a) for a, _, _ in good],
                {'Rho': [m.rho for m in ms], 'Coverage': [m.coverage for m in ms]})


@pytest.fixture(scope="module")
def niqe_params():
    return utils.load_niqe_params(os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz"))


@pytest.fixture(scope="module")
def lpips_params():
    return utils.lpips_params_from_state(*lm.synth_states())


@pytest.fixture(scope="module")
def protocols(golden, niqe_params, lpips_params):
    return {"evaluate": Plain(), "evaluate_auto_sigma": Auto(), "evaluate_sr": Sr(), "evaluate_yuv": Yuv(),
            "evaluate_blind": Blind(golden, niqe_params), "evaluate_perceptual": Perceptual(lpips_params),
            "evaluate_aligned": Aligned()}


GUARDED = ["evaluate", "evaluate_auto_sigma", "evaluate_sr", "evaluate_yuv", "evaluate_blind", "evaluate_perceptual",
           "evaluate_aligned"]


@pytest.fixture(params=GUARDED)
def proto(request, protocols, monkeypatch):
    p = protocols[request.param]
    p.fake = Fake(monkeypatch, p.is_bad, p.grow)
    monkeypatch.setattr(harness, "sr_pairs", fake_sr_pairs)
    return p


def same(a, b) -> bool:
    return a == b or (math.isnan(a) and math.isnan(b))


def check_statistics(row, want):
    """Every statistic of the row equals the one made directly from the per-frame values."""
    psnr, ssim, ms, extra = want
    direct = {'PSNR': np.mean(psnr), 'SSIM': np.mean(ssim), 'Std_PSNR': np.std(psnr), 'Std_SSIM': np.std(ssim),
              'Avg_Time_ms': np.mean(ms), 'Std_Time_ms': np.std(ms)}
    for col, vals in extra.items():
        direct[col], direct['Std_' + col] = np.mean(vals), np.std(vals)
    for col, value in direct.items():
        assert same(row[col], value), (col, row[col], value)
    assert direct['Std_Time_ms'] > 0


# --------------------------------------------------------------------------- 1, 5: a failed frame in the middle
def test_a_failed_frame_leaves_no_trace(proto):
    row = proto.run(iter(proto.items))
    good = [item for item in proto.items if item[-1] != "bad"]
    want = proto.want(good)
    assert set(LITERALS[proto.columns]) - set(BASE) - {'Sigma_Used'} == {c for k in want[3] for c in (k, 'Std_' + k)}
    check_statistics(row, want)
    assert row['Failed'] == [("bad", "RuntimeError: boom")]
    assert len(proto.fake.refs) == 3 and proto.fake.all_dead()           # the row is alive here and holds none of them
    if proto.columns == "COLUMNS_AUTO":
        assert list(row['Sigma_Used'].items()) == [(15, 1), (50, 2)]     # ordered by bank.levels; the bad 25 not there
        assert row['Sigma'] == 'auto' and row['Model_Params'] == 6       # the first level's model
    with pytest.raises(RuntimeError, match="boom"):
        proto.run(iter(proto.items), skip_failed=False)


# --------------------------------------------------------------------------- 2, 3: the empty loader and the columns
def test_empty_loader_and_columns(proto, tmp_path):
    row = proto.run(iter([]))
    columns = getattr(harness, proto.columns)
    assert columns == LITERALS[proto.columns]
    assert list(row)[:12] == LITERALS["COLUMNS"] and set(columns) <= set(row)
    for col in STATS + [c for c in columns[12:] if c != 'Sigma_Used']:
        assert math.isnan(row[col]), col
    assert row['Failed'] == [] and proto.fake.refs == []
    if proto.columns == "COLUMNS_AUTO":
        assert row['Sigma_Used'] == {}
    with open(harness.save_results([row], out_dir=str(tmp_path), columns=columns)) as f:
        assert list(csv.DictReader(f).fieldnames) == columns


def test_the_six_column_lists():
    for name, literal in LITERALS.items():
        assert getattr(harness, name) == literal, name


# --------------------------------------------------------------------------- 4: no partial records
def test_a_scorer_that_raises_after_the_prediction_leaves_no_trace(protocols, monkeypatch):
    """evaluate_perceptual on a 20 x 20 frame: the prediction and PSNR / SSIM succeed, LPIPS refuses the size."""
    p = protocols["evaluate_perceptual"]
    fake = Fake(monkeypatch)
    small = frames(2, 20, 20, 5)
    assert all(math.isfinite(v) for v in calculate_metrics(restore(small[0]), small[1]))
    with pytest.raises(ValueError):
        utils.calculate_lpips(restore(small[0]), small[1], p.params)
    good = [item for item in p.items if item[-1] != "bad"]
    row = p.run(iter([good[0], (small[0], small[1], "small"), good[1], good[2]]))
    check_statistics(row, p.want(good))
    assert [n for n, _ in row['Failed']] == ["small"] and row['Failed'][0][1].startswith("ValueError: ")
    assert len(fake.refs) == 4 and fake.all_dead()


# --------------------------------------------------------------------------- evaluate_stream
def test_the_stream_row_has_the_keys_of_evaluate():
    kw = dict(task="denoising", subtask="gaussian", dataset="synthetic", model_name="DnCNN")
    assert list(harness.evaluate_stream(module(), [], CPU, CFG, **kw)) == list(
        harness.evaluate(module(), [], CPU, CFG, **kw))
