"""The aligned scoring protocol (irm_amd/align.py, csrc/align.hip), the part that needs no GPU: the C ABI of
include/irm_hip_align.h against _hip.SIGNATURES_ALIGN, the library's argument refusals before any launch, the refusals
of the Python functions, and the float64 numpy statement on frames whose answer is known - recovery of a known
homography, identical frames, a pure integer shift, a flat frame - and the harness row made from it."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import align_cases as ac
from irm_amd import _hip, align, harness, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_align_prepare", "irm_ecc_iterate", "irm_aligned_metrics"]
CPU = torch.device("cpu")

#: 1.5 times the corner displacement measured with the statement: A 0.12487, B 0.06352 pixels
RECOVERY_BOUND = ac.RECOVERY_BOUND


def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip.load()


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_symbols():
    """include/irm_hip_align.h, included by irm_hip.h inside its extern "C" block after irm_hip_video.h, and
    _hip.SIGNATURES_ALIGN, disjoint from the other ten tables, match one to one; the library exports the symbols,
    load() binds them, and all-zero arguments return IRM_EINVAL before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_video.h"') < main.index('#include "irm_hip_align.h"') \
        < main.rindex("#ifdef __cplusplus")
    assert main.index('extern "C" {') < main.index('#include "irm_hip_align.h"')
    text = open(os.path.join(ROOT, "include", "irm_hip_align.h")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    assert text.count("ws_words >=") == 3, "the header states the workspace minimum of each entry"
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_ALIGN)
    others = (_hip.SIGNATURES, _hip.SIGNATURES_HALF, _hip.SIGNATURES_FRAMES, _hip.SIGNATURES_GRAM, _hip.SIGNATURES_YUV,
              _hip.SIGNATURES_INCEPTION, _hip.SIGNATURES_METRICS, _hip.SIGNATURES_NOISE, _hip.SIGNATURES_LPIPS,
              _hip.SIGNATURES_VIDEO)
    assert not set(_hip.SIGNATURES_ALIGN) & set().union(*others)
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b"}
    _lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_ALIGN[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_every_align_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_ALIGN: each
    symbol is called by name in a test_guard_bands_* function of tests/test_gpu_align.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_align.py")) as f:
        text = f.read()
    reached = set()
    for body in re.split(r"^def ", text, flags=re.M):
        if body.startswith("test_guard_bands_"):
            reached |= set(re.findall(r'"(irm_\w+)"', body))
    missing = sorted(set(_hip.SIGNATURES_ALIGN) - reached)
    assert not missing, f"align entry points without a guard-band case: {missing}"


def test_entries_refuse_bad_arguments_before_any_launch():
    """Each class of bad argument on its own, everything else valid.  The pointers are never followed: nothing is
    launched without a device, and a launch would return IRM_ELAUNCH, not IRM_EINVAL."""
    lib = _lib()
    h, w = 20, 70
    good = dict(pred=1 << 20, target=2 << 20, u16=1, H=h, W=w, gain=3 << 20, status=4 << 20, t=5 << 20, i=6 << 20,
                gx=7 << 20, gy=8 << 20, ws=9 << 20, map=10 << 20, rho=11 << 20, out=12 << 20, zr=13 << 20, cr=14 << 20,
                its=100, short=0)

    def prepare(**c):
        a = dict(good, **c)
        words = align.prepare_words(max(a["H"], 1), max(a["W"], 1)) + a["short"]
        return lib.irm_align_prepare(a["pred"], a["target"], a["u16"], a["H"], a["W"], a["gain"], a["status"], a["t"],
                                     a["i"], a["gx"], a["gy"], a["ws"], words, None)

    def iterate(**c):
        a = dict(good, **c)
        words = align.iterate_words(max(a["H"], 1), max(a["W"], 1)) + a["short"]
        return lib.irm_ecc_iterate(a["t"], a["i"], a["gx"], a["gy"], a["H"], a["W"], a["its"], a["map"], a["rho"],
                                   a["status"], a["ws"], words, None)

    def score(**c):
        a = dict(good, **c)
        words = align.metrics_words(max(a["H"], 11), max(a["W"], 11)) + a["short"]
        return lib.irm_aligned_metrics(a["pred"], a["target"], a["u16"], a["H"], a["W"], a["gain"], a["map"], a["out"],
                                       a["status"], a["zr"], a["cr"], a["ws"], words, None)

    assert align.prepare_words(h, w) == 2 * 2 and align.iterate_words(h, w) == 66 * 2 * 2
    assert align.metrics_words(h, w) == 6 * 1 * 2
    shared = [dict(H=10), dict(W=10), dict(H=0), dict(W=-3), dict(H=1 << 15, W=1 << 15), dict(ws=0), dict(ws=(9 << 20) + 4),
              dict(short=-1), dict(status=0 + 2)]
    for change in shared + [dict(pred=0), dict(target=0), dict(u16=2), dict(pred=(1 << 20) + 1), dict(gain=0),
                            dict(gain=(3 << 20) + 4), dict(t=0), dict(i=0), dict(gx=0), dict(gy=(8 << 20) + 2),
                            dict(status=0)]:
        assert prepare(**change) == -1, change
    for change in shared + [dict(t=0), dict(i=0), dict(gx=0), dict(gy=0), dict(its=0), dict(its=10001), dict(map=0),
                            dict(map=(10 << 20) + 4), dict(rho=0), dict(status=0), dict(t=(5 << 20) + 1)]:
        assert iterate(**change) == -1, change
    for change in shared + [dict(pred=0), dict(target=0), dict(u16=-1), dict(target=(2 << 20) + 1), dict(gain=0),
                            dict(map=0), dict(out=0), dict(out=(12 << 20) + 4), dict(zr=(13 << 20) + 2)]:
        assert score(**change) == -1, change


# --------------------------------------------------------------------------- the Python functions
def test_python_functions_refuse_bad_arguments(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library must not be called")
    monkeypatch.setattr(_hip, "call", boom)
    z8 = np.zeros((12, 12, 3), np.uint8)
    for fn in (align.calculate_metrics_aligned, align.align_to_target):
        with pytest.raises(ValueError, match="numpy"):
            fn(torch.zeros(12, 12, 3, dtype=torch.uint8), z8)
        with pytest.raises(ValueError, match="differ"):
            fn(z8, np.zeros((12, 13, 3), np.uint8))
        with pytest.raises(ValueError, match="differ"):
            fn(z8, z8.astype(np.uint16))
        with pytest.raises(ValueError, match="uint8 or uint16"):
            fn(z8.astype(np.float32), z8.astype(np.float32))
        with pytest.raises(ValueError, match="3 channels"):
            fn(z8[..., 0], z8[..., 0])
        with pytest.raises(ValueError, match="3 channels"):
            fn(z8[..., :1], z8[..., :1])
        with pytest.raises(ValueError, match="at least 11"):
            fn(z8[:10], z8[:10])
        for bad in (0, 2.5, 10001):
            with pytest.raises(ValueError, match="iterations"):
                fn(z8, z8, bad)
    t8 = torch.zeros(12, 12, 3, dtype=torch.uint8)
    for fn in (align.ecc_homography_device, align.calculate_metrics_aligned_device, align.align_to_target_device):
        with pytest.raises(ValueError, match="torch tensors"):
            fn(z8, z8)
        with pytest.raises(ValueError, match="differ"):
            fn(t8, t8[:, :11])
        with pytest.raises(ValueError, match="differ"):
            fn(t8, t8.to(torch.int16))
        with pytest.raises(ValueError, match="uint8 or uint16"):
            fn(t8.float(), t8.float())
        with pytest.raises(ValueError, match="3 channels"):
            fn(t8[..., 0], t8[..., 0])
        with pytest.raises(ValueError, match="at least 11"):
            fn(t8[:, :10], t8[:, :10])
        with pytest.raises(ValueError, match="iterations"):
            fn(t8, t8, 0)
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(t8, t8)                                            # valid CPU tensors
    for name in ("AlignedMetrics", "align_to_target", "align_to_target_device", "calculate_metrics_aligned",
                 "calculate_metrics_aligned_device", "ecc_homography_device"):
        assert getattr(utils, name) is getattr(align, name)
    assert "cv2" not in open(align.__file__).read().replace("cv2 and skimage are absent", "")


# --------------------------------------------------------------------------- the statement on known answers
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_statement_recovers_the_known_map(name):
    pred, target, truth = ac.pair(name)
    h, w = ac.CASES[name]
    off = ac.corner_displacement(np.eye(3), truth, h, w)
    assert 1.8 < off < 2.0                                          # the identity: the shift's 1.92, less the rotation's share
    assert RECOVERY_BOUND[name] < 0.25 * 1.92, "the case means nothing if the bound is not far below the identity"
    r = align.calculate_metrics_aligned(pred, target)
    got = ac.corner_displacement(r.map, truth, h, w)
    plain = utils.calculate_metrics(pred, target)
    print(f"case {name}: identity {off:.4f} px, statement {got:.5f} px, gain {r.gain:.6f}, rho {r.rho:.6f}, coverage "
          f"{r.coverage:.4f}, PSNR {r.psnr:.3f} (plain {plain[0]:.3f}), SSIM {r.ssim:.5f} (plain {plain[1]:.5f})")
    assert r.ok and got <= RECOVERY_BOUND[name], got
    assert r.coverage >= 0.9 and r.map[2, 2] == 1.0
    assert abs(r.gain - 1.0 / ac.GAIN) < 5e-3
    assert r.psnr > plain[0] + 15.0 and r.ssim > plain[1], "the aligned scores are far above the plain ones"


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_identical_frames_are_exact(dtype):
    target = ac.pair("B")[1]
    x = target if dtype == np.uint8 else target.astype(np.uint16) * 257
    zr, cr, r = align.align_to_target(x, x)
    assert (r.psnr, r.ssim) == (float("inf"), 1.0) and r.ok
    assert abs(r.rho - 1.0) <= 1e-12 and r.coverage == 1.0 and r.gain == 1.0
    assert np.abs(r.map - np.eye(3)).max() <= 1e-14
    peak = 255.0 if dtype == np.uint8 else 65535.0
    assert bool(cr.all()) and np.array_equal(zr, (x / peak).astype(np.float32))


@pytest.mark.parametrize("dx,dy", [(3, 0), (-2, 5), (0, -4), (7, 7)])
def test_integer_shift_with_a_hand_made_map(dx, dy):
    """A target pixel (x, y) reads the prediction at (x + dx, y + dy): every phase is 0, the bicubic weights are
    (0, 1, 0, 0), zr is the scaled prediction shifted, and the mask holds (W - |dx|) (H - |dy|) pixels."""
    target = ac.pair("B")[1]
    h, w = target.shape[:2]
    pred = np.roll(target, (dy, dx), axis=(0, 1))
    zr, cr, r = align.align_to_target(pred, target, m=ac.shift_map(dx, dy))
    assert int(cr.sum()) == (w - abs(dx)) * (h - abs(dy)) and r.coverage == cr.sum() / (h * w)
    ys, xs = np.nonzero(cr)
    assert ys.min() == max(0, -dy) and ys.max() == h - 1 - max(0, dy) and xs.min() == max(0, -dx)
    want = (r.gain * (pred.astype(np.float64) / 255.0)).astype(np.float32)
    assert np.array_equal(zr[ys, xs], want[ys + dy, xs + dx]) and not zr[cr == 0].any()
    # under the mask the prediction is the target: the error is the gain's, which the wrapped border moves off 1
    assert np.array_equal(pred[ys + dy, xs + dx], target[ys, xs]) and math.isnan(r.rho) and r.ok


def test_flat_and_black_frames_fail_without_raising():
    target = ac.pair("B")[1]
    flat = np.full_like(target, 90)
    r = align.calculate_metrics_aligned(flat, target)
    assert not r.ok and np.array_equal(r.map, np.eye(3)) and r.coverage == 1.0 and r.gain > 0
    r = align.calculate_metrics_aligned(np.zeros_like(target), target)
    assert not r.ok and r.gain == 0.0
    r = align.align_to_target(target, target, m=ac.shift_map(500, 0))[2]          # nothing of the frame is left
    assert not r.ok and r.coverage == 0.0 and math.isnan(r.psnr)


def test_sums_hook_and_one_round_algebra():
    """One round at the true map: dp from the one-pass sums equals dp from explicitly zero-meaned planes and a dense
    solve, to the accuracy the Hessian's condition number leaves."""
    pred, target, truth = ac.pair("B")
    g, _ = align.gain_of(pred, target)
    planes = align.planes_of(pred, target, g)
    terms = align.ecc_terms(planes, truth)
    s = terms.sum(axis=0)
    assert terms.shape[1] == align.N_SUMS == 66 and s[0] == terms.shape[0]
    dp, rho = align.ecc_update(s)
    i, t, jac = terms[:, 1], terms[:, 2], terms[:, 58:66]
    izm, tzm = i - i.mean(), t - t.mean()
    hm = jac.T @ jac
    assert np.allclose(hm, align.hessian_of(s), rtol=1e-12)
    bi, bt = jac.T @ izm, jac.T @ tzm
    hi = np.linalg.solve(hm, bi)
    lam = (izm @ izm - bi @ hi) / (tzm @ izm - bt @ hi)
    want = np.linalg.solve(hm, lam * bt - bi)
    cond = np.linalg.cond(hm)
    assert np.abs(dp - want).max() <= 1e-15 * cond * np.abs(want).max() + 1e-18
    assert abs(rho - (izm @ tzm) / math.sqrt((izm @ izm) * (tzm @ tzm))) <= 1e-12
    seen = []
    align.ecc_iterate(planes, 3, sums_hook=lambda v, it: (seen.append(it), v)[1])
    assert seen == [0, 1, 2]


# --------------------------------------------------------------------------- the harness row
def test_evaluate_aligned_host_row_without_a_model():
    """model=None, metrics="host": the "before" row needs no GPU.  A flat frame lands in Failed."""
    pred, target, _ = ac.pair("B")
    flat = np.full_like(target, 90)
    pred_a, target_a, _ = ac.pair("A")
    loader = [(pred, target, "b0"), (flat, target, "flat"), (pred_a, target_a, "a0")]
    row = harness.evaluate_aligned(None, loader, CPU, {}, metrics="host", iterations=30)
    assert set(harness.COLUMNS_ALIGNED) <= set(row) and harness.COLUMNS_ALIGNED[:12] == harness.COLUMNS
    assert harness.COLUMNS_ALIGNED[12:] == ['Rho', 'Coverage', 'Std_Rho', 'Std_Coverage']
    assert [n for n, _ in row['Failed']] == ["flat"] and "alignment failed" in row['Failed'][0][1]
    assert row['Model'] == "Input" and row['Model_Params'] == 0 and row['Avg_Time_ms'] == 0.0
    a, b = align.calculate_metrics_aligned(pred, target, 30), align.calculate_metrics_aligned(pred_a, target_a, 30)
    assert row['PSNR'] == np.mean([a.psnr, b.psnr]) and row['Std_PSNR'] == np.std([a.psnr, b.psnr])
    assert row['SSIM'] == np.mean([a.ssim, b.ssim]) and row['Rho'] == np.mean([a.rho, b.rho])
    assert row['Coverage'] == np.mean([a.coverage, b.coverage]) and row['Std_Coverage'] == np.std([a.coverage, b.coverage])
    with pytest.raises(ValueError, match="metrics"):
        harness.evaluate_aligned(None, loader, CPU, {}, metrics="gpu")
    with pytest.raises(ValueError, match="alignment failed"):
        harness.evaluate_aligned(None, loader, CPU, {}, metrics="host", iterations=5, skip_failed=False)
