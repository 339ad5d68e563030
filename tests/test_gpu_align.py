"""The aligned scoring protocol on the GPU (csrc/align.hip, include/irm_hip_align.h) against its float64 numpy statement
(irm_amd/align.py) on the two cases of tests/align_cases.py: one round of the iteration from a given map, the warp and
its scores for a given map, the whole protocol, identical frames, reproducibility, the three entry points between guard
bands, and the harness row.

Bounds.  A float64 sum of N terms, in any order, is within N 2^-52 sum|terms| of the exact one; the device and the
statement add the same terms (positions, masks and phases agree bit for bit: every operation is rounded separately, in
one stated order), so that is the bound on each sum, N = H W (3 H W for the squared error).  It is derived, not
measured; what the whole protocol may differ by is measured on the CPU (align_cases.CORNER_TOL, RHO_TOL)."""
import math

import numpy as np
import pytest
import torch

import align_cases as ac
from guards import Guards, clean, sentinel, two_fills
from irm_amd import _hip, align, dncnn, harness

pytestmark = pytest.mark.gpu
U = 2.0 ** -52
_STATEMENT = {}


def statement(name):
    """The statement's result on a case, once: (AlignedMetrics, planes, zr, cr)."""
    if name not in _STATEMENT:
        pred, target, _ = ac.pair(name)
        zr, cr, r = align.align_to_target(pred, target)
        planes = align.planes_of(pred, target, r.gain)
        for a in (zr, cr) + planes:
            a.setflags(write=False)
        _STATEMENT[name] = (r, planes, zr, cr)
    return _STATEMENT[name]


def maps_of(name):
    h, w = ac.CASES[name]
    return {"identity": np.eye(3), "truth": ac.pair(name)[2].copy(), "shift": ac.shift_map(3, -2),
            "outside": ac.outside_map(h, w)}


def up(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                  # a copy: the shared cases are read-only


def f64(values, dev):
    return torch.tensor(np.asarray(values, dtype=np.float64).reshape(-1), dtype=torch.float64, device=dev)


def psnr_ssim_tol(h, w):
    """What the final sums leave: PSNR = 10 log10(3 n / sse) with sse a sum of 3 H W non-negative terms, so
    |dPSNR| <= 10 / ln 10 x 3 H W 2^-52; each SSIM numerator is a sum of at most H W terms of magnitude at most 1 over an
    exact count, |dSSIM| <= H W 2^-52 x mean|term| <= H W 2^-52.  The measured share (a changed map) is 0: see
    align_cases.CORNER_TOL."""
    return 10.0 / math.log(10.0) * 3 * h * w * U, h * w * U


# --------------------------------------------------------------------------- 1. one round from a given map
def dp_bound(s, e, dp):
    """First-order bound, per component, on the change of dp when sum k changes by at most e[k].  The Jacobian's columns
    differ in scale by the frame size squared, so the system is taken in the scaled unknowns y = dp / d,
    d = diag(H)^-1/2 (Jacobi scaling: the Hessian gets a unit diagonal, and its condition number - the one printed -
    is what the data leave).  There H y = r, r = lambda bT - bI: |dy| <= |H^-1| (|dr| + |dH| |y|), with the changes of
    bI, bT, hi = H^-1 bI, lambda_n, lambda_d and lambda followed term by term.  The factor 2 at the end covers the
    second-order terms and the rounding of the 8 x 8 solve itself (8 2^-52 |H|, far below H W 2^-52 |H|).  Returns
    (bound [8], condition number of the scaled Hessian, bound on rho)."""
    d = 1.0 / np.sqrt(np.diag(align.hessian_of(s)))
    s, e = s.copy(), e.copy()
    for k, (i, j) in enumerate(align._IU):
        s[6 + k] *= d[i] * d[j]
        e[6 + k] *= d[i] * d[j]
    for base in (42, 50, 58):
        s[base:base + 8] *= d
        e[base:base + 8] *= d
    y = dp / d
    n = s[0]
    mi, mt = s[1] / n, s[2] / n
    hm, eh = align.hessian_of(s), align.hessian_of(e)
    cond = np.linalg.cond(hm)
    inv_norm = cond / np.linalg.norm(hm, 2)
    eh_f = np.linalg.norm(eh)
    ji, jt, j1 = s[42:50], s[50:58], s[58:66]
    bi, bt = ji - mi * j1, jt - mt * j1
    ebi = np.linalg.norm(e[42:50] + abs(mi) * e[58:66] + np.abs(j1) * e[1] / n)
    ebt = np.linalg.norm(e[50:58] + abs(mt) * e[58:66] + np.abs(j1) * e[2] / n)
    hi = np.linalg.solve(hm, bi)
    ehi = inv_norm * (ebi + eh_f * np.linalg.norm(hi))
    ni2, nt2, corr = s[3] - mi * s[1], s[4] - mt * s[2], s[5] - mi * s[2]
    eni2, ent2 = e[3] + 2 * abs(mi) * e[1], e[4] + 2 * abs(mt) * e[2]
    ecorr = e[5] + abs(mi) * e[2] + abs(mt) * e[1]
    nbi, nbt, nhi = np.linalg.norm(bi), np.linalg.norm(bt), np.linalg.norm(hi)
    ln, ld = ni2 - bi @ hi, corr - bt @ hi
    eln = eni2 + ebi * nhi + nbi * ehi
    eld = ecorr + ebt * nhi + nbt * ehi
    lam = ln / ld
    elam = (eln + abs(lam) * eld) / abs(ld)
    er = elam * nbt + abs(lam) * ebt + ebi
    rho = corr / math.sqrt(ni2 * nt2)
    erho = 2.0 * abs(rho) * (ecorr / abs(corr) + 0.5 * eni2 / ni2 + 0.5 * ent2 / nt2)
    return d * (2.0 * inv_norm * (er + eh_f * np.linalg.norm(y))), cond, erho


@pytest.mark.parametrize("which", ["identity", "truth"])
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_one_round_from_a_given_map(dev, name, which):
    pred, target, _ = ac.pair(name)
    h, w = ac.CASES[name]
    r, planes, _, _ = statement(name)
    m0 = maps_of(name)[which]
    # the device's own planes: bit for bit the statement's
    dplanes = torch.empty(4, h, w, dtype=torch.float32, device=dev)
    gain, status = torch.zeros(1, dtype=torch.float64, device=dev), torch.full((1,), 7, dtype=torch.int32, device=dev)
    ws = torch.zeros(max(align.prepare_words(h, w), align.iterate_words(h, w)), dtype=torch.float64, device=dev)
    p_dev, t_dev = up(pred, dev), up(target, dev)
    _hip.call("irm_align_prepare", _hip.ptr(p_dev), _hip.ptr(t_dev), 0, h, w, _hip.ptr(gain),
              _hip.ptr(status), *(_hip.ptr(dplanes[k]) for k in range(4)), _hip.ptr(ws), ws.numel())
    assert float(gain.cpu()[0]) == r.gain and int(status.cpu()[0]) == 0
    got_planes = dplanes.cpu().numpy()
    for k, label in enumerate(("T", "I", "Gx", "Gy")):
        assert np.array_equal(got_planes[k].view(np.uint32), planes[k].view(np.uint32)), \
            f"plane {label}: {int((got_planes[k] != planes[k]).sum())} of {h * w} values differ from the statement"
    dmap, rho = f64(m0, dev), torch.full((1,), -1.0, dtype=torch.float64, device=dev)
    _hip.call("irm_ecc_iterate", *(_hip.ptr(dplanes[k]) for k in range(4)), h, w, 1, _hip.ptr(dmap), _hip.ptr(rho),
              _hip.ptr(status), _hip.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0
    blocks = align.iterate_words(h, w) // align.N_SUMS
    got = ws.cpu().numpy()[:blocks * align.N_SUMS].reshape(blocks, align.N_SUMS).sum(axis=0)
    terms = align.ecc_terms(planes, m0)
    want, bound = terms.sum(axis=0), h * w * U * np.abs(terms).sum(axis=0)
    worst = float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300)))
    print(f"{name} {which}: n {int(want[0])}, largest |sum difference| / bound {worst:.3e}")
    assert got[0] == want[0] and (np.abs(got - want) <= bound).all(), np.nonzero(np.abs(got - want) > bound)
    dp, rho_want = align.ecc_update(want)
    after = dmap.cpu().numpy().reshape(3, 3)
    got_dp = np.array([after[i, j] - m0[i, j] for i, j in align._DP_AT])
    tol, cond, rho_tol = dp_bound(want, bound, dp)
    tol = tol + U * np.abs(m0).max()                                    # the rounding of M + dp and of the difference here
    print(f"{name} {which}: cond(H) {np.linalg.cond(align.hessian_of(want)):.3e}, scaled {cond:.3e}; dp {dp}, "
          f"|dp difference| {np.abs(got_dp - dp)}, bound {tol}; drho {abs(float(rho.cpu()[0]) - rho_want):.3e} ({rho_tol:.3e})")
    assert (np.abs(got_dp - dp) <= tol).all()
    assert after[2, 2] == 1.0 and abs(float(rho.cpu()[0]) - rho_want) <= rho_tol


# --------------------------------------------------------------------------- 2. the warp and its scores for a given map
@pytest.mark.parametrize("which", ["identity", "truth", "shift", "outside"])
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_aligned_metrics_for_a_given_map(dev, name, which):
    pred, target, _ = ac.pair(name)
    h, w = ac.CASES[name]
    gain = statement(name)[0].gain
    m = maps_of(name)[which]
    zr_want, cr_want = align.warp_to_target(pred, gain, m)
    want, mags = align.masked_sums(target, zr_want, cr_want, terms=True)
    out = torch.zeros(9, dtype=torch.float64, device=dev)
    zr = torch.empty(h, w, 3, dtype=torch.float32, device=dev)
    cr = torch.empty(h, w, dtype=torch.uint8, device=dev)
    ws = torch.zeros(align.metrics_words(h, w), dtype=torch.float64, device=dev)
    p_dev, t_dev, g_dev, m_dev = up(pred, dev), up(target, dev), f64([gain], dev), f64(m, dev)
    _hip.call("irm_aligned_metrics", _hip.ptr(p_dev), _hip.ptr(t_dev), 0, h, w, _hip.ptr(g_dev),
              _hip.ptr(m_dev), _hip.ptr(out), None, _hip.ptr(zr), _hip.ptr(cr), _hip.ptr(ws), ws.numel())
    got, got_cr, got_zr = out.cpu().numpy(), cr.cpu().numpy(), zr.cpu().numpy()
    assert np.array_equal(got_cr, cr_want.astype(np.uint8)), f"{int((got_cr != cr_want).sum())} mask bits differ"
    if which == "outside":
        assert 0.55 < got[8] < 0.75, "about a third of the frame lies outside"
    zr_err = float(np.abs(got_zr.astype(np.float64) - zr_want).max())
    print(f"{name} {which}: coverage {got[8]:.4f}, max |zr difference| {zr_err:.3e}, sums {got[:5]} want {want[:5]}")
    assert zr_err <= 1e-6
    assert got[1] == want[1] and np.array_equal(got[5:8], want[5:8]) and got[8] == want[8]
    assert abs(got[0] - want[0]) <= 3 * h * w * U * mags[0]
    for c in range(3):
        assert abs(got[2 + c] - want[2 + c]) <= h * w * U * mags[2 + c], c
    if which == "shift":
        assert int(got[1]) == (w - 3) * (h - 2)


# --------------------------------------------------------------------------- 3. the whole protocol
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_whole_protocol_against_the_statement(dev, name):
    pred, target, truth = ac.pair(name)
    h, w = ac.CASES[name]
    want, _, zr_want, cr_want = statement(name)
    zr, cr, got = align.align_to_target_device(up(pred, dev), up(target, dev))
    off = ac.corner_displacement(got.map, want.map, h, w)
    tp, ts = psnr_ssim_tol(h, w)
    print(f"{name}: corner displacement from the statement {off:.3e} px (tolerance {ac.CORNER_TOL[name]:.3e}), "
          f"dPSNR {abs(got.psnr - want.psnr):.3e} ({tp:.3e}), dSSIM {abs(got.ssim - want.ssim):.3e} ({ts:.3e}), "
          f"drho {abs(got.rho - want.rho):.3e} ({ac.RHO_TOL[name]:.3e}); PSNR {got.psnr:.4f} SSIM {got.ssim:.6f}")
    assert got.ok and want.ok and got.gain == want.gain and got.coverage == want.coverage
    assert off <= ac.CORNER_TOL[name]
    assert abs(got.psnr - want.psnr) <= tp and abs(got.ssim - want.ssim) <= ts
    assert abs(got.rho - want.rho) <= ac.RHO_TOL[name]
    assert ac.corner_displacement(got.map, truth, h, w) <= ac.RECOVERY_BOUND[name]
    assert np.array_equal(cr.cpu().numpy(), cr_want)
    assert float(np.abs(zr.cpu().numpy().astype(np.float64) - zr_want.astype(np.float64)).max()) <= 1e-6
    m, status = align.ecc_homography_device(up(pred, dev), up(target, dev))
    assert m.dtype == torch.float64 and m.shape == (3, 3) and m.is_cuda and int(status.cpu()[0]) == 0
    assert np.array_equal(m.cpu().numpy(), got.map)
    short = align.calculate_metrics_aligned_device(up(pred, dev), up(target, dev), iterations=7)
    host = align.calculate_metrics_aligned(pred, target, iterations=7)
    assert ac.corner_displacement(short.map, host.map, h, w) <= ac.CORNER_TOL[name] and short.coverage == host.coverage


# --------------------------------------------------------------------------- 4. identical frames
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_identical_frames_on_the_device(dev, dtype):
    target = ac.pair("B")[1]
    x = target if dtype == np.uint8 else target.astype(np.uint16) * 257
    t = up(x if dtype == np.uint8 else x.view(np.int16), dev)
    zr, cr, r = align.align_to_target_device(t, t.clone())
    assert (r.psnr, r.ssim) == (float("inf"), 1.0) and r.ok and r.gain == 1.0 and r.coverage == 1.0
    assert np.abs(r.map - np.eye(3)).max() <= 1e-13 and abs(r.rho - 1.0) <= 1e-12
    peak = 255.0 if dtype == np.uint8 else 65535.0
    assert bool(cr.all()) and np.array_equal(zr.cpu().numpy(), (x / peak).astype(np.float32))


def test_flat_and_black_frames_fail_on_the_device(dev):
    target = ac.pair("B")[1]
    t = up(target, dev)
    r = align.calculate_metrics_aligned_device(up(np.full_like(target, 90), dev), t)
    assert not r.ok and np.array_equal(r.map, np.eye(3)) and r.coverage == 1.0
    want = align.calculate_metrics_aligned(np.full_like(target, 90), target)
    assert r.gain == want.gain and abs(r.psnr - want.psnr) <= psnr_ssim_tol(*ac.CASES["B"])[0]
    r = align.calculate_metrics_aligned_device(torch.zeros_like(t), t)
    assert not r.ok and r.gain == 0.0
    m, status = align.ecc_homography_device(torch.zeros_like(t), t)
    assert int(status.cpu()[0]) == 1 and np.array_equal(m.cpu().numpy(), np.eye(3))


# --------------------------------------------------------------------------- 5. reproducibility
def test_two_calls_are_bit_identical(dev):
    pred, target, _ = ac.pair("A")
    p, t = up(pred, dev), up(target, dev)
    runs = [align.align_to_target_device(p, t) for _ in range(2)]
    (zr0, cr0, r0), (zr1, cr1, r1) = runs
    assert torch.equal(zr0.view(torch.int32), zr1.view(torch.int32)) and torch.equal(cr0, cr1)
    assert np.array_equal(r0.map.view(np.uint64), r1.map.view(np.uint64))
    assert np.array([r0[:5]]).tobytes() == np.array([r1[:5]]).tobytes() and r0.ok == r1.ok


# --------------------------------------------------------------------------- 6. guard bands
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_guard_bands_align_prepare(dev, name):
    """Frames between bands of zeros and then of ones: the result must not depend on them.  gain, status, the four
    planes and the workspace, at exactly the header's minimum, between sentinels: all intact."""
    pred, target, _ = ac.pair(name)
    h, w = ac.CASES[name]
    r, planes, _, _ = statement(name)

    def run(fill):
        g = Guards(dev)
        p, t = g.inp(torch.from_numpy(pred.copy()), fill=fill), g.inp(torch.from_numpy(target.copy()), fill=fill)
        gain, status = g.out("gain", (1,), torch.float64), g.out("status", (1,), torch.int32)
        outs = [g.out(label, (h, w)) for label in ("T", "I", "Gx", "Gy")]
        ws = g.out("ws", (align.prepare_words(h, w),), torch.float64)
        _hip.call("irm_align_prepare", _hip.ptr(p), _hip.ptr(t), 0, h, w, _hip.ptr(gain), _hip.ptr(status),
                  *(_hip.ptr(o) for o in outs), _hip.ptr(ws), ws.numel())
        g.check()
        return (gain.cpu(), status.cpu()) + tuple(o.cpu() for o in outs)
    got = two_fills(run)
    assert float(got[0][0]) == r.gain and int(got[1][0]) == 0
    for k in range(4):
        assert np.array_equal(got[2 + k].numpy().view(np.uint32), planes[k].view(np.uint32)), k


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_guard_bands_ecc_iterate(dev, name):
    """The planes between bands of NaN; map, rho, status and the workspace at its minimum between sentinels.  Two
    rounds from the identity equal the statement's two rounds."""
    h, w = ac.CASES[name]
    planes = statement(name)[1]
    g = Guards(dev)
    ins = [g.inp(torch.from_numpy(p.copy())) for p in planes]
    dmap, rho, status = g.out("map", (9,), torch.float64), g.out("rho", (1,), torch.float64), g.out("status", (1,), torch.int32)
    ws = g.out("ws", (align.iterate_words(h, w),), torch.float64)
    dmap.copy_(torch.eye(3, dtype=torch.float64).reshape(-1))
    status.zero_()
    _hip.call("irm_ecc_iterate", *(_hip.ptr(p) for p in ins), h, w, 2, _hip.ptr(dmap), _hip.ptr(rho), _hip.ptr(status),
              _hip.ptr(ws), ws.numel())
    g.check()
    want, rho_want, ok = align.ecc_iterate(planes, 2)
    got = clean(dmap).numpy().reshape(3, 3)
    assert ok and int(status.cpu()[0]) == 0 and abs(float(clean(rho)[0]) - rho_want) <= ac.RHO_TOL[name]
    assert ac.corner_displacement(got, want, h, w) <= ac.CORNER_TOL[name]
    assert not bool(torch.isnan(ws).any()), "a NaN from outside a plane reached the sums"


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_guard_bands_aligned_metrics(dev, name):
    """Frames between bands of zeros and then of ones, gain and map between bands of NaN; out, status, zr, cr and the
    workspace at its minimum between sentinels.  The map pushes a third of the frame outside."""
    pred, target, _ = ac.pair(name)
    h, w = ac.CASES[name]
    gain = statement(name)[0].gain
    m = ac.outside_map(h, w)
    zr_want, cr_want = align.warp_to_target(pred, gain, m)

    def run(fill):
        g = Guards(dev)
        p, t = g.inp(torch.from_numpy(pred.copy()), fill=fill), g.inp(torch.from_numpy(target.copy()), fill=fill)
        dgain, dmap = g.inp(torch.tensor([gain], dtype=torch.float64)), g.inp(torch.from_numpy(m.reshape(-1).copy()))
        out, status = g.out("out", (9,), torch.float64), g.out("status", (1,), torch.int32)
        zr, cr = g.out("zr", (h, w, 3)), g.out("cr", (h, w), torch.uint8)
        ws = g.out("ws", (align.metrics_words(h, w),), torch.float64)
        _hip.call("irm_aligned_metrics", _hip.ptr(p), _hip.ptr(t), 0, h, w, _hip.ptr(dgain), _hip.ptr(dmap), _hip.ptr(out),
                  _hip.ptr(status), _hip.ptr(zr), _hip.ptr(cr), _hip.ptr(ws), ws.numel())
        g.check()
        assert int(status.cpu()[0]) == sentinel(torch.int32), "status is written only where the mask is empty"
        return clean(out), clean(zr), cr.cpu()
    out, zr, cr = two_fills(run)
    assert np.array_equal(cr.numpy(), cr_want.astype(np.uint8))
    assert float(np.abs(zr.numpy().astype(np.float64) - zr_want).max()) <= 1e-6
    assert float(out[1]) == float(cr_want.sum())


# --------------------------------------------------------------------------- 7. the harness row
def test_evaluate_aligned_rows_device_and_host(dev):
    """Three synthetic pairs through a DnCNN of synthetic weights: the rows of metrics="device" and metrics="host" agree
    within the tolerances of the whole protocol, the columns are complete.  A flat frame, scored as it is (the
    "before" row: a conv net with zero padding does not leave a flat frame flat), lands in Failed."""
    model = dncnn.DnCNN(3, 3, 64, 20, "R").load_synthetic(42).eval().to(dev)
    cfg = dict(patch_size=64, patch_overlap=16)
    pa, ta, pb, tb = (a.copy() for name in "AB" for a in ac.pair(name)[:2])          # the shared cases are read-only
    loader = [(pa, ta, "a"), (pb, tb, "b"), (np.ascontiguousarray(pa[::-1]), np.ascontiguousarray(ta[::-1]), "a_flipped")]
    rows = {k: harness.evaluate_aligned(model, loader, dev, cfg, metrics=k, model_name="DnCNN") for k in ("device", "host")}
    d, hst = rows["device"], rows["host"]
    print({k: (d[k], hst[k]) for k in ("PSNR", "SSIM", "Rho", "Coverage", "Std_PSNR", "Std_SSIM")}, d["Failed"], hst["Failed"])
    assert d["Failed"] == hst["Failed"] == []
    assert set(harness.COLUMNS_ALIGNED) <= set(d) and set(harness.COLUMNS_ALIGNED) <= set(hst)
    tp, ts = psnr_ssim_tol(*ac.CASES["A"])
    assert abs(d["PSNR"] - hst["PSNR"]) <= tp and abs(d["SSIM"] - hst["SSIM"]) <= ts
    assert abs(d["Rho"] - hst["Rho"]) <= max(ac.RHO_TOL.values()) and d["Coverage"] == hst["Coverage"]
    assert d["Model_Params"] == hst["Model_Params"] > 0 and d["Avg_Time_ms"] > 0
    flat = np.full_like(tb, 90)
    before = harness.evaluate_aligned(None, [(pb, tb, "b"), (flat, tb, "flat")], dev, cfg)
    assert [n for n, _ in before["Failed"]] == ["flat"] and "alignment failed" in before["Failed"][0][1]
    want = align.calculate_metrics_aligned(pb, tb)
    assert abs(before["PSNR"] - want.psnr) <= tp and before["Coverage"] == want.coverage and before["Model"] == "Input"
