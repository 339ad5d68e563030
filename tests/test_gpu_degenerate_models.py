"""The precision ledger (tests/test_gpu_precision.py) on frames instead of noise: black, flat, letterboxed, checkered.

Machinery and bar are the ledger's (tests/ledger.py): the cases, the model builds, the CPU oracles and the one pass function
e_gpu <= K * e_32 + F * max|y64|, where e_32 and y64 come from the CPU oracle ON THE SAME FRAME - the oracle's own fp32
error moves by two orders of magnitude with the frame content, and the bar moves with it.  Restormer is held on both
rows, `out` and the `refinement` tap.  The oracle runs are cached in ledger.py's cache under (case, frame); the
WithBias variants that share weights, oracle and size (fused, unfused, IRM_GEMM_EXACT=1) share one run.

test_frame_table prints the table of DESIGN.md, section "Degenerate inputs"."""
import pytest
import torch

import degenerate as dg
import half_model as hm
import ledger
from irm_amd import dncnn

pytestmark = pytest.mark.gpu

FOUR = ("black", "flat_hot", "letterbox", "checker")
TWO = ("black", "letterbox")
PLAN = {
    "restormer_wb_64x64_b1": FOUR, "restormer_bf_64x64_b1": FOUR,
    "restormer_wb_64x64_b1_unfused": TWO, "restormer_wb_128x128_b1_exact": TWO,
    "mairunet_32x32_b1": TWO,
    "mair_flat_16x16_b1": dg.FRAMES, "dncnn_color20_29x45_b1": dg.FRAMES, "dncnn_gray17_37x53_b2": dg.FRAMES,
    "rednet_33x45_b1": dg.FRAMES, "fpn_mobilenet_96x160_b1": dg.FRAMES,
}
#: the case whose oracle run a case shares (same weights, same oracle function), and the size it runs at here
ORACLE_OF = {"restormer_wb_64x64_b1_unfused": "restormer_wb_64x64_b1", "restormer_wb_128x128_b1_exact": "restormer_wb_64x64_b1"}
SHAPE_OF = {"restormer_wb_128x128_b1_exact": (1, 3, 64, 64)}
PAIRS = [(case, kind) for case, kinds in PLAN.items() for kind in kinds]
_ROWS = {}      # (case, frame, row) -> (e_gpu, e_32, max|y64|, passed)


def frame_of(case, kind):
    _, shape, (lo, hi), _, _ = ledger.CASES[case]
    return dg.frame(kind, SHAPE_OF.get(case, shape), lo, hi)


def oracle(case, p, kind, x):
    """{row: (y64, e_32)}: the ledger's oracle on a frame, finite in both precisions."""
    ref = ledger.oracle(ORACLE_OF.get(case, case), p, frame=kind, x=x)
    for row, (y64, e32) in ref.items():
        assert bool(torch.isfinite(y64).all()) and e32 == e32 and e32 != float("inf"), (case, kind, row)
    return ref


def rows_of(case, kind, got, ref):
    """[(row, e_gpu, e_32, max|y64|, passed)], recorded for the table."""
    out = []
    for row, (y64, e32) in ref.items():
        e_gpu, ymax = float((got[row] - y64).abs().max()), float(y64.abs().max())
        ok = ledger.passes(e_gpu, e32, ymax)
        _ROWS[(case, kind, row)] = (e_gpu, e32, ymax, ok)
        print(f"{case:34s} {kind:10s} {row:11s} e_gpu {e_gpu:.3e}  e_32 {e32:.3e}  ratio {e_gpu / e32 if e32 else float('nan'):6.2f}  "
              f"|y64| max {ymax:.3g}  {'ok' if ok else 'FAIL'}")
        out.append((row, e_gpu, e32, ymax, ok))
    return out


@pytest.mark.parametrize("case,kind", PAIRS)
def test_ledger_on_frames(dev, monkeypatch, case, kind):
    """Measured on the MI355X: DESIGN.md, section 17, has the whole table.  No row is marked.  Three rows stood above the bar
    when these frames were first run, each a defect since fixed: MaIRUNet on black / letterbox at 15.8 / 12.1 x e_32 (out_proj
    on the fp16-emulated GEMM; now on the exact kernel, 1.4 / 1.5) and FPN-MobileNet on checker at 9.5 (float32 sums in the
    InstanceNorm statistics; now float64, 1.9 - and black 3.6 -> 2.1)."""
    model, p = ledger.build(case, dev, monkeypatch)
    x = frame_of(case, kind)
    ref = oracle(case, p, kind, x)
    got = ledger.run_gpu(case, dev, model, "refinement" in ref, x=x)
    exact_zero = case == "restormer_bf_64x64_b1" and kind == "black"
    for row, (y64, e32) in ref.items():
        assert bool(torch.isfinite(got[row]).all()), row
        if exact_zero:          # a bias-free network maps black to exact zeros at every layer: oracle and kernels alike
            assert e32 == 0.0 and not bool(y64.any()) and not bool(got[row].any()), row
        else:
            assert e32 > 0.0, row
    bad = [row for row, _, _, _, ok in rows_of(case, kind, got, ref) if not ok]
    assert not bad, f"above K * e_32 + F * |y64|max (K = {ledger.K}, F = 2^-22): {bad}"


def test_positive_control_letterbox(dev, monkeypatch):
    """As the ledger's control: one GEMM weight of the GPU model rounded through fp16 must fail the same pass function on
    the letterbox frame, on both rows.  The layer is the first block's ffn.project_out, not the ledger's
    latent.3.ffn.project_out: on this frame e_32 is 7x its noise value, and the float64 oracle with one weight rounded
    (no GPU involved) puts a rounded latent layer at 2 ... 3 x e_32, under the bar, while a layer of the first block,
    which every later layer amplifies, stands at 50 x e_32 (Degenerate inputs)."""
    case, kind = "restormer_wb_64x64_b1", "letterbox"
    model, p = ledger.build(case, dev, monkeypatch)
    x = frame_of(case, kind)
    ref = oracle(case, p, kind, x)
    w = model.encoder_level1[0].ffn.project_out.weight
    with torch.no_grad():
        w.copy_(w.half().float())
    got = ledger.run_gpu(case, dev, model, True, x=x)
    for row, (y64, e32) in ref.items():
        e_gpu = float((got[row] - y64).abs().max())
        print(f"control {kind} {row}: e_gpu {e_gpu:.3e}  e_32 {e32:.3e}  ratio {e_gpu / e32:.1f}")
        assert not ledger.passes(e_gpu, e32, float(y64.abs().max())), row


@pytest.mark.parametrize("kind", dg.FRAMES)
def test_dncnn_gray17_fp16_mode_on_frames(dev, kind):
    """The fp16 inference mode of the ledger's DnCNN case against the quantised chain with float64 sums, with
    test_gpu_half.test_model_vs_quantised_chain's own bar: 8 d0 + 2^-20 max|A| (d0: the chain's distance to itself with
    float32 sums on the same frame)."""
    case = "dncnn_gray17_37x53_b2"
    x = frame_of(case, kind)
    spec = hm.dncnn_spec(dncnn.DnCNN(1, 1, 64, 17, "R").load_synthetic(42))
    A = hm.run_chain(spec, x, "f64")
    d0 = float((A - hm.run_chain(spec, x, "f32")).abs().max())
    model = dncnn.DnCNN(1, 1, 64, 17, "R", precision="fp16").load_synthetic(42).eval().to(dev)
    with torch.no_grad():
        y = model(x.to(dev)).cpu().double()
    dist, bound = float((y - A).abs().max()), 8 * d0 + 2.0 ** -20 * float(A.abs().max())
    _ROWS[(case + " fp16", kind, "out")] = (dist, d0, float(A.abs().max()), dist <= bound)
    print(f"{case} fp16 {kind}: d0 = {d0:.3e}, max |gpu - A| = {dist:.3e}, bound = {bound:.3e}, max |A| = {float(A.abs().max()):.3f}")
    assert y.shape == A.shape and bool(torch.isfinite(y).all()) and dist <= bound


def test_frame_table(request):
    """Prints the frame table (case, frame, row, e_gpu, e_32, ratio).  Needs the whole module in one process, as the ledger's own
    table does: it skips itself under -k or a split of the module over workers - the run of the whole file is the one that counts."""
    ran = {(it.callspec.params["case"], it.callspec.params["kind"]) for it in request.session.items
           if it.module is request.module and it.originalname == "test_ledger_on_frames"}
    if ran != set(PAIRS):
        pytest.skip("only part of the frames was selected")
    print(f"\nledger on frames: K = {ledger.K}, F = {ledger.F:.3g}  (fp16 rows: e_32 column = d0, bar 8 d0 + 2^-20 |A|max)")
    print(f"{'case':34s} {'frame':10s} {'row':11s} {'e_gpu':>10s} {'e_32':>10s} {'ratio':>7s}")
    for (case, kind, row), (e_gpu, e32, _, ok) in _ROWS.items():
        print(f"{case:34s} {kind:10s} {row:11s} {e_gpu:10.3e} {e32:10.3e} {e_gpu / e32 if e32 else float('nan'):7.2f}{'' if ok else '  FAIL'}")
    assert len({k[:2] for k in _ROWS if not k[0].endswith("fp16")}) == len(PAIRS)
