"""Model-level precision ledger: every model path against the float64 oracle.

For each case, on the same seeded input:
  e_gpu = max|y_gpu - y64|   (y64: the CPU oracle run in float64 with the model's weights in float64)
  e_32  = max|y32 - y64|     (y32: the same oracle in fp32 - the arithmetic the reference itself performs)
and the case passes when e_gpu <= K * e_32 + F * max|y64|, with ONE pair (K, F) for the whole file.

The model-level goldens (tests/test_gpu_models.py, 1e-3 max-abs) sit ~1000x above the errors actually reached; this
bar sits a few times above plain fp32.  With every GEMM weight of Restormer rounded to fp16 the oracle's own error
grows ~1700x, with ONE layer (latent.3.ffn.project_out) rounded ~18x: K <= 8 keeps the one-layer case caught, which
test_positive_control_one_fp16_layer checks on the GPU model.

The cases (every dispatch outcome of restormer.py at least once), builds, oracles and runs are tests/ledger.py's, the bar
tests/block_model.py's; test_every_entry_point_is_reached asserts that every irm_* entry point ops.py launches was reached."""
import os
import re

import pytest
import torch

from block_model import F, K, passes, record_calls
from irm_amd import _hip
from ledger import CASES, build, oracle, run_gpu

pytestmark = pytest.mark.gpu

_ROWS = {}         # row -> (e_gpu, e_32, max|y64|, passed)
_REACHED = set()   # irm_* entry points launched while this module ran


@pytest.fixture(scope="module", autouse=True)
def _record_entry_points():
    yield from record_calls(_REACHED)


@pytest.mark.parametrize("case", list(CASES))
def test_ledger(dev, monkeypatch, case):
    model, p = build(case, dev, monkeypatch)
    ref = oracle(case, p)
    got = run_gpu(case, dev, model, "refinement" in ref)
    bad = []
    for row, (y64, e32) in ref.items():
        e_gpu = float((got[row] - y64).abs().max())
        ymax = float(y64.abs().max())
        ok = passes(e_gpu, e32, ymax)
        name = case if row == "out" else f"{case}:{row}"
        _ROWS[name] = (e_gpu, e32, ymax, ok)
        print(f"{name:48s} e_gpu {e_gpu:.3e}  e_32 {e32:.3e}  ratio {e_gpu / e32 if e32 else float('inf'):6.2f}  "
              f"|y64| max {ymax:.3g}  {'ok' if ok else 'FAIL'}")
        if not ok:
            bad.append(name)
    assert not bad, f"above K * e_32 + F * |y64|max (K = {K}, F = 2^{int(round(torch.log2(torch.tensor(F)).item()))}): {bad}"


def test_positive_control_one_fp16_layer(dev, monkeypatch):
    """One GEMM weight rounded through fp16 on the GPU model only (the oracle keeps the fp32 weights): the same pass
    function must reject it - the ledger would notice one kernel that lost the lo half of its split."""
    case = "restormer_wb_64x64_b1"
    model, p = build(case, dev, monkeypatch)
    ref = oracle(case, p)
    w = model.latent[3].ffn.project_out.weight
    with torch.no_grad():
        w.copy_(w.half().float())
    got = run_gpu(case, dev, model, True)
    for row, (y64, e32) in ref.items():
        e_gpu = float((got[row] - y64).abs().max())
        print(f"control {row}: e_gpu {e_gpu:.3e}  e_32 {e32:.3e}  ratio {e_gpu / e32:.1f}")
        assert not passes(e_gpu, e32, float(y64.abs().max())), row


def test_every_entry_point_is_reached(request):
    """Every irm_* entry point ops.py launches was reached by the ledger cases: a new kernel path
    cannot escape the ledger.  Also prints the ledger table.  Only meaningful when the whole ledger ran."""
    ran = {it.callspec.params["case"] for it in request.session.items
           if it.module is request.module and it.originalname == "test_ledger"}
    if ran != set(CASES) or len([r for r in _ROWS if ":" not in r]) != len(CASES):
        pytest.skip("only part of the ledger was selected")
    print(f"\nprecision ledger: K = {K}, F = {F:.3g}")
    print(f"{'case':48s} {'e_gpu':>10s} {'e_32':>10s} {'ratio':>7s}")
    for name, (e_gpu, e32, _, ok) in _ROWS.items():
        print(f"{name:48s} {e_gpu:10.3e} {e32:10.3e} {e_gpu / e32 if e32 else float('inf'):7.2f}{'' if ok else '  FAIL'}")
    with open(os.path.join(os.path.dirname(os.path.abspath(_hip.__file__)), "ops.py")) as f:
        launched = set(re.findall(r'"(irm_[a-z0-9_]+)"', f.read()))
    missing = sorted(launched - _REACHED)
    assert not missing, f"entry points no ledger case reaches: {missing}"
