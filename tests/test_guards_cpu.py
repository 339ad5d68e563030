"""Positive controls of tests/guards.py on CPU tensors (no GPU needed): every kind of stray access the helpers are
there to catch is committed on purpose by a torch expression standing in for a kernel, and must be caught.  Plus the
coverage rule: every entry point of the C ABI has a guard-band case."""
import os
import re

import pytest
import torch

from irm_amd import _hip

import guards
from guards import banded, has_nan, intact, outside, sentinel, sentinel_out, two_fills

CPU = torch.device("cpu")
HERE = os.path.dirname(os.path.abspath(__file__))


def test_layout_alignment_and_contents():
    t = torch.arange(2 * 3 * 5, dtype=torch.float32).view(2, 3, 5)
    buf, view = banded(t, CPU, batch_slack=8)
    assert torch.equal(view, t) and view.stride() == (23, 5, 1) and view.storage_offset() == guards.PAD
    assert buf.numel() == 2 * guards.PAD + 23 + 15
    assert int(outside(buf, view).sum()) == 2 * guards.PAD + 8
    assert bool(torch.isnan(buf[outside(buf, view)]).all())          # bands and slack hold the fill
    with pytest.raises(AssertionError):
        banded(t, CPU, pad=6)                                           # would break the 16-byte alignment
    with pytest.raises(AssertionError):
        banded(t, CPU, batch_slack=2)
    with pytest.raises(AssertionError):
        banded(torch.zeros(4, dtype=torch.int32), CPU)                  # integers cannot hold NaN: explicit fill


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.uint8, torch.int16, torch.int32, torch.int64])
def test_intact_catches_every_stray_write(dtype):
    def fresh():
        return sentinel_out((2, 3, 4), CPU, dtype, batch_slack=4)
    buf, view = fresh()
    view.fill_(1)                                                       # a well-behaved kernel
    assert intact(buf, view)
    if not dtype.is_floating_point:
        assert all(int(b) == guards.SENTINEL_BYTE for b in buf[:1].view(torch.uint8))
    first, last = guards.PAD, guards.PAD + 12 + 4 + 12 - 1              # the view's first and last element in buf
    for where in (first - 1, last + 1, 0, buf.numel() - 1, first + 12, first + 15):   # before, after, far ends, batch slack
        buf, view = fresh()
        buf[where] = 1
        assert not intact(buf, view), where
    buf, view = fresh()
    buf[first], buf[last], buf[first + 16] = 1, 1, 1                    # the view's own corners are not guards
    assert intact(buf, view)


def test_nan_band_catches_a_masked_over_read():
    t = torch.rand(2, 8)
    buf, x = banded(t, CPU, batch_slack=4)

    def kernel(leak):
        # sums each row; the sloppy version also loads one element past the row and multiplies it by zero
        return x.sum(1) + 0.0 * buf[guards.PAD + 8 + torch.tensor([0, 12])] if leak else x.sum(1)
    assert not has_nan(kernel(False)) and torch.allclose(kernel(False), t.sum(1))
    assert has_nan(kernel(True))
    before = 0.0 * buf[guards.PAD - 1] + x[0, 0]                        # one element before the operand
    assert has_nan(before)


def test_two_fills_catch_an_integer_over_read():
    t = torch.randint(0, 256, (3, 4), dtype=torch.uint8)

    def run(leak):
        def go(fill):
            buf, x = banded(t, CPU, fill)
            extra = buf[guards.PAD + t.numel()].long() if leak else 0   # one element past the frame
            return ((x.long().sum() + extra).view(1),)
        return go
    assert int(two_fills(run(False))[0]) == int(t.long().sum())
    with pytest.raises(AssertionError, match="outside an integer operand"):
        two_fills(run(True))
    for dtype in (torch.uint8, torch.int16, torch.int32):               # -1 sets every bit of any width
        buf, _ = banded(torch.zeros(4, dtype=dtype), CPU, -1)
        assert all(int(b) == 0xFF for b in buf[:2].view(torch.uint8))


def test_sentinels_are_no_plausible_results():
    assert sentinel(torch.float32) == 12345.0 and sentinel(torch.uint8) == 0xA5
    assert sentinel(torch.int16) == 0xA5A5 - (1 << 16) and sentinel(torch.int64) < 0


# --------------------------------------------------------------------------- every entry point has a guard-band case
#: wrapper call as it appears in the two test files -> the entry points that call reaches there
WRAPPERS = {
    "ops.ln_stats(": ["irm_ln_stats_f32"],
    "ops.gemm1x1(": ["irm_gemm1x1_f32", "irm_gemm1x1_f16x3_f32"],                       # split in (True, False)
    "ops.dwconv3x3(": ["irm_dwconv3x3_f32"],
    "ops.dwconv3x3_gate(": ["irm_dwconv3x3_gate_f32"],
    "ops.mdta_fold(": ["irm_mdta_gram_f32", "irm_mdta_gram_f16x3_f32", "irm_mdta_finalize_f32", "irm_mdta_finalize_f16x3_f32",
                       "irm_mdta_gram_tm_f32", "irm_mdta_gram_tm_f16x3_f32", "irm_mdta_finalize_frag_f16x3_f32"],
    "ops.gdfn_fused(": ["irm_gdfn_fused_f16x3_f32"],
    "ops.qkv_dw_fused(": ["irm_qkv_dw_fused_f16x3_f32", "irm_qkv_dw_fused_tm_f16x3_f32", "irm_qkv_dw_cm_f16x3_f32"],
    "ops.conv3x3(": ["irm_conv3x3_ep_f32", "irm_conv3x3_f16x3_ep_f32", "irm_conv3x3_thin_f32"],
    "ops.ln_split(": ["irm_ln_split_f16"],
    "ops.gemm_presplit(": ["irm_gemm_presplit_f16x3_f32"],
    "ops.ln_gemm_presplit(": ["irm_ln_gemm_presplit_f16x3_f32"],
    "ops.ln_gemm_presplit_cl(": ["irm_ln_gemm_presplit_cl_f16x3_f32"],
    "ops.gdfn_tail(": ["irm_gdfn_tail_f16x3_f32"],
    "ops.dwgemm(": ["irm_dwgemm_f32", "irm_dwgemm_f16x3_f32"],
    "ops.attn_gdfn_fused(": ["irm_attn_gdfn_fused_f16x3_f32"],
    "ops.qkv_gram_cm(": ["irm_qkv_gram_cm_f16x3_f32"],
    "ops.transpose(": ["irm_transpose_f32"],
    "ops.selective_scan(": ["irm_selective_scan_f32"],
    "ops.losh_combine(": ["irm_losh_combine_f32"],
    "ops.chan_norm_act(": ["irm_chan_norm_act_f32"],
    "ops.conv3x3_s2(": ["irm_conv3x3_s2_f32"],
    "ops.dwconv3x3_s2(": ["irm_dwconv3x3_s2_f32"],
    "ops.upsample_add(": ["irm_upsample_add_f32"],
    "ensemble.dihedral_chop(": ["irm_dihedral_chop_f32"],
    "ensemble.ensemble_merge(": ["irm_ensemble_merge_f32"],
}


def test_every_entry_point_has_a_guard_band_case():
    """Every symbol of _hip.SIGNATURES except irm_version is named in tests/test_gpu_guard_bands.py, or reached there
    or in test_gpu_ops.py::test_no_write_outside_the_output through a wrapper of the map above: a kernel added later
    fails here until it gets a case."""
    with open(os.path.join(HERE, "test_gpu_guard_bands.py")) as f:
        text = f.read()
    with open(os.path.join(HERE, "test_gpu_ops.py")) as f:
        ops_text = f.read()
    text += ops_text[ops_text.index("def test_no_write_outside_the_output"):]
    known = set(_hip.SIGNATURES)
    reached = set(re.findall(r'"(irm_\w+)"', text))
    for call, symbols in WRAPPERS.items():
        assert set(symbols) <= known, f"the map names an entry point the library does not have: {call}"
        if call in text:
            reached.update(symbols)
    missing = sorted(known - reached - {"irm_version"})
    assert not missing, f"entry points without a guard-band case: {missing}"
