"""Launch planners of the 1x1 GEMM and the 3x3 conv (ops.plan_gemm1x1, ops.plan_conv3x3), swept on the CPU: every plan
they make must be one the C switches accept, with no workgroup group left without a pass."""
import pytest

from irm_amd import ops
from variant_model import (CASE_STRUCTURES, CONV_VARIANTS, VARIANTS, expected_conv_variant, expected_variant, pass_structure,
                           passes_per_group)

GEMM_CTS = {3, 4, 6, 8, 9}               # gemm_entry (gemm_pw.hip)
CONV_CTS = {1, 2, 3, 4, 6}               # irm_conv3x3_f32 (conv3x3.hip)
CONV_F16_CTS = {1, 2, 3, 4, 8, 12}       # irm_conv3x3_f16x3_f32 (conv3x3_f16.hip)

# (N, B): single small images up to the 1280 x 720 frame and the bench batches
GEMM_SHAPES = [(16, 1), (240, 1), (4096, 1), (4096, 9), (65536, 1), (65536, 24), (1280 * 720, 1)]
# with W % 4 != 0 (a BSD68 image, a 1023-wide one) the exact planner's launches run on the generic kernel
CONV_SHAPES = [(4, 4, 1), (8, 32, 1), (13, 21, 2), (64, 64, 1), (128, 128, 9), (256, 256, 8), (720, 1280, 1),
               (321, 481, 1), (1023, 1024, 1), (1024, 1023, 1)]


def _ms(step):
    return sorted(set(range(1, 2049, step)) | {1, 15, 16, 17, 44, 48, 144, 180, 2048})


def _groups_nonempty(nchunks, yg):
    """Workgroup y of the launch takes passes y, y + yg, ... (gemm_ring_kernel, gemm_pw_kernel, the conv kernels)."""
    return all(-(-(nchunks - y) // yg) > 0 for y in range(yg))


@pytest.mark.parametrize("split,res", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("N,B", GEMM_SHAPES)
def test_gemm_plan_sweep(N, B, split, res):
    for M in _ms(1 if (N, B) == (4096, 1) else 5):
        for K in (48, 600):
            ct, yg = ops.plan_gemm1x1(M, K, N, B, split=split, res=res)
            mt = (M + 15) // 16
            nchunks = -(-mt // ct)
            assert ct in GEMM_CTS, (M, N, B, ct)
            assert 1 <= yg <= nchunks and _groups_nonempty(nchunks, yg), (M, N, B, ct, yg)
            v = expected_variant(split=split, M=M, K=K, N=N, B=B, ct=ct, ygroups=yg, ln=0, res=res, stats_out=False,
                                 w_bs=False, vec=N % 4 == 0)
            assert v in VARIANTS, (M, N, B, ct, yg, v)


@pytest.mark.parametrize("N,B", GEMM_SHAPES)
def test_gemm_plan_explicit_ct(N, B):
    """An explicit ct keeps its value; ygroups then comes from the pixel blocks."""
    for M in _ms(3):
        mt = (M + 15) // 16
        for ct in sorted(GEMM_CTS):
            got_ct, yg = ops.plan_gemm1x1(M, 96, N, B, ct=ct)
            assert got_ct == ct and 1 <= yg <= -(-mt // ct)


@pytest.mark.parametrize("res", [False, True])
def test_stats_out_rule(res):
    """stats_out is planned iff can_fuse_stats(M), and then as the C side needs it (gemm_pw.hip:644): every output tile
    in one pass, one group."""
    for M in _ms(1):
        mt = (M + 15) // 16
        for N, B in ((4096, 1), (65536, 2)):
            if ops.can_fuse_stats(M):
                ct, yg = ops.plan_gemm1x1(M, 96, N, B, res=res, stats_out=True)
                assert ct in GEMM_CTS and mt <= ct and yg == 1, (M, ct, yg)
                assert expected_variant(split=False, M=M, K=96, N=N, B=B, ct=ct, ygroups=yg, ln=0, res=res,
                                        stats_out=True, w_bs=False, vec=True) in VARIANTS
            else:
                with pytest.raises(AssertionError):
                    ops.plan_gemm1x1(M, 96, N, B, res=res, stats_out=True)
    assert ops.can_fuse_stats(144) and not ops.can_fuse_stats(145)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("H,W,B", CONV_SHAPES)
def test_conv_plan_sweep(H, W, B, split):
    for co in _ms(3):
        ct, yg = ops.plan_conv3x3(co, H, W, B, split=split)
        mt = (co + 15) // 16
        nchunks = -(-mt // ct)
        assert ct in (CONV_F16_CTS if split else CONV_CTS), (co, H, W, B, ct)
        assert 1 <= yg <= nchunks and _groups_nonempty(nchunks, yg), (co, H, W, B, ct, yg)
        if split:
            assert nchunks % yg == 0, (co, H, W, B, ct, yg)      # equal passes per group
            if W % 4:
                continue                                         # ops.conv3x3 sends such an image to the exact kernel
        # dense tensors: the kernel the plan lands on (tests/test_gpu_conv_variants.py tests it), and its pass structure
        bs = 64 * H * W
        v = expected_conv_variant("split" if split else "exact", 64, co, W, ct, bs, co * H * W, 0, True, True, True, True)
        assert v is not None and v[0] in CONV_VARIANTS, (co, H, W, B, ct, yg, v)
        assert v == expected_conv_variant("split" if split else "exact", 64, co, W, ct, bs, co * H * W, co * H * W, True,
                                          True, True, True)     # ... with a residual too
        structure = pass_structure(passes_per_group(mt, ct, yg))
        assert structure in CASE_STRUCTURES[v[0]], (co, H, W, B, ct, yg, v, structure)


def test_conv_plan_explicit_values_kept():
    assert ops.plan_conv3x3(192, 8, 32, 1, split=True, ct=3)[0] == 3
    assert ops.plan_conv3x3(192, 8, 32, 1, split=False, ct=2, ygroups=5) == (2, 5)
