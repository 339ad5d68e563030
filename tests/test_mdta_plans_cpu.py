"""The MDTA launch plans on the CPU (no GPU needed): every plan production asks of ops.mdta_plan falls into a class that
tests/test_gpu_mdta_plans.py runs (mdta_model.CASES), the planner's invariants, the positive control of the bars that file
holds the Gram records to, and pins of mdta_model itself."""
import itertools

import numpy as np
import pytest
import torch

import block_model as bm
import mdta_model as mm
from irm_amd import _hip, ops

SEED = 811

# (C, heads, divisor of the side) of the attention of a standard Restormer (dim 48, heads 1 / 2 / 4 / 8): the four levels,
# and decoder_level1 + refinement, which run at full resolution on 2 dim channels with heads[0] = 1 (c = 96)
LEVELS = [(48, 1, 1), (96, 2, 2), (192, 4, 4), (384, 8, 8)]
DECODER1 = (96, 1, 1)
# (B, H, W) of production forwards: the two Restormer workloads of tests/test_gpu_launch_replay.py (c3: 9 x 256^2 BiasFree, c4:
# 24 x 512^2 WithBias), the tiled 1280 x 720 call (6 tiles of 512^2 per frame; 12 and 24 per forward), the odd-size model test
PRODUCTION = [(9, 256, 256), (24, 512, 512), (6, 512, 512), (12, 512, 512), (1, 40, 56)]


def problems(B, H, W):
    for C, heads, d in LEVELS + [DECODER1]:
        yield B, C, heads, (H // d) * (W // d)


# --------------------------------------------------------------------------- coverage
def test_every_production_plan_class_has_a_gpu_case():
    gram = {(cls.family, cls.state) for cls in map(mm.case_class, mm.CASES)}
    splits = {z for _, _, _, z in mm.FINALIZE_CASES}
    missing = []
    for shape in PRODUCTION:
        for B, C, heads, N in problems(*shape):
            cls = mm.plan_class(B, C, heads, N, ops.mdta_plan(B, C, heads, N)[0])
            if (cls.family, cls.state) not in gram or cls.zsplit not in splits:
                missing.append((B, C, heads, N, cls))
    assert not missing, f"production plans without a case in mdta_model.CASES: {missing}"


def test_cases_reach_the_states_they_are_there_for():
    """The S_j, chunk counts and kernels of the cases, restated: a change of CASES that loses a state fails here."""
    S = mm.ring_stages
    assert [S(48, n, mm.WHOLE) for n in (64, 128, 192, 256, 448)] == [[1], [2], [3], [4], [7]]
    assert S(48, 448, 192) == [3, 2, 2] and S(48, 704, 256) == [4, 4, 3] and S(48, 1280, 448) == [7, 7, 6]
    assert S(48, 3136, 1600) == [25, 24]
    assert [S(96, n, mm.WHOLE) for n in (64, 128, 256, 448)] == [[2], [4], [8], [14]]
    assert S(96, 320, 128) == [4, 3, 3] and S(96, 448, 192) == [5, 5, 4] and S(96, 1216, 320) == [10, 10, 9, 9]
    classes = {(c.family, c.state) for c in map(mm.case_class, mm.CASES)}
    want = {"ring3": [((1,), False), ((2,), False), ((3,), False), ((4,), False), ((7,), False), ((1, 2), True), ((2, 3), True),
                      ((3, 4), True), ((4,), True), ((4, 7), True), ((7,), True)],
            "ring6": [((2,), False), ((4,), False), ((7,), False), ((3, 4), True), ((4,), True), ((7,), True)]}   # BP = 32: S is even in one workgroup
    for fam, states in want.items():
        assert not [s for s in states if (fam, s) not in classes], fam
    for sb, vec in itertools.product((1, 2, 3), (True, False)):
        states = {s for f, s in classes if f == f"guarded({sb}, {vec})"}
        assert {(3, "partial", "other"), (1, "partial", "other")} <= states, (sb, vec)        # chunk_id > 0 and a short tail
    for sb in (1, 2):
        states = {s for f, s in classes if f == f"guarded({sb}, True)"}
        assert {(3, "full", "0"), (2, "partial", "0")} <= states
    assert len({mm.case_id(c) for c in mm.CASES}) == len(mm.CASES)
    for case in mm.CASES:
        c, N = case.C // case.heads, case.H * case.W
        assert case.chunk % 64 == 0 and case.B == 2
        assert not case.tm or (N % 256 == 0 and c in (48, 96) and case.H % 8 == 0 and case.W % 32 == 0)
        assert not case.how or mm.case_class(case).family.endswith("False)")


# --------------------------------------------------------------------------- the planner
@pytest.mark.parametrize("B", [1, 2, 6, 9, 24])
def test_plan_invariants(B):
    for side in (64, 128, 256, 512):
        for _, C, heads, N in problems(B, side, side):
            c = C // heads
            chunk, nchunk, rec = ops.mdta_plan(B, C, heads, N)
            assert chunk % 64 == 0 and nchunk == -(-N // chunk) and rec == c * c + 2 * c
            if c in (48, 96) and N % 64 == 0:
                assert 128 <= chunk <= 4096
                assert nchunk <= N // (64 if c == 48 else 32), "a workgroup without a stage"
                assert min(mm.ring_stages(c, N, chunk)) >= 1


# --------------------------------------------------------------------------- the bars reject what the kernels could get wrong
CONTROLS = [mm.GramCase(48, 1, 8, 56, 192), mm.GramCase(96, 1, 8, 40, 128), mm.GramCase(96, 2, 8, 25, 64)]


@pytest.mark.parametrize("case", CONTROLS, ids=mm.case_id)
def test_bars_reject_a_stale_slot_and_a_dropped_tail(case):
    """One case per family.  stale: one block of q and k replaced by its predecessor (what a ring slot - or, in the guarded
    kernel, a 32-pixel register set - reused too early delivers); tail: the last block of a ring workgroup, or the partial last
    chunk of the guarded kernel, left out.  Both must miss the records' bars by 100x: one block moves the off-diagonal Gram
    entries by O(sqrt(BP)) products and the squared norms by O(BP), the bar is about 2^-22 N / 3 of one."""
    assert mm.case_class(case).family in ("ring3", "ring6", "guarded(3, True)") and case in mm.CASES
    C, heads, N = case.C, case.heads, case.H * case.W
    c = C // heads
    qkv, _, _, _ = mm.operands(SEED, mm.case_id(case), case.B, C, heads, case.H, case.W)
    q, k = qkv[:, :C].reshape(case.B, C, N), qkv[:, C:2 * C].reshape(case.B, C, N)
    ref = mm.gram_records_f64(q, k, heads)
    ymax = float(ref.abs().max())
    e32 = float((mm.gram_records(q, k, heads).double() - ref).abs().max())
    assert bm.passes(e32, e32, ymax)
    ring = c in (48, 96) and N % 64 == 0
    bp = (64 if c == 48 else 32) if ring else 32
    nchunk = -(-N // case.chunk)
    keep = N - bp if ring else (nchunk - 1) * case.chunk
    assert 0 < keep < N
    stale_q, stale_k = q.clone(), k.clone()
    blk = 2
    stale_q[..., blk * bp:(blk + 1) * bp], stale_k[..., blk * bp:(blk + 1) * bp] = q[..., (blk - 1) * bp:blk * bp], k[..., (blk - 1) * bp:blk * bp]
    for name, rec in (("stale", mm.gram_records_f64(stale_q, stale_k, heads)), ("tail", mm.gram_records_f64(q[..., :keep], k[..., :keep], heads))):
        e = float((rec - ref).abs().max())
        print(f"{mm.case_id(case)} {name}: e {e:.3e}  bar {bm.K * e32 + bm.F * ymax:.3e}  margin {e / (bm.K * e32 + bm.F * ymax):.1e}")
        assert not bm.passes(e, e32, ymax)
        assert e >= 100 * (bm.K * e32 + bm.F * ymax), name                      # the exact-f32 kernels' bar
        assert e / ymax >= 100 * (2 * e32 / ymax + 2e-7), name                   # the emulated kernels' bar


# --------------------------------------------------------------------------- the model
def _reduce_literal(part):
    """mdta_reduce_kernel line by line on numpy float32 scalars: part [nchunk][rec]."""
    nchunk, rec = part.shape
    out = np.zeros(rec, np.float32)
    for e in range(rec):
        sm = []
        for w in range(4):
            s, ch = np.float32(0.0), w
            while ch + 12 < nchunk:
                v0, v1, v2, v3 = part[ch, e], part[ch + 4, e], part[ch + 8, e], part[ch + 12, e]
                s = s + v0
                s = s + v1
                s = s + v2
                s = s + v3
                ch += 16
            while ch < nchunk:
                s = s + part[ch, e]
                ch += 4
            sm.append(s)
        out[e] = ((sm[0] + sm[1]) + sm[2]) + sm[3]
    return out


@pytest.mark.parametrize("nchunk", mm.REDUCE_NCHUNK + [33, 64])
def test_reduce_model(nchunk):
    part = mm.operands(SEED, f"r{nchunk}", 1, 16, 1, nchunk, 5)[0][0, :16].reshape(nchunk, 80) * 1000.0
    got = mm.reduce_f32(part, nchunk)
    assert got.dtype == torch.float32
    assert mm.same_bits(got, torch.from_numpy(_reduce_literal(part.numpy())))
    exact = part.double().sum(0)
    assert bool(((got.double() - exact).abs() <= nchunk * 2.0 ** -24 * part.double().abs().sum(0)).all())


def test_same_bits_sees_what_equal_does_not():
    z = torch.zeros(3)
    assert torch.equal(z, -z) and not mm.same_bits(z, -z) and mm.same_bits(z, z.clone())


@pytest.mark.parametrize("B,C,heads,zsplit", mm.FINALIZE_CASES)
def test_zsplit_model(B, C, heads, zsplit):
    assert mm.plan_class(B, C, heads, 64, mm.WHOLE).zsplit == zsplit
    assert mm.finalize_lds(C, heads, zsplit) <= 64 * 1024
    if (B, C, heads) == (129, 96, 1):
        assert mm.finalize_lds(C, heads, zsplit) == 56064 and mm.finalize_lds(C, heads, 1) > 64 * 1024
    if (B, C, heads) == (17, 384, 8):
        assert mm.finalize_lds(C, heads, zsplit) == 46464
    assert B * heads <= 65535


def test_plan_class_follows_the_dispatch():
    P = mm.plan_class
    assert P(2, 48, 1, 448, 192) == ("ring3", ((2, 3), True), 8) and P(2, 96, 1, 64, 4096) == ("ring6", ((2,), False), 8)
    assert P(2, 48, 1, 448, 192, aligned=False).family == "guarded(3, False)"           # the ring needs float4 rows
    assert P(2, 96, 2, 200, 64) == ("guarded(3, True)", (3, "partial", "other"), 8)
    assert P(2, 64, 2, 320, 64).state == (3, "full", "0") and P(2, 64, 2, 320, 256).state == (2, "partial", "0")
    assert P(2, 32, 2, 135, 64) == ("guarded(1, False)", (3, "partial", "other"), 8)
    assert P(2, 192, 1, 64, 4096).family == "guarded(3, True)"                           # c = 192: no ring
    plan = mm.explicit_plan(192)
    assert plan(2, 96, 2, 448) == (192, 3, 48 * 48 + 96)


def test_unpack_mfold_split_inverts_the_packer():
    m = mm.operands(SEED, "sp", 2, 96, 1, 1, 1)[3].view(1, 96, 96).repeat(2, 1, 1)
    m[1] *= -0.5
    packed = torch.cat([_hip.pack_gemm_weight_split(m[i]) for i in range(2)])
    hi = m.half().float()
    assert torch.equal(mm.unpack_mfold_split(packed, 2, 96), hi + (m - hi).half().float())
    assert packed.numel() == 2 * ops.mfold_numel(96)
