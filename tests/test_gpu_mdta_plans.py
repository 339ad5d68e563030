"""The MDTA core (csrc/mdta.hip) at the launch plans production uses, on the smallest shapes that reach them.

ops.mdta_plan answers one thing at the small N of the op tests: two ring stages per workgroup at c = 48, a single chunk in the
guarded kernel, zsplit = 8 in the finalize.  Here the plan is set explicitly (mdta_model.explicit_plan replaces ops.mdta_plan;
the launch still goes through ops.mdta_fold), so that every state of mdta_model's docstring runs: the ring kernels at S = 1, 2,
3, 4, 7 and more stages per workgroup, even and uneven across the workgroups, planar and tile-major, exact and emulated; the
guarded kernel with chunk_id > 0 and full, partial and 64-aligned last chunks for every (SB, VEC); the reduction at the
chunk counts of both of its loops; the finalize at every row split.  tests/test_mdta_plans_cpu.py ties production plans to
mdta_model.CASES and shows that the bars below reject a stale ring slot and a dropped tail by five orders of magnitude.

Every operand lies in guard bands (tests/guards.py): q, k between NaN with v = NaN, part / gsum / attn / mfold at exactly their
sizes between sentinels.  Bars are the suite's existing ones: the ledger's e <= K e_32 + F max|ref| for the exact-f32 kernels
(e_32: float32 torch on the device, TF32 off), test_mdta_gram_f16x3's e16 <= 2 e32 + 2e-7 for the emulated ones, test_mdta_fold's
2e-5 on the attention matrix and 1e-6 on the folded matrix; gsum equals mdta_model.reduce_f32 of the records bit for bit."""
import functools

import pytest
import torch

import block_model as bm
import guards
import mdta_model as mm
from guards import SLACK, Guards, clean
from irm_amd import _hip, ops, synth

pytestmark = pytest.mark.gpu

SEED = 4177
ATTN_TOL = 2e-5          # tests/test_gpu_ops.py::test_mdta_fold
MFOLD_TOL = 1e-6         # the same test, per unit of max(1, max|wout blockdiag(attn)|)
_WORST = {}              # kernel family -> (worst measured fraction of its bar, case)


@pytest.fixture(autouse=True)
def _no_tf32():
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = prev


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam, (ratio, case) in sorted(_WORST.items()):
        print(f"\nmdta plans: worst fraction of the bar, {fam}: {ratio:.3f} ({case})", end="")
    print()


def _note(family, ratio, case):
    if ratio > _WORST.get(family, (-1.0, ""))[0]:
        _WORST[family] = (ratio, case)


@pytest.fixture
def entries(monkeypatch):
    """The entry points reached through _hip.call, in order."""
    seen, real = [], _hip.call

    def call(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_hip, "call", call)
    return seen


@functools.lru_cache(maxsize=None)
def _data(B, C, heads, H, W):
    """Operands and float64 references of one problem; every chunk, layout and alignment of it runs on the same values."""
    qkv, scale, temp, wout = mm.operands(SEED, f"C{C}h{heads}{H}x{W}", B, C, heads, H, W)
    q, k = qkv[:, :C].double(), qkv[:, C:2 * C].double()
    return qkv, scale, temp, wout, mm.gram_records_f64(q, k, heads), bm.attention(q, k, temp, heads)


def _place(g, t, how):
    """t between NaN bands with SLACK floats between the images; how = "off1": starting one float off 16-byte alignment,
    "bs2": batch stride % 4 == 2."""
    if not how:
        return g.inp(t, SLACK)
    off, slack = (1, SLACK) if how == "off1" else (0, SLACK - 2)
    B, per = t.shape[0], t[0].numel()
    assert per % 4 == 0
    bs = per + slack
    buf = torch.full((2 * guards.PAD + off + (B - 1) * bs + per,), float("nan"), device=g.dev)
    view = buf.as_strided(t.shape, (bs,) + tuple(t.stride()[1:]), guards.PAD + off)
    view.copy_(t)
    g.ins.append(buf)
    assert (view.data_ptr() % 16 == 4) == (how == "off1") and (bs % 4 == 2) == (how == "bs2")
    return view


def _fold(g, qv, B, C, heads, nchunk, tg, wg, part_init=None, **kw):
    """ops.mdta_fold with part, gsum, attn and the folded matrix at exactly their sizes between sentinels."""
    c = C // heads
    rec = c * c + 2 * c
    part, gsum = g.out("part", (B * heads * nchunk * rec,)), g.out("gsum", (B * heads * rec,))
    attn = g.out("attn", (B, heads, c, c))
    mfold = g.out("mfold", (B * (ops.mfold_frag_numel(C) if kw.get("frag") else ops.mfold_numel(C)),))
    mfold.zero_()
    if part_init is not None:
        part.copy_(part_init.reshape(-1))
    ops.mdta_fold(qv, part, gsum, tg, wg, mfold, C, heads, attn=attn, **kw)
    g.check()
    return part.cpu(), gsum.cpu(), attn.cpu(), mfold.cpu()


def _gram(g, qv, case, tg, wg, scale):
    """One Gram + finalize launch sequence of the case, twice into fresh workspaces: every element of part written, gsum the
    fixed-order sum of part, no NaN anywhere, both runs bit-identical.  Returns (summed records [B][heads][rec], attention)."""
    B, C, heads, N = case.B, case.C, case.heads, case.H * case.W
    nchunk, rec = ops.mdta_plan(B, C, heads, N)[1:]
    assert nchunk == -(-N // case.chunk)
    runs = [_fold(g, qv, B, C, heads, nchunk, tg, wg, gram_scale=scale, tm=case.tm) for _ in range(2)]
    part, gsum, attn, mfold = runs[0]
    assert not guards.has_nan(part) and not bool((part == guards.SENTINEL).any()), "a record element was not written"
    for t in (gsum, attn, mfold):
        clean(t)
    assert mm.same_bits(gsum, mm.reduce_f32(part.view(B * heads, nchunk, rec), nchunk).view(-1)), "gsum is not the fixed-order sum of part"
    for a, b in zip(*runs):
        assert mm.same_bits(a, b), "the second launch differs"
    return gsum.view(B, heads, rec).double(), attn.double()


@pytest.mark.parametrize("case", mm.CASES, ids=mm.case_id)
def test_gram_plan(dev, monkeypatch, entries, case):
    B, C, heads, H, W = case.B, case.C, case.heads, case.H, case.W
    N = H * W
    cls = mm.case_class(case)
    ring = cls.family.startswith("ring")
    assert cls.zsplit == 8 and (ring or not case.tm)
    qkv, scale, temp, wout, ref, aref = _data(B, C, heads, H, W)
    ymax = float(ref.abs().max())
    # the yardstick: the same records in float32 torch on the device
    qd = qkv[:, :2 * C].to(dev)
    e_32 = float((mm.gram_records(qd[:, :C], qd[:, C:], heads).double().cpu() - ref).abs().max())
    layout = qkv.clone()
    if case.tm:
        layout[:, :2 * C] = bm.qk_to_tm(qkv[:, :2 * C])
    monkeypatch.setattr(ops, "mdta_plan", mm.explicit_plan(case.chunk))
    g = Guards(dev)
    qv, tg, wg = _place(g, layout, case.how), g.inp(temp), g.inp(wout)
    assert (qv.data_ptr() % 16 == 0 and qv.stride(0) % 4 == 0) == (not case.how)

    rec32, a32 = _gram(g, qv, case, tg, wg, None)
    assert entries[:2] == ["irm_mdta_gram_tm_f32" if case.tm else "irm_mdta_gram_f32", "irm_mdta_finalize_f32"]
    e = float((rec32 - ref).abs().max())
    bar = bm.K * e_32 + bm.F * ymax
    ea = float((a32 - aref).abs().max())
    print(f"\n{mm.case_id(case)} {cls.family} {cls.state}: records e {e:.3e} e_32 {e_32:.3e} max|ref| {ymax:.3e} e / bar {e / bar:.3f}; "
          f"attn {ea:.2e}", end="")
    _note(cls.family + (" tile-major" if case.tm else ""), e / bar, mm.case_id(case))
    assert bm.passes(e, e_32, ymax)
    assert ea <= ATTN_TOL
    if not ring:
        return
    del entries[:]
    rec16, a16 = _gram(g, qv, case, tg, wg, g.inp(scale))
    assert entries[0] == ("irm_mdta_gram_tm_f16x3_f32" if case.tm else "irm_mdta_gram_f16x3_f32")
    e32, e16 = e / ymax, float((rec16 - ref).abs().max()) / ymax
    ea16 = float((a16 - aref).abs().max())
    print(f"; f16x3 e16 {e16:.3e} e32 {e32:.3e} e16 / bar {e16 / (2 * e32 + 2e-7):.3f}; attn {ea16:.2e}", end="")
    _note(cls.family + " f16x3" + (" tile-major" if case.tm else ""), e16 / (2 * e32 + 2e-7), mm.case_id(case))
    assert e16 <= 2 * e32 + 2e-7
    assert ea16 <= ATTN_TOL


@pytest.mark.parametrize("nchunk", mm.REDUCE_NCHUNK)
@pytest.mark.parametrize("C,heads", [(48, 1), (32, 2)])
def test_reduce_alone(dev, C, heads, nchunk):
    """mdta_reduce_kernel on synthetic records (no Gram launch): Gram entries in +-1000, squared norms in 1 .. 1000."""
    B, c = 2, C // heads
    rec = c * c + 2 * c
    part = synth.uniform(SEED, f"red{C}n{nchunk}", (B * heads, nchunk, rec), -1000.0, 1000.0)
    part[..., c * c:] = synth.uniform(SEED, f"redn{C}n{nchunk}", (B * heads, nchunk, 2 * c), 1.0, 1000.0)
    ref = part.double().sum(1)
    e_32 = float((part.to(dev).sum(1).double().cpu() - ref).abs().max())
    g = Guards(dev)
    qv = g.inp(torch.full((B, 3 * C, 8, 8), float("nan")), SLACK)          # its shape only: nothing reads it
    tg, wg = g.inp(synth.uniform(SEED, "redt", (heads,), 2.0, 6.0)), g.inp(synth.uniform(SEED, f"redw{C}", (C, C), -0.3, 0.3))
    _, gsum, attn, mfold = _fold(g, qv, B, C, heads, nchunk, tg, wg, part_init=part, nchunk_ready=nchunk)
    clean(gsum), clean(attn), clean(mfold)
    gsum = gsum.view(B * heads, rec)
    assert mm.same_bits(gsum, mm.reduce_f32(part, nchunk))
    e, ymax = float((gsum.double() - ref).abs().max()), float(ref.abs().max())
    print(f"\nreduce c{c} nchunk {nchunk}: e {e:.3e} e_32 {e_32:.3e} e / bar {e / (bm.K * e_32 + bm.F * ymax):.3f}", end="")
    _note("reduce", e / (bm.K * e_32 + bm.F * ymax), f"c{c} nchunk {nchunk}")
    assert bm.passes(e, e_32, ymax)


@functools.lru_cache(maxsize=None)
def _fin_data(B, C, heads):
    qkv, _, temp, wout = mm.operands(SEED, f"fin{C}h{heads}", B, C, heads, 8, 8)
    q, k = qkv[:, :C].double(), qkv[:, C:2 * C].double()
    return mm.gram_records_f64(q, k, heads).float(), temp, wout, bm.attention(q, k, temp, heads)


def _unpack(layout, mfold, B, C):
    if layout == "frag":
        return _hip.unpack_mfold_frag(mfold, B, C)
    return mm.unpack_mfold_split(mfold, B, C) if layout == "split" else bm.unpack_mfold(mfold, B, C)


@pytest.mark.parametrize("layout", ["packed", "split", "frag"])
@pytest.mark.parametrize("B,C,heads,zsplit", mm.FINALIZE_CASES)
def test_finalize_row_split(dev, entries, B, C, heads, zsplit, layout):
    """mdta_finalize_kernel at every row split (no Gram launch: one float64-derived record per (image, head), N = 64): the
    attention matrix, the folded matrix in all three layouts, and image 0 byte for byte what a launch of that image alone
    (zsplit = 8) writes."""
    assert mm.plan_class(B, C, heads, 64, mm.WHOLE).zsplit == zsplit and mm.plan_class(1, C, heads, 64, mm.WHOLE).zsplit == 8
    part, temp, wout, aref = _fin_data(B, C, heads)
    kw = dict(split=layout == "split", frag=layout == "frag", nchunk_ready=1)
    g = Guards(dev)
    tg, wg = g.inp(temp), g.inp(wout)

    def run(nb):
        qv = g.inp(torch.full((nb, 3 * C, 8, 8), float("nan")), SLACK)
        _, gsum, attn, mfold = _fold(g, qv, nb, C, heads, 1, tg, wg, part_init=part[:nb], **kw)
        assert mm.same_bits(gsum, part[:nb].reshape(-1) + 0.0)              # one record: ((p + 0) + 0) + 0
        return clean(attn), clean(mfold)
    attn, mfold = run(B)
    assert entries[-1] == {"packed": "irm_mdta_finalize_f32", "split": "irm_mdta_finalize_f16x3_f32",
                           "frag": "irm_mdta_finalize_frag_f16x3_f32"}[layout] and len(entries) == 1
    ea = float((attn.double() - aref).abs().max())
    mref = torch.stack([wout.double() @ torch.block_diag(*attn[i].double()) for i in range(B)])
    em, mmax = float((_unpack(layout, mfold, B, C).double() - mref).abs().max()), max(1.0, float(mref.abs().max()))
    print(f"\nfinalize B{B} C{C} h{heads} zsplit {zsplit} {layout}: attn {ea:.2e} ({ea / ATTN_TOL:.3f} of the bar)  "
          f"folded {em:.2e} ({em / (MFOLD_TOL * mmax):.3f} of the bar)", end="")
    _note("finalize attention", ea / ATTN_TOL, f"B{B} C{C} h{heads} {layout}")
    _note("finalize folded matrix", em / (MFOLD_TOL * mmax), f"B{B} C{C} h{heads} {layout}")
    assert ea <= ATTN_TOL
    assert em < MFOLD_TOL * mmax
    attn1, mfold1 = run(1)
    assert mm.same_bits(attn[:1], attn1) and mm.same_bits(mfold[:mfold1.numel()], mfold1), "the row split reached the values"
