"""Model of the MDTA core's launch plans (csrc/mdta.hip): which kernel a Gram launch takes and which of its states it runs,
the float64 records it must produce, the float32 sum its reduction must produce bit for bit, and the cases
tests/test_gpu_mdta_plans.py runs and tests/test_mdta_plans_cpu.py ties production plans to.

The states, as the kernels define them:

  ring (mdta_gram_ring_kernel / mdta_gram_f16x3_kernel, 3-slot LDS-DMA ring): workgroup j of an (image, head) owns the
  S_j = ceil((N / BP - j) / nchunk) pixel blocks j, j + nchunk, ...  S = 1, 2: the prologue alone fills the ring; S = 3: the
  first in-loop issue; S = 4 .. 6: every slot that is reused is reused once; S >= 7: a slot is reused a second time, the
  steady state of every production plan.  The S_j of one launch differ by at most one (`uneven`).

  guarded (mdta_gram_kernel<SB, VEC>): nchunk contiguous chunks; chunk_id > 0 needs nchunk >= 2, a chunk between two others
  nchunk >= 3; the last chunk is full or partial, and a partial one ends on a 64-pixel step of the sweep or inside one.

  finalize: the output rows of the folded matrix are split over zsplit workgroups per (image, head).

Plain functions and tuples, no fixtures and no tests."""
from collections import namedtuple

import torch

#: (kernel family, the states one launch of it runs, row split of the finalize kernel)
PlanClass = namedtuple("PlanClass", "family state zsplit")


def explicit_plan(chunk):
    """A stand-in for ops.mdta_plan that answers `chunk` for every problem (monkeypatch.setattr(ops, "mdta_plan", ...)): the
    launch still goes through ops.mdta_fold and its asserts."""
    def plan(B, C, heads, N):
        c = C // heads
        return chunk, -(-N // chunk), c * c + 2 * c
    return plan


def finalize_lds(C, heads, zsplit):
    """Bytes of LDS of mdta_finalize_kernel: the record and this workgroup's rows of project_out."""
    c = C // heads
    return 4 * (c * c + 2 * c + -(-C // zsplit) * c)


def zsplit_of(B, C, heads):
    """mdta_finalize's loop: 8, halved while that is more than 512 workgroups and the larger row block still fits 64 KiB."""
    z = 8
    while z > 1 and B * heads * z > 512 and finalize_lds(C, heads, z // 2) <= 64 * 1024:
        z //= 2
    return z


def ring_stages(c, N, chunk):
    """S_j of every workgroup of one (image, head) of a ring launch."""
    bp = 64 if c == 48 else 32
    nchunk, nblocks = -(-N // chunk), N // bp
    return [-(-(nblocks - j) // nchunk) if j < nblocks else 0 for j in range(nchunk)]


def _bucket(S):
    return S if S <= 3 else 4 if S <= 6 else 7


def plan_class(B, C, heads, N, chunk, aligned=True):
    """The PlanClass of irm_mdta_gram_f32 + finalize on this problem; `aligned`: qkv and its batch stride are multiples of 16
    bytes (what the dispatch cannot know from the sizes)."""
    c = C // heads
    nchunk = -(-N // chunk)
    vec = N % 4 == 0 and aligned
    if vec and N % 64 == 0 and c in (48, 96):
        S = ring_stages(c, N, chunk)
        family, state = "ring3" if c == 48 else "ring6", (tuple(sorted({_bucket(s) for s in S})), len(set(S)) > 1)
    else:
        sb = 3 if c % 48 == 0 else 2 if c % 32 == 0 else 1
        last = N - (nchunk - 1) * chunk
        family = f"guarded({sb}, {vec})"
        state = (min(nchunk, 3), "full" if last == chunk else "partial", "0" if last % 64 == 0 else "other")
    return PlanClass(family, state, zsplit_of(B, C, heads))


def gram_records(q, k, heads):
    """[B][heads][c*c + 2c] summed record (G = q k^T, then |q_i|^2, then |k_j|^2) of q, k [B][C][...] in their own dtype, on
    their own device."""
    B, C = q.shape[:2]
    c = C // heads
    q, k = q.reshape(B, heads, c, -1), k.reshape(B, heads, c, -1)
    return torch.cat([(q @ k.transpose(-1, -2)).reshape(B, heads, c * c), (q * q).sum(-1), (k * k).sum(-1)], -1)


def gram_records_f64(q, k, heads):
    """What gsum must hold, in float64."""
    return gram_records(q.double(), k.double(), heads)


def reduce_f32(part, nchunk):
    """mdta_reduce_kernel's sum of float32 records [...][nchunk][rec] -> [...][rec]: wave w adds the chunks w, w + 4, ... in
    order to 0, then ((s0 + s1) + s2) + s3.  (The unrolled-by-16 loop adds in the same order.)"""
    assert part.dtype == torch.float32 and part.shape[-2] == nchunk
    s = []
    for w in range(4):
        acc = torch.zeros(part.shape[:-2] + part.shape[-1:], dtype=torch.float32, device=part.device)
        for ch in range(w, nchunk, 4):
            acc = acc + part[..., ch, :]
        s.append(acc)
    return ((s[0] + s[1]) + s[2]) + s[3]


def same_bits(a, b):
    """Bitwise equality of two float32 tensors (NaN and the sign of zero included)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def unpack_mfold_split(mf, nb, C):
    """irm_mdta_finalize_f16x3_f32's [mtile][stage][hi|lo][lane = 16 g + m][j] halves (part[16 mtile + m][16 stage + 4 j + g],
    _hip.pack_gemm_weight_split's order) -> hi + lo as float32 [nb][C][C]; C % 16 == 0."""
    mt = C // 16
    h = mf.detach().cpu().contiguous().view(torch.float16).view(nb, mt, mt, 2, 4, 16, 4).float()      # [mt][st][2][g][m][j]
    return (h[:, :, :, 0] + h[:, :, :, 1]).permute(0, 1, 4, 2, 5, 3).reshape(nb, C, C)


def operands(seed, tag, B, C, heads, H, W):
    """(qkv, gram_scale, temperature, wout) of one case from synth.uniform(seed, ...): q, k uniform in +-1 scaled per channel by
    a bound in 0.5 .. 40 and gram_scale = 2^14-ish / bound, as tests/test_gpu_ops.py::test_mdta_gram_f16x3 builds them; v
    holds NaN: the Gram pass and the finalize must not read it."""
    from irm_amd import synth
    bound = synth.uniform(seed, tag + "b", (2 * C,), 0.5, 40.0)
    qkv = synth.uniform(seed, tag + "q", (B, 3 * C, H, W), -1.0, 1.0)
    qkv[:, :2 * C] *= bound.view(1, 2 * C, 1, 1)
    qkv[:, 2 * C:] = float("nan")
    scale = torch.pow(2.0, torch.floor(torch.log2(2.0 ** 14.8 / bound))).float()
    assert float((qkv[:, :2 * C].abs() * scale.view(1, -1, 1, 1)).max()) < 65504
    return qkv, scale, synth.uniform(seed, tag + "t", (heads,), 2.0, 6.0), synth.uniform(seed, tag + "w", (C, C), -0.3, 0.3)


# --------------------------------------------------------------------------- the cases
#: one Gram launch sequence: B images of C channels in `heads` heads on H x W pixels at an explicit chunk.  tm: q, k
#: tile-major.  how: "" (16-byte aligned, batch stride a multiple of 4 floats), "off1" (qkv starts one float off 16-byte
#: alignment) or "bs2" (batch stride % 4 == 2); both send irm_mdta_gram_f32 to the guarded kernel without float4 loads.
GramCase = namedtuple("GramCase", "C heads H W chunk tm how B", defaults=(False, "", 2))
WHOLE = 4096        # a chunk >= N of every case: one workgroup (ring) or one chunk (guarded) per (image, head)


def _gram_cases():
    out = []
    # ring, c = 48: S = 1, 2, 3, 4, 7 in one workgroup; (3, 2, 2), (4, 4, 3), (7, 7, 6); (25, 24); and the two classes of
    # production plans below the steady state: (2, 1) (40 x 56 pixels at chunk 128) and (5, 5, 4) (9 images of 64 x 64 at C = 192)
    for C, heads in ((48, 1), (96, 2)):
        out += [GramCase(C, heads, 8, W, WHOLE) for W in (8, 16, 24, 32, 56)]
        out += [GramCase(C, heads, 8, 56, 192), GramCase(C, heads, 8, 88, 256), GramCase(C, heads, 8, 160, 448),
                GramCase(C, heads, 56, 56, 1600), GramCase(C, heads, 8, 24, 128), GramCase(C, heads, 8, 112, 320)]
    # ring, c = 96: S = 2, 4, 8, 14; (4, 3, 3), (5, 5, 4); (10, 10, 9, 9), the production steady state with uneven workgroups
    for C, heads in ((96, 1), (192, 2)):
        out += [GramCase(C, heads, 8, W, WHOLE) for W in (8, 16, 32, 56)]
        out += [GramCase(C, heads, 8, 40, 128), GramCase(C, heads, 8, 56, 192), GramCase(C, heads, 8, 152, 320)]
    # tile-major: one workgroup, and chunk 448 (stages 3 x 64 or 3 x 32 pixels apart hop across the 256-pixel tiles)
    for C, heads in ((96, 2), (192, 2)):
        out += [GramCase(C, heads, 8, 32, WHOLE, True)]
        out += [GramCase(C, heads, 8, W, chunk, True) for W in (96, 160) for chunk in (WHOLE, 448)]
    # guarded kernel, c = 16, 32, 48, 96 = SB 1, 2, 3 and 3 with four sub-blocks
    for C, heads in ((32, 2), (64, 2), (96, 2), (192, 2)):
        out += [GramCase(C, heads, 8, 25, 64), GramCase(C, heads, 8, 25, 256)]                  # float4 loads; 4 chunks, last 8 px; one
        if C // heads < 48:
            out += [GramCase(C, heads, 8, 40, 64), GramCase(C, heads, 8, 40, 256)]              # 5 full chunks; full + 64 px
        out += [GramCase(C, heads, 9, 15, 64), GramCase(C, heads, 5, 7, 64)]                    # scalar loads; 3 chunks, last 7 px; one
        out += [GramCase(C, heads, 8, 25, 64, False, "off1"), GramCase(C, heads, 8, 25, 64, False, "bs2")]
    return out


CASES = _gram_cases()


def case_id(case):
    return f"C{case.C}h{case.heads}-{case.H}x{case.W}-chunk{case.chunk}" + ("-tm" if case.tm else "") + (f"-{case.how}" if case.how else "")


def case_class(case):
    return plan_class(case.B, case.C, case.heads, case.H * case.W, case.chunk, aligned=not case.how)


#: finalize alone: (B, C, heads, zsplit the product code must pick); the last is the largest LDS that launches (56 064 B)
FINALIZE_CASES = [(2, 384, 8, 8), (9, 384, 8, 4), (17, 384, 8, 2), (65, 96, 2, 2), (257, 48, 1, 1), (129, 96, 1, 2)]

#: reduce alone: below one round of the four waves; the unrolled loop entered by wave 0 only (13) and by all four (16); the
#: remainders of both loops
REDUCE_NCHUNK = [1, 3, 4, 5, 12, 13, 16, 17, 29]
