"""Argument checks of the MDTA Gram / finalize entry points and of irm_gemm1x1_*: one bad argument at a time, every
call must return IRM_EINVAL (-1) before it touches HIP.  The pointers are made-up addresses that nothing dereferences;
the calls run in ONE child process that sees no GPU, so a check that went missing shows as a launch error (-2) there
instead of a kernel started on invented addresses."""
import json
import os
import subprocess
import sys

import pytest

from irm_amd import _hip

P = 1 << 20                                   # a 16-byte aligned, non-null "pointer"
_CODES = {_hip._P: "P", _hip._L: "L", _hip._I: "I", _hip._F: "F"}

# ---- Gram entries: (qkv, bs, [scale,] part, B, C, heads, N, chunk, stream); c = C / heads = 48, N = 256
GRAM = {"irm_mdta_gram_f32": dict(scale=False, ring_only=False, n_mult=0),
        "irm_mdta_gram_tm_f32": dict(scale=False, ring_only=True, n_mult=256),
        "irm_mdta_gram_f16x3_f32": dict(scale=True, ring_only=True, n_mult=64),
        "irm_mdta_gram_tm_f16x3_f32": dict(scale=True, ring_only=True, n_mult=256)}


def _gram_args(scale, qkv=P, bs=3 * 96 * 256, sc=P, part=P, B=1, C=96, heads=2, N=256, chunk=64):
    return [qkv, bs] + ([sc] if scale else []) + [part, B, C, heads, N, chunk, 0]


def _gram_cases():
    for name, k in GRAM.items():
        bad = [("null_qkv", dict(qkv=0)), ("null_part", dict(part=0))]
        if k["scale"]:
            bad.append(("null_scale", dict(sc=0)))
        for f in ("B", "C", "heads", "N", "chunk"):
            bad += [(f"{f}_zero", {f: 0}), (f"{f}_negative", {f: -1})]
        bad += [("C_not_a_multiple_of_heads", dict(heads=5)), ("chunk_not_a_multiple_of_64", dict(chunk=96)),
                ("B_65536", dict(B=65536))]
        if k["ring_only"]:
            bad += [("c_32", dict(C=64)), ("c_64", dict(C=128)), ("bs_not_a_multiple_of_4", dict(bs=3 * 96 * 256 + 2)),
                    ("qkv_off_16_bytes", dict(qkv=P + 4))]
        else:
            bad.append(("c_40", dict(C=40, heads=1)))
        if k["n_mult"] >= 64:
            bad.append(("N_not_a_multiple_of_64", dict(N=160)))
        if k["n_mult"] == 256:
            bad.append(("N_not_a_multiple_of_256", dict(N=320)))
        for tag, kw in bad:
            yield f"{name}-{tag}", name, _gram_args(k["scale"], **kw)


# ---- finalize entries: (part, gsum, temperature, wout, mfold, attn, B, C, heads, nchunk, stream)
FINALIZE = ("irm_mdta_finalize_f32", "irm_mdta_finalize_f16x3_f32", "irm_mdta_finalize_frag_f16x3_f32")


def _fin_args(ptrs=(P, P, P, P, P), B=1, C=96, heads=2, nchunk=4):
    return list(ptrs) + [0, B, C, heads, nchunk, 0]


def _fin_cases():
    for name in FINALIZE:
        bad = [(f"null_{n}", dict(ptrs=tuple(0 if j == i else P for j in range(5))))
               for i, n in enumerate(("part", "gsum", "temperature", "wout", "mfold"))]
        for f in ("B", "C", "heads", "nchunk"):
            bad.append((f"{f}_zero", {f: 0}))
        bad += [("C_not_a_multiple_of_heads", dict(heads=5)), ("B_times_heads_65536", dict(B=32768))]
        if "frag" in name:
            bad.append(("C_40", dict(C=40, heads=1)))
        for tag, kw in bad:
            yield f"{name}-{tag}", name, _fin_args(**kw)


# ---- irm_gemm1x1_*: (wp, w_bs, x, x_bs, y, y_bs, res, r_bs, bias, stats, lnw, lnb, ln_mode, act, B, M, K, N, ct, ygroups,
#                      stats_out, eps, res_scale, stream)
def _gemm_args(res=0, ln=0, ln_mode=0, act=0, ct=3):
    M = K = 48
    N = 256
    return [P, 0, P, K * N, P, M * N, res, M * N if res else 0, 0, ln, ln, ln, ln_mode, act, 1, M, K, N, ct, 1, 0, 1e-5, 0, 0]


def _gemm_cases():
    for name in ("irm_gemm1x1_f32", "irm_gemm1x1_f16x3_f32"):
        bad = [(f"ct_{ct}", dict(ct=ct)) for ct in (0, 2, 5, 7, 10)]
        bad += [("ln_mode_3", dict(ln=P, ln_mode=3)), ("act_4", dict(act=4))]
        if "f16x3" in name:                 # (the exact entry takes a residual behind a LayerNorm on its guarded kernel)
            bad.append(("residual_with_layernorm", dict(res=P, ln=P, ln_mode=1)))
        for tag, kw in bad:
            yield f"{name}-{tag}", name, _gemm_args(**kw)


CASES = list(_gram_cases()) + list(_fin_cases()) + list(_gemm_cases())

_CHILD = r"""
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
T = {"P": C.c_void_p, "L": C.c_long, "I": C.c_int, "F": C.c_float}
out = []
for name, codes, args in json.load(sys.stdin):
    f = getattr(lib, name)
    f.argtypes = [T[c] for c in codes]
    f.restype = C.c_int
    out.append(f(*args))
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def status():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    spec = [[name, "".join(_CODES[t] for t in _hip.SIGNATURES[name]), args] for _, name, args in CASES]
    for name, codes, args in spec:
        assert len(codes) == len(args), name
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _CHILD, _hip.LIB_PATH], input=json.dumps(spec), env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rcs = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(rcs) == len(CASES)
    return {cid: rc for (cid, _, _), rc in zip(CASES, rcs)}


@pytest.mark.parametrize("cid", [cid for cid, _, _ in CASES])
def test_entry_rejects_bad_argument(status, cid):
    assert status[cid] == -1
