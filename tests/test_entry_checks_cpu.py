"""Argument checks of the MDTA Gram / finalize entry points, of irm_gemm1x1_* and of the frame-side entries (tiler,
metrics, resize, NIQE): one bad argument at a time, every call must return IRM_EINVAL (-1) before it touches HIP.  The
pointers are made-up addresses that nothing dereferences; the calls run in ONE child process that sees no GPU, so a check that went missing shows as a launch error (-2) there
instead of a kernel started on invented addresses."""
import json
import os
import subprocess
import sys

import pytest

from irm_amd import _hip

P = 1 << 20                                   # a 16-byte aligned, non-null "pointer"
_CODES = {_hip._P: "P", _hip._L: "L", _hip._I: "I", _hip._F: "F", _hip._D: "D"}
_SIGNATURES = {**_hip.SIGNATURES, **_hip.SIGNATURES_FRAMES}

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


# ---- frame-side entries (tiler, metrics, resize, NIQE): a valid argument list by name, one field replaced per case.
# The shapes are the guard-band tests': a 37 x 51 x 3 frame, 32-pixel tiles padded to 40.
BIG = 1 << 40                                 # a workspace size in words that is never the short one
HWC_OVER = dict(H=32768, W=32768, C=3)        # 3 * 2^30 values > 2^31 - 1


def _zero_neg(*fields):
    return [(f"{f}_{tag}", {f: v}) for f in fields for tag, v in (("zero", 0), ("negative", -1))]


def _nulls(*fields):
    return [(f"null_{f}", {f: 0}) for f in fields]


_TILE = dict(H=37, W=51, C=3, th=32, tw=32, ph=40, pw=40, T=4)
_EXTRACT_BAD = (_zero_neg("H", "W", "C", "T", "th", "tw")
                + [("ph_below_th", dict(ph=31)), ("pw_below_tw", dict(pw=31)),
                   ("th_above_H", dict(th=38)), ("tw_above_W", dict(tw=52, pw=56)),
                   ("reflect_rows_not_below_tile", dict(th=8, ph=16)), ("reflect_cols_not_below_tile", dict(tw=8, pw=16))])
_BLEND = dict(H=37, W=51, Co=3, Cp=3, th=32, tw=32, ph=40, pw=40, ps=32, T=4)
_BLEND_BAD = (_zero_neg("H", "W", "Co", "T", "th", "tw")
              + [("Cp_below_Co", dict(Cp=2)), ("ph_below_th", dict(ph=31)), ("pw_below_tw", dict(pw=31)),
                 ("th_above_ps", dict(th=33)), ("tw_above_ps", dict(tw=33))])
_SCALED_BAD = [("scale_0", dict(scale=0)), ("scale_9", dict(scale=9)),
               ("H_scale_above_2p20", dict(H=(1 << 19) + 1, scale=2)), ("W_scale_above_2p20", dict(W=(1 << 19) + 1, scale=2)),
               ("window_index_2p31", dict(ps=46341))]
_FRAMES_BAD = [("is_u16_2", dict(is_u16=2)), ("K_65536", dict(K=65536)), ("C_2", dict(C=2)), ("HWC_above_int", HWC_OVER)]

FRAME = {
    "irm_tile_extract": (
        dict(img=P, is_u16=0, origins=P, noise=0, tiles=P, **_TILE, mean=0.0, inv_std=1.0, pad_zero=0, stream=0),
        _nulls("img", "origins", "tiles") + _EXTRACT_BAD),
    "irm_tile_extract_f32": (
        dict(img=P, range=P, origins=P, noise=0, tiles=P, **_TILE, pad_zero=0, stream=0),
        _nulls("img", "range", "origins", "tiles") + _EXTRACT_BAD),
    "irm_window_blend": (
        dict(pred=P, origins=P, window=P, out=P, is_u16=0, target=0, sse=0, **_BLEND, post_scale=1.0, post_shift=0.0,
             stream=0),
        _nulls("pred", "origins", "window", "out") + _BLEND_BAD),
    "irm_window_blend_scaled": (
        dict(pred=P, origins=P, window=P, out=P, is_u16=0, target=0, sse=0, **_BLEND, scale=3, post_scale=1.0,
             post_shift=0.0, stream=0),
        _nulls("pred", "origins", "window", "out") + _BLEND_BAD + _SCALED_BAD),
    "irm_window_blend_f32": (
        dict(pred=P, origins=P, window=P, out=P, range=P, **_BLEND, scale=3, stream=0),
        _nulls("pred", "origins", "window", "out", "range") + _BLEND_BAD + _SCALED_BAD),
    # 1 x 2 tiles of 16 rows x 64 pixels, K = 2: 8 workspace words
    "irm_frame_metrics": (
        dict(pred=P, target=P, is_u16=0, K=2, H=37, W=51, C=3, data_range=255.0, sse=P, ssim=P, ws=P, ws_words=BIG, stream=0),
        _nulls("pred", "target", "sse", "ssim", "ws") + _zero_neg("K", "H", "W", "C", "data_range") + _FRAMES_BAD
        + [("H_6", dict(H=6)), ("W_6", dict(W=6)), ("data_range_nan", dict(data_range=float("nan"))),
           ("short_workspace", dict(ws_words=7))]),
    "irm_frame_metrics_basicsr": (
        dict(pred=P, target=P, is_u16=0, K=2, H=37, W=51, C=3, crop_border=4, test_y_channel=0, bgr=0, sse=P, ssim=P,
             ws=P, ws_words=BIG, stream=0),
        _nulls("pred", "target", "sse", "ssim", "ws") + _zero_neg("K", "H", "W", "C") + _FRAMES_BAD
        + [("test_y_channel_2", dict(test_y_channel=2)), ("bgr_2", dict(bgr=2)), ("crop_border_negative", dict(crop_border=-1)),
           ("crop_border_16385", dict(H=40000, W=40000, C=1, crop_border=16385)),
           ("cropped_H_10", dict(H=18)), ("cropped_W_10", dict(W=18)), ("short_workspace", dict(ws_words=7))]),
    # shrinking by 2: 10 taps per output coordinate; enlarging: 6
    "irm_imresize_bicubic": (
        dict(src=P, is_u16=0, out=P, out_float=0, wh=P, ih=P, ww=P, iw=P, K=2, H=37, W=51, C=3, s=2, shrink=1, stream=0),
        _nulls("src", "out", "wh", "ih", "ww", "iw") + _zero_neg("K", "H", "W", "C", "s") + _FRAMES_BAD
        + [("out_float_2", dict(out_float=2)), ("shrink_2", dict(shrink=2)), ("s_1", dict(s=1)), ("s_5", dict(s=5)),
           ("H_below_support", dict(H=9)), ("W_below_support", dict(W=9)),
           ("H_below_support_enlarging", dict(H=5, shrink=0)), ("W_below_support_enlarging", dict(W=5, shrink=0)),
           ("H_32769", dict(H=32769, W=16, C=1)), ("W_32769", dict(H=16, W=32769, C=1)),
           ("output_above_int", dict(H=32768, W=32768, C=1, s=4, shrink=0))]),
    # 2 x 3 blocks of 96 x 96, K = 2: 432 feature words
    "irm_niqe_features": (
        dict(frames=P, is_u16=0, K=2, H=200, W=300, C=3, crop_border=0, bgr=0, window=P, table=P, feat=P, feat_words=BIG,
             stream=0),
        _nulls("frames", "window", "table", "feat") + _zero_neg("K", "H", "W", "C") + _FRAMES_BAD
        + [("bgr_2", dict(bgr=2)), ("crop_border_negative", dict(crop_border=-1)),
           ("crop_border_16385", dict(H=40000, W=40000, C=1, crop_border=16385)),
           ("cropped_H_95", dict(H=95)), ("cropped_W_95", dict(W=95)), ("one_block", dict(H=100, W=100)),
           ("short_feat_words", dict(feat_words=431))]),
}


def _frame_cases():
    for name, (good, bad) in FRAME.items():
        for tag, kw in bad:
            assert set(kw) <= set(good), (name, tag)
            yield f"{name}-{tag}", name, list({**good, **kw}.values())


CASES = list(_gram_cases()) + list(_fin_cases()) + list(_gemm_cases()) + list(_frame_cases())

_CHILD = r"""
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
T = {"P": C.c_void_p, "L": C.c_long, "I": C.c_int, "F": C.c_float, "D": C.c_double}
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
    spec = [[name, "".join(_CODES[t] for t in _SIGNATURES[name]), args] for _, name, args in CASES]
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
