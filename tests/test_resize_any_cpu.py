"""The resize to any size (irm_amd/resize.py, csrc/resize_any.hip), the part that needs no GPU: the float64 statement
against the reference goldens (tools/gen_golden_resize_any.py), the tap tables, hand values, semantics and refusals, the
C ABI of include/irm_hip_resize.h against _hip.SIGNATURES_RESIZE with the entry's refusals before any launch, and the
Resize stage of utils.run_model_chain."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from irm_amd import _hip, deblurganv2, resize, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ["irm_resize_taps", "irm_unit_quantise"]
KERNELS = ("bicubic", "lanczos3", "bilinear")
KW = {"bicubic": 4.0, "lanczos3": 6.0, "bilinear": 2.0}
CFG = {"patch_size": 64, "patch_overlap": 16}
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "resize_any.json")) as f:
        return json.load(f)


def sources(golden):
    g = golden("sr_protocol")
    return {name: np.ascontiguousarray(g[f"hr_{name}"][:61, :83]) for name in ("random", "synth")}


# --------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("name", ["random", "synth"])
@pytest.mark.parametrize("key", ["s0750", "s0667", "s0900", "s0400", "s0300", "s1250", "s1500"])
def test_resize_host_vs_reference(golden, meta, key, name):
    """4 x the distance the generator recorded, and never above 1e-4: the level accepted at x3 of the protocol resize,
    where the reference builds its coordinates in fp32 - the same cause acts at these scales."""
    s = meta["scales"][key]
    ref = golden("resize_any")[f"{key}_{name}"]
    got = utils.resize_host(sources(golden)[name], scale=s)
    assert got.dtype == np.float64 and got.shape == ref.shape == (math.ceil(61 * s), math.ceil(83 * s), 3)
    err = float(np.abs(got - ref.astype(np.float64)).max())
    bound = 4 * meta["resize_host_vs_reference"][f"{key}_{name}"]
    print(f"resize_host x{s:g} {name}: max-abs vs reference {err:.3e} (bound {bound:.3e})")
    assert 0 < bound <= 1e-4 and err <= bound


# --------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [18, 25, 61, 83, 720, 1280])
def test_resize_taps_properties(n, kernel):
    outs = sorted({max(1, round(n * f)) for f in (1 / 8, 1 / 5, 0.3, 0.5, 2 / 3, 0.9, 1.0, 1.25, 1.5, 2.0, 3.0, 4.0)})
    ran = 0
    for out in outs:
        scale = out / n
        width = KW[kernel] / scale if scale < 1 else KW[kernel]
        p = math.ceil(width) + 2
        if n < p:
            with pytest.raises(ValueError, match="shorter"):
                utils.resize_taps(n, out, scale, kernel)
            continue
        ran += 1
        w, i = utils.resize_taps(n, out, scale, kernel)
        assert w.shape == i.shape == (out, p) and w.dtype == np.float64 and i.dtype == np.int64
        assert float(np.abs(w.sum(1) - 1.0).max()) <= 1e-14
        assert float(np.abs(w.astype(np.float32).astype(np.float64).sum(1) - 1.0).max()) <= 1e-6     # what the device sums
        assert int(i.min()) >= 0 and int(i.max()) < n
        # the reflected source indices of every row cover a contiguous range (what the kernel's LDS window relies on)
        srt = np.sort(i, axis=1)
        assert int(np.diff(srt, axis=1).max(initial=0)) <= 1
        # and so do those of any run of rows: tile_span is the size of that range
        for tow in (8, 32):
            for x0 in range(0, out, tow):
                u = np.unique(i[x0:x0 + tow])
                assert u[-1] - u[0] + 1 == len(u) <= resize.tile_span(i, tow)
    assert ran >= 6
    # without antialiasing a shrinking table keeps the kernel's own width
    w, i = utils.resize_taps(n, max(1, n // 3), 1 / 3, kernel, antialias=False)
    assert w.shape[1] == math.ceil(KW[kernel]) + 2


@pytest.mark.parametrize("n", [18, 25, 96, 97, 131])
@pytest.mark.parametrize("scale", [0.5, 1.0 / 3.0, 0.25, 2, 3, 4])
def test_resize_taps_are_the_old_table_at_its_factors(n, scale):
    try:
        w0, i0 = utils.resize_table(n, scale)
    except ValueError:
        with pytest.raises(ValueError, match="shorter"):
            utils.resize_taps(n, math.ceil(n * scale), scale)
        return
    w1, i1 = utils.resize_taps(n, w0.shape[0], scale)
    assert w1.shape == w0.shape and np.array_equal(i0, i1)
    assert np.array_equal(w0.astype(np.float32), w1.astype(np.float32))


def test_hand_values():
    w, i = utils.resize_taps(16, 32, 2.0, "bilinear")                     # P = 4: a zero tap on either side
    for x in (6, 7, 20, 21):
        nz = w[x] != 0
        assert nz.sum() == 2 and np.array_equal(np.diff(i[x][nz]), [1])
        want = (0.25, 0.75) if x % 2 == 0 else (0.75, 0.25)
        assert np.allclose(w[x][nz], want, rtol=0, atol=1e-15), (x, w[x])
        assert i[x][nz][0] == (x - 1) // 2 if x % 2 == 0 else i[x][nz][0] == x // 2
    w, i = utils.resize_taps(16, 8, 0.5, "bilinear")                      # the (1, 3, 3, 1) / 8 row
    for x in (2, 5):
        nz = w[x] != 0
        assert np.allclose(w[x][nz], np.array([1, 3, 3, 1]) / 8.0, rtol=0, atol=1e-15)
        assert np.array_equal(i[x][nz], 2 * x + np.arange(-1, 3))
    # lanczos3, enlarging by 4: phases 0.375 and 0.125 of an interior row against the closed form
    w, i = utils.resize_taps(32, 128, 4.0, "lanczos3")

    def lanczos(d):
        d = abs(d)
        return 1.0 if d == 0 else 0.0 if d >= 3 else 3 * math.sin(math.pi * d) * math.sin(math.pi * d / 3) / (math.pi * d) ** 2
    for x in (60, 61):                                                    # 0-based output coordinates
        u = (x + 1) / 4.0 + 0.5 * (1 - 1 / 4.0)                           # 1-based source coordinate
        raw = np.array([lanczos(u - (j + 1)) for j in i[x]])
        assert abs(raw.sum() - 1.0) < 0.02 and (raw != 0).sum() == 6
        assert np.allclose(w[x], raw / raw.sum(), rtol=0, atol=1e-15)
    assert {round(float((x + 1) / 4.0 + 0.375) % 1, 3) for x in (60, 61)} == {0.625, 0.875}


# --------------------------------------------------------------------------- semantics
def test_size_and_scale_forms(golden):
    """scale=s puts s into both tables, size=(oh, ow) puts out / in: 61 x 0.3 = 18.3 and 83 x 0.3 = 24.9, so both forms
    make a 19 x 25 frame but from other coordinates (19 / 61 = 0.3115, 25 / 83 = 0.3012).  Where out / in is the scale,
    the two forms are the same table."""
    img = sources(golden)["synth"]
    a, b = utils.resize_host(img, scale=0.3), utils.resize_host(img, size=(19, 25))
    assert a.shape == b.shape == (19, 25, 3)
    assert float(np.abs(a - b).max()) > 1e-3
    assert float(np.abs(a[:, :3] - b[:, :3]).max()) > 1e-4 and float(np.abs(a[:3] - b[:3]).max()) > 1e-4
    half = img[:60, :82]
    assert np.array_equal(utils.resize_host(half, scale=0.5), utils.resize_host(half, size=(30, 41)))
    assert np.array_equal(utils.resize_host(half, scale=0.5), utils.imresize_host(half, 0.5))
    # an axis may shrink while the other grows
    mixed = utils.resize_host(img, size=(40, 200), kernel="lanczos3")
    assert mixed.shape == (40, 200, 3)
    assert np.array_equal(utils.resize_host(img, size=(61, 83)), img / 255.0)          # scale 1: the frame itself


@pytest.mark.parametrize("kernel", KERNELS)
def test_grey_uint16_and_float32(golden, kernel):
    img = sources(golden)["synth"]
    kw = dict(size=(40, 100), kernel=kernel)
    full = utils.resize_host(img, **kw)
    grey = utils.resize_host(img[:, :, 1].copy(), **kw)
    assert grey.shape == (40, 100) and np.array_equal(grey, full[:, :, 1])
    assert np.array_equal(utils.resize_host(img[:, :, 1:2].copy(), **kw)[:, :, 0], grey)
    u16 = img.astype(np.uint16) * 257
    assert float(np.abs(utils.resize_host(u16, **kw) - full).max()) <= 1e-12
    f32 = img.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(utils.resize_host(f32, **kw), utils.resize_host(f32.astype(np.float64).astype(np.float32), **kw))
    assert float(np.abs(utils.resize_host(f32, **kw) - full).max()) <= 2.0 ** -24 * 4          # the fp32 rounding of v / 255
    x = f32.astype(np.float64)                                             # a float32 frame is taken as it is
    wh, ih = utils.resize_taps(61, 40, 40 / 61, kernel)
    ww, iw = utils.resize_taps(83, 100, 100 / 83, kernel)
    mid = sum(wh[:, p, None, None] * x[ih[:, p]] for p in range(wh.shape[1]))
    want = sum(ww[None, :, p, None] * mid[:, iw[:, p]] for p in range(ww.shape[1]))
    assert float(np.abs(utils.resize_host(f32, **kw) - want).max()) <= 1e-14
    # the out kinds
    q = utils.resize_host(img, out="same", **kw)
    assert q.dtype == np.uint8 and np.array_equal(q, np.round(np.clip(full, 0, 1) * 255).astype(np.uint8))
    q16 = utils.resize_host(u16, out="same", **kw)
    assert q16.dtype == np.uint16
    assert np.array_equal(q16, np.round(np.clip(utils.resize_host(u16, **kw), 0, 1) * 65535).astype(np.uint16))
    unit = utils.resize_host(img, out="unit", **kw)
    assert unit.dtype == np.float64 and np.array_equal(unit, np.clip(full, 0, 1))
    same = utils.resize_host(f32, out="same", **kw)
    assert same.dtype == np.float32 and np.array_equal(same, utils.resize_host(f32, **kw).astype(np.float32))


def test_overshoot_on_the_host():
    yy, xx = np.mgrid[0:30, 0:36]
    img = ((((yy // 3) + (xx // 3)) % 2) * 255).astype(np.uint8)[:, :, None].repeat(3, 2)
    f = utils.resize_host(img, scale=1.5, kernel="lanczos3")
    assert f.min() < -0.05 and f.max() > 1.05
    u = utils.resize_host(img, scale=1.5, kernel="lanczos3", out="unit")
    assert u.min() == 0.0 and u.max() == 1.0
    b = utils.resize_host(img, scale=1.5, kernel="bilinear")
    assert b.min() >= 0.0 and b.max() <= 1.0 + 1e-15


# --------------------------------------------------------------------------- refusals
def test_refusals(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library must not be called")
    monkeypatch.setattr(_hip, "call", boom)
    img = np.zeros((61, 83, 3), np.uint8)
    for kw in (dict(), dict(size=(10, 10), scale=0.5)):
        with pytest.raises(ValueError, match="exactly one"):
            utils.resize_host(img, **kw)
        with pytest.raises(ValueError, match="exactly one"):
            utils.Resize(**kw)
    for kw in (dict(scale=0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(scale="2")):
        with pytest.raises(ValueError, match="positive number"):
            utils.resize_host(img, **kw)
    for size in ((0, 5), (5,), (5, 6, 7), (2.5, 3), 7, "ab"):
        with pytest.raises(ValueError, match="two positive integers"):
            utils.resize_host(img, size=size)
    with pytest.raises(ValueError, match="shorter"):
        utils.resize_host(img, size=(6, 11), kernel="lanczos3")            # 6 x 61 / 6 = 61 -> 63 taps on a side of 61
    with pytest.raises(ValueError, match="shorter"):
        utils.resize_host(img[:5], scale=2)
    with pytest.raises(ValueError, match="shorter"):
        utils.resize_taps(17, 5, 0.25)
    for kernel in ("nearest", "Bicubic", None, 3):
        with pytest.raises(ValueError, match="kernel"):
            utils.resize_host(img, scale=0.5, kernel=kernel)
        with pytest.raises(ValueError, match="kernel"):
            utils.resize_taps(64, 32, 0.5, kernel)
    with pytest.raises(ValueError, match="positive number"):
        utils.resize_taps(64, 32, 0)
    with pytest.raises(ValueError, match="at least 1"):
        utils.resize_taps(64, 0, 0.5)
    with pytest.raises(ValueError, match="out must be"):
        utils.resize_host(img, scale=0.5, out="uint8")
    for bad in (img.astype(np.float64), img.astype(np.int16), torch.zeros(61, 83, 3, dtype=torch.uint8), "frame"):
        with pytest.raises(ValueError, match="uint8, uint16 or float32 numpy"):
            utils.resize_host(bad, scale=0.5)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        utils.resize_host(np.zeros((61, 83, 2), np.uint8), scale=0.5)
    # the device call: CPU tensors and numpy arrays, as imresize_device refuses them
    for t in (torch.zeros(61, 83, 3, dtype=torch.uint8), torch.zeros(61, 83, 3), torch.zeros(61, 83, dtype=torch.int16)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            utils.resize_device(t, scale=0.5)
        with pytest.raises(ValueError, match="no CPU fallback"):
            utils.resize_device([t, t], size=(30, 40))
    with pytest.raises(ValueError, match="torch tensors"):
        utils.resize_device(img, scale=0.5)
    with pytest.raises(ValueError, match="no frames"):
        utils.resize_device([], scale=0.5)
    with pytest.raises(ValueError, match="uint8, uint16 or float32 frames"):
        utils.resize_device(torch.zeros(61, 83, 3, dtype=torch.float64), scale=0.5)
    with pytest.raises(ValueError, match="uint8 or uint16 frames"):            # the protocol resize keeps its refusal
        utils.imresize_device(torch.zeros(61, 83, 3), 0.5)
    with pytest.raises(ValueError, match="out must be"):
        utils.resize_device(torch.zeros(61, 83, 3), scale=0.5, out="float32")
    assert sorted(utils.RESIZE_KERNELS) == sorted(KERNELS)


def test_tow_choice(monkeypatch):
    """The widest tile whose window fits the preferred 16 KiB - at 1/4 bicubic the 32 columns of irm_imresize_bicubic -,
    else the widest under the entry's 32 KiB; a narrower budget gives a narrower tile; what never fits is refused."""
    def spans_of(n, out, scale, kernel):
        w, i = utils.resize_taps(n, out, scale, kernel)
        return w.shape[1], {tow: resize.tile_span(i, tow) for tow in resize.RESIZE_TOWS}
    p, spans = spans_of(1280, 320, 0.25, "bicubic")
    assert p == 18 and spans[32] == 142 and resize._pick_tow(spans, 3) == (32, 142)          # the old kernel sizes for 143
    assert resize._pick_tow(spans_of(320, 1280, 4, "bicubic")[1], 3)[0] == 128
    p, spans = spans_of(3840, 480, 0.125, "lanczos3")
    assert p == 50 and spans[32] in range(290, 300)                      # 8 x about 300 x 3 floats = 28 KiB
    assert all(spans[a] > spans[b] for a, b in zip(resize.RESIZE_TOWS, resize.RESIZE_TOWS[1:]))
    assert resize._pick_tow(spans, 3) == (16, spans[16]) and 8 * spans[16] * 3 * 4 <= 16384 < 8 * spans[32] * 3 * 4
    assert resize._pick_tow(spans, 1) == (32, spans[32])
    monkeypatch.setattr(resize, "RESIZE_WINDOW_PREFERRED", 32768)
    assert resize._pick_tow(spans, 3) == (32, spans[32]) and resize._pick_tow(spans, 1) == (64, spans[64])
    monkeypatch.setattr(resize, "RESIZE_WINDOW_BYTES", 12288)
    assert resize._pick_tow(spans, 3) == (8, spans[8])
    monkeypatch.setattr(resize, "RESIZE_WINDOW_BYTES", 4096)
    with pytest.raises(ValueError, match="window"):
        resize._pick_tow(spans, 3)
    monkeypatch.undo()
    p, spans = spans_of(4096, 256, 1 / 16, "lanczos3")                    # the largest table the entry promises to take
    assert p == 98 <= resize.RESIZE_MAX_TAPS
    tow, ncol = resize._pick_tow(spans, 3)                                # nothing under 16 KiB: 15 x 16 + 98 = 338 columns
    assert tow == 16 and 8 * spans[8] * 3 * 4 > 16384 and 8 * ncol * 3 * 4 <= 32768


# --------------------------------------------------------------------------- C ABI
def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip.load()


def test_header_declares_the_symbols():
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('extern "C" {') < main.index('#include "irm_hip_resize.h"') < main.rindex("#ifdef __cplusplus")
    text = open(os.path.join(ROOT, "include", "irm_hip_resize.h")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_RESIZE)
    others = [v for k, v in vars(_hip).items() if k.startswith("SIGNATURES") and k != "SIGNATURES_RESIZE"]
    assert len(others) >= 11 and not set(_hip.SIGNATURES_RESIZE) & set().union(*others)
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b"}
    _lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_RESIZE[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_kernel_source_keeps_the_repository_rules():
    csrc = os.path.join(os.path.dirname(_hip.LIB_PATH), "csrc")
    src = open(os.path.join(csrc, "resize_any.hip")).read()
    assert re.findall(r'^#include "(\w+\.h)"', src, flags=re.M) == ["irm_frame.h"]
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", src, flags=re.M)
    assert "atomic" not in src.lower().replace("no atomics", "")
    old = open(os.path.join(csrc, "resize.hip")).read()
    for line in ("acc = fmaf(w[p], mid[r * rowv + c * C + ch], acc);", "const float v = fminf(fmaxf(acc, 0.0f), 1.0f) * a.range;",
                 "reinterpret_cast<T*>(a.out)[o] = (T)rintf(v);"):
        assert line in src and line in old, line                   # the two kernels spell the same chains


P = 1 << 20                                   # a 16-byte aligned, non-null "pointer"
_CODES = {_hip._P: "P", _hip._L: "L", _hip._I: "I", _hip._F: "F", _hip._D: "D"}
# 1280 x 720 -> 1920 x 1080, bicubic: 6 taps per axis; 64 output columns touch 45 source columns
_TAPS = dict(src=P, in_kind=0, out=P, out_kind=0, wh=P, ih=P, ww=P, iw=P, K=2, H=720, W=1280, C=3, OH=1080, OW=1920, PH=6,
             PW=6, tow=64, ncol_max=45, stream=0)
ENTRY = {
    "irm_resize_taps": (_TAPS, [(f"null_{f}", {f: 0}) for f in ("src", "out", "wh", "ih", "ww", "iw")]
                        + [(f"{f}_{tag}", {f: v}) for f in ("K", "H", "W", "C", "OH", "OW", "PH", "PW", "tow", "ncol_max")
                           for tag, v in (("zero", 0), ("negative", -1))]
                        + [("in_kind_3", dict(in_kind=3)), ("in_kind_negative", dict(in_kind=-1)),
                           ("out_kind_3", dict(out_kind=3)), ("out_kind_negative", dict(out_kind=-1)),
                           ("quantised_f32", dict(in_kind=2, out_kind=0)),
                           ("K_65536", dict(K=65536)), ("C_2", dict(C=2)), ("HWC_above_int", dict(H=32768, W=32768, C=3)),
                           ("PH_above_H", dict(H=5)), ("PW_above_W", dict(W=5, ncol_max=5)),
                           ("PH_129", dict(PH=129)), ("PW_129", dict(PW=129)),
                           ("H_32769", dict(H=32769, W=16, C=1, ncol_max=16)), ("W_32769", dict(H=16, PH=6, W=32769, C=1)),
                           ("output_above_int", dict(OH=32768, OW=32768)), ("OH_PH_above_int", dict(OH=1 << 25, OW=8, PH=128, C=1)),
                           ("tow_24", dict(tow=24)), ("tow_256", dict(tow=256)), ("tow_4", dict(tow=4)),
                           ("ncol_above_W", dict(W=40, ncol_max=41)),
                           ("window_does_not_fit", dict(ncol_max=342)), ("window_does_not_fit_grey", dict(C=1, ncol_max=1025))]),
    "irm_unit_quantise": (dict(src=P, out=P, is_u16=0, n=1000, stream=0),
                          [("null_src", dict(src=0)), ("null_out", dict(out=0)), ("is_u16_2", dict(is_u16=2)),
                           ("n_zero", dict(n=0)), ("n_negative", dict(n=-1)), ("n_above_grid", dict(n=1 << 40))]),
}
CASES = [(f"{name}-{tag}", name, list({**good, **kw}.values())) for name, (good, bad) in ENTRY.items() for tag, kw in bad]
#: what the last valid value of a limit still passes: these reach the launch, which fails without a device (-2)
EDGES = [("irm_resize_taps-window_fits", "irm_resize_taps", list({**_TAPS, "ncol_max": 341}.values())),
         ("irm_resize_taps-128_taps", "irm_resize_taps", list({**_TAPS, "PH": 128, "PW": 128}.values())),
         ("irm_resize_taps-f32_unit", "irm_resize_taps", list({**_TAPS, "in_kind": 2, "out_kind": 2}.values()))]

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
    """All calls in ONE child process that sees no GPU (tests/test_entry_checks_cpu.py): the pointers are made-up
    addresses that nothing dereferences, and a check that went missing shows as a launch error (-2)."""
    _lib()
    every = CASES + EDGES
    for tag, name, args in every:
        assert set(ENTRY[name][0]) and len(args) == len(_hip.SIGNATURES_RESIZE[name]), tag
    spec = [[name, "".join(_CODES[t] for t in _hip.SIGNATURES_RESIZE[name]), args] for _, name, args in every]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _CHILD, _hip.LIB_PATH], input=json.dumps(spec), env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rcs = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(rcs) == len(every)
    return {cid: rc for (cid, _, _), rc in zip(every, rcs)}


@pytest.mark.parametrize("cid", [cid for cid, _, _ in CASES])
def test_entry_rejects_bad_argument(status, cid):
    assert status[cid] == -1


@pytest.mark.parametrize("cid", [cid for cid, _, _ in EDGES])
def test_entry_takes_the_last_valid_value(status, cid):
    assert status[cid] != -1


# --------------------------------------------------------------------------- the chain
class Never(torch.nn.Module):
    def forward(self, t):
        raise AssertionError("the model must not run")


def test_resize_is_a_frozen_value():
    r = utils.Resize(size=[60, 84], kernel="lanczos3")
    assert r.size == (60, 84) and r.scale is None and r.antialias is True
    assert r == utils.Resize(size=(60, 84), kernel="lanczos3") and hash(r) == hash(utils.Resize(size=(60, 84), kernel="lanczos3"))
    with pytest.raises(Exception):
        r.scale = 2
    assert utils.Resize(scale=0.75).plan(40, 56) == (30, 42) and r.plan(40, 56) == (60, 84)
    for kw in (dict(scale=0), dict(size=(0, 4)), dict(scale=2, kernel="nearest")):
        with pytest.raises(ValueError):
            utils.Resize(**kw)


def test_chain_validates_resize_stages_before_any_gpu_call():
    m = Never()
    img = np.zeros((40, 56, 3), np.uint8)
    rs = utils.Resize(scale=0.75)
    for stages in ([rs, m], [(rs, CFG)], [(m, CFG), "resize"], [(m, CFG), (60, 84)], [utils.Resize]):
        with pytest.raises(ValueError, match="run_model_chain"):
            utils.run_model_chain(stages, img, CPU)
    with pytest.raises(ValueError, match="DeblurGANv2"):
        utils.run_model_chain([rs, (deblurganv2.FPNMobileNet(), CFG)], img, CPU)
    with pytest.raises(ValueError, match="need_degradation"):
        utils.run_model_chain([rs, (m, CFG)], img, CPU, need_degradation=True, noise_level=15)
    with pytest.raises(ValueError, match="shorter"):                   # 40 rows to 5: 4 x 8 + 2 = 34 taps fit, Lanczos' 50 do not
        utils.run_model_chain([(m, CFG), utils.Resize(size=(5, 56), kernel="lanczos3")], img, CPU)
    sr = Never()
    sr.upscale = 2
    with pytest.raises(ValueError, match="shorter"):                   # the second Resize sees 5 rows
        utils.run_model_chain([utils.Resize(size=(5, 56)), utils.Resize(scale=2.0)], img, CPU)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        utils.run_model_chain([rs, (m, CFG)], np.zeros((40, 56, 6), np.uint8), CPU)
    # valid arguments at every position, no GPU: there is no CPU fallback
    for stages in ([rs], [rs, (m, CFG)], [(m, CFG), rs, (m, CFG)], [(m, CFG), rs], [(sr, CFG), utils.Resize(size=(60, 84))],
                   [(m, CFG), utils.Resize(size=(5, 56))]):
        for frame in (img, img.astype(np.uint16), img.astype(np.float32)):
            with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
                utils.run_model_chain(stages, frame, CPU)


def test_chain_stage_calls(monkeypatch):
    """What each stage is asked for: a Resize between two stages makes the clamped float32 frame, the first one reads the
    integer frame, the last one requantises - an integer frame to its own type, a float32 frame to the input's."""
    calls = []
    dts = {"float32": torch.float32, "uint8": torch.uint8, "uint16": torch.int16}

    def fake_model(model, frame, ps, ov, pad8, sigma, **kw):
        calls.append(("model", str(frame.dtype), tuple(frame.shape), kw["unit_range"], kw["out"]))
        s = int(getattr(model, "upscale", 1))
        return torch.zeros(s * frame.shape[0], s * frame.shape[1], min(3, frame.shape[2]), dtype=dts[kw["out"]]), None

    def fake_resize(frame, size=None, scale=None, kernel="bicubic", antialias=True, out="same"):
        calls.append(("resize", str(frame.dtype), tuple(frame.shape), (size, scale, kernel, antialias), out))
        oh, ow = utils.resize_plan(frame.shape[0], frame.shape[1], size, scale, kernel, antialias)[:2]
        dt = frame.dtype if out == "same" else dts.get(out, torch.float32)
        return torch.zeros(oh, ow, frame.shape[2], dtype=dt)
    monkeypatch.setattr(utils, "tiled_forward_device", fake_model)
    monkeypatch.setattr(utils, "resize_device", fake_resize)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)         # (the upload to 'cuda')
    a, sr = Never(), Never()
    sr.upscale = 2
    cuda = torch.device("cuda:0")
    u8, u16 = np.zeros((40, 56, 3), np.uint8), np.zeros((40, 56, 3), np.uint16)
    mid, first, lastr = utils.Resize(scale=1.5, kernel="lanczos3"), utils.Resize(scale=0.75), utils.Resize(size=(60, 84), antialias=False)

    out, ms = utils.run_model_chain([(a, CFG), mid, (sr, CFG)], u8, cuda)
    assert out.dtype == np.uint8 and out.shape == (120, 168, 3) and ms >= 0
    assert calls == [("model", "torch.uint8", (40, 56, 3), True, "float32"),
                     ("resize", "torch.float32", (40, 56, 3), (None, 1.5, "lanczos3", True), "unit"),
                     ("model", "torch.float32", (60, 84, 3), True, "uint8")]
    del calls[:]
    out, _ = utils.run_model_chain([first, (a, CFG)], u16, cuda)
    assert out.dtype == np.uint16 and out.shape == (30, 42, 3)
    assert calls == [("resize", "torch.int16", (40, 56, 3), (None, 0.75, "bicubic", True), "unit"),
                     ("model", "torch.float32", (30, 42, 3), True, "uint16")]
    del calls[:]
    for frame, out_arg, want in ((u8, "same", "uint8"), (u16, "same", "uint16"), (u8, "float32", "unit"),
                                 (u8.astype(np.float32), "same", "unit")):
        out, _ = utils.run_model_chain([(a, CFG), lastr], frame, cuda, out=out_arg)
        assert calls[-1] == ("resize", "torch.float32", (40, 56, 3), ((60, 84), None, "bicubic", False), want)
        assert out.shape == (60, 84, 3) and out.dtype == (np.float32 if want == "unit" else frame.dtype)
    del calls[:]
    for frame, out_arg, want in ((u8, "same", "same"), (u16, "same", "same"), (u16, "float32", "unit"),
                                 (u8.astype(np.float32), "same", "unit")):
        out, _ = utils.run_model_chain([first], frame, cuda, out=out_arg)
        assert len(calls) == 1 and calls.pop()[-1] == want
        assert out.shape == (30, 42, 3) and out.dtype == (np.float32 if want == "unit" else frame.dtype)
    out, _ = utils.run_model_chain([first, mid], u8, cuda)
    assert [c[1::3] for c in calls] == [("torch.uint8", "unit"), ("torch.float32", "uint8")] and out.shape == (45, 63, 3)
