"""Host side of dw_gram (include/irm_hip_gram.h, _hip.SIGNATURES_GRAM, ops.can_dw_gram): the header and the binding agree,
the entry point refuses bad arguments before any HIP call, and it has a guard-band case on the GPU side."""
import ctypes
import os
import re

from irm_amd import _hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irm_dw_gram_cm_f16x3_f32"]


def test_header_declares_the_symbol():
    """The entry point has a header of its own, include/irm_hip_gram.h, which irm_hip.h includes inside its extern "C"
    block, and a table of its own, _hip.SIGNATURES_GRAM: the two match one to one, the library exports the symbol, load()
    binds it, and it returns IRM_EINVAL for null pointers and zero sizes before any HIP call."""
    main = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert main.index('#include "irm_hip_gram.h"') < main.rindex("#ifdef __cplusplus")
    text = open(os.path.join(ROOT, "include", "irm_hip_gram.h")).read()
    declared = re.findall(r"^\s*int\s+(irm_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(SYMBOLS) == sorted(_hip.SIGNATURES_GRAM)
    assert not set(_hip.SIGNATURES_GRAM) & (set(_hip.SIGNATURES) | set(_hip.SIGNATURES_HALF) | set(_hip.SIGNATURES_FRAMES))
    kinds = {ctypes.c_void_p: r"\*", ctypes.c_long: r"^long\b", ctypes.c_int: r"^int\b", ctypes.c_float: r"^float\b"}
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert m, name
        decls = [a.strip() for a in m.group(1).split(",") if a.strip()]
        sig = _hip.SIGNATURES_GRAM[name]
        assert len(sig) == len(decls), name
        for decl, ct in zip(decls[:-1], sig[:-1]):                   # the last one is irm_stream_t, a pointer
            assert re.search(kinds[ct], decl), (name, decl, ct)
        assert decls[-1].startswith("irm_stream_t") and sig[-1] is ctypes.c_void_p
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
        assert fn(*[t(0) for t in sig]) == -1, name
        assert getattr(_hip.load(), name).argtypes == sig


def test_bad_arguments_are_refused_before_any_hip_call():
    """Plausible pointers (never dereferenced on the host) with one argument wrong at a time: C / heads != 48, H % 8,
    W % 32, tiles not a multiple of the chunk, a batch stride that is misaligned or shorter than the q, k planes, misaligned
    qkv / gscale, sizes beyond the 32-bit offsets, each null pointer."""
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    fn = getattr(ctypes.CDLL(_hip.LIB_PATH), SYMBOLS[0])
    fn.argtypes, fn.restype = _hip.SIGNATURES_GRAM[SYMBOLS[0]], ctypes.c_int
    P = 1 << 20

    def rc(qkv=P, bs=3 * 192 * 32 * 32, taps=P, bias=P, gs=P, part=P, B=1, C=192, heads=4, H=32, W=32):
        return fn(qkv, bs, taps, bias, gs, part, B, C, heads, H, W, None)
    for bad in (dict(heads=2), dict(heads=5), dict(C=96, heads=1), dict(H=36), dict(H=28), dict(W=48), dict(H=24), dict(H=8, W=96),
                dict(bs=3 * 192 * 32 * 32 + 2), dict(bs=192 * 32 * 32), dict(qkv=P + 4), dict(gs=P + 8), dict(part=P + 2),
                dict(H=2048, W=2048, bs=3 * 192 * 2048 * 2048), dict(qkv=None), dict(taps=None), dict(gs=None), dict(part=None),
                dict(B=0)):
        assert rc(**bad) == -1, bad


def test_can_dw_gram_matches_the_entry_checks():
    assert ops.can_dw_gram(192, 4, 128, 128) and ops.can_dw_gram(384, 8, 64, 64) and ops.can_dw_gram(192, 4, 16, 128)
    for C, heads, H, W in [(192, 2, 32, 32), (96, 2, 32, 32), (48, 1, 32, 32), (192, 4, 36, 32), (192, 4, 32, 48), (192, 4, 24, 32),
                           (192, 4, 8, 8), (384, 8, 8, 8)]:
        assert not ops.can_dw_gram(C, heads, H, W), (C, heads, H, W)
    # the records per (image, head) it implies are those of the header: H W / 1024
    assert (128 // 8) * (128 // 32) // ops.QKV_GRAM_NCH == 128 * 128 // 1024


def test_entry_point_has_a_guard_band_case():
    """The rule of test_guards_cpu.py::test_every_entry_point_has_a_guard_band_case for _hip.SIGNATURES_GRAM: the symbol is
    reached in tests/test_gpu_dw_gram.py, between guard bands (tests/guards.py), through its wrapper ops.dw_gram."""
    with open(os.path.join(ROOT, "tests", "test_gpu_dw_gram.py")) as f:
        text = f.read()
    with open(os.path.join(os.path.dirname(_hip.LIB_PATH), "ops.py")) as f:
        ops_text = f.read()
    body = ops_text[ops_text.index("def dw_gram("):]
    body = body[:body.index("\ndef ", 1)]
    assert SYMBOLS[0] in body
    case = text[text.index("def test_dw_gram_guard_bands"):]
    assert "ops.dw_gram(" in case and "Guards(" in case and "g.check()" in case
    assert set(_hip.SIGNATURES_GRAM) == set(SYMBOLS)
