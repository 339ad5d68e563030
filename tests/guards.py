"""Guard bands for kernel tests: operands placed in the middle of a larger buffer whose surroundings are checked.

Every entry point of include/irm_hip.h takes raw pointers, extents and batch strides; in the models those pointers
lead into workspaces and channel slices whose neighbours are live tensors.  A test that hands a kernel exact-size
allocations cannot see a read or a store one row, one float4 or one partial block past an operand.  Here

  * an input lies between bands of NaN (`banded`): a value read from the band and masked with `* 0` still poisons
    the result, so "no NaN in the output" is the over-read check.  Integer frames cannot hold NaN: the kernel runs
    twice, the bands once all zeros and once all ones, and the two results must be bitwise equal (`two_fills`);
  * an output or workspace lies between sentinels (`sentinel_out`), and `intact` says whether every element outside
    the view, the slack between batch images included, still holds the sentinel.

`Guards` holds the guarded operands of one launch sequence and `clean` brings a result to the host through the NaN check.

Plain functions and one holder class, no fixtures; tests/test_guards_cpu.py is the positive control of every check below.
"""
import math

import torch

#: not a plausible result of any kernel (the value tests/test_gpu_ops.py::test_no_write_outside_the_output uses)
SENTINEL = 12345.0
#: integer outputs: every byte of the surroundings holds this
SENTINEL_BYTE = 0xA5
PAD = 4096


def sentinel(dtype):
    """The guard value of an output of `dtype` as a Python number."""
    if dtype.is_floating_point:
        return SENTINEL
    n = torch.empty((), dtype=dtype).element_size()
    return int(torch.full((n,), SENTINEL_BYTE, dtype=torch.uint8).view(dtype)[0])


def int_fill(dtype, fill):
    """`fill` reduced to the bit pattern an integer `dtype` can hold (-1: all bits set, whatever the width)."""
    n = torch.empty((), dtype=dtype).element_size()
    raw = (int(fill) & ((1 << (8 * n)) - 1)).to_bytes(n, "little")
    return int(torch.tensor(list(raw), dtype=torch.uint8).view(dtype)[0])


def _place(shape, dtype, dev, fill, pad, batch_slack):
    shape = tuple(int(s) for s in shape)
    assert len(shape) >= 1 and pad % 4 == 0 and batch_slack % 4 == 0 and pad > 0
    assert batch_slack == 0 or len(shape) >= 2, "batch slack needs a batch axis"
    per = int(math.prod(shape[1:]))
    bs = per + batch_slack
    n = (shape[0] - 1) * bs + per
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    strides, s = [], 1
    for d in reversed(shape[1:]):
        strides.append(s)
        s *= d
    view = buf.as_strided(shape, (bs,) + tuple(reversed(strides)), pad)
    return buf, view


def banded(t, dev, fill=None, pad=PAD, batch_slack=0):
    """(buf, view): the CPU tensor `t` copied into the middle of a device buffer filled with `fill` (NaN for floats
    by default); the view has t's shape, dense inner axes and batch stride t[0].numel() + batch_slack, the slack
    between the images holds `fill` too.  pad and batch_slack are multiples of 4 elements (16-byte alignment)."""
    if fill is None:
        assert t.dtype.is_floating_point, "integer operands need an explicit fill (two_fills)"
        fill = float("nan")
    elif not t.dtype.is_floating_point:
        fill = int_fill(t.dtype, fill)
    buf, view = _place(t.shape, t.dtype, dev, fill, pad, batch_slack)
    view.copy_(t)
    return buf, view


def sentinel_out(shape, dev, dtype=torch.float32, pad=PAD, batch_slack=0):
    """(buf, view) with the layout of `banded` for an output or a workspace: everything holds the sentinel of the
    dtype.  The view's own contents are the sentinel as well until the kernel (or the test) writes them."""
    return _place(shape, dtype, dev, sentinel(dtype), pad, batch_slack)


def channel_slice(dev, B, C, extra, ch, H, W, off, fill):
    """A [B, C, H, W] channel slice at channel `ch` of a [B, C + extra, H, W] float32 buffer that starts `off` floats into
    its allocation, everything holding `fill`.  Returns (flat allocation, view)."""
    N = H * W
    flat = torch.full((B * (C + extra) * N + 4,), fill, dtype=torch.float32, device=dev)
    return flat, flat.as_strided((B, C, H, W), ((C + extra) * N, N, W, 1), off + ch * N)


def outside(buf, view):
    """Boolean mask over `buf`: True where an element does not belong to `view`."""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    off = view.storage_offset() - buf.storage_offset()
    mask.as_strided(view.shape, view.stride(), off).fill_(False)
    return mask


def intact(buf, view):
    """True if every element of `buf` outside `view` still holds the sentinel (front band, back band, batch slack)."""
    guard = buf[outside(buf, view)]
    return bool((guard == sentinel(buf.dtype)).all())


def has_nan(t):
    return bool(torch.isnan(t).any())


#: elements between the images of a strided operand (a multiple of 4: rows stay 16-byte aligned)
SLACK = 8


class Guards:
    """The guarded operands of one launch sequence: inp() bands an input, out() places an output or a workspace and
    remembers it, check() asserts that every remembered surrounding is intact.  Every buffer stays alive as long as
    the object does: a raw pointer taken from a temporary view would otherwise outlive its allocation."""

    def __init__(self, dev):
        self.dev, self.outs, self.ins = dev, [], []

    def inp(self, t, slack=0, fill=None):
        if t is None:
            return None
        buf, view = banded(t, self.dev, fill, batch_slack=slack)
        self.ins.append(buf)
        return view

    def out(self, name, shape, dtype=torch.float32, slack=0):
        buf, view = sentinel_out(shape, self.dev, dtype, batch_slack=slack)
        self.outs.append((name, buf, view))
        return view

    def check(self):
        torch.cuda.synchronize()
        bad = [name for name, buf, view in self.outs if not intact(buf, view)]
        assert not bad, f"writes outside: {bad}"


def clean(t):
    """The result on the host, after the check that no NaN (a guard element of an input) reached it."""
    t = t.cpu().contiguous()
    assert not has_nan(t), "a NaN from outside an input reached the result"
    return t


def guarded_fold(g, qkv, B, C, heads, N, temp, wout, part=None, nready=None, **kw):
    """ops.mdta_fold with part / gsum at exactly their record sizes and the folded matrix between sentinels of the Guards
    `g`; returns (attention, folded matrix)."""
    from irm_amd import ops
    _, nchunk, rec = ops.mdta_plan(B, C, heads, N)
    c = C // heads
    if part is None:
        part = g.out("part", (B * heads * nchunk * rec,))
    gsum, attn = g.out("gsum", (B * heads * rec,)), g.out("attn", (B, heads, c, c))
    mfold = g.out("mfold", (B * (ops.mfold_frag_numel(C) if kw.get("frag") else ops.mfold_numel(C)),))
    mfold.zero_()
    ops.mdta_fold(qkv, part, gsum, temp, wout, mfold, C, heads, attn=attn, nchunk_ready=nready, **kw)
    return attn, mfold


def two_fills(run):
    """Integer inputs: `run(fill)` builds its banded integer operands with `fill`, launches, and returns a tuple of
    CPU result tensors.  It runs with bands of zeros (0) and of ones (-1, all bits set in any integer type); the
    results must be bitwise equal.  Returns them."""
    a = run(0)
    b = run(-1)
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        same = torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))
        assert same, f"result {i} depends on what lies outside an integer operand"
    return a
