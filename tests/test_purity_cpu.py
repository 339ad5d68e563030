"""Positive controls of tests/purity.py and the cache-key tests that need no GPU.

1. Toy ModelHost subclasses made of torch ops commit, on purpose, each kind of impurity the helpers are there to catch;
   the checker must flag them and pass the clean toy.
2. `_hip.param_key` and `ModelHost._pack` on a small module tree with a counting `_build`: which changes of the weights
   rebuild the packed operands (exactly once), which do not, and the documented blind spot.
3. The `precision` of the conv stacks is part of that key: the packers are host code, so the real DnCNN and REDNet are
   held to it here."""
import contextlib

import pytest
import torch
import torch.nn as nn

from irm_amd import _hip, dncnn, rednet
from irm_amd.host import ModelHost

import guards
import purity

N = 1 << 16         # floats of a toy buffer


# --------------------------------------------------------------------------- 1. the helpers
def _nan_seen(t):
    """1.0 if `t` holds a NaN, else 0.0: what an undefined value does to a result."""
    return torch.isnan(t).any().float()


@contextlib.contextmanager
def _young_process():
    """torch.empty* hand out zero pages, as the allocator of a process that has freed nothing yet mostly does: the
    state in which an impure model passes every comparison.  (Real recycled memory would make the unpoisoned runs of
    the toys below differ from one another; here it holds the NaNs of the tests before.)"""
    saved = {n: getattr(torch, n) for n in ("empty", "empty_like", "empty_strided")}
    try:
        for n, fn in saved.items():
            setattr(torch, n, (lambda fn: lambda *a, **kw: fn(*a, **kw).zero_())(fn))
        yield
    finally:
        for n, fn in saved.items():
            setattr(torch, n, fn)


class SumsBeforeWriting(ModelHost):
    """Reads a workspace buffer it has not written in this call."""

    def forward(self, x):
        t = self._buf("acc", N, x.device)
        s = _nan_seen(t)
        t.copy_(x)
        return t + s


class AddsIntoEmpty(ModelHost):
    """Accumulates into a torch.empty output."""

    def forward(self, x):
        out = torch.empty(N, dtype=torch.float32)
        return x + _nan_seen(out)


class ReadsGrownSlot(ModelHost):
    """Writes the n values it was asked for and reduces over the first 2 n of the buffer as it is held: exact on a
    fresh model, whose buffer has n elements, and a read of what a larger earlier call left behind after one."""

    def forward(self, x):
        n = x.numel()
        self._buf("t", n, x.device).copy_(x)
        held = self._ws_by_stream[0]["t"]
        return x + _nan_seen(held[:2 * n])


class Clean(ModelHost):
    """Uses a workspace buffer, a zeroed one and an empty output, and writes each before it reads it."""

    def forward(self, x):
        t = self._buf("acc", 2 * N, x.device)[:N]
        t.copy_(x)
        z = self._zeros("zero", N, x.device)
        out = torch.empty_like(x)
        out.copy_(t * 2 + z)
        return out


class Wrapper(nn.Module):
    """A module around a model, as the self-ensemble is around its network."""

    def __init__(self, net):
        super().__init__()
        self.net = net


def _x(n=N, seed=0):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed))


def _uninitialised(model):
    with _young_process(), purity.zeros_recorded():
        return purity.check_uninitialised(model, lambda: model(_x()), type(model).__name__)


def test_poisoned_allocations_poisons_and_restores():
    saved = (torch.empty, torch.empty_like, torch.empty_strided)
    with purity.poisoned_allocations():
        assert torch.empty is not saved[0]
        for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
            assert bool(torch.isnan(torch.empty(7, 3, dtype=dt)).all())
            assert bool(torch.isnan(torch.empty_like(torch.zeros(5, dtype=dt))).all())
            assert bool(torch.isnan(torch.empty_strided((4, 3), (1, 4), dtype=dt)).all())
        for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
            t = torch.empty(9, dtype=dt)
            assert bool((t.view(torch.uint8) == guards.SENTINEL_BYTE).all()) and int(t[0]) == guards.sentinel(dt)
            assert int(torch.empty_like(torch.zeros(3, dtype=dt))[2]) == guards.sentinel(dt)
        assert torch.empty(0).numel() == 0
    assert (torch.empty, torch.empty_like, torch.empty_strided) == saved
    with pytest.raises(RuntimeError, match="inside"):
        with purity.poisoned_allocations():
            raise RuntimeError("inside")
    assert (torch.empty, torch.empty_like, torch.empty_strided) == saved


def test_same_bytes_and_finite():
    a = torch.arange(12, dtype=torch.float32).view(3, 4)
    assert purity.same_bytes(a, a.clone()) and purity.same_bytes({"out": a, "t": (a, a)}, {"out": a, "t": (a, a)})
    b = a.clone()
    b[1, 2] += 1
    b[2, 3] += 1
    v = purity.same_bytes(a, b)
    assert not v and "2 of 12" in v.why and "flat index 6" in v.why
    assert not purity.same_bytes(torch.tensor([0.0]), torch.tensor([-0.0]))        # equal as numbers, other bytes
    nan = torch.tensor([float("nan")])
    assert purity.same_bytes(nan, nan.clone())                                      # unequal as numbers, same bytes
    assert not purity.same_bytes(a, a.double()) and not purity.same_bytes(a, a.view(4, 3))
    assert not purity.same_bytes({"out": a}, {"out": a, "refinement": a})
    assert "[refinement]" in purity.same_bytes({"out": a, "refinement": a}, {"out": a, "refinement": b}).why
    assert purity.finite(a) and purity.finite({"i": torch.tensor([1, 2])})
    assert not purity.finite({"out": a, "t": nan}) and not purity.finite(torch.tensor([float("inf")]))
    assert not purity.finite(torch.tensor([float("nan")], dtype=torch.float16))


def test_the_checker_flags_a_buffer_read_before_it_is_written():
    with pytest.raises(purity.Impure):
        _uninitialised(SumsBeforeWriting())


def test_the_checker_flags_an_output_accumulated_into_empty():
    with pytest.raises(purity.Impure):
        _uninitialised(AddsIntoEmpty())


def test_the_checker_flags_a_slot_left_by_a_larger_earlier_call():
    n = 1000
    with _young_process(), purity.zeros_recorded():
        # on a fresh model, and under poison at one size, nothing shows: this is what the history check is for
        m = ReadsGrownSlot()
        purity.check_uninitialised(m, lambda: m(_x(n)), "ReadsGrownSlot")
        with pytest.raises(purity.Impure, match="calls before it"):
            purity.check_history(ReadsGrownSlot, lambda m: m(_x(n)), [lambda m: m(_x(4 * n, 1))], "ReadsGrownSlot")


def test_the_checker_passes_a_clean_model():
    _uninitialised(Clean())
    with _young_process(), purity.zeros_recorded():
        purity.check_history(Clean, lambda m: m(_x()), [lambda m: m(_x(N, 3))], "Clean")


def test_the_control_run_is_reported_apart_from_the_poison():
    calls = []

    def call():
        calls.append(0)
        return torch.tensor([float(len(calls))])
    with pytest.raises(purity.NotReproducible, match="not bit-reproducible"):
        purity.check_uninitialised(Clean(), call, "counter")


def test_poison_workspaces_leaves_zeros_alone_and_reaches_wrapped_models():
    m = Clean()
    m._ws = {"key": (1, 2), "a": torch.ones(4, dtype=torch.float16), "i": torch.zeros(3, dtype=torch.int32)}
    with purity.zeros_recorded():
        m(_x())
    m._ws_by_stream.setdefault(77, {})["other_stream"] = torch.ones(5)
    assert purity.poison_workspaces(Wrapper(m)) >= 4
    ws = m._ws_by_stream[0]
    assert bool((ws["zero"] == 0).all()), "a _zeros tensor was poisoned"
    assert bool(torch.isnan(ws["acc"]).all()) and bool(torch.isnan(m._ws_by_stream[77]["other_stream"]).all())
    assert bool(torch.isnan(m._ws["a"]).all()) and int(m._ws["i"][0]) == guards.sentinel(torch.int32)
    assert ModelHost._zeros.__qualname__ == "ModelHost._zeros", "zeros_recorded left its wrapper behind"
    # unrecorded (the model ran outside zeros_recorded): the zero tensor is not known and is poisoned
    m2 = Clean()
    m2(_x())
    purity.poison_workspaces(m2)
    assert bool(torch.isnan(m2._ws_by_stream[0]["zero"]).all())


# --------------------------------------------------------------------------- 2. param_key and _pack
class Tree(ModelHost):
    """Three levels of modules; _build counts its runs and snapshots the weights."""

    def __init__(self):
        super().__init__()
        self.head = nn.Linear(4, 6)
        self.body = nn.Sequential(nn.Sequential(nn.Linear(6, 6), nn.ReLU(), nn.Linear(6, 6)), nn.Linear(6, 5))
        self.tail = nn.Linear(5, 2, bias=False)
        self.builds = 0

    def _build(self):
        self.builds += 1
        return {k: v.detach().clone() for k, v in self.state_dict().items()}


DEEP = "body.0.2.weight"


def _tree(seed):
    torch.manual_seed(seed)
    return Tree()


def _packed_is_current(m):
    pk = m._pack()
    return all(torch.equal(pk[k], v) for k, v in m.state_dict().items())


@pytest.mark.parametrize("kind", list(purity.MUTATIONS))
def test_pack_rebuilds_exactly_once_after(kind):
    m, donor = _tree(1), _tree(2).state_dict()
    m._pack()
    k0 = _hip.param_key(m)
    assert m.builds == 1
    reach, mutate = purity.MUTATIONS[kind]
    before = {k: v.clone() for k, v in m.state_dict().items()}
    mutate(m, donor, DEEP)
    after = m.state_dict()
    changed = [k for k in after if not torch.equal(after[k], before[k])]
    assert changed == ([DEEP] if reach == "one" else list(after)), "the mutation did not do what its kind says"
    k1 = _hip.param_key(m)
    assert k1 != k0, f"{kind}: the key did not change"
    assert _packed_is_current(m) and m.builds == 2, f"{kind}: {m.builds - 1} rebuilds"
    m._pack()
    assert m.builds == 2 and _hip.param_key(m) == k1


def test_pack_is_kept_across_what_changes_no_weight():
    m = _tree(1)
    m._pack()
    k0 = _hip.param_key(m)
    for _ in range(3):
        m._pack()
    m.eval()
    m._pack()
    m.train()
    m._pack()
    for p in m.parameters():
        p.requires_grad_(False)
    m._pack()
    m.requires_grad_(True)
    m._pack()
    assert m.builds == 1 and _hip.param_key(m) == k0


def test_a_write_through_data_is_not_seen_until_invalidate():
    m, donor = _tree(1), _tree(2).state_dict()
    m._pack()
    k0 = _hip.param_key(m)
    m.__dict__["_irm_graphs"] = {"a graph": None}
    purity.write_through_data(m, donor, DEEP)
    assert torch.equal(m.state_dict()[DEEP], donor[DEEP])
    assert _hip.param_key(m) == k0, "param_key now sees p.data writes: update its documentation"
    m._pack()
    assert m.builds == 1 and not _packed_is_current(m)         # the documented limit
    _hip.invalidate(m)
    assert "_irm_graphs" not in m.__dict__
    assert _hip.param_key(m) != k0
    assert _packed_is_current(m) and m.builds == 2


def test_invalidate_reaches_the_models_below_and_above():
    net = _tree(1)
    w = Wrapper(net)
    net._pack()
    k0 = _hip.param_key(w)
    purity.write_through_data(net, _tree(2).state_dict(), DEEP)
    _hip.invalidate(w)                                          # on the wrapper: the network's pack goes too
    assert _packed_is_current(net) and net.builds == 2
    k1 = _hip.param_key(w)
    assert k1 != k0
    purity.write_through_data(net, _tree(3).state_dict(), DEEP)
    _hip.invalidate(net)                                        # on the network: the wrapper's key (its graphs) changes too
    assert _hip.param_key(w) != k1
    assert _packed_is_current(net) and net.builds == 3


def test_the_key_of_a_wrapper_carries_the_wrapped_models_mode():
    net = dncnn.DnCNN(1, 1, 64, 3, "R")
    w = Wrapper(net)
    k0 = _hip.param_key(w)
    assert _hip.param_key(w) == k0
    net.precision = "fp16"
    assert _hip.param_key(w) != k0


# --------------------------------------------------------------------------- 3. the precision switch
def _same_pack(a, b):
    fa, fb = list(purity._flat(_plain(a))), list(purity._flat(_plain(b)))
    return len(fa) == len(fb) and all(bool(purity.same_bytes(u, v)) for (_, u), (_, v) in zip(fa, fb))


def _plain(pack):
    """A pack as nested tuples of tensors and numbers (ConvWeight objects opened)."""
    if isinstance(pack, _hip.ConvWeight):
        return tuple(_plain(getattr(pack, s)) for s in pack.__slots__)
    if isinstance(pack, (list, tuple)):
        return tuple(_plain(p) for p in pack)
    return pack


STACKS = {"dncnn": lambda precision: dncnn.DnCNN(1, 1, 64, 4, "R", precision=precision).load_synthetic(42),
          "rednet": lambda precision: rednet.REDNet(1, 64, precision=precision).load_synthetic(42)}


@pytest.mark.parametrize("first,then", [("fp32", "fp16"), ("fp16", "fp32")])
@pytest.mark.parametrize("family", list(STACKS))
def test_pack_follows_the_precision(family, first, then):
    m = STACKS[family](first)
    stale = m._pack()
    assert m._pack() is stale
    k0 = _hip.param_key(m)
    m.precision = then
    assert m.precision == then and _hip.param_key(m) != k0
    want = STACKS[family](then)._pack()
    got = m._pack()
    assert got is not stale, "the pack of the other mode came back from the cache"
    assert _same_pack(got, want) and not _same_pack(got, stale)
    m.precision = first
    assert _same_pack(m._pack(), stale)


def test_precision_is_validated_when_set():
    d, r = dncnn.DnCNN(1, 1, 64, 4, "R"), rednet.REDNet(1, 64)
    for m in (d, r):
        with pytest.raises(ValueError, match="precision must be one of"):
            m.precision = "bf16"
        assert m.precision == "fp32"
    for m, make in ((dncnn.DnCNN(1, 1, 32, 4, "R"), lambda: dncnn.DnCNN(1, 1, 32, 4, "R", precision="fp16")),
                    (rednet.REDNet(1, 96), lambda: rednet.REDNet(1, 96, precision="fp16"))):
        with pytest.raises(ValueError, match="needs 64 or 128 hidden channels") as by_setter:
            m.precision = "fp16"
        with pytest.raises(ValueError, match="needs 64 or 128 hidden channels") as by_constructor:
            make()
        assert str(by_setter.value) == str(by_constructor.value) and m.precision == "fp32"
