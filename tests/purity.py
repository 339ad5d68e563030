"""Purity checks: a forward may depend on its weights and its input and on nothing else.

Three things besides those can reach an output: memory that `torch.empty` handed out and no kernel wrote (workspace
pad channels, carry slots, pixels a blend skips), what an earlier call of another size left in a buffer that is grown
and never shrunk, and state that selects a packing or a forward but is not part of a cache key.  The helpers here make
each of them visible as a change of BYTES, so no tolerance has to be chosen:

  * `poisoned_allocations()` makes every `torch.empty*` inside it return NaN (floats) or SENTINEL_BYTE in every byte
    (integers): the contents of `empty` are undefined by contract, so this is a legal implementation of it, and the
    one a long-lived process that reuses blocks comes closest to;
  * `poison_workspaces(model)` writes the same poison into every buffer a model already holds, except the tensors
    `ModelHost._zeros` handed out (they are zero by contract and recorded under `zeros_recorded()`);
  * `same_bytes(a, b)` compares byte views, `finite(t)` is the NaN / inf check;
  * `check_uninitialised` and `check_history` are the two procedures built from them; `fresh` / `run` reuse the model
    ledger's cases (no oracle run is needed: a model is compared with its own unpoisoned bytes).

Plain functions and context managers, no fixtures; tests/test_purity_cpu.py is the positive control of every helper.
"""
import contextlib

import torch

import guards
import ledger
from irm_amd import dncnn, host, mair, ops, rednet, synth

_ALLOCATORS = ("empty", "empty_like", "empty_strided")


class NotReproducible(AssertionError):
    """Two identical unpoisoned runs differ: the case cannot be held to its own bytes (not a finding about poison)."""


class Impure(AssertionError):
    """An output changed, or stopped being finite, under poison or after a detour."""


# --------------------------------------------------------------------------- poison
def poison_(t):
    """Fill `t` in place: NaN for floating types (fp16 and complex included), SENTINEL_BYTE in every byte otherwise."""
    if not isinstance(t, torch.Tensor) or t.numel() == 0 or t.device.type == "meta":
        return t
    with torch.no_grad():
        if t.dtype.is_floating_point or t.dtype.is_complex:
            t.fill_(float("nan"))
        elif t.dtype == torch.bool:
            t.fill_(True)
        elif t.dim() > 0 and t.is_contiguous():
            t.view(torch.uint8).fill_(guards.SENTINEL_BYTE)
        else:                       # (not guards.sentinel: it allocates with torch.empty, which may be this poison)
            raw = bytes([guards.SENTINEL_BYTE]) * t.element_size()
            t.fill_(int.from_bytes(raw, "little", signed=not str(t.dtype).startswith("torch.uint")))
    return t


@contextlib.contextmanager
def poisoned_allocations():
    """Inside: torch.empty, torch.empty_like and torch.empty_strided return poisoned tensors.  The originals are back
    on exit, whatever happened inside."""
    saved = {n: getattr(torch, n) for n in _ALLOCATORS}

    def wrap(fn):
        def alloc(*a, **kw):
            return poison_(fn(*a, **kw))
        return alloc
    try:
        for n, fn in saved.items():
            setattr(torch, n, wrap(fn))
        yield
    finally:
        for n, fn in saved.items():
            setattr(torch, n, fn)


@contextlib.contextmanager
def zeros_recorded():
    """Inside: every tensor ModelHost._zeros returns is remembered on the model that asked for it, so that
    poison_workspaces can leave it alone.  Models must run inside this from their first forward on."""
    orig = host.ModelHost._zeros

    def _zeros(self, key, numel, device):
        t = orig(self, key, numel, device)
        self.__dict__.setdefault("_purity_zeros", {})[id(t)] = t
        return t
    host.ModelHost._zeros = _zeros
    try:
        yield
    finally:
        host.ModelHost._zeros = orig


def _tensors(v):
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, dict):
        for u in v.values():
            yield from _tensors(u)
    elif isinstance(v, (list, tuple)):
        for u in v:
            yield from _tensors(u)


def poison_workspaces(model):
    """Poison every buffer the model holds between calls: all of `_ws_by_stream` (every stream) and the conv stacks'
    `_ws`, on the model (or each model of a list; None: no model) and on every module below it (a wrapped network),
    and the channel-statistics workspace ops.py keeps for the FPN models.  Tensors recorded by zeros_recorded() are
    skipped.  Returns how many were poisoned."""
    n = 0
    models = model if isinstance(model, (list, tuple)) else [] if model is None else [model]
    for m in (m for top in models for m in top.modules()):
        zeros = m.__dict__.get("_purity_zeros", {})
        for name in ("_ws_by_stream", "_ws"):
            for t in _tensors(m.__dict__.get(name)):
                if id(t) not in zeros:
                    poison_(t)
                    n += 1
    for t in _tensors(ops._STATS_WS):
        poison_(t)
        n += 1
    return n


# --------------------------------------------------------------------------- comparison
class Verdict:
    """The result of same_bytes: true iff equal, and says why not."""

    def __init__(self, why=""):
        self.why = why

    def __bool__(self):
        return not self.why

    def __repr__(self):
        return self.why or "same bytes"


def _flat(v, prefix=""):
    if isinstance(v, dict):
        for k in sorted(v, key=str):
            yield from _flat(v[k], f"{prefix}{k}.")
    elif isinstance(v, (list, tuple)):
        for i, u in enumerate(v):
            yield from _flat(u, f"{prefix}{i}.")
    elif v is not None:
        yield prefix.rstrip("."), v if isinstance(v, torch.Tensor) else torch.as_tensor(v)


def same_bytes(a, b):
    """Are `a` and `b` the same bytes?  Tensors, numpy arrays, or dicts / tuples of them.  The Verdict of a difference
    names the entry, the first differing element (flat index, both values) and how many elements differ."""
    fa, fb = list(_flat(a)), list(_flat(b))
    if [k for k, _ in fa] != [k for k, _ in fb]:
        return Verdict(f"different entries: {[k for k, _ in fa]} vs {[k for k, _ in fb]}")
    for (k, u), (_, v) in zip(fa, fb):
        what = f"[{k}] " if k else ""
        if u.dtype != v.dtype or u.shape != v.shape:
            return Verdict(f"{what}{u.dtype} {tuple(u.shape)} vs {v.dtype} {tuple(v.shape)}")
        u, v = u.detach().cpu().contiguous(), v.detach().cpu().contiguous()
        if u.numel() == 0:
            continue
        size = u.element_size()
        ne = (u.reshape(-1).view(torch.uint8).view(-1, size) != v.reshape(-1).view(torch.uint8).view(-1, size)).any(1)
        count = int(ne.sum())
        if count:
            i = int(ne.nonzero()[0])
            return Verdict(f"{what}{count} of {u.numel()} elements differ, the first at flat index {i}: "
                           f"{u.reshape(-1)[i].item()!r} vs {v.reshape(-1)[i].item()!r}")
    return Verdict()


def finite(a):
    """True iff no entry of `a` (as for same_bytes) holds a NaN or an infinity; integer entries always pass."""
    for _, t in _flat(a):
        if (t.dtype.is_floating_point or t.dtype.is_complex) and not bool(torch.isfinite(t).all()):
            return False
    return True


# --------------------------------------------------------------------------- the two procedures
def check_uninitialised(model, call, what=""):
    """call() -> result, twice unpoisoned (the control: NotReproducible if the two differ), then once with the model's
    buffers poisoned and under poisoned_allocations(): the third result must be finite and the bytes of the first
    (Impure otherwise).  Returns the first result."""
    y0 = call()
    y1 = call()
    v = same_bytes(y1, y0)
    if not v:
        raise NotReproducible(f"{what}: two unpoisoned runs differ, the case is not bit-reproducible ({v})")
    poison_workspaces(model)
    with poisoned_allocations():
        y2 = call()
    if not finite(y2):
        raise Impure(f"{what}: uninitialised memory reached the output (NaN / inf under poison)")
    v = same_bytes(y2, y0)
    if not v:
        raise Impure(f"{what}: the output depends on uninitialised memory ({v})")
    return y0


def check_history(make, base, detours, what=""):
    """make() -> a fresh model; base(model) -> result; detours: callables of the model whose results are dropped.
    base on a fresh model, the detours, the held buffers poisoned, base again: the same bytes.  Then a second fresh
    model, run after all of that in the same process: the same bytes again.  Returns the first result."""
    model = make()
    a0 = base(model)
    if not finite(a0):
        raise Impure(f"{what}: the first run on a fresh model is not finite")
    for d in detours:
        d(model)
    poison_workspaces(model)
    a1 = base(model)
    v = same_bytes(a1, a0)
    if not (v and finite(a1)):
        raise Impure(f"{what}: the output depends on the calls before it ({v})")
    v = same_bytes(base(make()), a0)
    if not v:
        raise Impure(f"{what}: a second fresh model in the same process gives other bytes ({v})")
    return a0


# --------------------------------------------------------------------------- weights changed after a forward
def middle_weight(model):
    """The name of a weight matrix in the middle of the tree (the one-parameter mutations change this one)."""
    names = [n for n, p in model.named_parameters()]
    mats = [n for n in names[len(names) // 2:] if dict(model.named_parameters())[n].dim() >= 2]
    return mats[0]


def _slot(model, name):
    path, _, leaf = name.rpartition(".")
    return (model.get_submodule(path) if path else model), leaf


def _copy(model, donor, name):
    with torch.no_grad():
        getattr(*_slot(model, name)).copy_(donor[name])


def _new_parameter(model, donor, name):
    owner, leaf = _slot(model, name)
    old = getattr(owner, leaf)
    setattr(owner, leaf, torch.nn.Parameter(donor[name].detach().clone().to(old.device, old.dtype)))


def _optimizer_step(model, donor, name):
    p = getattr(*_slot(model, name))
    p.requires_grad_(True)
    opt = torch.optim.SGD([p], lr=1.0)
    p.grad = p.detach() - donor[name].to(p.device, p.dtype)          # one step of size 1 lands (up to rounding) on the donor
    opt.step()
    p.grad = None


def write_through_data(model, donor, name):
    """The write _hip.param_key documents as invisible: `.data` carries a version counter of its own."""
    getattr(*_slot(model, name)).data.copy_(donor[name])


#: kind -> (what it reaches, mutate(model, donor state dict, name of the one parameter)).  "all": the model ends with
#: the donor's weights; "one": with its own and the donor's value of one parameter; "round": with its own weights
#: rounded through fp16.  Every kind is one that _hip.param_key must see.
MUTATIONS = {
    "copy_": ("one", _copy),
    "load_state_dict": ("all", lambda model, donor, name: model.load_state_dict(donor)),
    "load_state_dict_assign": ("all", lambda model, donor, name: model.load_state_dict(
        {k: v.detach().clone() for k, v in donor.items()}, assign=True)),
    "new_parameter": ("one", _new_parameter),
    "half_float": ("round", lambda model, donor, name: model.half().float()),
    "optimizer_step": ("one", _optimizer_step),
}


# --------------------------------------------------------------------------- cases
def sr_config(name):
    """A MaIR super-resolution configuration of tests/golden/mair_sr.json (the smallest ones of tests/test_gpu_mair_sr.py)."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mair_sr.json")) as f:
        return json.load(f)["configs"][name]


#: the cases beside the ledger's: name -> (model factory, input shape).  Inputs are uniform in [0, 1].
EXTRA = {
    "dncnn_gray17_fp16_24x40_b2": (lambda: dncnn.DnCNN(1, 1, 64, 17, "R", precision="fp16").load_synthetic(42),
                                   (2, 1, 24, 40)),
    "rednet_fp16_24x40_b2": (lambda: rednet.REDNet(precision="fp16").load_synthetic(42), (2, 1, 24, 40)),
    "mairplus_dncnn5_210x230_b1": (lambda: mair.MaIRPlus(dncnn.DnCNN(3, 3, 64, 5, "R").load_synthetic(42)),
                                   (1, 3, 210, 230)),
    "mairplus_mair_light_x2_12x20_b1": (lambda: mair.MaIRPlus(mair.MaIR(**sr_config("light_x2")).load_synthetic(42)),
                                        (1, 3, 12, 20)),
}
for _n in ("light_x2", "light_x3", "light_x4", "classic_x2", "classic_x3", "classic_x4"):
    EXTRA[f"mair_sr_{_n}_12x20_b1"] = (lambda _n=_n: mair.MaIR(**sr_config(_n)).load_synthetic(42), (1, 3, 12, 20))

CASES = list(ledger.CASES) + list(EXTRA)


def has_tap(case):
    """Whole Restormers also report the `refinement` tap (the trunk before the output conv)."""
    return case in ledger.CASES and case.startswith("restormer_") and "_block_" not in case


def fresh(case, dev, monkeypatch):
    """A new model of the case on `dev` with the synthetic weights of seed 42 (the ledger's build for its cases)."""
    if case in ledger.CASES:
        return ledger.build(case, dev, monkeypatch)[0]
    return EXTRA[case][0]().eval().to(dev)


def run(case, dev, model):
    """{row: CPU tensor} of one forward on the case's seeded input: 'out', and 'refinement' for a whole Restormer."""
    if case in ledger.CASES:
        return ledger.run_gpu(case, dev, model, has_tap(case))
    x = synth.uniform(7, f"purity_{case}", EXTRA[case][1], 0.0, 1.0)
    with torch.no_grad():
        return dict(out=model(x.to(dev)).cpu())
