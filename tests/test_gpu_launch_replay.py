"""The 1x1-GEMM and 3x3-conv launches production issues, replayed one by one against float64.

Each workload runs once, eagerly (model(x) at the bench's input shapes), with ops.gemm1x1 and ops.conv3x3 wrapped to
record every call's signature: its scalar arguments, the weight kind, and for every tensor its shape, batch stride,
offset in its buffer, 16-byte alignment, aliasing and max|.|; plus the kernel and tag ops.KernelTimer(detail=True) logs
(the tag holds the plan: ct and ygroups).  Each unique signature is then replayed alone with seeded weights of the
model's magnitude (packed by the same packer), inputs scaled to the recorded max|.|, and buffers with the recorded
layout.  The replay must log the same kernel and tag, and pass the bar of tests/test_gpu_precision.py image by image:
e <= K * e_32 + F * max|y64| with y64 in float64 and y32 in float32 (TF32 off), both on the device; the emulated
conv (conv3x3_f16x3) is held to its op-test bar instead, 2x the exact-f32 conv kernel on the same inputs.  Every GEMM launch
recorded must also be a variant tests/test_gpu_gemm_variants.py tests, and every conv launch a variant and a pass structure
tests/test_gpu_conv_variants.py tests."""
import os
import re

import pytest
import torch
import torch.nn.functional as TF

import block_model as bm
from block_model import F, K
from irm_amd import _hip, deblurganv2, dncnn, mair, ops, rednet, restormer
from variant_model import (CASE_STRUCTURES, CONV_VARIANTS, VARIANTS, expected_conv_variant, expected_variant, pass_structure,
                           passes_per_group)

pytestmark = pytest.mark.gpu


def _mair_cdn():
    import yaml
    with open(os.path.join(os.path.dirname(mair.__file__), "options", "test_MaIR_CDN_s25.yml")) as f:
        net = dict(yaml.safe_load(f)["network_g"])
    net.pop("type")
    return mair.MaIR(**net)


# workload -> (model factory, input shape): the inputs of one bench step (bench.py, tools/bench_configs.py)
WORKLOADS = {
    "c2_dncnn_8x256": (lambda: dncnn.DnCNN(1, 1, 64, 20, "R").eval(), (8, 1, 256, 256)),
    "c3_restormer_bf_9x256": (lambda: restormer.Restormer(LayerNorm_type="BiasFree").eval(), (9, 3, 256, 256)),
    "c4_restormer_wb_24x512": (lambda: restormer.Restormer(LayerNorm_type="WithBias").eval(), (24, 3, 512, 512)),
    "c5_mairunet_256": (lambda: mair.MaIRUNet(dim=48, num_blocks=[4, 6, 6, 8], num_refinement_blocks=4, ssm_ratio=2.0,
                                              flp_ratio=4.0, mlp_ratio=1.5, scan_len=4).eval(), (1, 3, 256, 256)),
    "mair_cdn_9x128": (lambda: _mair_cdn().eval(), (9, 3, 128, 128)),
    "rednet_9x128": (lambda: rednet.REDNet().eval(), (9, 1, 128, 128)),
    # train-mode BatchNorm as in the bench; the DeblurGANv2 hooks pad 720 to 736
    "fpn_mobilenet_1280x720": (lambda: deblurganv2.FPNMobileNet(), (1, 3, 736, 1280)),
}

_GEMM_T = ("x", "y", "res", "bias", "stats", "lnw", "lnb", "stats_out", "res_scale")
_CONV_T = ("x", "y", "res", "bias")
_RECORDED = {}      # workload -> {signature: launch record}
_TABLE = []


# --------------------------------------------------------------------------- recording
def _desc(t):
    """Layout and magnitude of one tensor argument (None stays None)."""
    if t is None:
        return None
    return dict(shape=tuple(t.shape), stride=tuple(t.stride()), off=t.storage_offset(), align=t.data_ptr() % 16,
                store=t.untyped_storage().data_ptr(), amax=float(t.abs().max()) if t.numel() else 0.0)


def _key(d):
    """The hashable layout part of a descriptor."""
    return None if d is None else (d["shape"], d["stride"], d["off"], d["align"])


def _aliases(ds):
    """Which named tensors share a buffer: name -> the first name with the same storage."""
    out, first = {}, {}
    for n, d in ds.items():
        if d is not None:
            out[n] = first.setdefault(d["store"], n)
    return tuple(sorted(out.items()))


def _gemm_weight_max(wp, split):
    if split:
        h = wp.reshape(-1).view(torch.float16).view(-1, 2, 256)[:, 0]          # the hi halves
        return float(h.float().abs().max())
    return float(wp.abs().max())


def _conv_weight_kind(wp):
    if isinstance(wp, _hip.ConvWeight):
        return "ConvWeight(" + ",".join(n for n in ("exact", "split", "raw") if getattr(wp, n) is not None) + ")"
    return "split" if isinstance(wp, tuple) else "exact"


def _conv_weight_max(wp):
    if isinstance(wp, _hip.ConvWeight):
        return float(wp.exact.abs().max())
    if isinstance(wp, tuple):
        h = wp[0].reshape(-1).view(torch.float16)
        return float(h.float().abs().max()) * wp[1] / 16.0          # packed as W * s, inv_scale = 16 / s
    return float(wp.abs().max())


def record(name, dev, monkeypatch):
    if name in _RECORDED:
        return _RECORDED[name]
    factory, shape = WORKLOADS[name]
    model = factory().load_synthetic(42).to(dev)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(5)).to(dev)
    timer = ops.KernelTimer(detail=True)
    seen = {}
    real_gemm, real_conv = ops.gemm1x1, ops.conv3x3

    def last_launch():
        return timer.records[-1][0]

    def gemm1x1(wp, x, y, M, K, **kw):
        ds = {n: _desc(kw.get(n)) for n in _GEMM_T if n not in ("x", "y")}
        ds["x"], ds["y"] = _desc(x), _desc(y)
        wmax = _gemm_weight_max(wp, kw.get("split", False))
        real_gemm(wp, x, y, M, K, **kw)
        scal = tuple(sorted((k, v) for k, v in kw.items() if k not in _GEMM_T))
        sig = ("gemm", M, K, scal, tuple((n, _key(ds[n])) for n in _GEMM_T), _aliases(ds), tuple(wp.shape), last_launch())
        r = seen.setdefault(sig, dict(op="gemm", M=M, K=K, kw=dict(scal), ds=ds, wshape=tuple(wp.shape), wmax=0.0,
                                      launch=last_launch(), count=0))
        r["wmax"] = max(r["wmax"], wmax)
        r["count"] += 1
        for n, d in ds.items():
            if d is not None:
                r["ds"][n]["amax"] = max(r["ds"][n]["amax"], d["amax"])

    def conv3x3(wp, x, y, ci, co, **kw):
        ds = {n: _desc(kw.get(n)) for n in ("res", "bias")}
        ds["x"], ds["y"] = _desc(x), _desc(y)
        real_conv(wp, x, y, ci, co, **kw)
        scal = tuple(sorted((k, v) for k, v in kw.items() if k not in _CONV_T))
        kind = _conv_weight_kind(wp)
        sig = ("conv", ci, co, scal, tuple((n, _key(ds.get(n))) for n in _CONV_T), _aliases(ds), kind, last_launch())
        r = seen.setdefault(sig, dict(op="conv", ci=ci, co=co, kw=dict(scal), ds=ds, kind=kind, wmax=0.0,
                                      launch=last_launch(), count=0))
        r["wmax"] = max(r["wmax"], _conv_weight_max(wp))
        r["count"] += 1
        for n, d in ds.items():
            if d is not None:
                r["ds"][n]["amax"] = max(r["ds"][n]["amax"], d["amax"])

    monkeypatch.setenv("IRM_TIMER_KEEP_EVENTS", "1")       # the timer's records stay readable after each launch
    monkeypatch.setattr(ops, "TIMER", timer)
    monkeypatch.setattr(ops, "gemm1x1", gemm1x1)
    monkeypatch.setattr(ops, "conv3x3", conv3x3)
    try:
        with torch.no_grad():
            model(x)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    timer.summary()
    del model
    torch.cuda.empty_cache()
    _RECORDED[name] = list(seen.values())
    return _RECORDED[name]


# --------------------------------------------------------------------------- replay
def _buffers(ds, dev, seed):
    """Fresh tensors with the recorded layouts; tensors that shared a buffer share one again."""
    groups = {}
    for n, d in ds.items():
        if d is not None:
            end = d["off"] + sum((s - 1) * st for s, st in zip(d["shape"], d["stride"])) + 1
            groups[d["store"]] = max(groups.get(d["store"], 0), end)
    flats = {s: torch.zeros(n + 4, device=dev) for s, n in groups.items()}
    g = torch.Generator(device=dev).manual_seed(seed)
    out = {}
    for n, d in ds.items():
        if d is None:
            out[n] = None
            continue
        t = flats[d["store"]].as_strided(d["shape"], d["stride"], d["off"])
        assert t.data_ptr() % 16 == d["align"], "torch allocations are 16-byte aligned"
        out[n] = t
    for n in ("x", "res", "bias", "lnw", "lnb", "res_scale"):
        if out.get(n) is not None:
            a = ds[n]["amax"]
            lo = a / 2 if n in ("lnw", "res_scale") else -a
            out[n].copy_(torch.rand(ds[n]["shape"], generator=g, device=dev) * (a - lo) + lo)
    return out


def _row(name, got, y64, y32):
    """(row, e, e_32, bar): the ledger bar e <= K * e_32 + F * max|y64|; NaN (unwritten) counts as infinite."""
    e = float((got.double() - y64).abs().nan_to_num(float("inf")).max())
    e32 = float((y32.double() - y64).abs().max())
    return name, e, e32, K * e32 + F * float(y64.abs().max())


def replay_gemm(r, dev, seed):
    M, Kc, kw = r["M"], r["K"], dict(r["kw"])
    split, ln = kw.get("split", False), kw.get("ln_mode", 0)
    t = _buffers(r["ds"], dev, seed)
    x, y = t["x"], t["y"]
    B, _, H, W = x.shape
    N = H * W
    inplace = t["res"] is not None and t["res"].data_ptr() == y.data_ptr()
    if t["stats"] is not None:
        ops.ln_stats(x[:, :Kc], t["stats"], kw.get("eps", 1e-5))
    res0 = t["res"].clone() if t["res"] is not None else None
    w_bs = kw.get("w_bs", 0)
    g = torch.Generator().manual_seed(seed + 1)
    wshape = (B, M, Kc) if w_bs else (M, Kc)
    w = (torch.rand(wshape, generator=g) * 2 - 1) * r["wmax"]
    pk = _hip.pack_gemm_weight_split if split else _hip.pack_gemm_weight
    packed = (torch.stack([pk(w[b]) for b in range(B)]) if w_bs else pk(w)).reshape(-1)
    wp = torch.zeros(torch.Size(r["wshape"]).numel())           # a per-batch buffer may hold more images than B
    assert packed.numel() <= wp.numel()
    wp[:packed.numel()] = packed
    wp = wp.reshape(r["wshape"]).to(dev)
    if not inplace:
        y.fill_(float("nan"))
    if t["stats_out"] is not None:
        t["stats_out"].fill_(float("nan"))
    timer = ops.KernelTimer(detail=True)
    ops.TIMER = timer
    try:
        ops.gemm1x1(wp, x, y, M, Kc, **{n: t[n] for n in _GEMM_T if n not in ("x", "y")}, **kw)
    finally:
        ops.TIMER = None
    launch = timer.records[-1][0]
    timer.summary()
    rows = []
    wd = w.to(dev)
    for b in range(B):
        ys = {}
        for dt in (torch.float64, torch.float32):
            xb = bm.layer_norm(x[b, :Kc].reshape(Kc, N).to(dt), t["lnw"], t["lnb"], ln, dim=0)
            yb = (wd[b] if w_bs else wd).to(dt) @ xb
            if t["bias"] is not None:
                yb = yb + t["bias"].to(dt).view(-1, 1)
            yb = bm.act(yb, kw.get("act", 0))
            if res0 is not None:
                rb = res0[b].reshape(-1, N)[:M].to(dt)
                yb = yb + (rb * t["res_scale"].to(dt).view(-1, 1) if t["res_scale"] is not None else rb)
            ys[dt] = yb
        y64 = ys[torch.float64]
        got = y[b].reshape(-1, N)[:M].double()
        rows.append(_row("y", got, y64, ys[torch.float32]))
        if t["stats_out"] is not None:
            for i, ref64, ref32 in ((0, y64.mean(0), ys[torch.float32].mean(0)),
                                    (1, 1 / torch.sqrt(y64.var(0, unbiased=False) + kw.get("eps", 1e-5)),
                                     1 / torch.sqrt(ys[torch.float32].var(0, unbiased=False) + kw.get("eps", 1e-5)))):
                rows.append(_row("mean" if i == 0 else "rstd", t["stats_out"].reshape(B, 2, N)[b, i], ref64, ref32))
    return launch, rows


def _conv_ref(x, w, bias, res, kw, dt):
    """One image: x [ci, H, W] -> the conv3x3 epilogue chain of conv3x3.hip (bias, relu1, res_mode, relu2, store)."""
    ci, H, W = x.shape
    xp = TF.pad(x.to(dt), (1, 1, 1, 1))
    y = 0
    for dy in range(3):
        for dx in range(3):
            y = y + torch.einsum("oc,chw->ohw", w[:, :, dy, dx].to(dt), xp[:, dy:dy + H, dx:dx + W])
    if bias is not None:
        y = y + bias.to(dt).view(-1, 1, 1)
    return bm.conv_epilogue(y[None], None if res is None else res[None], kw.get("relu1"), kw.get("res_mode", 0), kw.get("relu2"),
                            kw.get("store_mode", 0))[0]


def replay_conv(r, dev, seed):
    ci, co, kw = r["ci"], r["co"], dict(r["kw"])
    t = _buffers(r["ds"], dev, seed)
    x, y = t["x"], t["y"]
    B = x.shape[0]
    g = torch.Generator().manual_seed(seed + 1)
    w = (torch.rand((co, ci, 3, 3), generator=g) * 2 - 1) * r["wmax"]
    kind = r["kind"]
    if kind.startswith("ConvWeight"):
        wp = _hip.pack_conv3x3(w.to(dev))
        assert _conv_weight_kind(wp) == kind, (kind, _conv_weight_kind(wp))
    elif kind == "split":
        s, inv = _hip.pack_conv3x3_weight_split(w)
        wp = (s.to(dev), inv)
    else:
        wp = _hip.pack_conv3x3_weight(w).to(dev)
    res0 = t["res"].clone() if t["res"] is not None else None
    if res0 is None or t["res"].data_ptr() != y.data_ptr():
        y.fill_(float("nan"))
    timer = ops.KernelTimer(detail=True)
    ops.TIMER = timer
    try:
        ops.conv3x3(wp, x, y, ci, co, res=t["res"], bias=t["bias"], **kw)
    finally:
        ops.TIMER = None
    launch = timer.records[-1][0]
    timer.summary()
    yx = None
    if launch.startswith("conv3x3_f16x3"):
        # the split conv's own op-test bar (test_gpu_ops.test_conv3x3_f16x3): 2x the exact-f32 kernel on the same
        # inputs + fp32 output rounding.  Three fp16 products with a 2^-22 residual each put it at 3.5-5.5x plain fp32
        # per launch, above the ledger's K = 4 (which the models still meet: tests/test_gpu_precision.py)
        yx = torch.empty(y.shape, device=dev)
        rx = None if res0 is None else res0.clone()
        ops.conv3x3(_hip.pack_conv3x3_weight(w).to(dev), x, yx, ci, co, res=rx, bias=t["bias"],
                    **{k: v for k, v in kw.items() if k not in ("ct", "ygroups")})
    rows = []
    wd = w.to(dev)
    for b in range(B):
        ys = {dt: _conv_ref(x[b, :ci], wd, t["bias"], None if res0 is None else res0[b], kw, dt)
              for dt in (torch.float64, torch.float32)}
        y64 = ys[torch.float64]
        row = _row("y", y[b][:y64.shape[0]], y64, ys[torch.float32])
        if yx is not None:
            ex = float((yx[b][:y64.shape[0]].double() - y64).abs().max())
            row = row[:3] + (2.0 * ex + 4e-7 * max(1.0, float(y64.abs().max())),)
        rows.append(row)
    return launch, rows


def _gemm_variant(r):
    """The VARIANTS entry a recorded GEMM launch maps to, from its plan (tag) and buffers."""
    d, kw = r["ds"], r["kw"]
    tag = dict(re.findall(r"\b(ct|yg)(\d+)\b", r["launch"]))
    B, _, H, W = d["x"]["shape"]
    N = H * W
    bs = [d[n]["stride"][0] for n in ("x", "y", "res") if d[n] is not None]
    vec = N % 4 == 0 and all(s % 4 == 0 for s in bs) and all(d[n]["align"] == 0 for n in ("x", "y", "res", "stats")
                                                              if d[n] is not None)
    return expected_variant(split=kw.get("split", False), M=r["M"], K=r["K"], N=N, B=B, ct=int(tag["ct"]), ygroups=int(tag["yg"]),
                            ln=kw.get("ln_mode", 0), res=d["res"] is not None, stats_out=d["stats_out"] is not None,
                            w_bs=kw.get("w_bs", 0), vec=vec)


@pytest.fixture(scope="module")
def table():
    yield _TABLE
    if _TABLE:
        print(f"\nproduction launches replayed: e <= {K} * e_32 + F * max|y64| (split conv: 2 e_exact-kernel + 4e-7 max(1, "
              "max|y64|)), worst image")
        print(f"{'workload':24s} {'launch':78s} {'n':>4s} {'row':4s} {'e':>10s} {'e_32':>10s} {'ratio':>7s}")
        for wl, launch, n, row, e, e32, ok in _TABLE:
            print(f"{wl:24s} {launch[:78]:78s} {n:4d} {row:4s} {e:10.3e} {e32:10.3e} "
                  f"{e / e32 if e32 else float('inf'):7.2f}{'' if ok else '  FAIL'}")


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_replay(dev, monkeypatch, table, name):
    recs = record(name, dev, monkeypatch)
    assert recs, f"{name}: no gemm1x1 / conv3x3 launch recorded"
    bad = []
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        for i, r in enumerate(recs):
            launch, rows = (replay_gemm if r["op"] == "gemm" else replay_conv)(r, dev, 1000 + i)
            if launch != r["launch"]:
                bad.append(f"replay logged {launch!r}, production {r['launch']!r}")
            for row in ("y", "mean", "rstd"):
                sel = [x for x in rows if x[0] == row]
                if not sel:
                    continue
                worst = max(sel, key=lambda x: x[1] - x[3])
                ok = all(e <= bar for _, e, _, bar in sel)
                table.append((name, r["launch"], r["count"], row, worst[1], worst[2], ok))
                if not ok:
                    bad.append(f"{r['launch']} {row}: e {worst[1]:.3e} e_32 {worst[2]:.3e}")
            torch.cuda.empty_cache()
    finally:
        torch.backends.cuda.matmul.allow_tf32 = prev
    assert not bad, bad


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_production_gemms_are_in_the_grid(dev, monkeypatch, name):
    """Every GEMM launch production issues maps to a VARIANTS entry, i.e. one the variant grid tests."""
    recs = record(name, dev, monkeypatch)
    out = [(r["launch"], _gemm_variant(r)) for r in recs if r["op"] == "gemm"]
    for launch, v in out:
        print(f"{name:24s} {launch:70s} -> {v}")
    missing = sorted({f"{v} ({launch})" for launch, v in out if v not in VARIANTS})
    assert not missing, f"production runs variants the grid does not test: {missing}"


def _conv_variant(r):
    """(CONV_VARIANTS entry, pass structure) a recorded conv launch maps to, from its kernel group and plan (tag) and its
    buffers; packed weights are whole allocations, 16-byte aligned."""
    d = r["ds"]
    kind = {"conv3x3_thin": "thin", "conv3x3_f16x3": "split", "conv3x3": "exact"}[r["launch"].split(" ")[0]]
    tag = dict(re.findall(r"\b(ct|yg)(\d+)\b", r["launch"]))
    ct = int(tag["ct"]) if kind != "thin" else None
    res = d["res"]
    v = expected_conv_variant(kind, r["ci"], r["co"], d["x"]["shape"][3], ct, d["x"]["stride"][0], d["y"]["stride"][0],
                              res["stride"][0] if res is not None else 0, d["x"]["align"] == 0, d["y"]["align"] == 0,
                              res is None or res["align"] == 0, True)
    if v is None:
        return None, None
    structure = "single" if kind == "thin" else pass_structure(passes_per_group((r["co"] + 15) // 16, ct, int(tag["yg"])))
    return v[0], structure


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_production_convs_are_in_the_grid(dev, monkeypatch, name):
    """Every conv launch production issues maps to a CONV_VARIANTS entry, and runs a pass structure (a single pass per
    workgroup, or several with an even or an uneven split over the groups) that variant has a case for."""
    recs = record(name, dev, monkeypatch)
    out = [(r["launch"], *_conv_variant(r)) for r in recs if r["op"] == "conv"]
    for launch, v, structure in out:
        print(f"{name:24s} {launch:70s} -> {v} {structure}")
    missing = sorted({f"{v} {structure} ({launch})" for launch, v, structure in out
                      if v not in CONV_VARIANTS or structure not in CASE_STRUCTURES[v]})
    assert not missing, f"production runs conv variants or pass structures the grid does not test: {missing}"
