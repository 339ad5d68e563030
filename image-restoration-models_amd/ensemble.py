"""x8 self-ensemble with partitioned forward: the reference's MaIR+ inference mode (mairplus_model.py) and, without
the partitions, SRModel.test_selfensemble (sr_model.py:132-178).

The reference augments the input 8 ways (identity, vflip, hflip, both, and the transposes of those four), runs every
variant through the network as a grid of overlapping partitions of about 200 px ("chop and shave": 10 % overlap, a
right/bottom reflect pad so that the grid divides evenly), stitches the partition interiors at output scale, undoes
the transforms and takes the mean.  Here the data movement on either side of the network is one HIP kernel each
(csrc/ensemble.hip): ``irm_dihedral_chop_f32`` writes every partition of every variant straight into batched network
inputs, ``irm_ensemble_merge_f32`` reads the predictions and writes the mean.  Partitions of equal shape - across
variants and images - form one batch.

The geometry planner below is pure Python and needs no GPU.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
from torch import nn

from . import _hip, ops

#: partition target of the reference (one_img_test: `h // 200 + 1` sections) and its overlap (`split // 10`)
CHOP_SIZE, SHAVE_DIV = 200, 10
NUM_VARIANTS = 8


def variant_flags(variant: int) -> tuple:
    """(vflip, hflip, transpose) of variant 0..7 in the reference's order: aug = T^tr(hflip^hf(vflip^vf(img)))."""
    if not 0 <= variant < NUM_VARIANTS:
        raise ValueError(f"variant {variant}: the dihedral group has 8 members, 0..7")
    return bool(variant & 1), bool(variant & 2), bool(variant & 4)


def augment(x: torch.Tensor, variant: int) -> torch.Tensor:
    """The variant composed from torch ops (tests, tools: the kernels' data-movement oracle)."""
    vf, hf, tr = variant_flags(variant)
    if vf:
        x = x.flip(-2)
    if hf:
        x = x.flip(-1)
    return x.transpose(-2, -1) if tr else x


def deaugment(y: torch.Tensor, variant: int) -> torch.Tensor:
    vf, hf, tr = variant_flags(variant)
    if tr:
        y = y.transpose(-2, -1)
    if hf:
        y = y.flip(-1)
    if vf:
        y = y.flip(-2)
    return y


def chop_torch(x: torch.Tensor, variant: int, chop: bool = True) -> list:
    """The partitions of one variant composed from torch ops, in grid order: flip / transpose, reflect pad, slice.
    Not on the product path: the data-movement oracle of tests/test_gpu_ensemble.py and the baseline that
    tools/bench_mair_plus.py times against the chop kernel."""
    p = plan(x.shape[-2], x.shape[-1], variant, chop)
    a = torch.nn.functional.pad(augment(x, variant), (0, p.pad[1], 0, p.pad[0]), 'reflect')
    return [a[..., y0:y1, x0:x1] for (y0, y1, x0, x1) in p.rects]


def merge_torch(preds: list, H: int, W: int, scale: int = 1, chop: bool = True) -> torch.Tensor:
    """preds[variant][partition] ([B, Co, s ph, s pw], grid order) -> the stitched, cropped, de-augmented mean,
    composed from torch ops (slice writes, transpose, flips, stack + mean).  Not on the product path, see chop_torch."""
    s, outs = scale, []
    for v, parts in enumerate(preds):
        p = plan(H, W, v, chop)
        B, Co = parts[0].shape[:2]
        canvas = torch.zeros(B, Co, s * (p.size[0] + p.pad[0]), s * (p.size[1] + p.pad[1]), dtype=parts[0].dtype,
                             device=parts[0].device)
        for part, ((Y0, Y1, X0, X1), (oy, ox)) in zip(parts, p.interiors):
            canvas[..., s * Y0:s * Y1, s * X0:s * X1] = part[..., s * oy:s * (oy + Y1 - Y0), s * ox:s * (ox + X1 - X0)]
        outs.append(deaugment(canvas[..., :s * p.size[0], :s * p.size[1]], v))
    return torch.stack(outs).mean(0)


class AxisPlan(NamedTuple):
    """One axis of the augmented image: `n` sections of `split` after a reflect pad of `pad`; partition i is
    [starts[i], stops[i]) of the padded axis and its interior begins `inner[i]` pixels in."""
    n: int
    pad: int
    split: int
    shave: int
    starts: tuple
    stops: tuple
    inner: tuple


def plan_axis(extent: int, chop: bool = True) -> AxisPlan:
    n = extent // CHOP_SIZE + 1 if chop else 1
    pad = (n - extent % n) % n
    split = (extent + pad) // n
    shave = split // SHAVE_DIV
    starts = tuple(i * split - (shave if i > 0 else 0) for i in range(n))
    stops = tuple((i + 1) * split + (shave if i + 1 < n else 0) for i in range(n))
    inner = tuple(shave if i > 0 else 0 for i in range(n))
    return AxisPlan(n, pad, split, shave, starts, stops, inner)


class VariantPlan(NamedTuple):
    """Geometry of one variant.  Everything is in the coordinates of the AUGMENTED image (extents `size`), at input
    scale: rects[i * grid[1] + j] = (y0, y1, x0, x1) of partition (i, j) in the padded image, interiors[...] =
    ((Y0, Y1, X0, X1) in the padded output, (oy, ox) offset of that interior inside the partition's prediction)."""
    variant: int
    size: tuple
    pad: tuple
    grid: tuple
    split: tuple
    shave: tuple
    rects: tuple
    interiors: tuple
    rows: AxisPlan
    cols: AxisPlan


def plan(H: int, W: int, variant: int, chop: bool = True) -> VariantPlan:
    """(H, W, variant) -> pad, grid, partition rects, interior rects.  The reference pads and chops the augmented image,
    so a transposing variant plans the swapped extents."""
    tr = variant_flags(variant)[2]
    ha, wa = (W, H) if tr else (H, W)
    r, c = plan_axis(ha, chop), plan_axis(wa, chop)
    rects = tuple((r.starts[i], r.stops[i], c.starts[j], c.stops[j]) for i in range(r.n) for j in range(c.n))
    interiors = tuple(((i * r.split, (i + 1) * r.split, j * c.split, (j + 1) * c.split), (r.inner[i], c.inner[j]))
                      for i in range(r.n) for j in range(c.n))
    return VariantPlan(variant, (ha, wa), (r.pad, c.pad), (r.n, c.n), (r.split, c.split), (r.shave, c.shave),
                       rects, interiors, r, c)


class Geometry(NamedTuple):
    """Host description of one (B, H, W) call: the int32 table of csrc/ensemble.hip ((8 + P) rows of 8), the shape groups
    [(ph, pw, n_tiles, pixel offset)] in packed order, and the launch extents."""
    table: np.ndarray
    groups: tuple
    total_pixels: int
    P: int
    max_ph: int
    max_pw: int


def geometry(B: int, H: int, W: int, chop: bool = True) -> Geometry:
    """Packed layout: the partitions of one shape back to back, [partition][image] -> a [n * B][C][ph][pw] batch."""
    plans = {v: plan(H, W, v, chop) for v in range(NUM_VARIANTS)}
    shapes: dict = {}
    for v, p in plans.items():
        for idx, (y0, y1, x0, x1) in enumerate(p.rects):
            shapes.setdefault((y1 - y0, x1 - x0), []).append((v, idx))
    P = sum(len(p.rects) for p in plans.values())
    table = np.zeros((NUM_VARIANTS + P, 8), np.int32)
    p0, first = 0, {}
    for v, p in plans.items():
        table[v, :7] = (p.grid[0], p.grid[1], p.split[0], p.split[1], p.shave[0], p.shave[1], p0)
        first[v] = p0
        p0 += len(p.rects)
    groups, off = [], 0
    for (ph, pw), members in shapes.items():
        groups.append((ph, pw, len(members) * B, off))
        for v, idx in members:
            y0, _, x0, _ = plans[v].rects[idx]
            table[NUM_VARIANTS + first[v] + idx, :6] = (v, y0, x0, ph, pw, off)
            off += B * ph * pw
    if off >= 2 ** 31:
        raise ValueError(f"self-ensemble of {B} x {H} x {W}: {off} packed pixels do not fit the int32 geometry table")
    return Geometry(table, tuple(groups), off, P, max(s[0] for s in shapes), max(s[1] for s in shapes))


_GEO_CACHE: dict = {}


def _geometry_on(device, B: int, H: int, W: int, chop: bool):
    """(Geometry, device table), cached per input shape like mairunet_arch.scan_ids: a captured forward enqueues
    kernels only (the eager warm-up of utils.graphed_forward fills the cache)."""
    key = (B, H, W, bool(chop), str(device))
    if key not in _GEO_CACHE:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("self-ensemble geometry for a new input shape inside a graph capture: run the shape "
                               "eagerly once first (utils.graphed_forward does)")
        g = geometry(B, H, W, chop)
        _GEO_CACHE[key] = (g, torch.from_numpy(g.table).to(device))
    return _GEO_CACHE[key]


# launches: like the tiler's kernels (utils.py) these move data around the network and are not part of a model's
# numerical path, so they sit beside their caller; ops._launch keeps them visible to an installed KernelTimer
def dihedral_chop(x: torch.Tensor, table: torch.Tensor, packed: torch.Tensor, geo):
    """x [B][C][H][W] -> every partition of every variant of `geo` (Geometry; `table` its device copy) in the
    packed buffer: 1 read of the image, 1 write of the partitions."""
    ops._chk(x, "x")
    if not x.is_contiguous() or table.dtype != torch.int32 or not table.is_cuda or packed.dtype != torch.float32:
        raise ValueError("dihedral_chop: contiguous float32 image, int32 device table, float32 packed buffer")
    B, C, H, W = x.shape
    if packed.numel() < geo.total_pixels * C or table.numel() < (8 + geo.P) * 8:
        raise ValueError("dihedral_chop: packed buffer or table smaller than the geometry")
    ops._launch("dihedral_chop", 0.0, 4.0 * C * (B * H * W + geo.total_pixels), "irm_dihedral_chop_f32", _hip.ptr(x),
            _hip.ptr(table), _hip.ptr(packed), packed.numel() // C, B, C, H, W, geo.P, geo.max_ph, geo.max_pw,
            tag=f"{H}x{W} B{B} P{geo.P}")


def ensemble_merge(pred: torch.Tensor, table: torch.Tensor, out: torch.Tensor, geo, scale: int):
    """Packed predictions (scale x the partitions of `geo`, all 8 variants) -> out [B][Co][scale H][scale W], the mean
    of the 8 de-augmented stitched results: 8 reads + 1 write of the output."""
    ops._chk(out, "out")
    if not out.is_contiguous() or table.dtype != torch.int32 or not table.is_cuda or pred.dtype != torch.float32:
        raise ValueError("ensemble_merge: contiguous float32 output, int32 device table, float32 packed predictions")
    B, Co, sH, sW = out.shape
    if sH % scale or sW % scale:
        raise ValueError(f"ensemble_merge: output {sH}x{sW} is not a multiple of scale {scale}")
    if pred.numel() < geo.total_pixels * Co * scale * scale or table.numel() < (8 + geo.P) * 8:
        raise ValueError("ensemble_merge: packed predictions or table smaller than the geometry")
    ops._launch("ensemble_merge", 7.0 * out.numel(), 36.0 * out.numel(), "irm_ensemble_merge_f32", _hip.ptr(pred),
            _hip.ptr(table), _hip.ptr(out), pred.numel() // (Co * scale * scale), B, Co, sH // scale, sW // scale, geo.P,
            int(scale), tag=f"{sH}x{sW} B{B} s{scale}")


def _size_multiple(net) -> int:
    """Spatial multiple the network's forward needs: its `size_multiple` attribute, 8 for the U-shaped built-ins."""
    m = getattr(net, "size_multiple", None)
    if m is not None:
        return int(m)
    from .mair import MaIRUNet
    from .restormer import Restormer
    return 8 if isinstance(net, (Restormer, MaIRUNet)) else 1


class SelfEnsemble(nn.Module):
    """forward(x [B, C, H, W]) -> [B, Co, s H, s W], s = net.upscale: the mean over the 8 dihedral variants of
    net(variant), each run as the reference's grid of overlapping partitions (chop=True: MaIR+) or whole (chop=False:
    test_selfensemble).  chop kernel -> net on each shape group, in sub-batches of net.max_tiles_per_batch -> merge
    kernel.  chop=True needs a network that takes any H x W (flat MaIR, DnCNN, REDNet); a network that needs multiples
    of 8 is refused with an error when a partition is not one."""

    def __init__(self, net: nn.Module, chop: bool = False):
        super().__init__()
        self.net = net
        self.chop = bool(chop)
        # utils.graphed_forward may capture the whole call iff it may capture the network: everything this module adds
        # is two kernels on the current stream, torch allocations and device-to-device copies
        self.hip_graph = bool(getattr(net, "hip_graph", False))

    @property
    def upscale(self) -> int:
        return int(getattr(self.net, "upscale", 1) or 1)

    @property
    def max_tiles_per_batch(self) -> int:
        return int(getattr(self.net, "max_tiles_per_batch", 8))

    def release_workspace(self):
        """utils.graphed_forward's contract: this module keeps no buffers of its own between calls (the geometry tables
        are immutable and shared), the network's workspace is the network's."""
        rel = getattr(self.net, "release_workspace", None)
        if callable(rel):
            rel()

    def _check_admissible(self, geo: Geometry):
        m = _size_multiple(self.net)
        bad = [(ph, pw) for ph, pw, _, _ in geo.groups if ph % m or pw % m]
        if bad:
            raise ValueError(f"{type(self.net).__name__} takes sizes that are multiples of {m}; the self-ensemble "
                             f"{'partitions ' if self.chop else 'inputs '}{bad} are not"
                             + (" (chop=True is for networks that take any size; use chop=False on padded input)"
                                if self.chop else ""))

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise _hip.HipLibraryError("the self-ensemble runs on the GPU only (no CPU fallback); move the model and "
                                       "input to 'cuda'")
        if x.dim() != 4:
            raise ValueError(f"SelfEnsemble: expected [B, C, H, W], got {tuple(x.shape)}")
        x = x.float().contiguous()
        B, C, H, W = x.shape
        geo, table = _geometry_on(x.device, B, H, W, self.chop)
        self._check_admissible(geo)
        s, cap = self.upscale, max(self.max_tiles_per_batch, 1)
        packed = torch.empty(geo.total_pixels * C, dtype=torch.float32, device=x.device)
        dihedral_chop(x, table, packed, geo)
        pred, Co = None, None
        for ph, pw, n, off in geo.groups:
            tiles = packed[off * C:(off + n * ph * pw) * C].view(n, C, ph, pw)
            for i in range(0, n, cap):
                o = self.net(tiles[i:i + cap])
                k = min(cap, n - i)
                if pred is None:
                    Co = int(o.shape[1])
                    pred = torch.empty(geo.total_pixels * Co * s * s, dtype=torch.float32, device=x.device)
                if tuple(o.shape) != (k, Co, s * ph, s * pw):
                    raise ValueError(f"SelfEnsemble: net.upscale = {s}: expected {(k, Co, s * ph, s * pw)} for "
                                     f"{ph}x{pw} partitions, got {tuple(o.shape)}")
                pred[off * Co * s * s:(off + n * ph * pw) * Co * s * s].view(n, Co, s * ph, s * pw)[i:i + k].copy_(o)
        out = torch.empty(B, Co, s * H, s * W, dtype=torch.float32, device=x.device)
        ensemble_merge(pred, table, out, geo, s)
        return out
