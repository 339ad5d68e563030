"""The device tile pipeline, the layer under the reference's call surface (utils.py) and the frame stream (stream.py).

The reference's hot loop (src/utils.py:353-454, one synchronous forward + D2H + numpy blend per tile) runs here as ONE
device pipeline per image: ``irm_tile_extract`` (normalise / seeded noise / reflect pad) -> batched model forward over
all tiles, replayed from a HIP graph (``graphed_forward``) -> ``irm_window_blend`` (Gaussian blend, /weight,
requantise).  Results equal the reference loop's given equal per-tile predictions (same float32 operation order).
Also here, once: what the pipeline does for a given model (``model_route``) and the refusals its callers share.
"""
from __future__ import annotations

import collections
import contextlib
import dataclasses
import gc
import os

import numpy as np
import torch
from torch.nn import Module

from . import _hip, deblurganv2, ops
from .deblurganv2 import FPNInception, FPNMobileNet
from .frames import device_constant
from .mair import MaIR, MaIRPlus, MaIRUNet
from .restormer import Restormer

#: model classes whose forward is the HIP path (isinstance dispatch as in utils.py:280/292)
_PAD8_MODELS = (Restormer, MaIR, MaIRUNet, MaIRPlus)


def get_gaussian_weights(height: int, width: int, n_channels=3, sigma_scale=0.125):
    """src/utils.py:314-350: Gaussian blending window, float64 maths, centre at size/2."""
    yy = (np.arange(height) - height / 2.0) ** 2 / (2 * (height * sigma_scale) ** 2)
    xx = (np.arange(width) - width / 2.0) ** 2 / (2 * (width * sigma_scale) ** 2)
    g = np.exp(-(yy[:, None] + xx[None, :]))
    return np.repeat(g[:, :, np.newaxis], n_channels, axis=2).astype(np.float32)


def tile_origins(extent: int, patch: int, overlap: int) -> list:
    """src/utils.py:385-388."""
    stride = max(patch - overlap, 1)
    return list(range(0, extent - patch, stride)) + [max(extent - patch, 0)]


def tile_plan(h: int, w: int, patch_size, patch_overlap, pad_mode: str = "none") -> tuple:
    """The tile geometry of an h x w image (src/utils.py:379-388): (ps, origins, th, tw, ph, pw) - the patch size, the
    (y0, x0) origins in the reference's loop order (rows outer), the extent of a tile and its padded extent: up to a
    multiple of 8 for "reflect8", to the next multiple of 32 - always more - for "zero32" (DeblurGANv2's pad)."""
    if patch_size:
        ps = min(patch_size, max(h, w))
        ys, xs = tile_origins(h, ps, patch_overlap), tile_origins(w, ps, patch_overlap)
    else:
        ps, ys, xs = max(h, w), [0], [0]
    th, tw = min(ps, h), min(ps, w)
    ph, pw = th, tw
    if pad_mode == "reflect8":
        ph, pw = -(-th // 8) * 8, -(-tw // 8) * 8
    elif pad_mode == "zero32":
        ph, pw = (th // 32 + 1) * 32, (tw // 32 + 1) * 32
    return ps, [(y0, x0) for y0 in ys for x0 in xs], th, tw, ph, pw


def _side_stream(device, index: int):
    return device_constant(("side_stream", str(device), index), lambda: torch.cuda.Stream(device=device))


def _window_on(device, ps: int) -> torch.Tensor:
    return device_constant(("window", str(device), ps),
                           lambda: torch.from_numpy(get_gaussian_weights(ps, ps, 1)[:, :, 0].copy()).to(device))


#: floats of workspace irm_frame_minmax_f32 never needs more than (include/irm_hip_frames.h)
_MINMAX_WS_FLOATS = 2048


def _unit_range_on(device) -> torch.Tensor:
    """The constant value range (lo, hi, mul) = (0, 1, 1) of a frame that is in [0, 1] by contract, as the three-float
    device buffer the float32 tiler kernels read: no division on the way in, clip(v, 0, 1) on the way out."""
    return device_constant(("unit_range", str(device)), lambda: torch.tensor([0.0, 1.0, 1.0], dtype=torch.float32).to(device))


def _frame_range_on(img_dev: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """(min, max, max) of a float32 device frame, the reference's value range for a float image (utils.py:159-171,
    450-454), as a three-float device buffer; enqueued, never read by the host.  Non-finite values are outside the
    contract."""
    rng = torch.empty(3, dtype=torch.float32, device=img_dev.device)
    _hip.call("irm_frame_minmax_f32", _hip.ptr(img_dev), img_dev.numel(), _hip.ptr(rng), _hip.ptr(ws), ws.numel())
    return rng


def _upscale(model, need_degradation=False) -> int:
    """s of a super-resolving model (its outputs are s x the tile), else 1; degrading its input is refused."""
    s = int(getattr(model, "upscale", 1) or 1)
    if need_degradation and s > 1:
        raise ValueError("need_degradation with a super-resolution model: the reference defines no SR degradation")
    return s


#: bound of the per-model graph cache: entries, and bytes of graph-owned memory (static buffers + workspaces)
_GRAPH_MAX_ENTRIES, _GRAPH_MAX_BYTES = 8, 96 << 30


def _release_workspace(model: Module):
    rel = getattr(model, "release_workspace", None)
    if callable(rel):
        rel()


@contextlib.contextmanager
def _no_cyclic_gc():
    """No cyclic garbage collection inside the block: a capture must not be where dead cycles are freed.  A dead
    cycle can hold GPU objects whose release synchronises - another model's HIP graph (its destructor synchronises
    the device on ROCm), pinned host memory - and a synchronising call is illegal while a stream captures: the
    error is raised inside a destructor and ends the process.  torch.cuda.graph collected garbage on entry once and
    no longer does by default; what is dead stays dead until the capture has ended."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def graphed_forward(model: Module, x: torch.Tensor) -> torch.Tensor:
    """model(x) replayed from a HIP graph where that pays: the conv stacks and MaIR at small images are bound by
    the host's launch rate (hundreds of kernels of 10-60 us per image), not by the GPU.

    Opt-in per model (`model.hip_graph = True`, the default of the built-in model classes); off while a KernelTimer
    is installed (per-launch events need eager launches) and with IRM_NO_GRAPH=1.  The first call for an (input
    shape, stream, weights version) runs eagerly once (weight packing, LDS attributes), then captures the forward on
    torch's capture stream - every kernel of libirm_hip.so is enqueued on torch's current stream and allocates
    nothing, so the capture holds plain kernel nodes; later calls copy the input into the graph's static buffer and
    replay.  The returned tensor is the graph's static output: consume it (on the same stream) before the next call,
    as the tiler does.

    Ownership: a graph's kernels hold raw pointers, so every buffer they touch must live exactly as long as the
    graph.  The model's workspace is therefore dropped before the capture (`release_workspace()`), re-allocated
    INSIDE it - from the graph's private memory pool - and dropped again afterwards: the pool keeps those blocks for
    the graph alone, and no later eager call, other input shape or other graph can be handed the same memory
    (DnCNN's eagerly allocated layer buffers were freed on a shape change while an older graph still wrote
    to them).  The graphs live on the model object (`model._irm_graphs`), so they die with it; entries of other
    weight versions are dropped, the rest is bounded (least recently used)."""
    if (ops.TIMER is not None or not getattr(model, "hip_graph", False) or os.environ.get("IRM_NO_GRAPH")
            or not x.is_cuda or torch.cuda.is_current_stream_capturing()):
        return model(x)
    graphs = model.__dict__.get("_irm_graphs")
    if graphs is None:
        graphs = model.__dict__["_irm_graphs"] = {}
    version = _hip.param_key(model)
    key = (tuple(x.shape), x.device.index, torch.cuda.current_stream().cuda_stream, version)
    ent = graphs.pop(key, None)
    if ent is None:
        for k in [k for k in graphs if k[3] != version]:
            del graphs[k]                            # stale weights
        model(x)                                     # eager warm-up (packs weights, sets kernel attributes)
        _release_workspace(model)
        static_in = x.clone()
        g = torch.cuda.CUDAGraph()
        before = torch.cuda.memory_reserved(x.device)
        with _no_cyclic_gc(), torch.cuda.graph(g):
            static_out = model(static_in)
        _release_workspace(model)                    # the buffers stay reserved in g's private pool
        ent = (g, static_in, static_out, max(torch.cuda.memory_reserved(x.device) - before, 0))
        while graphs and (len(graphs) >= _GRAPH_MAX_ENTRIES
                          or sum(e[3] for e in graphs.values()) + ent[3] > _GRAPH_MAX_BYTES):
            del graphs[next(iter(graphs))]           # least recently used first (dict order = recency, see below)
    graphs[key] = ent                                # (re-)insert at the end: most recently used
    g, static_in, static_out, _ = ent
    static_in.copy_(x)
    g.replay()
    return static_out


def tiled_forward_device(model: Module, img_dev: torch.Tensor, patch_size, patch_overlap, pad8: bool,
                         noise_sigma=None, target_dev: torch.Tensor | None = None, max_batch: int = 8,
                         keep_tiles: list | None = None, hooks: str | None = None, unit_range: bool = False,
                         out: str = "same"):
    """Device pipeline for one uint8/uint16/float32 HWC image already on the GPU.

    Returns (out HWC device tensor, sse device tensor or None): uint8/uint16 like the input, float32 for a float32
    input or with out="float32" (tiled_forward_device_batch has the rules for float frames).
    Nothing here synchronises with the host.  hooks="deblurganv2" selects that model's normalize / pad /
    postprocess (src/deblurganv2/__init__.py:11-28) instead of /255 and the reflect pad to 8.
    """
    outs = tiled_forward_device_batch(model, [img_dev], patch_size, patch_overlap, pad8, noise_sigma,
                                      None if target_dev is None else [target_dev], max_batch, keep_tiles, hooks,
                                      unit_range, out)
    return outs[0]


def _check_out(out: str, hooks=None, is_f32: bool = False) -> None:
    """The refusals of `out` that need no frame: a name that is none, and a float32 result of DeblurGANv2's hooks
    (is_f32: so is a float32 frame).  The stream raises them when it is called, the batch call where it always did."""
    if out not in ("same", "float32", "uint8", "uint16"):
        raise ValueError(f"out must be 'same', 'float32', 'uint8' or 'uint16', not {out!r}")
    if hooks == "deblurganv2" and (is_f32 or out == "float32"):
        raise ValueError("hooks='deblurganv2' normalises raw integer values and requantises: no float32 frames")


def _value_kinds(dtype, out: str, unit_range: bool, hooks, has_targets: bool) -> tuple:
    """What the pipeline reads and writes for frames of `dtype` asked for as `out`: (is_f32, f32_out, out_dtype,
    out_u16).  No GPU call: the combinations without a meaning are refused here."""
    is_f32 = dtype == torch.float32
    if dtype.is_floating_point and not is_f32:
        raise ValueError(f"the device pipeline takes uint8, uint16 and float32 frames, not {dtype}")
    own = "float32" if is_f32 else "uint16" if dtype in (torch.uint16, torch.int16) else "uint8"
    kind = own if out == "same" else out
    f32_out = kind == "float32"
    if not f32_out and kind != own and not (is_f32 and unit_range):
        raise ValueError(f"out={out!r} for a {own} frame: an integer result comes from a frame of that type, or from a "
                         "float32 frame with unit_range=True")
    _check_out(out, hooks, is_f32)
    if f32_out and has_targets:
        raise ValueError("targets_dev needs an integer result: a float32 frame has no integer squared error")
    out_dtype = dtype if kind == own else torch.uint8 if kind == "uint8" else torch.int16
    return is_f32, f32_out, out_dtype, kind == "uint16"


def _forward_tiles(model: Module, tiles: torch.Tensor, max_batch: int) -> torch.Tensor:
    """The model's predictions for all tiles: batches of max_batch through graphed_forward, or - experimental -
    model.num_streams tile groups on side streams."""
    NT, dev = tiles.shape[0], tiles.device
    nstreams = min(int(getattr(model, "num_streams", 1)), NT)
    if nstreams > 1 and not os.environ.get("IRM_EXPERIMENTAL_STREAMS"):
        # EXPERIMENTAL, off in the product: on some GPUs of the pool overlapping forwards were not bit-reproducible
        # (rare stale read of an in-place updated buffer, cause not established: DESIGN.md section 6)
        raise ValueError("model.num_streams > 1 is experimental (not bit-reproducible on every GPU, DESIGN.md section 6); "
                         "set IRM_EXPERIMENTAL_STREAMS=1 to run it")
    if nstreams > 1:
        # independent tile groups on separate HIP streams: one group's HBM-bound kernels overlap the
        # other's MFMA-bound GEMMs; the groups join before the blend
        main = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(main)
        per = -(-NT // nstreams)
        done, outs = [], []
        for gi, i in enumerate(range(0, NT, per)):
            st = _side_stream(dev, gi)
            st.wait_event(ready)
            with torch.cuda.stream(st):
                o = model(tiles[i:i + per])              # (side streams: eager)
                outs.append((i, o))
                ev = torch.cuda.Event()
                ev.record(st)
                done.append(ev)
        for ev in done:
            main.wait_event(ev)
        pred = torch.empty(NT, *outs[0][1].shape[1:], dtype=torch.float32, device=dev)
        for i, o in outs:
            pred[i:i + o.shape[0]] = o
            o.record_stream(main)
        return pred
    pred = None
    for i in range(0, NT, max_batch):
        x = tiles[i:i + max_batch]
        o = graphed_forward(model, x) if callable(getattr(model, "forward", None)) else model(x)
        if pred is None:
            pred = o if o.shape[0] == NT else torch.empty(NT, *o.shape[1:], dtype=torch.float32, device=dev)
        if pred is not o:
            pred[i:i + o.shape[0]] = o
    return pred


def tiled_forward_device_batch(model: Module, imgs_dev: list, patch_size, patch_overlap, pad8: bool,
                               noise_sigma=None, targets_dev: list | None = None, max_batch: int = 8,
                               keep_tiles: list | None = None, hooks: str | None = None, unit_range: bool = False,
                               out: str = "same") -> list:
    """The device pipeline for SEVERAL images of one shape at once (throughput serving; the reference's loop,
    src/utils.py:353-454, is one image and one tile at a time): the tiles of all images form one batch axis, so the
    low-resolution levels of the network fill the GPU and every kernel's tail is paid once per batch instead of once per
    image (Restormer, 1280x720: 53.8 ms for one frame, 52.3 ms per frame for two, tools/bench_batch.py).  Each image is
    extracted, blended, requantised and scored exactly as in the single-image call - but the Gram kernels' chunk plan follows
    the batch size, so a frame may differ from that call's by +-1 in 0.1 % of its bytes (tests/test_gpu_fullsize.py) - and
    the list of (out, sse) pairs is returned in order.

    Float frames.  A float32 [H, W, C] frame gives a float32 [s H, s W, min(3, C)] frame.  unit_range=False is the
    reference's rule for a float image (utils.py:159-171, 450-454): the frame's own min / max are reduced on the device
    (irm_frame_minmax_f32), the frame is divided by max where max > 1, and the result is clip(v * max, min, max) - a max
    below 1 multiplies too, as it does there.  unit_range=True takes the frame as in [0, 1] by contract: no reduction,
    no division, the result is clip(v, 0, 1).  out="float32" returns the float32 frame for a uint8 / uint16 input as
    well: extracted as always (/255, /65535), blended with the unit range and not rounded; out="uint8" / "uint16" (the
    bit pattern in an int16 tensor, as on the way in) requantises a float32 frame that is in [0, 1] (unit_range=True) as
    an integer frame is: rint(clip(v * peak, 0, peak)).  A float32 result has no
    integer squared error (targets_dev raises ValueError), and hooks="deblurganv2" is defined on raw integer values
    with an integer result (a float32 input or out="float32" raises ValueError).  Non-finite values in a float frame
    are outside the contract."""
    img0 = imgs_dev[0]
    plan = _tile_pipeline_plan(model, tuple(img0.shape), img0.dtype, img0.device, patch_size, patch_overlap, pad8,
                               noise_sigma, hooks, unit_range, out, targets_dev is not None,
                               frames=[(tuple(im.shape), im.dtype) for im in imgs_dev])
    return _tile_pipeline_run(model, plan, imgs_dev, targets_dev, max_batch, keep_tiles)


@dataclasses.dataclass
class TilePipelinePlan:
    """What the device pipeline needs for frames of one shape and dtype and does not depend on their values: the tile
    geometry, the origins, the blend window and the noise field on the device, the value kinds and the hook constants.
    _tile_pipeline_plan makes it (no launch), _tile_pipeline_run holds the launches."""
    h: int
    w: int
    c: int
    c_out: int
    s: int
    ps: int
    th: int
    tw: int
    ph: int
    pw: int
    T: int
    dtype: torch.dtype
    device: torch.device
    zero32: bool
    norm_mean: float
    norm_inv_std: float
    post_scale: float
    post_shift: float
    is_f32: bool
    f32_out: bool
    out_dtype: torch.dtype
    out_u16: bool
    unit_range: bool
    org: torch.Tensor
    window: torch.Tensor
    noise: torch.Tensor | None

    @property
    def frame_dtype(self) -> torch.dtype:
        """dtype of a result frame."""
        return torch.float32 if self.f32_out else self.out_dtype


def noise_field(sigma, shape) -> np.ndarray:
    """The float64 field add_gaussian_noise adds to every tile (src/utils.py:29-36): the values of
    np.random.seed(0); np.random.normal(0, sigma / 255., shape), drawn from a generator of their own so that the
    process-wide numpy state is left alone."""
    return np.random.RandomState(0).normal(0, sigma / 255., shape)


def _tile_pipeline_plan(model: Module, shape: tuple, dtype, dev, patch_size, patch_overlap, pad8: bool, noise_sigma,
                        hooks, unit_range: bool, out: str, has_targets: bool = False,
                        frames: list | None = None) -> TilePipelinePlan:
    """The plan of tiled_forward_device_batch for [H, W, C] frames of `dtype` on `dev`, with that call's checks in
    its order (`frames`: the (shape, dtype) of every frame of the batch).  The origins and the noise field are per-
    device constants: a call after the first uploads nothing and draws nothing on the host."""
    _check_out(out)
    norm_mean, norm_inv_std, post_scale, post_shift = 0.0, 1.0, 1.0, 0.0
    pad_mode = "reflect8" if pad8 else "none"
    if hooks == "deblurganv2":
        norm_mean = float(np.float32(0.5) * np.float32(255.0))
        norm_inv_std = float(np.float32(1.0) / (np.float32(0.5) * np.float32(255.0)))
        post_scale, post_shift, pad_mode = 0.5, 1.0, "zero32"
    s = _upscale(model, noise_sigma is not None)
    h, w, c = shape
    if any(sh != (h, w, c) or dt != dtype for sh, dt in frames or ()):
        raise ValueError("tiled_forward_device_batch: the images of a batch must share shape and dtype")
    is_f32, f32_out, out_dtype, out_u16 = _value_kinds(dtype, out, unit_range, hooks, has_targets)
    dev = torch.device(dev)
    ps, origins, th, tw, ph, pw = tile_plan(h, w, patch_size, patch_overlap, pad_mode)
    org = device_constant(("origins", str(dev), tuple(origins)),
                          lambda: torch.tensor(origins, dtype=torch.int32).to(dev))
    noise = None
    if noise_sigma is not None:                      # utils.py:33: same field for every tile
        noise = device_constant(("noise", str(dev), float(noise_sigma), th, tw, c),
                                lambda: torch.from_numpy(noise_field(noise_sigma, (th, tw, c))).to(dev))
    return TilePipelinePlan(h, w, c, min(3, c), s, ps, th, tw, ph, pw, len(origins), dtype, dev, pad_mode == "zero32",
                            float(norm_mean), float(norm_inv_std), post_scale, post_shift, is_f32, f32_out, out_dtype,
                            out_u16, bool(unit_range), org, _window_on(dev, s * ps), noise)


def _tile_pipeline_run(model: Module, plan: TilePipelinePlan, imgs_dev: list, targets_dev: list | None = None,
                       max_batch: int = 8, keep_tiles: list | None = None, frames_out: list | None = None) -> list:
    """The launches of tiled_forward_device_batch for the K frames `imgs_dev` of `plan`'s shape: extract, forward,
    blend, all on the current stream.  `frames_out`, K [s H, s W, c_out] tensors of plan.frame_dtype, receives the
    results (the stream's static output slots); without it the frames are allocated here."""
    p, dev = plan, plan.device
    h, w, c, s, T, K = p.h, p.w, p.c, p.s, p.T, len(imgs_dev)
    org, noise, th, tw, ph, pw = p.org, p.noise, p.th, p.tw, p.ph, p.pw
    tiles = torch.empty(K * T, c, ph, pw, dtype=torch.float32, device=dev)
    ranges = [_unit_range_on(dev)] * K if (p.is_f32 or p.f32_out) else None
    if p.is_f32 and not p.unit_range:
        ws = torch.empty(_MINMAX_WS_FLOATS, dtype=torch.float32, device=dev)      # (one stream: the frames take turns)
        ranges = [_frame_range_on(im, ws) for im in imgs_dev]
    for k, im in enumerate(imgs_dev):
        if p.is_f32:
            _hip.call("irm_tile_extract_f32", _hip.ptr(im), _hip.ptr(ranges[k]), _hip.ptr(org), _hip.ptr(noise),
                      _hip.ptr(tiles[k * T:]), h, w, c, th, tw, ph, pw, T, int(p.zero32))
        else:
            _hip.call("irm_tile_extract", _hip.ptr(im), int(p.dtype in (torch.uint16, torch.int16)), _hip.ptr(org),
                      _hip.ptr(noise), _hip.ptr(tiles[k * T:]), h, w, c, th, tw, ph, pw, T, p.norm_mean,
                      p.norm_inv_std, int(p.zero32))
    if ops.TIMER is not None:
        ops.TIMER.break_chain()                    # the tile extraction above is not a timed launch
    pred = _forward_tiles(model, tiles, max_batch)
    if s > 1 and tuple(pred.shape[2:]) != (s * ph, s * pw):
        raise ValueError(f"model.upscale = {s}: expected {s * ph}x{s * pw} predictions for {ph}x{pw} tiles, "
                         f"got {tuple(pred.shape[2:])}")
    if keep_tiles is not None:
        keep_tiles.append(pred[:, :p.c_out, :s * th, :s * tw].clone())
    results = []
    for k in range(K):
        frame = (frames_out[k] if frames_out is not None
                 else torch.empty(s * h, s * w, p.c_out, dtype=p.frame_dtype, device=dev))
        sse, tgt = None, None
        if targets_dev is not None and targets_dev[k] is not None:
            sse, tgt = torch.zeros(1, dtype=torch.int64, device=dev), targets_dev[k]
        if p.f32_out:
            # extents in input pixels, predictions and window at output scale (irm_hip_frames.h)
            _hip.call("irm_window_blend_f32", _hip.ptr(pred[k * T:]), _hip.ptr(org), _hip.ptr(p.window),
                      _hip.ptr(frame), _hip.ptr(ranges[k]), h, w, p.c_out, pred.shape[1], th, tw, pred.shape[2] // s,
                      pred.shape[3] // s, p.ps, T, s)
        elif s > 1:
            # tiles cut at input scale, blended at output scale: origins x s, window of s * ps (irm_hip.h)
            _hip.call("irm_window_blend_scaled", _hip.ptr(pred[k * T:]), _hip.ptr(org), _hip.ptr(p.window),
                      _hip.ptr(frame), int(p.out_u16), _hip.ptr(tgt), _hip.ptr(sse), h, w, p.c_out, pred.shape[1], th, tw,
                      ph, pw, p.ps, T, s, p.post_scale, p.post_shift)
        else:
            _hip.call("irm_window_blend", _hip.ptr(pred[k * T:]), _hip.ptr(org), _hip.ptr(p.window), _hip.ptr(frame),
                      int(p.out_u16), _hip.ptr(tgt), _hip.ptr(sse), h, w, p.c_out, pred.shape[1], th, tw,
                      pred.shape[2], pred.shape[3], p.ps, T, p.post_scale, p.post_shift)
        results.append((frame, sse))
    return results


def _model_hooks(model) -> tuple:
    """(hooks, pad8) of the device pipeline for a model, by its class as the reference dispatches (utils.py:270-311):
    ("deblurganv2", True) for the two DeblurGANv2 generators, (None, True) - reflect pad to a multiple of 8 - for
    Restormer and MaIR, (None, False) otherwise."""
    if isinstance(model, (FPNMobileNet, FPNInception)):
        return "deblurganv2", True
    return None, isinstance(model, _PAD8_MODELS)



Route = collections.namedtuple("Route", "hooks pad8 s sigma max_batch")


def model_route(model, need_degradation=False, noise_level=None) -> Route:
    """What the pipeline does for `model` in a call with these degradation arguments: hooks and pad8 by the model class,
    s = model.upscale (degrading a super-resolving model's input is refused), the sigma of the seeded noise or None,
    and the tiles of one forward.  The one-frame calls, the chain, the YUV call and the stream all read it here."""
    s = _upscale(model, need_degradation)
    sigma = noise_level if (need_degradation and noise_level is not None) else None
    return Route(*_model_hooks(model), s, sigma, getattr(model, 'max_tiles_per_batch', 8))


def is_deblurgan(model) -> bool:
    """FPNMobileNet, or any class defined under the deblurganv2 package: wider than _model_hooks' reference dispatch."""
    return isinstance(model, FPNMobileNet) or type(model).__module__.startswith(deblurganv2.__name__ + ".")


def refuse_deblurgan(model, who: str, instead: str) -> None:
    """ValueError where a frame is float32 by construction (a chain, YUV planes) and the model is DeblurGANv2."""
    if is_deblurgan(model):
        raise ValueError(f"{who}: DeblurGANv2 normalises raw integer values and has no float32 frames; {instead}")


def cuda_device(device, who: str) -> torch.device:
    """torch.device(device), or HipLibraryError where it is no GPU: no call of this package falls back to the CPU."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _hip.HipLibraryError(f"{who} runs on the GPU only (no CPU fallback); pass a 'cuda' device")
    return dev
