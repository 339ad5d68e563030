"""Glue API with the reference's call surface (src/utils.py): model factory,
patch-config lookup and the tiled-patch inference loop; the metrics (metrics.py),
the super-resolution resize (resize.py), NIQE (niqe.py), the YUV 4:2:0
conversions (yuv.py) and the frame stream (stream.py) are re-exported.

The hot loop (reference: src/utils.py:353-454, one synchronous forward + D2H +
numpy blend per tile) runs here as ONE device pipeline per image:
``irm_tile_extract`` (normalise / seeded noise / reflect pad) -> batched model
forward over all tiles -> ``irm_window_blend`` (Gaussian blend, /weight,
requantise) -> one D2H of the uint8 result.  Results equal the reference loop's
given equal per-tile predictions (same float32 operation order).
"""
from __future__ import annotations

import contextlib
import dataclasses
import gc
import os
import time
from typing import Callable

import numpy as np
import torch
from torch.nn import Module

from . import _hip, deblurganv2, dncnn, mair, ops, rednet, restormer, yuv
from .frames import device_constant, to_device, to_host
from .metrics import (calculate_metrics, calculate_metrics_basicsr, calculate_metrics_basicsr_device,  # noqa: F401
                      calculate_metrics_device, frame_metrics_basicsr_device, frame_metrics_device, psnr, ssim)
from .niqe import (calculate_niqe, calculate_niqe_device, load_niqe_params, niqe_feature_distance,  # noqa: F401
                   niqe_features, niqe_features_device, niqe_gamma_table, niqe_plane, niqe_score)
from .resize import imresize_device, imresize_host, mod_crop, resize_table  # noqa: F401
from .yuv import (YUV_FORMATS, rgb_to_yuv420_device, rgb_to_yuv420_host, yuv420_to_rgb_device,  # noqa: F401
                  yuv420_to_rgb_host)
from .stream import group_frames, run_model_inference_stream  # noqa: F401
from .convnet_common import check_precision
from .configs import PATCH_CONFIG, ROOT_RESULTS_DIR, ROOT_WEIGHTS_DIR
from .restormer import Restormer
from .mair import MaIR, MaIRPlus, MaIRUNet
from .deblurganv2 import FPNInception, FPNMobileNet

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))

#: model classes whose forward is the HIP path (isinstance dispatch as in utils.py:280/292)
_PAD8_MODELS = (Restormer, MaIR, MaIRUNet, MaIRPlus)


def get_model_total_parameters(model: Module) -> int:
    return sum(p.numel() for p in model.parameters())


def add_gaussian_noise(img: np.ndarray, sigma: int | float = 15):
    """src/utils.py:29-36 (seed 0 on every call, float64 noise added into a float32 array)."""
    if img.dtype != np.float32 and img.dtype != np.float64:
        img = img.astype(np.float32) / 255.
    np.random.seed(seed=0)
    img += np.random.normal(0, sigma / 255., img.shape)
    return np.clip(img, 0, 1).astype(np.float32)


def normalize(img: np.ndarray):
    """src/utils.py:159-171."""
    if img.dtype == np.uint16:
        out = img.astype(np.float32) / 65535.0
    elif img.dtype == np.uint8:
        out = img.astype(np.float32) / 255.0
    else:
        peak = np.max(img)
        out = img.astype(np.float32) / peak if peak > 1.0 else img.astype(np.float32)
    return out.astype(np.float32)


def pad(x: torch.Tensor, downscale_factor: int = 8):
    """src/utils.py:174-181: reflect-pad right/bottom to the next multiple of the factor."""
    h, w = x.shape[-2:]
    padh = (h // downscale_factor + 1) * downscale_factor - h if h % downscale_factor else 0
    padw = (w // downscale_factor + 1) * downscale_factor - w if w % downscale_factor else 0
    return torch.nn.functional.pad(x, (0, padw, 0, padh), 'reflect')


def get_gaussian_weights(height: int, width: int, n_channels=3, sigma_scale=0.125):
    """src/utils.py:314-350: Gaussian blending window, float64 maths, centre at size/2."""
    yy = (np.arange(height) - height / 2.0) ** 2 / (2 * (height * sigma_scale) ** 2)
    xx = (np.arange(width) - width / 2.0) ** 2 / (2 * (width * sigma_scale) ** 2)
    g = np.exp(-(yy[:, None] + xx[None, :]))
    return np.repeat(g[:, :, np.newaxis], n_channels, axis=2).astype(np.float32)


def get_patch_config(task, subtask, model_name) -> dict | None:
    """src/utils.py:184-213."""
    model_key = model_name.split(' ')[0]
    if model_key == 'MaIR+':                      # the same network under the x8 self-ensemble: the same tiles
        model_key = 'MaIR'
    config = PATCH_CONFIG.get(model_key, None)
    if isinstance(config, list):
        if model_key == 'DeblurGANv2':
            config = config[0] if 'Inception' in model_name else config[1]
        elif model_key == 'MaIR':
            config = config[0] if subtask.lower() == 'gaussian' else config[1]
        elif model_key == 'Restormer':
            config = config[0] if task.lower() == 'denoising' else config[1]
        else:
            config = config[0]
    return config


def _restormer_opt(name: str) -> str:
    return os.path.join(_PKG_DIR, 'restormer', 'options', name + '.yml')


#: the model families that have the reduced-precision mode (get_model_instance(..., precision="fp16"))
HALF_PRECISION_FAMILIES = ('DnCNN', 'REDNet')


def get_model_instance(task, subtask, model_name, device: torch.device, gray=False,
                       sigma: int | float | None = None, precision: str = "fp32") -> torch.nn.Module:
    """src/utils.py:216-267: same (task, subtask, model, gray, sigma) -> weights table.  precision="fp16" (DnCNN and
    REDNet only, not reference-parity) selects their native-fp16 kernels."""
    model_key = model_name.split(' ')[0]
    check_precision(precision, "get_model_instance")
    if precision == "fp16" and model_key not in HALF_PRECISION_FAMILIES:
        raise ValueError(f"precision='fp16' is available for {' and '.join(HALF_PRECISION_FAMILIES)} only, "
                         f"not for {model_key}")
    if model_key == 'REDNet':
        if task == 'denoising' and subtask == 'gaussian' and sigma is not None:
            return rednet.get_model(f'{ROOT_WEIGHTS_DIR}/REDNet/{sigma}.pt', device, precision=precision)
    elif model_key == 'DnCNN':
        if task == 'denoising' and subtask == 'gaussian':
            if gray:
                if sigma is not None:
                    return dncnn.get_model(f'{ROOT_WEIGHTS_DIR}/DnCNN/dncnn_{sigma}.pth', 1, 17, device,
                                           precision=precision)
                return dncnn.get_model(f'{ROOT_WEIGHTS_DIR}/DnCNN/dncnn_gray_blind.pth', 1, 20, device,
                                       precision=precision)
            if sigma is None:
                return dncnn.get_model(f'{ROOT_WEIGHTS_DIR}/DnCNN/dncnn_color_blind.pth', 3, 20, device,
                                       precision=precision)
    elif model_key == 'Restormer':
        kind = 'Gray' if gray else 'Color'
        if task == 'denoising':
            if subtask == 'gaussian':
                suffix = f'Sigma{sigma}' if sigma is not None else ''
                return restormer.get_model(_restormer_opt(f'Gaussian{kind}Denoising_Restormer{suffix}'), device)
            if subtask == 'real':
                return restormer.get_model(_restormer_opt('RealDenoising_Restormer'), device)
        if task == 'deblurring':
            if subtask == 'defocus':
                if 'Dual-pixel' in model_name:
                    return restormer.get_model(_restormer_opt('DefocusDeblur_DualPixel_16bit_Restormer'), device)
                return restormer.get_model(_restormer_opt('DefocusDeblur_Single_8bit_Restormer'), device)
            if subtask == 'motion':
                return restormer.get_model(_restormer_opt('Deblurring_Restormer'), device)
    elif model_key in ('MaIR', 'MaIR+'):
        opt_dir = os.path.join(_PKG_DIR, 'mair', 'options')
        plus = model_key == 'MaIR+'               # the same option files (model_type: MaIRPlusModel), wrapped
        if task == 'denoising':
            if subtask == 'gaussian' and not gray and sigma is not None:
                return mair.get_model(os.path.join(opt_dir, f'test_MaIR_CDN_s{sigma}.yml'), plus=plus)
            if subtask == 'real':
                return mair.get_model(os.path.join(opt_dir, 'test_MaIR_RealDN.yml'), plus=plus)
        if task == 'deblurring' and subtask == 'motion':
            return mair.get_model(os.path.join(opt_dir, 'test_MaIR_MotionDeblur.yml'), plus=plus)
    elif model_key == 'DeblurGANv2':
        if task == 'deblurring' and subtask == 'motion':
            if 'Inception' in model_name:
                return deblurganv2.get_model(f'{ROOT_WEIGHTS_DIR}/DeblurGANv2/fpn_inception.h5', device)
            if 'MobileNet' in model_name:
                return deblurganv2.get_model(f'{ROOT_WEIGHTS_DIR}/DeblurGANv2/fpn_mobilenet.h5', device)
    raise ValueError('No model instance found for current configuration.')


# ---------------------------------------------------------------------------
# tiled-patch inference
# ---------------------------------------------------------------------------

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
    if (is_f32 or f32_out) and hooks == "deblurganv2":
        raise ValueError("hooks='deblurganv2' normalises raw integer values and requantises: no float32 frames")
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
    if out not in ("same", "float32", "uint8", "uint16"):
        raise ValueError(f"out must be 'same', 'float32', 'uint8' or 'uint16', not {out!r}")
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


def run_model_inference(model: Module, input_img: np.ndarray, device: torch.device,
                        normalize: Callable = normalize, patch_size: int | None = None, patch_overlap: int = 32,
                        need_degradation=False, noise_level=None, pad: Callable | None = None,
                        postprocess: Callable | None = None, progress_bar=None):
    """Run inference; returns (prediction, inference_time_ms) like src/utils.py:353-454.

    uint8/uint16 and float32 HWC images with the stock normalize/pad hooks take
    the device pipeline (a float32 image by the reference's rule for float
    images: divided by its max where that exceeds 1, clipped to its own min /
    max, float32 out); anything else (float64 / float16 images, custom hooks,
    DeblurGANv2 on a float image) takes a per-tile loop with the reference's
    host-side blend - the model forward is the HIP path in both."""
    output_img, ms, _ = _run_model_inference(model, input_img, device, normalize, patch_size, patch_overlap,
                                             need_degradation, noise_level, pad, postprocess)
    return output_img, ms


def _run_model_inference(model, input_img, device, normalize=normalize, patch_size=None, patch_overlap=32,
                         need_degradation=False, noise_level=None, pad=None, postprocess=None):
    """run_model_inference that also hands back the device pipeline's output tensor (uint8, uint16 as int16 bits, or
    float32; None after the per-tile host loop): (prediction, inference_time_ms, out_dev).  The time covers the same work as
    run_model_inference's, input upload through output download."""
    start_time = time.time()
    out = None
    _upscale(model, need_degradation)
    dg = (normalize is deblurganv2.normalize and pad is deblurganv2.pad and postprocess is deblurganv2.postprocess
          and input_img.dtype == np.uint8)
    stock = dg or (normalize is globals()['normalize'] and (pad is None or pad is globals()['pad'])
                   and postprocess is None
                   and (input_img.dtype in (np.uint8, np.uint16)
                        or (input_img.dtype == np.float32 and input_img.ndim == 3)))
    with torch.no_grad():
        if stock:
            img_dev = to_device(input_img, torch.device(device))
            sigma = noise_level if (need_degradation and noise_level is not None) else None
            out, _ = tiled_forward_device(model, img_dev, patch_size, patch_overlap, pad is not None, sigma,
                                          max_batch=getattr(model, 'max_tiles_per_batch', 8),
                                          hooks="deblurganv2" if dg else None)
            output_img = to_host(out)
        else:
            output_img = _run_tiles_on_host(model, input_img, device, normalize, patch_size, patch_overlap,
                                            need_degradation, noise_level, pad, postprocess)
    return output_img, (time.time() - start_time) * 1000, out


def _run_tiles_on_host(model, input_img, device, normalize_fn, patch_size, patch_overlap, need_degradation,
                       noise_level, pad_fn, postprocess):
    """Per-tile loop with arbitrary hooks (reference order of operations, utils.py:379-450)."""
    img = normalize_fn(input_img)
    h, w = img.shape[:2]
    ps, origins = tile_plan(h, w, patch_size, patch_overlap)[:2]
    c_out = min(3, img.shape[2])
    s = _upscale(model)                               # super resolution: blend at output scale
    acc = np.zeros((s * h, s * w, c_out), np.float32)
    wsum = np.zeros((s * h, s * w, c_out), np.float32)
    win = get_gaussian_weights(s * ps, s * ps, c_out)
    for y0, x0 in origins:
        tile = img[y0:y0 + ps, x0:x0 + ps, :].copy()
        if need_degradation and noise_level is not None:
            tile = add_gaussian_noise(tile, noise_level)
        t = torch.from_numpy(tile.transpose(2, 0, 1)).unsqueeze(0).to(device)
        if pad_fn is not None:
            hp, wp = t.shape[-2:]
            o = model(pad_fn(t))[:, :, :s * hp, :s * wp]
        else:
            o = model(t)
        if postprocess is not None:
            o = postprocess(o)
        p = o.squeeze(0).cpu().numpy().transpose(1, 2, 0)
        ch, cw = p.shape[:2]
        acc[s * y0:s * y0 + ch, s * x0:s * x0 + cw, :] += p * win[:ch, :cw]
        wsum[s * y0:s * y0 + ch, s * x0:s * x0 + cw, :] += win[:ch, :cw]
    acc /= np.maximum(wsum, 1e-8)
    if input_img.dtype == np.uint16:
        return np.clip(acc * 65535.0, 0, 65535).round().astype(np.uint16)
    if input_img.dtype == np.uint8:
        return np.clip(acc * 255.0, 0, 255).round().astype(np.uint8)
    lo, hi = np.min(input_img), np.max(input_img)
    return np.clip(acc * hi, lo, hi).astype(input_img.dtype)


def get_model_prediction(model: Module, input_image: np.ndarray, device: torch.device, patch_size: int,
                         patch_overlap: int, need_degradation=False, noise_level=None, progress_bar=None):
    """src/utils.py:270-311: dispatch on the model class (reflect-pad-to-8 models vs plain)."""
    pred, ms, _ = _get_model_prediction(model, input_image, device, patch_size, patch_overlap, need_degradation,
                                        noise_level)
    return pred, ms


def _get_model_prediction(model, input_image, device, patch_size, patch_overlap, need_degradation=False,
                          noise_level=None):
    """get_model_prediction through _run_model_inference: (prediction, inference_time_ms, out_dev or None)."""
    kw = dict(patch_size=patch_size, patch_overlap=patch_overlap, need_degradation=need_degradation,
              noise_level=noise_level)
    hooks, pad8 = _model_hooks(model)
    if hooks == "deblurganv2":                                  # utils.py:280-291
        return _run_model_inference(model, input_image, device, normalize=deblurganv2.normalize, pad=deblurganv2.pad,
                                    postprocess=deblurganv2.postprocess, **kw)
    if pad8:
        return _run_model_inference(model, input_image, device, pad=pad, **kw)
    return _run_model_inference(model, input_image, device, **kw)


def _model_hooks(model) -> tuple:
    """(hooks, pad8) of the device pipeline for a model, by its class as the reference dispatches (utils.py:270-311):
    ("deblurganv2", True) for the two DeblurGANv2 generators, (None, True) - reflect pad to a multiple of 8 - for
    Restormer and MaIR, (None, False) otherwise."""
    if isinstance(model, (FPNMobileNet, FPNInception)):
        return "deblurganv2", True
    return None, isinstance(model, _PAD8_MODELS)


def _chain_hooks(model) -> bool:
    """pad8 of a chain stage, by the model class as _get_model_prediction dispatches; DeblurGANv2 is refused."""
    if isinstance(model, FPNMobileNet) or type(model).__module__.startswith(deblurganv2.__name__ + "."):
        raise ValueError("run_model_chain: DeblurGANv2 normalises raw integer values and has no float32 frames; "
                         "run it on its own with get_model_prediction")
    return isinstance(model, _PAD8_MODELS)


def run_model_chain(stages, input_img: np.ndarray, device: torch.device, need_degradation=False, noise_level=None,
                    out: str = "same"):
    """Run several restoration models one after another on one frame: denoise then deblur, denoise then
    super-resolve.  Returns (image, inference_time_ms), the time from input upload through output download.

    `stages` is a sequence of (model, patch_config) with patch_config = {'patch_size': .., 'patch_overlap': ..} as
    get_patch_config returns it.  Every stage is the device pipeline of run_model_inference with the hooks
    get_model_prediction picks for the model class (reflect pad to 8 for Restormer / MaIR); a DeblurGANv2 model
    raises ValueError.  The frame is uploaded once and downloaded once.

    The reference has no chain; these semantics are this package's own:
      1. the first stage reads the input as run_model_inference does (uint8 / 255, uint16 / 65535); a float32 input is
         taken as in [0, 1] already (unit_range=True of tiled_forward_device: no division by its max);
      2. every frame between two stages is float32, clipped to [0, 1] and never rounded to 255 levels - the next model
         does not see a quantisation step as new noise - and stays on the device;
      3. need_degradation / noise_level apply to the first stage only;
      4. the last stage requantises to the input's dtype as run_model_inference does, or returns the float32 frame in
         [0, 1] for a float32 input or with out="float32".
    Super-resolving stages enlarge the frame for the stages after them; a 6-channel first stage yields 3 channels.  A
    one-stage chain on a uint8 / uint16 frame returns exactly what get_model_prediction returns."""
    try:
        stages = [(m, dict(cfg)) for m, cfg in stages]
    except (TypeError, ValueError):
        raise ValueError("run_model_chain: stages is a sequence of (model, patch_config) pairs") from None
    if not stages:
        raise ValueError("run_model_chain: at least one stage")
    for m, cfg in stages:
        if not callable(m) or set(cfg) != {"patch_size", "patch_overlap"}:
            raise ValueError("run_model_chain: a stage is (model, {'patch_size': .., 'patch_overlap': ..})")
    pad8 = [_chain_hooks(m) for m, _ in stages]
    if out not in ("same", "float32"):
        raise ValueError(f"out must be 'same' or 'float32', not {out!r}")
    if (not isinstance(input_img, np.ndarray) or input_img.ndim != 3
            or input_img.dtype not in (np.uint8, np.uint16, np.float32)):
        raise ValueError("run_model_chain: a uint8, uint16 or float32 [H, W, C] array")
    _upscale(stages[0][0], need_degradation)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _hip.HipLibraryError("run_model_chain runs on the GPU only (no CPU fallback); pass a 'cuda' device")
    start_time = time.time()
    with torch.no_grad():
        frame = to_device(input_img, dev)
        sigma = noise_level if (need_degradation and noise_level is not None) else None
        last = len(stages) - 1
        final = "float32" if out == "float32" else str(input_img.dtype)      # the last stage requantises
        for i, ((m, cfg), p8) in enumerate(zip(stages, pad8)):
            kind = final if i == last else "float32"
            frame, _ = tiled_forward_device(m, frame, cfg["patch_size"], cfg["patch_overlap"], p8,
                                            sigma if i == 0 else None,
                                            max_batch=getattr(m, 'max_tiles_per_batch', 8), unit_range=True, out=kind)
        output_img = to_host(frame)
    return output_img, (time.time() - start_time) * 1000


def run_model_inference_yuv(model: Module, planes, device: torch.device, *, fmt, matrix="bt709", full_range=False,
                            siting="left", luma_only=False, patch_size: int | None = None, patch_overlap: int = 32,
                            need_degradation=False, noise_level=None):
    """Restore one YUV 4:2:0 video frame: returns (planes, inference_time_ms), the planes in the format they came in
    and the time from their upload through the download of the result, as run_model_inference's.

    `planes` are numpy arrays, (y, u, v) for fmt "i420" and (y, uv) for "nv12" / "p010" (yuv.py has the layouts).
    They go up as they are - 1.5 bytes per pixel, 3 for "p010" -, irm_yuv420_to_rgb_f32 makes the float32 RGB frame
    in [0, 1], the device pipeline of run_model_inference runs on it with the hooks get_model_prediction picks for
    the model class (unit_range=True, out="float32": the frame is never rounded to 255 RGB levels),
    irm_rgb_f32_to_yuv420 makes the planes and they come down.  matrix, full_range and siting describe the frame
    (DESIGN.md section 16).  A super-resolving model returns the planes of an s H x s W frame.

    luma_only=True restores Y alone with a one-channel model (REDNet, the gray DnCNN): the chroma planes are not
    uploaded and come back as they are, so an up-scaling model raises ValueError (the chroma would need a resize).
    DeblurGANv2 raises ValueError: its hooks are defined on raw integer values."""
    if model is None or not callable(model):
        raise ValueError("run_model_inference_yuv: model must be a model, not None")
    if isinstance(model, FPNMobileNet) or type(model).__module__.startswith(deblurganv2.__name__ + "."):
        raise ValueError("run_model_inference_yuv: DeblurGANv2 normalises raw integer values and has no float32 "
                         "frames; convert with yuv420_to_rgb_host and run it with get_model_prediction")
    yuv._check_options(fmt, matrix, siting)
    depth = YUV_FORMATS[fmt][1]
    yuv._check_planes(planes, fmt, False, np.ndarray, (np.uint16,) if depth == 10 else (np.uint8,))
    s = _upscale(model, need_degradation)
    if luma_only and s > 1:
        raise ValueError(f"luma_only with model.upscale = {s}: the chroma planes would need a resize")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _hip.HipLibraryError("run_model_inference_yuv runs on the GPU only (no CPU fallback); pass a 'cuda' device")
    opts = dict(matrix=matrix, full_range=full_range, siting=siting, luma_only=luma_only)
    start_time = time.time()
    with torch.no_grad():
        up = tuple(to_device(p, dev) for p in (planes[:1] if luma_only else planes))
        frame = yuv420_to_rgb_device(up, fmt, **opts)
        sigma = noise_level if (need_degradation and noise_level is not None) else None
        frame, _ = tiled_forward_device(model, frame, patch_size, patch_overlap, isinstance(model, _PAD8_MODELS), sigma,
                                        max_batch=getattr(model, 'max_tiles_per_batch', 8), unit_range=True,
                                        out="float32")
        if luma_only:
            rgb_to_yuv420_device(frame, fmt, out=up, **opts)           # same size: Y is overwritten in place
            result = (to_host(up[0]),) + tuple(planes[1:])
        else:
            # the planes of the result lie behind one another in one buffer, as a decoder lays them out: one download
            oh, ow = frame.shape[0], frame.shape[1]
            sizes = [oh * ow] + ([oh * ow // 4] * 2 if fmt == "i420" else [oh * ow // 2])
            shapes = [(oh, ow)] + ([(oh // 2, ow // 2)] * 2 if fmt == "i420" else [(oh // 2, ow // 2, 2)])
            buf = torch.empty(sum(sizes), dtype=up[0].dtype, device=dev)
            rgb_to_yuv420_device(frame, fmt, out=tuple(p.view(s) for p, s in zip(buf.split(sizes), shapes)), **opts)
            host = to_host(buf)
            result = tuple(p.reshape(s) for p, s in zip(np.split(host, np.cumsum(sizes)[:-1]), shapes))
    return result, (time.time() - start_time) * 1000
