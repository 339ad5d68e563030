"""Glue API with the reference's call surface (src/utils.py): model factory,
patch-config lookup and the tiled-patch inference calls.  The device tile
pipeline they run on (pipeline.py: tile plan, graph cache, extract / forward /
blend), the metrics (metrics.py), the super-resolution resize (resize.py), NIQE
(niqe.py), LPIPS (perceptual.py), the YUV 4:2:0 conversions (yuv.py), the frame
stream (stream.py), the noise estimator (noise.py) and the aligned scores (align.py) are re-exported: every name this module had is
still reachable through it.  The bank of per-sigma checkpoints and the call that
routes a frame to the one for its estimated noise level live here.
"""
from __future__ import annotations

import os
import time
from typing import Callable

import numpy as np
import torch
from torch.nn import Module

from . import deblurganv2, dncnn, mair, rednet, restormer, yuv
from .align import (AlignedMetrics, align_to_target, align_to_target_device, calculate_metrics_aligned,  # noqa: F401
                    calculate_metrics_aligned_device, ecc_homography_device)
from .frames import plane_slots, to_device, to_host
from .metrics import (calculate_metrics, calculate_metrics_basicsr, calculate_metrics_basicsr_device,  # noqa: F401
                      calculate_metrics_device, calculate_metrics_f32_device, frame_metrics_basicsr_device,
                      frame_metrics_device, frame_metrics_f32_device, psnr, ssim)
from .noise import (estimate_noise_sigma, estimate_noise_sigma_device, estimate_noise_sigma_yuv,  # noqa: F401
                    estimate_noise_sigma_yuv_device, noise_sigma_from_stats, noise_stats, noise_stats_device,
                    noise_stats_yuv_device)
from .niqe import (calculate_niqe, calculate_niqe_device, load_niqe_params, niqe_feature_distance,  # noqa: F401
                   niqe_features, niqe_features_device, niqe_gamma_table, niqe_plane, niqe_score)
from .perceptual import (LpipsParams, calculate_lpips, calculate_lpips_device, frame_lpips_device,  # noqa: F401
                         load_lpips_params, lpips_params_from_state, lpips_taps)
from .pipeline import (_GRAPH_MAX_BYTES, _GRAPH_MAX_ENTRIES, _MINMAX_WS_FLOATS, _PAD8_MODELS, Restormer,  # noqa: F401
                       TilePipelinePlan, _forward_tiles, _frame_range_on, _model_hooks, _no_cyclic_gc,
                       _release_workspace, _side_stream, _tile_pipeline_plan, _tile_pipeline_run, _unit_range_on,
                       _upscale, _value_kinds, _window_on, cuda_device, get_gaussian_weights, graphed_forward,
                       is_deblurgan, model_route, noise_field, refuse_deblurgan, tile_origins, tile_plan,
                       tiled_forward_device, tiled_forward_device_batch)
from .resize import (RESIZE_KERNELS, Resize, imresize_device, imresize_host, mod_crop, resize_device,  # noqa: F401
                     resize_host, resize_plan, resize_table, resize_taps)
from .y4m import read_y4m, write_y4m  # noqa: F401
from .yuv import (YUV_FORMATS, YUV_LAYOUTS, YuvMetrics, calculate_metrics_yuv, calculate_metrics_yuv_device,  # noqa: F401
                  frame_metrics_yuv_device, rgb_to_yuv420_device, rgb_to_yuv420_host, rgb_to_yuv_device,
                  rgb_to_yuv_host, yuv420_to_rgb_device, yuv420_to_rgb_host, yuv_to_rgb_device, yuv_to_rgb_host)
from .stream import group_frames, run_model_inference_stream  # noqa: F401
from .convnet_common import check_precision
from .configs import PATCH_CONFIG, ROOT_RESULTS_DIR, ROOT_WEIGHTS_DIR

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))


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


def _is_patch_config(cfg) -> bool:
    """Whether cfg is {'patch_size': .., 'patch_overlap': ..}, the dict get_patch_config returns, and nothing else."""
    return isinstance(cfg, dict) and set(cfg) == {"patch_size", "patch_overlap"}


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
    return _run_model_inference(model, input_img, device, normalize, patch_size, patch_overlap, need_degradation,
                                noise_level, pad, postprocess)[:2]


def _run_model_inference(model, input_img, device, normalize=normalize, patch_size=None, patch_overlap=32,
                         need_degradation=False, noise_level=None, pad=None, postprocess=None):
    """run_model_inference that also hands back the device pipeline's output tensor (uint8, uint16 as int16 bits, or
    float32; None after the per-tile host loop): (prediction, inference_time_ms, out_dev).  The time covers the same work as
    run_model_inference's, input upload through output download."""
    start_time = time.time()
    out = None
    route = model_route(model, need_degradation, noise_level)       # the hooks are this call's arguments, not the route's
    dg = (normalize is deblurganv2.normalize and pad is deblurganv2.pad and postprocess is deblurganv2.postprocess
          and input_img.dtype == np.uint8)
    stock = dg or (normalize is globals()['normalize'] and (pad is None or pad is globals()['pad'])
                   and postprocess is None
                   and (input_img.dtype in (np.uint8, np.uint16)
                        or (input_img.dtype == np.float32 and input_img.ndim == 3)))
    with torch.no_grad():
        if stock:
            img_dev = to_device(input_img, torch.device(device))
            out, _ = tiled_forward_device(model, img_dev, patch_size, patch_overlap, pad is not None, route.sigma,
                                          max_batch=route.max_batch, hooks="deblurganv2" if dg else None)
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
    return _get_model_prediction(model, input_image, device, patch_size, patch_overlap, need_degradation, noise_level)[:2]


def _get_model_prediction(model, input_image, device, patch_size, patch_overlap, need_degradation=False,
                          noise_level=None):
    """get_model_prediction through _run_model_inference: (prediction, inference_time_ms, out_dev or None)."""
    kw = dict(patch_size=patch_size, patch_overlap=patch_overlap, need_degradation=need_degradation,
              noise_level=noise_level)
    hooks, pad8 = _model_hooks(model)
    if hooks == "deblurganv2":                                  # utils.py:280-291
        return _run_model_inference(model, input_image, device, normalize=deblurganv2.normalize, pad=deblurganv2.pad,
                                    postprocess=deblurganv2.postprocess, **kw)
    return _run_model_inference(model, input_image, device, pad=pad if pad8 else None, **kw)


class SigmaBank:
    """The checkpoints of one non-blind denoiser, one per noise level: `models` maps sigma (0..255 scale) to model.
    `levels` are the sigmas in ascending order; `pick` chooses the model for an estimated sigma."""

    def __init__(self, models: dict):
        try:
            items = sorted((float(s), s, m) for s, m in dict(models).items())
        except (TypeError, ValueError):
            raise ValueError("SigmaBank: models maps a positive sigma to a model") from None
        if not items or any(not (np.isfinite(f) and f > 0) or not callable(m) for f, _, m in items):
            raise ValueError("SigmaBank: models maps a positive sigma to a model, at least one")
        self.levels = [s for _, s, _ in items]
        self.models = {s: m for _, s, m in items}

    def pick(self, sigma_est) -> tuple:
        """(level, model) for an estimated sigma: the level nearest in log sigma, so the thresholds between two
        neighbours are their geometric mean (19.36 and 35.36 for 15 / 25 / 50); a tie goes to the lower level, an
        estimate <= 0 to the lowest.  NaN (a frame without an unsaturated block) raises ValueError."""
        sigma_est = float(sigma_est)
        if np.isnan(sigma_est):
            raise ValueError("SigmaBank.pick: the sigma estimate is NaN (no unsaturated block in the frame)")
        level = self.levels[0]
        for lo, hi in zip(self.levels, self.levels[1:]):
            if sigma_est > 0 and sigma_est * sigma_est > float(lo) * float(hi):      # above the geometric mean of the two neighbours
                level = hi
        return level, self.models[level]


def get_model_bank(task, subtask, model_name, device: torch.device, gray=False, sigmas=(15, 25, 50),
                   precision: str = "fp32") -> SigmaBank:
    """The SigmaBank of get_model_instance(task, subtask, model_name, device, gray, sigma, precision) over `sigmas`."""
    sigmas = list(sigmas)
    if not sigmas:
        raise ValueError("get_model_bank: at least one sigma")
    return SigmaBank({s: get_model_instance(task, subtask, model_name, device, gray=gray, sigma=s, precision=precision)
                      for s in sigmas})


def run_model_inference_auto(bank: SigmaBank, input_img: np.ndarray, device: torch.device,
                             patch_size: int | None = None, patch_overlap: int = 32):
    """Estimate the frame's noise level on the GPU and run the checkpoint trained for it: returns
    (prediction, inference_time_ms, sigma_est, sigma_used).

    The uint8 / uint16 frame is uploaded once; estimate_noise_sigma_device reads it there (one read-back of a few
    integers), bank.pick chooses the model, and the device pipeline call that get_model_prediction makes for that model
    (its hooks and pad8 by the model class) runs on the same device frame; one download.  The time covers all of it.  The
    prediction is byte-identical to get_model_prediction(bank.models[sigma_used], input_img, device, patch_size,
    patch_overlap).  There is no need_degradation: the frame is the noisy one, an estimate of a clean frame says
    nothing."""
    pred, ms, sigma_est, sigma_used, _ = _run_model_inference_auto(bank, input_img, device, patch_size, patch_overlap)
    return pred, ms, sigma_est, sigma_used


def _run_model_inference_auto(bank, input_img, device, patch_size=None, patch_overlap=32):
    """run_model_inference_auto that also hands back the device output tensor."""
    if not isinstance(bank, SigmaBank):
        raise ValueError("run_model_inference_auto: bank is a SigmaBank (get_model_bank)")
    if not isinstance(input_img, np.ndarray) or input_img.dtype not in (np.uint8, np.uint16):
        raise ValueError("run_model_inference_auto takes a uint8 or uint16 [H, W] or [H, W, C] array: a float frame has "
                         "no integer codes to estimate from")
    dev = cuda_device(device, "run_model_inference_auto")
    start_time = time.time()
    with torch.no_grad():
        img_dev = to_device(input_img, dev)
        sigma_est = estimate_noise_sigma_device(img_dev)
        sigma_used, model = bank.pick(sigma_est)
        route = model_route(model)
        out, _ = tiled_forward_device(model, img_dev, patch_size, patch_overlap, route.pad8, None,
                                      max_batch=route.max_batch, hooks=route.hooks)
        output_img = to_host(out)
    return output_img, (time.time() - start_time) * 1000, sigma_est, sigma_used, out


def run_model_chain(stages, input_img: np.ndarray, device: torch.device, need_degradation=False, noise_level=None,
                    out: str = "same"):
    """Run several restoration models one after another on one frame: denoise then deblur, denoise then
    super-resolve.  Returns (image, inference_time_ms), the time from input upload through output download.

    `stages` is a sequence of (model, patch_config) with patch_config = {'patch_size': .., 'patch_overlap': ..} as
    get_patch_config returns it.  Every stage is the device pipeline of run_model_inference with the hooks
    get_model_prediction picks for the model class (reflect pad to 8 for Restormer / MaIR); a DeblurGANv2 model
    raises ValueError.  A stage may also be a Resize(size=.. | scale=.., kernel, antialias): the frame is brought to
    that size on the device (resize_device).  The frame is uploaded once and downloaded once.

    The reference has no chain; these semantics are this package's own:
      1. the first stage reads the input as run_model_inference does (uint8 / 255, uint16 / 65535); a float32 input is
         taken as in [0, 1] already (unit_range=True of tiled_forward_device: no division by its max);
      2. every frame between two stages is float32, clipped to [0, 1] and never rounded to 255 levels - the next model
         does not see a quantisation step as new noise - and stays on the device;
      3. need_degradation / noise_level apply to the first stage only, which must then be a model;
      4. the last stage requantises to the input's dtype as run_model_inference does, or returns the float32 frame in
         [0, 1] for a float32 input or with out="float32";
      5. a Resize stage follows the same rules: as first stage it reads the uint8 / uint16 input directly; between two
         stages it maps the float32 frame to a float32 frame clamped to [0, 1] (out="unit": the overshoot of bicubic and
         Lanczos does not reach the next model, as a model stage's output is clipped); as last stage it requantises by
         the resize rule - clamp, x 255 (65535), round half to even - or returns the clamped float32 frame.  It resizes
         H first, then W, as basicsr's imresize does, not MATLAB's smaller-scale-first rule.  A chain of Resize stages
         alone is allowed.
    Super-resolving stages enlarge the frame for the stages after them; a 6-channel first stage yields 3 channels.  A
    one-stage chain on a uint8 / uint16 frame returns exactly what get_model_prediction returns (a model) or what
    resize_device returns (a Resize)."""
    def pair(model, cfg):
        return model, dict(cfg)
    try:
        stages = [st if isinstance(st, Resize) else pair(*st) for st in stages]
    except (TypeError, ValueError):
        raise ValueError("run_model_chain: stages is a sequence of (model, patch_config) pairs or Resize stages") from None
    if not stages:
        raise ValueError("run_model_chain: at least one stage")
    models = [st for st in stages if not isinstance(st, Resize)]
    for m, cfg in models:
        if not callable(m) or not _is_patch_config(cfg):
            raise ValueError("run_model_chain: a stage is (model, {'patch_size': .., 'patch_overlap': ..}) or a Resize")
    for m, _ in models:
        refuse_deblurgan(m, "run_model_chain", "run it on its own with get_model_prediction")
    if out not in ("same", "float32"):
        raise ValueError(f"out must be 'same' or 'float32', not {out!r}")
    if (not isinstance(input_img, np.ndarray) or input_img.ndim != 3
            or input_img.dtype not in (np.uint8, np.uint16, np.float32)):
        raise ValueError("run_model_chain: a uint8, uint16 or float32 [H, W, C] array")
    if need_degradation and isinstance(stages[0], Resize):
        raise ValueError("run_model_chain: need_degradation applies to the first stage, which is a Resize")
    routes = [None if isinstance(st, Resize) else model_route(st[0], need_degradation and i == 0, noise_level)
              for i, st in enumerate(stages)]
    h, w, c = input_img.shape
    for st, r in zip(stages, routes):                   # the sizes along the chain: a Resize that cannot run raises here
        if r is None:
            if c not in (1, 3):
                raise ValueError(f"run_model_chain: a Resize stage takes 1 or 3 channels, not {c}")
            h, w = st.plan(h, w)
        else:
            h, w, c = r.s * h, r.s * w, min(3, c)
    dev = cuda_device(device, "run_model_chain")
    start_time = time.time()
    with torch.no_grad():
        frame = to_device(input_img, dev)
        last = len(stages) - 1
        final = "float32" if out == "float32" else str(input_img.dtype)      # the last stage requantises
        for i, (st, r) in enumerate(zip(stages, routes)):
            kind = final if i == last else "float32"
            if r is None:
                as_is = kind != "float32" and frame.dtype != torch.float32    # an integer frame keeps its type
                frame = resize_device(frame, st.size, st.scale, st.kernel, st.antialias,
                                      out="unit" if kind == "float32" else "same" if as_is else kind)
            else:
                m, cfg = st
                frame, _ = tiled_forward_device(m, frame, cfg["patch_size"], cfg["patch_overlap"], r.pad8, r.sigma,
                                                max_batch=r.max_batch, unit_range=True, out=kind)
        output_img = to_host(frame)
    return output_img, (time.time() - start_time) * 1000


def run_model_inference_yuv(model: Module, planes, device: torch.device, *, fmt, matrix="bt709", full_range=False,
                            siting="left", luma_only=False, patch_size: int | None = None, patch_overlap: int = 32,
                            need_degradation=False, noise_level=None):
    """Restore one YUV video frame: returns (planes, inference_time_ms), the planes in the format they came in
    and the time from their upload through the download of the result, as run_model_inference's.

    `planes` are numpy arrays in any format of yuv.YUV_LAYOUTS - 4:2:0, 4:2:2 or 4:4:4 at 8, 10 or 12 bit -, (y, u, v)
    for the planar names ("i420", "i422p10", "i444p12", ..) and (y, uv) for the semi-planar ones ("nv12", "p010",
    "p210", ..).  They go up as they are - 1.5 bytes per pixel for "nv12", 6 for "i444p10" -, irm_yuv_to_rgb_f32 makes
    the float32 RGB frame in [0, 1], the device pipeline of run_model_inference runs on it with the hooks
    get_model_prediction picks for the model class (unit_range=True, out="float32": the frame is never rounded to 255
    RGB levels), irm_rgb_f32_to_yuv makes the planes and they come down.  matrix, full_range and siting describe the frame
    (DESIGN.md section 16).  A super-resolving model returns the planes of an s H x s W frame.

    luma_only=True restores Y alone with a one-channel model (REDNet, the gray DnCNN): the chroma planes are not
    uploaded and come back as they are, so an up-scaling model raises ValueError (the chroma would need a resize).
    DeblurGANv2 raises ValueError: its hooks are defined on raw integer values."""
    return _run_model_inference_yuv(model, planes, device, fmt=fmt, matrix=matrix, full_range=full_range, siting=siting,
                                    luma_only=luma_only, patch_size=patch_size, patch_overlap=patch_overlap,
                                    need_degradation=need_degradation, noise_level=noise_level)[:2]


def _run_model_inference_yuv(model, planes, device, *, fmt, matrix="bt709", full_range=False, siting="left",
                             luma_only=False, patch_size=None, patch_overlap=32, need_degradation=False,
                             noise_level=None):
    """run_model_inference_yuv that also hands back the device planes of the result, as frame_metrics_yuv_device
    takes them (the Y plane alone with luma_only): (planes, inference_time_ms, planes_dev)."""
    if model is None or not callable(model):
        raise ValueError("run_model_inference_yuv: model must be a model, not None")
    refuse_deblurgan(model, "run_model_inference_yuv",
                     "convert with yuv420_to_rgb_host and run it with get_model_prediction")
    yuv._check_layout_options(fmt, matrix, siting)
    yuv._check_planes(planes, fmt, False, np.ndarray, (yuv._np_dtype(fmt),))
    route = model_route(model, need_degradation, noise_level)
    if luma_only and route.s > 1:
        raise ValueError(f"luma_only with model.upscale = {route.s}: the chroma planes would need a resize")
    dev = cuda_device(device, "run_model_inference_yuv")
    opts = dict(matrix=matrix, full_range=full_range, siting=siting, luma_only=luma_only)
    start_time = time.time()
    with torch.no_grad():
        up = tuple(to_device(p, dev) for p in (planes[:1] if luma_only else planes))
        frame = yuv_to_rgb_device(up, fmt, **opts)
        frame, _ = tiled_forward_device(model, frame, patch_size, patch_overlap, route.pad8, route.sigma,
                                        max_batch=route.max_batch, unit_range=True, out="float32")
        if luma_only:
            rgb_to_yuv_device(frame, fmt, out=up, **opts)              # same size: Y is overwritten in place
            result, planes_dev = (to_host(up[0]),) + tuple(planes[1:]), up
        else:
            # the planes of the result lie behind one another in one buffer, as a decoder lays them out: one download
            buf, (views,), _ = plane_slots(yuv.plane_shapes(frame.shape[0], frame.shape[1], fmt), up[0].dtype, 1, dev, False)
            rgb_to_yuv_device(frame, fmt, out=tuple(views), **opts)
            host = to_host(buf)                                        # and the same views of it on the host
            result, planes_dev = tuple(host[v.storage_offset():][:v.numel()].reshape(v.shape) for v in views), tuple(views)
    return result, (time.time() - start_time) * 1000, planes_dev
