"""Benchmark-harness aggregate of the reference (scripts/tests.py:389-424): per image PSNR, SSIM and
inference time, per (dataset, model) their mean and standard deviation, one CSV row per combination with
the reference's column names.  Dataset file IO is out of scope - `loader` is any iterable yielding
(input_uint8_hwc, target_uint8_hwc, name), e.g. `synthetic_loader`.  For a super-resolving model (`model.upscale`
s > 1) the pairs are (low-resolution input, s x larger target); `sr_pairs` / `evaluate_sr` make them from HR frames
by the super-resolution protocol (MATLAB bicubic LR, border crop, Y-channel metrics).  Where no target exists
(real captures), `evaluate_blind` scores the frames by NIQE instead; `evaluate_perceptual` adds LPIPS, the perceptual
distance to the target, to the row of `evaluate`.  `evaluate_stream` is `evaluate` over the frame
stream (stream.py): several frames per forward, the copies under the forwards.  `evaluate_aligned` scores beam-splitter pairs (RealBlur) as published: after an ECC
alignment, under the mask of the warp (align.py).  `evaluate_yuv` takes YUV plane
tuples (4:2:0, 4:2:2, 4:4:4; `y4m_pairs` reads them from two YUV4MPEG2 files) and reports PSNR / SSIM per component.  `evaluate_auto_sigma` takes a bank of per-sigma checkpoints and runs, per
frame, the one trained for the noise level estimated on the GPU."""
from __future__ import annotations

import contextlib
import csv
import os
import time

import numpy as np

from . import stream, synth, y4m, yuv
from .align import calculate_metrics_aligned, calculate_metrics_aligned_device
from .frames import to_device, to_host
from .metrics import (calculate_metrics, calculate_metrics_basicsr, calculate_metrics_basicsr_device,
                      calculate_metrics_device, calculate_metrics_f32_device, psnr)
from .niqe import calculate_niqe, calculate_niqe_device
from .perceptual import calculate_lpips, calculate_lpips_device
from .resize import imresize_device, mod_crop
from .utils import (SigmaBank, _get_model_prediction, _run_model_inference_auto, _run_model_inference_yuv,
                    get_model_total_parameters)

COLUMNS = ['Task', 'Type', 'Dataset', 'Sigma', 'Model', 'Model_Params', 'PSNR', 'SSIM', 'Std_PSNR', 'Std_SSIM',
           'Avg_Time_ms', 'Std_Time_ms']
#: the columns of an `evaluate_blind` row: the reference's plus the no-reference score
COLUMNS_BLIND = COLUMNS + ['NIQE', 'Std_NIQE']
#: the columns of an `evaluate_yuv` row: the reference's, PSNR / SSIM being the luma values, plus the chroma planes'
#: the columns of an `evaluate_auto_sigma` row: the reference's plus the estimated and the used noise levels
COLUMNS_AUTO = COLUMNS + ['Sigma_Est', 'Std_Sigma_Est', 'Sigma_Used']
#: the columns of an `evaluate_perceptual` row: the reference's plus the perceptual distance to the target
COLUMNS_PERCEPTUAL = COLUMNS + ['LPIPS', 'Std_LPIPS']
#: the columns of an `evaluate_aligned` row: the reference's, PSNR / SSIM being the aligned ones, plus the correlation
#: the alignment reached and the share of the frame under the warp's mask
COLUMNS_ALIGNED = COLUMNS + ['Rho', 'Coverage', 'Std_Rho', 'Std_Coverage']
COLUMNS_YUV = COLUMNS + ['PSNR_U', 'PSNR_V', 'SSIM_U', 'SSIM_V', 'Std_PSNR_U', 'Std_PSNR_V', 'Std_SSIM_U', 'Std_SSIM_V']


def synthetic_loader(n_images: int, h: int = 720, w: int = 1280, c: int = 3, seed_base: int = 1000, blur: int = 15):
    """Same yield shape as src/data_loaders.py's generators, synthetic GoPro-shaped frames (synth.py)."""
    for i in range(n_images):
        inp, tgt = synth.synth_image_pair(i, h, w, c, seed_base=seed_base, blur=blur)
        yield inp, tgt, f"synthetic_{i:04d}.png"


def _check_metrics(metrics) -> None:
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics must be 'host' or 'device', not {metrics!r}")


@contextlib.contextmanager
def _frame_guard(failed: list, name, skip_failed: bool, model_name, dataset):
    """The work on one frame of a sweep: an exception in the block is recorded in `failed` as (name, "Type: message"),
    printed, and the frame skipped - unless skip_failed is false or it is an out-of-memory error: those propagate."""
    try:
        yield
    except Exception as e:                                      # noqa: BLE001 (reported, not swallowed)
        if not skip_failed or "out of memory" in str(e).lower():
            raise
        failed.append((name, f"{type(e).__name__}: {e}"))
        print(f"[harness] {model_name} on {dataset}: frame {name} failed ({type(e).__name__}: {e}); skipped")


def _host_metrics(pred, target_img, with_ssim: bool) -> tuple:
    """(psnr, ssim) of a downloaded prediction: calculate_metrics, or the PSNR alone and NaN."""
    if with_ssim:
        return calculate_metrics(pred, target_img)
    return psnr(target_img, pred, 255 if pred.dtype == np.uint8 else 65535), float('nan')


def evaluate(model, loader, device, patch_config: dict, *, task: str, subtask: str, dataset: str, model_name: str,
             sigma='N/A', need_degradation=False, noise_level=None, with_ssim=True, skip_failed=True,
             metrics="host") -> dict:
    """One results_table row (scripts/tests.py:399-412).

    The reference's loop lets any exception of a frame end the whole sweep (only a missing weight file is caught,
    tests.py:48-50).  Here a frame that raises is recorded and skipped (report the failed image
    ids instead of losing the run): the row's extra key 'Failed' lists (name, error) pairs and the statistics are
    taken over the frames that ran; `skip_failed=False` restores the reference's behaviour (the exception
    propagates).  Out-of-memory errors always propagate (src/utils.py:91-93 reports them to the caller).

    metrics="host" scores the downloaded prediction with calculate_metrics (numpy / scipy); metrics="device" scores the
    restored frame while it is still on the GPU (calculate_metrics_device for uint8 / uint16 frames;
    calculate_metrics_f32_device with data_range 1.0, the host's rule for float frames, where input and target are
    float32 arrays of the prediction's shape): the target is uploaded, and PSNR / SSIM differ from the host's by
    rounding only (the tests allow 1e-9).  A float target for an integer prediction, or the reverse, raises.  Either way
    the prediction and the timed work (input upload through output download) are the same, and the metrics are not
    timed."""
    _check_metrics(metrics)
    psnr_list, ssim_list, time_list, failed = [], [], [], []
    for input_img, target_img, name in loader:
        with _frame_guard(failed, name, skip_failed, model_name, dataset):
            pred, ms, pred_dev = _get_model_prediction(model, input_img, device, **patch_config,
                                                       need_degradation=need_degradation, noise_level=noise_level)
            if metrics == "device":
                p, s = _device_metrics(pred, pred_dev, target_img, device, input_img)
                if not with_ssim:
                    s = float('nan')
            else:
                p, s = _host_metrics(pred, target_img, with_ssim)
            psnr_list.append(p)
            ssim_list.append(s)
            time_list.append(ms)
    row = aggregate(psnr_list, ssim_list, time_list, task=task, subtask=subtask, dataset=dataset, sigma=sigma,
                    model_name=model_name, params=get_model_total_parameters(model))
    row['Failed'] = failed
    return row


def evaluate_auto_sigma(bank, loader, device, patch_config: dict, *, task: str, subtask: str, dataset: str,
                        model_name: str, metrics="host", with_ssim=True, skip_failed=True) -> dict:
    """The row of `evaluate` for a SigmaBank (utils.get_model_bank): per frame the noise level is estimated on the GPU
    and the checkpoint trained for it runs (utils.run_model_inference_auto; the timed work is that call's, the
    estimate included).  Scored as `evaluate` scores, failed frames handled as there.  The row's 'Sigma' is 'auto'; it
    adds 'Sigma_Est' and 'Std_Sigma_Est', mean and standard deviation of the estimates, and 'Sigma_Used', a dict of
    level -> number of frames that ran with it (COLUMNS_AUTO).  Model_Params counts one model of the bank."""
    _check_metrics(metrics)
    if not isinstance(bank, SigmaBank):
        raise ValueError("evaluate_auto_sigma: bank is a SigmaBank (utils.get_model_bank)")
    if not isinstance(patch_config, dict) or set(patch_config) != {"patch_size", "patch_overlap"}:
        raise ValueError("evaluate_auto_sigma: patch_config is {'patch_size': .., 'patch_overlap': ..}")
    psnr_list, ssim_list, time_list, est_list, failed = [], [], [], [], []
    used = {}
    for input_img, target_img, name in loader:
        with _frame_guard(failed, name, skip_failed, model_name, dataset):
            pred, ms, est, level, pred_dev = _run_model_inference_auto(bank, input_img, device, **patch_config)
            if metrics == "device":
                p, s = _device_metrics(pred, pred_dev, target_img, device, input_img)
                if not with_ssim:
                    s = float('nan')
            else:
                p, s = _host_metrics(pred, target_img, with_ssim)
            psnr_list.append(p)
            ssim_list.append(s)
            time_list.append(ms)
            est_list.append(est)
            used[level] = used.get(level, 0) + 1
    row = aggregate(psnr_list, ssim_list, time_list, task=task, subtask=subtask, dataset=dataset, sigma='auto',
                    model_name=model_name, params=get_model_total_parameters(bank.models[bank.levels[0]]))
    if not est_list:
        est_list = [float('nan')]
    row['Sigma_Est'], row['Std_Sigma_Est'] = np.mean(est_list), np.std(est_list)
    row['Sigma_Used'] = {level: used[level] for level in bank.levels if level in used}
    row['Failed'] = failed
    return row


def evaluate_stream(model, loader, device, patch_config: dict, *, task: str, subtask: str, dataset: str,
                    model_name: str, frames_per_step: int = 4, metrics="device", sigma='N/A', need_degradation=False,
                    noise_level=None, with_ssim=True) -> dict:
    """The row of `evaluate` from the frame stream (stream.py): groups of `frames_per_step` frames per forward, the
    copies under the forwards, the hooks by the model class as get_model_prediction picks them.

    metrics="device" scores a whole group with one launch of calculate_metrics_device's kernel (frame_metrics_device)
    on the device output slot, before the slot is used again; the targets go up through a pinned slot like the
    inputs, and the scores come down with the frames.  metrics="host" scores the yielded arrays with
    calculate_metrics.  The time of a frame is the stream's `ms`: its group's share of the wall time, the scoring of
    a device-scored group included - a throughput figure, so Avg_Time_ms x frames is the time of the sweep.

    There is no skip_failed: a frame that raises ends the sweep and the exception propagates, as in the reference's
    loop (scripts/tests.py).  The row's 'Failed' is always empty."""
    _check_metrics(metrics)
    k = stream._check_frames_per_step(frames_per_step)
    front = stream._Front(model, patch_config["patch_size"], patch_config["patch_overlap"], need_degradation,
                          noise_level, "same", False, triples=True, with_targets=metrics == "device")
    items = ((inp, tgt, tgt) for inp, tgt, _ in loader)
    psnr_list, ssim_list, time_list = [], [], []
    frames = stream._stream(front, items, device, k)
    try:
        for pred, ms, target_img, score in frames:
            if score is not None:
                p, s = stream.score_psnr(score[0], pred.shape, pred.dtype), score[1] if with_ssim else float('nan')
            else:
                p, s = _host_metrics(pred, target_img, with_ssim)
            psnr_list.append(p)
            ssim_list.append(s)
            time_list.append(ms)
    finally:
        frames.close()
    row = aggregate(psnr_list, ssim_list, time_list, task=task, subtask=subtask, dataset=dataset, sigma=sigma,
                    model_name=model_name, params=get_model_total_parameters(model))
    row['Failed'] = []
    return row


def _is_f32(a, shape=None) -> bool:
    return isinstance(a, np.ndarray) and a.dtype == np.float32 and (shape is None or a.shape == shape)


def _device_metrics(pred, pred_dev, target_img, device, input_img=None):
    """(psnr, ssim) of one frame on the GPU: pred_dev is the pipeline's output tensor (None after the host tile loop:
    the prediction is uploaded), the target goes up as the input did (uint16 as its int16 bit pattern).  A float32
    prediction of a float32 input with a float32 target of its shape is scored by the float kernel."""
    if _is_f32(input_img) and _is_f32(pred) and _is_f32(target_img, pred.shape):
        if pred_dev is None:
            pred_dev = to_device(pred, device)
        return calculate_metrics_f32_device(pred_dev, to_device(target_img, pred_dev.device))
    if not isinstance(target_img, np.ndarray) or target_img.dtype not in (np.uint8, np.uint16):
        raise ValueError("metrics='device' needs uint8 or uint16 target frames")
    if pred_dev is None:
        pred_dev = to_device(pred, device)
    return calculate_metrics_device(pred_dev, to_device(target_img, pred_dev.device))


def sr_pairs(hr_loader, scale: int, device):
    """Super-resolution pairs from HR frames: yields (lr, hr_mod_cropped, name) host arrays.  `hr_loader` yields
    (hr, name) or, like `synthetic_loader`, (input, target, name) - the target is the HR frame.  The HR frame is
    mod-cropped to a multiple of `scale`; the LR frame is MATLAB's antialiased bicubic imresize of it by 1 / scale, made
    on the GPU (imresize_device) and quantised to the HR dtype, as LR files are made."""
    if scale not in (2, 3, 4):
        raise ValueError(f"sr_pairs: scale must be 2, 3 or 4, not {scale!r}")
    for item in hr_loader:
        hr, name = (item[-2], item[-1])
        if not isinstance(hr, np.ndarray) or hr.dtype not in (np.uint8, np.uint16):
            raise ValueError("sr_pairs needs uint8 or uint16 HR frames")
        hr = np.ascontiguousarray(mod_crop(hr, scale))
        lr = imresize_device(to_device(hr, device), 1.0 / scale, out="same")
        yield to_host(lr), hr, name


def evaluate_sr(model, hr_loader, device, patch_config: dict, scale: int, *, task: str = "super-resolution",
                subtask: str | None = None, dataset: str = "synthetic", model_name: str | None = None, sigma='N/A',
                crop_border: int | None = None, test_y_channel: bool = True, channel_order: str = "rgb",
                skip_failed=True, metrics="device") -> dict:
    """One results_table row by the super-resolution protocol: per HR frame, mod-crop, LR by MATLAB bicubic on the
    GPU (`sr_pairs`), the model's x`scale` prediction, then basicsr's PSNR / SSIM with `crop_border` pixels (default:
    `scale`) cropped from every side, on the Y channel unless test_y_channel=False.  The timed region is what
    `evaluate` times (input upload through output download of the prediction); LR synthesis and scoring are outside
    it.  metrics="device" scores the prediction while it is on the GPU (calculate_metrics_basicsr_device),
    metrics="host" the downloaded one (calculate_metrics_basicsr); they differ by rounding only.
    model=None gives the bicubic baseline row: the prediction is imresize_device(lr, scale), the time that of the
    upload, the resize and the download.  Failed frames are handled as in `evaluate`."""
    _check_metrics(metrics)
    if scale not in (2, 3, 4):
        raise ValueError(f"evaluate_sr: scale must be 2, 3 or 4, not {scale!r}")
    if model is not None and int(getattr(model, "upscale", 1) or 1) != scale:
        raise ValueError(f"evaluate_sr: scale {scale} but model.upscale = {getattr(model, 'upscale', 1)}")
    crop = scale if crop_border is None else crop_border
    if int(crop) != crop or crop < 0:
        raise ValueError(f"crop_border must be a non-negative integer, not {crop_border!r}")
    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', not {channel_order!r}")
    if model_name is None:
        model_name = "Bicubic" if model is None else type(model).__name__
    psnr_list, ssim_list, time_list, failed = [], [], [], []
    for lr, hr, name in sr_pairs(hr_loader, scale, device):
        with _frame_guard(failed, name, skip_failed, model_name, dataset):
            if model is None:
                start = time.time()
                pred_dev = imresize_device(to_device(lr, device), scale, out="same")
                pred = to_host(pred_dev)
                ms = (time.time() - start) * 1000
            else:
                pred, ms, pred_dev = _get_model_prediction(model, lr, device, **patch_config)
            if pred.shape != hr.shape:
                raise ValueError(f"prediction {pred.shape} for an HR frame {hr.shape}")
            if metrics == "device":
                if pred_dev is None:
                    pred_dev = to_device(pred, device)
                p, s = calculate_metrics_basicsr_device(pred_dev, to_device(hr, pred_dev.device), crop, test_y_channel,
                                                        channel_order)
            else:
                p, s = calculate_metrics_basicsr(pred, hr, crop, test_y_channel, channel_order)
            psnr_list.append(p)
            ssim_list.append(s)
            time_list.append(ms)
    row = aggregate(psnr_list, ssim_list, time_list, task=task, subtask=subtask or f"x{scale}", dataset=dataset, sigma=sigma,
                    model_name=model_name, params=0 if model is None else get_model_total_parameters(model))
    row['Failed'] = failed
    return row


class y4m_pairs:
    """The loader of `evaluate_yuv` over two YUV4MPEG2 files, degraded input and target: yields (planes, target_planes,
    name) frame by frame, name = "<input file>#<frame index>".  ValueError if the two headers differ in frame size or
    format.  `fmt` and `siting` (and `full_range`, None if the input does not say) are the keyword values to pass on;
    `frames` is the number of pairs."""

    def __init__(self, input_path, target_path):
        self.input, self.target = y4m.read_y4m(input_path), y4m.read_y4m(target_path)
        a, b = self.input, self.target
        if (a.width, a.height) != (b.width, b.height):
            raise ValueError(f"y4m_pairs: {a.path} is {a.width} x {a.height}, {b.path} is {b.width} x {b.height}")
        if a.fmt != b.fmt:
            raise ValueError(f"y4m_pairs: {a.path} is {a.fmt!r}, {b.path} is {b.fmt!r}")
        self.fmt, self.siting, self.full_range = a.fmt, a.siting, a.full_range
        self.frames = min(a.frames, b.frames)

    def __len__(self):
        return self.frames

    def __iter__(self):
        base = os.path.basename(self.input.path)
        for i, (planes, target_planes) in enumerate(zip(self.input, self.target)):
            yield planes, target_planes, f"{base}#{i}"


def evaluate_yuv(model, loader, device, patch_config: dict, *, fmt, matrix="bt709", full_range=False, siting="left",
                 luma_only=False, metrics="device", task: str, subtask: str, dataset: str, model_name: str, sigma='N/A',
                 need_degradation=False, noise_level=None, skip_failed=True) -> dict:
    """One results_table row for YUV video frames: `loader` yields (planes, target_planes, name), the planes as
    run_model_inference_yuv takes them (numpy arrays in `fmt`, any name of yuv.YUV_LAYOUTS; matrix, full_range and
    siting describe the frames; `y4m_pairs` is such a loader).  The
    prediction and the timed region are run_model_inference_yuv's, plane upload through plane download; scoring is
    outside it.  metrics="device" scores the restored planes while they are on the GPU (calculate_metrics_yuv_device:
    the target planes are uploaded), metrics="host" the downloaded ones (calculate_metrics_yuv); they differ by
    rounding only.  The scores are per component, on the integer codes: the row has the reference's columns with PSNR /
    SSIM the luma values, plus PSNR_U, PSNR_V, SSIM_U, SSIM_V and their Std_ forms (COLUMNS_YUV); with luma_only the
    chroma columns are NaN.  Failed frames are handled as in `evaluate`."""
    _check_metrics(metrics)
    yuv._check_layout_options(fmt, matrix, siting)
    if not isinstance(patch_config, dict) or set(patch_config) != {"patch_size", "patch_overlap"}:
        raise ValueError("evaluate_yuv: patch_config is {'patch_size': .., 'patch_overlap': ..}")
    scores, time_list, failed = [], [], []
    for planes, target_planes, name in loader:
        with _frame_guard(failed, name, skip_failed, model_name, dataset):
            pred, ms, pred_dev = _run_model_inference_yuv(
                model, planes, device, fmt=fmt, matrix=matrix, full_range=full_range, siting=siting, luma_only=luma_only,
                need_degradation=need_degradation, noise_level=noise_level, **patch_config)
            if metrics == "device":
                if not isinstance(target_planes, (tuple, list)) or not all(isinstance(t, np.ndarray) for t in target_planes):
                    raise ValueError("evaluate_yuv: the target planes are numpy arrays")
                used = target_planes[:1] if luma_only else target_planes
                target_dev = tuple(to_device(t, pred_dev[0].device) for t in used)
                m = yuv.calculate_metrics_yuv_device(pred_dev, target_dev, fmt, luma_only)
            else:
                m = yuv.calculate_metrics_yuv(pred, target_planes, fmt, luma_only)
            del pred_dev
            scores.append(m)
            time_list.append(ms)
    row = aggregate([m.psnr_y for m in scores], [m.ssim_y for m in scores], time_list, task=task, subtask=subtask,
                    dataset=dataset, sigma=sigma, model_name=model_name, params=get_model_total_parameters(model))
    for col, field in (('PSNR_U', 'psnr_u'), ('PSNR_V', 'psnr_v'), ('SSIM_U', 'ssim_u'), ('SSIM_V', 'ssim_v')):
        vals = [getattr(m, field) for m in scores] or [float('nan')]
        row[col], row['Std_' + col] = np.mean(vals), np.std(vals)
    row['Failed'] = failed
    return row


def evaluate_blind(model, loader, device, patch_config: dict, *, niqe_params, crop_border: int = 0, metrics="device",
                   task: str = "blind", subtask: str = "N/A", dataset: str = "captures", model_name: str | None = None,
                   sigma='N/A', channel_order: str = "rgb", need_degradation=False, noise_level=None,
                   skip_failed=True) -> dict:
    """One results_table row for frames without a target: per frame the model's prediction and its NIQE
    (`niqe_params` from utils.load_niqe_params; `crop_border` pixels cropped from every side; the Y channel of colour
    frames read in `channel_order`).  `loader` yields (input, name) or (input, target, name); a target is ignored.
    The timed region is what `evaluate` times (input upload through output download); scoring is outside it.
    metrics="device" scores the prediction while it is on the GPU (calculate_niqe_device), metrics="host" the
    downloaded one (calculate_niqe); they differ by rounding only.  model=None scores the inputs themselves (the
    "before" row; its times are 0).  The row has the reference's columns - PSNR and SSIM are NaN - plus 'NIQE' and
    'Std_NIQE' (COLUMNS_BLIND).  Failed frames are handled as in `evaluate`."""
    _check_metrics(metrics)
    if model_name is None:
        model_name = "Input" if model is None else type(model).__name__
    niqe_list, time_list, failed = [], [], []
    for item in loader:
        input_img, name = item[0], item[-1]
        with _frame_guard(failed, name, skip_failed, model_name, dataset):
            if model is None:
                pred, ms, pred_dev = input_img, 0.0, None
            else:
                pred, ms, pred_dev = _get_model_prediction(model, input_img, device, **patch_config,
                                                           need_degradation=need_degradation, noise_level=noise_level)
            if metrics == "device":
                if not isinstance(pred, np.ndarray) or pred.dtype not in (np.uint8, np.uint16):
                    raise ValueError("metrics='device' needs uint8 or uint16 frames")
                if pred_dev is None:
                    pred_dev = to_device(pred, device)
                q = calculate_niqe_device(pred_dev, crop_border, niqe_params, channel_order=channel_order)
            else:
                q = calculate_niqe(pred, crop_border, niqe_params, channel_order=channel_order)
            niqe_list.append(q)
            time_list.append(ms)
    nan = [float('nan')] * len(niqe_list)
    row = aggregate(nan, nan, time_list, task=task, subtask=subtask, dataset=dataset, sigma=sigma,
                    model_name=model_name, params=0 if model is None else get_model_total_parameters(model))
    if not niqe_list:
        niqe_list = [float('nan')]
    row['NIQE'], row['Std_NIQE'] = np.mean(niqe_list), np.std(niqe_list)
    row['Failed'] = failed
    return row


def evaluate_perceptual(model, loader, device, patch_config: dict, *, lpips_params, metrics="device",
                        task: str = "perceptual", subtask: str = "N/A", dataset: str = "synthetic",
                        model_name: str | None = None, sigma='N/A', need_degradation=False, noise_level=None,
                        with_ssim=True, skip_failed=True) -> dict:
    """The row of `evaluate` with the perceptual distance beside PSNR and SSIM: per frame the model's prediction, its
    PSNR / SSIM as `evaluate` computes them and its LPIPS against the target (`lpips_params` from
    utils.load_lpips_params; 3-channel frames of at least 31 x 31).  The timed region is what `evaluate` times (input
    upload through output download); every score is outside it.  metrics="device" scores the prediction while it is
    on the GPU (calculate_lpips_device), metrics="host" the downloaded one (calculate_lpips); they differ by the
    float32 rounding of the trunk.  model=None scores the inputs themselves (the "before" row; its times are 0).  The
    row has the reference's columns plus 'LPIPS' and 'Std_LPIPS' (COLUMNS_PERCEPTUAL).  Failed frames are handled as in
    `evaluate`."""
    _check_metrics(metrics)
    if model_name is None:
        model_name = "Input" if model is None else type(model).__name__
    psnr_list, ssim_list, lpips_list, time_list, failed = [], [], [], [], []
    for input_img, target_img, name in loader:
        with _frame_guard(failed, name, skip_failed, model_name, dataset):
            if model is None:
                pred, ms, pred_dev = input_img, 0.0, None
            else:
                pred, ms, pred_dev = _get_model_prediction(model, input_img, device, **patch_config,
                                                           need_degradation=need_degradation, noise_level=noise_level)
            if metrics == "device":
                if pred_dev is None:
                    pred_dev = to_device(pred, device)
                p, s = _device_metrics(pred, pred_dev, target_img, device, input_img)
                if not with_ssim:
                    s = float('nan')
                q = calculate_lpips_device(pred_dev, to_device(target_img, pred_dev.device), lpips_params)
            else:
                p, s = _host_metrics(pred, target_img, with_ssim)
                q = calculate_lpips(pred, target_img, lpips_params)
            psnr_list.append(p)
            ssim_list.append(s)
            lpips_list.append(q)
            time_list.append(ms)
    row = aggregate(psnr_list, ssim_list, time_list, task=task, subtask=subtask, dataset=dataset, sigma=sigma,
                    model_name=model_name, params=0 if model is None else get_model_total_parameters(model))
    if not lpips_list:
        lpips_list = [float('nan')]
    row['LPIPS'], row['Std_LPIPS'] = np.mean(lpips_list), np.std(lpips_list)
    row['Failed'] = failed
    return row


def evaluate_aligned(model, loader, device, patch_config: dict, *, iterations: int = 100, metrics="device",
                     task: str = "deblurring", subtask: str = "motion", dataset: str = "RealBlur",
                     model_name: str | None = None, sigma='N/A', need_degradation=False, noise_level=None,
                     skip_failed=True) -> dict:
    """The row of `evaluate` for pairs that are only approximately registered (RealBlur_J, RealBlur_R): PSNR / SSIM are
    those of the aligned protocol (align.py: gain, ECC homography with `iterations` rounds, bicubic warp, scores under
    the warp's mask; uint8 / uint16 3-channel frames, both sides at least 11).  The timed region is what `evaluate` times
    (input upload through output download); alignment and scoring are outside it.  metrics="device" scores the
    prediction while it is on the GPU (calculate_metrics_aligned_device), metrics="host" the downloaded one with the
    float64 numpy statement (calculate_metrics_aligned).  model=None scores the inputs themselves (the "before" row; its
    times are 0).  The row adds 'Rho' and 'Coverage' and their standard deviations (COLUMNS_ALIGNED).  A frame whose
    alignment failed (flat frames, no overlap) goes to 'Failed' like any other failed frame."""
    _check_metrics(metrics)
    if model_name is None:
        model_name = "Input" if model is None else type(model).__name__
    scores, time_list, failed = [], [], []
    for input_img, target_img, name in loader:
        with _frame_guard(failed, name, skip_failed, model_name, dataset):
            if model is None:
                pred, ms, pred_dev = input_img, 0.0, None
            else:
                pred, ms, pred_dev = _get_model_prediction(model, input_img, device, **patch_config,
                                                           need_degradation=need_degradation, noise_level=noise_level)
            if metrics == "device":
                if not isinstance(target_img, np.ndarray) or target_img.dtype not in (np.uint8, np.uint16):
                    raise ValueError("metrics='device' needs uint8 or uint16 target frames")
                if pred_dev is None:
                    pred_dev = to_device(pred, device)
                m = calculate_metrics_aligned_device(pred_dev, to_device(target_img, pred_dev.device), iterations)
            else:
                m = calculate_metrics_aligned(pred, target_img, iterations)
            if not m.ok:
                raise ValueError(f"the alignment failed (rho {m.rho}, coverage {m.coverage})")
            scores.append(m)
            time_list.append(ms)
    row = aggregate([m.psnr for m in scores], [m.ssim for m in scores], time_list, task=task, subtask=subtask,
                    dataset=dataset, sigma=sigma, model_name=model_name,
                    params=0 if model is None else get_model_total_parameters(model))
    for col, field in (('Rho', 'rho'), ('Coverage', 'coverage')):
        vals = [getattr(m, field) for m in scores] or [float('nan')]
        row[col], row['Std_' + col] = np.mean(vals), np.std(vals)
    row['Failed'] = failed
    return row


def aggregate(psnr_list, ssim_list, time_list, *, task, subtask, dataset, sigma, model_name, params) -> dict:
    if not psnr_list:                      # every frame failed: an empty row, not a numpy warning
        psnr_list = ssim_list = time_list = [float('nan')]
    return {'Task': task.capitalize(), 'Type': subtask.capitalize(), 'Dataset': dataset, 'Sigma': sigma,
            'Model': model_name, 'Model_Params': params, 'PSNR': np.mean(psnr_list), 'SSIM': np.mean(ssim_list),
            'Std_PSNR': np.std(psnr_list), 'Std_SSIM': np.std(ssim_list), 'Avg_Time_ms': np.mean(time_list),
            'Std_Time_ms': np.std(time_list)}


def save_results(rows: list, out_dir: str = 'results', file_name: str = 'results_summary.csv', columns=None) -> str:
    """CSV with the reference's columns (scripts/tests.py:415-424; written with the csv module, not pandas), or with
    `columns` (COLUMNS_BLIND for `evaluate_blind` rows); a column a row lacks stays empty."""
    columns = COLUMNS if columns is None else list(columns)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, file_name)
    with open(path, 'w', newline='') as f:
        wr = csv.DictWriter(f, fieldnames=columns, extrasaction='ignore')
        wr.writeheader()
        for r in rows:
            wr.writerow(r)
    return path
