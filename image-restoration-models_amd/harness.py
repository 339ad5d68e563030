"""Benchmark-harness aggregate of the reference (scripts/tests.py:389-424): per image PSNR, SSIM and inference time,
per (dataset, model) their mean and standard deviation, one CSV row per combination with the reference's column names
(`aggregate`, `save_results`).  Dataset file IO is out of scope: `loader` is any iterable of (input, target, name),
e.g. `synthetic_loader`.  One function per protocol, each returning one row:

  evaluate             the reference's row: PSNR / SSIM of the prediction against the target
  evaluate_auto_sigma  the same over a bank of per-sigma checkpoints: per frame, the one for the sigma estimated there
  evaluate_stream      the same over the frame stream (stream.py): several frames per forward, copies under the forwards
  evaluate_sr          super-resolution: MATLAB bicubic LR from HR frames (`sr_pairs`), border crop, Y-channel metrics
  evaluate_yuv         YUV plane tuples (4:2:0, 4:2:2, 4:4:4; `y4m_pairs` reads Y4M files): PSNR / SSIM per component
  evaluate_blind       no target (real captures): NIQE in place of PSNR / SSIM
  evaluate_perceptual  `evaluate` plus LPIPS, the perceptual distance to the target
  evaluate_aligned     beam-splitter pairs (RealBlur) as published: after an ECC alignment, under the warp's mask

A protocol is its per-frame function, which returns one record (psnr, ssim, ms, extra values..); `_sweep` runs it over
the loader under `_frame_guard`, `_row` makes the row from the records."""
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
from .utils import (SigmaBank, _get_model_prediction, _is_patch_config, _run_model_inference_auto,
                    _run_model_inference_yuv, get_model_total_parameters)

COLUMNS = ['Task', 'Type', 'Dataset', 'Sigma', 'Model', 'Model_Params', 'PSNR', 'SSIM', 'Std_PSNR', 'Std_SSIM',
           'Avg_Time_ms', 'Std_Time_ms']


def _columns(extras, *more) -> list:
    """The columns of a protocol whose rows add `extras`: the reference's, the extras, their Std_ forms, then `more`."""
    return COLUMNS + list(extras) + ['Std_' + col for col in extras] + list(more)


# Per protocol, the per-frame values a record holds after (psnr, ssim, ms), in this order; `_row` turns each into a mean
# and a Std_ column, and the COLUMNS_ list that `save_results` takes is made from the same tuple.
EXTRA_BLIND = ('NIQE',)
EXTRA_AUTO = ('Sigma_Est',)
EXTRA_PERCEPTUAL = ('LPIPS',)
EXTRA_ALIGNED = ('Rho', 'Coverage')
EXTRA_YUV = ('PSNR_U', 'PSNR_V', 'SSIM_U', 'SSIM_V')
#: the columns of an `evaluate_blind` row: the reference's plus the no-reference score
COLUMNS_BLIND = _columns(EXTRA_BLIND)
#: the columns of an `evaluate_auto_sigma` row: the reference's plus the estimated and the used noise levels
COLUMNS_AUTO = _columns(EXTRA_AUTO, 'Sigma_Used')
#: the columns of an `evaluate_perceptual` row: the reference's plus the perceptual distance to the target
COLUMNS_PERCEPTUAL = _columns(EXTRA_PERCEPTUAL)
#: the columns of an `evaluate_aligned` row: the reference's, PSNR / SSIM being the aligned ones, plus the correlation
#: the alignment reached and the share of the frame under the warp's mask
COLUMNS_ALIGNED = _columns(EXTRA_ALIGNED)
#: the columns of an `evaluate_yuv` row: the reference's, PSNR / SSIM being the luma values, plus the chroma planes'
COLUMNS_YUV = _columns(EXTRA_YUV)


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


def _triples(loader):
    """The (input, target, name) items of a loader.  They are unpacked here, outside the guard: an item of another
    length is the loader's error, not a frame's, and propagates."""
    for input_img, target_img, name in loader:
        yield input_img, target_img, name


def _sweep(items, frame, skip_failed: bool, model_name, dataset) -> tuple:
    """Run `frame(*item[:-1])` for every item under `_frame_guard`, item[-1] being the frame's name: returns (records,
    failed).  `frame` returns one record - a tuple (psnr, ssim, ms, extra values..) of numbers, never an array or a
    tensor - and returns it last, so a frame adds either a complete record or an entry of `failed`, never a part."""
    records, failed = [], []
    for item in items:
        *args, name = item
        with _frame_guard(failed, name, skip_failed, model_name, dataset):
            records.append(frame(*args))
    return records, failed


def _row(records, failed, extras=(), also=None, **labels) -> dict:
    """The row of a sweep: `aggregate` over the records, then mean and Std_ of every column of `extras` (the record
    values after psnr, ssim, ms, in that order; NaN for no record), then the keys of `also`, then 'Failed'."""
    def column(i):
        return [r[i] for r in records]
    row = aggregate(column(0), column(1), column(2), **labels)
    for i, col in enumerate(extras, 3):
        vals = column(i) or [float('nan')]
        row[col], row['Std_' + col] = np.mean(vals), np.std(vals)
    row.update(also or {})
    row['Failed'] = failed
    return row


def _predict(model, input_img, device, patch_config, need_degradation, noise_level) -> tuple:
    """(prediction, ms, device output or None) of one frame; model=None is the "before" row: the input itself, 0 ms."""
    if model is None:
        return input_img, 0.0, None
    return _get_model_prediction(model, input_img, device, **patch_config, need_degradation=need_degradation,
                                 noise_level=noise_level)


def _name_of(model, model_name, baseline="Input"):
    """The row's model name where the caller gave none: the class, or `baseline` for model=None."""
    if model_name is not None:
        return model_name
    return baseline if model is None else type(model).__name__


def _params_of(model) -> int:
    return 0 if model is None else get_model_total_parameters(model)


def _on_device(pred, pred_dev, device):
    """The prediction on the GPU: the pipeline's output tensor, or `pred` uploaded where the host tile loop made it."""
    return to_device(pred, device) if pred_dev is None else pred_dev


def _host_metrics(pred, target_img, with_ssim: bool) -> tuple:
    """(psnr, ssim) of a downloaded prediction: calculate_metrics, or the PSNR alone and NaN."""
    if with_ssim:
        return calculate_metrics(pred, target_img)
    return psnr(target_img, pred, 255 if pred.dtype == np.uint8 else 65535), float('nan')


def _is_f32(a, shape=None) -> bool:
    return isinstance(a, np.ndarray) and a.dtype == np.float32 and (shape is None or a.shape == shape)


def _device_metrics(pred, pred_dev, target_img, device, input_img=None):
    """(psnr, ssim) of one frame on the GPU: pred_dev is the pipeline's output tensor (None after the host tile loop:
    the prediction is uploaded), the target goes up as the input did (uint16 as its int16 bit pattern).  A float32
    prediction of a float32 input with a float32 target of its shape is scored by the float kernel."""
    if _is_f32(input_img) and _is_f32(pred) and _is_f32(target_img, pred.shape):
        pred_dev = _on_device(pred, pred_dev, device)
        return calculate_metrics_f32_device(pred_dev, to_device(target_img, pred_dev.device))
    if not isinstance(target_img, np.ndarray) or target_img.dtype not in (np.uint8, np.uint16):
        raise ValueError("metrics='device' needs uint8 or uint16 target frames")
    pred_dev = _on_device(pred, pred_dev, device)
    return calculate_metrics_device(pred_dev, to_device(target_img, pred_dev.device))


def _psnr_ssim(pred, pred_dev, target_img, device, input_img, metrics, with_ssim: bool) -> tuple:
    """(psnr, ssim) as `evaluate` scores: on the GPU or of the downloaded prediction; NaN for SSIM without with_ssim."""
    if metrics == "device":
        p, s = _device_metrics(pred, pred_dev, target_img, device, input_img)
        return p, s if with_ssim else float('nan')
    return _host_metrics(pred, target_img, with_ssim)


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

    def frame(input_img, target_img):
        pred, ms, pred_dev = _get_model_prediction(model, input_img, device, **patch_config,
                                                   need_degradation=need_degradation, noise_level=noise_level)
        return _psnr_ssim(pred, pred_dev, target_img, device, input_img, metrics, with_ssim) + (ms,)
    records, failed = _sweep(_triples(loader), frame, skip_failed, model_name, dataset)
    return _row(records, failed, task=task, subtask=subtask, dataset=dataset, sigma=sigma, model_name=model_name,
                params=get_model_total_parameters(model))


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
    if not _is_patch_config(patch_config):
        raise ValueError("evaluate_auto_sigma: patch_config is {'patch_size': .., 'patch_overlap': ..}")

    def frame(input_img, target_img):
        pred, ms, est, level, pred_dev = _run_model_inference_auto(bank, input_img, device, **patch_config)
        return _psnr_ssim(pred, pred_dev, target_img, device, input_img, metrics, with_ssim) + (ms, est, level)
    records, failed = _sweep(_triples(loader), frame, skip_failed, model_name, dataset)
    levels = [r[4] for r in records]
    used = {level: levels.count(level) for level in bank.levels if level in levels}
    return _row(records, failed, EXTRA_AUTO, {'Sigma_Used': used}, task=task, subtask=subtask, dataset=dataset,
                sigma='auto', model_name=model_name, params=get_model_total_parameters(bank.models[bank.levels[0]]))


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
    records = []
    frames = stream._stream(front, items, device, k)
    try:
        for pred, ms, target_img, score in frames:
            if score is not None:
                p, s = stream.score_psnr(score[0], pred.shape, pred.dtype), score[1] if with_ssim else float('nan')
            else:
                p, s = _host_metrics(pred, target_img, with_ssim)
            records.append((p, s, ms))
    finally:
        frames.close()
    return _row(records, [], task=task, subtask=subtask, dataset=dataset, sigma=sigma, model_name=model_name,
                params=get_model_total_parameters(model))


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
    model_name = _name_of(model, model_name, "Bicubic")

    def frame(lr, hr):
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
            pred_dev = _on_device(pred, pred_dev, device)
            return calculate_metrics_basicsr_device(pred_dev, to_device(hr, pred_dev.device), crop, test_y_channel,
                                                    channel_order) + (ms,)
        return calculate_metrics_basicsr(pred, hr, crop, test_y_channel, channel_order) + (ms,)
    records, failed = _sweep(sr_pairs(hr_loader, scale, device), frame, skip_failed, model_name, dataset)
    return _row(records, failed, task=task, subtask=subtask or f"x{scale}", dataset=dataset, sigma=sigma,
                model_name=model_name, params=_params_of(model))


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
    if not _is_patch_config(patch_config):
        raise ValueError("evaluate_yuv: patch_config is {'patch_size': .., 'patch_overlap': ..}")

    def frame(planes, target_planes):                           # the result planes on the device live no longer than it
        pred, ms, pred_dev = _run_model_inference_yuv(
            model, planes, device, fmt=fmt, matrix=matrix, full_range=full_range, siting=siting, luma_only=luma_only,
            need_degradation=need_degradation, noise_level=noise_level, **patch_config)
        if metrics == "device":
            if not (isinstance(target_planes, (tuple, list)) and all(isinstance(t, np.ndarray) for t in target_planes)):
                raise ValueError("evaluate_yuv: the target planes are numpy arrays")
            used = target_planes[:1] if luma_only else target_planes
            target_dev = tuple(to_device(t, pred_dev[0].device) for t in used)
            m = yuv.calculate_metrics_yuv_device(pred_dev, target_dev, fmt, luma_only)
        else:
            m = yuv.calculate_metrics_yuv(pred, target_planes, fmt, luma_only)
        return m.psnr_y, m.ssim_y, ms, m.psnr_u, m.psnr_v, m.ssim_u, m.ssim_v
    records, failed = _sweep(_triples(loader), frame, skip_failed, model_name, dataset)
    return _row(records, failed, EXTRA_YUV, task=task, subtask=subtask, dataset=dataset, sigma=sigma,
                model_name=model_name, params=get_model_total_parameters(model))


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
    model_name = _name_of(model, model_name)

    def frame(input_img, *_target):
        pred, ms, pred_dev = _predict(model, input_img, device, patch_config, need_degradation, noise_level)
        if metrics == "device":
            if not isinstance(pred, np.ndarray) or pred.dtype not in (np.uint8, np.uint16):
                raise ValueError("metrics='device' needs uint8 or uint16 frames")
            q = calculate_niqe_device(_on_device(pred, pred_dev, device), crop_border, niqe_params,
                                      channel_order=channel_order)
        else:
            q = calculate_niqe(pred, crop_border, niqe_params, channel_order=channel_order)
        return float('nan'), float('nan'), ms, q
    records, failed = _sweep(loader, frame, skip_failed, model_name, dataset)
    return _row(records, failed, EXTRA_BLIND, task=task, subtask=subtask, dataset=dataset, sigma=sigma,
                model_name=model_name, params=_params_of(model))


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
    model_name = _name_of(model, model_name)

    def frame(input_img, target_img):
        pred, ms, pred_dev = _predict(model, input_img, device, patch_config, need_degradation, noise_level)
        if metrics == "device":
            pred_dev = _on_device(pred, pred_dev, device)
        p, s = _psnr_ssim(pred, pred_dev, target_img, device, input_img, metrics, with_ssim)
        if metrics == "device":
            q = calculate_lpips_device(pred_dev, to_device(target_img, pred_dev.device), lpips_params)
        else:
            q = calculate_lpips(pred, target_img, lpips_params)
        return p, s, ms, q
    records, failed = _sweep(_triples(loader), frame, skip_failed, model_name, dataset)
    return _row(records, failed, EXTRA_PERCEPTUAL, task=task, subtask=subtask, dataset=dataset, sigma=sigma,
                model_name=model_name, params=_params_of(model))


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
    model_name = _name_of(model, model_name)

    def frame(input_img, target_img):
        pred, ms, pred_dev = _predict(model, input_img, device, patch_config, need_degradation, noise_level)
        if metrics == "device":
            if not isinstance(target_img, np.ndarray) or target_img.dtype not in (np.uint8, np.uint16):
                raise ValueError("metrics='device' needs uint8 or uint16 target frames")
            pred_dev = _on_device(pred, pred_dev, device)
            m = calculate_metrics_aligned_device(pred_dev, to_device(target_img, pred_dev.device), iterations)
        else:
            m = calculate_metrics_aligned(pred, target_img, iterations)
        if not m.ok:
            raise ValueError(f"the alignment failed (rho {m.rho}, coverage {m.coverage})")
        return m.psnr, m.ssim, ms, m.rho, m.coverage
    records, failed = _sweep(_triples(loader), frame, skip_failed, model_name, dataset)
    return _row(records, failed, EXTRA_ALIGNED, task=task, subtask=subtask, dataset=dataset, sigma=sigma,
                model_name=model_name, params=_params_of(model))


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
