"""A sequence of frames through the device pipeline with the copies under the forwards.

The one-frame calls of utils.py upload from pageable memory, run, download and synchronise, one frame at a time.
`run_model_inference_stream` takes any iterable of frames, forms groups of `frames_per_step` consecutive frames of one
shape and dtype, runs each group as one tiled_forward_device_batch step (pipeline._tile_pipeline_plan /
_tile_pipeline_run on static buffers) and keeps two groups in flight: while group g computes, group g + 1 is copied up
and group g - 1 comes down.

Three streams: torch's current stream for EVERY kernel (tiler, model, converters, metrics), one upload stream and one
download stream, cached per device under keys of their own.  One copy stream would not do: the upload of g + 1 would
queue behind the download of g, which waits for the forward of g.  Two kernels never overlap.

Per (shape, dtype) a plan owns, allocated once, two slots of each buffer; slot g % 2 serves group g.  A slot may be
rewritten for group g + 2 only after

    buffer            condition                                         how
    pinned-in slot    the upload of g has completed                     the host waits on up[g]
    device-in slot    the compute of g is done                          the upload stream waits on done[g]
    device-out slot   the download of g is done                         the compute stream waits on down[g]
    pinned-out slot   the host has copied the frames of g out           program order: g is retired before g + 2 is enqueued

up / done / down are events recorded on the upload, compute and download stream.  Every buffer of a plan lives until
the generator has synchronised all three streams, so no record_stream is needed and nothing is freed per step.  The
steady state enqueues pinned asynchronous copies and kernels only: no pageable copy, no .cpu(), no .item().

The first group of a plan, and the first group of a plan with another number of frames, runs unpipelined (drain, fill,
upload, compute, synchronise): that is where graphed_forward captures, and a capture synchronises the device.
"""
from __future__ import annotations

import collections
import time

import numpy as np
import torch

from . import yuv
from .frames import device_constant, plane_slots, psnr_from_error
from .metrics import frame_metrics_device
from .pipeline import (_check_out, _tile_pipeline_plan, _tile_pipeline_run, _value_kinds, cuda_device, model_route,
                       refuse_deblurgan)

#: plans (buffers of one frame shape and dtype) a stream keeps, least recently used first out
MAX_PLANS = 4
#: groups in flight
DEPTH = 2

_TORCH_KIND = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16, np.dtype(np.float32): torch.float32}


def _grouped(items, prepare, frames_per_step: int):
    """Lists of at most `frames_per_step` consecutive prepared items of one key, lazily: prepare(item) -> (key, ...).
    A group is handed out as soon as it is full; another key or the end closes it early.  When the iterable or
    prepare raises, the frames before the offending one are handed out first and the error follows."""
    group, it, err = [], iter(items), None
    while True:
        try:
            p = prepare(next(it))
        except StopIteration:
            break
        except Exception as e:                                  # noqa: BLE001 (re-raised below)
            err = e
            break
        if group and p[0] != group[0][0]:
            yield group
            group = []
        group.append(p)
        if len(group) == frames_per_step:
            yield group
            group = []
    if group:
        yield group
    if err is not None:
        try:
            raise err
        finally:
            err = None                                          # no cycle error -> traceback -> this frame -> error


def group_frames(shapes_and_dtypes, frames_per_step: int) -> list:
    """The groups the stream forms, as lists of frame indices: consecutive frames with equal (shape, dtype) entries,
    at most `frames_per_step` per group, in input order.  Pure: 7 equal frames at 3 give [[0, 1, 2], [3, 4, 5], [6]]."""
    k = _check_frames_per_step(frames_per_step)
    return [[i for _, i in g] for g in _grouped(enumerate(shapes_and_dtypes), lambda t: (t[1], t[0]), k)]


def _check_frames_per_step(frames_per_step) -> int:
    if isinstance(frames_per_step, bool) or not isinstance(frames_per_step, (int, np.integer)) or frames_per_step < 1:
        raise ValueError(f"frames_per_step must be a positive integer, not {frames_per_step!r}")
    return int(frames_per_step)


class _Front:
    """What the stream does with one kind of frame: the checks that need no GPU (`prepare`), the layout of a frame in
    the input and output slots, and the device work of a group (`compute`).  This one is the plain [H, W, C] frame."""

    def __init__(self, model, patch_size, patch_overlap, need_degradation, noise_level, out, unit_range,
                 triples=False, with_targets=False):
        if model is None or not callable(model):
            raise ValueError("run_model_inference_stream: model must be a model, not None")
        self.model, self.patch_size, self.patch_overlap = model, patch_size, patch_overlap
        #: triples: an item is (frame, target or None, extra) and not the frame; with_targets: the targets go up too
        self.out, self.unit_range, self.triples, self.with_targets = out, bool(unit_range), triples, with_targets
        self.route = model_route(model, need_degradation, noise_level)
        _check_out(out, self.route.hooks)

    def prepare(self, item):
        """(key, arrays to upload, target or None, what comes back with the result) of one frame, or ValueError."""
        frame, target, extra = item if self.triples else (item, None, None)
        if not isinstance(frame, np.ndarray) or frame.ndim != 3 or frame.dtype not in _TORCH_KIND:
            raise ValueError("run_model_inference_stream: a frame is a uint8, uint16 or float32 [H, W, C] array")
        if min(frame.shape) < 1:
            raise ValueError(f"run_model_inference_stream: an empty frame, shape {frame.shape}")
        dtype = _TORCH_KIND[frame.dtype]
        _, f32_out, out_dtype, _ = _value_kinds(dtype, self.out, self.unit_range, self.route.hooks, False)
        if self.route.hooks == "deblurganv2" and frame.dtype != np.uint8:
            raise ValueError("DeblurGANv2 streams uint8 frames only: its hooks are defined on raw 8-bit values")
        if self.with_targets:
            h, w, c = frame.shape
            want = (self.route.s * h, self.route.s * w, min(3, c))
            if (not isinstance(target, np.ndarray) or target.dtype not in (np.uint8, np.uint16) or f32_out
                    or _TORCH_KIND[target.dtype] != out_dtype or target.shape != want):
                raise ValueError("metrics='device' needs uint8 or uint16 target frames of the prediction's shape and dtype")
        return (frame.shape, frame.dtype), (frame,), target if self.with_targets else None, extra

    def layout(self, key):
        """(tile plan arguments, input plane shapes, input dtype, output plane shapes, output dtype or None for the
        tile plan's)."""
        (h, w, c), dt = key
        return ((h, w, c), _TORCH_KIND[dt], self.out, self.unit_range), [(h, w, c)], _TORCH_KIND[dt], \
            [(self.route.s * h, self.route.s * w, min(3, c))], None

    def compute(self, plan, slot: int, k: int):
        _tile_pipeline_run(self.model, plan.tp, [f[0] for f in plan.dev_in[slot][:k]], None, self.route.max_batch, None,
                           frames_out=[f[0] for f in plan.dev_out[slot][:k]])

    def finish(self, extra, outs):
        """What the stream yields for a frame: `outs` are the caller's own copies of its output planes."""
        return outs[0]


class _YuvFront(_Front):
    """YUV plane tuples (any format of yuv.YUV_LAYOUTS): the route of run_model_inference_yuv with the planes of K frames behind one another."""

    def __init__(self, model, patch_size, patch_overlap, need_degradation, noise_level, fmt, matrix, full_range, siting,
                 luma_only):
        refuse_deblurgan(model, "run_model_inference_stream", "convert with yuv420_to_rgb_host and stream the RGB frames")
        yuv._check_layout_options(fmt, matrix, siting)
        super().__init__(model, patch_size, patch_overlap, need_degradation, noise_level, "float32", True)
        if luma_only and self.route.s > 1:
            raise ValueError(f"luma_only with model.upscale = {self.route.s}: the chroma planes would need a resize")
        self.fmt, self.luma_only = fmt, bool(luma_only)
        self.opts = dict(matrix=matrix, full_range=full_range, siting=siting, luma_only=self.luma_only)
        self.np_dtype = yuv._np_dtype(fmt)

    def prepare(self, planes):
        h, w = yuv._check_planes(planes, self.fmt, False, np.ndarray, (self.np_dtype,))
        return (h, w), tuple(planes[:1] if self.luma_only else planes), None, tuple(planes)

    def layout(self, key):
        h, w = key
        dt = _TORCH_KIND[np.dtype(self.np_dtype)]
        planes_in, planes_out = (yuv.plane_shapes(m * h, m * w, self.fmt, self.luma_only) for m in (1, self.route.s))
        return ((h, w, 1 if self.luma_only else 3), torch.float32, "float32", True), planes_in, dt, planes_out, dt

    def compute(self, plan, slot: int, k: int):
        rgb = [yuv.yuv_to_rgb_device(tuple(p), self.fmt, **self.opts) for p in plan.dev_in[slot][:k]]
        res = _tile_pipeline_run(self.model, plan.tp, rgb, None, self.route.max_batch, None)
        for (frame, _), planes in zip(res, plan.dev_out[slot][:k]):
            yuv.rgb_to_yuv_device(frame, self.fmt, out=tuple(planes), **self.opts)

    def finish(self, planes, outs):
        return tuple(outs) + tuple(planes[1:]) if self.luma_only else tuple(outs)     # the chroma as it came in


class _Plan:
    """The static buffers, events and tile plan of one (shape, dtype): two slots of each (module docstring)."""

    def __init__(self, front: _Front, key, k: int, device, with_targets: bool):
        (shape, dtype, out, unit_range), in_shapes, in_dtype, out_shapes, out_dtype = front.layout(key)
        r = front.route
        self.tp = _tile_pipeline_plan(front.model, shape, dtype, device, front.patch_size, front.patch_overlap, r.pad8,
                                      r.sigma, r.hooks, unit_range, out)
        out_dtype = out_dtype or self.tp.frame_dtype
        self.seen, self.count = set(), 0

        def slots(shapes, dtype, n=DEPTH):
            """n slots, pinned and on the device: (pinned buffers, their numpy views, device buffers, their views)."""
            pin = [plane_slots(shapes, dtype, k, device, True) for _ in range(n)]
            dev = [plane_slots(shapes, dtype, k, device, False) for _ in range(n)]
            return [p[0] for p in pin], [p[1] for p in pin], [d[0] for d in dev], [d[1] for d in dev]
        n_tgt = DEPTH if with_targets else 0
        self.pin_in, self.np_in, self.dev_in_buf, self.dev_in = slots(in_shapes, in_dtype)
        self.pin_out, self.np_out, self.dev_out_buf, self.dev_out = slots(out_shapes, out_dtype)
        self.pin_tgt, self.np_tgt, self.dev_tgt_buf, self.dev_tgt = slots(out_shapes, out_dtype, n_tgt)
        self.in_per, self.out_per = self.pin_in[0].numel() // k, self.pin_out[0].numel() // k
        self.dev_score = [torch.empty(2, k, dtype=torch.int64, device=device) for _ in range(n_tgt)]   # sse; the bits of ssim
        self.pin_score = [torch.empty(2, k, dtype=torch.int64, pin_memory=True) for _ in range(n_tgt)]
        self.up = [torch.cuda.Event() for _ in range(DEPTH)]
        self.done = [torch.cuda.Event() for _ in range(DEPTH)]
        self.down = [torch.cuda.Event() for _ in range(DEPTH)]

    def release(self) -> None:
        """Drop every buffer and event now (the three streams have been synchronised).  A traceback, and so a dead
        reference cycle, may keep this object alive for a while; the pinned memory must not wait for the cyclic
        collector, which could run inside a later graph capture, where releasing it is illegal."""
        for name, value in list(vars(self).items()):
            if isinstance(value, list):
                setattr(self, name, [])


def _copy_streams(device) -> tuple:
    return tuple(device_constant((name, str(device)), lambda: torch.cuda.Stream(device=device))
                 for name in ("stream_upload", "stream_download"))


def _fill(plan: _Plan, slot: int, group: list) -> None:
    """The frames (and targets) of a group into the pinned slot.  A function of its own: no view of pinned memory
    stays behind in a frame that an exception of the model may keep alive."""
    for dst, (_, arrays, _, _) in zip(plan.np_in[slot], group):
        for d, a in zip(dst, arrays):
            np.copyto(d, a)
    if plan.pin_tgt:
        for dst, (_, _, target, _) in zip(plan.np_tgt[slot], group):
            np.copyto(dst[0], target)


@torch.no_grad()
def _enqueue(front: _Front, plan: _Plan, slot: int, group: list, cur, up, down) -> None:
    """Fill, upload, compute and download of one group on its slot, under the four conditions of the module docstring."""
    k = len(group)
    plan.up[slot].synchronize()                                  # pinned-in: the upload of g - 2 has completed
    _fill(plan, slot, group)
    up.wait_event(plan.done[slot])                               # device-in: the compute of g - 2 is done
    with torch.cuda.stream(up):
        n = k * plan.in_per
        plan.dev_in_buf[slot][:n].copy_(plan.pin_in[slot][:n], non_blocking=True)
        if plan.pin_tgt:
            m = k * plan.out_per
            plan.dev_tgt_buf[slot][:m].copy_(plan.pin_tgt[slot][:m], non_blocking=True)
    plan.up[slot].record(up)
    cur.wait_event(plan.up[slot])
    cur.wait_event(plan.down[slot])                              # device-out: the download of g - 2 is done
    with torch.cuda.stream(cur):
        front.compute(plan, slot, k)
        if plan.pin_tgt:
            sse, ssim = frame_metrics_device([f[0] for f in plan.dev_out[slot][:k]], [f[0] for f in plan.dev_tgt[slot][:k]])
            plan.dev_score[slot][0, :k].copy_(sse)
            plan.dev_score[slot][1, :k].copy_(ssim.view(torch.int64))
    plan.done[slot].record(cur)
    down.wait_event(plan.done[slot])
    with torch.cuda.stream(down):                                # pinned-out: g - 2 was retired before this call
        m = k * plan.out_per
        plan.pin_out[slot][:m].copy_(plan.dev_out_buf[slot][:m], non_blocking=True)
        if plan.pin_tgt:
            plan.pin_score[slot].copy_(plan.dev_score[slot], non_blocking=True)
    plan.down[slot].record(down)


def _retire(front: _Front, plan: _Plan, slot: int, group: list) -> list:
    """Wait for the download of a group and copy its frames out of the pinned slot: [(result, extra, score)]."""
    plan.down[slot].synchronize()
    results = []
    for i, (views, (_, arrays, target, extra)) in enumerate(zip(plan.np_out[slot], group)):
        score = None
        if plan.pin_tgt:
            bits = plan.pin_score[slot][:, i].numpy().copy()
            score = (int(bits[0]), float(bits[1:].view(np.float64)[0]))
        results.append((front.finish(extra, [v.copy() for v in views]), extra, score))
    return results


def _stream(front: _Front, items, device, frames_per_step: int):
    """The generator under run_model_inference_stream and harness.evaluate_stream: (result, ms, extra, score) per
    frame in input order."""
    dev = torch.device(device)
    plans: collections.OrderedDict = collections.OrderedDict()
    pending: collections.deque = collections.deque()
    streams, err = None, None
    last = time.perf_counter()

    def retire():
        nonlocal last
        plan, slot, group = pending.popleft()
        results = _retire(front, plan, slot, group)
        now = time.perf_counter()
        ms, last = (now - last) * 1000.0 / len(group), now
        return [(r, ms, extra, score) for r, extra, score in results]

    groups = _grouped(items, front.prepare, frames_per_step)
    try:
        while True:
            try:
                group = next(groups)
                if streams is None:
                    cuda_device(dev, "run_model_inference_stream")
                    streams = (torch.cuda.current_stream(dev),) + _copy_streams(dev)
                key = group[0][0]
                plan = plans.get(key)
                fresh = plan is None or len(group) not in plan.seen
            except StopIteration:
                break
            except Exception as e:                              # noqa: BLE001 (re-raised after the groups in flight)
                err = e
                break
            while len(pending) > (0 if fresh else DEPTH - 1):
                yield from retire()
            try:
                if plan is None:
                    while len(plans) >= MAX_PLANS:
                        plans.popitem(last=False)[1].release()  # nothing of it is in flight: `pending` is empty here
                    plan = plans[key] = _Plan(front, key, frames_per_step, dev, front.with_targets)
                plans.move_to_end(key)
                slot, plan.count = plan.count % DEPTH, plan.count + 1
                _enqueue(front, plan, slot, group, *streams)
                plan.seen.add(len(group))
                pending.append((plan, slot, group))
            except Exception as e:                              # noqa: BLE001
                err = e
                break
            if fresh:
                yield from retire()
        while pending:                                          # the groups completed before the end or the error
            yield from retire()
        if err is not None:
            raise err
    finally:
        for st in streams or ():
            st.synchronize()
        for plan in plans.values():                             # nothing is in flight any more: free the buffers here,
            plan.release()                                      # not when a collector finds this frame (_Plan.release)
        plans.clear()
        pending.clear()
        err = plan = group = None


def run_model_inference_stream(model, frames, device, *, patch_size=None, patch_overlap=32, frames_per_step=4,
                               need_degradation=False, noise_level=None, out="same", unit_range=False, fmt=None,
                               matrix="bt709", full_range=False, siting="left", luma_only=False):
    """Restore a sequence of frames with the copies under the forwards: a generator of (prediction, ms) per frame of
    the iterable `frames`, in input order.

    fmt=None: frames are uint8 / uint16 / float32 [H, W, C] numpy arrays, and a prediction is what
    tiled_forward_device_batch(..., unit_range=, out=) gives for the frame, downloaded (uint16 through its int16 bit
    pattern).  fmt in yuv.YUV_LAYOUTS: a frame is the plane tuple run_model_inference_yuv takes and a prediction the plane
    tuple it returns, by the same route (matrix, full_range, siting and luma_only as there; out and unit_range do not
    apply).  The hooks follow the model class as get_model_prediction picks them, and what the one-frame calls refuse
    is refused here with ValueError - the arguments when the function is called, a frame when the iterable hands it
    over, after the frames before it have been yielded.  Nothing runs without a 'cuda' device (HipLibraryError).

    Consecutive frames of one shape and dtype form groups of `frames_per_step`; each group is one forward over the
    tiles of all its frames.  Another shape or dtype, or the end of the iterable, closes a group early.  Two groups
    are in flight: the upload of the next and the download of the previous one run under the forward of the current
    one (module docstring).  So results arrive up to 2 * frames_per_step frames after their input was taken.  A frame
    is copied into its pinned slot when its group is complete: an iterable that reuses one buffer for every frame has
    to hand out copies.

    `ms` is the host-clock interval between the results of this frame's group becoming available and those of the
    group before it - from the first next() for the first group - divided by the frames of the group: the `ms` of all
    frames add up to the wall time of the stream.  It is a throughput figure, not a latency.

    The yielded arrays are the caller's own copies.  Closing the generator early, an exception in the consumer, and an
    exception from the model or the iterable synchronise the stream's three GPU streams before they propagate; the
    frames of the groups completed before an error are yielded first."""
    k = _check_frames_per_step(frames_per_step)
    if fmt is None:
        front = _Front(model, patch_size, patch_overlap, need_degradation, noise_level, out, unit_range)
    else:
        if out != "same" or unit_range:
            raise ValueError("out and unit_range describe [H, W, C] frames: with fmt the planes come back in their format")
        front = _YuvFront(model, patch_size, patch_overlap, need_degradation, noise_level, fmt, matrix, full_range,
                          siting, luma_only)
    return _pairs(_stream(front, frames, device, k))


def _pairs(stream):
    try:
        for result, ms, _, _ in stream:
            yield result, ms
    finally:
        stream.close()                                          # synchronises the GPU streams (_stream's finally)


def score_psnr(sse: int, shape, dtype) -> float:
    """PSNR of a streamed frame from its integer squared error, as calculate_metrics_device takes it."""
    return psnr_from_error(255 if dtype == np.uint8 else 65535, sse / int(np.prod(shape)))
