"""Checkers of the resize to any size (irm_resize_taps) against its float64 statement utils.resize_host, shared by
tests/test_gpu_resize_any.py: the derived fp32 bound, the float and the quantised comparison, the frames, and a model
stand-in that records what a chain hands it."""
import numpy as np
import torch

from irm_amd import utils

PEAK = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0}


def fp32_bound(h, w, kw) -> float:
    """e = 2^-24 A^2 (PH + PW + 4) for a resize of an h x w frame with the arguments `kw` of resize_host, A the largest
    row sum of |w| over the two tables.  Where it comes from: every fp32 operation of a chain of P multiply-adds on
    values bounded by A (inputs in [0, 1], partial sums by the absolute row sum) rounds by at most 2^-24 A, half an ulp of
    a value below 2 A being counted with the next term; the H pass makes P_H of them, and its error passes through the W
    pass multiplied by at most A; the W pass adds P_W roundings of values up to A^2; the 4 covers v / 255, the two
    fp32 weights of a product and the conversion of the result."""
    oh, ow, sh, sw = utils.resize_plan(h, w, kw.get("size"), kw.get("scale"), kw.get("kernel", "bicubic"),
                                       kw.get("antialias", True))
    wh, _ = utils.resize_taps(h, oh, sh, kw.get("kernel", "bicubic"), kw.get("antialias", True))
    ww, _ = utils.resize_taps(w, ow, sw, kw.get("kernel", "bicubic"), kw.get("antialias", True))
    a = max(float(np.abs(wh).sum(1).max()), float(np.abs(ww).sum(1).max()))
    return 2.0 ** -24 * a * a * (wh.shape[1] + ww.shape[1] + 4)


def up(a: np.ndarray, dev) -> torch.Tensor:
    """A host frame on the GPU (uint16 as its int16 bit pattern)."""
    return torch.from_numpy(np.ascontiguousarray(a.view(np.int16) if a.dtype == np.uint16 else a)).to(dev)


def down(t: torch.Tensor, dtype=None) -> np.ndarray:
    a = t.view(torch.int16).cpu().numpy() if t.dtype == torch.uint16 else t.cpu().numpy()
    return a.view(np.uint16) if (dtype == np.uint16 or a.dtype == np.int16) else a


def as_dtype(u8: np.ndarray, kind: str, seed: int = 5) -> np.ndarray:
    """The uint8 frame as a frame of `kind`: 'u8' itself, 'u16' = 256 x the bytes + random low bytes, 'f32' = / 255."""
    if kind == "u8":
        return u8
    if kind == "u16":
        low = np.random.default_rng(seed).integers(0, 256, u8.shape).astype(np.uint16)
        return (u8.astype(np.uint16) * 256 + low).astype(np.uint16)
    return u8.astype(np.float32) / np.float32(255.0)


def check_float(got: np.ndarray, want: np.ndarray, e: float, what: str) -> float:
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: {got.shape} device fp32 vs float64 host max-abs {err:.3e} (bound {e:.3e})")
    assert err <= e, what
    return err


def check_quantised_near_ties(got: np.ndarray, want_float: np.ndarray, e: float, what: str) -> None:
    """`got` against round-half-to-even of clip(want_float) x peak: every value within 1, and a value differs only
    where the float64 value x peak lies within e x peak of a rounding boundary.  No cap on the differing share: with
    rational scales byte inputs land exactly on .5 boundaries, so the share is a property of the frame."""
    peak = PEAK[got.dtype]
    v = np.clip(want_float, 0.0, 1.0) * peak
    ref = np.round(v).astype(got.dtype)
    assert got.shape == ref.shape, what
    diff = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    to_boundary = np.abs(v - np.floor(v) - 0.5)
    bad = (diff > 0) & (to_boundary > e * peak)
    print(f"{what}: max difference {int(diff.max())}, {int((diff > 0).sum())} of {diff.size} differ, "
          f"{int(bad.sum())} of them away from a boundary")
    assert int(diff.max()) <= 1 and not bad.any(), what


def checker() -> np.ndarray:
    """The black / white checker of 3-pixel squares of tests/test_gpu_sr_protocol.py: 30 x 36 x 3 uint8."""
    yy, xx = np.mgrid[0:30, 0:36]
    return ((((yy // 3) + (xx // 3)) % 2) * 255).astype(np.uint8)[:, :, None].repeat(3, 2)


class Recorder(torch.nn.Module):
    """Stands in for a model in a chain: records the tiles it is given and returns them times `gain` (a power of two:
    exact)."""

    def __init__(self, gain=1.0):
        super().__init__()
        self.gain, self.seen = gain, []

    def forward(self, t):
        self.seen.append(t.detach().cpu().clone())
        return t * self.gain
