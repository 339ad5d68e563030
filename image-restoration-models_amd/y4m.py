"""YUV4MPEG2 (.y4m) files, the one uncompressed video container that needs no library: a reader that yields the planar
plane tuples run_model_inference_yuv, run_model_inference_stream(fmt=) and harness.evaluate_yuv take, and a writer.
Host only, numpy only.

A file is one header line, `YUV4MPEG2 W<w> H<h> F<n>:<d> I<p> A<n>:<d> C<tag> X<...>`, and then per frame a line that
starts with `FRAME` followed by the Y, U and V planes, row by row without padding; samples deeper than 8 bit are
little-endian 16-bit words with the code in the low bits.  The colour tag names sampling, depth and chroma siting:

    C420jpeg, C420 (and no C tag)   "i420", siting "center"
    C420mpeg2                       "i420", siting "left"
    C422, C444                      "i422", "i444", siting "left" (4:4:4 has no siting: the value is ignored)
    C420p10 .. C444p12              "i420p10" .. "i444p12", siting "left"

C420paldv (chroma co-sited vertically), Cmono*, C444alpha, 9-, 14- and 16-bit tags and interlaced files raise ValueError.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from .yuv import YUV_LAYOUTS, plane_shapes

MAGIC = b"YUV4MPEG2"
#: colour tag -> (fmt, siting)
TAGS = {"420jpeg": ("i420", "center"), "420": ("i420", "center"), "420mpeg2": ("i420", "left"),
        "422": ("i422", "left"), "444": ("i444", "left")}
TAGS.update({f"{s}p{d}": (f"i{s}p{d}", "left") for s in (420, 422, 444) for d in (10, 12)})
#: (fmt, siting) -> the tag write_y4m uses
_TAG_OF = {("i420", "center"): "420jpeg", ("i420", "left"): "420mpeg2", ("i422", "left"): "422", ("i444", "left"): "444",
           ("i444", "center"): "444"}
_TAG_OF.update({(f"i{s}p{d}", "left"): f"{s}p{d}" for s in (420, 422, 444) for d in (10, 12)})
_TAG_OF.update({(f"i444p{d}", "center"): f"444p{d}" for d in (10, 12)})


def _frame_layout(fmt, h: int, w: int):
    """The plane shapes of a frame, the stored dtype and the bytes of one frame."""
    shapes = plane_shapes(h, w, fmt)
    dt = np.dtype("u1") if YUV_LAYOUTS[fmt][3] == 8 else np.dtype("<u2")
    return shapes, dt, sum(s[0] * s[1] for s in shapes) * dt.itemsize


class Y4MReader:
    """An open-per-iteration reader: the header is parsed once, every iteration starts at the first frame.
    width, height, fps (a Fraction), fmt, siting, full_range (None unless an XCOLORRANGE tag says so), frames (whole
    frames in the file, from its size, assuming bare `FRAME` lines), header (the header line without its newline)."""

    def __init__(self, path):
        self.path = os.fspath(path)
        with open(self.path, "rb") as f:
            line = f.readline(4096)
        if not line.startswith(MAGIC + b" ") or not line.endswith(b"\n"):
            raise ValueError(f"{self.path}: not a YUV4MPEG2 file")
        self.header = line[:-1].decode("ascii", "replace")
        self._data = len(line)
        self.width = self.height = None
        self.fps, tag, self.full_range = Fraction(0), "420jpeg", None
        for token in self.header.split()[1:]:
            key, val = token[0], token[1:]
            if key == "W":
                self.width = int(val)
            elif key == "H":
                self.height = int(val)
            elif key == "F":
                n, _, d = val.partition(":")
                self.fps = Fraction(int(n), int(d or 1)) if int(d or 1) else Fraction(0)
            elif key == "I":
                if val in ("t", "b", "m"):
                    raise ValueError(f"{self.path}: interlaced material (I{val}) is not supported")
            elif key == "C":
                tag = val
            elif token.startswith("XCOLORRANGE="):
                rng = token.partition("=")[2]
                if rng not in ("FULL", "LIMITED"):
                    raise ValueError(f"{self.path}: unknown colour range tag {token}")
                self.full_range = rng == "FULL"
        if tag not in TAGS:
            raise ValueError(f"{self.path}: colour tag C{tag} is not supported (supported: "
                             f"{', '.join('C' + t for t in sorted(TAGS))})")
        if not self.width or not self.height or self.width <= 0 or self.height <= 0:
            raise ValueError(f"{self.path}: the header lacks a positive W and H")
        self.fmt, self.siting = TAGS[tag]
        sw, sh = YUV_LAYOUTS[self.fmt][:2]
        if self.width % sw or self.height % sh:
            raise ValueError(f"{self.path}: a C{tag} frame cannot be {self.width} x {self.height}")
        self._shapes, self._dtype, self._bytes = _frame_layout(self.fmt, self.height, self.width)
        self.frames = (os.path.getsize(self.path) - self._data) // (len(b"FRAME\n") + self._bytes)

    def __len__(self):
        return self.frames

    def __iter__(self):
        with open(self.path, "rb") as f:
            f.seek(self._data)
            index = 0
            while True:
                marker = f.readline(4096)
                if not marker:
                    return
                if not marker.startswith(b"FRAME") or not marker.endswith(b"\n") or marker[5:6] not in (b"\n", b" "):
                    raise ValueError(f"{self.path}: frame {index} does not start with a FRAME line")
                raw = f.read(self._bytes)
                if len(raw) != self._bytes:
                    raise ValueError(f"{self.path}: frame {index} is truncated ({len(raw)} of {self._bytes} bytes)")
                planes, at = [], 0
                for s in self._shapes:
                    n = s[0] * s[1]
                    native = self._dtype.newbyteorder("=")
                    planes.append(np.frombuffer(raw, self._dtype, n, at).astype(native).reshape(s))
                    at += n * self._dtype.itemsize
                yield tuple(planes)
                index += 1


def read_y4m(path) -> Y4MReader:
    """A Y4MReader of `path`; iterating it yields one (y, u, v) tuple of numpy arrays per frame."""
    return Y4MReader(path)


def write_y4m(path, frames, fmt, fps, siting="left", full_range=None) -> int:
    """Write planar frames - (y, u, v) tuples of numpy arrays in `fmt`, one of the planar names of YUV_LAYOUTS - to
    `path`; returns their number.  fps: an int, a Fraction or (numerator, denominator).  siting picks between C420jpeg
    ("center") and C420mpeg2 ("left") for "i420"; every other tag is "left" (4:4:4 ignores it).  full_range True /
    False adds XCOLORRANGE=FULL / LIMITED, None no tag."""
    if fmt not in YUV_LAYOUTS or YUV_LAYOUTS[fmt][2] != 3:
        raise ValueError(f"write_y4m writes the planar formats {sorted(f for f, v in YUV_LAYOUTS.items() if v[2] == 3)}, "
                         f"not {fmt!r}")
    if (fmt, siting) not in _TAG_OF:
        raise ValueError(f"no YUV4MPEG2 colour tag says {fmt!r} with siting {siting!r}")
    rate = Fraction(*fps) if isinstance(fps, (tuple, list)) else Fraction(fps).limit_denominator(1 << 20)
    if rate <= 0:
        raise ValueError(f"fps must be positive, not {fps!r}")
    dt = np.dtype("u1") if YUV_LAYOUTS[fmt][3] == 8 else np.dtype("<u2")
    count, shapes = 0, None
    with open(path, "wb") as f:
        for planes in frames:
            if not isinstance(planes, (tuple, list)) or len(planes) != 3 \
                    or not all(isinstance(p, np.ndarray) and p.dtype == dt.newbyteorder("=") for p in planes):
                raise ValueError(f"frame {count}: {fmt!r} frames are (y, u, v) numpy arrays of {dt.name}")
            if shapes is None:
                h, w = planes[0].shape
                shapes = plane_shapes(h, w, fmt)
                sw, sh = YUV_LAYOUTS[fmt][:2]
                if h % sh or w % sw:
                    raise ValueError(f"a {fmt!r} frame cannot be {h} x {w}")
                head = f"YUV4MPEG2 W{w} H{h} F{rate.numerator}:{rate.denominator} Ip A1:1 C{_TAG_OF[fmt, siting]}"
                if full_range is not None:
                    head += " XCOLORRANGE=" + ("FULL" if full_range else "LIMITED")
                f.write(head.encode("ascii") + b"\n")
            if [tuple(p.shape) for p in planes] != shapes:
                raise ValueError(f"frame {count}: the planes are {shapes}, not {[tuple(p.shape) for p in planes]}")
            f.write(b"FRAME\n")
            for p in planes:
                f.write(np.ascontiguousarray(p).astype(dt, copy=False).tobytes())
            count += 1
        if shapes is None:
            raise ValueError("write_y4m needs at least one frame: the header states the frame size")
    return count
