"""YUV4MPEG2 files (irm_amd/y4m.py) and harness.y4m_pairs: files written as byte literals read to the expected arrays,
write followed by read the identity for every planar format, every refusal, and the loader through evaluate_yuv."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import yuv_formats_model as fm
from irm_amd import _hip, harness, utils, y4m, yuv

CPU = torch.device("cpu")


def put(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(data)
    return str(path)


def test_a_420jpeg_file_written_by_hand(tmp_path):
    """4 x 2: eight luma bytes, then 2 x 1 U and 2 x 1 V; two frames, the second with a FRAME parameter."""
    data = (b"YUV4MPEG2 W4 H2 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n"
            b"FRAME\n" + bytes([1, 2, 3, 4, 5, 6, 7, 8]) + bytes([100, 101]) + bytes([200, 201])
            + b"FRAME Ip\n" + bytes([11, 12, 13, 14, 15, 16, 17, 18]) + bytes([110, 111]) + bytes([210, 211]))
    r = y4m.read_y4m(put(tmp_path, "a.y4m", data))
    assert (r.width, r.height, r.fmt, r.siting, r.full_range) == (4, 2, "i420", "center", None)
    assert r.fps == Fraction(30000, 1001) and r.frames == len(r) == 2
    frames = list(r)
    assert len(frames) == 2 and all(len(f) == 3 and all(p.dtype == np.uint8 for p in f) for f in frames)
    assert frames[0][0].tolist() == [[1, 2, 3, 4], [5, 6, 7, 8]]
    assert frames[0][1].tolist() == [[100, 101]] and frames[0][2].tolist() == [[200, 201]]
    assert frames[1][0].tolist() == [[11, 12, 13, 14], [15, 16, 17, 18]] and frames[1][2].tolist() == [[210, 211]]
    assert [f[0][0, 0] for f in r] == [1, 11], "a second iteration starts at the first frame"
    frames[0][0][0, 0] = 99                                              # the arrays are the caller's own
    assert next(iter(r))[0][0, 0] == 1


def test_a_422p10_file_written_by_hand(tmp_path):
    """4 x 3 at 10 bit: little-endian words, the code in the low bits; 12 luma words, then 2 x 3 U and 2 x 3 V."""
    le = lambda codes: b"".join(int(c).to_bytes(2, "little") for c in codes)        # noqa: E731
    y, u, v = list(range(1000, 1012)), [0, 1, 512, 513, 1022, 1023], [64, 940, 256, 257, 768, 769]
    data = b"YUV4MPEG2 W4 H3 F25:1 Ip C422p10 XCOLORRANGE=LIMITED\nFRAME\n" + le(y) + le(u) + le(v)
    assert le([1023]) == b"\xff\x03"
    r = y4m.read_y4m(put(tmp_path, "b.y4m", data))
    assert (r.width, r.height, r.fmt, r.siting, r.full_range, r.frames) == (4, 3, "i422p10", "left", False, 1)
    (py, pu, pv), = list(r)
    assert py.dtype == pu.dtype == np.uint16 and py.shape == (3, 4) and pu.shape == pv.shape == (3, 2)
    assert py.reshape(-1).tolist() == y and pu.reshape(-1).tolist() == u and pv.reshape(-1).tolist() == v
    assert yuv.yuv_to_rgb_host((py, pu, pv), r.fmt, siting=r.siting).shape == (3, 4, 3)


def test_the_colour_tags(tmp_path):
    want = {"C420jpeg": ("i420", "center"), "C420": ("i420", "center"), "": ("i420", "center"),
            "C420mpeg2": ("i420", "left"), "C422": ("i422", "left"), "C444": ("i444", "left")}
    want.update({f"C{s}p{d}": (f"i{s}p{d}", "left") for s in (420, 422, 444) for d in (10, 12)})
    assert len(want) == 12
    for tag, (fmt, siting) in want.items():
        r = y4m.read_y4m(put(tmp_path, "t.y4m", f"YUV4MPEG2 W2 H2 F1:1 {tag}\n".encode()))
        assert (r.fmt, r.siting, r.frames, r.full_range) == (fmt, siting, 0, None) and list(r) == []
    r = y4m.read_y4m(put(tmp_path, "t.y4m", b"YUV4MPEG2 W2 H2 F1:1 C444 XCOLORRANGE=FULL\n"))
    assert r.full_range is True


@pytest.mark.parametrize("fmt", fm.PLANAR)
def test_write_then_read_is_the_identity(tmp_path, fmt):
    assert len(fm.PLANAR) == 9
    sw, sh = fm.LAYOUTS[fmt][:2]
    h, w = 3 * sh, 5 * sw
    rng = np.random.default_rng(7)
    frames = [fm.random_planes(rng, fmt, h, w) for _ in range(3)]
    for siting, full in (("left", None), ("center", True), ("left", False)):
        if siting == "center" and fmt not in ("i420", "i444", "i444p10", "i444p12"):
            with pytest.raises(ValueError, match="siting"):
                y4m.write_y4m(str(tmp_path / "no.y4m"), frames, fmt, 24, siting=siting)
            continue
        path = str(tmp_path / f"{fmt}-{siting}.y4m")
        assert y4m.write_y4m(path, iter(frames), fmt, Fraction(24000, 1001), siting=siting, full_range=full) == 3
        r = y4m.read_y4m(path)
        assert (r.width, r.height, r.fmt, r.frames, r.full_range) == (w, h, fmt, 3, full)
        assert r.fps == Fraction(24000, 1001) and (r.siting == siting or sw == 1)
        back = list(r)
        assert len(back) == 3
        for f, b in zip(frames, back):
            assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(f, b))
        again = str(tmp_path / "again.y4m")
        y4m.write_y4m(again, back, r.fmt, r.fps, siting=r.siting, full_range=r.full_range)
        assert open(again, "rb").read() == open(path, "rb").read(), "bytes of the header included"
        assert open(path, "rb").readline().decode().rstrip("\n") == r.header
    assert y4m.write_y4m(str(tmp_path / "fps.y4m"), frames[:1], fmt, (30, 1)) == 1
    assert y4m.read_y4m(str(tmp_path / "fps.y4m")).fps == 30 and utils.read_y4m is y4m.read_y4m


def test_refusals(tmp_path):
    for tag in ("C420paldv", "Cmono", "Cmono16", "C444alpha", "C420p9", "C420p14", "C422p16", "C444p16", "C411"):
        with pytest.raises(ValueError, match=tag):
            y4m.read_y4m(put(tmp_path, "r.y4m", f"YUV4MPEG2 W4 H4 F25:1 Ip {tag}\n".encode()))
    for mode in ("It", "Ib", "Im"):
        with pytest.raises(ValueError, match=mode):
            y4m.read_y4m(put(tmp_path, "r.y4m", f"YUV4MPEG2 W4 H4 F25:1 {mode} C420jpeg\n".encode()))
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        y4m.read_y4m(put(tmp_path, "r.y4m", b"RIFF....AVI \n"))
    with pytest.raises(ValueError, match="W and H"):
        y4m.read_y4m(put(tmp_path, "r.y4m", b"YUV4MPEG2 W4 F25:1 C444\n"))
    with pytest.raises(ValueError, match="3 x 2"):
        y4m.read_y4m(put(tmp_path, "r.y4m", b"YUV4MPEG2 W3 H2 F25:1 C422\n"))
    with pytest.raises(ValueError, match="XCOLORRANGE"):
        y4m.read_y4m(put(tmp_path, "r.y4m", b"YUV4MPEG2 W2 H2 F25:1 C444 XCOLORRANGE=VIDEO\n"))
    # a truncated last frame, and a bad FRAME marker, name the frame
    frame = b"FRAME\n" + bytes(12)
    head = b"YUV4MPEG2 W2 H2 F25:1 C444\n"
    r = y4m.read_y4m(put(tmp_path, "r.y4m", head + frame + frame + frame[:-1]))
    assert r.frames == 2
    with pytest.raises(ValueError, match="frame 2 is truncated"):
        list(r)
    r = y4m.read_y4m(put(tmp_path, "r.y4m", head + frame + b"FRAMX\n" + bytes(12)))
    with pytest.raises(ValueError, match="frame 1 "):
        list(r)
    # the writer
    planes = fm.random_planes(np.random.default_rng(1), "i420", 2, 2)
    for bad in ("nv12", "p010", "p210", "yv12"):
        with pytest.raises(ValueError, match="planar"):
            y4m.write_y4m(str(tmp_path / "w.y4m"), [planes], bad, 25)
    with pytest.raises(ValueError, match="frame 0"):
        y4m.write_y4m(str(tmp_path / "w.y4m"), [tuple(p.astype(np.uint16) for p in planes)], "i420", 25)
    with pytest.raises(ValueError, match="frame 1"):
        y4m.write_y4m(str(tmp_path / "w.y4m"), [planes, fm.random_planes(np.random.default_rng(1), "i420", 2, 4)], "i420", 25)
    with pytest.raises(ValueError, match="fps"):
        y4m.write_y4m(str(tmp_path / "w.y4m"), [planes], "i420", 0)
    with pytest.raises(ValueError, match="at least one"):
        y4m.write_y4m(str(tmp_path / "w.y4m"), [], "i420", 25)


class Never(torch.nn.Module):
    def forward(self, t):
        raise AssertionError("the model must not run")


def test_y4m_pairs(tmp_path):
    rng = np.random.default_rng(3)
    a = [fm.random_planes(rng, "i422p10", 16, 16) for _ in range(3)]
    b = [fm.random_planes(rng, "i422p10", 16, 16) for _ in range(2)]
    pa, pb = str(tmp_path / "in.y4m"), str(tmp_path / "target.y4m")
    y4m.write_y4m(pa, a, "i422p10", 25, full_range=True)
    y4m.write_y4m(pb, b, "i422p10", 25)
    loader = harness.y4m_pairs(pa, pb)
    assert (loader.fmt, loader.siting, loader.full_range, loader.frames, len(loader)) == ("i422p10", "left", True, 2, 2)
    got = list(loader)
    assert [n for _, _, n in got] == ["in.y4m#0", "in.y4m#1"]
    for (x, t, _), fa, fb in zip(got, a, b):
        assert all(np.array_equal(p, q) for p, q in zip(x, fa)) and all(np.array_equal(p, q) for p, q in zip(t, fb))
    # mismatched headers
    y4m.write_y4m(str(tmp_path / "size.y4m"), [fm.random_planes(rng, "i422p10", 16, 18)], "i422p10", 25)
    y4m.write_y4m(str(tmp_path / "fmt.y4m"), [fm.random_planes(rng, "i422p12", 16, 16)], "i422p12", 25)
    with pytest.raises(ValueError, match="16 x 18|18 x 16"):
        harness.y4m_pairs(pa, str(tmp_path / "size.y4m"))
    with pytest.raises(ValueError, match="i422p12"):
        harness.y4m_pairs(pa, str(tmp_path / "fmt.y4m"))
    # through evaluate_yuv: valid arguments, no GPU - the frames reach run_model_inference_yuv's "no CPU fallback"
    kw = dict(task="denoising", subtask="gaussian", dataset="d", model_name="m")
    cfg = dict(patch_size=32, patch_overlap=8)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        harness.evaluate_yuv(Never(), loader, CPU, cfg, fmt=loader.fmt, siting=loader.siting,
                             full_range=loader.full_range, skip_failed=False, **kw)
    row = harness.evaluate_yuv(Never(), loader, CPU, cfg, fmt=loader.fmt, siting=loader.siting, **kw)
    assert [n for n, _ in row["Failed"]] == ["in.y4m#0", "in.y4m#1"]
