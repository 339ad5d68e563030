"""Device metrics path (irm_frame_metrics, utils.frame_metrics_device / calculate_metrics_device, harness metrics=)
checked without a GPU: the C-ABI symbol, the library's own argument checks (which return before touching HIP) and the
Python checks, which raise ValueError before the library is ever called."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from irm_amd import _hip, harness, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip.load()


def test_frame_metrics_symbol_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "irm_hip.h")).read()
    assert re.search(r"^int\s+irm_frame_metrics\s*\(", header, flags=re.M)
    assert "irm_frame_metrics" in _hip.SIGNATURES
    _lib()
    assert getattr(ctypes.CDLL(_hip.LIB_PATH), "irm_frame_metrics") is not None


def test_library_rejects_bad_geometry_before_any_launch():
    """Non-null placeholder pointers (never dereferenced: every check below fails before a launch)."""
    f = _lib().irm_frame_metrics
    fake = 4096

    def rc(k=1, h=720, w=1280, c=3, is_u16=0, data_range=255.0, ws_words=None):
        if ws_words is None:
            ws_words = 2 * k * -(-(h - 6) // 16) * -(-(w - 6) // (192 // max(c, 1)))
        return f(fake, fake, is_u16, k, h, w, c, data_range, fake, fake, fake, ws_words, None)

    assert rc(ws_words=2 * 45 * 20 - 1) == -1          # 720p RGB needs 2 x 45 x 20 words
    assert rc(c=2) == -1 and rc(c=4) == -1
    assert rc(h=6) == -1 and rc(w=6) == -1
    assert rc(k=0) == -1 and rc(is_u16=2) == -1
    assert rc(data_range=0.0) == -1 and rc(data_range=float("nan")) == -1
    assert rc(h=40000, w=40000, c=3) == -1               # more than 2^31 values in a frame


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library must not be called")
    monkeypatch.setattr(_hip, "call", boom)
    monkeypatch.setattr(_hip, "load", boom)


def test_cpu_tensors_raise_before_the_library(no_library):
    a = torch.zeros(32, 40, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        utils.calculate_metrics_device(a, a.clone())
    with pytest.raises(ValueError, match="GPU"):
        utils.frame_metrics_device([a], [a.clone()])
    with pytest.raises(ValueError, match="torch tensors"):
        utils.calculate_metrics_device(a.numpy(), a.numpy())


@pytest.mark.parametrize("shape", [(6, 40, 3), (40, 6, 3), (6, 6), (3, 100, 1)])
def test_side_shorter_than_7_raises(no_library, shape):
    a = torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at least 7"):
        utils.calculate_metrics_device(a, a.clone())
    with pytest.raises(ValueError, match="at least 7"):
        utils.frame_metrics_device([a], [a.clone()])


def test_mismatch_channels_and_dtype_raise(no_library):
    a = torch.zeros(16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="differ"):
        utils.calculate_metrics_device(a, torch.zeros(16, 17, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="differ"):
        utils.calculate_metrics_device(a, torch.zeros(16, 16, 3, dtype=torch.int16))
    with pytest.raises(ValueError, match="channels"):
        utils.calculate_metrics_device(torch.zeros(16, 16, 2, dtype=torch.uint8), torch.zeros(16, 16, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8 or uint16"):
        utils.calculate_metrics_device(a.float(), a.float())
    with pytest.raises(ValueError, match="same number"):
        utils.frame_metrics_device([a, a], [a])
    with pytest.raises(ValueError, match="same number"):
        utils.frame_metrics_device([], [])


def test_harness_rejects_unknown_metrics_mode():
    with pytest.raises(ValueError, match="metrics"):
        harness.evaluate(None, iter([]), "cpu", {}, task="denoising", subtask="gaussian", dataset="d", model_name="m",
                         metrics="gpu")


def test_host_metrics_unchanged_by_default_signature():
    """The harness default stays the host path; calculate_metrics itself is untouched (identical frames: inf, 1.0)."""
    import inspect
    assert inspect.signature(harness.evaluate).parameters["metrics"].default == "host"
    x = np.full((9, 9, 3), 7, np.uint8)
    assert utils.calculate_metrics(x, x.copy()) == (float("inf"), 1.0)
