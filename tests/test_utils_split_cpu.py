"""utils.py after its split by concern: the public surface it had before stays reachable through it, as the very
objects of the modules that now define them, and the tile geometry shared by the device pipeline and the host loop."""
import os
import subprocess
import sys

import pytest

from irm_amd import metrics, niqe, pipeline, resize, utils
from oracle import tiler_ref

#: the public names utils.py defined before the split
SURFACE = ['HALF_PRECISION_FAMILIES', 'PATCH_CONFIG', 'ROOT_RESULTS_DIR', 'ROOT_WEIGHTS_DIR', 'add_gaussian_noise',
           'calculate_metrics', 'calculate_metrics_basicsr', 'calculate_metrics_basicsr_device', 'calculate_metrics_device',
           'calculate_niqe', 'calculate_niqe_device', 'frame_metrics_basicsr_device', 'frame_metrics_device',
           'get_gaussian_weights', 'get_model_instance', 'get_model_prediction', 'get_model_total_parameters',
           'get_patch_config', 'graphed_forward', 'imresize_device', 'imresize_host', 'load_niqe_params', 'mod_crop',
           'niqe_feature_distance', 'niqe_features', 'niqe_features_device', 'niqe_gamma_table', 'niqe_plane', 'niqe_score',
           'normalize', 'pad', 'psnr', 'resize_table', 'run_model_chain', 'run_model_inference', 'ssim', 'tile_origins',
           'tiled_forward_device', 'tiled_forward_device_batch']
MOVED = {metrics: ['psnr', 'ssim', 'calculate_metrics', 'frame_metrics_device', 'calculate_metrics_device',
                   'calculate_metrics_basicsr', 'frame_metrics_basicsr_device', 'calculate_metrics_basicsr_device'],
         resize: ['mod_crop', 'resize_table', 'imresize_host', 'imresize_device'],
         niqe: ['load_niqe_params', 'niqe_gamma_table', 'niqe_features', 'niqe_score', 'niqe_feature_distance', 'niqe_plane',
                'calculate_niqe', 'calculate_niqe_device', 'niqe_features_device'],
         pipeline: ['graphed_forward', 'tiled_forward_device', 'tiled_forward_device_batch', 'tile_origins',
                    'get_gaussian_weights']}


def test_utils_keeps_its_public_surface():
    assert len(SURFACE) == len(set(SURFACE)) == 39
    missing = [n for n in SURFACE if not hasattr(utils, n)]
    assert not missing, missing
    moved = [n for names in MOVED.values() for n in names]
    assert len(moved) == len(set(moved)) == 26 and set(moved) <= set(SURFACE)
    for home, names in MOVED.items():
        for n in names:
            assert getattr(utils, n) is getattr(home, n), n
            assert getattr(home, n).__module__ == home.__name__, n
    for n in set(SURFACE) - set(moved):
        assert getattr(getattr(utils, n), "__module__", utils.__name__) == utils.__name__, n


_CHILD = """
import sys
import torch
import irm_amd
from irm_amd import pipeline, stream
front = stream._Front(torch.nn.Identity(), 32, 8, False, None, "same", False)
assert front.route == pipeline.model_route(front.model) == (None, False, 1, None, 8), front.route
assert stream.group_frames(["a", "a", "b"], 2) == [[0, 1], [2]]
assert "irm_amd.pipeline" in sys.modules and "irm_amd.utils" not in sys.modules, "stream.py imported utils"
"""


def test_the_stream_stands_on_the_pipeline_without_utils():
    """pipeline.py is a layer below utils.py and stream.py: a fresh interpreter that builds a stream front for a model
    and groups frames has never imported utils."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


#: (h, w, patch_size, overlap) -> ps, row origins, column origins, th, tw
PLANS = {(75, 61, 50, 10): (50, [0, 25], [0, 11], 50, 50),
         (40, 90, 64, 16): (64, [0], [0, 26], 40, 64),               # the image is shorter than the patch
         (64, 64, None, 32): (64, [0], [0], 64, 64),                 # no patch size: the whole image
         (100, 136, 64, 16): (64, [0, 36], [0, 48, 72], 64, 64)}
PADDED = {"none": {40: 40, 50: 50, 64: 64}, "reflect8": {40: 40, 50: 56, 64: 64}, "zero32": {40: 64, 50: 64, 64: 96}}


@pytest.mark.parametrize("shape", list(PLANS))
@pytest.mark.parametrize("pad_mode", list(PADDED))
def test_tile_plan(shape, pad_mode):
    h, w, patch, overlap = shape
    ps, ys, xs, th, tw = PLANS[shape]
    if patch:
        assert ys == tiler_ref.tile_origins(h, ps, overlap) and xs == tiler_ref.tile_origins(w, ps, overlap)
    want = (ps, [(y0, x0) for y0 in ys for x0 in xs], th, tw, PADDED[pad_mode][th], PADDED[pad_mode][tw])
    assert utils.tile_plan(h, w, patch, overlap, pad_mode) == want
    if pad_mode == "none":
        assert utils.tile_plan(h, w, patch, overlap) == want
