"""Whole-scene inference, the part that needs no GPU: the three C-ABI entries exist, the tile plan covers every scene, the
closed forms of tests/scene_spec.py equal a brute-force scan, the windows are usable weights, and predict_scene refuses a CPU
model."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from tests import scene_spec as SP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("stcd_scene_gather", "stcd_scene_stitch", "stcd_scene_finalize")
SIZES = (1, 255, 256, 257, 300, 1024)


def test_scene_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    declared = set(re.findall(r"\b(stcd_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in stcd_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(raw, name), f"{name} is not exported by the library"
    assert _lib.lib().stcd_abi_version() == 2            # additions only


@pytest.mark.parametrize("stride_of", [lambda t: t, lambda t: t // 2, lambda t: t // 4, lambda t: 37])
@pytest.mark.parametrize("tile", [256, 64])
def test_plan_tiles_covers_the_scene(tile, stride_of):
    from stcd_amd.scene import plan_tiles
    stride = stride_of(tile)
    for L in SIZES:
        plan = plan_tiles(L, SIZES[-1 - SIZES.index(L)], tile, stride)          # H and W take different values of the set
        for length, tiles in ((L, plan.tiles_y), (SIZES[-1 - SIZES.index(L)], plan.tiles_x)):
            assert tiles == SP.tiles_along(length, tile, stride)
            assert (tiles - 1) * stride < length, "the last tile starts past the scene"      # every tile overlaps the scene
            lo, hi = SP.covering(np.arange(length), tile, stride, tiles)
            assert (hi >= lo).all(), "a pixel no tile covers"
            for p in range(length):
                assert list(range(lo[p], hi[p] + 1)) == SP.covering_brute(p, tile, stride, tiles), (length, tile, stride, p)
        assert plan.n == plan.tiles_y * plan.tiles_x and plan.tile == tile and plan.stride == stride


def test_plan_tiles_defaults_and_errors():
    from stcd_amd.scene import plan_tiles
    assert tuple(plan_tiles(1024, 1024)) == (4, 4, 16, 256, 256)
    assert tuple(plan_tiles(1024, 1024, 256, 128)) == (7, 7, 49, 256, 128)
    assert tuple(plan_tiles(100, 70, 256)) == (1, 1, 1, 256, 256)               # a scene smaller than one tile
    for bad in (0, 257, -1):
        with pytest.raises(_lib.StcdError):
            plan_tiles(300, 300, 256, bad)


@pytest.mark.parametrize("tile", [8, 64, 256])
def test_hann_window_is_strictly_positive_and_symmetric(tile):
    from stcd_amd.scene import window_table
    w = window_table(tile, "hann")
    assert w.dtype == np.float32 and w.shape == (tile,)
    assert (w > 0).all()
    np.testing.assert_array_equal(w, w[::-1])
    i = np.arange(tile, dtype=np.float64)
    np.testing.assert_array_equal(w, (0.5 - 0.5 * np.cos(2 * np.pi * (i + 0.5) / tile)).astype(np.float32))
    np.testing.assert_array_equal(window_table(tile, "flat"), np.ones(tile, np.float32))
    with pytest.raises(_lib.StcdError):
        window_table(tile, "bartlett")


@pytest.mark.parametrize("kind", ["flat", "hann"])
@pytest.mark.parametrize("H,W,T,S", [(300, 420, 64, 32), (100, 70, 64, 16), (64, 64, 64, 64), (257, 255, 128, 37)])
def test_constant_logit_survives_the_blend(kind, H, W, T, S):
    from stcd_amd.scene import plan_tiles, window_table
    plan = plan_tiles(H, W, T, S)
    logits = np.full((plan.n, 2, T, T), 0.0, np.float32)
    logits[:, 0], logits[:, 1] = -1.75, 0.3
    acc, wsum = np.zeros((2, H, W)), np.zeros((H, W))
    SP.stitch(logits, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, window_table(T, kind), acc, wsum)
    assert (wsum > 0).all()
    np.testing.assert_allclose(acc[0] / wsum, np.float32(-1.75), rtol=1e-6)
    np.testing.assert_allclose(acc[1] / wsum, np.float32(0.3), rtol=1e-6)
    mask, prob, _ = SP.finalize(acc, wsum)
    assert mask.all()
    np.testing.assert_allclose(prob, 1 / (1 + np.exp(-(np.float64(np.float32(0.3)) + 1.75))), rtol=1e-6)


def test_spec_reflection_is_numpy_reflect():
    for L in (1, 2, 5, 70):
        base = np.arange(L)
        pad = 3 * L
        want = base if L == 1 else np.pad(base, (pad, pad), mode="reflect")
        got = SP.reflect(np.arange(-pad, L + pad), L)
        np.testing.assert_array_equal(got, np.zeros(L + 2 * pad, np.int64) if L == 1 else want)


def test_predict_scene_refuses_a_cpu_model():
    from stcd_amd.modules import SiamUnet_diff
    from stcd_amd.scene import predict_scene
    scene = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(_lib.StcdError):
        predict_scene(SiamUnet_diff(3, 2), scene, scene, tile=64)
    with pytest.raises(_lib.StcdError):
        predict_scene(torch.nn.Conv2d(3, 2, 1), scene, scene, tile=64)
