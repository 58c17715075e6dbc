"""Host-side checks of the D4 views of whole-scene inference: the numpy specification (tests/scene_tta_spec.py) is consistent
with itself and with tests/scene_spec.py, the header declares the two entries and _lib binds them, and predict_scene's new
argument errors are raised without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd.scene import MAX_MODELS, parse_tta, plan_tiles, predict_scene, window_table
from tests import scene_spec as SP
from tests import scene_tta_spec as TS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _asym(T, lead=(2, 3)):
    return np.arange(int(np.prod(lead)) * T * T, dtype=np.float64).reshape(*lead, T, T)


@pytest.mark.parametrize("T", [1, 2, 5, 8])
def test_the_eight_views_are_distinct_and_the_inverse_is_exact(T):
    x = _asym(T)
    views = [TS.d4_apply(x, d) for d in TS.VIEWS]
    for d in TS.VIEWS:
        np.testing.assert_array_equal(TS.d4_invert(views[d], d), x)
        np.testing.assert_array_equal(TS.d4_apply(TS.d4_invert(x, d), d), x)
    if T >= 2:
        for d in TS.VIEWS:
            for e in range(d):
                assert not np.array_equal(views[d], views[e]), (d, e)


@pytest.mark.parametrize("T", [1, 3, 6])
@pytest.mark.parametrize("d", TS.VIEWS)
def test_index_formulas_equal_the_slicing_form(d, T):
    x = _asym(T)
    np.testing.assert_array_equal(TS.d4_apply_index(x, d), TS.d4_apply(x, d))
    np.testing.assert_array_equal(TS.d4_invert_index(x, d), TS.d4_invert(x, d))


def test_the_code_is_mirror_then_transpose():
    x = _asym(4, lead=(1,))
    np.testing.assert_array_equal(TS.d4_apply(x, 1), x[..., ::-1])
    np.testing.assert_array_equal(TS.d4_apply(x, 2), x[..., ::-1, :])
    np.testing.assert_array_equal(TS.d4_apply(x, 4), x.swapaxes(-1, -2))
    np.testing.assert_array_equal(TS.d4_apply(x, 7), x[..., ::-1, ::-1].swapaxes(-1, -2))
    np.testing.assert_array_equal(TS.d4_apply(x, 5), np.rot90(x, 1, axes=(-2, -1)))      # mirror columns, then transpose
    np.testing.assert_array_equal(TS.d4_apply(x, 6), np.rot90(x, -1, axes=(-2, -1)))


@pytest.mark.parametrize("H,W,T,S", [(20, 13, 8, 4), (1, 5, 8, 8), (17, 9, 6, 3)])
def test_view_zero_is_the_upright_spec_and_views_stitch_back(H, W, T, S):
    rng = np.random.default_rng(H)
    scene = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    plan = plan_tiles(H, W, T, S)
    up = SP.gather(scene, T, S, plan.tiles_x, 0, plan.n, MEAN, STD)
    np.testing.assert_array_equal(TS.gather_d4(scene, T, S, plan.tiles_x, 0, plan.n, MEAN, STD, 0), up)
    logits = rng.standard_normal((plan.n, 2, T, T))
    win = window_table(T, "hann")
    want = SP.stitch(logits, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, win, np.zeros((2, H, W)), np.zeros((H, W)))
    for d in TS.VIEWS:
        np.testing.assert_array_equal(TS.gather_d4(scene, T, S, plan.tiles_x, 0, plan.n, MEAN, STD, d), TS.d4_apply_index(up, d))
        got = TS.stitch_d4(TS.d4_apply(logits, d), H, W, T, S, plan.tiles_x, plan.tiles_y, 0, win, np.zeros((2, H, W)), np.zeros((H, W)), d)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_header_declares_and_lib_binds_the_two_entries():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    for name, base in (("stcd_scene_gather_d4", "stcd_scene_gather"), ("stcd_scene_stitch_d4", "stcd_scene_stitch")):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in _lib.EXPORTS, f"{name} is not bound"
        fn, bfn = getattr(_lib.lib(), name), getattr(_lib.lib(), base)
        args, bargs = list(fn.argtypes), list(bfn.argtypes)
        assert fn.restype is bfn.restype and len(args) == len(bargs) + 1
        assert args[:-2] == bargs[:-1] and args[-2] is ctypes.c_int and args[-1] is bargs[-1]   # the base's arguments, int d4, the stream
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert re.search(r"\bint\s+d4\s*,\s*void\s*\*\s*hip_stream\s*$", decl.strip())
    assert _lib.lib().stcd_abi_version() == 2


@pytest.mark.parametrize("tta,want", TS.TTA_EXPECTED, ids=[str(i) for i in range(len(TS.TTA_EXPECTED))])
def test_parse_tta(tta, want):
    got = parse_tta(tta)
    assert got == want and all(type(d) is int for d in got)


@pytest.mark.parametrize("tta", TS.TTA_ERRORS, ids=[str(i) for i in range(len(TS.TTA_ERRORS))])
def test_parse_tta_errors(tta):
    with pytest.raises(_lib.StcdError, match="tta"):
        parse_tta(tta)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x1, x2):
        raise AssertionError("the model must not run: the arguments are wrong")


def test_predict_scene_argument_errors_need_no_gpu():
    a = np.zeros((8, 8, 3), np.uint8)
    m = _Tiny()                                                       # on the CPU: a valid call would end at the no-CPU-fallback error
    TS.check_argument_errors(predict_scene, m, _Tiny().to("meta"), ("scene_a", "scene_b"), ("label",))
    for tta in TS.TTA_ERRORS:
        with pytest.raises(_lib.StcdError, match="tta"):
            predict_scene(m, a, a, tile=8, tta=tta)
    with pytest.raises(_lib.StcdError, match="models"):
        predict_scene([], a, a, tile=8)
    with pytest.raises(_lib.StcdError, match="models"):
        predict_scene((), a, a, tile=8, tta="d4")
    with pytest.raises(_lib.StcdError, match="models"):
        predict_scene([m] * (MAX_MODELS + 1), a, a, tile=8)
    with pytest.raises(_lib.StcdError, match="Module"):
        predict_scene([m, "checkpoint.pt"], a, a, tile=8)
    with pytest.raises(_lib.StcdError, match="different devices"):
        predict_scene([m, _Tiny().to("meta")], a, a, tile=8)
    with pytest.raises(_lib.StcdError, match="GPU"):                  # the checks above passed: only the device is wrong
        predict_scene([m] * MAX_MODELS, a, a, tile=8, tta=[7, 0])
    assert MAX_MODELS == 8
