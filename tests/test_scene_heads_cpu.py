"""Host-side checks of whole-scene inference for SegCD's three maps and for UnetSeg: the numpy specification of
stcd_scene_finalize_seg (tests/scene_heads_spec.py) against a pixel-by-pixel loop, the header and the binding of the three new
entries, and the argument errors of predict_scene_seg / predict_scene_heads / scene_round(gate=...) that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from stcd_amd import _lib, selftrain
from stcd_amd.scene import SceneHeads, predict_scene_heads, predict_scene_seg
from tests import scene_heads_spec as HS
from tests import scene_tta_spec as TS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 7, 9


def _planes(classes, seed, seg_thr, chg_thr):
    """Small multiples of 1/4, so ties (a[1] == a[0], a[0] == threshold * wsum) are common, plus planted ones and a NaN."""
    rng = np.random.default_rng(seed)
    acc = rng.integers(-4, 5, size=(3 * classes, H, W)) / 4.0
    wsum = rng.integers(1, 4, size=(H, W)).astype(np.float64)
    for h in range(3):                                                # a tie in every head
        acc[h * classes:(h + 1) * classes, 0, 0] = 0.5 if classes == 2 else (chg_thr if h == 2 else seg_thr) * wsum[0, 0]
    acc[:, 3, 4] = np.nan                                             # compares false: class 0
    return acc, wsum


def _labels(seed):
    rng = np.random.default_rng(seed)
    labs = [rng.choice(np.array([0, 1, 7, 255], np.uint8), size=(H, W), p=[0.4, 0.3, 0.1, 0.2]) for _ in range(3)]
    labs[2][0, :] = 255                                               # a whole ignored row
    return labs


def _brute(acc, wsum, classes, seg_thr, chg_thr, labels, cm0):
    masks = np.zeros((4, H, W), np.uint8)
    cm = None if all(l is None for l in labels) else cm0.copy()
    for y in range(H):
        for x in range(W):
            for h in range(3):
                a = acc[h * classes:(h + 1) * classes, y, x]
                thr = chg_thr if h == 2 else seg_thr
                masks[h, y, x] = 1 if (a[1] > a[0] if classes == 2 else a[0] > thr * wsum[y, x]) else 0
            masks[3, y, x] = 1 if masks[2, y, x] == 1 and masks[0, y, x] != masks[1, y, x] else 0
            for r in range(4):
                lab = labels[min(r, 2)]
                if lab is None or lab[y, x] == 255:
                    continue
                cm[r, 2 * (1 if lab[y, x] >= 1 else 0) + masks[r, y, x]] += 1
    return masks, cm


@pytest.mark.parametrize("absent", [None, 0, 1, 2, "all"])
@pytest.mark.parametrize("classes", [1, 2])
def test_finalize_seg_spec_equals_a_pixel_loop(classes, absent):
    seg_thr, chg_thr = 0.25, -0.25
    acc, wsum = _planes(classes, 5 + classes, seg_thr, chg_thr)
    labels = _labels(11)
    if absent == "all":
        labels = [None, None, None]
    elif absent is not None:
        labels[absent] = None
    cm0 = np.arange(16, dtype=np.int64).reshape(4, 4) * 1000          # the counts are added to what cm holds
    with np.errstate(invalid="ignore"):
        sa, sb, ch, gt, prob, cm = HS.finalize_seg(acc, wsum, seg_thr, chg_thr, labels[0], labels[1], labels[2], cm0)
        masks, want_cm = _brute(acc, wsum, classes, seg_thr, chg_thr, labels, cm0)
    for got, want in zip((sa, sb, ch, gt), masks):
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want)
    assert prob.shape == (3, H, W)
    if absent == "all":
        assert cm is None
    else:
        np.testing.assert_array_equal(cm, want_cm)
        for r in range(4):                                            # the row of an absent label is left as it was
            if labels[min(r, 2)] is None:
                np.testing.assert_array_equal(cm[r], cm0[r])
            else:
                assert cm[r].sum() - cm0[r].sum() == int((labels[min(r, 2)] != 255).sum())
    assert not (sa[0, 0] or sb[0, 0] or ch[0, 0]) and not (sa[3, 4] or ch[3, 4])   # the tie and the NaN are class 0
    assert np.all(gt <= ch) and gt.any() and (gt != ch).any()


def test_header_declares_and_lib_lists_the_three_entries():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    for name in ("stcd_scene_gather_one_d4", "stcd_scene_stitch_heads_d4", "stcd_scene_finalize_seg"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in _lib.EXPORTS, f"{name} is not bound"
    assert re.search(r"#define\s+STCD_SCENE_MAX_HEADS\s+3\b", hdr)
    for cite in ("train_stcd.py:170-176", "decoders/unet/model.py:316-332", "train_sup.py:303"):
        assert cite in hdr, cite
    one, pair = _lib._PROTOS["stcd_scene_gather_one_d4"][1], _lib._PROTOS["stcd_scene_gather_d4"][1]
    assert len(one) == len(pair) - 2                                  # one scene and one batch fewer
    heads, single = _lib._PROTOS["stcd_scene_stitch_heads_d4"][1], _lib._PROTOS["stcd_scene_stitch_d4"][1]
    assert heads[0] is not single[0] and heads[1] is ctypes.c_int and list(heads[2:]) == list(single[1:])   # pointer array, n_heads, the rest
    assert len(_lib._PROTOS["stcd_scene_finalize_seg"][1]) == 17


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, *x):
        raise AssertionError("the model must not run: the arguments are wrong")


def test_predict_scene_seg_argument_errors_need_no_gpu():
    a = np.zeros((8, 8, 3), np.uint8)
    m = _Tiny()                                                       # on the CPU: a valid call ends at the no-CPU-fallback error
    TS.check_argument_errors(predict_scene_seg, m, _Tiny().to("meta"), ("scene",), ("label",))
    with pytest.raises(_lib.StcdError, match="GPU"):
        predict_scene_seg(m, a, tile=8)
    with pytest.raises(_lib.StcdError, match="GPU"):
        predict_scene_seg([m, m], a, tile=8, tta="d4", label=np.zeros((8, 8), np.uint8))
    with pytest.raises(_lib.StcdError, match="tta"):
        predict_scene_seg(m, a, tile=8, tta="rot90")
    with pytest.raises(_lib.StcdError, match="tta"):
        predict_scene_seg(m, a, tile=8, tta=[0, 0])
    with pytest.raises(_lib.StcdError, match=r"\[H,W,3\]"):
        predict_scene_seg(m, np.zeros((8, 8), np.uint8), tile=8)
    with pytest.raises(_lib.StcdError, match="label"):
        predict_scene_seg(m, a, tile=8, label=np.zeros((8, 7), np.uint8))
    with pytest.raises(_lib.StcdError, match="label"):
        predict_scene_seg(m, a, tile=8, label=np.zeros((8, 8), np.int64))
    with pytest.raises(_lib.StcdError, match="stride"):
        predict_scene_seg(m, a, tile=8, stride=9)
    with pytest.raises(_lib.StcdError, match="models"):
        predict_scene_seg([m] * 9, a, tile=8)


def test_predict_scene_heads_argument_errors_need_no_gpu():
    a = np.zeros((8, 8, 3), np.uint8)
    m = _Tiny()
    TS.check_argument_errors(predict_scene_heads, m, _Tiny().to("meta"), ("scene_a", "scene_b"), ("label", "label_a", "label_b"))
    with pytest.raises(_lib.StcdError, match="GPU"):
        predict_scene_heads(m, a, a, tile=8)
    with pytest.raises(_lib.StcdError, match="tta"):
        predict_scene_heads(m, a, a, tile=8, tta=[8])
    with pytest.raises(_lib.StcdError, match="differ in shape"):
        predict_scene_heads(m, a, np.zeros((8, 9, 3), np.uint8), tile=8)
    for key in ("label", "label_a", "label_b"):
        with pytest.raises(_lib.StcdError, match=key + " must be uint8"):
            predict_scene_heads(m, a, a, tile=8, **{key: np.zeros((9, 8), np.uint8)})
    with pytest.raises(_lib.StcdError, match="window"):
        predict_scene_heads(m, a, a, tile=8, window="hamming")
    with pytest.raises(_lib.StcdError, match="batch"):
        predict_scene_heads(m, a, a, tile=8, batch=0)
    with pytest.raises(_lib.StcdError, match="models"):
        predict_scene_heads([], a, a, tile=8)
    assert SceneHeads._fields == ("seg_a", "seg_b", "change", "gated", "prob", "cm", "scores")


def test_scene_round_rejects_an_unknown_gate_and_keeps_its_twelve_fields():
    a = np.zeros((8, 8, 3), np.uint8)
    for gate in ("change", "", 1, True):
        with pytest.raises(_lib.StcdError, match="gate"):
            selftrain.scene_round([_Tiny(), _Tiny()], a, a, cell=4, tile=8, gate=gate)
    fields = selftrain.SceneRound._fields
    assert fields[-2:] == ("seg_a", "seg_b") and len(fields) == 14
    r = selftrain.SceneRound(*range(12))                              # positional construction of the present twelve fields
    assert r.cell == 11 and r.seg_a is None and r.seg_b is None
