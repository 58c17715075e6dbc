"""The specification of the nearest-seed transform and of the split (tests/nearest_spec.py) against the distance transform's
(tests/edt_spec.py), its tie rule on hand-made masks, the split fixtures with the object counts they were designed for, and the
four entries in the header and the binding.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

from stcd_amd import _lib
from stcd_amd.objects import TILE
from tests import edt_spec as E
from tests import nearest_spec as N
from tests import objects_spec as SP
from tests import rings_spec as RS
from tests import simplify_spec as SS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("stcd_edt_nearest_scratch_bytes", "stcd_edt_nearest", "stcd_edt_gather", "stcd_objects_split_cut")


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, TILE), **RS.patterns(*shape), **SS.patterns(*shape)}


@pytest.mark.parametrize("shape", [(96, 96), (67, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_index_gives_the_distance_of_the_edt_spec(shape):
    over = SP.overlay_for(*shape)
    H, W = shape
    for name, mask in all_patterns(shape).items():
        for to, ignore in (("unset", None), ("set", None), ("boundary", None), ("boundary", over)):
            seed = E.seeds(mask, to, ignore)
            index = N.nearest_index(seed)
            assert np.array_equal(N.d2_of_index(index), E.squared_distance(mask, to, ignore)), (name, to)
            if seed.any():
                assert index.min() >= 0 and seed.reshape(-1)[index].all(), (name, to)           # every index points at a seed
                assert np.array_equal(index[seed], np.flatnonzero(seed)), (name, to)            # and a seed at itself
            else:
                assert (index == -1).all(), (name, to)


def test_the_tie_rule():
    m = np.zeros((9, 11), np.uint8)
    m[4, 2] = m[4, 8] = 1                                       # left and right of (4, 5): the smaller column
    assert N.nearest_seed(m)[4, 5] == 4 * 11 + 2
    m = np.zeros((9, 11), np.uint8)
    m[1, 5] = m[7, 5] = 1                                       # above and below (4, 5): the smaller row
    assert N.nearest_seed(m)[4, 5] == 1 * 11 + 5
    m = np.zeros((9, 11), np.uint8)
    m[2, 3] = m[2, 7] = m[6, 3] = m[6, 7] = 1                   # the corners of a square round (4, 5): the left column, then its upper seed
    index = N.nearest_seed(m)
    assert index[4, 5] == 2 * 11 + 3
    assert index[4, 6] == 2 * 11 + 7 and index[5, 5] == 6 * 11 + 3 and index[4, 4] == 2 * 11 + 3
    m = np.zeros((9, 11), np.uint8)
    m[2, 7] = m[6, 3] = 1                                       # a lower seed in a smaller column beats an upper one in a larger
    assert N.nearest_seed(m)[4, 5] == 6 * 11 + 3
    full = np.ones((5, 7), np.uint8)
    assert np.array_equal(N.nearest_seed(full), np.arange(35).reshape(5, 7)) and (N.nearest_seed(full, "unset") == -1).all()


def test_expand_labels_of_the_spec():
    lab = np.zeros((9, 12), np.int32)
    lab[4, 2], lab[4, 9] = 5, 3
    assert np.array_equal(N.expand_labels(lab, 0), lab)
    grown = N.expand_labels(lab, 2.5)
    assert grown[4, 4] == 5 and grown[4, 7] == 3 and grown[4, 5] == 0 and grown[2, 3] == 5 and grown[1, 2] == 0
    far = N.expand_labels(lab, 1000)
    assert (far[:, :6] == 5).all() and (far[:, 6:] == 3).all()                      # columns 5 and 6 are 3 from one seed, 4 from the other
    assert not N.expand_labels(np.zeros((4, 4), np.int32), 1000).any()


@pytest.mark.parametrize("name", sorted(N.DISCS))
def test_the_disc_fixtures(name):
    make, objects, cut = N.DISCS[name]
    mask = make()
    assert SP.label(mask)[1] == 1
    s = N.split_objects(mask, 9.5)
    assert (SP.label(s["mask"])[1], s["n_cores"], s["cut_pixels"], s["orphan_pixels"]) == (objects, objects, cut, 0)
    assert int((mask != 0).sum()) - int((s["mask"] != 0).sum()) == cut
    s = N.split_objects(mask, 5)
    assert (SP.label(s["mask"])[1], s["n_cores"], s["cut_pixels"]) == (1, 1, 0) and np.array_equal(s["mask"], mask)


def test_the_rectangle_and_arm_fixtures():
    mask = N.rectangles()
    s = N.split_objects(mask, 3)
    assert (s["n_cores"], s["cut_pixels"], SP.label(s["mask"])[1]) == (1, 0, 1)
    s = N.split_objects(mask, 6)
    assert s["n_cores"] == 2 and s["cut_pixels"] > 0 and SP.label(s["mask"])[1] == 2
    s = N.split_objects(mask, 6, min_core_area=10 ** 6)
    assert (s["n_cores"], s["cut_pixels"], s["orphan_pixels"]) == (0, 0, int((mask != 0).sum())) and not s["owner"].any()
    mask = N.arm()
    assert SP.label(mask)[1] == 2
    s = N.split_objects(mask, 3)
    assert s["n_cores"] == 2 and s["orphan_pixels"] > 0 and s["cut_pixels"] == 0 and SP.label(s["mask"])[1] == 2
    assert np.array_equal(s["mask"], mask)
    # without the comparison of the components the arm would see both owners: its orphans sit beside the left square's owner
    orphans = (mask != 0) & (s["owner"] == 0)
    assert set(np.unique(SP.label(mask)[0][orphans])) == {1}


def test_the_header_declares_and_the_binding_binds_the_entries():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    declared = set(re.findall(r"\b(stcd_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
    assert len(_lib._PROTOS["stcd_edt_nearest"][1]) == 10 and len(_lib._PROTOS["stcd_edt_gather"][1]) == 10
    assert len(_lib._PROTOS["stcd_objects_split_cut"][1]) == 11
