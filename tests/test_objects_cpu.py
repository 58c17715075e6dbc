"""Change objects, the part that needs no GPU: the specification of tests/objects_spec.py equals scipy.ndimage.label on the
pattern list, its filter and inversion obey their identities, the four C-ABI entries exist and refuse bad arguments before any HIP
call, and refine_round's host logic leaves every other field of a SceneRound alone (the launches replaced by the specification)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import objects as OB
from stcd_amd import selftrain as ST
from stcd_amd.metrics import scores_from_cm
from tests import objects_spec as SP
from tests import scene_round_spec as RS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = OB.TILE
SHAPES = [(1, 1), (1, T + 3), (T + 3, 1), (T, T), (T + 1, T + 1), (2 * T + 5, 3 * T - 1), (3 * T, 3 * T), (37, 131)]
FILTERS = [(5, 0), (0, 6), (4, 9), (30, 200)]


def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    declared = set(re.findall(r"\b(stcd_[a-z0-9_]+)\s*\(", hdr))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("stcd_objects_scratch_bytes", "stcd_objects_label", "stcd_objects_table", "stcd_mask_filter_objects"):
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name)
    assert _lib.lib().stcd_abi_version() == 2                   # additions only
    assert T == 64


# ------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_spec_labelling_is_scipys(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    cross, full = ndi.generate_binary_structure(2, 1), np.ones((3, 3), bool)
    for name, m in SP.patterns(*shape, T).items():
        for conn, structure in ((4, cross), (8, full)):
            want, n_want = ndi.label(m != 0, structure=structure)
            got, n = SP.label(m, conn)
            assert n == n_want and np.array_equal(got, want), (name, conn)


def test_spec_numbers_the_known_cases():
    p = SP.patterns(2 * T + 5, 3 * T - 1, T)
    H, W = p["empty"].shape
    assert SP.label(p["empty"], 8)[1] == 0 and SP.label(p["full"], 4)[1] == 1 and SP.label(p["corners"], 8)[1] == 4
    assert SP.label(p["checkerboard"], 8)[1] == 1 and SP.label(p["checkerboard"], 4)[1] == (H * W + 1) // 2
    for name in ("serpentine", "spiral", "comb"):
        assert SP.label(p[name], 4)[1] == 1 and SP.label(p[name], 8)[1] == 1, name
        assert np.count_nonzero(p[name]) >= H * W // 2 - H - W, name      # the path covers about half the scene
    for name in ("corner_diag_main", "corner_diag_anti"):
        assert SP.label(p[name], 8)[1] == 1 and SP.label(p[name], 4)[1] == 2, name
    lab, n = SP.label(p["corners"], 8)
    area, bbox, ov = SP.table(lab, n, SP.overlay_for(H, W))
    assert area.tolist() == [1, 1, 1, 1] and bbox.tolist() == [[0, 0, 0, 0], [0, W - 1, 0, W - 1], [H - 1, 0, H - 1, 0], [H - 1, W - 1, H - 1, W - 1]]
    assert ov.shape == (4, 2) and (ov[:, 1] <= ov[:, 0]).all() and (ov[:, 0] <= area).all()


def test_spec_labels_a_megapixel_in_seconds():
    import time
    m = (np.random.default_rng(7).random((1024, 1024)) < 0.593).astype(np.uint8)
    t0 = time.perf_counter()
    lab, n = SP.label(m, 4)
    assert time.perf_counter() - t0 < 20.0
    assert n > 1 and np.array_equal(lab != 0, m != 0)


@pytest.mark.parametrize("shape", [(T + 3, 1), (T + 1, T + 1), (2 * T + 5, 3 * T - 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_spec_filter_identities(shape):
    for name, m in SP.patterns(*shape, T).items():
        for conn in (4, 8):
            assert np.array_equal(SP.filter_objects(m, 1, 0, conn, 9), (m != 0).astype(np.uint8) * 9), (name, conn)
            lab, n = SP.label(m, conn, invert=True)
            lab2, n2 = SP.label((m == 0).astype(np.uint8), conn)
            assert n == n2 and np.array_equal(lab, lab2), (name, conn)
            for min_area, max_hole in FILTERS:
                once = SP.filter_objects(m, min_area, max_hole, conn)
                assert np.array_equal(SP.filter_objects(once, min_area, max_hole, conn), once), (name, conn, min_area, max_hole)
                if max_hole == 0:
                    assert not (once != 0)[m == 0].any()        # step 1 only clears
                if min_area <= 1:
                    assert (once != 0)[m != 0].all()            # step 2 only sets


def test_spec_hole_step_on_the_ring_cases():
    p = SP.patterns(2 * T + 5, 3 * T - 1, T)
    ring = p["rings"]
    filled = SP.filter_objects(ring, 0, 10 ** 6, 8, 1)
    assert filled.sum() > (ring != 0).sum()                     # both holes are filled ...
    assert SP.label(filled, 8, invert=True)[1] == 1             # ... and only the outside is left
    assert np.array_equal(SP.filter_objects(ring, 0, 5, 8, 1), (ring != 0).astype(np.uint8))          # both holes are larger than 5
    island = SP.filter_objects(p["ring_island"], 0, 10 ** 6, 8, 1)
    assert SP.label(island, 8)[1] == 1 and SP.label(island, 8, invert=True)[1] == 1
    for name in ("ring_on_border", "notch"):                    # an unset component touching the border is never filled
        m = p[name]
        out = SP.filter_objects(m, 0, 10 ** 6, 8, 1)
        lab, n = SP.label(m, 4, invert=True)
        edge = set(lab[0].tolist()) | set(lab[-1].tolist()) | set(lab[:, 0].tolist()) | set(lab[:, -1].tolist())
        assert len(edge - {0}) >= 2, name                       # the case has unset components at the border besides the outside
        for l in edge - {0}:
            assert not out[lab == l].any(), name


def test_spec_matching_counts():
    pred = np.zeros((20, 30), np.uint8)
    lab = np.zeros((20, 30), np.uint8)
    pred[2:6, 2:6] = 255; lab[2:6, 3:7] = 1                     # 12 of 16 pixels overlap: matched both ways
    pred[10:12, 10:20] = 255; lab[10:12, 18:20] = 1             # 4 of 20 predicted pixels hit; the label object is covered
    lab[15:18, 1:4] = 1                                         # missed
    pred[15:17, 25:28] = 255; lab[15:17, 25:28] = 255           # every pixel ignored: dropped
    assert SP.match_counts(pred, lab, 8, 0.5) == (2, 3, 1, 2)
    n_pred, n_label, tp_pred, tp_label, precision, recall, f1 = OB.score_tables(np.array([[16, 12], [20, 4], [0, 0]]), np.array([[16, 12], [4, 4], [9, 0]]), 0.5)
    assert (n_pred, n_label, tp_pred, tp_label) == (2, 3, 1, 2)
    assert precision == 0.5 and recall == 2 / 3 and f1 == pytest.approx(2 * 0.5 * (2 / 3) / (0.5 + 2 / 3))
    assert OB.score_tables(np.zeros((0, 2)), np.zeros((0, 2)))[4:] == (0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ the C entries' argument checks
def _bytes(h=10, w=12):
    return int(_lib.lib().stcd_objects_scratch_bytes(h, w))


def test_scratch_bytes():
    assert _bytes(0, 0) >= 8 and _bytes(10, 12) >= 9 * 120 + 8 and _bytes(10, 12) % 8 == 0
    assert _bytes(4096, 4096) >= 9 * 4096 * 4096
    assert _bytes(-1, 4) == 0 and _bytes(4, -1) == 0 and _bytes(1 << 16, 1 << 15) == 0 and _bytes(46341, 46341) == 0
    assert _bytes(46340, 46340) > 0                             # the largest square below 2^31 pixels


def _host():
    """HOST buffers: every call here is refused (or has nothing to launch) before any HIP call."""
    buf = np.zeros(65536, np.int64)
    return buf, buf.ctypes.data


def _label_call(height=10, width=12, connectivity=8, invert=0, null=None, short=0, odd=0):
    buf, base = _host()
    p = lambda name, off: None if null == name else C.c_void_p(base + off)
    rc = _lib.lib().stcd_objects_label(p("mask", 0), height, width, connectivity, invert, p("labels", 1024 + odd), p("count", 4096), p("scratch", 8192),
                                       max(_bytes(height, width), 8) - short, None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(null="mask"), dict(null="labels"), dict(null="count"), dict(null="scratch"), dict(height=-1), dict(width=-1),
                                dict(height=1 << 16, width=1 << 15), dict(height=46341, width=46341), dict(connectivity=6), dict(connectivity=0),
                                dict(invert=2), dict(short=4), dict(short=8), dict(odd=2)])
def test_label_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _label_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_objects_label: "), err


def _table_call(height=10, width=12, n=3, null=None, overlay=True, overlap=True):
    buf, base = _host()
    p = lambda name, off, on=True: None if null == name or not on else C.c_void_p(base + off)
    rc = _lib.lib().stcd_objects_table(p("labels", 0), height, width, n, p("overlay", 1024, overlay), p("area", 2048), p("bbox", 4096),
                                       p("overlap", 8192, overlap), None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(null="labels"), dict(null="area"), dict(null="bbox"), dict(overlay=False), dict(overlap=False), dict(height=-1),
                                dict(width=-1), dict(height=1 << 16, width=1 << 15), dict(n=-1), dict(n=121)])
def test_table_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _table_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_objects_table: "), err


def _filter_call(height=10, width=12, connectivity=8, min_area=4, max_hole=4, mask_value=255, null=None, inp=0, out=1024, scratch=8192, short=0):
    buf, base = _host()
    p = lambda name, off: None if null == name else C.c_void_p(base + off)
    rc = _lib.lib().stcd_mask_filter_objects(p("in", inp), height, width, connectivity, min_area, max_hole, mask_value, p("out", out), p("scratch", scratch),
                                             max(_bytes(height, width), 8) - short, None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(null="in"), dict(null="out"), dict(null="scratch"), dict(height=-1), dict(width=-1), dict(height=1 << 16, width=1 << 15),
                                dict(connectivity=6), dict(connectivity=-8), dict(mask_value=0), dict(mask_value=256), dict(max_hole=-1), dict(short=4),
                                dict(short=1), dict(out=0), dict(out=119), dict(inp=100, out=0), dict(scratch=1024 + 64), dict(inp=8192 + 16),
                                dict(scratch=8192 + 4)])
def test_filter_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _filter_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_mask_filter_objects: "), err


def test_entries_launch_nothing_for_an_empty_scene():
    for kw in (dict(height=0), dict(width=0), dict(height=0, width=0)):
        for call in (_label_call, _filter_call):
            rc, err = call(**kw)
            assert rc == 0, err
        rc, err = _table_call(n=0, **kw)
        assert rc == 0, err
    rc, err = _table_call(n=0, null="area")                     # no object: nothing to write, nothing launched
    assert rc == 0, err


def test_wrappers_refuse_what_is_not_a_gpu_mask():
    bad = torch.zeros((4, 4), dtype=torch.uint8)                # on the host
    for call in (lambda: OB.label_components(bad), lambda: OB.filter_objects(bad, 4, 4), lambda: OB.match_objects(bad, bad),
                 lambda: OB.object_table(OB.Components(torch.zeros((4, 4), dtype=torch.int32), 0))):
        with pytest.raises(_lib.StcdError):
            call()


# ------------------------------------------------------------------------------------------------ refine_round's host logic
def _same_scores(a, b):
    np.testing.assert_equal(a, b)                               # equality that takes NaN (an empty class) as equal
    return True


def _hand_made_round(H=70, W=90, cell=32):
    rng = np.random.default_rng(3)
    cells_y, cells_x = ST.cell_grid(H, W, cell)
    pseudo = (rng.random((H, W)) < 0.45).astype(np.uint8) * np.uint8(255)
    n = cells_y * cells_x
    names = [f"s_{cy:04d}_{cx:04d}.png" for cy in range(cells_y) for cx in range(cells_x)]
    full = np.zeros((cells_y, cells_x), bool)
    full[:H // cell, :W // cell] = True
    masks = [torch.from_numpy((rng.random((H, W)) < 0.5).astype(np.uint8)) for _ in range(2)]
    return ST.SceneRound(masks, torch.from_numpy(pseudo), rng.integers(0, 9, (cells_y, cells_x, 1, 2, 2)), rng.random((cells_y, cells_x)),
                         rng.integers(0, 9, (cells_y, cells_x, 2, 2)), rng.integers(0, 99, (2, 2)), {"stale": 1.0}, names, full, names[:2], names[2:4], cell,
                         masks[0], masks[1])


class _SpecLaunches:
    """filter_objects and scene_cell_agree as the specification states them, on host tensors."""

    def __init__(self, monkeypatch):
        self.filter_calls = []
        monkeypatch.setattr(ST, "_check_mask", lambda *a, **k: None)
        monkeypatch.setattr(OB, "filter_objects", self.filter_objects)
        monkeypatch.setattr(ST, "scene_cell_agree", self.scene_cell_agree)

    def filter_objects(self, mask, min_area=0, max_hole=0, connectivity=8, mask_value=255, check=True):
        self.filter_calls.append((min_area, max_hole, connectivity, mask_value))
        return torch.from_numpy(SP.filter_objects(mask.numpy(), min_area, max_hole, connectivity, mask_value))

    def scene_cell_agree(self, masks, cell, label=None, agree=None, cm=None):
        _, got = RS.cell_agree([m.numpy() for m in masks], cell, label=label.numpy())
        return None, torch.from_numpy(np.asarray(got, np.int64))


def test_refine_round_replaces_the_pseudo_label_and_carries_the_rest(monkeypatch):
    fake = _SpecLaunches(monkeypatch)
    rnd = _hand_made_round()
    H, W = rnd.pseudo.shape
    label = (np.random.default_rng(4).random((H, W)) < 0.4).astype(np.uint8)
    label[5:9, 5:30] = 255
    out = ST.refine_round(rnd, min_area=6, max_hole=3, connectivity=4, label=label)
    assert fake.filter_calls == [(6, 3, 4, 255)]
    want = SP.filter_objects(rnd.pseudo.numpy(), 6, 3, 4, 255)
    assert np.array_equal(out.pseudo.numpy(), want) and not np.array_equal(want, rnd.pseudo.numpy())
    cells_y, cells_x = ST.cell_grid(H, W, rnd.cell)
    assert out.cell_cm.shape == (cells_y, cells_x, 2, 2) and np.array_equal(out.cm, out.cell_cm.sum(axis=(0, 1)))
    valid = label != 255
    cm = np.bincount(2 * (label[valid] != 0).astype(np.int64) + (want[valid] != 0), minlength=4).reshape(2, 2)
    assert np.array_equal(out.cm, cm) and _same_scores(out.scores, scores_from_cm(cm))
    for field in ("masks", "agree", "reliability", "names", "full", "reliable", "unreliable", "cell", "seg_a", "seg_b"):
        assert getattr(out, field) is getattr(rnd, field), field
    none = ST.refine_round(rnd, min_area=6)
    assert none.cell_cm is None and none.cm is None and none.scores is None and fake.filter_calls[-1] == (6, 0, 8, 255)


def test_refine_round_refuses_bad_arguments_before_any_launch(monkeypatch):
    fake = _SpecLaunches(monkeypatch)
    rnd = _hand_made_round()
    for kw in (dict(connectivity=6), dict(max_hole=-1), dict(label=np.zeros((3, 3), np.uint8)), dict(label=np.zeros(rnd.pseudo.shape, np.float32))):
        with pytest.raises(_lib.StcdError):
            ST.refine_round(rnd, **kw)
    with pytest.raises(_lib.StcdError):
        ST.refine_round("round")
    assert fake.filter_calls == []


@pytest.mark.gpu
def test_refine_round_launch_on_a_hand_made_round():
    rnd = _hand_made_round()
    dev = torch.device("cuda:0")
    on_dev = rnd._replace(pseudo=rnd.pseudo.to(dev))
    label = (np.random.default_rng(4).random(tuple(rnd.pseudo.shape)) < 0.4).astype(np.uint8)
    out = ST.refine_round(on_dev, min_area=6, max_hole=3, connectivity=4, label=label)
    want = SP.filter_objects(rnd.pseudo.numpy(), 6, 3, 4, 255)
    assert np.array_equal(out.pseudo.cpu().numpy(), want)
    cm = np.bincount(2 * (label != 0).astype(np.int64).ravel() + (want != 0).ravel(), minlength=4).reshape(2, 2)
    assert np.array_equal(out.cm, cm) and _same_scores(out.scores, scores_from_cm(cm))
    assert out.masks is rnd.masks and out.names is rnd.names and out.cell == rnd.cell
