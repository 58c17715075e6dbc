"""Convex hulls and oriented boxes, the part that needs no GPU: the specification of tests/hull_spec.py agrees with the index-interval
QuickHull the kernels run and has the invariants the rule set promises, it gives the pinned hull totals and boxes, box_shape and
boxes_to_geojson read the integer columns as documented, and the four C-ABI entries exist."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import hull_spec as HS
from tests import objects_spec as SP
from tests import rings_spec as RS
from tests import simplify_spec as SS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = OB.TILE


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, T), **RS.patterns(*shape), **SS.patterns(*shape)}


@functools.lru_cache(maxsize=None)
def traced(shape, name, conn):
    rs = RS.rings(SP.label(all_patterns(shape)[name], conn)[0], conn)
    for a in rs[:4]:
        a.setflags(write=False)
    return rs


@functools.lru_cache(maxsize=None)
def hulled(shape, name, conn):
    return HS.hulls(traced(shape, name, conn))


def ring_of(rs, r):
    return [tuple(v) for v in rs.vertices[rs.offsets[r]:rs.offsets[r + 1]].tolist()]


def is_subsequence(short, long):
    it = iter(long)
    return all(any(v == w for w in it) for v in short)


@pytest.mark.parametrize("shape,conn", [((37, 131), 8), ((65, 65), 8), ((65, 65), 4)], ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"c{v}")
def test_the_interval_scheme_equals_the_set_based_hull_and_the_invariants_hold(shape, conn):
    rings = 0
    for name in all_patterns(shape):
        rs, hs = traced(shape, name, conn), hulled(shape, name, conn)
        assert hs.count == rs.count and np.array_equal(hs.object, rs.object), name
        assert hs.offsets[0] == 0 and hs.offsets[-1] == hs.vertices.shape[0], name
        for r in range(rs.count):
            P, H = ring_of(rs, r), ring_of(hs, r)
            kept, rounds = HS.hull_ring(P), []
            assert HS.hull_ring_intervals(P, rounds) == kept and rounds[0] <= len(P), (name, r)
            assert H == [P[k] for k in kept] and is_subsequence(H, P), (name, r)
            sign = 1 if int(rs.area2[r]) > 0 else -1
            assert len(H) >= 4 and HS.is_strictly_convex(H, sign), (name, r)             # travelled in the input's direction
            assert int(hs.area2[r]) == SS.area2_of(H) and int(hs.area2[r]) * sign >= int(rs.area2[r]) * sign > 0, (name, r)
            assert all(P.count(v) == 1 for v in H), (name, r)                            # no pinch vertex is a hull vertex
            rings += 1
    assert rings > 2000


PINS = [((65, 65), 8, "disks", 54, 7), ((65, 65), 8, "rot_rects", 26, 3), ((65, 65), 4, "noise_0.593", 1072, 78),
        ((192, 192), 8, "disks", 45, None), ((192, 192), 8, "rot_rects", 77, None), ((192, 192), 8, "annulus", 144, 17),
        ((192, 192), 8, "comb", 6, None), ((192, 192), 8, "spiral", 4, None), ((192, 192), 8, "checkerboard", 72206, None)]


@pytest.mark.parametrize("shape,conn,name,vertices,edge_sum", PINS, ids=[f"{s[0]}x{s[1]}-c{c}-{n}" for s, c, n, _, _ in PINS])
def test_pinned_hull_totals_and_edge_sums(shape, conn, name, vertices, edge_sum):
    hs = hulled(shape, name, conn)
    assert hs.vertices.shape[0] == vertices
    if edge_sum is not None:
        assert int(HS.boxes(hs).edge.sum()) == edge_sum
    if name == "annulus":
        assert int(np.diff(hs.offsets).max()) == 72


@pytest.mark.parametrize("m,n,largest,edge,area,L,dmin,dmax,z", [(3, 32, 27, 2, 8281, 13, -39, 52, 91), (6, 96, 147, 10, 1164241, 61, -522, 557, 1079),
                                                                (12, 368, 1125, 43, 248157009, 221, -7778, 7975, 15753),
                                                                (24, 1440, 8745, 175, 57141555849, 841, -118806, 120237, 239043)])
def test_pinned_convex_rings_and_their_boxes(m, n, largest, edge, area, L, dmin, dmax, z):
    ring = list(HS.convex_ring(m))
    assert len(ring) == n and max(max(p) for p in ring) == largest and min(min(p) for p in ring) == 0
    assert SS.area2_of(ring) > 0 and HS.is_strictly_convex(ring, 1) and HS.hull_ring(ring) == list(range(n))
    got_edge, origin, e, extent = HS.box_of(ring)
    assert got_edge == edge and origin == ring[edge] and e[0] ** 2 + e[1] ** 2 == L
    assert extent[0] == dmin and extent[1] == dmax and abs(extent[2]) == z and extent[2] > 0 and (dmax - dmin) * z == area
    sub = ring[::7]                                             # any in-order subsequence is strictly convex
    assert HS.is_strictly_convex(sub, 1) and HS.hull_ring(sub) == list(range(len(sub)))
    if m <= 12:
        mid = list(HS.with_midpoints(tuple(ring)))
        assert len(mid) == 2 * n and HS.hull_ring(mid) == HS.hull_ring_intervals(mid) == list(range(0, 2 * n, 2))
        back = mid[:1] + mid[:0:-1]                             # a hole's direction, and another start
        assert HS.hull_ring(back) == HS.hull_ring_intervals(back)
        turned = mid[5:] + mid[:5]
        assert HS.hull_ring(turned) == HS.hull_ring_intervals(turned) == list(range(1, 2 * n, 2))


def test_degenerate_rings_in_the_spec():
    assert HS.hull_ring([]) == [] and HS.hull_ring([(1, 1)] * 5) == [0] and HS.hull_ring([(2, 2), (2, 9)]) == [0, 1]
    line = [(0, 0), (0, 3), (0, 6), (0, 3)]
    assert HS.hull_ring(line) == HS.hull_ring_intervals(line) == [0, 2]
    assert HS.hull_ring([(0, 0), (0, 5), (5, 5)]) == [0, 1, 2]
    rs = SS.ringset([[], [(1, 1)] * 5, [(2, 2), (2, 9)], line, [(0, 0), (0, 5), (5, 5)]])
    hs = HS.hulls(rs)
    assert np.diff(hs.offsets).tolist() == [0, 1, 2, 2, 3] and hs.area2.tolist() == [0, 0, 0, 0, 25]
    bs = HS.boxes(hs)
    assert bs.edge.tolist() == [-1, -1, -1, -1, 0] and not bs.extent[:4].any() and not bs.origin[:4].any() and not bs.dir[:4].any()


def boxed(ring_list):
    rs = SS.ringset(ring_list)
    hs = HS.hulls(rs)
    return rs, hs, HS.boxes(hs)


def test_box_shape_on_rectangles():
    upright = [(2, 3), (2, 10), (6, 10), (6, 3)]                # 4 high, 7 wide, an outer ring
    tilted = [(0, 4), (3, 0), (11, 6), (8, 10)]                 # sides (3, -4) and (8, 6): 5 by 10, along 3-4-5 directions
    assert SS.area2_of(upright) > 0 and SS.area2_of(tilted) < 0
    tilted = tilted[:1] + tilted[:0:-1]
    rs, hs, bs = boxed([upright, tilted, [(1, 1), (1, 7)]])
    shape = OB.box_shape(bs, rs, hs)
    assert sorted(map(tuple, shape["corners"][0].tolist())) == sorted((float(y), float(x)) for y, x in upright)
    assert shape["width"][0] == 7.0 and shape["height"][0] == 4.0 and shape["angle"][0] == 0.0 and shape["area"][0] == 28.0
    assert sorted((round(y, 9), round(x, 9)) for y, x in shape["corners"][1].tolist()) == sorted((float(y), float(x)) for y, x in tilted)
    e = bs.dir[1]
    along = math.hypot(*e.tolist())
    assert {along, 50.0 / along} == {5.0, 10.0}
    assert abs(shape["width"][1] - along) <= 1e-12 and abs(shape["height"][1] - 50.0 / along) <= 1e-12
    want = math.atan2(int(e[0]), int(e[1])) % math.pi
    assert abs(shape["angle"][1] - want) <= 1e-12 and 0.0 <= shape["angle"][1] < math.pi
    assert shape["rectangularity"][0] == 1.0 and shape["rectangularity"][1] == 1.0 and shape["solidity"][0] == 1.0
    assert all(np.isnan(v[2]).all() for v in shape.values())    # edge -1
    # a rectangle object traced from pixels
    m = np.zeros((12, 12), np.uint8); m[2:7, 3:11] = 1
    rs = RS.rings(SP.label(m, 8)[0], 8)
    hs = HS.hulls(rs)
    shape = OB.box_shape(HS.boxes(hs), rs, hs)
    assert shape["rectangularity"].tolist() == [1.0] and shape["solidity"].tolist() == [1.0] and shape["area"].tolist() == [40.0]
    with pytest.raises(_lib.StcdError):
        OB.box_shape(HS.boxes(hs), hulls=hs)


def test_solidity_of_the_notch():
    shape = (65, 65)
    rs, hs = traced(shape, "notch", 8), hulled(shape, "notch", 8)
    got = OB.box_shape(HS.boxes(hs), rs, hs)
    outer = rs.area2 > 0
    assert outer.any() and (got["solidity"][outer] < 1.0).all() and (got["solidity"] > 0.0).all()
    assert (got["rectangularity"][outer] <= got["solidity"][outer]).all()                # the box holds the hull


def signed_area(coords):
    return sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(coords[:-1], coords[1:]))


@pytest.mark.parametrize("transform", [None, (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0)], ids=["lattice", "north-up"])
@pytest.mark.parametrize("name", ["nested_rings", "annulus", "rot_rects"])
def test_boxes_to_geojson(name, transform, tmp_path):
    shape = (65, 65)
    rs, hs = traced(shape, name, 8), hulled(shape, name, 8)
    bs = HS.boxes(hs)
    path = str(tmp_path / "boxes.geojson")
    doc = OB.boxes_to_geojson(bs, rs, path=path, transform=transform, properties=OB.box_shape(bs, rs, hs))
    assert json.load(open(path)) == doc
    labels = sorted(set(rs.object.tolist()))
    assert (rs.area2 < 0).any() or name == "rot_rects"          # holes give no box
    assert [f["properties"]["label"] for f in doc["features"]] == labels
    for f in doc["features"]:
        (ring,) = f["geometry"]["coordinates"]
        assert len(ring) == 5 and ring[0] == ring[-1] and signed_area(ring) > 0
        assert {"angle", "width", "height", "rectangularity", "solidity"} <= set(f["properties"])
        assert abs(signed_area(ring) / 2 - f["properties"]["area"] * (1.0 if transform is None else 0.25)) <= 1e-6
    plain = OB.boxes_to_geojson(bs, rs, transform=transform)
    assert "solidity" not in plain["features"][0]["properties"] and "rectangularity" in plain["features"][0]["properties"]
    assert [f["geometry"] for f in plain["features"]] == [f["geometry"] for f in doc["features"]]


def test_the_mirrored_thresholds_and_the_abi_names():
    src = open(os.path.join(REPO, "stcd_amd", "csrc", "kernels_hull.hip")).read()
    for py, c in (("HULL_WAVE_MAX", "HL_WAVE_MAX"), ("HULL_LDS_MAX", "HL_LDS_MAX"), ("BOX_WAVE_MAX", "BX_WAVE_MAX"), ("BOX_LDS_MAX", "BX_LDS_MAX")):
        assert f"#define {c} {getattr(OB, py)} " in src, py
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("stcd_rings_hull_scratch_bytes", "stcd_rings_hull_count", "stcd_rings_hull_write", "stcd_rings_boxes"):
        assert hasattr(raw, name) and name in _lib.EXPORTS, name
    l = _lib.lib()
    assert l.stcd_rings_hull_scratch_bytes(3, 100) == 48 + 8 + 24 + 800 + 16 + 4 * 400 + 100 + 4    # header, sums, area, slots, list, 4 int arrays, keep, padding
    assert l.stcd_rings_hull_scratch_bytes(-1, 0) == 0 and l.stcd_rings_hull_scratch_bytes(0, 1 << 31) == 0
    # refused on the host before any HIP call
    assert l.stcd_rings_hull_count(None, None, 0, 0, None, None, 0, None) != 0 and l.stcd_last_error().decode().startswith("stcd_rings_hull_count: ")
    assert l.stcd_rings_hull_write(None, None, 0, 0, 0, None, None, None, None, 0, None) != 0 and l.stcd_last_error().decode().startswith("stcd_rings_hull_write: ")
    assert l.stcd_rings_boxes(None, None, 0, 0, None, None, None, None, None, None) != 0 and l.stcd_last_error().decode().startswith("stcd_rings_boxes: ")
