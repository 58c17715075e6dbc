"""Ring rasterization, the part that needs no GPU: the specification of tests/raster_spec.py equals an independent rational crossing
test, inverts tests/rings_spec.py, partitions split polygons, clips exactly and gives the pinned fidelity counts; geojson_to_rings
undoes rings_to_geojson; the mirrored thresholds are the kernels'; the two C-ABI entries exist and refuse bad arguments before any
HIP call.  Every assertion is integer equality."""
import ctypes as C
import functools
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import objects_spec as SP
from tests import raster_spec as RA
from tests import rings_spec as RS
from tests import simplify_spec as SS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = OB.TILE
ids = lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, T), **RS.patterns(*shape), **SS.patterns(*shape)}


def rings_of(rs):
    return RA.ring_list(rs)


# ------------------------------------------------------------------------------------------------ the specification itself
def fraction_winding(rings, H, W):
    """The winding number of every pixel centre, edge by edge and pixel by pixel with rationals: an edge counts for a centre iff the
    centre's row line crosses it and the crossing is not right of the centre."""
    w = np.zeros((H, W), np.int64)
    half = Fraction(1, 2)
    for ring in rings:
        n = len(ring)
        for k in range(n):
            (ya, xa), (yb, xb) = ring[k], ring[(k + 1) % n]
            if ya == yb:
                continue
            s = 1 if yb < ya else -1
            for i in range(H):
                cy = i + half
                if not min(ya, yb) < cy < max(ya, yb):
                    continue
                xc = xa + Fraction(xb - xa) * (cy - ya) / (yb - ya)
                for j in range(W):
                    if xc <= j + half:
                        w[i, j] += s
    return w


def random_ring_sets(count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        rings = [[(int(rng.integers(0, 12)), int(rng.integers(0, 12))) for _ in range(int(rng.integers(0, 8)))] for _ in range(int(rng.integers(1, 4)))]
        yield rings, int(rng.integers(1, 10)), int(rng.integers(1, 10))


def test_spec_equals_the_fraction_crossing_test():
    beyond = crossing = 0
    for rings, H, W in random_ring_sets(60, 7):
        want = fraction_winding(rings, H, W)
        assert np.array_equal(RA.winding(rings, H, W), want), (rings, H, W)
        assert np.array_equal(RA.fill(rings, H, W, "positive"), want > 0) and np.array_equal(RA.fill(rings, H, W, "evenodd"), (want & 1) == 1)
        beyond += any(y > H or x > W for ring in rings for y, x in ring)
        crossing += bool((np.abs(want) > 1).any() or (want < 0).any())
    assert beyond >= 20 and crossing >= 10                      # rings partly beyond the frame, and self-intersecting ones


def check_inverts(labels, conn, where):
    H, W = labels.shape
    rs = RS.rings(labels, conn)
    rings = rings_of(rs)
    w = RA.winding(rings, H, W)
    assert np.array_equal(w, (labels > 0).astype(np.int64)), where
    for rule in RA.RULES:
        assert np.array_equal(RA.fill(rings, H, W, rule), labels > 0), (where, rule)
    assert np.array_equal(RA.fill(rings, H, W, "evenodd"), RS.fill_even_odd(rings, H, W)), where
    obj = rs.object.tolist()
    for k in sorted(set(obj)):
        mine = [ring for ring, o in zip(rings, obj) if o == k]
        for rule in RA.RULES:
            assert np.array_equal(RA.fill(mine, H, W, rule), labels == k), (where, k, rule)
    assert set(obj) == set(np.unique(labels).tolist()) - {0}, where


@pytest.mark.parametrize("conn", [4, 8])
def test_spec_inverts_the_rings_of_random_masks(conn):
    rng = np.random.default_rng(11)
    for k in range(12):
        H, W = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        mask = (rng.random((H, W)) < (0.35, 0.5, 0.65)[k % 3]).astype(np.uint8)
        check_inverts(SP.label(mask, conn)[0], conn, ("random", k))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", [(37, 131), (65, 65)], ids=ids)
def test_spec_inverts_the_rings_of_the_patterns(shape, conn):
    for name, m in all_patterns(shape).items():
        check_inverts(SP.label(m, conn)[0], conn, name)


def star_polygon(rng, n, r):
    """n lattice vertices at evenly spaced angles round (r, r), radii in [r / 2, r]: star-shaped round the centre, counter-clockwise
    as the project counts it (area2 > 0)."""
    ring = []
    for k in range(n):
        a = 2 * math.pi * k / n
        d = r * (0.5 + 0.5 * float(rng.random()))
        ring.append((int(math.floor(r + d * math.sin(a) + 0.5)), int(math.floor(r + d * math.cos(a) + 0.5))))
    if SS.area2_of(ring) < 0:
        ring = ring[:1] + ring[:0:-1]
    return ring


def convex_polygon(rng, n, size):
    """The hull of n random lattice points (Andrew's monotone chain, collinear points dropped), area2 > 0."""
    pts = sorted({(int(rng.integers(0, size + 1)), int(rng.integers(0, size + 1))) for _ in range(n)})
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and cross(h[-2], h[-1], p) <= 0:
                h.pop()
            h.append(p)
        return h[:-1]

    ring = half(pts) + half(pts[::-1])
    return ring if SS.area2_of(ring) > 0 else ring[:1] + ring[:0:-1]


def check_partition(ring, a, b, H, W, via=()):
    """The two parts of ``ring`` cut from vertex a to vertex b (through the points ``via``, inside the ring) partition its pixels."""
    one, two = ring[a:b + 1] + list(via)[::-1], ring[b:] + ring[:a + 1] + list(via)
    whole = RA.winding([ring], H, W)
    w1, w2 = RA.winding([one], H, W), RA.winding([two], H, W)
    assert np.array_equal(w1 + w2, whole), (ring, a, b)         # the chord's two directions toggle the same column
    assert whole.min() >= 0 and whole.max() <= 1 and w1.min() >= 0 and w2.min() >= 0, (ring, a, b)
    for rule in RA.RULES:
        f1, f2, f = (RA.fill([p], H, W, rule) for p in (one, two, ring))
        assert not (f1 & f2).any() and np.array_equal(f1 | f2, f), (ring, a, b, rule)      # no gap, no double cover


def test_chord_split_polygons_partition_the_pixels():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n, r = int(rng.integers(5, 11)), int(rng.integers(6, 14))
        ring = star_polygon(rng, n, r)
        a = int(rng.integers(0, n - 2))
        b = int(rng.integers(a + 2, n if a else n - 1))
        check_partition(ring, a, b, 2 * r + 1, 2 * r + 1, via=[(r, r)])                    # a star's chord may leave it: cut through its centre
        hull = convex_polygon(rng, 9, 2 * r)
        if len(hull) >= 4:
            a = int(rng.integers(0, len(hull) - 2))
            check_partition(hull, a, int(rng.integers(a + 2, len(hull) if a else len(hull) - 1)), 2 * r, 2 * r)
    # an edge through pixel centres: the diagonal of a square passes through (i + 1/2, i + 1/2)
    square = [(0, 0), (0, 4), (4, 4), (4, 0)]
    assert SS.area2_of(square) > 0
    check_partition(square, 0, 2, 4, 4)
    check_partition(square, 1, 3, 4, 4)
    lower = RA.fill([[(0, 0), (4, 4), (4, 0)]], 4, 4)           # a centre ON the edge counts as right of it: the diagonal goes to the upper part
    assert lower.astype(int).tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0]]
    assert RA.fill([[(0, 0), (0, 4), (4, 4)]], 4, 4).astype(int).tolist() == [[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1]]
    check_partition([(0, 0), (0, 9), (6, 9), (6, 0)], 0, 2, 6, 9)                           # slope 2 / 3


def test_a_smaller_frame_is_the_crop():
    for rings, H, W in random_ring_sets(20, 21):
        big = RA.winding(rings, 12, 12)
        assert np.array_equal(RA.winding(rings, H, W), big[:H, :W]), (rings, H, W)
    rs = RS.rings(SP.label(all_patterns((37, 131))["rot_rects"], 8)[0], 8)
    simple = SS.simplify(rs, 9)
    big = RA.fill(simple, 37, 131)
    for H, W in ((1, 1), (20, 131), (37, 50), (11, 17)):
        assert np.array_equal(RA.fill(simple, H, W), big[:H, :W]), (H, W)
    assert np.array_equal(RA.fill(simple, 50, 140)[:37, :131], big) and not RA.fill(simple, 50, 140)[37:].any() and not RA.fill(simple, 50, 140)[:, 131:].any()


def test_degenerate_rings_fill_nothing():
    for ring in ([], [(2, 2)], [(1, 1), (5, 4)], [(0, 0), (3, 2), (6, 4), (3, 2)], [(1, 1), (6, 1), (1, 1), (6, 1)]):
        assert not RA.delta_plane([ring], 8, 8).any(), ring
    box = [(1, 1), (1, 5), (4, 5), (4, 1)]
    assert SS.area2_of(box) > 0
    w = RA.winding([box, box], 6, 7)
    assert w.max() == 2 and np.array_equal(w == 2, RA.fill([box], 6, 7))
    assert np.array_equal(RA.fill([box, box], 6, 7, "positive"), RA.fill([box], 6, 7)) and not RA.fill([box, box], 6, 7, "evenodd").any()
    hole = box[:1] + box[:0:-1]                                  # the same ring clockwise: winding -1
    assert RA.winding([hole], 6, 7).min() == -1 and not RA.fill([hole], 6, 7, "positive").any()
    assert np.array_equal(RA.fill([hole], 6, 7, "evenodd"), RA.fill([box], 6, 7))


# pixels where the raster of the simplified rings differs from labels > 0, at 96 x 96, connectivity 8, rule positive: (q = 4, 9, 16), object pixels
FIDELITY = {"rot_rects": ((85, 99, 107), 3183), "disks": ((120, 139, 246), 4494), "annulus": ((164, 156, 156), 4249)}


@pytest.mark.parametrize("name", sorted(FIDELITY))
def test_pinned_fidelity_counts(name):
    counts, pixels = FIDELITY[name]
    labels = SP.label(SS.patterns(96, 96)[name], 8)[0]
    assert int((labels > 0).sum()) == pixels
    rs = RS.rings(labels, 8)
    for q, want in zip((4, 9, 16), counts):
        w = RA.winding(SS.simplify(rs, q), 96, 96)
        assert w.min() >= 0 and w.max() <= 1, (name, q)
        assert int(((w > 0) != (labels > 0)).sum()) == want, (name, q)
    assert np.array_equal(RA.winding(SS.simplify(rs, 0), 96, 96) > 0, labels > 0)


def test_confusion():
    mask = np.array([[0, 255, 1, 0], [7, 0, 255, 255]], np.uint8)
    over = np.array([[0, 0, 3, 1], [255, 255, 1, 0]], np.uint8)
    assert RA.confusion(mask, over).tolist() == [[1, 2], [1, 2]]
    assert RA.confusion(mask, np.full_like(over, 255)).sum() == 0


# ------------------------------------------------------------------------------------------------ geojson_to_rings
def host_rings(rs):
    return OB.Rings(*(torch.from_numpy(np.ascontiguousarray(a)) for a in rs[:4]), int(rs.count))


def assert_same_rings(got, want, where):
    assert got.count == want.count, where
    assert got.vertices.dtype == torch.int32 and got.offsets.dtype == torch.int64 and got.object.dtype == torch.int32 and got.area2.dtype == torch.int64
    assert all(not t.is_cuda for t in got[:4]), where
    for a, b in zip(got[:4], want[:4]):
        assert tuple(a.shape) == tuple(np.asarray(b).shape) and np.array_equal(a.numpy(), np.asarray(b)), where


@pytest.mark.parametrize("transform", [None, (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0), (0.0, -2.0, 64.0, 2.0, 0.0, -8.0), (0.25, 0.5, -3.0, -0.5, 0.25, 7.0)],
                         ids=["none", "north_up", "quarter_turn", "sheared"])
def test_geojson_round_trip(transform, tmp_path):
    rs = RS.rings(SP.label(RS.patterns(37, 131)["nested"], 8)[0], 8)
    assert (rs.area2 < 0).sum() == 2 and rs.count == 4
    doc = OB.rings_to_geojson(rs, transform=transform)
    assert_same_rings(OB.geojson_to_rings(doc, transform=transform), rs, transform)
    assert_same_rings(OB.geojson_to_rings(doc["features"][0], transform=transform), RS.RingSet(rs.vertices[:8], rs.offsets[:3], rs.object[:2], rs.area2[:2], 2), "one feature")
    path = str(tmp_path / "nested.geojson")
    OB.rings_to_geojson(host_rings(rs), path=path, transform=transform)
    assert_same_rings(OB.geojson_to_rings(path, transform=transform), rs, "from a file")
    # every pattern's rings survive when each object's rings are stored together (document order is per object)
    for name in ("rings", "ring_island", "notch", "annulus"):
        rs = RS.rings(SP.label(all_patterns((37, 131))[name], 8)[0], 8)
        back = OB.geojson_to_rings(OB.rings_to_geojson(rs, transform=transform), transform=transform)
        assert sorted(RA.ring_list(back)) == sorted(RA.ring_list(rs)), name
        assert np.array_equal(RA.fill(back, 37, 131), RA.fill(rs, 37, 131)), name


def test_geojson_geometries_and_rounding():
    outer = [[0, 0], [6, 0], [6, 5], [0, 5], [0, 0]]            # [x, y]: east then south on the lattice, the travel order of an outer ring
    hole = [[2, 1], [2, 3], [4, 3], [4, 1], [2, 1]]
    poly = {"type": "Polygon", "coordinates": [outer, hole]}
    got = OB.geojson_to_rings(poly)
    assert got.count == 2 and got.offsets.tolist() == [0, 4, 8] and got.object.tolist() == [1, 1] and got.area2.tolist() == [60, -8]
    assert got.vertices.tolist() == [[0, 0], [0, 6], [5, 6], [5, 0], [1, 2], [3, 2], [3, 4], [1, 4]]
    assert np.array_equal(RA.fill(got, 5, 6).astype(int), np.array([[1] * 6, [1, 1, 0, 0, 1, 1], [1, 1, 0, 0, 1, 1], [1] * 6, [1] * 6]))
    # the roles decide, not the stored direction: a ring of the wrong sign is reversed with its first vertex kept first
    flipped = OB.geojson_to_rings({"type": "Polygon", "coordinates": [outer[::-1], hole[::-1]]})
    assert flipped.area2.tolist() == [60, -8] and flipped.vertices.tolist() == got.vertices.tolist()
    # MultiPolygon: its polygons share the feature's object; labels are used when every feature has one
    multi = {"type": "MultiPolygon", "coordinates": [[outer, hole], [[[10, 10], [12, 10], [12, 13], [10, 13], [10, 10]]]]}
    got = OB.geojson_to_rings(multi)
    assert got.count == 3 and got.object.tolist() == [1, 1, 1] and got.area2.tolist() == [60, -8, 12]
    fc = {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"label": 7}, "geometry": multi},
                                                    {"type": "Feature", "properties": {"label": 3}, "geometry": poly}]}
    assert OB.geojson_to_rings(fc).object.tolist() == [7, 7, 7, 3, 3]
    fc["features"][1]["properties"] = {"label": 0}
    assert OB.geojson_to_rings(fc).object.tolist() == [1, 1, 1, 2, 2]
    fc["features"][1]["properties"] = None
    assert OB.geojson_to_rings(json.loads(json.dumps(fc))).object.tolist() == [1, 1, 1, 2, 2]
    assert OB.geojson_to_rings({"type": "FeatureCollection", "features": []}).count == 0
    # the closing vertex is dropped, and only a repeated one
    assert OB.geojson_to_rings({"type": "Polygon", "coordinates": [outer[:-1]]}).vertices.tolist() == OB.geojson_to_rings(poly).vertices.tolist()[:4]
    # floor(v + 1/2): 0.5 -> 1, 2.5 -> 3 (not to even), 2.49 -> 2, -0.5 -> 0
    got = OB.geojson_to_rings({"type": "Polygon", "coordinates": [[[-0.5, -0.4], [2.5, 0.49], [2.49, 4.5], [0.5, 3.5]]]})
    assert sorted(got.vertices.tolist()) == sorted([[0, 0], [0, 3], [5, 2], [4, 1]])
    # zero-area rings are dropped, after rounding
    thin = {"type": "Polygon", "coordinates": [outer, [[1, 1], [3, 1.2], [5, 1.4], [1, 1]], [[2, 2], [2, 2], [2, 2], [2, 2]]]}
    assert OB.geojson_to_rings(thin).area2.tolist() == [60]
    assert OB.geojson_to_rings({"type": "Polygon", "coordinates": [[[1, 1], [4, 1], [1, 1]]]}).count == 0
    # the largest coordinate is fine
    assert OB.geojson_to_rings({"type": "Polygon", "coordinates": [[[0, 0], [16384.4, 0], [16384, 16384.49]]]}).vertices.max().item() == 16384


@pytest.mark.parametrize("doc,transform", [
    ({"type": "LineString", "coordinates": [[0, 0], [1, 1]]}, None),
    ({"type": "Feature", "properties": {}, "geometry": {"type": "Point", "coordinates": [0, 0]}}, None),
    ({"type": "Feature", "properties": {}, "geometry": None}, None),
    ({"type": "FeatureCollection"}, None),
    ({"coordinates": []}, None),
    ({"type": "Polygon", "coordinates": [[[0, 0], [16384.5, 0], [5, 5]]]}, None),
    ({"type": "Polygon", "coordinates": [[[0, 0], [-0.51, 0], [5, 5]]]}, None),
    ({"type": "Polygon", "coordinates": [[[0, 0], [float("nan"), 0], [5, 5]]]}, None),
    ({"type": "Polygon", "coordinates": [[[0, 0], [3], [5, 5]]]}, None),
    ({"type": "Polygon", "coordinates": [[[0, 0], [3, 0], [5, 5]]]}, (1.0, 2.0, 0.0, 2.0, 4.0, 0.0)),
    ({"type": "Polygon", "coordinates": [[[0, 0], [3, 0], [5, 5]]]}, (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
    ({"type": "Polygon", "coordinates": [[[0, 0], [3, 0], [5, 5]]]}, (1.0, 0.0, 0.0)),
    ({"type": "Polygon", "coordinates": [[[0, 0], [3, 0], [5, 5]]]}, (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0)),        # lands below 0
])
def test_geojson_refusals(doc, transform):
    with pytest.raises(_lib.StcdError, match="geojson_to_rings"):
        OB.geojson_to_rings(doc, transform=transform)


# ------------------------------------------------------------------------------------------------ the C entries' argument checks
def test_thresholds_mirror_the_kernels():
    text = open(os.path.join(REPO, "stcd_amd", "csrc", "kernels_raster.hip")).read()
    assert int(re.search(r"#define RS_SPAN_MAX (\d+)", text).group(1)) == OB.RASTER_SPAN_MAX
    assert int(re.search(r"#define RS_ROW_CHUNK (\d+)", text).group(1)) == OB.RASTER_ROW_CHUNK
    assert int(re.search(r"#define RS_COORD_MAX (\d+)", text).group(1)) == RA.COORD_MAX
    assert OB.RASTER_SPAN_MAX >= 1 and OB.RASTER_ROW_CHUNK % 64 == 0


def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    declared = set(re.findall(r"\b(stcd_[a-z0-9_]+)\s*\(", hdr))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("stcd_rings_raster_scratch_bytes", "stcd_rings_raster"):
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name)
    assert _lib.lib().stcd_abi_version() == 2                   # additions only
    assert OB.Raster._fields == ("mask", "cm")


def _bytes(height=5, width=9):
    return int(_lib.lib().stcd_rings_raster_scratch_bytes(height, width))


def test_scratch_bytes():
    for H, W in ((1, 1), (5, 9), (3, 1024), (4096, 4096), (16384, 16384)):
        assert _bytes(H, W) == (16 + 4 * H * (W + 1) + 7) // 8 * 8, (H, W)
    for H, W in ((0, 4), (4, 0), (-1, 4), (4, -1), (16385, 4), (4, 16385)):
        assert _bytes(H, W) == 0, (H, W)


def _call(rings=3, verts=20, height=5, width=9, rule=0, mask_value=255, null=None, short=0, odd=None, overlay=False, cm=False):
    """HOST buffers: every call here is refused before any HIP call."""
    buf = np.zeros(65536, np.int64)
    base = buf.ctypes.data
    p = lambda name, off: None if null == name else C.c_void_p(base + off + (4 if odd == name else 0))
    rc = _lib.lib().stcd_rings_raster(p("vertices", 0), p("offsets", 1024), rings, verts, height, width, rule, mask_value,
                                      p("overlay", 2048) if overlay else None, p("cm", 3072) if cm else None, p("mask", 4096), p("scratch", 8192),
                                      max(_bytes(height, width), 8) - short, None)
    assert not buf.any()
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(null="vertices"), dict(null="offsets"), dict(null="mask"), dict(null="scratch"), dict(overlay=True), dict(cm=True),
                                dict(rings=-1), dict(verts=-1), dict(rings=1 << 31), dict(verts=1 << 31), dict(height=0), dict(width=0), dict(height=16385),
                                dict(width=16385), dict(height=-3), dict(rule=2), dict(rule=-1), dict(mask_value=0), dict(mask_value=256),
                                dict(odd="offsets"), dict(odd="scratch"), dict(odd="cm", overlay=True, cm=True), dict(short=8), dict(short=1)],
                         ids=lambda kw: "-".join(f"{k}_{v}" for k, v in kw.items()))
def test_raster_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_rings_raster: "), err


def test_wrapper_refuses_what_is_not_on_the_gpu():
    rs = SS.ringset([SS.staircase(8)])
    with pytest.raises(_lib.StcdError):
        OB.rasterize_rings(host_rings(rs), (16, 16))
    with pytest.raises(_lib.StcdError):
        OB.rasterize_rings(rs, (16, 16))                        # numpy arrays
    with pytest.raises(_lib.StcdError):
        OB.rasterize_rings(OB.geojson_to_rings({"type": "Polygon", "coordinates": [[[0, 0], [4, 0], [4, 4]]]}), (8, 8))     # CPU tensors
