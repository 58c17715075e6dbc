"""Change polygons, the part that needs no GPU: the specification of tests/rings_spec.py obeys the facts that pin it from outside
(scipy.ndimage.label's hole count, areas, the even-odd fill; the ring counts pin the saddle rule), rings_to_geojson builds what it
documents from the specification's arrays, and the three C-ABI entries exist and refuse bad arguments before any HIP call."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import objects_spec as SP
from tests import rings_spec as RS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = OB.TILE
SHAPES = [(1, 1), (1, T + 3), (T + 3, 1), (T + 1, T + 1), (37, 131)]
ids = lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def random_masks():
    rng = np.random.default_rng(2024)
    out = []
    for _ in range(60):
        H, W = (int(v) for v in rng.integers(1, 14, 2))
        out.append((rng.random((H, W)) < rng.choice([0.3, 0.5, 0.7])).astype(np.uint8))
    return out


def all_patterns(H, W):
    return {**SP.patterns(H, W, T), **RS.patterns(H, W)}


def ring_list(rs, r):
    return rs.vertices[rs.offsets[r]:rs.offsets[r + 1]]


def check_facts(mask, conn, ndi):
    """The facts of a mask's rings when labels and rings use the same connectivity."""
    lab, n = SP.label(mask, conn)
    rs = RS.rings(lab, conn)
    H, W = lab.shape
    assert rs.count == rs.object.shape[0] == rs.area2.shape[0] == rs.offsets.shape[0] - 1 and rs.offsets[0] == 0 and rs.offsets[-1] == rs.vertices.shape[0]
    assert rs.vertices.dtype == np.int32 and rs.offsets.dtype == np.int64 and rs.object.dtype == np.int32 and rs.area2.dtype == np.int64
    starts = []
    for r in range(rs.count):
        ring = ring_list(rs, r)
        assert ring.shape[0] >= 4 and ring.shape[0] % 2 == 0
        step = (ring[1] - ring[0]).tolist()
        assert rs.area2[r] != 0
        # the start edge is a corner: it runs east on an outer ring and south on a hole
        assert (step[0] == 0 and step[1] > 0) if rs.area2[r] > 0 else (step[0] > 0 and step[1] == 0), (r, step)
        assert not (np.diff(np.vstack([ring, ring[:1]]), axis=0) != 0).all(axis=1).any()               # axis-parallel sides only
        assert tuple(ring[0]) == tuple(ring[np.lexsort((ring[:, 1], ring[:, 0]))[0]])                  # the start is the ring's first vertex in raster order
        starts.append(tuple(ring[0]))
    assert starts == sorted(starts)
    pos = rs.area2 > 0
    assert int(pos.sum()) == n and np.array_equal(rs.object[pos], np.arange(1, n + 1))
    # holes: the components of unset pixels, under the complementary connectivity, that touch no border
    structure = np.ones((3, 3), bool) if conn == 4 else ndi.generate_binary_structure(2, 1)
    unset, n_unset = ndi.label(lab == 0, structure=structure)
    edge = set(unset[0].tolist()) | set(unset[-1].tolist()) | set(unset[:, 0].tolist()) | set(unset[:, -1].tolist())
    assert int((~pos).sum()) == n_unset - len(edge - {0})
    for k in range(1, n + 1):
        sel = np.nonzero(rs.object == k)[0]
        assert int(rs.area2[sel].sum()) == 2 * int((lab == k).sum())
        assert np.array_equal(RS.fill_even_odd([ring_list(rs, r) for r in sel], H, W), lab == k)
    return rs


# ------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize("conn", [4, 8])
def test_spec_facts_on_random_masks(conn):
    ndi = pytest.importorskip("scipy.ndimage")
    for m in random_masks():
        check_facts(m, conn, ndi)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_spec_facts_on_the_patterns(shape, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    for name, m in all_patterns(*shape).items():
        check_facts(m, conn, ndi)


def test_spec_known_rings():
    one = RS.rings(np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.int32), 8)
    assert one.count == 1 and one.vertices.tolist() == [[1, 1], [1, 2], [2, 2], [2, 1]] and one.area2.tolist() == [2] and one.object.tolist() == [1]
    # a saddle: one ring of 8 corners under 8 (the labels are one object), two squares under 4
    diag = np.array([[1, 0], [0, 1]], np.uint8)
    r8 = RS.rings(SP.label(diag, 8)[0], 8)
    assert r8.count == 1 and r8.vertices.tolist() == [[0, 0], [0, 1], [1, 1], [1, 2], [2, 2], [2, 1], [1, 1], [1, 0]] and r8.area2.tolist() == [4]
    r4 = RS.rings(SP.label(diag, 4)[0], 4)
    assert r4.count == 2 and r4.offsets.tolist() == [0, 4, 8] and r4.object.tolist() == [1, 2]
    # mismatched: one label, connectivity 4 -> the object has two outer rings; two labels, connectivity 8 -> never crosses to another label
    m48 = RS.rings(SP.label(diag, 8)[0], 4)
    assert m48.count == 2 and m48.object.tolist() == [1, 1] and (m48.area2 > 0).all()
    m84 = RS.rings(SP.label(diag, 4)[0], 8)
    assert m84.count == 2 and m84.object.tolist() == [1, 2] and np.array_equal(m84.vertices, r4.vertices)
    # the anti-diagonal under 8: a hole of the complement never appears, the ring passes the saddle vertex twice
    anti = RS.rings(SP.label(diag[::-1], 8)[0], 8)
    assert anti.count == 1 and anti.offsets.tolist() == [0, 8] and anti.vertices[0].tolist() == [0, 1]
    ring = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]], np.uint8)
    rr = RS.rings(SP.label(ring, 4)[0], 4)
    assert rr.count == 2 and rr.area2.tolist() == [18, -2] and rr.vertices[4:].tolist() == [[1, 1], [2, 1], [2, 2], [1, 2]]
    empty = RS.rings(np.zeros((3, 4), np.int32), 8)
    assert empty.count == 0 and empty.vertices.shape == (0, 2) and empty.offsets.tolist() == [0]


def test_spec_nested_and_comb():
    nested = RS.patterns(40, 50)["nested"]
    for conn in (4, 8):
        lab, n = SP.label(nested, conn)
        rs = RS.rings(lab, conn)
        assert n == 2 and rs.count == 4 and rs.object.tolist() == [1, 1, 2, 2] and (np.sign(rs.area2) == [1, -1, 1, -1]).all()
        comb = RS.patterns(192, 192)["comb"]
        lab, n = SP.label(comb, conn)
        rs = RS.rings(lab, conn)
        assert n == 1 and rs.count == 1 and rs.offsets.tolist() == [0, 24578]


# ------------------------------------------------------------------------------------------------ rings_to_geojson
def _shoelace2(coords):
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(coords[:-1], coords[1:]))


def _case():
    m = np.zeros((12, 14), np.uint8)
    m[1:8, 1:9] = 1; m[3:6, 3:7] = 0; m[4, 4] = 1               # a box, its hole, an island in the hole
    m[9:11, 10:13] = 1
    m[2, 2] = 0                                                 # a second hole of the box
    lab, n = SP.label(m, 8)
    return lab, n, RS.rings(lab, 8)


def test_geojson_structure_and_holes():
    lab, n, rs = _case()
    fc = OB.rings_to_geojson(rs)
    assert fc["type"] == "FeatureCollection" and len(fc["features"]) == n == 3
    for k, feat in enumerate(fc["features"], 1):
        assert feat["type"] == "Feature" and feat["geometry"]["type"] == "Polygon" and feat["properties"] == {"label": k}
        sel = np.nonzero(rs.object == k)[0]
        coords = feat["geometry"]["coordinates"]
        assert len(coords) == len(sel)
        want_order = [r for r in sel if rs.area2[r] > 0] + [r for r in sel if rs.area2[r] < 0]
        for got, r in zip(coords, want_order):
            ring = ring_list(rs, r)
            assert got[0] == got[-1] and len(got) == ring.shape[0] + 1                     # closed by repeating the first vertex
            assert got[:-1] == [[int(x), int(y)] for y, x in ring.tolist()]                # [x, y], stored order
            assert _shoelace2(got) == rs.area2[r]
        assert _shoelace2(coords[0]) > 0 and all(_shoelace2(c) < 0 for c in coords[1:])
    assert len(fc["features"][0]["geometry"]["coordinates"]) == 3 and len(fc["features"][1]["geometry"]["coordinates"]) == 1
    # numpy arrays, CPU tensors and a plain tuple of them give the same document
    as_tensors = OB.Rings(*(torch.from_numpy(np.ascontiguousarray(a)) for a in rs[:4]), rs.count)
    assert OB.rings_to_geojson(as_tensors) == fc
    assert OB.rings_to_geojson(RS.rings(np.zeros((3, 3), np.int32), 8)) == {"type": "FeatureCollection", "features": []}


def test_geojson_transform_and_orientation():
    lab, n, rs = _case()
    H = lab.shape[0]
    plain = OB.rings_to_geojson(rs)
    # a north-up geotransform: 0.5 m pixels, the origin at the scene's top-left corner
    tr = (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0)
    fc = OB.rings_to_geojson(rs, transform=tr)
    for f0, f1 in zip(plain["features"], fc["features"]):
        for c0, c1 in zip(f0["geometry"]["coordinates"], f1["geometry"]["coordinates"]):
            mapped = [[0.5 * x + 1000.0, -0.5 * y + 2000.0] for x, y in c0]
            assert c1[0] == c1[-1] == mapped[0] and c1[1:-1] == mapped[1:-1][::-1]         # mirrored: reverse travel order, same first vertex
            assert _shoelace2(c1) == 0.25 * _shoelace2(c0)
        rings = f1["geometry"]["coordinates"]
        assert _shoelace2(rings[0]) > 0 and all(_shoelace2(c) < 0 for c in rings[1:])       # RFC 7946: exterior counter-clockwise
    # a transform that does not mirror keeps the order; shear and offsets are applied as documented
    tr = (2.0, 1.0, 3.0, 0.5, 4.0, -7.0)
    fc = OB.rings_to_geojson(rs, transform=tr)
    c0, c1 = plain["features"][0]["geometry"]["coordinates"][0], fc["features"][0]["geometry"]["coordinates"][0]
    assert c1 == [[2.0 * x + 1.0 * y + 3.0, 0.5 * x + 4.0 * y - 7.0] for x, y in c0] and _shoelace2(c1) > 0


def test_geojson_properties_and_file(tmp_path):
    lab, n, rs = _case()
    overlay = (np.random.default_rng(1).random(lab.shape) < 0.5).astype(np.uint8)
    area, bbox, overlap = SP.table(lab, n, overlay)
    table = OB.ObjectTable(torch.from_numpy(area), torch.from_numpy(bbox), torch.from_numpy(overlap))
    path = tmp_path / "objects.geojson"
    fc = OB.rings_to_geojson(rs, path=str(path), properties=table)
    for k, feat in enumerate(fc["features"], 1):
        assert feat["properties"] == {"label": k, "area": int(area[k - 1]), "bbox": bbox[k - 1].tolist(), "overlap": overlap[k - 1].tolist()}
        assert sum(_shoelace2(c) for c in feat["geometry"]["coordinates"]) == 2 * feat["properties"]["area"]
    assert json.loads(path.read_text()) == fc
    bare = OB.rings_to_geojson(rs, properties=OB.ObjectTable(area, bbox, None))
    assert set(bare["features"][0]["properties"]) == {"label", "area", "bbox"}
    with pytest.raises(_lib.StcdError):
        OB.rings_to_geojson(rs, properties=OB.ObjectTable(area[:1], bbox[:1], None))


def test_geojson_refuses_an_object_with_two_outer_rings():
    diag = np.array([[1, 0], [0, 1]], np.uint8)
    rs = RS.rings(SP.label(diag, 8)[0], 4)                      # labels made with 8, rings asked with 4
    with pytest.raises(_lib.StcdError, match="more than one outer ring"):
        OB.rings_to_geojson(rs)
    with pytest.raises(_lib.StcdError):
        OB.rings_to_geojson(rs._replace(count=1))               # fields that do not fit together


# ------------------------------------------------------------------------------------------------ the C entries' argument checks
def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    declared = set(re.findall(r"\b(stcd_[a-z0-9_]+)\s*\(", hdr))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("stcd_rings_scratch_bytes", "stcd_rings_count", "stcd_rings_write"):
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name)
    assert _lib.lib().stcd_abi_version() == 2                   # additions only


def _bytes(h=10, w=12, cap=64):
    return int(_lib.lib().stcd_rings_scratch_bytes(h, w, cap))


def test_scratch_bytes_per_pixel_and_per_corner():
    assert _bytes(10, 12, 0) >= 32 + 4 * 11 * 13 and _bytes(10, 12, 0) % 8 == 0
    assert 37 * 1000 <= _bytes(10, 12, 1000) - _bytes(10, 12, 0) <= 37 * 1000 + 64
    assert 4 * 4097 * 4097 <= _bytes(4096, 4096, 0) <= 4.1 * 4097 * 4097
    assert _bytes(-1, 4) == 0 and _bytes(4, -1) == 0 and _bytes(1 << 16, 1 << 15) == 0 and _bytes(4, 4, -1) == 0 and _bytes(4, 4, 1 << 31) == 0
    assert _bytes(46340, 46340, 8) > 0                          # the largest square below 2^31 pixels


def _host():
    """HOST buffers: every call here is refused (or has nothing to launch) before any HIP call."""
    buf = np.zeros(65536, np.int64)
    return buf, buf.ctypes.data


def _count_call(height=10, width=12, connectivity=8, cap=64, null=None, short=0, odd=0):
    buf, base = _host()
    p = lambda name, off: None if null == name else C.c_void_p(base + off)
    rc = _lib.lib().stcd_rings_count(p("labels", 0), height, width, connectivity, cap, p("counts", 4096 + odd), p("scratch", 8192),
                                     max(_bytes(height, width, cap), 8) - short, None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(null="labels"), dict(null="counts"), dict(null="scratch"), dict(height=-1), dict(width=-1),
                                dict(height=1 << 16, width=1 << 15), dict(height=46341, width=46341), dict(connectivity=6), dict(connectivity=0),
                                dict(cap=-1), dict(cap=1 << 31), dict(short=8), dict(odd=4)])
def test_count_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _count_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_rings_count: "), err


def _write_call(height=10, width=12, connectivity=8, cap=64, rings=2, verts=12, null=None, short=0):
    buf, base = _host()
    p = lambda name, off: None if null == name else C.c_void_p(base + off)
    rc = _lib.lib().stcd_rings_write(p("labels", 0), height, width, connectivity, cap, rings, verts, p("vertices", 1024), p("offsets", 2048),
                                     p("object", 3072), p("area2", 4096), p("scratch", 8192), max(_bytes(height, width, cap), 8) - short, None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(null="labels"), dict(null="vertices"), dict(null="offsets"), dict(null="object"), dict(null="area2"),
                                dict(null="scratch"), dict(height=-1), dict(width=-1), dict(height=1 << 16, width=1 << 15), dict(connectivity=5),
                                dict(cap=-1), dict(short=8),
                                # an (R, V) pair that no count phase leaves
                                dict(rings=-1), dict(verts=-2), dict(rings=2, verts=6), dict(rings=1, verts=5), dict(rings=0, verts=4),
                                dict(rings=1, verts=0), dict(rings=2, verts=66), dict(height=1, width=1, rings=2, verts=18, cap=64)])
def test_write_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _write_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_rings_write: "), err


def test_entries_launch_nothing_for_an_empty_scene():
    for kw in (dict(height=0), dict(width=0), dict(height=0, width=0)):
        rc, err = _count_call(**kw)
        assert rc == 0, err
        rc, err = _write_call(rings=0, verts=0, **kw)
        assert rc == 0, err


def test_wrapper_refuses_what_is_not_a_gpu_label_image():
    for bad in (OB.Components(torch.zeros((4, 4), dtype=torch.int32), 1), OB.Components(torch.zeros((4, 4), dtype=torch.uint8), 1)):
        with pytest.raises(_lib.StcdError):
            OB.object_rings(bad)
