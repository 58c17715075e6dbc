"""Convex hulls and oriented boxes on the GPU: convex_hulls and oriented_boxes against the plain-Python specification of
tests/hull_spec.py, ring and hull lengths at the thresholds between the kernels' paths, orientation and start, degenerate rings, the
invariants that hold without the specification, reuse and the refusals.  Every output is an integer and every assertion on device
output is equality.  192 x 192 carries the comb (one ring of 24 578 vertices: the path whose state lives in global memory), the
spiral and the checkerboard (18 051 rings, most of 4 vertices)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import hull_spec as HS
from tests import objects_spec as SP
from tests import rings_spec as RS
from tests import simplify_spec as SS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = OB.TILE
WAVE, LDS, BWAVE, BLDS = OB.HULL_WAVE_MAX, OB.HULL_LDS_MAX, OB.BOX_WAVE_MAX, OB.BOX_LDS_MAX


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)               # a copy: the shared references are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, T), **RS.patterns(*shape), **SS.patterns(*shape)}


# the references: computed once per (shape, pattern, connectivity), shared by the tests and never written to
@functools.lru_cache(maxsize=None)
def want_label(shape, name, conn):
    lab, n = SP.label(all_patterns(shape)[name], conn)
    lab.setflags(write=False)
    return lab, n


@functools.lru_cache(maxsize=None)
def want_rings(shape, name, conn):
    rs = RS.rings(want_label(shape, name, conn)[0], conn)
    for a in rs[:4]:
        a.setflags(write=False)
    return rs


@functools.lru_cache(maxsize=None)
def want_hulls(shape, name, conn):
    hs = HS.hulls(want_rings(shape, name, conn))
    bs = HS.boxes(hs)
    for a in hs[:4] + bs[:4]:
        a.setflags(write=False)
    return hs, bs


@functools.lru_cache(maxsize=None)
def device_rings(shape, name, conn):
    """object_rings' result on the device; the tests clone nothing and must not write to it."""
    lab, n = want_label(shape, name, conn)
    got = OB.object_rings(OB.Components(dev(lab), n), conn)
    assert_equals_spec(got, want_rings(shape, name, conn), ("object_rings", name))
    return got


def as_rings(rs) -> OB.Rings:
    return OB.Rings(dev(rs.vertices), dev(rs.offsets), dev(rs.object), dev(rs.area2), int(rs.count))


def assert_equals_spec(got: OB.Rings, want: RS.RingSet, where):
    assert got.count == want.count, (where, got.count, want.count)
    assert got.vertices.dtype == torch.int32 and got.offsets.dtype == torch.int64 and got.object.dtype == torch.int32 and got.area2.dtype == torch.int64, where
    assert tuple(got.vertices.shape) == want.vertices.shape and tuple(got.offsets.shape) == want.offsets.shape, (where, tuple(got.vertices.shape), want.vertices.shape)
    assert all(t.device == DEV for t in got[:4]), where
    assert np.array_equal(host(got.offsets), want.offsets), where
    assert np.array_equal(host(got.object), want.object), where
    assert np.array_equal(host(got.area2), want.area2), where
    assert np.array_equal(host(got.vertices), want.vertices), where


def assert_boxes_equal(got: OB.OrientedBoxes, want: HS.BoxSet, where):
    assert got.count == want.count, (where, got.count, want.count)
    assert got.edge.dtype == torch.int32 and got.origin.dtype == torch.int32 and got.dir.dtype == torch.int32 and got.extent.dtype == torch.int64, where
    assert all(t.device == DEV for t in got[:4]), where
    for name in ("edge", "origin", "dir", "extent"):
        g, w = host(getattr(got, name)), getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w), (where, name, np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else g.shape)


def assert_hulls_and_boxes(rs, where, d=None):
    """convex_hulls and oriented_boxes of the RingSet ``rs`` equal the specification; returns the device results."""
    hs = HS.hulls(rs)
    got = OB.convex_hulls(as_rings(rs) if d is None else d)
    assert_equals_spec(got, hs, where)
    boxes = OB.oriented_boxes(got)
    assert_boxes_equal(boxes, HS.boxes(hs), where)
    return got, boxes


CASES = [(shape, conn, name) for shape, conn in (((37, 131), 8), ((65, 65), 8), ((65, 65), 4), ((192, 192), 8)) for name in all_patterns(shape)]


@pytest.mark.parametrize("shape,conn,name", CASES, ids=[f"{s[0]}x{s[1]}-c{c}-{n}" for s, c, n in CASES])
def test_device_equals_the_spec(shape, conn, name):
    hs, bs = want_hulls(shape, name, conn)
    got = OB.convex_hulls(device_rings(shape, name, conn))
    assert_equals_spec(got, hs, name)
    assert_boxes_equal(OB.oriented_boxes(got), bs, name)
    assert_boxes_equal(OB.oriented_boxes(got, check=False), bs, name)


def test_the_long_and_the_many():
    """What the 192 x 192 cases above run through."""
    shape = (192, 192)
    comb, board = (want_rings(shape, name, 8) for name in ("comb", "checkerboard"))
    assert comb.count == 1 and comb.vertices.shape[0] == 24578 > LDS
    assert board.count == 18051 and int((np.diff(board.offsets) == 4).sum()) >= 18000
    assert int(np.diff(want_hulls(shape, "annulus", 8)[0].offsets).max()) == 72 > BWAVE


def mixed(ring, reverse):
    """``ring`` three times in a ring set with short rings between, stored or in reverse ring order."""
    rings = [ring, SS.staircase(4, 1), ring, SS.staircase(4, 3), SS.staircase(6, 4), ring, SS.staircase(4, 6)]
    objects = list(range(1, len(rings) + 1))
    if reverse:
        rings, objects = rings[::-1], objects[::-1]
    return SS.ringset(rings, objects)


@pytest.mark.parametrize("reverse", [False, True], ids=["stored", "reversed"])
@pytest.mark.parametrize("n", [4, 6, WAVE - 2, WAVE, WAVE + 2, LDS - 2, LDS, LDS + 2])
def test_ring_lengths_at_the_hull_thresholds(n, reverse):
    rs = mixed(SS.staircase(n, 0), reverse)
    got, _ = assert_hulls_and_boxes(rs, (n, reverse))
    assert got.vertices.shape[0] < rs.vertices.shape[0] or n <= 4


@functools.lru_cache(maxsize=None)
def hull_of_size(h):
    ring = HS.convex_ring(24)
    return tuple(ring[k * len(ring) // h] for k in range(h))


@pytest.mark.parametrize("reverse", [False, True], ids=["stored", "reversed"])
@pytest.mark.parametrize("h", [3, 4, BWAVE - 1, BWAVE, BWAVE + 1, BLDS - 1, BLDS, BLDS + 1, 1440])
def test_hull_sizes_at_the_box_thresholds(h, reverse):
    ring = hull_of_size(h)
    assert len(set(ring)) == h
    rs = mixed(ring, reverse)
    got, boxes = assert_hulls_and_boxes(rs, (h, reverse))
    k = 0 if not reverse else 6
    assert int(got.offsets[k + 1] - got.offsets[k]) == h        # strictly convex: its own hull
    assert_boxes_equal(OB.oriented_boxes(as_rings(rs)), HS.boxes(rs), (h, reverse, "the rings themselves"))


@pytest.mark.parametrize("reverse", [False, True], ids=["stored", "reversed"])
def test_midpoints_above_the_lds_threshold(reverse):
    m = max(k for k in range(18, 25) if 2 * max(max(p) for p in HS.convex_ring(k)) <= SS.COORD_MAX)
    ring = HS.with_midpoints(HS.convex_ring(m))
    assert m >= 21 and len(ring) > LDS and max(max(p) for p in ring) <= SS.COORD_MAX
    rs = mixed(ring, reverse)
    got, _ = assert_hulls_and_boxes(rs, (m, reverse))
    k = 0 if not reverse else 6
    lo, hi = int(got.offsets[k]), int(got.offsets[k + 1])
    assert hi - lo == len(ring) // 2 and np.array_equal(host(got.vertices)[lo:hi], np.asarray(ring[::2], np.int32))


def turned(ring, k=5):
    """The ring in a hole's direction, started ``k`` positions on."""
    back = list(ring[:1]) + list(ring[:0:-1])
    return back[k % len(back):] + back[:k % len(back)]


def test_orientation_and_start():
    spiral = want_rings((65, 65), "spiral", 8)
    annulus = want_rings((65, 65), "annulus", 8)
    rings = [list(HS.with_midpoints(HS.convex_ring(6))), list(SS.staircase(WAVE + 2, 0)), list(SS.staircase(30, 1)), list(HS.convex_ring(12)),
             [tuple(v) for v in spiral.vertices[spiral.offsets[0]:spiral.offsets[1]].tolist()],
             [tuple(v) for v in annulus.vertices[annulus.offsets[0]:annulus.offsets[1]].tolist()]]
    rs = SS.ringset(rings + [turned(r) for r in rings] + [r[7:] + r[:7] for r in rings])
    assert (rs.area2 > 0).sum() == 2 * len(rings) and (rs.area2 < 0).sum() == len(rings)
    got, _ = assert_hulls_and_boxes(rs, "turned and rotated")
    n = len(rings)
    size = np.diff(host(got.offsets))
    assert np.array_equal(size[:n], size[n:2 * n]) and np.array_equal(size[:n], size[2 * n:])
    assert np.array_equal(host(got.area2)[:n], -host(got.area2)[n:2 * n]) and np.array_equal(host(got.area2)[:n], host(got.area2)[2 * n:])


def test_the_largest_coordinate():
    """The 128-bit comparison at its largest: rings moved so that their largest coordinate is 16384."""
    moved = []
    for ring in (HS.convex_ring(24), HS.with_midpoints(HS.convex_ring(6)), SS.staircase(WAVE + 2, 0), hull_of_size(3)):
        dy, dx = SS.COORD_MAX - max(p[0] for p in ring), SS.COORD_MAX - max(p[1] for p in ring)
        moved.append([(y + dy, x + dx) for y, x in ring])
    moved.append([(0, 0), (0, SS.COORD_MAX), (SS.COORD_MAX, SS.COORD_MAX), (SS.COORD_MAX, 0)])
    moved.append([(0, 3), (5, SS.COORD_MAX), (SS.COORD_MAX, SS.COORD_MAX - 3), (SS.COORD_MAX - 5, 0)])
    rs = SS.ringset(moved)
    assert rs.vertices.max() == SS.COORD_MAX
    _, boxes = assert_hulls_and_boxes(rs, "moved to 16384")
    assert int(boxes.edge[0]) == 175 and host(boxes.extent)[0].tolist() == [-118806, 120237, 239043]   # moving a ring does not change its box


def test_degenerate_rings():
    rs = SS.ringset([[], [(1, 1)] * 5, [(2, 2), (2, 9)], [(0, 0), (0, 3), (0, 6), (0, 3)], [(0, 0), (0, 5), (5, 5)], [(3, 3)], [(4, 4), (9, 9), (6, 6)],
                     [(7, 7)] * 70, [(0, k) for k in range(70)], SS.staircase(8)])
    got, boxes = assert_hulls_and_boxes(rs, "degenerate rings")
    assert np.diff(host(got.offsets)).tolist()[:9] == [0, 1, 2, 2, 3, 1, 2, 1, 2]
    assert host(boxes.edge).tolist()[:9] == [-1, -1, -1, -1, 0, -1, -1, -1, -1]
    # not hulls: the box rules ask for no convexity, and an edge of length 0 is passed over
    raw = SS.ringset([[(1, 1)] * 5, [(0, 0), (0, 0), (0, 5), (5, 5), (5, 5)], [(0, k) for k in range(70)], SS.staircase(12)])
    assert_boxes_equal(OB.oriented_boxes(as_rings(raw)), HS.boxes(raw), "rings that are no hulls")


def shoelace2(ring):
    y, x = ring[:, 0].astype(np.int64), ring[:, 1].astype(np.int64)
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def outer_only(rs: OB.Rings) -> OB.Rings:
    v, o, a = host(rs.vertices), host(rs.offsets), host(rs.area2)
    rings = [v[o[r]:o[r + 1]].tolist() for r in range(rs.count) if a[r] > 0]
    return as_rings(SS.ringset([[tuple(p) for p in ring] for ring in rings]))


@pytest.mark.parametrize("shape", [(37, 131), (65, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_invariants_without_the_spec(shape):
    for name in all_patterns(shape):
        rs = device_rings(shape, name, 8)
        out = OB.convex_hulls(rs)
        boxes = OB.oriented_boxes(out)
        assert out.count == rs.count and torch.equal(out.object, rs.object), name
        vin, oin, vout, oout = host(rs.vertices), host(rs.offsets), host(out.vertices), host(out.offsets)
        ain, aout = host(rs.area2), host(out.area2)
        assert oout[0] == 0 and oout[-1] == vout.shape[0] and (np.diff(oout) >= 4).all() and (np.diff(oout) <= np.diff(oin)).all(), name
        assert np.array_equal(np.sign(aout), np.sign(ain)) and (np.abs(aout) >= np.abs(ain)).all(), name
        shape_f = OB.box_shape(boxes, rs, out)
        edge, origin, e, extent = (host(t).astype(np.float64) for t in boxes[:4])
        assert (edge >= 0).all(), name
        for r in range(rs.count):
            P, S = vin[oin[r]:oin[r + 1]], vout[oout[r]:oout[r + 1]]
            k = 0
            for v in P:                                         # two pointers: S is a subsequence of P
                if k < len(S) and v[0] == S[k][0] and v[1] == S[k][1]:
                    k += 1
            assert k == len(S), (name, r)
            assert shoelace2(S) == aout[r], (name, r)
            assert HS.is_strictly_convex([tuple(p) for p in S.tolist()], 1 if ain[r] > 0 else -1), (name, r)
            L = e[r, 0] ** 2 + e[r, 1] ** 2
            rel = S.astype(np.float64) - origin[r]
            d, z = (rel[:, 0] * e[r, 0] + rel[:, 1] * e[r, 1]) / L, (e[r, 1] * rel[:, 0] - e[r, 0] * rel[:, 1]) / L
            assert (d >= extent[r, 0] / L - 1e-9).all() and (d <= extent[r, 1] / L + 1e-9).all(), (name, r)
            assert (z >= min(0.0, extent[r, 2] / L) - 1e-9).all() and (z <= max(0.0, extent[r, 2] / L) + 1e-9).all(), (name, r)
        assert (shape_f["solidity"] <= 1.0).all() and (shape_f["rectangularity"] <= shape_f["solidity"] + 1e-12).all(), name
        if (ain > 0).any():
            covered = OB.rasterize_rings(outer_only(out), shape).mask
            traced = OB.rasterize_rings(outer_only(rs), shape).mask
            assert bool((covered >= traced).all()) and bool(traced.any()), name


@pytest.mark.parametrize("name", ["nested_rings", "annulus", "rot_rects"])
def test_geojson_builds_on_the_result(name):
    shape = (65, 65)
    rings = device_rings(shape, name, 8)
    hulls = OB.convex_hulls(rings)
    boxes = OB.oriented_boxes(hulls)
    doc = OB.boxes_to_geojson(boxes, rings, transform=(0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0), properties=OB.box_shape(boxes, rings, hulls))
    assert len(doc["features"]) == want_label(shape, name, 8)[1]
    assert all(len(f["geometry"]["coordinates"]) == 1 and len(f["geometry"]["coordinates"][0]) == 5 and 0.0 < f["properties"]["solidity"] <= 1.0
               for f in doc["features"])
    hull_doc = OB.rings_to_geojson(hulls)                       # Rings out: the polygon writer takes the hulls unchanged
    assert len(hull_doc["features"]) == len(doc["features"])


def test_the_example_writes_the_boxes_of_the_traced_rings(tmp_path):
    import importlib.util
    import json
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "predict_scene_synth.py")
    spec = importlib.util.spec_from_file_location("predict_scene_synth_for_boxes", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    with pytest.raises(SystemExit):
        example.main(["--size", "256", "--boxes", str(tmp_path / "b.geojson")])             # only with --vector
    vector, boxes = str(tmp_path / "v.geojson"), str(tmp_path / "b.geojson")
    example.main(["--size", "256", "--vector", vector, "--boxes", boxes, "--simplify", "1.5"])
    polygons, rectangles = json.load(open(vector))["features"], json.load(open(boxes))["features"]
    assert [f["properties"]["label"] for f in rectangles] == [f["properties"]["label"] for f in polygons]
    for f in rectangles:
        (ring,) = f["geometry"]["coordinates"]
        assert len(ring) == 5 and ring[0] == ring[-1] and 0.0 < f["properties"]["rectangularity"] <= f["properties"]["solidity"] + 1e-12 <= 1.0 + 1e-12


def test_reuse_and_purity():
    a, b = ((192, 192), "noise_0.593"), ((37, 131), "rot_rects")
    ra, rb = device_rings(*a, 8), device_rings(*b, 8)
    before = tuple(t.clone() for t in ra[:4])
    first = OB.convex_hulls(ra)
    kept = tuple(t.clone() for t in first[:4])
    boxes = tuple(t.clone() for t in OB.oriented_boxes(first)[:4])
    second = OB.convex_hulls(ra)
    assert first.count == second.count and all(torch.equal(x, y) for x, y in zip(kept, second[:4]))
    assert all(torch.equal(x, y) for x, y in zip(before, ra[:4]))                       # the input is left untouched
    assert first.object.data_ptr() != ra.object.data_ptr()
    other = OB.convex_hulls(rb)                                 # another ring set in between: another scratch buffer from the cache
    assert_equals_spec(other, want_hulls(*b, 8)[0], "b")
    assert_boxes_equal(OB.oriented_boxes(other), want_hulls(*b, 8)[1], "b")
    again = OB.convex_hulls(ra)
    assert all(torch.equal(x, y) for x, y in zip(kept, again[:4])) and all(torch.equal(x, y) for x, y in zip(kept, first[:4]))
    assert all(torch.equal(x, y) for x, y in zip(boxes, OB.oriented_boxes(again)[:4]))
    assert all(torch.equal(x, y) for x, y in zip(kept, first[:4]))                      # oriented_boxes leaves its input untouched
    assert any(k[1] == "hull" for k in OB._SCRATCH if len(k) == 3)
    OB._SCRATCH.clear()
    fresh = OB.convex_hulls(ra)
    assert all(torch.equal(x, y) for x, y in zip(kept, fresh[:4]))
    assert_equals_spec(fresh, want_hulls(*a, 8)[0], "a")
    assert_boxes_equal(OB.oriented_boxes(fresh), want_hulls(*a, 8)[1], "a")


def test_empty_input_launches_nothing():
    empty = OB.Rings(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                     torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), 0)
    OB._SCRATCH.clear()
    out = OB.convex_hulls(empty)
    assert out.count == 0 and tuple(out.vertices.shape) == (0, 2) and host(out.offsets).tolist() == [0] and out.object.numel() == 0 and out.area2.numel() == 0
    boxes = OB.oriented_boxes(out)
    assert boxes.count == 0 and tuple(boxes.edge.shape) == (0,) and tuple(boxes.origin.shape) == (0, 2) and tuple(boxes.dir.shape) == (0, 2) and tuple(boxes.extent.shape) == (0, 3)
    assert not OB._SCRATCH                                      # not even a scratch buffer
    assert OB.boxes_to_geojson(boxes, out)["features"] == [] and OB.box_shape(boxes, out, out)["corners"].shape == (0, 4, 2)
    assert_equals_spec(OB.convex_hulls(OB.object_rings(OB.Components(torch.zeros((5, 7), dtype=torch.int32, device=DEV), 0))), HS.hulls(SS.ringset([])), "no object")


def test_the_wrappers_refuse():
    rs = SS.ringset([SS.staircase(8), SS.staircase(12, 1)])
    d = as_rings(rs)
    wide = torch.zeros((rs.vertices.shape[0], 4), dtype=torch.int32, device=DEV)
    for fn in (OB.convex_hulls, OB.oriented_boxes):
        bad = [lambda: fn(OB.Rings(*(t.cpu() for t in d[:4]), d.count)),
               lambda: fn(d._replace(vertices=d.vertices.to(torch.int64))),
               lambda: fn(d._replace(offsets=d.offsets.to(torch.int32))),
               lambda: fn(d._replace(object=d.object.to(torch.int64))),
               lambda: fn(d._replace(area2=d.area2.to(torch.int32))),
               lambda: fn(d._replace(vertices=wide[:, ::2])),                              # not contiguous
               lambda: fn(d._replace(count=1)),
               lambda: fn(d._replace(vertices=d.vertices.reshape(-1)))]
        for call in bad:
            with pytest.raises(_lib.StcdError):
                call()
        # found on the device: the status word
        off = rs.offsets.copy(); off[-1] -= 1
        with pytest.raises(_lib.StcdError, match="status 4"):
            fn(d._replace(offsets=dev(off)))
        off = rs.offsets.copy(); off[1] = off[2] + 1            # does not ascend
        with pytest.raises(_lib.StcdError, match="status 4"):
            fn(d._replace(offsets=dev(off)))
        v = rs.vertices.copy(); v[3, 1] = 16385
        with pytest.raises(_lib.StcdError, match="status 1"):
            fn(d._replace(vertices=dev(v)))
        v = rs.vertices.copy(); v[9, 0] = -1
        with pytest.raises(_lib.StcdError, match="status 1"):
            fn(d._replace(vertices=dev(v)))
    OB.oriented_boxes(d._replace(vertices=dev(v)), check=False)                             # reads nothing back, raises nothing
    assert_hulls_and_boxes(rs, "after the refusals", d)


def test_the_abi_directly_and_its_refusals():
    rs = SS.ringset([SS.staircase(WAVE + 6), SS.staircase(8, 1), SS.staircase(30, 2)])
    want = HS.hulls(rs)
    R, V, Vout = rs.count, rs.vertices.shape[0], want.vertices.shape[0]
    assert 3 * R <= Vout < V
    l = _lib.lib()
    vertices, offsets = dev(rs.vertices), dev(rs.offsets)
    nbytes = int(l.stcd_rings_hull_scratch_bytes(R, V)) + 64                             # a larger buffer is fine
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    count = lambda: _lib.check(l.stcd_rings_hull_count(p(vertices), p(offsets), R, V, p(counts), p(scratch), nbytes, stream))
    count()
    assert host(counts).tolist() == [Vout, 0]
    out = lambda: (torch.full((Vout, 2), -7, dtype=torch.int32, device=DEV), torch.full((R + 1,), -7, dtype=torch.int64, device=DEV),
                   torch.full((R,), -7, dtype=torch.int64, device=DEV))
    status = lambda: int(host(scratch[24:28]).view(np.int32)[0])

    def write(n_out, bufs, rings=R, verts=V, null=None, nb=nbytes):
        ptrs = [None if null == k else p(t) for k, t in enumerate(bufs)]
        rc = l.stcd_rings_hull_write(p(vertices), p(offsets), rings, verts, n_out, *ptrs, p(scratch), nb, stream)
        return rc, l.stcd_last_error().decode()

    # refused on the host, nothing launched: the outputs keep their fill
    bufs = out()
    for kw in (dict(rings=-1), dict(verts=-1), dict(rings=1 << 31), dict(null=0), dict(null=1), dict(null=2), dict(nb=64)):
        rc, err = write(Vout, bufs, **kw)
        assert rc != 0 and err.startswith("stcd_rings_hull_write: "), kw
    for n_out in (-1, V + 1):
        rc, err = write(n_out, bufs)
        assert rc != 0 and err.startswith("stcd_rings_hull_write: "), n_out
    for kw in (dict(R=-1), dict(nb=64), dict(R=1 << 31)):
        a = dict(R=R, nb=nbytes); a.update(kw)
        rc = l.stcd_rings_hull_count(p(vertices), p(offsets), a["R"], V, p(counts), p(scratch), a["nb"], stream)
        assert rc != 0 and l.stcd_last_error().decode().startswith("stcd_rings_hull_count: "), kw
    rc = l.stcd_rings_hull_count(p(vertices), p(offsets), R, V, None, p(scratch), nbytes, stream)
    assert rc != 0 and l.stcd_last_error().decode().startswith("stcd_rings_hull_count: ")
    assert all(bool((t == -7).all()) for t in bufs) and status() == 0 and host(counts).tolist() == [Vout, 0]
    # an n_out that could be a count phase's, but is not this one's: found on the device, nothing written, status bit 8
    for n_out in (Vout - 1, Vout + 1, V):
        bigger = (torch.full((V, 2), -7, dtype=torch.int32, device=DEV),) + bufs[1:]
        rc, err = write(n_out, bigger)
        assert rc == 0, err
        assert all(bool((t == -7).all()) for t in bigger) and status() & 8, n_out
        count()                                                 # a fresh count phase clears it
        assert status() == 0
    # other ring sizes than the count phase's: the same
    rc, err = write(Vout, bufs, rings=R - 1)
    assert rc == 0, err
    assert all(bool((t == -7).all()) for t in bufs) and status() & 8
    count()
    # the right one
    rc, err = write(Vout, bufs)
    assert rc == 0, err
    assert status() == 0
    hulls = OB.Rings(bufs[0], bufs[1], dev(rs.object), bufs[2], R)
    assert_equals_spec(hulls, want, "raw entries")
    # a count phase that leaves a status: its write phase writes nothing
    off = rs.offsets.copy(); off[-1] += 1
    _lib.check(l.stcd_rings_hull_count(p(vertices), p(dev(off)), R, V, p(counts), p(scratch), nbytes, stream))
    left = int(host(counts)[0])
    assert host(counts)[1] == 4 and 0 <= left <= V
    fresh = (torch.full((V, 2), -7, dtype=torch.int32, device=DEV),) + out()[1:]
    rc, err = write(left, fresh)
    assert rc == 0, err
    assert all(bool((t == -7).all()) for t in fresh) and status() & 8
    # the box entry: refused on the host with the outputs at their fill, then the right call
    box = lambda: (torch.full((R,), -7, dtype=torch.int32, device=DEV), torch.full((R, 2), -7, dtype=torch.int32, device=DEV),
                   torch.full((R, 2), -7, dtype=torch.int32, device=DEV), torch.full((R, 3), -7, dtype=torch.int64, device=DEV),
                   torch.full((1,), -7, dtype=torch.int32, device=DEV))

    def boxes(bufs, rings=R, verts=Vout, null=None):
        ptrs = [None if null == k else p(t) for k, t in enumerate(bufs)]
        rc = l.stcd_rings_boxes(p(hulls.vertices), p(hulls.offsets), rings, verts, *ptrs, stream)
        return rc, l.stcd_last_error().decode()

    bb = box()
    for kw in (dict(rings=-1), dict(verts=-1), dict(verts=1 << 31), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=4)):
        rc, err = boxes(bb, **kw)
        assert rc != 0 and err.startswith("stcd_rings_boxes: "), kw
    assert all(bool((t == -7).all()) for t in bb)
    rc, err = boxes(bb)
    assert rc == 0, err
    assert int(bb[4][0]) == 0
    assert_boxes_equal(OB.OrientedBoxes(*bb[:4], R), HS.boxes(want), "raw box entry")
    rc, err = boxes(bb, verts=Vout - 1)                         # offsets that do not end at n_vertices: found on the device
    assert rc == 0 and int(bb[4][0]) == 4, err
