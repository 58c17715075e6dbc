"""Ring rasterization on the GPU: rasterize_rings against the plain-Python specification of tests/raster_spec.py on traced and on
simplified rings, the round trip that needs no specification, frame widths and edge spans at the thresholds between the kernels'
paths, the overlay counts, reuse and the refusals.  Every output is an integer or a byte and every assertion is equality."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import objects_spec as SP
from tests import raster_spec as RA
from tests import rings_spec as RS
from tests import simplify_spec as SS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = OB.TILE
SPAN, CHUNK = OB.RASTER_SPAN_MAX, OB.RASTER_ROW_CHUNK
TOLERANCES = (None, 1.0, 1.5, 5.0)                             # None: the traced rings themselves


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)               # a copy: the shared references are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, T), **RS.patterns(*shape), **SS.patterns(*shape)}


@functools.lru_cache(maxsize=None)
def want_label(shape, name, conn):
    lab, n = SP.label(all_patterns(shape)[name], conn)
    lab.setflags(write=False)
    return lab, n


@functools.lru_cache(maxsize=None)
def device_rings(shape, name, conn, tolerance=None):
    """object_rings' (and simplify_rings') result on the device; the tests clone nothing and must not write to it."""
    if tolerance is not None:
        return OB.simplify_rings(device_rings(shape, name, conn), tolerance)
    lab, n = want_label(shape, name, conn)
    return OB.object_rings(OB.Components(dev(lab), n), conn)


def host_ringset(rings) -> RS.RingSet:
    return RS.RingSet(host(rings.vertices), host(rings.offsets), host(rings.object), host(rings.area2), int(rings.count))


def as_rings(rs) -> OB.Rings:
    return OB.Rings(dev(rs.vertices), dev(rs.offsets), dev(rs.object), dev(rs.area2), int(rs.count))


def assert_raster(rings, shape, where, winding=None, **kw):
    """Both rules on the device against the specification's winding numbers of the same rings."""
    H, W = shape
    w = RA.winding(host_ringset(rings), H, W) if winding is None else winding
    value = kw.get("mask_value", 255)
    for rule in RA.RULES:
        got = OB.rasterize_rings(rings, shape, rule=rule, **kw)
        assert got.mask.dtype == torch.uint8 and tuple(got.mask.shape) == (H, W) and got.mask.device == DEV and got.mask.is_contiguous(), where
        want = (w > 0) if rule == "positive" else (w & 1).astype(bool)
        assert np.array_equal(host(got.mask), want.astype(np.uint8) * np.uint8(value)), (where, rule)
        if "overlay" in kw:
            assert np.array_equal(host(got.cm), RA.confusion(want, host(kw["overlay"]))), (where, rule)
        else:
            assert got.cm is None
    return w


CASES = [(shape, conn, name) for shape, conn in (((1, 1), 4), ((1, 1), 8), ((37, 131), 4), ((37, 131), 8), ((65, 65), 4), ((65, 65), 8), ((192, 192), 8))
         for name in all_patterns(shape)]


@pytest.mark.parametrize("shape,conn,name", CASES, ids=[f"{s[0]}x{s[1]}-c{c}-{n}" for s, c, n in CASES])
def test_device_equals_the_spec(shape, conn, name):
    lab = want_label(shape, name, conn)[0]
    for tolerance in TOLERANCES:
        rings = device_rings(shape, name, conn, tolerance)
        w = assert_raster(rings, shape, (name, tolerance))
        if tolerance is None:                                   # trace, then fill, gives back the labels
            assert np.array_equal(w, (lab > 0).astype(np.int64)), name


@pytest.mark.parametrize("shape,conn", [((37, 131), 4), ((65, 65), 8), ((192, 192), 8)], ids=lambda v: str(v))
def test_round_trip_without_the_spec(shape, conn):
    for name in all_patterns(shape):
        lab, n = want_label(shape, name, conn)
        c = OB.Components(dev(lab), n)
        for rule in RA.RULES:
            got = OB.rasterize_rings(OB.object_rings(c, conn), shape, rule=rule)
            assert torch.equal(got.mask, (c.labels > 0).to(torch.uint8) * 255), (name, rule)
        # per object: the rings of object k alone fill labels == k
        rings = host_ringset(device_rings(shape, name, conn))
        for k in sorted(set(rings.object.tolist()))[:3]:
            keep = [r for r in range(rings.count) if rings.object[r] == k]
            sub = SS.ringset([rings.vertices[rings.offsets[r]:rings.offsets[r + 1]].tolist() for r in keep], [k] * len(keep))
            assert torch.equal(OB.rasterize_rings(as_rings(sub), shape, mask_value=1).mask, (c.labels == k).to(torch.uint8)), (name, k)


# ------------------------------------------------------------------------------------------------ the thresholds between the paths
@pytest.mark.parametrize("W", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5])
def test_frame_widths_at_the_chunk_thresholds(W):
    H = 3
    rings = [[(0, W - 5), (0, W), (3, W), (3, W - 5)],                                      # reaches the last column
             [(1, W - 9), (1, W + 7), (2, W + 7), (2, W - 9)],                              # and one past it
             [(0, 0), (3, CHUNK + 2), (3, 5)],                                              # slanted, across the first chunk's end
             [(0, CHUNK - 3), (0, CHUNK + 1), (2, CHUNK + 1), (2, CHUNK - 3)],
             [(1, 7), (1, W - 20), (3, W - 20), (3, 7)],                                    # a hole in nothing: winding -1 over most of two rows
             [(0, 2), (0, 3), (1, 3), (1, 2)]]
    rings[4] = rings[4][:1] + rings[4][:0:-1]
    rs = SS.ringset(rings)
    w = RA.winding(rs, H, W)
    assert w.min() == -1 and w.max() >= 2 and w[:, W - 1].all()  # the rules differ, and the last column is set
    over = dev(SP.overlay_for(H, W))
    assert_raster(as_rings(rs), (H, W), W, winding=w)
    assert_raster(as_rings(rs), (H, W), W, winding=w, overlay=over)
    if W % 16 == 0:                                             # the same frame through the byte path: an overlay that is not 16-byte aligned
        odd = torch.zeros(H * W + 1, dtype=torch.uint8, device=DEV)[1:].view(H, W)
        odd.copy_(over)
        assert_raster(as_rings(rs), (H, W), (W, "unaligned"), winding=w, overlay=odd)


@functools.lru_cache(maxsize=None)
def span_rings(reverse):
    rings = [SS.staircase(8, 1)]
    x = 10
    for h in (SPAN - 1, SPAN, SPAN + 1):
        rings.append([(2, x), (2, x + 3), (2 + h, x + 3), (2 + h, x)])
        rings.append([(h, x + 1), (h, x + 2), (h + 1, x + 2), (h + 1, x + 1)])              # a short ring inside
        x += 5
    rings.append([(0, 0), (SPAN + 9, 7), (SPAN + 9, 0)])        # a slanted edge longer than the span
    rings.append([(1, 30), (SPAN + 11, 36), (3, 39)])           # two of them, and beyond the frame's last row
    rings.append(SS.staircase(6, 2))
    objects = list(range(1, len(rings) + 1))
    if reverse:
        rings, objects = rings[::-1], objects[::-1]
    return SS.ringset(rings, objects)


@pytest.mark.parametrize("reverse", [False, True], ids=["stored", "reversed"])
def test_edge_spans_at_the_lane_threshold(reverse):
    shape = (SPAN + 10, 40)
    rs = span_rings(reverse)
    w = assert_raster(as_rings(rs), shape, reverse)
    assert np.array_equal(w, RA.winding(span_rings(not reverse), *shape))                  # the same pixels either way
    assert w.max() >= 1 and w[SPAN + 8, :6].all() and not w[SPAN + 9, :6].any()
    # a frame of fewer rows: every long edge is clipped to a short one
    assert_raster(as_rings(rs), (SPAN - 1, 40), (reverse, "clipped"), winding=w[:SPAN - 1])


def test_the_largest_triangle_into_a_small_frame():
    """num reaches 2^29 and the edges span 16384 rows: 32 bits hold it and the rows are clipped before the loop (16 rows are walked)."""
    rs = SS.ringset([[(0, 0), (0, 16384), (16384, 0)], [(0, 16384), (16384, 16384), (16384, 0)]])
    assert rs.area2.tolist() == [16384 * 16384, 16384 * 16384]
    w = assert_raster(as_rings(rs), (16, 16), "both halves")
    assert (w == 1).all()
    one = SS.ringset([[(0, 0), (0, 16384), (16384, 0)]])
    assert (assert_raster(as_rings(one), (16, 16), "upper left") == 1).all()
    far = SS.ringset([[(16384, 16384), (16384, 16380), (16370, 16384)], [(3, 0), (9, 16384), (9, 0)]])
    w = assert_raster(as_rings(far), (16, 16), "far corner")
    assert w[3:9].any() and not w[:3].any() and not w[9:].any()
    w = assert_raster(as_rings(far), (16384, 16), "16384 rows")
    assert w.shape == (16384, 16)


# ------------------------------------------------------------------------------------------------ other behaviour
@pytest.mark.parametrize("shape", [(37, 131), (64, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_overlay_counts(shape):
    H, W = shape
    name = "rot_rects"
    rings = device_rings(shape, name, 8, 1.5)
    over = SP.overlay_for(H, W)
    assert (over == 255).any() and (over == 3).any()
    for o in (over, np.zeros_like(over), np.full_like(over, 255), all_patterns(shape)[name]):
        w = assert_raster(rings, shape, "overlay", overlay=dev(o))
        got = OB.rasterize_rings(rings, shape, overlay=dev(o))
        assert int(got.cm.sum()) == int((o != 255).sum())
        assert got.cm.dtype == torch.int64 and tuple(got.cm.shape) == (2, 2) and got.cm.device == DEV
    # against the mask the rings were traced from: the pixels the tolerance cost
    m = all_patterns(shape)[name]
    got = OB.rasterize_rings(rings, shape, overlay=dev(m))
    assert int(got.cm[0, 1] + got.cm[1, 0]) == int(((w > 0) != (m > 0)).sum())
    exact = OB.rasterize_rings(device_rings(shape, name, 8), shape, overlay=dev(m))
    assert int(exact.cm[0, 1]) == 0 and int(exact.cm[1, 0]) == 0 and int(exact.cm[1, 1]) == int((m > 0).sum())


def test_mask_value_and_check_false():
    shape = (65, 65)
    rings = device_rings(shape, "disks", 8, 1.5)
    w = RA.winding(host_ringset(rings), *shape)
    for value in (1, 7, 255):
        assert_raster(rings, shape, value, winding=w, mask_value=value)
    over = dev(SP.overlay_for(*shape))
    a, b = OB.rasterize_rings(rings, shape, overlay=over), OB.rasterize_rings(rings, shape, overlay=over, check=False)
    assert torch.equal(a.mask, b.mask) and torch.equal(a.cm, b.cm)
    assert_raster(rings, shape, "check=False", winding=w, check=False)


def empty_rings():
    return OB.Rings(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                    torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), 0)


def test_an_empty_ring_set_gives_zeros():
    for shape in ((5, 7), (3, 1024)):
        OB._SCRATCH.clear()
        got = OB.rasterize_rings(empty_rings(), shape)
        assert tuple(got.mask.shape) == shape and not got.mask.any() and got.cm is None
        over = SP.overlay_for(*shape)
        got = OB.rasterize_rings(empty_rings(), shape, overlay=dev(over), rule="evenodd")
        assert not got.mask.any() and np.array_equal(host(got.cm), RA.confusion(np.zeros(shape, np.uint8), over))
        assert int(got.cm[0, 0]) == int((over == 0).sum()) and int(got.cm[1, 0]) == int(((over != 0) & (over != 255)).sum())
    # rings, but none with a vertex
    hollow = OB.Rings(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV),
                      torch.ones(3, dtype=torch.int32, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV), 3)
    assert not OB.rasterize_rings(hollow, (5, 7)).mask.any()
    assert not OB.rasterize_rings(OB.object_rings(OB.Components(torch.zeros((5, 7), dtype=torch.int32, device=DEV), 0)), (5, 7)).mask.any()


def test_reuse_and_purity():
    a, b = ((192, 192), "noise_0.593"), ((37, 131), "rot_rects")
    ra, rb = device_rings(*a, 8), device_rings(*b, 8, 1.5)
    wa, wb = RA.winding(host_ringset(ra), *a[0]), RA.winding(host_ringset(rb), *b[0])
    before = tuple(t.clone() for t in ra[:4])
    over = dev(SP.overlay_for(*a[0]))
    over_before = over.clone()
    first = OB.rasterize_rings(ra, a[0], overlay=over)
    kept = (first.mask.clone(), first.cm.clone())
    second = OB.rasterize_rings(ra, a[0], overlay=over)
    assert torch.equal(kept[0], second.mask) and torch.equal(kept[1], second.cm)           # cm is zeroed per call, not added to
    assert first.mask.data_ptr() != second.mask.data_ptr()
    assert all(torch.equal(x, y) for x, y in zip(before, ra[:4])) and torch.equal(over, over_before)   # the inputs are left untouched
    assert_raster(rb, b[0], "b", winding=wb)                    # another ring set and frame in between: another scratch buffer
    assert_raster(rb, a[0], "b into a's frame")                 # another ring set on a's scratch buffer: nothing of the earlier call is read
    again = OB.rasterize_rings(ra, a[0], overlay=over)
    assert torch.equal(kept[0], again.mask) and torch.equal(kept[1], again.cm) and torch.equal(kept[0], first.mask)
    assert_raster(ra, b[0], "a into b's frame", winding=wa[:b[0][0], :b[0][1]])            # the crop
    assert sum(1 for k in OB._SCRATCH if len(k) == 3 and k[1] == "raster") >= 2
    OB._SCRATCH.clear()
    fresh = OB.rasterize_rings(ra, a[0], overlay=over)
    assert torch.equal(kept[0], fresh.mask) and torch.equal(kept[1], fresh.cm)
    assert np.array_equal(host(fresh.mask), (wa > 0).astype(np.uint8) * np.uint8(255))


def test_the_wrapper_refuses():
    rs = SS.ringset([SS.staircase(8), SS.staircase(12, 1)])
    d = as_rings(rs)
    shape = (48, 48)
    w = RA.winding(rs, *shape)
    wide = torch.zeros((rs.vertices.shape[0], 4), dtype=torch.int32, device=DEV)
    good = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    bad = [lambda: OB.rasterize_rings(OB.Rings(*(t.cpu() for t in d[:4]), d.count), shape),
           lambda: OB.rasterize_rings(d._replace(vertices=d.vertices.to(torch.int64)), shape),
           lambda: OB.rasterize_rings(d._replace(offsets=d.offsets.to(torch.int32)), shape),
           lambda: OB.rasterize_rings(d._replace(vertices=wide[:, ::2]), shape),            # not contiguous
           lambda: OB.rasterize_rings(d._replace(count=1), shape),
           lambda: OB.rasterize_rings(d, (0, 48)), lambda: OB.rasterize_rings(d, (48, 16385)), lambda: OB.rasterize_rings(d, (48,)),
           lambda: OB.rasterize_rings(d, 48), lambda: OB.rasterize_rings(d, shape, rule="nonzero"), lambda: OB.rasterize_rings(d, shape, rule=0),
           lambda: OB.rasterize_rings(d, shape, mask_value=0), lambda: OB.rasterize_rings(d, shape, mask_value=256),
           lambda: OB.rasterize_rings(d, shape, overlay=good.cpu()), lambda: OB.rasterize_rings(d, shape, overlay=good[:, :47]),
           lambda: OB.rasterize_rings(d, shape, overlay=good.to(torch.int32)), lambda: OB.rasterize_rings(d, (48, 47), overlay=good)]
    for k, call in enumerate(bad):
        with pytest.raises(_lib.StcdError):
            call()
    # found on the device: the status word
    off = rs.offsets.copy(); off[-1] -= 1
    with pytest.raises(_lib.StcdError, match="status 4"):
        OB.rasterize_rings(d._replace(offsets=dev(off)), shape)
    off = rs.offsets.copy(); off[1] = off[2] + 1                # does not ascend
    with pytest.raises(_lib.StcdError, match="status 4"):
        OB.rasterize_rings(d._replace(offsets=dev(off)), shape)
    off = rs.offsets.copy(); off[0] = 1                         # does not start at 0
    with pytest.raises(_lib.StcdError, match="status 4"):
        OB.rasterize_rings(d._replace(offsets=dev(off)), shape)
    v = rs.vertices.copy(); v[3, 1] = 16385
    with pytest.raises(_lib.StcdError, match="status 1"):
        OB.rasterize_rings(d._replace(vertices=dev(v)), shape)
    v = rs.vertices.copy(); v[9, 0] = -1
    with pytest.raises(_lib.StcdError, match="status 1"):
        OB.rasterize_rings(d._replace(vertices=dev(v)), shape)
    OB.rasterize_rings(d._replace(vertices=dev(v)), shape, check=False)                    # nothing is read back, nothing raises
    v = rs.vertices.copy(); v[:, 1] += 16384 - v[:, 1].max()    # the largest coordinate itself is fine
    moved = RS.RingSet(v, rs.offsets, rs.object, rs.area2, rs.count)
    assert not assert_raster(as_rings(moved), shape, "x up to 16384").any()
    assert assert_raster(d, shape, "after the refusals", winding=w).any()


def test_the_abi_directly_and_its_refusals():
    rs = SS.ringset([SS.staircase(20), [(3, 30), (40, 33), (6, 38)]])
    H, W = 44, 40
    want = RA.fill(rs, H, W)
    l = _lib.lib()
    vertices, offsets = dev(rs.vertices), dev(rs.offsets)
    R, V = rs.count, rs.vertices.shape[0]
    nbytes = int(l.stcd_rings_raster_scratch_bytes(H, W)) + 64                              # a larger buffer is fine
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    mask = torch.full((H, W), 0x5A, dtype=torch.uint8, device=DEV)
    over = dev(SP.overlay_for(H, W))
    cm = torch.full((4,), 100, dtype=torch.int64, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(rings=R, verts=V, h=H, w=W, rule=0, value=9, o=over, c=cm, m=mask, v=vertices, off=offsets, s=scratch, nb=nbytes):
        rc = l.stcd_rings_raster(p(v), p(off), rings, verts, h, w, rule, value, p(o), p(c), p(m), p(s), nb, stream)
        return rc, l.stcd_last_error().decode()

    # refused on the host, nothing launched: the mask, cm and the scratch buffer keep their fill
    for kw in (dict(rings=-1), dict(verts=-1), dict(rings=1 << 31), dict(h=0), dict(w=16385), dict(rule=2), dict(value=0), dict(value=256), dict(o=None),
               dict(c=None), dict(m=None), dict(v=None), dict(off=None), dict(s=None), dict(nb=nbytes - 72), dict(s=scratch[4:]), dict(c=scratch[4:36].view(torch.int32))):
        rc, err = call(**kw)
        assert rc != 0 and err.startswith("stcd_rings_raster: "), kw
    assert bool((mask == 0x5A).all()) and host(cm).tolist() == [100] * 4 and bool((scratch == 0xAB).all())
    rc, err = call()
    assert rc == 0, err
    assert int(host(scratch[:4]).view(np.int32)[0]) == 0
    assert np.array_equal(host(mask), want.astype(np.uint8) * np.uint8(9))
    assert np.array_equal(host(cm).reshape(2, 2), RA.confusion(want, host(over)) + 100)    # added to what cm holds
    assert bool((scratch[nbytes - 64:] == 0xAB).all())          # nothing past the bytes the entry asks for
    rc, err = call(rule=1, o=None, c=None)
    assert rc == 0, err
    assert np.array_equal(host(mask), RA.fill(rs, H, W, "evenodd").astype(np.uint8) * np.uint8(9))
    # a status leaves the word in the header
    off = rs.offsets.copy(); off[1] += 1000
    rc, err = call(off=dev(off), o=None, c=None)
    assert rc == 0, err
    assert int(host(scratch[:4]).view(np.int32)[0]) == 4
    rc, err = call(o=None, c=None)
    assert rc == 0 and int(host(scratch[:4]).view(np.int32)[0]) == 0 and np.array_equal(host(mask), want.astype(np.uint8) * np.uint8(9))
