"""Change polygons on the GPU: object_rings against the plain-Python specification of tests/rings_spec.py, the invariants that hold
without it, mismatched connectivities, reuse and the raw entries' refusals.  Every output is an integer and every assertion is
equality.  The shapes are test_objects_gpu.py's: objects on zero, one and several tile seams, widths that are no multiple of
anything; 192 x 192 carries the comb, one ring of 24 578 corners, which takes the ranking past anything one block could shortcut."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import objects_spec as SP
from tests import rings_spec as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = OB.TILE
SHAPES = [(1, 1), (1, T + 3), (T + 3, 1), (T, T), (T + 1, T + 1), (2 * T + 5, 3 * T - 1), (3 * T, 3 * T), (37, 131)]
SMALL = SHAPES[:5]
ids = lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else str(s)


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)               # a copy: the shared patterns are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, T), **RS.patterns(*shape)}


# the references: computed once per (shape, pattern, connectivities), shared by the tests and never written to
@functools.lru_cache(maxsize=None)
def want_label(shape, name, conn):
    lab, n = SP.label(all_patterns(shape)[name], conn)
    lab.setflags(write=False)
    return lab, n


@functools.lru_cache(maxsize=None)
def want_rings(shape, name, label_conn, conn):
    rs = RS.rings(want_label(shape, name, label_conn)[0], conn)
    for a in rs[:4]:
        a.setflags(write=False)
    return rs


def components(shape, name, conn):
    lab, n = want_label(shape, name, conn)
    return OB.Components(dev(lab), n)


def assert_equals_spec(got: OB.Rings, want: RS.RingSet, where):
    assert got.count == want.count, (where, got.count, want.count)
    assert got.vertices.dtype == torch.int32 and got.offsets.dtype == torch.int64 and got.object.dtype == torch.int32 and got.area2.dtype == torch.int64, where
    assert tuple(got.vertices.shape) == want.vertices.shape and tuple(got.offsets.shape) == want.offsets.shape, where
    assert all(t.device == DEV for t in got[:4]), where
    assert np.array_equal(host(got.offsets), want.offsets), where
    assert np.array_equal(host(got.object), want.object), where
    assert np.array_equal(host(got.area2), want.area2), where
    assert np.array_equal(host(got.vertices), want.vertices), where


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_rings_equal_the_spec(shape, conn):
    for name in all_patterns(shape):
        got = OB.object_rings(components(shape, name, conn), conn)
        assert_equals_spec(got, want_rings(shape, name, conn, conn), name)


@pytest.mark.parametrize("conn", [4, 8])
def test_the_comb_is_one_long_ring(conn):
    shape = (3 * T, 3 * T)
    want = want_rings(shape, "comb", conn, conn)
    assert shape == (192, 192) and want.count == 1 and want.vertices.shape[0] == 24578 and want.vertices.shape[0] >= 20000
    got = OB.object_rings(components(shape, "comb", conn), conn)
    assert got.count == 1 and int(got.offsets[1]) == 24578
    assert_equals_spec(got, want, "comb")
    # the same through a capacity that is exact, and one that is too small at first (the count phase is repeated once)
    assert_equals_spec(OB.object_rings(components(shape, "comb", conn), conn, max_corners=24578), want, "exact capacity")
    assert_equals_spec(OB.object_rings(components(shape, "comb", conn), conn, max_corners=100), want, "repeated count phase")


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_invariants_without_the_spec(shape, conn):
    H, W = shape
    for name, m in all_patterns(shape).items():
        d = dev(m)
        comp = OB.label_components(d, conn)
        rs = OB.object_rings(comp, conn)
        obj, area2, offsets = host(rs.object), host(rs.area2), host(rs.offsets)
        pos = area2 > 0
        assert (area2 != 0).all() and int(pos.sum()) == comp.count and np.array_equal(obj[pos], np.arange(1, comp.count + 1)), name
        lengths = np.diff(offsets)
        assert offsets[0] == 0 and (lengths >= 4).all() and (lengths % 2 == 0).all() and offsets[-1] == rs.vertices.shape[0], name
        # per object, the rings' signed areas add up to the pixel count of object_table
        area = host(OB.object_table(comp).area)
        summed = np.zeros(comp.count, np.int64)
        np.add.at(summed, obj - 1, area2)
        assert np.array_equal(summed, 2 * area), name
        # the holes: the unset components, under the complementary connectivity, whose box touches no border
        unset = OB.label_components(d, 4 if conn == 8 else 8, invert=True)
        bbox = host(OB.object_table(unset).bbox).reshape(-1, 4)
        inner = (bbox[:, 0] > 0) & (bbox[:, 1] > 0) & (bbox[:, 2] < H - 1) & (bbox[:, 3] < W - 1)
        assert int((~pos).sum()) == int(inner.sum()), name
        if shape in SMALL:
            vertices, lab = host(rs.vertices), host(comp.labels)
            for k in range(1, comp.count + 1):
                fill = RS.fill_even_odd([vertices[offsets[r]:offsets[r + 1]] for r in np.nonzero(obj == k)[0]], H, W)
                assert np.array_equal(fill, lab == k), (name, k)


@pytest.mark.parametrize("label_conn,conn", [(4, 8), (8, 4)])
@pytest.mark.parametrize("shape", [(T + 1, T + 1), (2 * T + 5, 3 * T - 1), (37, 131)], ids=ids)
def test_mismatched_connectivity_equals_the_spec(shape, label_conn, conn):
    several = False
    for name in all_patterns(shape):
        want = want_rings(shape, name, label_conn, conn)
        got = OB.object_rings(components(shape, name, label_conn), conn)      # no error
        assert_equals_spec(got, want, name)
        several = several or int((want.area2 > 0).sum()) > want_label(shape, name, label_conn)[1]
    assert several == (conn == 4)                               # labels made with 8 and rings asked with 4: objects with several outer rings


def test_arbitrary_label_images():
    """Any int32 label image is taken: neighbouring objects that share sides, and labels <= 0 as background."""
    rng = np.random.default_rng(5)
    for shape in ((9, 11), (T + 2, T + 7)):
        lab = rng.integers(-1, 4, shape).astype(np.int32)
        for conn in (4, 8):
            got = OB.object_rings(OB.Components(dev(lab), 3), conn)
            assert_equals_spec(got, RS.rings(np.maximum(lab, 0), conn), (shape, conn))


def test_reuse_and_purity():
    a, b = (2 * T + 5, 3 * T - 1), (37, 131)
    name = "noise_0.593"
    ca, cb = components(a, name, 8), components(b, name, 8)
    before = ca.labels.clone()
    first = OB.object_rings(ca, 8)
    kept = tuple(t.clone() for t in first[:4])
    second = OB.object_rings(ca, 8)
    assert first.count == second.count and all(torch.equal(x, y) for x, y in zip(kept, second[:4]))
    assert torch.equal(ca.labels, before)                       # the labels are left untouched
    other = OB.object_rings(cb, 8)                              # another shape in between: another scratch buffer from the cache
    assert_equals_spec(other, want_rings(b, name, 8, 8), "b")
    again = OB.object_rings(ca, 8)
    assert all(torch.equal(x, y) for x, y in zip(kept, again[:4])) and all(torch.equal(x, y) for x, y in zip(kept, first[:4]))
    # one scratch buffer for two label images of one shape: a sparse one after a dense one reads nothing of the earlier call
    sparse = OB.object_rings(components(a, "corners", 8), 8)
    assert_equals_spec(sparse, want_rings(a, "corners", 8, 8), "corners after noise")
    OB._SCRATCH.clear()
    fresh = OB.object_rings(ca, 8)
    assert all(torch.equal(x, y) for x, y in zip(kept, fresh[:4]))


def test_empty_results_launch_nothing():
    for comp in (OB.Components(torch.zeros((5, 7), dtype=torch.int32, device=DEV), 0), OB.Components(torch.zeros((0, 7), dtype=torch.int32, device=DEV), 0)):
        rs = OB.object_rings(comp)
        assert rs.count == 0 and tuple(rs.vertices.shape) == (0, 2) and host(rs.offsets).tolist() == [0] and rs.object.numel() == 0 and rs.area2.numel() == 0
    # objects announced but none there: the entries run and find no ring
    rs = OB.object_rings(OB.Components(torch.zeros((5, 7), dtype=torch.int32, device=DEV), 2))
    assert rs.count == 0 and host(rs.offsets).tolist() == [0]
    d = dev(np.zeros((8, 8), np.int32))
    for call in (lambda: OB.object_rings(OB.Components(d, 1), 6), lambda: OB.object_rings(OB.Components(d[:, ::2], 1)),
                 lambda: OB.object_rings(OB.Components(d.to(torch.uint8), 1)), lambda: OB.object_rings(OB.Components(d, 65)),
                 lambda: OB.object_rings(OB.Components(d, 1), max_corners=-1)):
        with pytest.raises(_lib.StcdError):
            call()


def test_the_abi_directly_and_its_refusals():
    shape = (T + 1, T + 1)
    H, W = shape
    conn = 8
    lab, n = want_label(shape, "noise_0.407", conn)
    want = want_rings(shape, "noise_0.407", conn, conn)
    R, V = want.count, want.vertices.shape[0]
    l = _lib.lib()
    d = dev(lab)
    cap = V + 10
    nbytes = int(l.stcd_rings_scratch_bytes(H, W, cap)) + 64    # a larger buffer is fine
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    counts = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(l.stcd_rings_count(p(d), H, W, conn, cap, p(counts), p(scratch), nbytes, stream))
    assert host(counts).tolist() == [R, V, 0]
    out = lambda: (torch.full((V, 2), -7, dtype=torch.int32, device=DEV), torch.full((R + 1,), -7, dtype=torch.int64, device=DEV),
                   torch.full((R,), -7, dtype=torch.int32, device=DEV), torch.full((R,), -7, dtype=torch.int64, device=DEV))
    status = lambda: int(host(scratch[20:24]).view(np.int32)[0])

    def write(r, v, bufs, connectivity=conn, capacity=cap, height=H, width=W, null=None, nb=nbytes):
        ptrs = [None if null == k else p(t) for k, t in enumerate(bufs)]
        rc = l.stcd_rings_write(p(d), height, width, connectivity, capacity, r, v, *ptrs, p(scratch), nb, stream)
        return rc, l.stcd_last_error().decode()

    # refused on the host, nothing launched: the outputs keep their fill
    bufs = out()
    for kw in (dict(connectivity=6), dict(height=-1), dict(width=-1), dict(height=1 << 16, width=1 << 15), dict(null=0), dict(null=1), dict(null=2), dict(null=3),
               dict(nb=64), dict(capacity=-1)):
        rc, err = write(R, V, bufs, **kw)
        assert rc != 0 and err.startswith("stcd_rings_write: "), kw
    for r, v in ((-1, V), (R, -2), (R, V + 11), (R, 4 * R - 2), (R, V + 1), (0, V), (R, 0)):
        rc, err = write(r, v, bufs)
        assert rc != 0 and err.startswith("stcd_rings_write: "), (r, v)
    rc = l.stcd_rings_count(p(d), H, W, 5, cap, p(counts), p(scratch), nbytes, stream)
    assert rc != 0 and l.stcd_last_error().decode().startswith("stcd_rings_count: ")
    rc = l.stcd_rings_count(p(d), H, W, conn, cap, None, p(scratch), nbytes, stream)
    assert rc != 0 and l.stcd_last_error().decode().startswith("stcd_rings_count: ")
    assert all(bool((t == -7).all()) for t in bufs) and status() == 0
    # a pair that could be a count phase's, but is not this one's: found on the device, nothing written, status bit 8
    for r, v in ((R - 1, V), (R, V - 2)):
        bigger = (torch.full((V, 2), -7, dtype=torch.int32, device=DEV), torch.full((R + 1,), -7, dtype=torch.int64, device=DEV)) + bufs[2:]
        rc, err = write(r, v, bigger)
        assert rc == 0, err
        assert all(bool((t == -7).all()) for t in bigger) and status() & 8, (r, v)
        _lib.check(l.stcd_rings_count(p(d), H, W, conn, cap, p(counts), p(scratch), nbytes, stream))      # a fresh count phase clears it
        assert status() == 0
    # the right pair
    rc, err = write(R, V, bufs)
    assert rc == 0, err
    assert status() == 0
    assert_equals_spec(OB.Rings(*bufs, R), want, "raw entries")
    # a capacity below V: the exact V, status bit 4, no ring counted
    small = V - 1
    _lib.check(l.stcd_rings_count(p(d), H, W, conn, small, p(counts), p(scratch), nbytes, stream))
    assert host(counts).tolist() == [0, V, 4]
