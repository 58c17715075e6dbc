"""Ring simplification on the GPU: simplify_rings against the plain-Python specification of tests/simplify_spec.py, ring lengths at the
thresholds between the kernels' three paths, the invariants that hold without the specification, reuse and the refusals.  Every output
is an integer and every assertion is equality.  192 x 192 carries the comb (one ring of 24 578 vertices: the path whose state lives in
global memory), the spiral (379 levels in one ring) and the checkerboard (18 051 rings, most of 4 vertices)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import objects_spec as SP
from tests import rings_spec as RS
from tests import simplify_spec as SS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = OB.TILE
QS = (0, 1, 4, 9, 16, 64, 400, 2 ** 31 - 1)
WAVE, LDS = OB.SIMPLIFY_WAVE_MAX, OB.SIMPLIFY_LDS_MAX


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)               # a copy: the shared references are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, T), **RS.patterns(*shape), **SS.patterns(*shape)}


# the references: computed once per (shape, pattern, connectivity[, q]), shared by the tests and never written to
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
def want_simple(shape, name, conn, q):
    out = SS.simplify(want_rings(shape, name, conn), q)
    for a in out[:4]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device_rings(shape, name, conn):
    """object_rings' result on the device, checked against its own specification; the tests clone nothing and must not write to it."""
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


CASES = [(shape, conn, name) for shape, conn in (((37, 131), 8), ((65, 65), 8), ((65, 65), 4), ((192, 192), 8)) for name in all_patterns(shape)]


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("shape,conn,name", CASES, ids=[f"{s[0]}x{s[1]}-c{c}-{n}" for s, c, n in CASES])
def test_device_equals_the_spec(shape, conn, name, q):
    got = OB.simplify_rings(device_rings(shape, name, conn), tolerance=np.sqrt(q / 4.0) if q < 2 ** 31 - 1 else 1e9)
    assert OB.simplify_q(np.sqrt(q / 4.0)) == q or q == 2 ** 31 - 1
    assert_equals_spec(got, want_simple(shape, name, conn, q), (name, q))


def test_the_long_the_deep_and_the_many():
    """What the 192 x 192 cases above run through: the comb is one ring above SIMPLIFY_LDS_MAX, the spiral one ring of some 380
    levels within it, the checkerboard thousands of rings of 4 vertices."""
    shape = (192, 192)
    comb, spiral, board = (want_rings(shape, name, 8) for name in ("comb", "spiral", "checkerboard"))
    assert comb.count == 1 and comb.vertices.shape[0] == 24578 > LDS
    assert spiral.count == 1 and WAVE < spiral.vertices.shape[0] == 386 <= LDS
    detail = []
    SS.simplify(spiral, 16, detail)
    assert detail[0][1] >= 370
    assert board.count == 18051 and int((np.diff(board.offsets) == 4).sum()) >= 18000
    for q, n in ((4, 256), (16, 129), (2 ** 31 - 1, 3)):
        assert int(OB.simplify_rings(device_rings(shape, "comb", 8), tolerance=np.sqrt(q / 4.0) if n > 3 else 1e9).vertices.shape[0]) == n


@functools.lru_cache(maxsize=None)
def threshold_rings(n, reverse):
    rings = [SS.staircase(n, 0), SS.staircase(4, 1), SS.staircase(n, 2), SS.staircase(4, 3), SS.staircase(6, 4), SS.staircase(n, 5), SS.staircase(4, 6)]
    objects = list(range(1, len(rings) + 1))
    if reverse:
        rings, objects = rings[::-1], objects[::-1]
    return SS.ringset(rings, objects)


@pytest.mark.parametrize("reverse", [False, True], ids=["stored", "reversed"])
@pytest.mark.parametrize("n", [4, 6, WAVE - 2, WAVE, WAVE + 2, LDS - 2, LDS, LDS + 2])
def test_ring_lengths_at_the_path_thresholds(n, reverse):
    rs = threshold_rings(n, reverse)
    d = as_rings(rs)
    for q in (4, 64):
        want = SS.simplify(rs, q)
        assert want.vertices.shape[0] < rs.vertices.shape[0] or n <= 6
        assert_equals_spec(OB.simplify_rings(d, tolerance=np.sqrt(q / 4.0)), want, (n, reverse, q))
    if not reverse:                                             # the work split does not depend on where a ring sits
        fwd, bwd = SS.simplify(rs, 64), SS.simplify(threshold_rings(n, True), 64)
        R = rs.count
        for r in range(R):
            a = fwd.vertices[fwd.offsets[r]:fwd.offsets[r + 1]]
            b = bwd.vertices[bwd.offsets[R - 1 - r]:bwd.offsets[R - r]]
            assert np.array_equal(a, b)


def test_the_sign_rule_on_the_device():
    rs = SS.ringset([SS.staircase(8, 1), SS.SIGN_FLIP_RING, SS.staircase(4, 2)])
    d = as_rings(rs)
    got = OB.simplify_rings(d, tolerance=2.0)                   # q = 16
    assert_equals_spec(got, SS.simplify(rs, 16), "q = 16")
    lo, hi = (int(v) for v in host(got.offsets)[1:3])
    assert host(got.vertices)[lo:hi].tolist() == [list(v) for v in SS.SIGN_FLIP_RING] and int(got.area2[1]) == 200
    low = OB.simplify_rings(d, tolerance=1.0)                   # q = 4: reduced, not copied
    assert_equals_spec(low, SS.simplify(rs, 4), "q = 4")
    # rings below 4 vertices, and rings that are one point or one line, are copied whole
    odd = SS.ringset([[(0, 0), (0, 5), (5, 5)], [(1, 1)] * 5, [(0, 0), (0, 3), (0, 6), (0, 3)], [], [(2, 2), (2, 9)], SS.staircase(10)])
    assert_equals_spec(OB.simplify_rings(as_rings(odd), tolerance=1.0), SS.simplify(odd, 4), "short and degenerate rings")


def shoelace2(ring):
    y, x = ring[:, 0].astype(np.int64), ring[:, 1].astype(np.int64)
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


@pytest.mark.parametrize("tolerance", [0.0, 1.0, 1.5, 5.0])
@pytest.mark.parametrize("shape", [(37, 131), (65, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_invariants_without_the_spec(shape, tolerance):
    for name in all_patterns(shape):
        rs = device_rings(shape, name, 8)
        out = OB.simplify_rings(rs, tolerance)
        assert out.count == rs.count and torch.equal(out.object, rs.object), name
        vin, oin, vout, oout = host(rs.vertices), host(rs.offsets), host(out.vertices), host(out.offsets)
        ain, aout = host(rs.area2), host(out.area2)
        assert oout[0] == 0 and oout[-1] == vout.shape[0] and (np.diff(oout) >= 3).all() and (np.diff(oout) <= np.diff(oin)).all(), name
        assert np.array_equal(np.sign(aout), np.sign(ain)) and (aout != 0).all(), name
        for r in range(rs.count):
            P, S = vin[oin[r]:oin[r + 1]], vout[oout[r]:oout[r + 1]]
            assert np.array_equal(S[0], P[0]), (name, r)
            k = 0
            for v in P:                                         # two pointers: S is a subsequence of P
                if k < len(S) and v[0] == S[k][0] and v[1] == S[k][1]:
                    k += 1
            assert k == len(S), (name, r)
            assert shoelace2(S) == aout[r], (name, r)
        if tolerance == 0.0:
            assert np.array_equal(vout, vin) and np.array_equal(oout, oin) and np.array_equal(aout, ain), name


@pytest.mark.parametrize("name", ["nested_rings", "annulus", "noise_0.593"])
def test_geojson_builds_on_the_result(name):
    shape = (65, 65)
    lab, n = want_label(shape, name, 8)
    comp = OB.Components(dev(lab), n)
    simple = OB.simplify_rings(device_rings(shape, name, 8), tolerance=1.5)
    doc = OB.rings_to_geojson(simple, transform=(0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0), properties=OB.object_table(comp))
    assert len(doc["features"]) == n
    holes = sum(len(f["geometry"]["coordinates"]) - 1 for f in doc["features"])
    assert holes == int((want_rings(shape, name, 8).area2 < 0).sum())
    assert all(len(c) >= 4 and c[0] == c[-1] for f in doc["features"] for c in f["geometry"]["coordinates"])


def test_reuse_and_purity():
    a, b = ((192, 192), "noise_0.593"), ((37, 131), "rot_rects")
    ra, rb = device_rings(*a, 8), device_rings(*b, 8)
    before = tuple(t.clone() for t in ra[:4])
    first = OB.simplify_rings(ra, 1.5)
    kept = tuple(t.clone() for t in first[:4])
    second = OB.simplify_rings(ra, 1.5)
    assert first.count == second.count and all(torch.equal(x, y) for x, y in zip(kept, second[:4]))
    assert all(torch.equal(x, y) for x, y in zip(before, ra[:4]))                       # the input is left untouched
    assert first.object.data_ptr() != ra.object.data_ptr()
    other = OB.simplify_rings(rb, 1.5)                          # another ring set in between: another scratch buffer from the cache
    assert_equals_spec(other, want_simple(*b, 8, 9), "b")
    again = OB.simplify_rings(ra, 1.5)
    assert all(torch.equal(x, y) for x, y in zip(kept, again[:4])) and all(torch.equal(x, y) for x, y in zip(kept, first[:4]))
    # one scratch buffer, another tolerance: nothing of the earlier call is read
    assert_equals_spec(OB.simplify_rings(ra, 5.0), want_simple(*a, 8, 100), "q = 100 after q = 9")
    assert any(k[1] == "simplify" for k in OB._SCRATCH if len(k) == 3)
    OB._SCRATCH.clear()
    fresh = OB.simplify_rings(ra, 1.5)
    assert all(torch.equal(x, y) for x, y in zip(kept, fresh[:4]))
    assert_equals_spec(fresh, want_simple(*a, 8, 9), "a")


def test_empty_input_launches_nothing():
    empty = OB.Rings(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                     torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), 0)
    OB._SCRATCH.clear()
    out = OB.simplify_rings(empty, 1.5)
    assert out.count == 0 and tuple(out.vertices.shape) == (0, 2) and host(out.offsets).tolist() == [0] and out.object.numel() == 0 and out.area2.numel() == 0
    assert not OB._SCRATCH                                      # not even a scratch buffer
    assert_equals_spec(OB.simplify_rings(OB.object_rings(OB.Components(torch.zeros((5, 7), dtype=torch.int32, device=DEV), 0))), SS.simplify(SS.ringset([]), 9), "no object")


def test_the_wrapper_refuses():
    rs = SS.ringset([SS.staircase(8), SS.staircase(12, 1)])
    d = as_rings(rs)
    wide = torch.zeros((rs.vertices.shape[0], 4), dtype=torch.int32, device=DEV)
    bad = [lambda: OB.simplify_rings(d, -0.5),
           lambda: OB.simplify_rings(OB.Rings(*(t.cpu() for t in d[:4]), d.count)),
           lambda: OB.simplify_rings(d._replace(vertices=d.vertices.to(torch.int64))),
           lambda: OB.simplify_rings(d._replace(offsets=d.offsets.to(torch.int32))),
           lambda: OB.simplify_rings(d._replace(object=d.object.to(torch.int64))),
           lambda: OB.simplify_rings(d._replace(area2=d.area2.to(torch.int32))),
           lambda: OB.simplify_rings(d._replace(vertices=wide[:, ::2])),                    # not contiguous
           lambda: OB.simplify_rings(d._replace(count=1)),
           lambda: OB.simplify_rings(d._replace(vertices=d.vertices.reshape(-1)))]
    for k, call in enumerate(bad):
        with pytest.raises(_lib.StcdError):
            call()
    # found on the device: the status word
    off = rs.offsets.copy(); off[-1] -= 1
    with pytest.raises(_lib.StcdError, match="status 4"):
        OB.simplify_rings(d._replace(offsets=dev(off)))
    off = rs.offsets.copy(); off[1] = off[2] + 1                # does not ascend
    with pytest.raises(_lib.StcdError, match="status 4"):
        OB.simplify_rings(d._replace(offsets=dev(off)))
    v = rs.vertices.copy(); v[3, 1] = 16385
    with pytest.raises(_lib.StcdError, match="status 1"):
        OB.simplify_rings(d._replace(vertices=dev(v)))
    v = rs.vertices.copy(); v[9, 0] = -1
    with pytest.raises(_lib.StcdError, match="status 1"):
        OB.simplify_rings(d._replace(vertices=dev(v)))
    v = rs.vertices.copy(); v[:, 1] += 16384 - v[:, 1].max()    # the largest coordinate itself is fine
    moved = RS.RingSet(v, rs.offsets, rs.object, rs.area2, rs.count)
    assert_equals_spec(OB.simplify_rings(as_rings(moved), 1.0), SS.simplify(moved, 4), "x up to 16384")
    assert_equals_spec(OB.simplify_rings(d, 1.0), SS.simplify(rs, 4), "after the refusals")


def test_the_abi_directly_and_its_refusals():
    rs = SS.ringset([SS.staircase(WAVE + 6), SS.staircase(8, 1), SS.staircase(30, 2)])
    q = 16
    want = SS.simplify(rs, q)
    R, V, Vout = rs.count, rs.vertices.shape[0], want.vertices.shape[0]
    assert 3 * R <= Vout < V
    l = _lib.lib()
    vertices, offsets = dev(rs.vertices), dev(rs.offsets)
    nbytes = int(l.stcd_rings_simplify_scratch_bytes(R, V)) + 64                         # a larger buffer is fine
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    count = lambda: _lib.check(l.stcd_rings_simplify_count(p(vertices), p(offsets), R, V, q, p(counts), p(scratch), nbytes, stream))
    count()
    assert host(counts).tolist() == [Vout, 0]
    out = lambda: (torch.full((Vout, 2), -7, dtype=torch.int32, device=DEV), torch.full((R + 1,), -7, dtype=torch.int64, device=DEV),
                   torch.full((R,), -7, dtype=torch.int64, device=DEV))
    status = lambda: int(host(scratch[24:28]).view(np.int32)[0])

    def write(n_out, bufs, rings=R, verts=V, qq=q, null=None, nb=nbytes):
        ptrs = [None if null == k else p(t) for k, t in enumerate(bufs)]
        rc = l.stcd_rings_simplify_write(p(vertices), p(offsets), rings, verts, qq, n_out, *ptrs, p(scratch), nb, stream)
        return rc, l.stcd_last_error().decode()

    # refused on the host, nothing launched: the outputs keep their fill
    bufs = out()
    for kw in (dict(rings=-1), dict(verts=-1), dict(qq=-1), dict(qq=1 << 31), dict(null=0), dict(null=1), dict(null=2), dict(nb=64)):
        rc, err = write(Vout, bufs, **kw)
        assert rc != 0 and err.startswith("stcd_rings_simplify_write: "), kw
    for n_out in (-1, V + 1):
        rc, err = write(n_out, bufs)
        assert rc != 0 and err.startswith("stcd_rings_simplify_write: "), n_out
    for kw in (dict(q=-1), dict(R=-1), dict(nb=64)):
        a = dict(q=q, R=R, nb=nbytes); a.update(kw)
        rc = l.stcd_rings_simplify_count(p(vertices), p(offsets), a["R"], V, a["q"], p(counts), p(scratch), a["nb"], stream)
        assert rc != 0 and l.stcd_last_error().decode().startswith("stcd_rings_simplify_count: "), kw
    rc = l.stcd_rings_simplify_count(p(vertices), p(offsets), R, V, q, None, p(scratch), nbytes, stream)
    assert rc != 0 and l.stcd_last_error().decode().startswith("stcd_rings_simplify_count: ")
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
    assert_equals_spec(OB.Rings(bufs[0], bufs[1], dev(rs.object), bufs[2], R), want, "raw entries")
    # a count phase that leaves a status: its write phase writes nothing
    off = rs.offsets.copy(); off[-1] += 1
    _lib.check(l.stcd_rings_simplify_count(p(vertices), p(dev(off)), R, V, q, p(counts), p(scratch), nbytes, stream))
    left = int(host(counts)[0])
    assert host(counts)[1] == 4 and 0 <= left <= V
    fresh = (torch.full((V, 2), -7, dtype=torch.int32, device=DEV),) + out()[1:]
    rc, err = write(left, fresh)
    assert rc == 0, err
    assert all(bool((t == -7).all()) for t in fresh) and status() & 8
