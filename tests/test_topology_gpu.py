"""Ring topology on the GPU: ring_conflicts and simplify_rings_safe against the plain-Python specification of tests/topology_spec.py,
for every grid cell size, on traced, simplified and hull rings and on the hand-made ring sets that masks cannot give; the round cap,
the identities, purity, reuse and the refusals.  Every output is an integer and every assertion is equality.  tests/test_topology_cpu.py
shows that the cases need repair and that the specification mends them."""
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
from tests import topology_spec as TS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = OB.TILE
CELLS = (8, 32, 256, 0)
QS = (4, 9, 36)                                                 # tolerances 1.0, 1.5, 3.0
TILE = OB.TOPO_TILE


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)               # a copy: the shared references are read-only


def host(t):
    return t.cpu().numpy()


def tol(q):
    return float(np.sqrt(q / 4.0))


@functools.lru_cache(maxsize=None)
def masks(shape):
    if shape == "extra":
        return {"dent_cross": TS.dent_mask("cross"), "dent_jump": TS.dent_mask("jump"), "noise64": SP.patterns(64, 64, T)["noise_0.593"],
                "roofs96": TS.roofs(96, 96, 0)}
    extra = {k: v for k, v in SP.patterns(*shape, T).items() if k in ("noise_0.407", "noise_0.593", "serpentine", "corner_diag_main")}
    return {**RS.patterns(*shape), **SS.patterns(*shape), **extra}     # the last four need repair, and many rounds of it


# the references: computed once per case, shared by the tests and never written to
@functools.lru_cache(maxsize=None)
def traced(shape, name, conn):
    lab, _ = SP.label(masks(shape)[name], conn)
    rs = RS.rings(lab, conn)
    for a in rs[:4]:
        a.setflags(write=False)
    return rs


@functools.lru_cache(maxsize=None)
def ring_kind(shape, name, conn, kind):
    rs = traced(shape, name, conn)
    return rs if kind == "traced" else HS.hulls(rs) if kind == "hull" else SS.simplify(rs, kind)


@functools.lru_cache(maxsize=None)
def want_flags(shape, name, conn, kind):
    flags, _ = TS.conflicts(ring_kind(shape, name, conn, kind))
    flags.setflags(write=False)
    return flags


@functools.lru_cache(maxsize=None)
def want_safe(shape, name, conn, q, max_rounds=None):
    return TS.simplify_safe(traced(shape, name, conn), q, max_rounds)


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


def assert_flags(d: OB.Rings, want, where, cells=CELLS):
    for cell in cells:
        got = OB.ring_conflicts(d, cell=cell)
        assert got.flags.dtype == torch.uint8 and tuple(got.flags.shape) == want.shape and got.flags.device == DEV, (where, cell)
        assert np.array_equal(host(got.flags), want), (where, cell, np.flatnonzero(host(got.flags) != want)[:8])
        assert isinstance(got.count, int) and got.count == int(want.sum()), (where, cell)


def assert_safe(d: OB.Rings, want, where, cells=CELLS, max_rounds=None):
    rs, rounds, restored, conflicts = want
    for cell in cells:
        got = OB.simplify_rings_safe(d, tolerance=where[-1], max_rounds=max_rounds, cell=cell)
        assert (got.rounds, got.restored, got.conflicts) == (rounds, restored, conflicts), (where, cell, got[1:], want[1:])
        assert_equals_spec(got.rings, rs, (where, cell))


CASES = [(shape, conn, name) for shape, conn in (((37, 131), 8), ((65, 65), 8), ((65, 65), 4), ("extra", 8)) for name in masks(shape)]
IDS = [f"{s if isinstance(s, str) else f'{s[0]}x{s[1]}'}-c{c}-{n}" for s, c, n in CASES]


@pytest.mark.parametrize("shape,conn,name", CASES, ids=IDS)
def test_conflict_flags_equal_the_spec(shape, conn, name):
    for kind in ("traced",) + QS + ("hull",):
        assert_flags(as_rings(ring_kind(shape, name, conn, kind)), want_flags(shape, name, conn, kind), (name, kind))
    assert not want_flags(shape, name, conn, "traced").any()


@pytest.mark.parametrize("shape,conn,name", CASES, ids=IDS)
def test_safe_simplification_equals_the_spec(shape, conn, name):
    d = as_rings(traced(shape, name, conn))
    for q in QS:
        want = want_safe(shape, name, conn, q)
        assert_safe(d, want, (name, q, tol(q)))
        if want[1] == 0:                                        # nothing flagged: plain Douglas-Peucker, bit for bit
            assert_equals_spec(OB.simplify_rings(d, tol(q)), want[0], (name, q, "plain"))


def test_the_cases_that_need_repair_do():
    """What the comparison above runs through (tests/test_topology_cpu.py pins the figures): rounds, restores and residuals."""
    assert want_safe("extra", "dent_cross", 8, 36)[1:] == (1, 1, 0) and want_safe("extra", "dent_jump", 8, 36)[1:] == (1, 1, 0)
    assert want_safe("extra", "noise64", 8, 9)[1:] == (13, 337, 0) and want_safe("extra", "noise64", 8, 36)[1:] == (19, 440, 0)
    assert want_safe("extra", "roofs96", 8, 9)[1:] == (12, 13, 0)
    assert int(want_flags("extra", "noise64", 8, 9).sum()) > 0 and int(want_flags("extra", "dent_cross", 8, 36).sum()) == 3


# ------------------------------------------------------------------------------------------------ what masks cannot reach
SQUARE = [(0, 0), (0, 20), (20, 20), (20, 0)]


def shifted(ring, dy, dx):
    return [(y + dy, x + dx) for y, x in ring]


HAND = {
    "spike": [[(5, 5), (5, 40), (5, 20), (30, 20)]],
    "collinear_overlap": [shifted(SQUARE, 3, 3), [(23, 10), (23, 30), (40, 30), (40, 10)]],
    "vertex_on_edge": [shifted(SQUARE, 3, 3), [(13, 23), (5, 40), (25, 40)]],
    "crossing_squares": [shifted(SQUARE, 0, 0), shifted(SQUARE, 10, 10)],
    "shared_vertex_only": [shifted(SQUARE, 0, 0), shifted(SQUARE, 20, 20)],
    "frame_diagonal": [[(0, 0), (16384, 16384), (16384, 16380)], [(0, 16384), (16384, 0), (16380, 0)], [(8000, 8100), (8000, 8300), (8200, 8300)]],
    "frame_sides": [[(0, 0), (0, 16384), (16384, 16384), (16384, 0)], [(5, 5), (5, 16000), (9, 16000), (9, 5)]],
    "zero_length": [[(4, 4), (4, 4), (4, 30), (30, 30), (30, 30)], [(2, 10), (40, 10), (40, 12)]],
    "empty_and_short": [[], [(3, 3)], [(5, 5), (9, 9)], [(0, 7), (12, 7), (12, 9)], []],
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_ring_sets(name):
    rs = SS.ringset(HAND[name])
    flags, pairs = TS.conflicts(rs)
    expect = {"spike": 3, "collinear_overlap": 4, "vertex_on_edge": 3, "crossing_squares": 4, "shared_vertex_only": 0, "frame_diagonal": 6,
              "frame_sides": 0, "zero_length": 4, "empty_and_short": 4}
    assert int(flags.sum()) == expect[name], (name, flags.tolist())
    d = as_rings(rs)
    assert_flags(d, flags, name)
    for q in (9, 2 ** 31 - 1):
        want = TS.simplify_safe(rs, q)
        assert_safe(d, want, (name, q, tol(q) if q == 9 else 1e9))
    if name == "crossing_squares":                              # foreign rings that cross already: the loop ends, the residue is reported
        got = OB.simplify_rings_safe(d, 1.5)
        assert got.conflicts == 4 and got.rounds == 0 and got.restored == 0


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_one_cell_with_more_edges_than_a_tile(n):
    rs = SS.ringset(TS.fan(n, (300, 300)))
    flags, _ = TS.conflicts(rs)
    assert flags.reshape(n, 3)[:, 0].all()
    assert_flags(as_rings(rs), flags, ("fan", n))


@functools.lru_cache(maxsize=None)
def pocket_case(m):
    """A staircase ring whose longest chain under the widest tolerance has exactly ``m`` vertices, and a unit square inside that
    chain's pocket: plain Douglas-Peucker jumps over the square."""
    ring = list(SS.staircase(m + 1 if m % 2 else m + 2))
    if m % 2 == 0:
        del ring[9]                                             # an odd ring: the staircase with one corner cut
    kept, _, _ = SS.simplify_ring(ring, 2 ** 31 - 1)
    i, j = max(zip(kept, kept[1:]), key=lambda c: c[1] - c[0])
    assert j - i + 1 == m, (m, kept)
    Q = ring[i:j + 1]
    cy, cx = ring[(i + j) // 2]
    for dy in range(-12, 13):
        for dx in range(-12, 13):
            sq = [(cy + dy, cx + dx), (cy + dy, cx + dx + 1), (cy + dy + 1, cx + dx + 1), (cy + dy + 1, cx + dx)]
            if min(min(p) for p in sq) >= 0 and all(TS.on_or_inside(p, Q) for p in sq):
                rs = SS.ringset([sq, ring, shifted(SQUARE, 9000, 9000)])
                if not TS.conflicts(rs)[0].any():
                    return rs
    raise AssertionError(f"no square fits the pocket of {m} vertices")


@pytest.mark.parametrize("m", [63, 64, 65, 129, OB.SIMPLIFY_LDS_MAX + 3])
def test_pocket_chains_at_the_lane_and_block_sizes(m):
    rs = pocket_case(m)
    detail = {}
    want = TS.simplify_safe(rs, 2 ** 31 - 1, detail=detail)
    assert detail["flagged"][0] == 0 and detail["hits"][0] >= 1 and want[1] >= 1 and want[2] >= 1 and want[3] == 0
    assert_safe(as_rings(rs), want, (m, 1e9), cells=(8, 0) if m > 200 else CELLS)
    capped = TS.simplify_safe(rs, 2 ** 31 - 1, max_rounds=0)
    assert TS.parities(capped[0]) != TS.parities(rs) and TS.parities(want[0]) == TS.parities(rs)


# ------------------------------------------------------------------------------------------------ the interface
def test_the_round_cap_reports_what_is_left():
    d = as_rings(traced("extra", "noise64", 8))
    for cap in (0, 1, 3):
        want = want_safe("extra", "noise64", 8, 9, cap)
        assert want[1] == cap and want[3] > 0
        assert_safe(d, want, ("noise64", cap, 1.5), cells=(0, 32), max_rounds=cap)
    plain = OB.simplify_rings(d, 1.5)
    assert OB.ring_conflicts(plain).count == want_safe("extra", "noise64", 8, 9, 0)[3] == 55


def test_tolerance_zero_is_the_identity_and_empty_input_launches_nothing():
    rs = traced((65, 65), "comb", 8)
    d = as_rings(rs)
    got = OB.simplify_rings_safe(d, 0.0)
    assert (got.rounds, got.restored, got.conflicts) == (0, 0, 0)
    assert_equals_spec(got.rings, rs, "tolerance 0")
    assert got.rings.vertices.data_ptr() != d.vertices.data_ptr()
    empty = OB.Rings(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                     torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), 0)
    OB._SCRATCH.clear()
    out = OB.simplify_rings_safe(empty, 1.5)
    assert out.rings.count == 0 and tuple(out.rings.vertices.shape) == (0, 2) and host(out.rings.offsets).tolist() == [0] and out[1:] == (0, 0, 0)
    c = OB.ring_conflicts(empty)
    assert c.count == 0 and tuple(c.flags.shape) == (0,)
    c = OB.ring_conflicts(empty, check=False)
    assert int(c.count) == 0 and c.count.dtype == torch.int64
    assert not OB._SCRATCH                                      # not even a scratch buffer


def test_check_false_reads_nothing_back(monkeypatch):
    rs = ring_kind("extra", "noise64", 8, 9)
    want = want_flags("extra", "noise64", 8, 9)
    d = as_rings(rs)
    OB.ring_conflicts(d)                                        # the buffers exist

    def refuse(*a, **k):
        raise AssertionError("a host read")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy", "__int__", "__bool__", "__index__"):
            m.setattr(torch.Tensor, name, refuse)
        got = OB.ring_conflicts(d, check=False)
    assert torch.is_tensor(got.count) and got.count.dtype == torch.int64 and got.count.device == DEV
    assert int(got.count) == int(want.sum()) and np.array_equal(host(got.flags), want)
    bad = rs.vertices.copy(); bad[5, 0] = -3
    got = OB.ring_conflicts(d._replace(vertices=dev(bad)), check=False)    # a status: no exception, the count says so
    assert int(got.count) == -1


def test_purity_and_reuse():
    a, b = traced("extra", "noise64", 8), traced((65, 65), "disks", 8)
    da, db = as_rings(a), as_rings(b)
    first = OB.simplify_rings_safe(da, 3.0)
    flags = OB.ring_conflicts(OB.simplify_rings(da, 3.0))
    for _ in range(2):
        OB.simplify_rings_safe(db, 1.5); OB.ring_conflicts(db, cell=8)          # other work on the shared buffers in between
        again = OB.simplify_rings_safe(da, 3.0)
        assert again[1:] == first[1:] and all(torch.equal(x, y) for x, y in zip(again.rings[:4], first.rings[:4]))
        f2 = OB.ring_conflicts(OB.simplify_rings(da, 3.0))
        assert f2.count == flags.count and torch.equal(f2.flags, flags.flags)
    OB._SCRATCH.clear()                                         # and on fresh ones
    again = OB.simplify_rings_safe(da, 3.0)
    assert again[1:] == first[1:] and all(torch.equal(x, y) for x, y in zip(again.rings[:4], first.rings[:4]))
    # the inputs are left as they were
    assert np.array_equal(host(da.vertices), a.vertices) and np.array_equal(host(da.offsets), a.offsets)


def test_a_grid_with_more_entries_than_the_default_capacity():
    """Long edges enter many cells of the finest grid: the first call reports the capacity bit, the wrapper repeats it once."""
    ring = [(0, 0), (16384, 16380), (16384, 16384)]
    rs = SS.ringset([ring] + [shifted(ring, 0, 0)[::-1]])
    flags, _ = TS.conflicts(rs)
    assert flags.all()
    assert_flags(as_rings(rs), flags, "capacity", cells=(8,))
    want = TS.simplify_safe(rs, 9)
    assert_safe(as_rings(rs), want, ("capacity", 9, 1.5), cells=(8,))


def test_the_wrappers_refuse():
    rs = SS.ringset([SS.staircase(8), SS.staircase(12, 1)])
    d = as_rings(rs)
    wide = torch.zeros((rs.vertices.shape[0], 4), dtype=torch.int32, device=DEV)
    for fn in (OB.ring_conflicts, OB.simplify_rings_safe):
        bad = [lambda: fn(OB.Rings(*(t.cpu() for t in d[:4]), d.count)),
               lambda: fn(d._replace(vertices=d.vertices.to(torch.int64))),
               lambda: fn(d._replace(offsets=d.offsets.to(torch.int32))),
               lambda: fn(d._replace(object=d.object.to(torch.int64))),
               lambda: fn(d._replace(area2=d.area2.to(torch.int32))),
               lambda: fn(d._replace(vertices=wide[:, ::2])),                              # not contiguous
               lambda: fn(d._replace(count=1)),
               lambda: fn(d, cell=12), lambda: fn(d, cell=4), lambda: fn(d, cell=512), lambda: fn(d, cell=-8)]
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
    for call in (lambda: OB.simplify_rings_safe(d, -1.0), lambda: OB.simplify_rings_safe(d, float("nan")), lambda: OB.simplify_rings_safe(d, 1.5, max_rounds=-1)):
        with pytest.raises(_lib.StcdError):
            call()
    assert_safe(d, TS.simplify_safe(rs, 9), ("after the refusals", 9, 1.5))


def test_the_abi_directly_and_its_refusals():
    rs = traced("extra", "dent_cross", 8)
    want, rounds, restored, left = want_safe("extra", "dent_cross", 8, 36)
    plain = SS.simplify(rs, 36)
    R, V, E0, E1 = rs.count, rs.vertices.shape[0], plain.vertices.shape[0], want.vertices.shape[0]
    assert (R, V, E0, E1, rounds) == (2, 12, 8, 9, 1)
    l = _lib.lib()
    vertices, offsets = dev(rs.vertices), dev(rs.offsets)
    cell = 32
    nbytes = int(l.stcd_rings_topo_scratch_bytes(R, V, cell)) + 64                          # a larger buffer is fine
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    counts = torch.full((8,), -1, dtype=torch.int64, device=DEV)
    cap = 4 * V + 64
    entries = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    flags = torch.full((V,), 7, dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    err = lambda: l.stcd_last_error().decode()

    def conflicts(v=vertices, o=offsets, rings=R, verts=V, c=cell, f=flags, cn=counts, en=entries, cp=cap, sc=scratch, nb=nbytes):
        return l.stcd_rings_conflicts(p(v), p(o), rings, verts, c, p(f), p(cn), p(en), cp, p(sc), nb, stream)

    def begin(q=36, rings=R, verts=V, c=cell, cn=counts, nb=nbytes):
        return l.stcd_rings_safe_begin(p(vertices), p(offsets), rings, verts, q, c, p(cn), p(scratch), nb, stream)

    def round_(n_edges, restore=1, rings=R, verts=V, c=cell, en=entries, cp=cap, nb=nbytes):
        return l.stcd_rings_safe_round(p(vertices), p(offsets), rings, verts, c, n_edges, restore, p(counts), p(en), cp, p(scratch), nb, stream)

    # refused on the host, nothing launched: the outputs keep their fill
    for kw in (dict(v=None), dict(o=None), dict(f=None), dict(cn=None), dict(en=None), dict(sc=None), dict(rings=-1), dict(verts=-1), dict(rings=1 << 31),
               dict(c=12), dict(c=4), dict(c=512), dict(cp=-1), dict(cp=1 << 31), dict(nb=64)):
        assert conflicts(**kw) != 0 and err().startswith("stcd_rings_conflicts: "), kw
    odd = torch.zeros(4 * V + 2, dtype=torch.int32, device=DEV)
    assert conflicts(v=odd[1:]) != 0 and err().startswith("stcd_rings_conflicts: ")        # misaligned vertices
    for kw in (dict(q=-1), dict(q=1 << 31), dict(rings=-1), dict(c=3), dict(cn=None), dict(nb=64)):
        assert begin(**kw) != 0 and err().startswith("stcd_rings_safe_begin: "), kw
    for kw in (dict(n_edges=-1), dict(n_edges=V + 1), dict(c=24), dict(en=None), dict(cp=-1), dict(nb=64)):
        a = dict(n_edges=E0); a.update(kw)
        assert round_(**a) != 0 and err().startswith("stcd_rings_safe_round: "), kw
    assert bool((flags == 7).all()) and bool((counts == -1).all()) and bool((entries == -1).all())
    # the conflicts entry on the plain rings
    pv, po = dev(plain.vertices), dev(plain.offsets)
    pf = torch.full((E0,), 7, dtype=torch.uint8, device=DEV)
    assert conflicts(v=pv, o=po, verts=E0, f=pf) == 0, err()
    assert np.array_equal(host(pf), TS.conflicts(plain)[0]) and host(counts).tolist()[:2] == [0, E0] and int(counts[4]) == 3
    # a capacity that is too small: bit 16, the needed number, no flag
    assert conflicts(v=pv, o=po, verts=E0, f=pf, cp=2) == 0, err()
    c = host(counts).tolist()
    assert c[0] == 16 and c[2] > 2 and c[4] == -1 and not bool(pf.any())
    # the loop by hand
    assert begin() == 0, err()
    assert host(counts).tolist()[:2] == [0, E0]
    assert round_(E0 - 1) == 0, err()                           # not the device's own count: bit 8, nothing restored
    assert host(counts).tolist()[0] == 8
    assert round_(E0, cp=1) == 0, err()                         # too small a capacity: bit 16, nothing restored
    c = host(counts).tolist()
    assert c[0] == 16 and c[2] > 1 and c[3] == 0
    assert round_(E0, restore=0) == 0, err()                    # detection alone
    assert host(counts).tolist()[:6] == [0, E0, c[2], 0, 3, 0]
    assert round_(E0) == 0, err()
    assert host(counts).tolist()[:6] == [0, E0, c[2], 1, 3, 0]
    assert round_(E1) == 0, err()
    c = host(counts).tolist()
    assert c[:2] == [0, E1] and c[3:6] == [0, 0, 0]
    out = lambda n: (torch.full((n, 2), -7, dtype=torch.int32, device=DEV), torch.full((R + 1,), -7, dtype=torch.int64, device=DEV),
                     torch.full((R,), -7, dtype=torch.int64, device=DEV))

    def write(n_out, bufs, rings=R, verts=V, null=None, nb=nbytes, c=cell):
        ptrs = [None if null == k else p(t) for k, t in enumerate(bufs)]
        return l.stcd_rings_safe_write(p(vertices), p(offsets), rings, verts, c, n_out, *ptrs, p(counts), p(scratch), nb, stream)

    bufs = out(V)
    for kw in (dict(rings=-1), dict(verts=-1), dict(null=0), dict(null=1), dict(null=2), dict(nb=64), dict(c=7)):
        assert write(E1, bufs, **kw) != 0 and err().startswith("stcd_rings_safe_write: "), kw
    for n_out in (-1, V + 1):
        assert write(n_out, bufs) != 0 and err().startswith("stcd_rings_safe_write: "), n_out
    for n_out in (E1 - 1, E1 + 1, V):                           # could be a count, is not this one: found on the device, nothing written
        assert write(n_out, bufs) == 0, err()
        assert all(bool((t == -7).all()) for t in bufs) and int(counts[0]) & 8, n_out
        assert round_(E1, restore=0) == 0, err()                # a fresh pass clears the bit
        assert int(counts[0]) == 0
    bufs = out(E1)
    assert write(E1, bufs) == 0, err()
    assert int(counts[0]) == 0
    assert_equals_spec(OB.Rings(bufs[0], bufs[1], dev(rs.object), bufs[2], R), want, "raw entries")
    # what the wrapper gives on the same scratch size afterwards
    assert_safe(as_rings(rs), (want, rounds, restored, left), ("after the raw calls", 36, 3.0), cells=(cell,))


def test_end_to_end_on_roofs(tmp_path):
    """Mask -> rings -> safe simplification -> GeoJSON, mask and hulls: valid rings, and no worse a mask than plain Douglas-Peucker's."""
    m = TS.roofs(128, 128, 3)
    src = dev(m * np.uint8(255))
    comps = OB.label_components(src, 8)
    rings = OB.object_rings(comps, 8)
    rs = RS.rings(SP.label(m, 8)[0], 8)
    found = False
    for t in (1.5, 3.0):
        plain, safe = OB.simplify_rings(rings, t), OB.simplify_rings_safe(rings, t)
        want = TS.simplify_safe(rs, OB.simplify_q(t))
        assert_equals_spec(safe.rings, want[0], ("roofs128", t))
        assert safe[1:] == want[1:] and safe.conflicts == 0 and OB.ring_conflicts(safe.rings).count == 0
        found = found or safe.restored > 0
        overlay = dev(m)
        cm_plain, cm_safe = (host(OB.rasterize_rings(r, (128, 128), overlay=overlay).cm) for r in (plain, safe.rings))
        assert cm_safe[0, 1] + cm_safe[1, 0] <= cm_plain[0, 1] + cm_plain[1, 0], (t, cm_safe.tolist(), cm_plain.tolist())
        doc = OB.rings_to_geojson(safe.rings, tmp_path / f"safe_{t}.geojson")
        assert len(doc["features"]) == comps.count
        back = OB.geojson_to_rings(tmp_path / f"safe_{t}.geojson", device=DEV)
        assert back.vertices.shape[0] == safe.rings.vertices.shape[0] and OB.ring_conflicts(back).count == 0
        hulls = OB.convex_hulls(safe.rings)
        assert hulls.count == safe.rings.count and bool((hulls.area2.abs() >= safe.rings.area2.abs()).all())
    assert found, "the scene needs no repair at either tolerance: it proves nothing"
