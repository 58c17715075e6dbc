"""The topology rules without a GPU: tests/topology_spec.py against itself, on the inputs the GPU tests use, so that those tests
compare the device with a specification that is known to do what it says: traced rings have no conflict, plain Douglas-Peucker does
break topology on the pinned cases, the repair loop ends with no conflict, unchanged crossing parities, subsequences and right
areas, and at least one case needs several rounds.  Also the new C symbols and the constants the wrapper mirrors."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import objects_spec as SP
from tests import rings_spec as RS
from tests import simplify_spec as SS
from tests import topology_spec as TS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = OB.TILE


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    noise = {k: v for k, v in SP.patterns(*shape, T).items() if k.startswith("noise")}
    return {**RS.patterns(*shape), **SS.patterns(*shape), **noise}


@functools.lru_cache(maxsize=None)
def traced_mask(key, conn):
    kind, arg = key
    m = {"dent": lambda: TS.dent_mask(arg), "noise": lambda: SP.patterns(64, 64, T)["noise_0.593"], "roofs": lambda: TS.roofs(96, 96, arg)}[kind]()
    lab, _ = SP.label(m, conn)
    return RS.rings(lab, conn)


@functools.lru_cache(maxsize=None)
def safe(key, conn, q, max_rounds=None):
    detail = {}
    return TS.simplify_safe(traced_mask(key, conn), q, max_rounds, detail) + (detail,)


@pytest.mark.parametrize("shape,conn", [((37, 131), 8), ((65, 65), 8), ((65, 65), 4)])
def test_traced_rings_have_no_conflict(shape, conn):
    for name, m in all_patterns(shape).items():
        lab, _ = SP.label(m, conn)
        flags, pairs = TS.conflicts(RS.rings(lab, conn))
        assert not flags.any() and not pairs, name


def test_the_conflict_rule_on_hand_made_edges():
    c = TS.conflict
    assert c((0, 0), (4, 4), (0, 4), (4, 0))                                        # a proper crossing
    assert c((0, 0), (0, 8), (0, 4), (5, 4)) and c((0, 4), (5, 4), (0, 0), (0, 8))  # a vertex inside another edge
    assert c((0, 0), (0, 8), (0, 4), (0, 12)) and not c((0, 0), (0, 4), (0, 4), (0, 8))     # collinear: overlap, contact at a vertex
    assert c((0, 0), (0, 8), (0, 8), (0, 3))                                        # a spike: consecutive edges that fold back
    assert not c((0, 0), (0, 8), (0, 8), (5, 8)) and not c((0, 0), (4, 4), (4, 4), (0, 8))  # contact at a vertex of both
    assert not c((0, 0), (0, 0), (0, 0), (3, 3)) and not c((1, 1), (1, 1), (0, 0), (2, 2))  # a zero-length edge
    assert not c((0, 0), (0, 8), (1, 0), (1, 8)) and not c((0, 0), (4, 4), (0, 5), (4, 9))  # apart
    assert not c((0, 0), (4, 4), (4, 4), (8, 0))                                    # the known limit's building block: a shared vertex


def test_the_dents():
    for kind, plain_n, pairs_n, hits0, safe_n in (("cross", 8, 2, 0, 9), ("jump", 7, 0, 1, 8)):
        rs = traced_mask(("dent", kind), 8)
        assert rs.vertices.shape[0] == 12
        plain = SS.simplify(rs, 36)
        flags, pairs = TS.conflicts(plain)
        assert plain.vertices.shape[0] == plain_n and len(pairs) == pairs_n and bool(flags.any()) == (pairs_n > 0)
        out, rounds, restored, left, detail = safe(("dent", kind), 8, 36)
        assert detail["hits"][0] == hits0 and out.vertices.shape[0] == safe_n and (rounds, restored, left) == (1, 1, 0)
        # at tolerance 2.0 nothing is flagged and the result is plain Douglas-Peucker's
        out, rounds, restored, left, detail = safe(("dent", kind), 8, 16)
        want = SS.simplify(rs, 16)
        assert (rounds, restored, left) == (0, 0, 0) and detail["flagged"] == [0] and detail["hits"] == [0]
        assert all(np.array_equal(a, b) for a, b in zip(out[:4], want[:4]))


# (case, connectivity, q): plain Douglas-Peucker's conflict-flagged edges and pocket hits, then rounds and restored vertices
PINNED = [(("noise", 0), 8, 9, 55, 156, 13, 337), (("noise", 0), 8, 36, 76, 147, 19, 440),
          (("roofs", 0), 8, 9, 0, 2, 12, 13), (("roofs", 0), 8, 36, 0, 2, 13, 14)]


@pytest.mark.parametrize("key,conn,q,flagged,hits,rounds,restored", PINNED, ids=[f"{k[0]}-q{q}" for k, _, q, *_ in PINNED])
def test_plain_simplification_breaks_topology_and_the_repair_mends_it(key, conn, q, flagged, hits, rounds, restored):
    rs = traced_mask(key, conn)
    out, n_rounds, n_restored, left, detail = safe(key, conn, q)
    assert detail["flagged"][0] + detail["hits"][0] > 0                 # a case that needs no repair proves nothing
    assert (detail["flagged"][0], detail["hits"][0], n_rounds, n_restored) == (flagged, hits, rounds, restored)
    assert n_rounds >= 2 and left == 0
    assert not TS.conflicts(out)[0].any()
    assert TS.parities(out) == TS.parities(rs)
    assert out.count == rs.count and np.array_equal(out.object, rs.object)
    for r, (P, K, S) in enumerate(zip(TS.ring_lists(rs), detail["kept"], TS.ring_lists(out))):
        assert K[0] == 0 and K == sorted(set(K)) and [P[k] for k in K] == S
        assert set(detail["plain"][r]) <= set(K)
        assert int(out.area2[r]) == SS.area2_of(S) and (SS.area2_of(S) > 0) == (SS.area2_of(P) > 0)
    assert n_restored == out.vertices.shape[0] - SS.simplify(rs, q).vertices.shape[0]


def test_plain_simplification_moves_parities_where_the_repair_does_not():
    """What the parity check above is worth: on the jump dent plain Douglas-Peucker changes one."""
    rs = traced_mask(("dent", "jump"), 8)
    assert TS.parities(SS.simplify(rs, 36)) != TS.parities(rs)
    assert TS.parities(safe(("dent", "jump"), 8, 36)[0]) == TS.parities(rs)


def test_the_round_cap():
    full = safe(("noise", 0), 8, 9)
    capped = safe(("noise", 0), 8, 9, 1)
    assert capped[1] == 1 and capped[3] == full[4]["flagged"][1] == 21 and 0 < capped[2] < full[2]
    none = safe(("noise", 0), 8, 9, 0)
    assert none[1] == 0 and none[2] == 0 and none[3] == 55
    assert np.array_equal(none[0].vertices, SS.simplify(traced_mask(("noise", 0), 8), 9).vertices)


def test_foreign_rings_that_cross_already_still_end():
    rs = SS.ringset([[(0, 0), (0, 20), (20, 20), (20, 0)], [(10, 10), (10, 30), (30, 30), (30, 10)]])
    out, rounds, restored, left = TS.simplify_safe(rs, 9)
    assert left == 4 and rounds == 0 and np.array_equal(out.vertices, rs.vertices)
    stairs = SS.ringset([list(SS.staircase(40, 0)), [(y + 5, x + 5) for y, x in SS.staircase(40, 1)]])
    assert TS.conflicts(stairs)[0].any()
    out, rounds, restored, left = TS.simplify_safe(stairs, 36)
    assert left > 0 and rounds >= 1


def test_the_fan_and_the_long_chains():
    for n in (OB.TOPO_TILE - 1, OB.TOPO_TILE, OB.TOPO_TILE + 1):
        rings = TS.fan(n)
        assert len(rings) == n and len({(r[0], r[1]) for r in rings}) == n
        flags, _ = TS.conflicts(SS.ringset(rings))
        assert flags.reshape(n, 3)[:, 0].all()                          # every edge through the centre conflicts


def test_the_new_symbols_and_the_mirrored_constants():
    src = open(os.path.join(REPO, "stcd_amd", "csrc", "kernels_topo.hip")).read()
    assert f"#define TP_TILE {OB.TOPO_TILE} " in src and f"#define TP_CELL_DEFAULT {OB.TOPO_CELL}\n" in src
    header = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    protos = {"stcd_rings_topo_scratch_bytes": 3, "stcd_rings_conflicts": 12, "stcd_rings_safe_begin": 10, "stcd_rings_safe_round": 13,
              "stcd_rings_safe_write": 13}
    for name, nargs in protos.items():
        assert hasattr(raw, name) and name in _lib.EXPORTS, name
        assert len(_lib._PROTOS[name][1]) == nargs, name
        decl = header[header.index(f" {name}("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == nargs, (name, decl)               # the header declares as many arguments as the binding passes
    l = _lib.lib()
    assert l.stcd_rings_topo_scratch_bytes(-1, 0, 0) == 0 and l.stcd_rings_topo_scratch_bytes(0, 1 << 31, 0) == 0
    for cell in (3, 4, 12, 512, -8):
        assert l.stcd_rings_topo_scratch_bytes(3, 100, cell) == 0, cell
    sizes = [l.stcd_rings_topo_scratch_bytes(3, 100, cell) for cell in OB.TOPO_CELLS]
    assert sizes[0] == sizes[OB.TOPO_CELLS.index(OB.TOPO_CELL)] and all(a > b > 0 for a, b in zip(sizes[1:], sizes[2:]))
    assert l.stcd_rings_topo_scratch_bytes(3, 100, 256) >= l.stcd_rings_simplify_scratch_bytes(3, 100) + 64
