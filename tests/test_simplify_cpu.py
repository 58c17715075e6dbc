"""Ring simplification, the part that needs no GPU: the specification of tests/simplify_spec.py has the properties the rule set
promises and gives the pinned vertex totals, the tolerance becomes q as documented, the mirrored thresholds are the kernels', and the
three C-ABI entries exist and refuse bad arguments before any HIP call."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import objects as OB
from tests import objects_spec as SP
from tests import rings_spec as RS
from tests import simplify_spec as SS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = OB.TILE
QS = (0, 1, 4, 9, 16, 64, 400, 2 ** 31 - 1)
ids = lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, T), **RS.patterns(*shape), **SS.patterns(*shape)}      # merged as test_rings_gpu.all_patterns, plus the three


@functools.lru_cache(maxsize=None)
def traced(shape, name, conn):
    rs = RS.rings(SP.label(all_patterns(shape)[name], conn)[0], conn)
    for a in rs[:4]:
        a.setflags(write=False)
    return rs


def ring_of(rs, r):
    return [tuple(v) for v in rs.vertices[rs.offsets[r]:rs.offsets[r + 1]].tolist()]


def is_subsequence(short, long):
    it = iter(long)
    return all(any(v == w for w in it) for v in short)


def check_properties(rs, q, where):
    detail = []
    out = SS.simplify(rs, q, detail)
    assert out.count == rs.count and np.array_equal(out.object, rs.object), where
    assert out.offsets[0] == 0 and out.offsets[-1] == out.vertices.shape[0], where
    for r in range(rs.count):
        P, S = ring_of(rs, r), ring_of(out, r)
        kept, rounds, rule = detail[r]
        assert S == [P[k] for k in kept] and kept[0] == 0 and kept == sorted(set(kept)), (where, r)
        assert is_subsequence(S, P) and S[0] == P[0] and len(S) >= min(3, len(P)), (where, r)
        assert int(out.area2[r]) == SS.area2_of(S) and int(out.area2[r]) != 0, (where, r)
        assert (int(out.area2[r]) > 0) == (int(rs.area2[r]) > 0) and SS.area2_of(P) == int(rs.area2[r]), (where, r)
        assert rounds <= len(P), (where, r)
        if rule == 5:
            assert S == P, (where, r)
        if rule == 0:                                           # every dropped vertex lies within the tolerance of the side that replaces it
            n = len(P)
            for i, j in zip(kept, kept[1:] + [n]):
                a, b = P[i], P[j % n]
                for k in range(i + 1, j):
                    assert 4 * SS.key(P[k], a, b) <= q * (SS.seg_len2(a, b) or 1), (where, r, k)
    return out


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", [(37, 131), (65, 65)], ids=ids)
def test_spec_properties_on_the_patterns(shape, conn):
    for name in all_patterns(shape):
        rs = traced(shape, name, conn)
        for q in QS:
            out = check_properties(rs, q, (name, q))
            if q == 0:                                          # on a lattice outline no corner lies on the segment between two others of its chain
                assert np.array_equal(out.vertices, rs.vertices) and np.array_equal(out.offsets, rs.offsets) and np.array_equal(out.area2, rs.area2), name


def test_q_zero_is_the_identity_at_192():
    shape = (192, 192)
    for name in all_patterns(shape):
        rs = traced(shape, name, 8)
        out = SS.simplify(rs, 0)
        assert np.array_equal(out.vertices, rs.vertices) and np.array_equal(out.offsets, rs.offsets) and np.array_equal(out.area2, rs.area2), name


# computed on the CPU with these rules at 192 x 192, labels and rings both at connectivity 8
PINNED = [("comb", 4, 24578, 256), ("comb", 16, 24578, 129), ("comb", 2 ** 31 - 1, 24578, 3), ("spiral", 4, 386, 383), ("spiral", 16, 386, 381),
          ("serpentine", 4, 386, 288), ("serpentine", 16, 386, 287), ("noise_0.407", 4, 26972, 10754), ("noise_0.407", 16, 26972, 7541),
          ("noise_0.407", 2 ** 31 - 1, 26972, 4815), ("noise_0.593", 4, 27122, 13922), ("checkerboard", 4, 73728, 54154)]


@pytest.mark.parametrize("name,q,before,after", PINNED, ids=[f"{p[0]}-q{p[1]}" for p in PINNED])
def test_pinned_vertex_totals(name, q, before, after):
    rs = traced((192, 192), name, 8)
    assert rs.vertices.shape[0] == before
    assert SS.simplify(rs, q).vertices.shape[0] == after


def test_depth_is_not_logarithmic():
    """Why every ring iterates its own levels inside one kernel: the levels of the spiral and of the comb at 192 x 192."""
    for name, q, n, least in (("spiral", 16, 386, 370), ("comb", 16, 24578, 120)):
        detail = []
        SS.simplify(traced((192, 192), name, 8), q, detail)
        assert len(detail) == 1 and len(detail[0][0]) < n and detail[0][1] >= least, (name, detail[0][1])


def test_the_sign_rule_fires_on_the_hand_made_ring():
    ring = list(SS.SIGN_FLIP_RING)
    rs = SS.ringset([ring])
    assert rs.area2.tolist() == [200]
    for q in (16, 64, 400, 2 ** 31 - 1):
        detail = []
        out = SS.simplify(rs, q, detail)
        assert ring_of(out, 0) == ring and out.area2.tolist() == [200] and detail[0][2] == 5, q
    for q in (0, 4):
        detail = []
        out = SS.simplify(rs, q, detail)
        assert is_subsequence(ring_of(out, 0), ring) and detail[0][2] == 0 and out.area2[0] > 0, q
    # short and degenerate rings are copied whole
    for ring in ([(0, 0), (0, 5), (5, 5)], [(1, 1), (1, 1), (1, 1), (1, 1), (1, 1)], [(0, 0), (0, 3), (0, 6), (0, 3)], []):
        assert ring_of(SS.simplify(SS.ringset([ring]), 4), 0) == ring


def test_staircase_has_n_corners():
    for n in (4, 6, 62, 64, 66, 2046, 2048, 2050):
        ring = list(SS.staircase(n))
        assert len(ring) == n == len(set(ring)) and SS.area2_of(ring) > 0
        closed = ring + ring[:1]
        steps = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(closed, closed[1:])]
        assert all((dy == 0) != (dx == 0) for dy, dx in steps)                              # axis-parallel sides
        assert all((s[0] == 0) != (t[0] == 0) for s, t in zip(steps, steps[1:] + steps[:1]))  # and a turn at every vertex
        assert all(0 <= y <= SS.COORD_MAX and 0 <= x <= SS.COORD_MAX for y, x in ring)
    assert SS.staircase(66, 0) != SS.staircase(66, 1)
    check_properties(SS.ringset([SS.staircase(66), SS.staircase(4, 1), SS.staircase(200, 2)]), 64, "staircases")


def test_tolerance_becomes_q():
    for f in (SS.q_of, OB.simplify_q):
        assert [f(t) for t in (0, 0.4, 0.5, 1.0, 1.5, 2.0, 10)] == [0, 0, 1, 4, 9, 16, 400]
        assert f(1e9) == 2 ** 31 - 1 and f(float("inf")) == 2 ** 31 - 1 and f(23170.0) == 4 * 23170 ** 2 < 2 ** 31 - 1 == f(23171.0)
    for bad in (-1, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            SS.q_of(bad)
        with pytest.raises(_lib.StcdError):
            OB.simplify_q(bad)


def test_thresholds_mirror_the_kernels():
    text = open(os.path.join(REPO, "stcd_amd", "csrc", "kernels_simplify.hip")).read()
    assert int(re.search(r"#define SM_WAVE_MAX (\d+)", text).group(1)) == OB.SIMPLIFY_WAVE_MAX
    assert int(re.search(r"#define SM_LDS_MAX (\d+)", text).group(1)) == OB.SIMPLIFY_LDS_MAX
    assert int(re.search(r"#define SM_COORD_MAX (\d+)", text).group(1)) == SS.COORD_MAX
    assert 4 <= OB.SIMPLIFY_WAVE_MAX < OB.SIMPLIFY_LDS_MAX and OB.SIMPLIFY_WAVE_MAX % 2 == 0 and OB.SIMPLIFY_LDS_MAX % 2 == 0


# ------------------------------------------------------------------------------------------------ the C entries' argument checks
def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    declared = set(re.findall(r"\b(stcd_[a-z0-9_]+)\s*\(", hdr))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("stcd_rings_simplify_scratch_bytes", "stcd_rings_simplify_count", "stcd_rings_simplify_write"):
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name)
    assert _lib.lib().stcd_abi_version() == 2                   # additions only


def _bytes(rings=3, verts=20):
    return int(_lib.lib().stcd_rings_simplify_scratch_bytes(rings, verts))


def test_scratch_bytes():
    assert _bytes(0, 0) >= 48 and _bytes(0, 0) % 8 == 0
    assert 29 * 100000 <= _bytes(0, 100000) - _bytes(0, 0) <= 29 * 100000 + 8 * 26 + 64
    assert 12 * 1000 <= _bytes(1000, 0) - _bytes(0, 0) <= 12 * 1000 + 16
    assert _bytes(-1, 4) == 0 and _bytes(4, -1) == 0 and _bytes(1 << 31, 4) == 0 and _bytes(4, 1 << 31) == 0


def _host():
    """HOST buffers: every call here is refused before any HIP call."""
    buf = np.zeros(65536, np.int64)
    return buf, buf.ctypes.data


def _count_call(rings=3, verts=20, q=9, null=None, short=0, odd=0):
    buf, base = _host()
    p = lambda name, off: None if null == name else C.c_void_p(base + off)
    rc = _lib.lib().stcd_rings_simplify_count(p("vertices", 0), p("offsets", 1024), rings, verts, q, p("counts", 2048 + odd), p("scratch", 8192),
                                              max(_bytes(rings, verts), 8) - short, None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(null="vertices"), dict(null="offsets"), dict(null="counts"), dict(null="scratch"), dict(rings=-1), dict(verts=-1),
                                dict(rings=1 << 31), dict(verts=1 << 31), dict(q=-1), dict(q=1 << 31), dict(short=8), dict(odd=4)])
def test_count_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _count_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_rings_simplify_count: "), err


def _write_call(rings=3, verts=20, q=9, n_out=12, null=None, short=0, odd=0):
    buf, base = _host()
    p = lambda name, off: None if null == name else C.c_void_p(base + off)
    rc = _lib.lib().stcd_rings_simplify_write(p("vertices", 0), p("offsets", 1024), rings, verts, q, n_out, p("out_vertices", 2048 + odd),
                                              p("out_offsets", 3072), p("out_area2", 4096), p("scratch", 8192), max(_bytes(rings, verts), 8) - short, None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(null="vertices"), dict(null="offsets"), dict(null="out_vertices"), dict(null="out_offsets"), dict(null="out_area2"),
                                dict(null="scratch"), dict(rings=-1), dict(verts=-1), dict(rings=1 << 31), dict(verts=1 << 31), dict(q=-1), dict(q=1 << 31),
                                dict(short=8), dict(odd=4), dict(n_out=-1), dict(n_out=21)])
def test_write_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _write_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_rings_simplify_write: "), err


def test_wrapper_refuses_what_is_not_a_ring_set_on_the_gpu():
    rs = SS.ringset([SS.staircase(8)])
    cpu = OB.Rings(*(torch.from_numpy(np.ascontiguousarray(a)) for a in rs[:4]), rs.count)
    with pytest.raises(_lib.StcdError):
        OB.simplify_rings(cpu)
    with pytest.raises(_lib.StcdError):
        OB.simplify_rings(rs)                                   # numpy arrays
    with pytest.raises(_lib.StcdError):
        OB.simplify_rings(cpu, tolerance=-1.0)
