"""Plain-Python statement of ring simplification (include/stcd_hip.h: stcd_rings_simplify_count, stcd_rings_simplify_write;
stcd_amd/objects.py: simplify_rings): Douglas-Peucker over the rings of tests/rings_spec.py with two anchors per ring, exact integer
keys, lowest-index ties, a triangle at the least and the sign rule.  Python ints only, an explicit stack and no recursion (the comb
ring has 24 578 vertices and a recursion depth of 128, the spiral one of 379), so the device must equal it to the bit.  Also the
three mask patterns the simplification tests add to objects_spec.patterns / rings_spec.patterns, and ``staircase``.

One ring, vertices P[0..n-1] = (y, x), P[n] = P[0], tolerance as q = floor(4 * tolerance^2):

 1. key(p, a, b) = d^2 * L' with d the distance of p from the SEGMENT (a, b), L = |b - a|^2 and L' = L or 1 (``key``).
 2. anchors: vertex 0 and the vertex a1 farthest from it (lowest index on ties); chains [0, a1] and [a1, n].
 3. on a chain [i, j], j - i >= 2: the interior vertex k of largest key against (P[i], P[j]), lowest index on ties, is kept if
    4 * key > q * L', and [i, k], [k, j] are treated the same way; otherwise every interior vertex is dropped.
 4. if nothing but the anchors was kept: also the vertex of largest key against (P[0], P[a1]) among all others, lowest index on
    ties, whatever its key.
 5. area2 of the kept vertices (the formula of rings_spec.rings) is 0 or differs in sign from the input ring's own area2,
    recomputed from the input vertices: the ring is copied whole.  So are rings of fewer than 4 vertices."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests.rings_spec import RingSet

COORD_MAX = 16384                                               # coordinates lie in [0, COORD_MAX]: every key is at most 2^58
Q_MAX = 2 ** 31 - 1


def q_of(tolerance) -> int:
    """floor(4 * tolerance^2), clamped to 2^31 - 1; a tolerance below 0 (or NaN) raises."""
    t = float(tolerance)
    if not t >= 0.0:
        raise ValueError(f"tolerance must be >= 0, got {tolerance!r}")
    v = 4.0 * t * t
    return Q_MAX if v >= Q_MAX else int(math.floor(v))


def seg_len2(a, b) -> int:
    dy, dx = b[0] - a[0], b[1] - a[1]
    return dy * dy + dx * dx


def key(p, a, b) -> int:
    ey, ex = p[0] - a[0], p[1] - a[1]
    dy, dx = b[0] - a[0], b[1] - a[1]
    L = dy * dy + dx * dx
    if L == 0:
        return ey * ey + ex * ex
    t = ey * dy + ex * dx
    if t <= 0:
        return (ey * ey + ex * ex) * L
    if t >= L:
        fy, fx = p[0] - b[0], p[1] - b[1]
        return (fy * fy + fx * fx) * L
    c = ey * dx - ex * dy
    return c * c


def area2_of(P) -> int:
    a = 0
    for (yt, xt), (yh, xh) in zip(P, P[1:] + P[:1]):
        a += xt * yh - xh * yt
    return a


def _argmax_key(P, lo, hi, a, b, skip=()):
    """(index, key) of the largest key among P[lo..hi-1] against (a, b), the lowest index on ties; (-1, -1) for none."""
    best, bk = -1, -1
    for k in range(lo, hi):
        if k in skip:
            continue
        v = key(P[k], a, b)
        if v > bk:
            best, bk = k, v
    return best, bk


def simplify_ring(P, q: int):
    """``(kept indices ascending, rounds, rule)`` for one ring ``P`` (a list of (y, x) tuples of Python ints): rounds is the
    number of level-synchronous rounds a device needs (the recursion depth of step 3 plus the round that splits nothing), rule is
    0, 4 (the triangle rule added a vertex) or 5 (copied whole)."""
    n = len(P)
    assert all(0 <= y <= COORD_MAX and 0 <= x <= COORD_MAX for y, x in P), "coordinate outside [0, 16384]"
    if n < 4:
        return list(range(n)), 0, 5
    a1, far = 0, 0
    for k in range(1, n):
        d = seg_len2(P[0], P[k])
        if d > far:
            a1, far = k, d
    keep = [False] * n
    keep[0] = keep[a1] = True
    depth = 0
    stack = [(0, a1, 1), (a1, n, 1)]
    while stack:
        i, j, level = stack.pop()
        if j - i < 2:
            continue
        depth = max(depth, level)
        a, b = P[i], P[j % n]
        k, v = _argmax_key(P, i + 1, j, a, b)
        if 4 * v > q * (seg_len2(a, b) or 1):
            keep[k] = True
            stack.append((i, k, level + 1))
            stack.append((k, j, level + 1))
    rule = 0
    if sum(keep) == len({0, a1}):
        k, _ = _argmax_key(P, 0, n, P[0], P[a1], skip=(0, a1))
        keep[k] = True
        rule = 4
    kept = [k for k in range(n) if keep[k]]
    a_in, a_out = area2_of(P), area2_of([P[k] for k in kept])
    if a_out == 0 or (a_out > 0) != (a_in > 0):
        return list(range(n)), depth, 5
    return kept, depth, rule


def simplify(rs, q: int, detail=None) -> RingSet:
    """The simplified ``RingSet``; ``detail``, a list, receives ``(kept indices, rounds, rule)`` per ring."""
    vertices = np.asarray(rs.vertices).reshape(-1, 2).tolist()
    offsets = np.asarray(rs.offsets).tolist()
    verts, offs, area2 = [], [0], []
    for r in range(int(rs.count)):
        P = [tuple(v) for v in vertices[offsets[r]:offsets[r + 1]]]
        kept, rounds, rule = simplify_ring(P, q)
        if detail is not None:
            detail.append((kept, rounds, rule))
        ring = [P[k] for k in kept]
        verts.extend(ring)
        offs.append(len(verts))
        area2.append(area2_of(ring))
    return RingSet(np.asarray(verts, np.int32).reshape(-1, 2), np.asarray(offs, np.int64), np.array(rs.object, np.int32),
                   np.asarray(area2, np.int64), int(rs.count))


# the hand-made ring on which the sign rule fires: area2 = 200, returned whole for every q >= 16
SIGN_FLIP_RING = ((8, 0), (8, 100), (10, 100), (10, 55), (0, 55), (0, 45), (10, 45), (10, 0))


def ringset(ring_list, objects=None) -> RingSet:
    """A ``RingSet`` of hand-made rings (lists of (y, x)); area2 is theirs, the objects are 1, 2, ... unless given."""
    verts, offs = [], [0]
    for ring in ring_list:
        verts.extend(tuple(v) for v in ring)
        offs.append(len(verts))
    objects = list(range(1, len(ring_list) + 1)) if objects is None else objects
    return RingSet(np.asarray(verts, np.int32).reshape(-1, 2), np.asarray(offs, np.int64), np.asarray(objects, np.int32),
                   np.asarray([area2_of([tuple(v) for v in ring]) for ring in ring_list], np.int64), len(ring_list))


@functools.lru_cache(maxsize=None)
def staircase(n: int, seed: int = 0):
    """A lattice ring with exactly ``n`` corners (even, >= 4), a tuple of (y, x): from (0, 0) east and south in turn, (n - 2) / 2
    times each, with seeded step sizes in 1..7 so that the keys are not all ties, then west to x = 0 and north home: the travel
    order of an outer ring (area2 > 0)."""
    assert n >= 4 and n % 2 == 0 and 7 * (n - 2) // 2 <= COORD_MAX
    steps = np.random.default_rng(1000 + seed).integers(1, 8, n - 2).tolist()
    ring = [(0, 0)]
    y = x = 0
    for k in range((n - 2) // 2):
        x += steps[2 * k]
        ring.append((y, x))
        y += steps[2 * k + 1]
        ring.append((y, x))
    ring.append((y, 0))
    assert len(ring) == n
    return tuple(ring)


# ------------------------------------------------------------------------------------------------ the three patterns of these tests
@functools.lru_cache(maxsize=None)
def patterns(H: int, W: int):
    """``disks``: seeded discs, some overlapping.  ``rot_rects``: seeded rectangles along integer directions (dy, dx), the
    staircase outlines a rotated roof gives.  ``annulus``: one ring-shaped object round the centre with a disc in its hole.  All
    with integer arithmetic only."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    rng = np.random.default_rng(4242)
    s = max(min(H, W), 2)
    out = {}
    m = np.zeros((H, W), np.uint8)
    for _ in range(max(2, H * W // 900)):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, max(s // 5, 2) + 1))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    out["disks"] = m
    m = np.zeros((H, W), np.uint8)
    for _ in range(max(2, H * W // 1200)):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        dy, dx = int(rng.integers(-5, 6)), int(rng.integers(1, 6))
        a, b = int(rng.integers(1, max(s // 4, 2) + 1)), int(rng.integers(1, max(s // 8, 2) + 1))
        d2 = dy * dy + dx * dx
        u, v = (yy - cy) * dy + (xx - cx) * dx, (yy - cy) * dx - (xx - cx) * dy
        m[(u * u <= a * a * d2) & (v * v <= b * b * d2)] = 1
    out["rot_rects"] = m
    m = np.zeros((H, W), np.uint8)
    cy, cx = H // 2, W // 2
    d2 = (yy - cy) ** 2 + (xx - cx) ** 2
    ro, ri, rc = max(s * 9 // 20, 1), s // 4, s // 10
    m[(d2 <= ro * ro) & (d2 > ri * ri)] = 1
    if rc >= 1 and ri - rc >= 2:
        m[d2 <= rc * rc] = 1
    out["annulus"] = m
    for v in out.values():
        v.setflags(write=False)
    return out
