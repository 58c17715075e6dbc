"""Plain-Python statement of the convex hulls and oriented boxes of rings (include/stcd_hip.h: stcd_rings_hull_count,
stcd_rings_hull_write, stcd_rings_boxes; stcd_amd/objects.py: convex_hulls, oriented_boxes).  Python ints only, so the device must
equal it to the bit.  Also ``convex_ring`` and ``with_midpoints``, the rings that give hulls of any exact size.

Hull of one ring, vertices P[0..n-1] = (y, x) in [0, 16384]:

 1. a coordinate that occurs more than once counts at its lowest index only.
 2. the hull ring is the subsequence of P, in input order, of the STRICT extreme points of the convex hull of the point set: a
    point collinear with its hull neighbours is not one.  Found here on the set (Andrew's monotone chain over the sorted distinct
    points), so the rule does not depend on how a device finds it; ``hull_ring_intervals`` is the index-interval QuickHull a device
    runs, and equals it on rings that do not cross themselves.
 3. area2 is recomputed from the kept vertices (the formula of rings_spec.rings); object, count and ring order are unchanged.
 4. 0, 1 or 2 distinct points, or points all on one line, give 0, 1 or 2 vertices and area2 0.

Oriented box of one hull H[0..h-1]:

 5. h < 3: edge -1 and zeros.
 6. for edge i from H[i] to H[(i + 1) % h]: e = (ey, ex), L = ey^2 + ex^2; for every j: d_j = (H[j] - H[i]) . e and
    z_j = ex (y_j - y_i) - ey (x_j - x_i).  W = max d - min d; Z = max z if max z >= -min z, else min z (on a convex hull all z_j
    have one sign).  The box on edge i has area W |Z| / L.  An edge with L = 0 (no hull has one) is passed over.
 7. the chosen edge has the smallest area, compared exactly (W_i |Z_i| L_b < W_b |Z_b| L_i), the lowest i on ties; no edge with
    L > 0: edge -1 and zeros.
 8. the box: origin H[i], dir e, extent (min d, max d, Z).  With n = (ex, -ey) in (y, x) a point H[i] + a e + b n has d = a L and
    z = b L: the corners are (a, b) = (dmin / L, 0), (dmax / L, 0), (dmax / L, Z / L), (dmin / L, Z / L)."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

from tests.rings_spec import RingSet
from tests.simplify_spec import COORD_MAX, area2_of, ringset, staircase  # noqa: F401  (re-exported for the tests)


class BoxSet(NamedTuple):
    edge: np.ndarray                    # int32 [count]: the hull edge the box stands on, -1 for none
    origin: np.ndarray                  # int32 [count,2]: H[edge] as (y, x)
    dir: np.ndarray                     # int32 [count,2]: (ey, ex)
    extent: np.ndarray                  # int64 [count,3]: (dmin, dmax, Z)
    count: int


def _cross(o, a, b) -> int:
    """> 0 where o -> a -> b turns from +x towards +y."""
    return (a[1] - o[1]) * (b[0] - o[0]) - (a[0] - o[0]) * (b[1] - o[1])


def hull_ring(P):
    """The kept indices, ascending, of one ring ``P`` (a list of (y, x) tuples of Python ints): rules 1, 2 and 4."""
    assert all(0 <= y <= COORD_MAX and 0 <= x <= COORD_MAX for y, x in P), "coordinate outside [0, 16384]"
    first = {}
    for k, p in enumerate(P):
        first.setdefault(p, k)
    pts = sorted(first, key=lambda p: (p[1], p[0]))
    if len(pts) <= 2:
        return sorted(first[p] for p in pts)
    chain = []
    for seq in (pts, pts[::-1]):
        half = []
        for p in seq:
            while len(half) >= 2 and _cross(half[-2], half[-1], p) <= 0:
                half.pop()
            half.append(p)
        chain.extend(half[:-1])
    return sorted(first[p] for p in set(chain))


def hull_ring_intervals(P, detail=None):
    """The same indices by the scheme of the kernels: the anchors are the lexicographic minimum and maximum of (x, y), lowest index
    each; the two chains between them are index intervals in travel order (the second wraps); on a chain the vertex strictly outside
    the chord with the largest |cross| is kept, the first in travel order on ties, and the chain splits there.  "Outside" is decided
    by the sign of the ring's own area2.  ``detail``, a list, receives the number of level-synchronous rounds."""
    n = len(P)
    if n == 0:
        return []
    lo = min(range(n), key=lambda k: (P[k][1], P[k][0], k))
    hi = min(range(n), key=lambda k: (-P[k][1], -P[k][0], k))
    if lo == hi:
        return [lo]
    sign = -1 if area2_of(list(P)) < 0 else 1
    i0, i1 = min(lo, hi), max(lo, hi)
    keep = {i0, i1}
    depth = 0
    stack = [(i0, i1, 1), (i1, i0 + n, 1)]
    while stack:
        i, j, level = stack.pop()
        a, b = P[i % n], P[j % n]
        best, bk = -1, 0
        for k in range(i + 1, j):
            c = -sign * _cross(a, b, P[k % n])
            if c > bk:
                best, bk = k, c
        if best >= 0:
            depth = max(depth, level)
            keep.add(best % n)
            stack.append((i, best, level + 1))
            stack.append((best, j, level + 1))
    if detail is not None:
        detail.append(depth + 1)
    return sorted(keep)


def hulls(rs) -> RingSet:
    """The hull ``RingSet`` of a ``RingSet``."""
    vertices = np.asarray(rs.vertices).reshape(-1, 2).tolist()
    offsets = np.asarray(rs.offsets).tolist()
    verts, offs, area2 = [], [0], []
    for r in range(int(rs.count)):
        P = [tuple(v) for v in vertices[offsets[r]:offsets[r + 1]]]
        ring = [P[k] for k in hull_ring(P)]
        verts.extend(ring)
        offs.append(len(verts))
        area2.append(area2_of(ring))
    return RingSet(np.asarray(verts, np.int32).reshape(-1, 2), np.asarray(offs, np.int64), np.array(rs.object, np.int32),
                   np.asarray(area2, np.int64), int(rs.count))


def box_of(H):
    """``(edge, (y, x), (ey, ex), (dmin, dmax, Z))`` of one hull ``H`` (a sequence of (y, x) tuples): rules 5 to 8.  O(h^2), so a
    result is kept per hull."""
    return _box_of(tuple(H))


@functools.lru_cache(maxsize=None)
def _box_of(H):
    h = len(H)
    none = (-1, (0, 0), (0, 0), (0, 0, 0))
    if h < 3:
        return none
    best, b_area, b_len = none, 0, 0
    for i in range(h):
        (y0, x0), (y1, x1) = H[i], H[(i + 1) % h]
        ey, ex = y1 - y0, x1 - x0
        L = ey * ey + ex * ex
        if L == 0:
            continue
        d = [(y - y0) * ey + (x - x0) * ex for y, x in H]
        z = [ex * (y - y0) - ey * (x - x0) for y, x in H]
        Z = max(z) if max(z) >= -min(z) else min(z)
        A = (max(d) - min(d)) * abs(Z)
        if best[0] < 0 or A * b_len < b_area * L:
            best, b_area, b_len = (i, (y0, x0), (ey, ex), (min(d), max(d), Z)), A, L
    return best


def boxes(hs) -> BoxSet:
    """The ``BoxSet`` of a hull ``RingSet`` (or of any ``RingSet``: the rules do not ask for convexity)."""
    vertices = np.asarray(hs.vertices).reshape(-1, 2).tolist()
    offsets = np.asarray(hs.offsets).tolist()
    rows = [box_of([tuple(v) for v in vertices[offsets[r]:offsets[r + 1]]]) for r in range(int(hs.count))]
    R = len(rows)
    return BoxSet(np.asarray([b[0] for b in rows], np.int32).reshape(R), np.asarray([b[1] for b in rows], np.int32).reshape(R, 2),
                  np.asarray([b[2] for b in rows], np.int32).reshape(R, 2), np.asarray([b[3] for b in rows], np.int64).reshape(R, 3), R)


def is_strictly_convex(H, sign: int) -> bool:
    """Every turn of the closed ring ``H`` (at least 3 vertices) has the sign of ``sign``."""
    h = len(H)
    return h >= 3 and all(_cross(H[k], H[(k + 1) % h], H[(k + 2) % h]) * sign > 0 for k in range(h))


# ------------------------------------------------------------------------------------------------ rings with hulls of an exact size
def _half(v) -> int:
    dy, dx = v
    return 0 if dy < 0 else 2 if dy == 0 and dx < 0 else 1      # atan2(dy, dx) in (-pi, 0), in [0, pi), pi itself


def _by_angle(u, v) -> int:
    hu, hv = _half(u), _half(v)
    if hu != hv:
        return -1 if hu < hv else 1
    c = u[1] * v[0] - u[0] * v[1]                               # > 0: v has the larger angle
    return -1 if c > 0 else 1 if c < 0 else 0


@functools.lru_cache(maxsize=None)
def convex_ring(m: int):
    """A strictly convex outer ring (area2 > 0), a tuple of (y, x): the primitive vectors (dy, dx) with max(|dy|, |dx|) <= m,
    sorted by atan2(dy, dx) ascending (exactly: by half-plane, then by cross product), summed up and shifted to non-negative
    coordinates.  32 / 96 / 368 / 1440 vertices for m = 3 / 6 / 12 / 24; any in-order subsequence of it is strictly convex."""
    vecs = [(dy, dx) for dy in range(-m, m + 1) for dx in range(-m, m + 1) if math.gcd(dy, dx) == 1]
    vecs.sort(key=functools.cmp_to_key(_by_angle))
    ring, y, x = [], 0, 0
    for dy, dx in vecs:
        ring.append((y, x))
        y, x = y + dy, x + dx
    assert (y, x) == (0, 0)
    y0, x0 = min(p[0] for p in ring), min(p[1] for p in ring)
    ring = tuple((p[0] - y0, p[1] - x0) for p in ring)
    assert area2_of(list(ring)) > 0 and is_strictly_convex(ring, 1)
    return ring


def with_midpoints(ring):
    """``ring`` with its coordinates doubled and the midpoint of every edge inserted: the hull is the even positions."""
    out = []
    for (y0, x0), (y1, x1) in zip(ring, ring[1:] + ring[:1]):
        out.append((2 * y0, 2 * x0))
        out.append((y0 + y1, x0 + x1))
    return tuple(out)
