"""Plain-Python statement of the topology rules over rings (include/stcd_hip.h: stcd_rings_conflicts, stcd_rings_safe_begin /
_round / _write; stcd_amd/objects.py: ring_conflicts, simplify_rings_safe): which edges of a ring set conflict, when the pocket of a
simplified edge is hit, and the repair loop that restores vertices until neither happens.  Python ints only and every pair is looked
at (numpy is used for one necessary condition alone: two closed segments that share a point have bounding boxes that share one), so the
device must equal it to the bit and nothing here knows of a grid.

Rings are those of tests/rings_spec.py: P[0..n-1] = (y, x), closed implicitly.  Edge k of ring r runs from P[k] to P[(k + 1) % n] and
has the global index offsets[r] + k.  orient(a, b, c) = (b.y - a.y)(c.x - a.x) - (b.x - a.x)(c.y - a.y), below 2^30 in magnitude for
coordinates in [0, 16384].

CONFLICT of two distinct edges (a, b) and (c, d), of one ring or of two (``conflict``):
 1. a zero-length edge conflicts with nothing.
 2. all four orientations 0 (collinear): iff the overlap of the two edges along the axis in which a and b differ has positive length.
 3. otherwise: no endpoint value may be common to both (a != c, a != d, b != c, b != d), and the closed segments must share a point:
    both orientation sign products are negative, or one orientation is 0 and that point lies in the other edge's bounding box.
So proper crossings, a vertex inside another edge, collinear overlaps and spikes conflict; contact at a vertex of both does not
(consecutive edges, the pinch corners of traced rings).  Known limit: a crossing exactly through a vertex both rings share is not seen.

POCKET HIT.  A current edge from kept vertex i to the next kept vertex j (j = n for the edge that closes the ring: vertex 0 is always
kept) with j - i >= 2 has the pocket P[i], P[i + 1], ..., P[j % n], a closed polygon.  The edge is hit iff the first vertex of any
OTHER ring lies on the pocket's boundary (orientation 0 against one of its sides and within that side's bounding box) or inside it:
the number of sides (u, v), taken with u.y < v.y, with u.y <= p.y < v.y (the half-open row rule of tests/raster_spec.py) and
(v.x - u.x)(p.y - u.y) > (p.x - u.x)(v.y - u.y) (the side passes right of p) is odd (``pocket_hit``).

TOPOLOGY-SAFE SIMPLIFICATION at q (``simplify_safe``):
 1. round 0: simplify_spec.simplify_ring per ring, a keep mask over the input vertices.
 2. a round flags every current edge that conflicts with another current edge or whose pocket is hit.
 3. every flagged edge with dropped vertices restores the vertex of largest simplify_spec.key against (P[i], P[j % n]) among
    i + 1 .. j - 1, lowest index on ties; all restores of a round at once.
 4. every ring whose mask changed: kept area2 0 or of another sign than the input's -> all of its vertices are kept.
 5. repeat from 2 until a round restores nothing; with ``max_rounds`` rounds done, one more detection and no restore.
The result has the same rings in the same order, each a subsequence of its input with vertex 0 kept, area2 recomputed; ``rounds``
counts the rounds that restored something, ``restored`` the vertices kept beyond round 0's, ``conflicts`` the edges of the result that
rule CONFLICT flags (0 for conflict-free input without a cap)."""
from __future__ import annotations

import functools

import numpy as np

from tests import simplify_spec as SS
from tests.rings_spec import RingSet

COORD_MAX = SS.COORD_MAX


def orient(a, b, c) -> int:
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def in_box(p, a, b) -> bool:
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def conflict(a, b, c, d) -> bool:
    """Rule CONFLICT for the edges (a, b) and (c, d)."""
    if a == b or c == d:
        return False
    o1, o2, o3, o4 = orient(a, b, c), orient(a, b, d), orient(c, d, a), orient(c, d, b)
    if o1 == 0 and o2 == 0 and o3 == 0 and o4 == 0:
        ax = 0 if a[0] != b[0] else 1
        return min(max(a[ax], b[ax]), max(c[ax], d[ax])) - max(min(a[ax], b[ax]), min(c[ax], d[ax])) > 0
    if a == c or a == d or b == c or b == d:
        return False
    if ((o1 < 0 < o2) or (o2 < 0 < o1)) and ((o3 < 0 < o4) or (o4 < 0 < o3)):
        return True
    return (o1 == 0 and in_box(c, a, b)) or (o2 == 0 and in_box(d, a, b)) or (o3 == 0 and in_box(a, c, d)) or (o4 == 0 and in_box(b, c, d))


def ring_lists(rs):
    """A list of rings, each a list of (y, x) tuples of Python ints."""
    v = np.asarray(rs.vertices).reshape(-1, 2).tolist()
    o = np.asarray(rs.offsets).tolist()
    return [[tuple(p) for p in v[o[r]:o[r + 1]]] for r in range(int(rs.count))]


def edge_flags(edges):
    """``(flags, pairs)`` for a list of edges ``(a, b)``: flags[e] is 1 iff edge e conflicts with any other, pairs the set of (e, f),
    e < f, that do."""
    E = len(edges)
    flags = [0] * E
    pairs = set()
    if E == 0:
        return flags, pairs
    arr = np.asarray(edges, np.int64).reshape(E, 4)                 # ay, ax, by, bx
    ylo, yhi = np.minimum(arr[:, 0], arr[:, 2]), np.maximum(arr[:, 0], arr[:, 2])
    xlo, xhi = np.minimum(arr[:, 1], arr[:, 3]), np.maximum(arr[:, 1], arr[:, 3])
    for e in range(E):
        near = np.nonzero((ylo[e + 1:] <= yhi[e]) & (yhi[e + 1:] >= ylo[e]) & (xlo[e + 1:] <= xhi[e]) & (xhi[e + 1:] >= xlo[e]))[0]
        a, b = edges[e]
        for f in (near + e + 1).tolist():
            if conflict(a, b, *edges[f]):
                flags[e] = flags[f] = 1
                pairs.add((e, f))
    return flags, pairs


def conflicts(rs):
    """``(flags uint8 [V], pairs)`` over every edge of the ring set, in the order of the vertices."""
    edges = []
    for P in ring_lists(rs):
        n = len(P)
        edges.extend((P[k], P[(k + 1) % n]) for k in range(n))
    flags, pairs = edge_flags(edges)
    return np.asarray(flags, np.uint8), pairs


def on_or_inside(p, Q) -> bool:
    """p on the boundary of the closed polygon Q or inside it (rule POCKET HIT)."""
    m = len(Q)
    odd = False
    for k in range(m):
        u, v = Q[k], Q[(k + 1) % m]
        if orient(u, v, p) == 0 and in_box(p, u, v):
            return True
        if u[0] == v[0]:
            continue
        if u[0] > v[0]:
            u, v = v, u
        if u[0] <= p[0] < v[0] and (v[1] - u[1]) * (p[0] - u[0]) > (p[1] - u[1]) * (v[0] - u[0]):
            odd = not odd
    return odd


def crossing_parity(p, Q) -> int:
    """The crossing number of the closed polygon Q around p, mod 2 (the inside half of ``on_or_inside`` alone)."""
    m = len(Q)
    odd = 0
    for k in range(m):
        u, v = Q[k], Q[(k + 1) % m]
        if u[0] == v[0]:
            continue
        if u[0] > v[0]:
            u, v = v, u
        if u[0] <= p[0] < v[0] and (v[1] - u[1]) * (p[0] - u[0]) > (p[1] - u[1]) * (v[0] - u[0]):
            odd ^= 1
    return odd


def current_edges(rings, kept):
    """``[(ring, i, j)]`` over the current edges in the order of their first vertices; j = n closes the ring."""
    out = []
    for r, (P, K) in enumerate(zip(rings, kept)):
        for t, i in enumerate(K):
            out.append((r, i, K[t + 1] if t + 1 < len(K) else len(P)))
    return out


def pocket_hit(rings, r, i, j) -> bool:
    P = rings[r]
    n = len(P)
    if j - i < 2:
        return False
    Q = [P[k % n] for k in range(i, j + 1)]
    y0, y1 = min(p[0] for p in Q), max(p[0] for p in Q)
    x0, x1 = min(p[1] for p in Q), max(p[1] for p in Q)
    for s, S in enumerate(rings):
        if s == r or not S:
            continue
        p = S[0]
        if y0 <= p[0] <= y1 and x0 <= p[1] <= x1 and on_or_inside(p, Q):
            return True
    return False


def detect(rings, kept):
    """``(edges, conflict flags, pocket flags)`` of the current state."""
    cur = current_edges(rings, kept)
    cflags, _ = edge_flags([(rings[r][i], rings[r][j % len(rings[r])]) for r, i, j in cur])
    pflags = [1 if pocket_hit(rings, r, i, j) else 0 for r, i, j in cur]
    return cur, cflags, pflags


def simplify_safe(rs, q: int, max_rounds=None, detail=None):
    """``(RingSet, rounds, restored, conflicts)``; ``detail``, a dict, receives ``kept`` (the kept indices per ring), ``plain`` (round
    0's), and per detection pass the number of conflict-flagged and of pocket-hit edges (``flagged``, ``hits``)."""
    rings = ring_lists(rs)
    plain = [SS.simplify_ring(P, q)[0] for P in rings]
    kept = [list(K) for K in plain]
    a_in = [SS.area2_of(P) for P in rings]
    rounds = 0
    flagged, hits = [], []
    while True:
        cur, cflags, pflags = detect(rings, kept)
        flagged.append(sum(cflags))
        hits.append(sum(pflags))
        if max_rounds is not None and rounds >= max_rounds:
            break
        add = [set() for _ in rings]
        for (r, i, j), c, p in zip(cur, cflags, pflags):
            if (c or p) and j - i >= 2:
                P = rings[r]
                k, _ = SS._argmax_key(P, i + 1, j, P[i], P[j % len(P)])
                add[r].add(k)
        if not any(add):
            break
        for r, A in enumerate(add):
            if A:
                K = sorted(set(kept[r]) | A)
                a_out = SS.area2_of([rings[r][k] for k in K])
                if a_out == 0 or (a_out > 0) != (a_in[r] > 0):
                    K = list(range(len(rings[r])))
                kept[r] = K
        rounds += 1
    verts, offs, area2 = [], [0], []
    for P, K in zip(rings, kept):
        ring = [P[k] for k in K]
        verts.extend(ring)
        offs.append(len(verts))
        area2.append(SS.area2_of(ring))
    out = RingSet(np.asarray(verts, np.int32).reshape(-1, 2), np.asarray(offs, np.int64), np.array(rs.object, np.int32),
                  np.asarray(area2, np.int64), int(rs.count))
    if detail is not None:
        detail.update(kept=kept, plain=plain, flagged=flagged, hits=hits)
    restored = sum(len(K) for K in kept) - sum(len(K) for K in plain)
    return out, rounds, restored, flagged[-1]


def parities(rs):
    """The crossing parity of every ring around every other ring's first vertex: a tuple of R tuples."""
    rings = ring_lists(rs)
    return tuple(tuple(crossing_parity(S[0], P) if s != r and S else 0 for s, S in enumerate(rings)) for r, P in enumerate(rings))


# ------------------------------------------------------------------------------------------------ the masks of these tests
def dent_mask(kind: str) -> np.ndarray:
    """A block with a 3-pixel dent and a small object in it: ``cross`` stands in the dent and reaches out of it, ``jump`` lies wholly
    inside.  At tolerance 3.0 plain Douglas-Peucker crosses the first and jumps over the second; at 2.0 it does neither."""
    m = np.zeros((40, 40), np.uint8)
    m[2:31, 2:38] = 1
    m[2:5, 10:21] = 0
    if kind == "cross":
        m[0:4, 12:19] = 1
    else:
        assert kind == "jump"
        m[3, 12:19] = 1
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def roofs(H: int, W: int, seed: int = 0) -> np.ndarray:
    """About H * W / 384 seeded rectangles along integer directions, the outlines rotated roofs give; integer arithmetic only."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    rng = np.random.default_rng(7000 + seed)
    s = max(min(H, W), 2)
    m = np.zeros((H, W), np.uint8)
    for _ in range(max(2, H * W // 384)):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        dy, dx = int(rng.integers(-5, 6)), int(rng.integers(1, 6))
        a, b = int(rng.integers(2, max(s // 8, 3) + 1)), int(rng.integers(2, max(s // 16, 3) + 1))
        d2 = dy * dy + dx * dx
        u, v = (yy - cy) * dy + (xx - cx) * dx, (yy - cy) * dx - (xx - cx) * dy
        m[(u * u <= a * a * d2) & (v * v <= b * b * d2)] = 1
    m.setflags(write=False)
    return m


def fan(n: int, centre=(100, 100)):
    """n rings of 3 vertices whose first edges all pass through ``centre``: short edges along n distinct directions, one grid cell
    holding all of them.  Every first edge conflicts with every other."""
    rings = []
    cy, cx = centre
    d = 1
    while len(rings) < n:
        for dy, dx in ((d, 1), (d, -1), (1, d), (1, -d)) if d > 1 else ((1, 1), (1, -1)):
            if len(rings) < n:                                      # from centre - (dy, dx) to centre + (dy, dx), then one step east
                rings.append([(cy - dy, cx - dx), (cy + dy, cx + dx), (cy + dy, cx + dx + 1)])
        d += 1
    assert d <= min(cy, cx)
    return rings
