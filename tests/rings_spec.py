"""numpy / plain-Python statement of the boundary rings of a label image (include/stcd_hip.h: stcd_rings_count, stcd_rings_write;
stcd_amd/objects.py: object_rings): the directed unit edges of every object, the successor map with its saddle rule, its cycles
reduced to corners, plus the even-odd fill that inverts them and the two patterns the ring tests add to objects_spec.patterns.
Everything is an integer, so the tests ask for equality.

Lattice: vertex (y, x), 0 <= y <= H, 0 <= x <= W; pixel (i, j) is the unit square between (i, j) and (i + 1, j + 1).  Pixel (i, j)
of object k owns one directed edge per side whose neighbour is not k (outside the scene: not k):

    top     (i, j)         -> (i, j + 1)       dir 0, east
    right   (i, j + 1)     -> (i + 1, j + 1)   dir 1, south
    bottom  (i + 1, j + 1) -> (i + 1, j)       dir 2, west
    left    (i + 1, j)     -> (i, j)           dir 3, north

The key of an edge is (tail y, tail x, dir), ordered lexicographically."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))                      # head - tail of an edge of dir 0..3


class RingSet(NamedTuple):
    vertices: np.ndarray                # int32 [V,2]: (y, x), the corners of all rings, ring after ring
    offsets: np.ndarray                 # int64 [R+1]: ring r is vertices[offsets[r]:offsets[r + 1]]
    object: np.ndarray                  # int32 [R]: the label of the ring's object
    area2: np.ndarray                   # int64 [R]: twice the signed area, positive for an outer ring, negative for a hole
    count: int                          # R


def _owner(y, x, d):
    """The pixel that owns the edge with tail (y, x) and dir d."""
    return ((y, x), (y, x - 1), (y - 1, x - 1), (y - 1, x))[d]


def edges(labels: np.ndarray):
    """``{(tail y, tail x, dir): label}`` over every object pixel's sides whose neighbour carries another label."""
    lab = np.asarray(labels)
    H, W = lab.shape
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = lab
    mid = pad[1:-1, 1:-1]
    out = {}
    # (neighbour, tail offset from the pixel, dir)
    for nb, (ty, tx), d in ((pad[:-2, 1:-1], (0, 0), 0), (pad[1:-1, 2:], (0, 1), 1), (pad[2:, 1:-1], (1, 1), 2), (pad[1:-1, :-2], (1, 0), 3)):
        ys, xs = np.nonzero((mid > 0) & (nb != mid))
        for y, x, k in zip(ys.tolist(), xs.tolist(), mid[ys, xs].tolist()):
            out[(y + ty, x + tx, d)] = k
    return out


def successor(E, key, connectivity):
    """The edge of the same object that leaves the head of ``key``; at a saddle, the one owned by the other pixel under
    connectivity 8 and the one owned by the same pixel under connectivity 4."""
    y, x, d = key
    k = E[key]
    hy, hx = y + STEP[d][0], x + STEP[d][1]
    cand = [(hy, hx, t) for t in range(4) if E.get((hy, hx, t)) == k]
    if len(cand) == 1:
        return cand[0]
    assert len(cand) == 2, (key, cand)
    same = [c for c in cand if _owner(*c) == _owner(y, x, d)]
    other = [c for c in cand if _owner(*c) != _owner(y, x, d)]
    assert len(same) == 1 and len(other) == 1, (key, cand)
    return other[0] if connectivity == 8 else same[0]


def rings(labels: np.ndarray, connectivity: int = 8) -> RingSet:
    assert connectivity in (4, 8)
    E = edges(labels)
    succ = {key: successor(E, key, connectivity) for key in E}
    verts, offsets, objs, area2 = [], [0], [], []
    seen = set()
    for start in sorted(E):                                     # the first edge of a cycle in key order is its smallest
        if start in seen:
            continue
        cycle = [start]
        seen.add(start)
        e = succ[start]
        while e != start:
            assert e not in seen and E[e] == E[start]
            seen.add(e)
            cycle.append(e)
            e = succ[e]
        ring = [(e[0], e[1]) for prev, e in zip([cycle[-1]] + cycle[:-1], cycle) if prev[2] != e[2]]
        assert ring and ring[0] == (start[0], start[1])        # the start edge is a corner
        a = 0
        for (yt, xt), (yh, xh) in zip(ring, ring[1:] + ring[:1]):
            a += xt * yh - xh * yt
        verts.extend(ring)
        offsets.append(len(verts))
        objs.append(E[start])
        area2.append(a)
    return RingSet(np.asarray(verts, np.int32).reshape(-1, 2), np.asarray(offsets, np.int64), np.asarray(objs, np.int32),
                   np.asarray(area2, np.int64), len(objs))


def fill_even_odd(ring_list, H: int, W: int) -> np.ndarray:
    """bool [H,W]: the pixels inside an odd number of the rings (each an ``[n,2]`` array of (y, x) corners).  A pixel's centre lies
    left of a downward or upward vertical side once per crossing: the crossings of a row are toggled and summed along x."""
    toggle = np.zeros((H, W + 1), np.int64)
    for ring in ring_list:
        ring = np.asarray(ring, np.int64).reshape(-1, 2)
        for (y0, x0), (y1, x1) in zip(ring.tolist(), np.roll(ring, -1, axis=0).tolist()):
            if x0 == x1 and y0 != y1:
                toggle[min(y0, y1):max(y0, y1), x0] += 1
    return (np.cumsum(toggle, axis=1)[:, :W] & 1).astype(bool)


# ------------------------------------------------------------------------------------------------ the two patterns of the ring tests
@functools.lru_cache(maxsize=None)
def patterns(H: int, W: int):
    """``nested``: a box, a hole in it, an island in the hole, a hole in the island (what of them fits).  ``comb``: rows 0::3 full,
    rows 1::3 set at even columns, column 0 full: one object whose single ring turns at almost every vertex."""
    m = np.zeros((H, W), np.uint8)
    for k, v in enumerate((1, 0, 1, 0)):
        lo = 1 + 2 * k
        if H - lo > lo and W - lo > lo:
            m[lo:H - lo, lo:W - lo] = v
    out = {"nested": m}
    m = np.zeros((H, W), np.uint8)
    m[0::3, :] = 1
    m[1::3, 0::2] = 1
    m[:, 0] = 1
    out["comb"] = m
    for v in out.values():
        v.setflags(write=False)
    return out
