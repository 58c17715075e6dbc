"""Plain-Python / numpy statement of ring rasterization (include/stcd_hip.h: stcd_rings_raster; stcd_amd/objects.py:
rasterize_rings): rings in the layout of tests/rings_spec.py back to pixels.  Python ints only, so the device must equal it to the bit.

Pixel (i, j) is the unit square between the lattice vertices (i, j) and (i + 1, j + 1), sampled at its centre (i + 1/2, j + 1/2).
Ring r is closed implicitly: edges run from vertex k to vertex k + 1 mod n.  An edge with y0 == y1 contributes nothing.  Another edge
is taken with y0 < y1, dy = y1 - y0 and sign s = +1 if it ran north as stored (y1 < y0 before the swap), else -1; it touches row i
iff y0 <= i < y1 and 0 <= i < H (a row's centre line never passes through a lattice vertex), and there

    num = 2 * x0 * dy + (x1 - x0) * (2 * i + 1 - 2 * y0)       # 2 * dy * (x of the crossing)
    j*  = (num + dy - 1) // (2 * dy)                           # the first j with j + 1/2 >= crossing: a centre ON an edge is right of it
    j*  = min(max(j*, 0), W)                                   # column W is outside the frame
    delta[i][j*] += s

The winding number is w[i][j] = sum of delta[i][0..j]; rule "positive" sets a pixel iff w > 0, rule "evenodd" iff w is odd."""
from __future__ import annotations

import numpy as np

COORD_MAX = 16384                                               # coordinates lie in [0, COORD_MAX], frames are at most COORD_MAX x COORD_MAX
RULES = ("positive", "evenodd")


def ring_list(rings):
    """A list of rings, each a list of (y, x) tuples of Python ints, from a ``RingSet`` / ``Rings`` of arrays or from a list of rings."""
    if hasattr(rings, "offsets"):
        v = np.asarray(rings.vertices).reshape(-1, 2).tolist()
        o = np.asarray(rings.offsets).tolist()
        return [[tuple(p) for p in v[o[r]:o[r + 1]]] for r in range(int(rings.count))]
    return [[(int(p[0]), int(p[1])) for p in np.asarray(ring, np.int64).reshape(-1, 2).tolist()] for ring in rings]


def delta_plane(rings, H: int, W: int) -> np.ndarray:
    """int64 [H, W + 1]: what the edges add."""
    assert 1 <= H <= COORD_MAX and 1 <= W <= COORD_MAX
    delta = np.zeros((H, W + 1), np.int64)
    for ring in ring_list(rings):
        n = len(ring)
        for k in range(n):
            (y0, x0), (y1, x1) = ring[k], ring[(k + 1) % n]
            assert 0 <= min(y0, x0, y1, x1) and max(y0, x0, y1, x1) <= COORD_MAX, "coordinate outside [0, 16384]"
            if y0 == y1:
                continue
            s = -1
            if y1 < y0:
                y0, x0, y1, x1, s = y1, x1, y0, x0, 1
            dy = y1 - y0
            for i in range(y0, min(y1, H)):
                num = 2 * x0 * dy + (x1 - x0) * (2 * i + 1 - 2 * y0)
                assert 0 <= num < 2 ** 31
                j = (num + dy - 1) // (2 * dy)
                delta[i, min(max(j, 0), W)] += s
    return delta


def winding(rings, H: int, W: int) -> np.ndarray:
    """int64 [H,W]: the winding number of every pixel centre."""
    return np.cumsum(delta_plane(rings, H, W), axis=1)[:, :W]


def fill(rings, H: int, W: int, rule: str = "positive") -> np.ndarray:
    """bool [H,W]: the pixels the rule sets."""
    assert rule in RULES
    w = winding(rings, H, W)
    return w > 0 if rule == "positive" else (w & 1).astype(bool)


def confusion(mask, overlay) -> np.ndarray:
    """int64 [2,2]: cm[overlay set, mask set] over the pixels whose overlay byte is not 255; >= 1 is set in both."""
    mask, overlay = np.asarray(mask), np.asarray(overlay)
    assert mask.shape == overlay.shape
    valid = overlay != 255
    lab, pr = (overlay != 0) & valid, (mask != 0) & valid
    return np.array([[np.count_nonzero(valid & ~lab & ~pr), np.count_nonzero(~lab & pr)],
                     [np.count_nonzero(lab & ~pr), np.count_nonzero(lab & pr)]], np.int64)
