"""numpy statement of the change objects (include/stcd_hip.h: stcd_objects_label, stcd_objects_table, stcd_mask_filter_objects;
stcd_amd/objects.py: match_objects): run-based two-pass union-find, raster-order numbering, the table, the two-step filter and
the matching, plus the masks the CPU and the GPU tests share.  Everything is an integer, so the tests ask for equality."""
from __future__ import annotations

import functools

import numpy as np


# ------------------------------------------------------------------------------------------------ labelling
def label(mask: np.ndarray, connectivity: int = 8, invert: bool = False):
    """``(labels int32 [H,W], n)``: 0 background, 1..n the components of the non-zero (``invert``: zero) pixels, numbered in
    raster order of each component's first pixel.  First pass: the runs of every row, in raster order; runs of neighbouring rows
    that touch (8: also diagonally) are united, the smaller run index becoming the root.  Second pass: the roots are numbered in
    run order (a root is its component's first run, which starts at the component's first pixel) and every run is painted."""
    assert connectivity in (4, 8)
    m = (np.asarray(mask) != 0) != bool(invert)
    H, W = m.shape
    pad = np.zeros((H, W + 2), np.int8)
    pad[:, 1:-1] = m
    d = np.diff(pad, axis=1)                                    # [H,W+1]: +1 where a run starts, -1 at its exclusive end
    ry, rs = np.nonzero(d == 1)
    re = np.nonzero(d == -1)[1]                                 # the same order: row-major, and runs of a row do not overlap
    R = int(ry.shape[0])
    parent = list(range(R))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    reach = 1 if connectivity == 8 else 0
    first = np.searchsorted(ry, np.arange(H + 1))               # runs of row y: first[y] .. first[y + 1]
    s, e = rs.tolist(), re.tolist()
    for y in range(1, H):
        a, a1, b, b1 = first[y - 1], first[y], first[y], first[y + 1]
        while a < a1 and b < b1:
            if s[a] < e[b] + reach and s[b] < e[a] + reach:     # [s, e) of the two rows touch
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if e[a] < e[b]:                                     # the run that ends first can touch no later run of the other row
                a += 1
            else:
                b += 1
    number = np.zeros(R, np.int64)
    n = 0
    for r in range(R):
        root = find(r)
        if root == r:
            n += 1
            number[r] = n
        else:
            number[r] = number[root]                            # root < r: numbered already
    paint = np.zeros((H, W + 1), np.int64)
    paint[ry, rs] += number
    paint[ry, re] -= number
    return np.cumsum(paint, axis=1)[:, :W].astype(np.int32), n


# ------------------------------------------------------------------------------------------------ the table
def table(labels: np.ndarray, n: int, overlay=None):
    """``(area int64 [n], bbox int32 [n,4] = (y0, x0, y1, x1) inclusive, overlap int64 [n,2] or None)``; overlay: >= 1 is set, 255
    is ignored; overlap = (pixels of the object that are not ignored, those of them where the overlay is set)."""
    labels = np.asarray(labels)
    ys, xs = np.nonzero(labels)
    l = labels[ys, xs].astype(np.int64) - 1
    area = np.bincount(l, minlength=n).astype(np.int64)
    bbox = np.zeros((n, 4), np.int32)
    big = np.iinfo(np.int32).max
    y0, x0, y1, x1 = np.full(n, big, np.int64), np.full(n, big, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    np.minimum.at(y0, l, ys); np.minimum.at(x0, l, xs); np.maximum.at(y1, l, ys); np.maximum.at(x1, l, xs)
    bbox[:, 0], bbox[:, 1], bbox[:, 2], bbox[:, 3] = y0, x0, y1, x1
    overlap = None
    if overlay is not None:
        o = np.asarray(overlay)[ys, xs]
        counted = o != 255
        overlap = np.stack([np.bincount(l[counted], minlength=n), np.bincount(l[counted & (o != 0)], minlength=n)], axis=1).astype(np.int64)
    return area, bbox, overlap


# ------------------------------------------------------------------------------------------------ the filter
def filter_objects(mask: np.ndarray, min_area: int = 0, max_hole: int = 0, connectivity: int = 8, mask_value: int = 255) -> np.ndarray:
    """Step 1: set components below ``min_area`` pixels are cleared (``min_area <= 1``: skipped).  Step 2, on that result: unset
    components, with the complementary connectivity, of at most ``max_hole`` pixels that touch no border are set (0: skipped)."""
    m = np.asarray(mask) != 0
    if min_area > 1:
        lab, n = label(m, connectivity)
        keep = np.concatenate([[False], np.bincount(lab.ravel(), minlength=n + 1)[1:] >= min_area])
        m = keep[lab]
    if max_hole > 0:
        lab, n = label(m, 4 if connectivity == 8 else 8, invert=True)
        fill = np.concatenate([[False], np.bincount(lab.ravel(), minlength=n + 1)[1:] <= max_hole])
        for edge in (lab[0, :], lab[-1, :], lab[:, 0], lab[:, -1]):
            fill[edge[edge > 0]] = False
        m = m | fill[lab]
    return m.astype(np.uint8) * np.uint8(mask_value)


# ------------------------------------------------------------------------------------------------ matching
def match_counts(pred: np.ndarray, lab: np.ndarray, connectivity: int = 8, min_overlap: float = 0.5):
    """``(n_pred, n_label, tp_pred, tp_label)``: objects of ``pred`` against the label and the reverse; an object with no counted
    pixel is dropped, an object is matched if hits >= min_overlap * counted.  The prediction is an overlay as 0 / 1: none of its
    pixels is ignored, whatever byte marks them."""
    pred, lab = np.asarray(pred), np.asarray(lab)
    res = []
    for mask, overlay in ((pred != 0, lab), ((lab != 0) & (lab != 255), (pred != 0).astype(np.uint8))):
        l, n = label(mask, connectivity)
        ov = table(l, n, overlay)[2]
        ov = ov[ov[:, 0] > 0]
        res.append((int(ov.shape[0]), int(sum(1 for c, h in ov.tolist() if h >= min_overlap * c))))
    return res[0][0], res[1][0], res[0][1], res[1][1]


# ------------------------------------------------------------------------------------------------ the masks of the tests
def _box(m, y0, x0, y1, x1, v=1):
    """The outline of the rectangle (inclusive corners), clipped to the scene."""
    H, W = m.shape
    for y in range(max(y0, 0), min(y1, H - 1) + 1):
        for x in range(max(x0, 0), min(x1, W - 1) + 1):
            if y in (y0, y1) or x in (x0, x1):
                m[y, x] = v


def _spiral(H, W):
    m = np.zeros((H, W), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    turns = 0
    inside = lambda a, b: 0 <= a < H and 0 <= b < W
    while turns < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not m[ny, nx] and not (inside(fy, fx) and m[fy, fx]):
            y, x = ny, nx
            m[y, x] = 1
            turns = 0
        else:
            dy, dx = dx, -dy                                    # turn right
            turns += 1
    return m


def _serpentine(H, W):
    m = np.zeros((H, W), np.uint8)
    m[0::2, :] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


NOISE = (0.1, 0.407, 0.593, 0.9)                                # 0.407 and 0.593: the two percolation thresholds


@functools.lru_cache(maxsize=None)
def patterns(H: int, W: int, T: int):
    """``{name: uint8 [H,W]}`` (values 0 and a non-zero byte), the same for every caller; T is the kernels' tile edge, so that
    objects cross the seams where the scene has any."""
    z = lambda: np.zeros((H, W), np.uint8)
    out = {"empty": z(), "full": np.full((H, W), 255, np.uint8)}
    m = z(); m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = 1
    out["corners"] = m
    yy, xx = np.mgrid[0:H, 0:W]
    out["checkerboard"] = (((yy + xx) & 1) == 0).astype(np.uint8) * np.uint8(7)
    out["serpentine"] = _serpentine(H, W)
    out["spiral"] = _spiral(H, W)
    m = z(); m[0, :] = 1; m[:, 0::2] = 1
    out["comb"] = m
    if H > T and W > T:                                         # the scene has a point where four tiles meet
        m = z(); m[T - 1, T - 1] = m[T, T] = 1
        out["corner_diag_main"] = m
        m = z(); m[T - 1, T] = m[T, T - 1] = 1
        out["corner_diag_anti"] = m
    for k, p in enumerate(NOISE):
        out[f"noise_{p}"] = (np.random.default_rng(100 + k).random((H, W)) < p).astype(np.uint8) * np.uint8(255)
    # rings around the first tile corner (or what of them fits)
    c = min(T, max(H // 2, 1)), min(T, max(W // 2, 1))
    m = z(); _box(m, c[0] - 6, c[1] - 7, c[0] + 5, c[1] + 8); _box(m, 1, 1, 4, 5)
    out["rings"] = m
    m = z(); _box(m, c[0] - 12, c[1] - 12, c[0] + 12, c[1] + 12); _box(m, c[0] - 8, c[1] - 8, c[0] + 8, c[1] + 8); _box(m, c[0] - 3, c[1] - 3, c[0] + 3, c[1] + 3)
    out["nested_rings"] = m
    m = z(); _box(m, c[0] - 7, c[1] - 7, c[0] + 7, c[1] + 7)
    if H > c[0] and W > c[1]:
        m[c[0] - 1:c[0] + 1, c[1] - 1:c[1] + 1] = 1
    out["ring_island"] = m
    m = z(); _box(m, -1, c[1] - 4, 5, c[1] + 4); _box(m, c[0] - 3, W - 6, c[0] + 3, W); _box(m, H - 5, -1, H, 6)
    out["ring_on_border"] = m
    m = z(); _box(m, 0, 2, 6, 9); m[0, 5:7] = 0                 # a box at the top border with a notch open to it
    _box(m, c[0] - 4, 0, c[0] + 4, 7); m[min(c[0], H - 1), 0] = 0
    out["notch"] = m
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def overlay_for(H: int, W: int) -> np.ndarray:
    """A label-like overlay: blocks of 0 / 1, some 255 (ignored) pixels, one other non-zero value."""
    rng = np.random.default_rng(H * 1000 + W)
    o = (rng.random((-(-H // 5), -(-W // 7))) < 0.4).astype(np.uint8).repeat(5, axis=0).repeat(7, axis=1)[:H, :W].copy()
    o[rng.random((H, W)) < 0.05] = 255
    o[(o == 1) & (rng.random((H, W)) < 0.1)] = 3
    o.setflags(write=False)
    return o
