"""The exact squared Euclidean distance transform, the disc buffers and the boundary match in plain numpy int64 and Python ints: the
specification of stcd_amd/distance.py (stcd_amd/csrc/kernels_edt.hip, include/stcd_hip.h).  Every quantity is an integer.

A mask is uint8 ``[H,W]``; a pixel is set iff its byte is non-zero; pixel (i, j) is a lattice point and the squared distance of two
pixels is ``(i - i')**2 + (j - j')**2``.  ``d2[i][j]`` is the minimum squared distance from (i, j) to a seed pixel inside the frame,
0 on a seed and ``NO_SEED`` when the frame holds no seed.  Seeds: ``unset`` (scipy's convention: the zero pixels), ``set`` (the
object pixels), ``boundary`` (``boundary`` below).  Nothing outside the frame is ever a seed."""
import numpy as np

NO_SEED = 2 ** 30                       # above the largest real value, 2 * 16383**2
NONE = -1                               # "no seed in this column" of column_distance
VOID = 255                              # the byte of an ignore plane that marks a void pixel
MODES = ("unset", "set", "boundary")
MAX_TOLERANCES = 8
_BLOCK_ELEMS = 1 << 22                  # the row pass evaluates columns in blocks of about this many int64 costs (32 MiB)


def buffer_q(radius) -> int:
    """floor(radius**2), clamped to NO_SEED - 1 so that "no seed" is never within a radius."""
    r = float(radius)
    if not r >= 0.0:
        raise ValueError(f"radius must be >= 0, got {radius!r}")
    v = r * r
    return NO_SEED - 1 if v >= NO_SEED - 1 else int(np.floor(v))


def boundary(mask: np.ndarray, ignore=None) -> np.ndarray:
    """bool [H,W]: p is set, p is not void, and a 4-neighbour of p inside the frame is unset and not void."""
    m = np.asarray(mask) != 0
    void = np.zeros(m.shape, bool) if ignore is None else np.asarray(ignore) == VOID
    free = ~m & ~void
    near = np.zeros(m.shape, bool)
    near[1:] |= free[:-1]
    near[:-1] |= free[1:]
    near[:, 1:] |= free[:, :-1]
    near[:, :-1] |= free[:, 1:]
    return m & ~void & near


def seeds(mask: np.ndarray, to: str = "unset", ignore=None) -> np.ndarray:
    m = np.asarray(mask)
    if to == "unset":
        return m == 0
    if to == "set":
        return m != 0
    if to == "boundary":
        return boundary(m, ignore)
    raise ValueError(to)


def column_distance(seed: np.ndarray) -> np.ndarray:
    """int64 [H,W]: the distance along column j from row i to the nearest seed of that column, NONE where the column has none."""
    seed = np.asarray(seed, bool)
    H, W = seed.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    far = np.int64(4 * H + 4)
    above = np.maximum.accumulate(np.where(seed, rows, -far), axis=0)                       # the last seed at or above
    below = np.minimum.accumulate(np.where(seed, rows, far)[::-1], axis=0)[::-1]            # the first seed at or below
    g = np.minimum(rows - above, below - rows)
    return np.where(g > H, NONE, g)


def row_minimum(g: np.ndarray) -> np.ndarray:
    """int64 [H,W]: min over k of (j - k)**2 + g[i][k]**2 by brute force, a column without a seed carrying NO_SEED; clamped to NO_SEED."""
    g = np.asarray(g, np.int64)
    H, W = g.shape
    h = np.where(g == NONE, np.int64(NO_SEED), g * g)
    k = np.arange(W, dtype=np.int64)
    out = np.empty((H, W), np.int64)
    block = max(1, min(W, _BLOCK_ELEMS // max(1, H * W)))
    for j0 in range(0, W, block):
        j = np.arange(j0, min(j0 + block, W), dtype=np.int64)
        cost = (j[:, None] - k[None, :]) ** 2                   # [block, W]
        out[:, j0:j0 + j.shape[0]] = (h[:, None, :] + cost[None]).min(axis=2)
    return np.minimum(out, NO_SEED)


def d2_of_seeds(seed: np.ndarray) -> np.ndarray:
    return row_minimum(column_distance(seed))


def squared_distance(mask: np.ndarray, to: str = "unset", ignore=None) -> np.ndarray:
    return d2_of_seeds(seeds(mask, to, ignore))


def threshold(d2: np.ndarray, q: int, keep_above: bool, mask_value: int = 255) -> np.ndarray:
    hit = (d2 > q) if keep_above else (d2 <= q)
    return hit.astype(np.uint8) * np.uint8(mask_value)


def dilate(mask, q, mask_value=255):
    return threshold(squared_distance(mask, "set"), q, False, mask_value)


def erode(mask, q, mask_value=255):
    return threshold(squared_distance(mask, "unset"), q, True, mask_value)


def buffer_mask(mask: np.ndarray, radius, op: str = "dilate", mask_value: int = 255) -> np.ndarray:
    q = buffer_q(radius)
    if op == "dilate":
        return dilate(mask, q, mask_value)
    if op == "erode":
        return erode(mask, q, mask_value)
    if op == "close":
        return erode(dilate(mask, q, mask_value), q, mask_value)
    if op == "open":
        return dilate(erode(mask, q, mask_value), q, mask_value)
    raise ValueError(op)


def match_counts(pred: np.ndarray, label: np.ndarray, qs) -> np.ndarray:
    """int64 [2][2 + T]: side 0 the boundary of pred measured against that of label, side 1 the reverse: (n, max_d2, within[t])."""
    qs = [int(q) for q in qs]
    if not 1 <= len(qs) <= MAX_TOLERANCES:
        raise ValueError("1 to 8 tolerances")
    bp, bl = boundary(pred, label), boundary(label, label)
    out = np.zeros((2, 2 + len(qs)), np.int64)
    for side, (own, other) in enumerate(((bp, bl), (bl, bp))):
        d = d2_of_seeds(other)[own]
        out[side, 0] = d.size
        out[side, 1] = int(d.max()) if d.size else 0
        for t, q in enumerate(qs):
            out[side, 2 + t] = int((d <= q).sum())
    return out


def scores(counts: np.ndarray):
    """(precision [T], recall [T], f1 [T], hausdorff2) from match_counts' integers; an empty denominator gives 0.0."""
    counts = np.asarray(counts, np.int64)
    n0, n1 = int(counts[0, 0]), int(counts[1, 0])
    precision = tuple(int(w) / n0 if n0 else 0.0 for w in counts[0, 2:])
    recall = tuple(int(w) / n1 if n1 else 0.0 for w in counts[1, 2:])
    f1 = tuple(2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall))
    return precision, recall, f1, max(int(counts[0, 1]), int(counts[1, 1]))
