"""The nearest-seed transform, label growth and the distance-transform split in plain numpy: the specification of
``distance.nearest_seed``, ``distance.expand_labels`` and ``objects.split_objects`` (stcd_amd/csrc/kernels_edt.hip and
kernels_split.hip, include/stcd_hip.h).  Every quantity is an integer.

``nearest_index`` is a brute force over the seeds and knows nothing of rows, columns or a separable method: the seeds are listed by
(column, row) and every pixel takes the FIRST seed of minimum squared distance, which is the tie rule: the smallest column, then
the smallest row.  Seeds, modes and the ignore plane are those of tests/edt_spec.py."""
import numpy as np

from tests import edt_spec as E
from tests import objects_spec as SP

NO_SEED = E.NO_SEED
_BLOCK_ELEMS = 1 << 20                  # pixels x seeds evaluated at a time (4 MiB of int32: it stays in the cache)


def nearest_index(seed: np.ndarray) -> np.ndarray:
    """int64 [H,W]: ``y * W + x`` of the nearest seed (y, x) of every pixel, -1 everywhere if there is none."""
    seed = np.asarray(seed, bool)
    H, W = seed.shape
    sx, sy = np.nonzero(seed.T)                                 # ordered by column, then by row
    out = np.full(H * W, -1, np.int64)
    if sx.size == 0:
        return out.reshape(H, W)
    sx, sy = sx.astype(np.int32), sy.astype(np.int32)           # int32 holds every value: 2 * 16383**2 < 2**31
    block = max(1, _BLOCK_ELEMS // sx.size)
    for p0 in range(0, H * W, block):
        p = np.arange(p0, min(p0 + block, H * W), dtype=np.int32)
        d = (p // W)[:, None] - sy[None, :]
        d *= d
        e = (p % W)[:, None] - sx[None, :]
        e *= e
        d += e
        k = np.argmin(d, axis=1)                                # the first minimum
        out[p] = sy[k].astype(np.int64) * W + sx[k]
    return out.reshape(H, W)


def nearest_seed(mask: np.ndarray, to: str = "set", ignore=None) -> np.ndarray:
    return nearest_index(E.seeds(mask, to, ignore))


def d2_of_index(index: np.ndarray) -> np.ndarray:
    """int64 [H,W]: the squared distance from every pixel to the pixel its index names, NO_SEED where the index is -1."""
    index = np.asarray(index, np.int64)
    H, W = index.shape
    ii, jj = np.indices((H, W), dtype=np.int64)
    return np.where(index < 0, np.int64(NO_SEED), (index // W - ii) ** 2 + (index % W - jj) ** 2)


def gather_at(index: np.ndarray, values: np.ndarray, q: int) -> np.ndarray:
    """int64 [H,W]: ``values[index[p]]`` where ``d2[p] <= q``, else 0, for an index plane of ``nearest_index``."""
    near = d2_of_index(index) <= int(q)                         # q < NO_SEED: the index is valid there
    return np.where(near, np.asarray(values, np.int64).reshape(-1)[np.where(near, index, 0)], 0)


def gather(seed: np.ndarray, values: np.ndarray, q: int) -> np.ndarray:
    return gather_at(nearest_index(seed), values, q)


def expand_labels(labels: np.ndarray, distance) -> np.ndarray:
    labels = np.asarray(labels)
    return gather(labels != 0, labels, E.buffer_q(distance))


def split_objects(mask: np.ndarray, radius, min_core_area: int = 0, connectivity: int = 8, mask_value: int = 255) -> dict:
    """``{"mask", "owner", "n_cores", "cut_pixels", "orphan_pixels"}`` by the five steps of ``objects.split_objects``."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    core = E.buffer_mask(mask, radius, "erode")
    if min_core_area > 0:
        core = SP.filter_objects(core, min_area=min_core_area, connectivity=connectivity)
    Lc, n_cores = SP.label(core, connectivity)
    L0, _ = SP.label(m, connectivity)
    index = nearest_index(core != 0)
    valid = m & (index >= 0)
    at = np.where(valid, index, 0)
    owner = np.where(valid & (L0.reshape(-1)[at] == L0), Lc.reshape(-1)[at], 0).astype(np.int64)
    pad = np.zeros((H + 1, W + 2), np.int64)                    # a frame of owner 0 right, below and left
    pad[:H, 1:W + 1] = owner
    cut = np.zeros((H, W), bool)
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        nb = pad[dy:dy + H, 1 + dx:1 + dx + W]
        cut |= (owner != 0) & (nb != 0) & (nb != owner)
    return {"mask": (m & ~cut).astype(np.uint8) * np.uint8(mask_value), "owner": owner.astype(np.int32), "n_cores": int(n_cores),
            "cut_pixels": int(cut.sum()), "orphan_pixels": int((m & (owner == 0)).sum())}


# ------------------------------------------------------------------------------------------------ the fixtures of the split tests
def _disc(m, cy, cx, r):
    yy, xx = np.indices(m.shape)
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255


def discs_row():
    m = np.zeros((96, 131), np.uint8)
    for k in range(5):
        _disc(m, 48, 21 + 22 * k, 14)
    return m


def discs_column():
    m = np.zeros((150, 40), np.uint8)
    for k in range(6):
        _disc(m, 20 + 22 * k, 20, 14)
    return m


def discs_diagonal():
    m = np.zeros((140, 140), np.uint8)
    for k in range(7):
        _disc(m, 22 + 16 * k, 22 + 16 * k, 14)
    return m


DISCS = {"row": (discs_row, 5, 136), "column": (discs_column, 6, 85), "diagonal": (discs_diagonal, 7, 138)}      # objects and cut pixels at radius 9.5


def rectangles():
    m = np.zeros((40, 60), np.uint8)
    m[5:25, 5:25] = 255
    m[15:35, 22:50] = 255
    return m


def arm():
    """Two squares of 20 pixels, two unset columns apart, and a 2-pixel arm of the left one that runs along the top of the right
    one's side: nearer to the right square's core than to its own."""
    m = np.zeros((40, 60), np.uint8)
    m[10:30, 5:25] = 255
    m[10:30, 27:47] = 255
    m[6:8, 20:40] = 255                                         # the arm, above the right square with one unset row between
    m[6:10, 20:22] = 255                                        # and its foot on the left square
    return m
