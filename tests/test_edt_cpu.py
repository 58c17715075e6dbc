"""The specification of the distance transform (tests/edt_spec.py) against scipy and against direct loops, on the host: what the GPU
tests then hold the device to.  Every quantity is an integer and every assertion is equality."""
import numpy as np
import pytest
from scipy import ndimage

from stcd_amd import distance as DT
from stcd_amd._lib import StcdError
from tests import edt_spec as E


def random_seeds(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def scipy_d2(seed: np.ndarray) -> np.ndarray:
    """distance_transform_edt's nearest-seed indices turned into integer squared distances (its floats are not compared)."""
    if not seed.any():
        return np.full(seed.shape, E.NO_SEED, np.int64)
    idx = ndimage.distance_transform_edt(~seed, return_distances=False, return_indices=True).astype(np.int64)
    ii, jj = np.indices(seed.shape)
    return (idx[0] - ii) ** 2 + (idx[1] - jj) ** 2


def disc(q: int) -> np.ndarray:
    r = int(np.floor(np.sqrt(q)))
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return y * y + x * x <= q


@pytest.mark.parametrize("shape", [(97, 131), (300, 1100), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("density", [1 / 64, 0.3])
def test_spec_equals_scipy(shape, density):
    seed = random_seeds(shape, density, 7)
    assert np.array_equal(E.d2_of_seeds(seed), scipy_d2(seed))


def test_spec_without_a_seed_and_with_one():
    assert (E.d2_of_seeds(np.zeros((5, 9), bool)) == E.NO_SEED).all()
    one = np.zeros((40, 23), bool)
    one[39, 0] = True
    ii, jj = np.indices(one.shape)
    assert np.array_equal(E.d2_of_seeds(one), (ii - 39) ** 2 + jj ** 2)
    g = E.column_distance(one)
    assert (g[:, 1:] == E.NONE).all() and g[:, 0].tolist() == list(range(39, -1, -1))
    m = np.array([[0, 3, 255]], np.uint8)
    assert E.squared_distance(m, "unset").tolist() == [[0, 1, 4]] and E.squared_distance(m, "set").tolist() == [[1, 0, 0]]


@pytest.mark.parametrize("radius", [0, 1, 1.5, 2, 7.3])
def test_disc_buffers_equal_scipy(radius):
    m = random_seeds((97, 131), 0.02, 3) | (ndimage.binary_dilation(random_seeds((97, 131), 0.004, 4), iterations=6))
    m[0, :20] = True                                            # objects touching the frame
    m[40:60, 128:] = True
    q = E.buffer_q(radius)
    mask = m.astype(np.uint8) * np.uint8(7)
    want = ndimage.binary_dilation(m, structure=disc(q))
    assert np.array_equal(E.buffer_mask(mask, radius, "dilate", 1), want.astype(np.uint8))
    want = ndimage.binary_erosion(m, structure=disc(q), border_value=1)
    assert np.array_equal(E.buffer_mask(mask, radius, "erode", 255), want.astype(np.uint8) * np.uint8(255))


def test_close_contains_mask_contains_open():
    m = (random_seeds((96, 96), 0.05, 11) | ndimage.binary_dilation(random_seeds((96, 96), 0.01, 12), iterations=4)).astype(np.uint8)
    for radius in (0, 1, 2.5, 6):
        closed, opened = E.buffer_mask(m, radius, "close", 1), E.buffer_mask(m, radius, "open", 1)
        assert (closed >= m).all() and (m >= opened).all(), radius
        if radius == 0:
            assert np.array_equal(closed, m) and np.array_equal(opened, m)
            assert np.array_equal(E.buffer_mask(m, 0, "dilate", 1), m) and np.array_equal(E.buffer_mask(m, 0, "erode", 1), m)
    assert (E.buffer_mask(m, 300, "dilate", 1) == 1).all() and not E.buffer_mask(m, 300, "erode", 1).any()
    assert not E.buffer_mask(np.zeros((5, 5), np.uint8), 1e9, "dilate").any()     # no seed is within no radius
    assert E.buffer_mask(np.ones((5, 5), np.uint8), 1e9, "erode").all()           # and the frame edge does not erode


def boundary_by_loops(mask, ignore):
    H, W = mask.shape
    out = np.zeros((H, W), bool)
    for i in range(H):
        for j in range(W):
            if mask[i, j] == 0 or (ignore is not None and ignore[i, j] == 255):
                continue
            for y, x in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                if 0 <= y < H and 0 <= x < W and mask[y, x] == 0 and not (ignore is not None and ignore[y, x] == 255):
                    out[i, j] = True
    return out


def test_boundary_equals_the_double_loop():
    rng = np.random.default_rng(5)
    mask = (ndimage.binary_dilation(rng.random((24, 31)) < 0.04, iterations=2)).astype(np.uint8) * np.uint8(255)
    mask[0, :] = 255
    mask[:, 30] = 9
    ignore = np.zeros((24, 31), np.uint8)
    ignore[10:14] = 255                                         # a void band across objects
    ignore[:, :2] = 255
    ignore[rng.random((24, 31)) < 0.05] = 255
    ignore[rng.random((24, 31)) < 0.05] = 254                   # not the void byte
    for ig in (None, ignore):
        got = E.boundary(mask, ig)
        assert np.array_equal(got, boundary_by_loops(mask, ig))
        assert got.any()
    full = np.ones((6, 7), np.uint8)
    assert not E.boundary(full).any()                           # the frame edge is no boundary
    assert not E.boundary(mask, np.full((24, 31), 255, np.uint8)).any()


def test_buffer_q():
    assert [E.buffer_q(r) for r in (0, 1, 1.5, 2, 7.3, 16383.9)] == [0, 1, 2, 4, 53, 268432179]
    assert E.buffer_q(1e9) == E.NO_SEED - 1 and E.buffer_q(float("inf")) == E.NO_SEED - 1
    for r in (0, 0.99, 1, 1.5, 2, 7.3, 1e9):
        assert DT.buffer_q(r) == E.buffer_q(r)
    for bad in (-1, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            E.buffer_q(bad)
        with pytest.raises(StcdError):
            DT.buffer_q(bad)
    assert DT.NO_SEED == E.NO_SEED == 2 ** 30 and DT.MAX_TOLERANCES == E.MAX_TOLERANCES == 8


def scene96():
    rng = np.random.default_rng(96)
    label = ndimage.binary_dilation(rng.random((96, 96)) < 0.004, iterations=5).astype(np.uint8)
    pred = np.roll(label, (2, -3), (0, 1)) | (rng.random((96, 96)) < 0.002).astype(np.uint8)
    label[:, 90:] = 255                                         # an ignored margin
    return pred, label


def test_pinned_counts_of_one_scene():
    pred, label = scene96()
    counts = E.match_counts(pred, label, [E.buffer_q(t) for t in (1.0, 2.0, 4.0)])
    assert counts.tolist() == PINNED_COUNTS
    precision, recall, f1, h2 = E.scores(counts)
    assert h2 == max(PINNED_COUNTS[0][1], PINNED_COUNTS[1][1])
    assert precision[1] == PINNED_COUNTS[0][3] / PINNED_COUNTS[0][0] and recall[2] == PINNED_COUNTS[1][4] / PINNED_COUNTS[1][0]
    assert DT.scores_from_counts(counts) == (precision, recall, f1, h2)
    # the counts by loops over the boundary pixels
    bp, bl = boundary_by_loops(pred, label), boundary_by_loops(label, label)
    P, Lb = np.argwhere(bp), np.argwhere(bl)
    d = ((P[:, None, :] - Lb[None, :, :]) ** 2).sum(axis=2)
    assert [len(P), int(d.min(axis=1).max()), int((d.min(axis=1) <= 4).sum())] == [counts[0, 0], counts[0, 1], counts[0, 3]]
    assert [len(Lb), int(d.min(axis=0).max()), int((d.min(axis=0) <= 4).sum())] == [counts[1, 0], counts[1, 1], counts[1, 3]]
    # empty sides
    zero = np.zeros_like(pred)
    assert E.match_counts(zero, label, [4]).tolist() == [[0, 0, 0], [int(bl.sum()), E.NO_SEED, 0]]
    assert E.match_counts(zero, zero, [4]).tolist() == [[0, 0, 0], [0, 0, 0]]
    assert E.scores(E.match_counts(zero, zero, [4])) == ((0.0,), (0.0,), (0.0,), 0)


PINNED_COUNTS = [[626, 80, 283, 324, 611], [597, 17, 284, 329, 595]]      # (n, max_d2, within 1.0, 2.0, 4.0) per side
