"""The nearest-seed transform on the GPU: nearest_seed and expand_labels of stcd_amd/distance.py and split_objects of
stcd_amd/objects.py against the numpy specification of tests/nearest_spec.py, against closed forms at the largest frames, at the
sizes where the kernels change path, on the ties the separable method can get wrong, and the reuse and refusal rules.  Every output
is an integer or a byte and every assertion is equality."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import distance as DT
from stcd_amd import objects as OB
from tests import edt_spec as E
from tests import nearest_spec as N
from tests import objects_spec as SP
from tests import rings_spec as RS
from tests import simplify_spec as SS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CH, COLS, THREADS, LANE = DT.COL_CHUNK, DT.COL_BLOCK_COLS, DT.ROW_THREADS, DT.ROW_LANE_MAX
SHAPES = ((96, 96), (67, 131))


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)                # a copy: the shared references are read-only


def host(t):
    return t.cpu().numpy()


def unaligned(x):
    """The same bytes at an odd address: rows are read as bytes, not as words."""
    x = np.ascontiguousarray(x)
    t = torch.zeros(x.size + 1, dtype=torch.uint8, device=DEV)[1:].view(*x.shape)
    t.copy_(torch.from_numpy(x))
    return t


@functools.lru_cache(maxsize=None)
def all_patterns(shape):
    return {**SP.patterns(*shape, OB.TILE), **RS.patterns(*shape), **SS.patterns(*shape)}


def assert_nearest(mask, where, modes=E.MODES, ignore=None, tensor=dev):
    """index against the spec, d2 against squared_distance bit for bit, and the plain call against the one that returns both."""
    m = tensor(mask)
    for to in modes:
        ig = ignore if to == "boundary" else None
        igt = None if ig is None else tensor(ig)
        index, d2 = DT.nearest_seed(m, to=to, ignore=igt, return_distance=True)
        for t in (index, d2):
            assert t.dtype == torch.int32 and tuple(t.shape) == mask.shape and t.device == DEV and t.is_contiguous(), where
        want = N.nearest_seed(mask, to, ig)
        assert np.array_equal(host(index), want), (where, to)
        assert torch.equal(d2, DT.squared_distance(m, to=to, ignore=igt)), (where, to)
        assert np.array_equal(host(d2), N.d2_of_index(want)), (where, to)
        assert torch.equal(DT.nearest_seed(m, to=to, ignore=igt), index), (where, to)


# ------------------------------------------------------------------------------------------------ the index against the spec
CASES = [(shape, name) for shape in SHAPES for name in all_patterns(shape)]
CASE_IDS = [f"{s[0]}x{s[1]}-{n}" for s, n in CASES]


@pytest.mark.parametrize("shape,name", CASES, ids=CASE_IDS)
def test_nearest_seed_equals_the_spec(shape, name):
    mask = all_patterns(shape)[name]
    assert_nearest(mask, name)
    assert_nearest(mask, (name, "ignore"), modes=("boundary",), ignore=SP.overlay_for(*shape))


# ------------------------------------------------------------------------------------------------ the thresholds between the paths
def sizes_around(*constants):
    out = {1, 2, 3}
    for c in constants:
        out |= {c - 1, c, c + 1}
    return sorted(out)


def sparse(shape, seed):
    return (np.random.default_rng(seed).random(shape) < 1 / 64).astype(np.uint8) * np.uint8(255)


def single(shape, at):
    m = np.zeros(shape, np.uint8)
    m[at] = 1
    return m


@pytest.mark.parametrize("W", sizes_around(LANE, THREADS, COLS, 2 * COLS))
def test_widths_at_the_thresholds(W):
    shape = (8, W)
    over = SP.overlay_for(*shape)
    few = ("set", "boundary")                                   # the brute force over nearly W * 8 seeds is left to the narrow frames
    for k, mask in enumerate((sparse(shape, W), single(shape, (5, W - 1)), single(shape, (2, W // 2)))):
        assert_nearest(mask, (W, k), modes=E.MODES if W <= 2 * THREADS else few, ignore=over if k == 0 else None)
        if k == 0:
            assert_nearest(mask, (W, "bytes"), modes=few, ignore=over, tensor=unaligned)       # an odd address, and for odd W an odd width


@pytest.mark.parametrize("H", sizes_around(CH, 2 * CH, 4 * CH))
def test_heights_at_the_thresholds(H):
    shape = (H, 8)
    over = SP.overlay_for(*shape)
    for k, mask in enumerate((sparse(shape, H), single(shape, (H - 1, 3)), single(shape, (0, 7)), single(shape, (H // 2, 0)))):
        assert_nearest(mask, (H, k), ignore=over if k == 0 else None)
    blocks = np.zeros(shape, np.uint8)
    blocks[max(H // 2 - 3, 0):H // 2 + 3, 2:7] = 1              # boundaries across a chunk cut
    assert_nearest(blocks, (H, "blocks"), ignore=over)
    assert_nearest(blocks, (H, "blocks, bytes"), ignore=over, tensor=unaligned)


# ------------------------------------------------------------------------------------------------ ties
def test_a_column_tie_across_a_chunk_cut():
    """Seeds at rows 60 and 68 of one column seen from row 64: the upper one comes from the carried table, the lower one from the
    chunk's own bits; the smaller row wins.  And the mirror pair 59 / 67 from row 63: own bits above, the table below."""
    for up, dn in ((60, 68), (59, 67)):
        at = (up + dn) // 2
        for W, c in ((8, 5), (7, 0)):
            mask = np.zeros((130, W), np.uint8)
            mask[up, c] = mask[dn, c] = 1
            got = host(DT.nearest_seed(dev(mask)))
            assert got[at, c] == up * W + c, (up, dn, W)
            assert (got[at] == up * W + c).all(), (up, dn, W)   # the whole row ties
            assert_nearest(mask, (up, dn, W), modes=("set",))


def test_a_row_tie_between_columns_of_different_waves():
    for W in (301, 320, 1100):
        mask = np.zeros((5, W), np.uint8)
        mask[:, 10] = mask[:, 300] = 1
        got = host(DT.nearest_seed(dev(mask)))
        assert (got[:, 155] == np.arange(5) * W + 10).all() and (got[:, 156] == np.arange(5) * W + 300).all(), W
        assert_nearest(mask, W, modes=("set",))


def test_a_diagonal_tie():
    for H, W, y0, y1, x0, x1 in ((9, 11, 2, 6, 3, 7), (130, 320, 60, 68, 10, 300), (131, 323, 59, 67, 11, 301)):
        mask = np.zeros((H, W), np.uint8)
        mask[y0, x0] = mask[y0, x1] = mask[y1, x0] = mask[y1, x1] = 1
        got = host(DT.nearest_seed(dev(mask)))
        assert got[(y0 + y1) // 2, (x0 + x1) // 2] == y0 * W + x0, (H, W)                    # the smallest column, then the smallest row
        assert_nearest(mask, (H, W), modes=("set",))
    mask = np.zeros((9, 11), np.uint8)
    mask[2, 7] = mask[6, 3] = 1                                 # the lower seed in the smaller column beats the upper one in the larger
    assert host(DT.nearest_seed(dev(mask)))[4, 5] == 6 * 11 + 3


# ------------------------------------------------------------------------------------------------ degenerate and extreme frames
@pytest.mark.parametrize("shape", [(1, 1), (1, 77), (1, 1030), (77, 1), (130, 1), (2, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_degenerate_frames(shape):
    for k, mask in enumerate((np.zeros(shape, np.uint8), np.ones(shape, np.uint8), single(shape, (shape[0] - 1, shape[1] // 2)), sparse(shape, 5))):
        assert_nearest(mask, (shape, k))
    n = shape[0] * shape[1]
    assert bool((DT.nearest_seed(torch.zeros(shape, dtype=torch.uint8, device=DEV)) == -1).all())
    identity = torch.arange(n, dtype=torch.int32, device=DEV).view(shape)
    assert torch.equal(DT.nearest_seed(torch.ones(shape, dtype=torch.uint8, device=DEV)), identity)


@pytest.mark.parametrize("shape", [(16384, 16), (16, 16384)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_corner_seed_in_the_longest_frames(shape):
    H, W = shape
    ii = torch.arange(H, dtype=torch.int64, device=DEV)[:, None]
    jj = torch.arange(W, dtype=torch.int64, device=DEV)[None, :]
    for ci, cj in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        mask = torch.zeros(shape, dtype=torch.uint8, device=DEV)
        mask[ci, cj] = 200
        index, d2 = DT.nearest_seed(mask, return_distance=True)
        assert bool((index == ci * W + cj).all()), (ci, cj)
        assert torch.equal(d2, ((ii - ci) ** 2 + (jj - cj) ** 2).to(torch.int32)), (ci, cj)
    empty = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    index, d2 = DT.nearest_seed(empty, return_distance=True)
    assert bool((index == -1).all()) and bool((d2 == DT.NO_SEED).all())
    assert torch.equal(DT.nearest_seed(empty, to="unset"), torch.arange(H * W, dtype=torch.int32, device=DEV).view(shape))


# ------------------------------------------------------------------------------------------------ expand_labels
DISTANCES = (0, 1, 2.5, 1000)


@pytest.mark.parametrize("shape,name", CASES, ids=CASE_IDS)
def test_expand_labels_equals_the_spec(shape, name):
    mask = all_patterns(shape)[name]
    comps = OB.label_components(dev(mask))
    lab = SP.label(mask)[0]
    assert np.array_equal(host(comps.labels), lab)
    index = N.nearest_index(lab != 0)                           # once for the four distances
    for distance in DISTANCES:
        got = DT.expand_labels(comps, distance)
        assert got.dtype == torch.int32 and tuple(got.shape) == shape and got.is_contiguous() and got.data_ptr() != comps.labels.data_ptr()
        assert np.array_equal(host(got), N.gather_at(index, lab, E.buffer_q(distance))), (name, distance)
        assert torch.equal(DT.expand_labels(comps.labels, distance), got), (name, distance)           # the plane alone is taken too
        if distance == 0:
            assert torch.equal(got, comps.labels), name
    if name == "empty":
        assert not bool(DT.expand_labels(comps, 1000).any())
    assert np.array_equal(host(comps.labels), lab)              # the input is left untouched


def test_expand_labels_of_foreign_labels():
    """Any int32 plane is a label plane: negative and large values travel unchanged, and the spec's own expand_labels agrees."""
    rng = np.random.default_rng(12)
    lab = np.zeros((45, 83), np.int32)
    at = rng.random(lab.shape) < 0.01
    lab[at] = rng.integers(-2 ** 31, 2 ** 31 - 1, int(at.sum()), dtype=np.int64).astype(np.int32)
    lab[at & (lab == 0)] = 1
    for distance in (1.5, 4, 1000):
        assert np.array_equal(host(DT.expand_labels(dev(lab), distance)), N.expand_labels(lab, distance)), distance


# ------------------------------------------------------------------------------------------------ split_objects
def assert_split(mask, radius, where, **kw):
    want = N.split_objects(mask, radius, **kw)
    m = dev(mask)
    got = OB.split_objects(m, radius, **kw)
    assert got.mask.dtype == torch.uint8 and got.owner.dtype == torch.int32 and tuple(got.mask.shape) == tuple(got.owner.shape) == mask.shape, where
    assert got.mask.data_ptr() != m.data_ptr() and torch.equal(m, dev(mask)), where
    assert np.array_equal(host(got.mask), want["mask"]), where
    assert np.array_equal(host(got.owner), want["owner"]), where
    assert (got.n_cores, got.cut_pixels, got.orphan_pixels) == (want["n_cores"], want["cut_pixels"], want["orphan_pixels"]), where
    lazy = OB.split_objects(m, radius, check=False, **kw)
    assert torch.equal(lazy.mask, got.mask) and torch.equal(lazy.owner, got.owner) and lazy.n_cores == got.n_cores, where
    assert torch.is_tensor(lazy.cut_pixels) and (int(lazy.cut_pixels), int(lazy.orphan_pixels)) == (got.cut_pixels, got.orphan_pixels), where
    # the properties: a subset of the mask, the cut pixels are what is missing, and no component of the result holds two owners
    # unless orphan pixels join them (the documented limit: an orphan region that touches two owners keeps them joined; the noise
    # patterns at radius 1 have such regions), so without orphans no component holds two owners at all
    value = kw.get("mask_value", 255)
    out, owner = host(got.mask), host(got.owner)
    assert ((out == 0) | ((out == value) & (mask != 0))).all(), where
    assert int((mask != 0).sum()) - int((out != 0).sum()) == got.cut_pixels, where
    orphan = (out != 0) & (owner == 0)
    assert int(orphan.sum()) == got.orphan_pixels, where        # orphans are never cut
    for connectivity in (4, 8):
        lab = host(OB.label_components(got.mask, connectivity).labels)
        owned = (lab != 0) & (owner != 0)
        if not owned.any():
            continue
        pairs = np.unique(np.stack([lab[owned], owner[owned]], axis=1), axis=0)
        ids, owners = np.unique(pairs[:, 0], return_counts=True)
        joined = ids[owners > 1]
        assert np.isin(joined, lab[orphan]).all(), (where, connectivity)
        if got.orphan_pixels == 0:
            assert joined.size == 0, (where, connectivity)
    return got


@pytest.mark.parametrize("name", sorted(N.DISCS))
def test_split_of_the_disc_fixtures(name):
    make, objects, cut = N.DISCS[name]
    mask = make()
    got = assert_split(mask, 9.5, name)
    assert (got.n_cores, got.cut_pixels, OB.label_components(got.mask).count) == (objects, cut, objects)
    got = assert_split(mask, 5, (name, 5))
    assert (got.n_cores, got.cut_pixels, OB.label_components(got.mask).count) == (1, 0, 1)
    assert_split(mask, 9.5, (name, "options"), connectivity=4, mask_value=7, min_core_area=3)


def test_split_of_rectangles_and_of_the_arm():
    mask = N.rectangles()
    got = assert_split(mask, 3, "rectangles, 3")
    assert (got.n_cores, got.cut_pixels, OB.label_components(got.mask).count) == (1, 0, 1)
    got = assert_split(mask, 6, "rectangles, 6")
    assert got.n_cores == 2 and got.cut_pixels > 0 and OB.label_components(got.mask).count == 2
    got = assert_split(mask, 6, "no core survives", min_core_area=10 ** 6)
    assert (got.n_cores, got.cut_pixels, got.orphan_pixels) == (0, 0, int((mask != 0).sum())) and not bool(got.owner.any())
    assert_split(mask, 6, "one core survives", min_core_area=40)
    arm = N.arm()
    got = assert_split(arm, 3, "arm")
    assert got.n_cores == 2 and got.orphan_pixels > 0 and got.cut_pixels == 0 and OB.label_components(got.mask).count == 2
    for shape in ((40, 60), (1, 1), (3, 70)):
        got = assert_split(np.zeros(shape, np.uint8), 2, ("empty", shape))
        assert (got.n_cores, got.cut_pixels, got.orphan_pixels) == (0, 0, 0) and not bool(got.mask.any())
        got = assert_split(np.full(shape, 9, np.uint8), 2, ("full", shape), mask_value=3)
        assert (got.n_cores, got.cut_pixels, got.orphan_pixels) == (1, 0, 0) and bool((got.mask == 3).all()) and bool((got.owner == 1).all())


@pytest.mark.parametrize("shape,name", CASES, ids=CASE_IDS)
def test_split_of_the_patterns(shape, name):
    mask = all_patterns(shape)[name]
    assert_split(mask, 1, (name, 1))
    assert_split(mask, 2, (name, 2))


def test_split_across_block_edges():
    """Touching discs across the 256-column and 4-row blocks of the cut pass, at a width that is no multiple of anything."""
    mask = np.zeros((37, 531), np.uint8)
    yy, xx = np.indices(mask.shape)
    for k in range(23):
        mask[(yy - 18 - (k % 3)) ** 2 + (xx - 14 - 22 * k) ** 2 <= 14 * 14] = 255
    got = assert_split(mask, 9.5, "chain")
    assert got.n_cores == 23 and OB.label_components(got.mask).count == 23 and got.cut_pixels > 0


# ------------------------------------------------------------------------------------------------ reuse and refusals
def test_reuse_and_purity():
    a, b = np.array(all_patterns((96, 96))["rings"]), np.array(all_patterns((67, 131))["spiral"])
    wa, wb = N.nearest_seed(a, "set"), N.nearest_seed(b, "set")
    da, db = dev(a), dev(b)
    d2a = DT.squared_distance(da, to="set").clone()
    first = DT.nearest_seed(da)
    kept = first.clone()
    second = DT.nearest_seed(da)
    assert torch.equal(kept, second) and first.data_ptr() != second.data_ptr() and np.array_equal(host(kept), wa)
    assert np.array_equal(host(DT.nearest_seed(db)), wb)        # another shape in between: another scratch buffer
    assert torch.equal(DT.nearest_seed(da), kept) and torch.equal(da, dev(a))
    # the transforms that were there share the scratch buffer with the new ones and give what they gave
    assert torch.equal(DT.squared_distance(da, to="set"), d2a) and np.array_equal(host(d2a), E.squared_distance(a, "set"))
    grown = DT.expand_labels(OB.label_components(da), 2.5)
    assert np.array_equal(host(DT.buffer_mask(da, 2, op="close")), E.buffer_mask(a, 2, "close"))
    assert torch.equal(DT.expand_labels(OB.label_components(da), 2.5), grown)
    s1 = OB.split_objects(dev(N.discs_row()), 9.5)
    assert np.array_equal(host(DT.squared_distance(db, to="boundary")), E.squared_distance(b, "boundary"))
    s2 = OB.split_objects(dev(N.discs_row()), 9.5)
    assert torch.equal(s1.mask, s2.mask) and torch.equal(s1.owner, s2.owner) and s1[2:] == s2[2:]      # counts are cleared per call
    counts = DT.boundary_scores(da, dev(np.roll(a, 2, 0)), (1.0, 3.0)).counts
    assert np.array_equal(host(counts), E.match_counts(a, np.roll(a, 2, 0), [1, 9]))
    assert torch.equal(DT.nearest_seed(da), kept)
    DT._SCRATCH.clear()
    assert torch.equal(DT.nearest_seed(da), kept)


def test_the_wrappers_refuse():
    good = torch.zeros((48, 40), dtype=torch.uint8, device=DEV)
    wide = torch.zeros((48, 80), dtype=torch.uint8, device=DEV)
    big = torch.zeros((1, 16385), dtype=torch.uint8, device=DEV)
    lab = torch.zeros((48, 40), dtype=torch.int32, device=DEV)
    bad = [lambda: DT.nearest_seed(good.cpu()), lambda: DT.nearest_seed(good.to(torch.int32)), lambda: DT.nearest_seed(wide[:, ::2]),
           lambda: DT.nearest_seed(good[0]), lambda: DT.nearest_seed(big), lambda: DT.nearest_seed(good[:0]), lambda: DT.nearest_seed(good, to="edge"),
           lambda: DT.nearest_seed(good, to="set", ignore=good), lambda: DT.nearest_seed(good, to="boundary", ignore=good.cpu()),
           lambda: DT.nearest_seed(good, to="boundary", ignore=good[:, :39]), lambda: DT.nearest_seed(good, to="boundary", ignore=lab),
           lambda: DT.expand_labels(lab.cpu(), 1), lambda: DT.expand_labels(good, 1), lambda: DT.expand_labels(lab.to(torch.int64), 1),
           lambda: DT.expand_labels(lab[0], 1), lambda: DT.expand_labels(lab[:, ::2], 1), lambda: DT.expand_labels(lab, -1),
           lambda: DT.expand_labels(lab, float("nan")), lambda: DT.expand_labels(lab[:0], 1),
           lambda: DT.expand_labels(torch.zeros((1, 16385), dtype=torch.int32, device=DEV), 1),
           lambda: OB.split_objects(good.cpu(), 2), lambda: OB.split_objects(lab, 2), lambda: OB.split_objects(wide[:, ::2], 2),
           lambda: OB.split_objects(big, 2), lambda: OB.split_objects(good, -1), lambda: OB.split_objects(good, float("nan")),
           lambda: OB.split_objects(good, 2, min_core_area=-1), lambda: OB.split_objects(good, 2, connectivity=6),
           lambda: OB.split_objects(good, 2, mask_value=0), lambda: OB.split_objects(good, 2, mask_value=256)]
    for k, call in enumerate(bad):
        with pytest.raises(_lib.StcdError):
            call()
    assert bool((DT.nearest_seed(good, to="unset").view(-1) == torch.arange(48 * 40, device=DEV)).all())
    assert not bool(DT.expand_labels(lab, 3).any()) and OB.split_objects(good, 2).n_cores == 0


def test_the_abi_directly_and_its_refusals():
    H, W = 44, 40
    mask_h = np.array(all_patterns((96, 96))["rings"])[:H, :W].copy()
    values_h = np.arange(1, H * W + 1, dtype=np.int32).reshape(H, W)
    l = _lib.lib()
    assert l.stcd_edt_nearest_scratch_bytes(H, W) == l.stcd_edt_scratch_bytes(H, W) > 0
    assert l.stcd_edt_nearest_scratch_bytes(0, W) == 0 and l.stcd_edt_nearest_scratch_bytes(H, 16385) == 0
    nbytes = int(l.stcd_edt_nearest_scratch_bytes(H, W)) + 64   # a larger buffer is fine
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    mask, values = dev(mask_h), dev(values_h)
    index = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    out = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    cut = torch.full((H, W), 0x5A, dtype=torch.uint8, device=DEV)
    owner = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), 100, dtype=torch.int64, device=DEV)
    odd = torch.zeros(4 * H * W + 8, dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def near(m=mask, ig=None, h=H, w=W, seeds=1, d=d2, ix=index, s=scratch, nb=nbytes):
        return l.stcd_edt_nearest(p(m), p(ig), h, w, seeds, p(d), p(ix), p(s), nb, stream), l.stcd_last_error().decode()

    def gather(m=mask, h=H, w=W, seeds=1, q=4, v=values, o=out, s=scratch, nb=nbytes):
        return l.stcd_edt_gather(p(m), h, w, seeds, q, p(v), p(o), p(s), nb, stream), l.stcd_last_error().decode()

    def split(m=mask, l0=values, lc=values, ix=index, h=H, w=W, value=9, o=cut, ow=owner, c=counts):
        return l.stcd_objects_split_cut(p(m), p(l0), p(lc), p(ix), h, w, value, p(o), p(ow), p(c), stream), l.stcd_last_error().decode()

    # refused on the host, nothing launched: the outputs and the scratch buffer keep their fill
    for kw in (dict(m=None), dict(ix=None), dict(s=None), dict(h=0), dict(w=16385), dict(seeds=3), dict(seeds=-1), dict(ig=mask), dict(nb=nbytes - 72),
               dict(nb=0), dict(s=scratch[4:]), dict(ix=odd[1:]), dict(d=odd[2:])):
        rc, err = near(**kw)
        assert rc != 0 and err.startswith("stcd_edt_nearest: "), kw
    for kw in (dict(m=None), dict(v=None), dict(o=None), dict(s=None), dict(h=16385), dict(seeds=3), dict(q=-1), dict(o=values), dict(o=mask),
               dict(v=odd[1:]), dict(o=odd[2:]), dict(nb=nbytes - 72), dict(s=scratch[8:])):
        rc, err = gather(**kw)
        assert rc != 0 and err.startswith("stcd_edt_gather: "), kw
    for kw in (dict(m=None), dict(l0=None), dict(lc=None), dict(ix=None), dict(o=None), dict(c=None), dict(h=0), dict(w=16385), dict(value=0),
               dict(value=256), dict(o=mask), dict(l0=odd[1:]), dict(ow=odd[2:]), dict(c=odd[4:])):
        rc, err = split(**kw)
        assert rc != 0 and err.startswith("stcd_objects_split_cut: "), kw
    assert "scratch too small" in near(nb=nbytes - 72)[1] and "values" in gather(o=values)[1]
    for t, fill in ((index, -7), (d2, -7), (out, -7), (owner, -7), (cut, 0x5A), (counts, 100), (scratch, 0xAB)):
        assert bool((t == fill).all())
    want = N.nearest_seed(mask_h, "set")
    rc, err = near(d=None)
    assert rc == 0, err
    assert np.array_equal(host(index), want) and bool((d2 == -7).all())                     # no d2 plane asked for, none written
    rc, err = near(seeds=2, ig=dev(SP.overlay_for(H, W)))
    assert rc == 0, err
    assert np.array_equal(host(index), N.nearest_seed(mask_h, "boundary", SP.overlay_for(H, W)))
    assert np.array_equal(host(d2), E.squared_distance(mask_h, "boundary", SP.overlay_for(H, W)))
    rc, err = gather()
    assert rc == 0, err
    assert np.array_equal(host(out), N.gather(mask_h != 0, values_h, 4))
    rc, err = gather(q=2 ** 31 - 1)                             # no seed is within no q; here every pixel has one
    assert rc == 0, err
    assert np.array_equal(host(out), want + 1)
    # the cut pass on planes of its own: every pixel its own core, one component; an index out of range counts as none
    rc, err = near(d=None)
    assert rc == 0, err
    index[0, 0] = H * W
    index[0, 1] = -5
    ones = torch.ones((H, W), dtype=torch.int32, device=DEV)
    full = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    rc, err = split(m=full, l0=ones, ow=None)
    assert rc == 0, err
    assert bool((owner == -7).all())
    rc, err = split(m=full, l0=ones)
    assert rc == 0, err
    own = want + 1
    own[0, 0] = own[0, 1] = 0
    pad = np.zeros((H + 1, W + 2), np.int64)
    pad[:H, 1:W + 1] = own
    hit = np.zeros((H, W), bool)
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        nb = pad[dy:dy + H, 1 + dx:1 + dx + W]
        hit |= (own != 0) & (nb != 0) & (nb != own)
    assert np.array_equal(host(owner), own) and np.array_equal(host(cut), np.where(hit, 0, 9))
    assert host(counts).tolist() == [int(hit.sum()), 2, 100, 100]                          # cleared, two counters
    assert bool((scratch[nbytes - 64:] == 0xAB).all())          # nothing past the bytes the entry asks for
