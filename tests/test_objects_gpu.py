"""Change objects on the GPU: label_components, object_table, filter_objects, match_objects and refine_round against the numpy
specification of tests/objects_spec.py.  Every output is an integer and every assertion is equality.  The shapes put objects on
zero, one and several tile seams (T = objects.TILE) and use widths that are no multiple of anything."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stcd_amd import _lib, synth
from stcd_amd import objects as OB
from stcd_amd import selftrain as ST
from stcd_amd.metrics import scores_from_cm
from tests import objects_spec as SP
from tests import scene_round_spec as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = OB.TILE
SHAPES = [(1, 1), (1, T + 3), (T + 3, 1), (T, T), (T + 1, T + 1), (2 * T + 5, 3 * T - 1), (3 * T, 3 * T), (37, 131)]
FILTERS = [(1, 0), (5, 0), (0, 6), (4, 9), (0, 10 ** 9)]
ids = lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else str(s)


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)               # a copy: the shared patterns are read-only


def host(t):
    return t.cpu().numpy()


# the references: computed once per (shape, pattern, arguments), shared by the tests and never written to
@functools.lru_cache(maxsize=None)
def want_label(shape, name, conn, invert=False):
    lab, n = SP.label(SP.patterns(*shape, T)[name], conn, invert)
    lab.setflags(write=False)
    return lab, n


@functools.lru_cache(maxsize=None)
def want_filter(shape, name, conn, min_area, max_hole):
    out = SP.filter_objects(SP.patterns(*shape, T)[name], min_area, max_hole, conn, 255)
    out.setflags(write=False)
    return out


def _check_table(got: OB.ObjectTable, lab, n, overlay, where):
    area, bbox, overlap = SP.table(lab, n, overlay)
    assert got.area.dtype == torch.int64 and got.bbox.dtype == torch.int32 and tuple(got.area.shape) == (n,) and tuple(got.bbox.shape) == (n, 4), where
    assert np.array_equal(host(got.area), area), where
    assert np.array_equal(host(got.bbox), bbox), where
    if overlay is None:
        assert got.overlap is None, where
    else:
        assert got.overlap.dtype == torch.int64 and np.array_equal(host(got.overlap), overlap), where


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_labels_count_and_table_equal_the_spec(shape, conn):
    overlay = SP.overlay_for(*shape)
    d_overlay = dev(overlay)
    for name, m in SP.patterns(*shape, T).items():
        d = dev(m)
        for invert in (False, True):
            lab, n = want_label(shape, name, conn, invert)
            got = OB.label_components(d, conn, invert=invert)
            assert got.labels.dtype == torch.int32 and tuple(got.labels.shape) == shape
            assert got.count == n, (name, invert, got.count, n)
            assert np.array_equal(host(got.labels), lab), (name, invert)
            if not invert:
                _check_table(OB.object_table(got, d_overlay), lab, n, overlay, name)
                _check_table(OB.object_table(got), lab, n, None, name)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_filtered_mask_equals_the_spec(shape, conn):
    for name, m in SP.patterns(*shape, T).items():
        d = dev(m)
        for min_area, max_hole in FILTERS:
            got = OB.filter_objects(d, min_area, max_hole, conn)
            assert got.dtype == torch.uint8 and got.data_ptr() != d.data_ptr()
            assert np.array_equal(host(got), want_filter(shape, name, conn, min_area, max_hole)), (name, min_area, max_hole)
        assert torch.equal(d, dev(m))                           # the input is left alone
        unchecked = OB.filter_objects(d, 4, 9, conn, check=False)
        assert np.array_equal(host(unchecked), want_filter(shape, name, conn, 4, 9)), name
        assert np.array_equal(host(OB.filter_objects(d, 4, 9, conn, mask_value=1)), want_filter(shape, name, conn, 4, 9) // 255), name


def test_the_known_counts():
    shape = (2 * T + 5, 3 * T - 1)
    H, W = shape
    p = SP.patterns(*shape, T)
    count = lambda name, conn: OB.label_components(dev(p[name]), conn).count
    assert count("empty", 8) == 0 and count("full", 4) == 1 and count("corners", 8) == 4
    assert count("checkerboard", 8) == 1 and count("checkerboard", 4) == (H * W + 1) // 2
    for name in ("serpentine", "spiral", "comb"):
        assert count(name, 4) == 1 and count(name, 8) == 1, name
    for name in ("corner_diag_main", "corner_diag_anti"):      # where four tiles meet
        assert count(name, 8) == 1 and count(name, 4) == 2, name


def test_a_megapixel_at_the_percolation_threshold():
    m = (np.random.default_rng(7).random((1024, 1024)) < 0.593).astype(np.uint8)
    lab, n = SP.label(m, 4)
    d = dev(m)
    got = OB.label_components(d, 4)
    assert got.count == n and np.array_equal(host(got.labels), lab)
    overlay = (np.random.default_rng(8).random((1024, 1024)) < 0.3).astype(np.uint8)
    _check_table(OB.object_table(got, dev(overlay)), lab, n, overlay, "1024")
    # step 1 of the filter from the same labelling: an object stays if its area reaches min_area
    area = np.bincount(lab.ravel(), minlength=n + 1)
    area[0] = 0
    assert np.array_equal(host(OB.filter_objects(d, 40, 0, 4)), (area >= 40)[lab].astype(np.uint8) * 255)


def test_misaligned_masks_and_odd_widths():
    """No alignment demand: the mask, the output's width and the overlay start at odd addresses."""
    H, W = T + 9, 131
    m = SP.patterns(H, W, T)["noise_0.593"]
    buf = torch.zeros(H * W + 3, dtype=torch.uint8, device=DEV)
    d = buf[3:].view(H, W)
    d.copy_(dev(m))
    assert d.data_ptr() % 2 == 1 and d.is_contiguous()
    got = OB.label_components(d, 8)
    lab, n = want_label((H, W), "noise_0.593", 8)
    assert got.count == n and np.array_equal(host(got.labels), lab)
    obuf = torch.zeros(H * W + 1, dtype=torch.uint8, device=DEV)
    o = obuf[1:].view(H, W)
    overlay = SP.overlay_for(H, W)
    o.copy_(dev(overlay))
    _check_table(OB.object_table(got, o), lab, n, overlay, "misaligned")
    assert np.array_equal(host(OB.filter_objects(d, 6, 12, 8)), want_filter((H, W), "noise_0.593", 8, 6, 12))


def test_two_runs_give_the_same_bits():
    shape = (2 * T + 5, 3 * T - 1)
    for name in ("noise_0.407", "noise_0.593", "spiral"):
        d = dev(SP.patterns(*shape, T)[name])
        overlay = dev(SP.overlay_for(*shape))
        runs = []
        for _ in range(2):
            c = OB.label_components(d, 8)
            t = OB.object_table(c, overlay)
            runs.append((c.labels.clone(), c.count, t.area, t.bbox, t.overlap, OB.filter_objects(d, 7, 11, 8), OB.filter_objects(d, 7, 11, 8, check=False)))
        a, b = runs
        assert a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[:1] + a[2:], b[:1] + b[2:])), name
        assert torch.equal(a[5], a[6]), name                    # check=False is the same mask


def test_the_abi_directly_status_word_and_custom_value():
    H, W = T + 1, T + 1
    m = SP.patterns(H, W, T)["noise_0.407"]
    d, out = dev(m), torch.full((H, W), 77, dtype=torch.uint8, device=DEV)
    nbytes = int(_lib.lib().stcd_objects_scratch_bytes(H, W)) + 64                          # a larger buffer: the status word is at ITS end
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(_lib.lib().stcd_mask_filter_objects(p(d), H, W, 4, 3, 5, 9, p(out), p(scratch), nbytes, stream))
    assert np.array_equal(host(out), want_filter((H, W), "noise_0.407", 4, 3, 5) // 255 * 9)
    assert host(scratch[-4:]).view(np.int32)[0] == 0
    labels = torch.full((H, W), -5, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().stcd_objects_label(p(d), H, W, 8, 1, p(labels), p(count), p(scratch), nbytes, stream))
    lab, n = want_label((H, W), "noise_0.407", 8, True)
    assert int(count.item()) == n and np.array_equal(host(labels), lab) and host(scratch[-4:]).view(np.int32)[0] == 0
    # the table is overwritten, not added to, and a label past n is skipped
    area = torch.full((n,), 99, dtype=torch.int64, device=DEV)
    bbox = torch.full((n, 4), 99, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().stcd_objects_table(p(labels), H, W, n, None, p(area), p(bbox), None, stream))
    want_area, want_bbox, _ = SP.table(lab, n)
    assert np.array_equal(host(area), want_area) and np.array_equal(host(bbox), want_bbox)
    if n > 1:
        _lib.check(_lib.lib().stcd_objects_table(p(labels), H, W, n - 1, None, p(area), p(bbox), None, stream))
        assert np.array_equal(host(area)[:n - 1], want_area[:n - 1]) and host(area)[n - 1] == want_area[n - 1]


@pytest.mark.parametrize("conn", [4, 8])
def test_match_objects_counts_equal_the_spec(conn):
    shape = (2 * T + 5, 3 * T - 1)
    label = SP.overlay_for(*shape)
    d_label = dev(label)
    for name, m in SP.patterns(*shape, T).items():
        got = OB.match_objects(dev(m), d_label, conn, 0.5)
        want = SP.match_counts(m, label, conn, 0.5)
        assert (got.n_pred, got.n_label, got.tp_pred, got.tp_label) == want, name
        assert got.precision == (want[2] / want[0] if want[0] else 0.0) and got.recall == (want[3] / want[1] if want[1] else 0.0), name
    # a prediction against itself: every object is found
    m = SP.patterns(*shape, T)["noise_0.407"]
    same = OB.match_objects(dev(m), dev((m != 0).astype(np.uint8)), conn)
    assert same.n_pred == same.tp_pred == same.n_label == same.tp_label == SP.label(m, conn)[1] and same.f1 == 1.0
    with pytest.raises(_lib.StcdError):
        OB.match_objects(dev(m), d_label[:-1])


def test_wrappers_refuse_bad_arguments():
    d = dev(np.zeros((8, 8), np.uint8))
    for call in (lambda: OB.label_components(d, 6), lambda: OB.filter_objects(d, 4, -1), lambda: OB.filter_objects(d, 4, 4, 5),
                 lambda: OB.filter_objects(d, 4, 4, 8, mask_value=0), lambda: OB.label_components(d.to(torch.int32)),
                 lambda: OB.label_components(d[:, ::2]), lambda: OB.object_table(OB.Components(d, 0)),
                 lambda: OB.object_table(OB.label_components(d), overlay=d[:4])):
        with pytest.raises(_lib.StcdError):
            call()
    empty = torch.zeros((0, 5), dtype=torch.uint8, device=DEV)
    assert OB.label_components(empty).count == 0 and tuple(OB.filter_objects(empty, 3, 3).shape) == (0, 5)


def test_refine_round_on_a_real_scene_round():
    from stcd_amd.modules import SiamUnet_diff
    H = W = 256
    a, b, lab = synth.make_pairs_u8(1, H, W, seed=33)
    a, b, lab = a[0], b[0], lab[0].copy()
    lab[:4, :] = 255
    torch.manual_seed(710)
    model = SiamUnet_diff(3, 1, dtype="fp32").to(DEV)
    rnd = ST.scene_round(model, a, b, cell=128, tile=128, label=lab, stem="t")
    pseudo = host(rnd.pseudo)
    assert 0 < np.count_nonzero(pseudo) < pseudo.size          # the checkpoint sees something
    for min_area, max_hole, conn in ((12, 20, 8), (3, 0, 4)):
        out = ST.refine_round(rnd, min_area=min_area, max_hole=max_hole, connectivity=conn, label=lab)
        want = SP.filter_objects(pseudo, min_area, max_hole, conn, 255)
        assert np.array_equal(host(out.pseudo), want)
        _, cm = RS.cell_agree([want], 128, lab)
        assert np.array_equal(out.cell_cm, cm.reshape(2, 2, 2, 2)) and np.array_equal(out.cm, cm.sum(axis=0).reshape(2, 2))
        ws = scores_from_cm(cm.sum(axis=0).reshape(2, 2))
        np.testing.assert_equal(out.scores, ws)                # equality that takes NaN (an empty class) as equal
        assert out.masks is rnd.masks and out.names is rnd.names and out.reliable is rnd.reliable and out.cell == 128
    bare = ST.refine_round(rnd, min_area=12)
    assert bare.cm is None and bare.scores is None and np.array_equal(host(bare.pseudo), SP.filter_objects(pseudo, 12, 0, 8, 255))
