"""Whole-scene inference for SegCD's three maps and for UnetSeg on the GPU: stcd_scene_gather_one_d4, stcd_scene_stitch_heads_d4 and
stcd_scene_finalize_seg through the C ABI against the single-head entries and the numpy specifications, then predict_scene_seg,
predict_scene_heads and scene_round(gate="seg") end to end.

Tolerances.  The three entries promise the bits of the entries they generalise, so the kernel tests are equalities (floats compared
by torch.equal, probabilities with a NaN by their bit patterns).  The end-to-end tests compare with a host composition built from the
float64 specifications; they are made exact by construction instead of by a tolerance: the stand-in networks round their INPUT to
multiples of 1/8 (the spec gather and the kernel differ by at most 2e-6, tests/test_scene_gpu.py; the nearest rounding boundary of any
normalised byte value is 1.1e-4 away, asserted below), have weights that are multiples of 1/4 and use elementwise arithmetic only, so
both sides see the same logits, multiples of 1/32 below 64 in size.  With the flat window the sums are then exact in fp32 (at most 4
covering tiles x 2 views x 2 models of 17-bit numbers), ties included, although a pixel's logit there depends on the tile and the
view (the stand-ins' shifted term).  With the Hann window acc differs from the spec by about 1e-6 of wsum * max|logits|
(test_scene_gpu.py), so a mask can differ where a decision is that close; sums of different dyadic logits under equal weights (the
same tile in two views) cancel exactly in mathematics and by rounding only in floating point, so there the stand-ins drop the shifted
term and a second checkpoint is the first with doubled weights: every covering tile, view and checkpoint then gives a pixel a
logit of the same sign, and the test asserts on the SPEC's numbers that every decision
is either an exact tie (all covering logits equal: a tie on both sides) or clear by 1e-4 on that scale before it holds the masks,
the gate and the matrices to equality.  Probabilities keep test_scene_gpu.py's bound, atol 1e-6 (flat) and 1e-5 (Hann)."""
import ctypes as C

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import selftrain as ST
from stcd_amd.pseudo import MEAN, STD
from stcd_amd.scene import SceneHeads, plan_tiles, predict_scene, predict_scene_heads, predict_scene_seg, window_table
from tests import scene_heads_spec as HS
from tests import scene_round_spec as RS
from tests import scene_spec as SP
from tests import scene_tta_spec as TS
from tests import selftrain_spec as SS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the vector path, a scene smaller than a tile, odd width with one staging patch and a partial one, T % 4 != 0, several patches
SHAPES = [(100, 70, 64, 32), (1, 5, 64, 64), (130, 67, 72, 40), (100, 70, 30, 14), (257, 255, 128, 64)]
CASES = [(shape, d) for i, shape in enumerate(SHAPES) for d in (range(8) if i in (0, 3) else (0, 3, 5))]
CASE_IDS = ["{}x{}-T{}-S{}-d{}".format(*shape, d) for shape, d in CASES]
# small grids, T % 4 == 0 and T % 4 != 0, on which view 0 is also held against the pair entry without d4
UPRIGHT_CASES = [((20, 13, 8, 4), 0), ((17, 9, 6, 3), 0)]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scene(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def _offset_by_one(shape, fill=0.0):
    """A contiguous fp32 view that starts 4 bytes past a 16-byte boundary, and its buffer."""
    buf = torch.full((int(np.prod(shape)) + 1,), fill, dtype=torch.float32, device=DEV)
    view = buf[1:].view(shape)
    assert view.data_ptr() % 16 == 4
    return view, buf


M3, S3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)


# ------------------------------------------------------------------ 1. gather_one_d4
def gather_one(scene, T, S, first, n, d, out=None):
    H, W, _ = scene.shape
    plan = plan_tiles(H, W, T, S)
    x = torch.full((n, 3, T, T), float("nan"), dtype=torch.float32, device=DEV) if out is None else out
    _lib.check(_lib.lib().stcd_scene_gather_one_d4(_p(scene), H, W, T, S, plan.tiles_x, first, n, M3, S3, _p(x), d, _stream()))
    return x


def gather_pair_x1(scene, T, S, first, n, d):
    H, W, _ = scene.shape
    plan = plan_tiles(H, W, T, S)
    x1 = torch.full((n, 3, T, T), float("nan"), dtype=torch.float32, device=DEV)
    x2 = torch.full_like(x1, float("nan"))
    _lib.check(_lib.lib().stcd_scene_gather_d4(_p(scene), _p(scene), H, W, T, S, plan.tiles_x, first, n, M3, S3, _p(x1), _p(x2), d, _stream()))
    assert torch.equal(x1, x2)
    return x1


@pytest.mark.parametrize("shape,d", CASES + UPRIGHT_CASES, ids=CASE_IDS + ["{}x{}-T{}-S{}-d{}".format(*shape, d) for shape, d in UPRIGHT_CASES])
def test_gather_one_is_x1_of_the_pair_gather_on_the_same_scene(shape, d):
    H, W, T, S = shape
    scene = _dev(_scene(H, W, 3 + H + T)[0])
    plan = plan_tiles(H, W, T, S)
    want = gather_pair_x1(scene, T, S, 0, plan.n, d)
    got = gather_one(scene, T, S, 0, plan.n, d)
    assert not torch.isnan(got).any() and torch.equal(got, want)
    if d == 0:                                                         # the pair entry without d4 writes the same x1 and x2
        x1 = torch.full_like(want, float("nan"))
        x2 = torch.full_like(want, float("nan"))
        _lib.check(_lib.lib().stcd_scene_gather(_p(scene), _p(scene), H, W, T, S, plan.tiles_x, 0, plan.n, M3, S3, _p(x1), _p(x2), _stream()))
        assert torch.equal(x1, want) and torch.equal(x2, want)
    if plan.n > 2:                                                     # a range that does not start at tile 0
        first = plan.n // 2
        assert torch.equal(gather_one(scene, T, S, first, plan.n - first, d), want[first:])


def test_gather_one_unaligned_output_takes_the_scalar_path():
    H, W, T, S = SHAPES[0]
    scene = _dev(_scene(H, W, 5)[0])
    plan = plan_tiles(H, W, T, S)
    for d in range(8):
        view, buf = _offset_by_one((plan.n, 3, T, T))
        gather_one(scene, T, S, 0, plan.n, d, out=view)
        assert torch.equal(view, gather_pair_x1(scene, T, S, 0, plan.n, d)), d
        assert float(buf[0]) == 0.0


# ------------------------------------------------------------------ 2. stitch_heads_d4
def stitch_single(logits, H, W, T, S, window, acc, wsum, d, chunk=None):
    plan = plan_tiles(H, W, T, S)
    chunk = logits.shape[0] if chunk is None else chunk
    for first in range(0, logits.shape[0], chunk):
        part = logits[first:first + chunk]
        _lib.check(_lib.lib().stcd_scene_stitch_d4(_p(part), part.shape[1], H, W, T, S, plan.tiles_x, plan.tiles_y, first, part.shape[0],
                                                   _p(window), _p(acc), _p(wsum), d, _stream()))


def stitch_heads(heads, H, W, T, S, window, acc, wsum, d, chunk=None):
    """heads: a list of [n,classes,T,T] tensors; every tile into acc [len(heads) * classes, H, W] / wsum, `chunk` tiles per call."""
    plan = plan_tiles(H, W, T, S)
    total, classes = heads[0].shape[0], heads[0].shape[1]
    chunk = total if chunk is None else chunk
    for first in range(0, total, chunk):
        parts = [h[first:first + chunk] for h in heads]
        ptrs = (C.c_void_p * len(parts))(*[t.data_ptr() for t in parts])
        _lib.check(_lib.lib().stcd_scene_stitch_heads_d4(ptrs, len(parts), classes, H, W, T, S, plan.tiles_x, plan.tiles_y, first,
                                                         parts[0].shape[0], _p(window), _p(acc), _p(wsum), d, _stream()))


def _zeros(planes, H, W):
    return torch.zeros((planes, H, W), dtype=torch.float32, device=DEV), torch.zeros((H, W), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("shape,d", CASES, ids=CASE_IDS)
def test_stitch_heads_is_the_single_head_stitch_per_head(shape, d):
    H, W, T, S = shape
    plan = plan_tiles(H, W, T, S)
    gen = torch.Generator().manual_seed(4 + H + d)
    win = _dev(window_table(T, "hann"))
    for classes in (1, 2):
        logits = [torch.randn((plan.n, classes, T, T), generator=gen).to(DEV) for _ in range(3)]
        alone = []
        for lg in logits:                                              # every head alone, its own zeroed acc and wsum
            acc, wsum = _zeros(classes, H, W)
            stitch_single(lg, H, W, T, S, win, acc, wsum, d)
            alone.append((acc, wsum))
        for n_heads in (1, 2, 3):
            for chunk in (None, 3):                                    # one call, and calls of 3 tiles
                acc, wsum = _zeros(n_heads * classes, H, W)
                stitch_heads(logits[:n_heads], H, W, T, S, win, acc, wsum, d, chunk)
                for h in range(n_heads):
                    assert torch.equal(acc[h * classes:(h + 1) * classes], alone[h][0]), (classes, n_heads, chunk, h)
                    assert torch.equal(wsum, alone[h][1]), (classes, n_heads, chunk, h)
        assert float(alone[0][1].min()) > 0.0


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=["64-32", "30-14"])
def test_stitch_heads_chain_of_views_into_one_acc(shape):
    H, W, T, S = shape
    plan = plan_tiles(H, W, T, S)
    gen = torch.Generator().manual_seed(8)
    win = _dev(window_table(T, "hann"))
    for classes in (1, 2):
        views = {d: [torch.randn((plan.n, classes, T, T), generator=gen).to(DEV) for _ in range(3)] for d in (0, 6, 1)}
        acc, wsum = _zeros(3 * classes, H, W)
        for d in (0, 6, 1):
            stitch_heads(views[d], H, W, T, S, win, acc, wsum, d, chunk=4)
        for h in range(3):
            acc1, wsum1 = _zeros(classes, H, W)
            for d in (0, 6, 1):
                stitch_single(views[d][h], H, W, T, S, win, acc1, wsum1, d)
            assert torch.equal(acc[h * classes:(h + 1) * classes], acc1) and torch.equal(wsum, wsum1), (classes, h)


def test_stitch_heads_unaligned_acc_and_odd_width():
    H, W, T, S = SHAPES[2]
    assert W == 67
    plan = plan_tiles(H, W, T, S)
    gen = torch.Generator().manual_seed(10)
    win = _dev(window_table(T, "hann"))
    for d in (0, 3, 5):
        logits = [torch.randn((plan.n, 2, T, T), generator=gen).to(DEV) for _ in range(3)]
        acc, buf = _offset_by_one((6, H, W))
        wsum = torch.zeros((H, W), dtype=torch.float32, device=DEV)
        stitch_heads(logits, H, W, T, S, win, acc, wsum, d)
        for h in range(3):
            acc1, wsum1 = _zeros(2, H, W)
            stitch_single(logits[h], H, W, T, S, win, acc1, wsum1, d)
            assert torch.equal(acc[2 * h:2 * h + 2], acc1) and torch.equal(wsum, wsum1), (d, h)
        assert float(buf[0]) == 0.0


def _dyadic(shape, rng, lim=512):
    return (rng.integers(-lim, lim + 1, size=shape) / 64.0).astype(np.float32)


@pytest.mark.parametrize("shape,d", CASES, ids=CASE_IDS)
def test_stitch_heads_dyadic_flat_window_is_exact(shape, d):
    """Multiples of 2^-6 within +-8 and at most 16 covering tiles: every sum is exact in fp32 and must equal the float64 spec."""
    H, W, T, S = shape
    plan = plan_tiles(H, W, T, S)
    rng = np.random.default_rng(H + S + d)
    for classes in (1, 2):
        logits = [_dyadic((plan.n, classes, T, T), rng) for _ in range(3)]
        acc, wsum = _zeros(3 * classes, H, W)
        stitch_heads([_dev(l) for l in logits], H, W, T, S, None, acc, wsum, d, chunk=5)
        got = acc.cpu().numpy().astype(np.float64)
        for h in range(3):
            want_acc, want_wsum = TS.stitch_d4(logits[h], H, W, T, S, plan.tiles_x, plan.tiles_y, 0, None, np.zeros((classes, H, W)),
                                               np.zeros((H, W)), d)
            assert want_wsum.min() >= 1 and want_wsum.max() <= 16
            np.testing.assert_array_equal(got[h * classes:(h + 1) * classes], want_acc, err_msg=f"head {h}")
            np.testing.assert_array_equal(wsum.cpu().numpy().astype(np.float64), want_wsum)


# ------------------------------------------------------------------ 3. finalize_seg
SEG_THR, CHG_THR = 0.25, -0.5


def _planes(H, W, classes, seed):
    """Dyadic planes (every comparison is exact in fp32 and in the float64 spec), ties and a NaN planted in every head."""
    rng = np.random.default_rng(seed)
    wsum = (rng.integers(1, 17, size=(H, W)) / 4.0).astype(np.float32)
    acc = _dyadic((3 * classes, H, W), rng, 256)
    tie = rng.random((H, W)) < 0.1
    tie[0, 0] = tie[-1, -1] = True
    for h in range(3):
        if classes == 2:
            acc[2 * h + 1][tie] = acc[2 * h][tie]
        else:
            acc[h][tie] = ((CHG_THR if h == 2 else SEG_THR) * wsum)[tie]
    nan = (H // 2, W // 2)
    acc[:, nan[0], nan[1]] = np.nan
    tie[nan] = False
    labels = [rng.choice(np.array([0, 0, 1, 2, 200, 255], np.uint8), size=(H, W)) for _ in range(3)]
    labels[2][0, :] = 255
    return acc, wsum, tie, nan, labels


def finalize_seg(acc, wsum, classes, labels=(None, None, None), want_gated=True, want_prob=True, cm=None):
    H, W = wsum.shape
    out = torch.full((4, H, W), 9, dtype=torch.uint8, device=DEV)
    prob = torch.full((3, H, W), -1.0, dtype=torch.float32, device=DEV) if want_prob else None
    if cm is None and any(l is not None for l in labels):
        cm = torch.zeros((4, 4), dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().stcd_scene_finalize_seg(_p(acc), _p(wsum), classes, H, W, C.c_float(SEG_THR), C.c_float(CHG_THR), _p(labels[0]),
                                                  _p(labels[1]), _p(labels[2]), _p(out[0]), _p(out[1]), _p(out[2]),
                                                  _p(out[3]) if want_gated else None, _p(prob), _p(cm), _stream()))
    return out, prob, cm


def finalize_one(acc, wsum, classes, threshold, label=None):
    H, W = wsum.shape
    mask = torch.full((H, W), 9, dtype=torch.uint8, device=DEV)
    prob = torch.full((H, W), -1.0, dtype=torch.float32, device=DEV)
    cm = torch.zeros(4, dtype=torch.int64, device=DEV) if label is not None else None
    _lib.check(_lib.lib().stcd_scene_finalize(_p(acc), _p(wsum), classes, H, W, C.c_float(threshold), _p(label), _p(mask), _p(prob), _p(cm),
                                              _stream()))
    return mask, prob, cm


@pytest.mark.parametrize("classes", [2, 1])
@pytest.mark.parametrize("H,W", [(100, 72), (37, 67), (1, 5)])          # 16-byte path; odd width; one short row
def test_finalize_seg_is_finalize_per_head_and_the_spec(H, W, classes):
    acc_np, wsum_np, tie, nan, labels_np = _planes(H, W, classes, 3 * H + classes)
    acc, wsum, labels = _dev(acc_np), _dev(wsum_np), [_dev(l) for l in labels_np]
    out, prob, cm = finalize_seg(acc, wsum, classes, labels)
    for h, thr in enumerate((SEG_THR, SEG_THR, CHG_THR)):               # masks, prob and the matrix of every head: that entry's bits
        mask1, prob1, cm1 = finalize_one(acc[h * classes:(h + 1) * classes].contiguous(), wsum, classes, thr, labels[h])
        assert torch.equal(out[h], mask1), h
        assert torch.equal(prob[h].view(torch.int32), prob1.view(torch.int32)), h
        assert torch.equal(cm[h], cm1), h
    with np.errstate(invalid="ignore"):
        sa, sb, ch, gt, _, want_cm = HS.finalize_seg(acc_np, wsum_np, SEG_THR, CHG_THR, *labels_np)
    for got, want in zip(out.cpu().numpy(), (sa, sb, ch, gt)):
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cm.cpu().numpy(), want_cm)
    o = out.cpu().numpy()
    assert not o[:3][:, tie].any() and not o[:, nan[0], nan[1]].any()   # a tie and a NaN are class 0
    assert torch.equal(out[3], out[2] & (out[0] != out[1]).to(torch.uint8))
    if H > 1:
        assert 0 < int(out[3].sum()) < int(out[2].sum())
    # cm is added to; the row of an absent label and, without gated, row 3 are left untouched; masks do not depend on the options
    for absent in (0, 1, 2):
        given = [None if h == absent else l for h, l in enumerate(labels)]
        given_np = [None if h == absent else l for h, l in enumerate(labels_np)]
        preset = torch.arange(16, dtype=torch.int64, device=DEV).reshape(4, 4) * 1000 + 7
        out2, _, cm2 = finalize_seg(acc, wsum, classes, given, want_prob=False, cm=preset.clone())
        with np.errstate(invalid="ignore"):
            want2 = HS.finalize_seg(acc_np, wsum_np, SEG_THR, CHG_THR, *given_np, cm=preset.cpu().numpy())[-1]
        np.testing.assert_array_equal(cm2.cpu().numpy(), want2)
        for r in range(4):
            if min(r, 2) == absent:
                assert torch.equal(cm2[r], preset[r])
        assert torch.equal(out2, out)
    preset = torch.full((4, 4), -5, dtype=torch.int64, device=DEV)
    out3, _, cm3 = finalize_seg(acc, wsum, classes, labels, want_gated=False, cm=preset.clone())
    assert torch.equal(cm3[3], preset[3]) and torch.equal(cm3[:3], cm[:3] - 5)
    assert torch.equal(out3[:3], out[:3]) and bool((out3[3] == 9).all())
    out4, prob4, cm4 = finalize_seg(acc, wsum, classes)                 # no label at all: no cm
    assert cm4 is None and torch.equal(out4, out) and torch.equal(prob4.view(torch.int32), prob.view(torch.int32))


# ------------------------------------------------------------------ 4. rejections: nothing is launched, nothing is written
def test_abi_rejects_bad_arguments_and_writes_nothing():
    l = _lib.lib()
    H, W, T, S = SHAPES[0]
    plan = plan_tiles(H, W, T, S)
    scene = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    x = torch.full((plan.n, 3, T, T), 3.0, dtype=torch.float32, device=DEV)
    lg = [torch.ones((plan.n, 2, T, T), dtype=torch.float32, device=DEV) for _ in range(4)]
    acc = torch.full((8, H, W), 5.0, dtype=torch.float32, device=DEV)
    wsum = torch.full((H, W), 6.0, dtype=torch.float32, device=DEV)
    masks = torch.full((4, H, W), 9, dtype=torch.uint8, device=DEV)
    prob = torch.full((3, H, W), -1.0, dtype=torch.float32, device=DEV)
    cm = torch.full((4, 4), 11, dtype=torch.int64, device=DEV)
    label = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    st = _stream()

    def gather(d=0, n=plan.n, pa=scene):
        return l.stcd_scene_gather_one_d4(_p(pa), H, W, T, S, plan.tiles_x, 0, n, M3, S3, _p(x), d, st)

    def stitch(n_heads=3, classes=2, d=0, n=plan.n, null_at=None):
        vals = [None if h == null_at else t.data_ptr() for h, t in enumerate(lg[:max(n_heads, 1)])]
        ptrs = (C.c_void_p * len(vals))(*vals)
        return l.stcd_scene_stitch_heads_d4(ptrs, n_heads, classes, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, n, None, _p(acc), _p(wsum), d, st)

    def finalize(classes=2, la=None, lc=None, cm_=None, sa=masks[0]):
        return l.stcd_scene_finalize_seg(_p(acc), _p(wsum), classes, H, W, C.c_float(0.0), C.c_float(0.0), _p(la), None, _p(lc), _p(sa),
                                         _p(masks[1]), _p(masks[2]), _p(masks[3]), _p(prob), _p(cm_), st)

    for call, entry, word in ((lambda: stitch(n_heads=0), b"stcd_scene_stitch_heads_d4", b"n_heads"),
                              (lambda: stitch(n_heads=4), b"stcd_scene_stitch_heads_d4", b"n_heads"),
                              (lambda: stitch(classes=3), b"stcd_scene_stitch_heads_d4", b"classes"),
                              (lambda: stitch(d=8), b"stcd_scene_stitch_heads_d4", b"d4"),
                              (lambda: stitch(null_at=1), b"stcd_scene_stitch_heads_d4", b"null"),
                              (lambda: stitch(n=plan.n + 1), b"check_scene_grid", b"tile range"),         # the shared grid check reports under its own name
                              (lambda: gather(d=8), b"stcd_scene_gather_one_d4", b"d4"),
                              (lambda: gather(d=-1), b"stcd_scene_gather_one_d4", b"d4"),
                              (lambda: gather(pa=None), b"stcd_scene_gather_one_d4", b"null"),
                              (lambda: gather(n=-1), b"check_scene_grid", b"tile range"),
                              (lambda: finalize(classes=3), b"stcd_scene_finalize_seg", b"classes"),
                              (lambda: finalize(la=label), b"stcd_scene_finalize_seg", b"cm"),        # a label without cm
                              (lambda: finalize(lc=label), b"stcd_scene_finalize_seg", b"cm"),
                              (lambda: finalize(cm_=cm), b"stcd_scene_finalize_seg", b"cm"),          # cm without a label
                              (lambda: finalize(sa=None), b"stcd_scene_finalize_seg", b"null")):
        assert call() != 0
        err = l.stcd_last_error()
        assert entry in err and word in err, err
    for d in range(8):                                                 # an empty range is valid and launches nothing
        assert gather(d, n=0) == 0 and stitch(d=d, n=0) == 0
    torch.cuda.synchronize()
    assert bool((x == 3.0).all()) and bool((acc == 5.0).all()) and bool((wsum == 6.0).all())
    assert bool((masks == 9).all()) and bool((prob == -1.0).all()) and bool((cm == 11).all())


# ------------------------------------------------------------------ 5. the Python layer on stand-in networks
QUANT = 8.0


def test_the_stand_ins_cannot_see_the_gather_tolerance():
    """Every normalised byte value is at least 1e-4 from a rounding boundary of round(x * 8): 50 times the gather's 2e-6."""
    v = (np.arange(256)[:, None] / 255.0 - np.asarray(MEAN)) / np.asarray(STD)
    assert np.abs((v * QUANT) % 1.0 - 0.5).min() / QUANT > 1e-4


class _Maps(torch.nn.Module):
    """`outs` maps of `classes` channels from a fixed 3 -> outs * classes pointwise mix plus, with `shift`, one shifted term (so it
    is not D4-equivariant and a pixel's logit depends on the tile and the view), without a bias (equal scenes give all-zero maps:
    exact ties), in elementwise arithmetic on inputs rounded to 1/8 with weights that are multiples of 1/4: exact in fp32."""

    def __init__(self, outs, classes, seed, pair=True, shift=True, scale=1.0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        co = outs * classes
        self.w = torch.nn.Parameter(torch.randint(-4, 5, (co, 3), generator=g) / 4.0 * scale)
        self.v = torch.nn.Parameter(torch.randint(-4, 5, (co,), generator=g) / 4.0)
        self.outs, self.classes, self.pair, self.shift = outs, classes, pair, shift

    def forward(self, *xs):
        assert len(xs) == (2 if self.pair else 1)
        q = [torch.round(x * QUANT) / QUANT for x in xs]
        x = q[0] - q[1] if self.pair else q[0]
        shifted = torch.roll(x[:, 0], 1, -1) if self.shift else torch.zeros_like(x[:, 0])
        y = torch.stack([self.w[o, 0] * x[:, 0] + self.w[o, 1] * x[:, 1] + self.w[o, 2] * x[:, 2] + self.v[o] * shifted
                         for o in range(self.w.shape[0])], 1)
        if self.outs == 1:
            return y
        return tuple(y[:, h * self.classes:(h + 1) * self.classes] for h in range(self.outs))


def _stand_ins(outs, classes, seed, n_models, window, pair):
    """flat: independent checkpoints with the shifted term.  hann (module docstring): no shifted term, and checkpoint k is the first
    one with its weights times k + 1, so that two checkpoints never cancel at a pixel either."""
    if window == "flat":
        return [_Maps(outs, classes, seed + k, pair).to(DEV) for k in range(n_models)]
    return [_Maps(outs, classes, seed, pair, shift=False, scale=k + 1.0).to(DEV) for k in range(n_models)]


PH, PW, PT, PS, PB = 100, 150, 64, 48, 4


def _py_scene():
    a, b = _scene(PH, PW, 51)
    b[:40] = a[:40]                                                    # no difference: exact ties on a band of the scene
    rng = np.random.default_rng(52)
    labels = [rng.choice(np.array([0, 0, 1, 3, 255], np.uint8), size=(PH, PW)) for _ in range(3)]
    return a, b, labels


def _compose(models, views, scenes, window, batch):
    """The host composition, float64: spec gather of every view, the same modules on the same batches, the spec stitch.
    -> (acc [outs * classes, H, W], wsum, max |logit|)"""
    plan = plan_tiles(PH, PW, PT, PS)
    win = None if window == "flat" else window_table(PT, window)
    acc = wsum = None
    big = 0.0
    for m in models:
        m.eval()
        for d in views:
            for first in range(0, plan.n, batch):
                n = min(batch, plan.n - first)
                xs = [_dev(TS.gather_d4(s, PT, PS, plan.tiles_x, first, n, MEAN, STD, d).astype(np.float32)) for s in scenes]
                with torch.no_grad():
                    out = m(*xs)
                maps = [out] if torch.is_tensor(out) else list(out)
                logits = np.concatenate([t.float().cpu().numpy() for t in maps], 1)          # heads along the channel axis
                big = max(big, float(np.abs(logits).max()))
                if acc is None:
                    acc, wsum = np.zeros((logits.shape[1], PH, PW)), np.zeros((PH, PW))
                TS.stitch_d4(logits, PH, PW, PT, PS, plan.tiles_x, plan.tiles_y, first, win, acc, wsum, d)
    return acc, wsum, big


def _assert_decisions_are_clear(acc, wsum, big, classes, ties):
    """See the module docstring: on the spec's numbers every decision is an exact tie or clear of fp32's error by 100 times."""
    for h in range(acc.shape[0] // classes):
        a = acc[h * classes:(h + 1) * classes]
        diff = np.abs(a[1] - a[0]) if classes == 2 else np.abs(a[0])
        assert ((diff == 0) | (diff > 1e-4 * wsum * big)).all(), h
        assert (diff > 0).any() and (not ties or (diff[:40] == 0).all())


@pytest.mark.parametrize("n_models,tta", [(1, None), (1, (6, 1)), (2, None), (2, (6, 1))])
@pytest.mark.parametrize("classes", [2, 1])
@pytest.mark.parametrize("window", ["flat", "hann"])
def test_predict_scene_heads_is_the_host_composition(window, classes, n_models, tta):
    a, b, labels = _py_scene()
    models = _stand_ins(3, classes, 60, n_models, window, pair=True)
    model = models if n_models > 1 else models[0]
    kw = dict(tile=PT, stride=PS, window=window, tta=tta)
    res = predict_scene_heads(model, a, b, batch=PB, label=labels[2], label_a=labels[0], label_b=labels[1], return_prob=True, **kw)
    assert isinstance(res, SceneHeads)
    acc, wsum, big = _compose(models, (0,) if tta is None else tta, (a, b), window, PB)
    _assert_decisions_are_clear(acc, wsum, big, classes, ties=tta is None or window == "hann")  # the shifted term leaves the band in a transposed view
    sa, sb, ch, gt, prob, cm = HS.finalize_seg(acc, wsum, 0.0, 0.0, labels[0], labels[1], labels[2])
    for key, want in zip(HS.ROWS, (sa, sb, ch, gt)):
        got = getattr(res, key)
        assert got.dtype == torch.uint8 and got.device.type == "cuda" and tuple(got.shape) == (PH, PW)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=key)
    np.testing.assert_allclose(res.prob.cpu().numpy(), prob, rtol=0, atol=1e-6 if window == "flat" else 1e-5)
    assert sorted(res.cm) == sorted(HS.ROWS) and sorted(res.scores) == sorted(HS.ROWS)
    for r, key in enumerate(HS.ROWS):
        assert res.cm[key].shape == (2, 2) and res.cm[key].dtype == np.int64
        np.testing.assert_array_equal(res.cm[key].ravel(), cm[r], err_msg=key)
    assert 0 < int(res.gated.sum()) < int(res.change.sum()) < PH * PW
    if tta is None or window == "hann":
        assert not (res.seg_a[:40].any() or res.seg_b[:40].any() or res.change[:40].any())      # the tie band is class 0
    # the result does not depend on the batch, nor on the run; the change map is predict_scene's mask
    for batch in (1, PB):
        again = predict_scene_heads(model, a, b, batch=batch, return_prob=True, **kw)
        assert all(torch.equal(getattr(again, k), getattr(res, k)) for k in HS.ROWS + ("prob",)), batch
        assert again.cm == {} and again.scores == {}
    plain = predict_scene(model, a, b, batch=PB, label=labels[2], return_prob=True, **kw)
    assert torch.equal(res.change, plain.mask) and torch.equal(res.prob[2], plain.prob)
    np.testing.assert_array_equal(res.cm["change"], plain.cm)
    only_a = predict_scene_heads(model, a, b, batch=PB, label_a=labels[0], **kw)
    assert sorted(only_a.cm) == ["seg_a"] and only_a.prob is None
    np.testing.assert_array_equal(only_a.cm["seg_a"], res.cm["seg_a"])


# A one-class threshold that fp32 holds exactly and no logit of the stand-ins (multiples of 1/32) equals.  On a blended value exactly
# on a non-zero threshold the kernel's decision is rounding under the Hann window (acc adds the rounded weight, wsum the fused one:
# kernels_scene.hip), so the Hann cases must have no such pixel; under the flat window averages of different logits may hit it, and
# there the arithmetic is exact on both sides: class 0.
SEG_SCENE_THR = 19.0 / 64.0


@pytest.mark.parametrize("n_models,tta", [(1, None), (1, (6, 1)), (2, None), (2, (6, 1))])
@pytest.mark.parametrize("classes", [2, 1])
@pytest.mark.parametrize("window", ["flat", "hann"])
def test_predict_scene_seg_is_the_host_composition(window, classes, n_models, tta):
    a, _, labels = _py_scene()
    models = _stand_ins(1, classes, 70, n_models, window, pair=False)
    model = models if n_models > 1 else models[0]
    kw = dict(tile=PT, stride=PS, window=window, tta=tta, threshold=SEG_SCENE_THR)
    res = predict_scene_seg(model, a, batch=PB, label=labels[0], return_prob=True, **kw)
    acc, wsum, big = _compose(models, (0,) if tta is None else tta, (a,), window, PB)
    if classes == 2:
        diff = np.abs(acc[1] - acc[0])
    else:
        diff = np.abs(acc[0] - SEG_SCENE_THR * wsum)
    assert ((diff == 0) | (diff > 1e-4 * wsum * big)).all()
    if window == "hann" and classes == 1:
        assert (diff > 0).all()                                       # see SEG_SCENE_THR
    mask, prob, cm = SP.finalize(acc, wsum, SEG_SCENE_THR, labels[0])
    np.testing.assert_array_equal(res.mask.cpu().numpy(), mask)
    np.testing.assert_allclose(res.prob.cpu().numpy(), prob, rtol=0, atol=1e-6 if window == "flat" else 1e-5)
    np.testing.assert_array_equal(res.cm.ravel(), cm)
    assert 0 < int(res.mask.sum()) < PH * PW and res.scores is not None
    for batch in (1, PB):
        again = predict_scene_seg(model, a, batch=batch, return_prob=True, **kw)
        assert torch.equal(again.mask, res.mask) and torch.equal(again.prob, res.prob) and again.cm is None


class _Raises(torch.nn.Module):
    def __init__(self, after, pair):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.after, self.calls, self.pair = after, 0, pair

    def forward(self, *xs):
        self.calls += 1
        if self.calls > self.after:
            raise RuntimeError("boom")
        y = xs[0][:, :2] + self.w
        return (y, y, y) if self.pair else y


@pytest.mark.parametrize("training", [True, False])
def test_modes_are_restored_after_a_forward_that_raises(training):
    a, b = _scene(64, 64, 45)
    for pair in (True, False):
        good, bad = _Raises(10 ** 9, pair).to(DEV), _Raises(3, pair).to(DEV)
        good.train(training)
        bad.train(not training)
        with pytest.raises(RuntimeError, match="boom"):
            if pair:
                predict_scene_heads([good, bad], a, b, tile=32, stride=32, batch=2, tta="flip")
            else:
                predict_scene_seg([good, bad], a, tile=32, stride=32, batch=2, tta="flip")
        assert good.training is training and bad.training is (not training)
        assert good.calls == 8 and bad.calls == 4


class _Returns(torch.nn.Module):
    def __init__(self, what):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.what = what

    def forward(self, x1, x2=None):
        y = x1[:, :2] + self.w
        return self.what(y)


def test_anything_but_three_equal_maps_is_rejected():
    a, b = _scene(64, 64, 46)
    for what, word in ((lambda y: y, "one tensor"), (lambda y: [y], "list of 1"), (lambda y: [y] * 5, "list of 5"),
                       (lambda y: (y, y), "tuple of 2"), (lambda y: (y, y, y[:, :1]), "differ in shape"),
                       (lambda y: (y, y, y[..., :16]), "map 2"), (lambda y: (y, y, None), "NoneType")):
        with pytest.raises(_lib.StcdError, match=word):
            predict_scene_heads(_Returns(what).to(DEV), a, b, tile=32)
    for what, word in ((lambda y: (y, y, y), "tuple"), (lambda y: y[..., :16], "expected")):
        with pytest.raises(_lib.StcdError, match=word):
            predict_scene_seg(_Returns(what).to(DEV), a, tile=32)


# ------------------------------------------------------------------ 6. the real networks, once
def test_segcd_and_unetseg_share_a_checkpoint_on_one_scene():
    from stcd_amd.segcd import SegCD, UnetSeg
    torch.manual_seed(5)
    seg = SegCD("resnet18").to(DEV)
    unet = UnetSeg("resnet18")
    unet.load_state_dict(seg.state_dict())
    unet.to(DEV)
    H, W = 96, 128
    a, b = _scene(H, W, 81)
    kw = dict(tile=64, stride=32, batch=4, window="hann")
    res = predict_scene_heads(seg, a, b, return_prob=True, label=np.zeros((H, W), np.uint8), **kw)
    for key in HS.ROWS:
        t = getattr(res, key)
        assert t.dtype == torch.uint8 and tuple(t.shape) == (H, W) and t.device.type == "cuda" and int(t.max()) <= 1
    assert res.prob.dtype == torch.float32 and tuple(res.prob.shape) == (3, H, W) and bool(torch.isfinite(res.prob).all())
    assert bool((res.gated <= res.change).all())
    assert sorted(res.cm) == ["change", "gated"] and int(res.cm["change"].sum()) == H * W
    assert torch.equal(res.change, predict_scene(seg, a, b, **kw).mask)
    one = predict_scene_seg(unet, a, return_prob=True, **kw)
    assert one.mask.dtype == torch.uint8 and tuple(one.mask.shape) == (H, W) and bool(torch.isfinite(one.prob).all())


# ------------------------------------------------------------------ 7. scene_round(gate=...)
def test_scene_round_with_the_seg_gate_and_without():
    a, b, labels = _py_scene()
    models = [_Maps(3, 1, 90 + k).to(DEV) for k in range(2)]
    models[0].train()
    models[1].eval()
    cell = 32
    kw = dict(tile=PT, stride=PS, batch=PB, window="hann", tta=(6, 1))
    heads = [predict_scene_heads(m, a, b, **kw) for m in models]
    r = ST.scene_round(models, a, b, cell=cell, close_radius=2, label=labels[2], stem="t", gate="seg", **kw)
    assert [m.training for m in models] == [True, False]
    assert len(r.masks) == 2 and all(torch.equal(got, h.gated) for got, h in zip(r.masks, heads))
    assert torch.equal(r.seg_a, heads[-1].seg_a) and torch.equal(r.seg_b, heads[-1].seg_b)
    ms = [h.gated.cpu().numpy() for h in heads]
    assert 0 < int(ms[-1].sum()) < int(heads[-1].change.sum())
    want_agree, _ = RS.cell_agree(ms, cell)
    want_pseudo = RS.close_fast(ms[-1], 2, 255)
    _, want_cm = RS.cell_agree([want_pseudo], cell, labels[2])
    np.testing.assert_array_equal(r.pseudo.cpu().numpy(), want_pseudo)
    np.testing.assert_array_equal(r.agree.reshape(-1, 1, 4), want_agree)
    np.testing.assert_array_equal(r.cell_cm.reshape(-1, 4), want_cm)
    want_rel = SS.reliability_per_pair(want_agree)
    np.testing.assert_allclose(r.reliability.ravel(), want_rel, rtol=1e-12)
    listed = [i for i in range(len(r.names)) if r.full.ravel()[i]]
    assert r.names == RS.cell_names(PH, PW, cell, "t") and len(listed) == 12
    assert (r.reliable, r.unreliable) == SS.split([r.names[i] for i in listed], want_rel[listed])
    # gate=None is the call without the keyword
    plain = ST.scene_round(models, a, b, cell=cell, close_radius=2, label=labels[2], stem="t", **kw)
    none = ST.scene_round(models, a, b, cell=cell, close_radius=2, label=labels[2], stem="t", gate=None, **kw)
    assert none.seg_a is None and none.seg_b is None and plain.seg_a is None and plain.seg_b is None
    for f in ST.SceneRound._fields:
        x, y = getattr(none, f), getattr(plain, f)
        if f == "masks":
            assert all(torch.equal(p, q) for p, q in zip(x, y))
        elif torch.is_tensor(x):
            assert torch.equal(x, y), f
        elif isinstance(x, np.ndarray):
            np.testing.assert_array_equal(x, y, err_msg=f)
        elif isinstance(x, dict):
            assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x), f
        else:
            assert x == y, f
    assert all(torch.equal(m, h.change) for m, h in zip(none.masks, heads))
    with pytest.raises(_lib.StcdError, match="gate"):
        ST.scene_round(models, a, b, cell=cell, gate="change", **kw)
