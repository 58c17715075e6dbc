"""The D4 views of whole-scene inference on the GPU: stcd_scene_gather_d4 / stcd_scene_stitch_d4 through the C ABI against the
upright entries and tests/scene_tta_spec.py, and predict_scene(tta=..., [models]) end to end.

Tolerances: the gather keeps the upright gather's arithmetic, so it is bit-equal to that entry followed by the index permutation
and within that entry's bound of the float64 spec (atol 2e-6, tests/test_scene_gpu.py).  The stitch on logits that are multiples
of 2^-6 with |x| <= 8 is exact in fp32 under the flat window for up to 8 views x 16 covering tiles (|sum| <= 1024 at a
granularity of 2^-6: 17 bits), so it must equal the float64 spec bit for bit; with the Hann window it is held bit-equal to the
upright entry on the un-transformed logits, which tests/test_scene_gpu.py holds to the spec."""
import ctypes as C

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd.metrics import ConfuseMatrixMeter
from stcd_amd.pseudo import MEAN, STD
from stcd_amd.scene import plan_tiles, predict_scene, window_table
from tests import scene_spec as SP
from tests import scene_tta_spec as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VIEWS = TS.VIEWS


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scene(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def t_apply(x, d):
    """scene_tta_spec.d4_apply on a torch tensor (a copy)."""
    dims = [dim for dim, bit in ((-2, 2), (-1, 1)) if d & bit]
    f = torch.flip(x, dims) if dims else x
    return (f.transpose(-1, -2) if d & 4 else f).contiguous()


def t_invert(y, d):
    f = y.transpose(-1, -2) if d & 4 else y
    dims = [dim for dim, bit in ((-2, 2), (-1, 1)) if d & bit]
    return (torch.flip(f, dims) if dims else f).contiguous()


def gpu_gather(a, b, T, S, first, n, d=None):
    """d None: the upright entry."""
    H, W, _ = a.shape
    plan = plan_tiles(H, W, T, S)
    x1 = torch.full((n, 3, T, T), float("nan"), dtype=torch.float32, device=DEV)
    x2 = torch.full_like(x1, float("nan"))
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    l = _lib.lib()
    if d is None:
        _lib.check(l.stcd_scene_gather(_p(a), _p(b), H, W, T, S, plan.tiles_x, first, n, m3, s3, _p(x1), _p(x2), _stream()))
    else:
        _lib.check(l.stcd_scene_gather_d4(_p(a), _p(b), H, W, T, S, plan.tiles_x, first, n, m3, s3, _p(x1), _p(x2), d, _stream()))
    return x1, x2


def gpu_stitch(logits, H, W, T, S, window, acc, wsum, d=None, chunk=None):
    """Every tile of `logits` into acc / wsum in place, `chunk` tiles per call (ascending); d None: the upright entry."""
    plan = plan_tiles(H, W, T, S)
    l = _lib.lib()
    total = logits.shape[0]
    chunk = total if chunk is None else chunk
    for first in range(0, total, chunk):
        part = logits[first:first + chunk]
        if d is None:
            _lib.check(l.stcd_scene_stitch(_p(part), part.shape[1], H, W, T, S, plan.tiles_x, plan.tiles_y, first, part.shape[0], _p(window),
                                           _p(acc), _p(wsum), _stream()))
        else:
            _lib.check(l.stcd_scene_stitch_d4(_p(part), part.shape[1], H, W, T, S, plan.tiles_x, plan.tiles_y, first, part.shape[0],
                                              _p(window), _p(acc), _p(wsum), d, _stream()))


def _zeros(classes, H, W):
    return torch.zeros((classes, H, W), dtype=torch.float32, device=DEV), torch.zeros((H, W), dtype=torch.float32, device=DEV)


def gpu_finalize(acc, wsum, want_prob=False):
    classes, H, W = acc.shape
    mask = torch.full((H, W), 7, dtype=torch.uint8, device=DEV)
    prob = torch.full((H, W), float("nan"), dtype=torch.float32, device=DEV) if want_prob else None
    _lib.check(_lib.lib().stcd_scene_finalize(_p(acc), _p(wsum), classes, H, W, C.c_float(0.0), None, _p(mask), _p(prob), None, _stream()))
    return mask, prob


# ------------------------------------------------------------------ 1. gather
# reflection on both edges; a scene smaller than a tile; one full 64 x 64 staging patch plus a partial one; the scalar path
# UPRIGHT_SHAPES: small grids, T % 4 == 0 and T % 4 != 0, on which the entries without d4 are held against their d4 == 0 siblings
UPRIGHT_SHAPES = [(20, 13, 8, 4), (17, 9, 6, 3)]
GATHER_SHAPES = [(100, 70, 64, 32), (1, 5, 64, 64), (130, 67, 72, 40), (100, 70, 30, 14)] + UPRIGHT_SHAPES
_upright = {}


def _upright_tiles(H, W, T, S):
    """The upright gather and its float64 spec, computed once per shape and left unchanged."""
    key = (H, W, T, S)
    if key not in _upright:
        a, b = _scene(H, W, 3 + H + T)
        plan = plan_tiles(H, W, T, S)
        x1, x2 = gpu_gather(_dev(a), _dev(b), T, S, 0, plan.n)
        spec = [SP.gather(s, T, S, plan.tiles_x, 0, plan.n, MEAN, STD) for s in (a, b)]
        _upright[key] = (_dev(a), _dev(b), plan, x1, x2, spec)
    return _upright[key]


@pytest.mark.parametrize("d", VIEWS)
@pytest.mark.parametrize("H,W,T,S", GATHER_SHAPES)
def test_gather_d4_is_the_upright_gather_permuted(H, W, T, S, d):
    a, b, plan, x1, x2, spec = _upright_tiles(H, W, T, S)
    y1, y2 = gpu_gather(a, b, T, S, 0, plan.n, d)
    for got, up, want, name in ((y1, x1, spec[0], "x1"), (y2, x2, spec[1], "x2")):
        np.testing.assert_array_equal(got.cpu().numpy(), t_apply(up, d).cpu().numpy(), err_msg=name)
        np.testing.assert_allclose(got.cpu().numpy(), TS.d4_apply(want, d), rtol=0, atol=2e-6, err_msg=name)
    if d == 0:
        assert torch.equal(y1, x1) and torch.equal(y2, x2)
    if plan.n > 2:                                                     # a range that does not start at tile 0
        first = plan.n // 2
        z1, z2 = gpu_gather(a, b, T, S, first, plan.n - first, d)
        assert torch.equal(z1, y1[first:]) and torch.equal(z2, y2[first:])


def test_gather_d4_unaligned_outputs_take_the_scalar_path():
    H, W, T, S = 100, 70, 64, 32
    a, b, plan, x1, x2, _ = _upright_tiles(H, W, T, S)
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    for d in VIEWS:
        buf1 = torch.zeros(x1.numel() + 1, dtype=torch.float32, device=DEV)
        buf2 = torch.zeros_like(buf1)
        y1, y2 = buf1[1:].view_as(x1), buf2[1:].view_as(x2)           # 4 bytes past a 16-byte boundary
        _lib.check(_lib.lib().stcd_scene_gather_d4(_p(a), _p(b), H, W, T, S, plan.tiles_x, 0, plan.n, m3, s3, _p(y1), _p(y2), d, _stream()))
        assert torch.equal(y1, t_apply(x1, d)) and torch.equal(y2, t_apply(x2, d)), d
        assert float(buf1[0]) == 0.0 and float(buf2[0]) == 0.0


# ------------------------------------------------------------------ 2. stitch, exact
def _dyadic(shape, rng, lim=512):
    return (rng.integers(-lim, lim + 1, size=shape) / 64.0).astype(np.float32)


STITCH_SHAPES = [(100, 70, 64, 32), (100, 70, 64, 16), (257, 255, 128, 64), (1, 5, 64, 64), (100, 70, 30, 14)]


@pytest.mark.parametrize("classes", [2, 1])
@pytest.mark.parametrize("H,W,T,S", STITCH_SHAPES)
def test_stitch_d4_flat_window_is_exact(H, W, T, S, classes):
    plan = plan_tiles(H, W, T, S)
    rng = np.random.default_rng(H + S + classes)
    for d in VIEWS:
        logits = _dyadic((plan.n, classes, T, T), rng)                # the network's outputs for view d
        acc, wsum = _zeros(classes, H, W)
        gpu_stitch(_dev(logits), H, W, T, S, None, acc, wsum, d, chunk=7)
        want_acc, want_wsum = TS.stitch_d4(logits, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, None, np.zeros((classes, H, W)),
                                           np.zeros((H, W)), d)
        assert want_wsum.min() >= 1 and want_wsum.max() <= 16
        np.testing.assert_array_equal(wsum.cpu().numpy().astype(np.float64), want_wsum, err_msg=f"d4 {d}")
        np.testing.assert_array_equal(acc.cpu().numpy().astype(np.float64), want_acc, err_msg=f"d4 {d}")


@pytest.mark.parametrize("classes", [2, 1])
@pytest.mark.parametrize("H,W,T,S", STITCH_SHAPES)
def test_stitch_d4_chain_of_eight_views_is_exact_and_ties_are_class_zero(H, W, T, S, classes):
    """All eight views into one acc / wsum.  At the planted pixels the class difference of every tile is + delta in the even
    views and - delta in the odd ones, so the views cancel: acc[1] == acc[0] exactly, and a tie is class 0."""
    plan = plan_tiles(H, W, T, S)
    rng = np.random.default_rng(H + S)
    tie = rng.random((H, W)) < 0.02
    tie[0, 0] = tie[H - 1, W - 1] = True
    t = np.arange(T)
    base = _dyadic((plan.n, T, T), rng, 256)                           # |x| <= 4, so base +- delta stays within 8
    delta = _dyadic((plan.n, T, T), rng, 256)
    acc, wsum = _zeros(classes, H, W)
    want_acc, want_wsum = np.zeros((classes, H, W)), np.zeros((H, W))
    for d in VIEWS:
        up = _dyadic((plan.n, classes, T, T), rng)                    # upright logits of view d
        if classes == 2:
            for k in range(plan.n):
                ky, kx = divmod(k, plan.tiles_x)
                ys, xs = ky * S + t, kx * S + t
                inside = (ys < H)[:, None] & (xs < W)[None, :]
                planted = np.zeros((T, T), bool)
                planted[inside] = tie[np.minimum(ys, H - 1)[:, None], np.minimum(xs, W - 1)[None, :]][inside]
                up[k, 0][planted] = base[k][planted]
                up[k, 1][planted] = (base[k] + (delta[k] if d % 2 == 0 else -delta[k]))[planted]
        view = np.ascontiguousarray(TS.d4_apply(up, d))
        gpu_stitch(_dev(view), H, W, T, S, None, acc, wsum, d, chunk=5)
        TS.stitch_d4(view, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, None, want_acc, want_wsum, d)
    assert want_wsum.min() >= 8 and want_wsum.max() <= 128
    np.testing.assert_array_equal(wsum.cpu().numpy().astype(np.float64), want_wsum)
    np.testing.assert_array_equal(acc.cpu().numpy().astype(np.float64), want_acc)
    mask, _ = gpu_finalize(acc, wsum)
    want_mask, _, _ = SP.finalize(want_acc, want_wsum)
    np.testing.assert_array_equal(mask.cpu().numpy(), want_mask)
    if classes == 2:
        np.testing.assert_array_equal(want_acc[1][tie], want_acc[0][tie])       # the planted ties are ties ...
        assert not mask.cpu().numpy()[tie].any()                                  # ... and a tie is class 0
        assert mask.cpu().numpy().any()


# ------------------------------------------------------------------ 3. stitch, Hann: the upright entry on the un-transformed logits
@pytest.mark.parametrize("classes", [2, 1])
@pytest.mark.parametrize("H,W,T,S", [(300, 420, 64, 32), (100, 70, 64, 32)] + UPRIGHT_SHAPES)
def test_stitch_d4_hann_is_bit_equal_to_the_upright_entry(H, W, T, S, classes):
    plan = plan_tiles(H, W, T, S)
    gen = torch.Generator().manual_seed(4 + H)
    win = _dev(window_table(T, "hann"))
    acc0 = torch.randn((classes, H, W), generator=gen).to(DEV)        # the same starting chain for both
    wsum0 = torch.rand((H, W), generator=gen).to(DEV)
    for d in VIEWS:
        view = torch.randn((plan.n, classes, T, T), generator=gen).to(DEV)
        acc, wsum = acc0.clone(), wsum0.clone()
        gpu_stitch(view, H, W, T, S, win, acc, wsum, d)
        want_acc, want_wsum = acc0.clone(), wsum0.clone()
        gpu_stitch(t_invert(view, d), H, W, T, S, win, want_acc, want_wsum)
        assert torch.equal(acc, want_acc) and torch.equal(wsum, want_wsum), f"d4 {d}"
        assert not torch.equal(acc, acc0)
        if d == 0:
            acc, wsum = acc0.clone(), wsum0.clone()
            gpu_stitch(view, H, W, T, S, win, acc, wsum)
            assert torch.equal(acc, want_acc) and torch.equal(wsum, want_wsum)


def test_stitch_d4_unaligned_scene_width_and_logits():
    """W % 4 != 0 (scalar acc path) is in the shapes above; here the logits start 4 bytes past a 16-byte boundary."""
    H, W, T, S = 100, 72, 64, 32
    plan = plan_tiles(H, W, T, S)
    gen = torch.Generator().manual_seed(9)
    win = _dev(window_table(T, "hann"))
    for d in VIEWS:
        buf = torch.randn(plan.n * 2 * T * T + 1, generator=gen).to(DEV)
        view = buf[1:].view(plan.n, 2, T, T)
        acc, wsum = _zeros(2, H, W)
        gpu_stitch(view, H, W, T, S, win, acc, wsum, d)
        want_acc, want_wsum = _zeros(2, H, W)
        gpu_stitch(t_invert(view, d), H, W, T, S, win, want_acc, want_wsum)
        assert torch.equal(acc, want_acc) and torch.equal(wsum, want_wsum), f"d4 {d}"


# ------------------------------------------------------------------ 4. the chain does not depend on the split or the run
def test_eight_view_chain_does_not_depend_on_the_split_or_the_run():
    H, W, T, S = 100, 70, 64, 32
    plan = plan_tiles(H, W, T, S)
    gen = torch.Generator().manual_seed(6)
    views = [torch.randn((plan.n, 2, T, T), generator=gen).to(DEV) for _ in VIEWS]
    win = _dev(window_table(T, "hann"))

    def chain(chunk):
        acc, wsum = _zeros(2, H, W)
        for d in VIEWS:
            gpu_stitch(views[d], H, W, T, S, win, acc, wsum, d, chunk=chunk)
        return acc, wsum

    acc, wsum = chain(None)
    for chunk in (1, 3):
        acc_c, wsum_c = chain(chunk)
        assert torch.equal(acc_c, acc) and torch.equal(wsum_c, wsum), f"calls of {chunk} tiles differ from one call"
    acc_r, wsum_r = chain(None)
    assert torch.equal(acc_r, acc) and torch.equal(wsum_r, wsum)


# ------------------------------------------------------------------ 5. predict_scene
class _Pointwise(torch.nn.Module):
    """A fixed 1 x 1 mix of x1 - x2, written as elementwise operations so that it is D4-equivariant to the bit, rounded to
    multiples of 2^-6 within +-8 so that eight equal views add up exactly."""

    def __init__(self, classes):
        super().__init__()
        w = torch.tensor([[0.75, -1.25, 0.5], [-0.5, 1.0, 1.5]])[:classes]
        self.w = torch.nn.Parameter(w)
        self.b = torch.nn.Parameter(torch.tensor([0.25, -0.125])[:classes])

    def forward(self, x1, x2):
        diff = x1 - x2
        out = torch.stack([self.w[c, 0] * diff[:, 0] + self.w[c, 1] * diff[:, 1] + self.w[c, 2] * diff[:, 2] + self.b[c]
                           for c in range(self.w.shape[0])], 1)
        return torch.clamp(torch.round(out * 64.0) / 64.0, -8.0, 8.0)


@pytest.mark.parametrize("classes", [2, 1])
def test_predict_scene_d4_of_an_equivariant_model_is_the_upright_prediction(classes):
    model = _Pointwise(classes).to(DEV)
    a, b = _scene(100, 70, 31)
    b[:50] = a[:50]                                                   # no difference: a constant logit on half the scene
    plain = predict_scene(model, a, b, tile=32, stride=32, window="flat", return_prob=True)
    for tta in ("d4", "flip", (6, 3)):
        res = predict_scene(model, a, b, tile=32, stride=32, window="flat", return_prob=True, tta=tta)
        assert torch.equal(res.mask, plain.mask), tta
        np.testing.assert_allclose(res.prob.cpu().numpy(), plain.prob.cpu().numpy(), rtol=0, atol=1e-6)
    assert 0 < int(plain.mask.sum()) < plain.mask.numel()


def _diff_model(seed):
    from stcd_amd.modules import SiamUnet_diff
    torch.manual_seed(seed)
    return SiamUnet_diff(3, 2, dtype="fp32").to(DEV)


def _host_composition(models, views, a, b, T, S, batch, win, label):
    """What a user composes from torch permutations around the upright entries, in predict_scene's order."""
    from stcd_amd.modules import frozen_weights
    H, W, _ = a.shape
    plan = plan_tiles(H, W, T, S)
    acc, wsum = _zeros(2, H, W)
    l = _lib.lib()
    for m in models:
        m.eval()
        with torch.no_grad(), frozen_weights(m):
            for d in views:
                for first in range(0, plan.n, batch):
                    n = min(batch, plan.n - first)
                    x1, x2 = gpu_gather(a, b, T, S, first, n)
                    logits = m(t_apply(x1, d), t_apply(x2, d)).float()
                    up = t_invert(logits, d)
                    _lib.check(l.stcd_scene_stitch(_p(up), 2, H, W, T, S, plan.tiles_x, plan.tiles_y, first, n, _p(win), _p(acc), _p(wsum),
                                                   _stream()))
    mask = torch.empty((H, W), dtype=torch.uint8, device=DEV)
    prob = torch.empty((H, W), dtype=torch.float32, device=DEV)
    cm = torch.zeros(4, dtype=torch.int64, device=DEV)
    _lib.check(l.stcd_scene_finalize(_p(acc), _p(wsum), 2, H, W, C.c_float(0.0), _p(label), _p(mask), _p(prob), _p(cm), _stream()))
    return mask, prob, cm


@pytest.mark.parametrize("n_models,tta,views", [(1, "d4", VIEWS), (2, (6, 1), (6, 1))])
def test_predict_scene_tta_is_the_host_composition(n_models, tta, views):
    H, W, T, S, batch = 100, 70, 64, 32, 4
    models = [_diff_model(1234 + k) for k in range(n_models)]
    a, b = _scene(H, W, 41)
    label = (np.random.default_rng(5).random((H, W)) < 0.3).astype(np.uint8)
    label[:7, :9] = 255
    res = predict_scene(models if n_models > 1 else models[0], a, b, tile=T, stride=S, batch=batch, window="hann", label=label,
                        return_prob=True, tta=tta)
    mask, prob, cm = _host_composition(models, views, _dev(a), _dev(b), T, S, batch, _dev(window_table(T, "hann")), _dev(label))
    assert torch.equal(res.mask, mask) and torch.equal(res.prob, prob)
    np.testing.assert_array_equal(res.cm.ravel(), cm.cpu().numpy())
    meter = ConfuseMatrixMeter(n_class=2)
    meter.update_cm(res.mask.cpu().numpy(), np.where(label == 255, 255, label >= 1))
    np.testing.assert_array_equal(res.cm, meter.cm.astype(np.int64))


def test_predict_scene_of_a_model_twice_is_the_model():
    m = _diff_model(77)
    a, b = _scene(100, 70, 43)
    one = predict_scene(m, a, b, tile=64, stride=64, window="flat", return_prob=True)
    two = predict_scene([m, m], a, b, tile=64, stride=64, window="flat", return_prob=True)
    assert torch.equal(two.mask, one.mask) and torch.equal(two.prob, one.prob)      # acc and wsum both exactly double


def test_predict_scene_defaults_are_the_single_upright_view():
    m = _diff_model(78)
    a, b = _scene(100, 70, 44)
    kw = dict(tile=64, stride=32, window="hann", return_prob=True)
    old = predict_scene(m, a, b, **kw)
    for model, tta in ((m, None), ([m], None), ((m,), (0,))):
        new = predict_scene(model, a, b, tta=tta, **kw)
        assert torch.equal(new.mask, old.mask) and torch.equal(new.prob, old.prob)


class _Raises(torch.nn.Module):
    def __init__(self, after):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.after, self.calls = after, 0

    def forward(self, x1, x2):
        self.calls += 1
        if self.calls > self.after:
            raise RuntimeError("boom")
        return x1[:, :2] - x2[:, :2] + self.w


@pytest.mark.parametrize("training", [True, False])
def test_predict_scene_restores_every_mode_after_an_exception(training):
    good, bad = _Raises(10 ** 9).to(DEV), _Raises(3).to(DEV)
    good.train(training)
    bad.train(not training)
    a, b = _scene(64, 64, 45)
    with pytest.raises(RuntimeError, match="boom"):
        predict_scene([good, bad], a, b, tile=32, stride=32, batch=2, tta="flip")     # bad fails in its second view
    assert good.training is training and bad.training is (not training)
    assert good.calls == 8 and bad.calls == 4


def test_predict_scene_rejects_models_that_disagree_on_the_classes():
    a, b = _scene(64, 64, 46)
    with pytest.raises(_lib.StcdError, match="classes"):
        predict_scene([_Pointwise(2).to(DEV), _Pointwise(1).to(DEV)], a, b, tile=32)


# ------------------------------------------------------------------ 6. argument checks of the ABI (nothing is launched)
def test_abi_rejects_a_d4_outside_the_group_and_writes_nothing():
    l = _lib.lib()
    H, W, T, S = 100, 70, 64, 32
    plan = plan_tiles(H, W, T, S)
    a = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    x1 = torch.full((plan.n, 3, T, T), 3.0, dtype=torch.float32, device=DEV)
    x2 = torch.full_like(x1, 4.0)
    lg = torch.ones((plan.n, 2, T, T), dtype=torch.float32, device=DEV)
    acc = torch.full((2, H, W), 5.0, dtype=torch.float32, device=DEV)
    wsum = torch.full((H, W), 6.0, dtype=torch.float32, device=DEV)
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    st = _stream()

    def gather(d, n=plan.n, S_=S, pa=a):
        return l.stcd_scene_gather_d4(_p(pa), _p(a), H, W, T, S_, plan.tiles_x, 0, n, m3, s3, _p(x1), _p(x2), d, st)

    def stitch(d, n=plan.n, classes=2, ty=plan.tiles_y):
        return l.stcd_scene_stitch_d4(_p(lg), classes, H, W, T, S, plan.tiles_x, ty, 0, n, None, _p(acc), _p(wsum), d, st)

    for d in (-1, 8):
        assert gather(d) != 0
        assert b"d4" in l.stcd_last_error() and b"stcd_scene_gather_d4" in l.stcd_last_error()
        assert stitch(d) != 0
        assert b"d4" in l.stcd_last_error() and b"stcd_scene_stitch_d4" in l.stcd_last_error()
    # the checks of the upright entries apply unchanged, for a mirror view and a transposing one
    bad = [f(d, **kw) for d in (3, 5) for f, kw in ((gather, dict(n=-1)), (gather, dict(S_=0)), (gather, dict(S_=T + 1)), (gather, dict(pa=None)),
                                                     (gather, dict(n=plan.n + 1)), (stitch, dict(n=-1)), (stitch, dict(classes=3)),
                                                     (stitch, dict(ty=plan.tiles_y + 1)), (stitch, dict(n=plan.n + 1)))]
    assert all(rc != 0 for rc in bad), bad
    for d in VIEWS:                                                   # an empty range is valid and launches nothing
        assert gather(d, n=0) == 0 and stitch(d, n=0) == 0
    torch.cuda.synchronize()
    assert bool((x1 == 3.0).all()) and bool((x2 == 4.0).all()) and bool((acc == 5.0).all()) and bool((wsum == 6.0).all())
