"""Whole-scene inference on the GPU: stcd_scene_gather / _stitch / _finalize through the C ABI against tests/scene_spec.py, and
predict_scene end to end over the engine's families and a plain torch module.

Tolerances: the gather shares k_pseudo_pair's arithmetic and its bound (atol 2e-6, tests/test_pseudo_gpu.py).  The stitch on
dyadic logits is exact in fp32 and must equal the float64 spec bit for bit; with the Hann window a pixel's sum is at most 16
fused multiply-adds, each within 2^-24 of wsum * max|logits|, about 1e-6 in all: the bound is 1e-5 on that per-pixel scale."""
import ctypes as C

import numpy as np
import pytest
import torch

from stcd_amd import _lib, synth
from stcd_amd.metrics import ConfuseMatrixMeter
from stcd_amd.pseudo import MEAN, STD
from stcd_amd.scene import plan_tiles, predict_scene, window_table
from tests import scene_spec as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scene(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def gpu_gather(a, b, T, S, first, n):
    H, W, _ = a.shape
    plan = plan_tiles(H, W, T, S)
    x1 = torch.full((n, 3, T, T), float("nan"), dtype=torch.float32, device=DEV)
    x2 = torch.full_like(x1, float("nan"))
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    _lib.check(_lib.lib().stcd_scene_gather(_p(a), _p(b), H, W, T, S, plan.tiles_x, first, n, m3, s3, _p(x1), _p(x2), _stream()))
    return x1, x2


def gpu_stitch(logits, H, W, T, S, window, acc, wsum, first=0, n=None):
    plan = plan_tiles(H, W, T, S)
    n = logits.shape[0] if n is None else n
    _lib.check(_lib.lib().stcd_scene_stitch(_p(logits), logits.shape[1], H, W, T, S, plan.tiles_x, plan.tiles_y, first, n, _p(window),
                                            _p(acc), _p(wsum), _stream()))


def gpu_stitch_all(logits, H, W, T, S, window, chunk=None):
    """acc, wsum after stitching every tile, `chunk` tiles per call (ascending)."""
    acc = torch.zeros((logits.shape[1], H, W), dtype=torch.float32, device=DEV)
    wsum = torch.zeros((H, W), dtype=torch.float32, device=DEV)
    total = logits.shape[0]
    chunk = total if chunk is None else chunk
    for first in range(0, total, chunk):
        part = logits[first:first + chunk]
        gpu_stitch(part, H, W, T, S, window, acc, wsum, first, part.shape[0])
    return acc, wsum


def gpu_finalize(acc, wsum, threshold=0.0, label=None, want_prob=True):
    classes, H, W = acc.shape
    mask = torch.full((H, W), 7, dtype=torch.uint8, device=DEV)
    prob = torch.full((H, W), float("nan"), dtype=torch.float32, device=DEV) if want_prob else None
    cm = torch.zeros(4, dtype=torch.int64, device=DEV) if label is not None else None
    _lib.check(_lib.lib().stcd_scene_finalize(_p(acc), _p(wsum), classes, H, W, C.c_float(threshold), _p(label), _p(mask), _p(prob), _p(cm),
                                              _stream()))
    return mask, prob, cm


# ------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize("T,S", [(64, 64), (64, 32), (256, 128)])
@pytest.mark.parametrize("H,W", [(300, 420), (256, 256), (100, 70), (1, 5)])
def test_gather_matches_spec(H, W, T, S):
    a, b = _scene(H, W, 3 + H + T)
    plan = plan_tiles(H, W, T, S)
    x1, x2 = gpu_gather(_dev(a), _dev(b), T, S, 0, plan.n)
    for got, scene, name in ((x1, a, "x1"), (x2, b, "x2")):
        want = SP.gather(scene, T, S, plan.tiles_x, 0, plan.n, MEAN, STD)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=2e-6, err_msg=name)
    if plan.n > 2:                                                     # a range that does not start at tile 0
        first, n = plan.n // 2, plan.n - plan.n // 2
        y1, y2 = gpu_gather(_dev(a), _dev(b), T, S, first, n)
        assert torch.equal(y1, x1[first:]) and torch.equal(y2, x2[first:])


@pytest.mark.parametrize("T", [64, 256])
def test_gather_of_a_one_tile_scene_is_the_synth_normalisation(T):
    a, b = _scene(T, T, 5)
    x1, x2 = gpu_gather(_dev(a), _dev(b), T, T, 0, 1)
    np.testing.assert_allclose(x1.cpu().numpy(), synth.normalize_nchw(a[None]), rtol=0, atol=2e-6)
    np.testing.assert_allclose(x2.cpu().numpy(), synth.normalize_nchw(b[None]), rtol=0, atol=2e-6)


# ------------------------------------------------------------------ 2. stitch, exact
def _dyadic_logits(H, W, T, S, classes, seed):
    """Integers in [-512, 512] / 64; where `tie` marks a scene pixel every covering tile holds class 1 == class 0."""
    rng = np.random.default_rng(seed)
    plan = plan_tiles(H, W, T, S)
    logits = (rng.integers(-512, 513, size=(plan.n, classes, T, T)) / 64.0).astype(np.float32)
    tie = rng.random((H, W)) < 0.02
    tie[0, 0] = tie[H - 1, W - 1] = True
    if classes == 2:
        t = np.arange(T)
        for k in range(plan.n):
            ky, kx = divmod(k, plan.tiles_x)
            ys, xs = ky * S + t, kx * S + t
            inside = (ys < H)[:, None] & (xs < W)[None, :]
            planted = np.zeros((T, T), bool)
            planted[inside] = tie[np.minimum(ys, H - 1)[:, None], np.minimum(xs, W - 1)[None, :]][inside]
            logits[k, 1][planted] = logits[k, 0][planted]
    return plan, logits, tie


@pytest.mark.parametrize("classes", [2, 1])
@pytest.mark.parametrize("div", [1, 2, 4])
@pytest.mark.parametrize("H,W,T", [(300, 420, 64), (100, 70, 64), (257, 255, 128), (1, 5, 64)])
def test_stitch_flat_window_is_exact(H, W, T, div, classes):
    S = T // div
    plan, logits, tie = _dyadic_logits(H, W, T, S, classes, seed=H + div)
    acc, wsum = gpu_stitch_all(_dev(logits), H, W, T, S, None, chunk=7)
    want_acc, want_wsum = SP.stitch(logits, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, None, np.zeros((classes, H, W)), np.zeros((H, W)))
    assert want_wsum.min() >= 1 and want_wsum.max() <= 16
    np.testing.assert_array_equal(wsum.cpu().numpy().astype(np.float64), want_wsum)
    np.testing.assert_array_equal(acc.cpu().numpy().astype(np.float64), want_acc)
    mask, _, _ = gpu_finalize(acc, wsum)
    want_mask, _, _ = SP.finalize(want_acc, want_wsum)
    np.testing.assert_array_equal(mask.cpu().numpy(), want_mask)
    if classes == 2:
        np.testing.assert_array_equal(want_acc[1][tie], want_acc[0][tie])       # the planted ties are ties ...
        assert not mask.cpu().numpy()[tie].any()                                  # ... and a tie is class 0
    # an explicit table of ones is the NULL window
    acc1, wsum1 = gpu_stitch_all(_dev(logits), H, W, T, S, _dev(window_table(T, "flat")))
    assert torch.equal(acc1, acc) and torch.equal(wsum1, wsum)


# ------------------------------------------------------------------ 3. stitch, split invariance
@pytest.mark.parametrize("H,W,T", [(300, 420, 64), (100, 70, 64)])
def test_stitch_does_not_depend_on_the_split_or_the_run(H, W, T):
    S = T // 2
    plan = plan_tiles(H, W, T, S)
    logits = torch.randn((plan.n, 2, T, T), generator=torch.Generator().manual_seed(4)).to(DEV)
    win = _dev(window_table(T, "hann"))
    acc, wsum = gpu_stitch_all(logits, H, W, T, S, win)
    for chunk in (1, 5):
        acc_c, wsum_c = gpu_stitch_all(logits, H, W, T, S, win, chunk=chunk)
        assert torch.equal(acc_c, acc) and torch.equal(wsum_c, wsum), f"calls of {chunk} tiles differ from one call"
    acc_r, wsum_r = gpu_stitch_all(logits, H, W, T, S, win)
    assert torch.equal(acc_r, acc) and torch.equal(wsum_r, wsum)


# ------------------------------------------------------------------ 4. stitch, Hann accuracy on the per-pixel scale
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("H,W,T,S", [(300, 420, 64, 32), (300, 420, 128, 64), (100, 70, 64, 32)])
def test_stitch_hann_accuracy(H, W, T, S, seed):
    plan = plan_tiles(H, W, T, S)
    logits = np.random.default_rng(seed).standard_normal((plan.n, 2, T, T)).astype(np.float32)
    win = window_table(T, "hann")
    acc, wsum = gpu_stitch_all(_dev(logits), H, W, T, S, _dev(win), chunk=16)
    want_acc, want_wsum = SP.stitch(logits, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, win, np.zeros((2, H, W)), np.zeros((H, W)))
    L = float(np.abs(logits).max())
    got_acc, got_wsum = acc.cpu().numpy().astype(np.float64), wsum.cpu().numpy().astype(np.float64)
    err = np.abs(got_acc - want_acc) / (want_wsum * L)
    print(f"hann {H}x{W} T={T} S={S} seed={seed}: max |acc - spec| / (wsum L) = {err.max():.3e}, "
          f"max wsum rel err = {(np.abs(got_wsum - want_wsum) / want_wsum).max():.3e}")
    assert (np.abs(got_acc - want_acc) <= 1e-5 * want_wsum * L).all()
    np.testing.assert_allclose(got_wsum, want_wsum, rtol=1e-5, atol=0)
    mask, _, _ = gpu_finalize(acc, wsum)
    want_mask, _, _ = SP.finalize(want_acc, want_wsum)
    clear = np.abs(want_acc[1] - want_acc[0]) > 1e-4 * want_wsum * L
    left_out = 1.0 - clear.mean()
    print(f"    mask compared on {clear.mean() * 100:.3f} % of the scene ({left_out * 100:.3f} % left out)")
    assert left_out <= 0.002
    np.testing.assert_array_equal(mask.cpu().numpy()[clear], want_mask[clear])


# ------------------------------------------------------------------ 5. finalize
@pytest.mark.parametrize("classes", [2, 1])
@pytest.mark.parametrize("H,W", [(300, 420), (100, 70), (1, 5)])
def test_finalize_prob_and_confusion_matrix(H, W, classes):
    rng = np.random.default_rng(H + classes)
    wsum = rng.uniform(0.01, 4.0, size=(H, W)).astype(np.float32)
    acc = (rng.standard_normal((classes, H, W)) * 3.0 * wsum).astype(np.float32)
    label = rng.choice(np.array([0, 0, 0, 1, 2, 200], np.uint8), size=(H, W))
    label[rng.random((H, W)) < 0.05] = 255
    label[0, 0], label[-1, -1] = 255, 1
    mask, prob, cm = gpu_finalize(_dev(acc), _dev(wsum), 0.0, _dev(label))
    want_mask, want_prob, want_cm = SP.finalize(acc, wsum, 0.0, label)
    np.testing.assert_array_equal(mask.cpu().numpy(), want_mask)
    np.testing.assert_allclose(prob.cpu().numpy(), want_prob, rtol=0, atol=1e-6)
    meter = ConfuseMatrixMeter(n_class=2)
    meter.update_cm(mask.cpu().numpy(), np.where(label == 255, 255, label >= 1))
    np.testing.assert_array_equal(cm.cpu().numpy(), meter.cm.astype(np.int64).ravel())
    np.testing.assert_array_equal(cm.cpu().numpy(), want_cm)
    assert int(cm.sum()) == int((label != 255).sum())
    # without prob and label: the same mask
    mask2, _, _ = gpu_finalize(_dev(acc), _dev(wsum), 0.0, None, want_prob=False)
    assert torch.equal(mask2, mask)


@pytest.mark.parametrize("threshold", [0.0, 0.5])
@pytest.mark.parametrize("H,W", [(64, 64), (33, 47)])
def test_finalize_one_class_threshold_is_exact_and_strict(H, W, threshold):
    rng = np.random.default_rng(W)
    wsum = rng.integers(1, 17, size=(H, W)).astype(np.float32)
    acc = (rng.integers(-512, 513, size=(1, H, W)) / 64.0).astype(np.float32) * wsum
    on = rng.random((H, W)) < 0.1
    on[0, 0] = on[-1, -1] = True
    acc[0][on] = (threshold * wsum)[on]                               # exactly on the threshold: class 0
    mask, _, _ = gpu_finalize(_dev(acc), _dev(wsum), threshold, want_prob=False)
    want_mask, _, _ = SP.finalize(acc, wsum, threshold)
    np.testing.assert_array_equal(mask.cpu().numpy(), want_mask)
    assert not mask.cpu().numpy()[on].any()
    above = acc[0] / wsum > threshold
    np.testing.assert_array_equal(mask.cpu().numpy().astype(bool), above)


# ------------------------------------------------------------------ 6. end to end
class _Plain(torch.nn.Module):
    """Not an engine module: nothing in the three kernels depends on the engine."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(6, 2, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(2)

    def forward(self, x1, x2):
        return self.bn(self.conv(torch.cat([x1, x2], 1)))


def _model(name):
    torch.manual_seed(1234)
    if name == "diff":
        from stcd_amd.modules import SiamUnet_diff
        return SiamUnet_diff(3, 2, dtype="fp32").to(DEV), 32
    if name == "snunet":
        from stcd_amd.modules import SNUNet_ECAM
        return SNUNet_ECAM(3, 2, dtype="fp32").to(DEV), 32
    if name == "segcd":
        from stcd_amd.segcd import SegCD
        return SegCD().to(DEV), 64
    if name == "changeformer":
        from stcd_amd.changeformer import ChangeFormerV6
        return ChangeFormerV6().to(DEV), 64
    return _Plain().to(DEV), 32


def _direct_mask(model, x1, x2):
    """arg-max (two classes) or logit > 0 (one class) of a direct eval forward, as models/trainer.py:197-203 reads it."""
    model.eval()
    with torch.no_grad():
        out = model(x1, x2)
    out = out[-1] if isinstance(out, (list, tuple)) else out
    pred = out.argmax(1) if out.shape[1] == 2 else (out[:, 0] > 0)
    return pred.to(torch.uint8)


MODELS = ["diff", "snunet", "segcd", "changeformer", "plain"]


@pytest.mark.parametrize("name", MODELS)
def test_predict_scene_one_tile_equals_a_direct_forward(name):
    model, T = _model(name)
    a, b, _ = synth.make_pairs_u8(1, T, T, seed=21)
    x1, x2 = gpu_gather(_dev(a[0]), _dev(b[0]), T, T, 0, 1)           # the normalised scene (pinned to the spec above)
    want = _direct_mask(model, x1, x2)[0]
    res = predict_scene(model, a[0], b[0], tile=T, stride=T, window="flat")
    assert res.mask.shape == (T, T) and res.mask.dtype == torch.uint8 and res.prob is None and res.cm is None
    assert torch.equal(res.mask, want)


@pytest.mark.parametrize("name", MODELS)
def test_predict_scene_two_by_two_tiles_short_last_batch(name):
    model, T = _model(name)
    a, b, _ = synth.make_pairs_u8(1, 2 * T, 2 * T, seed=22)
    x1, x2 = gpu_gather(_dev(a[0]), _dev(b[0]), T, T, 0, 4)
    parts = [_direct_mask(model, x1[:3], x2[:3]), _direct_mask(model, x1[3:], x2[3:])]      # predict_scene's batches: 3 + 1
    tiles = torch.cat(parts, 0)
    want = torch.cat([torch.cat([tiles[0], tiles[1]], 1), torch.cat([tiles[2], tiles[3]], 1)], 0)
    res = predict_scene(model, _dev(a[0]), _dev(b[0]), tile=T, stride=T, batch=3, window="flat")
    assert torch.equal(res.mask, want)


@pytest.mark.parametrize("name", MODELS)
def test_predict_scene_overlap_hann_label_and_mode(name):
    model, _ = _model(name)
    H, W = 300, 420
    a, b, lab = synth.make_pairs_u8(1, H, W, seed=23)
    label = lab[0].copy()
    label[:10, :17] = 255
    for training in (True, False):
        model.train(training)
        res = predict_scene(model, a[0], b[0], tile=128, stride=64, window="hann", label=label, return_prob=True)
        assert model.training is training, "predict_scene did not restore the model's mode"
        assert tuple(res.mask.shape) == (H, W) and tuple(res.prob.shape) == (H, W)
        assert res.cm.shape == (2, 2) and int(res.cm.sum()) == int((label != 255).sum())
        assert set(res.scores) >= {"precision", "recall", "f1", "iou", "oa"}
        assert bool(torch.isfinite(res.prob).all())
        again = predict_scene(model, a[0], b[0], tile=128, stride=64, window="hann", label=label, return_prob=True)
        assert torch.equal(again.mask, res.mask) and torch.equal(again.prob, res.prob)
        np.testing.assert_array_equal(again.cm, res.cm)


def test_predict_scene_argument_errors_come_before_any_launch():
    model, T = _model("plain")
    a, b = _scene(64, 64, 1)
    with pytest.raises(_lib.StcdError):
        predict_scene(model, a, b[:32], tile=32)                      # scenes of different shape
    with pytest.raises(_lib.StcdError):
        predict_scene(model, a.astype(np.float32), b, tile=32)        # wrong dtype
    with pytest.raises(_lib.StcdError):
        predict_scene(model, a, b, tile=32, stride=33)                # stride > tile
    with pytest.raises(_lib.StcdError):
        predict_scene(model, a, b, tile=32, window="bartlett")
    with pytest.raises(_lib.StcdError):
        predict_scene(model, a, b, tile=32, label=np.zeros((64, 63), np.uint8))


# ------------------------------------------------------------------ 7. argument checks of the ABI (nothing is launched)
def test_abi_rejects_invalid_arguments():
    l = _lib.lib()
    H, W, T, S = 100, 70, 64, 32
    plan = plan_tiles(H, W, T, S)
    a = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    x = torch.zeros((plan.n, 3, T, T), dtype=torch.float32, device=DEV)
    lg = torch.zeros((plan.n, 2, T, T), dtype=torch.float32, device=DEV)
    acc = torch.zeros((2, H, W), dtype=torch.float32, device=DEV)
    wsum = torch.zeros((H, W), dtype=torch.float32, device=DEV)
    mask = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    cm = torch.zeros(4, dtype=torch.int64, device=DEV)
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    st = _stream()

    def gather(S_=S, tx=plan.tiles_x, first=0, n=plan.n, pa=a, px=x, T_=T):
        return l.stcd_scene_gather(_p(pa), _p(a), H, W, T_, S_, tx, first, n, m3, s3, _p(px), _p(x), st)

    def stitch(S_=S, classes=2, first=0, n=plan.n, pl=lg, pacc=acc, tx=plan.tiles_x, ty=plan.tiles_y):
        return l.stcd_scene_stitch(_p(pl), classes, H, W, T, S_, tx, ty, first, n, None, _p(pacc), _p(wsum), st)

    def finalize(classes=2, pm=mask, plab=None, pcm=None):
        return l.stcd_scene_finalize(_p(acc), _p(wsum), classes, H, W, C.c_float(0.0), _p(plab), _p(pm), None, _p(pcm), st)

    assert gather() == 0 and stitch() == 0 and finalize() == 0
    assert gather(n=0) == 0 and stitch(n=0) == 0                      # an empty range is valid and launches nothing
    bad = [gather(S_=0), gather(S_=T + 1), gather(n=-1), gather(first=1), gather(first=-1), gather(first=plan.n, n=1), gather(pa=None),
           gather(px=None), gather(tx=plan.tiles_x + 1), gather(T_=0),
           stitch(S_=0), stitch(S_=T + 1), stitch(classes=0), stitch(classes=3), stitch(n=-1), stitch(first=1), stitch(first=plan.n, n=1),
           stitch(pl=None), stitch(pacc=None), stitch(tx=plan.tiles_x - 1), stitch(ty=plan.tiles_y + 1),
           finalize(classes=0), finalize(classes=3), finalize(pm=None), finalize(plab=mask), finalize(pcm=cm)]
    assert all(rc != 0 for rc in bad), bad
    assert l.stcd_scene_stitch(_p(lg), 3, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, plan.n, None, _p(acc), _p(wsum), st) != 0
    assert b"classes" in l.stcd_last_error()
    torch.cuda.synchronize()
