"""Focal / mIoU / min-max IoU losses, CPU side: the formulas stated in stcd_amd.losses (restated here in float64 torch) reproduce
the reference's own vectors (tests/golden/g22_losses.npz, made by make_loss_golden.py), including the label-225 quirk and the even
split of a tied minimum; get_alpha's counts; the new entry points exist and refuse what they do not support."""
import numpy as np
import pytest
import torch

from stcd_amd import _lib, losses

FOCAL = ["fl_none_g2", "fl_counts_g2", "fl_float_g05", "fl_counts_sum", "fl_prob", "fl_225", "fl_none_g05_sum"]
IOU = ["miou_c2", "miou_c4", "mm_tie", "mm_c4"]


def focal_alpha(g, tag, C):
    """The per-class alpha vector of a fixture case (FocalLoss's alpha rules)."""
    prm = g[f"{tag}/params"]
    kind, bi, af = int(prm[4]), int(prm[5]), float(prm[6])
    if kind == 0:
        return torch.ones(C, dtype=torch.float64)
    if kind == 1:
        a = torch.as_tensor(g[f"{tag}/alpha_counts"], dtype=torch.float64)
        return 1.0 / (a / a.sum())
    a = torch.full((C,), 1.0 - af, dtype=torch.float64)
    a[bi] = af
    return a


def focal_restated(x, target, alpha, gamma, smooth, size_average, fused):
    """loss = -alpha[label] (1-pt)^gamma log(pt), pt = sum_c clamp(onehot, smooth/(C-1), 1-smooth)_c p_c + smooth; 225 -> 0."""
    C = x.shape[1]
    p = torch.softmax(x, 1) if fused else x
    p = p.movedim(1, -1).reshape(-1, C)
    lab = target.reshape(-1).long()
    lab = torch.where(lab == 225, torch.zeros_like(lab), lab)
    k = torch.nn.functional.one_hot(lab, C).to(p.dtype)
    if smooth:
        k = k.clamp(smooth / (C - 1), 1.0 - smooth)
    pt = (k * p).sum(1) + smooth
    loss = -alpha.to(p.dtype)[lab] * (1 - pt) ** gamma * pt.log()
    return loss.mean() if size_average else loss.sum()


def iou_restated(x, target, weight, mode):
    """iou[n,c] = sum p t / (sum (p + t - p t) + 1e-8); mode 0: -mean(w iou); mode 1: -min(iou) - mean(iou)."""
    N, C = x.shape[:2]
    p = torch.softmax(x, 1).reshape(N, C, -1)
    t = torch.nn.functional.one_hot(target.reshape(N, -1).long(), C).movedim(-1, 1).to(p.dtype)
    inter = (p * t).sum(2)
    union = (p + t - p * t).sum(2)
    iou = inter / (union + 1e-8)
    if mode == 0:
        w = torch.ones(C, dtype=p.dtype) if weight is None else weight.to(p.dtype)
        return -(w * iou).mean()
    return -iou.min() - iou.mean()


def _check(got, grad, g, tag, rtol):
    want, gref = float(g[f"{tag}/loss"]), g[f"{tag}/grad"]
    assert abs(got.item() - want) <= rtol * abs(want), (tag, got.item(), want)
    err = np.abs(grad.detach().numpy() - gref).max()
    assert err <= rtol * np.abs(gref).max(), (tag, err, np.abs(gref).max())


@pytest.mark.parametrize("tag", FOCAL)
def test_focal_restatement_matches_reference_vectors(golden, tag):
    g = golden("g22_losses.npz")
    prm = g[f"{tag}/params"]
    gamma, smooth, size_average, fused = float(prm[0]), float(prm[1]), bool(prm[2]), bool(prm[3])
    x = torch.from_numpy(g[f"{tag}/x"]).double().requires_grad_(True)
    loss = focal_restated(x, torch.from_numpy(g[f"{tag}/target"]), focal_alpha(g, tag, x.shape[1]), gamma, smooth, size_average, fused)
    loss.backward()
    _check(loss, x.grad, g, tag, 1e-6)


@pytest.mark.parametrize("tag", IOU)
def test_iou_restatement_matches_reference_vectors(golden, tag):
    g = golden("g22_losses.npz")
    w = g[f"{tag}/weight"]
    x = torch.from_numpy(g[f"{tag}/x"]).double().requires_grad_(True)
    loss = iou_restated(x, torch.from_numpy(g[f"{tag}/target"]), torch.from_numpy(w) if w.size else None, int(g[f"{tag}/mode"]))
    loss.backward()
    _check(loss, x.grad, g, tag, 1e-6)


def test_label_225_counts_as_class_zero_in_the_fixture(golden):
    g = golden("g22_losses.npz")
    assert (g["fl_225/target"] == 225).any()
    x = torch.from_numpy(g["fl_225/x"]).double()
    tgt = torch.from_numpy(g["fl_225/target"])
    a = focal_alpha(g, "fl_225", 2)
    as0 = focal_restated(x, torch.where(tgt == 225, torch.zeros_like(tgt), tgt), a, 2.0, 1e-5, True, True)
    as1 = focal_restated(x, torch.where(tgt == 225, torch.ones_like(tgt), tgt), a, 2.0, 1e-5, True, True)
    want = float(g["fl_225/loss"])
    assert abs(as0.item() - want) <= 1e-6 * abs(want) and abs(as1.item() - want) > 1e-2 * abs(want)


def test_tied_minimum_gradient_is_split_evenly(golden):
    """The two samples of mm_tie are identical: the min is attained once per sample, and each receives half of its gradient."""
    g = golden("g22_losses.npz")
    x = torch.from_numpy(g["mm_tie/x"]).double()
    assert torch.equal(x[0], x[1])
    gr = g["mm_tie/grad"]
    np.testing.assert_array_equal(gr[0], gr[1])
    # the restatement's full-reduction min() splits the tie the same way
    xx = x.clone().requires_grad_(True)
    iou_restated(xx, torch.from_numpy(g["mm_tie/target"]), None, 1).backward()
    assert np.abs(xx.grad.numpy() - gr).max() <= 1e-6 * np.abs(gr).max()


def test_get_alpha_counts_and_does_not_touch_the_batch(golden):
    g = golden("g22_losses.npz")
    batches = [{"L": torch.from_numpy(l.copy())} for l in g["alpha/labels"]]
    assert losses.get_alpha(batches) == [int(v) for v in g["alpha/counts"]]
    for b, l in zip(batches, g["alpha/labels"]):
        np.testing.assert_array_equal(b["L"].numpy(), l)          # 255 is still 255: the batch was not rewritten
    # float labels (what the trainer's loaders may hold) count the same
    fb = [{"L": b["L"].float()} for b in batches]
    assert losses.get_alpha(fb) == [int(v) for v in g["alpha/counts"]]


def test_new_entry_points_are_exported():
    names = set(_lib.EXPORTS)
    assert {"stcd_loss_focal", "stcd_loss_iou", "stcd_loss_iou_scratch_bytes"} <= names
    l = _lib.lib()
    assert l.stcd_loss_iou_scratch_bytes(16, 2, 256 * 256) > 0
    assert l.stcd_loss_iou_scratch_bytes(16, 17, 256 * 256) == 0


def test_unsupported_class_counts_are_refused_at_the_abi():
    """The checks run before anything touches the device: non-null dummy pointers are never dereferenced."""
    l = _lib.lib()
    buf = torch.zeros(8)
    p = buf.data_ptr()
    for C in (1, 17):
        assert l.stcd_loss_focal(p, p, 1, C, 4, None, 2.0, 1e-5, 1, p, None, p, None) != 0
        assert b"classes must be in [2, 16]" in l.stcd_last_error()
        assert l.stcd_loss_iou(p, p, 1, C, 4, None, 0, p, None, p, None) != 0
        assert b"classes must be in [2, 16]" in l.stcd_last_error()
    assert l.stcd_loss_iou(p, p, 1, 2, 4, None, 2, p, None, p, None) != 0 and b"mode" in l.stcd_last_error()


def test_losses_refuse_cpu_tensors_and_bad_alpha():
    x = torch.zeros(1, 2, 4, 4)
    t = torch.zeros(1, 1, 4, 4)
    for fn in (losses.FocalLoss(apply_nonlin=losses.softmax_helper), losses.mIoULoss(n_classes=2), losses.mmIoULoss(2)):
        with pytest.raises(_lib.StcdError):
            fn(x, t)
    with pytest.raises(ValueError):
        losses.FocalLoss(smooth=2.0)
    fl = losses.FocalLoss(alpha=[10, 0])
    with pytest.raises(ValueError):
        fl._alpha_vector(2, torch.device("cpu"))
    with pytest.raises(TypeError):
        losses.FocalLoss(alpha=3)._alpha_vector(2, torch.device("cpu"))
    np.testing.assert_allclose(losses.FocalLoss(alpha=[30, 10])._alpha_vector(2, torch.device("cpu")).numpy(), [4 / 3, 4.0], rtol=1e-6)
    np.testing.assert_allclose(losses.FocalLoss(alpha=0.25, balance_index=1)._alpha_vector(2, torch.device("cpu")).numpy(), [0.75, 0.25])


def test_softmax_helper_is_the_class_axis_softmax():
    x = torch.randn(2, 3, 5, 4, dtype=torch.float64)
    torch.testing.assert_close(losses.softmax_helper(x), torch.softmax(x, 1))
