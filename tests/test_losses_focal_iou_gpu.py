"""Focal / mIoU / min-max IoU through stcd_amd.losses -> stcd_loss_focal / stcd_loss_iou on the GPU: the reference's own vectors
(tests/golden/g22_losses.npz), the upstream gradient, bit-reproducibility, bench-sized agreement with a torch restatement, the
NaN convention for labels out of range, and CDTrainer with --loss fl / miou / mmiou end to end."""
import os

import numpy as np
import pytest
import torch

from stcd_amd import losses
from tests._util import t
from tests.test_losses_focal_iou_cpu import FOCAL, IOU, focal_alpha, focal_restated, iou_restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-4


def _focal_module(g, tag):
    prm = g[f"{tag}/params"]
    gamma, smooth, size_average, fused, kind, bi, af = prm.tolist()
    alpha = None if kind == 0 else ([int(v) for v in g[f"{tag}/alpha_counts"]] if kind == 1 else float(af))
    return losses.FocalLoss(apply_nonlin=losses.softmax_helper if fused else None, alpha=alpha, gamma=gamma,
                            balance_index=int(bi), smooth=smooth, size_average=bool(size_average))


def _iou_module(g, tag, C):
    if int(g[f"{tag}/mode"]) == 0:
        return losses.mIoULoss(weight=t(g[f"{tag}/weight"]).to(DEV), size_average=True, n_classes=C)
    return losses.mmIoULoss(n_classes=C)


def _bounds(loss, grad, want_loss, want_grad, what):
    want_grad = np.asarray(want_grad, np.float64)
    rel = abs(loss - want_loss) / abs(want_loss)
    gerr = np.abs(np.asarray(grad, np.float64) - want_grad).max() / np.abs(want_grad).max()
    assert rel <= LOSS_RTOL, f"{what}: loss {loss} vs {want_loss} (relative error {rel:.2e})"
    assert gerr <= GRAD_RTOL, f"{what}: max|g - g_ref| / max|g_ref| = {gerr:.2e}"


@pytest.mark.parametrize("tag", FOCAL + IOU)
def test_reference_vectors(golden, tag):
    g = golden("g22_losses.npz")
    x = t(g[f"{tag}/x"]).to(DEV).requires_grad_(True)
    tgt = t(g[f"{tag}/target"]).to(DEV)
    fn = _focal_module(g, tag) if tag in FOCAL else _iou_module(g, tag, x.shape[1])
    loss = fn(x, tgt.float())                        # the trainer hands a float N*1*H*W label
    loss.backward()
    _bounds(loss.item(), x.grad.cpu().numpy(), float(g[f"{tag}/loss"]), g[f"{tag}/grad"], tag)
    # integer N*H*W labels give the same bits
    x2 = t(g[f"{tag}/x"]).to(DEV).requires_grad_(True)
    l2 = fn(x2, tgt[:, 0])
    l2.backward()
    assert l2.item() == loss.item() and torch.equal(x2.grad, x.grad)


@pytest.mark.parametrize("tag", ["fl_counts_g2", "fl_prob", "miou_c4", "mm_tie"])
def test_upstream_gradient_is_honoured(golden, tag):
    g = golden("g22_losses.npz")
    x = t(g[f"{tag}/x"]).to(DEV).requires_grad_(True)
    fn = _focal_module(g, tag) if tag in FOCAL else _iou_module(g, tag, x.shape[1])
    (3.0 * fn(x, t(g[f"{tag}/target"]).to(DEV))).backward()
    _bounds(float(g[f"{tag}/loss"]), x.grad.cpu().numpy(), float(g[f"{tag}/loss"]), 3.0 * g[f"{tag}/grad"], tag + " x3")


def test_focal_with_another_nonlinearity_runs_it_in_torch(golden):
    """apply_nonlin = any callable other than softmax_helper: applied in torch, then the probability path; autograd chains the two."""
    g = golden("g22_losses.npz")
    fused = _focal_module(g, "fl_counts_g2")
    other = losses.FocalLoss(apply_nonlin=lambda z: torch.softmax(z, 1), alpha=fused.alpha, gamma=2, smooth=1e-5)
    x = t(g["fl_counts_g2/x"]).to(DEV).requires_grad_(True)
    loss = other(x, t(g["fl_counts_g2/target"]).to(DEV))
    loss.backward()
    _bounds(loss.item(), x.grad.cpu().numpy(), float(g["fl_counts_g2/loss"]), g["fl_counts_g2/grad"], "torch softmax + probability path")


def _bench_inputs(shape, seed, C=2):
    rng = np.random.default_rng(seed)
    N, _, H, W = shape
    x = t((2.0 * rng.standard_normal(shape)).astype(np.float32)).to(DEV)
    lab = t((rng.random((N, 1, H, W)) < 0.05).astype(np.int64)).to(DEV)     # a change mask: a few percent of the pixels
    return x, lab


def _three_losses(lab):
    counts = torch.bincount(lab.flatten().cpu(), minlength=2).tolist()
    freq = np.asarray(counts, np.float64) / sum(counts)
    w = 1 - torch.from_numpy(freq).to(DEV)
    return {"fl": (losses.FocalLoss(apply_nonlin=losses.softmax_helper, alpha=counts, gamma=2, smooth=1e-5),
                   lambda x, y: focal_restated(x, y, 1.0 / torch.tensor(freq, dtype=torch.float64, device=DEV), 2.0, 1e-5, True, True)),
            "miou": (losses.mIoULoss(weight=w, n_classes=2), lambda x, y: iou_restated(x, y, w, 0)),
            "mmiou": (losses.mmIoULoss(n_classes=2), lambda x, y: iou_restated(x, y, None, 1))}


@pytest.mark.parametrize("shape", [(16, 2, 256, 256), (4, 2, 512, 512)])
def test_bench_sized_against_the_restatement_and_bit_reproducible(shape):
    x, lab = _bench_inputs(shape, 5)
    for name, (fn, ref) in _three_losses(lab).items():
        runs = []
        for _ in range(2):
            xg = x.clone().requires_grad_(True)
            loss = fn(xg, lab.float())
            loss.backward()
            runs.append((loss.detach().clone(), xg.grad.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{name}: two calls differ"
        loss, grad = runs[0]
        assert torch.isfinite(loss) and torch.isfinite(grad).all(), name
        xr = x.double().requires_grad_(True)
        want = ref(xr, lab)
        want.backward()
        _bounds(loss.item(), grad.cpu().numpy(), want.item(), xr.grad.cpu().numpy(), f"{name} {shape}")


def test_identical_samples_tie_exactly_at_bench_size():
    """Chunking of the IoU partials depends on H*W alone: two identical samples give bit-identical (I, U), so the min is tied and
    its gradient is split evenly -- each sample receives the same gradient, bit for bit."""
    x, lab = _bench_inputs((2, 2, 256, 256), 6)
    x[1], lab[1] = x[0], lab[0]
    xg = x.clone().requires_grad_(True)
    losses.mmIoULoss(2)(xg, lab).backward()
    assert torch.equal(xg.grad[0], xg.grad[1])
    xr = x.double().requires_grad_(True)
    iou_restated(xr, lab, None, 1).backward()
    _bounds(1.0, xg.grad.cpu().numpy(), 1.0, xr.grad.cpu().numpy(), "tie at 256x256")


def test_out_of_range_label_gives_nan():
    rng = np.random.default_rng(8)
    x = t(rng.standard_normal((2, 2, 16, 16)).astype(np.float32)).to(DEV)
    for fn, bads in ((losses.FocalLoss(apply_nonlin=losses.softmax_helper), (2, -1, 255, 10 ** 12)),
                     (losses.mIoULoss(n_classes=2), (2, -1, 225)), (losses.mmIoULoss(2), (2, 255))):
        for bad in bads:
            lab = t((rng.random((2, 1, 16, 16)) < 0.3).astype(np.int64)).to(DEV)
            lab[1, 0, 3, 5] = bad
            xg = x.clone().requires_grad_(True)
            loss = fn(xg, lab)
            loss.backward()
            assert torch.isnan(loss), (type(fn).__name__, bad)
            assert torch.isnan(xg.grad[1, :, 3, 5]).all(), (type(fn).__name__, bad)
    # 225 is class 0 for the focal loss, as in the reference: finite
    lab = torch.zeros(2, 1, 16, 16, dtype=torch.int64, device=DEV)
    lab[0, 0, 0, 0] = 225
    assert torch.isfinite(losses.FocalLoss(apply_nonlin=losses.softmax_helper)(x, lab))


# ------------------------------------------------------------------ CDTrainer with --loss fl / miou / mmiou
def _loaders(n_train=8):
    from tests.test_trainer_gpu import PairSet
    return {"train": torch.utils.data.DataLoader(PairSet(n_train, 64, 1, True), batch_size=4, shuffle=False),
            "val": torch.utils.data.DataLoader(PairSet(4, 64, 2, True), batch_size=4)}


def _recording(tr):
    rec = []
    fn = tr._pxl_loss

    def wrapped(pred, gt):
        out = fn(pred, gt)
        rec.append(out.detach())
        return out
    tr._pxl_loss = wrapped
    return rec


@pytest.mark.parametrize("loss", ["fl", "miou", "mmiou"])
def test_cdtrainer_trains_with_the_loss(tmp_path, loss):
    from stcd_amd.trainer import CDTrainer
    from tests.test_trainer_gpu import _args

    torch.manual_seed(0)
    loaders = _loaders(16)
    args = _args(str(tmp_path), net_G="SiamUnet_abs", loss=loss)
    tr = CDTrainer(args, loaders)
    counts = losses.get_alpha(loaders["train"])
    if loss == "fl":
        assert isinstance(tr._pxl_loss, losses.FocalLoss) and tr._pxl_loss.alpha == counts
        assert tr._pxl_loss.apply_nonlin is losses.softmax_helper and tr._pxl_loss.gamma == 2 and tr._pxl_loss.smooth == 1e-5
    elif loss == "miou":
        assert isinstance(tr._pxl_loss, losses.mIoULoss) and tr._pxl_loss.classes == 2
        freq = np.asarray(counts, np.float64) / sum(counts)
        np.testing.assert_allclose(tr._pxl_loss.weights.cpu().numpy(), 1 - freq, rtol=1e-12)
    else:
        assert isinstance(tr._pxl_loss, losses.mmIoULoss) and tr._pxl_loss.classes == 2
    rec = _recording(tr)
    tr.train_models()
    vals = torch.stack(rec).cpu().numpy()
    steps = len(loaders["train"])
    assert len(vals) == 2 * steps and np.isfinite(vals).all()
    assert vals[steps:].mean() < vals[:steps].mean(), vals                 # the second epoch's loss is below the first's
    ck = torch.load(os.path.join(args.checkpoint_dir, "last_ckpt.pt"), weights_only=False)
    assert ck["epoch_id"] == 1 and len(tr.VAL_ACC) == 2
    assert os.path.exists(os.path.join(args.checkpoint_dir, "best_ckpt.pt"))
    # resume continues at epoch 2 with the same loss
    tr2 = CDTrainer(_args(str(tmp_path), net_G="SiamUnet_abs", loss=loss, max_epochs=3), loaders)
    rec2 = _recording(tr2)
    tr2.train_models()
    assert tr2.epoch_to_start == 2 and len(tr2.VAL_ACC) == 3 and len(rec2) == steps
    assert np.isfinite(torch.stack(rec2).cpu().numpy()).all()


def test_cdtrainer_changeformer_multi_scale_focal_loss(tmp_path):
    """ChangeFormerV6 with --loss fl and multi_scale_train == "True": one FocalLoss call per map at the map's own size (the label
    resized by nearest), the auxiliary heads learn."""
    from stcd_amd.trainer import CDTrainer
    from tests.test_trainer_gpu import _args

    torch.manual_seed(0)
    args = _args(str(tmp_path), net_G="ChangeFormerV6", loss="fl", multi_scale_train="True", multi_scale_infer="False",
                 multi_pred_weights=[0.5, 0.5, 0.5, 0.8, 1.0], lr=2e-4, max_epochs=2, embed_dim=64)
    tr = CDTrainer(args, _loaders())
    assert isinstance(tr._pxl_loss, losses.FocalLoss)
    before = {k: v.detach().clone() for k, v in tr.net_G.state_dict().items()
              if "make_pred_c3" in k and v.dtype.is_floating_point and "running" not in k}
    rec = _recording(tr)
    tr.train_models()
    vals = torch.stack(rec).cpu().numpy()
    assert len(vals) == 5 * 2 * 2 and np.isfinite(vals).all()              # five maps x two steps x two epochs
    after = tr.net_G.state_dict()
    assert before and all(not torch.equal(v, after[k]) for k, v in before.items())
