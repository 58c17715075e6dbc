#!/usr/bin/env python3
"""Generate tests/golden/g22_losses.npz from the REFERENCE's own loss classes (models/losses.py: get_alpha, FocalLoss,
mIoULoss, mmIoULoss), run on the CPU in float64 so that the vectors are the exact target.

Run in the authoring container only (needs a checkout of the reference, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_loss_golden.py <reference checkout>

The fixture holds arrays only: inputs (fp32, what the kernels read; the reference runs on them cast to float64), targets, the
settings of each case, loss values (float64) and d loss / d input (the float64 result rounded to fp32).
  fl_*   FocalLoss: alpha None / class counts / float (balance_index=1), gamma 2 and 0.5, size_average True and False,
         apply_nonlin=softmax_helper on logits and None on probabilities, labels 225 (counted as class 0)
  miou_* mIoULoss with C = 2 and 4
  mm_*   mmIoULoss, one batch whose two samples are identical (the min is tied between them)
  alpha  get_alpha counts of a small synthetic loader (labels 0 / 1 / 255)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
# settings vector of a focal case: gamma, smooth, size_average, fused softmax, alpha kind (0 None, 1 counts, 2 float),
# balance_index, alpha float value
FL_KIND = {None: 0, "counts": 1, "float": 2}


def load_reference(root):
    path = os.path.join(root, "models", "losses.py")
    spec = importlib.util.spec_from_file_location("reference_losses", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def t2n(t):
    return t.detach().cpu().numpy().copy()


def main(root):
    R = load_reference(root)
    d = {}
    rng = np.random.default_rng(2207)

    def labels(shape, C, p_change=None):
        if p_change is not None and C == 2:
            return (rng.random(shape) < p_change).astype(np.int64)
        return rng.integers(0, C, size=shape).astype(np.int64)

    def focal(tag, shape, gamma, alpha_kind, size_average=True, fused=True, with225=False, balance_index=0, alpha_float=0.25):
        N, C, H, W = shape
        x = (rng.standard_normal(shape) * 2.0).astype(np.float32)
        tgt = labels((N, 1, H, W), C, 0.15)
        if with225:
            tgt[rng.random(tgt.shape) < 0.1] = 225
        if alpha_kind == "counts":
            alpha = [int(v) for v in np.bincount(np.where(tgt == 225, 0, tgt).ravel(), minlength=C)]
        elif alpha_kind == "float":
            alpha = float(alpha_float)
        else:
            alpha = None
        if not fused:        # probabilities in, the gradient is d loss / d probability
            x = torch.softmax(torch.from_numpy(x).double(), 1).float().numpy()
        xt = torch.from_numpy(x).double().requires_grad_(True)
        fl = R.FocalLoss(apply_nonlin=R.softmax_helper if fused else None, alpha=alpha, gamma=gamma, balance_index=balance_index,
                         smooth=1e-5, size_average=size_average)
        loss = fl(xt, torch.from_numpy(tgt.copy()))          # a copy: the reference rewrites 225 -> 0 in the caller's tensor
        loss.backward()
        d[f"{tag}/x"], d[f"{tag}/target"] = x, tgt
        d[f"{tag}/loss"], d[f"{tag}/grad"] = t2n(loss), t2n(xt.grad).astype(np.float32)
        d[f"{tag}/params"] = np.array([gamma, 1e-5, float(size_average), float(fused), FL_KIND[alpha_kind], balance_index,
                                       alpha_float if alpha_kind == "float" else 0.0], np.float64)
        d[f"{tag}/alpha_counts"] = np.array(alpha if alpha_kind == "counts" else [], np.int64)

    focal("fl_none_g2", (2, 2, 32, 32), 2.0, None)
    focal("fl_counts_g2", (3, 4, 24, 40), 2.0, "counts")
    focal("fl_float_g05", (2, 2, 32, 32), 0.5, "float", balance_index=1)
    focal("fl_counts_sum", (2, 2, 32, 32), 2.0, "counts", size_average=False)
    focal("fl_prob", (2, 3, 16, 16), 2.0, None, fused=False)
    focal("fl_225", (2, 2, 32, 32), 2.0, "counts", with225=True)
    focal("fl_none_g05_sum", (2, 3, 24, 20), 0.5, None, size_average=False)

    def iou(tag, shape, mode, tie=False):
        N, C, H, W = shape
        x = (rng.standard_normal(shape) * 2.0).astype(np.float32)
        tgt = labels((N, 1, H, W), C, 0.3)
        if tie:
            x[1], tgt[1] = x[0], tgt[0]
        xt = torch.from_numpy(x).double().requires_grad_(True)
        if mode == 0:
            freq = np.bincount(tgt.ravel(), minlength=C) / tgt.size
            weight = 1 - torch.from_numpy(freq)             # the trainer's weights (models/trainer.py:106-108)
            loss = R.mIoULoss(weight=weight, n_classes=C)(xt, torch.from_numpy(tgt))
            d[f"{tag}/weight"] = t2n(weight)
        else:
            loss = R.mmIoULoss(n_classes=C)(xt, torch.from_numpy(tgt))
            d[f"{tag}/weight"] = np.zeros(0)
        loss.backward()
        if tie:
            g = t2n(xt.grad)
            assert np.array_equal(g[0], g[1]), "tie case: the two identical samples must receive the same gradient"
        d[f"{tag}/x"], d[f"{tag}/target"] = x, tgt
        d[f"{tag}/loss"], d[f"{tag}/grad"] = t2n(loss), t2n(xt.grad).astype(np.float32)
        d[f"{tag}/mode"] = np.array(mode, np.int64)

    iou("miou_c2", (2, 2, 32, 32), 0)
    iou("miou_c4", (3, 4, 24, 40), 0)
    iou("mm_tie", (2, 2, 32, 32), 1, tie=True)
    iou("mm_c4", (3, 4, 24, 40), 1)

    # get_alpha over a small loader: batches of {"L": [b, 1, h, w]} with labels 0, 1 and 255 (255 counts as class 0)
    batches = []
    for b in range(3):
        lab = (rng.random((2, 1, 16, 16)) < 0.2).astype(np.int64)
        lab[rng.random(lab.shape) < 0.05] = 255
        batches.append(lab)
    counts = R.get_alpha([{"L": torch.from_numpy(l.copy())} for l in batches])
    d["alpha/labels"] = np.stack(batches)
    d["alpha/counts"] = np.array(counts, np.int64)

    path = os.path.join(OUT, "g22_losses.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in d.items()})
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.dont_write_bytecode = True
    torch.set_num_threads(4)
    main(sys.argv[1])
