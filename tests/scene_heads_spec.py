"""numpy restatement of stcd_scene_finalize_seg (include/stcd_hip.h), built on tests/scene_spec.py: the three masks of SegCD's
stitched heads, the decision-level gate sketched in train_stcd.py:170-176 and the four confusion matrices.  Like scene_spec it states the
library's own specification and lives beside the tests; not collected by pytest."""
import numpy as np

from tests import scene_spec as SP

ROWS = ("seg_a", "seg_b", "change", "gated")


def count(pred, label):
    """int64 [4], cm[2 * label + pred] over the pixels whose label is not 255 (>= 1 is set)."""
    ok = label != 255
    return np.bincount(2 * (label[ok] >= 1).astype(np.int64) + (pred[ok] != 0).astype(np.int64), minlength=4).astype(np.int64)


def finalize_seg(acc, wsum, seg_threshold=0.0, change_threshold=0.0, label_a=None, label_b=None, label_c=None, cm=None):
    """acc [3 * classes, H, W] in the order (t1, t2, change) over one wsum [H, W] ->
    (seg_a, seg_b, change, gated uint8 [H,W], prob float64 [3,H,W], cm int64 [4,4] or None).
    Each head is scene_spec.finalize on its own planes; gated = change & (seg_a != seg_b); row r of cm is added to only where its
    label is given (rows 2 and 3 share label_c), starting from the `cm` passed in (zeros if None and a label is given)."""
    acc = np.asarray(acc)
    classes = acc.shape[0] // 3
    assert acc.shape[0] == 3 * classes and classes in (1, 2)
    masks, probs = [], []
    for h, thr in enumerate((seg_threshold, seg_threshold, change_threshold)):
        m, p, _ = SP.finalize(acc[h * classes:(h + 1) * classes], wsum, thr)
        masks.append(m)
        probs.append(p)
    gated = (masks[2] & (masks[0] != masks[1])).astype(np.uint8)
    labels = (label_a, label_b, label_c, label_c)
    out = None
    if any(l is not None for l in labels):
        out = np.zeros((4, 4), np.int64) if cm is None else np.array(cm, np.int64).reshape(4, 4).copy()
        for r, (pred, lab) in enumerate(zip(masks + [gated], labels)):
            if lab is not None:
                out[r] += count(pred, np.asarray(lab))
    return masks[0], masks[1], masks[2], gated, np.stack(probs), out
