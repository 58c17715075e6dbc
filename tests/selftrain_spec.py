"""numpy / plain-Python statement of the self-training round (include/stcd_hip.h: stcd_selftrain_score; stcd_amd/selftrain.py:
reliability, split_reliable).  It says what /root/reference/train_stcd.py:102-134,155-177 compute, one pair and one checkpoint at
a time, in the order the reference walks them; the GPU tests hold the kernel to `score`, the CPU tests hold the vectorised host
code to the loops below and both to the fixture recorded from the reference's own metric class.  Not collected by pytest."""
import numpy as np


def predict(logits, threshold=0.0):
    """fp32 [B,classes,hw] -> bool [B,hw].  One class: strictly above the threshold; two: class 1 strictly above class 0 (a tie is
    class 0, torch.argmax).  NaN compares false."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32 and logits.ndim == 3 and logits.shape[1] in (1, 2)
    with np.errstate(invalid="ignore"):
        if logits.shape[1] == 1:
            return logits[:, 0] > np.float32(threshold)
        return logits[:, 1] > logits[:, 0]


def score(logits_list, threshold=0.0, label=None, mask_value=1):
    """-> (mask uint8 [B,hw], agree int64 [B,K-1,4] or None, cm int64 [4] or None); agree[b, i, 2 * last + pred_i], cm[2 * label + pred_last]."""
    preds = [predict(l, threshold) for l in logits_list]
    last = preds[-1]
    B = last.shape[0]
    mask = (last * mask_value).astype(np.uint8)
    agree = None
    if len(preds) > 1:
        agree = np.zeros((B, len(preds) - 1, 4), np.int64)
        for b in range(B):
            for i in range(len(preds) - 1):
                agree[b, i] = np.bincount(2 * last[b].astype(np.int64) + preds[i][b].astype(np.int64), minlength=4)
    cm = None
    if label is not None:
        label = np.asarray(label)
        ok = label != 255
        cm = np.bincount(2 * (label[ok] >= 1).astype(np.int64) + last[ok].astype(np.int64), minlength=4).astype(np.int64)
    return mask, agree, cm


def iou1(m):
    """IoU of class 1 of a 2 x 2 matrix m[label, pred] of float64 counts, the reference's formula (train_stcd.py:553-561):
    diag / (row sums + column sums - diag).  0 / 0 is NaN."""
    m = np.asarray(m, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return m[1, 1] / ((m[1, 0] + m[1, 1]) + (m[0, 1] + m[1, 1]) - m[1, 1])


def reliability_cumulative(agree):
    """The reference's literal loop (:102-125): ONE matrix for the whole run, never reset; after each addBatch the IoU of class 1 of
    what has accumulated so far is appended; reliability = sum(mIOU) / len(mIOU)."""
    agree = np.asarray(agree).reshape(len(agree), -1, 2, 2)
    running = np.zeros((2, 2), np.float64)
    out = []
    for per_pair in agree:
        ious = []
        for m in per_pair:
            running += m
            ious.append(iou1(running))
        out.append(sum(ious) / len(ious))
    return np.asarray(out, np.float64)


def reliability_per_pair(agree):
    """The library's default: a fresh matrix per pair and checkpoint; an empty union is full agreement, 1.0."""
    agree = np.asarray(agree).reshape(len(agree), -1, 2, 2)
    out = []
    for per_pair in agree:
        ious = []
        for m in per_pair:
            v = iou1(m)
            ious.append(1.0 if m[1, 1] + m[1, 0] + m[0, 1] == 0 else v)
        out.append(sum(ious) / len(ious))
    return np.asarray(out, np.float64)


def order(rel):
    """Indices by descending reliability, ties in input order (Python's stable sort with reverse=True, :127), NaN last in input order."""
    rel = [float(r) for r in rel]
    pairs = [(i, r) for i, r in enumerate(rel) if r == r]
    pairs.sort(key=lambda e: e[1], reverse=True)
    return [i for i, _ in pairs] + [i for i, r in enumerate(rel) if r != r]


def split(names, rel):
    ranked = [names[i] for i in order(rel)]
    return ranked[:len(ranked) // 2], ranked[len(ranked) // 2:]
