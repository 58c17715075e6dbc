#!/usr/bin/env python3
"""Writes tests/golden/selftrain_metric.npz: what the reference's OWN metric class makes of the reliability loop.

/root/reference/train_stcd.py cannot be imported (it parses argv and touches cuDNN at import), so the single class
``SegmentationMetric`` (:515-593) is compiled from the file by ``ast`` into a namespace of torch / nn (the recipe of
tests/golden/make_golden.py, g21): no reference text enters this repository, the fixture holds arrays only.

Two cases (a: K = 3, N = 24, 32 x 32; b: K = 4, N = 17, 20 x 12), each with
  <c>/masks        uint8 [K,N,h,w] in {0,1}: the K checkpoints' binary predictions (random rectangles plus flipped pixels)
  <c>/cumulative   float64 [N]: the reliabilities of the reference's literal loop (:102-125): ONE metric for the whole loop, on the
                   CPU (the reference asks for 'cuda:0', which its reset() does not recognise, so its matrix lives on the CPU too)
  <c>/order        int64: the order its stable sort (:127) gives, over the pairs whose cumulative reliability is finite (all of case
                   a; case b starts with a pair without change, whose 0 / 0 leaves Python's sort without a defined answer)
  <c>/fresh        float64 [N,K-1]: IoU of class 1 from a fresh metric per pair and checkpoint (NaN where the union is empty)

The generator asserts what makes the comparison strict; see the asserts in `case`.

    python tests/golden/make_selftrain_golden.py
"""
import ast
import os

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference/train_stcd.py"


def reference_metric():
    nodes = [n for n in ast.parse(open(REFERENCE).read()).body if isinstance(n, ast.ClassDef) and n.name == "SegmentationMetric"]
    assert len(nodes) == 1
    ns = {"torch": torch, "nn": nn}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), REFERENCE, "exec"), ns)
    return ns["SegmentationMetric"]


def make_masks(rng, K, N, h, w, empty, last_empty, identical):
    masks = np.zeros((K, N, h, w), np.uint8)
    for n in range(N):
        if n in empty:
            continue
        base = np.zeros((h, w), bool)
        for _ in range(int(rng.integers(1, 4))):
            rh, rw = int(rng.integers(2, h // 2 + 1)), int(rng.integers(2, w // 2 + 1))
            y0, x0 = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
            base[y0:y0 + rh, x0:x0 + rw] = True
        for k in range(K):
            flip = rng.random((h, w)) < 0.03 * (K - k)                # the earlier the checkpoint, the noisier
            masks[k, n] = base if n in identical else base ^ flip
        if n in last_empty:
            masks[K - 1, n] = 0
    return masks


def case(Metric, seed, K, N, h, w, empty, last_empty, identical):
    masks = make_masks(np.random.default_rng(seed), K, N, h, w, empty, last_empty, identical)
    # ---- the reference's loop, :102-125, batch size 1, predictions as [1,1,h,w] int tensors on the CPU
    metric = Metric(numClass=2, device="cuda:0")
    id_to_reliability = []
    for n in range(N):
        preds = [torch.from_numpy(masks[k, n]).int().reshape(1, 1, h, w) for k in range(K)]
        mIOU = []
        for i in range(len(preds) - 1):
            metric.addBatch(preds[i], preds[-1])
            mIOU.append(metric.IntersectionOverUnion()[1])
        reliability = sum(mIOU) / len(mIOU)
        id_to_reliability.append((n, reliability))
    cumulative = np.array([float(r) for _, r in id_to_reliability], np.float64)
    finite = [e for e in id_to_reliability if not bool(torch.isnan(e[1]))]
    finite.sort(key=lambda elem: elem[1], reverse=True)
    order = np.array([e[0] for e in finite], np.int64)
    # ---- a fresh metric per pair and checkpoint
    fresh = np.empty((N, K - 1), np.float64)
    for n in range(N):
        last = torch.from_numpy(masks[K - 1, n]).int().reshape(1, 1, h, w)
        for i in range(K - 1):
            m = Metric(numClass=2, device="cuda:0")
            m.addBatch(torch.from_numpy(masks[i, n]).int().reshape(1, 1, h, w), last)
            fresh[n, i] = float(m.IntersectionOverUnion()[1])
    # ---- what the comparison needs in order to be strict
    assert np.isfinite(cumulative[1:]).all(), "cumulative reliabilities must be finite from the second pair on"
    fin = cumulative[np.isfinite(cumulative)]
    assert len(set(fin.tolist())) == len(fin), "cumulative reliabilities must be pairwise distinct (unique order)"
    all_empty = [n for n in range(N) if not masks[:, n].any()]
    assert len(all_empty) >= 3 and np.isnan(fresh[all_empty]).all(), "at least three pairs with an empty union in every matrix"
    only_last = [n for n in range(N) if not masks[K - 1, n].any() and all(masks[k, n].any() for k in range(K - 1))]
    assert len(only_last) >= 1 and (fresh[only_last] == 0).all(), "at least one pair with an empty last mask only"
    assert all((fresh[n] == 1.0).all() for n in identical), "identical masks agree fully"
    return {"masks": masks, "cumulative": cumulative, "order": order, "fresh": fresh}


def main():
    Metric = reference_metric()
    out = {}
    for tag, kw in (("a", dict(seed=4101, K=3, N=24, h=32, w=32, empty={3, 9, 17}, last_empty={6}, identical={12})),
                    ("b", dict(seed=4102, K=4, N=17, h=20, w=12, empty={0, 5, 11, 15}, last_empty={8}, identical={13}))):
        for k, v in case(Metric, **kw).items():
            out[f"{tag}/{k}"] = v
        c = out[f"{tag}/cumulative"]
        print(f"case {tag}: {int(np.isnan(c).sum())} NaN, cumulative in [{np.nanmin(c):.4f}, {np.nanmax(c):.4f}], order starts {out[f'{tag}/order'][:6].tolist()}")
    path = os.path.join(HERE, "selftrain_metric.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
