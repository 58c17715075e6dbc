"""Throughput of the reliability split of one self-training round, pairs/s: the device path against the reference's method.
python tools/selftrain_bench.py --model diff|segcd [--k 3] [--pairs 8192] [--batch 16] [--size 256] [--rounds 5]

Four legs over the same K checkpoints (bf16 eval forward, frozen weights) and the same pairs, a seeded pool of device-resident
batches walked round and round; every leg ends in a device synchronise inside its timed window:
  a  stcd_amd.selftrain.select_reliable: one stcd_selftrain_score launch per batch, counts copied back once per 64 batches
  b  the same K forwards, then the reference's op sequence per pair and checkpoint (train_stcd.py:111-125): sigmoid, > 0.5, .int(),
     .cpu(), and torch.bincount on the host into one float64 matrix
  c  the same op sequence kept on the device in torch, per batch (one bincount per earlier checkpoint with a per-pair offset), the
     counts copied back once per 64 batches
  d  the bare K forwards
The legs alternate within one process, every shape is warmed up first; the figures are the medians of --rounds rounds, the spread
is their min and max.  One JSON line."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import selftrain, synth
from stcd_amd.scene import _change_logits

ap = argparse.ArgumentParser(); ap.add_argument("--model", default="diff", choices=("diff", "segcd")); ap.add_argument("--k", type=int, default=3)
ap.add_argument("--pairs", type=int, default=8192); ap.add_argument("--batch", type=int, default=16); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--pool", type=int, default=8, help="distinct batches in the pool")
ap.add_argument("--flush", type=int, default=64)
a = ap.parse_args()
dev = "cuda:0"
models = []
for i in range(a.k):
    torch.manual_seed(900 + i)
    if a.model == "segcd":
        from stcd_amd.segcd import SegCD
        models.append(SegCD(dtype="bf16").to(dev).eval())
    else:
        from stcd_amd.modules import SiamUnet_diff
        models.append(SiamUnet_diff(3, 1, dtype="bf16").to(dev).eval())
pool = []
for j in range(a.pool):
    x1, x2, _ = synth.make_batch(a.batch, a.size, a.size, seed=40 + j)
    pool.append((torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)))
K, B = a.k, a.batch


def walk(pairs):
    for n in range(pairs // B):
        x1, x2 = pool[n % len(pool)]
        yield n, x1, x2


def leg_a(pairs):
    sel = selftrain.select_reliable(models, ((x1, x2, None, [f"{n}_{j}" for j in range(B)]) for n, x1, x2 in walk(pairs)), flush=a.flush)
    torch.cuda.synchronize()
    return sel.reliability


def leg_b(pairs):
    cm = torch.zeros((2, 2), dtype=torch.float64)                      # the reference's metric: created once, never reset
    rel = []
    with selftrain._evaluating(models):
        for n, x1, x2 in walk(pairs):
            outs = [_change_logits(m(x1, x2)).float() for m in models]
            for j in range(B):
                preds = [(torch.sigmoid(o[j:j + 1]) > 0.5).int().cpu() for o in outs]
                ious = []
                for i in range(K - 1):
                    cm += torch.bincount(2 * preds[-1].flatten() + preds[i].flatten(), minlength=4).reshape(2, 2)
                    ious.append(cm[1, 1] / (cm[1].sum() + cm[:, 1].sum() - cm[1, 1]))
                rel.append(sum(ious) / len(ious))
        torch.cuda.synchronize()
    return rel


def leg_c(pairs):
    offset = (4 * torch.arange(B, device=dev)).reshape(B, 1)
    pending, done = [], []
    with selftrain._evaluating(models):
        for n, x1, x2 in walk(pairs):
            preds = [(torch.sigmoid(_change_logits(m(x1, x2)).float()) > 0.5).int().reshape(B, -1) for m in models]
            pending.append(torch.stack([torch.bincount((offset + 2 * preds[-1] + preds[i]).flatten(), minlength=4 * B) for i in range(K - 1)]))
            if len(pending) >= a.flush:
                done.append(torch.stack(pending).cpu()); pending = []
        if pending:
            done.append(torch.stack(pending).cpu())
        torch.cuda.synchronize()
    agree = torch.cat(done).reshape(-1, K - 1, B, 2, 2).permute(0, 2, 1, 3, 4).reshape(-1, K - 1, 2, 2).numpy()
    return selftrain.reliability(agree)


def leg_d(pairs):
    with selftrain._evaluating(models):
        for n, x1, x2 in walk(pairs):
            for m in models:
                m(x1, x2)
        torch.cuda.synchronize()


legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
warm = min(a.pairs, B * max(len(pool), a.flush + 1))
ra = leg_a(warm); leg_b(B * 2); rc = leg_c(warm); leg_d(warm)                 # every shape and code path once, untimed
same = bool(np.array_equal(ra, rc))                                          # (only a logit in (0, 6e-8] may part "x > 0" from "sigmoid(x) > 0.5")
rates = {k: [] for k in legs}
for r in range(a.rounds):
    for k, fn in legs.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(a.pairs)
        rates[k].append(a.pairs / (time.perf_counter() - t0))
med = {k: statistics.median(v) for k, v in rates.items()}
print(json.dumps({"tool": "selftrain_bench", "model": a.model, "k": K, "pairs": a.pairs, "batch": B, "size": a.size, "rounds": a.rounds, "dtype": "bf16", "a_equals_c": same,
                  "pairs_per_s": {k: round(v, 1) for k, v in med.items()},
                  "spread": {k: [round(min(v), 1), round(max(v), 1)] for k, v in rates.items()},
                  "a_over_b": round(med["a"] / med["b"], 3), "a_over_c": round(med["a"] / med["c"], 3), "a_over_d": round(med["a"] / med["d"], 3),
                  "legs": {"a": "select_reliable", "b": "reference op sequence per pair, host bincount", "c": "op sequence on the device in torch",
                           "d": "bare forwards"}}), flush=True)
