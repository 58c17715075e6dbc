#!/usr/bin/env python3
"""One self-training round of the reference (/root/reference/train_stcd.py:40-52 CLI, :72-87 three checkpoints, :96-135 reliability
split, :137-204 pseudo-labels) on the HIP engine.  ``SiamUnet_diff(3, 1)`` trains on synthetic pairs (stcd_amd.synth) for
``--n_epochs`` and saves a checkpoint at each third (the reference's 20 / 40 / 60 of 60); the three checkpoints then score a
held-out set: ``select_reliable`` writes ``list/reliable_ids.txt`` and ``list/unreliable_ids.txt``, ``generate_pseudo_labels``
writes the masks of the unreliable half under ``pseudo_label/`` with the last checkpoint and the reference's score line is printed.
With ``--load_path`` holding three ``.pth`` files the training is skipped.

    python examples/selftrain_round_synth.py --n_epochs 6 --batch_size 8 --img_height 128 --img_width 128
"""
import argparse
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from stcd_amd import synth
from stcd_amd.modules import SiamUnet_diff
from stcd_amd.optim import FlatAdam
from stcd_amd.selftrain import generate_pseudo_labels, select_reliable

parser = argparse.ArgumentParser()      # the flags of train_stcd.py:40-52 that apply
parser.add_argument("--n_epochs", type=int, default=6, help="number of epochs of training; a checkpoint at each third")
parser.add_argument("--save_name", type=str, default="runs/STCD_round", help="checkpoints, list/ and pseudo_label/ go here")
parser.add_argument("--batch_size", type=int, default=8)
parser.add_argument("--img_height", type=int, default=128)
parser.add_argument("--img_width", type=int, default=128)
parser.add_argument("--load_path", type=str, default="", help="directory with three .pth checkpoints (sorted by name): skips training")
parser.add_argument("--train_pairs", type=int, default=64)
parser.add_argument("--pairs", type=int, default=64, help="held-out pairs the round scores")
parser.add_argument("--cumulative", action="store_true", help="the reference's never-reset metric instead of the per-pair IoU")


def device_pairs(n, h, w, seed, device):
    a, b, label = synth.make_pairs_u8(n, h, w, seed)
    return (torch.from_numpy(synth.normalize_nchw(a)).to(device), torch.from_numpy(synth.normalize_nchw(b)).to(device),
            torch.from_numpy(label).to(device))


def batches(x1, x2, label, names, batch):
    for s in range(0, len(names), batch):
        yield x1[s:s + batch], x2[s:s + batch], label[s:s + batch], names[s:s + batch]


def train_checkpoints(args, device):
    """-> the state_dicts after each third of the epochs (the reference keeps '%.2f_model.pth' % epoch, train_stcd.py:510)."""
    torch.manual_seed(1337)
    model = SiamUnet_diff(3, 1).to(device)
    optimizer = FlatAdam(model, lr=0.001, betas=(0.9, 0.999))
    x1, x2, label = device_pairs(args.train_pairs, args.img_height, args.img_width, 300, device)
    target = label.float().unsqueeze(1)
    rng = np.random.default_rng(301)
    thirds = sorted({max(1, round(args.n_epochs * k / 3)) for k in (1, 2, 3)})
    paths = []
    for epoch in range(1, args.n_epochs + 1):
        model.train()
        order = torch.from_numpy(rng.permutation(args.train_pairs)).to(device)
        total = torch.zeros((), device=device)
        steps = args.train_pairs // args.batch_size
        for i in range(steps):
            idx = order[i * args.batch_size:(i + 1) * args.batch_size]
            optimizer.zero_grad()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(model(x1[idx], x2[idx]), target[idx])
            loss.backward()
            optimizer.step()
            total += loss.detach()
        print("epoch %d: loss %.4f" % (epoch, total.item() / max(steps, 1)), flush=True)
        if epoch in thirds:
            paths.append(os.path.join(args.save_name, "%.2f_model.pth" % epoch))
            torch.save(model.state_dict(), paths[-1])
    return paths


def main(argv=None):
    args = parser.parse_args(argv)
    assert torch.cuda.is_available(), "the engine needs a GPU (no CPU fallback)"
    device = "cuda:0"
    os.makedirs(args.save_name, exist_ok=True)
    if args.load_path:
        paths = sorted(glob.glob(os.path.join(args.load_path, "*.pth")))
        assert len(paths) == 3, f"--load_path must hold three .pth files, found {len(paths)}"
    else:
        paths = train_checkpoints(args, device)
    models = []
    for p in paths:                                                             # train_stcd.py:75-87
        print("=> loading checkpoint '%s'" % p)
        m = SiamUnet_diff(3, 1)
        m.load_state_dict(torch.load(p, map_location="cpu"))
        models.append(m.to(device))

    x1, x2, label = device_pairs(args.pairs, args.img_height, args.img_width, 302, device)
    names = ["pair_%04d.png" % i for i in range(args.pairs)]
    t0 = time.perf_counter()
    sel = select_reliable(models, batches(x1, x2, label, names, args.batch_size), list_dir=os.path.join(args.save_name, "list"),
                          cumulative=args.cumulative)
    print("reliability split of %d pairs by %d checkpoints in %.3f s: %d reliable (min %.3f), %d unreliable (max %.3f)" %
          (len(names), len(models), time.perf_counter() - t0, len(sel.reliable), min(sel.reliability[names.index(n)] for n in sel.reliable),
           len(sel.unreliable), np.nanmax([sel.reliability[names.index(n)] for n in sel.unreliable])))
    idx = torch.tensor([names.index(n) for n in sel.unreliable], device=device)
    s = generate_pseudo_labels(models[-1], batches(x1[idx], x2[idx], label[idx], sel.unreliable, args.batch_size),
                               os.path.join(args.save_name, "pseudo_label"))
    print("change predictions:  train f1 %.3f, iou: %.3f, OA %.3f, Pre: %.3f, Rec: %.3f"             # train_stcd.py:203-204
          % (s["f1"][1], s["iou"][1], s["oa"], s["precision"][1], s["recall"][1]))
    return sel, s


if __name__ == "__main__":
    main()
