#!/usr/bin/env python3
"""The self-training round of the reference (train_stcd.py:96-204) on one WHOLE scene pair instead of pre-cut crops
(the reference cuts its mosaics offline, split.py:17-46).  ``SiamUnet_diff(3, 1)`` trains on synthetic pairs for ``--n_epochs`` and
keeps a checkpoint at each third, as examples/selftrain_round_synth.py does (or three ``.pth`` files are loaded from ``--load_path``,
for instance that example's ``runs/STCD_round``); each checkpoint labels a synthetic mosaic through ``predict_scene``; ``scene_round``
turns the three stitched masks into a reliability per 256-pixel cell and a closed pseudo-label scene without leaving the device, ``export_cells`` writes the
tile set ``CD_Dataset`` reads (``A/``, ``B/``, ``pseudo_label/``, ``label/``, ``list/reliable_ids.txt``, ``list/unreliable_ids.txt``)
and the reference's score line is printed for the pseudo-label scene, followed by one line of object-level scores
(``objects.match_objects``).  ``--min_area`` / ``--max_hole`` clean the pseudo-label at object level first (``refine_round``: small
blobs cleared, small holes filled, on the device); at their default 0 the tile set and the score line are what they were without them.

    python examples/selftrain_scene_synth.py --size 1024 --cell 256 --stride 128 --window hann --close_radius 2 --min_area 64 --max_hole 32
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
from stcd_amd.objects import match_objects
from stcd_amd.selftrain import export_cells, refine_round, scene_round

parser = argparse.ArgumentParser()
parser.add_argument("--save_name", type=str, default="runs/STCD_scene_round", help="the tile set goes here")
parser.add_argument("--load_path", type=str, default="", help="directory with three .pth checkpoints (sorted by name)")
parser.add_argument("--n_epochs", type=int, default=6, help="epochs of training; a checkpoint at each third")
parser.add_argument("--train_pairs", type=int, default=64, help="128 x 128 training pairs")
parser.add_argument("--size", type=int, default=1024, help="edge of the synthetic scene, a multiple of 256")
parser.add_argument("--cell", type=int, default=256)
parser.add_argument("--tile", type=int, default=256)
parser.add_argument("--stride", type=int, default=128)
parser.add_argument("--batch_size", type=int, default=16)
parser.add_argument("--window", type=str, default="hann", choices=("flat", "hann"))
parser.add_argument("--tta", type=str, default="", choices=("", "flip", "d4"))
parser.add_argument("--close_radius", type=int, default=2, help="2 is the reference's 5 x 5 closing (train_stcd.py:186-188); 0: none")
parser.add_argument("--min_area", type=int, default=0, help="clear pseudo-label objects of fewer pixels (0: none)")
parser.add_argument("--max_hole", type=int, default=0, help="fill pseudo-label holes of at most this many pixels (0: none)")
parser.add_argument("--cumulative", action="store_true", help="the reference's never-reset metric instead of the per-cell IoU")


def train_checkpoints(args, device):
    """-> three state_dicts, after each third of the epochs (train_stcd.py:72-87 loads the 20 / 40 / 60 of 60)."""
    torch.manual_seed(1337)
    model = SiamUnet_diff(3, 1).to(device)
    optimizer = FlatAdam(model, lr=0.001, betas=(0.9, 0.999))
    a, b, label = synth.make_pairs_u8(args.train_pairs, 128, 128, 300)
    x1, x2 = torch.from_numpy(synth.normalize_nchw(a)).to(device), torch.from_numpy(synth.normalize_nchw(b)).to(device)
    target = torch.from_numpy(label).to(device).float().unsqueeze(1)
    rng = np.random.default_rng(301)
    thirds = [max(1, round(args.n_epochs * k / 3)) for k in (1, 2, 3)]
    states = []
    for epoch in range(1, args.n_epochs + 1):
        model.train()
        order = torch.from_numpy(rng.permutation(args.train_pairs)).to(device)
        for i in range(args.train_pairs // 8):
            idx = order[i * 8:(i + 1) * 8]
            optimizer.zero_grad()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(model(x1[idx], x2[idx]), target[idx])
            loss.backward()
            optimizer.step()
        print("epoch %d: loss %.4f" % (epoch, loss.item()), flush=True)
        states += [{k: v.detach().clone() for k, v in model.state_dict().items()}] * thirds.count(epoch)
    return states


def mosaic(size, seed):
    """One scene pair and its label from size / 256 squared synthetic 256-pixel pairs side by side: every part of it has its own changes."""
    n = size // 256
    a, b, label = synth.make_pairs_u8(n * n, 256, 256, seed)
    join = lambda v: np.ascontiguousarray(v.reshape((n, n, 256, 256) + v.shape[3:]).swapaxes(1, 2).reshape((size, size) + v.shape[3:]))
    return join(a), join(b), join(label)


def main(argv=None):
    args = parser.parse_args(argv)
    assert torch.cuda.is_available(), "the engine needs a GPU (no CPU fallback)"
    device = "cuda:0"
    models = []
    if args.load_path:
        paths = sorted(glob.glob(os.path.join(args.load_path, "*.pth")))
        assert len(paths) == 3, f"--load_path must hold three .pth files, found {len(paths)}"
        for p in paths:                                                         # train_stcd.py:75-87
            print("=> loading checkpoint '%s'" % p)
            m = SiamUnet_diff(3, 1)
            m.load_state_dict(torch.load(p, map_location="cpu"))
            models.append(m.to(device))
    else:
        for state in train_checkpoints(args, device):
            m = SiamUnet_diff(3, 1)
            m.load_state_dict(state)
            models.append(m.to(device))
    assert args.size >= 256 and args.size % 256 == 0, "--size is a multiple of 256"
    a, b, label = (torch.from_numpy(v).to(device) for v in mosaic(args.size, seed=303))

    t0 = time.perf_counter()
    r = scene_round(models, a, b, cell=args.cell, tile=args.tile, stride=args.stride, batch=args.batch_size, window=args.window,
                    tta=args.tta or None, close_radius=args.close_radius, label=label, cumulative=args.cumulative)
    torch.cuda.synchronize()
    listed = r.reliability[r.full]
    print("round over a %d x %d scene by %d checkpoints in %.3f s: %d cells (%d full), reliability of the full cells %.3f .. %.3f, "
          "%d reliable, %d unreliable" % (args.size, args.size, len(models), time.perf_counter() - t0, r.full.size, int(r.full.sum()),
                                          np.nanmin(listed) if listed.size else float("nan"), np.nanmax(listed) if listed.size else float("nan"),
                                          len(r.reliable), len(r.unreliable)))
    if args.min_area > 0 or args.max_hole > 0:
        before = int(torch.count_nonzero(r.pseudo))
        r = refine_round(r, min_area=args.min_area, max_hole=args.max_hole, label=label)
        print("object filter (min_area %d, max_hole %d): %d -> %d pseudo-label pixels" % (args.min_area, args.max_hole, before, int(torch.count_nonzero(r.pseudo))))
    export_cells(r, a, b, args.save_name, label=label)
    print("wrote %d cells under %s/{A,B,pseudo_label,label} and the two lists under %s/list" % (int(r.full.sum()), args.save_name, args.save_name))
    s = r.scores
    print("change predictions:  train f1 %.3f, iou: %.3f, OA %.3f, Pre: %.3f, Rec: %.3f"             # train_stcd.py:203-204
          % (s["f1"][1], s["iou"][1], s["oa"], s["precision"][1], s["recall"][1]))
    o = match_objects(r.pseudo, label)
    print("change objects:  %d predicted (%d matched), %d labelled (%d found), object f1 %.3f, Pre: %.3f, Rec: %.3f"
          % (o.n_pred, o.tp_pred, o.n_label, o.tp_label, o.f1, o.precision, o.recall))
    return r


if __name__ == "__main__":
    main()
