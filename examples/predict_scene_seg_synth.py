#!/usr/bin/env python3
"""Whole-scene inference for the models the reference's scripts train: SegCD's three maps over a scene pair, and the single-image
UnetSeg that shares its checkpoint over one scene.

``SegCD`` (train_pse_cd.py:426, train_stcd.py:638) returns ``(mask_t1, mask_t2, change)``; ``stcd_amd.scene.predict_scene_heads``
stitches all three and applies the decision-level gate sketched at train_stcd.py:170-176, ``change & (seg_a != seg_b)``.
``UnetSeg`` (train_sup.py:303) is pre-trained on single images and its ``state_dict`` is what SegCD starts from;
``stcd_amd.scene.predict_scene_seg`` runs it over one scene.  The pair is synthetic: rectangle "buildings" on a textured ground, the
building labels are the rectangles per date and the change label is their symmetric difference.  With ``--load_path`` the weights of
a trained SegCD are used, otherwise the scores are those of a randomly initialised network and only show the plumbing.

    python examples/predict_scene_seg_synth.py --size 1024 --tile 256 --stride 128 --window hann
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from stcd_amd.scene import plan_tiles, predict_scene_heads, predict_scene_seg
from stcd_amd.segcd import SegCD, UnetSeg

parser = argparse.ArgumentParser()
parser.add_argument("--size", type=int, default=1024, help="scene edge in pixels (LEVIR-CD scenes are 1024 x 1024)")
parser.add_argument("--tile", type=int, default=256, help="a multiple of 32 (SegCD)")
parser.add_argument("--stride", type=int, default=128, help="<= tile; tile = no overlap")
parser.add_argument("--batch", type=int, default=16)
parser.add_argument("--window", type=str, default="hann", choices=("flat", "hann"))
parser.add_argument("--tta", type=str, default="none", choices=("none", "flip", "d4"))
parser.add_argument("--encoder", type=str, default="resnet18")
parser.add_argument("--load_path", type=str, default="", help="state_dict of a trained SegCD(encoder)")
parser.add_argument("--seed", type=int, default=7)


def make_buildings(size, seed):
    """Two uint8 [size,size,3] scenes and uint8 [size,size] building labels: rectangles on noise; a third of them stand in A only, a
    third in B only, a third in both."""
    rng = np.random.default_rng(seed)
    ground = rng.integers(60, 120, size=(size, size, 3), dtype=np.uint8)
    scenes = [ground.copy(), np.clip(ground.astype(np.int16) + rng.integers(-8, 9, size=(size, size, 3)), 0, 255).astype(np.uint8)]
    labels = [np.zeros((size, size), np.uint8), np.zeros((size, size), np.uint8)]
    for k in range(max(3, size * size // 16384)):
        h, w = (int(v) for v in rng.integers(size // 64 + 4, size // 16 + 8, size=2))
        y, x = int(rng.integers(0, size - h)), int(rng.integers(0, size - w))
        colour = rng.integers(150, 256, size=3, dtype=np.uint8)
        for date in ((0,), (1,), (0, 1))[k % 3]:
            scenes[date][y:y + h, x:x + w] = colour
            labels[date][y:y + h, x:x + w] = 1
    return scenes[0], scenes[1], labels[0], labels[1]


def score_line(name, s):
    return f"{name:7s} OA {s['oa']:.4f}  precision {s['precision'][1]:.4f}  recall {s['recall'][1]:.4f}  F1 {s['f1'][1]:.4f}  IoU {s['iou'][1]:.4f}"


def main(argv=None):
    args = parser.parse_args(argv)
    assert torch.cuda.is_available(), "the engine needs a GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    a, b, lab_a, lab_b = make_buildings(args.size, args.seed)
    lab_c = lab_a ^ lab_b                                             # change: a building in one date only
    scene_a, scene_b, lab_a, lab_b, lab_c = (torch.from_numpy(v).to(dev) for v in (a, b, lab_a, lab_b, lab_c))

    torch.manual_seed(args.seed)
    segcd = SegCD(encoder_name=args.encoder)
    if args.load_path:
        segcd.load_state_dict(torch.load(args.load_path, map_location="cpu"))
    unet = UnetSeg(encoder_name=args.encoder)
    unet.load_state_dict(segcd.state_dict())                          # the same state_dict: a supervised checkpoint loads both ways
    segcd.to(dev)
    unet.to(dev)

    plan = plan_tiles(args.size, args.size, args.tile, args.stride)
    kw = dict(tile=args.tile, stride=args.stride, batch=args.batch, window=args.window, tta=None if args.tta == "none" else args.tta)
    t0 = time.perf_counter()
    res = predict_scene_heads(segcd, scene_a, scene_b, label=lab_c, label_a=lab_a, label_b=lab_b, return_prob=True, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{args.size} x {args.size} pair, {plan.tiles_y} x {plan.tiles_x} tiles of {plan.tile} at stride {plan.stride} ({args.window}, tta {args.tta}), "
          f"SegCD({args.encoder}): {dt * 1e3:.1f} ms including the first-call set-up")
    print(f"pixels set: seg_a {int(res.seg_a.sum())}  seg_b {int(res.seg_b.sum())}  change {int(res.change.sum())}  gated {int(res.gated.sum())}; "
          f"labelled: a {int(lab_a.sum())}  b {int(lab_b.sum())}  change {int(lab_c.sum())}")
    for key in ("seg_a", "seg_b", "change", "gated"):
        print(score_line(key, res.scores[key]))
    one = predict_scene_seg(unet, scene_a, label=lab_a, **kw)
    print(score_line("unetseg", one.scores) + f"   (scene A alone; differs from seg_a in {int((one.mask != res.seg_a).sum())} pixels)")
    return res, one


if __name__ == "__main__":
    main()
