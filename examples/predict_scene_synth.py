#!/usr/bin/env python3
"""Whole-scene inference on the HIP engine: two co-registered uint8 scenes in, one change mask and its scores out.

The reference crops its scenes into 256-pixel tiles offline (/root/reference/split.py:17-46) and its test-time evaluator
(models/evaluator.py) does not run; ``stcd_amd.scene.predict_scene`` tiles, normalises, predicts and stitches on the device.
The scene is synthetic (stcd_amd.synth); with ``--load_path`` the weights of a trained ``SiamUnet_diff`` are used, otherwise the
scores are those of a randomly initialised network and only show the plumbing.

    python examples/predict_scene_synth.py --size 1024 --tile 256 --stride 128 --window hann --tta d4
    python examples/predict_scene_synth.py --touching 40 --split 8 --vector buildings.geojson --boxes boxes.geojson
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from stcd_amd import synth
from stcd_amd.modules import SiamUnet_diff
from stcd_amd.scene import plan_tiles, predict_scene

parser = argparse.ArgumentParser()
parser.add_argument("--size", type=int, default=1024, help="scene edge in pixels (LEVIR-CD scenes are 1024 x 1024)")
parser.add_argument("--tile", type=int, default=256)
parser.add_argument("--stride", type=int, default=128, help="<= tile; tile = no overlap")
parser.add_argument("--batch", type=int, default=16)
parser.add_argument("--window", type=str, default="hann", choices=("flat", "hann"))
parser.add_argument("--tta", type=str, default="none", choices=("none", "flip", "d4"),
                    help="test-time augmentation: average the 4 mirror views or all 8 symmetries of the square")
parser.add_argument("--load_path", type=str, default="", help="state_dict of a trained SiamUnet_diff(3, 2)")
parser.add_argument("--seed", type=int, default=7)
parser.add_argument("--vector", type=str, default="", metavar="OUT.geojson",
                    help="also write the predicted change objects as GeoJSON polygons (pixel coordinates)")
parser.add_argument("--min_area", type=int, default=4, help="with --vector: objects below this many pixels are dropped")
parser.add_argument("--max_hole", type=int, default=4, help="with --vector: holes of at most this many pixels are filled")
parser.add_argument("--simplify", type=float, default=None, metavar="TOL",
                    help="with --vector: simplify the outlines with this tolerance in pixels (objects.simplify_rings), e.g. 1.5; "
                         "the polygons are then rasterized again (objects.rasterize_rings) and scored against the mask they came from")
parser.add_argument("--topology", action="store_true",
                    help="with --vector ... --simplify: repair the simplified outlines' topology (objects.simplify_rings_safe): no two edges "
                         "cross and no object ends up inside another's polygon; prints the rounds, the restored vertices and what plain "
                         "Douglas-Peucker leaves")
parser.add_argument("--boxes", type=str, default="", metavar="OUT.geojson",
                    help="with --vector: also write every object's minimum-area rectangle (objects.convex_hulls + oriented_boxes on the traced "
                         "outlines, not the simplified ones) with its angle, width, height, rectangularity and solidity")
parser.add_argument("--boundary", type=float, default=None, metavar="T",
                    help="also print boundary precision, recall and F1 at T pixels and the Hausdorff distance of the prediction against the "
                         "label (distance.boundary_scores); with --vector ... --simplify the same scores of the simplified polygons' raster "
                         "against the mask they came from")
parser.add_argument("--split", type=float, default=None, metavar="R",
                    help="with --vector: split objects that touch before they are labelled (objects.split_objects): the mask is eroded by "
                         "a disc of R pixels to cores, every pixel goes to its nearest core and a cut is made where two owners meet, so "
                         "that --vector and --boxes write one polygon and one rectangle per building")
parser.add_argument("--min_core", type=int, default=0, metavar="A", help="with --split: cores of fewer than A pixels are dropped")
parser.add_argument("--touching", type=int, default=0, metavar="N",
                    help="with --vector: vectorise a synthetic mask of N rectangles that touch their neighbours instead of the prediction "
                         "(an untrained network predicts no buildings): what --split is for")
parser.add_argument("--vector_label", type=str, default="", metavar="IN.geojson",
                    help="read the label from GeoJSON polygons in pixel coordinates (objects.geojson_to_rings + rasterize_rings) instead of the synthetic one")


def print_boundary(what, scores, tolerance):
    h2 = scores.hausdorff2
    hd = "undefined (one boundary is empty)" if h2 >= 2 ** 30 else f"{h2 ** 0.5:.2f} px"
    print(f"{what}: boundary precision {scores.precision[0]:.4f}  recall {scores.recall[0]:.4f}  F1 {scores.f1[0]:.4f} at {tolerance} px "
          f"({scores.n_pred} / {scores.n_label} boundary pixels); Hausdorff distance {hd}")


def touching_rectangles(size, n, dev):
    """uint8 [size,size] on the device: n rectangles in rows, each overlapping the next by a few pixels at a corner."""
    m = np.zeros((size, size), np.uint8)
    h, w, y, x = 40, 56, 8, 8
    for k in range(n):
        if x + w > size - 8:
            y, x = y + h + 42, 8
        if y + h + 30 > size:
            break
        dy = 30 * (k % 2)                                       # every second one lower: they share 10 rows
        m[y + dy:y + dy + h, x:x + w] = 255
        x += w - 5                                              # the next one starts 5 columns inside this one
    return torch.from_numpy(m).to(dev)


def main(argv=None):
    args = parser.parse_args(argv)
    if args.boxes and not args.vector:
        parser.error("--boxes needs --vector")
    if (args.split is not None or args.touching) and not args.vector:
        parser.error("--split and --touching need --vector")
    if args.topology and not (args.vector and args.simplify is not None):
        parser.error("--topology needs --vector and --simplify")
    assert torch.cuda.is_available(), "the engine needs a GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    a, b, label = synth.make_pairs_u8(1, args.size, args.size, args.seed)          # uint8 [1,H,W,3] x 2, uint8 [1,H,W] in {0,1}
    scene_a, scene_b, label = (torch.from_numpy(v[0]).to(dev) for v in (a, b, label))

    torch.manual_seed(args.seed)
    model = SiamUnet_diff(3, 2)
    if args.load_path:
        model.load_state_dict(torch.load(args.load_path, map_location="cpu"))
    model.to(dev)

    if args.vector_label:
        # vector ground truth: the polygons (pixel coordinates) rasterized on the device replace the synthetic label
        from stcd_amd import objects
        truth = objects.geojson_to_rings(args.vector_label, device=dev)
        label = objects.rasterize_rings(truth, (args.size, args.size), mask_value=1).mask
        print(f"label from {args.vector_label}: {truth.count} rings, {int(truth.vertices.shape[0])} vertices, {int(label.sum())} labelled pixels")

    plan = plan_tiles(args.size, args.size, args.tile, args.stride)
    t0 = time.perf_counter()
    res = predict_scene(model, scene_a, scene_b, tile=args.tile, stride=args.stride, batch=args.batch, window=args.window,
                        label=label, return_prob=True, tta=None if args.tta == "none" else args.tta)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s = res.scores
    print(f"{args.size} x {args.size} scene, {plan.tiles_y} x {plan.tiles_x} tiles of {plan.tile} at stride {plan.stride} ({args.window}, tta {args.tta}): "
          f"{dt * 1e3:.1f} ms including the first-call set-up")
    print(f"change pixels predicted {int(res.mask.sum())} / labelled {int((label >= 1).sum())}; mean change probability {float(res.prob.mean()):.4f}")
    print(f"confusion matrix [label, pred]: {res.cm.tolist()}")
    print(f"OA {s['oa']:.4f}  precision {s['precision'][1]:.4f}  recall {s['recall'][1]:.4f}  F1 {s['f1'][1]:.4f}  IoU {s['iou'][1]:.4f}")
    if args.boundary is not None:
        from stcd_amd import distance
        print_boundary("prediction against the label", distance.boundary_scores(res.mask.contiguous(), label.contiguous(), (args.boundary,)), args.boundary)
    if args.vector:
        # the mask as vector data: small objects and small holes removed, the rest numbered, outlined and written as polygons
        from stcd_amd import objects
        source = touching_rectangles(args.size, args.touching, dev) if args.touching else res.mask.contiguous()
        clean = objects.filter_objects(source, args.min_area, args.max_hole)
        if args.split is not None:
            # neighbours that touch are one component: cut them apart where the nearest cores change
            before = objects.label_components(clean).count
            split = objects.split_objects(clean, args.split, min_core_area=args.min_core)
            clean = split.mask
            print(f"split at {args.split} px: {split.n_cores} cores, {split.cut_pixels} pixels cut, {split.orphan_pixels} orphan pixels; "
                  f"{before} objects before, {objects.label_components(clean).count} after")
        comp = objects.label_components(clean)
        rings = objects.object_rings(comp)
        traced = int(rings.vertices.shape[0])
        if args.boxes:
            # footprint rectangles: the hull and the minimum-area rectangle of every traced ring, on the device
            hulls = objects.convex_hulls(rings)
            boxes = objects.oriented_boxes(hulls)
            shape = objects.box_shape(boxes, rings, hulls)
            doc = objects.boxes_to_geojson(boxes, rings, path=args.boxes, properties=shape)
            outer = (rings.area2 > 0).cpu().numpy()
            print(f"{len(doc['features'])} rectangles written to {args.boxes}: {int(hulls.vertices.shape[0])} hull vertices of {traced}; "
                  f"median rectangularity {float(np.median(shape['rectangularity'][outer])) if outer.any() else float('nan'):.3f}, "
                  f"median solidity {float(np.median(shape['solidity'][outer])) if outer.any() else float('nan'):.3f}")
        if args.simplify is not None:
            if args.topology:
                plain = objects.simplify_rings(rings, tolerance=args.simplify)
                safe = objects.simplify_rings_safe(rings, tolerance=args.simplify)
                rings = safe.rings
                print(f"simplified at {args.simplify} px with the topology repaired: {traced} vertices before, {int(rings.vertices.shape[0])} after, "
                      f"{safe.restored} of them restored in {safe.rounds} rounds, {safe.conflicts} conflicting edges left; plain Douglas-Peucker "
                      f"keeps {int(plain.vertices.shape[0])} vertices and leaves {objects.ring_conflicts(plain).count} conflicting edges")
            else:
                rings = objects.simplify_rings(rings, tolerance=args.simplify)
                print(f"simplified at {args.simplify} px (Douglas-Peucker on the device): {traced} vertices before, {int(rings.vertices.shape[0])} after")
            # what the tolerance cost in pixels: the polygons rasterized again, with the mask they came from as overlay
            from stcd_amd.metrics import scores_from_cm
            cm = objects.rasterize_rings(rings, clean.shape, overlay=(clean != 0).to(torch.uint8)).cm.cpu().numpy()      # 0 / 1: an overlay byte of 255 is ignored
            fid = scores_from_cm(cm)
            print(f"polygons against their mask: {int(cm[0, 1] + cm[1, 0])} pixels differ, IoU {fid['iou'][1]:.4f}, F1 {fid['f1'][1]:.4f}")
            if args.boundary is not None:                       # the same cost in the tolerance's own unit: the distance between the outlines
                from stcd_amd import distance
                raster = objects.rasterize_rings(rings, clean.shape, mask_value=1).mask
                print_boundary("polygons against their mask", distance.boundary_scores(raster, (clean != 0).to(torch.uint8), (args.boundary,)), args.boundary)
        doc = objects.rings_to_geojson(rings, path=args.vector, properties=objects.object_table(comp))
        print(f"{len(doc['features'])} polygons ({rings.count} rings, {int(rings.vertices.shape[0])} vertices) written to {args.vector}")
    return res


if __name__ == "__main__":
    main()
