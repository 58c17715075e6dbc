"""Ring rasterization on whole scenes, milliseconds per scene: objects.rasterize_rings against what it sits beside.
python tools/raster_bench.py [--size 4096] [--tolerance 1.5] [--rounds 9] [--crop 512] [--out profiles/raster_bench.json]

The two seeded scenes of tools/simplify_bench.py, labelled once with connectivity 8 and traced with objects.object_rings:
  rects  axis-parallel rectangles plus salt, so nearly every ring has 4 vertices and nearly every edge spans few rows
  roofs  about 600 rotated rectangles and discs, whose outlines are staircases of 50 to 600 vertices
Per scene, the legs alternating within one process, each between two device events with a synchronise after it:
  t  objects.rasterize_rings(check=False) of the traced rings (every edge of a staircase is one row or one column)
  s  objects.rasterize_rings(check=False) of the rings simplified at --tolerance (few edges, slanted, tens of rows each)
  o  leg s with the scene's mask (as 0 / 1) as overlay: the confusion counts in the same pass
  r  objects.object_rings on the same labels (both phases and its host read): the on-device yardstick of the chain
  c  selftrain.mask_close on the scene's mask: a one-launch pass over the same pixels
  f  the floor the same bytes cost with torch ops alone: zero_() of an int32 [H, W + 1] tensor, then a uint8 [H,W] written from it
     by one converting copy
"kernel_us" is the device time of every k_raster_* kernel per rasterize_rings call of legs t and s, from torch.profiler (null where
the profiler reports no kernels).  The host route runs ON A --crop SQUARED CROP ONLY and is reported as exactly that, not extrapolated
to the scene: .cpu() of the crop's simplified rings + tests/raster_spec.fill, and PIL's ImageDraw.polygon where PIL imports (PIL samples
differently: its pixels are not compared).  Every shape is warmed up first; the figures are the medians of --rounds rounds, the spread
is their min and max.  One JSON line, also written to --out."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import objects, selftrain
from tests import raster_spec

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--tolerance", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=9); ap.add_argument("--crop", type=int, default=512)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "raster_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")
S = a.size


def scene_rects():
    rng = np.random.default_rng(60)                                    # tools/rings_bench.py's scene
    m = np.zeros((S, S), np.uint8)
    for _ in range(600):
        h, w = rng.integers(8, 97, 2)
        y, x = rng.integers(0, max(S - h, 1)), rng.integers(0, max(S - w, 1))
        m[y:y + h, x:x + w] = 255
        if h >= 24 and w >= 24 and rng.random() < 0.3:
            c = int(rng.integers(2, 7))
            m[y + h // 2 - c // 2:y + h // 2 + c - c // 2, x + w // 2 - c // 2:x + w // 2 + c - c // 2] = 0
    m[rng.random((S, S)) < 0.002] = 255
    return m


def scene_roofs():
    rng = np.random.default_rng(61)                                    # tools/simplify_bench.py's scene
    m = np.zeros((S, S), np.uint8)
    for k in range(600):
        cy, cx = (int(v) for v in rng.integers(0, S, 2))
        if k % 3 == 2:                                                 # a disc
            r = int(rng.integers(8, 61))
            y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, S), max(cx - r, 0), min(cx + r + 1, S)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            m[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
        else:                                                          # a rectangle along the integer direction (dy, dx)
            dy, dx = int(rng.integers(-7, 8)), int(rng.integers(1, 8))
            ha, hb = int(rng.integers(10, 81)), int(rng.integers(6, 41))
            r = ha + hb
            y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, S), max(cx - r, 0), min(cx + r + 1, S)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            d2 = dy * dy + dx * dx
            u, v = (yy - cy) * dy + (xx - cx) * dx, (yy - cy) * dx - (xx - cx) * dy
            m[y0:y1, x0:x1][(u * u <= ha * ha * d2) & (v * v <= hb * hb * d2)] = 255
    return m


def spans(rings, H):
    """The clipped row span of every edge that is not horizontal, on the host."""
    v, o = rings.vertices.cpu().numpy().astype(np.int64), rings.offsets.cpu().numpy()
    nxt = np.arange(1, v.shape[0] + 1)
    nxt[o[1:][np.diff(o) > 0] - 1] = o[:-1][np.diff(o) > 0]
    y0, y1 = np.minimum(v[:, 0], v[nxt, 0]), np.maximum(v[:, 0], v[nxt, 0])
    d = np.minimum(y1, H) - y0
    return d[d > 0]


def histogram(values, bins):
    values = np.asarray(values, np.int64)
    out, lo = {}, 0
    for hi in bins:
        out[f"{lo + 1}-{hi}"] = int(((values > lo) & (values <= hi)).sum())
        lo = hi
    out[f">{lo}"] = int((values > lo).sum())
    return out


def measure(mask):
    M = torch.from_numpy(mask).to(dev)
    comp = objects.label_components(M)
    traced = objects.object_rings(comp)
    simple = objects.simplify_rings(traced, a.tolerance)
    shape = (S, S)
    overlay = (M != 0).to(torch.uint8)                                 # 0 / 1: a byte of 255 would be ignored
    plane = torch.empty((S, S + 1), dtype=torch.int32, device=dev)
    floor_mask = torch.empty(shape, dtype=torch.uint8, device=dev)

    def leg_f():
        plane.zero_()
        floor_mask.copy_(plane[:, :S])

    legs = {"t": lambda: objects.rasterize_rings(traced, shape, check=False), "s": lambda: objects.rasterize_rings(simple, shape, check=False),
            "o": lambda: objects.rasterize_rings(simple, shape, overlay=overlay, check=False), "r": lambda: objects.object_rings(comp),
            "c": lambda: selftrain.mask_close(M), "f": leg_f}
    first = {k: fn() for k, fn in legs.items()}                        # every shape and code path once, untimed
    torch.cuda.synchronize()
    exact = bool(torch.equal(first["t"].mask, (comp.labels > 0).to(torch.uint8) * 255))
    cm = first["o"].cm.cpu().numpy()
    ms = {k: [] for k in legs}
    for r in range(a.rounds):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}

    kernel_us = None
    try:
        from torch.profiler import ProfilerActivity, profile
        kernel_us = {}
        for k in ("t", "s"):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(a.rounds):
                    legs[k]()
                torch.cuda.synchronize()
            rows = {}
            for e in prof.key_averages():
                if "k_raster_" in e.key:
                    name = e.key.split("(")[0].split("<")[0].split("::")[-1]
                    total = getattr(e, "device_time_total", None)
                    total = e.cuda_time_total if total is None else total
                    rows[name] = round(total / a.rounds, 2)
            kernel_us[k] = rows or None
    except Exception as exc:                                           # the profiler is an observer: the figures above stand without it
        print(f"torch.profiler gave no kernel table: {exc!r}", file=sys.stderr)

    # the host route, on the crop only
    K = min(a.crop, S)
    crop = objects.simplify_rings(objects.object_rings(objects.Components(comp.labels[:K, :K].contiguous(), comp.count)), a.tolerance)
    want = objects.rasterize_rings(crop, (K, K)).mask.cpu().numpy()
    host = {}
    t0 = time.perf_counter()
    ring_list = raster_spec.ring_list(raster_spec_ringset(crop))
    got = raster_spec.fill(ring_list, K, K)
    host["spec_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    same = bool(np.array_equal(got.astype(np.uint8) * np.uint8(255), want))
    try:
        from PIL import Image, ImageDraw
        t0 = time.perf_counter()
        v, o, area2 = crop.vertices.cpu().numpy(), crop.offsets.cpu().numpy(), crop.area2.cpu().numpy()
        img = Image.new("L", (K, K), 0)
        draw = ImageDraw.Draw(img)
        for want_outer in (True, False):                               # outer rings first, then the holes over them
            for r in range(crop.count):
                if (area2[r] > 0) == want_outer and o[r + 1] - o[r] >= 3:
                    draw.polygon([(int(x), int(y)) for y, x in v[o[r]:o[r + 1]]], fill=255 if want_outer else 0)
        pil = np.asarray(img)
        host["pil_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        host["pil_pixels_set"] = int((pil > 0).sum())
    except ImportError:
        host["pil_ms"] = None
    return {"objects": int(comp.count), "rings": int(traced.count), "vertices_traced": int(traced.vertices.shape[0]),
            "vertices_simplified": int(simple.vertices.shape[0]), "traced_raster_equals_labels": exact,
            "simplified_vs_mask": {"cm": cm.tolist(), "pixels_differ": int(cm[0, 1] + cm[1, 0]), "object_pixels": int(cm[1].sum())},
            "edge_spans_traced": histogram(spans(traced, S), [1, 4, objects.RASTER_SPAN_MAX, 64, 256]),
            "edge_spans_simplified": histogram(spans(simple, S), [1, 4, objects.RASTER_SPAN_MAX, 64, 256]),
            "scratch_MB": round(16 / 2 ** 20 + 4 * S * (S + 1) / 2 ** 20, 2),
            "ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "kernel_us": kernel_us,
            "t_over_f": round(med["t"] / med["f"], 3), "s_over_f": round(med["s"] / med["f"], 3),
            "t_over_r": round(med["t"] / med["r"], 3), "s_over_r": round(med["s"] / med["r"], 3), "t_over_c": round(med["t"] / med["c"], 3),
            "host_on_crop": {"crop": K, "rings": int(crop.count), "vertices": int(crop.vertices.shape[0]), "device_equals_spec": same, **host}}


def raster_spec_ringset(rings):
    from tests.rings_spec import RingSet
    return RingSet(*(t.cpu().numpy() for t in rings[:4]), rings.count)


result = {"tool": "raster_bench", "size": S, "tolerance": a.tolerance, "connectivity": 8, "rounds": a.rounds,
          "legs": {"t": "rasterize_rings(check=False) of the traced rings", "s": "rasterize_rings(check=False) of the simplified rings",
                   "o": "leg s with the mask as overlay (confusion counts)", "r": "object_rings on the same labels", "c": "mask_close on the mask",
                   "f": "floor: zero_() of int32 [H, W + 1] + one converting copy into uint8 [H,W]"},
          "scenes": {"rects": measure(scene_rects()), "roofs": measure(scene_roofs())}}
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
