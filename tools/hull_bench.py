"""Convex hulls and oriented boxes on whole scenes, milliseconds per scene: objects.convex_hulls and objects.oriented_boxes against the
objects.simplify_rings and objects.object_rings they stand beside.
python tools/hull_bench.py [--size 4096] [--rounds 7] [--crop 512] [--out profiles/hull_bench.json]

The two seeded scenes of tools/simplify_bench.py, labelled once with connectivity 8 and traced with objects.object_rings:
  rects  axis-parallel rectangles plus salt, so nearly every ring has 4 vertices
  roofs  about 600 rotated rectangles and discs, whose outlines are staircases of 50 to 600 vertices
Per scene, every leg timed between two device events (the second followed by a synchronise) and the legs alternating within one process:
  c  objects.convex_hulls on the rings of the scene: both phases and the one host read between them
  b  objects.oriented_boxes(check=False) on those hulls: one launch, no host read
  s  objects.simplify_rings at tolerance 1.5 on the same rings, and
  r  objects.object_rings on the same labels: the on-device yardsticks
  h  the host route ON A --crop SQUARED CROP ONLY, by the host clock: .cpu() of the crop's rings + tests/hull_spec.hulls and
     tests/hull_spec.boxes; reported as exactly that, not extrapolated to the scene
"kernel_us" is the device time of every k_hull_* kernel per convex_hulls + oriented_boxes call, from torch.profiler (null where the
profiler reports no kernels).  "ring_lengths" and "hull_sizes" count the scene's rings by length before and after (the bins end at the
kernels' thresholds among others).  The device's hulls and boxes of the crop are compared with the specification's.  Every shape is
warmed up first; the figures are the medians of --rounds rounds, the spread is their min and max.  One JSON line, also written to --out."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import _lib, objects
from tests import hull_spec

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--crop", type=int, default=512)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hull_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")
S = a.size
TOLERANCE = 1.5


def scene_rects():
    rng = np.random.default_rng(60)                                    # tools/simplify_bench.py's scene
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


RING_BINS = [4, 8, 16, 32, objects.HULL_WAVE_MAX, 128, 256, 512, 1024, objects.HULL_LDS_MAX]
HULL_BINS = [2, 4, 8, 16, 32, objects.BOX_WAVE_MAX, 128, 256, 512, objects.BOX_LDS_MAX]


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
    rings = objects.object_rings(comp)
    hulls = objects.convex_hulls(rings)
    K = min(a.crop, S)
    crop = objects.object_rings(objects.Components(comp.labels[:K, :K].contiguous(), comp.count))

    legs = {"c": lambda: objects.convex_hulls(rings), "b": lambda: objects.oriented_boxes(hulls, check=False),
            "s": lambda: objects.simplify_rings(rings, TOLERANCE), "r": lambda: objects.object_rings(comp)}

    def leg_h():
        host = hull_spec.RingSet(*(t.cpu().numpy() for t in crop[:4]), crop.count)
        hs = hull_spec.hulls(host)
        return hs, hull_spec.boxes(hs)

    for fn in legs.values():                                           # every shape and code path once, untimed
        fn()
    want_h, want_b = leg_h()
    got_h = objects.convex_hulls(crop)
    got_b = objects.oriented_boxes(got_h)
    same = got_h.count == want_h.count and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got_h[:4], want_h[:4])) and \
        all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got_b[:4], want_b[:4]))
    ms = {k: [] for k in legs}
    host_s = []
    for r in range(a.rounds):
        for k, fn in legs.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[k].append(ev[0].elapsed_time(ev[1]))
        if r < 2:                                                      # the host route is slow and steady: two rounds
            hull_spec._box_of.cache_clear()
            t0 = time.perf_counter()
            leg_h()
            host_s.append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in ms.items()}

    kernel_us = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(a.rounds):
                legs["c"](); legs["b"]()
                torch.cuda.synchronize()
        rows = {}
        for e in prof.key_averages():
            if "k_hull_" in e.key:
                name = e.key.split("(")[0].split("::")[-1]
                total = getattr(e, "device_time_total", None)
                total = e.cuda_time_total if total is None else total
                rows[name] = [round(total / a.rounds, 2), e.count // a.rounds]
        kernel_us = rows or None
    except Exception as exc:                                           # the profiler is an observer: the figures above stand without it
        print(f"torch.profiler gave no kernel table: {exc!r}", file=sys.stderr)

    lengths = torch.diff(rings.offsets).cpu().numpy()
    sizes = torch.diff(hulls.offsets).cpu().numpy()
    R = rings.count
    return {"objects": int(comp.count), "rings": R, "vertices_before": int(rings.vertices.shape[0]), "vertices_after": int(hulls.vertices.shape[0]),
            "longest_ring": int(lengths.max()) if R else 0, "largest_hull": int(sizes.max()) if R else 0,
            "scratch_MB": round(int(_lib.lib().stcd_rings_hull_scratch_bytes(R, int(rings.vertices.shape[0]))) / 2 ** 20, 2),
            "device_equals_spec_on_crop": bool(same), "crop": K, "crop_rings": int(crop.count),
            "crop_vertices": [int(crop.vertices.shape[0]), int(want_h.vertices.shape[0])],
            "ms": {**{k: round(v, 3) for k, v in med.items()}, "h": round(statistics.median(host_s) * 1e3, 3)},
            "spread_ms": {**{k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}, "h": [round(min(host_s) * 1e3, 3), round(max(host_s) * 1e3, 3)]},
            "kernel_us": kernel_us, "c_over_s": round(med["c"] / med["s"], 3), "c_over_r": round(med["c"] / med["r"], 3),
            "ring_lengths": histogram(lengths, RING_BINS), "hull_sizes": histogram(sizes, HULL_BINS)}


result = {"tool": "hull_bench", "size": S, "connectivity": 8, "rounds": a.rounds, "simplify_tolerance": TOLERANCE,
          "legs": {"c": "convex_hulls: count phase, one host read, write phase", "b": "oriented_boxes(check=False) on the hulls",
                   "s": f"simplify_rings at {TOLERANCE} on the same rings", "r": "object_rings on the same labels",
                   "h": f".cpu() + tests/hull_spec.hulls and boxes on the rings of the {min(a.crop, S)} x {min(a.crop, S)} crop only, host clock (not extrapolated)"},
          "scenes": {"rects": measure(scene_rects()), "roofs": measure(scene_roofs())}}
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
