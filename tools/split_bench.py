"""The nearest-seed transform, label growth and the object split on whole scenes, milliseconds per scene.
python tools/split_bench.py [--size 4096] [--rounds 9] [--crop 512] [--radius 6] [--out profiles/split_bench.json]

Two scenes, the seeded ones of tools/edt_bench.py and tools/simplify_bench.py (rects: axis-parallel rectangles plus salt; roofs:
about 600 rotated rectangles and discs, many of which touch).  Per scene, the legs alternating within one process, each between two
device events with a synchronise after it:
  n   distance.nearest_seed(to="set"): the index plane alone
  nd  distance.nearest_seed(to="set", return_distance=True): index and d2
  e   distance.expand_labels(components, 3): the seed bytes, one transform, the gather in its epilogue
  x   objects.split_objects(radius, check=False): erosion, two labellings (with their host reads), the transform, the cut
  s   distance.squared_distance(to="set") on the same mask: the yardstick of n
  l   objects.label_components + objects.object_table on the same mask: the yardstick of x
"n_over_s" is the figure to watch: the index variant writes 4 (nd: 8) bytes per pixel where s writes 4.  "kernel_us" is the device
time of every k_edt_* and k_split_* kernel per call of legs n, nd, e, x and s, from torch.profiler (null where the profiler reports
no kernels).  The host route runs ON A --crop SQUARED CROP ONLY and is reported as exactly that, not extrapolated to the scene:
.cpu() of the crop + scipy.ndimage.distance_transform_edt(return_indices=True); its distances must equal the device's, its indices
may differ where seeds tie (scipy has another tie rule), so the count of differing pixels is reported and each of them is checked
to be a tie.  Every shape is warmed up first; the figures are the medians of --rounds rounds, the spread is their min and max.  One
JSON line, also written to --out."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import distance, objects

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--crop", type=int, default=512); ap.add_argument("--radius", type=float, default=6.0)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "split_bench.json"))
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


def host_route(crop):
    """scipy's feature transform of the crop against the device's: equal distances, and indices that differ only between ties."""
    from scipy import ndimage
    K = crop.shape[0]
    index, d2 = (t.cpu().numpy().astype(np.int64) for t in distance.nearest_seed(crop, return_distance=True))
    seed = crop.cpu().numpy() != 0
    if not seed.any():
        return {"crop": K, "scipy_ms": None, "device_d2_equals_scipy": bool((index == -1).all()), "index_differs": 0, "all_ties": True}
    t0 = time.perf_counter()
    idx = ndimage.distance_transform_edt(~seed, return_distances=False, return_indices=True).astype(np.int64)
    ms = (time.perf_counter() - t0) * 1e3
    ii, jj = np.indices(seed.shape)
    theirs = (idx[0] - ii) ** 2 + (idx[1] - jj) ** 2
    differs = idx[0] * K + idx[1] != index
    return {"crop": K, "scipy_ms": round(ms, 1), "device_d2_equals_scipy": bool(np.array_equal(theirs, d2)), "index_differs": int(differs.sum()),
            "all_ties": bool(seed.reshape(-1)[index].all() and np.array_equal((index // K - ii) ** 2 + (index % K - jj) ** 2, d2))}


def measure(mask):
    M = torch.from_numpy(mask).to(dev)
    comps = objects.label_components(M)

    def leg_l():
        return objects.object_table(objects.label_components(M))

    legs = {"n": lambda: distance.nearest_seed(M), "nd": lambda: distance.nearest_seed(M, return_distance=True),
            "e": lambda: distance.expand_labels(comps, 3), "x": lambda: objects.split_objects(M, a.radius, check=False),
            "s": lambda: distance.squared_distance(M, to="set"), "l": leg_l}
    first = {k: fn() for k, fn in legs.items()}                        # every shape and code path once, untimed
    torch.cuda.synchronize()
    split = objects.split_objects(M, a.radius)
    facts = {"set_pixels": int((M != 0).sum()), "objects": comps.count, "cores": split.n_cores, "cut_pixels": split.cut_pixels,
             "orphan_pixels": split.orphan_pixels, "objects_after_split": objects.label_components(split.mask).count,
             "d2_of_nd_equals_s": bool(torch.equal(first["nd"][1], first["s"])), "index_of_nd_equals_n": bool(torch.equal(first["nd"][0], first["n"])),
             "pixels_grown_by_3": int((first["e"] != 0).sum()) - int((M != 0).sum())}
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
        for k in ("n", "nd", "e", "x", "s"):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(a.rounds):
                    legs[k]()
                torch.cuda.synchronize()
            rows = {}
            for e in prof.key_averages():
                if "k_edt_" in e.key or "k_split_" in e.key:
                    name = e.key.split("(")[0].split("<")[0].split("::")[-1]
                    total = getattr(e, "device_time_total", None)
                    total = e.cuda_time_total if total is None else total
                    rows[name] = round(rows.get(name, 0.0) + total / a.rounds, 2)
            kernel_us[k] = rows or None
    except Exception as exc:                                           # the profiler is an observer: the figures above stand without it
        print(f"torch.profiler gave no kernel table: {exc!r}", file=sys.stderr)

    K = min(a.crop, S)
    return {"facts": facts, "ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "kernel_us": kernel_us, "n_over_s": round(med["n"] / med["s"], 3), "nd_over_s": round(med["nd"] / med["s"], 3),
            "e_over_s": round(med["e"] / med["s"], 3), "x_over_l": round(med["x"] / med["l"], 3), "host_on_crop": host_route(M[:K, :K].contiguous())}


result = {"tool": "split_bench", "size": S, "rounds": a.rounds, "radius": a.radius,
          "legs": {"n": "nearest_seed(to='set')", "nd": "nearest_seed(to='set', return_distance=True)", "e": "expand_labels(components, 3)",
                   "x": f"split_objects({a.radius}, check=False)", "s": "squared_distance(to='set')", "l": "label_components + object_table"},
          "scenes": {"rects": measure(scene_rects()), "roofs": measure(scene_roofs())}}
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
