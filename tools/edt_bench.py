"""The distance transform on whole scenes, milliseconds per scene: stcd_amd/distance.py against what it sits beside.
python tools/edt_bench.py [--size 4096] [--rounds 9] [--crop 512] [--out profiles/edt_bench.json]

Four scenes: the two seeded scenes of tools/simplify_bench.py (rects: axis-parallel rectangles plus salt; roofs: about 600 rotated
rectangles and discs), a mask with a single set pixel and an empty one.  The last two are there to show that the time does not
depend on the data: the row pass bounds its work by the width, not by the distances it finds.
Per scene, the legs alternating within one process, each between two device events with a synchronise after it:
  u   distance.squared_distance(to="unset")
  s   distance.squared_distance(to="set")
  b2  distance.buffer_mask(radius 2, "close"): two transforms, two thresholds
  c2  selftrain.mask_close(radius 2): the one-launch square window it sits beside (5 x 5, not a disc: the pixels differ)
  b12 distance.buffer_mask(radius 12, "close"): a radius no square-window launch takes; the same cost as b2
  m   distance.boundary_scores(pred, label, (2.0,), check=False): two transforms and the counts, no host read; pred is the scene,
      label the scene rolled by (3, 4)
  l   objects.label_components + objects.object_table on the same mask: the on-device yardstick of the chain (with its host read)
"kernel_us" is the device time of every k_edt_* kernel per call of legs u, s and m, from torch.profiler (null where the profiler
reports no kernels), and "row_bytes" what the row pass of leg s moves (g read, d2 written) with the rate that kernel time gives.
The host route runs ON A --crop SQUARED CROP ONLY and is reported as exactly that, not extrapolated to the scene: .cpu() of the crop +
scipy.ndimage.distance_transform_edt (its indices turned into integer squared distances, which must equal the device's).
Every shape is warmed up first; the figures are the medians of --rounds rounds, the spread is their min and max.  One JSON line,
also written to --out."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import distance, objects, selftrain

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--crop", type=int, default=512)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "edt_bench.json"))
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


def scene_single():
    m = np.zeros((S, S), np.uint8)
    m[S // 3, (2 * S) // 3] = 255
    return m


def scene_empty():
    return np.zeros((S, S), np.uint8)


def scipy_d2(seed):
    from scipy import ndimage
    if not seed.any():
        return np.full(seed.shape, distance.NO_SEED, np.int64)
    idx = ndimage.distance_transform_edt(~seed, return_distances=False, return_indices=True).astype(np.int64)
    ii, jj = np.indices(seed.shape)
    return (idx[0] - ii) ** 2 + (idx[1] - jj) ** 2


def measure(mask):
    M = torch.from_numpy(mask).to(dev)
    label = torch.roll((M != 0).to(torch.uint8), (3, 4), (0, 1)).contiguous()      # 0 / 1: a byte of 255 would be void

    def leg_l():
        return objects.object_table(objects.label_components(M))

    legs = {"u": lambda: distance.squared_distance(M, to="unset"), "s": lambda: distance.squared_distance(M, to="set"),
            "b2": lambda: distance.buffer_mask(M, 2, op="close"), "c2": lambda: selftrain.mask_close(M, 2),
            "b12": lambda: distance.buffer_mask(M, 12, op="close"), "m": lambda: distance.boundary_scores(M, label, (2.0,), check=False),
            "l": leg_l}
    first = {k: fn() for k, fn in legs.items()}                        # every shape and code path once, untimed
    torch.cuda.synchronize()
    scores = distance.boundary_scores(M, label, (2.0,))
    closed = {"set_pixels": int((M != 0).sum()), "disc2_close": int((first["b2"] != 0).sum()), "square2_close": int((first["c2"] != 0).sum()),
              "disc12_close": int((first["b12"] != 0).sum())}
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
        for k in ("u", "s", "m"):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(a.rounds):
                    legs[k]()
                torch.cuda.synchronize()
            rows = {}
            for e in prof.key_averages():
                if "k_edt_" in e.key:
                    name = e.key.split("(")[0].split("<")[0].split("::")[-1]
                    total = getattr(e, "device_time_total", None)
                    total = e.cuda_time_total if total is None else total
                    rows[name] = round(rows.get(name, 0.0) + total / a.rounds, 2)
            kernel_us[k] = rows or None
    except Exception as exc:                                           # the profiler is an observer: the figures above stand without it
        print(f"torch.profiler gave no kernel table: {exc!r}", file=sys.stderr)
    row_bytes = 2 * S * ((S + 3) // 4 * 4) + 4 * S * S                 # g read as uint16, d2 written as int32
    row_us = (kernel_us or {}).get("s") and kernel_us["s"].get("k_edt_row")
    row = {"bytes": row_bytes, "kernel_us": row_us, "GB_per_s": round(row_bytes / row_us / 1e3, 1) if row_us else None}

    # the host route, on the crop only
    K = min(a.crop, S)
    crop = M[:K, :K].contiguous()
    want = distance.squared_distance(crop, to="set").cpu().numpy()
    t0 = time.perf_counter()
    got = scipy_d2(crop.cpu().numpy() != 0)
    host = {"crop": K, "scipy_ms": round((time.perf_counter() - t0) * 1e3, 1), "device_equals_scipy": bool(np.array_equal(got, want))}
    return {"closing": closed,
            "boundary_vs_rolled": {"n_pred": scores.n_pred, "n_label": scores.n_label, "precision": round(scores.precision[0], 4),
                                   "recall": round(scores.recall[0], 4), "f1": round(scores.f1[0], 4), "hausdorff2": scores.hausdorff2},
            "scratch_MB": round(int(distance._scratch_for(dev, S, S).numel()) / 2 ** 20, 2),
            "ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "kernel_us": kernel_us, "row_pass_of_s": row,
            "s_over_l": round(med["s"] / med["l"], 3), "b2_over_c2": round(med["b2"] / med["c2"], 3), "b12_over_b2": round(med["b12"] / med["b2"], 3),
            "host_on_crop": host}


result = {"tool": "edt_bench", "size": S, "rounds": a.rounds,
          "legs": {"u": "squared_distance(to='unset')", "s": "squared_distance(to='set')", "b2": "buffer_mask(2, 'close')", "c2": "mask_close(2), the 5 x 5 square",
                   "b12": "buffer_mask(12, 'close')", "m": "boundary_scores(mask, mask rolled by (3, 4), (2.0,), check=False)",
                   "l": "label_components + object_table"},
          "scenes": {"rects": measure(scene_rects()), "roofs": measure(scene_roofs()), "single": measure(scene_single()), "empty": measure(scene_empty())}}
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
