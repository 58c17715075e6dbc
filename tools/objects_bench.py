"""Change objects on one whole scene mask, milliseconds per scene: the device path against the host route it replaces.
python tools/objects_bench.py [--size 4096] [--rects 600] [--salt 0.002] [--min_area 64] [--max_hole 32] [--rounds 5] [--out profiles/objects_bench.json]

One seeded synthetic mask of --size squared on the device: --rects filled rectangles (the buildings, some with a courtyard) plus salt
noise of density --salt (the false alarms the filter is for).  Every leg ends in a device synchronise inside its timed window:
  f  objects.filter_objects(min_area, max_hole, check=False): both steps, no host read
  l  objects.label_components + objects.object_table: labels, count (one 8-byte copy), area and boxes
  h  the host route: .cpu() of the mask, scipy.ndimage.label + np.bincount + remap of the small objects where scipy is present,
     else the numpy labeller of tests/objects_spec.py ("host_labeller" says which)
  c  selftrain.mask_close at radius 2 on the same mask: the yardstick of a one-pass scene operation
with the algorithmic GB/s of each: bytes that any implementation must move (f and c: the mask read and the mask written, 2 B per
pixel; l: the mask read and the int32 labels written, 5 B per pixel; h as f).  The legs alternate within one process, every shape
is warmed up first; the figures are the medians of --rounds rounds, the spread is their min and max.  One JSON line, also written
to --out."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import objects, selftrain

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--rects", type=int, default=600)
ap.add_argument("--salt", type=float, default=0.002); ap.add_argument("--min_area", type=int, default=64); ap.add_argument("--max_hole", type=int, default=32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "objects_bench.json"))
a = ap.parse_args()
dev = "cuda:0"
S = a.size
rng = np.random.default_rng(60)
m = np.zeros((S, S), np.uint8)
for _ in range(a.rects):
    h, w = rng.integers(8, 97, 2)
    y, x = rng.integers(0, max(S - h, 1)), rng.integers(0, max(S - w, 1))
    m[y:y + h, x:x + w] = 255
    if h >= 24 and w >= 24 and rng.random() < 0.3:                     # a courtyard: a hole the filter fills when it is small
        c = int(rng.integers(2, 7))
        m[y + h // 2 - c // 2:y + h // 2 + c - c // 2, x + w // 2 - c // 2:x + w // 2 + c - c // 2] = 0
m[rng.random((S, S)) < a.salt] = 255
M = torch.from_numpy(m).to(dev)

try:
    from scipy import ndimage
    host_labeller = "scipy.ndimage.label"
    full = np.ones((3, 3), bool)
    label_host = lambda x: ndimage.label(x, structure=full)
except ImportError:
    from tests import objects_spec
    host_labeller = "tests/objects_spec.py"
    label_host = lambda x: objects_spec.label(x, 8)


def leg_f():
    out = objects.filter_objects(M, a.min_area, a.max_hole, check=False)
    torch.cuda.synchronize()
    return out


def leg_l():
    c = objects.label_components(M)
    t = objects.object_table(c)
    torch.cuda.synchronize()
    return c, t


def leg_h():
    x = M.cpu().numpy() != 0
    lab, n = label_host(x)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= a.min_area
    keep[0] = False
    return keep[lab].astype(np.uint8) * np.uint8(255), n, area[1:]      # step 1 only: the hole step would be a second labelling


def leg_c():
    out = selftrain.mask_close(M, 2, 255)
    torch.cuda.synchronize()
    return out


legs = {"f": leg_f, "l": leg_l, "h": leg_h, "c": leg_c}
first = {k: fn() for k, fn in legs.items()}                            # every shape and code path once, untimed
(comp, tab), (h_mask, h_n, h_area) = first["l"], first["h"]
same = comp.count == h_n and np.array_equal(tab.area.cpu().numpy(), h_area) \
    and np.array_equal(objects.filter_objects(M, a.min_area, 0).cpu().numpy(), h_mask)
secs = {k: [] for k in legs}
for r in range(a.rounds):
    for k, fn in legs.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        secs[k].append(time.perf_counter() - t0)
med = {k: statistics.median(v) for k, v in secs.items()}
bytes_of = {"f": 2 * S * S, "l": 5 * S * S, "h": 2 * S * S, "c": 2 * S * S}
line = json.dumps({"tool": "objects_bench", "size": S, "rects": a.rects, "salt": a.salt, "min_area": a.min_area, "max_hole": a.max_hole, "connectivity": 8,
                   "rounds": a.rounds, "objects": int(comp.count), "set_fraction": round(float((M != 0).float().mean()), 4),
                   "pixels_changed_by_filter": int((first["f"] != M).sum()), "host_labeller": host_labeller, "device_equals_host": bool(same),
                   "ms": {k: round(v * 1e3, 3) for k, v in med.items()},
                   "spread_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in secs.items()},
                   "algorithmic_GBps": {k: round(bytes_of[k] / med[k] * 1e-9, 2) for k in legs},
                   "h_over_f": round(med["h"] / med["f"], 2), "h_over_l": round(med["h"] / med["l"], 2), "f_over_c": round(med["f"] / med["c"], 2),
                   "l_over_c": round(med["l"] / med["c"], 2),
                   "legs": {"f": "filter_objects(check=False), both steps", "l": "label_components + object_table",
                            "h": ".cpu() + host labelling + bincount + remap (step 1 only)", "c": "mask_close, radius 2"}})
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
