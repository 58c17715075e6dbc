"""Change polygons on one whole scene, milliseconds per scene: objects.object_rings against the labelling it follows.
python tools/rings_bench.py [--size 4096] [--rects 600] [--salt 0.002] [--rounds 5] [--crop 512] [--out profiles/rings_bench.json]

The scene is tools/objects_bench.py's (same generator, same seed), labelled once with connectivity 8.  Every leg ends in a device
synchronise inside its timed window:
  r  objects.object_rings: both phases and the one host read between them
  l  objects.label_components + objects.object_table on the same mask: the on-device yardstick
  h  the host route ON A --crop SQUARED CROP ONLY: .cpu() of the crop's labels + tests/rings_spec.rings; reported as exactly that,
     not extrapolated to the scene
"phase_ms" times stcd_rings_count and stcd_rings_write separately with device events (no host read between them: R and V are
known from the first call); "kernel_us" is the device time of every k_ring_* kernel per object_rings call, from torch.profiler
(null where the profiler reports no kernels).  "algorithmic_GBps" of r: the bytes any implementation must move, the int32 labels
read once and the four outputs written once.  The legs alternate within one process, every shape is warmed up first; the figures
are the medians of --rounds rounds, the spread is their min and max.  One JSON line, also written to --out."""
import argparse, ctypes as C, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import _lib, objects
from tests import rings_spec

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--rects", type=int, default=600)
ap.add_argument("--salt", type=float, default=0.002); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--crop", type=int, default=512)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rings_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")
S = a.size
rng = np.random.default_rng(60)                                        # tools/objects_bench.py's scene
m = np.zeros((S, S), np.uint8)
for _ in range(a.rects):
    h, w = rng.integers(8, 97, 2)
    y, x = rng.integers(0, max(S - h, 1)), rng.integers(0, max(S - w, 1))
    m[y:y + h, x:x + w] = 255
    if h >= 24 and w >= 24 and rng.random() < 0.3:
        c = int(rng.integers(2, 7))
        m[y + h // 2 - c // 2:y + h // 2 + c - c // 2, x + w // 2 - c // 2:x + w // 2 + c - c // 2] = 0
m[rng.random((S, S)) < a.salt] = 255
M = torch.from_numpy(m).to(dev)
comp = objects.label_components(M)
K = min(a.crop, S)
crop = objects.Components(comp.labels[:K, :K].contiguous(), comp.count)


def leg_r():
    out = objects.object_rings(comp)
    torch.cuda.synchronize()
    return out


def leg_l():
    c = objects.label_components(M)
    t = objects.object_table(c)
    torch.cuda.synchronize()
    return c, t


def leg_h():
    return rings_spec.rings(crop.labels.cpu().numpy(), 8)


legs = {"r": leg_r, "l": leg_l, "h": leg_h}
first = {k: fn() for k, fn in legs.items()}                            # every shape and code path once, untimed
rings = first["r"]
R, V = rings.count, int(rings.vertices.shape[0])
got = objects.object_rings(crop)
same = got.count == first["h"].count and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got[:4], first["h"][:4]))
secs = {k: [] for k in legs}
for r in range(a.rounds):
    for k, fn in legs.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        secs[k].append(time.perf_counter() - t0)
med = {k: statistics.median(v) for k, v in secs.items()}

# the two entries on their own, with device events
l = _lib.lib()
cap = min(S * S // 4 + 4096, 4 * (S + 1) * (S + 1))                     # object_rings' default capacity
repeated = V > cap
cap = max(cap, V)
nbytes = int(l.stcd_rings_scratch_bytes(S, S, cap))
scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
counts = torch.empty(3, dtype=torch.int64, device=dev)
outs = (torch.empty((V, 2), dtype=torch.int32, device=dev), torch.empty(R + 1, dtype=torch.int64, device=dev),
        torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int64, device=dev))
p = lambda t: C.c_void_p(t.data_ptr())
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
phase = {"count": [], "write": []}
for r in range(a.rounds + 1):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    _lib.check(l.stcd_rings_count(p(comp.labels), S, S, 8, cap, p(counts), p(scratch), nbytes, stream))
    ev[1].record()
    _lib.check(l.stcd_rings_write(p(comp.labels), S, S, 8, cap, R, V, *(p(t) for t in outs), p(scratch), nbytes, stream))
    ev[2].record()
    torch.cuda.synchronize()
    if r:                                                              # the first round warms up
        phase["count"].append(ev[0].elapsed_time(ev[1])); phase["write"].append(ev[1].elapsed_time(ev[2]))
same = same and counts.cpu().tolist() == [R, V, 0] and all(torch.equal(x, y) for x, y in zip(outs, rings[:4]))

kernel_us = None
try:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(a.rounds):
            leg_r()
    rows = {}
    for e in prof.key_averages():
        if "k_ring_" in e.key:
            name = e.key.split("(")[0].split("::")[-1]
            total = getattr(e, "device_time_total", None)
            total = e.cuda_time_total if total is None else total
            rows[name] = [round(total / a.rounds, 2), e.count // a.rounds]
    kernel_us = rows or None
except Exception as exc:                                               # the profiler is an observer: the figures above stand without it
    kernel_us = None
    print(f"torch.profiler gave no kernel table: {exc!r}", file=sys.stderr)

bytes_r = 4 * S * S + 8 * V + 8 * (R + 1) + 4 * R + 8 * R
line = json.dumps({"tool": "rings_bench", "size": S, "rects": a.rects, "salt": a.salt, "connectivity": 8, "rounds": a.rounds, "objects": int(comp.count),
                   "rings": R, "vertices": V, "jump_rounds": int(math.ceil(math.log2(V))) if V > 1 else 0, "jump_launches": int(math.ceil(math.log2(cap))) if cap > 1 else 0,
                   "max_corners": cap, "count_phase_repeated": bool(repeated), "scratch_MB": round(nbytes / 2 ** 20, 1),
                   "longest_ring": int(torch.diff(rings.offsets).max()) if R else 0,
                   "device_equals_spec_on_crop": bool(same), "crop": K, "crop_rings": first["h"].count,
                   "ms": {k: round(v * 1e3, 3) for k, v in med.items()},
                   "spread_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in secs.items()},
                   "phase_ms": {k: round(statistics.median(v), 3) for k, v in phase.items()},
                   "kernel_us": kernel_us,
                   "algorithmic_GBps": {"r": round(bytes_r / med["r"] * 1e-9, 2), "l": round(5 * S * S / med["l"] * 1e-9, 2)},
                   "r_over_l": round(med["r"] / med["l"], 2),
                   "legs": {"r": "object_rings: count phase, one host read, write phase", "l": "label_components + object_table",
                            "h": f".cpu() + tests/rings_spec.rings on the {K} x {K} crop only (not extrapolated)"}})
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
