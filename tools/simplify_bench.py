"""Ring simplification on whole scenes, milliseconds per scene: objects.simplify_rings against the objects.object_rings it follows.
python tools/simplify_bench.py [--size 4096] [--tolerance 1.5] [--rounds 7] [--crop 512] [--out profiles/simplify_bench.json]

Two seeded scenes, labelled once with connectivity 8:
  rects  tools/rings_bench.py's: axis-parallel rectangles plus salt, so nearly every ring has 4 vertices
  roofs  about 600 rotated rectangles and discs, whose outlines are staircases of 50 to 600 vertices
Per scene, every leg ending in a device synchronise inside its timed window and the legs alternating within one process:
  s  objects.simplify_rings at --tolerance on the rings of the scene: both phases and the one host read between them
  r  objects.object_rings on the same labels: the on-device yardstick
  h  the host route ON A --crop SQUARED CROP ONLY: .cpu() of the crop's rings + tests/simplify_spec.simplify; reported as exactly
     that, not extrapolated to the scene
"phase_ms" times stcd_rings_simplify_count and stcd_rings_simplify_write separately with device events (no host read between them:
V' is known from the first call); "kernel_us" is the device time of every k_simplify_* kernel per simplify_rings call, from
torch.profiler (null where the profiler reports no kernels).  "ring_lengths" counts the scene's rings by length (the bins end at
the kernels' thresholds among others), "levels" the same rings by the levels of Douglas-Peucker they need (the rounds of the kernels
are one more), from an untimed run of the specification over the whole scene, which is also compared with the device's result.  Every
shape is warmed up first; the figures are the medians of --rounds rounds, the spread is their min and max.  One JSON line, also written to
--out."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import _lib, objects
from tests import simplify_spec

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--tolerance", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--crop", type=int, default=512)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "simplify_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")
S = a.size
q = objects.simplify_q(a.tolerance)


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
    rng = np.random.default_rng(61)
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


BINS = [4, 8, 16, 32, objects.SIMPLIFY_WAVE_MAX, 128, 256, 512, 1024, objects.SIMPLIFY_LDS_MAX]


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
    K = min(a.crop, S)
    crop = objects.object_rings(objects.Components(comp.labels[:K, :K].contiguous(), comp.count))

    def leg_s():
        out = objects.simplify_rings(rings, a.tolerance)
        torch.cuda.synchronize()
        return out

    def leg_r():
        out = objects.object_rings(comp)
        torch.cuda.synchronize()
        return out

    detail = []

    def leg_h():
        del detail[:]
        host = simplify_spec.RingSet(*(t.cpu().numpy() for t in crop[:4]), crop.count)
        return simplify_spec.simplify(host, q, detail)

    legs = {"s": leg_s, "r": leg_r, "h": leg_h}
    first = {k: fn() for k, fn in legs.items()}                        # every shape and code path once, untimed
    simple = first["s"]
    got = objects.simplify_rings(crop, a.tolerance)
    same = got.count == first["h"].count and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got[:4], first["h"][:4]))
    secs = {k: [] for k in legs}
    for r in range(a.rounds):
        for k, fn in legs.items():
            if k == "h" and r >= 2:                                    # the host route is slow and steady: two rounds
                continue
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            secs[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in secs.items()}

    # the two entries on their own, with device events
    l = _lib.lib()
    R, V, Vout = rings.count, int(rings.vertices.shape[0]), int(simple.vertices.shape[0])
    nbytes = int(l.stcd_rings_simplify_scratch_bytes(R, V))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    outs = (torch.empty((Vout, 2), dtype=torch.int32, device=dev), torch.empty(R + 1, dtype=torch.int64, device=dev), torch.empty(R, dtype=torch.int64, device=dev))
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    phase = {"count": [], "write": []}
    for r in range(a.rounds + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.check(l.stcd_rings_simplify_count(p(rings.vertices), p(rings.offsets), R, V, q, p(counts), p(scratch), nbytes, stream))
        ev[1].record()
        _lib.check(l.stcd_rings_simplify_write(p(rings.vertices), p(rings.offsets), R, V, q, Vout, *(p(t) for t in outs), p(scratch), nbytes, stream))
        ev[2].record()
        torch.cuda.synchronize()
        if r:                                                          # the first round warms up
            phase["count"].append(ev[0].elapsed_time(ev[1])); phase["write"].append(ev[1].elapsed_time(ev[2]))
    same = same and counts.cpu().tolist() == [Vout, 0] and torch.equal(outs[0], simple.vertices) and torch.equal(outs[1], simple.offsets) and torch.equal(outs[2], simple.area2)

    kernel_us = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(a.rounds):
                leg_s()
        rows = {}
        for e in prof.key_averages():
            if "k_simplify_" in e.key:
                name = e.key.split("(")[0].split("::")[-1]
                total = getattr(e, "device_time_total", None)
                total = e.cuda_time_total if total is None else total
                rows[name] = [round(total / a.rounds, 2), e.count // a.rounds]
        kernel_us = rows or None
    except Exception as exc:                                           # the profiler is an observer: the figures above stand without it
        print(f"torch.profiler gave no kernel table: {exc!r}", file=sys.stderr)

    # untimed: the specification over every ring of the scene, for the levels each ring needs and one more equality
    levels = []
    whole_scene = simplify_spec.simplify(simplify_spec.RingSet(*(t.cpu().numpy() for t in rings[:4]), rings.count), q, levels)
    same_scene = all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(simple[:4], whole_scene[:4]))
    lengths = torch.diff(rings.offsets).cpu().numpy()
    return {"objects": int(comp.count), "rings": R, "vertices_before": V, "vertices_after": Vout, "longest_ring": int(lengths.max()) if R else 0,
            "scratch_MB": round(nbytes / 2 ** 20, 2), "device_equals_spec_on_crop": bool(same), "crop": K, "crop_rings": int(crop.count),
            "crop_vertices": [int(crop.vertices.shape[0]), int(first["h"].vertices.shape[0])],
            "ms": {k: round(v * 1e3, 3) for k, v in med.items()},
            "spread_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in secs.items()},
            "phase_ms": {k: round(statistics.median(v), 3) for k, v in phase.items()},
            "kernel_us": kernel_us, "s_over_r": round(med["s"] / med["r"], 3),
            "ring_lengths": histogram(lengths, BINS),
            "levels": histogram([d[1] for d in levels], [1, 2, 4, 8, 16, 32, 64]), "most_levels": max([d[1] for d in levels] + [0]),
            "triangle_rule": int(sum(1 for d in levels if d[2] == 4)), "whole_by_the_sign_rule": int(sum(1 for d in levels if d[2] == 5)),
            "device_equals_spec_on_scene": bool(same_scene)}


result = {"tool": "simplify_bench", "size": S, "tolerance": a.tolerance, "q": q, "connectivity": 8, "rounds": a.rounds,
          "legs": {"s": "simplify_rings: count phase, one host read, write phase", "r": "object_rings on the same labels",
                   "h": f".cpu() + tests/simplify_spec.simplify on the rings of the {min(a.crop, S)} x {min(a.crop, S)} crop only (not extrapolated)"},
          "scenes": {"rects": measure(scene_rects()), "roofs": measure(scene_roofs())}}
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
