"""Topology-safe ring simplification on whole scenes, milliseconds per scene: objects.simplify_rings_safe and objects.ring_conflicts
against the objects.simplify_rings and objects.object_rings they follow.
python tools/topology_bench.py [--size 4096] [--rounds 7] [--crop 512] [--out profiles/topology_bench.json]

The two seeded scenes of tools/simplify_bench.py (rects: axis-parallel rectangles plus salt; roofs: rotated rectangles and discs),
labelled once with connectivity 8.  Per scene, every leg between two device events with a synchronise after the second, the legs
alternating within one process:
  safe15 / safe30  objects.simplify_rings_safe at tolerance 1.5 / 3.0: round 0, every round with its host read, the write
  plain15 / plain30  objects.simplify_rings at the same tolerances: the yardstick the safe path is reported as a multiple of
  ct / cs  objects.ring_conflicts(check=False) on the traced rings / on the plainly simplified rings (1.5)
  r  objects.object_rings on the same labels
  h  the host route ON A --crop SQUARED CROP ONLY: .cpu() of the crop's rings + tests/topology_spec.simplify_safe at 1.5; reported as
     exactly that, not extrapolated to the scene
"kernel_us" is the device time of every k_topo_* (and k_simplify_*) kernel per simplify_rings_safe call at 1.5, from torch.profiler
(null where the profiler reports no kernels).  Per tolerance: rounds, restored vertices, the conflicting edges and pocket hits plain
Douglas-Peucker leaves (the first detection pass), "per_round_ms" = (safe - plain) / (rounds + 1) detection passes.  Every shape is
warmed up first; the figures are medians of --rounds rounds, the spread is their min and max.  One JSON line, also written to --out."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import _lib, objects
from tests import rings_spec, topology_spec

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--crop", type=int, default=512)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "topology_bench.json"))
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


def first_pass(rings, tolerance):
    """(conflicting edges, pocket hits) of plain Douglas-Peucker on ``rings``: the counts of the first detection pass, from the raw entries."""
    l = _lib.lib()
    R, V, q = rings.count, int(rings.vertices.shape[0]), objects.simplify_q(tolerance)
    nbytes = int(l.stcd_rings_topo_scratch_bytes(R, V, 0))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(l.stcd_rings_safe_begin(p(rings.vertices), p(rings.offsets), R, V, q, 0, p(counts), p(scratch), nbytes, stream))
    E = int(counts[1])
    cap = 8 * E + 65536
    entries = torch.empty(cap, dtype=torch.int32, device=dev)
    _lib.check(l.stcd_rings_safe_round(p(rings.vertices), p(rings.offsets), R, V, 0, E, 0, p(counts), p(entries), cap, p(scratch), nbytes, stream))
    c = counts.cpu().tolist()
    return (c[4], c[5]) if c[0] == 0 else (None, None)


def measure(name, mask):
    M = torch.from_numpy(mask).to(dev)
    comp = objects.label_components(M)
    rings = objects.object_rings(comp)
    K = min(a.crop, S)
    crop = objects.object_rings(objects.Components(comp.labels[:K, :K].contiguous(), comp.count))
    plain15 = objects.simplify_rings(rings, 1.5)

    legs = {"safe15": lambda: objects.simplify_rings_safe(rings, 1.5), "plain15": lambda: objects.simplify_rings(rings, 1.5),
            "safe30": lambda: objects.simplify_rings_safe(rings, 3.0), "plain30": lambda: objects.simplify_rings(rings, 3.0),
            "ct": lambda: objects.ring_conflicts(rings, check=False), "cs": lambda: objects.ring_conflicts(plain15, check=False),
            "r": lambda: objects.object_rings(comp)}
    first = {k: fn() for k, fn in legs.items()}                        # every shape and code path once, untimed
    torch.cuda.synchronize()
    print(f"{name}: warmed up, {rings.count} rings, {int(rings.vertices.shape[0])} vertices", file=sys.stderr, flush=True)
    ms = {k: [] for k in legs}
    for r in range(a.rounds):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            fn()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"{name}: device legs done", file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    host = rings_spec.RingSet(*(t.cpu().numpy() for t in crop[:4]), crop.count)
    want = topology_spec.simplify_safe(host, objects.simplify_q(1.5))
    host_ms = (time.perf_counter() - t0) * 1e3
    got = objects.simplify_rings_safe(crop, 1.5)
    same = got[1:] == want[1:] and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got.rings[:4], want[0][:4]))
    print(f"{name}: host route on the crop done", file=sys.stderr, flush=True)

    kernel_us = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(a.rounds):
                legs["safe15"]()
            torch.cuda.synchronize()
        rows = {}
        for e in prof.key_averages():
            if "k_topo_" in e.key or "k_simplify_" in e.key:
                kname = e.key.split("(")[0].split("::")[-1].split("<")[0]
                total = getattr(e, "device_time_total", None)
                total = e.cuda_time_total if total is None else total
                row = rows.setdefault(kname, [0.0, 0])
                row[0] = round(row[0] + total / a.rounds, 2); row[1] += e.count // a.rounds
        kernel_us = rows or None
    except Exception as exc:                                           # the profiler is an observer: the figures above stand without it
        print(f"torch.profiler gave no kernel table: {exc!r}", file=sys.stderr)

    out = {"objects": int(comp.count), "rings": rings.count, "vertices": int(rings.vertices.shape[0]),
           "scratch_MB": round(int(_lib.lib().stcd_rings_topo_scratch_bytes(rings.count, int(rings.vertices.shape[0]), 0)) / 2 ** 20, 2),
           "ms": {k: round(v, 3) for k, v in med.items()}, "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
           "conflicts_traced": int(first["ct"].count), "conflicts_plain15": int(first["cs"].count), "kernel_us": kernel_us,
           "crop": K, "crop_rings": int(crop.count), "crop_vertices": int(crop.vertices.shape[0]), "host_crop_ms": round(host_ms, 1),
           "device_equals_spec_on_crop": bool(same)}
    for t, tag in ((1.5, "15"), (3.0, "30")):
        safe, plain = first["safe" + tag], first["plain" + tag]
        flagged, hits = first_pass(rings, t)
        out["tolerance_" + tag] = {"rounds": safe.rounds, "restored": safe.restored, "conflicts_left": safe.conflicts,
                                   "vertices_plain": int(plain.vertices.shape[0]), "vertices_safe": int(safe.rings.vertices.shape[0]),
                                   "plain_conflicting_edges": flagged, "plain_pocket_hits": hits,
                                   "safe_over_plain": round(med["safe" + tag] / med["plain" + tag], 2),
                                   "per_round_ms": round((med["safe" + tag] - med["plain" + tag]) / (safe.rounds + 1), 3)}
    return out


result = {"tool": "topology_bench", "size": S, "connectivity": 8, "cell": objects.TOPO_CELL, "rounds": a.rounds,
          "legs": {"safe15 / safe30": "simplify_rings_safe at 1.5 / 3.0", "plain15 / plain30": "simplify_rings at 1.5 / 3.0",
                   "ct": "ring_conflicts(check=False) on the traced rings", "cs": "ring_conflicts(check=False) on simplify_rings(1.5)",
                   "r": "object_rings on the same labels",
                   "h": f".cpu() + tests/topology_spec.simplify_safe on the rings of the {min(a.crop, S)} x {min(a.crop, S)} crop only (not extrapolated)"},
          "scenes": {"rects": measure("rects", scene_rects()), "roofs": measure("roofs", scene_roofs())}}
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
