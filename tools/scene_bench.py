"""Whole-scene inference throughput: predict_scene (tile, forward, stitch on the device) against a host tiler and the bare forward.
python tools/scene_bench.py --model diff|conc|snunet|snunet_conc|segcd [--size 4096] [--tile 256] [--stride 256|128] [--batch 16] [--reps 20]
python tools/scene_bench.py --tta d4|flip --model diff|segcd [--stride 256|128] [--rounds 5] [--json out.json]      (see tta_mode below)

Three rates, each in megapixels/s of scene and tile-pairs/s:
  device : stcd_amd.scene.predict_scene (bf16 eval forward, frozen weights), flat window, no label; mean of --reps calls in one timed window
  host   : what a user has to write without it, numpy and torch only: crop with reflection, normalise, upload, the same forward,
           download, numpy blend and arg-max
  forward: the eval-forward loop of tools/infer_bench.py alone, at the same batch and tile (frozen weights), as tile-pairs/s"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import synth
from stcd_amd.modules import frozen_weights
from stcd_amd.scene import plan_tiles, predict_scene

ap = argparse.ArgumentParser(); ap.add_argument("--model", default="diff"); ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--tile", type=int, default=256); ap.add_argument("--stride", type=int, default=256); ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--reps", type=int, default=20); ap.add_argument("--steps", type=int, default=500); ap.add_argument("--no-host", action="store_true")
ap.add_argument("--tta", default=None, choices=("flip", "d4")); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--json", default="")
a = ap.parse_args()
dev = "cuda:0"
if a.model == "segcd":
    from stcd_amd.segcd import SegCD
    m = SegCD().to(dev).eval()
else:
    from stcd_amd import modules
    m = {"diff": modules.SiamUnet_diff, "conc": modules.SiamUnet_conc, "snunet": modules.SNUNet_ECAM, "snunet_conc": modules.Siam_NestedUNet_Conc}[a.model](3, 2).to(dev).eval()
H = W = a.size
T, S = a.tile, a.stride
plan = plan_tiles(H, W, T, S)
# one synthetic tile pair repeated over the scene: the content does not change the cost
ta, tb, _ = synth.make_pairs_u8(1, 512, 512, seed=5)
rep = -(-a.size // 512)
sa = np.ascontiguousarray(np.tile(ta[0], (rep, rep, 1))[:H, :W]); sb = np.ascontiguousarray(np.tile(tb[0], (rep, rep, 1))[:H, :W])


def report(name, dt):
    print(f"{name:8s} {a.model} {H}x{W} tile {T} stride {S} batch {a.batch}: {dt * 1e3:9.2f} ms  {H * W / dt / 1e6:9.1f} Mpx/s  {plan.n / dt:9.0f} tile-pairs/s", flush=True)


def timed(fn, reps):
    """mean seconds per call over one synchronised window of `reps` calls, after a warm-up call (workspace, filter images, allocator)"""
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


da, db = torch.from_numpy(sa).to(dev), torch.from_numpy(sb).to(dev)


def tta_mode():
    """--tta: test-time augmentation, three rates in transformed tile-pairs/s (views x tiles per call), alternated a, b, c for
    --rounds rounds in this one process so that clock and thermal drift fall on all three alike:
      a  predict_scene(tta=...): stcd_scene_gather_d4 / stcd_scene_stitch_d4 write and read the views directly
      b  the same views composed from torch.flip / transpose(...).contiguous() around the upright entries: what a user writes today
      c  the bare eval forward over views x tiles batches
    and, with events around single launches, a transposing and a mirror gather / stitch launch against the d4 = 0 launch of the
    same call (they move the same bytes)."""
    import ctypes as C, json
    from stcd_amd import _lib
    from stcd_amd.scene import parse_tta
    views = parse_tta(a.tta)
    l = _lib.lib()
    m3, s3 = (C.c_float * 3)(*synth.MEAN), (C.c_float * 3)(*synth.STD)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def flip(x, d):
        dims = [dim for dim, bit in ((-2, 2), (-1, 1)) if d & bit]
        return torch.flip(x, dims) if dims else x

    def run_a():
        return predict_scene(m, da, db, tile=T, stride=S, batch=a.batch, tta=a.tta).mask

    def run_b():
        x1 = torch.empty((a.batch, 3, T, T), dtype=torch.float32, device=dev); x2 = torch.empty_like(x1)
        acc = wsum = None
        with torch.no_grad(), frozen_weights(m):
            for d in views:
                for first in range(0, plan.n, a.batch):
                    n = min(a.batch, plan.n - first)
                    _lib.check(l.stcd_scene_gather(ptr(da), ptr(db), H, W, T, S, plan.tiles_x, first, n, m3, s3, ptr(x1), ptr(x2), stream()))
                    v1, v2 = flip(x1[:n], d), flip(x2[:n], d)
                    if d & 4:
                        v1, v2 = v1.transpose(-1, -2), v2.transpose(-1, -2)
                    out = m(v1.contiguous(), v2.contiguous())
                    out = (out[-1] if isinstance(out, (list, tuple)) else out).float()
                    out = flip(out.transpose(-1, -2) if d & 4 else out, d).contiguous()
                    if acc is None:
                        acc = torch.zeros((out.shape[1], H, W), dtype=torch.float32, device=dev); wsum = torch.zeros((H, W), dtype=torch.float32, device=dev)
                    _lib.check(l.stcd_scene_stitch(ptr(out), out.shape[1], H, W, T, S, plan.tiles_x, plan.tiles_y, first, n, None, ptr(acc), ptr(wsum), stream()))
            mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
            _lib.check(l.stcd_scene_finalize(ptr(acc), ptr(wsum), out.shape[1], H, W, C.c_float(0.0), None, ptr(mask), None, None, stream()))
        return mask

    x1, x2, _ = synth.make_batch(a.batch, T, T, seed=5)
    A, B = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    calls = len(views) * -(-plan.n // a.batch)

    def run_c():
        with torch.no_grad(), frozen_weights(m):
            for _ in range(calls):
                m(A, B)

    same = bool(torch.equal(run_a(), run_b()))                        # the same launches in the same order: the same mask
    run_c(); torch.cuda.synchronize()
    pairs = len(views) * plan.n
    rates = {"a": [], "b": [], "c": []}
    for _ in range(a.rounds):
        for name, fn in (("a", run_a), ("b", run_b), ("c", run_c)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
            rates[name].append(pairs * a.reps / (time.perf_counter() - t0))

    # ---- single launches under events: a batch of tiles, median of 20 after 3 warm-up launches
    n = min(a.batch, plan.n)
    g1 = torch.empty((n, 3, T, T), dtype=torch.float32, device=dev); g2 = torch.empty_like(g1)
    lg = torch.randn((n, 2, T, T), device=dev)
    acc = torch.zeros((2, H, W), dtype=torch.float32, device=dev); wsum = torch.zeros((H, W), dtype=torch.float32, device=dev)

    def launch_us(fn):
        ts = []
        for i in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ts))

    launches = {}
    for d in (0, 3, 4, 7):
        launches[f"gather_d{d}_us"] = launch_us(lambda: _lib.check(l.stcd_scene_gather_d4(ptr(da), ptr(db), H, W, T, S, plan.tiles_x, 0, n, m3, s3, ptr(g1), ptr(g2), d, stream())))
        launches[f"stitch_d{d}_us"] = launch_us(lambda: _lib.check(l.stcd_scene_stitch_d4(ptr(lg), 2, H, W, T, S, plan.tiles_x, plan.tiles_y, 0, n, None, ptr(acc), ptr(wsum), d, stream())))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    res = {"model": a.model, "size": a.size, "tile": T, "stride": S, "batch": a.batch, "tta": a.tta, "views": len(views), "masks_equal": same, "reps": a.reps, "rounds": a.rounds,
           "pairs_per_s": {k: [round(x, 1) for x in v] for k, v in rates.items()}, "median_pairs_per_s": {k: round(v, 1) for k, v in med.items()},
           "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in rates.items()},
           "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4), "launch_us": {k: round(v, 2) for k, v in launches.items()}}
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(res) + "\n")


if a.tta:
    tta_mode()
    sys.exit(0)

# ---- device path: the scenes already sit in HBM, as the training tiles do
dev_mask = None
def run_device():
    global dev_mask
    dev_mask = predict_scene(m, da, db, tile=T, stride=S, batch=a.batch).mask
report("device", timed(run_device, a.reps))


# ---- host tiler: numpy crops and blend around the same forward
def reflect(i, L):
    if L == 1:
        return np.zeros_like(i)
    p = 2 * (L - 1); i = i % p
    return np.where(i >= L, p - i, i)

host_mask = None
def run_host():
    global host_mask
    mean = np.asarray(synth.MEAN, np.float32); std = np.asarray(synth.STD, np.float32)
    acc = None; wsum = np.zeros((H, W), np.float32); t = np.arange(T)
    with torch.no_grad(), frozen_weights(m):
        for first in range(0, plan.n, a.batch):
            ks = range(first, min(first + a.batch, plan.n))
            xa = np.empty((len(ks), T, T, 3), np.uint8); xb = np.empty_like(xa)
            for j, k in enumerate(ks):
                ky, kx = divmod(k, plan.tiles_x)
                ys, xs = ky * S + t, kx * S + t
                if ys[-1] < H and xs[-1] < W:
                    xa[j] = sa[ys[0]:ys[0] + T, xs[0]:xs[0] + T]; xb[j] = sb[ys[0]:ys[0] + T, xs[0]:xs[0] + T]
                else:
                    ys, xs = reflect(ys, H), reflect(xs, W)
                    xa[j] = sa[ys][:, xs]; xb[j] = sb[ys][:, xs]
            x1 = torch.from_numpy(np.ascontiguousarray(((xa.astype(np.float32) / 255.0 - mean) / std).transpose(0, 3, 1, 2))).to(dev)
            x2 = torch.from_numpy(np.ascontiguousarray(((xb.astype(np.float32) / 255.0 - mean) / std).transpose(0, 3, 1, 2))).to(dev)
            out = m(x1, x2)
            out = (out[-1] if isinstance(out, (list, tuple)) else out).float().cpu().numpy()
            if acc is None:
                acc = np.zeros((out.shape[1], H, W), np.float32)
            for j, k in enumerate(ks):
                ky, kx = divmod(k, plan.tiles_x)
                y0, x0 = ky * S, kx * S
                h, w = min(T, H - y0), min(T, W - x0)
                acc[:, y0:y0 + h, x0:x0 + w] += out[j, :, :h, :w]; wsum[y0:y0 + h, x0:x0 + w] += 1.0
    host_mask = (acc[1] > acc[0]) if acc.shape[0] == 2 else (acc[0] > 0)
if not a.no_host:
    report("host", timed(run_host, 1))
    diff = int((torch.from_numpy(host_mask).to(dev) != (dev_mask == 1)).sum())
    print(f"         masks of the two paths differ in {diff} of {H * W} pixels (only near-ties may: the host normalises with a division)")

# ---- the bare eval forward at the same batch and tile (tools/infer_bench.py's loop)
x1, x2, _ = synth.make_batch(a.batch, T, T, seed=5)
A, B = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
with torch.no_grad(), frozen_weights(m):
    for _ in range(5):
        m(A, B)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(a.steps):
        m(A, B)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.steps
print(f"forward  {a.model} eval forward, {a.batch} pairs {T}x{T}, frozen_weights: {dt * 1e3:.3f} ms  {a.batch / dt:.0f} tile-pairs/s  "
      f"({a.batch * T * T / dt / 1e6:.1f} Mpx/s of tiles)")
