"""The self-training round on one whole scene pair, seconds per scene: the device path against what a user composes without it.
python tools/scene_round_bench.py [--size 4096] [--k 3] [--cell 256] [--tile 256] [--stride 256] [--batch 16] [--rounds 5] [--out profiles/scene_round_bench.json]

Over the same K checkpoints (SiamUnet_diff(3, 1), bf16 eval forward) and one seeded device-resident scene pair; every leg ends in a
device synchronise inside its timed window:
  a  stcd_amd.selftrain.scene_round at close_radius 2: K predict_scene calls, stcd_scene_cell_agree, stcd_mask_close, one copy of the counts
  b  the K bare predict_scene calls: the floor
and, on the K masks of leg b (the forwards left out), the post-processing alone:
  p  the two launches and the copy of the counts, as scene_round runs them
  t  the same composed from torch ops on the device: a reshape and one bincount per earlier checkpoint over (cell, last, pred), and
     the closing as -max_pool2d(-max_pool2d(x, 5, 1, 2), 5, 1, 2) on a float copy
  h  the host route the reference's method implies: .cpu() of the K masks and a numpy bincount per cell and earlier checkpoint (the
     closing is left out: the stack ships no cv2)
and the two kernels alone between device events, in GB/s of their own bytes (cell_agree: K * H * W read; close: H * W read and
H * W written).  The legs alternate within one process, every shape is warmed up first; the figures are the medians of --rounds rounds,
the spread is their min and max.  One JSON line, also written to --out."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from stcd_amd import selftrain, synth
from stcd_amd.modules import SiamUnet_diff
from stcd_amd.scene import predict_scene

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=4096); ap.add_argument("--k", type=int, default=3)
ap.add_argument("--cell", type=int, default=256); ap.add_argument("--tile", type=int, default=256); ap.add_argument("--stride", type=int, default=256)
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--kernel_reps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scene_round_bench.json"))
a = ap.parse_args()
assert a.size % a.cell == 0, "the torch composition reshapes the scene into whole cells"
dev = "cuda:0"
K, S, CELL, R = a.k, a.size, a.cell, 2
models = []
for i in range(K):
    torch.manual_seed(900 + i)
    models.append(SiamUnet_diff(3, 1, dtype="bf16").to(dev).eval())
small = 512                                                            # one synthetic block, tiled: the generator's box filter is host work
sa, sb, _ = synth.make_pairs_u8(1, small, small, seed=50)
reps = -(-S // small)
A = torch.from_numpy(np.tile(sa[0], (reps, reps, 1))[:S, :S].copy()).to(dev)
B = torch.from_numpy(np.tile(sb[0], (reps, reps, 1))[:S, :S].copy()).to(dev)
kw = dict(tile=a.tile, stride=a.stride, batch=a.batch)
n = S // CELL


def leg_a():
    r = selftrain.scene_round(models, A, B, cell=CELL, close_radius=R, **kw)
    torch.cuda.synchronize()
    return r


def leg_b():
    masks = [predict_scene(m, A, B, **kw).mask for m in models]
    torch.cuda.synchronize()
    return masks


def post_hip(masks):
    agree = selftrain.scene_cell_agree(masks, CELL)[0]
    pseudo = selftrain.mask_close(masks[-1], R, 255)
    agree = agree.cpu().numpy()
    torch.cuda.synchronize()
    return agree.reshape(n * n, K - 1, 4), pseudo


cell_id = None


def post_torch(masks):
    global cell_id
    if cell_id is None:
        cell_id = (4 * torch.arange(n * n, device=dev).reshape(n, 1, n, 1)).expand(n, CELL, n, CELL)
    last = (masks[-1] != 0).long().reshape(n, CELL, n, CELL)
    agree = torch.stack([torch.bincount((cell_id + 2 * last + (masks[i] != 0).long().reshape(n, CELL, n, CELL)).flatten(), minlength=4 * n * n)
                         for i in range(K - 1)], 1)
    x = (masks[-1] != 0).float()[None, None]
    k = 2 * R + 1
    pseudo = ((-F.max_pool2d(-F.max_pool2d(x, k, 1, R), k, 1, R))[0, 0] * 255).to(torch.uint8)
    agree = agree.cpu().numpy()
    torch.cuda.synchronize()
    return agree.reshape(n * n, 4, K - 1).transpose(0, 2, 1), pseudo


def post_host(masks):
    ms = [m.cpu().numpy() != 0 for m in masks]
    agree = np.zeros((n * n, K - 1, 4), np.int64)
    for cy in range(n):
        for cx in range(n):
            win = (slice(cy * CELL, (cy + 1) * CELL), slice(cx * CELL, (cx + 1) * CELL))
            last = 2 * ms[-1][win].ravel().astype(np.int64)
            for i in range(K - 1):
                agree[cy * n + cx, i] = np.bincount(last + ms[i][win].ravel(), minlength=4)
    return agree, None


def kernel_seconds(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.kernel_reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / a.kernel_reps


ra = leg_a(); masks = leg_b()                                          # every shape and code path once, untimed
same = all(torch.equal(x, y) for x, y in zip(ra.masks, masks))
(ha, hp), (ta, tp), (oa, _) = post_hip(masks), post_torch(masks), post_host(masks)
same = same and np.array_equal(ha, ta) and np.array_equal(ha, oa) and np.array_equal(ha, ra.agree.reshape(n * n, K - 1, 4)) and torch.equal(hp, tp) \
    and torch.equal(hp, ra.pseudo)
legs = {"a": leg_a, "b": leg_b, "p": lambda: post_hip(masks), "t": lambda: post_torch(masks), "h": lambda: post_host(masks)}
secs = {k: [] for k in legs}
for r in range(a.rounds):
    for k, fn in legs.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        secs[k].append(time.perf_counter() - t0)
med = {k: statistics.median(v) for k, v in secs.items()}
# the entries themselves through ctypes, buffers and arguments prepared once: the host's enqueue cost bounds these from below
import ctypes as C
from stcd_amd import _lib
agree_buf = torch.zeros((n, n, K - 1, 2, 2), dtype=torch.int64, device=dev)
close_out = torch.empty_like(masks[-1])
ptrs = (C.c_void_p * K)(*[m.data_ptr() for m in masks])
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
l, vp = _lib.lib(), lambda t: C.c_void_p(t.data_ptr())
t_agree = kernel_seconds(lambda: _lib.check(l.stcd_scene_cell_agree(ptrs, K, S, S, CELL, n, n, None, vp(agree_buf), None, stream)))
t_close = kernel_seconds(lambda: _lib.check(l.stcd_mask_close(vp(masks[-1]), S, S, R, 255, vp(close_out), stream)))
line = json.dumps({"tool": "scene_round_bench", "model": "diff", "dtype": "bf16", "k": K, "size": S, "cell": CELL, "tile": a.tile, "stride": a.stride, "batch": a.batch,
                   "close_radius": R, "rounds": a.rounds, "all_routes_equal": bool(same), "change_fraction_last": round(float((masks[-1] != 0).float().mean()), 4),
                   "seconds": {k: round(v, 6) for k, v in med.items()},
                   "spread": {k: [round(min(v), 6), round(max(v), 6)] for k, v in secs.items()},
                   "a_over_b": round(med["a"] / med["b"], 4), "post_share_of_forwards": round(med["p"] / med["b"], 4),
                   "t_over_p": round(med["t"] / med["p"], 3), "h_over_p": round(med["h"] / med["p"], 3),
                   "kernels": {"cell_agree_us": round(t_agree * 1e6, 2), "cell_agree_GBps": round(K * S * S / t_agree * 1e-9, 1),
                               "mask_close_us": round(t_close * 1e6, 2), "mask_close_GBps": round(2 * S * S / t_close * 1e-9, 1),
                               "note": "back-to-back launches through the C ABI between two device events: per-launch time, not below the host's enqueue cost"},
                   "legs": {"a": "scene_round, close_radius 2", "b": "K bare predict_scene calls", "p": "cell_agree + mask_close + copy of the counts",
                            "t": "bincount + max_pool2d closing in torch on the device", "h": ".cpu() of K masks + numpy bincount per cell (no closing)"}})
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
