"""SegCD's three maps over one whole scene pair, ms per pair: predict_scene_heads against what the single-head entries allow.
python tools/scene_heads_bench.py [--model segcd] [--encoder resnet50|resnet18] [--size 4096] [--stride 256|128] [--tta d4] [--rounds 5]
                                  [--out profiles/scene_heads_bench.json]

One SegCD(encoder) (bf16 eval forward) and one seeded device-resident scene pair with a change label; every leg ends in a device
synchronise inside its timed window:
  a  stcd_amd.scene.predict_scene_heads: per batch one stcd_scene_stitch_heads_d4, at the end one stcd_scene_finalize_seg
  b  the same gathers and forwards with the composition the single-head entries allow: per batch three stcd_scene_stitch_d4 calls into
     three acc / wsum pairs; at the end three stcd_scene_finalize calls, the gate in torch ops and a torch.bincount for its matrix
  c  the same gathers and the bare eval forwards: the floor
and the two new kernels alone between device events, in GB/s of their own bytes (stitch: the logits of one batch read, the planes
of acc and wsum under the batch's tiles read and written; finalize: 3 * classes + 1 fp32 planes and one label read, 4 bytes a pixel
written).  The legs alternate within one process, every shape is warmed up first; the figures are the medians of --rounds rounds, the
spread is their min and max.  One JSON line, also written to --out."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stcd_amd import _lib, synth
from stcd_amd.modules import frozen_weights
from stcd_amd.pseudo import MEAN, STD
from stcd_amd.scene import parse_tta, plan_tiles, predict_scene_heads
from stcd_amd.segcd import SegCD

ap = argparse.ArgumentParser(); ap.add_argument("--model", default="segcd", choices=("segcd",))
ap.add_argument("--encoder", default="resnet50", choices=("resnet50", "resnet18")); ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--tile", type=int, default=256); ap.add_argument("--stride", type=int, default=256); ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--tta", default="none", choices=("none", "flip", "d4")); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--kernel_reps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scene_heads_bench.json"))
a = ap.parse_args()
dev = "cuda:0"
S, T, ST, NB = a.size, a.tile, a.stride, a.batch
tta = None if a.tta == "none" else a.tta
views = parse_tta(tta)
torch.manual_seed(910)
model = SegCD(encoder_name=a.encoder, dtype="bf16").to(dev).eval()
small = 512                                                            # one synthetic block, tiled: the generator's box filter is host work
sa, sb, sl = synth.make_pairs_u8(1, small, small, seed=50)
reps = -(-S // small)
A = torch.from_numpy(np.tile(sa[0], (reps, reps, 1))[:S, :S].copy()).to(dev)
B = torch.from_numpy(np.tile(sb[0], (reps, reps, 1))[:S, :S].copy()).to(dev)
LAB = torch.from_numpy(np.tile(sl[0], (reps, reps))[:S, :S].copy()).to(dev)
plan = plan_tiles(S, S, T, ST)
l, vp = _lib.lib(), lambda t: None if t is None else C.c_void_p(t.data_ptr())
m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
x1 = torch.empty((NB, 3, T, T), dtype=torch.float32, device=dev)
x2 = torch.empty_like(x1)


def forwards(each):
    """The gathers and eval forwards of predict_scene_heads; `each(out, first, n, d4)` gets every batch's three maps."""
    with torch.no_grad(), frozen_weights(model):
        for d4 in views:
            for first in range(0, plan.n, NB):
                n = min(NB, plan.n - first)
                _lib.check(l.stcd_scene_gather_d4(vp(A), vp(B), S, S, T, ST, plan.tiles_x, first, n, m3, s3, vp(x1), vp(x2), d4, stream))
                each(model(x1[:n], x2[:n]), first, n, d4)


def leg_a():
    r = predict_scene_heads(model, A, B, tile=T, stride=ST, batch=NB, label=LAB, tta=tta)
    torch.cuda.synchronize()
    return r


def leg_b():
    pairs = []

    def each(out, first, n, d4):
        if not pairs:
            classes = out[0].shape[1]
            pairs.extend((torch.zeros((classes, S, S), dtype=torch.float32, device=dev), torch.zeros((S, S), dtype=torch.float32, device=dev))
                         for _ in range(3))
        for t, (acc, wsum) in zip(out, pairs):
            t = t.float().contiguous()
            _lib.check(l.stcd_scene_stitch_d4(vp(t), t.shape[1], S, S, T, ST, plan.tiles_x, plan.tiles_y, first, n, None, vp(acc), vp(wsum), d4, stream))

    forwards(each)
    masks = [torch.empty((S, S), dtype=torch.uint8, device=dev) for _ in range(3)]
    cm = torch.zeros(4, dtype=torch.int64, device=dev)
    for h, (acc, wsum) in enumerate(pairs):
        lab = LAB if h == 2 else None
        _lib.check(l.stcd_scene_finalize(vp(acc), vp(wsum), acc.shape[0], S, S, C.c_float(0.0), vp(lab), vp(masks[h]), None,
                                         vp(cm) if h == 2 else None, stream))
    gated = masks[2] & (masks[0] != masks[1]).to(torch.uint8)
    ok = LAB != 255
    gcm = torch.bincount(2 * (LAB[ok] >= 1).long() + gated[ok].long(), minlength=4)
    cms = (cm.cpu().numpy(), gcm.cpu().numpy())
    torch.cuda.synchronize()
    return masks, gated, cms


def leg_c():
    forwards(lambda out, first, n, d4: None)
    torch.cuda.synchronize()


def kernel_seconds(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.kernel_reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / a.kernel_reps


ra = leg_a(); masks, gated, cms = leg_b(); leg_c()                     # every shape and code path once, untimed
same = torch.equal(ra.seg_a, masks[0]) and torch.equal(ra.seg_b, masks[1]) and torch.equal(ra.change, masks[2]) and torch.equal(ra.gated, gated) \
    and np.array_equal(ra.cm["change"].ravel(), cms[0]) and np.array_equal(ra.cm["gated"].ravel(), cms[1])
legs = {"a": leg_a, "b": leg_b, "c": leg_c}
secs = {k: [] for k in legs}
for r in range(a.rounds):
    for k, fn in legs.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        secs[k].append(time.perf_counter() - t0)
med = {k: statistics.median(v) for k, v in secs.items()}
# the two entries themselves through ctypes, buffers and arguments prepared once: the host's enqueue cost bounds these from below
classes = 1
n = min(NB, plan.n)
heads = [torch.randn((n, classes, T, T), device=dev) for _ in range(3)]
acc = torch.zeros((3 * classes, S, S), dtype=torch.float32, device=dev)
wsum = torch.ones((S, S), dtype=torch.float32, device=dev)
out4 = torch.empty((4, S, S), dtype=torch.uint8, device=dev)
cm16 = torch.zeros((4, 4), dtype=torch.int64, device=dev)
ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in heads])
t_st = kernel_seconds(lambda: _lib.check(l.stcd_scene_stitch_heads_d4(ptrs, 3, classes, S, S, T, ST, plan.tiles_x, plan.tiles_y, 0, n, None, vp(acc),
                                                                      vp(wsum), 0, stream)))
t_st5 = kernel_seconds(lambda: _lib.check(l.stcd_scene_stitch_heads_d4(ptrs, 3, classes, S, S, T, ST, plan.tiles_x, plan.tiles_y, 0, n, None, vp(acc),
                                                                       vp(wsum), 5, stream)))
t_fin = kernel_seconds(lambda: _lib.check(l.stcd_scene_finalize_seg(vp(acc), vp(wsum), classes, S, S, C.c_float(0.0), C.c_float(0.0), None, None, vp(LAB),
                                                                    vp(out4[0]), vp(out4[1]), vp(out4[2]), vp(out4[3]), None, vp(cm16), stream)))
last = n - 1                                                           # the scene rectangle the batch's tiles reach, as the launch computes it
rows = min(S, (last // plan.tiles_x) * ST + T)
cols = S if last // plan.tiles_x > 0 else min(S, (last % plan.tiles_x) * ST + T)
st_bytes = 4 * (3 * classes * n * T * T + 2 * (3 * classes + 1) * rows * cols)
fin_bytes = S * S * (4 * (3 * classes + 1) + 1 + 4)
a_vs_b = med["a"] / med["b"]
line = json.dumps({"tool": "scene_heads_bench", "model": a.model, "encoder": a.encoder, "dtype": "bf16", "size": S, "tile": T, "stride": ST, "batch": NB,
                   "tta": a.tta, "views": len(views), "tiles": plan.n, "rounds": a.rounds, "all_routes_equal": bool(same),
                   "ms": {k: round(v * 1e3, 3) for k, v in med.items()},
                   "spread_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in secs.items()},
                   "a_over_b": round(a_vs_b, 4), "a_minus_c_ms": round((med["a"] - med["c"]) * 1e3, 3), "b_minus_c_ms": round((med["b"] - med["c"]) * 1e3, 3),
                   "verdict": "a beats b" if a_vs_b < 1.0 else "a does NOT beat b",
                   "kernels": {"classes": classes, "stitch_heads_tiles": n, "stitch_heads_d4_0_us": round(t_st * 1e6, 2),
                               "stitch_heads_d4_0_GBps": round(st_bytes / t_st * 1e-9, 1), "stitch_heads_d4_5_us": round(t_st5 * 1e6, 2),
                               "stitch_heads_d4_5_GBps": round(st_bytes / t_st5 * 1e-9, 1), "finalize_seg_us": round(t_fin * 1e6, 2),
                               "finalize_seg_GBps": round(fin_bytes / t_fin * 1e-9, 1),
                               "note": "back-to-back launches through the C ABI between two device events: per-launch time, not below the host's enqueue cost"},
                   "legs": {"a": "predict_scene_heads with the change label", "b": "3 x stcd_scene_stitch_d4 per batch, 3 x stcd_scene_finalize, gate and bincount in torch",
                            "c": "the gathers and the bare eval forwards"}})
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
