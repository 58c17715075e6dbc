"""Training-step time of ResNet (define_G name "base_resnet18", the BIT family's CNN baseline) with 5 and with 4 stages beside
SegCD(resnet18) -- the same BasicBlock kernels serve both -- in ONE process: bf16, FlatAdamW, the timed region of bench.py
(zero_grad, forward, loss, backward, fused optimizer step; wall clock over a window of steps between two synchronisations,
quiet_gc).  The models are alternated window by window, every one warmed up first; the result is the median over the windows with
min-max beside it, pairs/s, and the achieved algorithmic TFLOP/s: 2 x MACs of every convolution, computed here from the shapes, for
forward + weight gradient + data gradient (the stem has no data gradient).

    python tools/base_resnet_bench.py [--batch 16] [--size 256] [--windows 5] [--steps 20] [--out profiles/base_resnet_bench.json]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stcd_amd import synth
from stcd_amd.bit import ResNet
from stcd_amd.losses import bce_dice_with_logits, cross_entropy
from stcd_amd.optim import FlatAdamW
from stcd_amd.segcd import SegCD
from stcd_amd.train_loop import quiet_gc

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--windows", type=int, default=5); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = "cuda:0"
x1, x2, lab = synth.make_batch(a.batch, a.size, a.size, seed=1337)
A, B, L = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev), torch.from_numpy(lab).to(dev)
L1 = L.float().unsqueeze(1)


def trunk_macs(hw, strides, nstage, blocks=(2, 2, 2, 2)):
    """(MACs of one image through the stem and `nstage` BasicBlock stages, MACs of the stem alone, output pixels, output channels,
    [(pixels, channels)] of the stem and every stage); hw = input pixels."""
    px = hw // 4
    stem = px * 49 * 3 * 64
    macs, feats = stem, [(px, 64)]
    px //= 4                                             # max-pool
    cin = 64
    for li in range(nstage):
        c = (64, 128, 256, 512)[li]
        for b in range(blocks[li]):
            s = strides[li] if b == 0 else 1
            px //= s * s
            macs += px * 9 * cin * c + px * 9 * c * c
            if b == 0 and (s != 1 or cin != c):
                macs += px * cin * c
            cin = c
        feats.append((px, cin))
    return macs, stem, px, cin, feats


def gflop_per_pair(name, hw):
    if name == "segcd_resnet18":
        macs, stem, px, c, feats = trunk_macs(hw, (1, 2, 2, 2), 4)
        skips = feats[:-1][::-1] + [(0, 0)]              # f4, f3, f2, f1, none
        for i, cout in enumerate((256, 128, 64, 32, 16)):
            px *= 4
            macs += px * 9 * (c + skips[i][1]) * cout + px * 9 * cout * cout
            c = cout
        fwd, first = 2 * macs + 3 * hw * 9 * 16, 2 * stem          # two dates; the head runs on 3 maps per pair (one class)
    else:
        nstage = 4 if name.endswith("s5") else 3
        macs, stem, px, c, _ = trunk_macs(hw, (1, 2, 1, 1), nstage)
        macs += 4 * px * 9 * c * 32                      # conv_pred on the nearest x2 map
        fwd, first = 2 * macs + hw * 9 * 32 * 32 + hw * 9 * 32 * 2, 2 * stem
    return 2.0 * (3 * fwd - first) / 1e9, 2.0 * fwd / 1e9


def build(name):
    torch.manual_seed(1)
    if name == "segcd_resnet18":
        m = SegCD(encoder_name="resnet18", dtype="bf16")
    else:
        m = ResNet(3, 2, resnet_stages_num=int(name[-1]), dtype="bf16")
    m = m.to(dev).train()
    opt = FlatAdamW(m, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)

    def step():
        opt.zero_grad(set_to_none=True)
        out = m(A, B)
        loss = bce_dice_with_logits(out[2], L1) if isinstance(out, tuple) else cross_entropy(out, L)
        loss.backward()
        opt.step()
        return loss
    return step


names = ("base_resnet18_s5", "base_resnet18_s4", "segcd_resnet18")
steps = {n: build(n) for n in names}
for n in names:
    for _ in range(a.warmup):
        steps[n]()
torch.cuda.synchronize()
ms = {n: [] for n in names}
with quiet_gc():
    for w in range(a.windows):
        for n in names:
            steps[n]()                   # the other models ran in between: one step outside the window
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = steps[n]()
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / a.steps * 1e3)
            assert torch.isfinite(loss).item(), n
res = {"batch": a.batch, "size": a.size, "dtype": "bf16", "windows": a.windows, "steps_per_window": a.steps,
       "device": torch.cuda.get_device_name(0)}
for n in names:
    v = sorted(ms[n])
    med = v[len(v) // 2]
    train_gf, fwd_gf = gflop_per_pair(n, a.size * a.size)
    res[n] = {"median_ms": round(med, 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3), "pairs_per_s": round(a.batch / med * 1e3, 1),
              "algorithmic_gflop_per_pair_step": round(train_gf, 2), "algorithmic_gflop_per_pair_forward": round(fwd_gf, 2),
              "achieved_algorithmic_tflops": round(train_gf * a.batch / med, 1)}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
