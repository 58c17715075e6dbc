"""Training-step time of Siam_NestedUNet_Conc (fused map, and deep supervision) beside SNUNet_ECAM in ONE process: bf16,
cross_entropy + FlatAdamW, the timed region of bench.py (zero_grad, forward, loss, backward, fused optimizer step; wall clock over
a window of steps between two synchronisations, quiet_gc).  The three models are alternated window by window, every one warmed up
first; the result is the median over the windows with min-max beside it.

    python tools/snunet_conc_bench.py [--batch 16] [--size 256] [--windows 5] [--steps 20] [--out profiles/snunet_conc_bench.json]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stcd_amd import modules, synth
from stcd_amd.losses import cross_entropy
from stcd_amd.optim import FlatAdamW
from stcd_amd.train_loop import quiet_gc

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--windows", type=int, default=5); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = "cuda:0"
WEIGHTS = (0.5, 0.5, 0.5, 0.8, 1.0)
x1, x2, lab = synth.make_batch(a.batch, a.size, a.size, seed=1337)
A, B, L = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev), torch.from_numpy(lab).to(dev)


def build(name):
    torch.manual_seed(1)
    if name == "snunet":
        m = modules.SNUNet_ECAM(3, 2, dtype="bf16")
    else:
        m = modules.Siam_NestedUNet_Conc(3, 2, dtype="bf16", deep_supervision=name == "snunet_conc_ds")
    m = m.to(dev).train()
    opt = FlatAdamW(m, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)

    def step():
        opt.zero_grad(set_to_none=True)
        out = m(A, B)
        if isinstance(out, list):      # deep supervision: CDTrainer's multi-scale loss
            loss = sum(w * cross_entropy(p, L) for w, p in zip(WEIGHTS, out))
        else:
            loss = cross_entropy(out, L)
        loss.backward()
        opt.step()
        return loss
    return step


names = ("snunet", "snunet_conc", "snunet_conc_ds")
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
    res[n] = {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3),
              "pairs_per_s": round(a.batch / v[len(v) // 2] * 1e3, 1)}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
