"""Training-step time of the three BIT configurations (bit_pos_s4, bit_pos_s4_dd8, bit_pos_s4_dd8_dedim8) beside their CNN baseline
with the same trunk (base_resnet18 with 4 stages) in ONE process, by tools/base_resnet_bench.py's method: bf16, FlatAdamW, the timed
region of bench.py (zero_grad, forward, loss, backward, fused optimizer step; wall clock over a window of steps between two
synchronisations, quiet_gc), the models alternated window by window, every one warmed up first; medians with min-max.

The token path's cost is the BIT step minus the base_resnet18_s4 step.  Its yardstick: tests/bit_spec.token_path -- the same
computation composed from torch ops -- forward + backward on the device on a tensor of conv_pred's shape [2 * batch, 32, size / 4,
size / 4], timed the same way in float32 and in bfloat16 (the faster of the two is the yardstick).  Beside it the decoder kernels'
own time from the engine's event instrumentation (the figures tools/kernel_table.py prints), against their byte floor: the forward
reads x and writes the output once plus the dec_depth - 1 stored layer inputs; the backward reads those, the output gradient, and
writes the input gradient once (the running gradient between layers: fp32).

    python tools/bit_bench.py [--batch 16] [--size 256] [--windows 5] [--steps 10] [--out profiles/bit_bench.json]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stcd_amd import synth
from stcd_amd.bit import BASE_Transformer, ResNet
from stcd_amd.losses import cross_entropy
from stcd_amd.optim import FlatAdamW
from stcd_amd.train_loop import quiet_gc
from tests import bit_spec as S

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--windows", type=int, default=5); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = "cuda:0"
x1, x2, lab = synth.make_batch(a.batch, a.size, a.size, seed=1337)
A, B, L = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev), torch.from_numpy(lab).to(dev)
CFG = {"bit_pos_s4": (1, 64), "bit_pos_s4_dd8": (8, 64), "bit_pos_s4_dd8_dedim8": (8, 8)}
models = {}


def build(name):
    torch.manual_seed(1)
    if name == "base_resnet18_s4":
        m = ResNet(3, 2, resnet_stages_num=4, dtype="bf16")
    else:
        m = BASE_Transformer(3, 2, "learned", resnet_stages_num=4, dec_depth=CFG[name][0], decoder_dim_head=CFG[name][1], dtype="bf16")
        m.load_state_dict(S.synth_state(*CFG[name], 2, 1))
    m = m.to(dev).train()
    models[name] = m
    opt = FlatAdamW(m, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)

    def step():
        opt.zero_grad(set_to_none=True)
        out = m(A, B)
        loss = cross_entropy(out[-1] if isinstance(out, list) else out, L)
        loss.backward()
        opt.step()
        return loss
    return step


def build_yardstick(name, dtype):
    dd, dh = CFG[name]
    st = {k: v.to(dev, dtype).requires_grad_(True) for k, v in S.synth_state(dd, dh, 2, 1).items()
          if k.startswith("transformer") or k in ("pos_embedding", "conv_a.weight")}
    g = torch.Generator(device="cpu").manual_seed(3)
    p = torch.randn(2 * a.batch, 32, a.size // 4, a.size // 4, generator=g).to(dev, dtype).requires_grad_(True)
    dy = torch.randn(2 * a.batch, 32, a.size // 4, a.size // 4, generator=g).to(dev, dtype)

    def step():
        for v in st.values():
            v.grad = None
        p.grad = None
        out = S.token_path(st, p)
        out.backward(dy)
        return out.float().sum()
    return step


names = ["base_resnet18_s4"] + list(CFG)
steps = {n: build(n) for n in names}
for n in CFG:
    for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        steps[f"torch_token_path_{tag}:{n}"] = build_yardstick(n, dt)
order = list(steps)
for n in order:
    for _ in range(a.warmup):
        steps[n]()
torch.cuda.synchronize()
ms = {n: [] for n in order}
with quiet_gc():
    for w in range(a.windows):
        for n in order:
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
med = {}
for n in order:
    v = sorted(ms[n])
    med[n] = v[len(v) // 2]
    res[n] = {"median_ms": round(med[n], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3)}
rows = 2.0 * a.batch * (a.size // 4) ** 2
for n, (dd, dh) in CFG.items():
    cost = med[n] - med["base_resnet18_s4"]
    yard = min(med[f"torch_token_path_fp32:{n}"], med[f"torch_token_path_bf16:{n}"])
    # the decoder kernels' own time: a few instrumented steps (events around every launch; not part of the timed windows)
    eng = models[n]._engine
    eng.profile_enable(True)
    for _ in range(3):
        steps[n]()
    torch.cuda.synchronize()
    k = eng.profile_kernels()
    eng.profile_enable(False)
    kern = {}
    for kn in ("k_bit_dec_fwd", "k_bit_dec_bwd", "k_bit_tok_fwd", "k_bit_tok_bwd"):
        r = k.get(kn)
        if r and r["launches"]:
            t = r["ms"] / r["launches"]
            kern[kn] = {"ms": round(t, 4), "gb_per_s": round(r["bytes"] / r["launches"] / t / 1e6, 1), "tflops": round(r["flops"] / r["launches"] / t / 1e9, 2)}
    floor_bytes = rows * 32 * 2 * ((dd + 1) + (dd + 2)) + rows * 32 * 8 * (dd - 1)
    res[n].update({"token_path_ms": round(cost, 3), "torch_yardstick_ms": round(yard, 3), "yardstick_over_token_path": round(yard / cost, 2),
                   "kernels": kern, "decoder_byte_floor_mb": round(floor_bytes / 1e6, 1)})
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
