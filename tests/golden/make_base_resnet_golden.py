#!/usr/bin/env python3
"""Generate tests/golden/g24_base_resnet_*.npz from the REFERENCE's own ``ResNet`` class (models/networks.py:223-304, the network
``define_G("base_resnet18")`` builds).

Run in the authoring container only (needs /root/reference, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_base_resnet_golden.py

models/networks.py cannot be imported (it pulls in timm), so the class definition is compiled from the file by ``ast`` (as
make_golden.py does for other classes) and handed ``torch``, ``nn``, the importable ``models.help_funcs.TwoLayerConv2d`` and a
``models`` namespace whose resnet18 / resnet34 call the reference's own models.resnet functions with ``pretrained=False`` FORCED:
the class hard-wires ``pretrained=True``, which would fetch a checkpoint -- that call is never reached here.

The fixtures hold DATA only: inputs, a target, outputs, the loss, gradient summaries / samples (tests/_util.gf_index) and a few
BatchNorm buffers.  Weights are not stored: generator and tests rebuild them from tests/base_resnet_spec.synth_state's seed.
Expected values come from the reference run in float64 (stored as float32: 6e-8 relative).  The reference is run once more in
float32, and the script ASSERTS that this run stays within rel-l2 <= 2.5e-2 / cosine >= 0.999 of the float64 one for every gradient
tensor a test compares -- half the tests' bound (5e-2 / 0.998) --, and that its logits use at most half (eval: a quarter) of the tests' rtol = atol =
1e-3, so a fixture cannot be conditioned worse than the bound it is used with.  A shape that fails this gets another seed, never
another bound (resnet34 at 1 x 32 x 32: seed 2403 gave eval maps of scale 80, on which the fp32 engine's sequential accumulation
left 3 of 2048 logits 2e-3 off).  The same holds for
the bf16 test: the reference with bf16 storage emulated must use at most 3/4 of ITS bounds (resnet34 at 1 x 32 x 32, 16 values per
trunk BatchNorm: seed 2406 moved the training loss by 6e-2 that way, 2408 is the next seed that passes every assertion).
"""
import ast
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(1, "/root/reference")
sys.dont_write_bytecode = True

import numpy as np                                      # noqa: E402
import torch                                            # noqa: E402
import torch.nn as nn                                   # noqa: E402
import torch.nn.functional as F                         # noqa: E402

from models import resnet as ref_resnet                 # noqa: E402  (reference)
from models.help_funcs import TwoLayerConv2d            # noqa: E402  (reference)

from tests import base_resnet_spec as S                 # noqa: E402  (only for synth_state)
from tests._util import gf_index, rel_l2_cos            # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
COND_REL, COND_COS = 2.5e-2, 0.999
RS_BN = {"resnet18": ("resnet.bn1", "resnet.layer3.0.downsample.1", None, "classifier.1"),
         "resnet34": ("resnet.bn1", "resnet.layer2.0.downsample.1", None, "classifier.1")}
torch.set_num_threads(8)


def reference_class():
    path = "/root/reference/models/networks.py"
    node = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.ClassDef) and n.name == "ResNet"]
    assert len(node) == 1

    def no_download(fn):
        def build(pretrained=True, **kw):
            return fn(pretrained=False, **kw)          # never pretrained=True: no checkpoint is fetched
        return build

    models = types.SimpleNamespace(resnet18=no_download(ref_resnet.resnet18), resnet34=no_download(ref_resnet.resnet34))
    ns = {"torch": torch, "nn": nn, "TwoLayerConv2d": TwoLayerConv2d, "models": models}
    exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), ns)
    return ns["ResNet"]


def t2n(t):
    return t.detach().cpu().numpy().copy()


def fixture(fname, backbone, stages, B, H, W, seed):
    print(f"G24 {fname}: {backbone}, resnet_stages_num {stages}, {B} x {H} x {W}, seed {seed}")
    Ref = reference_class()
    rng = np.random.default_rng(seed)
    x1 = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    # the second date: independent of the first and twice its amplitude, so that |x1 - x2| is as large as the maps it is formed from.
    # With strongly correlated dates (x2 = x1 + 0.5 n was tried first) the differencing cancels a common part 4 - 6 x the difference, and
    # bf16 STORAGE alone -- measured below on the reference, no engine involved -- moves the eval logits by 5.7e-2 / 7.9e-2 / 6.1e-2:
    # beyond the bf16 test's bound, which was taken from maps that no differencing precedes (DESIGN.md section 4 has the figures)
    x2 = (2.0 * rng.standard_normal((B, 3, H, W))).astype(np.float32)
    target = (rng.random((B, H, W)) < 0.3).astype(np.int64)
    last_bn = "resnet.layer{}.{}.bn2".format(stages - 1, S.BLOCKS[backbone][stages - 2] - 1)
    watch = [b if b else last_bn for b in RS_BN[backbone]]

    def run(dtype):
        out = {}
        m = Ref(input_nc=3, output_nc=2, resnet_stages_num=stages, backbone=backbone, output_sigmoid=False)
        assert list(m.state_dict()) == [n for n, _, _ in S.param_specs(backbone, stages, 2)]
        m.load_state_dict(S.synth_state(backbone, stages, 2, seed, perturb_running=True))
        m.to(dtype).eval()
        a, b = torch.from_numpy(x1).to(dtype), torch.from_numpy(x2).to(dtype)
        with torch.no_grad():
            out["eval/logits"] = t2n(m(a, b))
        m.load_state_dict(S.synth_state(backbone, stages, 2, seed))
        m.to(dtype).train()
        logits = m(a, b)
        loss = F.cross_entropy(logits, torch.from_numpy(target))
        loss.backward()
        out["train/logits"], out["loss"] = t2n(logits), loss.item()
        out["grads"] = {n: (None if p.grad is None else t2n(p.grad)) for n, p in m.named_parameters()}
        sd = m.state_dict()
        for bn in watch:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                out[f"rs/{bn}.{k}"] = t2n(sd[f"{bn}.{k}"])
        return out

    r64, r32 = run(torch.float64), run(torch.float32)
    # conditioning for the bf16 test: the reference itself with bf16 STORAGE emulated (conv filters, the inputs and every module's
    # output rounded to bf16, arithmetic in float32 -- where the engine's bf16 mode rounds) must use at most 3/4 of that test's bounds
    # (eval logits rel-l2 <= 4e-2, loss within 2e-2 relative); the engine differs from this emulation by summation order only
    q = lambda x: x.to(torch.bfloat16).float()

    def bf16_storage(perturb, training):
        m = Ref(input_nc=3, output_nc=2, resnet_stages_num=stages, backbone=backbone, output_sigmoid=False)
        m.load_state_dict(S.synth_state(backbone, stages, 2, seed, perturb_running=perturb))
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, nn.Conv2d):
                    mod.weight.copy_(q(mod.weight))
        for mod in m.modules():
            if isinstance(mod, (nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d, nn.Upsample)):
                mod.register_forward_hook(lambda _m, _i, o: q(o))
        m.train(training)
        with torch.no_grad():
            return m(q(torch.from_numpy(x1)), q(torch.from_numpy(x2)))
    e_eval = rel_l2_cos(bf16_storage(True, False).numpy(), r64["eval/logits"])[0]
    e_loss = abs(F.cross_entropy(bf16_storage(False, True), torch.from_numpy(target)).item() - r64["loss"]) / abs(r64["loss"])
    print(f"  reference with bf16 storage vs float64: eval logits rel-l2 {e_eval:.2e} (bf16 test: 4e-2), loss {e_loss:.2e} relative (2e-2)")
    assert e_eval <= 0.75 * 4e-2 and e_loss <= 0.75 * 2e-2, f"{fname}: bf16 storage alone uses more than 3/4 of the bf16 test's bounds: change the seed"
    unused = sorted(n for n, g in r64["grads"].items() if g is None)
    want_unused = ["resnet.fc.bias", "resnet.fc.weight"] + ([n for n, _, k in S.param_specs(backbone, stages, 2)
                                                              if n.startswith("resnet.layer4.") and k in ("conv", "bn_w", "bn_b")] if stages == 4 else [])
    assert unused == sorted(want_unused), unused
    # conditioning: the reference against itself at the tests' working precision
    worst = (0.0, 1.0, "")
    for n, g in r64["grads"].items():
        if g is None:
            continue
        if n == "conv_pred.bias":      # cancels in x1 - x2: an exactly zero gradient by construction, nothing to condition
            assert float(np.abs(g).max()) < 1e-12 and float(np.abs(r32["grads"][n]).max()) < 1e-6
            continue
        rel, cos = rel_l2_cos(r32["grads"][n], g)
        if rel > worst[0]:
            worst = (rel, min(worst[1], cos), n)
        assert rel <= COND_REL and cos >= COND_COS, f"{fname}: the reference's float32 gradient of {n} is {rel:.2e} / {cos:.6f} from its float64 one: change the seed"
    # ... and the logits: the float32 run uses at most half of the tests' rtol = atol = 1e-3 (eval-mode maps with perturbed running
    # statistics are not normalised: a state whose maps grow large makes the ABSOLUTE part of that bound meaningless)
    for k in ("eval/logits", "train/logits"):
        use = float((np.abs(r32[k] - r64[k]) / (1e-3 + 1e-3 * np.abs(r64[k]))).max())
        print(f"  reference float32 vs float64 {k}: {use:.2f} of the tests' bound, map scale {float(np.abs(r64[k]).max()):.1f}")
        # eval: a quarter -- nothing re-normalises the eval maps, and torch's blocked float32 sums are ~sqrt(K) / log2(K) (~5 x at
        # K = 9 x 512) tighter than a kernel that accumulates the K products in sequence, as the engine's fp32 mode does
        room = 0.25 if k.startswith("eval") else 0.5
        assert use <= room, f"{fname}: {k} of the reference's float32 run uses {use:.2f} of the bound (room {room}): change the seed"
    dl = float(np.abs(r32["train/logits"] - r64["train/logits"]).max())
    print(f"  reference float32 vs float64: worst gradient rel-l2 {worst[0]:.2e} ({worst[2]}), logits {dl:.1e}, loss {abs(r32['loss'] - r64['loss']):.1e}")
    d = {"x1": x1, "x2": x2, "target": target, "seed": np.int64(seed), "stages": np.int64(stages), "loss": np.float64(r64["loss"]),
         "eval/logits": r64["eval/logits"].astype(np.float32), "train/logits": r64["train/logits"].astype(np.float32)}
    for n, g in r64["grads"].items():
        g = np.zeros(1) if g is None else g.ravel().astype(np.float64)
        k = g.size
        idx = (np.arange(24) * max(k // 24, 1)) % k
        d["gs/" + n] = np.concatenate([[g.sum(), np.linalg.norm(g)], g[:8] if k >= 8 else np.pad(g, (0, 8 - k)), g[idx]])
        if r64["grads"][n] is not None:
            d["gf/" + n] = g[gf_index(n, k)].astype(np.float32)
    for k, v in r64.items():
        if k.startswith("rs/"):
            d[k] = v.astype(np.float32) if v.dtype.kind == "f" else v
    path = os.path.join(OUT, fname)
    np.savez_compressed(path, **d)
    print(f"  wrote {fname}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    fixture("g24_base_resnet_r18_s5.npz", "resnet18", 5, 2, 64, 64, 2401)
    fixture("g24_base_resnet_r18_s4.npz", "resnet18", 4, 3, 32, 64, 2402)
    fixture("g24_base_resnet_r34_s5.npz", "resnet34", 5, 1, 32, 32, 2408)
