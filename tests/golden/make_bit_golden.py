#!/usr/bin/env python3
"""Generate tests/golden/g25_bit_*.npz from the REFERENCE's own ``BASE_Transformer`` class (models/networks.py:307-441, the network
``define_G("base_transformer_pos_s4*")`` builds).

Run in the authoring container only (needs /root/reference, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bit_golden.py

As make_base_resnet_golden.py: models/networks.py cannot be imported (it pulls in timm), so the class definitions ``ResNet`` and
``BASE_Transformer`` are compiled from the file by ``ast`` and handed ``torch``, ``nn``, ``F``, ``rearrange``, the importable
``models.help_funcs`` classes and a ``models`` namespace whose resnet18 calls the reference's own function with ``pretrained=False``
FORCED (the class hard-wires ``pretrained=True``, which would fetch a checkpoint -- that call is never reached here).

The fixtures hold DATA only: inputs, a target, outputs, the loss, gradient summaries / samples (tests/bit_spec.fixture_index) and a few
BatchNorm buffers.  Weights are not stored: generator and tests rebuild them from tests/bit_spec.synth_state's seed.  Expected values
come from the reference run in float64 (stored as float32).  The script ASSERTS, and a seed that fails is replaced, never a bound:

  * the state_dict order (pos_embedding first, then ResNet's keys, conv_a, transformer, transformer_decoder; 158 keys for dec_depth 1);
  * which gradients are None (resnet.fc.*, resnet.layer4.*) and that the LAST decoder layer's net.3.bias gradient is exactly zero
    (it is added to both dates and cancels in x1 - x2) while conv_pred.bias' no longer is;
  * that the softmaxes are not flat on these inputs: decoder layer 0 mean(max_j p * 4) >= 1.5, tokenizer mean(max_n a * n) >= 2;
  * the reference's own float32 run uses <= 1/2 (train) / 1/4 (eval) of the tests' logits bound (rtol = atol = 1e-3) and <= 1/2 of the
    gradient bound (rel-l2 5e-2 / cosine 0.998);
  * the reference with bf16 STORAGE emulated where the engine's bf16 mode stores (conv filters, inputs, the output of every trunk /
    classifier module and of every decoder layer; conv_a, the tokens and the encoder stay float32) uses <= 3/4 of the bf16 test's
    bounds (eval logits rel-l2 4e-2, loss 2e-2 relative).
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
from einops import rearrange                            # noqa: E402

from models import help_funcs as ref_help               # noqa: E402  (reference)
from models import resnet as ref_resnet                 # noqa: E402  (reference)

from tests import bit_spec as S                         # noqa: E402  (synth_state; the softmax condition on the inputs)
from tests._util import rel_l2_cos            # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
COND_REL, COND_COS = 2.5e-2, 0.999
WATCH_BN = ("resnet.bn1", "resnet.layer3.0.downsample.1", "resnet.layer3.1.bn2", "classifier.1")
torch.set_num_threads(8)


def reference_class():
    path = "/root/reference/models/networks.py"
    nodes = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.ClassDef) and n.name in ("ResNet", "BASE_Transformer")]
    assert [n.name for n in nodes] == ["ResNet", "BASE_Transformer"]

    def no_download(fn):
        def build(pretrained=True, **kw):
            return fn(pretrained=False, **kw)          # never pretrained=True: no checkpoint is fetched
        return build

    models = types.SimpleNamespace(resnet18=no_download(ref_resnet.resnet18), resnet34=no_download(ref_resnet.resnet34))
    ns = {"torch": torch, "nn": nn, "F": F, "rearrange": rearrange, "models": models, "TwoLayerConv2d": ref_help.TwoLayerConv2d,
          "Transformer": ref_help.Transformer, "TransformerDecoder": ref_help.TransformerDecoder}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns["BASE_Transformer"]


def t2n(t):
    return t.detach().cpu().numpy().copy()


def fixture(fname, dd, dh, B, H, W, seed):
    print(f"G25 {fname}: dec_depth {dd}, decoder_dim_head {dh}, {B} x {H} x {W}, seed {seed}")
    Ref = reference_class()
    rng = np.random.default_rng(seed)
    x1 = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    x2 = (2.0 * rng.standard_normal((B, 3, H, W))).astype(np.float32)      # independent dates: see make_base_resnet_golden.py
    target = (rng.random((B, H, W)) < 0.3).astype(np.int64)
    specs = S.param_specs(dd, dh, 2)
    last_b = f"transformer_decoder.layers.{dd - 1}.1.fn.fn.net.3.bias"

    def build():
        return Ref(input_nc=3, output_nc=2, token_len=4, resnet_stages_num=4, with_pos="learned", enc_depth=1, dec_depth=dd, decoder_dim_head=dh)

    def run(dtype):
        out = {}
        m = build()
        keys = list(m.state_dict())
        assert keys == [n for n, _, _ in specs] and keys[:2] == ["pos_embedding", "resnet.conv1.weight"]
        assert dd != 1 or len(keys) == 158
        for n, shape, _ in specs:
            assert tuple(m.state_dict()[n].shape) == tuple(shape), n
        m.load_state_dict(S.synth_state(dd, dh, 2, seed, perturb_running=True))
        m.to(dtype).eval()
        a, b = torch.from_numpy(x1).to(dtype), torch.from_numpy(x2).to(dtype)
        with torch.no_grad():
            o = m(a, b)
            assert isinstance(o, list) and len(o) == 1
            out["eval/logits"] = t2n(o[0])
        m.load_state_dict(S.synth_state(dd, dh, 2, seed))
        m.to(dtype).train()
        cap = {}
        hk = m.conv_pred.register_forward_hook(lambda _m, _i, o: cap.setdefault("p", []).append(o.detach()))
        logits = m(a, b)[0]
        hk.remove()
        loss = F.cross_entropy(logits, torch.from_numpy(target))
        loss.backward()
        out["train/logits"], out["loss"] = t2n(logits), loss.item()
        out["grads"] = {n: (None if p.grad is None else t2n(p.grad)) for n, p in m.named_parameters()}
        out["conv_pred"] = torch.cat(cap["p"], dim=0)
        out["tokens"] = m.tokens.detach()
        sd = m.state_dict()
        for bn in WATCH_BN:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                out[f"rs/{bn}.{k}"] = t2n(sd[f"{bn}.{k}"])
        return out

    r64, r32 = run(torch.float64), run(torch.float32)
    # ---- the inputs of the token path must exercise its softmaxes (spec functions on the reference's own conv_pred maps / tokens)
    st64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in S.synth_state(dd, dh, 2, seed).items()}
    with torch.no_grad():
        p = r64["conv_pred"]
        _, a_tok = S.tokenizer(st64, p, return_attention=True)
        enc = r64["tokens"]
        mem = torch.cat([enc[:, :4], enc[:, 4:]], dim=0)
        _, a_dec = S.decoder(st64, p.flatten(2).transpose(1, 2), mem, return_attention=True)
    peak_tok = float((a_tok.max(dim=-1).values * a_tok.shape[-1]).mean())
    peak_dec = float((a_dec.max(dim=-1).values * 4).mean())
    print(f"  softmax peaks: tokenizer mean(max * n) {peak_tok:.2f} (>= 2), decoder layer 0 mean(max * 4) {peak_dec:.2f} (>= 1.5)")
    assert peak_tok >= 2.0 and peak_dec >= 1.5, f"{fname}: flat softmax on these inputs: change the seed"

    # ---- bf16 storage emulated on the reference, where the engine's bf16 mode rounds
    q = lambda x: x.to(torch.bfloat16).float()

    def bf16_storage(perturb, training):
        m = build()
        m.load_state_dict(S.synth_state(dd, dh, 2, seed, perturb_running=perturb))
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, nn.Conv2d) and mod is not m.conv_a:
                    mod.weight.copy_(q(mod.weight))
        for mod in m.modules():
            if isinstance(mod, (nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d, nn.Upsample)) and mod is not m.conv_a:
                mod.register_forward_hook(lambda _m, _i, o: q(o))
        for layer in m.transformer_decoder.layers:
            layer[1].register_forward_hook(lambda _m, _i, o: q(o))
        m.train(training)
        with torch.no_grad():
            return m(q(torch.from_numpy(x1)), q(torch.from_numpy(x2)))[0]
    e_eval = rel_l2_cos(bf16_storage(True, False).numpy(), r64["eval/logits"])[0]
    e_loss = abs(F.cross_entropy(bf16_storage(False, True), torch.from_numpy(target)).item() - r64["loss"]) / abs(r64["loss"])
    print(f"  reference with bf16 storage vs float64: eval logits rel-l2 {e_eval:.2e} (bf16 test: 4e-2), loss {e_loss:.2e} relative (2e-2)")
    assert e_eval <= 0.75 * 4e-2 and e_loss <= 0.75 * 2e-2, f"{fname}: bf16 storage alone uses more than 3/4 of the bf16 test's bounds: change the seed"

    unused = sorted(n for n, g in r64["grads"].items() if g is None)
    want_unused = ["resnet.fc.bias", "resnet.fc.weight"] + [n for n, _, k in specs if n.startswith("resnet.layer4.") and k in ("conv", "bn_w", "bn_b")]
    assert unused == sorted(want_unused), unused
    assert float(np.abs(r64["grads"][last_b]).max()) < 1e-12 and float(np.abs(r32["grads"][last_b]).max()) < 1e-5
    assert float(np.abs(r64["grads"]["conv_pred.bias"]).max()) > 1e-6
    worst = (0.0, 1.0, "")
    for n, g in r64["grads"].items():
        if g is None or n == last_b:
            continue
        rel, cos = rel_l2_cos(r32["grads"][n], g)
        if rel > worst[0]:
            worst = (rel, min(worst[1], cos), n)
        assert rel <= COND_REL and cos >= COND_COS, f"{fname}: the reference's float32 gradient of {n} is {rel:.2e} / {cos:.6f} from its float64 one: change the seed"
    for k in ("eval/logits", "train/logits"):
        use = float((np.abs(r32[k] - r64[k]) / (1e-3 + 1e-3 * np.abs(r64[k]))).max())
        print(f"  reference float32 vs float64 {k}: {use:.3f} of the tests' bound, map scale {float(np.abs(r64[k]).max()):.1f}")
        room = 0.25 if k.startswith("eval") else 0.5
        assert use <= room, f"{fname}: {k} of the reference's float32 run uses {use:.2f} of the bound (room {room}): change the seed"
    print(f"  reference float32 vs float64: worst gradient rel-l2 {worst[0]:.2e} ({worst[2]}), loss {abs(r32['loss'] - r64['loss']):.1e}")
    d = {"x1": x1, "x2": x2, "target": target, "seed": np.int64(seed), "dec_depth": np.int64(dd), "decoder_dim_head": np.int64(dh),
         "loss": np.float64(r64["loss"]), "eval/logits": r64["eval/logits"].astype(np.float32), "train/logits": r64["train/logits"].astype(np.float32),
         "peaks": np.array([peak_tok, peak_dec]), "bf16_storage": np.array([e_eval, e_loss])}
    for n, g in r64["grads"].items():
        g = np.zeros(1) if g is None else g.ravel().astype(np.float64)
        k = g.size
        idx = (np.arange(24) * max(k // 24, 1)) % k
        d["gs/" + n] = np.concatenate([[g.sum(), np.linalg.norm(g)], g[:8] if k >= 8 else np.pad(g, (0, 8 - k)), g[idx]])
        if r64["grads"][n] is not None:
            d["gf/" + n] = g[S.fixture_index(n, k)].astype(np.float32)
    for k, v in r64.items():
        if k.startswith("rs/"):
            d[k] = v.astype(np.float32) if v.dtype.kind == "f" else v
    path = os.path.join(OUT, fname)
    np.savez_compressed(path, **d)
    print(f"  wrote {fname}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    fixture("g25_bit_s4.npz", 1, 64, 2, 64, 64, 2501)
    fixture("g25_bit_s4_dd8.npz", 8, 64, 3, 32, 64, 2502)
    fixture("g25_bit_s4_dd8_dedim8.npz", 8, 8, 1, 32, 32, 2503)
