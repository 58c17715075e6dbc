#!/usr/bin/env python3
"""Generate tests/golden/g23_snunet_conc_*.npz from the REFERENCE's own Siam_NestedUNet_Conc (models/SNUNet.py:155-243).

Run in the authoring container only (needs /root/reference, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_snunet_conc_golden.py

Data only, as make_golden.py: inputs, outputs, losses, gradient summaries ("gs/") and samples ("gf/", tests/_util.gf_index),
and the ordered state_dict keys / shapes.  Weights are rebuilt by generator and tests from tests.snunet_conc_spec.synth_state.

  g23_snunet_conc_{1,2}.npz   the G2 recipe: pair [2,3,32,32], eval logits (perturbed running statistics), train step
  g23_snunet_conc_ds_2.npz    the same train step with forward hooks on final1..4: five maps, weighted loss, gradients
  g23_snunet_conc_128.npz     the G7 recipe: train step at [2,3,128,128]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(1, "/root/reference")
sys.dont_write_bytecode = True

import numpy as np
import torch

from models.SNUNet import Siam_NestedUNet_Conc      # noqa: E402  (reference)
from models import losses as ref_losses             # noqa: E402

from tests import snunet_conc_spec as spec          # noqa: E402  (only for synth_state / DS_WEIGHTS)
from tests._util import gf_index                    # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)


def save(name, **arrs):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print(f"  wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def t2n(t):
    return t.detach().cpu().numpy().copy()


def grad_summary(model):
    out = {}
    for name, p in model.named_parameters():
        g = p.grad.detach().flatten().double()
        n = g.numel()
        idx = (np.arange(24) * max(n // 24, 1)) % n
        out["gs/" + name] = np.concatenate([[g.sum().item(), g.norm().item()], t2n(g[:8]) if n >= 8 else np.pad(t2n(g), (0, 8 - n)),
                                            t2n(g[idx])])
        out["gf/" + name] = t2n(p.grad).ravel()[gf_index(name, n)]
    return out


def rand_pair(seed, n, h, w):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    b = (a + 0.5 * rng.standard_normal((n, 3, h, w))).astype(np.float32)
    return torch.from_numpy(a), torch.from_numpy(b)


def layout(model):
    sd = model.state_dict()
    keys = list(sd.keys())
    shapes = np.full((len(keys), 4), -1, dtype=np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    return {"sd_keys": np.array(keys, dtype="U64"), "sd_shapes": shapes,
            "n_params": sum(p.numel() for p in model.parameters())}


def running_stats(model):
    d = {}
    sd = model.state_dict()
    for k in ("conv0_0.bn1", "conv3_0.bn2", "conv4_0.bn1", "conv0_4.bn2"):
        d[f"rs/{k}.running_mean"] = t2n(sd[f"{k}.running_mean"])
        d[f"rs/{k}.running_var"] = t2n(sd[f"{k}.running_var"])
        d[f"rs/{k}.num_batches_tracked"] = t2n(sd[f"{k}.num_batches_tracked"])
    return d


def g2():
    for label in (1, 2):
        print(f"G23 snunet_conc label={label}")
        seed = 2300 + label
        d = {"seed": seed, "label": label}
        x1, x2 = rand_pair(seed + 1, 2, 32, 32)
        d["x1"], d["x2"] = t2n(x1), t2n(x2)
        m = Siam_NestedUNet_Conc(3, label)
        d.update(layout(m))
        m.load_state_dict(spec.synth_state(3, label, seed, perturb_running=True))
        m.eval()
        with torch.no_grad():
            d["logits_eval"] = t2n(m(x1, x2))
        m = Siam_NestedUNet_Conc(3, label)
        m.load_state_dict(spec.synth_state(3, label, seed))
        m.train()
        logits = m(x1, x2)
        rng = np.random.default_rng(seed + 4)
        tgt = torch.from_numpy((rng.random((2, 32, 32)) < 0.2).astype(np.int64))
        d["target"] = t2n(tgt)
        if label == 2:
            loss = ref_losses.cross_entropy(logits, tgt)
        else:
            loss = ref_losses.cd_loss(torch.sigmoid(logits), tgt.float().unsqueeze(1))
        loss.backward()
        d["logits_train"], d["loss"] = t2n(logits), loss.item()
        d.update(grad_summary(m))
        d.update(running_stats(m))
        save(f"g23_snunet_conc_{label}.npz", **d)


def g2_ds():
    """Deep supervision: output1..4 exist inside the reference's forward (SNUNet.py:238-241); forward hooks hand them out attached
    to the graph, and the loss is CDTrainer's multi-scale sum (trainer.py:300-309) with multi_pred_weights (0.5, 0.5, 0.5, 0.8, 1)."""
    print("G23 snunet_conc deep supervision label=2")
    label, seed = 2, 2302           # the state, pair and target of g23_snunet_conc_2.npz
    d = {"seed": seed, "label": label, "weights": np.asarray(spec.DS_WEIGHTS)}
    x1, x2 = rand_pair(seed + 1, 2, 32, 32)
    d["x1"], d["x2"] = t2n(x1), t2n(x2)
    m = Siam_NestedUNet_Conc(3, label)
    m.load_state_dict(spec.synth_state(3, label, seed))
    m.train()
    side = {}
    for k in (1, 2, 3, 4):
        getattr(m, f"final{k}").register_forward_hook(lambda mod, inp, out, k=k: side.__setitem__(k, out))
    out = m(x1, x2)
    maps = [side[1], side[2], side[3], side[4], out]
    rng = np.random.default_rng(seed + 4)
    tgt = torch.from_numpy((rng.random((2, 32, 32)) < 0.2).astype(np.int64))
    d["target"] = t2n(tgt)
    loss = sum(w * ref_losses.cross_entropy(p, tgt) for w, p in zip(spec.DS_WEIGHTS, maps))
    loss.backward()
    for k, p in enumerate(maps):
        d[f"map{k}"] = t2n(p)
    d["loss"] = loss.item()
    d.update(grad_summary(m))
    save("g23_snunet_conc_ds_2.npz", **d)


def g7():
    print("G23 snunet_conc 128x128")
    seed = 2370
    d = {"seed": seed}
    x1, x2 = rand_pair(seed + 1, 2, 128, 128)
    rng = np.random.default_rng(seed + 4)
    tgt = torch.from_numpy((rng.random((2, 128, 128)) < 0.2).astype(np.int64))
    m = Siam_NestedUNet_Conc(3, 2)
    m.load_state_dict(spec.synth_state(3, 2, seed))
    m.train()
    logits = m(x1, x2)
    loss = ref_losses.cross_entropy(logits, tgt)
    loss.backward()
    d["loss"] = loss.item()
    lf = logits.detach().flatten()
    idx = (np.arange(8192) * 7) % lf.numel()
    d["logits_sample_idx"], d["logits_sample"] = idx, t2n(lf[torch.from_numpy(idx)])
    d["logits_absmean"] = lf.abs().mean().item()
    d.update(grad_summary(m))
    save("g23_snunet_conc_128.npz", **d)


if __name__ == "__main__":
    torch.manual_seed(0)
    g2()
    g2_ds()
    g7()
