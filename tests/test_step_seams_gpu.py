"""The step's merged entry launches against the launches they replace, bit for bit.

The FC-Siam engine opens a forward with ONE k_step_prologue launch (dropout masks, filter pack, arena zero-fill, input pack) and a
backward with a k_gout_pack launch whose extra blocks clear the gradient buffer; on the backward's tail the slab reduce of the
encoder's weight gradients is split by group (the early groups' part follows them on the side stream, the last group and its part
run on the caller's stream).  stcd_set_debug bit 1 (value 2) brings back the separate launches (k_dropout_gen, k_pack_jobs, two
memsets, k_in_pack) and the one reduce launch on the tail.  Both plans call the same device functions with the same element per
thread and sum every output in the same order, so two modules built from the same parameters, one per plan, must agree in every bit of: logits, loss, every
gradient, BatchNorm running statistics and num_batches_tracked, and the parameters after FlatAdamW.step -- after each of two
consecutive training steps (the second one runs on a workspace and a gradient buffer that the first has left dirty, so it covers
the zero-fills).
"""
import numpy as np
import pytest
import torch

from oracle import fcsiam_ref as R
from stcd_amd import losses
from stcd_amd.modules import SiamUnet_conc, SiamUnet_diff, Unet
from stcd_amd.optim import FlatAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLS = {"diff": SiamUnet_diff, "conc": SiamUnet_conc, "fcef": Unet}
SEPARATE = 2      # stcd_set_debug bit 1


def make(arch, dtype, seed, separate):
    m = CLS[arch](3, 2, dtype=dtype)
    m.load_state_dict(R.synth_state(arch, 3, 2, seed, perturb_running=True))
    m.to(DEV).train()
    m._engine.set_debug(SEPARATE if separate else 0)
    return m


def data(seed, B, H, W):
    rng = np.random.default_rng(seed)
    x1 = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).to(DEV)
    x2 = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).to(DEV)
    tgt = (rng.random((B, H, W)) < 0.3).astype(np.int64)
    tgt[rng.random((B, H, W)) < 0.05] = 255
    return x1, x2, torch.from_numpy(tgt).to(DEV)


def state_of(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def train_step(m, opt, x1, x2, tgt, masks=None):
    """-> everything the step leaves behind, as clones"""
    if masks is not None:
        m.set_dropout_masks(masks)
    logits = m(x1, x2)
    loss = losses.cross_entropy(logits, tgt)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    return {"logits": logits.detach().clone(), "loss": loss.detach().clone(), "grads": grads, "state": state_of(m)}


def assert_same(a, b, what):
    assert torch.equal(a["logits"], b["logits"]), f"{what}: logits differ"
    assert torch.equal(a["loss"], b["loss"]), f"{what}: loss differs ({a['loss'].item()} vs {b['loss'].item()})"
    assert bool(torch.isfinite(a["loss"])) and bool(torch.isfinite(a["logits"]).all()), f"{what}: degenerate step"
    assert a["grads"].keys() == b["grads"].keys()
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), f"{what}: gradient of {k} differs"
    assert any(float(g.abs().max()) > 0 for g in a["grads"].values()), f"{what}: all gradients vanish"
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:      # parameters, running_mean / running_var, num_batches_tracked
        assert torch.equal(a["state"][k], b["state"][k]), f"{what}: {k} differs after the step"


CASES = [
    # id, arch, dtype, (B, H, W), variant
    ("diff", "diff", "bf16", (2, 32, 32), None),
    ("conc", "conc", "bf16", (2, 32, 32), None),
    ("fcef", "fcef", "bf16", (2, 32, 32), None),
    ("diff-b3-24x40", "diff", "bf16", (3, 24, 40), None),
    ("diff-odd-100", "diff", "bf16", (1, 100, 100), None),      # the size of tests/golden/g6_odd.npz
    ("diff-fp32", "diff", "fp32", (2, 32, 32), None),
    ("diff-explicit-masks", "diff", "bf16", (2, 32, 32), "masks"),
    ("diff-p0", "diff", "bf16", (2, 32, 32), "p0"),
    ("diff-stage-hook", "diff", "bf16", (2, 32, 32), "hook"),
]


@pytest.mark.parametrize("cid,arch,dtype,shape,variant", CASES, ids=[c[0] for c in CASES])
def test_two_training_steps_bit_for_bit(cid, arch, dtype, shape, variant):
    B, H, W = shape
    seed = 4100 + len(cid)
    runs = []
    for separate in (False, True):
        m = make(arch, dtype, seed, separate)
        if variant == "p0":
            m.set_dropout_p(0.0)
        calls = []
        if variant == "hook":
            m.grad_stage_hook = lambda stage, g, calls=calls: calls.append((stage, g.numel()))
        opt = FlatAdamW(m, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
        steps = []
        for k in range(2):
            x1, x2, tgt = data(seed + 10 + k, B, H, W)
            masks = R.synth_masks(arch, B, seed + 20 + k) if variant == "masks" else None
            steps.append(train_step(m, opt, x1, x2, tgt, masks))
        if variant == "hook":
            assert [c[0] for c in calls] == [0, 1, 0, 1], "the staged backward ran as stage 0 then stage 1, per step"
        # the plan that ran IS the one the case is about (two engines on the same launches would agree for nothing)
        fused, early, final, tail = m._engine.seam_plan()
        if separate:
            assert (fused, early, final, tail) == (0, 0, 0, 0), (fused, early, final, tail)
        elif dtype == "fp32":      # no grouped weight gradients, hence no slabs to reduce: the entry is merged, the tail has nothing to split
            assert (fused, early, final, tail) == (1, 0, 0, 0), (fused, early, final, tail)
        else:
            assert fused == 1 and early > 0 and final > 0, (fused, early, final)
            # single-call backward: early part behind its groups on the side stream (bit 0), final group on the caller's stream (bit 1);
            # the staged backward of a hook runs on one stream: bit 0 alone
            assert tail == (1 if variant == "hook" else 3), tail
        runs.append(steps)
    for k in range(2):
        assert_same(runs[0][k], runs[1][k], f"{cid} step {k + 1}")
    assert not torch.equal(runs[0][0]["logits"], runs[0][1]["logits"])      # the second step is another step


def test_eval_forward_under_frozen_weights_twice():
    """The second eval forward under frozen_weights() has an empty pack range (the vouched tag) and, like every eval forward, no
    masks and no zeroing: it must repeat the first, and both must equal a fresh engine on the separate launches."""
    seed = 4177
    x1, x2, _ = data(seed + 1, 2, 32, 32)
    outs = []
    for separate in (False, True):
        m = make("diff", "bf16", seed, separate)
        m.eval()
        with torch.no_grad(), m.frozen_weights():
            a = m(x1, x2).clone()
            b = m(x1, x2).clone()
        torch.cuda.synchronize()
        assert torch.equal(a, b), "the second forward under one weights tag differs from the first"
        assert m._engine.seam_plan()[0] == (0 if separate else 1)
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        outs.append(a)
    assert torch.equal(outs[0], outs[1])
    # ... and a training step after it packs again (the training forward never relies on a vouch)
    runs = []
    for separate in (False, True):
        m = make("diff", "bf16", seed, separate)
        m.eval()
        with torch.no_grad(), m.frozen_weights():
            m(x1, x2)
        m.train()
        opt = FlatAdamW(m, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
        xa, xb, tgt = data(seed + 2, 2, 32, 32)
        runs.append(train_step(m, opt, xa, xb, tgt))
    assert_same(runs[0], runs[1], "training step after a frozen eval forward")
