"""Engine lifecycle: a module that has trained, validated, been reconfigured and trained again must compute what a module that
never ran anything else computes from the same state.

The engine keeps state between calls -- the shape-bound plan (a dozen vectors rebuilt by every configure_*), caches keyed on the
workspace address (uploaded job tables, packed filter images and their weights tag), the training flag and the Python ticket, the
side stream and its events, the zeroed accumulator range, the dropout step counter, and the accumulate path of the backward.
Nearly every other GPU test builds a module, runs one shape in one mode and throws it away; here one `used` module walks through
what train_loop.py, a loader's smaller last batch and predict_scene do to it, and after EVERY call a fresh module loaded from the
snapshot taken before that call repeats that one call (tests/lifecycle_spec.py holds the rows and the yardstick).

Comparison: bf16 rows bit for bit (outputs, every parameter's gradient, BatchNorm running buffers, num_batches_tracked) -- every
reduction of the engine is fixed-order.  fp32 rows: outputs and buffers bit for bit; gradients bit for bit for BIT (its own tests
claim that), within 2e-5 relative l2 per tensor elsewhere (the project's bound for two fp32 summation orders).
The reused module gets every workspace at ONE address (lifecycle_spec.share_one_workspace): the workspace is the caller's, and
torch's caching allocator hands a freed block back only by luck of the sizes -- with the allocator's own addresses 2 of the 16
rows noticed a stcd_configure that keeps packed_tag / packed_ws, with one address all 16 do (step 6.3).

RESULTS (MI355X)
----------------
* No row needed a fix in the plan or the caches: all 16 rows are bit-identical to a fresh engine at every step, fp32 included --
  NO fp32 tensor used the 2e-5 bound (SiamUnet_diff fp32 and BIT fp32: every gradient tensor torch.equal; worst fp32 gradient
  rel-l2 between used and fresh: 0).  The fresh fp32 SiamUnet_diff step 8 against the float64 oracle: max |dlogit| 1.1e-5, worst
  gradient rel-l2 5.8e-6.
* Second backward through one forward (loss.backward(retain_graph=True); loss.backward()): before this change it was ACCEPTED AND
  WRONG -- neither refused nor exact.  Running the engine's backward twice through one forward changed 66 of 86 gradient tensors of
  SiamUnet_diff (worst rel-l2 3.5e+1), 126 of 146 of SNUNet_ECAM (2.8), 91 of 92 of SegCD resnet18 (1.4e+1), 188 of 226 of
  ChangeFormer TINY (5.9e+3): the backward kernels overwrite stored activations and output gradients in place.  Now refused:
  _EngineFn.backward marks its ticket consumed, and stcd_backward clears the training flag after stage -1 / stage 1 (stage 0
  followed by stage 1, the staged backward of stcd_amd.ddp, keeps working).
* Wall time of this file: 24 tests in 15 s (slowest case 0.9 s); the whole -m gpu suite with it: 1106 tests in 464 s (two runs, 125 s + 339 s),
  so the parent commit's suite, the same without this file, takes about 449 s.
"""
import dataclasses

import numpy as np
import pytest
import torch

from stcd_amd._lib import StcdError
from tests import lifecycle_spec as L
from tests._util import COS_MIN, REL_L2_MAX, rel_l2_cos

pytestmark = pytest.mark.gpu
DEV = L.DEV
IDS = [r.id for r in L.ROWS]


def checked_call(row, used, call, label, fp32_worst=None):
    """`call` on the reused module and on a fresh module loaded from the snapshot taken just before; -> (snapshot, fresh result)."""
    snap, steps = L.snapshot(used), used._steps
    if call.tgt is not None:
        used.zero_grad()
    L.pin_dropout(row, used, call, steps)
    ru = L.one_call(row, used, call)
    fresh = L.fresh_like(row, snap, call.tgt is not None)
    L.pin_dropout(row, fresh, call, steps)
    rf = L.one_call(row, fresh, call)
    L.compare(row, label, ru, rf, used._engine, fp32_worst)
    if call.tgt is not None:
        assert L.grads_are_views(used), f"{row.id} {label}: p.grad left the flat gradient buffer"
        assert float(rf.grads.abs().max()) > 0.0 and all(bool(torch.isfinite(o).all()) for o in rf.outs), f"{row.id} {label}: the fresh step is degenerate"
    return snap, rf


def anchor_to_the_oracle(row, snap, call, fresh):
    """Fresh against used is self-consistency only: the fresh fp32 SiamUnet_diff step is also held against oracle.fcsiam_ref in
    float64 with the same masks, at the bounds of test_fp32_odd_size_backward_matches_oracle (logits 1e-3, every gradient tensor
    relative l2 <= 2e-2 and cosine >= 0.9995, gradients that vanish by construction below 1e-5)."""
    from oracle import fcsiam_ref as R
    ref = {k: (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in snap.items()}
    names = [k for k, v in ref.items() if v.dtype.is_floating_point and "running" not in k]
    for k in names:
        ref[k].requires_grad_(True)
    masks = {k: v.double() for k, v in L.masks_of(row, call).items()}
    logits = R.forward(row.arch, ref, call.x1.cpu().double(), call.x2.cpu().double(), training=True, masks=masks)
    R.cross_entropy(logits, call.tgt.cpu()).backward()
    err = float((fresh.outs[-1].cpu().double() - logits.detach()).abs().max())
    assert err < 1e-3, f"{row.id}: the fresh step's logits differ from the float64 oracle by {err:.3e}"
    m = row.make()
    worst = 0.0
    for info in m._engine.params:
        got = fresh.grads[info.offset:info.offset + info.numel].cpu().numpy()
        want = ref[info.name].grad.numpy().ravel()
        if np.abs(want).max() < 1e-5:
            assert np.abs(got).max() < 1e-5, info.name
            continue
        rel, cos = rel_l2_cos(got, want)
        worst = max(worst, rel)
        assert rel <= REL_L2_MAX and cos >= COS_MIN, f"{row.id}: fresh gradient of {info.name} against the float64 oracle: rel-l2 {rel:.3e}, cosine {cos:.6f}"
    print(f"{row.id}: fresh step 8 against the float64 oracle: max |dlogit| {err:.2e}, worst gradient rel-l2 {worst:.2e}")


@pytest.mark.parametrize("row", L.ROWS, ids=IDS)
def test_reused_engine_equals_a_fresh_one(row):
    """Training step at S1; parameters rewritten in place (p += 0.01 p, as an optimizer does: a stale filter image then shows);
    eval forward at S2; training step at S2; rewrite; inside ONE frozen_weights() context eval forwards at S1, S1 with other inputs
    (the skip-repack path), S2 (same tag, but the engine reconfigures: the filters must be packed again) and S1 (a workspace is
    set up again, at the old address); rewrite outside the context; training step back at S1.  Every call is compared
    with a fresh module (module docstring).  The fp32 SiamUnet_diff row also ties the fresh side of the last step to the float64
    oracle."""
    fp32_worst = {}
    used = L.new_module(row)
    L.share_one_workspace(row, used)      # S1 and S2 at one workspace address: the case the pointer-keyed caches must survive
    checked_call(row, used, L.make_call(row.s1, 1, True), "step 1 (train S1)", fp32_worst)
    L.rewrite_parameters(used)
    checked_call(row, used, L.make_call(row.s2, 2, False), "step 3 (eval S2)")
    checked_call(row, used, L.make_call(row.s2, 3, True), "step 4 (train S2)", fp32_worst)
    L.rewrite_parameters(used)
    used.eval()
    with used.frozen_weights():
        checked_call(row, used, L.make_call(row.s1, 4, False), "step 6.1 (frozen eval S1)")
        checked_call(row, used, L.make_call(row.s1, 5, False), "step 6.2 (frozen eval S1, other inputs: no repack)")
        checked_call(row, used, L.make_call(row.s2, 6, False), "step 6.3 (frozen eval S2: reconfigured under one tag)")
        checked_call(row, used, L.make_call(row.s1, 7, False), "step 6.4 (frozen eval S1: a workspace allocated again)")
    L.rewrite_parameters(used)
    last = L.make_call(row.s1, 8, True)
    snap, fresh = checked_call(row, used, last, "step 8 (train S1 again)", fp32_worst)
    if row.dtype == "fp32":
        print(f"{row.id}: fp32 gradient tensors that differed between the reused and a fresh engine: "
              + (", ".join(f"{k} {v:.2e}" for k, v in sorted(fp32_worst.items())) or "none (bit-identical)"))
    if row.id == "diff-fp32":
        anchor_to_the_oracle(row, snap, last, fresh)


@pytest.mark.parametrize("row_id", ["diff-bf16", "segcd_r18-bf16", "changeformer_tiny-bf16"])
def test_gradient_accumulation_and_zeroing(row_id):
    """_run_backward takes another path when p.grad exists: two micro-batches without zero_grad leave p.grad == g1 + g2 bit for bit
    (g1, g2 from two fresh modules, added in fp32 by torch); after zero_grad(set_to_none=False) and after zero_grad() one step
    equals the fresh step; after every variant p.grad are still the views of _flat_grads that FlatAdam / FlatAdamW read in place."""
    row = L.BY_ID[row_id]
    used = L.new_module(row).train()
    c1, c2 = L.make_call(row.s1, 11, True), L.make_call(row.s1, 12, True)
    _, f1 = checked_call(row, used, c1, "micro-batch 1")
    snap, steps = L.snapshot(used), used._steps
    L.pin_dropout(row, used, c2, steps)
    r2 = L.one_call(row, used, c2)                           # no zero_grad: accumulates
    fresh = L.fresh_like(row, snap, True)
    L.pin_dropout(row, fresh, c2, steps)
    f2 = L.one_call(row, fresh, c2)
    L.compare(row, "micro-batch 2 (forward, buffers)", dataclasses.replace(r2, grads=None), dataclasses.replace(f2, grads=None), used._engine)
    assert L.grads_are_views(used)
    for p, info in zip(used.parameters(), used._engine.params):
        sl = slice(info.offset, info.offset + info.numel)
        want = (f1.grads[sl] + f2.grads[sl]).view(info.shape)
        assert torch.equal(p.grad, want), f"{row.id}: accumulated gradient of {info.name} is not g1 + g2, rel-l2 {float((p.grad - want).norm() / want.norm().clamp_min(1e-30)):.3e}"
    assert float((f1.grads - f2.grads).abs().max()) > 0.0
    used.zero_grad(set_to_none=False)
    snap, steps = L.snapshot(used), used._steps
    c3 = L.make_call(row.s1, 13, True)
    L.pin_dropout(row, used, c3, steps)
    r3 = L.one_call(row, used, c3)                           # p.grad exists and is zero: the accumulate path again
    fresh = L.fresh_like(row, snap, True)
    L.pin_dropout(row, fresh, c3, steps)
    L.compare(row, "after zero_grad(set_to_none=False)", r3, L.one_call(row, fresh, c3), used._engine)
    assert L.grads_are_views(used)
    checked_call(row, used, L.make_call(row.s1, 14, True), "after zero_grad()")      # checked_call sets the gradients to None first


@pytest.mark.parametrize("row_id", ["diff-bf16", "snunet_ecam-bf16", "segcd_r18-bf16", "changeformer_tiny-bf16"])
def test_lifecycle_guards_are_loud_and_leave_the_engine_usable(row_id):
    """The engine keeps ONE step of activations: the backward of a training forward A after any later forward of the module
    (training at another shape, eval, training mode under no_grad) raises "overwritten"; a backward through an eval output raises
    "eval-mode"; a second backward through one forward (retain_graph=True) must raise or reproduce the first gradients bit for bit.
    After each refusal a full training step equals the fresh step."""
    row = L.BY_ID[row_id]
    used = L.new_module(row).train()
    L.share_one_workspace(row, used)
    A, other = L.make_call(row.s1, 21, True), L.make_call(row.s2, 22, True)

    def forward_a():
        used.train()
        used.zero_grad()
        L.pin_dropout(row, used, A, used._steps)
        return L.loss_of(row, L.forward_of(row, used, A), A.tgt)

    for n, how in enumerate(("training at another shape", "eval", "training mode under no_grad")):
        loss = forward_a()
        if how == "training at another shape":
            L.pin_dropout(row, used, other, used._steps)
            L.forward_of(row, used, other)
        elif how == "eval":
            used.eval()
            L.forward_of(row, used, A)
            used.train()
        else:
            with torch.no_grad():
                L.forward_of(row, used, A)
        with pytest.raises(StcdError, match="overwritten"):
            loss.backward()
        checked_call(row, used, L.make_call(row.s1, 30 + n, True), f"recovery after a backward refused for a later forward ({how})")
    used.eval()
    out = L.forward_of(row, used, A)
    with pytest.raises(StcdError, match="eval-mode"):
        L.loss_of(row, out, A.tgt).backward()
    checked_call(row, used, L.make_call(row.s1, 34, True), "recovery after a backward refused for an eval output")
    loss = forward_a()
    loss.backward(retain_graph=True)
    first = used._flat_grads.clone()
    used.zero_grad(set_to_none=False)
    try:
        loss.backward()
    except StcdError as e:
        refused = str(e)
    else:
        refused = None
        assert torch.equal(used._flat_grads, first), f"{row.id}: a second backward through one forward was accepted and gave other gradients"
    print(f"{row.id}: second backward through one forward: " + ("refused" if refused else "accepted, bit-identical"))
    checked_call(row, used, L.make_call(row.s1, 35, True), "recovery after the second backward")


def test_second_stcd_backward_through_one_forward_is_refused():
    """At the C ABI: stage -1 and stage 1 consume the forward (the backward kernels overwrite stored tensors in place), stage 0
    followed by stage 1 -- the staged backward of stcd_amd.ddp -- keeps working, and a refused call leaves the engine usable."""
    from stcd_amd.engine import Engine
    from tests.test_kernel_plan_gpu import synth_params
    eng = Engine("diff", 3, 2, "bf16")
    eng.set_dropout_p(0.0)
    eng.configure(2, 32, 32, torch.device(DEV))
    params, bn = synth_params(eng, 23)
    gen = torch.Generator().manual_seed(43)
    x1, x2 = torch.randn(2, 3, 32, 32, generator=gen).to(DEV), torch.randn(2, 3, 32, 32, generator=gen).to(DEV)
    logits = torch.zeros(2, 2, 32, 32, device=DEV)
    dlogits = (1e-3 * torch.randn(2, 2, 32, 32, generator=gen)).to(DEV)
    grads = [torch.zeros_like(params) for _ in range(3)]
    eng.forward(x1, x2, params, bn, logits, True, None, seed=7)
    eng.backward(dlogits, params, grads[0], -1)
    for stage in (-1, 0, 1):
        with pytest.raises(StcdError, match="no backward has consumed"):
            eng.backward(dlogits, params, grads[1], stage)
    eng.forward(x1, x2, params, bn, logits, True, None, seed=7)
    eng.backward(dlogits, params, grads[1], -1)
    torch.cuda.synchronize()
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0.0
    eng.set_wgrad_side(False)                      # the plan of the staged (data-parallel) backward
    eng.configure(2, 32, 32, torch.device(DEV))
    eng.forward(x1, x2, params, bn, logits, True, None, seed=7)
    eng.backward(dlogits, params, grads[2], 0)
    eng.backward(dlogits, params, grads[2], 1)
    with pytest.raises(StcdError, match="no backward has consumed"):
        eng.backward(dlogits, params, grads[2], 1)
    torch.cuda.synchronize()
    rel = float((grads[2].double() - grads[0].double()).norm() / grads[0].double().norm())
    assert rel <= 2e-5, rel                        # another K-split of the same bf16 products (the side-stream test's bound)
    eng.forward(x1, x2, params, bn, logits, False, None, seed=7)
    with pytest.raises(StcdError, match="training-mode forward"):
        eng.backward(dlogits, params, grads[2], -1)
