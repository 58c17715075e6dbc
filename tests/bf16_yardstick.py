"""Order-noise yardstick of the bf16 parity tests (reference side only; no GPU, no engine).

oracle/fcsiam_bf16.py rounds exactly the tensors the engine's bf16 mode stores and does everything else in the arithmetic of its
inputs.  Run once in float32 arithmetic and once in float64 arithmetic -- the same roundings, another accumulation order / width --
the two sets of gradients are two CORRECT bf16 evaluations of one step.  Their per-tensor cosines measure how far such evaluations
decorrelate on a fixture (a stored value that sits within an fp32 ulp of a bf16 rounding boundary rounds the other way, and the
ReLU / max-pool / |a - b| gates downstream amplify it): the distance an engine that differs from the emulation only in accumulation
order may show, and the part of a test's allowance that the reference alone uses up."""
import torch

from oracle import fcsiam_bf16 as E
from oracle import fcsiam_ref as R
from tests import _util


def oracle_grads(arch, st, x1, x2, tgt, masks, emulate, dtype=torch.float32):
    """(loss, logits, {name: gradient}) of one training step of the fp32 oracle (emulate=False) or of the bf16 emulation, in `dtype`
    arithmetic.  `st` is left unchanged."""
    cast = lambda v: v.to(dtype) if v.dtype.is_floating_point else v.clone()
    ref = {k: cast(v).clone() for k, v in st.items()}
    for k, v in ref.items():
        if v.dtype.is_floating_point and "running" not in k:
            v.requires_grad_(True)
    mk = None if masks is None else {k: cast(v) for k, v in masks.items()}
    x1, x2 = cast(x1), cast(x2)
    logits = E.forward(arch, ref, x1, x2, mk) if emulate else R.forward(arch, ref, x1, x2, training=True, masks=mk)
    loss = R.cross_entropy(logits, tgt)
    loss.backward()
    return loss.item(), logits.detach(), {k: v.grad for k, v in ref.items() if v.requires_grad}


def cosines(got, ref):
    """sorted [(cosine, relative l2, name)] over the tensors of `ref` that carry a gradient (worst first)"""
    out = []
    for k, g in ref.items():
        if _util.zero_grad_by_construction(k) or float(g.abs().max()) < 1e-9:
            continue
        rel, cos = _util.rel_l2_cos(got[k].double().numpy(), g.double().numpy())
        out.append((cos, rel, k))
    return sorted(out)


def worst_median(cs):
    return cs[0][0], cs[len(cs) // 2][0]


def yardstick(arch, st, x1, x2, tgt, masks, g32=None):
    """Cosines of the emulation's gradients in float32 arithmetic against the same emulation in float64 arithmetic.  `g32`: the
    float32 gradients, where the caller has them already."""
    if g32 is None:
        g32 = oracle_grads(arch, st, x1, x2, tgt, masks, True)[2]
    g64 = oracle_grads(arch, st, x1, x2, tgt, masks, True, torch.float64)[2]
    return cosines(g32, g64)
