"""TEST INFRASTRUCTURE ONLY -- the FC-Siam oracle (oracle/fcsiam_ref.py, pinned to the reference by tests/golden) with bf16 rounding
at exactly the points where the HIP engine's bf16 mode STORES a tensor, forward and backward, fp32 arithmetic everywhere else:

  forward   input image; filter images of every convolution (forward and data-gradient products use the bf16 filter, the weight
            gradient itself stays fp32); every conv / transposed-conv output Y (BatchNorm statistics are those of the rounded
            values, stcd_amd/csrc/kernels_conv_mfma.hip epilogues); every activation A = dropout(relu(BN(Y))); pooled maps and the
            skip fusion |a1 - a2| / a2 - a1 (formed from the rounded activations and rounded once more: k_bn_act_pair)
  backward  the gradient of every one of those tensors is rounded once where the engine writes its gradient buffer (dA: the
            data-gradient conv's output, or pool + fusion gradient summed then rounded -- k_skip_bwd; dY: k_bn_bwd_apply's output);
            d(logits) is rounded when it is packed for the last layer's gradient launches (k_gout_pack)

Per network (stcd_amd/csrc/engine.hip: forward_fcsiam, xconc_forward, xconc_backward, the encoder loop of backward_fcsiam):

  diff, sub   two streams; the fused skip is formed from the rounded activations and rounded once more; its gradient and the pool
              gradient are summed in fp32 and rounded once (k_skip_bwd)
  conc        two streams; the skip IS the stored activation (inside the concat buffer: not rounded a second time).  Backward: the
              decoder conv's data gradient stores the gradient of the whole concat buffer (rounded); k_pool_bwd(accumulate = 1) then
              reads that stored value, adds the pool gradient in fp32 and stores the sum -- rounded AGAIN (skip_branch below)
  fcef        ONE stream over cat(x1, x2) (k_in_pack, concat mode: the concatenated input is stored rounded); skip and skip gradient
              as conc, one date
  xconc       two streams; per level the cross_conc block (cross_conc below), in order: G = pairwise depthwise conv of the stored
              skip activations, stored rounded (k_pairdw_* read the fp32 filter from the parameter buffer: no bf16 filter image);
              R = relu(BN(G)) stored rounded, batch statistics of the rounded G; Y = conv_res of R with the bf16 filter image, stored
              rounded; A = relu(BN(Y)) stored rounded into the concat slice; no dropout inside the block.  Backward: dA (the concat
              gradient), dY, dR, dG are each rounded where they are written; k_pairdw_bwd_data stores both dates' skip gradient
              (rounded) and the pool gradient is accumulated onto it as for conc (rounded again)

q and ste keep the dtype of their argument, so the same emulation runs in float64 arithmetic with the same roundings
(tests/bf16_yardstick.py: the distance between two correct bf16 evaluations).

What this file is for: rounding noise of ~20 bf16-stored layers moves whole-network gradients far from
the fp32 reference's, so a bound against the fp32 reference alone cannot tell rounding from a wrong term.  Against THIS emulation
the engine's bf16 gradients must agree closely (tests/test_bf16_emulation_gpu.py): what is left is accumulation order and the
rare activation that sits within one fp32 ulp of a bf16 rounding boundary.
"""
from __future__ import annotations

import contextlib

import torch

from . import fcsiam_ref as R


class _Q(torch.autograd.Function):
    """round to bf16 in the forward (fwd=True) and / or round the gradient in the backward (bwd=True)"""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return x.bfloat16().to(x.dtype) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (g.bfloat16().to(g.dtype) if ctx.bwd else g), None, None


def q(x, fwd=True, bwd=True):
    return _Q.apply(x, fwd, bwd)


def ste(w):
    """bf16 filter image in the products, fp32 weight gradient (straight through)"""
    return w + (w.detach().bfloat16().to(w.dtype) - w.detach())


@contextlib.contextmanager
def emulate():
    """Inside: oracle.fcsiam_ref.forward computes what the engine's bf16 mode stores."""
    orig = (R.conv3x3, R.convT3x3_s1, R.convT3x3_s2, R.maxpool2, R._cbrd, torch.abs)
    c3, t1, t2, mp = orig[0], orig[1], orig[2], orig[3]

    def cbrd(x, st, sfx, training, mask, conv):
        y = q(conv(x, ste(st[f"conv{sfx}.weight"]), st[f"conv{sfx}.bias"]))
        z = R.batchnorm(y, st[f"bn{sfx}.weight"], st[f"bn{sfx}.bias"], st[f"bn{sfx}.running_mean"], st[f"bn{sfx}.running_var"], training)
        if training:
            st[f"bn{sfx}.num_batches_tracked"] += 1
        a = torch.relu(z)
        if training and mask is not None:
            a = a * mask[:, :, None, None]
        return q(a)

    R._cbrd = cbrd
    R.maxpool2 = lambda x: q(mp(x), fwd=False)                                   # max of bf16 values is exact; d(pooled) is stored
    R.convT3x3_s2 = lambda x, w, b: q(t2(x, ste(w), b))                          # up-conv output inside the concat buffer
    R.convT3x3_s1 = lambda x, w, b: q(t1(x, ste(w), b), fwd=False)               # conv11d: fp32 logits, bf16 d(logits)
    try:
        yield
    finally:
        R.conv3x3, R.convT3x3_s1, R.convT3x3_s2, R.maxpool2, R._cbrd = orig[:5]


def skip_branch(f, date):
    """The skip activation as the concat / cross_conc consumer reads it (conc, fcef, xconc).  Forward: the stored activation itself, not
    rounded again.  Backward: that consumer's data gradient is STORED in the activation's gradient buffer (rounded: the decoder conv's
    data-gradient launch writes the whole concat gradient, k_pairdw_bwd_data both dates' halves) before k_pool_bwd(accumulate = 1)
    reads it back, adds the pool gradient in fp32 and stores the sum (rounded again, by the q(a) of the producing layer)."""
    return q(f, fwd=False)


def cross_conc(st, l, f1, f2):
    """The cross_conc block as xconc_forward / xconc_backward store it (training mode, no dropout inside the block)."""
    n, c, h, w = f1.shape
    p = f"cross_conc{l}."
    pair = torch.stack((skip_branch(f1, 0), skip_branch(f2, 1)), 2).reshape(n, 2 * c, h, w)
    # k_pairdw_* read the fp32 filter from the parameter buffer: no bf16 filter image here
    g = q(torch.nn.functional.conv2d(pair, st[p + "diff.0.weight"], st[p + "diff.0.bias"], padding=1, groups=c))       # G, dG
    z = R.batchnorm(g, st[p + "diff.1.weight"], st[p + "diff.1.bias"], st[p + "diff.1.running_mean"], st[p + "diff.1.running_var"], True)
    st[p + "diff.1.num_batches_tracked"] += 1
    r = q(torch.relu(z))                                                                                                # R, dR
    y = q(R.conv3x3(r, ste(st[p + "conv_res.0.weight"]), st[p + "conv_res.0.bias"]))                                    # Y, dY
    z = R.batchnorm(y, st[p + "conv_res.1.weight"], st[p + "conv_res.1.bias"], st[p + "conv_res.1.running_mean"],
                    st[p + "conv_res.1.running_var"], True)
    st[p + "conv_res.1.num_batches_tracked"] += 1
    return q(torch.relu(z))                                                                                             # A in the concat slice


def forward(arch, st, x1, x2, masks):
    """Training-mode forward of the emulation, all five networks of oracle.fcsiam_ref.ARCHS.  The loops of R.forward are restated to
    place the roundings that sit between its layers (tests/test_bf16_emulation_cpu.py: with every rounding a no-op this IS R.forward)."""
    assert arch in R.ARCHS
    with emulate():
        B = x1.shape[0]
        skips, bott = [], None
        x1, x2 = q(x1, bwd=False), q(x2, bwd=False)
        for t, x in enumerate((torch.cat((x1, x2), 1),) if arch == "fcef" else (x1, x2)):
            feats = []
            for stage in R.ENCODER:
                for sfx, _, _ in stage:
                    x = R._cbrd(x, st, sfx, True, None if masks is None else masks[f"do{sfx}"][t * B:(t + 1) * B], R.conv3x3)
                feats.append(x)
                x = R.maxpool2(x)
            skips.append(feats)
            bott = x
        x = bott
        for lvl, (up, c, convs) in zip((3, 2, 1, 0), R.DECODER):
            f1, f2 = skips[0][lvl], skips[-1][lvl]
            x = R.pad_to(R.convT3x3_s2(x, st[f"{up}.weight"], st[f"{up}.bias"]), f1)
            if arch == "xconc":
                x = torch.cat((x, cross_conc(st, lvl + 1, f1, f2)), 1)
            elif arch == "fcef":
                x = torch.cat((x, skip_branch(f1, 0)), 1)
            elif arch == "conc":
                x = torch.cat((x, skip_branch(f1, 0), skip_branch(f2, 1)), 1)
            elif arch == "diff":
                x = torch.cat((x, q(torch.abs(f1 - f2))), 1)
            else:
                x = torch.cat((x, q(f2 - f1)), 1)
            for sfx, _, _ in convs:
                if sfx == "11d":
                    x = R.convT3x3_s1(x, st["conv11d.weight"], st["conv11d.bias"])
                else:
                    x = R._cbrd(x, st, sfx, True, None if masks is None else masks[f"do{sfx}"], R.convT3x3_s1)
        return x
