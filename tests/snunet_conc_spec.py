"""CPU restatement (torch, fp32) of Siam_NestedUNet_Conc, "SNUNet-CD without attention" (SNUNet.py:155-243).

TEST INFRASTRUCTURE ONLY.  The trunk is oracle.snunet_ref's (conv_block_nested, up: the two classes share it line for
line, SNUNet.py:163-193 / :211-235); the tail is written out as the reference computes it (:238-242): four 1x1 convs on
x0_1..x0_4, their concat, one more 1x1 conv.  Pinned by tests/golden/g23_snunet_conc_*.npz (test_snunet_conc_cpu.py); GPU
tests compare with it at shapes that have no fixture.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import snunet_ref as S

HEAD = ("final1", "final2", "final3", "final4", "conv_final")
DS_WEIGHTS = (0.5, 0.5, 0.5, 0.8, 1.0)


def synth_state(in_ch: int, out_ch: int, seed: int, perturb_running: bool = False):
    """Trunk from snunet_ref.synth_state (same seed, same values as SNUNet_ECAM's fixtures), head tensors drawn the same
    way from a generator of their own: weights ~ N(0, 2 / fan_in), biases ~ 0.05 N(0, 1) (non-zero)."""
    full = S.synth_state(in_ch, out_ch, seed, perturb_running)
    st = OrderedDict((k, v) for k, v in full.items() if not k.startswith(("ca.", "ca1.", "conv_final.")))
    rng = np.random.default_rng(seed + 7777)
    for name in HEAD:
        cin = 4 * out_ch if name == "conv_final" else S.FILTERS[0]
        w = rng.standard_normal((out_ch, cin, 1, 1)) * math.sqrt(2.0 / cin)
        b = rng.standard_normal((out_ch,)) * 0.05
        st[name + ".weight"] = torch.from_numpy(w.astype(np.float32)).clone()
        st[name + ".bias"] = torch.from_numpy(b.astype(np.float32)).clone()
    return st


def forward(st, xa, xb, training=False, deep_supervision=False):
    """-> output, or [output1, output2, output3, output4, output] with deep_supervision."""
    up = lambda name, x: S.convT2x2_s2(x, st[f"{name}.up.weight"], st[f"{name}.up.bias"])
    blk = lambda name, x: S.block(x, st, name, training)
    pool = lambda x: F.max_pool2d(x, 2)
    cat = lambda *t: torch.cat(t, 1)
    x0_0A = blk("conv0_0", xa)
    x1_0A = blk("conv1_0", pool(x0_0A))
    x2_0A = blk("conv2_0", pool(x1_0A))
    x3_0A = blk("conv3_0", pool(x2_0A))
    x0_0B = blk("conv0_0", xb)
    x1_0B = blk("conv1_0", pool(x0_0B))
    x2_0B = blk("conv2_0", pool(x1_0B))
    x3_0B = blk("conv3_0", pool(x2_0B))
    x4_0B = blk("conv4_0", pool(x3_0B))
    x0_1 = blk("conv0_1", cat(x0_0A, x0_0B, up("Up1_0", x1_0B)))
    x1_1 = blk("conv1_1", cat(x1_0A, x1_0B, up("Up2_0", x2_0B)))
    x0_2 = blk("conv0_2", cat(x0_0A, x0_0B, x0_1, up("Up1_1", x1_1)))
    x2_1 = blk("conv2_1", cat(x2_0A, x2_0B, up("Up3_0", x3_0B)))
    x1_2 = blk("conv1_2", cat(x1_0A, x1_0B, x1_1, up("Up2_1", x2_1)))
    x0_3 = blk("conv0_3", cat(x0_0A, x0_0B, x0_1, x0_2, up("Up1_2", x1_2)))
    x3_1 = blk("conv3_1", cat(x3_0A, x3_0B, up("Up4_0", x4_0B)))
    x2_2 = blk("conv2_2", cat(x2_0A, x2_0B, x2_1, up("Up3_1", x3_1)))
    x1_3 = blk("conv1_3", cat(x1_0A, x1_0B, x1_1, x1_2, up("Up2_2", x2_2)))
    x0_4 = blk("conv0_4", cat(x0_0A, x0_0B, x0_1, x0_2, x0_3, up("Up1_3", x1_3)))
    outs = [F.conv2d(x, st[f"final{i + 1}.weight"], st[f"final{i + 1}.bias"]) for i, x in enumerate((x0_1, x0_2, x0_3, x0_4))]
    out = F.conv2d(cat(*outs), st["conv_final.weight"], st["conv_final.bias"])
    return outs + [out] if deep_supervision else out


def trainable(st):
    return [k for k, v in st.items() if v.dtype.is_floating_point and "running" not in k]


def ds_loss(maps, tgt, weights=DS_WEIGHTS):
    """sum_k w_k * cross_entropy(map_k): CDTrainer's multi-scale loss (trainer.py:300-309) with multi_pred_weights."""
    return sum(w * F.cross_entropy(m, tgt) for w, m in zip(weights, maps))
