"""The kernel plan, pinned: which convolution / weight-gradient kernel every launch of a step runs on.

For each case one training step (dropout 0) and one eval forward run with the engine's event instrumentation on, and
{kernel name: launches} from Engine.profile_kernels() is compared with PLAN below.  The engine chooses a launch's kernel in one
place (conv_kernel in csrc/engine.hip); this table is what that choice must keep producing.

PLAN was captured on the commit BEFORE the chooser existed (93d5faa), on an MI355X, by running this file's print mode against that
commit's library, one fresh process per case:

    PYTHONPATH=. python tests/test_kernel_plan_gpu.py                        # every case: prints the PLAN literal
    PYTHONPATH=. python tests/test_kernel_plan_gpu.py diff_2x64x64_bf16      # one case, as a JSON line (with result hashes)

A row may differ from that capture only where the old instrumentation named a kernel that then did not run (a launcher rejected
and the cascade slid on); launch totals per case are equal without exception.  No such row exists: the capture is embedded as is."""
import hashlib
import json
import sys

import pytest
import torch

from stcd_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MIT_B0 = dict(embed_dims=(32, 64, 160, 256), depths=(2, 2, 2, 2), num_heads=(1, 2, 5, 8), sr_ratios=(8, 4, 2, 1), mlp_ratio=4,
              patch1=7, patch=3, embedding_dim=256)
NO_DROP = dict(drop_rate=0.0, attn_drop=0.0, drop_path_rate=0.0, diff_drop=0.0)

# id: (arch, dtype, B, H, W, ChangeFormer config or None, environment)
CASES = {
    "diff_2x64x64_bf16": ("diff", "bf16", 2, 64, 64, None, {}),
    "diff_1x48x80_bf16": ("diff", "bf16", 1, 48, 80, None, {}),
    "conc_3x48x80_bf16": ("conc", "bf16", 3, 48, 80, None, {}),            # odd batch: n % groups
    "fcef_2x32x32_bf16": ("fcef", "bf16", 2, 32, 32, None, {}),
    "xconc_2x32x32_bf16": ("xconc", "bf16", 2, 32, 32, None, {}),
    "snunet_2x32x32_bf16": ("snunet", "bf16", 2, 32, 32, None, {}),
    "snunet_conc_ds_2x32x32_bf16": ("snunet_conc_ds", "bf16", 2, 32, 32, None, {}),
    "segcd_resnet50_1x64x64_bf16": ("segcd_resnet50", "bf16", 1, 64, 64, None, {}),
    "segcd_resnet18_1x64x64_bf16": ("segcd_resnet18", "bf16", 1, 64, 64, None, {}),
    "base_resnet18_2x64x64_bf16": ("base_resnet18_s5", "bf16", 2, 64, 64, None, {}),
    "bit_2x64x64_bf16": ("bit_s4_dd8_dh8", "bf16", 2, 64, 64, None, {}),
    "changeformer_1x64x64_bf16": ("changeformer", "bf16", 1, 64, 64, NO_DROP, {}),
    "changeformer_mitb0_1x64x64_bf16": ("changeformer", "bf16", 1, 64, 64, dict(MIT_B0, **NO_DROP), {}),
    # the smallest map on which the 256 -> 256 decoder layers reach both LDS-DMA kernels: k_conv_dma from 256 * 192 output positions,
    # k_wgrad_dma from 65536 on maps at least 64 wide
    "changeformer_1x256x256_bf16": ("changeformer", "bf16", 1, 256, 256, NO_DROP, {}),
    "diff_2x64x64_fp32": ("diff", "fp32", 2, 64, 64, None, {}),
    "diff_2x64x64_bf16_no_small": ("diff", "bf16", 2, 64, 64, None, {"STCD_NO_SMALL_KERNEL": "1"}),
    "diff_2x64x64_bf16_no_res": ("diff", "bf16", 2, 64, 64, None, {"STCD_NO_RES_KERNEL": "1"}),
    "diff_2x64x64_bf16_no_gemm": ("diff", "bf16", 2, 64, 64, None, {"STCD_NO_GEMM_KERNEL": "1"}),
    "diff_2x64x64_bf16_no_tile": ("diff", "bf16", 2, 64, 64, None, {"STCD_NO_TILE_KERNEL": "1"}),
    "diff_2x64x64_bf16_virt_act": ("diff", "bf16", 2, 64, 64, None, {"STCD_VIRT_ACT": "1"}),
    "diff_2x64x64_bf16_bwdsum_res": ("diff", "bf16", 2, 64, 64, None, {"STCD_BWDSUM_RES": "1"}),
    "diff_2x64x64_bf16_force_ref": ("diff", "bf16", 2, 64, 64, None, {"STCD_FORCE_REF_KERNELS": "1"}),
    "changeformer_1x64x64_bf16_halo": ("changeformer", "bf16", 1, 64, 64, NO_DROP, {"STCD_HALO_KERNEL": "1"}),
}


def synth_params(eng, seed):
    """A plausible state in the engine's flat layout: small random filters, normalisation scales near one, running variance one."""
    gen = torch.Generator().manual_seed(seed)
    flat = torch.zeros(eng.param_floats)
    for p in eng.params:
        v = torch.randn(p.numel, generator=gen)
        if len(p.shape) == 1 and p.name.endswith("weight"):
            v = 1.0 + 0.1 * v
        elif len(p.shape) == 1:
            v = 0.1 * v
        else:
            v = v / (p.numel / p.shape[0]) ** 0.5
        flat[p.offset:p.offset + p.numel] = v
    bn = torch.zeros(eng.bn_floats)
    for b in eng.bns:
        bn[b.offset + b.channels:b.offset + 2 * b.channels] = 1.0
    return flat.to(DEV), bn.to(DEV)


def run_case(case):
    """-> ({"train": {kernel: launches}, "eval": {...}}, {"logits" / "grads" / "bn": tensor}, workspace bytes).  The environment of the
    case must be set before the call: the engine reads its switches when it is created."""
    arch, dtype, B, H, W, cf, _env = CASES[case]
    eng = Engine(arch, 3, 2, dtype, cf)
    if arch != "changeformer":
        eng.set_dropout_p(0.0)
    eng.configure(B, H, W, torch.device(DEV))
    params, bn = synth_params(eng, 23)
    grads = torch.zeros_like(params)
    gen = torch.Generator().manual_seed(43)
    x1 = torch.randn(B, 3, H, W, generator=gen).to(DEV)
    x2 = torch.randn(B, 3, H, W, generator=gen).to(DEV)
    logits = torch.zeros(eng.output_floats(), device=DEV)
    dlogits = (1e-3 * torch.randn(eng.output_floats(), generator=gen)).to(DEV)
    plan = {}
    eng.profile_enable(True)
    eng.forward(x1, x2, params, bn, logits, True, None, seed=7)
    eng.backward(dlogits, params, grads)
    torch.cuda.synchronize()
    plan["train"] = {k: v["launches"] for k, v in sorted(eng.profile_kernels().items())}
    out = {"logits": logits.clone(), "grads": grads.clone(), "bn": bn.clone()}
    eng.profile_enable(True)
    eng.forward(x1, x2, params, bn, logits, False, None, seed=7)
    torch.cuda.synchronize()
    plan["eval"] = {k: v["launches"] for k, v in sorted(eng.profile_kernels().items())}
    eng.profile_enable(False)
    return plan, out, int(eng.workspace.numel())


# PLAN: see the module docstring
PLAN = {
    "diff_2x64x64_bf16": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 13,
                  "k_conv_gemm<2>": 2, "k_conv_mfma<1>": 5, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 8,
                  "k_conv_small<1, 5>": 3, "k_conv_small<bwd>": 2, "k_conv_tile<1>": 23, "k_pack_jobs|k_reduce_dw": 1,
                  "k_reduce_jobs": 2, "k_skip_bwd_pair": 4, "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 2,
                  "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 1,
                  "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 4,
                 "k_conv_res<1, 32, false>": 4, "k_conv_small<1, 5>": 3, "k_conv_tile<1>": 12, "k_pack_jobs|k_reduce_dw": 1},
    },
    "diff_1x48x80_bf16": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 13,
                  "k_conv_gemm<2>": 2, "k_conv_mfma<1>": 5, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 8,
                  "k_conv_small<1, 5>": 3, "k_conv_small<bwd>": 2, "k_conv_tile<1>": 23, "k_pack_jobs|k_reduce_dw": 1,
                  "k_reduce_jobs": 2, "k_skip_bwd_pair": 4, "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 2,
                  "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 1,
                  "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 4,
                 "k_conv_res<1, 32, false>": 4, "k_conv_small<1, 5>": 3, "k_conv_tile<1>": 12, "k_pack_jobs|k_reduce_dw": 1},
    },
    "conc_3x48x80_bf16": {
        "train": {"k_bn_act": 19, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 2, "k_bn_reduce<T, 1>": 17, "k_conv_gemm<2>": 2,
                  "k_conv_mfma<1>": 6, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 9, "k_conv_small<1, 5>": 3,
                  "k_conv_small<bwd>": 2, "k_conv_tile<1>": 21, "k_pack_jobs|k_reduce_dw": 1, "k_pool_bwd|k_fuse|k_slice": 4,
                  "k_reduce_jobs": 2, "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 2,
                  "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 1,
                  "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 19, "k_conv_mfma<1>": 2, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 5,
                 "k_conv_small<1, 5>": 3, "k_conv_tile<1>": 10, "k_pack_jobs|k_reduce_dw": 1},
    },
    "fcef_2x32x32_bf16": {
        "train": {"k_bn_act": 19, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 17, "k_conv_gemm<2>": 2,
                  "k_conv_mfma<1>": 5, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 8, "k_conv_small<1, 5>": 3,
                  "k_conv_small<bwd>": 2, "k_conv_tile<1>": 23, "k_pack_jobs|k_reduce_dw": 1, "k_pool_bwd|k_fuse|k_slice": 4,
                  "k_reduce_jobs": 2, "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 2,
                  "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 1,
                  "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 19, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 4,
                 "k_conv_small<1, 5>": 3, "k_conv_tile<1>": 12, "k_pack_jobs|k_reduce_dw": 1},
    },
    "xconc_2x32x32_bf16": {
        "train": {"k_bn_act": 23, "k_bn_bwd_apply": 23, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 21, "k_conv_gemm<2>": 2,
                  "k_conv_mfma<1>": 5, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 10, "k_conv_small<1, 5>": 5,
                  "k_conv_small<bwd>": 2, "k_conv_tile<1>": 27, "k_pack_jobs|k_reduce_dw": 1, "k_pairdw_bwd": 4,
                  "k_pairdw_fwd": 4, "k_pool_bwd|k_fuse|k_slice": 4, "k_reduce_jobs": 2, "k_wgrad_group<1, 1, false>": 1,
                  "k_wgrad_group<1, 1, true>": 2, "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1,
                  "k_wgrad_group<2, 2, false>": 1, "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 23, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 5,
                 "k_conv_small<1, 5>": 4, "k_conv_tile<1>": 14, "k_pack_jobs|k_reduce_dw": 1, "k_pairdw_fwd": 4},
    },
    "snunet_2x32x32_bf16": {
        "train": {"k_bn_act": 30, "k_bn_bwd_apply": 30, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 30, "k_conv_gemm<2>": 16,
                  "k_conv_mfma<1>": 3, "k_conv_mfma_x4<1>": 10, "k_conv_res<1, 32, false>": 44, "k_conv_res<1, 64, false>": 8,
                  "k_pack_jobs|k_reduce_dw": 1, "k_pool_bwd|k_fuse|k_slice": 4, "k_reduce_jobs": 1,
                  "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, false>": 1, "k_wgrad_group<2, 2, true>": 1,
                  "k_wgrad_group<4, 2, false>": 1, "k_wgrad_group<4, 2, true>": 1},
        "eval": {"k_bn_act": 30, "k_conv_gemm<2>": 4, "k_conv_mfma<1>": 2, "k_conv_mfma_x4<1>": 10,
                 "k_conv_res<1, 32, false>": 21, "k_conv_res<1, 64, false>": 4, "k_pack_jobs|k_reduce_dw": 1},
    },
    "snunet_conc_ds_2x32x32_bf16": {
        "train": {"k_bn_act": 30, "k_bn_bwd_apply": 30, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 30, "k_conv_gemm<2>": 16,
                  "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 10, "k_conv_res<1, 32, false>": 44, "k_conv_res<1, 64, false>": 8,
                  "k_pack_jobs|k_reduce_dw": 1, "k_pool_bwd|k_fuse|k_slice": 4, "k_reduce_jobs": 1,
                  "k_snhead_bwd|k_snhead_reduce|k_snhead_chain": 1, "k_snhead_fwd": 1, "k_wgrad_group<1, 2, true>": 1,
                  "k_wgrad_group<2, 2, true>": 1, "k_wgrad_group<4, 2, false>": 1, "k_wgrad_group<4, 2, true>": 1},
        "eval": {"k_bn_act": 30, "k_conv_gemm<2>": 4, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 10,
                 "k_conv_res<1, 32, false>": 21, "k_conv_res<1, 64, false>": 4, "k_pack_jobs|k_reduce_dw": 1,
                 "k_snhead_fwd": 1},
    },
    "segcd_resnet50_1x64x64_bf16": {
        "train": {"k_bn_act": 63, "k_bn_bwd_apply": 63, "k_bn_reduce<T, 1>": 63, "k_conv_gemm<2>": 81, "k_conv_gemm<stem>": 1,
                  "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 3, "k_conv_res<1, 32, false>": 24, "k_conv_res<1, 64, false>": 13,
                  "k_conv_small<1, 5>": 4, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 1, "k_wgrad_group<1, 1, true>": 1,
                  "k_wgrad_group<1, 2, false>": 1, "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1,
                  "k_wgrad_group<2, 2, false>": 1, "k_wgrad_group<2, 2, true>": 1},
        "eval": {"k_bn_act": 63, "k_conv_gemm<2>": 43, "k_conv_gemm<stem>": 1, "k_conv_res<1, 32, false>": 12,
                 "k_conv_res<1, 64, false>": 6, "k_conv_small<1, 5>": 2, "k_pack_jobs|k_reduce_dw": 1},
    },
    "segcd_resnet18_1x64x64_bf16": {
        "train": {"k_bn_act": 30, "k_bn_bwd_apply": 30, "k_bn_reduce<T, 1>": 30, "k_conv_gemm<2>": 16, "k_conv_gemm<stem>": 1,
                  "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 3, "k_conv_res<1, 32, false>": 27, "k_conv_res<1, 64, false>": 9,
                  "k_conv_small<1, 5>": 4, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 1, "k_wgrad_group<1, 1, true>": 1,
                  "k_wgrad_group<1, 2, false>": 1, "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1,
                  "k_wgrad_group<2, 2, false>": 1, "k_wgrad_group<2, 2, true>": 1},
        "eval": {"k_bn_act": 30, "k_conv_gemm<2>": 10, "k_conv_gemm<stem>": 1, "k_conv_res<1, 32, false>": 14,
                 "k_conv_res<1, 64, false>": 4, "k_conv_small<1, 5>": 2, "k_pack_jobs|k_reduce_dw": 1},
    },
    "base_resnet18_2x64x64_bf16": {
        "train": {"k_bias_grad": 1, "k_bilinear": 1, "k_bilinear_bwd": 1, "k_bn_act": 21, "k_bn_bwd_apply": 21,
                  "k_bn_reduce<T, 1>": 21, "k_conv_gemm<2>": 14, "k_conv_gemm<stem>": 1, "k_conv_mfma<1>": 3,
                  "k_conv_mfma_x4<1>": 1, "k_conv_res<1, 32, false>": 18, "k_conv_res<1, 64, false>": 8, "k_fuse": 1,
                  "k_fuse_bwd": 1, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 1, "k_upsample2": 1,
                  "k_wgrad_group<1, 2, false>": 1, "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1,
                  "k_wgrad_group<2, 2, false>": 1, "k_wgrad_group<2, 2, true>": 1},
        "eval": {"k_bilinear": 1, "k_bn_act": 21, "k_conv_gemm<2>": 7, "k_conv_gemm<stem>": 1, "k_conv_mfma<1>": 2,
                 "k_conv_res<1, 32, false>": 9, "k_conv_res<1, 64, false>": 4, "k_fuse": 1, "k_pack_jobs|k_reduce_dw": 1,
                 "k_upsample2": 1},
    },
    "bit_2x64x64_bf16": {
        "train": {"k_bias_grad": 1, "k_bilinear": 1, "k_bilinear_bwd": 1, "k_bit_dec_bwd": 1, "k_bit_dec_fold": 1,
                  "k_bit_dec_fwd": 1, "k_bit_enc<false>": 1, "k_bit_enc<true>": 1,
                  "k_bit_sum_parts|k_bit_dec_unfold|k_bit_dec_mfinish": 1, "k_bit_tok_bwd": 1, "k_bit_tok_fwd": 1,
                  "k_bn_act": 16, "k_bn_bwd_apply": 16, "k_bn_reduce<T, 1>": 16, "k_conv_gemm<2>": 5, "k_conv_gemm<stem>": 1,
                  "k_conv_mfma<1>": 2, "k_conv_mfma_x4<1>": 1, "k_conv_res<1, 32, false>": 18, "k_conv_res<1, 64, false>": 8,
                  "k_fuse": 1, "k_fuse_bwd": 1, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 1, "k_upsample2": 1,
                  "k_wgrad_group<1, 2, false>": 1, "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1,
                  "k_wgrad_group<2, 2, false>": 1, "k_wgrad_group<2, 2, true>": 1},
        "eval": {"k_bilinear": 1, "k_bit_dec_fold": 1, "k_bit_dec_fwd": 1, "k_bit_enc<false>": 1, "k_bit_tok_fwd": 1,
                 "k_bn_act": 16, "k_conv_gemm<2>": 3, "k_conv_gemm<stem>": 1, "k_conv_mfma<1>": 1,
                 "k_conv_res<1, 32, false>": 9, "k_conv_res<1, 64, false>": 4, "k_fuse": 1, "k_pack_jobs|k_reduce_dw": 1,
                 "k_upsample2": 1},
    },
    "changeformer_1x64x64_bf16": {
        "train": {"k_attn_bwd": 13, "k_attn_fwd": 13, "k_bn_act": 9, "k_chan_moments": 9, "k_col2im": 13, "k_colsum_group": 2,
                  "k_conv_gemm<2>": 203, "k_conv_mfma<1>": 6, "k_dwgelu_bwd": 13, "k_dwgelu_fwd": 13, "k_im2col": 14,
                  "k_ln_bwd": 44, "k_ln_fwd": 44, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2, "k_resid_drop": 26,
                  "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 2, "k_wgrad_group<4, 2, true>": 1},
        "eval": {"k_attn_fwd": 13, "k_bn_act": 9, "k_conv_gemm<2>": 104, "k_conv_mfma<1>": 5, "k_dwgelu_fwd": 13,
                 "k_im2col": 14, "k_ln_fwd": 44, "k_pack_jobs|k_reduce_dw": 1, "k_resid_drop": 26},
    },
    "changeformer_mitb0_1x64x64_bf16": {
        "train": {"k_attn_bwd": 8, "k_attn_fwd": 8, "k_bn_act": 9, "k_chan_moments": 9, "k_col2im": 9, "k_colsum_group": 2,
                  "k_conv_gemm<2>": 88, "k_conv_mfma<1>": 63, "k_dwgelu_bwd": 8, "k_dwgelu_fwd": 8, "k_im2col": 10,
                  "k_ln_bwd": 30, "k_ln_fwd": 30, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2, "k_resid_drop": 16,
                  "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 2, "k_wgrad_group<4, 2, true>": 1},
        "eval": {"k_attn_fwd": 8, "k_bn_act": 9, "k_conv_gemm<2>": 47, "k_conv_mfma<1>": 33, "k_dwgelu_fwd": 8, "k_im2col": 10,
                 "k_ln_fwd": 30, "k_pack_jobs|k_reduce_dw": 1, "k_resid_drop": 16},
    },
    "changeformer_1x256x256_bf16": {
        "train": {"k_attn_bwd": 13, "k_attn_fwd": 13, "k_bn_act": 9, "k_chan_moments": 9, "k_col2im": 13, "k_colsum_group": 2,
                  "k_conv_dma": 4, "k_conv_gemm<2>": 187, "k_conv_gemm<4>": 12, "k_conv_mfma<1>": 5, "k_conv_mfma<8>": 1,
                  "k_dwgelu_bwd": 13, "k_dwgelu_fwd": 13, "k_im2col": 14, "k_ln_bwd": 44, "k_ln_fwd": 44,
                  "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2, "k_resid_drop": 26, "k_wgrad_dma": 1, "k_wgrad_gemm<4>": 2,
                  "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 2, "k_wgrad_group<4, 2, true>": 1},
        "eval": {"k_attn_fwd": 13, "k_bn_act": 9, "k_conv_dma": 2, "k_conv_gemm<2>": 96, "k_conv_gemm<4>": 6,
                 "k_conv_mfma<1>": 5, "k_dwgelu_fwd": 13, "k_im2col": 14, "k_ln_fwd": 44, "k_pack_jobs|k_reduce_dw": 1,
                 "k_resid_drop": 26},
    },
    "diff_2x64x64_fp32": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 19, "k_bn_reduce<T, 1>": 15,
                  "k_conv_ref": 59, "k_pack_jobs|k_reduce_dw": 1, "k_skip_bwd_pair": 4, "k_wgrad_ref": 36},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_ref": 36, "k_pack_jobs|k_reduce_dw": 1},
    },
    "diff_2x64x64_bf16_no_small": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 3, "k_bn_reduce<T, 1>": 15,
                  "k_conv_gemm<2>": 2, "k_conv_mfma<1>": 10, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 8,
                  "k_conv_tile<1>": 23, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2, "k_skip_bwd_pair": 4,
                  "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 2, "k_wgrad_group<1, 2, true>": 1,
                  "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 1, "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_mfma<1>": 4, "k_conv_mfma_x4<1>": 4,
                 "k_conv_res<1, 32, false>": 4, "k_conv_tile<1>": 12, "k_pack_jobs|k_reduce_dw": 1},
    },
    "diff_2x64x64_bf16_no_res": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 7, "k_bn_reduce<T, 1>": 13,
                  "k_conv_gemm<2>": 22, "k_conv_mfma<1>": 16, "k_conv_mfma_x4<1>": 4, "k_conv_small<1, 5>": 3,
                  "k_conv_small<bwd>": 2, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2, "k_skip_bwd_pair": 4,
                  "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 2, "k_wgrad_group<1, 2, true>": 1,
                  "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 1, "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_gemm<2>": 10, "k_conv_mfma<1>": 7, "k_conv_mfma_x4<1>": 4,
                 "k_conv_small<1, 5>": 3, "k_pack_jobs|k_reduce_dw": 1},
    },
    "diff_2x64x64_bf16_no_gemm": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 13,
                  "k_conv_mfma<1>": 7, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 8, "k_conv_small<1, 5>": 3,
                  "k_conv_small<bwd>": 2, "k_conv_tile<1>": 23, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2,
                  "k_skip_bwd_pair": 4, "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 2,
                  "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 1,
                  "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 4,
                 "k_conv_res<1, 32, false>": 4, "k_conv_small<1, 5>": 3, "k_conv_tile<1>": 12, "k_pack_jobs|k_reduce_dw": 1},
    },
    "diff_2x64x64_bf16_no_tile": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 13,
                  "k_conv_gemm<2>": 2, "k_conv_mfma<1>": 5, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 30,
                  "k_conv_res<1, 64, false>": 1, "k_conv_small<1, 5>": 3, "k_conv_small<bwd>": 2, "k_pack_jobs|k_reduce_dw": 1,
                  "k_reduce_jobs": 2, "k_skip_bwd_pair": 4, "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 2,
                  "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 1,
                  "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 4,
                 "k_conv_res<1, 32, false>": 15, "k_conv_res<1, 64, false>": 1, "k_conv_small<1, 5>": 3,
                 "k_pack_jobs|k_reduce_dw": 1},
    },
    "diff_2x64x64_bf16_virt_act": {
        "train": {"k_bn_act": 3, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 15,
                  "k_conv_gemm<2>": 2, "k_conv_mfma<1>": 5, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 16,
                  "k_conv_small<1, 5>": 5, "k_conv_tile<1>": 15, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2,
                  "k_skip_bwd_pair": 4, "k_wgrad_group<1, 1, false>": 1, "k_wgrad_group<1, 1, true>": 3,
                  "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 2, "k_wgrad_group<2, 2, false>": 1,
                  "k_wgrad_group<2, 2, true>": 4},
        "eval": {"k_bn_act": 3, "k_bn_act_pair": 4, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 4,
                 "k_conv_res<1, 32, false>": 12, "k_conv_small<1, 5>": 3, "k_conv_tile<1>": 4, "k_pack_jobs|k_reduce_dw": 1},
    },
    "diff_2x64x64_bf16_bwdsum_res": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 1, "k_bn_reduce<T, 1>": 4,
                  "k_conv_gemm<2>": 2, "k_conv_mfma<1>": 5, "k_conv_mfma_x4<1>": 4, "k_conv_res<1, 32, false>": 6,
                  "k_conv_res<bwd>": 9, "k_conv_small<1, 5>": 3, "k_conv_small<bwd>": 2, "k_conv_tile<1>": 16,
                  "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2, "k_skip_bwd_pair": 4, "k_wgrad_group<1, 1, false>": 1,
                  "k_wgrad_group<1, 1, true>": 2, "k_wgrad_group<1, 2, true>": 1, "k_wgrad_group<2, 1, true>": 1,
                  "k_wgrad_group<2, 2, false>": 1, "k_wgrad_group<2, 2, true>": 2},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_mfma<1>": 1, "k_conv_mfma_x4<1>": 4,
                 "k_conv_res<1, 32, false>": 4, "k_conv_small<1, 5>": 3, "k_conv_tile<1>": 12, "k_pack_jobs|k_reduce_dw": 1},
    },
    "diff_2x64x64_bf16_force_ref": {
        "train": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_bn_bwd_apply": 19, "k_bn_reduce<T, 0>": 19, "k_bn_reduce<T, 1>": 15,
                  "k_conv_ref": 59, "k_pack_jobs|k_reduce_dw": 1, "k_skip_bwd_pair": 4, "k_wgrad_ref": 36},
        "eval": {"k_bn_act": 15, "k_bn_act_pair": 4, "k_conv_ref": 36, "k_pack_jobs|k_reduce_dw": 1},
    },
    "changeformer_1x64x64_bf16_halo": {
        "train": {"k_attn_bwd": 13, "k_attn_fwd": 13, "k_bn_act": 9, "k_chan_moments": 9, "k_col2im": 13, "k_colsum_group": 2,
                  "k_conv_gemm<2>": 203, "k_conv_mfma<1>": 6, "k_dwgelu_bwd": 13, "k_dwgelu_fwd": 13, "k_im2col": 14,
                  "k_ln_bwd": 44, "k_ln_fwd": 44, "k_pack_jobs|k_reduce_dw": 1, "k_reduce_jobs": 2, "k_resid_drop": 26,
                  "k_wgrad_group<2, 1, true>": 1, "k_wgrad_group<2, 2, false>": 2, "k_wgrad_group<4, 2, true>": 1},
        "eval": {"k_attn_fwd": 13, "k_bn_act": 9, "k_conv_gemm<2>": 104, "k_conv_mfma<1>": 5, "k_dwgelu_fwd": 13,
                 "k_im2col": 14, "k_ln_fwd": 44, "k_pack_jobs|k_reduce_dw": 1, "k_resid_drop": 26},
    },
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_plan_is_the_pinned_one(monkeypatch, case):
    for k, v in CASES[case][6].items():
        monkeypatch.setenv(k, v)
    plan, out, _ = run_case(case)
    print(json.dumps({case: plan}))
    for mode in ("train", "eval"):
        assert sum(plan[mode].values()) == sum(PLAN[case][mode].values()), (mode, plan[mode], PLAN[case][mode])
        assert plan[mode] == PLAN[case][mode], (mode, sorted(set(plan[mode].items()) ^ set(PLAN[case][mode].items())))
    for k, t in out.items():
        assert bool(torch.isfinite(t).all()), k


def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


if __name__ == "__main__":
    import os
    import subprocess
    if len(sys.argv) > 1:      # one case in this process: a JSON line with the plan, the result hashes and the workspace size
        case = sys.argv[1]
        os.environ.update(CASES[case][6])
        plan, out, ws = run_case(case)
        print("CASE " + json.dumps({"case": case, "plan": plan, "hash": {k: _digest(t) for k, t in out.items()}, "ws_bytes": ws}))
    else:                      # every case in a process of its own (some switches are read once per process): the PLAN literal
        print("PLAN = {")
        for case in CASES:
            line = subprocess.run([sys.executable, __file__, case], check=True, capture_output=True, text=True).stdout
            rec = json.loads([ln for ln in line.splitlines() if ln.startswith("CASE ")][-1][5:])
            print(f"    {case!r}: {{")
            for mode in ("train", "eval"):
                print(f"        {mode!r}: {rec['plan'][mode]!r},")
            print("    },")
        print("}")
