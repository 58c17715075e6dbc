"""CPU restatement of BIT, ``BASE_Transformer`` (/root/reference/models/networks.py:307-441 with models/help_funcs.py;
``define_G("base_transformer_pos_s4*")``), written from its description -- the yardstick of tests/test_bit_*.py on shapes no
fixture holds.  Pinned to the reference's own class by the fixtures tests/golden/g25_bit_*.npz (test_bit_cpu.py).

    trunk per date: tests/base_resnet_spec.py (resnet18, resnet_stages_num 4) up to conv_pred -> [B, 32, H/4, W/4]
    tokenizer per date: a = softmax over the n = (H/4)(W/4) positions of conv_a(x) (1x1, 32 -> 4, no bias); tokens[l] = sum_n a[l, n] x[n]
    encoder per pair: cat(tokens1, tokens2) [8, 32] + pos_embedding; x += Attention(LN(x)) (8 heads, dim_head 64, to_qkv without bias,
        to_out with bias); x += FF(LN'(x)) (32 -> 64 -> 32, exact GELU); the first / last 4 rows go back to date 1 / date 2
    decoder per date, memory m = that date's 4 encoded tokens, dec_depth layers: x += CrossAttn(LN(x), LN(m)) -- ONE LayerNorm for
        both; x += FF(LN'(x))
    both attentions scale the dot products by dim ** -0.5 = 32 ** -0.5 (not dim_head ** -0.5); LayerNorm eps 1e-5
    tail: |x1 - x2|, bilinear x4, classifier (base_resnet_spec)

All functions follow the dtype and device of the state they are given.  ``store`` (token_path / forward): a rounding function applied
where the engine's bf16 mode stores a pixel map inside the token path -- every decoder layer's output -- with a straight-through
gradient; tokens, folded matrices and all arithmetic stay in the state's precision.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import base_resnet_spec as R

HEADS, DIM, MLP, TOKENS = 8, 32, 64, 4
SCALE = DIM ** -0.5
QK_GAIN = 2.5      # synth_state: to_q / to_k of the decoder (and to_qkv's q / k rows) are this many times PyTorch's default Linear init


def _layer_specs(pre, inner, cross):
    sp = [(pre + "0.fn.norm.weight", (DIM,), "ln_w"), (pre + "0.fn.norm.bias", (DIM,), "ln_b")]
    if cross:
        sp += [(pre + "0.fn.fn.to_q.weight", (inner, DIM), "lin_qk"), (pre + "0.fn.fn.to_k.weight", (inner, DIM), "lin_qk"),
               (pre + "0.fn.fn.to_v.weight", (inner, DIM), "lin")]
    else:
        sp += [(pre + "0.fn.fn.to_qkv.weight", (3 * inner, DIM), "lin_qkv")]
    sp += [(pre + "0.fn.fn.to_out.0.weight", (DIM, inner), "lin"), (pre + "0.fn.fn.to_out.0.bias", (DIM,), "lin_b")]
    sp += [(pre + "1.fn.norm.weight", (DIM,), "ln_w"), (pre + "1.fn.norm.bias", (DIM,), "ln_b")]
    sp += [(pre + "1.fn.fn.net.0.weight", (MLP, DIM), "lin"), (pre + "1.fn.fn.net.0.bias", (MLP,), "lin_b")]
    sp += [(pre + "1.fn.fn.net.3.weight", (DIM, MLP), "lin"), (pre + "1.fn.fn.net.3.bias", (DIM,), "lin_b")]
    return sp


def param_specs(dec_depth=1, decoder_dim_head=64, out_ch=2):
    """[(name, shape, kind)] in the reference's ``state_dict`` order: pos_embedding (a parameter of the root module) first, then
    ResNet's keys, conv_a, transformer.layers.0.*, transformer_decoder.layers.*."""
    sp = [("pos_embedding", (1, 2 * TOKENS, DIM), "pos")] + R.param_specs("resnet18", 4, out_ch)
    sp += [("conv_a.weight", (TOKENS, DIM, 1, 1), "conv_a")]
    sp += _layer_specs("transformer.layers.0.", HEADS * 64, False)
    for l in range(dec_depth):
        sp += _layer_specs(f"transformer_decoder.layers.{l}.", HEADS * decoder_dim_head, True)
    return sp


def synth_state(dec_depth=1, decoder_dim_head=64, out_ch=2, seed=0, perturb_running=False):
    """Deterministic float32 state: base_resnet_spec.synth_state for ResNet's keys; pos_embedding ~ N(0, 1); Linear tensors by
    PyTorch's default rule (uniform, bound 1 / sqrt(fan_in)), with to_q / to_k (and to_qkv's q / k rows) QK_GAIN times larger:
    with the default scale the decoder's 4-way softmax is almost uniform (mean of max_j p * 4 = 1.02 - 1.05 on the reference) and
    a wrong softmax gradient would pass unnoticed; LayerNorm affine values perturbed around (1, 0), small biases."""
    st = {}
    base = R.synth_state("resnet18", 4, out_ch, seed, perturb_running)
    rng = np.random.default_rng(seed + 7919)
    for name, shape, kind in param_specs(dec_depth, decoder_dim_head, out_ch):
        if name in base:
            st[name] = base[name]
            continue
        if kind == "pos":
            v = rng.standard_normal(shape)
        elif kind == "ln_w":
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif kind == "ln_b":
            v = 0.1 * rng.standard_normal(shape)
        elif kind == "lin_b":
            v = 0.1 * rng.uniform(-1.0, 1.0, shape)
        else:
            bound = 1.0 / np.sqrt(shape[1])
            v = rng.uniform(-bound, bound, shape)
            if kind == "lin_qk":
                v *= QK_GAIN
            elif kind == "lin_qkv":
                v[:2 * shape[0] // 3] *= QK_GAIN
        st[name] = torch.from_numpy(np.asarray(v, np.float32))
    return st


GF_BIT = 1024


def fixture_index(name, numel):
    """Indices of the elements of a gradient tensor that the g25 fixtures hold: tests/_util.gf_index for ResNet's tensors, at most
    GF_BIT elements for the (many, small) tensors of the transformer layers."""
    from tests._util import gf_index
    if not name.startswith("transformer") or numel <= GF_BIT:
        return gf_index(name, numel)
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()) + numel)
    return np.sort(rng.choice(numel, GF_BIT, replace=False))


def _ln(x, st, name):
    return F.layer_norm(x, (DIM,), st[name + ".weight"], st[name + ".bias"], 1e-5)


def _heads(t):          # [b, n, heads * d] -> [b, heads, n, d]
    b, n, _ = t.shape
    return t.view(b, n, HEADS, -1).transpose(1, 2)


def _attend(q, k, v, w_out, b_out):
    attn = (torch.einsum("bhid,bhjd->bhij", _heads(q), _heads(k)) * SCALE).softmax(dim=-1)
    out = torch.einsum("bhij,bhjd->bhid", attn, _heads(v)).transpose(1, 2).flatten(2)
    return out @ w_out.t() + b_out, attn


def _ff(x, st, pre):
    h = F.gelu(_ln(x, st, pre + "1.fn.norm") @ st[pre + "1.fn.fn.net.0.weight"].t() + st[pre + "1.fn.fn.net.0.bias"])
    return h @ st[pre + "1.fn.fn.net.3.weight"].t() + st[pre + "1.fn.fn.net.3.bias"]


def tokenizer(st, x, return_attention=False):
    """x [b, 32, h, w] -> tokens [b, 4, 32]"""
    a = F.conv2d(x, st["conv_a.weight"]).flatten(2).softmax(dim=-1)
    tok = torch.einsum("bln,bcn->blc", a, x.flatten(2))
    return (tok, a) if return_attention else tok


def encoder(st, tokens):
    """tokens [B, 8, 32] (date 1's four, then date 2's) -> [B, 8, 32]"""
    pre = "transformer.layers.0."
    x = tokens + st["pos_embedding"]
    q, k, v = (_ln(x, st, pre + "0.fn.norm") @ st[pre + "0.fn.fn.to_qkv.weight"].t()).chunk(3, dim=-1)
    x = x + _attend(q, k, v, st[pre + "0.fn.fn.to_out.0.weight"], st[pre + "0.fn.fn.to_out.0.bias"])[0]
    return x + _ff(x, st, pre)


def decoder(st, x, m, store=None, return_attention=False):
    """x [b, n, 32] pixel rows, m [b, 4, 32] memory -> [b, n, 32]"""
    l, attn0 = 0, None
    while f"transformer_decoder.layers.{l}.0.fn.norm.weight" in st:
        pre = f"transformer_decoder.layers.{l}."
        xn, mn = _ln(x, st, pre + "0.fn.norm"), _ln(m, st, pre + "0.fn.norm")
        y, attn = _attend(xn @ st[pre + "0.fn.fn.to_q.weight"].t(), mn @ st[pre + "0.fn.fn.to_k.weight"].t(),
                          mn @ st[pre + "0.fn.fn.to_v.weight"].t(), st[pre + "0.fn.fn.to_out.0.weight"], st[pre + "0.fn.fn.to_out.0.bias"])
        if l == 0:
            attn0 = attn
        x = x + y
        x = x + _ff(x, st, pre)
        if store is not None:
            x = x + (store(x) - x).detach()
        l += 1
    return (x, attn0) if return_attention else x


def token_path(st, p, store=None):
    """conv_pred's output for both dates, date-major [2B, 32, h, w] -> the maps the differencing reads, same shape."""
    n2, c, h, w = p.shape
    B = n2 // 2
    tok = tokenizer(st, p)
    enc = encoder(st, torch.cat([tok[:B], tok[B:]], dim=1))
    m = torch.cat([enc[:, :TOKENS], enc[:, TOKENS:]], dim=0)
    x = decoder(st, p.flatten(2).transpose(1, 2), m, store)
    return x.transpose(1, 2).reshape(n2, c, h, w)


def forward(st, x1, x2, training, store=None):
    """[logits] -> here the logits tensor [B, out_ch, H, W] (the class wraps it in a one-element list).  training: batch statistics,
    and ``st``'s running statistics / num_batches_tracked are updated in place in the reference's call order."""
    p = torch.cat([R._single(st, x1, training, 3), R._single(st, x2, training, 3)], dim=0)
    x = token_path(st, p, store)
    B = x1.shape[0]
    x = F.interpolate(torch.abs(x[:B] - x[B:]), scale_factor=4, mode="bilinear", align_corners=False)
    x = torch.relu(R._bn(F.conv2d(x, st["classifier.0.weight"], None, 1, 1), st, "classifier.1", training))
    return F.conv2d(x, st["classifier.3.weight"], st["classifier.3.bias"], 1, 1)
