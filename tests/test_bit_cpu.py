"""BIT (``BASE_Transformer``) without a GPU: the CPU restatement (tests/bit_spec.py) against the vectors captured from the
reference's own class (G25, tests/golden/make_bit_golden.py), and the nn.Module boundary -- registry names, state_dict layout,
strict loading, deepcopy, init_weights, argument checks.  Constructing the module needs the built library, no device."""
import copy
import types

import numpy as np
import pytest
import torch

from tests import bit_spec as S
from tests._util import rel_l2_cos

FIXTURES = [("g25_bit_s4.npz", 1, 64), ("g25_bit_s4_dd8.npz", 8, 64), ("g25_bit_s4_dd8_dedim8.npz", 8, 8)]


def _f64(st):
    return {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in st.items()}


def _unused(name):
    return name.startswith("resnet.fc.") or name.startswith("resnet.layer4.")


@pytest.mark.parametrize("fixture,dd,dh", FIXTURES)
def test_spec_reproduces_the_reference_vectors(golden, fixture, dd, dh):
    """float64 against float64 (stored as float32): logits rtol = atol = 1e-6, every gradient rel-l2 <= 1e-5 (the fixture's storage
    precision)."""
    g = golden(fixture)
    seed = int(g["seed"])
    assert (int(g["dec_depth"]), int(g["decoder_dim_head"])) == (dd, dh)
    x1, x2 = torch.from_numpy(g["x1"]).double(), torch.from_numpy(g["x2"]).double()
    with torch.no_grad():
        ev = S.forward(_f64(S.synth_state(dd, dh, 2, seed, perturb_running=True)), x1, x2, training=False)
    np.testing.assert_allclose(ev.numpy(), g["eval/logits"], rtol=1e-6, atol=1e-6)
    st = _f64(S.synth_state(dd, dh, 2, seed))
    params = [n for n, _, k in S.param_specs(dd, dh, 2) if k not in ("rm", "rv", "nbt")]
    for n in params:
        st[n].requires_grad_(True)
    out = S.forward(st, x1, x2, training=True)
    np.testing.assert_allclose(out.detach().numpy(), g["train/logits"], rtol=1e-6, atol=1e-6)
    loss = torch.nn.functional.cross_entropy(out, torch.from_numpy(g["target"]))
    assert abs(loss.item() - float(g["loss"])) < 1e-9
    loss.backward()
    assert [n for n in params if st[n].grad is None] == [n for n in params if _unused(n)]
    last_b = f"transformer_decoder.layers.{dd - 1}.1.fn.fn.net.3.bias"
    worst = (0.0, "")
    for n in params:
        if st[n].grad is None:
            assert "gf/" + n not in g and float(np.abs(g["gs/" + n]).max()) == 0.0
        elif n == last_b:      # added to both dates: cancels in x1 - x2
            assert float(st[n].grad.abs().max()) < 1e-12 and float(np.abs(g["gs/" + n]).max()) < 1e-12
        else:
            got = st[n].grad.flatten().numpy()[S.fixture_index(n, st[n].numel())]
            rel, _ = rel_l2_cos(got, g["gf/" + n])
            worst = max(worst, (rel, n))
            assert rel <= 1e-5, (n, rel)
            np.testing.assert_allclose(st[n].grad.norm().item(), g["gs/" + n][1], rtol=1e-9, err_msg=n)
    assert float(st["conv_pred.bias"].grad.abs().max()) > 1e-6      # no longer cancels: the token path differs per date
    print(f"{fixture}: worst gradient rel-l2 {worst[0]:.1e} ({worst[1]})")
    for k in [k for k in g if k.startswith("rs/")]:
        np.testing.assert_allclose(st[k[3:]].numpy(), g[k], rtol=1e-6, atol=1e-7, err_msg=k)


def test_the_fixtures_exercise_the_softmaxes(golden):
    """The condition the generator asserts on its inputs, recorded in the fixtures: neither softmax of the token path is flat."""
    for fixture, _, _ in FIXTURES:
        peak_tok, peak_dec = golden(fixture)["peaks"]
        assert peak_tok >= 2.0 and peak_dec >= 1.5, fixture


@pytest.mark.parametrize("dd,dh,nkeys", [(1, 64, 158), (8, 64, 249), (8, 8, 249)])
def test_state_dict_layout_and_strict_round_trip(dd, dh, nkeys):
    from stcd_amd.bit import BASE_Transformer
    m = BASE_Transformer(3, 2, "learned", resnet_stages_num=4, dec_depth=dd, decoder_dim_head=dh, dtype="fp32")
    sd = m.state_dict()
    specs = S.param_specs(dd, dh, 2)
    assert list(sd) == [n for n, _, _ in specs] and len(sd) == nkeys
    assert list(sd)[:2] == ["pos_embedding", "resnet.conv1.weight"]
    for n, shape, _ in specs:
        assert tuple(sd[n].shape) == tuple(shape), n
    st = S.synth_state(dd, dh, 2, 5, perturb_running=True)
    m.load_state_dict(st, strict=True)
    m2 = BASE_Transformer(3, 2, "learned", resnet_stages_num=4, dec_depth=dd, decoder_dim_head=dh, dtype="fp32")
    m2.load_state_dict(m.state_dict(), strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, st[k]), k
    with pytest.raises(RuntimeError):
        m2.load_state_dict({k: v for k, v in st.items() if k != "conv_a.weight"}, strict=True)
    # the engine enumerates every parameter in named_parameters() order, pos_embedding at flat offset 0
    assert [p.name for p in m._engine.params] == [n for n, _ in m.named_parameters()]
    assert m._engine.params[0].name == "pos_embedding" and m._engine.params[0].offset == 0
    assert m.RETURNS_LIST is True


def test_holders_are_named_and_typed_like_the_reference():
    import torch.nn as nn
    from stcd_amd import bit
    m = bit.BASE_Transformer(3, 2, "learned", resnet_stages_num=4, dec_depth=8, decoder_dim_head=8, dtype="fp32")
    attn, ff = m.transformer.layers[0]
    assert type(attn).__name__ == "Residual" and type(attn.fn).__name__ == "PreNorm" and type(attn.fn.fn).__name__ == "Attention"
    assert isinstance(attn.fn.norm, nn.LayerNorm) and isinstance(attn.fn.fn.to_qkv, nn.Linear) and attn.fn.fn.to_qkv.bias is None
    assert type(ff.fn.fn).__name__ == "FeedForward" and isinstance(ff.fn.fn.net[1], nn.GELU) and isinstance(ff.fn.fn.net[3], nn.Linear)
    cross, _ = m.transformer_decoder.layers[7]
    assert type(cross).__name__ == "Residual2" and type(cross.fn).__name__ == "PreNorm2" and type(cross.fn.fn).__name__ == "Cross_Attention"
    assert cross.fn.fn.to_q.weight.shape == (64, 32) and cross.fn.fn.to_out[0].weight.shape == (32, 64)
    assert cross.fn.fn.scale == 32 ** -0.5 and attn.fn.fn.scale == 32 ** -0.5
    assert isinstance(m.conv_a, nn.Conv2d) and m.conv_a.bias is None and m.token_len == 4


def test_deepcopy_keeps_configuration_and_weights():
    from stcd_amd.bit import BASE_Transformer
    m = BASE_Transformer(3, 1, "learned", resnet_stages_num=4, dec_depth=8, decoder_dim_head=8, output_sigmoid=True, dtype="fp32")
    c = copy.deepcopy(m)
    assert type(c) is BASE_Transformer and c.dec_depth == 8 and c.decoder_dim_head == 8 and c.output_sigmoid is True
    assert c._engine.arch == m._engine.arch == "bit_s4_dd8_dh8" and c._engine.dtype == "fp32"
    assert c.pos_embedding is not m.pos_embedding
    for (k, a), (_, b) in zip(m.state_dict().items(), c.state_dict().items()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("kw", [dict(tokenizer=False), dict(token_trans=False), dict(with_decoder=False), dict(decoder_softmax=False),
                                dict(with_decoder_pos="learned"), dict(with_decoder_pos="fix"), dict(with_pos=None), dict(with_pos="fix"),
                                dict(if_upsample_2x=False), dict(resnet_stages_num=5), dict(backbone="resnet34"), dict(dec_depth=4),
                                dict(decoder_dim_head=16), dict(enc_depth=2), dict(dim_head=32), dict(token_len=8), dict(output_nc=3)])
def test_unsupported_arguments_are_refused(kw):
    from stcd_amd.bit import BASE_Transformer
    args = dict(input_nc=3, output_nc=2, with_pos="learned", resnet_stages_num=4)
    args.update(kw)
    with pytest.raises(NotImplementedError, match=r"\(1, 64\) / \(8, 64\) / \(8, 8\)"):
        BASE_Transformer(**args)


def _args(name):
    return types.SimpleNamespace(net_G=name, n_class=5)


@pytest.mark.parametrize("name,dd,dh", [("bit_pos_s4", 1, 64), ("bit_pos_s4_dd8", 8, 64), ("bit_pos_s4_dd8_dedim8", 8, 8)])
def test_define_g_builds_the_configuration(name, dd, dh):
    import stcd_amd
    from stcd_amd import networks
    from stcd_amd.bit import BASE_Transformer
    torch.manual_seed(3)
    net = networks.define_G(_args(name))
    assert type(net) is BASE_Transformer and networks.BASE_Transformer is BASE_Transformer and stcd_amd.BASE_Transformer is BASE_Transformer
    assert (net.dec_depth, net.decoder_dim_head, net.enc_depth, net.dim_head, net.token_len, net.resnet_stages_num) == (dd, dh, 1, 64, 4, 4)
    assert len(net.transformer_decoder.layers) == dd and net.transformer_decoder.layers[0][0].fn.fn.to_k.weight.shape == (8 * dh, 32)
    assert net.classifier[3].out_channels == 2 and net.output_sigmoid is False           # args.n_class is ignored (networks.py:174-182)
    # init_net ran init_weights: Linear (and Conv) weights ~ N(0, 0.02), Linear bias 0; pos_embedding (no module) keeps randn;
    # LayerNorm is neither Conv, Linear nor BatchNorm2d: untouched
    ca = net.transformer_decoder.layers[dd - 1][0].fn.fn
    ffn = net.transformer.layers[0][1].fn.fn.net
    assert abs(float(net.transformer.layers[0][0].fn.fn.to_qkv.weight.detach().std()) - 0.02) < 2e-3
    assert abs(float(ca.to_q.weight.detach().std()) - 0.02) < 4e-3 and abs(float(ffn[0].weight.detach().std()) - 0.02) < 2e-3
    assert float(ca.to_out[0].bias.detach().abs().max()) == 0.0 and float(ffn[3].bias.detach().abs().max()) == 0.0
    assert abs(float(net.conv_a.weight.detach().std()) - 0.02) < 6e-3
    assert 0.8 < float(net.pos_embedding.detach().std()) < 1.2
    ln = net.transformer_decoder.layers[0][0].fn.norm
    assert float((ln.weight.detach() - 1).abs().max()) == 0.0 and float(ln.bias.detach().abs().max()) == 0.0


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "base_transformer_pos_s4_dd8", "base_transformer_pos_s4_dd8_dedim8"])
def test_the_reference_names_still_raise(name):
    from stcd_amd import networks
    with pytest.raises(NotImplementedError, match="outside the accelerated hot path"):
        networks.define_G(_args(name))
