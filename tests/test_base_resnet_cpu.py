"""``ResNet`` (define_G name "base_resnet18", the BIT family's CNN baseline) without a GPU: the CPU restatement
(tests/base_resnet_spec.py) against the vectors captured from the reference's own class (G24), and the nn.Module boundary --
registry, state_dict layout, strict loading, init_weights, argument checks.  Constructing the module needs the built library, no
device."""
import types

import numpy as np
import pytest
import torch

from tests import base_resnet_spec as S
from tests._util import check_grad

FIXTURES = [("g24_base_resnet_r18_s5.npz", "resnet18", 5), ("g24_base_resnet_r18_s4.npz", "resnet18", 4),
            ("g24_base_resnet_r34_s5.npz", "resnet34", 5)]


def _f64(st):
    return {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in st.items()}


@pytest.mark.parametrize("fixture,backbone,stages", FIXTURES)
def test_spec_reproduces_the_reference_vectors(golden, fixture, backbone, stages):
    """float64 against float64 (stored as float32): what is left is the fixture's storage precision."""
    g = golden(fixture)
    seed = int(g["seed"])
    x1, x2 = torch.from_numpy(g["x1"]).double(), torch.from_numpy(g["x2"]).double()
    with torch.no_grad():
        ev = S.forward(_f64(S.synth_state(backbone, stages, 2, seed, perturb_running=True)), x1, x2, training=False)
    np.testing.assert_allclose(ev.numpy(), g["eval/logits"], rtol=1e-5, atol=1e-5)
    st = _f64(S.synth_state(backbone, stages, 2, seed))
    params = [n for n, _, k in S.param_specs(backbone, stages, 2) if k in ("conv", "fc", "bias", "bn_w", "bn_b")]
    for n in params:
        st[n].requires_grad_(True)
    out = S.forward(st, x1, x2, training=True)
    np.testing.assert_allclose(out.detach().numpy(), g["train/logits"], rtol=1e-5, atol=1e-5)
    loss = torch.nn.functional.cross_entropy(out, torch.from_numpy(g["target"]))
    assert abs(loss.item() - float(g["loss"])) < 1e-9
    loss.backward()
    unused = [n for n in params if st[n].grad is None]
    assert unused == [n for n in params if n.startswith("resnet.fc.") or (stages == 4 and n.startswith("resnet.layer4."))]
    for n in params:
        if st[n].grad is None:
            assert "gf/" + n not in g and float(np.abs(g["gs/" + n]).max()) == 0.0
        elif n == "conv_pred.bias":            # cancels in x1 - x2
            assert float(st[n].grad.abs().max()) < 1e-12 and float(np.abs(g["gs/" + n]).max()) < 1e-12
        else:
            check_grad(n, st[n].grad, g, rel_max=1e-5, cos_min=1 - 1e-9)
    for k in [k for k in g if k.startswith("rs/")]:
        np.testing.assert_allclose(st[k[3:]].numpy(), g[k], rtol=1e-6, atol=1e-7, err_msg=k)
    assert int(g["rs/resnet.bn1.num_batches_tracked"]) == 2 and int(g["rs/classifier.1.num_batches_tracked"]) == 1


def _args(name):
    return types.SimpleNamespace(net_G=name, n_class=5)


def test_define_g_builds_the_class():
    from stcd_amd import networks
    from stcd_amd.bit import ResNet
    import stcd_amd
    net = networks.define_G(_args("base_resnet18"))
    assert type(net) is ResNet and networks.ResNet is ResNet and stcd_amd.ResNet is ResNet
    assert net.resnet_stages_num == 5 and net.conv_pred.in_channels == 512
    assert net.classifier[3].out_channels == 2           # the reference ignores args.n_class here (networks.py:173)
    assert net.output_sigmoid is False
    # init_net ran init_weights: Conv / Linear weights ~ N(0, 0.02), bias 0; BatchNorm2d weight ~ N(1, 0.02)
    assert abs(float(net.resnet.layer3[0].conv1.weight.detach().std()) - 0.02) < 2e-3
    assert abs(float(net.resnet.fc.weight.detach().std()) - 0.02) < 2e-3 and float(net.resnet.fc.bias.detach().abs().max()) == 0.0
    assert abs(float(net.classifier[1].weight.detach().mean()) - 1.0) < 2e-2 and float(net.classifier[1].weight.detach().std()) > 1e-3
    assert float(net.conv_pred.bias.detach().abs().max()) == 0.0


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "base_transformer_pos_s4_dd8", "base_transformer_pos_s4_dd8_dedim8"])
def test_the_transformer_names_stay_off_the_path(name):
    from stcd_amd import networks
    with pytest.raises(NotImplementedError, match="outside the accelerated hot path"):
        networks.define_G(_args(name))


@pytest.mark.parametrize("backbone", ["resnet18", "resnet34"])
@pytest.mark.parametrize("stages", [5, 4])
def test_state_dict_layout_and_strict_round_trip(backbone, stages):
    from stcd_amd.bit import ResNet
    m = ResNet(3, 2, resnet_stages_num=stages, backbone=backbone, dtype="fp32")
    sd = m.state_dict()
    specs = S.param_specs(backbone, stages, 2)
    assert list(sd) == [n for n, _, _ in specs]
    assert len(sd) == (132 if backbone == "resnet18" else 228)
    for n, shape, _ in specs:
        assert tuple(sd[n].shape) == tuple(shape), n
    assert "resnet.fc.weight" in sd and "resnet.layer4.1.bn2.running_var" in sd          # kept at 4 stages too
    st = S.synth_state(backbone, stages, 2, 5, perturb_running=True)
    m.load_state_dict(st, strict=True)
    m2 = ResNet(3, 2, resnet_stages_num=stages, backbone=backbone, dtype="fp32")
    m2.load_state_dict(m.state_dict(), strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, st[k]), k
    # the engine enumerates every parameter, in this order (HipChangeDetector._check_layout ran in the constructor)
    assert [p.name for p in m._engine.params] == [n for n, _ in m.named_parameters()]


def test_deepcopy_keeps_configuration_and_weights():
    import copy
    from stcd_amd.bit import ResNet
    m = ResNet(3, 1, resnet_stages_num=4, backbone="resnet34", output_sigmoid=True, dtype="fp32")
    c = copy.deepcopy(m)
    assert c.resnet_stages_num == 4 and c.output_sigmoid is True and c._engine.arch == "base_resnet34_s4" and c._engine.dtype == "fp32"
    for (k, a), (_, b) in zip(m.state_dict().items(), c.state_dict().items()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("kw", [dict(backbone="resnet50"), dict(resnet_stages_num=3), dict(if_upsample_2x=False), dict(input_nc=4),
                                dict(output_nc=3), dict(backbone="vgg16")])
def test_unsupported_arguments_are_refused(kw):
    from stcd_amd.bit import ResNet
    args = dict(input_nc=3, output_nc=2)
    args.update(kw)
    with pytest.raises(NotImplementedError, match="resnet18 / resnet34"):
        ResNet(**args)


def test_backbone_weights_from_a_file(tmp_path):
    from stcd_amd.bit import ResNet
    st = S.synth_state("resnet18", 5, 2, 9)
    back = {k[len("resnet."):]: v for k, v in st.items() if k.startswith("resnet.")}
    path = str(tmp_path / "backbone.pth")
    torch.save(back, path)
    m = ResNet(3, 2, backbone_weights=path, dtype="fp32")
    assert torch.equal(m.resnet.layer4[1].conv2.weight, back["layer4.1.conv2.weight"]) and torch.equal(m.resnet.fc.bias, back["fc.bias"])
    with pytest.raises(KeyError):
        ResNet(3, 2, backbone_weights="no-such-weights", dtype="fp32")
