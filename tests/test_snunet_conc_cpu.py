"""Siam_NestedUNet_Conc (SNUNet-CD without attention, SNUNet.py:155-243) without a GPU: the CPU restatement
(tests/snunet_conc_spec.py) against the vectors captured from the reference, and the module / C ABI / registry layout."""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from tests import snunet_conc_spec as spec
from tests.test_oracle_golden import TOL, _check_grad, _loss, _t


def _train_state(label, seed):
    st = spec.synth_state(3, label, seed)
    params = spec.trainable(st)
    for k in params:
        st[k].requires_grad_(True)
    return st, params


@pytest.mark.parametrize("label", [1, 2])
def test_spec_eval_and_train_step(golden, label):
    """The assertions and tolerances of test_oracle_golden.py::test_snunet_eval_and_train_step (the spec shares that trunk)."""
    g = golden(f"g23_snunet_conc_{label}.npz")
    seed = int(g["seed"])
    x1, x2 = _t(g["x1"]), _t(g["x2"])
    st = spec.synth_state(3, label, seed, perturb_running=True)
    assert all(st[f"final{k}.bias"].abs().min() > 0 for k in (1, 2, 3, 4)) and st["conv_final.bias"].abs().min() > 0
    with torch.no_grad():
        np.testing.assert_allclose(spec.forward(st, x1, x2).numpy(), g["logits_eval"], **TOL)
    st, params = _train_state(label, seed)
    logits = spec.forward(st, x1, x2, training=True)
    np.testing.assert_allclose(logits.detach().numpy(), g["logits_train"], rtol=2e-4, atol=5e-5)
    loss = _loss(label, logits, _t(g["target"]))
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    loss.backward()
    for k in params:
        _check_grad(k, st[k].grad, g, 3e-3, 3e-4)
    for k in [k for k in g if k.startswith("rs/")]:
        np.testing.assert_allclose(st[k[3:]].detach().numpy(), g[k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_spec_deep_supervision_step(golden):
    g = golden("g23_snunet_conc_ds_2.npz")
    assert tuple(g["weights"]) == spec.DS_WEIGHTS
    st, params = _train_state(2, int(g["seed"]))
    maps = spec.forward(st, _t(g["x1"]), _t(g["x2"]), training=True, deep_supervision=True)
    assert len(maps) == 5
    for k, m in enumerate(maps):
        np.testing.assert_allclose(m.detach().numpy(), g[f"map{k}"], rtol=2e-4, atol=5e-5, err_msg=f"map{k}")
    loss = spec.ds_loss(maps, _t(g["target"]))
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    loss.backward()
    for k in params:
        _check_grad(k, st[k].grad, g, 3e-3, 3e-4)


def test_spec_train_step_128(golden):
    g = golden("g23_snunet_conc_128.npz")
    seed = int(g["seed"])
    rng = np.random.default_rng(seed + 1)
    a = rng.standard_normal((2, 3, 128, 128)).astype(np.float32)
    b = (a + 0.5 * rng.standard_normal((2, 3, 128, 128))).astype(np.float32)
    tgt = _t((np.random.default_rng(seed + 4).random((2, 128, 128)) < 0.2).astype(np.int64))
    st, params = _train_state(2, seed)
    logits = spec.forward(st, _t(a), _t(b), training=True)
    got = logits.detach().flatten().numpy()[g["logits_sample_idx"]]
    np.testing.assert_allclose(got, g["logits_sample"], rtol=2e-4, atol=5e-5)
    loss = _loss(2, logits, tgt)
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    loss.backward()
    for k in params:
        _check_grad(k, st[k].grad, g, 3e-3, 3e-4)


def _fixture_layout(g):
    keys = [str(k) for k in g["sd_keys"]]
    shapes = [tuple(int(v) for v in row if v >= 0) for row in g["sd_shapes"]]
    return keys, shapes


@pytest.mark.parametrize("label,count", [(1, 12032297), (2, 12032442)])
def test_state_dict_layout_is_the_reference_layout(golden, label, count):
    from stcd_amd import Siam_NestedUNet_Conc

    g = golden(f"g23_snunet_conc_{label}.npz")
    keys, shapes = _fixture_layout(g)
    assert len(keys) == 240 and int(g["n_params"]) == count
    for ds in (False, True):
        m = Siam_NestedUNet_Conc(3, label, deep_supervision=ds)
        sd = m.state_dict()
        assert list(sd.keys()) == keys
        assert [tuple(v.shape) for v in sd.values()] == shapes
        assert sum(p.numel() for p in m.parameters()) == count
        st = spec.synth_state(3, label, seed=3, perturb_running=True)      # a reference-shaped checkpoint loads strictly, and round-trips
        assert list(st.keys()) == keys
        m.load_state_dict(st, strict=True)
        assert all(torch.equal(v, st[k]) for k, v in m.state_dict().items())


@pytest.mark.parametrize("arch", [_lib.ARCH_SNUNET_CONC, _lib.ARCH_SNUNET_CONC_DS])
@pytest.mark.parametrize("label", [1, 2])
def test_abi_parameter_table_and_plan(golden, arch, label):
    g = golden(f"g23_snunet_conc_{label}.npz")
    keys, shapes = _fixture_layout(g)
    want = [(k, s) for k, s in zip(keys, shapes) if "running_" not in k and "num_batches_tracked" not in k]
    l = _lib.lib()
    h = C.c_void_p()
    _lib.check(l.stcd_create(arch, 3, label, _lib.DTYPE_BF16, C.byref(h)))
    try:
        ti = _lib.TensorInfo()
        got = []
        for i in range(l.stcd_num_params(h)):
            _lib.check(l.stcd_param_info(h, i, C.byref(ti)))
            got.append((ti.name.decode(), tuple(ti.shape[k] for k in range(ti.ndim))))
        assert got == want
        assert not any(n.startswith(("ca.", "ca1.")) for n, _ in got)
        b, e = C.c_int64(), C.c_int64()
        _lib.check(l.stcd_grad_stage_range(h, 0, C.byref(b), C.byref(e)))       # one backward stage, as STCD_ARCH_SNUNET
        assert (b.value, e.value) == (0, l.stcd_param_floats(h))
        _lib.check(l.stcd_grad_stage_range(h, 1, C.byref(b), C.byref(e)))
        assert (b.value, e.value) == (0, 0)
        assert l.stcd_configure(h, 16, 250, 250) != 0 and b"divisible by 16" in l.stcd_last_error()
        _lib.check(l.stcd_configure(h, 16, 256, 256))
        maps = 5 if arch == _lib.ARCH_SNUNET_CONC_DS else 1
        assert l.stcd_output_floats(h) == maps * 16 * label * 256 * 256
        ecam = C.c_void_p()
        _lib.check(l.stcd_create(_lib.ARCH_SNUNET, 3, label, _lib.DTYPE_BF16, C.byref(ecam)))
        try:
            _lib.check(l.stcd_configure(ecam, 16, 256, 256))
            assert 0 < l.stcd_workspace_bytes(h) < l.stcd_workspace_bytes(ecam)      # the ECAM buffers are gone
        finally:
            l.stcd_destroy(ecam)
    finally:
        l.stcd_destroy(h)


def test_deep_supervision_refuses_more_than_two_classes():
    l = _lib.lib()
    h = C.c_void_p()
    assert l.stcd_create(_lib.ARCH_SNUNET_CONC_DS, 3, 3, _lib.DTYPE_BF16, C.byref(h)) != 0
    assert b"label_ch" in l.stcd_last_error()
    assert l.stcd_create(_lib.ARCH_SNUNET_CONC, 3, 3, _lib.DTYPE_BF16, C.byref(h)) == 0
    l.stcd_destroy(h)
    assert l.stcd_abi_version() == 2


def test_define_g_and_deepcopy():
    from stcd_amd import Siam_NestedUNet_Conc, SNUNet_ECAM
    from stcd_amd.networks import define_G

    net = define_G(SimpleNamespace(net_G="SNUNet_conc", n_class=2))
    assert type(net) is Siam_NestedUNet_Conc and not net.deep_supervision and net.OUT_MAPS == 1
    net = define_G(SimpleNamespace(net_G="SNUNet_conc", n_class=2, multi_scale_train="True"))
    assert type(net) is Siam_NestedUNet_Conc and net.deep_supervision and net.OUT_MAPS == 5
    assert type(define_G(SimpleNamespace(net_G="SNUNet", n_class=2, multi_scale_train="True"))) is SNUNet_ECAM
    net.eval()
    twin = copy.deepcopy(net)
    assert twin.deep_supervision and not twin.training and twin.OUT_MAPS == 5 and twin._engine.arch == "snunet_conc_ds"
    assert all(torch.equal(v, twin.state_dict()[k]) for k, v in net.state_dict().items())
    with pytest.raises(_lib.StcdError):
        net(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))       # no CPU fallback
