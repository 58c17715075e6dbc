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


# ---------------------------------------------------------------------------------------------------------------------
# The SNUNet workspace tensor table (stcd_ws_tensor_*), which tests/test_snunet_inplace_gpu.py reads.
# stcd_workspace_bytes of the commit BEFORE the table existed, label_ch 2, debug off: the table may not move a byte of the plan.
WS_BYTES_BEFORE = {
    ("snunet", "bf16", (2, 32, 64)): 332711168, ("snunet", "bf16", (16, 256, 256)): 10416133120,
    ("snunet", "fp32", (2, 32, 64)): 271798272, ("snunet", "fp32", (16, 256, 256)): 20028562944,
    ("snunet_conc", "bf16", (2, 32, 64)): 330010880, ("snunet_conc", "bf16", (16, 256, 256)): 9858392576,
    ("snunet_conc", "fp32", (2, 32, 64)): 266964224, ("snunet_conc", "fp32", (16, 256, 256)): 18917711104,
    ("snunet_conc_ds", "bf16", (2, 32, 64)): 330081024, ("snunet_conc_ds", "bf16", (16, 256, 256)): 9860510208,
    ("snunet_conc_ds", "fp32", (2, 32, 64)): 267034368, ("snunet_conc_ds", "fp32", (16, 256, 256)): 18919828736,
}
SN_ARCH = {"snunet": _lib.ARCH_SNUNET, "snunet_conc": _lib.ARCH_SNUNET_CONC, "snunet_conc_ds": _lib.ARCH_SNUNET_CONC_DS}
SN_BLOCKS = [f"conv{l}_{j}" for l in range(5) for j in range(5 - l)]                     # 15
SN_UPS = [f"Up{l}_{j}" for l in range(1, 5) for j in range(5 - l)]                       # 10
SN_F = (32, 64, 128, 256, 512)


def _sn_table(arch, dtype, shape, debug):
    l = _lib.lib()
    h = C.c_void_p()
    _lib.check(l.stcd_create(SN_ARCH[arch], 3, 2, _lib.DTYPE_IDS[dtype], C.byref(h)))
    try:
        _lib.check(l.stcd_set_debug(h, debug))
        _lib.check(l.stcd_configure(h, *shape))
        wt, out = _lib.WsTensor(), {}
        for i in range(l.stcd_ws_tensor_count(h)):
            _lib.check(l.stcd_ws_tensor_get(h, i, C.byref(wt)))
            assert wt.name.decode() not in out, wt.name
            out[wt.name.decode()] = SimpleNamespace(off=wt.offset_bytes, n=wt.n, h=wt.h, w=wt.w, c=wt.c, ld=wt.ld, dtype=wt.dtype)
        return out, l.stcd_workspace_bytes(h)
    finally:
        l.stcd_destroy(h)


def _sn_expected_names(arch, debug):
    names = set()
    for b in SN_BLOCKS:
        lvl, j = int(b[4]), int(b[6])
        names |= {f"{b}.{k}" for k in ("in", "Y1", "A1", "Y2", "Out", "dZ2", "dY2", "dY1")}
        if b != "conv0_0":
            names.add(b + ".dIn")
        if j == 0 and lvl < 4:
            names |= {b + ".P", b + ".dP"}
    names |= {f"{u}.{k}" for u in SN_UPS for k in ("in", "Y", "dY", "dIn")}
    names |= {"ecam.in", "ecam.Y", "ecam.dY", "conv_final.dY"} if arch == "snunet" else {"head.in"}
    retained = {b + ".dOut" for b in SN_BLOCKS} | {"ecam.dIn" if arch == "snunet" else "head.dIn"}
    return names | (retained if debug else set()), retained


def _sn_planned_views(B):
    """child -> (parent, channel offset, first image): the aliases the plan has on purpose (configure_snunet)."""
    v = {}
    for j in range(1, 5):
        v[f"conv0_{j}.Out"] = ("HEAD.in", 32 * (j - 1), 0)                                # x0_1..x0_4 live in the head's input
    for lvl in range(1, 5):                                                                # an encoder level reads the pooled level above;
        v[f"conv{lvl}_0.in"] = (f"conv{lvl - 1}_0.P", 0, B if lvl == 4 else 0)             # conv4_0: the date-1 half alone
        v[f"conv{lvl}_0.dIn"] = (f"conv{lvl - 1}_0.dP", 0, B if lvl == 4 else 0)
    for lvl in range(4):
        for j in range(1, 5 - lvl):                                                        # convL_J = [xL_0 A, xL_0 B, xL_1..xL_{J-1}, Up tail]
            up, low = f"Up{lvl + 1}_{j - 1}", f"conv{lvl + 1}_{j - 1}"
            v[up + ".Y"] = (f"conv{lvl}_{j}.in", (j + 1) * SN_F[lvl], 0)
            v[up + ".dY"] = (f"conv{lvl}_{j}.dIn", (j + 1) * SN_F[lvl], 0)
            v[up + ".in"] = (low + ".Out", 0, B if (j == 1 and lvl + 1 < 4) else 0)        # below an encoder level: its date-1 half
    return v


@pytest.mark.parametrize("shape", [(2, 32, 64), (16, 256, 256)])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("arch", list(SN_ARCH))
def test_workspace_tensor_table(arch, dtype, shape):
    """The table names 15 blocks, 10 transposed convs and the head; every tensor lies inside the workspace; two tensors share
    bytes only where the plan aliases them on purpose (_sn_planned_views; conv0_1..conv0_4's .Out / .dY2 interleave as 32-channel
    slices of the head's 128-channel input / gradient buffer); without the debug bit the workspace is byte for byte the size it
    was before the table existed, and the three retained copies (convL_J.dOut, ecam.dIn / head.dIn) exist with the bit alone."""
    B, H, W = shape
    es = 2 if dtype == "bf16" else 4
    off_tab, off_bytes = _sn_table(arch, dtype, shape, 0)
    on_tab, on_bytes = _sn_table(arch, dtype, shape, 1)
    want_on, retained = _sn_expected_names(arch, 1)
    assert set(off_tab) == _sn_expected_names(arch, 0)[0] and set(on_tab) == want_on
    assert len(SN_BLOCKS) == 15 and len(SN_UPS) == 10 and not (retained & set(off_tab))
    assert off_bytes == WS_BYTES_BEFORE[(arch, dtype, shape)]
    assert on_bytes > off_bytes
    assert all(vars(on_tab[k]) == vars(t) for k, t in off_tab.items()), "the debug copies moved a tensor of the plan"
    assert all(on_tab[k].off >= off_bytes for k in retained)          # the copies sit behind everything else
    head = "ecam.in" if arch == "snunet" else "head.in"
    views = {k: ((head if p == "HEAD.in" else p), c, n) for k, (p, c, n) in _sn_planned_views(B).items()}

    for tab, total in ((off_tab, off_bytes), (on_tab, on_bytes)):
        span = {}
        for k, t in tab.items():
            assert t.dtype == _lib.DTYPE_IDS[dtype] and t.ld >= t.c > 0 and t.off >= 0 and t.off % 16 == 0, k
            span[k] = (t.off, t.off + ((t.n * t.h * t.w - 1) * t.ld + t.c) * es)
            assert span[k][1] <= total, k
            lvl = int(k[4]) if k.startswith("conv") and k[4].isdigit() else (int(k[2]) if k.startswith("Up") else 0)
            if k.startswith("Up"):
                hw = (H >> lvl, W >> lvl) if k.endswith((".in", ".dIn")) else (H >> (lvl - 1), W >> (lvl - 1))
                assert (t.n, t.h, t.w, t.c) == (B, *hw, SN_F[lvl]), k
            elif k.startswith("conv") and k[4].isdigit():
                j = int(k[6])
                n = 2 * B if (j == 0 and lvl < 4) else B
                cin = (8 if lvl == 0 else SN_F[lvl - 1]) if j == 0 else (j + 1) * SN_F[lvl] + SN_F[lvl + 1]
                sfx = k.split(".")[1]
                hw = (H >> (lvl + 1), W >> (lvl + 1)) if sfx in ("P", "dP") else (H >> lvl, W >> lvl)
                assert (t.n, t.h, t.w, t.c) == (n, *hw, cin if sfx in ("in", "dIn") else SN_F[lvl]), k
            else:
                assert (t.n, t.h, t.w, t.c) == (B, H, W, 8 if k == "conv_final.dY" else 128), k
        for k, (p, coff, n0) in views.items():       # each planned view sits exactly where the plan puts it
            c, q = tab[k], tab[p]
            assert c.ld == q.ld and (c.h, c.w) == (q.h, q.w) and n0 + c.n <= q.n and coff + c.c <= q.c, (k, p)
            assert c.off == q.off + ((n0 * q.h * q.w) * q.ld + coff) * es, (k, p)
        names = sorted(tab)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                if span[a][1] <= span[b][0] or span[b][1] <= span[a][0]:
                    continue
                if views.get(a, ("",))[0] == b or views.get(b, ("",))[0] == a:
                    continue
                # the one other contact: the four 32-channel slices of the head's input / gradient buffer interleave pixel by pixel
                ta, tb = tab[a], tab[b]
                slices = a[:6] == "conv0_" and b[:6] == "conv0_" and a[6] in "1234" and b[6] in "1234" and \
                    a.split(".")[1] == b.split(".")[1] and a.split(".")[1] in ("Out", "dY2")
                d = (tb.off - ta.off) % (ta.ld * es)
                assert slices and ta.ld == tb.ld == 128 and ta.c * es <= d and d + tb.c * es <= ta.ld * es, (a, b, span[a], span[b])


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
