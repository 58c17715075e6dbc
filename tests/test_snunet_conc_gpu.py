"""Siam_NestedUNet_Conc (SNUNet-CD without attention, SNUNet.py:155-243) through the HIP engine, both forms (fused map /
deep supervision), against the vectors captured from the reference (tests/golden/g23_snunet_conc_*.npz) and, at shapes
without a fixture, against the CPU restatement tests/snunet_conc_spec.py.  Every bound is the one the project's SNUNet_ECAM
tests use (tests/test_engine_gpu.py): the trunk is the same, the head adds one 128-term dot product."""
import os

import numpy as np
import pytest
import torch

from stcd_amd import Siam_NestedUNet_Conc
from tests import snunet_conc_spec as spec
from tests._util import ACHIEVED, REL_L2_MAX, COS_MIN, check_grad, gf_index, rel_l2_cos, t, zero_grad_by_construction
from tests.test_engine_gpu import BF16_GRAD, BF16_LOGIT_ERR, BF16_LOSS_ERR, loss_fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(label, dtype, st, ds=False, train=True):
    m = Siam_NestedUNet_Conc(3, label, dtype=dtype, deep_supervision=ds)
    m.load_state_dict(st)
    m.to(DEV)
    return m.train() if train else m.eval()


@pytest.mark.parametrize("label", [1, 2])
def test_fp32_matches_reference_vectors(golden, label):
    """The assertions of test_snunet_fp32_matches_reference_vectors: eval and train logits, loss, every parameter gradient and
    the BatchNorm running statistics against the reference's."""
    g = golden(f"g23_snunet_conc_{label}.npz")
    seed = int(g["seed"])
    x1, x2 = t(g["x1"]).to(DEV), t(g["x2"]).to(DEV)
    m = _model(label, "fp32", spec.synth_state(3, label, seed, perturb_running=True), train=False)
    with torch.no_grad():
        out = m(x1, x2)
        assert torch.is_tensor(out)
        np.testing.assert_allclose(out.cpu().numpy(), g["logits_eval"], rtol=1e-3, atol=2e-4)
    m = _model(label, "fp32", spec.synth_state(3, label, seed))
    logits = m(x1, x2)
    print("max |dlogit|", np.abs(logits.detach().cpu().numpy() - g["logits_train"]).max())
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["logits_train"], rtol=1e-3, atol=2e-4)
    loss = loss_fn(label, logits, t(g["target"]).to(DEV))
    print("loss", loss.item(), float(g["loss"]))
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    for name, p in m.named_parameters():
        check_grad(name, p.grad, g, tag=f"fp32 snunet_conc({label}) vs reference G23")
    sd = m.state_dict()
    for k in [k for k in g if k.startswith("rs/")]:
        np.testing.assert_allclose(sd[k[3:]].cpu().numpy(), g[k], rtol=1e-4, atol=1e-6, err_msg=k)


def test_fp32_deep_supervision_matches_reference_vectors(golden):
    """The five maps, the weighted loss sum_k w_k CE(map_k) and every gradient, same bounds; the last map is the plain engine's
    output bit for bit."""
    g = golden("g23_snunet_conc_ds_2.npz")
    seed = int(g["seed"])
    x1, x2 = t(g["x1"]).to(DEV), t(g["x2"]).to(DEV)
    st = spec.synth_state(3, 2, seed)
    m = _model(2, "fp32", st, ds=True)
    maps = m(x1, x2)
    assert isinstance(maps, list) and len(maps) == 5
    for k, p in enumerate(maps):
        print(f"map{k} max |d|", np.abs(p.detach().cpu().numpy() - g[f"map{k}"]).max())
        np.testing.assert_allclose(p.detach().cpu().numpy(), g[f"map{k}"], rtol=1e-3, atol=2e-4, err_msg=f"map{k}")
    loss = spec.ds_loss(maps, t(g["target"]).to(DEV), tuple(g["weights"]))
    print("loss", loss.item(), float(g["loss"]))
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    for name, p in m.named_parameters():
        check_grad(name, p.grad, g, tag="fp32 snunet_conc deep supervision vs reference G23")
    plain = _model(2, "fp32", st)(x1, x2)
    assert torch.equal(plain, maps[-1])
    with torch.no_grad():       # eval mode splits the same way
        ev = _model(2, "fp32", st, ds=True, train=False)(x1, x2)
        assert isinstance(ev, list) and len(ev) == 5 and all(e.shape == (2, 2, 32, 32) for e in ev)
        assert torch.equal(ev[-1], _model(2, "fp32", st, train=False)(x1, x2))


def test_deep_supervision_loss_on_last_map_only(golden):
    """A loss on out[-1] alone: the four side maps carry a zero gradient, and the step equals the plain engine's."""
    g = golden("g23_snunet_conc_2.npz")
    seed = int(g["seed"])
    x1, x2, tgt = t(g["x1"]).to(DEV), t(g["x2"]).to(DEV), t(g["target"]).to(DEV)
    st = spec.synth_state(3, 2, seed)
    grads = []
    for ds in (False, True):
        m = _model(2, "fp32", st, ds=ds)
        out = m(x1, x2)
        loss_fn(2, out[-1] if ds else out, tgt).backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
        if ds:
            for name, p in m.named_parameters():
                check_grad(name, p.grad, g)
    for n in grads[0]:
        rel = (grads[0][n] - grads[1][n]).abs().max().item() / max(grads[0][n].abs().max().item(), 1e-30)
        assert rel < 1e-5, (n, rel)


@pytest.mark.parametrize("label", [1, 2])
def test_bf16_tracks_reference_vectors(golden, label):
    """The bounds of test_snunet_bf16_tracks_reference_vectors: mean |dlogit| < 4e-2, max < 0.35 (times max(1, max |logit|)),
    loss within 2e-2, gradient cosine > 0.9 for every tensor of >= 256 elements (> 0.8 in the first encoder block)."""
    g = golden(f"g23_snunet_conc_{label}.npz")
    seed = int(g["seed"])
    x1, x2 = t(g["x1"]).to(DEV), t(g["x2"]).to(DEV)
    m = _model(label, "bf16", spec.synth_state(3, label, seed))
    logits = m(x1, x2)
    err = np.abs(logits.detach().cpu().numpy() - g["logits_train"])
    scale = max(1.0, float(np.abs(g["logits_train"]).max()))
    print("mean / max |dlogit|, scale", err.mean(), err.max(), scale)
    assert err.mean() < 4e-2 * scale and err.max() < 0.35 * scale, (err.mean(), err.max(), scale)
    loss = loss_fn(label, logits, t(g["target"]).to(DEV))
    print("loss", loss.item(), float(g["loss"]))
    assert abs(loss.item() - float(g["loss"])) < 2e-2 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    worst = {"rest": 1.0, "first": 1.0}
    low = []
    for name, p in m.named_parameters():
        if zero_grad_by_construction(name) or p.numel() < 256:
            continue
        a = p.grad.flatten().cpu().double().numpy()[gf_index(name, p.numel())]
        _, cos = rel_l2_cos(a, g["gf/" + name])
        k = "first" if name.startswith("conv0_0.") else "rest"
        worst[k] = min(worst[k], cos)
        if cos <= (0.8 if k == "first" else 0.9):
            low.append((name, cos))
    print("worst cosine (all but conv0_0, conv0_0)", worst)
    ACHIEVED[f"bf16 snunet_conc({label}) vs reference G23 [worst cosine: all but conv0_0, conv0_0]"] = (worst["rest"], worst["first"])
    assert not low, low


def test_bf16_train_step_128_tracks_reference_vectors(golden):
    """The `snunet` row of test_train_step_128_tracks_reference_vectors (bf16): mean |dlogit| <= 6 % of mean |logit|, loss within
    2e-2, per-tensor gradient cosine / relative l2 per BF16_GRAD["snunet"]; fp32 first, at the fp32 bounds."""
    g = golden("g23_snunet_conc_128.npz")
    seed = int(g["seed"])
    rng = np.random.default_rng(seed + 1)
    a = rng.standard_normal((2, 3, 128, 128)).astype(np.float32)
    b = (a + 0.5 * rng.standard_normal((2, 3, 128, 128))).astype(np.float32)
    x1, x2 = t(a).to(DEV), t(b).to(DEV)
    tgt = t((np.random.default_rng(seed + 4).random((2, 128, 128)) < 0.2).astype(np.int64)).to(DEV)
    st = spec.synth_state(3, 2, seed)

    m = _model(2, "fp32", st)
    logits = m(x1, x2)
    got = logits.detach().flatten().cpu().numpy()[g["logits_sample_idx"]]
    loss = torch.nn.functional.cross_entropy(logits, tgt)
    loss.backward()
    np.testing.assert_allclose(got, g["logits_sample"], rtol=1e-3, atol=1e-4)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    for name, p in m.named_parameters():
        check_grad(name, p.grad, g, tag="fp32 snunet_conc 128x128 step vs reference G23")

    m = _model(2, "bf16", st)
    logits = m(x1, x2)
    got = logits.detach().flatten().cpu().numpy()[g["logits_sample_idx"]]
    loss = torch.nn.functional.cross_entropy(logits, tgt)
    loss.backward()
    err = np.abs(got - g["logits_sample"]).mean() / float(g["logits_absmean"])
    dloss = abs(loss.item() - float(g["loss"]))
    worst = [0.0, 1.0, 0.0, 1.0]
    for name, p in m.named_parameters():
        if zero_grad_by_construction(name) or p.numel() < 64:
            continue
        s = p.grad.flatten().cpu().double().numpy()[gf_index(name, p.numel())]
        rel, cos = rel_l2_cos(s, g["gf/" + name])
        k = 2 if name.startswith("conv0_0.") else 0
        worst[k], worst[k + 1] = max(worst[k], rel), min(worst[k + 1], cos)
    print("bf16 128: logit err, dloss, worst (rel, cos) rest / first", err, dloss, worst)
    ACHIEVED["bf16 snunet_conc 128x128 step vs reference G23 [all but first block]"] = (worst[0], worst[1])
    ACHIEVED["bf16 snunet_conc 128x128 step vs reference G23 [first encoder block]"] = (worst[2], worst[3])
    ACHIEVED["bf16 snunet_conc 128x128 step vs reference G23 [mean |dlogit| / mean |logit|, |dloss|]"] = (float(err), dloss)
    assert err < BF16_LOGIT_ERR, err
    assert dloss < BF16_LOSS_ERR, (loss.item(), float(g["loss"]))
    cos_min, rel_max = BF16_GRAD["snunet"]
    assert worst[1] >= cos_min and worst[0] <= rel_max, worst
    assert worst[3] >= cos_min and worst[2] <= rel_max, worst


@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("label", [1, 2])
def test_fp32_odd_shape_against_the_spec(label, ds):
    """[3,3,48,80] (no fixture): logits and every gradient against the CPU restatement, the fp32 bounds."""
    seed = 411 + label
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((3, 3, 48, 80)).astype(np.float32)
    b = (a + 0.5 * rng.standard_normal((3, 3, 48, 80))).astype(np.float32)
    tgt = t((rng.random((3, 48, 80)) < 0.25).astype(np.int64))
    wts = (0.5, 0.5, 0.5, 0.8, 1.0)

    def total(maps, y):
        maps = maps if isinstance(maps, list) else [maps]
        return sum(w * loss_fn(label, p, y) for w, p in zip(wts[-len(maps):], maps))

    st = spec.synth_state(3, label, seed)
    params = spec.trainable(st)
    for k in params:
        st[k].requires_grad_(True)
    ref = spec.forward(st, t(a), t(b), training=True, deep_supervision=ds)
    ref_loss = total(ref, tgt)
    ref_loss.backward()

    m = _model(label, "fp32", spec.synth_state(3, label, seed), ds=ds)
    out = m(t(a).to(DEV), t(b).to(DEV))
    for p, r in zip(out if ds else [out], ref if ds else [ref]):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().numpy(), rtol=1e-3, atol=2e-4)
    loss = total(out, tgt.to(DEV))
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * max(1.0, abs(ref_loss.item()))
    loss.backward()
    for name, p in m.named_parameters():
        want = st[name].grad
        if zero_grad_by_construction(name):
            assert p.grad.abs().max().item() < 1e-5, name
            continue
        rel, cos = rel_l2_cos(p.grad.cpu().numpy(), want.numpy())
        assert rel <= REL_L2_MAX and cos >= COS_MIN, (name, rel, cos)


@pytest.mark.parametrize("ds", [False, True])
def test_full_size_properties_bf16(ds):
    """16 pairs of 256 x 256, bf16, as test_full_size_properties_bf16: (a) the eval batch equals its two halves bit for bit;
    (b) doubling the output gradient doubles every parameter gradient (rel < 5e-5); (c) two identical training steps give
    identical bytes, logits and all gradients -- with a gradient on all five maps for the deep-supervision form."""
    from stcd_amd import synth

    a, b, _ = synth.make_batch(16, 256, 256, seed=79)
    A, B = t(a).to(DEV), t(b).to(DEV)
    torch.manual_seed(7)
    m = Siam_NestedUNet_Conc(3, 2, dtype="bf16", deep_supervision=ds).to(DEV)
    with torch.no_grad():
        for k in (1, 2, 3, 4):
            getattr(m, f"final{k}").bias.normal_(0, 0.05)
        m.conv_final.bias.normal_(0, 0.05)
    cat = (lambda o: torch.cat(o)) if ds else (lambda o: o)
    m.eval()
    with torch.no_grad():
        full = cat(m(A, B)).clone()
        maps = (lambda o: [x.clone() for x in o]) if ds else (lambda o: [o.clone()])
        h0 = maps(m(A[:8], B[:8]))
        h1 = maps(m(A[8:], B[8:]))
    assert torch.isfinite(full).all()
    assert torch.equal(full, torch.cat([torch.cat([p, q]) for p, q in zip(h0, h1)]))
    m.train()
    runs = []
    wts = (0.5, 0.5, 0.5, 0.8, 1.0) if ds else (1.0,)
    for scale in (1.0, 2.0, 1.0):
        m.zero_grad(set_to_none=True)
        out = m(A, B)
        outs = out if ds else [out]
        torch.autograd.backward(outs, [torch.ones_like(o) * (1e-3 * scale * w) for o, w in zip(outs, wts)])
        runs.append((torch.cat(outs).detach().clone(), torch.cat([p.grad.flatten() for p in m.parameters()]).clone()))
        if scale == 1.0 and len(runs) == 1:
            for name, p in m.named_parameters():
                assert torch.isfinite(p.grad).all(), name
                if not zero_grad_by_construction(name):
                    assert p.grad.abs().max().item() > 0, name
    # the running statistics move between the passes, the batch statistics (what a training forward uses) do not
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], runs[2][0])
    rel = ((runs[1][1] - 2.0 * runs[0][1]).abs().max() / runs[1][1].abs().max()).item()
    print("linearity rel", rel)
    assert rel < 5e-5, rel
    assert torch.equal(runs[0][1], runs[2][1])


def test_bf16_kernel_families_agree():
    """The recipe and bounds of test_bf16_kernel_families_agree (4 x 64 x 64): the reference FMA kernels, the generic MFMA kernels
    and the default path reach the same head and agree: mean |dlogit| < 2e-2, max < 0.2, loss within 1e-2, gradient cosine > 0.99,
    running statistics within 2e-3."""
    from tests.test_engine_gpu import _TOGGLES

    seed, label, n, h, w = 123, 2, 4, 64, 64
    rng = np.random.default_rng(seed)
    x1 = t(rng.standard_normal((n, 3, h, w)).astype(np.float32)).to(DEV)
    x2 = t(rng.standard_normal((n, 3, h, w)).astype(np.float32)).to(DEV)
    tgt = t((rng.random((n, h, w)) < 0.3).astype(np.int64)).to(DEV)
    st = spec.synth_state(3, label, seed)
    res = {}
    generic = {k: "1" for k in _TOGGLES[1:]}
    for tag, env in (("ref", {"STCD_FORCE_REF_KERNELS": "1"}), ("generic", generic), ("default", {})):
        for k in _TOGGLES:
            os.environ.pop(k, None)
        os.environ.update(env)
        try:
            m = Siam_NestedUNet_Conc(3, label, dtype="bf16", deep_supervision=True)
        finally:
            for k in env:
                os.environ.pop(k, None)
        m.load_state_dict(st)
        m.to(DEV).train()
        maps = m(x1, x2)
        loss = spec.ds_loss(maps, tgt)
        loss.backward()
        gr = torch.cat([p.grad.flatten() for p in m.parameters()]).cpu().double()
        res[tag] = (torch.cat(maps).detach().cpu(), loss.item(), gr, m.state_dict()["conv0_0.bn2.running_var"].cpu())
    for tag in ("generic", "default"):
        d = (res[tag][0] - res["ref"][0]).abs()
        cos = (res[tag][2] @ res["ref"][2] / (res[tag][2].norm() * res["ref"][2].norm())).item()
        print(tag, "mean / max |dlogit|", d.mean().item(), d.max().item(), "dloss", abs(res[tag][1] - res["ref"][1]), "cos", cos)
        assert d.mean().item() < 2e-2 and d.max().item() < 0.2, (tag, d.mean().item(), d.max().item())
        assert abs(res[tag][1] - res["ref"][1]) < 1e-2, tag
        assert cos > 0.99, (tag, cos)
        np.testing.assert_allclose(res[tag][3].numpy(), res["ref"][3].numpy(), rtol=2e-3)


def test_multi_scale_training_steps_and_inference_tools():
    """Three FlatAdamW steps of CDTrainer's multi-scale loss (multi_scale_train="True", multi_pred_weights (0.5, 0.5, 0.5, 0.8, 1))
    on a fixed synthetic batch: finite, and lower after the third step than before the first; predict_scene and
    selftrain.score_batch take the model in both forms."""
    from types import SimpleNamespace

    from stcd_amd import selftrain, synth
    from stcd_amd.networks import define_G
    from stcd_amd.optim import FlatAdamW
    from stcd_amd.scene import predict_scene

    a, b, y = synth.make_batch(4, 64, 64, seed=31)
    A, B, L = t(a).to(DEV), t(b).to(DEV), t(y).to(DEV).long()
    torch.manual_seed(11)
    net = define_G(SimpleNamespace(net_G="SNUNet_conc", n_class=2, multi_scale_train="True"), init_type="kaiming", gpu_ids=[0])
    assert net.deep_supervision
    net.train()
    opt = FlatAdamW(net, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    weights = (0.5, 0.5, 0.5, 0.8, 1.0)

    def step(update):
        opt.zero_grad()
        preds = net(A, B)
        assert isinstance(preds, list) and len(preds) == 5
        loss = sum(w * torch.nn.functional.cross_entropy(p, L) for w, p in zip(weights, preds))
        if update:
            loss.backward()
            opt.step()
        return loss.item()

    losses = [step(True) for _ in range(3)]
    with torch.no_grad():
        after = step(False)
    print("losses", losses, after)
    assert all(np.isfinite(losses)) and np.isfinite(after)
    assert after < losses[0], (losses, after)

    rng = np.random.default_rng(3)
    sa = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    sb = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    plain = Siam_NestedUNet_Conc(3, 2, dtype="bf16").to(DEV)
    plain.load_state_dict(net.state_dict())
    masks = [predict_scene(mm, sa, sb, tile=32, stride=32, batch=5).mask for mm in (net, plain)]
    assert masks[0].shape == (96, 128) and torch.equal(masks[0], masks[1])
    assert net.training and plain.training          # previous modes restored
    sc = selftrain.score_batch([plain, net], A, B)
    assert sc.mask.shape == (4, 64, 64)
    agree = sc.agree.cpu().numpy()[:, 0]
    assert (agree[:, 0, 1] == 0).all() and (agree[:, 1, 0] == 0).all()       # same weights, same last map: full agreement


def test_graphed_step_and_gradient_hook():
    """GraphedTrainStep (the recipe of test_graphed_training_step_equals_the_eager_one) on the deep-supervision form with a loss on
    all five maps: the replayed steps end bit-identical to the eager ones; and a grad_stage_hook sees the whole flat gradient at
    stage 0 (one backward stage) with the bytes of the hook-free backward."""
    from stcd_amd import synth
    from stcd_amd.optim import FlatAdam
    from stcd_amd.train_loop import GraphedTrainStep, Poly

    a, b, lab = synth.make_batch(12, 64, 64, seed=9)
    A, B, L = t(a).to(DEV), t(b).to(DEV), t(lab).to(DEV)
    loss_of = lambda out, y: spec.ds_loss(out, y)

    def build():
        torch.manual_seed(3)
        return Siam_NestedUNet_Conc(3, 2, dtype="bf16", deep_supervision=True).to(DEV).train()

    results = []
    for graphed in (False, True):
        m = build()
        opt = FlatAdam(m, lr=1e-3)
        sched = Poly(opt, 1, 6)
        step = GraphedTrainStep(m, opt, loss_of, (A[:2], B[:2]), L[:2]) if graphed else None
        losses = []
        for it in range(6):
            sl = slice(2 * it, 2 * it + 2)
            if graphed:
                losses.append(step(A[sl], B[sl], L[sl]).clone())
            else:
                opt.zero_grad(set_to_none=True)
                loss = loss_of(m(A[sl], B[sl]), L[sl])
                loss.backward()
                opt.step()
                losses.append(loss.detach().clone())
            sched.step(epoch=0)
        torch.cuda.synchronize()
        results.append((torch.stack(losses).cpu(), m._flat_params.detach().cpu().clone(), m._flat_bn.detach().cpu().clone()))
    assert torch.equal(results[0][0], results[1][0]), (results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1]) and torch.equal(results[0][2], results[1][2])
    assert float(results[0][0][-1]) < float(results[0][0][0])

    grads, seen = [], []
    for hooked in (False, True):
        m = build()
        if hooked:
            m.grad_stage_hook = lambda stage, flat: seen.append((stage, flat.numel(), flat.clone()))
        loss_of(m(A[:4], B[:4]), L[:4]).backward()
        grads.append(m._flat_grads.clone())
    assert [(s, n) for s, n, _ in seen] == [(0, grads[0].numel()), (1, 0)]
    assert torch.equal(seen[0][2], grads[1]) and torch.equal(grads[0], grads[1])
