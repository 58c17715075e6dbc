"""BIT (``BASE_Transformer``) on the HIP engine, through the nn.Module boundary -> C ABI: against the vectors captured from the
reference's own class (G25, tests/golden/make_bit_golden.py), against the CPU restatement (tests/bit_spec.py) on other shapes, the
token path (tokenizer, token encoder, decoder) in place, determinism, and the trainer / scene-inference tools."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from stcd_amd.bit import BASE_Transformer
from tests import bit_spec as S
from tests._util import rel_l2_cos, t
from tests.test_segcd_gpu import SEG_COS, SEG_REL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = [("g25_bit_s4.npz", 1, 64), ("g25_bit_s4_dd8.npz", 8, 64), ("g25_bit_s4_dd8_dedim8.npz", 8, 8)]
INPLACE_FP32 = 2e-4      # the project's fp32 in-place tolerance (test_base_resnet_gpu.test_new_steps_in_place)


def _unused(name):
    return name.startswith("resnet.fc.") or name.startswith("resnet.layer4.")


def _last_bias(dd):
    return f"transformer_decoder.layers.{dd - 1}.1.fn.fn.net.3.bias"


def _model(dd, dh, dtype, state, training, out_ch=2, **kw):
    m = BASE_Transformer(3, out_ch, "learned", resnet_stages_num=4, dec_depth=dd, decoder_dim_head=dh, dtype=dtype, **kw)
    m.load_state_dict(state)
    m.to(DEV).train(training)
    return m


def _nchw(x):
    return x.permute(0, 3, 1, 2).float().contiguous()


def _cancelling_bias_ok(m, dd, B):
    """The last decoder layer's net.3.bias is added to both dates and cancels in x1 - x2: the engine sums +g and -g, so its gradient
    is rounding noise -- at most the fp32 in-place tolerance relative to ONE date's sum."""
    dY = m._engine.ws_tensors()["bit.dec.dY"].float()
    per_date = dY[:B].sum(dim=(0, 1, 2))
    g = dict(m.named_parameters())[_last_bias(dd)].grad
    return float(g.norm() / per_date.norm().clamp_min(1e-30))


@pytest.mark.parametrize("fixture,dd,dh", FIXTURES)
def test_fp32_matches_reference_vectors(golden, fixture, dd, dh):
    """Bounds: logits rtol = atol = 1e-3 (the capture script keeps the reference's own float32-vs-float64 gap under a quarter (eval) /
    half (train) of it), loss within 1e-4, every gradient at SegCD's per-tensor bar (the reference's own gap stays under half of it),
    unused tensors exactly zero, BatchNorm statistics and call counts as in the ResNet test."""
    g = golden(fixture)
    seed = int(g["seed"])
    x1, x2 = t(g["x1"]).to(DEV), t(g["x2"]).to(DEV)
    B = x1.shape[0]
    m = _model(dd, dh, "fp32", S.synth_state(dd, dh, 2, seed, perturb_running=True), False)
    with torch.no_grad():
        ev = m(x1, x2)
    assert isinstance(ev, list) and len(ev) == 1
    print(f"{fixture}: eval max |dlogit| {float(np.abs(ev[0].cpu().numpy() - g['eval/logits']).max()):.2e}")
    np.testing.assert_allclose(ev[0].cpu().numpy(), g["eval/logits"], rtol=1e-3, atol=1e-3)

    m = _model(dd, dh, "fp32", S.synth_state(dd, dh, 2, seed), True)
    out = m(x1, x2)
    assert isinstance(out, list) and len(out) == 1
    out = out[0]
    print(f"{fixture}: train max |dlogit| {float(np.abs(out.detach().cpu().numpy() - g['train/logits']).max()):.2e}")
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["train/logits"], rtol=1e-3, atol=1e-3)
    loss = torch.nn.functional.cross_entropy(out, t(g["target"]).to(DEV))
    print(f"{fixture}: loss {loss.item():.7f} vs {float(g['loss']):.7f}")
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    worst = (0.0, 1.0, "")
    for name, p in m.named_parameters():
        if _unused(name):
            assert "gf/" + name not in g and p.grad is not None and float(p.grad.abs().max()) == 0.0, name
        elif name == _last_bias(dd):
            assert float(np.abs(g["gs/" + name]).max()) < 1e-12
            r = _cancelling_bias_ok(m, dd, B)
            print(f"{fixture}: cancelling {name}: {r:.1e} of one date's sum")
            assert r <= INPLACE_FP32
        else:
            got = p.grad.detach().cpu().numpy().ravel()[S.fixture_index(name, p.numel())]
            rel, cos = rel_l2_cos(got, g["gf/" + name])
            if rel > worst[0]:
                worst = (rel, min(worst[1], cos), name)
            assert rel <= SEG_REL and cos >= SEG_COS, (name, rel, cos)
            np.testing.assert_allclose(p.grad.double().norm().item(), g["gs/" + name][1], rtol=2 * SEG_REL, err_msg=name + " (l2 norm)")
    print(f"{fixture}: worst gradient rel-l2 {worst[0]:.2e} ({worst[2]}), cos {worst[1]:.6f}")
    sd = m.state_dict()
    for k in [k for k in g if k.startswith("rs/") and "num_batches" not in k]:
        np.testing.assert_allclose(sd[k[3:]].cpu().numpy(), g[k], rtol=1e-4, atol=5e-5, err_msg=k)
    for k in [k for k in sd if k.endswith(".num_batches_tracked")]:
        want = 0 if _unused(k) else (1 if k.startswith("classifier.") else 2)
        assert int(sd[k]) == want, k
    for k in [k for k in g if k.startswith("rs/") and "num_batches" in k]:
        assert int(sd[k[3:]]) == int(g[k]), k


@pytest.mark.parametrize("B,H,W,dd,dh", [(5, 32, 32, 1, 64), (2, 96, 64, 8, 64)])
def test_fp32_matches_the_spec_on_other_shapes(B, H, W, dd, dh):
    """Odd 2B / a non-power-of-two n = 384 rows per image (three 128-row tiles of the decoder's backward, two 256-row blocks of its
    forward) / non-square inputs against the CPU restatement in float64; the bounds of the fixture test."""
    seed = 190 + B
    rng = np.random.default_rng(seed)
    x1 = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    x2 = torch.from_numpy((2.0 * rng.standard_normal((B, 3, H, W))).astype(np.float32))
    tgt = torch.from_numpy((rng.random((B, H, W)) < 0.3).astype(np.int64))
    st = S.synth_state(dd, dh, 2, seed)
    m = _model(dd, dh, "fp32", st, True)
    out = m(x1.to(DEV), x2.to(DEV))[0]
    loss = torch.nn.functional.cross_entropy(out, tgt.to(DEV))
    loss.backward()
    st64 = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in st.items()}
    for k, v in st64.items():
        if v.dtype.is_floating_point and "running" not in k:
            v.requires_grad_(True)
    ro = S.forward(st64, x1.double(), x2.double(), training=True)
    rloss = torch.nn.functional.cross_entropy(ro, tgt)
    rloss.backward()
    print(f"bit fp32 vs float64 spec B={B} {H}x{W} dd{dd} dh{dh}: max |dlogit| {float((out.detach().cpu() - ro.detach().float()).abs().max()):.2e}, "
          f"loss {loss.item():.7f} vs {rloss.item():.7f}")
    np.testing.assert_allclose(out.detach().cpu().numpy(), ro.detach().float().numpy(), rtol=1e-3, atol=1e-3)
    assert abs(loss.item() - rloss.item()) < 1e-4
    worst = (0.0, 1.0, "")
    for name, p in m.named_parameters():
        ref = st64[name].grad
        if ref is None:
            assert _unused(name) and float(p.grad.abs().max()) == 0.0, name
            continue
        if name == _last_bias(dd):
            assert float(ref.abs().max()) < 1e-12 and _cancelling_bias_ok(m, dd, B) <= INPLACE_FP32
            continue
        r, c = rel_l2_cos(p.grad.cpu().double().numpy(), ref.numpy())
        if r > worst[0]:
            worst = (r, min(worst[1], c), name)
        assert r <= SEG_REL and c >= SEG_COS, (name, r, c)
    print(f"   worst gradient rel-l2 {worst[0]:.2e} ({worst[2]}), cos {worst[1]:.6f}")
    sd = m.state_dict()
    for k in ("resnet.bn1", "resnet.layer3.0.downsample.1", "classifier.1"):
        np.testing.assert_allclose(sd[k + ".running_mean"].cpu().numpy(), st64[k + ".running_mean"].float().numpy(), rtol=1e-4, atol=5e-5)
        np.testing.assert_allclose(sd[k + ".running_var"].cpu().numpy(), st64[k + ".running_var"].float().numpy(), rtol=1e-4, atol=5e-5)
        assert int(sd[k + ".num_batches_tracked"]) == int(st64[k + ".num_batches_tracked"]) == (1 if k == "classifier.1" else 2)


def _token_path_in_place(dtype, B, H, W, dd, dh):
    """Runs one training step with the debug tensors on and returns {step: rel-l2} of tokenizer, encoder and decoder, each against
    the spec (float64; ``store`` = bf16 rounding at the engine's storage points in bf16 mode) applied to the step's OWN stored input
    and output gradient, plus the same figures for the emulation itself against the plain float64 spec."""
    rng = np.random.default_rng(31 + B)
    x1 = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).to(DEV)
    x2 = torch.from_numpy((2.0 * rng.standard_normal((B, 3, H, W))).astype(np.float32)).to(DEV)
    tgt = torch.from_numpy((rng.random((B, H, W)) < 0.3).astype(np.int64)).to(DEV)
    st = S.synth_state(dd, dh, 2, 11)
    m = BASE_Transformer(3, 2, "learned", resnet_stages_num=4, dec_depth=dd, decoder_dim_head=dh, dtype=dtype)
    m.load_state_dict(st)
    m._engine.set_debug(1)
    m.to(DEV).train()
    torch.nn.functional.cross_entropy(m(x1, x2)[0], tgt).backward()
    torch.cuda.synchronize()
    ws = m._engine.ws_tensors()
    bf = dtype == "bf16"
    q = (lambda x: x.to(torch.bfloat16).to(x.dtype)) if bf else None
    f64 = lambda x: _nchw(x).double().cpu()
    P, Y, dY, dIn, cp_dY = (f64(ws[k]) for k in ("bit.dec.in", "bit.dec.Y", "bit.dec.dY", "bit.dec.dIn", "conv_pred.dY"))
    assert torch.equal(P, f64(ws["conv_pred.Y"])) and P.shape == (2 * B, 32, H // 4, W // 4)
    ti, to, dto, dti = (ws["bit.tokens." + k].double().cpu().reshape(2 * B, 4, 32) for k in ("in", "Y", "dY", "dIn"))
    assert ws["bit.tokens.in"].dtype == torch.float32
    sd = {k: v.double() for k, v in st.items() if v.dtype.is_floating_point}
    par = {n: p for n, p in m.named_parameters()}
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    got, emu = {}, {}

    def both(key, engine_value, fn):
        """fn(store) -> the spec's value; engine against fn(q), and (bf16) fn(q) against fn(None)"""
        want = fn(q)
        got[key] = rel(engine_value, want)
        if bf:
            emu[key] = rel(want, fn(None))

    # ---- tokenizer: tokens, and conv_pred.dY = decoder dIn + tokenizer data gradient (one rounding of the sum in bf16 mode)
    def tok(store, what):
        Pr = P.clone().requires_grad_(True)
        sw = {"conv_a.weight": sd["conv_a.weight"].clone().requires_grad_(True)}
        tk = S.tokenizer(sw, Pr)
        tk.backward(dti)
        total = dIn + Pr.grad
        return {"out": tk.detach(), "dx": store(total) if store else total, "dw": sw["conv_a.weight"].grad}[what]
    both("tokenizer tokens", ti, lambda s: tok(s, "out"))
    both("tokenizer data gradient", cp_dY, lambda s: tok(s, "dx"))
    both("tokenizer conv_a gradient", par["conv_a.weight"].grad.double().cpu(), lambda s: tok(s, "dw"))

    # ---- encoder (fp32 in both modes: nothing is rounded)
    def enc(what):
        tin = torch.cat([ti[:B], ti[B:]], dim=1).requires_grad_(True)
        sw = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("transformer.") or k == "pos_embedding"}
        en = S.encoder(sw, tin)
        en.backward(torch.cat([dto[:B], dto[B:]], dim=1))
        if what == "out":
            return torch.cat([en[:, :4], en[:, 4:]], dim=0).detach()
        if what == "din":
            return torch.cat([tin.grad[:, :4], tin.grad[:, 4:]], dim=0)
        return sw[what].grad
    both("encoder tokens", to, lambda s: enc("out"))
    both("encoder token gradient", dti, lambda s: enc("din"))
    for k in ("pos_embedding", "transformer.layers.0.0.fn.fn.to_qkv.weight", "transformer.layers.0.0.fn.fn.to_out.0.weight",
              "transformer.layers.0.0.fn.norm.weight", "transformer.layers.0.1.fn.fn.net.0.weight", "transformer.layers.0.1.fn.fn.net.3.bias"):
        both("encoder " + k, par[k].grad.double().cpu(), lambda s, k=k: enc(k))

    # ---- decoder
    dec_keys = [k for k in sd if k.startswith("transformer_decoder.")]

    def dec(store, what):
        Pr = P.clone().requires_grad_(True)
        mem = to.clone().requires_grad_(True)
        sw = {k: sd[k].clone().requires_grad_(True) for k in dec_keys}
        o = S.decoder(sw, Pr.flatten(2).transpose(1, 2), mem, store).transpose(1, 2).reshape(P.shape)
        o.backward(dY)
        if what == "out":
            return o.detach()
        if what == "din":
            return store(Pr.grad) if store else Pr.grad
        if what == "dmem":
            return mem.grad
        return sw[what].grad
    both("decoder output", Y, lambda s: dec(s, "out"))
    both("decoder data gradient", dIn, lambda s: dec(s, "din"))
    both("decoder memory gradient", dto, lambda s: dec(s, "dmem"))
    for l in sorted({0, dd - 1}):
        for sfx in ("0.fn.norm.weight", "0.fn.norm.bias", "0.fn.fn.to_q.weight", "0.fn.fn.to_k.weight", "0.fn.fn.to_v.weight",
                    "0.fn.fn.to_out.0.weight", "0.fn.fn.to_out.0.bias", "1.fn.norm.weight", "1.fn.fn.net.0.weight", "1.fn.fn.net.0.bias",
                    "1.fn.fn.net.3.weight") + (("1.fn.fn.net.3.bias",) if l < dd - 1 else ()):
            k = f"transformer_decoder.layers.{l}.{sfx}"
            both("decoder " + k[len("transformer_decoder."):], par[k].grad.double().cpu(), lambda s, k=k: dec(s, k))
    return got, emu


@pytest.mark.parametrize("B,H,W,dd,dh", [(2, 64, 64, 1, 64), (5, 32, 32, 8, 8)])
def test_token_path_in_place_fp32(B, H, W, dd, dh):
    """Tokenizer, encoder and decoder (outputs, data / memory gradients, parameter gradients of the first and last layer) against the
    float64 spec on the step's own stored tensors, at the project's fp32 in-place tolerance 2e-4 rel-l2."""
    got, _ = _token_path_in_place("fp32", B, H, W, dd, dh)
    print(f"fp32 B={B} {H}x{W} dd{dd} dh{dh}: " + ", ".join(f"{k} {v:.1e}" for k, v in got.items()))
    bad = {k: v for k, v in got.items() if not v <= INPLACE_FP32}
    assert not bad, bad


@pytest.mark.parametrize("B,H,W,dd,dh", [(3, 32, 64, 8, 64), (2, 64, 96, 1, 64)])
def test_token_path_in_place_bf16(B, H, W, dd, dh):
    """bf16 storage: the yardstick is the float64 spec with bf16 rounding emulated where the engine stores a pixel map inside the
    token path (every decoder layer's output, the decoder's data gradient, the summed conv_pred gradient); tokens, encoder and the
    folded matrices are fp32 in both modes.  Bound per quantity: 1.5 x the emulation's own distance from the plain float64 spec on
    these inputs (summation-order room, as the project's bf16 tests take over their emulation), never above 2e-2.  A quantity the
    rounding does not touch at all (emulation distance exactly 0: tokens, conv_a gradient, everything of the encoder, and with
    dec_depth 1 every decoder gradient but the data gradient -- the one rounded layer output has a straight-through gradient) is an
    fp32 quantity and is held to the fp32 in-place tolerance 2e-4; no rounded quantity falls under that floor (smallest emulation
    distance measured: 4.7e-4).

    Measured on the MI355X, engine vs emulation / emulation vs float64 / bound:
        3 x 32 x 64, dec_depth 8:  decoder output 9.4e-5 / 4.7e-3 / 7.1e-3; decoder data gradient 4.3e-5 / 1.7e-3 / 2.6e-3; decoder
            memory gradient 4.5e-5 / 2.8e-3 / 4.2e-3; summed conv_pred gradient 4.8e-9 / 1.6e-3 / 2.4e-3; decoder parameter gradients,
            layer 0: 6.9e-6 ... 6.2e-5 / 4.7e-4 ... 4.4e-3, layer 7: 4.7e-5 ... 1.1e-4 / 2.9e-3 ... 6.2e-3 (the largest emulation
            distance, layers.7.1.fn.norm.weight: bound 9.3e-3, under the 2e-2 cap); fp32 quantities <= 7.3e-7
        2 x 64 x 96, dec_depth 1:  decoder output 6.3e-5 / 1.7e-3 / 2.6e-3; decoder data gradient 0 / 1.7e-3 / 2.6e-3 and summed
            conv_pred gradient 0 / 1.4e-3 / 2.1e-3 (bit-identical after the rounding); fp32 quantities <= 5.5e-6"""
    got, emu = _token_path_in_place("bf16", B, H, W, dd, dh)
    print(f"bf16 B={B} {H}x{W} dd{dd} dh{dh}: " + ", ".join(f"{k} {got[k]:.1e} / {emu[k]:.1e}" for k in got))
    assert max(emu.values()) * 1.5 <= 2e-2, "the emulation itself is further than the cap allows: the storage points are wrong"
    bad = {k: (got[k], emu[k]) for k in got if not got[k] <= (1.5 * emu[k] if emu[k] > 0.0 else INPLACE_FP32)}
    assert not bad, bad


@pytest.mark.parametrize("fixture,dd,dh", FIXTURES)
def test_bf16_tracks_reference_vectors(golden, fixture, dd, dh):
    """bf16 storage end to end against the reference's vectors, with the assertions of test_base_resnet_gpu.test_bf16_tracks_
    reference_vectors: eval logits rel-l2 <= 4e-2, loss within 2e-2 relative, gradient-norm ratios median in [0.8, 1.25] / min >= 0.4
    / max <= 2.5, cosine >= 0.99 for the last conv.  The capture script measures bf16 storage on the reference itself (2.20e-2 /
    2.38e-2 / 1.62e-2 eval rel-l2 on the three fixtures) and refuses a fixture on which that alone uses more than 3/4 of these bounds.

    Achieved on the MI355X (eval rel-l2 / loss rel / ratio median [min, max] / last-conv cosine):
        bit_s4 (2 x 64 x 64)              2.08e-2 / 7.3e-4 / 0.997 [0.89, 1.08] / 0.99989
        bit_s4_dd8 (3 x 32 x 64)          2.38e-2 / 4.1e-4 / 0.992 [0.89, 1.11] / 0.99972
        bit_s4_dd8_dedim8 (1 x 32 x 32)   1.64e-2 / 6.5e-3 / 1.014 [0.89, 1.16] / 0.99971"""
    g = golden(fixture)
    seed = int(g["seed"])
    x1, x2 = t(g["x1"]).to(DEV), t(g["x2"]).to(DEV)
    m = _model(dd, dh, "bf16", S.synth_state(dd, dh, 2, seed, perturb_running=True), False)
    with torch.no_grad():
        ev = m(x1, x2)[0]
    r_eval, _ = rel_l2_cos(ev.cpu().numpy(), g["eval/logits"])
    m = _model(dd, dh, "bf16", S.synth_state(dd, dh, 2, seed), True)
    loss = torch.nn.functional.cross_entropy(m(x1, x2)[0], t(g["target"]).to(DEV))
    loss.backward()
    d_loss = abs(loss.item() - float(g["loss"])) / abs(float(g["loss"]))
    ratios, head = [], {}
    for name, p in m.named_parameters():
        if "gf/" + name not in g or name == _last_bias(dd):
            continue
        ref = g["gf/" + name]
        got = p.grad.detach().cpu().numpy().ravel()[S.fixture_index(name, p.numel())]
        nr = float(np.linalg.norm(ref))
        if nr < 1e-10:
            continue
        ratios.append(float(np.linalg.norm(got)) / nr)
        if name.startswith("classifier.3."):
            head[name] = rel_l2_cos(got, ref)[1]
    ratios = np.array(ratios)
    print(f"bit bf16 vs reference {fixture[4:-4]}: eval rel-l2 {r_eval:.2e}, loss rel {d_loss:.2e}, gradient norm ratios median "
          f"{np.median(ratios):.3f} range [{ratios.min():.2f}, {ratios.max():.2f}], last conv cosine {min(head.values()):.5f}")
    assert r_eval <= 4e-2
    assert d_loss < 2e-2
    assert 0.8 <= np.median(ratios) <= 1.25 and ratios.min() >= 0.4 and ratios.max() <= 2.5
    assert len(head) == 2 and min(head.values()) >= 0.99


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_identical_steps_are_bit_identical(dtype):
    """Every reduction of the token path goes through per-block partials summed in a fixed order: two identical training steps give
    bit-identical logits and gradients."""
    rng = np.random.default_rng(5)
    x1 = torch.from_numpy(rng.standard_normal((3, 3, 32, 64)).astype(np.float32)).to(DEV)
    x2 = torch.from_numpy(rng.standard_normal((3, 3, 32, 64)).astype(np.float32)).to(DEV)
    tgt = torch.from_numpy((rng.random((3, 32, 64)) < 0.3).astype(np.int64)).to(DEV)
    st = S.synth_state(8, 64, 2, 13)
    runs = []
    for _ in range(2):
        m = _model(8, 64, dtype, st, True)
        out = m(x1, x2)[0]
        torch.nn.functional.cross_entropy(out, tgt).backward()
        runs.append((out.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
        assert _unused(n) or float(runs[0][1][n].abs().max()) > 0.0, n


@pytest.mark.parametrize("name", ["bit_pos_s4", "bit_pos_s4_dd8_dedim8"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_thirty_trainer_steps_learn(name, dtype, tmp_path, monkeypatch):
    """Thirty FlatAdamW steps of CDTrainer (built by define_G, cross-entropy) on one fixed synthetic 8 x 64 x 64 batch: the loss stays
    finite and falls by more than 25 % (mean of the last five steps against the first step) -- ResNet's criterion."""
    from stcd_amd import synth
    from stcd_amd.optim import FlatAdamW
    from stcd_amd.trainer import CDTrainer

    monkeypatch.setenv("STCD_DTYPE", dtype)
    a, b, lab = synth.make_batch(8, 64, 64, seed=3)
    batch = {"A": torch.from_numpy(a), "B": torch.from_numpy(b), "L": torch.from_numpy(lab).unsqueeze(1)}
    tmp = str(tmp_path)
    args = NS(net_G=name, n_class=2, gpu_ids=[0], lr=1e-3, optimizer="adamw", lr_policy="linear", max_epochs=1, lr_decay_iters=1,
              batch_size=8, checkpoint_dir=os.path.join(tmp, "ckpt"), vis_dir=os.path.join(tmp, "vis"), weight_dir=os.path.join(tmp, "w"),
              loss="ce", multi_scale_train="False", multi_scale_infer="False", multi_pred_weights=[1.0], shuffle_AB=False, pretrain=None)
    torch.manual_seed(5)
    tr = CDTrainer(args, {"train": [batch], "val": [batch]})
    assert type(tr.net_G) is BASE_Transformer and tr.net_G._engine.dtype == dtype and isinstance(tr.optimizer_G, FlatAdamW)
    tr.net_G.train()
    losses = []
    for _ in range(30):
        tr._forward_pass(batch)
        tr.optimizer_G.zero_grad()
        tr._backward_G()
        tr.optimizer_G.step()
        losses.append(tr.G_loss.item())
    losses = np.array(losses)
    print(f"{name} {dtype}: 30 CDTrainer steps, loss {losses[0]:.4f} -> {losses[-5:].mean():.4f}")
    assert np.isfinite(losses).all()
    assert losses[-5:].mean() < 0.75 * losses[0], losses


def test_scene_inference_and_reliability_split():
    """One predict_scene call (96 x 96 scene, tile 64) and one select_reliable call: the eval path and the list return type fit the
    tools."""
    from stcd_amd.scene import predict_scene
    rng = np.random.default_rng(3)
    sa = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    sb = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    m = _model(8, 8, "bf16", S.synth_state(8, 8, 2, 7, perturb_running=True), True)
    res = predict_scene(m, sa, sb, tile=64, stride=32, batch=4)
    assert res.mask.shape == (96, 96) and m.training
    from stcd_amd.selftrain import select_reliable
    m2 = _model(8, 8, "bf16", S.synth_state(8, 8, 2, 8, perturb_running=True), True)
    xa = torch.from_numpy(rng.standard_normal((4, 3, 32, 32)).astype(np.float32)).to(DEV)
    xb = torch.from_numpy(rng.standard_normal((4, 3, 32, 32)).astype(np.float32)).to(DEV)
    names = [f"p{i}.png" for i in range(4)]
    sel = select_reliable([m, m2], [(xa, xb, None, names)])
    assert sorted(sel.reliable + sel.unreliable) == names and sel.agree.shape == (4, 1, 2, 2) and int(sel.agree.sum()) > 0
    assert m.training and m2.training


def test_sizes_and_sigmoid():
    m = _model(1, 64, "fp32", S.synth_state(1, 64, 1, 3, perturb_running=True), False, out_ch=1, output_sigmoid=True)
    x = torch.randn(1, 3, 32, 64, device=DEV)
    with torch.no_grad():
        p = m(x, x.flip(3))
    assert isinstance(p, list) and p[0].shape == (1, 1, 32, 64) and float(p[0].min()) >= 0.0 and float(p[0].max()) <= 1.0
    with pytest.raises(Exception, match="divisible by 32"):
        m(torch.zeros(1, 3, 40, 40, device=DEV), torch.zeros(1, 3, 40, 40, device=DEV))
