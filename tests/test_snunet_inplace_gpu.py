"""SNUNet family, layer-local: every block, transposed conv and head of one training step checked IN PLACE.

One step of SNUNet_ECAM / Siam_NestedUNet_Conc (with and without deep supervision) runs on the HIP engine with debug bit 0 set;
then every stored tensor of the step (stcd_ws_tensor_*; tests/test_snunet_conc_cpu.py checks the table itself) is compared with a
float64 restatement of the ONE operation that produced it, applied on the CPU to the tensors that operation itself read -- so a
wrong term in one branch of configure_snunet / sn_block_forward / sn_block_backward cannot hide behind the rounding of the forty
layers around it.  The restatements are those of oracle/snunet_ref.py and tests/snunet_conc_spec.py (conv_block_nested, up,
ChannelAttention, the Conc head), written out per step; weights are rounded to bf16 where the engine packs them in bf16 (every
3x3 conv, transposed conv and conv_final; the ECAM MLPs and the Conc head read the fp32 parameters).

Bounds (relative l2 unless said otherwise; none is fitted to what the engine gives):
  * exact (torch.equal): whatever one kernel writes to several places or only moves -- every concat slice against its producer,
    the pooled map, conv4_0's input, the zeroed date-0 half of conv3_0.dP, the packed output gradient, conv1.bias.grad as a copy
    of bn2.bias.grad.
  * the bounds test_fcsiam_every_layer_in_place has for the same quantity: conv output (data gradients of a conv launch included:
    one conv, one rounding) 5e-6 fp32 / 3e-3 bf16; BatchNorm + ReLU (the residual form relu(bn2(Y2) + Y1) included: the same
    kernel, one more fp32 addition before the one rounding) 5e-6 / 4e-3; weight gradient from stored operands 5e-6; a bias in front
    of a training-mode BatchNorm (conv2.bias: mathematically zero) 1e-5 / 4e-3 of sum|dY|.
  * every other fp32 quantity: INPLACE_FP32 = 2e-4 (tests/test_bit_gpu.py).
  * every other bf16 quantity, the rule of test_token_path_in_place_bf16: the restatement is evaluated with bf16 rounding at the
    engine's storage points; the engine must stay within 1.5 x that emulation's own distance from the unrounded float64 value on
    these inputs, never above 2e-2; a quantity no rounding touches (emulation distance exactly 0) is held to 2e-4.
  * sums of nearly cancelling terms (BatchNorm's dgamma / dbeta, the four ECAM weight gradients) are measured against the sum of
    the absolute values of their terms instead of their own norm.

Measured on the MI355X: see the docstring of test_every_block_upconv_and_head_in_place.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import snunet_ref as S
from tests import snunet_conc_spec as spec
from tests.test_bit_gpu import INPLACE_FP32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILT = S.FILTERS
BLOCKS = [f"conv{l}_{j}" for l in range(5) for j in range(5 - l)]
CAP = 2e-2
# (fp32, bf16): tests/test_engine_gpu.py::test_fcsiam_every_layer_in_place
FIXED = {"conv": (5e-6, 3e-3), "bn+relu": (5e-6, 4e-3), "wgrad": (5e-6, 5e-6), "zero bias": (1e-5, 4e-3)}
CASES = [("ecam", "fp32", 2, 32, 64), ("ecam", "bf16", 3, 64, 64), ("conc", "bf16", 2, 64, 32), ("conc_ds", "fp32", 3, 32, 32)]


def _ident(x):
    return x


def _q(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _enc(name):
    """encoder level with both dates in one tensor (two BatchNorm groups)"""
    return name[6] == "0" and name[4] != "4"


# ---- the four expectations the description's perturbation runs replace, one at a time
def _block_out(z2, y1):
    """conv_block_nested: relu(bn2(conv2(.)) + identity), identity = conv1's raw output"""
    return torch.relu(z2 + y1)


def _dy1(bn1_back, dz2):
    """d(Y1) = bn1's backward + the gated gradient arriving through the identity branch"""
    return bn1_back + dz2


def _up_source(W, low, B):
    """what UpL_J reads: the lower block's output; below an encoder level the date-1 images alone (x{L}_0B)"""
    return W[low + ".Out"][B:] if _enc(low) else W[low + ".Out"]


def _gather_terms(W, name, B, head):
    """every contribution to d(Out) of block `name`, as full-size tensors: the base term (max-pool backward / the head's data
    gradient), each consumer's concat-gradient slice, and the data gradient of the transposed conv that up-samples Out"""
    lvl, j = int(name[4]), int(name[6])
    C = FILT[lvl]
    out = W[name + ".Out"]
    terms = []
    if name + ".P" in W:
        o = out.clone().requires_grad_(True)
        F.max_pool2d(o, 2).backward(W[name + ".dP"])
        terms.append(("max-pool", o.grad))
    if lvl == 0 and j >= 1:
        terms.append(("head", W[head + ".dIn"][:, 32 * (j - 1):32 * j]))
    for jc in range(max(j, 0) + 1, 5 - lvl):              # the consumers conv{lvl}_{jc}: cat(xL_0 A, xL_0 B, xL_1 .. xL_{jc-1}, up)
        d = W[f"conv{lvl}_{jc}.dIn"]
        if j == 0:
            terms.append((f"conv{lvl}_{jc}", torch.cat([d[:, :C], d[:, C:2 * C]]) if _enc(name) else None))
        else:
            terms.append((f"conv{lvl}_{jc}", d[:, (j + 1) * C:(j + 2) * C]))
    if lvl >= 1:
        u = W[f"Up{lvl}_{j}.dIn"]
        terms.append((f"Up{lvl}_{j}", torch.cat([torch.zeros_like(u), u]) if _enc(name) else u))
    assert all(t is not None and t.shape == out.shape for _, t in terms), name
    return terms


# ---- float64 BatchNorm (training mode), per date group
def _bn(y, groups):
    n = y.shape[0] // groups
    xh, inv = [], []
    for g in range(groups):
        v = y[g * n:(g + 1) * n]
        mu, var = v.mean(dim=(0, 2, 3), keepdim=True), v.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        inv.append(torch.rsqrt(var + 1e-5))
        xh.append((v - mu) * inv[-1])
    return torch.cat(xh), inv


def _bn_back(dz, xh, inv, gamma, groups):
    n = dz.shape[0] // groups
    out = []
    for g in range(groups):
        d, x = dz[g * n:(g + 1) * n], xh[g * n:(g + 1) * n]
        out.append(gamma.view(1, -1, 1, 1) * inv[g] * (d - d.mean(dim=(0, 2, 3), keepdim=True) - x * (d * x).mean(dim=(0, 2, 3), keepdim=True)))
    return torch.cat(out)


def _csum(x):
    return x.sum(dim=(0, 2, 3))


class _Checks:
    def __init__(self, bf, tag):
        self.bf, self.tag, self.rec, self.bad = bf, tag, [], []

    def _add(self, kind, name, r, emu, bound):
        self.rec.append((kind, name, r, emu, bound))
        if not r <= bound:
            self.bad.append((kind, name, f"{r:.3e}", f"emulation {emu:.3e}", f"bound {bound:.3e}"))

    def exact(self, kind, name, got, want):
        ok = got.shape == want.shape and torch.equal(got, want)
        self._add(kind + " (exact)", name, 0.0 if ok else float("inf"), 0.0, 0.0)

    def fixed(self, key, kind, name, got, want, scale=None):
        den = float(want.norm()) if scale is None else scale
        self._add(kind, name, float((got - want).norm()) / max(den, 1e-300), 0.0, FIXED[key][self.bf])

    def emul(self, kind, name, got, fn, scale=None):
        """fn(store) -> the restatement with `store` applied wherever the engine stores; `scale`: the sum of |terms| of a cancelling sum"""
        want = fn(_q if self.bf else _ident)
        den = max(float((want if scale is None else scale).norm()), 1e-300)
        r = float((got - want).norm()) / den
        emu = float((want - fn(_ident)).norm()) / den if self.bf else 0.0
        self._add(kind, name, r, emu, min(1.5 * emu, CAP) if emu > 0.0 else INPLACE_FP32)

    def worst(self):
        w = {}
        for kind, name, r, emu, bound in self.rec:
            if kind not in w or r / max(bound, 1e-300) >= w[kind][0] / max(w[kind][2], 1e-300):
                w[kind] = (r, emu, bound, name)
        return w


def _conv(x, w, b, dy):
    """3x3 conv in float64 -> (output, weight gradient, data gradient) for the output gradient dy"""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1)
    y.backward(dy)
    return y.detach(), w.grad, x.grad


def _engine_step(arch, dtype, B, H, W_):
    """One training step on the engine, debug bit 0 on -> everything the checks read, as float64 NCHW tensors on the CPU"""
    rng = np.random.default_rng(97 + B + H)
    x1 = torch.from_numpy(rng.standard_normal((B, 3, H, W_)).astype(np.float32))
    x2 = torch.from_numpy((x1.numpy() + 0.5 * rng.standard_normal((B, 3, H, W_))).astype(np.float32))
    tgt = torch.from_numpy((rng.random((B, H, W_)) < 0.25).astype(np.int64))
    with torch.random.fork_rng(devices=[]):      # the constructor's random initialisation (replaced below) leaves the global generator alone
        if arch == "ecam":
            from stcd_amd.modules import SNUNet_ECAM
            m, st = SNUNet_ECAM(3, 2, dtype=dtype), S.synth_state(3, 2, 23)
        else:
            from stcd_amd import Siam_NestedUNet_Conc
            m, st = Siam_NestedUNet_Conc(3, 2, dtype=dtype, deep_supervision=arch == "conc_ds"), spec.synth_state(3, 2, 23)
    m.load_state_dict(st)
    m._engine.set_debug(1)
    m.to(DEV).train()
    out = m(x1.to(DEV), x2.to(DEV))
    maps = list(out) if isinstance(out, (list, tuple)) else [out]
    for o in maps:
        o.retain_grad()
    (spec.ds_loss(maps, tgt.to(DEV)) if len(maps) == 5 else F.cross_entropy(maps[0], tgt.to(DEV))).backward()
    torch.cuda.synchronize()
    W = {k: v.permute(0, 3, 1, 2).double().cpu().contiguous() for k, v in m._engine.ws_tensors().items()}
    logits = [o.detach().double().cpu() for o in maps]
    glog = [o.grad.double().cpu() for o in maps]
    par = {n: p.detach().double().cpu() for n, p in m.named_parameters()}
    grad = {n: p.grad.double().cpu() for n, p in m.named_parameters()}
    return dict(W=W, par=par, grad=grad, logits=logits, glog=glog, x1=x1.double(), x2=x2.double())


def _run_case(arch, dtype, B, H, W_, step=_engine_step):
    """-> the _Checks of one training step of `arch` at B x H x W_"""
    bf = dtype == "bf16"
    store = _q if bf else _ident
    d = step(arch, dtype, B, H, W_)
    W, par, grad, logits, glog, x1, x2 = (d[k] for k in ("W", "par", "grad", "logits", "glog", "x1", "x2"))
    head = "ecam" if arch == "ecam" else "head"
    wq = (lambda w: w.to(torch.bfloat16).double()) if bf else _ident
    ck = _Checks(bf, f"{arch} {dtype} {B}x{H}x{W_}")

    # ------------------------------------------------------------------ concatenation: one kernel, the same bits everywhere
    x_in = W["conv0_0.in"]
    ck.exact("input", "conv0_0.in", x_in, torch.cat([torch.cat([store(x1), store(x2)]),
                                                      torch.zeros(2 * B, 5, H, W_, dtype=torch.float64)], 1))
    for lvl in range(1, 5):
        p = W[f"conv{lvl - 1}_0.P"]
        ck.exact("concat", f"conv{lvl}_0.in", W[f"conv{lvl}_0.in"], p[B:] if lvl == 4 else p)       # x4_0 exists for date B alone
    for lvl in range(4):
        C, e = FILT[lvl], W[f"conv{lvl}_0.Out"]
        for j in range(1, 5 - lvl):
            X = W[f"conv{lvl}_{j}.in"]
            assert X.shape[1] == (j + 1) * C + FILT[lvl + 1]
            ck.exact("concat", f"conv{lvl}_{j}.in[x{lvl}_0A]", X[:, :C], e[:B])
            ck.exact("concat", f"conv{lvl}_{j}.in[x{lvl}_0B]", X[:, C:2 * C], e[B:])
            for k in range(1, j):
                ck.exact("concat", f"conv{lvl}_{j}.in[x{lvl}_{k}]", X[:, (k + 1) * C:(k + 2) * C], W[f"conv{lvl}_{k}.Out"])
            ck.exact("concat", f"conv{lvl}_{j}.in[up]", X[:, (j + 1) * C:], W[f"Up{lvl + 1}_{j - 1}.Y"])
            ck.exact("concat", f"Up{lvl + 1}_{j - 1}.in", W[f"Up{lvl + 1}_{j - 1}.in"], _up_source(W, f"conv{lvl + 1}_{j - 1}", B))
    for j in range(1, 5):
        ck.exact("concat", f"{head}.in[x0_{j}]", W[head + ".in"][:, 32 * (j - 1):32 * j], W[f"conv0_{j}.Out"])
    ck.exact("gather", "conv3_0.dP[date A] == 0", W["conv3_0.dP"][:B], torch.zeros_like(W["conv3_0.dP"][:B]))

    # ------------------------------------------------------------------ the fifteen blocks
    for name in BLOCKS:
        groups = 2 if _enc(name) else 1
        cin = 3 if name == "conv0_0" else W[name + ".in"].shape[1]
        X, Y1, A1, Y2, Out = W[name + ".in"][:, :cin], W[name + ".Y1"], W[name + ".A1"], W[name + ".Y2"], W[name + ".Out"]
        dOut, dZ2, dY2, dY1 = W[name + ".dOut"], W[name + ".dZ2"], W[name + ".dY2"], W[name + ".dY1"]
        g1, b1, g2, b2 = (par[f"{name}.bn{k}.{w}"] for k in (1, 2) for w in ("weight", "bias"))
        # forward
        y1, dw1, din = _conv(X, wq(par[name + ".conv1.weight"]), par[name + ".conv1.bias"], dY1)
        ck.fixed("conv", "conv output", name + ".Y1", Y1, y1)
        xh1, inv1 = _bn(Y1, groups)
        ck.fixed("bn+relu", "bn+relu", name + ".A1", A1, torch.relu(xh1 * g1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1)))
        y2, dw2, t = _conv(A1, wq(par[name + ".conv2.weight"]), par[name + ".conv2.bias"], dY2)
        ck.fixed("conv", "conv output", name + ".Y2", Y2, y2)
        xh2, inv2 = _bn(Y2, groups)
        ck.fixed("bn+relu", "residual bn+relu", name + ".Out", Out, _block_out(xh2 * g2.view(1, -1, 1, 1) + b2.view(1, -1, 1, 1), Y1))
        if name + ".P" in W:
            ck.exact("max-pool", name + ".P", W[name + ".P"], F.max_pool2d(Out, 2))
        # gather: the sum of every contribution, rounded once
        terms = _gather_terms(W, name, B, head)
        ck.emul("gathered dOut", name + ".dOut", dOut, lambda s: s(sum(t_ for _, t_ in terms)))
        # backward
        ck.emul("dZ2", name + ".dZ2", dZ2, lambda s: dOut * (Out > 0))
        ck.emul("bn2 backward", name + ".dY2", dY2, lambda s: s(_bn_back(dZ2, xh2, inv2, g2, groups)))
        ck.emul("dgamma", name + ".bn2.weight.grad", grad[name + ".bn2.weight"], lambda s: _csum(dZ2 * xh2), _csum((dZ2 * xh2).abs()))
        ck.emul("dbeta", name + ".bn2.bias.grad", grad[name + ".bn2.bias"], lambda s: _csum(dZ2), _csum(dZ2.abs()))
        ck.exact("conv1 bias gradient", name + ".conv1.bias.grad", grad[name + ".conv1.bias"], grad[name + ".bn2.bias"])
        ck.emul("dbeta", name + ".conv1.bias.grad", grad[name + ".conv1.bias"], lambda s: _csum(dZ2), _csum(dZ2.abs()))
        ck.fixed("wgrad", "weight gradient", name + ".conv2.weight.grad", grad[name + ".conv2.weight"], dw2)
        gate = (A1 > 0).double()
        ck.emul("bn1 backward + identity", name + ".dY1", dY1, lambda s: s(_dy1(_bn_back(s(t) * gate, xh1, inv1, g1, groups), dZ2)))
        ck.emul("dgamma", name + ".bn1.weight.grad", grad[name + ".bn1.weight"], lambda s: _csum(s(t) * gate * xh1), _csum((t * gate * xh1).abs()))
        ck.emul("dbeta", name + ".bn1.bias.grad", grad[name + ".bn1.bias"], lambda s: _csum(s(t) * gate), _csum((t * gate).abs()))
        ck.fixed("wgrad", "weight gradient", name + ".conv1.weight.grad", grad[name + ".conv1.weight"], dw1)
        if name != "conv0_0":
            ck.fixed("conv", "data gradient", name + ".dIn", W[name + ".dIn"], din)
        else:
            assert name + ".dIn" not in W
        # a bias in front of a training-mode BatchNorm: zero by construction, both sides against sum|dY2|
        ck.fixed("zero bias", "conv2.bias.grad / sum|dY2|", name + ".conv2.bias.grad", grad[name + ".conv2.bias"].abs().max().view(1),
                 torch.zeros(1, dtype=torch.float64), scale=float(_csum(dY2.abs()).max()))

    # ------------------------------------------------------------------ the ten transposed convs
    for lvl in range(1, 5):
        for j in range(5 - lvl):
            u = f"Up{lvl}_{j}"
            x = _up_source(W, f"conv{lvl}_{j}", B).clone().requires_grad_(True)
            w = wq(par[u + ".up.weight"]).clone().requires_grad_(True)
            y = F.conv_transpose2d(x, w, par[u + ".up.bias"], stride=2)
            y.backward(W[u + ".dY"])
            ck.fixed("conv", "transposed conv output", u + ".Y", W[u + ".Y"], y.detach())
            ck.fixed("conv", "transposed conv data gradient", u + ".dIn", W[u + ".dIn"], x.grad)
            ck.fixed("wgrad", "weight gradient", u + ".up.weight.grad", grad[u + ".up.weight"], w.grad)
            ck.emul("transposed conv bias gradient", u + ".up.bias.grad", grad[u + ".up.bias"], lambda s: _csum(W[u + ".dY"]))

    # ------------------------------------------------------------------ the head
    E = W[head + ".in"]
    if arch == "ecam":
        _ecam_checks(ck, W, par, grad, logits[0], glog[0], wq, store)
    else:
        Er = E.clone().requires_grad_(True)
        hp = {k: par[k].clone().requires_grad_(True) for k in par if k.startswith(("final", "conv_final"))}
        outs = [F.conv2d(Er[:, 32 * i:32 * i + 32], hp[f"final{i + 1}.weight"], hp[f"final{i + 1}.bias"]) for i in range(4)]
        fused = F.conv2d(torch.cat(outs, 1), hp["conv_final.weight"], hp["conv_final.bias"])
        ours = outs + [fused] if len(logits) == 5 else [fused]
        torch.autograd.backward(ours, glog)
        for k, (a, b) in enumerate(zip(logits, ours)):
            ck.fixed("conv", "head output", f"map{k}", a, b.detach())
        ck.fixed("conv", "head data gradient", "head.dIn", W["head.dIn"], Er.grad)
        for k, v in hp.items():
            ck.emul("head parameter gradient", k + ".grad", grad[k], lambda s: v.grad)
    return ck


def _ecam_checks(ck, W, par, grad, logits, glog, wq, store):
    E, Z, dZ, G = W["ecam.in"], W["ecam.Y"], W["ecam.dY"], W["conv_final.dY"]
    N, C4, HW = E.shape[0], 128, E.shape[2] * E.shape[3]
    names = ("ca.fc1.weight", "ca.fc2.weight", "ca1.fc1.weight", "ca1.fc2.weight")

    def ecam(s):
        """ChannelAttention x 2 (oracle/snunet_ref.py) with the engine's stores: `intra` as a tensor of the activation dtype
        (straight-through), Z, and d(E) twice -- k_ecam_bwd1 stores ca * dZ, k_ecam_bwd2 adds the pooled paths to it and stores"""
        Er = E.clone().requires_grad_(True)
        w = {k: par[k].clone().requires_grad_(True) for k in names}
        intra = (Er[:, :32] + Er[:, 32:64]) + (Er[:, 64:96] + Er[:, 96:])
        intra = intra + (s(intra) - intra).detach()

        def att(x, w1, w2):      # ties of the maximum -> the lowest pixel index on both sides (torch.max over a flat map)
            avg, mx = x.mean(dim=(2, 3)), x.flatten(2).max(dim=2).values
            mlp = lambda v: torch.relu(v @ w1[:, :, 0, 0].t()) @ w2[:, :, 0, 0].t()
            return torch.sigmoid(mlp(avg) + mlp(mx))[:, :, None, None]
        ca1 = att(intra, w["ca1.fc1.weight"], w["ca1.fc2.weight"])
        ca = att(Er, w["ca.fc1.weight"], w["ca.fc2.weight"])
        z = ca * (E + ca1.repeat(1, 4, 1, 1))          # E detached here: the direct path is stored on its own, below
        z.backward(dZ)
        res = {k: w[k].grad for k in names}
        res["Z"] = s(z.detach())
        res["dE"] = s(s(ca.detach() * dZ) + Er.grad)
        res["ca"], res["ca1"] = ca.detach(), ca1.detach()
        return res
    cache = {}
    run = lambda s: cache.setdefault(s, ecam(s))
    ck.emul("ECAM output", "ecam.Y", Z, lambda s: run(s)["Z"])
    ck.emul("ECAM data gradient", "ecam.dIn", W["ecam.dIn"], lambda s: run(s)["dE"])
    # the sums of |terms| behind each weight gradient: |dZ (E + ca1)| and |dZ ca| per pixel, carried through the MLPs' backward
    r = run(_ident)
    ca, ca1 = r["ca"][:, :, 0, 0], r["ca1"][:, :, 0, 0]
    intra = (E[:, :32] + E[:, 32:64]) + (E[:, 64:96] + E[:, 96:])
    datt = {"ca": (dZ * (E + r["ca1"].repeat(1, 4, 1, 1))).abs().sum(dim=(2, 3)),
            "ca1": (dZ * r["ca"]).abs().sum(dim=(2, 3)).view(N, 4, 32).sum(1)}
    for key, x, a in (("ca", E, ca), ("ca1", intra, ca1)):
        w1, w2 = par[key + ".fc1.weight"][:, :, 0, 0], par[key + ".fc2.weight"][:, :, 0, 0]
        avg, mx = x.mean(dim=(2, 3)), x.flatten(2).max(dim=2).values
        h0, h1 = avg @ w1.t(), mx @ w1.t()
        dpre = datt[key] * a * (1 - a)
        s2 = torch.einsum("nc,nk->ck", dpre, torch.relu(h0) + torch.relu(h1))
        dh = [(h > 0).double() * (dpre @ w2.abs()) for h in (h0, h1)]
        s1 = torch.einsum("nk,nc->kc", dh[0], avg.abs()) + torch.einsum("nk,nc->kc", dh[1], mx.abs())
        ck.emul("ECAM weight gradient", key + ".fc1.weight.grad", grad[key + ".fc1.weight"][:, :, 0, 0], lambda s: run(s)[key + ".fc1.weight"][:, :, 0, 0], s1)
        ck.emul("ECAM weight gradient", key + ".fc2.weight.grad", grad[key + ".fc2.weight"][:, :, 0, 0], lambda s: run(s)[key + ".fc2.weight"][:, :, 0, 0], s2)
    # conv_final (1x1, 128 -> 2, bf16-packed filter) and the packed output gradient
    z = Z.clone().requires_grad_(True)
    w = wq(par["conv_final.weight"]).clone().requires_grad_(True)
    y = F.conv2d(z, w, par["conv_final.bias"])
    ck.fixed("conv", "head output", "logits", logits, y.detach())
    ck.exact("packed output gradient", "conv_final.dY", G, torch.cat([store(glog), torch.zeros(N, 6, *glog.shape[2:], dtype=torch.float64)], 1))
    y.backward(G[:, :2])
    ck.fixed("conv", "head data gradient", "ecam.dY", dZ, z.grad)
    ck.fixed("wgrad", "weight gradient", "conv_final.weight.grad", grad["conv_final.weight"], w.grad)
    ck.emul("conv_final bias gradient", "conv_final.bias.grad", grad["conv_final.bias"], lambda s: _csum(glog))     # summed from the fp32 values


@pytest.mark.parametrize("arch,dtype,B,H,W_", CASES, ids=[f"{a}-{d}-{b}x{h}x{w}" for a, d, b, h, w in CASES])
def test_every_block_upconv_and_head_in_place(arch, dtype, B, H, W_):
    """Odd and even B, non-square maps, 2 x 2 maps at level 4 (32-pixel sides), both heads, both dtypes.

    Measured on the MI355X, worst of each kind (engine vs restatement / the emulation's own distance from float64 / bound); every
    exact check held in every case:
      fp32 (SNUNet_ECAM 2 x 32 x 64; Conc with deep supervision 3 x 32 x 32 within 30 % of these): conv output 1.4e-6 / - / 5e-6;
        bn+relu 4.5e-7, residual bn+relu 6.2e-8 / - / 5e-6; data gradient 9.3e-7, transposed conv output 2.9e-7 and data gradient
        8.2e-7 / - / 5e-6; weight gradients 2.6e-8 / - / 5e-6; conv2.bias.grad 0 of sum|dY2|; against 2e-4: gathered dOut 4.9e-8,
        dZ2 0, bn2 backward 5.4e-7, bn1 backward + identity 4.9e-7, dgamma 4.8e-7 and dbeta 3.9e-7 (of the sums of |terms|),
        transposed conv bias gradient 2.8e-8; ECAM output 1.2e-7, data gradient 3.9e-7, weight gradients 5.9e-7, conv_final bias
        gradient 8.9e-9; Conc head parameter gradients 6.5e-8; head output 1.7e-7 and head data gradient 4.0e-8 / - / 5e-6.
      bf16 (SNUNet_ECAM 3 x 64 x 64 | Conc 2 x 64 x 32): the one-rounding kinds sit at the rounding itself -- conv output 1.67e-3 |
        1.69e-3 / - / 3e-3, bn+relu 1.68e-3 and residual bn+relu 1.69e-3 | 1.68e-3 / - / 4e-3, data gradients and transposed conv
        outputs 1.66e-3 .. 1.69e-3 / - / 3e-3, head data gradient 1.66e-3 | 1.64e-3 / - / 3e-3; weight gradients 2.1e-7 | 1.7e-7 / -
        / 5e-6; emulated kinds: gathered dOut 0 (bit-identical after the rounding) | 1.8e-5 / 1.69e-3 / 2.54e-3; bn2 backward
        4.1e-5 / 1.66e-3 / 2.48e-3 | 2.9e-5 / 1.65e-3 / 2.48e-3; bn1 backward + identity 4.1e-5 / 1.95e-3 / 2.93e-3 | 4.1e-5 / 1.90e-3 /
        2.85e-3; bn1's dgamma 3.0e-5 / 5.3e-4 / 7.9e-4 | 1.4e-5 / 4.6e-4 / 7.0e-4 and dbeta 2.9e-5 / 4.4e-4 / 6.7e-4 | 7.7e-6 / 3.8e-4 /
        5.7e-4; ECAM output 1.5e-5 / 1.54e-3 / 2.31e-3, data gradient 2.1e-6 / 8.3e-3 / 1.25e-2 (rounding `intra` makes ties that move
        an arg-max pixel: the largest emulation distance, under the 2e-2 cap), weight gradients 2.5e-7 / 1.0e-5 / 1.5e-5; untouched by
        rounding, against 2e-4: dZ2 0, bn2's dgamma / dbeta <= 3e-5 of the sums of |terms|, transposed conv bias gradient 3.8e-8,
        conv_final bias gradient 1.3e-8, Conc head parameter gradients 7.1e-8; head output 7.5e-8 | 1.0e-7 / - / 3e-3."""
    ck = _run_case(arch, dtype, B, H, W_)
    for kind, (r, emu, bound, name) in ck.worst().items():
        print(f"{ck.tag}: {kind}: worst {r:.2e} / emulation {emu:.2e} / bound {bound:.2e} ({name})")
    assert len(ck.rec) >= 350
    assert not ck.bad, ck.bad
