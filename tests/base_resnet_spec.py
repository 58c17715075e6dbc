"""CPU restatement of the BIT family's CNN baseline, ``ResNet`` (/root/reference/models/networks.py:223-304,
``define_G("base_resnet18")``), written from its description -- the yardstick of tests/test_base_resnet_*.py on shapes no fixture
holds.  Pinned to the reference's own class by the fixtures tests/golden/g24_base_resnet_*.npz (test_base_resnet_cpu.py).

    trunk (per date, shared weights, so every trunk BatchNorm is called twice per forward: date 1 then date 2):
        conv1 7x7 s2 p3 (no bias), bn1, ReLU, max-pool 3x3 s2 p1, layer1 (64), layer2 (128, stride 2), layer3 (256, stride 1),
        layer4 (512, stride 1; skipped when resnet_stages_num == 4) -- BasicBlocks; a 1x1 down-sample conv + BN on the identity
        branch where the stride or the width changes
    tail: per date nearest x2, conv_pred (3x3 p1, bias, -> 32); |x1 - x2|; bilinear x4 (align_corners=False); classifier =
        conv3x3 32 -> 32 (no bias), BatchNorm2d (ONE call per forward), ReLU, conv3x3 32 -> out_ch (bias)

All functions follow the dtype of the state they are given (float64 for reference values).
"""
import numpy as np
import torch
import torch.nn.functional as F

BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
PLANES = (64, 128, 256, 512)
STRIDES = (1, 2, 1, 1)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _bn_specs(name, c):
    return [(name + ".weight", (c,), "bn_w"), (name + ".bias", (c,), "bn_b"), (name + ".running_mean", (c,), "rm"),
            (name + ".running_var", (c,), "rv"), (name + ".num_batches_tracked", (), "nbt")]


def param_specs(backbone="resnet18", stages=5, out_ch=2):
    """[(name, shape, kind)] in the reference's ``state_dict`` order: resnet.* (all four layers and the unused fc, whatever
    ``stages`` is), classifier.{0,1,3}.*, conv_pred.*."""
    sp = [("resnet.conv1.weight", (64, 3, 7, 7), "conv")] + _bn_specs("resnet.bn1", 64)
    inpl = 64
    for li, (nb, pl, st) in enumerate(zip(BLOCKS[backbone], PLANES, STRIDES)):
        for b in range(nb):
            pre = f"resnet.layer{li + 1}.{b}"
            sp += [(pre + ".conv1.weight", (pl, inpl, 3, 3), "conv")] + _bn_specs(pre + ".bn1", pl)
            sp += [(pre + ".conv2.weight", (pl, pl, 3, 3), "conv")] + _bn_specs(pre + ".bn2", pl)
            if b == 0 and (st != 1 or inpl != pl):
                sp += [(pre + ".downsample.0.weight", (pl, inpl, 1, 1), "conv")] + _bn_specs(pre + ".downsample.1", pl)
            inpl = pl
    sp += [("resnet.fc.weight", (1000, 512), "fc"), ("resnet.fc.bias", (1000,), "bias")]
    sp += [("classifier.0.weight", (32, 32, 3, 3), "conv")] + _bn_specs("classifier.1", 32)
    sp += [("classifier.3.weight", (out_ch, 32, 3, 3), "conv"), ("classifier.3.bias", (out_ch,), "bias")]
    sp += [("conv_pred.weight", (32, 512 if stages == 5 else 256, 3, 3), "conv"), ("conv_pred.bias", (32,), "bias")]
    return sp


def synth_state(backbone="resnet18", stages=5, out_ch=2, seed=0, perturb_running=False):
    """Deterministic float32 state: the backbone's default init (kaiming normal, fan_out) for every conv, BatchNorm affine values
    perturbed around (1, 0) so that their gradients and the running-statistic updates are exercised, small biases."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, shape, kind in param_specs(backbone, stages, out_ch):
        if kind == "conv":
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
        elif kind == "fc":
            v = rng.standard_normal(shape) * 0.02
        elif kind in ("bias", "bn_b"):
            v = 0.1 * rng.standard_normal(shape)
        elif kind == "bn_w":
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif kind == "rm":
            v = 0.1 * rng.standard_normal(shape) if perturb_running else np.zeros(shape)
        elif kind == "rv":
            v = 1.0 + 0.2 * np.abs(rng.standard_normal(shape)) if perturb_running else np.ones(shape)
        else:
            st[name] = torch.zeros((), dtype=torch.int64)
            continue
        st[name] = torch.from_numpy(np.asarray(v, np.float32))
    return st


def _bn(x, st, name, training):
    g, b, rm, rv = st[name + ".weight"], st[name + ".bias"], st[name + ".running_mean"], st[name + ".running_var"]
    if training:
        n = x.numel() // x.shape[1]
        mean = x.mean(dim=(0, 2, 3))
        var = ((x - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
        with torch.no_grad():
            rm.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean.detach())
            rv.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * var.detach() * (n / max(n - 1, 1)))
            st[name + ".num_batches_tracked"] += 1
    else:
        mean, var = rm, rv
    return (x - mean[None, :, None, None]) * (torch.rsqrt(var + BN_EPS) * g)[None, :, None, None] + b[None, :, None, None]


def _single(st, x, training, nstage):
    x = F.conv2d(x, st["resnet.conv1.weight"], None, 2, 3)
    x = F.max_pool2d(torch.relu(_bn(x, st, "resnet.bn1", training)), 3, 2, 1)
    for li in range(nstage):
        b = 0
        while f"resnet.layer{li + 1}.{b}.conv1.weight" in st:
            pre = f"resnet.layer{li + 1}.{b}"
            stride = STRIDES[li] if b == 0 else 1
            y = torch.relu(_bn(F.conv2d(x, st[pre + ".conv1.weight"], None, stride, 1), st, pre + ".bn1", training))
            y = _bn(F.conv2d(y, st[pre + ".conv2.weight"], None, 1, 1), st, pre + ".bn2", training)
            if pre + ".downsample.0.weight" in st:
                x = _bn(F.conv2d(x, st[pre + ".downsample.0.weight"], None, stride, 0), st, pre + ".downsample.1", training)
            x = torch.relu(y + x)
            b += 1
    x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, st["conv_pred.weight"], st["conv_pred.bias"], 1, 1)


def forward(st, x1, x2, training):
    """logits [B, out_ch, H, W].  training: batch statistics, and ``st``'s running statistics / num_batches_tracked are updated in
    place in the reference's call order."""
    nstage = 4 if st["conv_pred.weight"].shape[1] == 512 else 3
    p1 = _single(st, x1, training, nstage)
    p2 = _single(st, x2, training, nstage)
    x = F.interpolate(torch.abs(p1 - p2), scale_factor=4, mode="bilinear", align_corners=False)
    x = torch.relu(_bn(F.conv2d(x, st["classifier.0.weight"], None, 1, 1), st, "classifier.1", training))
    return F.conv2d(x, st["classifier.3.weight"], st["classifier.3.bias"], 1, 1)
