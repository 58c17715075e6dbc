"""Rows and the fresh-engine yardstick of the engine lifecycle tests (test_lifecycle_cpu.py, test_lifecycle_gpu.py).

TEST INFRASTRUCTURE ONLY.  One table of (family, constructor, state builder, dtype, S1, S2, how dropout is pinned): S1 and S2
differ in batch AND map size, and are the smallest shapes at which the tile, tap-list, grouped weight-gradient and decoder
kernels of the family get another plan.  The yardstick of a reused engine is a module that never ran anything else: `snapshot`
before a call, `fresh_like` from that snapshot, `one_call` on both, `compare`.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn.functional as F

DEV = "cuda:0"
FP32_GRAD_REL_L2 = 2e-5      # the project's bound for two fp32 summation orders of one gradient (test_engine_gpu.py, side-stream test)
ODD = (3, 100, 100)          # tests/golden/g6_odd.npz was captured at 100 x 100: ReplicationPad2d on three of the four levels


@dataclass(frozen=True)
class Row:
    id: str
    make: Callable[[], torch.nn.Module]      # a new module on the CPU, as the family's own tests construct it
    state: Callable[[], dict]                # the state builder those tests use
    dtype: str
    s1: Tuple[int, int, int]
    s2: Tuple[int, int, int]
    pin: str                                 # "masks": set_dropout_masks(synth_masks), "seed": set_seed, "steps": equal _steps
    arch: str = ""                           # oracle.fcsiam_ref's name (pin == "masks")
    single: bool = False                     # forward(x) instead of forward(x1, x2)
    loss: str = "last"                       # cross-entropy on the last map, or "all": summed over every map the module returns
    exact_fp32_grads: bool = False           # the family's own tests assert fp32 bit identity (BIT)


def _fcsiam(arch, dtype, s1, s2, tag=""):
    from oracle import fcsiam_ref as R
    from stcd_amd import modules as M
    cls = {"diff": M.SiamUnet_diff, "conc": M.SiamUnet_conc, "fcef": M.Unet, "xconc": M.SiamUnet_cross_conc}[arch]
    return Row(f"{arch}-{dtype}{tag}", lambda: cls(3, 2, dtype=dtype), lambda: R.synth_state(arch, 3, 2, 5, perturb_running=True),
               dtype, s1, s2, "masks", arch=arch)


def _snunet(ds):
    if ds:
        from stcd_amd.modules import Siam_NestedUNet_Conc
        from tests import snunet_conc_spec as C
        return Row("snunet_conc_ds-bf16", lambda: Siam_NestedUNet_Conc(3, 2, dtype="bf16", deep_supervision=True),
                   lambda: C.synth_state(3, 2, 5, perturb_running=True), "bf16", (2, 32, 32), (3, 16, 48), "steps", loss="all")
    from oracle import snunet_ref as S
    from stcd_amd.modules import SNUNet_ECAM
    return Row("snunet_ecam-bf16", lambda: SNUNet_ECAM(3, 2, dtype="bf16"), lambda: S.synth_state(3, 2, 5, perturb_running=True),
               "bf16", (2, 32, 32), (3, 16, 48), "steps")


def _segcd(name):
    from oracle import segcd_ref as G
    from stcd_amd import segcd
    cls = getattr(segcd, name)
    return Row(f"{name.lower()}_r18-bf16", lambda: cls(encoder_name="resnet18", classes=2, dtype="bf16"),
               lambda: G.synth_state(3, 2, 5, perturb_running=True, encoder="resnet18"), "bf16", (2, 32, 32), (3, 32, 64), "steps",
               single=name == "UnetSeg", loss="last" if name == "UnetSeg" else "all")


def _resnet():
    from stcd_amd.bit import ResNet
    from tests import base_resnet_spec as B
    return Row("base_resnet18_s4-bf16", lambda: ResNet(3, 2, resnet_stages_num=4, backbone="resnet18", dtype="bf16"),
               lambda: B.synth_state("resnet18", 4, 2, 5, perturb_running=True), "bf16", (2, 32, 32), (3, 32, 64), "steps")


def _bit(dtype):
    from stcd_amd.bit import BASE_Transformer
    from tests import bit_spec as B
    return Row(f"bit_dd8_dh8-{dtype}", lambda: BASE_Transformer(3, 2, "learned", resnet_stages_num=4, dec_depth=8, decoder_dim_head=8, dtype=dtype),
               lambda: B.synth_state(8, 8, 2, 5, perturb_running=True), dtype, (2, 32, 32), (3, 32, 64), "steps", exact_fp32_grads=True)


CF_TINY = dict(embed_dims=(64, 64, 128, 128), depths=(2, 1, 1, 2), num_heads=(1, 2, 2, 4))      # TINY of test_changeformer_gpu.py


def _changeformer(aux):
    from oracle import changeformer_ref as R
    from stcd_amd.changeformer import ChangeFormerV6

    def make():
        m = ChangeFormerV6(3, 2, False, dtype="bf16", embed_dim=64, config=dict(CF_TINY))
        if aux:
            m.set_multi_scale_train(True)
        return m
    return Row("changeformer_tiny" + ("_multi_scale" if aux else "") + "-bf16", make,
               lambda: R.synth_state(R.CFConfig.tiny(2), 5, perturb_running=True), "bf16", (2, 32, 32), (1, 64, 64), "seed",
               loss="all" if aux else "last")


def rows() -> List[Row]:
    return [_fcsiam("diff", "bf16", (2, 32, 32), (3, 48, 80)), _fcsiam("diff", "fp32", (2, 32, 32), (3, 48, 80)),
            _fcsiam("diff", "bf16", (2, 32, 32), ODD, "-odd"), _fcsiam("conc", "bf16", (2, 32, 32), (3, 48, 80)),
            _fcsiam("fcef", "bf16", (2, 64, 64), (3, 32, 32)), _fcsiam("xconc", "bf16", (2, 64, 64), (3, 48, 80)),
            _snunet(False), _snunet(True), _segcd("SegCD"), _segcd("FFCTLCD"), _segcd("UnetSeg"), _resnet(), _bit("bf16"), _bit("fp32"),
            _changeformer(False), _changeformer(True)]


ROWS = rows()
BY_ID = {r.id: r for r in ROWS}


# ----------------------------------------------------------------------------------------------------------- one call
@dataclass
class Call:
    """One forward (+ backward when `tgt` is given) at one shape; `seed` pins the dropout of a training call."""
    x1: torch.Tensor
    x2: torch.Tensor
    tgt: Optional[torch.Tensor]
    seed: int = 0


def make_call(shape, seed, train) -> Call:
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x1, x2 = torch.randn(B, 3, H, W, generator=g), torch.randn(B, 3, H, W, generator=g)
    tgt = (torch.rand(B, H, W, generator=g) < 0.3).long()
    return Call(x1.to(DEV), x2.to(DEV), tgt.to(DEV) if train else None, seed)


def masks_of(row: Row, call: Call):
    from oracle import fcsiam_ref as R
    return R.synth_masks(row.arch, call.x1.shape[0], 1000 + call.seed)


def pin_dropout(row: Row, m, call: Call, steps: int):
    """What the suite already uses: explicit Dropout2d masks (FC-Siam: the mask table is part of the shape-bound plan, so NOT p = 0),
    ChangeFormer's set_seed, and everywhere the module's step counter (the hash seed of a forward without masks)."""
    m._steps = steps
    if call.tgt is None:
        return
    if row.pin == "masks":
        m.set_dropout_masks(masks_of(row, call))
    elif row.pin == "seed":
        m.set_seed(4242 + call.seed)


def loss_of(row: Row, out, tgt):
    maps = list(out) if isinstance(out, (list, tuple)) else [out]
    if row.loss == "last":
        maps = maps[-1:]
    total = 0.0
    for p in maps:
        t = tgt
        if p.shape[-2:] != tgt.shape[-2:]:      # ChangeFormer's auxiliary maps: nearest-resized ground truth (models/trainer.py:300-309)
            t = F.interpolate(tgt.float().unsqueeze(1), size=p.shape[-2:], mode="nearest").squeeze(1).long()
        total = total + F.cross_entropy(p, t)
    return total


@dataclass
class Result:
    outs: List[torch.Tensor]
    grads: Optional[torch.Tensor]
    bn: torch.Tensor
    nbt: torch.Tensor


def forward_of(row: Row, m, call: Call):
    return m(call.x1) if row.single else m(call.x1, call.x2)


def one_call(row: Row, m, call: Call) -> Result:
    """Eval forward under no_grad (no target) or one training step: forward, cross-entropy, backward.  -> every map of the output,
    the flat gradient buffer after the backward, the BatchNorm running buffers and num_batches_tracked afterwards."""
    if call.tgt is None:
        m.eval()
        with torch.no_grad():
            out = forward_of(row, m, call)
        grads = None
    else:
        m.train()
        out = forward_of(row, m, call)
        loss_of(row, out, call.tgt).backward()
        grads = m._flat_grads.clone()
    outs = [o.detach().clone() for o in (out if isinstance(out, (list, tuple)) else [out])]
    return Result(outs, grads, m._flat_bn.clone(), m._nbt.clone())


def snapshot(m) -> dict:
    """Parameters, BatchNorm running buffers and num_batches_tracked."""
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def fresh_like(row: Row, snap: dict, training: bool):
    m = row.make()
    m.load_state_dict(snap)
    return m.to(DEV).train(training)


def new_module(row: Row):
    m = row.make()
    m.load_state_dict(row.state())
    return m.to(DEV)


def share_one_workspace(row: Row, m):
    """Every configuration of `m` gets its workspace at ONE address.  The workspace is the caller's (include/stcd_hip.h), and
    torch's caching allocator hands a freed block back whenever it fits -- by luck of the sizes.  The engine's pointer-keyed caches
    (uploaded job tables, packed filter images) must not mistake the new configuration's workspace for the old one, so the reused
    module of the lifecycle tests always meets that case: Engine.configure's own allocation is replaced by a slice of one arena
    sized for the larger of the row's two shapes."""
    from stcd_amd import _lib
    eng, l = m._engine, _lib.lib()
    probe = row.make()._engine                   # sized on a second engine: stcd_configure touches no device
    need = 0
    for shape in (row.s1, row.s2):
        _lib.check(l.stcd_configure(probe._h, *shape))
        need = max(need, int(l.stcd_workspace_bytes(probe._h)))
    arena = torch.empty(need, dtype=torch.uint8, device=DEV)
    plain = eng.configure

    def configure(batch, height, width, device):
        if eng.shape == (batch, height, width) and eng.workspace is not None and eng.workspace.device == device:
            return
        plain(batch, height, width, device)
        n = eng.workspace.numel()
        assert n <= arena.numel() and arena.device == eng.workspace.device
        eng.workspace = arena[:n]
    eng.configure = configure
    return arena


def rewrite_parameters(m):
    """In place under no_grad, the way an optimizer does: a stale filter image then shows as a difference."""
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01 * p)


# ----------------------------------------------------------------------------------------------------------- comparison
def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def compare(row: Row, step: str, used: Result, fresh: Result, engine, fp32_worst: Optional[dict] = None):
    """bf16: bit identity of outputs, of every parameter's gradient slice and of the BatchNorm buffers.  fp32: the same, except
    that gradients of the families without an fp32 bit-identity claim may differ by FP32_GRAD_REL_L2 per tensor; what needed the
    bound is collected in `fp32_worst` (name -> rel-l2)."""
    assert len(used.outs) == len(fresh.outs), f"{row.id} {step}: {len(used.outs)} maps against {len(fresh.outs)}"
    for i, (a, b) in enumerate(zip(used.outs, fresh.outs)):
        assert a.shape == b.shape and torch.equal(a, b), f"{row.id} {step}: output map {i} of the reused engine differs from a fresh engine's, rel-l2 {_rel(a, b) if a.shape == b.shape else 'shape'}"
    for info in engine.bns:
        sl = slice(info.offset, info.offset + 2 * info.channels)
        assert torch.equal(used.bn[sl], fresh.bn[sl]), f"{row.id} {step}: running statistics of {info.name} differ, rel-l2 {_rel(used.bn[sl], fresh.bn[sl]):.3e}"
    assert torch.equal(used.nbt, fresh.nbt), f"{row.id} {step}: num_batches_tracked differs"
    assert (used.grads is None) == (fresh.grads is None)
    if used.grads is None:
        return
    loose = row.dtype == "fp32" and not row.exact_fp32_grads
    for info in engine.params:
        sl = slice(info.offset, info.offset + info.numel)
        a, b = used.grads[sl], fresh.grads[sl]
        if torch.equal(a, b):
            continue
        rel = _rel(a, b)
        if loose and fp32_worst is not None:
            fp32_worst[info.name] = max(fp32_worst.get(info.name, 0.0), rel)
        assert loose and rel <= FP32_GRAD_REL_L2, f"{row.id} {step}: gradient of {info.name} differs from a fresh engine's, rel-l2 {rel:.3e}"


def grads_are_views(m) -> bool:
    """p.grad is the view of _flat_grads the fused optimizers read in place (FlatAdam / FlatAdamW copy anything else first)."""
    base = m._flat_grads.data_ptr()
    return all(p.grad is not None and p.grad.data_ptr() == base + 4 * info.offset for p, info in zip(m.parameters(), m._engine.params))
