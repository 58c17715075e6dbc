"""The LDS-DMA tile kernel (k_conv_tile, stcd_op_conv impl 8): k_conv_res's 16 x 16 tile with the filter slice and the halo of all
input channels requested by `buffer_load ... lds` before the first MFMA (kernels_conv_tile.hip).

Per op against the plain-C oracle with the bound tests/test_ops_gpu.py applies to impl 1, and bit for bit against impl 1 (the
resident-filter kernel: same fragment image, same accumulation order per output element); a repeatability screen of the counted
vmcnt / barrier pipeline; and the plan switch inside SiamUnet_diff / SiamUnet_conc (STCD_NO_TILE_KERNEL=1 is the parent's plan)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fcsiam_ref as R
from oracle import ops_c as O
from stcd_amd import _lib
from stcd_amd.modules import SiamUnet_conc, SiamUnet_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAPS3 = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
FLIPPED = [(-dy, -dx) for dy, dx in TAPS3]      # the order a data gradient passes: tap t reads the mirrored neighbour


def geom(n, h, w, ci, co, ldo, taps):
    g = _lib.ConvGeom()
    g.n, g.hi, g.wi, g.ci, g.ldi = n, h, w, ci, ci
    g.hm, g.wm, g.in_stride = h, w, 1
    g.ho, g.wo, g.out_stride, g.oy0, g.ox0 = h, w, 1, 0, 0
    g.co, g.ldo, g.ntaps = co, ldo, len(taps)
    for i, (dy, dx) in enumerate(taps):
        g.dy[i], g.dx[i] = dy, dx
    return g


def run_conv(impl, g, x, w, bias, out):
    l = _lib.lib()
    nbytes = l.stcd_op_scratch_bytes(C.byref(g))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(l.stcd_op_conv(_lib.DTYPE_BF16, impl, C.byref(g), C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()),
                              C.c_void_p(bias.data_ptr()) if bias is not None else None, C.c_void_p(out.data_ptr()),
                              C.c_void_p(scratch.data_ptr()), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).bfloat16()


def operands(n, h, w, ci, co, seed):
    rng = np.random.default_rng(seed)
    x = rnd(rng, n, h, w, ci).to(DEV)
    wt = rnd(rng, 9, ci, co, scale=1.0 / np.sqrt(9 * ci)).float().to(DEV)
    bias = torch.from_numpy(rng.standard_normal(co).astype(np.float32)).to(DEV)
    return x, wt, bias


def oracle(x, wt, bias, taps):
    """NCHW oracle; tap t with offset (dy, dx) is filter position (ky, kx) = (dy + 1, dx + 1)"""
    ci, co = wt.shape[1], wt.shape[2]
    w_ref = np.zeros((co, ci, 3, 3), np.float32)
    for t, (dy, dx) in enumerate(taps):
        w_ref[:, :, dy + 1, dx + 1] = wt[t].cpu().numpy().T
    return O.conv2d_fwd(x.float().cpu().numpy().transpose(0, 3, 1, 2), w_ref, bias.cpu().numpy(), 1).transpose(0, 2, 3, 1)


CASES = [  # n, h, w, ci, co, ldo / co, taps
    (2, 16, 16, 64, 64, 1, TAPS3),        # one full tile per image, one part, two blocks per CU
    (2, 20, 12, 128, 128, 1, TAPS3),      # partial tiles on both axes, whole K = two parts
    (1, 8, 8, 128, 128, 1, TAPS3),        # maps smaller than a tile: the level-4 maps of the 64 x 64 ...
    (3, 3, 5, 128, 64, 1, TAPS3),         # ... and 48 x 80 network tests
    (2, 32, 32, 256, 128, 1, TAPS3),      # four parts through two buffers
    (1, 48, 16, 64, 32, 1, TAPS3),        # a narrow output slice (two n-tiles in all)
    (2, 20, 12, 128, 64, 2, TAPS3),       # ldo = 2 co: the other half of a concat-sized buffer must keep its poison
    (2, 20, 12, 64, 128, 1, FLIPPED),     # the tap order of a data gradient
    (40, 8, 8, 128, 256, 1, TAPS3),       # 40 tiles over the 32 blocks of each slice: eight blocks walk two tiles, the next tile's
    (40, 8, 8, 256, 128, 1, TAPS3),       # parts requested under this tile's MFMAs and stores (whole K / two of four parts in flight)
]


@pytest.mark.parametrize("n,h,w,ci,co,ldm,taps", CASES)
def test_tile_kernel_vs_oracle_and_resident_filter_kernel(n, h, w, ci, co, ldm, taps):
    x, wt, bias = operands(n, h, w, ci, co, ci * 1000 + co + h)
    ldo = co * ldm
    g = geom(n, h, w, ci, co, ldo, taps)
    outs = {}
    for impl in (1, 8):
        out = torch.full((n, h, w, ldo), 7.0, dtype=torch.bfloat16, device=DEV)
        run_conv(impl, g, x, wt, bias, out)
        outs[impl] = out
    ref = oracle(x, wt, bias, taps)
    np.testing.assert_allclose(outs[8][..., :co].float().cpu().numpy(), ref, rtol=2 ** -7, atol=2e-3, err_msg="tile kernel vs oracle")
    assert torch.equal(outs[8], outs[1]), float((outs[8].float() - outs[1].float()).abs().max())
    if ldm > 1:
        assert torch.equal(outs[8][..., co:], torch.full_like(outs[8][..., co:], 7.0))


def test_tile_kernel_is_repeatable():
    """Race screen of the pipeline (a counted vmcnt and a barrier decide what a fragment read sees; an early read passes whenever the
    DMA happens to land first): the kernel is deterministic, so twelve launches into fresh buffers -- four parts through two
    buffers, parts 2 and 3 requested under the MFMAs of parts 0 and 1 -- must reproduce the first bit for bit."""
    n, h, w, ci, co = 2, 32, 32, 256, 128
    x, wt, bias = operands(n, h, w, ci, co, 5)
    g = geom(n, h, w, ci, co, co, TAPS3)
    first = None
    junk = torch.empty(16 << 20, dtype=torch.uint8, device=DEV)
    for it in range(12):
        out = torch.empty(n, h, w, co, dtype=torch.bfloat16, device=DEV)
        run_conv(8, g, x, wt, bias, out)
        if it % 3 == 0:
            junk.fill_(it)                                 # shifts cache state and timing between launches
        if first is None:
            first = out.clone()
        else:
            assert torch.equal(out, first), f"run {it} differs"


# What two plans of the PARENT differ by on exactly these inputs (STCD_NO_RES_KERNEL=1 against its default: the same layers on
# another kernel, whose BatchNorm partial sums are split over other blocks), measured on MI355X with this file's seeds:
#   arch  B  H  W   logits max |d| / max |ref|   running statistics max |d|   gradients rel-l2
PARENT_PLAN_DIFF = {
    ("diff", 2, 64, 64): (1.088347e-02, 5.362034e-04, 7.961810e-02),
    ("conc", 3, 48, 80): (7.031165e-03, 3.231764e-04, 3.275584e-02),
}


@pytest.mark.parametrize("arch,B,H,W", sorted(PARENT_PLAN_DIFF))
def test_tile_plan_equals_the_resident_filter_plan_inside_the_network(monkeypatch, arch, B, H, W):
    """A training step (dropout 0) with the default plan -- the 64- to 256-channel layers of levels 3 and 4 on k_conv_tile -- against
    STCD_NO_TILE_KERNEL=1 (the parent's plan).  Every stored conv output is bit-equal wherever the layer's input is; logits,
    BatchNorm running statistics and gradients may differ only by what another split of the BatchNorm partial sums over blocks
    causes, bounded by what the parent's own two plans differ by on these inputs (PARENT_PLAN_DIFF).
    MEASURED (MI355X): this plan against STCD_NO_TILE_KERNEL=1 differs by 0 in all three figures at both sizes (every block of either
    kernel sums one tile here, and the int64 accumulators add the partial rows exactly); the parent's two plans by 1.1e-2 / 5.4e-4 /
    8.0e-2 (diff) and 7.0e-3 / 3.2e-4 / 3.3e-2 (conc)."""
    cls = {"diff": SiamUnet_diff, "conc": SiamUnet_conc}[arch]
    rng = np.random.default_rng(43)
    x1 = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).to(DEV)
    x2 = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).to(DEV)
    tgt = torch.from_numpy((rng.random((B, H, W)) < 0.2).astype(np.int64)).to(DEV)
    st = R.synth_state(arch, 3, 2, 23)
    res = []
    for off in ("0", "1"):
        monkeypatch.setenv("STCD_NO_TILE_KERNEL", off)
        m = cls(3, 2, dtype="bf16")
        m.load_state_dict(st)
        m.set_dropout_p(0.0)
        m.to(DEV).train()
        out = m(x1, x2)
        out = out[0] if isinstance(out, (list, tuple)) else out
        torch.nn.functional.cross_entropy(out, tgt).backward()
        torch.cuda.synchronize()
        ws = {k: v.clone() for k, v in m._engine.ws_tensors().items() if k.endswith(".Y") or k.endswith(".in")}
        res.append((out.detach().clone(), m._flat_bn.clone(), m._flat_grads.clone(), ws))
    a, b = res
    checked = 0
    for k in sorted(a[3]):
        if not k.endswith(".Y"):
            continue
        kin = k[:-2] + ".in"
        if kin in a[3] and torch.equal(a[3][kin], b[3][kin]):
            assert torch.equal(a[3][k], b[3][k]), (k, float((a[3][k].float() - b[3][k].float()).abs().max()))
            checked += 1
    assert checked >= 3, checked
    d_logit = float((a[0] - b[0]).abs().max() / b[0].abs().max())
    d_bn = float((a[1] - b[1]).abs().max())
    d_grad = float((a[2].double() - b[2].double()).norm() / b[2].double().norm())
    print(f"tile plan vs resident-filter plan {arch} {B}x{H}x{W}: logits {d_logit:.3e}  running statistics {d_bn:.3e}  gradients {d_grad:.3e}  "
          f"({checked} conv outputs bit-equal)")
    bound = PARENT_PLAN_DIFF[(arch, B, H, W)]
    assert d_logit <= bound[0] and d_bn <= bound[1] and d_grad <= bound[2], (d_logit, d_bn, d_grad, bound)
