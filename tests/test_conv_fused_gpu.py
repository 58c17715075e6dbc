"""What the engine fuses into its bf16 conv kernels, per kernel, against the plain fp64 reference of tests/conv_fused_spec.py:
the per-(group, channel) sums in int64 fixed point (k_conv_small / _res / _tile / _gemm), the ConvEpi epilogue (k_conv_gemm /
_halo / _dma) and the BatchNorm-backward sums of a data gradient (k_conv_small / _res), through stcd_op_conv_fused, which
launches the NAMED kernel with the engine's own plan for the requested groups.

The exact cases use operands for which every summation order gives the same bits (see the spec): they assert EQUALITY.  The only
tolerances in this file are the two derived ones -- `S.sum_bound` for sums of real-valued outputs, and one bf16 ulp of the largest
expected value for the real-valued epilogue."""
import ctypes as C

import pytest
import torch

from stcd_amd import _lib
from tests import conv_fused_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KID = {S.SMALL: _lib.CONV_SMALL, S.RES: _lib.CONV_RES, S.TILE: _lib.CONV_TILE, S.GEMM: _lib.CONV_GEMM, S.HALO: _lib.CONV_HALO,
       S.DMA: _lib.CONV_DMA}
PREFILL = 7.0                       # output buffers start as 7.0: pad channels and positions a scatter skips must keep it
GUARD, GUARD_WORD = 256, 0x5A5A5A5A5A5A5A5A       # guard words on either side of an accumulator: more than any slice offset here, so
                                                   # an add whose channel index is off by a slice lands in them (and is seen), not outside
_SHARED = {}


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def shared(c, real=False):
    """device operands and the fp64 reference of a shape: computed once, shared by every test of that shape, never written"""
    key = (c.shape_key, real)
    if key not in _SHARED:
        x, w, b = (t.to(DEV) for t in (S.real_operands(c) if real else S.exact_operands(c)))
        _SHARED[key] = (x, w, b, None if real else S.conv_ref(c, x, w, b))
    return _SHARED[key]


def geom_of(c, ldo):
    g = _lib.ConvGeom()
    g.n, g.hi, g.wi, g.ci, g.ldi = c.n, c.h, c.w, c.ci, c.ci
    g.hm, g.wm, g.in_stride = c.hm, c.wm, c.in_stride
    g.ho, g.wo, g.out_stride, g.oy0, g.ox0 = c.ho, c.wo, c.out_stride, c.o0[0], c.o0[1]
    g.co, g.ldo, g.ntaps = c.co, ldo, len(c.taps)
    for i, (dy, dx) in enumerate(c.taps):
        g.dy[i], g.dx[i] = dy, dx
    return g


class Acc:
    """an accumulator [bn_rep][groups][2][C] between guard words, prefilled with non-zero values (the kernels add)"""

    def __init__(self, rep, groups, Cn):
        self.shape = (rep, groups, 2, Cn)
        nbody = rep * groups * 2 * Cn
        self.buf = torch.full((GUARD + nbody + GUARD,), GUARD_WORD, dtype=torch.int64, device=DEV)
        self.pre = (torch.arange(nbody, dtype=torch.int64, device=DEV) * 2654435761 % 1000003 - 500000).view(self.shape)
        self.body.copy_(self.pre)

    @property
    def body(self):
        return self.buf[GUARD:-GUARD].view(self.shape)

    def total(self):
        """what was added, summed over the replicas: [groups][2][C]; the guards must be untouched"""
        assert bool((self.buf[:GUARD] == GUARD_WORD).all()) and bool((self.buf[-GUARD:] == GUARD_WORD).all()), "guard words overwritten"
        return (self.body - self.pre).sum(0)

    def untouched(self):
        return bool((self.buf[:GUARD] == GUARD_WORD).all()) and bool((self.buf[-GUARD:] == GUARD_WORD).all()) and torch.equal(self.body, self.pre)


def launch(c, x, w, b, groups=None, acc=None, c0=0, scales=(S.FS1, S.FS2), epi=None, bwd=None, relu=0, expect_fail=False, out=None):
    """one stcd_op_conv_fused call -> (out [n][ho][wo][co + 8], the request with its out-values)"""
    l = _lib.lib()
    ldo = c.co + 8
    g = geom_of(c, ldo)
    if out is None:
        out = torch.full((c.n, c.ho, c.wo, ldo), PREFILL, dtype=torch.bfloat16, device=DEV)
    f = _lib.ConvFused()
    f.kernel, f.groups = KID[c.kernel], c.groups if groups is None else groups
    f.alpha = f.beta = 1.0
    keep = [out]
    if acc is not None:
        f.sum_acc, f.sum_c0, f.sum_c, f.sum_scale1, f.sum_scale2 = acc.body.data_ptr(), c0, acc.shape[3], scales[0], scales[1]
    if epi is not None or relu:
        epi = epi or {}
        f.use_epi, f.relu = 1, relu
        gate, res = epi.get("gate"), epi.get("res")
        if gate is not None:
            f.gate, f.ldg = gate.data_ptr(), gate.shape[-1]
        if res is not None:
            f.res, f.ldr = res.data_ptr(), res.shape[-1]
            f.alpha, f.beta = epi["alpha"], epi["beta"]
    if bwd is not None:
        f.bw_y, f.bw_ldy, f.bw_stat, f.bw_acc = bwd["Y"].data_ptr(), bwd["Y"].shape[-1], bwd["stat"].data_ptr(), bwd["acc"].body.data_ptr()
        f.bw_mask = bwd["mask"].data_ptr() if bwd["mask"] is not None else None
    nbytes = l.stcd_op_scratch_bytes(C.byref(g))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = l.stcd_op_conv_fused(C.byref(g), C.byref(f), ptr(x), ptr(w), ptr(b), ptr(out), ptr(scratch), nbytes,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if expect_fail:
        return out, f, rc, l.stcd_last_error().decode("utf-8", "replace")
    _lib.check(rc)
    assert f.blocks >= 1 and f.tiles_per_group >= 1 and 1 <= f.blocks_per_group <= f.blocks and f.bn_rep >= 1
    assert bool((out[..., c.co:] == PREFILL).all()), "the pad channels of the output were written"
    return out, f


def stored(out, c):
    """the values at the positions and channels the launch owns, as fp64"""
    return out[:, c.o0[0]::c.out_stride, c.o0[1]::c.out_stride, :c.co].double()


def expect_acc(v, c, groups, scales):
    s1, s2 = S.group_sums(v, groups, c.c0, c.nsum)
    return torch.stack((S.fixed(s1, scales[0]), S.fixed(s2, scales[1])), 1)      # [groups][2][C]


# ------------------------------------------------------------------ fused sums
@pytest.mark.parametrize("c", S.SUM_CASES, ids=lambda c: c.id)
def test_fused_sums_exact(c):
    x, w, b, yref = shared(c)
    want = S.rne_bf16(yref.clamp_min(0.0) if c.relu else yref)          # (integers <= 256: the rounding changes nothing)
    out0, f0 = launch(c, x, w, b, relu=c.relu)
    assert torch.equal(stored(out0, c), want), "stored output differs from the fp64 reference"
    acc = Acc(f0.bn_rep, c.groups, c.nsum)
    out1, f = launch(c, x, w, b, acc=acc, c0=c.c0, scales=c.scales, relu=c.relu)
    assert torch.equal(out1, out0), "the sums request changed the output"
    assert (f.blocks, f.tiles_per_group, f.blocks_per_group) == (f0.blocks, f0.tiles_per_group, f0.blocks_per_group)
    got = acc.total()
    assert torch.equal(got, expect_acc(want, c, c.groups, c.scales)), "accumulators differ from the exact fixed-point sums"
    # what the case is in the table for
    if c.tag == "walk":
        assert f.tiles_per_group > f.blocks_per_group and f.tiles_per_group % f.blocks_per_group != 0, (f.tiles_per_group, f.blocks_per_group)
    if c.tag == "t128":
        assert f.tile_m == 128 and f.tiles_per_group == (c.n // c.groups) * c.hm * c.wm // 128
    if c.kernel == S.GEMM:
        mg = (c.n // c.groups) * c.hm * c.wm
        assert f.tiles_per_group == -(-mg // f.tile_m)
        if (c.h, c.w) == (5, 7):
            assert mg == 105 and mg % f.tile_m != 0
    if c.kernel in S.GROUP1_KERNELS and c.groups > 1:
        # one group on the same operands: bit-equal output, and the two group accumulators sum to the single-group one
        acc1 = Acc(f0.bn_rep, 1, c.nsum)
        out2, _ = launch(c, x, w, b, groups=1, acc=acc1, c0=c.c0, scales=c.scales)
        assert torch.equal(out2, out0)
        assert torch.equal(acc1.total(), got.sum(0, keepdim=True))
        assert torch.equal(acc1.total(), expect_acc(want, c, 1, c.scales))


@pytest.mark.parametrize("c", S.ROUNDED_CASES, ids=lambda c: c.id)
def test_fused_sums_are_of_the_rounded_values(c):
    """y in 257 ... 511: the stored output is RNE-bf16(y) (even integers), and the sums are of the STORED values"""
    x, w, b, yref = shared(c)
    want = S.rne_bf16(yref)
    out0, f0 = launch(c, x, w, b)
    assert torch.equal(stored(out0, c), want)
    acc = Acc(f0.bn_rep, c.groups, c.co)
    out1, _ = launch(c, x, w, b, acc=acc)
    assert torch.equal(out1, out0)
    got = acc.total()
    assert torch.equal(got, expect_acc(want, c, c.groups, c.scales)), "the sums are not those of the rounded, stored values"
    assert not torch.equal(got, expect_acc(yref, c, c.groups, c.scales))


@pytest.mark.parametrize("c", S.REAL_SUM_CASES, ids=lambda c: c.id)
def test_fused_sums_real_valued(c):
    """standard-normal operands: the fused sums against the fp64 sums of the kernel's own stored output, within
    (n + 1) * 2^-24 * sum|x| + B / (2 * scale)   (S.sum_bound: any fp32 summation order + one llrint per atomic add)"""
    x, w, b, _ = shared(c, real=True)
    out0, f0 = launch(c, x, w, b)
    acc = Acc(f0.bn_rep, c.groups, c.co)
    out1, f = launch(c, x, w, b, acc=acc)
    assert torch.equal(out1, out0)
    v = stored(out1, c).reshape(c.groups, -1, c.co)
    nvals = v.shape[1]
    assert nvals <= 512
    got = acc.total().double()
    worst = []
    for which, (scale, vals) in enumerate(((S.FS1, v), (S.FS2, v * v))):
        err = (got[:, which] / scale - vals.sum(1)).abs()
        bound = S.sum_bound(nvals, vals.abs().sum(1), f.blocks, scale)
        worst.append(float((err / bound).max()))
        assert bool((err <= bound).all()), (which, float((err / bound).max()))
    print(f"\n{c.id}: fused-sum error / bound: sum(y) {worst[0]:.3e}, sum(y^2) {worst[1]:.3e}  (n = {nvals}, B = {f.blocks})")


# ------------------------------------------------------------------ ConvEpi
def epi_args(c, gate, res):
    e = {}
    if c.mode in ("gate", "all"):
        e["gate"] = gate
    if c.mode in ("res", "all"):
        e.update(res=res, alpha=c.alpha, beta=c.beta)
    return e


@pytest.mark.parametrize("c", S.EPI_CASES, ids=lambda c: c.id)
def test_conv_epi_exact(c):
    x, w, b, yref = shared(c)
    gate, res = (t.to(DEV) for t in S.epi_operands(c))
    sub = lambda t: t[:, c.o0[0]::c.out_stride, c.o0[1]::c.out_stride, :c.co]
    want, summed = S.epi_ref(yref, c.relu, sub(gate) if c.mode in ("gate", "all") else None, sub(res) if c.mode in ("res", "all") else None,
                             c.alpha, c.beta)
    want_sums = c.kernel == S.GEMM and c.mode == "all"
    acc = Acc(8, 1, c.co) if want_sums else None
    out, f = launch(c, x, w, b, acc=acc, epi=epi_args(c, gate, res), relu=c.relu)
    assert torch.equal(stored(out, c), want), "stored output differs from the reference epilogue"
    if c.out_stride > 1:                                        # positions the scatter skips keep the prefill
        rest = out.clone()
        rest[:, c.o0[0]::c.out_stride, c.o0[1]::c.out_stride] = PREFILL
        assert bool((rest == PREFILL).all())
    if want_sums:       # of the relu'd, rounded value BEFORE gate and residual, as the kernel documents
        assert f.bn_rep == 8
        assert torch.equal(acc.total(), expect_acc(summed, c, 1, c.scales))
        assert not torch.equal(acc.total(), expect_acc(want, c, 1, c.scales))


@pytest.mark.parametrize("c", S.EPI_REAL_CASES, ids=lambda c: c.id)
def test_conv_epi_real_valued(c):
    """expected = bf16(alpha * gate(relu(y0)) + beta * res) formed in fp32 from the SAME kernel's plain output y0; within one bf16
    ulp of the largest expected value (2^-7 * max|expected|: the project's output bound)"""
    x, w, b, _ = shared(c, real=True)
    gate, res = (t.to(DEV) for t in S.epi_operands(c, real=True))
    y0, _ = launch(c, x, w, b)
    out, _ = launch(c, x, w, b, epi=epi_args(c, gate, res), relu=c.relu)
    v = y0[..., :c.co].float().clamp_min(0.0)
    v = torch.where(gate[..., :c.co].float() > 0, v, torch.zeros_like(v))
    want = (c.alpha * v + c.beta * res[..., :c.co].float()).bfloat16().float()
    err = (out[..., :c.co].float() - want).abs().max().item()
    tol = 2.0 ** -7 * want.abs().max().item()
    print(f"\n{c.id}: epilogue error / bound {err / tol:.3e}")
    assert err <= tol


# ------------------------------------------------------------------ BatchNorm-backward sums of a data gradient
@pytest.mark.parametrize("c", S.BWD_CASES, ids=lambda c: c.id)
def test_bwdsum_exact(c):
    x, w, b, yref = shared(c)
    Y, stat, mask = (t.to(DEV) if t is not None else None for t in S.bwd_operands(c))
    dA0, f0 = launch(c, x, w, b)
    assert torch.equal(stored(dA0, c), yref)
    acc = Acc(f0.bn_rep, c.groups, c.co)
    dA1, f = launch(c, x, w, b, bwd=dict(Y=Y, stat=stat, mask=mask, acc=acc))
    assert torch.equal(dA1, dA0), "the sums request changed the stored data gradient"
    s1, s2 = S.bwd_sums(stored(dA0, c), Y, stat, mask, c.groups)
    want = torch.stack((S.fixed(s1, S.BS), S.fixed(s2, S.BS)), 1)
    assert torch.equal(acc.total(), want), "accumulators differ from the exact sum(dz), sum(dz * xhat) at 2^36"


# ------------------------------------------------------------------ refused combinations: an error with a message, nothing launched
def _reject_cases():
    small, res, tile = S.Case(S.SMALL, 2, 16, 16, 16, 16, 2), S.Case(S.RES, 2, 16, 16, 32, 32, 2), S.Case(S.TILE, 2, 16, 16, 64, 64, 2)
    halo, dma = S.Case(S.HALO, 1, 16, 16, 128, 128), S.Case(S.DMA, 1, 16, 16, 128, 256)
    gemm = S.Case(S.GEMM, 2, 16, 16, 64, 64, 2, taps=S.TAP1)
    # (two groups need two images: the one-image halo / dma shapes would be refused for n % groups, not for the kernel)
    halo2, dma2 = S.Case(S.HALO, 2, 16, 16, 128, 128, 2), S.Case(S.DMA, 2, 16, 16, 128, 256, 2)
    return [("sums-on-halo", halo, "sums"), ("sums-on-dma", dma, "sums"),
            ("bwdsum-on-ragged-small", S.Case(S.SMALL, 2, 20, 18, 16, 16, 2), "bwd"),
            ("n-not-divisible-by-groups", S.Case(S.RES, 3, 16, 16, 32, 32, 2), "plain"),
            ("epilogue-on-small", small, "epi"), ("epilogue-on-res", res, "epi"), ("epilogue-on-tile", tile, "epi"),
            # the rest of what the capability table (conv_caps, common.h) refuses
            ("bwdsum-on-tile", tile, "bwd"), ("bwdsum-on-gemm", gemm, "bwd"), ("bwdsum-on-halo", halo, "bwd"), ("bwdsum-on-dma", dma, "bwd"),
            ("two-groups-on-halo", halo2, "plain"), ("two-groups-on-dma", dma2, "plain"),
            ("bwdsum-with-sums-on-small", small, "bwd+sums"), ("bwdsum-with-sums-on-res", res, "bwd+sums"),
            ("slice-sums-on-small", S.Case(S.SMALL, 2, 16, 16, 16, 16, 2, c0=8, C=8), "sums")]


@pytest.mark.parametrize("name,c,what", _reject_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_unsupported_combinations_are_refused(name, c, what):
    x, w, b, _ = shared(c)
    acc, bacc = Acc(8, c.groups, c.nsum), Acc(8, c.groups, c.co)
    kw = {}
    if "sums" in what:
        kw.update(acc=acc, c0=c.c0)
    if what == "epi":
        kw["relu"] = 1
    if "bwd" in what:
        Y, stat, mask = (t.to(DEV) if t is not None else None for t in S.bwd_operands(c))
        kw["bwd"] = dict(Y=Y, stat=stat, mask=mask, acc=bacc)
    out, f, rc, msg = launch(c, x, w, b, expect_fail=True, **kw)
    assert rc != 0 and "stcd_op_conv_fused" in msg and len(msg) > 30, (rc, msg)
    assert bool((out == PREFILL).all()) and acc.untouched() and bacc.untouched(), "a refused request launched something"
