"""tests/conv_fused_spec.py on the CPU: its fp64 reference against torch's own convolution and sums, and -- on the reference
alone -- the conditions under which the exact-integer and rounded-value recipes ask the kernels for EQUALITY (every product and
partial sum an integer below 2^24).  Nothing here touches the library."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import conv_fused_spec as S


@functools.lru_cache(maxsize=None)
def _ref(key, c):
    x, w, b = S.exact_operands(c)
    return S.conv_ref(c, x, w, b)


def ref(c):
    return _ref(c.shape_key, S.Case("", c.n, c.h, c.w, c.ci, c.co, taps=c.taps, in_stride=c.in_stride, bias=c.bias))


def _uniq(cases):
    seen, out = set(), []
    for c in cases:
        k = (c.shape_key, c.groups)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


_TORCH_CASES = [next(c for c in S.SUM_CASES if (c.kernel, c.h, c.w, c.groups) == (S.RES, 20, 37, 2)),
                next(c for c in S.SUM_CASES if c.in_stride == 2)]


@pytest.mark.parametrize("c", _TORCH_CASES, ids=lambda c: c.id)
def test_reference_is_torch_conv2d_and_torch_sums(c):
    """a ragged 3x3 case with two groups and the stride-2 1x1 case: conv2d in fp64 (integers: both are exact), sums by torch"""
    x, w, b = S.exact_operands(c)
    got = S.conv_ref(c, x, w, b)
    k = 3 if len(c.taps) == 9 else 1
    wt = w.double().reshape(k, k, c.ci, c.co).permute(3, 2, 0, 1)            # tap (dy, dx) -> (ky, kx) = (dy + 1, dx + 1)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), wt, b.double(), stride=c.in_stride, padding=k // 2).permute(0, 2, 3, 1)
    assert got.shape == want.shape == (c.n, c.hm, c.wm, c.co)
    assert torch.equal(got, want)
    s1, s2 = S.group_sums(got, c.groups)
    npg = c.n // c.groups
    for g in range(c.groups):
        part = want[g * npg:(g + 1) * npg]
        assert torch.equal(s1[g], part.sum((0, 1, 2))) and torch.equal(s2[g], part.pow(2).sum((0, 1, 2)))
    q1 = S.fixed(s1, S.FS1)
    assert q1.dtype == torch.int64 and torch.equal(q1.double() / S.FS1, s1)


def test_case_tables_cover_what_the_kernels_branch_on():
    ids = [c.id for c in S.SUM_CASES + S.ROUNDED_CASES + S.REAL_SUM_CASES + S.EPI_CASES + S.EPI_REAL_CASES + S.BWD_CASES]
    assert len(set(c.id for c in S.SUM_CASES)) == len(S.SUM_CASES) and len(set(c.id for c in S.EPI_CASES)) == len(S.EPI_CASES), ids
    for k in (S.SMALL, S.RES, S.TILE, S.GEMM):
        assert sum(c.kernel == k for c in S.ROUNDED_CASES) == 1 and sum(c.kernel == k for c in S.REAL_SUM_CASES) == 1
    for c in S.ROUNDED_CASES:
        assert (c.h, c.w, c.groups, c.n) == (8, 16, 2, 2)
    for c in S.REAL_SUM_CASES:
        assert (c.n // c.groups) * c.hm * c.wm <= 512
    for c in S.SUM_CASES:      # a slice request is a strict sub-range that starts on a 16-channel tile
        assert 0 <= c.c0 and c.c0 + c.nsum <= c.co and c.c0 % 16 == 0
    assert {(c.alpha, c.beta) for c in S.EPI_CASES if c.mode in ("res", "all")} == {(a, b) for a in (1.0, 0.5, 2.0) for b in (1.0, -1.0)}
    assert {(c.kernel, c.mode) for c in S.EPI_CASES} == {(k, m) for k in (S.GEMM, S.HALO, S.DMA) for m in ("relu", "gate", "res", "all")}
    assert any(not c.mask for c in S.BWD_CASES) and any(c.mask for c in S.BWD_CASES)


@pytest.mark.parametrize("c", _uniq(S.SUM_CASES + S.EPI_CASES + S.BWD_CASES), ids=lambda c: c.id)
def test_exact_integer_recipe_is_exact(c):
    """max|y| <= 256, sum(y^2) per (group, channel) < 2^24, y not constant -- with the margin the recipe was chosen for"""
    ymax, s2max = S.exact_conditions(c, ref(c))
    assert ymax <= 128 and s2max < 2 ** 22, (ymax, s2max)        # (a wide margin: nothing here sits near the edge)
    if c.groups > 1:        # the one-group launch of the same operands sums both groups into one entry
        S.exact_conditions(S.Case(**{**c.__dict__, "groups": 1}), ref(c))


@pytest.mark.parametrize("c", S.EPI_CASES, ids=lambda c: c.id)
def test_epilogue_recipe_stays_exact_in_fp32(c):
    """alpha * v + beta * res is a multiple of 1/2 below 2^23 (fp32 forms it exactly, fused or not), the gate holds both zeros
    and both signs, the unused channels are NaN, and the epilogue changes the output"""
    y = ref(c)
    gate, res = S.epi_operands(c)
    assert gate.shape[-1] > c.co and res.shape[-1] > c.co and gate.shape[-1] != res.shape[-1]
    assert bool(gate[..., c.co:].isnan().all()) and bool(res[..., c.co:].isnan().all())
    gv = gate[..., :c.co].float()
    assert bool((gv > 0).any()) and bool((gv < 0).any())
    assert bool(((gv == 0) & torch.signbit(gv)).any()) and bool(((gv == 0) & ~torch.signbit(gv)).any())
    if c.out_stride == 1:
        g = gate[..., :c.co] if c.mode in ("gate", "all") else None
        r = res[..., :c.co] if c.mode in ("res", "all") else None
        out, summed = S.epi_ref(y, c.relu, g, r, c.alpha, c.beta)
        assert not torch.equal(out, y)
        assert bool(((2 * out) == (2 * out).round()).all()) and float(out.abs().max()) < 2 ** 23
        if c.relu:
            assert float(summed.min()) == 0.0 and bool((y < 0).any())


@pytest.mark.parametrize("c", S.ROUNDED_CASES, ids=lambda c: c.id)
def test_rounded_value_recipe_rounds(c):
    """y in 257 ... 511 with odd values among them; <= 186 values per (group, channel); the sums of the stored values are exact in
    fp32 (< 2^24) and differ from the sums of y"""
    y = ref(c)
    assert (c.n // c.groups) * c.hm * c.wm <= 186
    assert 257 <= float(y.min()) and float(y.max()) <= 511 and bool((y == y.round()).all())
    assert bool((y % 2 == 1).any())
    st = S.rne_bf16(y)
    assert bool((st % 2 == 0).all()) and float((st - y).abs().max()) == 1.0
    s1, s2 = S.group_sums(st, c.groups)
    u1, u2 = S.group_sums(y, c.groups)
    assert float(s2.max()) < 2 ** 24 and float(u2.max()) < 2 ** 24
    assert bool((s1 != u1).any()) and bool((s2 != u2).any())


@pytest.mark.parametrize("c", S.BWD_CASES, ids=lambda c: c.id)
def test_bwdsum_recipe_is_exact(c):
    """every term dz and dz * (y - mean) * invstd is a multiple of 1/2 and the sum of their magnitudes stays below 2^23, so any
    fp32 summation order is exact; z takes both signs and exactly 0; the mask drops and doubles"""
    dA = S.rne_bf16(ref(c))
    assert torch.equal(dA, ref(c))
    Y, stat, mask = S.bwd_operands(c)
    dz, dzx, z = S.bwd_terms(dA, Y, stat, mask, c.groups)
    assert bool((z == 0).any()) and bool((z > 0).any()) and bool((z < 0).any()) and bool((z == z.round()).all())
    for t in (dz, dzx):
        assert bool(((2 * t) == (2 * t).round()).all())
        assert float(t.abs().reshape(c.groups, -1, c.co).sum(1).max()) < 2 ** 23
    assert bool((dzx != 0).any()) and bool((dz != 0).any())
    if c.mask:
        assert set(mask.unique().tolist()) == {0.0, 2.0}
    else:
        assert mask is None
    s1, s2 = S.bwd_sums(dA, Y, stat, mask, c.groups)
    q = S.fixed(s2, S.BS)
    assert torch.equal(q.double() / S.BS, s2) and float(s2.abs().max()) * S.BS < 2 ** 62
    assert stat.shape == (c.groups, 4, c.co) and set(stat[:, 1].unique().tolist()) <= {0.5, 1.0, 2.0}
    # the fused forms' geometry (conv_small_bwdsum_ok / conv_res_bwdsum_ok): k_conv_small wants whole 8 x 16 tiles and 16 channels
    if c.kernel == S.SMALL:
        assert c.co == 16 and c.h % 8 == 0 and c.w % 16 == 0 and (9 * c.ci + 31) // 32 in (3, 5)


def test_sum_bound_formula():
    assert S.sum_bound(512, 100.0, 4, S.FS1) == 513 * 2.0 ** -24 * 100.0 + 4 / (2 * 2.0 ** 26)
