"""Cases, operand recipes and a plain fp64 reference for the features the engine fuses into its bf16 conv kernels (reached per
kernel through stcd_op_conv_fused): per-(group, channel) sums of the rounded output in int64 fixed point, the ConvEpi epilogue,
and the BatchNorm-backward sums of a data gradient.  This module does not import the library; tests/test_conv_fused_cpu.py checks
it on the CPU, tests/test_conv_fused_gpu.py compares the kernels with it.

The exact-integer recipe.  x and w take values in {-1, 0, +1} with a quarter of the entries non-zero, the bias is an integer in
[-2, 2].  Every product and every partial sum of the convolution AND of the per-channel sums is then an integer below 2^24, which
fp32 holds exactly: MFMA, per-thread fp32 sums, shuffles, LDS reductions and the fixed-point add (llrint of an integer times a
power of two) give the same bits in every order.  The tests therefore ask for equality, of the stored bf16 output and of the
accumulators.  `exact_conditions` states what makes that valid (checked for every case by the CPU test): max|y| <= 256 (integers up
to 256 are bf16 values), sum(y^2) per (group, channel) < 2^24 (which bounds sum|y| too: |y| <= y^2 for integers), y not constant.

The rounded-value recipe.  The same operands with bias +300 on an 8 x 16 map, one image per group: y lies in 257 ... 511, where
bf16 holds the even integers only.  The stored output is RNE-bf16(y), and the sums must be those of the STORED values (exact
again: even integers, at most 128 per (group, channel)), which differ from the sums of y."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

TAPS3 = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
TAP1 = ((0, 0),)
TAPS4 = ((0, 0), (0, 1), (1, 0), (1, 1))           # one sub-pixel phase of a 2x2-tap data gradient (tests/test_ops_gpu.py DMA_CASES)
SMALL, RES, TILE, GEMM, HALO, DMA = "small", "res", "tile", "gemm", "halo", "dma"
FS1, FS2, BS = 2.0 ** 26, 2.0 ** 18, 2.0 ** 36      # BatchNorm statistics sum(y), sum(y^2); backward sums / bias gradients


@dataclass(frozen=True)
class Case:
    kernel: str
    n: int
    h: int                 # the INPUT map
    w: int
    ci: int
    co: int
    groups: int = 1
    taps: Tuple[Tuple[int, int], ...] = TAPS3
    in_stride: int = 1
    out_stride: int = 1
    o0: Tuple[int, int] = (0, 0)
    c0: int = 0            # summed channel slice [c0, c0 + C); C None: all channels
    C: Optional[int] = None
    scales: Tuple[float, float] = (FS1, FS2)
    relu: int = 0
    bias: Optional[int] = None       # None: integers in [-2, 2]; else this constant
    mode: str = ""         # ConvEpi sub-case: relu / gate / res / all
    alpha: float = 1.0
    beta: float = 1.0
    mask: bool = True      # BwdSum: Dropout2d factors given (False: NULL)
    tag: str = ""

    @property
    def hm(self): return (self.h + self.in_stride - 1) // self.in_stride
    @property
    def wm(self): return (self.w + self.in_stride - 1) // self.in_stride
    @property
    def ho(self): return self.hm * self.out_stride
    @property
    def wo(self): return self.wm * self.out_stride
    @property
    def nsum(self): return self.co - self.c0 if self.C is None else self.C
    @property
    def shape_key(self):   # cases with the same key share operands and the reference convolution
        return (self.n, self.h, self.w, self.ci, self.co, self.taps, self.in_stride, self.bias)
    @property
    def id(self):
        s = f"{self.kernel}-{self.n}x{self.h}x{self.w}-{self.ci}-{self.co}-g{self.groups}-t{len(self.taps)}"
        for t in (self.tag, self.mode):
            if t:
                s += "-" + t
        return s


# ---- fused sums, exact-integer recipe (n counts both dates when groups = 2)
SUM_CASES = [
    # k_conv_small <1, 3> / <1, 5>; a ragged 8 x 16 tile grid
    Case(SMALL, 2, 16, 16, 8, 16, 2), Case(SMALL, 6, 24, 16, 16, 16, 2), Case(SMALL, 2, 20, 18, 16, 16, 1),
    Case(SMALL, 2, 264, 512, 8, 16, 2, tag="walk"),                        # 1056 tiles per group over its 1024 blocks
    # k_conv_res: ragged border tiles; odd batch with one group; 128 channels in; one tile per block at 128 tiles per group
    Case(RES, 2, 16, 16, 32, 32, 2), Case(RES, 6, 20, 37, 32, 48, 2), Case(RES, 3, 48, 80, 64, 32, 1), Case(RES, 4, 33, 16, 128, 64, 2),
    Case(RES, 16, 64, 64, 32, 32, 2),
    Case(RES, 2, 150, 200, 32, 128, 2, tag="walk"),                        # 130 ragged tiles per group: more than the blocks that share them
    Case(RES, 2, 12, 16, 256, 32, 2, tag="cw64"),                          # the 64-channel-step form (Ci = 256, small map)
    Case(RES, 6, 20, 37, 32, 48, 2, c0=16, C=16, scales=(BS, BS), tag="slice"),   # a concat slice's bias gradient
    # k_conv_tile
    Case(TILE, 2, 16, 16, 64, 64, 2), Case(TILE, 6, 20, 37, 128, 32, 2), Case(TILE, 3, 32, 32, 256, 128, 1),
    Case(TILE, 2, 130, 120, 64, 128, 2, tag="walk"),                       # 72 ragged tiles per group
    # k_conv_gemm: 1x1 unless noted; Mg = 105 (ragged M-tile); stride-2 1x1; the 128 x 128 tile; K = 2048; 3x3 taps
    Case(GEMM, 4, 32, 32, 64, 64, 2, taps=TAP1), Case(GEMM, 6, 5, 7, 64, 128, 2, taps=TAP1),
    Case(GEMM, 4, 32, 32, 256, 512, 2, taps=TAP1, in_stride=2), Case(GEMM, 4, 32, 32, 256, 1024, 2, taps=TAP1, tag="t128"),
    Case(GEMM, 2, 8, 8, 2048, 512, 2, taps=TAP1), Case(GEMM, 2, 9, 11, 512, 64, 1),
    Case(GEMM, 6, 5, 7, 64, 128, 2, taps=TAP1, c0=48, C=32, scales=(BS, BS), tag="slice"),      # crosses the 64-channel tile boundary
    Case(GEMM, 4, 32, 32, 64, 64, 2, taps=TAP1, relu=1, tag="relu"),
]
GROUP1_KERNELS = (SMALL, RES, TILE)     # also launched with one group on the same operands: the two group sums add up to its sum

# ---- fused sums, rounded-value recipe: 8 x 16, one image per group
ROUNDED_CASES = [Case(SMALL, 2, 8, 16, 16, 16, 2, bias=300), Case(RES, 2, 8, 16, 32, 32, 2, bias=300),
                 Case(TILE, 2, 8, 16, 64, 32, 2, bias=300), Case(GEMM, 2, 8, 16, 64, 64, 2, bias=300)]

# ---- fused sums, real-valued operands (standard normal, rounded to bf16): <= 512 values per (group, channel)
REAL_SUM_CASES = [Case(SMALL, 2, 16, 16, 16, 16, 2), Case(RES, 2, 16, 16, 32, 32, 2), Case(TILE, 2, 16, 16, 64, 64, 2),
                  Case(GEMM, 2, 16, 16, 64, 64, 2, taps=TAP1)]

# ---- ConvEpi, exact-integer recipe
_EPI_SHAPES = [
    Case(GEMM, 4, 32, 32, 256, 64), Case(GEMM, 3, 12, 20, 64, 128, taps=TAPS4, out_stride=2, o0=(1, 0)),
    Case(HALO, 1, 16, 16, 128, 128), Case(HALO, 2, 20, 37, 128, 256),
    Case(DMA, 1, 16, 16, 128, 256), Case(DMA, 2, 20, 37, 128, 256), Case(DMA, 2, 24, 40, 256, 256, taps=TAPS4, out_stride=2, o0=(1, 0)),
]
_AB = [(1.0, 1.0), (0.5, -1.0), (2.0, 1.0), (0.5, 1.0), (2.0, -1.0), (1.0, -1.0)]      # alpha in {1, 0.5, 2} x beta in {1, -1}


def _epi_cases():
    out, k = [], 0
    for shp in _EPI_SHAPES:
        for mode in ("relu", "gate", "res", "all"):
            a, b = (1.0, 1.0)
            if mode in ("res", "all"):
                a, b = _AB[k % len(_AB)]
                k += 1
            out.append(Case(**{**shp.__dict__, "mode": mode, "alpha": a, "beta": b, "relu": int(mode in ("relu", "all"))}))
    return out


EPI_CASES = _epi_cases()
EPI_REAL_CASES = [Case(GEMM, 2, 16, 16, 64, 64, mode="all", relu=1, alpha=0.5, beta=-1.0),
                  Case(HALO, 1, 16, 16, 128, 128, mode="all", relu=1, alpha=2.0, beta=1.0),
                  Case(DMA, 1, 16, 16, 128, 256, mode="all", relu=1, alpha=0.5, beta=1.0)]

# ---- BwdSum (the data gradient's conv is the exact-integer recipe's)
BWD_CASES = [Case(SMALL, 2, 16, 16, 16, 16, 2, mask=False), Case(SMALL, 4, 24, 32, 8, 16, 2),
             Case(RES, 2, 16, 16, 32, 32, 2), Case(RES, 6, 20, 37, 64, 32, 2)]


# ------------------------------------------------------------------ operand recipes (CPU tensors; deterministic per shape)
def _rng(c: Case, salt: int):
    return np.random.default_rng([c.n, c.h, c.w, c.ci, c.co, len(c.taps), c.in_stride, salt])


def _ternary(rng, shape):
    return ((rng.random(shape) < 0.25) * (rng.integers(0, 2, shape) * 2 - 1)).astype(np.float32)


def exact_operands(c: Case):
    """x bf16 [n][h][w][ci], w fp32 [taps][ci][co], bias fp32 [co]"""
    rng = _rng(c, 1)
    x = torch.from_numpy(_ternary(rng, (c.n, c.h, c.w, c.ci))).bfloat16()
    w = torch.from_numpy(_ternary(rng, (len(c.taps), c.ci, c.co)))
    b = rng.integers(-2, 3, c.co).astype(np.float32) if c.bias is None else np.full(c.co, float(c.bias), np.float32)
    return x, w, torch.from_numpy(b)


def real_operands(c: Case):
    rng = _rng(c, 2)
    x = torch.from_numpy(rng.standard_normal((c.n, c.h, c.w, c.ci)).astype(np.float32)).bfloat16()
    w = torch.from_numpy(rng.standard_normal((len(c.taps), c.ci, c.co)).astype(np.float32)).bfloat16().float()
    b = torch.from_numpy(rng.standard_normal(c.co).astype(np.float32)).bfloat16().float()
    return x, w, b


def epi_operands(c: Case, pad_g=8, pad_r=16, real=False):
    """gate, res: bf16 [n][ho][wo][co + pad] with NaN in the channels past co (they belong to nobody: never read).
    gate in {-1, -0.0, 0, +1} (both zeros gate off); res integers in [-8, 8] (real: standard normal)."""
    rng = _rng(c, 3)
    shp = (c.n, c.ho, c.wo)
    gate = torch.full(shp + (c.co + pad_g,), float("nan"), dtype=torch.bfloat16)
    gate[..., :c.co] = torch.from_numpy(np.array([-1.0, -0.0, 0.0, 1.0], np.float32)[rng.integers(0, 4, shp + (c.co,))]).bfloat16()
    res = torch.full(shp + (c.co + pad_r,), float("nan"), dtype=torch.bfloat16)
    r = rng.standard_normal(shp + (c.co,)).astype(np.float32) if real else rng.integers(-8, 9, shp + (c.co,)).astype(np.float32)
    res[..., :c.co] = torch.from_numpy(r).bfloat16()
    return gate, res


def bwd_operands(c: Case):
    """Y bf16 [n][h][w][co] integers in [-3, 3]; stat fp32 [groups][4][co] = integer mean, invstd in {0.5, 1, 2}, scale in
    {-1, 1, 2}, integer shift in [-2, 2] (z = y * scale + shift is an integer of either sign, 0 included); mask fp32 [n][co] in
    {0, 2} or None"""
    rng = _rng(c, 4)
    Y = torch.from_numpy(rng.integers(-3, 4, (c.n, c.h, c.w, c.co)).astype(np.float32)).bfloat16()
    stat = np.empty((c.groups, 4, c.co), np.float32)
    stat[:, 0] = rng.integers(-2, 3, (c.groups, c.co))
    stat[:, 1] = np.array([0.5, 1.0, 2.0], np.float32)[rng.integers(0, 3, (c.groups, c.co))]
    stat[:, 2] = np.array([-1.0, 1.0, 2.0], np.float32)[rng.integers(0, 3, (c.groups, c.co))]
    stat[:, 3] = rng.integers(-2, 3, (c.groups, c.co))
    mask = torch.from_numpy((2.0 * rng.integers(0, 2, (c.n, c.co))).astype(np.float32)) if c.mask else None
    return Y, torch.from_numpy(stat), mask


# ------------------------------------------------------------------ the fp64 reference (any device)
def conv_ref(c: Case, x, w, bias):
    """y [n][hm][wm][co] fp64 = bias + sum_t X(m * in_stride + tap_t) . W[t], zero outside the image (shift + matmul per tap)."""
    dev = x.device
    xd, wd = x.double(), w.double()
    y = bias.double().view(1, 1, 1, c.co).expand(c.n, c.hm, c.wm, c.co).clone()
    for t, (dy, dx) in enumerate(c.taps):
        ys = torch.arange(c.hm, device=dev) * c.in_stride + dy
        xs = torch.arange(c.wm, device=dev) * c.in_stride + dx
        ok = ((ys >= 0) & (ys < c.h)).view(1, -1, 1, 1) & ((xs >= 0) & (xs < c.w)).view(1, 1, -1, 1)
        sub = xd[:, ys.clamp(0, c.h - 1)][:, :, xs.clamp(0, c.w - 1)] * ok
        y += (sub.reshape(-1, c.ci) @ wd[t]).reshape(c.n, c.hm, c.wm, c.co)
    return y


def rne_bf16(v):
    """round-to-nearest-even to bf16, returned as fp64 (the values the tests feed are fp32-exact, so there is ONE rounding)"""
    return v.float().bfloat16().double()


def group_sums(v, groups, c0=0, C=None):
    """v [n][..][co] fp64 (the STORED values) -> (sum v, sum v^2), each [groups][C] fp64, over the images of each group"""
    n, co = v.shape[0], v.shape[-1]
    C = co - c0 if C is None else C
    g = v[..., c0:c0 + C].reshape(groups, -1, C)
    return g.sum(1), (g * g).sum(1)


def fixed(s, scale):
    """fp64 sums -> the int64 fixed-point value the accumulators hold (exact for the exact recipes: integer * power of two)"""
    return torch.round(s * scale).to(torch.int64)


def epi_ref(y, relu, gate, res, alpha, beta):
    """ConvEpi in the order common.h documents: v = relu(v); v = round(v); v = gate > 0 ? v : 0; out = round(alpha * v + beta * res).
    Returns (out, v after relu and rounding -- what the fused sums of k_conv_gemm see)."""
    v = y.clamp_min(0.0) if relu else y
    v = rne_bf16(v)
    summed = v
    if gate is not None:
        v = torch.where(gate.double() > 0, v, torch.zeros_like(v))
    if res is not None:
        v = rne_bf16(alpha * v + beta * res.double())
    return v, summed


def bwd_terms(dA, Y, stat, mask, groups):
    """k_bn_reduce<T, 1>'s terms: dz = dA * mask * (y * scale + shift > 0) and dz * (y - mean) * invstd, both [n][h][w][co] fp64.
    dA: the STORED (rounded) data gradient."""
    n, co = dA.shape[0], dA.shape[-1]
    gi = torch.arange(n, device=dA.device) // (n // groups)
    st = stat.double()[gi]                                        # [n][4][co]
    mean, inv, sc, sh = (st[:, k].view(n, 1, 1, co) for k in range(4))
    yd = Y.double()
    z = yd * sc + sh
    dz = dA * (mask.double().view(n, 1, 1, co) if mask is not None else 1.0)
    dz = torch.where(z > 0, dz, torch.zeros_like(dz))
    return dz, dz * (yd - mean) * inv, z


def bwd_sums(dA, Y, stat, mask, groups):
    dz, dzx, _ = bwd_terms(dA, Y, stat, mask, groups)
    co = dA.shape[-1]
    return dz.reshape(groups, -1, co).sum(1), dzx.reshape(groups, -1, co).sum(1)


def exact_conditions(c: Case, y):
    """what makes the exact-integer recipe exact for this case; y: conv_ref (before the epilogue)"""
    assert float(y.abs().max()) <= 256, (c.id, float(y.abs().max()))
    assert bool((y == y.round()).all()), c.id
    _, s2 = group_sums(y, c.groups)
    assert float(s2.max()) < 2 ** 24, (c.id, float(s2.max()))
    assert float(y.min()) < float(y.max()), c.id
    return float(y.abs().max()), float(s2.max())


def sum_bound(nvals, sum_abs, blocks, scale):
    """|fused sum - fp64 sum of the same stored values| <= (n + 1) * 2^-24 * sum|x| + B / (2 * scale): the worst-case fp32 error of
    ANY summation order of n values (n - 1 additions, each off by <= 2^-24 of a partial sum <= sum|x|) plus one rounding of each
    value (the squares), plus one llrint (<= 1/2 unit of 1 / scale) per atomic add, of which there are at most B = blocks."""
    return (nvals + 1) * 2.0 ** -24 * sum_abs + blocks / (2.0 * scale)
