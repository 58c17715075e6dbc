// kernels_snhead.hip -- the head of Siam_NestedUNet_Conc (SNUNet-CD without attention, SNUNet.py:195-199, 238-242):
//     output_i = final_i(x0_i), i = 1..4 (Conv2d(32, L, 1));  output = conv_final(cat(output_1..4)) (Conv2d(4L, L, 1)).
// x0_1..x0_4 sit side by side in the 128-channel NHWC buffer E, and the head is linear, so it runs as ONE 1x1 conv 128 -> NO
// whose filter is composed from the ten parameter tensors in every block's prologue (a few hundred FMAs, no launch of its own, no
// stale image under frozen weights):
//     W_eff[:, 32i:32i+32] = Wf[:, iL:iL+L] . W_i      b_eff = bf + sum_i Wf[:, iL:iL+L] . b_i
//     plain id:            NO = L   rows = W_eff
//     deep supervision:    NO = 5L  rows [iL, iL+L) = W_i on channel block i (zero elsewhere), rows [4L, 5L) = W_eff
// Both ids read / write the fp32 NCHW maps directly, map-major ([NM * B, L, H, W], NM = 1 or 5: output1..4, then the fused map);
// neither output_1..4 nor their concat nor a packed output gradient ever exists as a B.H.W tensor.  The kernels stream E once
// per direction: 16 lanes own the 128 channels of a pixel (16 B each), a wave owns chunks of 64 consecutive pixels (H.W is a
// multiple of 256, so a chunk never straddles two images) and meets the maps with one coalesced access per output row.
// Backward: dE = W_all^T . G (written once), and the filter / bias gradients of the composed conv as per-block partial sums in a
// FIXED order (lane -> wave -> block), folded by k_snhead_reduce in block order and turned into the ten parameter gradients by
// k_snhead_chain -- no float atomics, the same bytes every run.
// NOC (2 or 10) is the compiled row count; rows >= NO are zero padding.  The fused rows go through the same instructions for
// either NOC, so the last map of the deep-supervision id equals the plain id's output bit for bit.
#include "common.h"

namespace stcd {

static constexpr int SNH_C = 128;             // channels of E (4 x 32)
static constexpr int SNH_THREADS = 256;

template <int NOC>
__device__ __forceinline__ void snhead_compose(const SnHeadParams& p, float* sW, float* sB) {
    const int L = p.L, NO = p.ds ? 5 * L : L, f0 = p.ds ? 4 * L : 0;
    for (int idx = threadIdx.x; idx < NOC * SNH_C; idx += SNH_THREADS) {
        const int o = idx / SNH_C, c = idx % SNH_C, i = c >> 5, cc = c & 31;
        float v = 0.f;
        if (o < f0) {
            const int m = o / L, l = o - m * L;
            if (m == i) v = p.w[i][l * 32 + cc];
        } else if (o < NO) {
            const int l = o - f0;
            for (int k = 0; k < L; ++k) v = fmaf(p.wf[l * 4 * L + i * L + k], p.w[i][k * 32 + cc], v);
        }
        sW[idx] = v;
    }
    for (int o = threadIdx.x; o < NOC; o += SNH_THREADS) {
        float v = 0.f;
        if (o < f0) {
            const int m = o / L;
            v = p.b[m][o - m * L];
        } else if (o < NO) {
            const int l = o - f0;
            for (int i = 0; i < 4; ++i)
                for (int k = 0; k < L; ++k) v = fmaf(p.wf[l * 4 * L + i * L + k], p.b[i][k], v);
            v += p.bf[l];
        }
        sB[o] = v;
    }
}

// element offset of row o of the map-major fp32 NCHW maps at (image n, pixel 0)
__device__ __forceinline__ int64_t snhead_row_off(int o, int L, int B, int n, int64_t HW) {
    const int m = o / L, l = o - m * L;
    return (((int64_t)m * B + n) * L + l) * HW;
}

template <typename T, int NOC>
__global__ void __launch_bounds__(SNH_THREADS)
k_snhead_fwd(const T* __restrict__ E, int ld, SnHeadParams p, float* __restrict__ out, int B, int64_t HW, int64_t nchunks) {
    __shared__ float sW[NOC * SNH_C];
    __shared__ float sB[NOC];
    snhead_compose<NOC>(p, sW, sB);
    __syncthreads();
    const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
    const int NO = p.ds ? 5 * p.L : p.L;
    float w[NOC][8];
#pragma unroll
    for (int o = 0; o < NOC; ++o)
#pragma unroll
        for (int k = 0; k < 8; ++k) w[o][k] = sW[o * SNH_C + sub * 8 + k];
    const int64_t nw = (int64_t)gridDim.x * (SNH_THREADS / 64);
    for (int64_t chunk = (int64_t)blockIdx.x * (SNH_THREADS / 64) + (threadIdx.x >> 6); chunk < nchunks; chunk += nw) {
        const int64_t p0 = chunk * 64;
        float res[NOC];
#pragma unroll
        for (int o = 0; o < NOC; ++o) res[o] = 0.f;
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
            float v[8];
            load8<T>(E + (p0 + it * 4 + grp) * ld + sub * 8, v);
#pragma unroll
            for (int o = 0; o < NOC; ++o) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) a = fmaf(w[o][k], v[k], a);
                a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64); a += __shfl_xor(a, 8, 64);
                res[o] = sub == it ? a : res[o];
            }
        }
        // this lane now holds every row of pixel p0 + sub * 4 + grp: 64 lanes = 64 consecutive floats of each row
        const int n = (int)(p0 / HW);
        const int64_t hw = p0 - (int64_t)n * HW + sub * 4 + grp;
#pragma unroll
        for (int o = 0; o < NOC; ++o)
            if (o < NO) out[snhead_row_off(o, p.L, B, n, HW) + hw] = res[o] + sB[o];
    }
}

// part: [gridDim.x][NOC * 128 + NOC] = per-block sums of G (x) E, then of G
template <typename T, int NOC>
__global__ void __launch_bounds__(SNH_THREADS)
k_snhead_bwd(const T* __restrict__ E, int ld, SnHeadParams p, const float* __restrict__ G, T* __restrict__ dE, int ldd,
             float* __restrict__ part, int B, int64_t HW, int64_t nchunks) {
    __shared__ float sW[NOC * SNH_C];
    __shared__ float sB[NOC];
    __shared__ float sR[SNH_THREADS / 64][NOC * SNH_C + NOC];
    snhead_compose<NOC>(p, sW, sB);
    __syncthreads();
    const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4, wave = threadIdx.x >> 6;
    const int NO = p.ds ? 5 * p.L : p.L;
    float w[NOC][8], dw[NOC][8], gs[NOC];
#pragma unroll
    for (int o = 0; o < NOC; ++o) {
        gs[o] = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { w[o][k] = sW[o * SNH_C + sub * 8 + k]; dw[o][k] = 0.f; }
    }
    const int64_t nw = (int64_t)gridDim.x * (SNH_THREADS / 64);
    for (int64_t chunk = (int64_t)blockIdx.x * (SNH_THREADS / 64) + wave; chunk < nchunks; chunk += nw) {
        const int64_t p0 = chunk * 64;
        const int n = (int)(p0 / HW);
        const int64_t hw = p0 - (int64_t)n * HW + sub * 4 + grp;
        float gv[NOC];          // the output gradient of pixel p0 + sub * 4 + grp, every row (coalesced per row)
#pragma unroll
        for (int o = 0; o < NOC; ++o) {
            gv[o] = o < NO ? G[snhead_row_off(o, p.L, B, n, HW) + hw] : 0.f;
            gs[o] += gv[o];
        }
#pragma unroll 2
        for (int it = 0; it < 16; ++it) {
            const int64_t pix = p0 + it * 4 + grp;
            float v[8], d[8];
            load8<T>(E + pix * ld + sub * 8, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = 0.f;
#pragma unroll
            for (int o = 0; o < NOC; ++o) {
                const float g = __shfl(gv[o], (lane & 48) | it, 64);
#pragma unroll
                for (int k = 0; k < 8; ++k) { dw[o][k] = fmaf(g, v[k], dw[o][k]); d[k] = fmaf(w[o][k], g, d[k]); }
            }
            store8<T>(dE + pix * ldd + sub * 8, d);
        }
    }
    // lanes of equal `sub` hold the same filter slice: fold the four pixel groups, then the waves, in a fixed order
#pragma unroll
    for (int o = 0; o < NOC; ++o) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float a = dw[o][k];
            a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
            if (grp == 0) sR[wave][o * SNH_C + sub * 8 + k] = a;
        }
        const float b = wave_sum(gs[o]);
        if (lane == 0) sR[wave][NOC * SNH_C + o] = b;
    }
    __syncthreads();
    constexpr int PS = NOC * SNH_C + NOC;
    for (int i = threadIdx.x; i < PS; i += SNH_THREADS) {
        float a = sR[0][i];
#pragma unroll
        for (int q = 1; q < SNH_THREADS / 64; ++q) a += sR[q][i];
        part[(int64_t)blockIdx.x * PS + i] = a;
    }
}

// red[i] = sum over blocks of part[blk][i], in block order (fp64 running sum)
__global__ void k_snhead_reduce(const float* __restrict__ part, int nblk, int ps, float* __restrict__ red) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ps) return;
    double a = 0.0;
    for (int b = 0; b < nblk; ++b) a += (double)part[(int64_t)b * ps + i];
    red[i] = (float)a;
}

// the chain rule from the composed conv's gradients (S = rows of W_eff, D_i = row block i on channel block i, g = bias sums) to
// the ten parameter gradients:
//     dW_i = D_i + Wf[:, iL:iL+L]^T . S[:, 32i:32i+32]         db_i = g_i + Wf[:, iL:iL+L]^T . g_f
//     dWf[:, iL:iL+L] = S[:, 32i:32i+32] . W_i^T + g_f (x) b_i    dbf = g_f
__global__ void k_snhead_chain(const float* __restrict__ red, int noc, SnHeadParams p, SnHeadGrads g) {
    const int L = p.L, f0 = p.ds ? 4 * L : 0, t = threadIdx.x;
    const float* S = red + (int64_t)f0 * SNH_C;          // [L][128]
    const float* gb = red + (int64_t)noc * SNH_C;        // [noc]
    const float* gf = gb + f0;
    for (int idx = t; idx < 4 * L * 32; idx += blockDim.x) {          // dW_i[l'][cc]
        const int i = idx / (L * 32), r = idx - i * L * 32, lp = r >> 5, cc = r & 31;
        float v = p.ds ? red[(int64_t)(i * L + lp) * SNH_C + 32 * i + cc] : 0.f;
        for (int l = 0; l < L; ++l) v = fmaf(p.wf[l * 4 * L + i * L + lp], S[l * SNH_C + 32 * i + cc], v);
        g.w[i][r] = v;
    }
    for (int idx = t; idx < 4 * L; idx += blockDim.x) {               // db_i[l']
        const int i = idx / L, lp = idx - i * L;
        float v = p.ds ? gb[i * L + lp] : 0.f;
        for (int l = 0; l < L; ++l) v = fmaf(p.wf[l * 4 * L + i * L + lp], gf[l], v);
        g.b[i][lp] = v;
    }
    for (int idx = t; idx < L * 4 * L; idx += blockDim.x) {           // dWf[l][iL + l']
        const int l = idx / (4 * L), q = idx - l * 4 * L, i = q / L, lp = q - i * L;
        float v = gf[l] * p.b[i][lp];
        for (int cc = 0; cc < 32; ++cc) v = fmaf(S[l * SNH_C + 32 * i + cc], p.w[i][lp * 32 + cc], v);
        g.wf[idx] = v;
    }
    for (int l = t; l < L; l += blockDim.x) g.bf[l] = gf[l];
}

static inline int snhead_noc(int L, int ds) { return (ds || L > 2) ? 10 : 2; }
static inline int64_t snhead_chunks(int B, int64_t HW) { return (int64_t)B * HW / 64; }
// the block count is a function of the shape alone: the partial sums, and so the gradients, do not depend on the device
static inline int snhead_bwd_blocks(int B, int64_t HW) {
    const int64_t n = (snhead_chunks(B, HW) + 3) / 4;
    return (int)(n < 512 ? n : 512);
}

int64_t snhead_scratch_floats(int B, int64_t HW, int L, int ds) {
    const int noc = snhead_noc(L, ds);
    return (int64_t)(snhead_bwd_blocks(B, HW) + 1) * (noc * SNH_C + noc);
}

void launch_snhead_forward(int dt, const void* E, int ld, const SnHeadParams& p, float* out, int B, int64_t HW, hipStream_t s) {
    const int noc = snhead_noc(p.L, p.ds);
    const int64_t nch = snhead_chunks(B, HW);
    int64_t nb = (nch + 3) / 4;
    if (nb > 2048) nb = 2048;
#define SNH_FWD(T, N) k_snhead_fwd<T, N><<<(int)nb, SNH_THREADS, 0, s>>>((const T*)E, ld, p, out, B, HW, nch)
    if (dt == BF16) { if (noc == 2) SNH_FWD(bf16, 2); else SNH_FWD(bf16, 10); }
    else { if (noc == 2) SNH_FWD(float, 2); else SNH_FWD(float, 10); }
#undef SNH_FWD
}

void launch_snhead_backward(int dt, const void* E, int ld, const SnHeadParams& p, const SnHeadGrads& g, const float* G, void* dE,
                            int ldd, float* scratch, int B, int64_t HW, hipStream_t s) {
    const int noc = snhead_noc(p.L, p.ds), ps = noc * SNH_C + noc;
    const int64_t nch = snhead_chunks(B, HW);
    const int nb = snhead_bwd_blocks(B, HW);
    float* red = scratch + (int64_t)nb * ps;
#define SNH_BWD(T, N) k_snhead_bwd<T, N><<<nb, SNH_THREADS, 0, s>>>((const T*)E, ld, p, G, (T*)dE, ldd, scratch, B, HW, nch)
    if (dt == BF16) { if (noc == 2) SNH_BWD(bf16, 2); else SNH_BWD(bf16, 10); }
    else { if (noc == 2) SNH_BWD(float, 2); else SNH_BWD(float, 10); }
#undef SNH_BWD
    k_snhead_reduce<<<(ps + 63) / 64, 64, 0, s>>>(scratch, nb, ps, red);
    k_snhead_chain<<<1, 256, 0, s>>>(red, noc, p, g);
}

}  // namespace stcd
