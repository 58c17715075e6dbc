// kernels_ew.hip -- HBM-bound elementwise / reduction kernels of the change-detection engine (gfx950).
//
// Everything here is bandwidth work: every thread moves 8 channels (16 B in bf16, 32 B in fp32) per access,
// consecutive lanes touch consecutive 16-B chunks of NHWC rows, reductions go wave -> LDS -> one partial per
// block (no same-address atomics on the hot path).  Semantics restated from:
//   BatchNorm2d + ReLU + Dropout2d   /root/reference/models/SiamUnet_diff.py:19-20, applied :99
//   F.max_pool2d(2,2)                /root/reference/models/SiamUnet_diff.py:101
//   |T1-T2| / T2-T1 skip fusion      SiamUnet_diff.py:150 / SiamUnet_sub.py:150
//   ReplicationPad2d                 SiamUnet_diff.py:149
#include <cstdlib>

#include "common.h"

namespace stcd {

// 8 consecutive fp32 values (16-B aligned) as two float4 loads
__device__ __forceinline__ void ld8f(const float* p, float (&v)[8]) {
    float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}


// 8 consecutive activation values as they sit in memory: the load is issued now, the conversion happens at first use
// (software pipelining across a barrier / a table build: load8 would convert -- and therefore wait -- immediately)
template <typename T> struct Raw8;
template <> struct Raw8<bf16> {
    uint4 v;
    // makes the packed registers opaque to the optimiser: a second get() after it unpacks again instead of keeping the first
    // unpack's eight floats alive in between (register budget of the kernels that visit a value in two phases)
    __device__ __forceinline__ void opaque() { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
    __device__ __forceinline__ void ld(const bf16* p) { v = *reinterpret_cast<const uint4*>(p); }
    __device__ __forceinline__ void get(float (&o)[8]) const {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { o[2 * i] = __uint_as_float(w[i] << 16); o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    }
};
template <> struct Raw8<float> {
    float4 a, b;
    __device__ __forceinline__ void opaque() {}
    __device__ __forceinline__ void ld(const float* p) { a = *reinterpret_cast<const float4*>(p); b = *reinterpret_cast<const float4*>(p + 4); }
    __device__ __forceinline__ void get(float (&o)[8]) const { o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w; }
};

// V (4 or 8) consecutive values: the narrower piece halves a thread's registers where a kernel holds many pieces at once
template <typename T, int V> struct RawV;
template <typename T> struct RawV<T, 8> : Raw8<T> {};
template <> struct RawV<bf16, 4> {
    uint2 v;
    __device__ __forceinline__ void opaque() { asm volatile("" : "+v"(v.x), "+v"(v.y)); }
    __device__ __forceinline__ void ld(const bf16* p) { v = *reinterpret_cast<const uint2*>(p); }
    __device__ __forceinline__ void get(float (&o)[4]) const {
        o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
        o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
    }
};
template <> struct RawV<float, 4> {
    float4 a;
    __device__ __forceinline__ void opaque() {}
    __device__ __forceinline__ void ld(const float* p) { a = *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ void get(float (&o)[4]) const { o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; }
};
template <int V> __device__ __forceinline__ void ldVf(const float* p, float (&v)[V]) {
#pragma unroll
    for (int i = 0; i < V / 4; ++i) {
        const float4 a = *reinterpret_cast<const float4*>(p + 4 * i);
        v[4 * i] = a.x; v[4 * i + 1] = a.y; v[4 * i + 2] = a.z; v[4 * i + 3] = a.w;
    }
}
template <typename T, int V> __device__ __forceinline__ void storeV(T* p, const float (&v)[V]);
template <> __device__ __forceinline__ void storeV<bf16, 8>(bf16* p, const float (&v)[8]) { store8<bf16>(p, v); }
template <> __device__ __forceinline__ void storeV<float, 8>(float* p, const float (&v)[8]) { store8<float>(p, v); }
template <> __device__ __forceinline__ void storeV<bf16, 4>(bf16* p, const float (&v)[4]) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
}
template <> __device__ __forceinline__ void storeV<float, 4>(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// grid of the kernels that build a per-block BatchNorm table in their prologue: capped at ~2 resident rounds of the
// chip so the table (one dependent round trip + a few double operations per channel) is built <= 2048 times per launch
static inline int ew_grid(int64_t total_threads) { return (int)std::min<int64_t>(cdiv(total_threads, 256), 2048); }
// channel slabs of the BatchNorm consumer kernels: 64 channels per block from 128 channels up (a pixel's slab is one 128-B line)
static inline int bn_slabs(int C) {
    constexpr int min_c = 128;
    return (C >= min_c && C % 64 == 0) ? C / 64 : 1;
}

// grouped view: element (g, n_in_group, pix, c) at p + g*goff + (n_in_group*HW + pix)*ld + c
struct GV {
    int ld;
    int64_t goff;
};

// ------------------------------------------------------------------ pack / unpack at the NCHW fp32 boundary
template <typename T>
__global__ void k_in_pack(const float* __restrict__ x1, const float* __restrict__ x2, T* __restrict__ X, int B, int cin,
                          int64_t HW, int64_t total, int concat) {
    in_pack_body<T>(x1, x2, X, B, cin, HW, total, concat, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// dates = 2: images [x1; x2] (2B of them); dates = 1: x1 alone (single-image networks: x2 is not read); dates = 0: B images of
// cat(x1, x2) along the channels (2 * cin <= 8)
void launch_in_pack(int dt, const float* x1, const float* x2, void* X, int B, int cin, int H, int W, hipStream_t s, int dates) {
    const int concat = dates == 0 ? 1 : 0;
    int64_t HW = (int64_t)H * W, n = (int64_t)(concat ? 1 : dates) * B * HW;
    if (dt == BF16) k_in_pack<bf16><<<cdiv(n, 256), 256, 0, s>>>(x1, x2, (bf16*)X, B, cin, HW, n, concat);
    else k_in_pack<float><<<cdiv(n, 256), 256, 0, s>>>(x1, x2, (float*)X, B, cin, HW, n, concat);
}

// blocks [0, pack_blocks): g fp32 NCHW -> G [B,H,W,8] (+ the per-channel sums of g, keyed by the block index as before the zero blocks
// existed); blocks behind them: zero-fill of [zero_p, zero_p + zero_bytes), the backward's gradient buffer, instead of a memset launch
template <typename T>
__global__ void __launch_bounds__(256)
k_gout_pack(const float* __restrict__ g, T* __restrict__ G, int B, int L, int64_t HW, long long* __restrict__ bias_acc,
            int pack_blocks, char* __restrict__ zero_p, int64_t zero_bytes) {
    __shared__ float red[4][8];
    if ((int)blockIdx.x >= pack_blocks) {      // the blocks behind the pack's clear [zero_p, zero_p + zero_bytes): the backward's gradient buffer
        zero_fill_body(zero_p, zero_bytes, (int64_t)blockIdx.x - pack_blocks);
        return;
    }
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = 0.f;
    if (i < (int64_t)B * HW) {
        int n = (int)(i / HW);
        int64_t p = i - (int64_t)n * HW;
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = c < L ? g[((int64_t)n * L + c) * HW + p] : 0.f;
        store8<T>(G + i * 8, v);
    }
    if (bias_acc) {      // the last conv's bias gradient = sum over pixels of d(logits): summed here, from the fp32 values
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float t_ = wave_sum(v[c]);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = t_;
        }
        __syncthreads();
        if ((int)threadIdx.x < L)
            bn_acc_add(bias_acc, blockIdx.x, 1, 8, 0, 0, threadIdx.x,
                       (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]), BN_BS);
    }
}

int launch_gout_pack(int dt, const float* g, void* G, int B, int L, int H, int W, hipStream_t s, long long* bias_acc, void* zero_p,
                     int64_t zero_bytes) {
    int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
    if (!zero_p || zero_bytes <= 0) { zero_p = nullptr; zero_bytes = 0; }
    else if (!zero_fill_ok(zero_p, zero_bytes)) return 1;      // (the caller clears such a buffer with a memset of its own)
    const int64_t blocks = (n + 255) / 256 + zero_fill_blocks(zero_bytes);
    if (blocks > 0x7fffffff) return 1;
    const int pb = cdiv(n, 256), grid = (int)blocks;
    if (dt == BF16) k_gout_pack<bf16><<<grid, 256, 0, s>>>(g, (bf16*)G, B, L, HW, bias_acc, pb, (char*)zero_p, zero_bytes);
    else k_gout_pack<float><<<grid, 256, 0, s>>>(g, (float*)G, B, L, HW, bias_acc, pb, (char*)zero_p, zero_bytes);
    return 0;
}

__global__ void k_bias_finish(const BiasJob* __restrict__ jobs, const char* __restrict__ ws, float* __restrict__ grads) {
    const BiasJob& jb = jobs[blockIdx.x];
    const long long* acc = reinterpret_cast<const long long*>(ws + jb.acc_off);
    for (int c = threadIdx.x; c < jb.valid; c += blockDim.x) grads[jb.out_off + c] = (float)bn_acc_get(acc, 1, jb.C, 0, 0, c, jb.scale);
}
void launch_bias_finish(const BiasJob* jobs_dev, int njobs, const char* ws, float* grads, hipStream_t s) {
    if (njobs > 0) k_bias_finish<<<njobs, 128, 0, s>>>(jobs_dev, ws, grads);
}

// ------------------------------------------------------------------ weight pack / unpack (tiny)
__global__ void k_pack_w(PackSpec ps, const float* __restrict__ src, float* __restrict__ dst) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = (int64_t)ps.ntaps * ps.kpad * ps.wld;
    if (i >= total) return;
    int n = (int)(i % ps.wld);
    int k = (int)((i / ps.wld) % ps.kpad);
    int t = (int)(i / ((int64_t)ps.wld * ps.kpad));
    float v = 0.f;
    if (n < ps.N && k < ps.K) {
        int64_t a = ps.kn_major ? ((int64_t)k * ps.N + n) : ((int64_t)n * ps.K + k);
        v = src[(a * ps.ks + ps.ky[t]) * ps.ks + ps.kx[t]];
    }
    dst[i] = v;
}
void launch_pack_w(const PackSpec& ps, const float* src, float* dst, hipStream_t s) {
    int64_t total = (int64_t)ps.ntaps * ps.kpad * ps.wld;
    k_pack_w<<<cdiv(total, 256), 256, 0, s>>>(ps, src, dst);
}
__global__ void k_unpack_dw(PackSpec ps, const double* __restrict__ dwe, float* __restrict__ gsrc) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = (int64_t)ps.ntaps * ps.K * ps.N;
    if (i >= total) return;
    int n = (int)(i % ps.N);
    int k = (int)((i / ps.N) % ps.K);
    int t = (int)(i / ((int64_t)ps.N * ps.K));
    int64_t a = ps.kn_major ? ((int64_t)k * ps.N + n) : ((int64_t)n * ps.K + k);
    gsrc[(a * ps.ks + ps.ky[t]) * ps.ks + ps.kx[t]] = (float)dwe[((int64_t)t * ps.kpad + k) * ps.wld + n];
}
void launch_unpack_dw(const PackSpec& ps, const double* dwe, float* gsrc, hipStream_t s) {
    int64_t total = (int64_t)ps.ntaps * ps.K * ps.N;
    k_unpack_dw<<<cdiv(total, 256), 256, 0, s>>>(ps, dwe, gsrc);
}

// Block reduction of per-thread partial sums s1[V], s2[V] (V consecutive channels of channel block threadIdx.x % cb; pixel lane
// threadIdx.x / cb; 256 threads): every thread parks its partials, then 2 * CS threads each walk the 256 / cb lanes of one channel in
// lane order -- a fixed serial float sum.  Output (which, c) = block_reduce2_get(...).
// Round 4 tried a butterfly over the wave's lanes (ds_bpermute) + one LDS slot per wave instead of the serial walk (128 dependent LDS
// reads at 16 channels).  Time: neutral (small launches 10 -> 9 us; the large ones are bound by instruction issue / HBM, not by this
// epilogue).  Numerics: every variant is a valid sum, but (a) a FLOAT tree differs from the serial walk by an ulp, which the
// reference's tiny-batch fixtures (BatchNorm over 8 values, variance << mean^2) amplify to 1e-2; (b) an exact DOUBLE sum handed to the
// 2^-36 fixed-point accumulators leaves a sub-grid remainder that is not invariant under scaling the gradients by a power of two --
// through flipped bf16 roundings it grew to 1e-2 along SegCD's 50 BatchNorm layers (test_segcd_full_size_properties_bf16); (c) the
// exact sum rounded to float once restores (b) and moves the bf16 engine away from its emulating oracle on ChangeFormer's 2 x 2 maps
// (0.985 -> 0.93).  None is more right than the serial walk every bound of tests/ was measured with; it stays.
template <int V>
__device__ __forceinline__ int block_reduce2(const float (&s1)[V], const float (&s2)[V], const int cb, float* __restrict__ red) {
#pragma unroll
    for (int j = 0; j < V; ++j) { red[threadIdx.x * 2 * V + j] = s1[j]; red[threadIdx.x * 2 * V + V + j] = s2[j]; }
    return 256 / cb;
}
template <int V>
__device__ __forceinline__ float block_reduce2_get(const float* __restrict__ red, const int n, const int cb, const int which, const int c) {
    float a = 0.f;
    for (int l = 0; l < n; ++l) a += red[(l * cb + c / V) * 2 * V + which * V + (c % V)];
    return a;
}
__device__ __forceinline__ int block_reduce16(const float (&s1)[8], const float (&s2)[8], const int cb, float* __restrict__ red) {
    return block_reduce2<8>(s1, s2, cb, red);
}
__device__ __forceinline__ float block_reduce16_get(const float* __restrict__ red, const int n, const int cb, const int which, const int c) {
    return block_reduce2_get<8>(red, n, cb, which, c);
}

// ------------------------------------------------------------------ batch-norm statistics
// One block = one contiguous pixel chunk of one group.  thread -> (pixel lane, channel block of 8).
// MODE 0: sums of y and y^2.  MODE 1 (backward): sums of dz and dz*xhat with dz = dA*mask*(z>0).
// chunks per group: ~2048 16-byte pieces (8 per thread) per block, so small-spatial / wide-channel layers still
// spread over the whole chip (a 32x32x128-channel map used to get 16 blocks)
int bn_stats_chunks(int64_t ppg, int C) {
    constexpr int per = 2048;
    int64_t c = ppg * (C / 8) / per;
    if (c < 1) c = 1;
    if (c > 1024) c = 1024;
    return (int)c;
}

// NS > 0: the gradient is first GATHERED from up to NS extra views (dense-concat consumers, see SliceViews): all loads of a
// trip are issued before any arithmetic (predicated, branch-free), two pixels per trip to bound the registers.
template <typename T, int MODE, int NS = 0, bool RES = false, bool MASK = false>
__global__ void __launch_bounds__(256)
k_bn_reduce(const T* __restrict__ Y, int ldy, const T* __restrict__ dA, GV dav, const float* __restrict__ stat,
            const float* __restrict__ mask, const T* __restrict__ res, int ldres, int C, int npg, int64_t HW, int relu,
            int64_t ppg, int nchunk, long long* __restrict__ acc, const SliceViews xs, int base_valid, T* __restrict__ dA_sum,
            int nslab) {
    __shared__ float red[256 * 16];
    // block -> (channel slab, pixel chunk): wide layers give a block 64 channels (one 128-B line per pixel) of many pixels, so
    // it ends with 128 atomic adds instead of 2*C
    const int CS = C / nslab, slab = blockIdx.x % nslab, cbase = slab * CS;
    const int g = blockIdx.y, chunk = blockIdx.x / nslab;
    const int cb = CS >> 3;                  // channel blocks of the slab (power of two, <= 256)
    const int lanes = 256 / cb;
    const int mycb = threadIdx.x % cb, lane = threadIdx.x / cb;
    const int cofs = cbase + mycb * 8;       // first channel of this thread
    const int64_t per = (ppg + nchunk - 1) / nchunk;
    const int64_t p0 = (int64_t)chunk * per, p1 = min(ppg, p0 + per);
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
    float mean[8], invstd[8], scale[8], shift[8];
    if (MODE == 1) {
        const float* st = stat + (int64_t)g * 4 * C + cofs;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            mean[j] = st[j]; invstd[j] = st[C + j]; scale[j] = st[2 * C + j]; shift[j] = st[3 * C + j];
        }
    }
    const T* yb = Y + ((int64_t)g * ppg) * ldy + cofs;
    // 4 pixels per trip, every load of the trip issued before the arithmetic (a block owns only ~8 pixels per thread:
    // one load in flight at a time made the small maps pure latency)
    constexpr int U = NS > 0 ? 2 : 4;
    for (int64_t p = p0 + lane; p < p1; p += U * lanes) {
        float y[U][8], d[U][8], rs[U][8], mk[U][8];
        bool ok[U];
        float ex[U][NS > 0 ? NS : 1][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t pu = p + (int64_t)u * lanes;
            ok[u] = pu < p1;
            const int64_t pc = ok[u] ? pu : p;
            load8<T>(yb + pc * ldy, y[u]);
            if (MODE == 1) {
                if constexpr (NS == 0) load8<T>(dA + g * dav.goff + pc * dav.ld + cofs, d[u]);
                else {
                    if (base_valid) load8<T>(dA + g * dav.goff + pc * dav.ld + cofs, d[u]);
                    else {
#pragma unroll
                        for (int j = 0; j < 8; ++j) d[u][j] = 0.f;
                    }
                }
                if constexpr (NS > 0) {   // every consumer's concat-gradient slice: requested here, summed below
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        const bool on = k < xs.n && ((xs.gmask[k] >> g) & 1);
                        const int kk = on ? k : 0;                       // an inactive slot re-reads view 0 (valid address), x 0
                        load8<T>(reinterpret_cast<const T*>(xs.p[kk]) + ((xs.gmask[kk] & (xs.gmask[kk] - 1)) ? g * xs.goff[kk] : 0) + pc * xs.ld[kk] + cofs, ex[u][k]);
                    }
                }
                if constexpr (RES) load8<T>(res + ((int64_t)g * ppg + pc) * ldres + cofs, rs[u]);
                if constexpr (MASK) {
                    const int nig = (int)((uint32_t)pc / (uint32_t)HW);
                    const float4* mp = reinterpret_cast<const float4*>(mask + ((int64_t)(g * npg + nig)) * C + cofs);
                    const float4 m0 = mp[0], m1 = mp[1];
                    mk[u][0] = m0.x; mk[u][1] = m0.y; mk[u][2] = m0.z; mk[u][3] = m0.w;
                    mk[u][4] = m1.x; mk[u][5] = m1.y; mk[u][6] = m1.z; mk[u][7] = m1.w;
                }
            }
        }
        if constexpr (NS > 0) {       // fp32 sum of the gathered slices, ONE rounding, written back for the apply pass
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const bool on = k < xs.n && ((xs.gmask[k] >> g) & 1);
#pragma unroll
                    for (int j = 0; j < 8; ++j) d[u][j] += on ? ex[u][k][j] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) d[u][j] = round_as<T>(d[u][j]);
                if (ok[u]) {
                    const int64_t pu = p + (int64_t)u * lanes;
                    store8<T>(dA_sum + g * dav.goff + pu * dav.ld + cofs, d[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            if (MODE == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { s1[j] += y[u][j]; s2[j] += y[u][j] * y[u][j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float z = y[u][j] * scale[j] + shift[j];
                    if constexpr (RES) z += rs[u][j];
                    float dz = d[u][j] * (MASK ? mk[u][j] : 1.f);
                    if (relu && !(z > 0.f)) dz = 0.f;
                    s1[j] += dz;
                    s2[j] += dz * (y[u][j] - mean[j]) * invstd[j];
                }
            }
        }
    }
    const int nred = block_reduce16(s1, s2, cb, red);
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * CS; o += 256) {
        int which = o / CS, c = o - which * CS;
        const float a_ = block_reduce16_get(red, nred, cb, which, c);
        bn_acc_add(acc, chunk, gridDim.y, C, g, which, cbase + c, a_, MODE == 0 ? (which ? BN_FS2 : BN_FS1) : BN_BS);
    }
}

void launch_bn_stats(int dt, const void* Y, int ld, int C, int groups, int64_t ppg, long long* acc, hipStream_t s) {
    const int nslab = bn_slabs(C);
    int nchunk = bn_stats_chunks(ppg, C / nslab);
    dim3 grid(nchunk * nslab, groups);
    GV z{0, 0};
    if (dt == BF16)
        k_bn_reduce<bf16, 0><<<grid, 256, 0, s>>>((const bf16*)Y, ld, nullptr, z, nullptr, nullptr, nullptr, 0, C, 0, 1, 0, ppg, nchunk, acc, SliceViews(), 1, nullptr, nslab);
    else
        k_bn_reduce<float, 0><<<grid, 256, 0, s>>>((const float*)Y, ld, nullptr, z, nullptr, nullptr, nullptr, 0, C, 0, 1, 0, ppg, nchunk, acc, SliceViews(), 1, nullptr, nslab);
}


// (bn_fwd_table: common.h -- the convolution kernels that apply a BatchNorm while staging their input use it too)
// tab: [groups][5][C] = (scale, shift, b, mean, c) of dY = scale*dz + b*(y - mean) + c  (see k_bn_bwd_apply)
__device__ __forceinline__ void bn_bwd_table(float* tab, const long long* __restrict__ bacc, const float* __restrict__ stat,
                                             float* __restrict__ dgamma, float* __restrict__ dbeta, int C, int groups, int64_t ppg,
                                             bool publish, int cbase = 0, int CS = 0, float* __restrict__ dbeta_copy = nullptr) {
    if (CS == 0) CS = C;                         // channel slab [cbase, cbase + CS), see bn_fwd_table
    const double inv_n = 1.0 / (double)ppg;
    for (int cl = threadIdx.x; cl < CS; cl += blockDim.x) {
        const int c = cbase + cl;
        double tg = 0.0, tb = 0.0;
        for (int g = 0; g < groups; ++g) {
            const double s1 = bn_acc_get(bacc, groups, C, g, 0, c, BN_BS), s2 = bn_acc_get(bacc, groups, C, g, 1, c, BN_BS);
            const float* st = stat + (int64_t)g * 4 * C;
            const double mean = st[c], invstd = st[C + c], scale = st[2 * C + c];
            const double k1 = s1 * inv_n, k2 = s2 * inv_n;
            float* bw = tab + (int64_t)g * 5 * CS;
            bw[cl] = (float)scale;
            bw[CS + cl] = st[3 * C + c];
            bw[2 * CS + cl] = (float)(-scale * k2 * invstd);
            bw[3 * CS + cl] = (float)mean;
            bw[4 * CS + cl] = (float)(-scale * k1);
            tb += s1; tg += s2;
        }
        if (publish && dgamma) { dgamma[c] = (float)tg; dbeta[c] = (float)tb; if (dbeta_copy) dbeta_copy[c] = (float)tb; }
    }
}

__global__ void k_bn_eval_prepare(int C, int groups, const float* __restrict__ gamma, const float* __restrict__ beta,
                                  const float* __restrict__ rmean, const float* __restrict__ rvar, float* __restrict__ stat,
                                  float eps) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float invstd = 1.f / sqrtf(rvar[c] + eps);
    for (int g = 0; g < groups; ++g) {
        float* st = stat + (int64_t)g * 4 * C;
        st[c] = rmean[c];
        st[C + c] = invstd;
        st[2 * C + c] = gamma[c] * invstd;
        st[3 * C + c] = beta[c] - rmean[c] * gamma[c] * invstd;
    }
}
void launch_bn_eval_prepare(int C, int groups, const float* gamma, const float* beta, const float* rmean,
                            const float* rvar, float* stat, float eps, hipStream_t s) {
    k_bn_eval_prepare<<<cdiv(C, 64), 64, 0, s>>>(C, groups, gamma, beta, rmean, rvar, stat, eps);
}

// ------------------------------------------------------------------ BN-apply + ReLU + Dropout2d (+ 2x2 max-pool)
// thread -> (2x2 cell, channel block).  One pass: reads the raw conv output once, writes the activation once
// and, when a pool follows, the pooled map too (saves re-reading the full-resolution tensor).
// RES (and OPT / RES of the two backward kernels): whether the optional residual / extra tensor exists is a TEMPLATE parameter --
// as a run-time `if (res) load` every such load sat in its own block behind an s_waitcnt vmcnt(0), so the 4 pixels of a thread
// were fetched one round trip after the other instead of as one batch.
template <typename T, bool RES, bool MASK>
__global__ void __launch_bounds__(256)
k_bn_act(const T* __restrict__ Y, int ldy, T* __restrict__ A, GV av, T* __restrict__ P, int ldp,
         float* __restrict__ stat, const float* __restrict__ mask, const T* __restrict__ res, int ldres, int C, int npg,
         int H, int W, int relu, int64_t total, const long long* __restrict__ facc, const float* __restrict__ gamma,
         const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar, int groups, float momentum, float eps,
         const SliceViews xd, int nslab, int g_first) {
    extern __shared__ float bn_tab[];           // [groups][2][CS]
    // block -> (channel slab, block inside the slab): the slab's blocks walk its (quad, 8-channel chunk) items grid-stride
    const int CS = C / nslab, slab = blockIdx.x % nslab, bi = blockIdx.x / nslab, bps = gridDim.x / nslab, cbase = slab * CS;
    bn_fwd_table(bn_tab, facc, gamma, beta, rmean, rvar, stat, C, groups, (int64_t)npg * H * W, momentum, eps, bi == 0, cbase, CS, g_first);
    __syncthreads();
    const int64_t total_s = total / nslab;
    for (int64_t i64 = (int64_t)bi * blockDim.x + threadIdx.x; i64 < total_s; i64 += (int64_t)bps * blockDim.x) {
    const int cb = CS >> 3, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1, Hp = H >> 1, Wp = W >> 1;
    // 32-bit index arithmetic (the launcher guarantees total < 2^31)
    uint32_t r = (uint32_t)i64;
    const int c0l = (int)(r % (uint32_t)cb) * 8, c0 = cbase + c0l; r /= (uint32_t)cb;
    const int xc = (int)(r % (uint32_t)Wc); r /= (uint32_t)Wc;
    const int yc = (int)(r % (uint32_t)Hc);
    const int n = (int)(r / (uint32_t)Hc);
    const int g = n / npg, nig = n - g * npg;
    float sc[8], sh[8], mk[8];
    {
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = bn_tab[(g * 2 + 0) * CS + c0l + j]; sh[j] = bn_tab[(g * 2 + 1) * CS + c0l + j]; }
        if constexpr (MASK) {
            // the Dropout2d factor (0 or 1 / (1 - p), never negative) is folded into scale / shift: relu(z) * mk == relu(y * (sc * mk) +
            // sh * mk) -- the same arithmetic as the staging transform of a virtual activation (common.h xf_fold8 / xf_act8), so a layer
            // gives the same bits whether its activation is materialised here or formed in its consumer's loader.  (With a residual the
            // ReLU sees z + res: those layers -- SNUNet's -- have no mask.)
            const float4* mp = reinterpret_cast<const float4*>(mask + (int64_t)n * C + c0);
            const float4 m0 = mp[0], m1 = mp[1];
            mk[0] = m0.x; mk[1] = m0.y; mk[2] = m0.z; mk[3] = m0.w; mk[4] = m1.x; mk[5] = m1.y; mk[6] = m1.z; mk[7] = m1.w;
#pragma unroll
            for (int j = 0; j < 8; ++j) { sc[j] *= mk[j]; sh[j] *= mk[j]; }
        }
    }
    // the 2x2 quad: all loads first (clamped inside the map), then the arithmetic and the stores
    float v[4][8], rs[4][8];
    bool ok[4];
    int64_t pix[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = 2 * yc + (k >> 1), x = 2 * xc + (k & 1);
        ok[k] = y < H && x < W;
        pix[k] = ((int64_t)n * H + (ok[k] ? y : 2 * yc)) * W + (ok[k] ? x : 2 * xc);
        load8<T>(Y + pix[k] * ldy + c0, v[k]);
        if constexpr (RES) load8<T>(res + pix[k] * ldres + c0, rs[k]);
    }
    float best[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float z = fmaf(v[k][j], sc[j], sh[j]);
            if constexpr (RES) z += MASK ? rs[k][j] * mk[j] : rs[k][j];    // residual add before the ReLU (SNUNet conv_block_nested, SNUNet.py:25)
            if (relu) z = z > 0.f ? z : 0.f;     // (+0 for -0 and NaN, as the packed-bf16 ReLU of xf_act8)
            v[k][j] = round_as<T>(z);
            best[j] = k == 0 ? v[k][j] : fmaxf(best[j], v[k][j]);   // pooled cells are complete quads: every k is inside
        }
        if (ok[k]) {
            const int y = 2 * yc + (k >> 1), x = 2 * xc + (k & 1);
            const int64_t pg = ((int64_t)nig * H + y) * W + x;
            store8<T>(A + g * av.goff + pg * av.ld + c0, v[k]);
            for (int e = 0; e < xd.n; ++e)      // dense concatenation: the consumers' input slices, written here (no copy kernels)
                if ((xd.gmask[e] >> g) & 1)
                    store8<T>(reinterpret_cast<T*>(xd.p[e]) + ((xd.gmask[e] & (xd.gmask[e] - 1)) ? g * xd.goff[e] : 0) + pg * xd.ld[e] + c0, v[k]);
        }
    }
    if (P && yc < Hp && xc < Wp) store8<T>(P + (((int64_t)n * Hp + yc) * Wp + xc) * ldp + c0, best);
    }
}

// Skip layers (last conv of an encoder level): both dates of a pair in one thread, so the bi-temporal skip fusion
// F = |a1 - a2| (mode 0) or a2 - a1 (mode 1) is written in the same pass -- the separate fusion kernel would re-read
// both activations.  Same arithmetic as k_bn_act per date (affine, ReLU, Dropout2d mask, rounding, 2x2 max-pool).
// STORE_A = false: the activations themselves are not written -- nothing but the backward of this very layer would read them,
// and k_skip_bwd_pair recomputes them from Y with the same arithmetic (one tensor pass less here, one less there).
template <typename T, bool MASK, bool STORE_A>
__global__ void __launch_bounds__(256)
k_bn_act_pair(const T* __restrict__ Y, int ldy, T* __restrict__ A, GV av, T* __restrict__ P, int ldp, T* __restrict__ F, int ldf,
              int fmode, float* __restrict__ stat, const float* __restrict__ mask, int C, int npg, int H, int W, int64_t total,
              const long long* __restrict__ facc, const float* __restrict__ gamma, const float* __restrict__ beta,
              float* __restrict__ rmean, float* __restrict__ rvar, float momentum, float eps) {
    extern __shared__ float bn_tab[];           // [2][2][C]
    const int cb = C >> 3, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1, Hp = H >> 1, Wp = W >> 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    Raw8<T> rv[2][4];                            // both dates' quad, requested before the table is built (see k_bn_act)
    auto fetch = [&](int64_t i64) {
        uint32_t r = (uint32_t)i64;
        const int c0 = (int)(r % (uint32_t)cb) * 8; r /= (uint32_t)cb;
        const int xc = (int)(r % (uint32_t)Wc); r /= (uint32_t)Wc;
        const int yc = (int)(r % (uint32_t)Hc);
        const int nb = (int)(r / (uint32_t)Hc);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = 2 * yc + (k >> 1), x = 2 * xc + (k & 1);
            const bool ok = y < H && x < W;
            const int64_t pix = ((int64_t)nb * H + (ok ? y : 2 * yc)) * W + (ok ? x : 2 * xc);
#pragma unroll
            for (int g = 0; g < 2; ++g) rv[g][k].ld(Y + ((int64_t)g * npg * H * W + pix) * ldy + c0);
        }
    };
    int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 < total) fetch(i64);
    bn_fwd_table(bn_tab, facc, gamma, beta, rmean, rvar, stat, C, 2, (int64_t)npg * H * W, momentum, eps, blockIdx.x == 0);
    __syncthreads();
    while (i64 < total) {
        uint32_t r = (uint32_t)i64;
        const int c0 = (int)(r % (uint32_t)cb) * 8; r /= (uint32_t)cb;
        const int xc = (int)(r % (uint32_t)Wc); r /= (uint32_t)Wc;
        const int yc = (int)(r % (uint32_t)Hc);
        const int nb = (int)(r / (uint32_t)Hc);
        bool ok[4];
        int64_t pix[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = 2 * yc + (k >> 1), x = 2 * xc + (k & 1);
            ok[k] = y < H && x < W;
            pix[k] = ((int64_t)nb * H + (ok[k] ? y : 2 * yc)) * W + (ok[k] ? x : 2 * xc);
        }
        float vv[2][4][8];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k) rv[g][k].get(vv[g][k]);
        const int64_t nxt = i64 + stride;
        if (nxt < total) fetch(nxt);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float sc[8], sh[8], mk[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { sc[j] = bn_tab[(g * 2 + 0) * C + c0 + j]; sh[j] = bn_tab[(g * 2 + 1) * C + c0 + j]; }
            if constexpr (MASK) {                 // folded Dropout2d factor, as k_bn_act
                ld8f(mask + ((int64_t)g * npg + nb) * C + c0, mk);
#pragma unroll
                for (int j = 0; j < 8; ++j) { sc[j] *= mk[j]; sh[j] *= mk[j]; }
            }
            float best[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float z = fmaf(vv[g][k][j], sc[j], sh[j]);
                    z = z > 0.f ? z : 0.f;
                    vv[g][k][j] = round_as<T>(z);
                    best[j] = k == 0 ? vv[g][k][j] : fmaxf(best[j], vv[g][k][j]);
                }
                if (STORE_A && ok[k]) store8<T>(A + g * av.goff + pix[k] * av.ld + c0, vv[g][k]);
                if (g == 1 && ok[k]) {
                    float f[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) f[j] = fmode == 0 ? fabsf(vv[0][k][j] - vv[1][k][j]) : vv[1][k][j] - vv[0][k][j];
                    store8<T>(F + pix[k] * ldf + c0, f);
                }
            }
            if (P && yc < Hp && xc < Wp) store8<T>(P + ((((int64_t)g * npg + nb) * Hp + yc) * Wp + xc) * ldp + c0, best);
        }
        i64 = nxt;
    }
}
void launch_bn_act_pair(int dt, const BnActArgs& a, void* F, int ldf, int fmode, hipStream_t s) {
    const int64_t total = (int64_t)a.npg * ((a.H + 1) / 2) * ((a.W + 1) / 2) * (a.C / 8);
    GV av{a.lda, a.a_group_off};
    const size_t lds = (size_t)2 * 2 * a.C * 4;
    const int grid = ew_grid(total);
#define ACT_PAIR(T_, M_) do { if (a.A) ACT_PAIR_K(T_, M_, true); else ACT_PAIR_K(T_, M_, false); } while (0)
#define ACT_PAIR_K(T_, M_, SA_) k_bn_act_pair<T_, M_, SA_><<<grid, 256, lds, s>>>((const T_*)a.Y, a.ldy, (T_*)a.A, av, (T_*)a.P, a.ldp, (T_*)F, ldf, fmode, a.stat, a.mask, a.C, a.npg, a.H, a.W, total, a.facc, a.gamma, a.beta, a.running_mean, a.running_var, a.momentum, a.eps)
    if (dt == BF16) { if (a.mask) ACT_PAIR(bf16, true); else ACT_PAIR(bf16, false); }
    else { if (a.mask) ACT_PAIR(float, true); else ACT_PAIR(float, false); }
#undef ACT_PAIR
#undef ACT_PAIR_K
}

void launch_bn_act(int dt, const BnActArgs& a, hipStream_t s) {
    int64_t total = (int64_t)a.groups * a.npg * ((a.H + 1) / 2) * ((a.W + 1) / 2) * (a.C / 8);
    GV av{a.lda, a.a_group_off};
    const int nslab = bn_slabs(a.C);
    const size_t lds = (size_t)a.groups * 2 * (a.C / nslab) * 4;
    const int grid = std::max(1, ew_grid(total) / nslab) * nslab;
#define BN_ACT(T_, R_) do { if (a.mask) BN_ACT_M(T_, R_, true); else BN_ACT_M(T_, R_, false); } while (0)
#define BN_ACT_M(T_, R_, M_) k_bn_act<T_, R_, M_><<<grid, 256, lds, s>>>((const T_*)a.Y, a.ldy, (T_*)a.A, av, (T_*)a.P, a.ldp, a.stat, a.mask, (const T_*)a.res, a.ldres, a.C, a.npg, a.H, a.W, a.relu, total, a.facc, a.gamma, a.beta, a.running_mean, a.running_var, a.groups, a.momentum, a.eps, a.extra, nslab, a.g_first)
    if (dt == BF16) { if (a.res) BN_ACT(bf16, true); else BN_ACT(bf16, false); }
    else { if (a.res) BN_ACT(float, true); else BN_ACT(float, false); }
#undef BN_ACT
#undef BN_ACT_M
}

template <typename T>
__global__ void k_maxpool(const T* __restrict__ A, int lda, T* __restrict__ P, int ldp, int H, int W, int C, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3, Hp = H >> 1, Wp = W >> 1;
    int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    int xp = (int)(r % Wp); r /= Wp;
    int yp = (int)(r % Hp);
    int n = (int)(r / Hp);
    float best[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v[8];
        load8<T>(A + (((int64_t)n * H + 2 * yp + (k >> 1)) * W + 2 * xp + (k & 1)) * lda + c0, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = k == 0 ? v[j] : fmaxf(best[j], v[j]);
    }
    store8<T>(P + (((int64_t)n * Hp + yp) * Wp + xp) * ldp + c0, best);
}
void launch_maxpool(int dt, const void* A, int lda, void* P, int ldp, int N, int H, int W, int C, hipStream_t s) {
    int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
    if (total == 0) return;
    if (dt == BF16) k_maxpool<bf16><<<cdiv(total, 256), 256, 0, s>>>((const bf16*)A, lda, (bf16*)P, ldp, H, W, C, total);
    else k_maxpool<float><<<cdiv(total, 256), 256, 0, s>>>((const float*)A, lda, (float*)P, ldp, H, W, C, total);
}

// dA (+)= dP routed to the FIRST maximum (scan order (0,0),(0,1),(1,0),(1,1)) of each window of A
template <typename T>
__global__ void k_pool_bwd(const T* __restrict__ A, GV av, const T* __restrict__ dP, int ldp, T* __restrict__ dA, GV dav,
                           int npg, int H, int W, int C, int accumulate, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1, Hp = H >> 1, Wp = W >> 1;
    int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    int xc = (int)(r % Wc); r /= Wc;
    int yc = (int)(r % Hc);
    int n = (int)(r / Hc);
    int g = n / npg, nig = n - g * npg;
    bool pooled = yc < Hp && xc < Wp;
    float a[4][8], gp[8];
    int arg[8];
    if (pooled) {
        load8<T>(dP + (((int64_t)n * Hp + yc) * Wp + xc) * ldp + c0, gp);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            load8<T>(A + g * av.goff + (((int64_t)nig * H + 2 * yc + (k >> 1)) * W + 2 * xc + (k & 1)) * av.ld + c0, a[k]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int b = 0;
            float bv = a[0][j];
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (a[k][j] > bv) { bv = a[k][j]; b = k; }
            arg[j] = b;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int y = 2 * yc + (k >> 1), x = 2 * xc + (k & 1);
        if (y >= H || x >= W) continue;
        T* dst = dA + g * dav.goff + (((int64_t)nig * H + y) * W + x) * dav.ld + c0;
        float v[8];
        if (accumulate) load8<T>(dst, v);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
        }
        if (pooled) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (arg[j] == k) v[j] += gp[j];
        }
        store8<T>(dst, v);
    }
}

// ------------------------------------------------------------------ skip fusion
template <typename T>
__global__ void k_fuse(int mode, const T* __restrict__ A, GV av, T* __restrict__ D, int ldd, int64_t HW, int C, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3;
    int c0 = (int)(i % cb) * 8;
    int64_t p = i / cb;   // n*HW + pix over the B pairs
    float a[8], b[8], o[8];
    load8<T>(A + p * av.ld + c0, a);
    load8<T>(A + av.goff + p * av.ld + c0, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = mode == 0 ? fabsf(a[j] - b[j]) : b[j] - a[j];
    store8<T>(D + p * ldd + c0, o);
}
template <typename T>
__global__ void k_fuse_bwd(int mode, const T* __restrict__ A, GV av, const T* __restrict__ dD, int ldd, T* __restrict__ dA,
                           GV dav, int64_t HW, int C, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3;
    int c0 = (int)(i % cb) * 8;
    int64_t p = i / cb;
    float a[8], b[8], g[8], da[8], db[8];
    load8<T>(dD + p * ldd + c0, g);
    if (mode == 0) {
        load8<T>(A + p * av.ld + c0, a);
        load8<T>(A + av.goff + p * av.ld + c0, b);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float sgn = mode == 0 ? (float)((a[j] > b[j]) - (a[j] < b[j])) : -1.f;
        da[j] = sgn * g[j];
        db[j] = -sgn * g[j];
    }
    store8<T>(dA + p * dav.ld + c0, da);
    store8<T>(dA + dav.goff + p * dav.ld + c0, db);
}


// ------------------------------------------------------------------ backward of an encoder skip layer, one pass
// The last conv of an encoder level feeds the 2x2 max-pool AND the bi-temporal skip.  Its dA is the sum of the pool
// gradient (routed to the first maximum of each window, as k_pool_bwd) and the skip-fusion gradient (sign(a1-a2)*g for
// |a1-a2|, -/+g for a2-a1, as k_fuse_bwd); the BatchNorm backward then needs sum(dz) and sum(dz*xhat) of it.  Doing the
// three in one pass saves three tensor round trips per level.  grid = (chunks, 2 dates); thread = one 2x2 quad x 8
// channels of one image; partial rows as k_bn_reduce<T,1> writes them (chunks = gridDim.x rows per date).
template <typename T, bool MASK, int MODE>
__global__ void __launch_bounds__(256)
k_skip_bwd(int mode, const T* __restrict__ A, GV av, const T* __restrict__ Y, int ldy, const T* __restrict__ dD, int ldd,
           const T* __restrict__ dP, int ldp, T* __restrict__ dA, GV dav, const float* __restrict__ stat,
           const float* __restrict__ mask, int B, int H, int W, int C, int64_t total, long long* __restrict__ bacc) {
    __shared__ float red[256 * 16];
    const int g = blockIdx.y;
    const int cb = C >> 3, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1, Hp = H >> 1, Wp = W >> 1;
    const int lanes = 256 / cb, mycb = threadIdx.x % cb, lane = threadIdx.x / cb;
    const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
    if (i64 < total) {
        uint32_t r = (uint32_t)i64;
        const int c0 = (int)(r % (uint32_t)cb) * 8; r /= (uint32_t)cb;
        const int xc = (int)(r % (uint32_t)Wc); r /= (uint32_t)Wc;
        const int yc = (int)(r % (uint32_t)Hc);
        const int nb = (int)(r / (uint32_t)Hc);             // image inside the date
        const bool pooled = yc < Hp && xc < Wp;
        float mean[8], invstd[8], scale[8], shift[8], mk[8];
        const float* st = stat + (int64_t)g * 4 * C + c0;
        ld8f(st, mean); ld8f(st + C, invstd); ld8f(st + 2 * C, scale); ld8f(st + 3 * C, shift);
        if constexpr (MASK) ld8f(mask + ((int64_t)g * B + nb) * C + c0, mk);
        // this date's and the other date's activations of the quad (clamped inside the map), pooled gradient
        float as[4][8], ao[4][8], gp[8];
        bool ok[4];
        int64_t pix[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = 2 * yc + (k >> 1), x = 2 * xc + (k & 1);
            ok[k] = y < H && x < W;
            pix[k] = ((int64_t)nb * H + (ok[k] ? y : 2 * yc)) * W + (ok[k] ? x : 2 * xc);
            load8<T>(A + g * av.goff + pix[k] * av.ld + c0, as[k]);
            if constexpr (MODE == 0) load8<T>(A + (1 - g) * av.goff + pix[k] * av.ld + c0, ao[k]);
        }
        // branch-free: an un-pooled border cell re-reads cell (0, 0) of its image and ignores it (arg = -1 below)
        load8<T>(dP + ((((int64_t)g * B + nb) * Hp + (pooled ? yc : 0)) * Wp + (pooled ? xc : 0)) * ldp + c0, gp);
        // the second phase's inputs are requested here as well, before the arg-max arithmetic waits for the first phase
        float gk4[4][8], y4[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            load8<T>(dD + pix[k] * ldd + c0, gk4[k]);
            load8<T>(Y + ((int64_t)g * B * H * W + pix[k]) * ldy + c0, y4[k]);
        }
        int arg[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int b = 0;
            float bvv = as[0][j];
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (as[k][j] > bvv) { bvv = as[k][j]; b = k; }
            arg[j] = pooled ? b : -1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v[8];
            const float (&gk)[8] = gk4[k];
            const float (&y)[8] = y4[k];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // date 0 receives +sign(a0-a1)*g, date 1 the negative; "sub" (f2 - f1): date 0 gets -g, date 1 +g
                float sgn;
                if constexpr (MODE == 0) { const float d = g == 0 ? as[k][j] - ao[k][j] : ao[k][j] - as[k][j]; sgn = (float)((d > 0.f) - (d < 0.f)); }
                else sgn = -1.f;
                if (g == 1) sgn = -sgn;
                float da = sgn * gk[j];
                if (arg[j] == k) da += gp[j];
                da = round_as<T>(da);
                v[j] = da;
                const float z = fmaf(y[j], scale[j], shift[j]);    // (explicit contraction: k_skip_bwd_pair must give the same bits)
                float dz = MASK ? da * mk[j] : da;
                if (!(z > 0.f)) dz = 0.f;
                if (ok[k]) { s1[j] += dz; s2[j] = fmaf(__fmul_rn(dz, y[j] - mean[j]), invstd[j], s2[j]); }
            }
            if (ok[k]) store8<T>(dA + g * dav.goff + pix[k] * dav.ld + c0, v);
        }
    }
    const int nred = block_reduce16(s1, s2, cb, red);
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * C; o += 256) {
        const int which = o / C, c = o - which * C;
        const float a_ = block_reduce16_get(red, nred, cb, which, c);
        bn_acc_add(bacc, blockIdx.x, 2, C, g, which, c, a_, BN_BS);
    }
}

// The same backward with BOTH dates of a pair in one thread and the activations RECOMPUTED from Y (k_bn_act_pair<STORE_A =
// false> did not write them): a = round(max(fma(y, scale * mk, shift * mk), 0)) is the forward's arithmetic on the forward's
// published scale / shift, so the arg-max and the sign of a1 - a2 are the ones the stored activations would give.  Per pair the
// pass reads Y (2 dates), dD, dP and writes dA (2 dates): 5.5 date-tensors, against 10.5 of the per-date kernel above (each
// date read both dates' A, its Y, the shared dD).
// These kernels are INSTRUCTION-bound, not HBM-bound (the per-date kernel: 1950 instructions per thread = 61 per element, 52 us
// of pure VALU issue at 524288 x 2 threads against 91 us measured and ~45 us of HBM time), so this one is written for the
// instruction count: grid = (x chunks, row pairs, pairs) -- no integer division; EVEN sizes take a path without border
// predicates; the skip gradient sign(a0 - a1) * g is formed ONCE per pair element (date 1 uses its negative); a running
// arg-max instead of a second walk.  Partial sums: the same per-thread values as the per-date kernel and an exact (double)
// block sum, so both plans give the same BatchNorm sums.  thread = one 2x2 quad x 8 channels of a PAIR.
template <typename T, bool MASK, int MODE, bool EVEN, int V>
__global__ void __launch_bounds__(256, (V == 4 && sizeof(T) == 2) ? 4 : 1)
k_skip_bwd_pair(const T* __restrict__ Y, int ldy, const T* __restrict__ dD, int ldd, const T* __restrict__ dP, int ldp,
                T* __restrict__ dA, GV dav, const float* __restrict__ stat, const float* __restrict__ mask, int B, int H, int W,
                int C, int lcb, long long* __restrict__ bacc) {
    __shared__ float red[256 * 16];
    const int cb = 1 << lcb, Wc = (W + 1) >> 1, Hp = H >> 1, Wp = W >> 1;
    const int yc = blockIdx.y, nb = blockIdx.z;
    const int tx = blockIdx.x * 256 + threadIdx.x;
    const int xc = tx >> lcb, c0 = (tx & (cb - 1)) * V;
    float s1[2][V], s2[2][V];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int j = 0; j < V; ++j) s1[g][j] = s2[g][j] = 0.f;
    if (xc < Wc) {
        const bool pooled = EVEN || (yc < Hp && xc < Wp);
        bool ok[4];
        uint32_t pix[4];
        RawV<T, V> ry[2][4], rg[4], rp[2];
        const uint32_t gstride = (uint32_t)B * H * W;        // pixels per date (the launcher checks 2 * B * H * W < 2^31)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = 2 * yc + (k >> 1), x = 2 * xc + (k & 1);
            ok[k] = EVEN || (y < H && x < W);
            pix[k] = ((uint32_t)nb * H + (ok[k] ? y : 2 * yc)) * W + (ok[k] ? x : 2 * xc);
#pragma unroll
            for (int g = 0; g < 2; ++g) ry[g][k].ld(Y + (uint64_t)(g * gstride + pix[k]) * ldy + c0);
            rg[k].ld(dD + (uint64_t)pix[k] * ldd + c0);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g)     // an un-pooled border cell re-reads cell (0, 0) of its image and ignores it
            rp[g].ld(dP + (uint64_t)((((uint32_t)g * B + nb) * Hp + (pooled ? yc : 0)) * Wp + (pooled ? xc : 0)) * ldp + c0);
        // ---- phase A: the forward's activations of both dates, pixel by pixel -> skip gradient t, running arg-max
        float t[4][V], best[2][V];
        int bk[2][V];
        {
            float sc[2][V], sh[2][V];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const float* st = stat + (g * 4 + 2) * C + c0;
                ldVf<V>(st, sc[g]); ldVf<V>(st + C, sh[g]);
                if constexpr (MASK) {
                    float mk[V];
                    ldVf<V>(mask + ((int64_t)g * B + nb) * C + c0, mk);
#pragma unroll
                    for (int j = 0; j < V; ++j) { sc[g][j] *= mk[j]; sh[g][j] *= mk[j]; }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float a[2][V], gk[V];
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    float y[V];
                    ry[g][k].get(y);
#pragma unroll
                    for (int j = 0; j < V; ++j) a[g][j] = round_as<T>(fmaxf(fmaf(y[j], sc[g][j], sh[g][j]), 0.f));
                }
                rg[k].get(gk);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    // date 0 receives +sign(a0 - a1) * g, date 1 the negative; "sub" (f2 - f1): date 0 gets -g, date 1 +g
                    if constexpr (MODE == 0) {
                        const float d = a[0][j] - a[1][j];          // branch-free: g with d's sign bit flipped in, 0 where d == 0
                        const float sg = __uint_as_float(__float_as_uint(gk[j]) ^ (__float_as_uint(d) & 0x80000000u));
                        t[k][j] = d == 0.f ? 0.f : sg;
                    } else t[k][j] = -gk[j];
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        if (k == 0) { best[g][j] = a[g][j]; bk[g][j] = 0; }
                        else if (a[g][j] > best[g][j]) { best[g][j] = a[g][j]; bk[g][j] = k; }     // first maximum wins
                    }
                }
            }
        }
        // ---- phase B: per date, dA = skip gradient + pool gradient; BatchNorm backward partial sums of it
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            __builtin_amdgcn_sched_barrier(0);      // keep each date's table loads behind the previous phase (register budget)
            float mean[V], invstd[V], scale[V], shift[V], mk[V], gp[V];
            const float* st = stat + (int64_t)g * 4 * C + c0;
            ldVf<V>(st, mean); ldVf<V>(st + C, invstd); ldVf<V>(st + 2 * C, scale); ldVf<V>(st + 3 * C, shift);
            if constexpr (MASK) ldVf<V>(mask + ((int64_t)g * B + nb) * C + c0, mk);
            rp[g].get(gp);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float v[V], y[V];
                ry[g][k].opaque();
                ry[g][k].get(y);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    float da = g ? -t[k][j] : t[k][j];
                    if (pooled && bk[g][j] == k) da += gp[j];
                    da = round_as<T>(da);
                    v[j] = da;
                    const float z = fmaf(y[j], scale[j], shift[j]);
                    float dz = MASK ? da * mk[j] : da;
                    if (!(z > 0.f) || !ok[k]) dz = 0.f;
                    s1[g][j] += dz;
                    s2[g][j] = fmaf(__fmul_rn(dz, y[j] - mean[j]), invstd[j], s2[g][j]);
                }
                if (ok[k]) storeV<T, V>(dA + g * dav.goff + (uint64_t)pix[k] * dav.ld + c0, v);
            }
        }
    }
    const int rep = blockIdx.x + blockIdx.y + blockIdx.z * 5;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (g) __syncthreads();
        const int nred = block_reduce2<V>(s1[g], s2[g], cb, red);
        __syncthreads();
        for (int o = threadIdx.x; o < 2 * C; o += 256) {
            const int which = o / C, c = o - which * C;
            const float a_ = block_reduce2_get<V>(red, nred, cb, which, c);
            bn_acc_add(bacc, rep, 2, C, g, which, c, a_, BN_BS);
        }
    }
}

// ------------------------------------------------------------------ replication pad of trailing rows / cols
template <typename T>
__global__ void k_rep_pad(T* __restrict__ D, int ld, int H, int W, int h0, int w0, int C, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3;
    int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    int x = (int)(r % W); r /= W;
    int y = (int)(r % H);
    int n = (int)(r / H);
    if (y < h0 && x < w0) return;
    int ys = min(y, h0 - 1), xs = min(x, w0 - 1);
    float v[8];
    load8<T>(D + (((int64_t)n * H + ys) * W + xs) * ld + c0, v);
    store8<T>(D + (((int64_t)n * H + y) * W + x) * ld + c0, v);
}
// backward: edge pixel (h0-1 / w0-1) accumulates the gradients of its replicas; thread per interior edge pixel
template <typename T>
__global__ void k_rep_pad_bwd(T* __restrict__ dD, int ld, int H, int W, int h0, int w0, int C, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3;
    int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    int x = (int)(r % w0); r /= w0;
    int y = (int)(r % h0);
    int n = (int)(r / h0);
    bool ey = (y == h0 - 1) && H > h0, ex = (x == w0 - 1) && W > w0;
    if (!ey && !ex) return;
    float acc[8], v[8];
    load8<T>(dD + (((int64_t)n * H + y) * W + x) * ld + c0, acc);
    for (int yy = y; yy < (ey ? H : y + 1); ++yy)
        for (int xx = x; xx < (ex ? W : x + 1); ++xx) {
            if (yy == y && xx == x) continue;
            load8<T>(dD + (((int64_t)n * H + yy) * W + xx) * ld + c0, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += v[j];
        }
    store8<T>(dD + (((int64_t)n * H + y) * W + x) * ld + c0, acc);
}

// ------------------------------------------------------------------ BN backward: apply
// dY = scale*(dz - k1 - xhat*k2) = scale*dz + b*(y - mean) + c with per-(group,channel) constants prepared by
// k_bn_bwd_finalize: bw[g][0..4][C] = (scale, shift, b = -scale*k2*invstd, mean, c = -scale*k1).
// (y - mean) is formed explicitly: folding mean into c cancels catastrophically in fp32.
// thread -> (4 consecutive pixels, 8 channels): the 4x8 constants are loaded once as float4s.
template <typename T, int PX, int OPT, bool MASK>       // OPT: 0 plain, 1 a residual (res), 2 an extra gradient term (extra); MASK: Dropout2d mask
__global__ void __launch_bounds__(256)
k_bn_bwd_apply(const T* __restrict__ dA, GV dav, T* __restrict__ dY, int lddy, const T* __restrict__ Y, int ldy,
               const float* __restrict__ stat, const long long* __restrict__ bacc, float* __restrict__ dgamma, float* __restrict__ dbeta,
               int groups, const float* __restrict__ mask, const T* __restrict__ res, int ldres,
               T* __restrict__ dZout, int lddz, const T* __restrict__ extra, int ldex, int C, int npg, int64_t HW, int relu,
               int64_t total, int nslab, float* __restrict__ dbeta_copy) {
    extern __shared__ float bw_tab[];           // [groups][5][CS]
    const int CS = C / nslab, slab = blockIdx.x % nslab, bi = blockIdx.x / nslab, bps = gridDim.x / nslab, cbase = slab * CS;
    bn_bwd_table(bw_tab, bacc, stat, dgamma, dbeta, C, groups, (int64_t)npg * HW, bi == 0, cbase, CS, dbeta_copy);
    __syncthreads();
    const int64_t total_s = total / nslab;
    for (int64_t i = (int64_t)bi * blockDim.x + threadIdx.x; i < total_s; i += (int64_t)bps * blockDim.x) {
    const int cb = CS >> 3;
    const uint32_t iu = (uint32_t)i;               // launcher guarantees total < 2^31
    const int c0l = (int)(iu % (uint32_t)cb) * 8, c0 = cbase + c0l;
    const int64_t p0 = (int64_t)(iu / (uint32_t)cb) * PX;  // first of PX pixels (PX > 1 only when HW % PX == 0: same image)
    const int n = (int)((uint32_t)p0 / (uint32_t)HW);
    const int g = n / npg;
    const int64_t pig0 = p0 - (int64_t)g * npg * HW;
    float sc[8], sh[8], kb[8], mu[8], kc[8], mk[8];
    const float* w = bw_tab + (int64_t)g * 5 * CS + c0l;
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = w[j]; sh[j] = w[CS + j]; kb[j] = w[2 * CS + j]; mu[j] = w[3 * CS + j]; kc[j] = w[4 * CS + j]; }
    if constexpr (MASK) ld8f(mask + (int64_t)n * C + c0, mk);
    // all loads of the PX pixels first (dY may alias dA: every thread reads its own elements before it writes them)
    float y[PX][8], d[PX][8], rs[PX][8], ex[PX][8];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        load8<T>(Y + (p0 + k) * ldy + c0, y[k]);
        load8<T>(dA + g * dav.goff + (pig0 + k) * dav.ld + c0, d[k]);
        if constexpr (OPT == 1) load8<T>(res + (p0 + k) * ldres + c0, rs[k]);
        if constexpr (OPT == 2) load8<T>(extra + (p0 + k) * ldex + c0, ex[k]);
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        float o[8], dzv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float dz = MASK ? d[k][j] * mk[j] : d[k][j];
            float z = y[k][j] * sc[j] + sh[j];
            if constexpr (OPT == 1) z += rs[k][j];
            if (relu && !(z > 0.f)) dz = 0.f;
            dzv[j] = dz;
            o[j] = sc[j] * dz + kb[j] * (y[k][j] - mu[j]) + kc[j];
            if constexpr (OPT == 2) o[j] += ex[k][j];
        }
        if (dZout) store8<T>(dZout + (p0 + k) * lddz + c0, dzv);
        store8<T>(dY + (p0 + k) * lddy + c0, o);
    }
    }
}
// ------------------------------------------------------------------ bias gradient (layers without a following BN)
template <typename T>
__global__ void __launch_bounds__(256)
k_bias_grad(const T* __restrict__ dY, int ld, int64_t pixels, int C, float* __restrict__ db, long long* __restrict__ acc_i) {
    __shared__ float red[256 * 8];
    const int cb = C >> 3, lanes = 256 / cb;
    const int mycb = threadIdx.x % cb, lane = threadIdx.x / cb;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    const int64_t stride = (int64_t)gridDim.x * lanes;
    int64_t p = (int64_t)blockIdx.x * lanes + lane;
    for (; p + 3 * stride < pixels; p += 4 * stride) {      // 4 independent loads in flight per thread
        float v[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) load8<T>(dY + (p + u * stride) * ld + mycb * 8, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += v[u][j];
    }
    for (; p < pixels; p += stride) {
        float v[8];
        load8<T>(dY + p * ld + mycb * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x * 8 + j] = s[j];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int l = 0; l < lanes; ++l) acc += red[(l * cb + (c >> 3)) * 8 + (c & 7)];
        // blocks meet in the 64-bit fixed-point accumulator of the BatchNorm sums (exact integer adds: the result does not depend
        // on the block order; k_bias_finish converts) -- float atomicAdd (rounds 1-3) made two runs of one step differ
        if (acc_i) bn_acc_add(acc_i, blockIdx.x, 1, C, 0, 0, c, acc, BN_BS);
        else atomicAdd(db + c, acc);
    }
}
// parity (fp32) mode: one block per 8-channel group walks every pixel in a fixed order and tree-reduces in LDS, so the
// result does not depend on scheduling (the bf16 kernel above meets in integer accumulators when given one)
__global__ void __launch_bounds__(256)
k_bias_grad_det(const float* __restrict__ dY, int ld, int64_t pixels, int C, float* __restrict__ db) {
    __shared__ double red[256];
    const int c = blockIdx.x;
    double acc = 0.0;
    for (int64_t p = threadIdx.x; p < pixels; p += 256) acc += (double)dY[p * ld + c];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) db[c] += (float)red[0];
}
void launch_bias_grad(int dt, const void* dY, int ld, int64_t pixels, int C, float* db, hipStream_t s, long long* acc_i) {
    if (dt != BF16) {
        k_bias_grad_det<<<C, 256, 0, s>>>((const float*)dY, ld, pixels, C, db);
        return;
    }
    int lanes = 256 / (C / 8);
    int grid = (int)std::min<int64_t>(256, (pixels + 4 * lanes - 1) / (4 * lanes));   // <= 256 atomic adders per channel
    if (grid < 1) grid = 1;
    if (dt == BF16) k_bias_grad<bf16><<<grid, 256, 0, s>>>((const bf16*)dY, ld, pixels, C, db, acc_i);
    else k_bias_grad<float><<<grid, 256, 0, s>>>((const float*)dY, ld, pixels, C, db, acc_i);
}

// ------------------------------------------------------------------ dropout masks, fill
__global__ void k_dropout_gen(float* __restrict__ mask, int64_t n, uint64_t seed, float p) {
    dropout_gen_body(mask, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n, seed, p);
}
void launch_dropout_gen(float* mask, int64_t n, uint64_t seed, float p, hipStream_t s) {
    if (n > 0) k_dropout_gen<<<cdiv(n, 256), 256, 0, s>>>(mask, n, seed, p);
}
__global__ void k_fill(float* p, int64_t n, float v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
void launch_fill(float* p, int64_t n, float v, hipStream_t s) {
    if (n > 0) k_fill<<<cdiv(n, 256), 256, 0, s>>>(p, n, v);
}

// ------------------------------------------------------------------ channel-slice copy / accumulate (dense concatenation)
template <typename T>
__global__ void k_slice(T* __restrict__ dst, int ldd, const T* __restrict__ src, int lds, int C, int accumulate, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3;
    const uint32_t iu = (uint32_t)i;
    const int c0 = (int)(iu % (uint32_t)cb) * 8;
    const int64_t p = iu / (uint32_t)cb;
    float v[8];
    load8<T>(src + p * lds + c0, v);
    if (accumulate) {
        float w[8];
        load8<T>(dst + p * ldd + c0, w);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += w[j];
    }
    store8<T>(dst + p * ldd + c0, v);
}
void launch_slice(int dt, void* dst, int ldd, const void* src, int lds, int64_t pixels, int C, int accumulate, hipStream_t s) {
    int64_t total = pixels * (C / 8);
    if (total == 0) return;
    if (dt == BF16) k_slice<bf16><<<cdiv(total, 256), 256, 0, s>>>((bf16*)dst, ldd, (const bf16*)src, lds, C, accumulate, total);
    else k_slice<float><<<cdiv(total, 256), 256, 0, s>>>((float*)dst, ldd, (const float*)src, lds, C, accumulate, total);
}

// ------------------------------------------------------------------ ECAM (SNUNet.py:46-59, :144-149)
// out = cat(x0_1..x0_4) lives in one [N,HW,4*C1] buffer X (C1 = 32); intra = sum of its four C1-slices.
// pool[n][0][c] = mean_hw X[n,.,c], pool[n][1][c] = max_hw X[n,.,c]   (c < 4*C1)
// pool[n][2][c'] = mean_hw intra, pool[n][3][c'] = max_hw intra        (c' < C1)  -- stored at c' of rows 2,3
// Two phases.  Phase 1: block = (pixel chunk, image); thread = (pixel lane, 8-channel block): every pixel row is read
// once, as whole 16-B pieces (a block per channel re-read the tensor 160 times at a 256-B stride); the threads of the
// first C1/8 channel blocks also form the intra sum.  Per-block partials (sum, max, arg max) go to `part`
// [n][chunk][3][C4 + C1]; phase 2 folds the chunks in order (ties -> lowest pixel index, as torch.max over a flat map).
constexpr int ECAM_CHUNKS = 128;
template <typename T>
__global__ void __launch_bounds__(256)
k_ecam_pool_part(const T* __restrict__ X, int ld, int64_t HW, int C4, float* __restrict__ part) {
    extern __shared__ float esm[];                 // [3][lanes][C4 + C1]
    const int n = blockIdx.y, chunk = blockIdx.x, C1 = C4 / 4, CT = C4 + C1;
    const int cb = C4 >> 3, lanes = 256 / cb;
    const int mycb = threadIdx.x % cb, lane = threadIdx.x / cb;
    const bool do_intra = mycb < (C1 >> 3);
    const int64_t per = (HW + gridDim.x - 1) / gridDim.x;
    const int64_t p0 = (int64_t)chunk * per, p1 = min(HW, p0 + per);
    float sm[8], mx[8], smi[8], mxi[8];
    int am[8], ami[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sm[j] = smi[j] = 0.f; mx[j] = mxi[j] = -INFINITY; am[j] = ami[j] = 0; }
    for (int64_t p = p0 + lane; p < p1; p += lanes) {
        const T* px = X + ((int64_t)n * HW + p) * ld + mycb * 8;
        float x0[8], x1[8], x2[8], x3[8];
        load8<T>(px, x0);
        if (do_intra) { load8<T>(px + C1, x1); load8<T>(px + 2 * C1, x2); load8<T>(px + 3 * C1, x3); }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sm[j] += x0[j];
            if (x0[j] > mx[j]) { mx[j] = x0[j]; am[j] = (int)p; }
        }
        if (do_intra) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // the oracle materialises `intra` as a tensor of the activation dtype
                const float v = round_as<T>((x0[j] + x1[j]) + (x2[j] + x3[j]));
                smi[j] += v;
                if (v > mxi[j]) { mxi[j] = v; ami[j] = (int)p; }
            }
        }
    }
    float* ssum = esm; float* smax = esm + lanes * CT; int* sarg = reinterpret_cast<int*>(esm + 2 * lanes * CT);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = mycb * 8 + j;
        ssum[lane * CT + c] = sm[j]; smax[lane * CT + c] = mx[j]; sarg[lane * CT + c] = am[j];
        if (do_intra) { ssum[lane * CT + C4 + c] = smi[j]; smax[lane * CT + C4 + c] = mxi[j]; sarg[lane * CT + C4 + c] = ami[j]; }
    }
    __syncthreads();
    float* out = part + ((int64_t)n * gridDim.x + chunk) * 3 * CT;
    for (int c = threadIdx.x; c < CT; c += 256) {
        float s_ = 0.f, m_ = -INFINITY;
        int a_ = 0x7fffffff;
        for (int l = 0; l < lanes; ++l) {
            s_ += ssum[l * CT + c];
            const float m2 = smax[l * CT + c];
            const int a2 = sarg[l * CT + c];
            if (m2 > m_ || (m2 == m_ && a2 < a_)) { m_ = m2; a_ = a2; }
        }
        out[c] = s_; out[CT + c] = m_; reinterpret_cast<int*>(out)[2 * CT + c] = a_;
    }
}
// pool[n][0][c] = mean_hw X[n,:,c], pool[n][1][c] = max_hw (with arg max in argm[n][0][c])   (c < C4)
// pool[n][2][c'] = mean_hw intra, pool[n][3][c'] = max_hw intra        (c' < C1)  -- stored at c' of rows 2,3
__global__ void k_ecam_pool_fin(const float* __restrict__ part, int nchunk, int64_t HW, int C4, float* __restrict__ pool,
                                int64_t* __restrict__ argm) {
    const int n = blockIdx.x, C1 = C4 / 4, CT = C4 + C1;
    for (int c = threadIdx.x; c < CT; c += blockDim.x) {
        float s_ = 0.f, m_ = -INFINITY;
        int a_ = 0x7fffffff;
        for (int k = 0; k < nchunk; ++k) {
            const float* r = part + ((int64_t)n * nchunk + k) * 3 * CT;
            s_ += r[c];
            const float m2 = r[CT + c];
            const int a2 = reinterpret_cast<const int*>(r)[2 * CT + c];
            if (m2 > m_ || (m2 == m_ && a2 < a_)) { m_ = m2; a_ = a2; }
        }
        const bool intra = c >= C4;
        const int cc = intra ? c - C4 : c;
        float* pr = pool + (int64_t)n * 4 * C4;
        pr[(intra ? 2 : 0) * C4 + cc] = s_ / (float)HW;
        pr[(intra ? 3 : 1) * C4 + cc] = m_;
        argm[(int64_t)n * 2 * C4 + (intra ? C4 : 0) + cc] = a_;
    }
}

// att[n][c] = sigmoid(W2 relu(W1 avg) + W2 relu(W1 max)); also keeps the hidden pre-activations for backward.
// one block per (n, which): which 0 -> ca over C4 channels (hidden C4/16), 1 -> ca1 over C1 channels (hidden C1/4)
__global__ void k_ecam_mlp(const float* __restrict__ pool, int C4, const float* __restrict__ w1a, const float* __restrict__ w2a,
                           const float* __restrict__ w1b, const float* __restrict__ w2b, float* __restrict__ att,
                           float* __restrict__ hid) {
    const int n = blockIdx.x, which = blockIdx.y, C1 = C4 / 4;
    const int C = which ? C1 : C4, Hd = which ? C1 / 4 : C4 / 16;
    const float* w1 = which ? w1b : w1a;     // [Hd][C]
    const float* w2 = which ? w2b : w2a;     // [C][Hd]
    const float* avg = pool + (int64_t)n * 4 * C4 + (which ? 2 : 0) * C4;
    const float* mx = avg + C4;
    __shared__ float h[2][16];
    float* hrow = hid + ((int64_t)n * 2 + which) * 2 * 16;
    if ((int)threadIdx.x < 2 * Hd) {
        const int k = threadIdx.x % Hd, src = threadIdx.x / Hd;
        const float* v = src ? mx : avg;
        float a = 0.f;
        for (int c = 0; c < C; ++c) a += w1[k * C + c] * v[c];
        hrow[src * 16 + k] = a;             // pre-ReLU
        h[src][k] = fmaxf(a, 0.f);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float o = 0.f;
        for (int k = 0; k < Hd; ++k) o += w2[c * Hd + k] * (h[0][k] + h[1][k]);
        att[((int64_t)n * 2 + which) * C4 + c] = 1.f / (1.f + expf(-o));
    }
}

// Z[n,p,c] = ca[n,c] * (X[n,p,c] + ca1[n, c % C1])
template <typename T>
__global__ void k_ecam_apply(const T* __restrict__ X, int ld, T* __restrict__ Z, int ldz, const float* __restrict__ att, int64_t HW,
                             int C4, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C4 >> 3, C1 = C4 / 4;
    const uint32_t iu = (uint32_t)i;
    const int c0 = (int)(iu % (uint32_t)cb) * 8;
    const int64_t p = iu / (uint32_t)cb;
    const int n = (int)((uint32_t)p / (uint32_t)HW);
    const float* ca = att + (int64_t)n * 2 * C4, *ca1 = ca + C4;
    float x[8], z[8];
    load8<T>(X + p * ld + c0, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = ca[c0 + j] * (x[j] + ca1[(c0 + j) % C1]);
    store8<T>(Z + p * ldz + c0, z);
}

// backward, pass 1: dX = ca * dZ (written), and per-(n,c) sums  S1[c] = sum_p dZ*(X + ca1)  (-> d ca),
// S2[c] = sum_p dZ*ca (-> d ca1 after folding the 4 slices).  block = (n, channel block of 8), threads over pixels.
template <typename T>
__global__ void __launch_bounds__(256)
k_ecam_bwd1(const T* __restrict__ X, int ld, const T* __restrict__ dZ, int lddz, T* __restrict__ dX, int lddx,
            const float* __restrict__ att, int64_t HW, int C4, float* __restrict__ part) {
    // block = (pixel chunk, image); thread = (pixel lane, 8-channel block): whole pixel rows, once.  Partial sums per
    // block -> part[n][chunk][2][C4]; k_ecam_sums_fin folds the chunks in order.
    extern __shared__ float esm[];                 // [lanes][2 * C4]
    const int n = blockIdx.y, chunk = blockIdx.x, C1 = C4 / 4;
    const int cb = C4 >> 3, lanes = 256 / cb;
    const int mycb = threadIdx.x % cb, lane = threadIdx.x / cb, c0 = mycb * 8;
    const float* ca = att + (int64_t)n * 2 * C4, *ca1 = ca + C4;
    const int64_t per = (HW + gridDim.x - 1) / gridDim.x;
    const int64_t p0 = (int64_t)chunk * per, p1 = min(HW, p0 + per);
    float s1[8], s2[8], cav[8], c1v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = s2[j] = 0.f; cav[j] = ca[c0 + j]; c1v[j] = ca1[(c0 + j) % C1]; }
    for (int64_t p = p0 + lane; p < p1; p += 2 * lanes) {
        const int64_t q0 = (int64_t)n * HW + p, q1 = q0 + lanes;
        const bool two = p + lanes < p1;
        float x[2][8], g[2][8], o[8];
        load8<T>(X + q0 * ld + c0, x[0]);
        load8<T>(dZ + q0 * lddz + c0, g[0]);
        load8<T>(X + (two ? q1 : q0) * ld + c0, x[1]);
        load8<T>(dZ + (two ? q1 : q0) * lddz + c0, g[1]);
#pragma unroll
        for (int j = 0; j < 8; ++j) { o[j] = cav[j] * g[0][j]; s1[j] += g[0][j] * (x[0][j] + c1v[j]); s2[j] += o[j]; }
        store8<T>(dX + q0 * lddx + c0, o);
        if (two) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { o[j] = cav[j] * g[1][j]; s1[j] += g[1][j] * (x[1][j] + c1v[j]); s2[j] += o[j]; }
            store8<T>(dX + q1 * lddx + c0, o);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { esm[lane * 2 * C4 + c0 + j] = s1[j]; esm[lane * 2 * C4 + C4 + c0 + j] = s2[j]; }
    __syncthreads();
    float* out = part + ((int64_t)n * gridDim.x + chunk) * 2 * C4;
    for (int c = threadIdx.x; c < 2 * C4; c += 256) {
        float a_ = 0.f;
        for (int l = 0; l < lanes; ++l) a_ += esm[l * 2 * C4 + c];
        out[c] = a_;
    }
}
__global__ void k_ecam_sums_fin(const float* __restrict__ part, int nchunk, int C4, float* __restrict__ sums) {
    const int n = blockIdx.x;
    for (int c = threadIdx.x; c < 2 * C4; c += blockDim.x) {
        float a_ = 0.f;
        for (int k = 0; k < nchunk; ++k) a_ += part[((int64_t)n * nchunk + k) * 2 * C4 + c];
        sums[(int64_t)n * 2 * C4 + c] = a_;
    }
}

// backward of the two channel-attention MLPs: from d att (= S1 for ca; folded S2 for ca1) to d avg / d max per channel
// and the fc weight gradients.  One block per MLP (`which`) walks the images in order, so the weight gradients are sums over n
// in ONE fixed order (rounds 1-3: one block per (n, which) meeting through float atomics -- not reproducible run to run).
__global__ void k_ecam_mlp_bwd(const float* __restrict__ pool, const float* __restrict__ att, const float* __restrict__ hid,
                               const float* __restrict__ sums, int C4, const float* __restrict__ w1a, const float* __restrict__ w2a,
                               const float* __restrict__ w1b, const float* __restrict__ w2b, float* __restrict__ gw1a,
                               float* __restrict__ gw2a, float* __restrict__ gw1b, float* __restrict__ gw2b,
                               float* __restrict__ dpool, int N) {
    const int which = blockIdx.x, C1 = C4 / 4;
    const int C = which ? C1 : C4, Hd = which ? C1 / 4 : C4 / 16;
    const float* w1 = which ? w1b : w1a; const float* w2 = which ? w2b : w2a;
    float* gw1 = which ? gw1b : gw1a; float* gw2 = which ? gw2b : gw2a;
    __shared__ float dpre[512];      // d(pre-sigmoid) per channel
    __shared__ float dh[2][16];
    // thread -> channels c = threadIdx.x, + blockDim.x, ...: at most 4 per thread (C <= 512, 128 threads); Hd <= 16 (hid rows)
    float g1[4][16], g2[4][16];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < 16; ++k) g1[u][k] = g2[u][k] = 0.f;
    const int lpp = (int)blockDim.x / (2 * Hd);     // lanes per (src, k) pair of the hidden-gradient sums (8 at Hd = 8)
    const bool split = lpp >= 1 && (lpp & (lpp - 1)) == 0 && lpp <= 64 && lpp * 2 * Hd == (int)blockDim.x;
    for (int n = 0; n < N; ++n) {
        const float* avg = pool + (int64_t)n * 4 * C4 + (which ? 2 : 0) * C4;
        const float* mx = avg + C4;
        const float* a = att + ((int64_t)n * 2 + which) * C4;
        const float* hrow = hid + ((int64_t)n * 2 + which) * 2 * 16;
        __syncthreads();             // dpre / dh of the previous image are done with
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            float datt;
            if (!which) datt = sums[((int64_t)n * 2 + 0) * C4 + c];
            else datt = sums[((int64_t)n * 2 + 1) * C4 + c] + sums[((int64_t)n * 2 + 1) * C4 + c + C1] +
                        sums[((int64_t)n * 2 + 1) * C4 + c + 2 * C1] + sums[((int64_t)n * 2 + 1) * C4 + c + 3 * C1];
            dpre[c] = datt * a[c] * (1.f - a[c]);
        }
        __syncthreads();
        if (split) {                 // lpp lanes per pair, fixed strided partial sums + a fixed xor tree
            const int pair = threadIdx.x / lpp, sub = threadIdx.x % lpp, k = pair % Hd, src = pair / Hd;
            float g = 0.f;
            for (int c = sub; c < C; c += lpp) g += dpre[c] * w2[c * Hd + k];
            for (int o = 1; o < lpp; o <<= 1) g += __shfl_xor(g, o, 64);
            if (sub == 0) dh[src][k] = hrow[src * 16 + k] > 0.f ? g : 0.f;
        } else if ((int)threadIdx.x < 2 * Hd) {
            const int k = threadIdx.x % Hd, src = threadIdx.x / Hd;
            float g = 0.f;
            for (int c = 0; c < C; ++c) g += dpre[c] * w2[c * Hd + k];
            dh[src][k] = hrow[src * 16 + k] > 0.f ? g : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = threadIdx.x + u * blockDim.x;
            if (c >= C) continue;
            float da = 0.f, dm = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k >= Hd) continue;
                da += dh[0][k] * w1[k * C + c];
                dm += dh[1][k] * w1[k * C + c];
                g2[u][k] += dpre[c] * (fmaxf(hrow[k], 0.f) + fmaxf(hrow[16 + k], 0.f));
                g1[u][k] += dh[0][k] * avg[c] + dh[1][k] * mx[c];
            }
            dpool[((int64_t)n * 4 + (which ? 2 : 0)) * C4 + c] = da;
            dpool[((int64_t)n * 4 + (which ? 3 : 1)) * C4 + c] = dm;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = threadIdx.x + u * blockDim.x;
        if (c >= C) continue;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k >= Hd) continue;
            gw2[c * Hd + k] = g2[u][k];
            gw1[k * C + c] = g1[u][k];
        }
    }
}

// backward, pass 2: dX[n,p,c] += davg[c]/HW + [p == argmax_c] dmax[c]  + (same through intra: channel c % C1)
template <typename T>
__global__ void k_ecam_bwd2(T* __restrict__ dX, int lddx, const float* __restrict__ dpool, const int64_t* __restrict__ argm, int64_t HW,
                            int C4, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C4 >> 3, C1 = C4 / 4;
    const uint32_t iu = (uint32_t)i;
    const int c0 = (int)(iu % (uint32_t)cb) * 8;
    const int64_t q = iu / (uint32_t)cb;
    const int n = (int)((uint32_t)q / (uint32_t)HW);
    const int64_t p = q - (int64_t)n * HW;
    const float* dp = dpool + (int64_t)n * 4 * C4;
    const int64_t* am = argm + (int64_t)n * 2 * C4;
    const float inv = 1.f / (float)HW;
    const int ci = c0 % C1;                         // 8 consecutive channels stay inside one C1 slice (C1 % 8 == 0)
    float davg[8], dmax[8], diavg[8], dimax[8], v[8];
    ld8f(dp + c0, davg); ld8f(dp + C4 + c0, dmax); ld8f(dp + 2 * C4 + ci, diavg); ld8f(dp + 3 * C4 + ci, dimax);
    longlong2 a0[4], a1[4];                         // arg-max pixel of the 8 plain / 8 intra channels (16-B loads)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a0[k] = *reinterpret_cast<const longlong2*>(am + c0 + 2 * k);
        a1[k] = *reinterpret_cast<const longlong2*>(am + C4 + ci + 2 * k);
    }
    load8<T>(dX + q * lddx + c0, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t ap = (j & 1) ? a0[j >> 1].y : a0[j >> 1].x, ai = (j & 1) ? a1[j >> 1].y : a1[j >> 1].x;
        float add = davg[j] * inv + (ap == p ? dmax[j] : 0.f);
        add += diavg[j] * inv + (ai == p ? dimax[j] : 0.f);
        v[j] += add;
    }
    store8<T>(dX + q * lddx + c0, v);
}

int64_t ecam_part_floats(int N, int C4) { return (int64_t)N * ECAM_CHUNKS * 3 * (C4 + C4 / 4); }
void launch_ecam_forward(int dt, const void* X, int ld, void* Z, int ldz, int N, int64_t HW, int C4, const float* w1a,
                         const float* w2a, const float* w1b, const float* w2b, float* pool, int64_t* argm, float* att,
                         float* hid, float* part, hipStream_t s) {
    const int CT = C4 + C4 / 4, lanes = 256 / (C4 / 8);
    const int nchunk = (int)std::min<int64_t>(ECAM_CHUNKS, (HW + lanes - 1) / lanes);
    dim3 g1(nchunk, N);
    const size_t sm1 = (size_t)3 * lanes * CT * 4;
    if (dt == BF16) k_ecam_pool_part<bf16><<<g1, 256, sm1, s>>>((const bf16*)X, ld, HW, C4, part);
    else k_ecam_pool_part<float><<<g1, 256, sm1, s>>>((const float*)X, ld, HW, C4, part);
    k_ecam_pool_fin<<<N, 256, 0, s>>>(part, nchunk, HW, C4, pool, argm);
    k_ecam_mlp<<<dim3(N, 2), 128, 0, s>>>(pool, C4, w1a, w2a, w1b, w2b, att, hid);
    int64_t total = (int64_t)N * HW * (C4 / 8);
    if (dt == BF16) k_ecam_apply<bf16><<<cdiv(total, 256), 256, 0, s>>>((const bf16*)X, ld, (bf16*)Z, ldz, att, HW, C4, total);
    else k_ecam_apply<float><<<cdiv(total, 256), 256, 0, s>>>((const float*)X, ld, (float*)Z, ldz, att, HW, C4, total);
}
void launch_ecam_backward(int dt, const void* X, int ld, const void* dZ, int lddz, void* dX, int lddx, int N, int64_t HW, int C4,
                          const float* w1a, const float* w2a, const float* w1b, const float* w2b, float* gw1a, float* gw2a,
                          float* gw1b, float* gw2b, const float* pool, const int64_t* argm, const float* att, const float* hid,
                          float* sums, float* dpool, float* part, hipStream_t s) {
    const int lanes = 256 / (C4 / 8);
    const int nchunk = (int)std::min<int64_t>(ECAM_CHUNKS, (HW + lanes - 1) / lanes);
    dim3 g1(nchunk, N);
    const size_t sm1 = (size_t)lanes * 2 * C4 * 4;
    if (dt == BF16) k_ecam_bwd1<bf16><<<g1, 256, sm1, s>>>((const bf16*)X, ld, (const bf16*)dZ, lddz, (bf16*)dX, lddx, att, HW, C4, part);
    else k_ecam_bwd1<float><<<g1, 256, sm1, s>>>((const float*)X, ld, (const float*)dZ, lddz, (float*)dX, lddx, att, HW, C4, part);
    k_ecam_sums_fin<<<N, 256, 0, s>>>(part, nchunk, C4, sums);
    k_ecam_mlp_bwd<<<2, 128, 0, s>>>(pool, att, hid, sums, C4, w1a, w2a, w1b, w2b, gw1a, gw2a, gw1b, gw2b, dpool, N);
    int64_t total = (int64_t)N * HW * (C4 / 8);
    if (dt == BF16) k_ecam_bwd2<bf16><<<cdiv(total, 256), 256, 0, s>>>((bf16*)dX, lddx, dpool, argm, HW, C4, total);
    else k_ecam_bwd2<float><<<cdiv(total, 256), 256, 0, s>>>((float*)dX, lddx, dpool, argm, HW, C4, total);
}

// ------------------------------------------------------------------ typed launch wrappers using grouped views
#define DISPATCH(dt, KERNEL, ...)                          \
    do {                                                   \
        if ((dt) == BF16) KERNEL(bf16, __VA_ARGS__);       \
        else KERNEL(float, __VA_ARGS__);                   \
    } while (0)

void launch_bn_bwd_reduce(int dt, const void* dA, int ldda, int64_t da_goff, const void* Y, int ldy, const float* stat,
                          const float* mask, int C, int groups, int npg, int64_t HW, int relu, long long* bacc,
                          hipStream_t s, const void* res, int ldres, const SliceViews* extra_src, int base_valid, void* dA_sum) {
    const SliceViews xs = extra_src ? *extra_src : SliceViews();
    const int nslab = bn_slabs(C);
    if (xs.n > 0) {
        const int ns = xs.n <= 2 ? 2 : xs.n <= 4 ? 4 : MAX_VIEWS;
#define RED_NS(T_, N_) RED_NS_R(T_, N_, res != nullptr)
#define RED_NS_R(T_, N_, HASRES_) if (HASRES_) RED_NS_M(T_, N_, true); else RED_NS_M(T_, N_, false)
#define RED_NS_M(T_, N_, R_) do { if (mask) RED_NS_K(T_, N_, R_, true); else RED_NS_K(T_, N_, R_, false); } while (0)
#define RED_NS_K(T_, N_, R_, M_) k_bn_reduce<T_, 1, N_, R_, M_><<<dim3(bn_stats_chunks((int64_t)npg * HW, C / nslab) * nslab, groups), 256, 0, s>>>((const T_*)Y, ldy, (const T_*)dA, GV{ldda, da_goff}, stat, mask, (const T_*)res, ldres, C, npg, HW, relu, (int64_t)npg * HW, bn_stats_chunks((int64_t)npg * HW, C / nslab), bacc, xs, base_valid, (T_*)dA_sum, nslab)
        if (dt == BF16) { if (ns == 2) RED_NS(bf16, 2); else if (ns == 4) RED_NS(bf16, 4); else RED_NS(bf16, MAX_VIEWS); }
        else { if (ns == 2) RED_NS(float, 2); else if (ns == 4) RED_NS(float, 4); else RED_NS(float, MAX_VIEWS); }
#undef RED_NS
#undef RED_NS_R
#undef RED_NS_M
#undef RED_NS_K
        return;
    }
    int64_t ppg = (int64_t)npg * HW;
    int nchunk = bn_stats_chunks(ppg, C / nslab);
    dim3 grid(nchunk * nslab, groups);
    GV dav{ldda, da_goff};
#define RED0(T_, R_) do { if (mask) RED0_M(T_, R_, true); else RED0_M(T_, R_, false); } while (0)
#define RED0_M(T_, R_, M_) k_bn_reduce<T_, 1, 0, R_, M_><<<grid, 256, 0, s>>>((const T_*)Y, ldy, (const T_*)dA, dav, stat, mask, (const T_*)res, ldres, C, npg, HW, relu, ppg, nchunk, bacc, xs, base_valid, (T_*)dA_sum, nslab)
    if (dt == BF16) { if (res) RED0(bf16, true); else RED0(bf16, false); }
    else { if (res) RED0(float, true); else RED0(float, false); }
#undef RED0
#undef RED0_M
}

void launch_bn_bwd_apply(int dt, const void* dA, int ldda, int64_t da_goff, void* dY, int lddy, const void* Y, int ldy,
                         const float* stat, const long long* bacc, float* dgamma, float* dbeta, const float* mask, int C, int groups,
                         int npg, int64_t HW, int relu, hipStream_t s, const void* res, int ldres, void* dZout, int lddz,
                         const void* extra, int ldex, float* dbeta_copy) {
    GV dav{ldda, da_goff};
    const int nslab = bn_slabs(C);
    const size_t lds = (size_t)groups * 5 * (C / nslab) * 4;
    const int px = (HW % 4 == 0) ? 4 : 1;        // odd-sized maps (ReplicationPad2d branch): one pixel per thread
    int64_t total = (int64_t)groups * npg * HW / px * (C / 8);
    const int grid = std::max(1, ew_grid(total) / nslab) * nslab;
#define BWD_APPLY(T_, PX_) do { if (res) BWD_APPLY_M(T_, PX_, 1); else if (extra) BWD_APPLY_M(T_, PX_, 2); else BWD_APPLY_M(T_, PX_, 0); } while (0)
#define BWD_APPLY_M(T_, PX_, O_) do { if (mask) BWD_APPLY_O(T_, PX_, O_, true); else BWD_APPLY_O(T_, PX_, O_, false); } while (0)
#define BWD_APPLY_O(T_, PX_, O_, M_) k_bn_bwd_apply<T_, PX_, O_, M_><<<grid, 256, lds, s>>>((const T_*)dA, dav, (T_*)dY, lddy, (const T_*)Y, ldy, stat, bacc, dgamma, dbeta, groups, mask, (const T_*)res, ldres, (T_*)dZout, lddz, (const T_*)extra, ldex, C, npg, HW, relu, total, nslab, dbeta_copy)
    if (dt == BF16) { if (px == 4) BWD_APPLY(bf16, 4); else BWD_APPLY(bf16, 1); }
    else { if (px == 4) BWD_APPLY(float, 4); else BWD_APPLY(float, 1); }
#undef BWD_APPLY
}

void launch_pool_bwd(int dt, const void* A, int lda, int64_t a_goff, const void* dP, int ldp, void* dA, int ldda,
                     int64_t da_goff, int groups, int npg, int H, int W, int C, int accumulate, hipStream_t s) {
    int64_t total = (int64_t)groups * npg * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
    GV av{lda, a_goff}, dav{ldda, da_goff};
    if (dt == BF16)
        k_pool_bwd<bf16><<<cdiv(total, 256), 256, 0, s>>>((const bf16*)A, av, (const bf16*)dP, ldp, (bf16*)dA, dav, npg, H, W, C, accumulate, total);
    else
        k_pool_bwd<float><<<cdiv(total, 256), 256, 0, s>>>((const float*)A, av, (const float*)dP, ldp, (float*)dA, dav, npg, H, W, C, accumulate, total);
}

void launch_skip_bwd(int dt, int mode, const void* A, int lda, int64_t a_goff, const void* Y, int ldy, const void* dD, int ldd,
                     const void* dP, int ldp, void* dA, int ldda, int64_t da_goff, const float* stat, const float* mask, int B,
                     int H, int W, int C, long long* partial, hipStream_t s) {
    const int64_t total = (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
    GV av{lda, a_goff}, dav{ldda, da_goff};
    dim3 grid((unsigned)cdiv(total, 256), 2);
#define SKIP_BWD(T_, M_) do { if (mode == 0) SKIP_BWD_K(T_, M_, 0); else SKIP_BWD_K(T_, M_, 1); } while (0)
#define SKIP_BWD_K(T_, M_, MODE_) k_skip_bwd<T_, M_, MODE_><<<grid, 256, 0, s>>>(mode, (const T_*)A, av, (const T_*)Y, ldy, (const T_*)dD, ldd, (const T_*)dP, ldp, (T_*)dA, dav, stat, mask, B, H, W, C, total, partial)
    if (dt == BF16) { if (mask) SKIP_BWD(bf16, true); else SKIP_BWD(bf16, false); }
    else { if (mask) SKIP_BWD(float, true); else SKIP_BWD(float, false); }
#undef SKIP_BWD
#undef SKIP_BWD_K
}

// channels per thread: 8 (2 waves / SIMD, fewer instructions per element) or 4 (4 waves / SIMD).  Measured at 16 pairs of 256 x 256
// (us, V = 8 / V = 4): level 1 (16 ch, 256^2) 75.3 / 60.4; level 2 32.1 / 32.0; level 3 23.1 / 27.5; level 4 13.4 / 19.4 -- the
// narrow piece pays where the map is large enough for the latency hiding to matter.
static int skip_pair_v(int B, int H, int W, int C) {
    return (int64_t)B * H * W * C >= ((int64_t)12 << 20) ? 4 : 8;
}
bool skip_pair_supported(int B, int H, int W, int C) {
    const int V = skip_pair_v(B, H, W, C), cb = C / V;
    return C % 8 == 0 && cb >= 1 && cb * V <= 256 && (cb & (cb - 1)) == 0 && (int64_t)2 * B * H * W < ((int64_t)1 << 31) &&
           B <= 65535 && (H + 1) / 2 <= 65535;
}
void launch_skip_bwd_pair(int dt, int mode, const void* Y, int ldy, const void* dD, int ldd, const void* dP, int ldp, void* dA,
                          int ldda, int64_t da_goff, const float* stat, const float* mask, int B, int H, int W, int C,
                          long long* partial, hipStream_t s) {
    const int V = skip_pair_v(B, H, W, C), cb = C / V;
    int lcb = 0;
    while ((1 << lcb) < cb) ++lcb;
    if (!skip_pair_supported(B, H, W, C))
    {   // (skip_pair_supported(): the engine plans this kernel only for shapes that pass)
        set_error("launch_skip_bwd_pair: channels per thread-slab must be a power of two, channels <= 256, 2 * B * H * W < 2^31");
        return;
    }
    GV dav{ldda, da_goff};
    const dim3 grid((unsigned)cdiv((int64_t)((W + 1) / 2) * cb, 256), (unsigned)((H + 1) / 2), (unsigned)B);
    const bool even = !(H & 1) && !(W & 1);
#define SKIP_PAIR(T_, M_) do { if (mode == 0) SKIP_PAIR_E(T_, M_, 0); else SKIP_PAIR_E(T_, M_, 1); } while (0)
#define SKIP_PAIR_E(T_, M_, MODE_) do { if (even) SKIP_PAIR_V(T_, M_, MODE_, true); else SKIP_PAIR_V(T_, M_, MODE_, false); } while (0)
#define SKIP_PAIR_V(T_, M_, MODE_, E_) do { if (V == 8) SKIP_PAIR_K(T_, M_, MODE_, E_, 8); else SKIP_PAIR_K(T_, M_, MODE_, E_, 4); } while (0)
#define SKIP_PAIR_K(T_, M_, MODE_, E_, V_) k_skip_bwd_pair<T_, M_, MODE_, E_, V_><<<grid, 256, 0, s>>>((const T_*)Y, ldy, (const T_*)dD, ldd, (const T_*)dP, ldp, (T_*)dA, dav, stat, mask, B, H, W, C, lcb, partial)
    if (dt == BF16) { if (mask) SKIP_PAIR(bf16, true); else SKIP_PAIR(bf16, false); }
    else { if (mask) SKIP_PAIR(float, true); else SKIP_PAIR(float, false); }
#undef SKIP_PAIR
#undef SKIP_PAIR_E
#undef SKIP_PAIR_V
#undef SKIP_PAIR_K
}

void launch_fuse(int dt, int mode, const void* A, int lda, int64_t a_goff, void* D, int ldd, int B, int64_t HW, int C,
                 hipStream_t s) {
    int64_t total = (int64_t)B * HW * (C / 8);
    GV av{lda, a_goff};
    if (dt == BF16) k_fuse<bf16><<<cdiv(total, 256), 256, 0, s>>>(mode, (const bf16*)A, av, (bf16*)D, ldd, HW, C, total);
    else k_fuse<float><<<cdiv(total, 256), 256, 0, s>>>(mode, (const float*)A, av, (float*)D, ldd, HW, C, total);
}
void launch_fuse_bwd(int dt, int mode, const void* A, int lda, int64_t a_goff, const void* dD, int ldd, void* dA, int ldda,
                     int64_t da_goff, int B, int64_t HW, int C, hipStream_t s) {
    int64_t total = (int64_t)B * HW * (C / 8);
    GV av{lda, a_goff}, dav{ldda, da_goff};
    if (dt == BF16)
        k_fuse_bwd<bf16><<<cdiv(total, 256), 256, 0, s>>>(mode, (const bf16*)A, av, (const bf16*)dD, ldd, (bf16*)dA, dav, HW, C, total);
    else
        k_fuse_bwd<float><<<cdiv(total, 256), 256, 0, s>>>(mode, (const float*)A, av, (const float*)dD, ldd, (float*)dA, dav, HW, C, total);
}
void launch_rep_pad(int dt, void* D, int ld, int N, int H, int W, int h0, int w0, int C, hipStream_t s) {
    if (h0 >= H && w0 >= W) return;
    int64_t total = (int64_t)N * H * W * (C / 8);
    if (dt == BF16) k_rep_pad<bf16><<<cdiv(total, 256), 256, 0, s>>>((bf16*)D, ld, H, W, h0, w0, C, total);
    else k_rep_pad<float><<<cdiv(total, 256), 256, 0, s>>>((float*)D, ld, H, W, h0, w0, C, total);
}
void launch_rep_pad_bwd(int dt, void* dD, int ld, int N, int H, int W, int h0, int w0, int C, hipStream_t s) {
    if (h0 >= H && w0 >= W) return;
    int64_t total = (int64_t)N * h0 * w0 * (C / 8);
    if (dt == BF16) k_rep_pad_bwd<bf16><<<cdiv(total, 256), 256, 0, s>>>((bf16*)dD, ld, H, W, h0, w0, C, total);
    else k_rep_pad_bwd<float><<<cdiv(total, 256), 256, 0, s>>>((float*)dD, ld, H, W, h0, w0, C, total);
}

}  // namespace stcd

// =====================================================================================================================
// Kernels of the ResNet-50 UNet change detector (smp.SegCD, the model the reference's scripts train):
//   nn.Conv2d(3, 64, 7, stride 2, padding 3, bias=False)     /root/reference/models/resnet.py:152-153
//   nn.MaxPool2d(3, stride 2, padding 1)                     /root/reference/models/resnet.py:156
//   F.interpolate(scale_factor=2, mode="nearest") + cat      /root/reference/segmentation_models_pytorch/decoders/unet/decoder.py:36-38
//   change = min(head(|d1 - d2|), |m1 - m2|)                 /root/reference/segmentation_models_pytorch/decoders/unet/model.py:323-330
namespace stcd {

// ---- stem: direct 7x7 stride-2 convolution over the packed 8-channel input (cin <= 8 real channels), Co = 64.
// thread = (output pixel, 8 output channels); the 7x7xcin x 8 filter slice of a thread's channel block sits in LDS.
template <typename T>
__global__ void __launch_bounds__(256)
k_stem_fwd(const T* __restrict__ X, const float* __restrict__ w, T* __restrict__ Y, int N, int H, int W, int cin, int Ho, int Wo, int Co) {
    extern __shared__ float wl[];                  // [49][cin][Co]
    for (int i = threadIdx.x; i < 49 * cin * Co; i += blockDim.x) {
        const int co = i % Co, ci = (i / Co) % cin, t = i / (Co * cin);
        wl[i] = w[((int64_t)co * cin + ci) * 49 + t];
    }
    __syncthreads();
    const int cb = Co >> 3;
    const int64_t total = (int64_t)N * Ho * Wo * cb;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int ky = 0; ky < 7; ++ky) {
        const int iy = 2 * oy - 3 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 7; ++kx) {
            const int ix = 2 * ox - 3 + kx;
            if (ix < 0 || ix >= W) continue;
            float x[8];
            load8<T>(X + (((int64_t)n * H + iy) * W + ix) * 8, x);
            const float* wt = wl + (int64_t)(ky * 7 + kx) * cin * Co + c0;
            for (int ci = 0; ci < cin; ++ci) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += x[ci] * wt[ci * Co + j];
            }
        }
    }
    store8<T>(Y + (((int64_t)n * Ho + oy) * Wo + ox) * Co + c0, acc);
}
void launch_stem_fwd(int dt, const void* X, const float* w, void* Y, int N, int H, int W, int cin, int Co, hipStream_t s) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t total = (int64_t)N * Ho * Wo * (Co / 8);
    const size_t lds = (size_t)49 * cin * Co * 4;
    if (dt == BF16) k_stem_fwd<bf16><<<cdiv(total, 256), 256, lds, s>>>((const bf16*)X, w, (bf16*)Y, N, H, W, cin, Ho, Wo, Co);
    else k_stem_fwd<float><<<cdiv(total, 256), 256, lds, s>>>((const float*)X, w, (float*)Y, N, H, W, cin, Ho, Wo, Co);
}
// dW[co][ci][ky][kx] = sum over positions of X(2oy-3+ky, 2ox-3+kx)[ci] * dY(oy,ox)[co]; grid = (position chunks, 49 taps),
// block = 4 position lanes x 64 output channels.  Every block writes its partial filter [chunk][tap][co][ci] and k_stem_wgrad_fin
// adds the chunks in index order: reproducible run to run (rounds 1-3 met through float atomics on dW).
template <typename T>
__global__ void __launch_bounds__(256)
k_stem_wgrad(const T* __restrict__ X, const T* __restrict__ dY, float* __restrict__ part, int N, int H, int W, int cin, int Ho, int Wo, int Co) {
    __shared__ float red[4][64][8];
    const int t = blockIdx.y, ky = t / 7, kx = t % 7;
    const int co = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int64_t npos = (int64_t)N * Ho * Wo;
    const int64_t per = (npos + gridDim.x - 1) / gridDim.x, p0 = (int64_t)blockIdx.x * per, p1 = min(npos, p0 + per);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int64_t p = p0 + lane; p < p1; p += 4) {
        const int ox = (int)(p % Wo);
        const int64_t r = p / Wo;
        const int oy = (int)(r % Ho), n = (int)(r / Ho);
        const int iy = 2 * oy - 3 + ky, ix = 2 * ox - 3 + kx;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        float x[8];
        load8<T>(X + (((int64_t)n * H + iy) * W + ix) * 8, x);
        const float g = co < Co ? (float)dY[p * Co + co] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += x[j] * g;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[lane][co][j] = acc[j];
    __syncthreads();
    if (lane == 0 && co < Co)
        for (int ci = 0; ci < cin; ++ci)
            part[(((int64_t)blockIdx.x * 49 + t) * Co + co) * cin + ci] = (red[0][co][ci] + red[1][co][ci]) + (red[2][co][ci] + red[3][co][ci]);
}
__global__ void k_stem_wgrad_fin(const float* __restrict__ part, int chunks, int cin, int Co, float* __restrict__ dW) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // (t, co, ci)
    if (i >= 49 * Co * cin) return;
    const int ci = i % cin, co = (i / cin) % Co, t = i / (cin * Co);
    float a = 0.f;
    for (int k = 0; k < chunks; ++k) a += part[(int64_t)k * 49 * Co * cin + i];
    dW[((int64_t)co * cin + ci) * 49 + t] = a;
}
static int stem_wgrad_chunks(int N, int H, int W) { return (int)std::min<int64_t>(256, ((int64_t)N * (H / 2) * (W / 2) + 1023) / 1024); }
int64_t stem_wgrad_part_floats(int N, int H, int W, int cin, int Co) { return (int64_t)stem_wgrad_chunks(N, H, W) * 49 * Co * cin; }
void launch_stem_wgrad(int dt, const void* X, const void* dY, float* dW, int N, int H, int W, int cin, int Co, hipStream_t s, float* part) {
    const int Ho = H / 2, Wo = W / 2;
    const int chunks = stem_wgrad_chunks(N, H, W);
    dim3 grid(chunks, 49);
    if (dt == BF16) k_stem_wgrad<bf16><<<grid, 256, 0, s>>>((const bf16*)X, (const bf16*)dY, part, N, H, W, cin, Ho, Wo, Co);
    else k_stem_wgrad<float><<<grid, 256, 0, s>>>((const float*)X, (const float*)dY, part, N, H, W, cin, Ho, Wo, Co);
    k_stem_wgrad_fin<<<cdiv((int64_t)49 * Co * cin, 256), 256, 0, s>>>(part, chunks, cin, Co, dW);
}

// ---- 3x3 stride-2 padding-1 max-pool (H, W even) and its gradient (first maximum in scan order, as torch).
// The forward also records WHICH of the 9 window positions won (one byte per pooled element, idx [N,Ho,Wo,C]): the
// backward then reads (index, dP) of the <= 4 windows an input pixel belongs to instead of re-scanning their 9 inputs each
// (the scan version read ~20 pieces per pixel: 369 us on the 32 x 128 x 128 x 64 stem map; this one ~6).
template <typename T>
__global__ void k_maxpool3(const T* __restrict__ A, int lda, T* __restrict__ P, int ldp, unsigned char* __restrict__ idx, int H, int W, int C,
                           int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3, Ho = H / 2, Wo = W / 2;
    const int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    float best[8];
    unsigned char arg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; arg[j] = 255; }
    for (int ky = 0; ky < 3; ++ky) {
        const int y = 2 * oy - 1 + ky;
        if (y < 0 || y >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int x = 2 * ox - 1 + kx;
            if (x < 0 || x >= W) continue;
            float v[8];
            load8<T>(A + (((int64_t)n * H + y) * W + x) * lda + c0, v);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (v[j] > best[j] || arg[j] == 255) { best[j] = v[j]; arg[j] = (unsigned char)(ky * 3 + kx); }     // strict >: the FIRST maximum
        }
    }
    store8<T>(P + (((int64_t)n * Ho + oy) * Wo + ox) * ldp + c0, best);
    if (idx) {
        uint2 pk;
        pk.x = arg[0] | (arg[1] << 8) | (arg[2] << 16) | ((unsigned)arg[3] << 24);
        pk.y = arg[4] | (arg[5] << 8) | (arg[6] << 16) | ((unsigned)arg[7] << 24);
        *reinterpret_cast<uint2*>(idx + (((int64_t)n * Ho + oy) * Wo + ox) * C + c0) = pk;
    }
}
void launch_maxpool3(int dt, const void* A, int lda, void* P, int ldp, int N, int H, int W, int C, hipStream_t s, unsigned char* idx) {
    const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
    if (dt == BF16) k_maxpool3<bf16><<<cdiv(total, 256), 256, 0, s>>>((const bf16*)A, lda, (bf16*)P, ldp, idx, H, W, C, total);
    else k_maxpool3<float><<<cdiv(total, 256), 256, 0, s>>>((const float*)A, lda, (float*)P, ldp, idx, H, W, C, total);
}
// dA(y,x) = sum over the (up to 4) windows that contain (y,x) of dP(window) * [window's recorded winner is (y,x)]
template <typename T>
__global__ void k_maxpool3_bwd(const unsigned char* __restrict__ idx, const T* __restrict__ dP, int ldp, T* __restrict__ dA, int ldda, int H,
                               int W, int C, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3, Ho = H / 2, Wo = W / 2;
    const int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    float out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = 0.f;
    // rows: an even y lies in window oy = y/2 only (as its middle row), an odd y in windows (y-1)/2 (bottom row) and (y+1)/2 (top row)
    const int oy0 = y >> 1, noy = (y & 1) ? 2 : 1, ox0 = x >> 1, nox = (x & 1) ? 2 : 1;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int oy = oy0 + a;
        if (a >= noy || oy >= Ho) continue;
        const int ky = y - (2 * oy - 1);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ox = ox0 + b;
            if (b >= nox || ox >= Wo) continue;
            const int k = ky * 3 + (x - (2 * ox - 1));
            const int64_t pp = ((int64_t)n * Ho + oy) * Wo + ox;
            const uint2 pk = *reinterpret_cast<const uint2*>(idx + pp * C + c0);
            float g[8];
            load8<T>(dP + pp * ldp + c0, g);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned w = j < 4 ? pk.x : pk.y;
                out[j] += (int)((w >> (8 * (j & 3))) & 255u) == k ? g[j] : 0.f;
            }
        }
    }
    store8<T>(dA + (((int64_t)n * H + y) * W + x) * ldda + c0, out);
}
void launch_maxpool3_bwd(int dt, const unsigned char* idx, const void* dP, int ldp, void* dA, int ldda, int N, int H, int W, int C,
                         hipStream_t s) {
    const int64_t total = (int64_t)N * H * W * (C / 8);
    if (dt == BF16) k_maxpool3_bwd<bf16><<<cdiv(total, 256), 256, 0, s>>>(idx, (const bf16*)dP, ldp, (bf16*)dA, ldda, H, W, C, total);
    else k_maxpool3_bwd<float><<<cdiv(total, 256), 256, 0, s>>>(idx, (const float*)dP, ldp, (float*)dA, ldda, H, W, C, total);
}

// ---- nearest x2 up-sampling into a channel slice of the decoder's concat buffer, and its gradient (sum of the 2x2 block)
template <typename T>
__global__ void k_upsample2(const T* __restrict__ X, int ldx, T* __restrict__ D, int ldd, int h, int w, int C, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3;
    const int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    const int x = (int)(r % w); r /= w;
    const int y = (int)(r % h);
    const int n = (int)(r / h);
    const uint4* src = reinterpret_cast<const uint4*>(X + (((int64_t)n * h + y) * w + x) * ldx + c0);
    float v[8];
    load8<T>(reinterpret_cast<const T*>(src), v);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        store8<T>(D + (((int64_t)n * 2 * h + 2 * y + (k >> 1)) * 2 * w + 2 * x + (k & 1)) * ldd + c0, v);
}
void launch_upsample2(int dt, const void* X, int ldx, void* D, int ldd, int N, int h, int w, int C, hipStream_t s) {
    const int64_t total = (int64_t)N * h * w * (C / 8);
    if (dt == BF16) k_upsample2<bf16><<<cdiv(total, 256), 256, 0, s>>>((const bf16*)X, ldx, (bf16*)D, ldd, h, w, C, total);
    else k_upsample2<float><<<cdiv(total, 256), 256, 0, s>>>((const float*)X, ldx, (float*)D, ldd, h, w, C, total);
}
template <typename T>
__global__ void k_upsample2_bwd(const T* __restrict__ dD, int ldd, T* __restrict__ dX, int ldx, int h, int w, int C, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cb = C >> 3;
    const int c0 = (int)(i % cb) * 8;
    int64_t r = i / cb;
    const int x = (int)(r % w); r /= w;
    const int y = (int)(r % h);
    const int n = (int)(r / h);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v[8];
        load8<T>(dD + (((int64_t)n * 2 * h + 2 * y + (k >> 1)) * 2 * w + 2 * x + (k & 1)) * ldd + c0, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
    store8<T>(dX + (((int64_t)n * h + y) * w + x) * ldx + c0, acc);
}
void launch_upsample2_bwd(int dt, const void* dD, int ldd, void* dX, int ldx, int N, int h, int w, int C, hipStream_t s) {
    const int64_t total = (int64_t)N * h * w * (C / 8);
    if (dt == BF16) k_upsample2_bwd<bf16><<<cdiv(total, 256), 256, 0, s>>>((const bf16*)dD, ldd, (bf16*)dX, ldx, h, w, C, total);
    else k_upsample2_bwd<float><<<cdiv(total, 256), 256, 0, s>>>((const float*)dD, ldd, (float*)dX, ldx, h, w, C, total);
}

// ---- SegCD output combination on fp32 NCHW maps raw = [m1; m2; diffea] (3 x n elements):
//      out = [m1; m2; min(diffea, |m1 - m2|)]; gradient g = [g1; g2; gc] -> d raw (torch.min splits ties 0.5 / 0.5, abs' = sign)
__global__ void k_segcd_combine(const float* __restrict__ raw, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float m1 = raw[i], m2 = raw[n + i], df = raw[2 * n + i];
    const float ds = fabsf(m1 - m2);
    // torch.min propagates NaN (fminf would return the other operand and hide a diverged branch)
    out[i] = m1; out[n + i] = m2; out[2 * n + i] = (df != df || ds != ds) ? df + ds : fminf(df, ds);
}
__global__ void k_segcd_combine_bwd(const float* __restrict__ raw, const float* __restrict__ g, float* __restrict__ draw, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float m1 = raw[i], m2 = raw[n + i], df = raw[2 * n + i], gc = g[2 * n + i];
    const float d = m1 - m2, ds = fabsf(d);
    // a NaN in either branch poisons both gradients, as torch.min's backward does through the NaN it forwarded
    const float wf = (df != df || ds != ds) ? df + ds : (df < ds ? 1.f : (df == ds ? 0.5f : 0.f));
    const float gs = gc * (1.f - wf) * (float)((d > 0.f) - (d < 0.f));
    draw[i] = g[i] + gs; draw[n + i] = g[n + i] - gs; draw[2 * n + i] = gc * wf;
}
void launch_segcd_combine(const float* raw, float* out, int64_t n, hipStream_t s) { k_segcd_combine<<<cdiv(n, 256), 256, 0, s>>>(raw, out, n); }
void launch_segcd_combine_bwd(const float* raw, const float* g, float* draw, int64_t n, hipStream_t s) {
    k_segcd_combine_bwd<<<cdiv(n, 256), 256, 0, s>>>(raw, g, draw, n);
}

}  // namespace stcd
