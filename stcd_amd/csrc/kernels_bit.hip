// kernels_bit.hip -- the token path of BIT (BASE_Transformer, models/networks.py:307-441) between conv_pred and |x1 - x2| (gfx950):
// semantic tokenizer, one-layer token encoder, cross-attention decoder over every pixel of both dates.  fp32 arithmetic throughout;
// only the pixel maps take the engine dtype (T).  Every reduction goes through per-block partials and a fixed-order finish
// (k_bit_sum_parts): no floating-point atomics, results are bit-identical run to run.
//
// Parameter block of one transformer layer, as the reference registers it (Residual(PreNorm(Attention)), Residual(PreNorm(FeedForward));
// to_q / to_k / to_v of the decoder's Cross_Attention are contiguous exactly like the encoder's to_qkv rows), I = heads * dim_head:
//   norm.weight 32 | norm.bias 32 | to_q [I,32] | to_k [I,32] | to_v [I,32] | to_out.0.weight [32,I] | to_out.0.bias 32 |
//   norm.weight 32 | norm.bias 32 | net.0.weight [64,32] | net.0.bias 64 | net.3.weight [32,64] | net.3.bias 32
//
// Decoder: per (layer, image) the projections are folded against the 4 memory tokens once (k_bit_dec_fold):
//   A[c][(h,j)] = s * sum_d Wq[h dh + d][c] K[j][h dh + d],  P[(h,j)][c] = sum_d V[j][h dh + d] Wo[c][h dh + d],  s = 32^-0.5
// so a pixel row needs LN, z = xhat A (32 x 32), softmax in 8 groups of 4, y = x + p P + b_o, LN', the 32 -> 64 -> 32 FeedForward: one
// thread per row, all depth layers in one launch, no [rows, heads * dim_head] tensor.  The backward recomputes the row's forward
// from the stored layer input, and forms dA / dP per image and the FeedForward / LayerNorm gradients per layer as block-level outer
// products over LDS-staged row vectors; k_bit_dec_unfold turns dA, dP into dWq, dWk, dWv, dWo and d(memory).
#include "common.h"

namespace stcd {

constexpr float BIT_EPS = 1e-5f;
constexpr float BIT_SCALE = 0.17677669529663687f;      // dim ** -0.5 with dim = 32 (help_funcs.py:71,122), NOT dim_head ** -0.5
constexpr int DEC_PART = 6400;                         // floats of one decoder-backward partial: dA 1024 | dP 1024 | norm 64 | to_out bias .. net.3.bias 4288
constexpr int DEC_CONST = 6400;                        // LDS constants of one decoder layer: A | P | W1 [k][c] | W2t [k][c] | 256 vector entries
constexpr int DEC_BWD_ROWS = 128;
constexpr int STG_LD = 33;                             // padded row of a staged [rows][32] array (odd stride: no bank conflicts on the row index)

struct BitOff { int g1, b1, wq, wk, wv, wo, bo, g2, b2, w1, bb1, w2, bb2, size; };
__host__ __device__ inline BitOff bit_off(int I) {
    BitOff o;
    o.g1 = 0; o.b1 = 32; o.wq = 64; o.wk = 64 + 32 * I; o.wv = 64 + 64 * I; o.wo = 64 + 96 * I; o.bo = 64 + 128 * I;
    o.g2 = o.bo + 32; o.b2 = o.g2 + 32; o.w1 = o.b2 + 32; o.bb1 = o.w1 + 2048; o.w2 = o.bb1 + 64; o.bb2 = o.w2 + 2048; o.size = o.bb2 + 32;
    return o;
}
int64_t bit_layer_floats(int dh) { return bit_off(8 * dh).size; }

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}
__device__ __forceinline__ float sum32(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename T>
__device__ __forceinline__ void load32(const T* p, float (&v)[32]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float t[8];
        load8<T>(p + 8 * q, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[8 * q + k] = t[k];
    }
}
template <typename T>
__device__ __forceinline__ void store32(T* p, const float (&v)[32]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = v[8 * q + k];
        store8<T>(p + 8 * q, t);
    }
}

// out[b * osb + i] (+)= sum_p part[b * bs + p * ps + i], p in ascending order
__global__ void __launch_bounds__(256) k_bit_sum_parts(float* __restrict__ out, int64_t osb, const float* __restrict__ part, int nparts,
                                                        int64_t ps, int64_t bs, int n, int nbatch, int add) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * nbatch) return;
    const int b = (int)(idx / n), i = (int)(idx - (int64_t)b * n);
    const float* p = part + b * bs + i;
    float s = 0.f;
    for (int k = 0; k < nparts; ++k) s += p[k * ps];
    float* o = out + b * osb + i;
    *o = add ? *o + s : s;
}
static void sum_parts(float* out, int64_t osb, const float* part, int nparts, int64_t ps, int64_t bs, int n, int nbatch, int add, hipStream_t s) {
    const int64_t tot = (int64_t)n * nbatch;
    k_bit_sum_parts<<<dim3((unsigned)((tot + 255) / 256)), 256, 0, s>>>(out, osb, part, nparts, ps, bs, n, nbatch, add);
}

// ------------------------------------------------------------------------------------------------ tokenizer
// One block per image.  logits[l][r] = sum_c Wa[l][c] x[r][c]; a = softmax over the n positions; tokens[l] = sum_r a[l][r] x[r].
// stat[img][l] = (max, sum of exp) for the backward.
template <typename T>
__global__ void __launch_bounds__(256) k_bit_tok_fwd(const T* __restrict__ x, const float* __restrict__ wa, float* __restrict__ tok,
                                                      float* __restrict__ stat, int n) {
    __shared__ float sw[128];
    __shared__ float red[4][132];
    __shared__ float sM[4];
    const int img = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t < 128) sw[t] = wa[t];
    __syncthreads();
    const T* xi = x + (int64_t)img * n * 32;
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int r = t; r < n; r += 256) {
        float v[32];
        load32<T>(xi + (int64_t)r * 32, v);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 32; ++c) s += v[c] * sw[l * 32 + c];
            mx[l] = fmaxf(mx[l], s);
        }
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) { mx[l] = wave_max(mx[l]); if (lane == 0) red[wv][l] = mx[l]; }
    __syncthreads();
    if (t < 4) sM[t] = fmaxf(fmaxf(red[0][t], red[1][t]), fmaxf(red[2][t], red[3][t]));
    __syncthreads();
    const float M[4] = {sM[0], sM[1], sM[2], sM[3]};
    float acc[4][32], sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int c = 0; c < 32; ++c) acc[l][c] = 0.f;
    for (int r = t; r < n; r += 256) {
        float v[32];
        load32<T>(xi + (int64_t)r * 32, v);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 32; ++c) s += v[c] * sw[l * 32 + c];
            const float e = expf(s - M[l]);
            sum[l] += e;
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[l][c] += e * v[c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 4; ++l) {
#pragma unroll
        for (int c = 0; c < 32; ++c) { const float s = wave_sum(acc[l][c]); if (lane == 0) red[wv][l * 32 + c] = s; }
        const float s = wave_sum(sum[l]);
        if (lane == 0) red[wv][128 + l] = s;
    }
    __syncthreads();
    if (t < 128) {
        const int l = t >> 5;
        const float S = ((red[0][128 + l] + red[1][128 + l]) + red[2][128 + l]) + red[3][128 + l];
        tok[(int64_t)img * 128 + t] = (((red[0][t] + red[1][t]) + red[2][t]) + red[3][t]) / S;
        if ((t & 31) == 0) { stat[img * 8 + 2 * l] = M[l]; stat[img * 8 + 2 * l + 1] = S; }
    }
}

// g = d(tokens) [img][4][32].  da = x g^T, ds = a (da - sum_r a da), dx = dec_din + a^T g + ds Wa, dWa partial [img][4][32] = sum_r ds x
template <typename T>
__global__ void __launch_bounds__(256) k_bit_tok_bwd(const T* __restrict__ x, const float* __restrict__ wa, const float* __restrict__ stat,
                                                      const float* __restrict__ g, const T* __restrict__ dec_din, T* __restrict__ dx,
                                                      float* __restrict__ part, int n) {
    __shared__ float sw[128], sg[128];
    __shared__ float red[4][128];
    __shared__ float sdot[4];
    const int img = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t < 128) { sw[t] = wa[t]; sg[t] = g[(int64_t)img * 128 + t]; }
    __syncthreads();
    const T* xi = x + (int64_t)img * n * 32;
    float M[4], iS[4], dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < 4; ++l) { M[l] = stat[img * 8 + 2 * l]; iS[l] = 1.f / stat[img * 8 + 2 * l + 1]; }
    for (int r = t; r < n; r += 256) {
        float v[32];
        load32<T>(xi + (int64_t)r * 32, v);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            float s = 0.f, da = 0.f;
#pragma unroll
            for (int c = 0; c < 32; ++c) { s += v[c] * sw[l * 32 + c]; da += v[c] * sg[l * 32 + c]; }
            dot[l] += expf(s - M[l]) * iS[l] * da;
        }
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) { const float s = wave_sum(dot[l]); if (lane == 0) red[wv][l] = s; }
    __syncthreads();
    if (t < 4) sdot[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 4; ++l) dot[l] = sdot[l];
    float acc[4][32];
#pragma unroll
    for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int c = 0; c < 32; ++c) acc[l][c] = 0.f;
    for (int r = t; r < n; r += 256) {
        float v[32], o[32];
        load32<T>(xi + (int64_t)r * 32, v);
        load32<T>(dec_din + ((int64_t)img * n + r) * 32, o);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            float s = 0.f, da = 0.f;
#pragma unroll
            for (int c = 0; c < 32; ++c) { s += v[c] * sw[l * 32 + c]; da += v[c] * sg[l * 32 + c]; }
            const float a = expf(s - M[l]) * iS[l], ds = a * (da - dot[l]);
#pragma unroll
            for (int c = 0; c < 32; ++c) { o[c] += a * sg[l * 32 + c] + ds * sw[l * 32 + c]; acc[l][c] += ds * v[c]; }
        }
        store32<T>(dx + ((int64_t)img * n + r) * 32, o);
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int c = 0; c < 32; ++c) { const float s = wave_sum(acc[l][c]); if (lane == 0) red[wv][l * 32 + c] = s; }
    __syncthreads();
    if (t < 128) part[(int64_t)img * 128 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

void launch_bit_tok_fwd(int dt, const void* x, const float* wa, float* tok, float* stat, int NI, int n, hipStream_t s) {
    if (dt == BF16) k_bit_tok_fwd<bf16><<<NI, 256, 0, s>>>((const bf16*)x, wa, tok, stat, n);
    else k_bit_tok_fwd<float><<<NI, 256, 0, s>>>((const float*)x, wa, tok, stat, n);
}
void launch_bit_tok_bwd(int dt, const void* x, const float* wa, const float* stat, const float* dtok, const void* dec_din, void* dx,
                        float* part, float* dwa, int NI, int n, hipStream_t s) {
    if (dt == BF16) k_bit_tok_bwd<bf16><<<NI, 256, 0, s>>>((const bf16*)x, wa, stat, dtok, (const bf16*)dec_din, (bf16*)dx, part, n);
    else k_bit_tok_bwd<float><<<NI, 256, 0, s>>>((const float*)x, wa, stat, dtok, (const float*)dec_din, (float*)dx, part, n);
    sum_parts(dwa, 0, part, NI, 128, 0, 128, 1, 1, s);
}

// ------------------------------------------------------------------------------------------------ token encoder
// One block per pair, thread (i, c) of the [8, 32] token matrix (tokens of date 0 then date 1, + pos_embedding), heads one after the
// other so that LDS holds one head's q, k, v.  BWD: recomputes the forward, then back-propagates; parameter gradients go to
// part[b][layer block | pos_embedding 256] (every entry written exactly once), summed over the pairs afterwards.
struct EncSmem {
    float u[256], q[512], k[512], v[512], att[64], oh[512], v2[256], pre[512], hdn[512];
    float dT[256], dT1[256], dpre[512], doh[512], datt[64], dd[64], dq[512], dk[512], dv[512], stg[256], stg2[256];
};
template <bool BWD>
__global__ void __launch_bounds__(256) k_bit_enc(const float* __restrict__ tok_in, const float* __restrict__ pos, const float* __restrict__ lp,
                                                  float* __restrict__ tok_out, const float* __restrict__ dtok_out, float* __restrict__ dtok_in,
                                                  float* __restrict__ part, int B, int dh) {
    __shared__ EncSmem S;
    const int b = blockIdx.x, t = threadIdx.x, i = t >> 5, c = t & 31, I = 8 * dh;
    const BitOff o = bit_off(I);
    const int64_t tix = ((int64_t)((i >> 2) * B + b) * 4 + (i & 3)) * 32 + c;
    const float x0 = tok_in[tix] + pos[t];
    const float mu1 = sum32(x0) * (1.f / 32.f), d1 = x0 - mu1;
    const float rs1 = rsqrtf(sum32(d1 * d1) * (1.f / 32.f) + BIT_EPS), xh1 = d1 * rs1;
    S.u[t] = xh1 * lp[o.g1 + c] + lp[o.b1 + c];
    __syncthreads();
    auto head_fwd = [&](int h) {
        for (int idx = t; idx < 24 * dh; idx += 256) {
            const int which = idx / (8 * dh), rem = idx - which * 8 * dh, ii = rem / dh, d = rem - ii * dh;
            const float* w = lp + o.wq + (int64_t)(which * I + h * dh + d) * 32;
            float s = 0.f;
#pragma unroll
            for (int cc = 0; cc < 32; ++cc) s += S.u[ii * 32 + cc] * w[cc];
            (which == 0 ? S.q : which == 1 ? S.k : S.v)[ii * dh + d] = s;
        }
        __syncthreads();
        if (t < 64) {
            const int ii = t >> 3, j = t & 7;
            float s = 0.f;
            for (int d = 0; d < dh; ++d) s += S.q[ii * dh + d] * S.k[j * dh + d];
            S.att[t] = s * BIT_SCALE;
        }
        __syncthreads();
        if (t < 8) {
            float m = S.att[t * 8], e[8], sum = 0.f;
            for (int j = 1; j < 8; ++j) m = fmaxf(m, S.att[t * 8 + j]);
            for (int j = 0; j < 8; ++j) { e[j] = expf(S.att[t * 8 + j] - m); sum += e[j]; }
            for (int j = 0; j < 8; ++j) S.att[t * 8 + j] = e[j] / sum;
        }
        __syncthreads();
        for (int idx = t; idx < 8 * dh; idx += 256) {
            const int ii = idx / dh, d = idx - ii * dh;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += S.att[ii * 8 + j] * S.v[j * dh + d];
            S.oh[idx] = s;
        }
        __syncthreads();
    };
    float acc = 0.f;
    for (int h = 0; h < 8; ++h) {
        head_fwd(h);
        const float* w = lp + o.wo + (int64_t)c * I + h * dh;
        for (int d = 0; d < dh; ++d) acc += S.oh[i * dh + d] * w[d];
        __syncthreads();
    }
    const float t1 = x0 + acc + lp[o.bo + c];
    const float mu2 = sum32(t1) * (1.f / 32.f), d2 = t1 - mu2;
    const float rs2 = rsqrtf(sum32(d2 * d2) * (1.f / 32.f) + BIT_EPS), xh2 = d2 * rs2;
    S.v2[t] = xh2 * lp[o.g2 + c] + lp[o.b2 + c];
    __syncthreads();
    for (int idx = t; idx < 512; idx += 256) {
        const int ii = idx >> 6, kk = idx & 63;
        float s = lp[o.bb1 + kk];
#pragma unroll
        for (int cc = 0; cc < 32; ++cc) s += S.v2[ii * 32 + cc] * lp[o.w1 + kk * 32 + cc];
        S.pre[idx] = s; S.hdn[idx] = gelu_f(s);
    }
    __syncthreads();
    float t2 = t1 + lp[o.bb2 + c];
    for (int kk = 0; kk < 64; ++kk) t2 += S.hdn[i * 64 + kk] * lp[o.w2 + c * 64 + kk];
    if (!BWD) { tok_out[tix] = t2; return; }

    float* P = part + (int64_t)b * (o.size + 256);
    const float dt2 = dtok_out[tix];
    S.dT[t] = dt2;
    __syncthreads();
    for (int idx = t; idx < 2048; idx += 256) {          // d net.3.weight [c][k]
        const int cc = idx >> 6, kk = idx & 63;
        float s = 0.f;
#pragma unroll
        for (int ii = 0; ii < 8; ++ii) s += S.dT[ii * 32 + cc] * S.hdn[ii * 64 + kk];
        P[o.w2 + idx] = s;
    }
    if (t < 32) { float s = 0.f; for (int ii = 0; ii < 8; ++ii) s += S.dT[ii * 32 + t]; P[o.bb2 + t] = s; }
    for (int idx = t; idx < 512; idx += 256) {
        const int ii = idx >> 6, kk = idx & 63;
        float s = 0.f;
#pragma unroll
        for (int cc = 0; cc < 32; ++cc) s += S.dT[ii * 32 + cc] * lp[o.w2 + cc * 64 + kk];
        S.dpre[idx] = s * gelu_d(S.pre[idx]);
    }
    __syncthreads();
    for (int idx = t; idx < 2048; idx += 256) {          // d net.0.weight [k][c]
        const int kk = idx >> 5, cc = idx & 31;
        float s = 0.f;
#pragma unroll
        for (int ii = 0; ii < 8; ++ii) s += S.dpre[ii * 64 + kk] * S.v2[ii * 32 + cc];
        P[o.w1 + idx] = s;
    }
    if (t < 64) { float s = 0.f; for (int ii = 0; ii < 8; ++ii) s += S.dpre[ii * 64 + t]; P[o.bb1 + t] = s; }
    float dv2 = 0.f;
    for (int kk = 0; kk < 64; ++kk) dv2 += S.dpre[i * 64 + kk] * lp[o.w1 + kk * 32 + c];
    S.stg[t] = dv2 * xh2; S.stg2[t] = dv2;
    float dt1;
    {
        const float dxh = dv2 * lp[o.g2 + c];
        const float m1 = sum32(dxh) * (1.f / 32.f), m2 = sum32(dxh * xh2) * (1.f / 32.f);
        dt1 = dt2 + rs2 * (dxh - m1 - xh2 * m2);
    }
    S.dT1[t] = dt1;
    __syncthreads();
    if (t < 32) {
        float a = 0.f, bb = 0.f, cc = 0.f;
        for (int ii = 0; ii < 8; ++ii) { a += S.stg[ii * 32 + t]; bb += S.stg2[ii * 32 + t]; cc += S.dT1[ii * 32 + t]; }
        P[o.g2 + t] = a; P[o.b2 + t] = bb; P[o.bo + t] = cc;
    }
    float du = 0.f;
    for (int h = 0; h < 8; ++h) {
        head_fwd(h);
        for (int idx = t; idx < 32 * dh; idx += 256) {   // d to_out.0.weight [c][h dh + d]
            const int cc = idx / dh, d = idx - cc * dh;
            float s = 0.f;
#pragma unroll
            for (int ii = 0; ii < 8; ++ii) s += S.dT1[ii * 32 + cc] * S.oh[ii * dh + d];
            P[o.wo + (int64_t)cc * I + h * dh + d] = s;
        }
        for (int idx = t; idx < 8 * dh; idx += 256) {
            const int ii = idx / dh, d = idx - ii * dh;
            float s = 0.f;
#pragma unroll
            for (int cc = 0; cc < 32; ++cc) s += S.dT1[ii * 32 + cc] * lp[o.wo + (int64_t)cc * I + h * dh + d];
            S.doh[idx] = s;
        }
        __syncthreads();
        if (t < 64) {
            const int ii = t >> 3, j = t & 7;
            float s = 0.f;
            for (int d = 0; d < dh; ++d) s += S.doh[ii * dh + d] * S.v[j * dh + d];
            S.datt[t] = s;
        }
        __syncthreads();
        if (t < 8) {
            float dot = 0.f;
            for (int j = 0; j < 8; ++j) dot += S.att[t * 8 + j] * S.datt[t * 8 + j];
            for (int j = 0; j < 8; ++j) S.dd[t * 8 + j] = S.att[t * 8 + j] * (S.datt[t * 8 + j] - dot) * BIT_SCALE;
        }
        __syncthreads();
        for (int idx = t; idx < 8 * dh; idx += 256) {
            const int ii = idx / dh, d = idx - ii * dh;
            float a = 0.f, bb = 0.f, cc = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a += S.dd[ii * 8 + j] * S.k[j * dh + d];
                bb += S.dd[j * 8 + ii] * S.q[j * dh + d];
                cc += S.att[j * 8 + ii] * S.doh[j * dh + d];
            }
            S.dq[idx] = a; S.dk[idx] = bb; S.dv[idx] = cc;
        }
        __syncthreads();
        for (int idx = t; idx < 96 * dh; idx += 256) {   // d to_qkv rows of this head
            const int which = idx / (32 * dh), rem = idx - which * 32 * dh, d = rem >> 5, cc = rem & 31;
            const float* src = which == 0 ? S.dq : which == 1 ? S.dk : S.dv;
            float s = 0.f;
#pragma unroll
            for (int ii = 0; ii < 8; ++ii) s += src[ii * dh + d] * S.u[ii * 32 + cc];
            P[o.wq + (int64_t)(which * I + h * dh + d) * 32 + cc] = s;
        }
        for (int d = 0; d < dh; ++d) {
            const int64_t r = (int64_t)(h * dh + d) * 32 + c;
            du += S.dq[i * dh + d] * lp[o.wq + r] + S.dk[i * dh + d] * lp[o.wk + r] + S.dv[i * dh + d] * lp[o.wv + r];
        }
        __syncthreads();
    }
    S.stg[t] = du * xh1; S.stg2[t] = du;
    const float dxh = du * lp[o.g1 + c];
    const float m1 = sum32(dxh) * (1.f / 32.f), m2 = sum32(dxh * xh1) * (1.f / 32.f);
    const float dt0 = dt1 + rs1 * (dxh - m1 - xh1 * m2);
    __syncthreads();
    if (t < 32) {
        float a = 0.f, bb = 0.f;
        for (int ii = 0; ii < 8; ++ii) { a += S.stg[ii * 32 + t]; bb += S.stg2[ii * 32 + t]; }
        P[o.g1 + t] = a; P[o.b1 + t] = bb;
    }
    dtok_in[tix] = dt0;
    P[o.size + t] = dt0;
}

void launch_bit_enc_fwd(const float* tok_in, const float* pos, const float* lp, float* tok_out, int B, int dh, hipStream_t s) {
    k_bit_enc<false><<<B, 256, 0, s>>>(tok_in, pos, lp, tok_out, nullptr, nullptr, nullptr, B, dh);
}
int64_t bit_enc_part_floats(int B, int dh) { return (int64_t)B * (bit_off(8 * dh).size + 256); }
void launch_bit_enc_bwd(const float* tok_in, const float* pos, const float* lp, const float* dtok_out, float* dtok_in, float* part,
                        float* g_lp, float* g_pos, int B, int dh, hipStream_t s) {
    const int LS = bit_off(8 * dh).size;
    k_bit_enc<true><<<B, 256, 0, s>>>(tok_in, pos, lp, nullptr, dtok_out, dtok_in, part, B, dh);
    sum_parts(g_lp, 0, part, B, LS + 256, 0, LS, 1, 1, s);
    sum_parts(g_pos, 0, part + LS, B, LS + 256, 0, 256, 1, 1, s);
}

// ------------------------------------------------------------------------------------------------ decoder: fold / unfold
// grid (L, NI), thread (j, c): LN of the image's 4 memory tokens with the layer's norm, K / V per head, A and P (see the header).
// AP [L][NI][A 32x32 | P 32x32]
__global__ void __launch_bounds__(128) k_bit_dec_fold(const float* __restrict__ tok, const float* __restrict__ dp, float* __restrict__ AP,
                                                       int NI, int dh) {
    __shared__ float mh[128], K[256], V[256];
    const int l = blockIdx.x, img = blockIdx.y, t = threadIdx.x, j = t >> 5, c = t & 31, I = 8 * dh;
    const BitOff o = bit_off(I);
    const float* lp = dp + (int64_t)l * o.size;
    const float x = tok[(int64_t)img * 128 + t];
    const float mu = sum32(x) * (1.f / 32.f), d0 = x - mu;
    const float rs = rsqrtf(sum32(d0 * d0) * (1.f / 32.f) + BIT_EPS);
    mh[t] = d0 * rs * lp[o.g1 + c] + lp[o.b1 + c];
    __syncthreads();
    float* out = AP + ((int64_t)l * NI + img) * 2048;
    for (int h = 0; h < 8; ++h) {
        for (int idx = t; idx < 8 * dh; idx += 128) {
            const int which = idx / (4 * dh), rem = idx - which * 4 * dh, jj = rem / dh, d = rem - jj * dh;
            const float* w = lp + (which ? o.wv : o.wk) + (int64_t)(h * dh + d) * 32;
            float s = 0.f;
#pragma unroll
            for (int cc = 0; cc < 32; ++cc) s += mh[jj * 32 + cc] * w[cc];
            (which ? V : K)[jj * dh + d] = s;
        }
        __syncthreads();
        float a = 0.f, p = 0.f;
        for (int d = 0; d < dh; ++d) {
            a += lp[o.wq + (int64_t)(h * dh + d) * 32 + c] * K[j * dh + d];
            p += V[j * dh + d] * lp[o.wo + (int64_t)c * I + h * dh + d];
        }
        out[c * 32 + h * 4 + j] = a * BIT_SCALE;
        out[1024 + (h * 4 + j) * 32 + c] = p;
        __syncthreads();
    }
}

// grid (L, 8 heads), 256 threads; loops over the images in order, the head's slices of dWq / dWk / dWv / dWo in registers (each owned
// by this block alone: plain stores into the gradient buffer).  d(mhat) of (layer, image, head) goes to dmh [L][NI][8][4][32].
__global__ void __launch_bounds__(256) k_bit_dec_unfold(const float* __restrict__ tok, const float* __restrict__ dp, const float* __restrict__ dAP,
                                                         float* __restrict__ gdp, float* __restrict__ dmh, int NI, int dh) {
    __shared__ float mh[128], K[256], V[256], dK[256], dV[256], sA[1024], sP[1024];
    const int l = blockIdx.x, h = blockIdx.y, t = threadIdx.x, I = 8 * dh;
    const BitOff o = bit_off(I);
    const float* lp = dp + (int64_t)l * o.size;
    float* gp = gdp + (int64_t)l * o.size;
    float aq[8], ak[8], av[8], ao[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) aq[r] = ak[r] = av[r] = ao[r] = 0.f;
    for (int img = 0; img < NI; ++img) {
        if (t < 128) {
            const int c = t & 31;
            const float x = tok[(int64_t)img * 128 + t];
            const float mu = sum32(x) * (1.f / 32.f), d0 = x - mu;
            const float rs = rsqrtf(sum32(d0 * d0) * (1.f / 32.f) + BIT_EPS);
            mh[t] = d0 * rs * lp[o.g1 + c] + lp[o.b1 + c];
        }
        const float* ap = dAP + ((int64_t)l * NI + img) * 2048;
        for (int idx = t; idx < 1024; idx += 256) { sA[idx] = ap[idx]; sP[idx] = ap[1024 + idx]; }
        __syncthreads();
        for (int idx = t; idx < 8 * dh; idx += 256) {
            const int which = idx / (4 * dh), rem = idx - which * 4 * dh, jj = rem / dh, d = rem - jj * dh;
            const float* w = lp + (which ? o.wv : o.wk) + (int64_t)(h * dh + d) * 32;
            float s = 0.f;
#pragma unroll
            for (int cc = 0; cc < 32; ++cc) s += mh[jj * 32 + cc] * w[cc];
            (which ? V : K)[jj * dh + d] = s;
        }
        for (int idx = t; idx < 8 * dh; idx += 256) {      // dK[j][d] = s sum_c dA[c][hj] Wq[hd][c];  dV[j][d] = sum_c dP[hj][c] Wo[c][hd]
            const int which = idx / (4 * dh), rem = idx - which * 4 * dh, jj = rem / dh, d = rem - jj * dh;
            float s = 0.f;
            if (which == 0) {
                for (int cc = 0; cc < 32; ++cc) s += sA[cc * 32 + h * 4 + jj] * lp[o.wq + (int64_t)(h * dh + d) * 32 + cc];
                dK[jj * dh + d] = s * BIT_SCALE;
            } else {
                for (int cc = 0; cc < 32; ++cc) s += sP[(h * 4 + jj) * 32 + cc] * lp[o.wo + (int64_t)cc * I + h * dh + d];
                dV[jj * dh + d] = s;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int idx = t + 256 * r;
            if (idx < 32 * dh) {
                {   // [hd][c] order: dWq, dWk, dWv
                    const int d = idx >> 5, cc = idx & 31;
                    float q = 0.f, k = 0.f, v = 0.f;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        q += sA[cc * 32 + h * 4 + jj] * K[jj * dh + d];
                        k += dK[jj * dh + d] * mh[jj * 32 + cc];
                        v += dV[jj * dh + d] * mh[jj * 32 + cc];
                    }
                    aq[r] += q * BIT_SCALE; ak[r] += k; av[r] += v;
                }
                {   // [c][hd] order: dWo
                    const int cc = idx / dh, d = idx - cc * dh;
                    float w = 0.f;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) w += sP[(h * 4 + jj) * 32 + cc] * V[jj * dh + d];
                    ao[r] += w;
                }
            }
        }
        if (t < 128) {
            const int jj = t >> 5, c = t & 31;
            float s = 0.f;
            for (int d = 0; d < dh; ++d) {
                const int64_t r = (int64_t)(h * dh + d) * 32 + c;
                s += dK[jj * dh + d] * lp[o.wk + r] + dV[jj * dh + d] * lp[o.wv + r];
            }
            dmh[(((int64_t)l * NI + img) * 8 + h) * 128 + t] = s;
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int idx = t + 256 * r;
        if (idx < 32 * dh) {
            const int d = idx >> 5, cc = idx & 31;
            const int64_t row = (int64_t)(h * dh + d) * 32 + cc;
            gp[o.wq + row] = aq[r]; gp[o.wk + row] = ak[r]; gp[o.wv + row] = av[r];
            const int c2 = idx / dh, d2 = idx - c2 * dh;
            gp[o.wo + (int64_t)c2 * I + h * dh + d2] = ao[r];
        }
    }
}

// grid L, thread (j, c): per image d(mhat) = sum over the heads, LayerNorm backward -> dm [L][NI][4][32]; the norm's weight / bias
// gradients from the memory side are ADDED to the pixel side's sums already in the gradient buffer (PreNorm2 shares one LayerNorm).
__global__ void __launch_bounds__(128) k_bit_dec_mfinish(const float* __restrict__ tok, const float* __restrict__ dp, const float* __restrict__ dmh,
                                                          float* __restrict__ gdp, float* __restrict__ dm, int NI, int dh) {
    __shared__ float sg[128], sb[128];
    const int l = blockIdx.x, t = threadIdx.x, c = t & 31;
    const BitOff o = bit_off(8 * dh);
    const float* lp = dp + (int64_t)l * o.size;
    float* gp = gdp + (int64_t)l * o.size;
    const float g1 = lp[o.g1 + c];
    float ag = 0.f, ab = 0.f;
    for (int img = 0; img < NI; ++img) {
        const float x = tok[(int64_t)img * 128 + t];
        const float mu = sum32(x) * (1.f / 32.f), d0 = x - mu;
        const float rs = rsqrtf(sum32(d0 * d0) * (1.f / 32.f) + BIT_EPS), xh = d0 * rs;
        float dv = 0.f;
        for (int h = 0; h < 8; ++h) dv += dmh[(((int64_t)l * NI + img) * 8 + h) * 128 + t];
        ag += dv * xh; ab += dv;
        const float dxh = dv * g1;
        const float m1 = sum32(dxh) * (1.f / 32.f), m2 = sum32(dxh * xh) * (1.f / 32.f);
        dm[((int64_t)l * NI + img) * 128 + t] = rs * (dxh - m1 - xh * m2);
    }
    sg[t] = ag; sb[t] = ab;
    __syncthreads();
    if (t < 32) {
        gp[o.g1 + t] += ((sg[t] + sg[32 + t]) + sg[64 + t]) + sg[96 + t];
        gp[o.b1 + t] += ((sb[t] + sb[32 + t]) + sb[64 + t]) + sb[96 + t];
    }
}

void launch_bit_dec_fold(const float* tok, const float* dp, float* AP, int NI, int L, int dh, hipStream_t s) {
    k_bit_dec_fold<<<dim3(L, NI), 128, 0, s>>>(tok, dp, AP, NI, dh);
}

// ------------------------------------------------------------------------------------------------ decoder: pixel rows
// LDS constants of one layer
struct DecC { const float *A, *P, *W1, *W2t, *g1, *b1, *bo, *g2, *b2, *bb1, *bb2; };
__device__ __forceinline__ DecC dec_consts(const float* C) {
    DecC k;
    k.A = C; k.P = C + 1024; k.W1 = C + 2048; k.W2t = C + 4096;
    k.g1 = C + 6144; k.b1 = k.g1 + 32; k.bo = k.b1 + 32; k.g2 = k.bo + 32; k.b2 = k.g2 + 32; k.bb1 = k.b2 + 32; k.bb2 = k.bb1 + 64;
    return k;
}
__device__ __forceinline__ void dec_load_consts(float* C, const float* __restrict__ ap, const float* __restrict__ lp, const BitOff& o, int t, int nt) {
    for (int i = t; i < 2048; i += nt) { C[i] = ap[i]; C[2048 + i] = lp[o.w1 + i]; C[4096 + i] = lp[o.w2 + (i & 31) * 64 + (i >> 5)]; }
    for (int i = t; i < 32; i += nt) {
        C[6144 + i] = lp[o.g1 + i]; C[6176 + i] = lp[o.b1 + i]; C[6208 + i] = lp[o.bo + i]; C[6240 + i] = lp[o.g2 + i]; C[6272 + i] = lp[o.b2 + i];
        C[6304 + i] = lp[o.bb1 + i]; C[6336 + i] = lp[o.bb1 + 32 + i]; C[6368 + i] = lp[o.bb2 + i];
    }
}
// attention half of a layer on one row: xh = LN(x) before the affine, p = the 8 x 4 softmax, y = x + p P + b_o
__device__ __forceinline__ void dec_row_attn(const float (&x)[32], const DecC& k, float (&xh)[32], float& rs, float (&p)[32], float (&y)[32]) {
    float mu = 0.f;
#pragma unroll
    for (int c = 0; c < 32; ++c) mu += x[c];
    mu *= (1.f / 32.f);
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < 32; ++c) { xh[c] = x[c] - mu; var += xh[c] * xh[c]; }
    rs = rsqrtf(var * (1.f / 32.f) + BIT_EPS);
#pragma unroll
    for (int q = 0; q < 32; ++q) p[q] = 0.f;
#pragma unroll
    for (int c = 0; c < 32; ++c) {
        xh[c] *= rs;
        const float u = xh[c] * k.g1[c] + k.b1[c];
#pragma unroll
        for (int q = 0; q < 32; ++q) p[q] += u * k.A[c * 32 + q];
    }
#pragma unroll
    for (int h = 0; h < 8; ++h) {
        const float m = fmaxf(fmaxf(p[4 * h], p[4 * h + 1]), fmaxf(p[4 * h + 2], p[4 * h + 3]));
        float e[4], s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { e[j] = expf(p[4 * h + j] - m); s += e[j]; }
        const float is = 1.f / s;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[4 * h + j] = e[j] * is;
    }
#pragma unroll
    for (int c = 0; c < 32; ++c) y[c] = x[c] + k.bo[c];
#pragma unroll
    for (int q = 0; q < 32; ++q)
#pragma unroll
        for (int c = 0; c < 32; ++c) y[c] += p[q] * k.P[q * 32 + c];
}
// yh = LN(y) before the affine, v = yh g2 + b2
__device__ __forceinline__ void dec_row_ln2(const float (&y)[32], const DecC& k, float (&yh)[32], float& rs, float (&v)[32]) {
    float mu = 0.f;
#pragma unroll
    for (int c = 0; c < 32; ++c) mu += y[c];
    mu *= (1.f / 32.f);
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < 32; ++c) { yh[c] = y[c] - mu; var += yh[c] * yh[c]; }
    rs = rsqrtf(var * (1.f / 32.f) + BIT_EPS);
#pragma unroll
    for (int c = 0; c < 32; ++c) { yh[c] *= rs; v[c] = yh[c] * k.g2[c] + k.b2[c]; }
}

// grid (ceil(n / 256), NI): one thread per pixel row, all L layers; the layer inputs 1 .. L-1 go to xs (training; nullptr: eval), every
// layer boundary is rounded to the storage type so that the backward's recomputation starts from exactly what the forward used.
template <typename T>
__global__ void __launch_bounds__(256) k_bit_dec_fwd(const T* __restrict__ src, T* __restrict__ dst, T* __restrict__ xs, const float* __restrict__ AP,
                                                      const float* __restrict__ dp, int n, int NI, int L, int dh) {
    __shared__ float C[DEC_CONST];
    const int img = blockIdx.y, t = threadIdx.x, row = blockIdx.x * 256 + t;
    const bool valid = row < n;
    const BitOff o = bit_off(8 * dh);
    const DecC k = dec_consts(C);
    const int64_t ro = ((int64_t)img * n + row) * 32;
    float x[32];
    if (valid) load32<T>(src + ro, x);
    else {
#pragma unroll
        for (int c = 0; c < 32; ++c) x[c] = 0.f;
    }
    for (int l = 0; l < L; ++l) {
        __syncthreads();
        dec_load_consts(C, AP + ((int64_t)l * NI + img) * 2048, dp + (int64_t)l * o.size, o, t, 256);
        __syncthreads();
        if (l > 0 && xs && valid) store32<T>(xs + (int64_t)(l - 1) * NI * n * 32 + ro, x);
        float xh[32], p[32], y[32], rs;
        dec_row_attn(x, k, xh, rs, p, y);
        dec_row_ln2(y, k, xh, rs, p);                     // xh: yhat, p: v = LN'(y)
#pragma unroll
        for (int c = 0; c < 32; ++c) x[c] = y[c] + k.bb2[c];
        for (int kk = 0; kk < 64; ++kk) {
            float s = k.bb1[kk];
#pragma unroll
            for (int c = 0; c < 32; ++c) s += p[c] * k.W1[kk * 32 + c];
            const float g = gelu_f(s);
#pragma unroll
            for (int c = 0; c < 32; ++c) x[c] += g * k.W2t[kk * 32 + c];
        }
#pragma unroll
        for (int c = 0; c < 32; ++c) x[c] = round_as<T>(x[c]);
    }
    if (valid) store32<T>(dst + ro, x);
}

// out(a, b0 + j) += sum_r Sa[r][a] * Sb[r][b0 + j], j < 8, over the DEC_BWD_ROWS staged rows
__device__ __forceinline__ void outer8(float (&acc)[8], const float* Sa, const float* Sb, int a, int b0) {
    for (int r = 0; r < DEC_BWD_ROWS; ++r) {
        const float va = Sa[r * STG_LD + a];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += va * Sb[r * STG_LD + b0 + j];
    }
}
__device__ __forceinline__ float colsum32(const float* S, int col, int quarter) {
    float s = 0.f;
    for (int r = quarter * 32; r < quarter * 32 + 32; ++r) s += S[r * STG_LD + col];
    return s;
}
template <typename T>
__device__ __forceinline__ void stage32(float* S, int t, const float (&v)[32]) {
#pragma unroll
    for (int c = 0; c < 32; ++c) S[t * STG_LD + c] = v[c];
}

// grid (nchunk, NI), 128 threads = 128 rows per tile; layers in reverse order, for each layer the block walks its tiles (tile = chunk,
// chunk + nchunk, ...).  The running gradient travels between layers through dG (fp32, [NI][n][32]); the last layer reads ddst, layer 0
// writes dIn.  part [L][NI][nchunk][DEC_PART].
template <typename T>
__global__ void __launch_bounds__(DEC_BWD_ROWS) k_bit_dec_bwd(const T* __restrict__ src, const T* __restrict__ xs, const T* __restrict__ ddst,
                                                               float* __restrict__ dG, T* __restrict__ dIn, const float* __restrict__ AP,
                                                               const float* __restrict__ dp, float* __restrict__ part, int n, int NI, int L, int dh) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* C = smem;
    float* S1 = smem + DEC_CONST;
    float* S2 = S1 + DEC_BWD_ROWS * STG_LD;
    float* S3 = S2 + DEC_BWD_ROWS * STG_LD;
    float* S4 = S3 + DEC_BWD_ROWS * STG_LD;
    const int chunk = blockIdx.x, nchunk = gridDim.x, img = blockIdx.y, t = threadIdx.x;
    const int a = t >> 2, b0 = (t & 3) * 8, col = t & 31, quarter = t >> 5;
    const BitOff o = bit_off(8 * dh);
    const DecC k = dec_consts(C);
    const int ntiles = (n + DEC_BWD_ROWS - 1) / DEC_BWD_ROWS;
    for (int l = L - 1; l >= 0; --l) {
        __syncthreads();
        dec_load_consts(C, AP + ((int64_t)l * NI + img) * 2048, dp + (int64_t)l * o.size, o, t, DEC_BWD_ROWS);
        __syncthreads();
        float accA[8], accP[8], accW1[2][8], accW2[2][8], vb1[2] = {0.f, 0.f}, vbb2 = 0.f, vg2 = 0.f, vb2 = 0.f, vbo = 0.f, vg1 = 0.f, vb1n = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { accA[j] = accP[j] = 0.f; accW1[0][j] = accW1[1][j] = accW2[0][j] = accW2[1][j] = 0.f; }
        const T* xin = l == 0 ? src : xs + (int64_t)(l - 1) * NI * n * 32;
        for (int tile = chunk; tile < ntiles; tile += nchunk) {
            const int row = tile * DEC_BWD_ROWS + t;
            const bool valid = row < n;
            const int64_t ro = ((int64_t)img * n + row) * 32;
            float x[32], dout[32];
            if (valid) {
                load32<T>(xin + ro, x);
                if (l == L - 1) load32<T>(ddst + ro, dout);
                else load32<float>(dG + ro, dout);
            } else {
#pragma unroll
                for (int c = 0; c < 32; ++c) { x[c] = 0.f; dout[c] = 0.f; }
            }
            float xh[32], p[32], y[32], yh[32], v[32], rs1, rs2;
            dec_row_attn(x, k, xh, rs1, p, y);
            dec_row_ln2(y, k, yh, rs2, v);
            // ---- FeedForward backward, hidden units in two halves of 32
            stage32<T>(S3, t, dout);
            stage32<T>(S4, t, v);
            float dv[32];
#pragma unroll
            for (int c = 0; c < 32; ++c) dv[c] = 0.f;
            for (int half = 0; half < 2; ++half) {
                for (int kk = 0; kk < 32; ++kk) {
                    const int kh = half * 32 + kk;
                    float s = k.bb1[kh], dh_ = 0.f;
#pragma unroll
                    for (int c = 0; c < 32; ++c) { s += v[c] * k.W1[kh * 32 + c]; dh_ += dout[c] * k.W2t[kh * 32 + c]; }
                    const float dpre = dh_ * gelu_d(s);
#pragma unroll
                    for (int c = 0; c < 32; ++c) dv[c] += dpre * k.W1[kh * 32 + c];
                    S1[t * STG_LD + kk] = gelu_f(s);
                    S2[t * STG_LD + kk] = dpre;
                }
                __syncthreads();
                outer8(accW2[half], S3, S1, a, b0);        // d net.3.weight [c][k]: a = c, b = k
                outer8(accW1[half], S2, S4, a, b0);        // d net.0.weight [k][c]: a = k, b = c
                vb1[half] += colsum32(S2, col, quarter);
                if (half == 0) vbb2 += colsum32(S3, col, quarter);
                __syncthreads();
            }
            // ---- LayerNorm' backward: dy = dout + ...
            float m1 = 0.f, m2 = 0.f;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                S1[t * STG_LD + c] = dv[c] * yh[c];
                S2[t * STG_LD + c] = dv[c];
                dv[c] *= k.g2[c];
                m1 += dv[c]; m2 += dv[c] * yh[c];
            }
            m1 *= (1.f / 32.f); m2 *= (1.f / 32.f);
#pragma unroll
            for (int c = 0; c < 32; ++c) dout[c] += rs2 * (dv[c] - m1 - yh[c] * m2);      // dout: now dy
            // ---- attention backward
            stage32<T>(S3, t, p);
            stage32<T>(S4, t, dout);
            __syncthreads();
            vg2 += colsum32(S1, col, quarter);
            vb2 += colsum32(S2, col, quarter);
            vbo += colsum32(S4, col, quarter);
            outer8(accP, S3, S4, a, b0);                   // dP [hj][c]
            __syncthreads();
            float dz[32];
#pragma unroll
            for (int q = 0; q < 32; ++q) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 32; ++c) s += dout[c] * k.P[q * 32 + c];
                dz[q] = s;
            }
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                float dot = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) dot += p[4 * h + j] * dz[4 * h + j];
#pragma unroll
                for (int j = 0; j < 4; ++j) dz[4 * h + j] = p[4 * h + j] * (dz[4 * h + j] - dot);
            }
            m1 = 0.f; m2 = 0.f;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                float du = 0.f;
#pragma unroll
                for (int q = 0; q < 32; ++q) du += k.A[c * 32 + q] * dz[q];
                S1[t * STG_LD + c] = xh[c] * k.g1[c] + k.b1[c];          // u
                S2[t * STG_LD + c] = dz[c];
                S3[t * STG_LD + c] = du * xh[c];
                S4[t * STG_LD + c] = du;
                du *= k.g1[c];
                m1 += du; m2 += du * xh[c];
                dv[c] = du;
            }
            m1 *= (1.f / 32.f); m2 *= (1.f / 32.f);
#pragma unroll
            for (int c = 0; c < 32; ++c) dout[c] += rs1 * (dv[c] - m1 - xh[c] * m2);      // dout: now dx
            __syncthreads();
            outer8(accA, S1, S2, a, b0);                   // dA [c][hj]
            vg1 += colsum32(S3, col, quarter);
            vb1n += colsum32(S4, col, quarter);
            if (valid) {
                if (l == 0) store32<T>(dIn + ro, dout);
                else store32<float>(dG + ro, dout);
            }
            __syncthreads();
        }
        // ---- this block's partial sums of layer l
        float* Pp = part + (((int64_t)l * NI + img) * nchunk + chunk) * DEC_PART;
        const int TB = 2112;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            Pp[a * 32 + b0 + j] = accA[j];
            Pp[1024 + a * 32 + b0 + j] = accP[j];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                Pp[TB + 96 + (half * 32 + a) * 32 + b0 + j] = accW1[half][j];
                Pp[TB + 96 + 2048 + 64 + a * 64 + half * 32 + b0 + j] = accW2[half][j];
            }
        }
        // the vector sums: four row quarters per column, added in order
        float* V = S1;
        V[(0 * 4 + quarter) * 32 + col] = vg1;  V[(1 * 4 + quarter) * 32 + col] = vb1n; V[(2 * 4 + quarter) * 32 + col] = vbo;
        V[(3 * 4 + quarter) * 32 + col] = vg2;  V[(4 * 4 + quarter) * 32 + col] = vb2;  V[(5 * 4 + quarter) * 32 + col] = vb1[0];
        V[(6 * 4 + quarter) * 32 + col] = vb1[1]; V[(7 * 4 + quarter) * 32 + col] = vbb2;
        __syncthreads();
        if (t < 32) {
            float s[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) s[q] = ((V[(q * 4) * 32 + t] + V[(q * 4 + 1) * 32 + t]) + V[(q * 4 + 2) * 32 + t]) + V[(q * 4 + 3) * 32 + t];
            Pp[2048 + t] = s[0]; Pp[2080 + t] = s[1];
            Pp[TB + t] = s[2]; Pp[TB + 32 + t] = s[3]; Pp[TB + 64 + t] = s[4];
            Pp[TB + 96 + 2048 + t] = s[5]; Pp[TB + 96 + 2048 + 32 + t] = s[6];
            Pp[TB + 96 + 2048 + 64 + 2048 + t] = s[7];
        }
    }
}

void launch_bit_dec_fwd(int dt, const void* src, void* dst, void* xs, const float* AP, const float* dp, int n, int NI, int L, int dh, hipStream_t s) {
    const dim3 grid((n + 255) / 256, NI);
    if (dt == BF16) k_bit_dec_fwd<bf16><<<grid, 256, 0, s>>>((const bf16*)src, (bf16*)dst, (bf16*)xs, AP, dp, n, NI, L, dh);
    else k_bit_dec_fwd<float><<<grid, 256, 0, s>>>((const float*)src, (float*)dst, (float*)xs, AP, dp, n, NI, L, dh);
}
int bit_dec_chunks(int n) { const int tiles = (n + DEC_BWD_ROWS - 1) / DEC_BWD_ROWS; return tiles < 8 ? tiles : 8; }
int64_t bit_dec_part_floats(int n, int NI, int L) { return (int64_t)L * NI * bit_dec_chunks(n) * DEC_PART; }
// returns non-zero (error set) when the kernel's dynamic LDS cannot be granted or the launch fails
int launch_bit_dec_bwd(int dt, const void* src, const void* xs, const void* ddst, float* dG, void* dIn, const float* AP, const float* dp,
                        float* part, int n, int NI, int L, int dh, hipStream_t s) {
    const int lds = (DEC_CONST + 4 * DEC_BWD_ROWS * STG_LD) * 4;
    // per call: the attribute belongs to the current device's copy of the kernel (a table look-up on the host, no device work)
    const dim3 grid(bit_dec_chunks(n), NI);
    if (dt == BF16) {
        STCD_HIP(hipFuncSetAttribute((const void*)k_bit_dec_bwd<bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        k_bit_dec_bwd<bf16><<<grid, DEC_BWD_ROWS, lds, s>>>((const bf16*)src, (const bf16*)xs, (const bf16*)ddst, dG, (bf16*)dIn, AP, dp, part, n, NI, L, dh);
    } else {
        STCD_HIP(hipFuncSetAttribute((const void*)k_bit_dec_bwd<float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        k_bit_dec_bwd<float><<<grid, DEC_BWD_ROWS, lds, s>>>((const float*)src, (const float*)xs, (const float*)ddst, dG, (float*)dIn, AP, dp, part, n, NI, L, dh);
    }
    STCD_HIP(hipGetLastError());
    return 0;
}
// after launch_bit_dec_bwd: sums the partials (dAP [L][NI][2048]; norm / to_out bias / FeedForward gradients into gdp), unfolds dA, dP
// into the projection gradients and d(memory) (dmh, dm: scratch), dtok [NI][4][32] = sum over the layers of dm
void launch_bit_dec_finish(const float* part, float* dAP, const float* tok, const float* dp, float* gdp, float* dmh, float* dm, float* dtok,
                           int n, int NI, int L, int dh, hipStream_t s) {
    const int nc = bit_dec_chunks(n);
    const BitOff o = bit_off(8 * dh);
    sum_parts(dAP, 2048, part, nc, DEC_PART, (int64_t)nc * DEC_PART, 2048, L * NI, 0, s);
    sum_parts(gdp, o.size, part + 2048, NI * nc, DEC_PART, (int64_t)NI * nc * DEC_PART, 64, L, 1, s);
    sum_parts(gdp + o.bo, o.size, part + 2112, NI * nc, DEC_PART, (int64_t)NI * nc * DEC_PART, 4288, L, 1, s);
    k_bit_dec_unfold<<<dim3(L, 8), 256, 0, s>>>(tok, dp, dAP, gdp, dmh, NI, dh);
    k_bit_dec_mfinish<<<L, 128, 0, s>>>(tok, dp, dmh, gdp, dm, NI, dh);
    sum_parts(dtok, 0, dm, L, (int64_t)NI * 128, 0, NI * 128, 1, 0, s);
}

}  // namespace stcd
