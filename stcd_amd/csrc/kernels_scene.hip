// kernels_scene.hip -- whole-scene inference around the eval forward: tile gather, overlap stitch, finalize (gfx950).
//
// What these replace in the reference (semantics, not code):
//   offline 256-pixel crops of a scene           /root/reference/split.py:17-46
//   ToTensor + Normalize on the host             /root/reference/data/dataset.py:499-500
//   arg-max / threshold of the prediction        /root/reference/models/trainer.py:197-203
//   SegmentationMetric.genConfusionMatrix        /root/reference/train_pse_cd.py:361-368
// The reference never puts the crops back together, so the overlap blend (window weights, ascending tile order) is this
// library's own specification; tests/scene_spec.py restates it in numpy.
//
// The tile grid is regular: tile k = (ky, kx) = (k / tiles_x, k % tiles_x) has origin (ky * S, kx * S).  All three
// kernels are memory-bound and follow kernels_ew.hip: one thread owns 4 consecutive x positions, the fp32 side moves in
// 16-byte loads and stores whenever the row pitch allows it, pixel indices are 64-bit.  The stitch is a GATHER over scene
// pixels: a thread adds the tiles that cover its pixels in ascending tile index, so there are no float atomics, the bits
// do not depend on the run, and splitting the tiles into calls (in ascending order) continues the same chain of fmaf.
#include <algorithm>

#include "common.h"

namespace stcd {

#define SCENE_MAX_BLOCKS 2048      // grid-stride above this: 8 blocks per CU

// mirror reflection without repeating the edge sample (numpy 'reflect'): period 2 (L - 1)
__device__ __forceinline__ int64_t scene_reflect(int64_t i, int64_t L) {
    if (L == 1) return 0;
    const int64_t m = 2 * (L - 1);
    i = ((i % m) + m) % m;
    return i >= L ? m - i : i;
}

// 4 consecutive HWC pixels (12 bytes) of one scene row -> u[3 * j + c] as floats; three dword loads when the address allows it
__device__ __forceinline__ void scene_load12(const uint8_t* __restrict__ p, float (&u)[12]) {
    if (((uintptr_t)p & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            u[b] = (float)((w0 >> (8 * b)) & 255u);
            u[4 + b] = (float)((w1 >> (8 * b)) & 255u);
            u[8 + b] = (float)((w2 >> (8 * b)) & 255u);
        }
    } else {
#pragma unroll
        for (int b = 0; b < 12; ++b) u[b] = (float)p[b];
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256)
k_scene_gather(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, int H, int W, int T, int S, int tiles_x, int first_tile,
               int gpr, int64_t total, float m0, float m1, float m2, float is0, float is1, float is2, float* __restrict__ x1,
               float* __restrict__ x2) {
    const float mean[3] = {m0, m1, m2}, istd[3] = {is0, is1, is2};
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int xg = (int)(g % gpr);
        const int64_t r = g / gpr;
        const int ty = (int)(r % T);
        const int64_t n = r / T;
        const int64_t k = first_tile + n;
        const int64_t ky = k / tiles_x, kx = k - ky * tiles_x;
        const int tx0 = xg * 4;
        const int64_t y = scene_reflect(ky * S + ty, H), gx0 = kx * S + tx0;
        const uint8_t* ra = A + y * W * 3;
        const uint8_t* rb = B + y * W * 3;
        float ua[12], ub[12];
        if (gx0 + 3 < W) {                                            // four scene pixels in a row: no reflection along x
            scene_load12(ra + gx0 * 3, ua);
            scene_load12(rb + gx0 * 3, ub);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t x = scene_reflect(gx0 + j, W);
#pragma unroll
                for (int c = 0; c < 3; ++c) { ua[3 * j + c] = (float)ra[x * 3 + c]; ub[3 * j + c] = (float)rb[x * 3 + c]; }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float va[4], vb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                             // k_pseudo_pair's arithmetic, to the operation
                va[j] = (ua[3 * j + c] * (1.f / 255.f) - mean[c]) * istd[c];
                vb[j] = (ub[3 * j + c] * (1.f / 255.f) - mean[c]) * istd[c];
            }
            const int64_t o = ((n * 3 + c) * T + ty) * T + tx0;
            if (VEC) {
                *reinterpret_cast<float4*>(x1 + o) = make_float4(va[0], va[1], va[2], va[3]);
                *reinterpret_cast<float4*>(x2 + o) = make_float4(vb[0], vb[1], vb[2], vb[3]);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (tx0 + j < T) { x1[o + j] = va[j]; x2[o + j] = vb[j]; }
            }
        }
    }
}

static inline unsigned scene_blocks(int64_t threads) { return (unsigned)std::min<int64_t>(SCENE_MAX_BLOCKS, (threads + 255) / 256); }
static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

void launch_scene_gather(const uint8_t* A, const uint8_t* B, int H, int W, int T, int S, int tiles_x, int first_tile, int n_tiles,
                         const float* mean, const float* std_, float* x1, float* x2, hipStream_t s) {
    const int gpr = (T + 3) / 4;
    const int64_t total = (int64_t)n_tiles * T * gpr;
    if (total == 0) return;
    const float is0 = 1.f / std_[0], is1 = 1.f / std_[1], is2 = 1.f / std_[2];
    if (T % 4 == 0 && aligned_to(x1, 16) && aligned_to(x2, 16))
        k_scene_gather<true><<<scene_blocks(total), 256, 0, s>>>(A, B, H, W, T, S, tiles_x, first_tile, gpr, total, mean[0], mean[1], mean[2],
                                                                 is0, is1, is2, x1, x2);
    else
        k_scene_gather<false><<<scene_blocks(total), 256, 0, s>>>(A, B, H, W, T, S, tiles_x, first_tile, gpr, total, mean[0], mean[1], mean[2],
                                                                  is0, is1, is2, x1, x2);
}

// ------------------------------------------------------------------ stitch: acc += w * logit, wsum += w, per scene pixel
// The launch covers the rectangle [y0, y0 + rows) x [x0, x0 + 4 * gpr) of the scene that this call's tiles can reach (x0 a
// multiple of 4).  Tiles covering row y: ky * S <= y < ky * S + T, i.e. ky in [y < T ? 0 : (y - T) / S + 1, min(y / S, tiles_y - 1)];
// likewise along x.  A thread walks ky then kx upwards, which is ascending tile index for each of its four pixels.
template <int CLS>
__global__ void __launch_bounds__(256)
k_scene_stitch(const float* __restrict__ logits, int H, int W, int T, int S, int tiles_x, int tiles_y, int64_t first_tile, int64_t n_tiles,
               const float* __restrict__ window, float* __restrict__ acc, float* __restrict__ wsum, int y0, int x0, int gpr, int64_t total,
               int vec_l, int vec_a) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int xs = x0 + (int)(g % gpr) * 4;
        const int y = y0 + (int)(g / gpr);
        if (xs >= W) continue;
        const int xe = min(xs + 3, W - 1);
        const int ky_lo = y < T ? 0 : (y - T) / S + 1, ky_hi = min(y / S, tiles_y - 1);
        const int kx_lo = xs < T ? 0 : (xs - T) / S + 1, kx_hi = min(xe / S, tiles_x - 1);
        const int64_t pix = (int64_t)y * W + xs;
        float a[CLS][4], ws[4];
        bool touched = false;
        for (int ky = ky_lo; ky <= ky_hi; ++ky) {
            const int ty = y - ky * S;
            const float wy = window ? window[ty] : 1.f;
            for (int kx = kx_lo; kx <= kx_hi; ++kx) {
                const int64_t k = (int64_t)ky * tiles_x + kx - first_tile;
                if (k < 0 || k >= n_tiles) continue;                  // another call's tile
                if (!touched) {                                       // the chain continues from what earlier calls left
                    touched = true;
                    if (vec_a) {
                        const float4 w4 = *reinterpret_cast<const float4*>(wsum + pix);
                        ws[0] = w4.x; ws[1] = w4.y; ws[2] = w4.z; ws[3] = w4.w;
#pragma unroll
                        for (int c = 0; c < CLS; ++c) {
                            const float4 a4 = *reinterpret_cast<const float4*>(acc + c * HW + pix);
                            a[c][0] = a4.x; a[c][1] = a4.y; a[c][2] = a4.z; a[c][3] = a4.w;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool ok = xs + j < W;
                            ws[j] = ok ? wsum[pix + j] : 0.f;
#pragma unroll
                            for (int c = 0; c < CLS; ++c) a[c][j] = ok ? acc[c * HW + pix + j] : 0.f;
                        }
                    }
                }
                const int tx0 = xs - kx * S;
                const float* lp = logits + (k * CLS * T + ty) * T;    // class 0 row of this tile; class c is c * T * T further
                if (vec_l && tx0 >= 0 && tx0 + 3 < T) {               // xs, S and T are multiples of 4 here, so tx0 is one too
                    float wx[4] = {1.f, 1.f, 1.f, 1.f};
                    if (window) {
                        const float4 w4 = *reinterpret_cast<const float4*>(window + tx0);
                        wx[0] = w4.x; wx[1] = w4.y; wx[2] = w4.z; wx[3] = w4.w;
                    }
                    float l[CLS][4];
#pragma unroll
                    for (int c = 0; c < CLS; ++c) {
                        const float4 l4 = *reinterpret_cast<const float4*>(lp + (int64_t)c * T * T + tx0);
                        l[c][0] = l4.x; l[c][1] = l4.y; l[c][2] = l4.z; l[c][3] = l4.w;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float w = wy * wx[j];
#pragma unroll
                        for (int c = 0; c < CLS; ++c) a[c][j] = fmaf(w, l[c][j], a[c][j]);
                        ws[j] += w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int tx = tx0 + j;
                        if (tx < 0 || tx >= T || xs + j >= W) continue;
                        const float w = wy * (window ? window[tx] : 1.f);
#pragma unroll
                        for (int c = 0; c < CLS; ++c) a[c][j] = fmaf(w, lp[(int64_t)c * T * T + tx], a[c][j]);
                        ws[j] += w;
                    }
                }
            }
        }
        if (!touched) continue;
        if (vec_a) {
            *reinterpret_cast<float4*>(wsum + pix) = make_float4(ws[0], ws[1], ws[2], ws[3]);
#pragma unroll
            for (int c = 0; c < CLS; ++c) *reinterpret_cast<float4*>(acc + c * HW + pix) = make_float4(a[c][0], a[c][1], a[c][2], a[c][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (xs + j >= W) continue;
                wsum[pix + j] = ws[j];
#pragma unroll
                for (int c = 0; c < CLS; ++c) acc[c * HW + pix + j] = a[c][j];
            }
        }
    }
}

void launch_scene_stitch(const float* logits, int classes, int H, int W, int T, int S, int tiles_x, int tiles_y, int first_tile, int n_tiles,
                         const float* window, float* acc, float* wsum, hipStream_t s) {
    if (n_tiles == 0) return;
    const int last = first_tile + n_tiles - 1;
    const int ky0 = first_tile / tiles_x, ky1 = last / tiles_x;
    const int y0 = ky0 * S, y1 = (int)std::min<int64_t>(H, (int64_t)ky1 * S + T);
    int x0 = 0, x1 = W;
    if (ky0 == ky1) {                                                 // one tile row: only the columns its tiles reach
        x0 = ((first_tile % tiles_x) * S) & ~3;
        x1 = (int)std::min<int64_t>(W, (int64_t)(last % tiles_x) * S + T);
    }
    const int gpr = (x1 - x0 + 3) / 4;
    const int64_t total = (int64_t)(y1 - y0) * gpr;
    if (total <= 0) return;
    const int vec_l = T % 4 == 0 && S % 4 == 0 && aligned_to(logits, 16) && (!window || aligned_to(window, 16));
    const int vec_a = W % 4 == 0 && aligned_to(acc, 16) && aligned_to(wsum, 16);
    if (classes == 2)
        k_scene_stitch<2><<<scene_blocks(total), 256, 0, s>>>(logits, H, W, T, S, tiles_x, tiles_y, first_tile, n_tiles, window, acc, wsum, y0, x0,
                                                              gpr, total, vec_l, vec_a);
    else
        k_scene_stitch<1><<<scene_blocks(total), 256, 0, s>>>(logits, H, W, T, S, tiles_x, tiles_y, first_tile, n_tiles, window, acc, wsum, y0, x0,
                                                              gpr, total, vec_l, vec_a);
}

// ------------------------------------------------------------------ finalize: mask, optional probability, optional confusion matrix
template <int CLS>
__global__ void __launch_bounds__(256)
k_scene_finalize(const float* __restrict__ acc, const float* __restrict__ wsum, int H, int W, float threshold, const uint8_t* __restrict__ label,
                 uint8_t* __restrict__ mask, float* __restrict__ prob, unsigned long long* __restrict__ cm, int gpr, int64_t total, int vec) {
    __shared__ unsigned int bins[4];
    if (threadIdx.x < 4) bins[threadIdx.x] = 0;
    __syncthreads();
    unsigned int loc[4] = {0, 0, 0, 0};
    const int64_t HW = (int64_t)H * W;
    const bool need_ws = CLS == 1 || prob != nullptr;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int xs = (int)(g % gpr) * 4;
        const int64_t pix = (g / gpr) * W + xs;
        float a[CLS][4], ws[4] = {1.f, 1.f, 1.f, 1.f};
        uint8_t lab[4] = {255, 255, 255, 255};
        if (vec) {
#pragma unroll
            for (int c = 0; c < CLS; ++c) {
                const float4 a4 = *reinterpret_cast<const float4*>(acc + c * HW + pix);
                a[c][0] = a4.x; a[c][1] = a4.y; a[c][2] = a4.z; a[c][3] = a4.w;
            }
            if (need_ws) {
                const float4 w4 = *reinterpret_cast<const float4*>(wsum + pix);
                ws[0] = w4.x; ws[1] = w4.y; ws[2] = w4.z; ws[3] = w4.w;
            }
            if (label) {
                const uint32_t l4 = *reinterpret_cast<const uint32_t*>(label + pix);
#pragma unroll
                for (int j = 0; j < 4; ++j) lab[j] = (uint8_t)(l4 >> (8 * j));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = xs + j < W;
#pragma unroll
                for (int c = 0; c < CLS; ++c) a[c][j] = ok ? acc[c * HW + pix + j] : 0.f;
                if (need_ws && ok) ws[j] = wsum[pix + j];
                if (label && ok) lab[j] = label[pix + j];
            }
        }
        uint8_t pr[4];
        float pb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // a tie is class 0 (torch.argmax takes the first maximum); one class: strictly above threshold * wsum
            pr[j] = CLS == 2 ? (a[CLS - 1][j] > a[0][j]) : (a[0][j] > threshold * ws[j]);
            if (prob) {                                               // softmax class 1 == sigmoid of the logit difference
                const float d = (CLS == 2 ? a[CLS - 1][j] - a[0][j] : a[0][j]) / ws[j];
                pb[j] = 1.f / (1.f + expf(-d));
            }
            if (lab[j] != 255) loc[2 * (lab[j] >= 1) + pr[j]]++;      // lanes past the row end carry 255
        }
        if (vec) {
            *reinterpret_cast<uint32_t*>(mask + pix) = (uint32_t)pr[0] | ((uint32_t)pr[1] << 8) | ((uint32_t)pr[2] << 16) | ((uint32_t)pr[3] << 24);
            if (prob) *reinterpret_cast<float4*>(prob + pix) = make_float4(pb[0], pb[1], pb[2], pb[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (xs + j >= W) continue;
                mask[pix + j] = pr[j];
                if (prob) prob[pix + j] = pb[j];
            }
        }
    }
    if (!cm) return;                                                  // uniform: no thread skips the barrier alone
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned int v = loc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&bins[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 4 && bins[threadIdx.x]) atomicAdd(cm + threadIdx.x, (unsigned long long)bins[threadIdx.x]);
}

void launch_scene_finalize(const float* acc, const float* wsum, int classes, int H, int W, float threshold, const uint8_t* label,
                           uint8_t* mask, float* prob, int64_t* cm, hipStream_t s) {
    const int gpr = (W + 3) / 4;
    const int64_t total = (int64_t)H * gpr;
    const int vec = W % 4 == 0 && aligned_to(acc, 16) && aligned_to(wsum, 16) && aligned_to(mask, 4) && (!label || aligned_to(label, 4)) &&
                    (!prob || aligned_to(prob, 16));
    // a block keeps its counts in 32 bits: 2048 blocks of 256 threads over a 5 x 10^8-pixel strip see 10^6 pixels each
    const uint8_t* lab = label;
    unsigned long long* cmu = (unsigned long long*)cm;                // label and cm come together (checked by the caller)
    if (classes == 2)
        k_scene_finalize<2><<<scene_blocks(total), 256, 0, s>>>(acc, wsum, H, W, threshold, lab, mask, prob, cmu, gpr, total, vec);
    else
        k_scene_finalize<1><<<scene_blocks(total), 256, 0, s>>>(acc, wsum, H, W, threshold, lab, mask, prob, cmu, gpr, total, vec);
}

}  // namespace stcd
