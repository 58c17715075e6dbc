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
//
// The D4 views (stcd_scene_gather_d4 / stcd_scene_stitch_d4; d4 bit 0 mirrors columns, bit 1 mirrors rows, bit 2 transposes, the
// transpose last): the gather writes view d4 of each tile, the stitch reads logits that are in view d4 through the inverse, and
// weights, tile order and the fmaf chain stay in upright coordinates, so more views are more links in the same chain.  The mirror
// views (1..3) are the upright kernels with the 4-pixel group reversed in registers (template MIR; MIR == 0 is the upright code).
// The transposing views (4..7) go through LDS so that both global sides run along their own fast axis: k_scene_gather_t stages a
// 64 x 64 patch of scene rows and writes tile rows whose fast axis is the scene's y; k_scene_stitch_t owns a 64 x 64 scene patch
// and, per covering tile, stages the logit sub-block with lanes along the logits' fast axis and reads it back transposed.
//
// One scene and several heads (stcd_scene_gather_one_d4 / stcd_scene_stitch_heads_d4 / stcd_scene_finalize_seg; UnetSeg takes one
// image, train_sup.py:303, and SegCD's forward returns (mask_t1, mask_t2, change), decoders/unet/model.py:316-332): the gather kernels
// with the second scene compiled out (template PAIR), the stitch kernels with NH heads per launch (NH == 1 is the single-head entry:
// one code, so the same bits per head by construction), and a finalize of the three heads in one pass that also forms the gate of
// train_stcd.py:170-176.
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

// MIR: bit 0 mirrors the tile's columns, bit 1 its rows (d4 in 0..3); the values are those of MIR == 0, only the address moves.
// PAIR == false is stcd_scene_gather_one_d4: B and x2 are not touched, x1 is the same code and so the same bits
template <bool VEC, int MIR, bool PAIR>
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
        const uint8_t* rb = PAIR ? B + y * W * 3 : ra;
        float ua[12], ub[12] = {};
        if (gx0 + 3 < W) {                                            // four scene pixels in a row: no reflection along x
            scene_load12(ra + gx0 * 3, ua);
            if (PAIR) scene_load12(rb + gx0 * 3, ub);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t x = scene_reflect(gx0 + j, W);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    ua[3 * j + c] = (float)ra[x * 3 + c];
                    if (PAIR) ub[3 * j + c] = (float)rb[x * 3 + c];
                }
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
            if (MIR == 0) {
                const int64_t o = ((n * 3 + c) * T + ty) * T + tx0;
                if (VEC) {
                    *reinterpret_cast<float4*>(x1 + o) = make_float4(va[0], va[1], va[2], va[3]);
                    if (PAIR) *reinterpret_cast<float4*>(x2 + o) = make_float4(vb[0], vb[1], vb[2], vb[3]);
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (tx0 + j < T) { x1[o + j] = va[j]; if (PAIR) x2[o + j] = vb[j]; }
                }
            } else {
                const int64_t o = ((n * 3 + c) * T + ((MIR & 2) ? T - 1 - ty : ty)) * T;
                if (VEC && (MIR & 1)) {                               // T % 4 == 0: the mirrored group starts at a multiple of 4
                    *reinterpret_cast<float4*>(x1 + o + (T - 4 - tx0)) = make_float4(va[3], va[2], va[1], va[0]);
                    if (PAIR) *reinterpret_cast<float4*>(x2 + o + (T - 4 - tx0)) = make_float4(vb[3], vb[2], vb[1], vb[0]);
                } else if (VEC) {
                    *reinterpret_cast<float4*>(x1 + o + tx0) = make_float4(va[0], va[1], va[2], va[3]);
                    if (PAIR) *reinterpret_cast<float4*>(x2 + o + tx0) = make_float4(vb[0], vb[1], vb[2], vb[3]);
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (tx0 + j < T) {
                            const int ox = (MIR & 1) ? T - 1 - tx0 - j : tx0 + j;
                            x1[o + ox] = va[j]; if (PAIR) x2[o + ox] = vb[j];
                        }
                }
            }
        }
    }
}

// ---- transposing views of the gather (d4 & 4): Xd[c,i,j] = X[c,p,q] with p = (d4 & 2) ? T-1-j : j, q = (d4 & 1) ? T-1-i : i.
// A block owns the upright patch [p0, p0 + 64) x [q0, q0 + 64) of one tile.  Staging: a thread reads 4 consecutive scene pixels
// of one row (scene_load12's three dwords when the address allows it) and keeps them as bytes, rows of 64 * 3 bytes at a pitch of
// 49 dwords.  Writing: 16 lanes cover 64 consecutive j of one output row i (256 contiguous bytes), each lane converting the four
// bytes of its four p with the upright kernel's arithmetic.
#define SCENE_PATCH 64
#define SCENE_GPITCH 49            // dwords per staged row: 48 hold the 192 bytes, + 1 makes the pitch odd

// the 12 bytes of 4 consecutive tile pixels starting at scene column gx0 (reflected past the right edge) as three little-endian dwords
__device__ __forceinline__ void scene_load12_raw(const uint8_t* __restrict__ row, int64_t gx0, int W, uint32_t* __restrict__ w) {
    const uint8_t* p = row + gx0 * 3;
    if (gx0 + 3 < W && ((uintptr_t)p & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
        return;
    }
    uint32_t v[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t x = gx0 + 3 < W ? gx0 + j : scene_reflect(gx0 + j, W);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[(3 * j + c) >> 2] |= (uint32_t)row[x * 3 + c] << (8 * ((3 * j + c) & 3));
    }
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2];
}

template <bool VEC, bool PAIR>
__global__ void __launch_bounds__(256)
k_scene_gather_t(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, int H, int W, int T, int S, int tiles_x, int first_tile,
                 int ppa, int64_t n_patches, int d4, float m0, float m1, float m2, float is0, float is1, float is2, float* __restrict__ x1,
                 float* __restrict__ x2) {
    __shared__ uint32_t lds[PAIR ? 2 : 1][SCENE_PATCH][SCENE_GPITCH];  // B's plane is lds[PAIR]: no index past the end when it is absent
    const float mean[3] = {m0, m1, m2}, istd[3] = {is0, is1, is2};
    const int t4 = (threadIdx.x & 15) * 4, tr = threadIdx.x >> 4;
    for (int64_t blk = blockIdx.x; blk < n_patches; blk += gridDim.x) {   // uniform per block: the barriers are safe
        const int q0 = (int)(blk % ppa) * SCENE_PATCH;
        const int64_t r = blk / ppa;
        const int p0 = (int)(r % ppa) * SCENE_PATCH;
        const int64_t n = r / ppa;
        const int64_t k = first_tile + n;
        const int64_t ky = k / tiles_x, kx = k - ky * tiles_x;
        const int pn = min(SCENE_PATCH, T - p0), qn = min(SCENE_PATCH, T - q0);
        __syncthreads();                                              // the previous patch has been read
        if (t4 < qn)
            for (int pl = tr; pl < pn; pl += 16) {
                const int64_t y = scene_reflect(ky * S + p0 + pl, H), gx0 = kx * S + q0 + t4;
                scene_load12_raw(A + y * W * 3, gx0, W, &lds[0][pl][3 * (t4 >> 2)]);
                if (PAIR) scene_load12_raw(B + y * W * 3, gx0, W, &lds[PAIR][pl][3 * (t4 >> 2)]);
            }
        __syncthreads();
        if (t4 >= pn) continue;                                       // no barrier below
        const int jb = (d4 & 2) ? T - p0 - pn : p0, ib = (d4 & 1) ? T - q0 - qn : q0;   // where the patch lands in the view
        for (int il = tr; il < qn; il += 16) {
            const int ql = (d4 & 1) ? qn - 1 - il : il;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float va[4], vb[4] = {};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int pl = min(t4 + j, pn - 1);               // past the patch (T % 4 != 0): computed, not stored
                    const int ps = (d4 & 2) ? pn - 1 - pl : pl;
                    const float ua = (float)reinterpret_cast<const uint8_t*>(&lds[0][ps][0])[ql * 3 + c];
                    va[j] = (ua * (1.f / 255.f) - mean[c]) * istd[c];  // k_scene_gather's arithmetic, to the operation
                    if (PAIR) {
                        const float ub = (float)reinterpret_cast<const uint8_t*>(&lds[PAIR][ps][0])[ql * 3 + c];
                        vb[j] = (ub * (1.f / 255.f) - mean[c]) * istd[c];
                    }
                }
                const int64_t o = ((n * 3 + c) * T + ib + il) * T + jb + t4;
                if (VEC) {                                            // T % 4 == 0: pn and jb are multiples of 4
                    *reinterpret_cast<float4*>(x1 + o) = make_float4(va[0], va[1], va[2], va[3]);
                    if (PAIR) *reinterpret_cast<float4*>(x2 + o) = make_float4(vb[0], vb[1], vb[2], vb[3]);
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (t4 + j < pn) { x1[o + j] = va[j]; if (PAIR) x2[o + j] = vb[j]; }
                }
            }
        }
    }
}

static inline unsigned scene_blocks(int64_t threads) { return (unsigned)std::min<int64_t>(SCENE_MAX_BLOCKS, (threads + 255) / 256); }
static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <int MIR, bool PAIR>
static void scene_gather_rows(const uint8_t* A, const uint8_t* B, int H, int W, int T, int S, int tiles_x, int first_tile, int n_tiles,
                              const float* mean, const float* std_, float* x1, float* x2, hipStream_t s) {
    const int gpr = (T + 3) / 4;
    const int64_t total = (int64_t)n_tiles * T * gpr;
    const float is0 = 1.f / std_[0], is1 = 1.f / std_[1], is2 = 1.f / std_[2];
    if (T % 4 == 0 && aligned_to(x1, 16) && aligned_to(x2, 16))
        k_scene_gather<true, MIR, PAIR><<<scene_blocks(total), 256, 0, s>>>(A, B, H, W, T, S, tiles_x, first_tile, gpr, total, mean[0],
                                                                            mean[1], mean[2], is0, is1, is2, x1, x2);
    else
        k_scene_gather<false, MIR, PAIR><<<scene_blocks(total), 256, 0, s>>>(A, B, H, W, T, S, tiles_x, first_tile, gpr, total, mean[0],
                                                                             mean[1], mean[2], is0, is1, is2, x1, x2);
}

// PAIR == false (stcd_scene_gather_one_d4): B and x2 are NULL, which counts as aligned
template <bool PAIR>
static void scene_gather_d4(const uint8_t* A, const uint8_t* B, int H, int W, int T, int S, int tiles_x, int first_tile, int n_tiles,
                            const float* mean, const float* std_, float* x1, float* x2, int d4, hipStream_t s) {
    if (n_tiles == 0) return;
    if (d4 & 4) {
        const int ppa = (T + SCENE_PATCH - 1) / SCENE_PATCH;
        const int64_t n_patches = (int64_t)n_tiles * ppa * ppa;
        const unsigned blocks = (unsigned)std::min<int64_t>(SCENE_MAX_BLOCKS, n_patches);
        const float is0 = 1.f / std_[0], is1 = 1.f / std_[1], is2 = 1.f / std_[2];
        if (T % 4 == 0 && aligned_to(x1, 16) && aligned_to(x2, 16))
            k_scene_gather_t<true, PAIR><<<blocks, 256, 0, s>>>(A, B, H, W, T, S, tiles_x, first_tile, ppa, n_patches, d4, mean[0], mean[1],
                                                               mean[2], is0, is1, is2, x1, x2);
        else
            k_scene_gather_t<false, PAIR><<<blocks, 256, 0, s>>>(A, B, H, W, T, S, tiles_x, first_tile, ppa, n_patches, d4, mean[0], mean[1],
                                                                mean[2], is0, is1, is2, x1, x2);
        return;
    }
    switch (d4) {
        case 0: scene_gather_rows<0, PAIR>(A, B, H, W, T, S, tiles_x, first_tile, n_tiles, mean, std_, x1, x2, s); break;
        case 1: scene_gather_rows<1, PAIR>(A, B, H, W, T, S, tiles_x, first_tile, n_tiles, mean, std_, x1, x2, s); break;
        case 2: scene_gather_rows<2, PAIR>(A, B, H, W, T, S, tiles_x, first_tile, n_tiles, mean, std_, x1, x2, s); break;
        default: scene_gather_rows<3, PAIR>(A, B, H, W, T, S, tiles_x, first_tile, n_tiles, mean, std_, x1, x2, s); break;
    }
}

// B == NULL (and then x2 == NULL) is the one-scene gather
void launch_scene_gather_d4(const uint8_t* A, const uint8_t* B, int H, int W, int T, int S, int tiles_x, int first_tile, int n_tiles,
                            const float* mean, const float* std_, float* x1, float* x2, int d4, hipStream_t s) {
    if (B)
        scene_gather_d4<true>(A, B, H, W, T, S, tiles_x, first_tile, n_tiles, mean, std_, x1, x2, d4, s);
    else
        scene_gather_d4<false>(A, nullptr, H, W, T, S, tiles_x, first_tile, n_tiles, mean, std_, x1, nullptr, d4, s);
}

// ------------------------------------------------------------------ stitch: acc += w * logit, wsum += w, per scene pixel
// The launch covers the rectangle [y0, y0 + rows) x [x0, x0 + 4 * gpr) of the scene that this call's tiles can reach (x0 a
// multiple of 4).  Tiles covering row y: ky * S <= y < ky * S + T, i.e. ky in [y < T ? 0 : (y - T) / S + 1, min(y / S, tiles_y - 1)];
// likewise along x.  A thread walks ky then kx upwards, which is ascending tile index for each of its four pixels.
// MIR as in k_scene_gather: the logits are in view MIR of the tile, weights and order stay upright.
// wsum takes the weight as ONE fused multiply-add, wsum = fmaf(window[ty], window[tx], wsum), while acc takes the rounded product,
// acc = fmaf(w, logit, acc) with w = window[ty] * window[tx]: that is what `ws += w` has always compiled to here (the compiler
// contracts it), and it is written out so that every instantiation gives the same bits whatever the vectoriser does with it.
// NH heads (stcd_scene_stitch_heads_d4; NH == 1 is stcd_scene_stitch_d4): head h adds lg.p[h] into the planes h * CLS .. of acc with
// the chain it would run alone; the covering ranges, the window weight and wsum are worked out once per pixel for all of them
template <int NH, int CLS, int MIR>
__global__ void __launch_bounds__(256)
k_scene_stitch(const SceneHeadPtrs lg, int H, int W, int T, int S, int tiles_x, int tiles_y, int64_t first_tile, int64_t n_tiles,
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
        float a[NH * CLS][4], ws[4];
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
                        for (int c = 0; c < NH * CLS; ++c) {
                            const float4 a4 = *reinterpret_cast<const float4*>(acc + c * HW + pix);
                            a[c][0] = a4.x; a[c][1] = a4.y; a[c][2] = a4.z; a[c][3] = a4.w;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool ok = xs + j < W;
                            ws[j] = ok ? wsum[pix + j] : 0.f;
#pragma unroll
                            for (int c = 0; c < NH * CLS; ++c) a[c][j] = ok ? acc[c * HW + pix + j] : 0.f;
                        }
                    }
                }
                const int tx0 = xs - kx * S;
                const int64_t lo = (k * CLS * T + ((MIR & 2) ? T - 1 - ty : ty)) * T;   // class 0 row of this tile; class c is c * T * T further
                if (vec_l && tx0 >= 0 && tx0 + 3 < T) {               // xs, S and T are multiples of 4 here, so tx0 is one too
                    float wx[4] = {1.f, 1.f, 1.f, 1.f};
                    if (window) {
                        const float4 w4 = *reinterpret_cast<const float4*>(window + tx0);
                        wx[0] = w4.x; wx[1] = w4.y; wx[2] = w4.z; wx[3] = w4.w;
                    }
                    float l[NH * CLS][4];
#pragma unroll
                    for (int h = 0; h < NH; ++h)
#pragma unroll
                        for (int c = 0; c < CLS; ++c) {
                            const float4 l4 = *reinterpret_cast<const float4*>(lg.p[h] + lo + (int64_t)c * T * T + ((MIR & 1) ? T - 4 - tx0 : tx0));
                            float* lc = l[h * CLS + c];
                            if (MIR & 1) { lc[0] = l4.w; lc[1] = l4.z; lc[2] = l4.y; lc[3] = l4.x; }
                            else { lc[0] = l4.x; lc[1] = l4.y; lc[2] = l4.z; lc[3] = l4.w; }
                        }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float w = wy * wx[j];
#pragma unroll
                        for (int c = 0; c < NH * CLS; ++c) a[c][j] = fmaf(w, l[c][j], a[c][j]);
                        ws[j] = fmaf(wy, wx[j], ws[j]);               // see the note on wsum above the kernel
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int tx = tx0 + j;
                        if (tx < 0 || tx >= T || xs + j >= W) continue;
                        const float wxj = window ? window[tx] : 1.f, w = wy * wxj;
#pragma unroll
                        for (int h = 0; h < NH; ++h)
#pragma unroll
                            for (int c = 0; c < CLS; ++c)
                                a[h * CLS + c][j] = fmaf(w, lg.p[h][lo + (int64_t)c * T * T + ((MIR & 1) ? T - 1 - tx : tx)], a[h * CLS + c][j]);
                        ws[j] = fmaf(wy, wxj, ws[j]);
                    }
                }
            }
        }
        if (!touched) continue;
        if (vec_a) {
            *reinterpret_cast<float4*>(wsum + pix) = make_float4(ws[0], ws[1], ws[2], ws[3]);
#pragma unroll
            for (int c = 0; c < NH * CLS; ++c) *reinterpret_cast<float4*>(acc + c * HW + pix) = make_float4(a[c][0], a[c][1], a[c][2], a[c][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (xs + j >= W) continue;
                wsum[pix + j] = ws[j];
#pragma unroll
                for (int c = 0; c < NH * CLS; ++c) acc[c * HW + pix + j] = a[c][j];
            }
        }
    }
}

// ---- transposing views of the stitch (d4 & 4): the logit of the upright tile pixel (ty, tx) is Ld[c, i, j] with
// i = (d4 & 1) ? T-1-tx : tx and j = (d4 & 2) ? T-1-ty : ty, so the logits' fast axis runs along the scene's y.  A block owns a
// 64 x 64 scene patch, a thread 4 rows of 4 consecutive x (16 register chains per head and class).  The tile loop runs over the
// union of the patch's covering ranges and is uniform per block; a pixel joins a tile by the predicate that defines its own covering
// range, so every pixel sees its tiles in ascending index exactly as in k_scene_stitch.  Per tile the thread works out the weights of
// its 16 pixels once; then, one head at a time (so that LDS stays float[CLS][64][65] for any NH): a wave stages 64 consecutive j of
// one logit row (256 contiguous bytes) into lds[c][x][y], rows of 65 dwords, and after the barrier a thread reads lds[c][x][y] for
// its pixels: 16 lanes 4 rows of 65 apart and 4 neighbouring y, two lanes per bank, which is the floor for 64 lanes.
#define SCENE_SPITCH (SCENE_PATCH + 1)
template <int NH, int CLS>
__global__ void __launch_bounds__(256)
k_scene_stitch_t(const SceneHeadPtrs lg, int H, int W, int T, int S, int tiles_x, int tiles_y, int64_t first_tile, int64_t n_tiles,
                 const float* __restrict__ window, float* __restrict__ acc, float* __restrict__ wsum, int y0, int x0, int pcols,
                 int64_t n_patches, int d4, int vec_a) {
    __shared__ float lds[CLS][SCENE_PATCH][SCENE_SPITCH];
    const int64_t HW = (int64_t)H * W;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t4 = (threadIdx.x & 15) * 4, tr = threadIdx.x >> 4;
    for (int64_t blk = blockIdx.x; blk < n_patches; blk += gridDim.x) {   // uniform per block, and so is everything around a barrier
        const int py = y0 + (int)(blk / pcols) * SCENE_PATCH, px = x0 + (int)(blk % pcols) * SCENE_PATCH;
        const int ye = min(py + SCENE_PATCH - 1, H - 1), xe = min(px + SCENE_PATCH - 1, W - 1);
        const int ky_lo = py < T ? 0 : (py - T) / S + 1, ky_hi = min(ye / S, tiles_y - 1);
        const int kx_lo = px < T ? 0 : (px - T) / S + 1, kx_hi = min(xe / S, tiles_x - 1);
        const int xs = px + t4;
        float a[NH * CLS][4][4], ws[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                 // the chain continues from what earlier calls left
            const int y = py + tr + 16 * r;
            const int64_t pix = (int64_t)y * W + xs;
            if (vec_a && y < H && xs < W) {
                const float4 w4 = *reinterpret_cast<const float4*>(wsum + pix);
                ws[r][0] = w4.x; ws[r][1] = w4.y; ws[r][2] = w4.z; ws[r][3] = w4.w;
#pragma unroll
                for (int c = 0; c < NH * CLS; ++c) {
                    const float4 a4 = *reinterpret_cast<const float4*>(acc + c * HW + pix);
                    a[c][r][0] = a4.x; a[c][r][1] = a4.y; a[c][r][2] = a4.z; a[c][r][3] = a4.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = y < H && xs + j < W;
                    ws[r][j] = ok ? wsum[pix + j] : 0.f;
#pragma unroll
                    for (int c = 0; c < NH * CLS; ++c) a[c][r][j] = ok ? acc[c * HW + pix + j] : 0.f;
                }
            }
        }
        bool touched = false;
        for (int ky = ky_lo; ky <= ky_hi; ++ky)
            for (int kx = kx_lo; kx <= kx_hi; ++kx) {
                const int64_t k = (int64_t)ky * tiles_x + kx - first_tile;
                if (k < 0 || k >= n_tiles) continue;                  // another call's tile (uniform)
                const int ty0 = py - ky * S, tx0 = px - kx * S;       // tile coordinates of the patch origin: may be negative
                float wgt[4][4] = {};                                 // this tile's weight at the thread's pixels, once for all heads
                unsigned on = 0;                                      // bit 4 * r + j: the pixel is in the scene and in the tile
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int yl = tr + 16 * r, ty = ty0 + yl;
                    if (py + yl >= H || ty < 0 || ty >= T) continue;
                    const float wy = window ? window[ty] : 1.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int tx = tx0 + t4 + j;
                        if (tx < 0 || tx >= T || xs + j >= W) continue;
                        const float wxj = window ? window[tx] : 1.f;
                        wgt[r][j] = wy * wxj;
                        ws[r][j] = fmaf(wy, wxj, ws[r][j]);           // as k_scene_stitch
                        on |= 1u << (4 * r + j);
                    }
                }
                touched |= on != 0;
#pragma unroll
                for (int h = 0; h < NH; ++h) {
                    __syncthreads();                                  // the previous tile or head has been read
                    {
                        const int ty = ty0 + lane;
                        if (ty >= 0 && ty < T) {
                            const int j = (d4 & 2) ? T - 1 - ty : ty;
                            for (int xl = wv; xl < SCENE_PATCH; xl += 4) {
                                const int tx = tx0 + xl;
                                if (tx < 0 || tx >= T) continue;
                                const int i = (d4 & 1) ? T - 1 - tx : tx;
                                const float* lp = lg.p[h] + ((k * CLS * T + i) * T + j);
#pragma unroll
                                for (int c = 0; c < CLS; ++c) lds[c][xl][lane] = lp[(int64_t)c * T * T];
                            }
                        }
                    }
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (!(on & (1u << (4 * r + j)))) continue;
#pragma unroll
                            for (int c = 0; c < CLS; ++c)
                                a[h * CLS + c][r][j] = fmaf(wgt[r][j], lds[c][t4 + j][tr + 16 * r], a[h * CLS + c][r][j]);
                        }
                }
            }
        if (!touched) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = py + tr + 16 * r;
            const int64_t pix = (int64_t)y * W + xs;
            if (y >= H || xs >= W) continue;
            if (vec_a) {
                *reinterpret_cast<float4*>(wsum + pix) = make_float4(ws[r][0], ws[r][1], ws[r][2], ws[r][3]);
#pragma unroll
                for (int c = 0; c < NH * CLS; ++c)
                    *reinterpret_cast<float4*>(acc + c * HW + pix) = make_float4(a[c][r][0], a[c][r][1], a[c][r][2], a[c][r][3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (xs + j >= W) continue;
                    wsum[pix + j] = ws[r][j];
#pragma unroll
                    for (int c = 0; c < NH * CLS; ++c) acc[c * HW + pix + j] = a[c][r][j];
                }
            }
        }
    }
}

// classes in {1, 2}, n_heads in 1..STCD_SCENE_MAX_HEADS (checked by the callers) -> the template arguments
#define STCD_STITCH_SHAPES(X) \
    switch (2 * n_heads + (classes == 2)) { \
        case 2: X(1, 1); break; \
        case 3: X(1, 2); break; \
        case 4: X(2, 1); break; \
        case 5: X(2, 2); break; \
        case 6: X(3, 1); break; \
        default: X(3, 2); break; \
    }

void launch_scene_stitch_heads_d4(const SceneHeadPtrs& lg, int n_heads, int classes, int H, int W, int T, int S, int tiles_x, int tiles_y,
                                  int first_tile, int n_tiles, const float* window, float* acc, float* wsum, int d4, hipStream_t s) {
    if (n_tiles == 0) return;
    const int last = first_tile + n_tiles - 1;
    const int ky0 = first_tile / tiles_x, ky1 = last / tiles_x;
    const int y0 = ky0 * S, y1 = (int)std::min<int64_t>(H, (int64_t)ky1 * S + T);
    int x0 = 0, x1 = W;
    if (ky0 == ky1) {                                                 // one tile row: only the columns its tiles reach
        x0 = ((first_tile % tiles_x) * S) & ~3;
        x1 = (int)std::min<int64_t>(W, (int64_t)(last % tiles_x) * S + T);
    }
    if (y1 <= y0 || x1 <= x0) return;
    const int vec_a = W % 4 == 0 && aligned_to(acc, 16) && aligned_to(wsum, 16);
    if (d4 & 4) {
        const int pcols = (x1 - x0 + SCENE_PATCH - 1) / SCENE_PATCH;
        const int64_t n_patches = (int64_t)((y1 - y0 + SCENE_PATCH - 1) / SCENE_PATCH) * pcols;
        const unsigned blocks = (unsigned)std::min<int64_t>(SCENE_MAX_BLOCKS, n_patches);
#define STCD_STITCH_T(NH, CLS) \
    k_scene_stitch_t<NH, CLS><<<blocks, 256, 0, s>>>(lg, H, W, T, S, tiles_x, tiles_y, first_tile, n_tiles, window, acc, wsum, y0, x0, pcols, \
                                                    n_patches, d4, vec_a)
        STCD_STITCH_SHAPES(STCD_STITCH_T)
#undef STCD_STITCH_T
        return;
    }
    const int gpr = (x1 - x0 + 3) / 4;
    const int64_t total = (int64_t)(y1 - y0) * gpr;
    int vec_l = T % 4 == 0 && S % 4 == 0 && (!window || aligned_to(window, 16));
    for (int h = 0; h < n_heads; ++h) vec_l = vec_l && aligned_to(lg.p[h], 16);
#define STCD_STITCH_ROWS(NH, CLS) \
    switch (d4) { \
        case 0: k_scene_stitch<NH, CLS, 0><<<scene_blocks(total), 256, 0, s>>>(lg, H, W, T, S, tiles_x, tiles_y, first_tile, n_tiles, window, acc, \
                                                                              wsum, y0, x0, gpr, total, vec_l, vec_a); break; \
        case 1: k_scene_stitch<NH, CLS, 1><<<scene_blocks(total), 256, 0, s>>>(lg, H, W, T, S, tiles_x, tiles_y, first_tile, n_tiles, window, acc, \
                                                                              wsum, y0, x0, gpr, total, vec_l, vec_a); break; \
        case 2: k_scene_stitch<NH, CLS, 2><<<scene_blocks(total), 256, 0, s>>>(lg, H, W, T, S, tiles_x, tiles_y, first_tile, n_tiles, window, acc, \
                                                                              wsum, y0, x0, gpr, total, vec_l, vec_a); break; \
        default: k_scene_stitch<NH, CLS, 3><<<scene_blocks(total), 256, 0, s>>>(lg, H, W, T, S, tiles_x, tiles_y, first_tile, n_tiles, window, acc, \
                                                                               wsum, y0, x0, gpr, total, vec_l, vec_a); break; \
    }
    STCD_STITCH_SHAPES(STCD_STITCH_ROWS)
#undef STCD_STITCH_ROWS
}
#undef STCD_STITCH_SHAPES

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

// ------------------------------------------------------------------ finalize of three stitched heads in one pass (stcd_scene_finalize_seg)
// acc holds the heads of SegCD's forward in its order, (mask_t1, mask_t2, change), CLS planes each over ONE wsum.  Per head the mask and
// the probability are k_scene_finalize's expressions, so they are its bits; gated = change & (seg_a != seg_b) is the decision-level gate
// sketched in train_stcd.py:170-176.  cm: four matrices of four counters, rows seg_a / seg_b / change / gated, counted
// only where that row's label (and, for row 3, gated) was given; the reduction is k_scene_finalize's, 16 counters instead of 4.
template <int CLS>
__global__ void __launch_bounds__(256)
k_scene_finalize_seg(const float* __restrict__ acc, const float* __restrict__ wsum, int H, int W, float seg_threshold, float change_threshold,
                     const uint8_t* __restrict__ label_a, const uint8_t* __restrict__ label_b, const uint8_t* __restrict__ label_c,
                     uint8_t* __restrict__ seg_a, uint8_t* __restrict__ seg_b, uint8_t* __restrict__ change, uint8_t* __restrict__ gated,
                     float* __restrict__ prob, unsigned long long* __restrict__ cm, int gpr, int64_t total, int vec) {
    __shared__ unsigned int bins[16];
    if (threadIdx.x < 16) bins[threadIdx.x] = 0;
    __syncthreads();
    unsigned int loc[4][4] = {};
    const int64_t HW = (int64_t)H * W;
    const bool need_ws = CLS == 1 || prob != nullptr;
    const uint8_t* const labels[3] = {label_a, label_b, label_c};
    uint8_t* const masks[3] = {seg_a, seg_b, change};
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int xs = (int)(g % gpr) * 4;
        const int64_t pix = (g / gpr) * W + xs;
        float ws[4] = {1.f, 1.f, 1.f, 1.f};
        if (need_ws) {
            if (vec) {
                const float4 w4 = *reinterpret_cast<const float4*>(wsum + pix);
                ws[0] = w4.x; ws[1] = w4.y; ws[2] = w4.z; ws[3] = w4.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (xs + j < W) ws[j] = wsum[pix + j];
            }
        }
        uint8_t pr[3][4], lab[4];
#pragma unroll
        for (int h = 0; h < 3; ++h) {
            const float* ah = acc + (int64_t)h * CLS * HW;
            const float threshold = h == 2 ? change_threshold : seg_threshold;
            float a[CLS][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) lab[j] = 255;
            if (vec) {
#pragma unroll
                for (int c = 0; c < CLS; ++c) {
                    const float4 a4 = *reinterpret_cast<const float4*>(ah + c * HW + pix);
                    a[c][0] = a4.x; a[c][1] = a4.y; a[c][2] = a4.z; a[c][3] = a4.w;
                }
                if (labels[h]) {
                    const uint32_t l4 = *reinterpret_cast<const uint32_t*>(labels[h] + pix);
#pragma unroll
                    for (int j = 0; j < 4; ++j) lab[j] = (uint8_t)(l4 >> (8 * j));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = xs + j < W;
#pragma unroll
                    for (int c = 0; c < CLS; ++c) a[c][j] = ok ? ah[c * HW + pix + j] : 0.f;
                    if (labels[h] && ok) lab[j] = labels[h][pix + j];
                }
            }
            float pb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                             // k_scene_finalize's rules: a tie is class 0, strict >, NaN is class 0
                pr[h][j] = CLS == 2 ? (a[CLS - 1][j] > a[0][j]) : (a[0][j] > threshold * ws[j]);
                if (prob) {
                    const float d = (CLS == 2 ? a[CLS - 1][j] - a[0][j] : a[0][j]) / ws[j];
                    pb[j] = 1.f / (1.f + expf(-d));
                }
                if (lab[j] != 255) loc[h][2 * (lab[j] >= 1) + pr[h][j]]++;   // lanes past the row end carry 255
            }
            if (vec) {
                *reinterpret_cast<uint32_t*>(masks[h] + pix) =
                    (uint32_t)pr[h][0] | ((uint32_t)pr[h][1] << 8) | ((uint32_t)pr[h][2] << 16) | ((uint32_t)pr[h][3] << 24);
                if (prob) *reinterpret_cast<float4*>(prob + h * HW + pix) = make_float4(pb[0], pb[1], pb[2], pb[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (xs + j >= W) continue;
                    masks[h][pix + j] = pr[h][j];
                    if (prob) prob[h * HW + pix + j] = pb[j];
                }
            }
        }
        if (gated) {                                                  // lab still holds label_c (h == 2 ran last)
            uint8_t gt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gt[j] = pr[2][j] & (pr[0][j] != pr[1][j]);
                if (lab[j] != 255) loc[3][2 * (lab[j] >= 1) + gt[j]]++;
            }
            if (vec) {
                *reinterpret_cast<uint32_t*>(gated + pix) = (uint32_t)gt[0] | ((uint32_t)gt[1] << 8) | ((uint32_t)gt[2] << 16) | ((uint32_t)gt[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (xs + j < W) gated[pix + j] = gt[j];
            }
        }
    }
    if (!cm) return;                                                  // uniform: no thread skips the barrier alone
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (!labels[min(k >> 2, 2)] || (k >= 12 && !gated)) continue; // a row without its label stays untouched (uniform)
        unsigned int v = loc[k >> 2][k & 3];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&bins[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 16 && bins[threadIdx.x]) atomicAdd(cm + threadIdx.x, (unsigned long long)bins[threadIdx.x]);
}

void launch_scene_finalize_seg(const float* acc, const float* wsum, int classes, int H, int W, float seg_threshold, float change_threshold,
                               const uint8_t* label_a, const uint8_t* label_b, const uint8_t* label_c, uint8_t* seg_a, uint8_t* seg_b,
                               uint8_t* change, uint8_t* gated, float* prob, int64_t* cm, hipStream_t s) {
    const int gpr = (W + 3) / 4;
    const int64_t total = (int64_t)H * gpr;
    int vec = W % 4 == 0 && aligned_to(acc, 16) && aligned_to(wsum, 16) && (!prob || aligned_to(prob, 16));
    for (const void* p : {(const void*)label_a, (const void*)label_b, (const void*)label_c, (const void*)seg_a, (const void*)seg_b,
                          (const void*)change, (const void*)gated})
        vec = vec && aligned_to(p, 4);                                // NULL counts as aligned
    unsigned long long* cmu = (unsigned long long*)cm;                // block counts in 32 bits: see launch_scene_finalize
    if (classes == 2)
        k_scene_finalize_seg<2><<<scene_blocks(total), 256, 0, s>>>(acc, wsum, H, W, seg_threshold, change_threshold, label_a, label_b, label_c,
                                                                    seg_a, seg_b, change, gated, prob, cmu, gpr, total, vec);
    else
        k_scene_finalize_seg<1><<<scene_blocks(total), 256, 0, s>>>(acc, wsum, H, W, seg_threshold, change_threshold, label_a, label_b, label_c,
                                                                    seg_a, seg_b, change, gated, prob, cmu, gpr, total, vec);
}

}  // namespace stcd
