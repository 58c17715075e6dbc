// kernels_selftrain.hip -- the self-training round between two trainings: K checkpoints score the same pairs (gfx950).
//
// What this replaces in the reference (semantics, not code):
//   sigmoid, > 0.5, .int(), .cpu() per checkpoint and pair, metric.addBatch(preds[i], preds[-1])   /root/reference/train_stcd.py:111-125
//   sigmoid, > 0.5, .int(), cd_total.addBatch(pred.cpu(), label.cpu()), the 0 / 255 mask           /root/reference/train_stcd.py:155-177,182
// One launch reads the raw change output of every checkpoint once (4 * n_models * classes bytes per pixel) and writes one byte:
// the last checkpoint's mask.  What leaves besides is integer counts: per pair and earlier checkpoint the 2 x 2 agreement with the
// last checkpoint, and over all pairs the confusion matrix of the last checkpoint against the label.
//
// A thread owns 4 consecutive pixels of one pair (16-byte loads when hw % 4 == 0 and every pointer allows it, as kernels_scene.hip);
// a block stays inside one pair, so its counts need one reduction per pair it visits: registers -> wave (shuffles) -> block (LDS)
// -> one 64-bit integer atomic per block and cell.  Per earlier model three sums are kept (|pred_i|, |pred_i & last|, and |last|
// once); the four cells follow with the block's own pixel count.  No float atomics: every output is a pure function of the inputs.
#include <algorithm>

#include "common.h"

namespace stcd {

#define SELFTRAIN_MAX_BLOCKS 2048  // grid-stride above this: 8 blocks per CU
#define SELFTRAIN_COUNTERS (2 * (STCD_SELFTRAIN_MAX_MODELS - 1) + 2 + 4)

// counter slots of a thread / block: [2 i] = |pred_i|, [2 i + 1] = |pred_i & last| for the earlier models i, then |last|, the pixel
// count, and the four cells of the label matrix (those run over all pairs of the block, the others over one pair)
enum { ST_LAST = 2 * (STCD_SELFTRAIN_MAX_MODELS - 1), ST_PIX = ST_LAST + 1, ST_CM = ST_LAST + 2 };

__device__ __forceinline__ unsigned long long st_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int CLS, bool VEC>
__global__ void __launch_bounds__(256)
k_selftrain_score(SelftrainPtrs lg, int nm, int batch, int64_t hw, float threshold, const uint8_t* __restrict__ label, uint32_t mask_value,
                  uint8_t* __restrict__ mask, unsigned long long* __restrict__ agree, unsigned long long* __restrict__ cm) {
    constexpr int MAXM = STCD_SELFTRAIN_MAX_MODELS;
    __shared__ unsigned long long part[4][SELFTRAIN_COUNTERS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t groups = (hw + 3) / 4;
    unsigned int cmloc[4] = {0, 0, 0, 0};
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {             // uniform over the block: the barriers below are safe
        unsigned int np[MAXM - 1], nb[MAXM - 1], nlast = 0, npix = 0;
#pragma unroll
        for (int i = 0; i < MAXM - 1; ++i) np[i] = nb[i] = 0;
        const int64_t base = (int64_t)b * CLS * hw;                   // class 0 of pair b; class 1 is hw further
        for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
            const int64_t p = g * 4;
            uint32_t pred[MAXM], last = 0;                            // bit j: pixel p + j is change for model k
#pragma unroll
            for (int k = 0; k < MAXM; ++k) {
                pred[k] = 0;
                if (k >= nm) continue;                                // nm is uniform
                const float* q = lg.p[k] + base + p;
                float x0[4], x1[4];
                if (VEC) {
                    const float4 a = *reinterpret_cast<const float4*>(q);
                    x0[0] = a.x; x0[1] = a.y; x0[2] = a.z; x0[3] = a.w;
                    if (CLS == 2) {
                        const float4 c = *reinterpret_cast<const float4*>(q + hw);
                        x1[0] = c.x; x1[1] = c.y; x1[2] = c.z; x1[3] = c.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool ok = p + j < hw;
                        x0[j] = ok ? q[j] : 0.f;
                        if (CLS == 2) x1[j] = ok ? q[hw + j] : 0.f;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // a tie is class 0 (torch.argmax takes the first maximum); one class: strictly above the threshold; NaN is class 0
                    const bool c = CLS == 2 ? (x1[j] > x0[j]) : (x0[j] > threshold);
                    pred[k] |= (uint32_t)(c && (VEC || p + j < hw)) << j;
                }
                if (k == nm - 1) last = pred[k];                      // no run-time index into the register array
            }
            const uint32_t valid = VEC ? 15u : (p + 3 < hw ? 15u : (1u << (int)(hw - p)) - 1u);
#pragma unroll
            for (int i = 0; i < MAXM - 1; ++i) {
                if (i >= nm - 1) continue;
                np[i] += __popc(pred[i]);
                nb[i] += __popc(pred[i] & last);
            }
            nlast += __popc(last);
            npix += __popc(valid);
            uint32_t lab4 = 0xffffffffu;                              // 255: ignored
            if (label) {
                const uint8_t* lp = label + (int64_t)b * hw + p;
                if (VEC) lab4 = *reinterpret_cast<const uint32_t*>(lp);
                else {
                    lab4 = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) lab4 |= (uint32_t)(p + j < hw ? lp[j] : 255) << (8 * j);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t l = (lab4 >> (8 * j)) & 255u;
                    if (l != 255u) cmloc[2 * (l >= 1u) + ((last >> j) & 1u)]++;
                }
            }
            uint8_t* mp = mask + (int64_t)b * hw + p;
            if (VEC) {
                *reinterpret_cast<uint32_t*>(mp) = (((last >> 0) & 1u) | (((last >> 1) & 1u) << 8) | (((last >> 2) & 1u) << 16) | (((last >> 3) & 1u) << 24)) * mask_value;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (p + j < hw) mp[j] = (uint8_t)(((last >> j) & 1u) * mask_value);
            }
        }
        if (nm == 1) continue;                                        // uniform: no agreement to report
        // this pair's counts of the block: wave sums, then the block's through LDS
#pragma unroll
        for (int i = 0; i < MAXM - 1; ++i) {
            if (i >= nm - 1) continue;
            const unsigned long long a = st_wave_sum(np[i]), c = st_wave_sum(nb[i]);
            if (lane == 0) { part[wave][2 * i] = a; part[wave][2 * i + 1] = c; }
        }
        {
            const unsigned long long a = st_wave_sum(nlast), c = st_wave_sum(npix);
            if (lane == 0) { part[wave][ST_LAST] = a; part[wave][ST_PIX] = c; }
        }
        __syncthreads();
        if ((int)threadIdx.x < nm - 1) {
            const int i = threadIdx.x;
            unsigned long long P = 0, B = 0, L = 0, N = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { P += part[w][2 * i]; B += part[w][2 * i + 1]; L += part[w][ST_LAST]; N += part[w][ST_PIX]; }
            unsigned long long* a = agree + ((int64_t)b * (nm - 1) + i) * 4;      // a[2 * last + pred_i]
            const unsigned long long c00 = N - P - L + B, c01 = P - B, c10 = L - B;
            if (c00) atomicAdd(a + 0, c00);
            if (c01) atomicAdd(a + 1, c01);
            if (c10) atomicAdd(a + 2, c10);
            if (B) atomicAdd(a + 3, B);
        }
        __syncthreads();                                              // part is written again for the block's next pair
    }
    if (!cm) return;                                                  // uniform
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long v = st_wave_sum(cmloc[k]);
        if (lane == 0) part[wave][ST_CM + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = part[0][ST_CM + threadIdx.x] + part[1][ST_CM + threadIdx.x] + part[2][ST_CM + threadIdx.x] + part[3][ST_CM + threadIdx.x];
        if (v) atomicAdd(cm + threadIdx.x, v);
    }
}

static inline bool st_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

void launch_selftrain_score(const SelftrainPtrs& lg, int n_models, int batch, int classes, int64_t hw, float threshold, const uint8_t* label,
                            int mask_value, uint8_t* mask, int64_t* agree, int64_t* cm, hipStream_t s) {
    if (batch == 0 || hw == 0) return;
    bool vec = hw % 4 == 0 && st_aligned(mask, 4) && (!label || st_aligned(label, 4));
    for (int k = 0; k < n_models; ++k) vec = vec && st_aligned(lg.p[k], 16);
    // a thread counts in 32 bits: it sees at most 4 * ceil(groups / (256 * gx)) pixels per pair, and cm over at most `batch / gy` pairs
    const int64_t groups = (hw + 3) / 4;
    const unsigned gy = (unsigned)std::min(batch, 65535);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((groups + 255) / 256, std::max<unsigned>(1u, SELFTRAIN_MAX_BLOCKS / gy)));
    const dim3 grid(gx, gy);
    unsigned long long* ag = (unsigned long long*)agree;
    unsigned long long* cmu = (unsigned long long*)cm;
#define ST_LAUNCH(CLS, VEC) k_selftrain_score<CLS, VEC><<<grid, 256, 0, s>>>(lg, n_models, batch, hw, threshold, label, (uint32_t)mask_value, mask, ag, cmu)
    if (classes == 2) { if (vec) ST_LAUNCH(2, true); else ST_LAUNCH(2, false); }
    else              { if (vec) ST_LAUNCH(1, true); else ST_LAUNCH(1, false); }
#undef ST_LAUNCH
}

}  // namespace stcd
