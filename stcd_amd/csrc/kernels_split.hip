// kernels_split.hip -- the cut of the distance-transform split (stcd_objects_split_cut, include/stcd_hip.h; stcd_amd/objects.py:
// split_objects; tests/nearest_spec.py states every output).  The core mask, its components and the nearest-seed transform are made by
// the entries that exist (stcd_mask_buffer, stcd_objects_label, stcd_edt_nearest); what is left is one pass over the pixels:
//
//   owner[p] = Lc[index[p]] if p is set, index[p] >= 0 and L0[index[p]] == L0[p], else 0  (a set pixel with owner 0 is an orphan)
//   p is cut iff owner[p] != 0 and one of the neighbours right, down-left, down, down-right has a non-zero owner other than owner[p]
//
// k_split_cut: a block of 256 threads takes SPLIT_ROWS rows of 256 columns.  The owners of those rows, of one row below and of one
// column left and right are computed once into LDS ((SPLIT_ROWS + 1) x 258 int32, 5 KiB; 1.26 owner evaluations per pixel, each
// three dependent loads), then every thread reads its own owner and the four later neighbours' from LDS, writes the byte and, when
// asked, the owner, and counts cut and orphan pixels: reduced per wave and block before one 64-bit integer atomic per block and
// counter, which is order-free.  An index outside [0, H W) reads nothing and gives owner 0.
#include "common.h"

namespace stcd {

#define SPLIT_THREADS 256
#define SPLIT_ROWS 4
#define SPLIT_LINE (SPLIT_THREADS + 2)         // a row of owners with the columns left and right of the block's
#define SPLIT_DIM_MAX 16384

struct SplitSrc {
    const uint8_t* mask;
    const int32_t* labels;                     // L0: the components of mask
    const int32_t* core_labels;                // Lc: the components of the core mask
    const int32_t* index;                      // the nearest core pixel, -1: none
    int H, W;
};

// owner of pixel (y, x); 0 outside the frame
__device__ __forceinline__ int32_t split_owner(const SplitSrc& s, int y, int x) {
    if ((unsigned)y >= (unsigned)s.H || (unsigned)x >= (unsigned)s.W) return 0;
    const int p = y * s.W + x;                                         // H W <= 2^28
    if (!s.mask[p]) return 0;
    const int32_t a = s.index[p];
    if ((uint32_t)a >= (uint32_t)(s.H * s.W)) return 0;
    return s.labels[a] == s.labels[p] ? s.core_labels[a] : 0;
}

__global__ void __launch_bounds__(SPLIT_THREADS)
k_split_cut(SplitSrc s, int mask_value, uint8_t* __restrict__ out, int32_t* __restrict__ owner, unsigned long long* __restrict__ counts) {
    __shared__ int32_t own[SPLIT_ROWS + 1][SPLIT_LINE];
    __shared__ unsigned part[SPLIT_THREADS / 64][2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j0 = blockIdx.x * SPLIT_THREADS, i0 = blockIdx.y * SPLIT_ROWS;
    for (int e = tid; e < (SPLIT_ROWS + 1) * SPLIT_LINE; e += SPLIT_THREADS) {
        const int r = e / SPLIT_LINE, c = e - r * SPLIT_LINE;
        own[r][c] = split_owner(s, i0 + r, j0 - 1 + c);
    }
    __syncthreads();
    unsigned cut = 0, orphan = 0;
    const int j = j0 + tid, c = tid + 1;
    if (j < s.W) {
#pragma unroll
        for (int r = 0; r < SPLIT_ROWS; ++r) {
            const int i = i0 + r;
            if (i >= s.H) break;
            const int p = i * s.W + j;
            const bool set = s.mask[p] != 0;
            const int32_t o = own[r][c];
            bool hit = false;
            if (o != 0) {
                const int32_t nb[4] = {own[r][c + 1], own[r + 1][c - 1], own[r + 1][c], own[r + 1][c + 1]};
#pragma unroll
                for (int k = 0; k < 4; ++k) hit = hit || (nb[k] != 0 && nb[k] != o);
            }
            out[p] = set && !hit ? (uint8_t)mask_value : (uint8_t)0;
            if (owner) owner[p] = o;
            cut += hit ? 1u : 0u;
            orphan += set && o == 0 ? 1u : 0u;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        cut += __shfl_xor(cut, d, 64);
        orphan += __shfl_xor(orphan, d, 64);
    }
    if (lane == 0) { part[wave][0] = cut; part[wave][1] = orphan; }
    __syncthreads();
    if (tid < 2) {
        const unsigned long long sum = (unsigned long long)part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (sum) atomicAdd(counts + tid, sum);
    }
}

namespace {
inline bool split_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
}  // namespace
}  // namespace stcd

using namespace stcd;

extern "C" {

int stcd_objects_split_cut(const uint8_t* mask, const int32_t* labels, const int32_t* core_labels, const int32_t* index, int height, int width,
                           int mask_value, uint8_t* out, int32_t* owner, int64_t* counts, void* hip_stream) {
    STCD_CHECK(mask && labels && core_labels && index && out && counts, "null pointer argument");
    STCD_CHECK(height >= 1 && height <= SPLIT_DIM_MAX && width >= 1 && width <= SPLIT_DIM_MAX, "height and width must be in [1, 16384]");
    STCD_CHECK(mask_value >= 1 && mask_value <= 255, "mask_value must be in [1, 255]");
    STCD_CHECK(split_aligned(labels, 4) && split_aligned(core_labels, 4) && split_aligned(index, 4) && split_aligned(owner, 4),
               "labels, core_labels, index and owner must be 4-byte aligned");
    STCD_CHECK(split_aligned(counts, 8), "counts must be 8-byte aligned");
    const int64_t px = (int64_t)height * width;
    STCD_CHECK(!((const char*)mask < (const char*)out + px && (const char*)out < (const char*)mask + px), "out must not overlap mask");
    hipStream_t s = (hipStream_t)hip_stream;
    STCD_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
    SplitSrc src;
    src.mask = mask; src.labels = labels; src.core_labels = core_labels; src.index = index; src.H = height; src.W = width;
    const dim3 grid((unsigned)((width + SPLIT_THREADS - 1) / SPLIT_THREADS), (unsigned)((height + SPLIT_ROWS - 1) / SPLIT_ROWS));
    k_split_cut<<<grid, SPLIT_THREADS, 0, s>>>(src, mask_value, out, owner, (unsigned long long*)counts);
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
