// kernels_raster.hip -- change polygons back to pixels: the rings of kernels_rings.hip / kernels_simplify.hip (or any rings in that
// layout) rasterized into a uint8 mask on the device (gfx950), with its C-ABI entries.  tests/raster_spec.py states every output in
// plain Python and include/stcd_hip.h the rule.  Integers only and integer atomics only, which are order-free: the delta plane, and
// with it every output, is a pure function of the input.
//
// A pixel (i, j) is sampled at its centre (i + 1/2, j + 1/2).  An edge with y0 != y1, taken with y0 < y1 and dy = y1 - y0, crosses
// the centre line of every row y0 <= i < y1 once, at x = num / (2 dy) with num = 2 x0 dy + (x1 - x0) (2 i + 1 - 2 y0), and toggles
// the first column whose centre is not left of the crossing, j* = ceil(num / (2 dy) - 1/2) = floor((num + dy - 1) / (2 dy)), clamped
// to [0, width]: delta[i][j*] += s, s = +1 for an edge stored northwards and -1 for one stored southwards.  0 <= num <= 2^29 for
// coordinates in [0, 16384], so 32 bits hold it.  The winding number of a pixel is the sum of its row's deltas up to its column.
//
//   (clear)          hipMemsetAsync over the header and the plane, on every call
//   k_raster_edges   one thread per edge (= per vertex: the edge that leaves it).  The thread finds its ring by binary search in
//                    offsets, checks that ring's offsets and its two vertices' range, clips the row span to [0, height) and adds s
//                    at delta[i][j*] with a 32-bit atomic that returns nothing.  A lane walks its own edge while the clipped span
//                    is at most RS_SPAN_MAX rows; longer edges are collected per wavefront with a ballot and the 64 lanes stride
//                    over the rows of each, so a side of 16384 rows costs a lane 256 rows and not 16384.  No thread walks a ring.
//                    Threads 0..R also check that offsets ascend from 0 to V.
//   k_raster_scan    one wavefront per row, four rows per block: the row's inclusive sum of delta in chunks of RS_ROW_CHUNK columns
//                    (16 per lane, a 32-bit wave scan of the lane totals, the chunk's total carried into the next), the fill rule,
//                    the mask bytes and, with an overlay, the confusion counts of the same pixels, reduced per wave and block
//                    before one 64-bit atomic per block and counter.  16-byte mask stores and overlay loads when width % 16 == 0
//                    and the pointers are 16-byte aligned, bytes otherwise.
#include <algorithm>

#include "common.h"

namespace stcd {

#define RS_SPAN_MAX 32                         // RASTER_SPAN_MAX of stcd_amd/objects.py: the longest clipped row span a lane walks alone
#define RS_ROW_CHUNK 1024                      // RASTER_ROW_CHUNK: columns a wavefront scans per step, 64 lanes x RS_LANE_COLS
#define RS_LANE_COLS 16
#define RS_COORD_MAX 16384                     // coordinates lie in [0, RS_COORD_MAX], frames are at most RS_COORD_MAX x RS_COORD_MAX

enum { RS_ST_RANGE = 1, RS_ST_OFFSETS = 4 };

struct RsHeader {                              // the first 16 bytes of the scratch buffer; the plane int32 [height][width + 1] follows
    int status;
    int pad_[3];
};

struct RsEdge { int y0, x0, y1, x1, s; };      // y0 < y1; s as stored

// the column the edge toggles in row i (y0 <= i < y1), clamped to [0, W]
__device__ __forceinline__ int rs_column(const RsEdge& e, int i, int W) {
    int j = e.x0;
    if (e.x1 != e.x0) {                                                // a vertical side needs no division
        const int dy = e.y1 - e.y0;
        const unsigned num = (unsigned)(2 * e.x0 * dy + (e.x1 - e.x0) * (2 * i + 1 - 2 * e.y0));   // 0 <= num <= 2^29
        j = (int)((num + (unsigned)dy - 1u) / (2u * (unsigned)dy));
    }
    return min(max(j, 0), W);
}

__device__ __forceinline__ void rs_toggle(int* __restrict__ delta, const RsEdge& e, int i, int W) {
    atomicAdd(delta + (int64_t)i * (W + 1) + rs_column(e, i, W), e.s);                 // the result is not used: no return value
}

__global__ void __launch_bounds__(256)
k_raster_edges(const int2* __restrict__ vertices, const long long* __restrict__ offsets, long long R, long long V, int H, int W,
               RsHeader* __restrict__ hdr, int* __restrict__ delta) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int bad = 0;
    if (t < R) {                                                       // every offset is looked at once
        const long long a = offsets[t], b = offsets[t + 1];
        if (a > b || (t == 0 && a != 0) || (t == R - 1 && b != V)) bad |= RS_ST_OFFSETS;
    }
    RsEdge e = {0, 0, 0, 0, 0};
    int lo = 0, hi = 0;                                                // the clipped row span
    if (t < V) {
        long long a = 0, b = R - 1;                                    // the last ring r with offsets[r] <= t
        while (a < b) {
            const long long m = (a + b + 1) >> 1;
            if (offsets[m] <= t) a = m; else b = m - 1;
        }
        const long long o0 = offsets[a], o1 = offsets[a + 1];
        if (o0 < 0 || o0 > t || o1 <= t || o1 > V) {                   // offsets that do not ascend: nothing of this ring is read
            bad |= RS_ST_OFFSETS;
        } else {
            const int2 p = vertices[t], q = vertices[t + 1 < o1 ? t + 1 : o0];         // both indices are in [o0, o1)
            const int py = p.x, px = p.y, qy = q.x, qx = q.y;          // a vertex is stored as (y, x)
            if ((unsigned)py > (unsigned)RS_COORD_MAX || (unsigned)px > (unsigned)RS_COORD_MAX || (unsigned)qy > (unsigned)RS_COORD_MAX ||
                (unsigned)qx > (unsigned)RS_COORD_MAX) {
                bad |= RS_ST_RANGE;                                    // the edge is skipped: num stays within 32 bits whatever the input
            } else if (py != qy) {
                const bool north = qy < py;
                e.y0 = north ? qy : py; e.x0 = north ? qx : px;
                e.y1 = north ? py : qy; e.x1 = north ? px : qx;
                e.s = north ? 1 : -1;
                lo = e.y0; hi = min(e.y1, H);                          // y0 >= 0: rows are clipped before any loop
            }
        }
    }
    if (bad) atomicOr(&hdr->status, bad);
    const int span = hi - lo;                                          // <= 0: nothing to do
    if (span > 0 && span <= RS_SPAN_MAX)
        for (int i = lo; i < hi; ++i) rs_toggle(delta, e, i, W);
    unsigned long long longs = __ballot(span > RS_SPAN_MAX);           // uniform over the wavefront: every lane is still here
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        RsEdge f;
        f.y0 = __shfl(e.y0, src, 64); f.x0 = __shfl(e.x0, src, 64); f.y1 = __shfl(e.y1, src, 64); f.x1 = __shfl(e.x1, src, 64);
        f.s = __shfl(e.s, src, 64);
        const int flo = __shfl(lo, src, 64), fhi = __shfl(hi, src, 64);
        for (int i = flo + lane; i < fhi; i += 64) rs_toggle(delta, f, i, W);
    }
}

__device__ __forceinline__ int rs_wave_scan(int v, int lane) {        // inclusive; rg_wave_scan of ring_scan.h in 32 bits
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

__device__ __forceinline__ unsigned rs_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
k_raster_scan(const int* __restrict__ delta, int H, int W, int rule, int mask_value, const uint8_t* __restrict__ overlay,
              unsigned long long* __restrict__ cm, uint8_t* __restrict__ mask) {
    __shared__ unsigned part[4][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;                               // the wavefront's row
    unsigned nvalid = 0, nlab = 0, npred = 0, nboth = 0;               // at most 16384 each
    if (i < H) {                                                       // uniform over the wavefront
        const int* __restrict__ row = delta + (int64_t)i * (W + 1);
        const int64_t base = (int64_t)i * W;
        int carry = 0;
        for (int c0 = 0; c0 < W; c0 += RS_ROW_CHUNK) {                 // uniform
            const int j0 = c0 + lane * RS_LANE_COLS;
            const int n = min(max(W - j0, 0), RS_LANE_COLS);           // VEC: 0 or 16
            int v[RS_LANE_COLS];
            if (n == RS_LANE_COLS) {
#pragma unroll
                for (int k = 0; k < RS_LANE_COLS; k += 4) __builtin_memcpy(v + k, row + j0 + k, 16);      // 4-byte aligned: W + 1 ints a row
            } else {
#pragma unroll
                for (int k = 0; k < RS_LANE_COLS; ++k) v[k] = k < n ? row[j0 + k] : 0;
            }
#pragma unroll
            for (int k = 1; k < RS_LANE_COLS; ++k) v[k] += v[k - 1];
            const int inc = rs_wave_scan(v[RS_LANE_COLS - 1], lane);
            const int before = carry + inc - v[RS_LANE_COLS - 1];
            carry += __shfl(inc, 63, 64);
            uint32_t set = 0;                                          // bit k: pixel j0 + k is set
#pragma unroll
            for (int k = 0; k < RS_LANE_COLS; ++k) {
                const int w = before + v[k];
                set |= (uint32_t)(rule ? (w & 1) : (w > 0)) << k;
            }
            if constexpr (VEC) {
                if (n) {
                    uint32_t o[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t b = (set >> (4 * k)) & 15u;     // four pixels to four bytes
                        o[k] = ((b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21)) * (uint32_t)mask_value;
                    }
                    *reinterpret_cast<uint4*>(mask + base + j0) = make_uint4(o[0], o[1], o[2], o[3]);
                    if (overlay) {
                        const uint4 a = *reinterpret_cast<const uint4*>(overlay + base + j0);
                        const uint32_t lw[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                        for (int k = 0; k < RS_LANE_COLS; ++k) {
                            const uint32_t b = (lw[k >> 2] >> (8 * (k & 3))) & 255u;
                            const uint32_t valid = b != 255u, lab = valid & (b != 0u), pr = valid & ((set >> k) & 1u);
                            nvalid += valid; nlab += lab; npred += pr; nboth += lab & pr;
                        }
                    }
                }
            } else {
                for (int k = 0; k < n; ++k) {
                    const uint32_t p = (set >> k) & 1u;
                    mask[base + j0 + k] = p ? (uint8_t)mask_value : (uint8_t)0;
                    if (overlay) {
                        const uint32_t b = overlay[base + j0 + k];
                        const uint32_t valid = b != 255u, lab = valid & (b != 0u), pr = valid & p;
                        nvalid += valid; nlab += lab; npred += pr; nboth += lab & pr;
                    }
                }
            }
        }
    }
    if (!overlay) return;                                              // uniform over the grid
    const unsigned a = rs_wave_sum(nvalid), b = rs_wave_sum(nlab), c = rs_wave_sum(npred), d = rs_wave_sum(nboth);
    if (lane == 0) { part[wave][0] = a - b - c + d; part[wave][1] = c - d; part[wave][2] = b - d; part[wave][3] = d; }   // cm[2 * overlay + raster]
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long n = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) n += part[w][threadIdx.x];
        if (n) atomicAdd(cm + threadIdx.x, n);
    }
}

namespace {

inline bool rs_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool rs_shape_ok(int height, int width) { return height >= 1 && height <= RS_COORD_MAX && width >= 1 && width <= RS_COORD_MAX; }
inline int64_t rs_bytes(int height, int width) {
    return ((int64_t)sizeof(RsHeader) + 4 * (int64_t)height * ((int64_t)width + 1) + 7) / 8 * 8;
}

}  // namespace
}  // namespace stcd

using namespace stcd;

extern "C" {

int64_t stcd_rings_raster_scratch_bytes(int height, int width) {
    if (!rs_shape_ok(height, width)) return 0;
    return rs_bytes(height, width);
}

int stcd_rings_raster(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int height, int width, int rule,
                      int mask_value, const uint8_t* overlay, int64_t* cm, uint8_t* mask, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    STCD_CHECK((vertices || n_vertices == 0) && offsets && mask && scratch, "null pointer argument");   // no vertex: no vertex buffer
    STCD_CHECK((overlay == nullptr) == (cm == nullptr), "overlay and cm must be given together");
    STCD_CHECK(n_rings >= 0 && n_vertices >= 0, "n_rings and n_vertices must be >= 0");
    STCD_CHECK(n_rings < ((int64_t)1 << 31) && n_vertices < ((int64_t)1 << 31), "n_rings and n_vertices must be below 2^31");
    STCD_CHECK(rs_shape_ok(height, width), "height and width must be in [1, 16384]");
    STCD_CHECK(rule == 0 || rule == 1, "rule must be 0 (positive) or 1 (evenodd)");
    STCD_CHECK(mask_value >= 1 && mask_value <= 255, "mask_value must be in [1, 255]");
    STCD_CHECK(rs_aligned(vertices, 8) && rs_aligned(offsets, 8) && rs_aligned(cm, 8) && rs_aligned(scratch, 8),
               "vertices, offsets, cm and scratch must be 8-byte aligned");
    STCD_CHECK(scratch_bytes >= rs_bytes(height, width), "scratch too small (stcd_rings_raster_scratch_bytes)");
    hipStream_t s = (hipStream_t)hip_stream;
    RsHeader* hdr = (RsHeader*)scratch;
    int* delta = (int*)((char*)scratch + sizeof(RsHeader));
    const long long R = n_rings, V = n_vertices;
    STCD_HIP(hipMemsetAsync(scratch, 0, (size_t)rs_bytes(height, width), s));         // never what an earlier call left
    if (R > 0 && V > 0)
        k_raster_edges<<<(unsigned)((std::max(R, V) + 255) / 256), 256, 0, s>>>((const int2*)vertices, (const long long*)offsets, R, V, height, width,
                                                                                hdr, delta);
    const unsigned grid = (unsigned)((height + 3) / 4);
    const bool vec = width % 16 == 0 && rs_aligned(mask, 16) && rs_aligned(overlay, 16);
    if (vec) k_raster_scan<true><<<grid, 256, 0, s>>>(delta, height, width, rule, mask_value, overlay, (unsigned long long*)cm, mask);
    else     k_raster_scan<false><<<grid, 256, 0, s>>>(delta, height, width, rule, mask_value, overlay, (unsigned long long*)cm, mask);
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
