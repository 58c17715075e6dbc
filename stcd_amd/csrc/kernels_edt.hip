// kernels_edt.hip -- the exact squared Euclidean distance transform of a uint8 mask on the device (gfx950), with the three things
// read off it: the int32 plane itself, a threshold (the disc buffers: dilate, erode and from them open and close at any radius) and
// the boundary match of two masks (boundary precision / recall and the Hausdorff distance).  tests/edt_spec.py states every output
// in numpy and include/stcd_hip.h the definitions.  Integers only; the d2 path has no atomic at all, the match counts meet in 64-bit
// integer atomics, which are order-free: every output is a pure function of the input.
//
// Separable and exact: d2[i][j] = min_k (j - k)^2 + g[i][k]^2, g[i][k] the distance along column k from row i to the column's
// nearest seed.  Four launches per transform, whatever the data:
//
//   k_edt_col_seeds  a thread per (chunk of EDT_COL_CHUNK rows, EDT_LANE_COLS columns): consecutive lanes take consecutive 4-byte
//                    words of a mask row.  The seed predicate (unset / set / boundary with its four neighbour reads and the void
//                    plane) is evaluated in this loader, edt_chunk_bits; no seed plane is ever written.  In boundary mode three rows'
//                    states roll through registers and the bytes beside a lane's four come from its neighbours by a shuffle, so
//                    every row of a chunk (and one above and below) is loaded once.  The chunk's seeds of a column
//                    are 64 bits in a register; the thread leaves (first, last) seed row of the chunk per column in a small table,
//                    ushort2 [chunks][width rounded up to 4].
//   k_edt_col_carry  a thread per column walks the table down and up (at most 256 entries, eight loads in flight) and replaces `last` by the last seed row
//                    of any chunk above and `first` by the first seed row of any chunk below: the carry across the cuts.
//   k_edt_col_dist   the loader again; the nearest seed above and below inside the chunk by count-leading / find-first on the 64
//                    bits (no walk), outside it from the table; g as uint16 (0xFFFF: the column has no seed), 8-byte stores.
//   k_edt_row<EPI>   a block of 256 threads per row.  The row of g and the argmins live in LDS as uint16 (4 bytes per column, 64 KiB
//                    at 16384).  The cost (j - k)^2 + h[k] is Monge for any h, so the leftmost argmin k*(j) is non-decreasing in j:
//                    the middle column's argmin is resolved over the whole row, then the middles of the two halves within
//                    [k*(left), k*(right)], and so on: ceil(log2(W + 1)) levels inside the kernel with a barrier between them,
//                    the summed range of a level at most W plus its midpoints, independent of the data (no window bounded by the
//                    best distance: a nearly empty mask costs what a full one costs).  Levels of fewer than four midpoints are
//                    reduced by the whole block; from there on a lane scans a range of up to EDT_ROW_LANE_MAX alone and longer
//                    ranges are collected per wavefront with a ballot and reduced by its 64 lanes (k_raster_edges' way with long
//                    edges); midpoints are dealt round-robin to the four waves.  Ties go to the lower k.
//                    Epilogue, a template parameter: EDT_EPI_D2 stores the int32 plane, EDT_EPI_MASK the threshold as bytes,
//                    EDT_EPI_MATCH accumulates n, max d2 and within[t] at the boundary pixels of the other mask (evaluated by
//                    edt_seed4 in place), reduced per wave and block before one integer atomic per block and counter.
//
// The nearest-seed transform (stcd_edt_nearest, stcd_edt_gather) keeps the seed the minimum came from.  Its third launch is
// k_edt_col_near: k_edt_col_dist's body with bit 15 of g set where the column's nearer seed is strictly below the row (a tie goes
// to the seed above, the smaller row; g <= 16383 leaves the bit free and EDT_NONE stays EDT_NONE), so no second plane is written
// and the scratch buffer is unchanged.  k_edt_row<EDT_EPI_INDEX / _GATHER> strips that bit while it loads the row into LDS, into a
// side line of a byte per four columns (4 KiB at 16384: 68 KiB per block, still two blocks per CU of 160 KiB), so h and the argmin
// search are exactly those of the other epilogues; the epilogue rebuilds the seed row of column arg[j] as i - h or i + h and
// writes the linear index (and d2), or values[index] under the threshold.  Leftmost argmin column, then the upper seed: the
// smallest column wins a tie, then the smallest row.
#include <algorithm>

#include "common.h"

namespace stcd {

#define EDT_COL_CHUNK 64                       // COL_CHUNK of stcd_amd/distance.py: rows per column chunk, one bit each in a 64-bit register
#define EDT_LANE_COLS 4                        // columns (mask bytes) per lane of the column pass and of the row pass's epilogue
#define EDT_THREADS 256                        // ROW_THREADS: threads per block; the row pass deals this many midpoints per step
#define EDT_ROW_LANE_MAX 64                    // ROW_LANE_MAX: the longest argmin range a lane scans alone; a wavefront takes longer ones
#define EDT_ROW_BLOCK_MIDS 4                   // levels with fewer midpoints than this are reduced by the whole block
#define EDT_DIM_MAX 16384
#define EDT_NONE 0xFFFFu                       // g: the column has no seed; table: no seed row
#define EDT_NO_SEED (1 << 30)                  // NO_SEED
#define EDT_MAX_Q 8
#define EDT_BELOW 0x8000u                      // g of k_edt_col_near: the nearer seed of the column is below the row

enum { EDT_SEED_UNSET = 0, EDT_SEED_SET = 1, EDT_SEED_BOUNDARY = 2 };
enum { EDT_EPI_D2 = 0, EDT_EPI_MASK = 1, EDT_EPI_MATCH = 2, EDT_EPI_INDEX = 3, EDT_EPI_GATHER = 4 };

struct EdtSrc {                                // a mask and how to read seeds off it
    const uint8_t* mask;
    const uint8_t* ignore;                     // boundary mode: byte 255 is void; may be nullptr
    int H, W, mode;
    int vec;                                   // W % 4 == 0 and both planes 4-byte aligned: a row word is one 32-bit load
};

struct EdtEpi {
    int32_t* d2;                               // EDT_EPI_D2; EDT_EPI_INDEX: may be nullptr
    int32_t* index;                            // EDT_EPI_INDEX
    const int32_t* values; int32_t* gathered;  // EDT_EPI_GATHER, with q
    uint8_t* out; int q, keep_above, mask_value;      // EDT_EPI_MASK
    EdtSrc own;                                // EDT_EPI_MATCH: the mask whose boundary pixels are measured
    unsigned long long* counts;                // (n, max_d2, within[0..nq-1]) of this side
    int nq; int qs[EDT_MAX_Q];
    int vec;                                   // 16-byte (d2, index, gathered) / 4-byte (out) stores: W % 4 == 0 and the pointers aligned
};

// bytes j0 .. j0 + 3 of row i, byte k in bits 8k; a pixel outside the frame reads 0.  vec: see EdtSrc (then j0 + 3 < W)
__device__ __forceinline__ uint32_t edt_bytes4(const uint8_t* __restrict__ p, int i, int j0, int H, int W, bool vec) {
    if ((unsigned)i >= (unsigned)H) return 0u;
    const uint8_t* __restrict__ row = p + (int64_t)i * W;
    if (vec) return *reinterpret_cast<const uint32_t*>(row + j0);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (j0 + k < W) v |= (uint32_t)row[j0 + k] << (8 * k);
    return v;
}
// bit k: byte k of w is non-zero / is 255
__device__ __forceinline__ uint32_t edt_nz4(uint32_t w) {
    return (w & 0xFFu ? 1u : 0u) | (w & 0xFF00u ? 2u : 0u) | (w & 0xFF0000u ? 4u : 0u) | (w & 0xFF000000u ? 8u : 0u);
}
__device__ __forceinline__ uint32_t edt_ff4(uint32_t w) { return edt_nz4(~w) ^ 15u; }

// boundary mode, one row: bits 0..3 the candidates (inside the frame, set, not void) among the columns j0 .. j0 + 3, bits 8..13 the
// free pixels (inside the frame, unset, not void) among the columns j0 - 1 .. j0 + 4.  A row outside the frame gives 0.
// EVERY LANE OF THE WAVEFRONT WITH j0 < W CALLS THIS TOGETHER, for one row i, lane l + 1 holding the columns j0 + 4 of lane l: with
// whole words (vec) the bytes left and right of a lane's four come from its neighbours' words by a shuffle, and only the first
// and the last lane load theirs.  A lane whose neighbour has left (j0 + 4 >= W) does not read what the shuffle gave it.
__device__ __forceinline__ uint32_t edt_row_state(const EdtSrc& s, int i, int j0) {
    const int H = s.H, W = s.W;
    if ((unsigned)i >= (unsigned)H) return 0u;                         // uniform: one row per call
    const bool vec = s.vec != 0;
    const uint8_t* __restrict__ ig = s.ignore;
    const uint32_t in4 = W - j0 >= 4 ? 15u : (1u << (W - j0)) - 1u;                    // the columns inside the frame
    const uint32_t mw = edt_bytes4(s.mask, i, j0, H, W, vec), iw = ig ? edt_bytes4(ig, i, j0, H, W, vec) : 0u;
    const uint32_t set = edt_nz4(mw), vd = edt_ff4(iw);
    const bool has_l = j0 > 0, has_r = j0 + 4 < W;
    const int64_t base = (int64_t)i * W;
    uint32_t lm = 1u, li = 0u, rm = 1u, ri = 0u;                       // the neighbour bytes of mask and ignore; outside the frame: not free
    if (vec) {
        const int lane = threadIdx.x & 63;
        lm = __shfl_up(mw, 1, 64) >> 24; li = __shfl_up(iw, 1, 64) >> 24;
        rm = __shfl_down(mw, 1, 64) & 255u; ri = __shfl_down(iw, 1, 64) & 255u;
        if (lane == 0 && has_l) { lm = s.mask[base + j0 - 1]; li = ig ? ig[base + j0 - 1] : 0u; }
        if (lane == 63 && has_r) { rm = s.mask[base + j0 + 4]; ri = ig ? ig[base + j0 + 4] : 0u; }
    } else {
        if (has_l) { lm = s.mask[base + j0 - 1]; li = ig ? ig[base + j0 - 1] : 0u; }
        if (has_r) { rm = s.mask[base + j0 + 4]; ri = ig ? ig[base + j0 + 4] : 0u; }
    }
    uint32_t free6 = (~set & ~vd & in4) << 1;                                          // bit k: column j0 - 1 + k
    if (has_l && lm == 0u && li != 255u) free6 |= 1u;
    if (has_r && rm == 0u && ri != 255u) free6 |= 32u;
    return (set & ~vd & in4) | (free6 << 8);
}
// the boundary pixels of a row from its state and those of the rows above and below: a candidate with a free 4-neighbour
__device__ __forceinline__ uint32_t edt_boundary4(uint32_t up, uint32_t cur, uint32_t dn) {
    const uint32_t f = cur >> 8;
    return cur & ((up >> 9) | (dn >> 9) | f | (f >> 2)) & 15u;
}

// bit k: pixel (i, j0 + k) is a seed.  Requires 0 <= i < H, 0 <= j0 < W, j0 % 4 == 0; called as edt_row_state is.
__device__ __forceinline__ uint32_t edt_seed4(const EdtSrc& s, int i, int j0) {
    if (s.mode != EDT_SEED_BOUNDARY) {
        const uint32_t in4 = s.W - j0 >= 4 ? 15u : (1u << (s.W - j0)) - 1u;
        const uint32_t set = edt_nz4(edt_bytes4(s.mask, i, j0, s.H, s.W, s.vec != 0));
        return (s.mode == EDT_SEED_SET ? set : ~set) & in4;
    }
    return edt_boundary4(edt_row_state(s, i - 1, j0), edt_row_state(s, i, j0), edt_row_state(s, i + 1, j0));      // no early exit: see edt_row_state
}

// the seeds of chunk c of the four columns from j0 on: bit r of bits[k] is pixel (c * EDT_COL_CHUNK + r, j0 + k).  In boundary mode
// the states of three rows roll through registers: every row of the chunk and one above and below is loaded once.
__device__ __forceinline__ void edt_chunk_bits(const EdtSrc& s, int c, int j0, uint64_t (&bits)[EDT_LANE_COLS]) {
    const int r0 = c * EDT_COL_CHUNK, n = min(EDT_COL_CHUNK, s.H - r0);
#pragma unroll
    for (int k = 0; k < EDT_LANE_COLS; ++k) bits[k] = 0;
    const bool rolling = s.mode == EDT_SEED_BOUNDARY;
    uint32_t up = 0, cur = 0;
    if (rolling) { up = edt_row_state(s, r0 - 1, j0); cur = edt_row_state(s, r0, j0); }
    for (int r = 0; r < n; ++r) {
        uint32_t s4;
        if (rolling) {
            const uint32_t dn = edt_row_state(s, r0 + r + 1, j0);
            s4 = edt_boundary4(up, cur, dn);
            up = cur; cur = dn;
        } else {
            s4 = edt_seed4(s, r0 + r, j0);
        }
#pragma unroll
        for (int k = 0; k < EDT_LANE_COLS; ++k) bits[k] |= (uint64_t)((s4 >> k) & 1u) << r;
    }
}

// tab: uint32 [chunks][Wp], low half the first seed row of the chunk in that column, high half the last (EDT_NONE: none)
__global__ void __launch_bounds__(EDT_THREADS)
k_edt_col_seeds(EdtSrc s, int Wp, uint32_t* __restrict__ tab) {
    const int j0 = (blockIdx.x * EDT_THREADS + threadIdx.x) * EDT_LANE_COLS, c = blockIdx.y;
    if (j0 >= s.W) return;                                             // j0 + 3 < Wp
    uint64_t bits[EDT_LANE_COLS];
    edt_chunk_bits(s, c, j0, bits);
    const int r0 = c * EDT_COL_CHUNK;
    uint32_t e[EDT_LANE_COLS];
#pragma unroll
    for (int k = 0; k < EDT_LANE_COLS; ++k) {
        const uint64_t b = bits[k];
        e[k] = b ? (uint32_t)(r0 + __ffsll((long long)b) - 1) | ((uint32_t)(r0 + 63 - __clzll((long long)b)) << 16) : (EDT_NONE | (EDT_NONE << 16));
    }
    *reinterpret_cast<uint4*>(tab + (int64_t)c * Wp + j0) = make_uint4(e[0], e[1], e[2], e[3]);      // 16-byte aligned: Wp % 4 == 0
}

__global__ void __launch_bounds__(EDT_THREADS)
k_edt_col_carry(int W, int Wp, int chunks, uint32_t* tab) {
    const int j = blockIdx.x * EDT_THREADS + threadIdx.x;
    if (j >= W) return;
    // eight entries are loaded before the first is rewritten: the loads do not wait for the carried value
    uint32_t run = EDT_NONE;                                           // the last seed row of the chunks above
    for (int c0 = 0; c0 < chunks; c0 += 8) {
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = c0 + k < chunks ? tab[(int64_t)(c0 + k) * Wp + j] : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (c0 + k >= chunks) break;
            const uint32_t last = e[k] >> 16;
            tab[(int64_t)(c0 + k) * Wp + j] = (e[k] & 0xFFFFu) | (run << 16);
            if (last != EDT_NONE) run = last;
        }
    }
    run = EDT_NONE;                                                    // the first seed row of the chunks below
    for (int c0 = chunks - 1; c0 >= 0; c0 -= 8) {
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = c0 - k >= 0 ? tab[(int64_t)(c0 - k) * Wp + j] : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (c0 - k < 0) break;
            const uint32_t first = e[k] & 0xFFFFu;
            tab[(int64_t)(c0 - k) * Wp + j] = (e[k] & 0xFFFF0000u) | run;
            if (first != EDT_NONE) run = first;
        }
    }
}

// g: uint16 [H][Wp]; BELOW: with EDT_BELOW where the nearer seed is strictly below row i
template <bool BELOW>
__device__ __forceinline__ void edt_col_dist(const EdtSrc& s, int Wp, const uint32_t* __restrict__ tab, uint16_t* __restrict__ g) {
    const int j0 = (blockIdx.x * EDT_THREADS + threadIdx.x) * EDT_LANE_COLS, c = blockIdx.y;
    if (j0 >= s.W) return;
    uint64_t bits[EDT_LANE_COLS];
    edt_chunk_bits(s, c, j0, bits);
    const uint4 t4 = *reinterpret_cast<const uint4*>(tab + (int64_t)c * Wp + j0);
    const uint32_t e[EDT_LANE_COLS] = {t4.x, t4.y, t4.z, t4.w};
    const int r0 = c * EDT_COL_CHUNK, n = min(EDT_COL_CHUNK, s.H - r0);
    for (int r = 0; r < n; ++r) {
        const int i = r0 + r;
        uint32_t d[EDT_LANE_COLS];
#pragma unroll
        for (int k = 0; k < EDT_LANE_COLS; ++k) {
            const uint32_t below = e[k] & 0xFFFFu, above = e[k] >> 16;
            const uint64_t lo = bits[k] & (~0ull >> (63 - r)), hi = bits[k] >> r;      // the chunk's seeds at or above / at or below row i
            uint32_t up = EDT_NONE, dn = EDT_NONE;
            if (lo) up = (uint32_t)(r - (63 - __clzll((long long)lo)));
            else if (above != EDT_NONE) up = (uint32_t)i - above;
            if (hi) dn = (uint32_t)(__ffsll((long long)hi) - 1);
            else if (below != EDT_NONE) dn = below - (uint32_t)i;
            d[k] = min(up, dn);                                        // at most 16383, or EDT_NONE
            if constexpr (BELOW) d[k] |= dn < up ? EDT_BELOW : 0u;     // dn < up: dn is a distance
        }
        *reinterpret_cast<uint2*>(g + (int64_t)i * Wp + j0) = make_uint2(d[0] | (d[1] << 16), d[2] | (d[3] << 16));    // 8-byte aligned
    }
}

__global__ void __launch_bounds__(EDT_THREADS)
k_edt_col_dist(EdtSrc s, int Wp, const uint32_t* __restrict__ tab, uint16_t* __restrict__ g) { edt_col_dist<false>(s, Wp, tab, g); }
__global__ void __launch_bounds__(EDT_THREADS)
k_edt_col_near(EdtSrc s, int Wp, const uint32_t* __restrict__ tab, uint16_t* __restrict__ g) { edt_col_dist<true>(s, Wp, tab, g); }

// ------------------------------------------------------------------------------------------------ the row pass
__device__ __forceinline__ unsigned long long edt_key(const uint16_t* __restrict__ h, int j, int k) {     // (cost, k): the minimum is the leftmost argmin
    const uint32_t hv = h[k];
    const uint32_t h2 = hv == EDT_NONE ? (uint32_t)EDT_NO_SEED : hv * hv;
    const int d = j - k;
    return ((unsigned long long)((uint32_t)(d * d) + h2) << 32) | (uint32_t)k;
}
// two g values of k_edt_col_near in one word: the EDT_BELOW bits (bit 0: the low half) are taken out of w
__device__ __forceinline__ uint32_t edt_strip2(uint32_t& w) {
    const uint32_t lo = (w & 0xFFFFu) != EDT_NONE ? w & EDT_BELOW : 0u, hi = (w >> 16) != EDT_NONE ? w & (EDT_BELOW << 16) : 0u;
    w &= ~(lo | hi);
    return (lo >> 15) | (hi >> 30);
}
__device__ __forceinline__ unsigned long long edt_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ unsigned edt_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned edt_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, 64));
    return v;
}

template <int EPI>
__global__ void __launch_bounds__(EDT_THREADS)
k_edt_row(const uint16_t* __restrict__ g, int H, int W, int Wp, EdtEpi ep) {
    extern __shared__ __attribute__((aligned(16))) uint16_t edt_lds[];
    __shared__ unsigned long long red[4];
    __shared__ unsigned part[4][2 + EDT_MAX_Q];
    uint16_t* __restrict__ h = edt_lds;                                // [Wp]
    uint16_t* __restrict__ arg = edt_lds + Wp;                         // [Wp]: arg[j] = k*(j)
    constexpr bool NEAR = EPI == EDT_EPI_INDEX || EPI == EDT_EPI_GATHER;      // g is k_edt_col_near's
    uint8_t* __restrict__ below = reinterpret_cast<uint8_t*>(edt_lds + 2 * Wp);       // NEAR: [Wp / 4], bit k: the seed of column 4 b + k is below row i
    const int i = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint16_t* __restrict__ grow = g + (int64_t)i * Wp;
    for (int j = tid * 4; j < Wp; j += EDT_THREADS * 4) {
        uint2 w = *reinterpret_cast<const uint2*>(grow + j);
        if constexpr (NEAR) {
            const uint32_t b01 = edt_strip2(w.x), b23 = edt_strip2(w.y);
            below[j >> 2] = (uint8_t)(b01 | (b23 << 2));
        }
        *reinterpret_cast<uint2*>(h + j) = w;
    }
    __syncthreads();

    int L = 1;
    while ((1 << L) <= W) ++L;                                         // 2^L > W: levels 0 .. L - 1
    for (int l = 0; l < L; ++l) {
        // 1-based positions J = s (2 m + 1) <= W, between the resolved J - s and J + s (multiples of 2 s; 0 and above W: the frame)
        const int s = 1 << (L - 1 - l);
        const int M = (W / s + 1) >> 1;
        if (M < EDT_ROW_BLOCK_MIDS) {
            for (int m = 0; m < M; ++m) {
                const int J = s * (2 * m + 1), j = J - 1;
                const int klo = J - s >= 1 ? arg[J - s - 1] : 0, khi = J + s <= W ? arg[J + s - 1] : W - 1;
                unsigned long long best = ~0ull;
                for (int k = klo + tid; k <= khi; k += EDT_THREADS) best = min(best, edt_key(h, j, k));
                best = edt_wave_min(best);
                if (lane == 0) red[wave] = best;
                __syncthreads();
                if (tid == 0) arg[j] = (uint16_t)(uint32_t)min(min(red[0], red[1]), min(red[2], red[3]));
                __syncthreads();
            }
        } else {
            for (int base = 0; base < M; base += EDT_THREADS) {        // uniform over the block
                const int m = base + lane * 4 + wave;                  // round-robin over the waves
                const bool have = m < M;
                int j = 0, klo = 0, khi = -1;
                if (have) {
                    const int J = s * (2 * m + 1);
                    j = J - 1;
                    klo = J - s >= 1 ? arg[J - s - 1] : 0;
                    khi = J + s <= W ? arg[J + s - 1] : W - 1;
                }
                const int len = khi - klo + 1;
                if (have && len <= EDT_ROW_LANE_MAX) {
                    unsigned long long best = ~0ull;
                    for (int k = klo; k <= khi; ++k) best = min(best, edt_key(h, j, k));
                    arg[j] = (uint16_t)(uint32_t)best;
                }
                unsigned long long longs = __ballot(have && len > EDT_ROW_LANE_MAX);      // every lane of the wavefront is here
                while (longs) {
                    const int src = __ffsll((long long)longs) - 1;
                    longs &= longs - 1;
                    const int jj = __shfl(j, src, 64), a = __shfl(klo, src, 64), b = __shfl(khi, src, 64);
                    unsigned long long best = ~0ull;
                    for (int k = a + lane; k <= b; k += 64) best = min(best, edt_key(h, jj, k));
                    best = edt_wave_min(best);
                    if (lane == src) arg[j] = (uint16_t)(uint32_t)best;
                }
            }
            __syncthreads();                                           // a level reads only what earlier levels wrote
        }
    }

    // ---- epilogue: four columns per lane
    unsigned cnt[2 + EDT_MAX_Q];
#pragma unroll
    for (int t = 0; t < 2 + EDT_MAX_Q; ++t) cnt[t] = 0;
    const int64_t base = (int64_t)i * W;
    for (int j0 = tid * EDT_LANE_COLS; j0 < W; j0 += EDT_THREADS * EDT_LANE_COLS) {
        const int n = min(W - j0, EDT_LANE_COLS);
        uint32_t v[EDT_LANE_COLS];
#pragma unroll
        for (int k = 0; k < EDT_LANE_COLS; ++k)
            v[k] = k < n ? min((uint32_t)(edt_key(h, j0 + k, arg[j0 + k]) >> 32), (uint32_t)EDT_NO_SEED) : 0u;
        if constexpr (EPI == EDT_EPI_D2) {
            if (ep.vec) *reinterpret_cast<uint4*>(ep.d2 + base + j0) = make_uint4(v[0], v[1], v[2], v[3]);
            else
                for (int k = 0; k < n; ++k) ep.d2[base + j0 + k] = (int32_t)v[k];
        } else if constexpr (NEAR) {
            int32_t at[EDT_LANE_COLS];                                 // the linear index of the nearest seed, -1: the frame has none
#pragma unroll
            for (int k = 0; k < EDT_LANE_COLS; ++k) {
                at[k] = -1;
                if (k < n) {
                    const int a = arg[j0 + k];
                    const int hv = h[a];
                    if (hv != (int)EDT_NONE) at[k] = (((below[a >> 2] >> (a & 3)) & 1) ? i + hv : i - hv) * W + a;
                }
            }
            if constexpr (EPI == EDT_EPI_INDEX) {
                if (ep.vec) {
                    *reinterpret_cast<int4*>(ep.index + base + j0) = make_int4(at[0], at[1], at[2], at[3]);
                    if (ep.d2) *reinterpret_cast<uint4*>(ep.d2 + base + j0) = make_uint4(v[0], v[1], v[2], v[3]);
                } else {
                    for (int k = 0; k < n; ++k) ep.index[base + j0 + k] = at[k];
                    if (ep.d2)
                        for (int k = 0; k < n; ++k) ep.d2[base + j0 + k] = (int32_t)v[k];
                }
            } else {
                int32_t o[EDT_LANE_COLS];
#pragma unroll
                for (int k = 0; k < EDT_LANE_COLS; ++k) o[k] = k < n && v[k] <= (uint32_t)ep.q ? ep.values[at[k]] : 0;      // q < NO_SEED: at[k] >= 0
                if (ep.vec) *reinterpret_cast<int4*>(ep.gathered + base + j0) = make_int4(o[0], o[1], o[2], o[3]);
                else
                    for (int k = 0; k < n; ++k) ep.gathered[base + j0 + k] = o[k];
            }
        } else if constexpr (EPI == EDT_EPI_MASK) {
            uint32_t o = 0;
#pragma unroll
            for (int k = 0; k < EDT_LANE_COLS; ++k) {
                const bool hit = ep.keep_above ? v[k] > (uint32_t)ep.q : v[k] <= (uint32_t)ep.q;
                o |= (hit ? (uint32_t)ep.mask_value : 0u) << (8 * k);
            }
            if (ep.vec) *reinterpret_cast<uint32_t*>(ep.out + base + j0) = o;
            else
                for (int k = 0; k < n; ++k) ep.out[base + j0 + k] = (uint8_t)(o >> (8 * k));
        } else {
            const uint32_t own = edt_seed4(ep.own, i, j0);             // bits beyond the frame are clear
#pragma unroll
            for (int k = 0; k < EDT_LANE_COLS; ++k) {
                if (!((own >> k) & 1u)) continue;
                cnt[0] += 1u;
                cnt[1] = max(cnt[1], v[k]);
#pragma unroll
                for (int t = 0; t < EDT_MAX_Q; ++t) cnt[2 + t] += (t < ep.nq && v[k] <= (uint32_t)ep.qs[t]) ? 1u : 0u;
            }
        }
    }
    if constexpr (EPI == EDT_EPI_MATCH) {
#pragma unroll
        for (int t = 0; t < 2 + EDT_MAX_Q; ++t) {
            const unsigned r = t == 1 ? edt_wave_max(cnt[t]) : edt_wave_sum(cnt[t]);
            if (lane == 0) part[wave][t] = r;
        }
        __syncthreads();
        if (tid < 2 + ep.nq) {
            if (tid == 1) {
                const unsigned mx = max(max(part[0][1], part[1][1]), max(part[2][1], part[3][1]));
                if (mx) atomicMax(ep.counts + 1, (unsigned long long)mx);
            } else {
                const unsigned long long sum = (unsigned long long)part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
                if (sum) atomicAdd(ep.counts + tid, sum);
            }
        }
    }
}

namespace {

inline bool edt_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool edt_shape_ok(int height, int width) { return height >= 1 && height <= EDT_DIM_MAX && width >= 1 && width <= EDT_DIM_MAX; }
inline int edt_wp(int width) { return (width + 3) / 4 * 4; }
inline int edt_chunks(int height) { return (height + EDT_COL_CHUNK - 1) / EDT_COL_CHUNK; }
inline int64_t edt_g_bytes(int height, int width) { return ((int64_t)2 * height * edt_wp(width) + 15) / 16 * 16; }
inline int64_t edt_bytes(int height, int width) { return edt_g_bytes(height, width) + (int64_t)4 * edt_chunks(height) * edt_wp(width); }
inline bool edt_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}

EdtSrc edt_src(const uint8_t* mask, const uint8_t* ignore, int height, int width, int mode) {
    EdtSrc s;
    s.mask = mask; s.ignore = ignore; s.H = height; s.W = width; s.mode = mode;
    s.vec = width % 4 == 0 && edt_aligned(mask, 4) && edt_aligned(ignore, 4);
    return s;
}

// the four launches of one transform; the caller has checked every argument
template <int EPI>
hipError_t edt_run(const EdtSrc& src, const EdtEpi& ep, void* scratch, hipStream_t s) {
    const int H = src.H, W = src.W, Wp = edt_wp(W), chunks = edt_chunks(H);
    uint16_t* g = (uint16_t*)scratch;
    uint32_t* tab = (uint32_t*)((char*)scratch + edt_g_bytes(H, W));
    const dim3 cgrid((unsigned)((Wp / EDT_LANE_COLS + EDT_THREADS - 1) / EDT_THREADS), (unsigned)chunks);
    k_edt_col_seeds<<<cgrid, EDT_THREADS, 0, s>>>(src, Wp, tab);
    k_edt_col_carry<<<(unsigned)((W + EDT_THREADS - 1) / EDT_THREADS), EDT_THREADS, 0, s>>>(W, Wp, chunks, tab);
    constexpr bool NEAR = EPI == EDT_EPI_INDEX || EPI == EDT_EPI_GATHER;      // the side line of LDS: a byte per four columns
    if constexpr (NEAR) k_edt_col_near<<<cgrid, EDT_THREADS, 0, s>>>(src, Wp, tab, g);
    else k_edt_col_dist<<<cgrid, EDT_THREADS, 0, s>>>(src, Wp, tab, g);
    static bool attr_set = false;                                      // per instantiation: the row of 16384 needs 64 KiB beside the static LDS
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute((const void*)k_edt_row<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 4 * EDT_DIM_MAX + (NEAR ? EDT_DIM_MAX / 4 : 0));
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    k_edt_row<EPI><<<(unsigned)H, EDT_THREADS, (size_t)4 * Wp + (NEAR ? Wp / 4 : 0), s>>>(g, H, W, Wp, ep);
    return hipGetLastError();
}

}  // namespace
}  // namespace stcd

using namespace stcd;

extern "C" {

int64_t stcd_edt_scratch_bytes(int height, int width) {
    if (!edt_shape_ok(height, width)) return 0;
    return edt_bytes(height, width);
}

int stcd_edt(const uint8_t* mask, const uint8_t* ignore, int height, int width, int seeds, int32_t* d2, void* scratch, int64_t scratch_bytes,
             void* hip_stream) {
    STCD_CHECK(mask && d2 && scratch, "null pointer argument");
    STCD_CHECK(edt_shape_ok(height, width), "height and width must be in [1, 16384]");
    STCD_CHECK(seeds >= EDT_SEED_UNSET && seeds <= EDT_SEED_BOUNDARY, "seeds must be 0 (unset), 1 (set) or 2 (boundary)");
    STCD_CHECK(!ignore || seeds == EDT_SEED_BOUNDARY, "an ignore plane is read by seeds == 2 (boundary) alone");
    STCD_CHECK(edt_aligned(d2, 4) && edt_aligned(scratch, 16), "d2 must be 4-byte and scratch 16-byte aligned");
    STCD_CHECK(scratch_bytes >= edt_bytes(height, width), "scratch too small (stcd_edt_scratch_bytes)");
    EdtEpi ep = {};
    ep.d2 = d2;
    ep.vec = width % 4 == 0 && edt_aligned(d2, 16);
    STCD_HIP(edt_run<EDT_EPI_D2>(edt_src(mask, ignore, height, width, seeds), ep, scratch, (hipStream_t)hip_stream));
    return 0;
}

int stcd_mask_buffer(const uint8_t* mask, int height, int width, int seeds, int q, int keep_above, int mask_value, uint8_t* out, void* scratch,
                     int64_t scratch_bytes, void* hip_stream) {
    STCD_CHECK(mask && out && scratch, "null pointer argument");
    STCD_CHECK(edt_shape_ok(height, width), "height and width must be in [1, 16384]");
    STCD_CHECK(seeds >= EDT_SEED_UNSET && seeds <= EDT_SEED_BOUNDARY, "seeds must be 0 (unset), 1 (set) or 2 (boundary)");
    STCD_CHECK(q >= 0, "q must be >= 0");
    STCD_CHECK(keep_above == 0 || keep_above == 1, "keep_above must be 0 or 1");
    STCD_CHECK(mask_value >= 1 && mask_value <= 255, "mask_value must be in [1, 255]");
    STCD_CHECK(!edt_overlap(mask, (int64_t)height * width, out, (int64_t)height * width), "out must not overlap mask");
    STCD_CHECK(edt_aligned(scratch, 16), "scratch must be 16-byte aligned");
    STCD_CHECK(scratch_bytes >= edt_bytes(height, width), "scratch too small (stcd_edt_scratch_bytes)");
    EdtEpi ep = {};
    ep.out = out; ep.q = q; ep.keep_above = keep_above; ep.mask_value = mask_value;
    ep.vec = width % 4 == 0 && edt_aligned(out, 4);
    STCD_HIP(edt_run<EDT_EPI_MASK>(edt_src(mask, nullptr, height, width, seeds), ep, scratch, (hipStream_t)hip_stream));
    return 0;
}

int stcd_boundary_match(const uint8_t* pred, const uint8_t* label, int height, int width, const int32_t* q, int n_q, int64_t* counts,
                        void* scratch, int64_t scratch_bytes, void* hip_stream) {
    STCD_CHECK(pred && label && counts && scratch, "null pointer argument");
    STCD_CHECK(edt_shape_ok(height, width), "height and width must be in [1, 16384]");
    STCD_CHECK(n_q >= 0 && n_q <= EDT_MAX_Q, "n_q must be in [0, 8]");
    STCD_CHECK(q || n_q == 0, "null pointer argument");
    for (int t = 0; t < n_q; ++t) STCD_CHECK(q[t] >= 0, "every q must be >= 0");
    STCD_CHECK(edt_aligned(counts, 8) && edt_aligned(scratch, 16), "counts must be 8-byte and scratch 16-byte aligned");
    STCD_CHECK(scratch_bytes >= edt_bytes(height, width), "scratch too small (stcd_edt_scratch_bytes)");
    hipStream_t s = (hipStream_t)hip_stream;
    const int stride = 2 + n_q;
    STCD_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * 2 * stride, s));
    const EdtSrc bp = edt_src(pred, label, height, width, EDT_SEED_BOUNDARY), bl = edt_src(label, label, height, width, EDT_SEED_BOUNDARY);
    EdtEpi ep = {};
    ep.nq = n_q;
    for (int t = 0; t < n_q; ++t) ep.qs[t] = q[t];
    ep.own = bp; ep.counts = (unsigned long long*)counts;              // side 0: the boundary of pred against that of label
    STCD_HIP(edt_run<EDT_EPI_MATCH>(bl, ep, scratch, s));
    ep.own = bl; ep.counts = (unsigned long long*)counts + stride;     // side 1: the reverse
    STCD_HIP(edt_run<EDT_EPI_MATCH>(bp, ep, scratch, s));
    return 0;
}

int64_t stcd_edt_nearest_scratch_bytes(int height, int width) { return stcd_edt_scratch_bytes(height, width); }

int stcd_edt_nearest(const uint8_t* mask, const uint8_t* ignore, int height, int width, int seeds, int32_t* d2, int32_t* index, void* scratch,
                     int64_t scratch_bytes, void* hip_stream) {
    STCD_CHECK(mask && index && scratch, "null pointer argument");
    STCD_CHECK(edt_shape_ok(height, width), "height and width must be in [1, 16384]");
    STCD_CHECK(seeds >= EDT_SEED_UNSET && seeds <= EDT_SEED_BOUNDARY, "seeds must be 0 (unset), 1 (set) or 2 (boundary)");
    STCD_CHECK(!ignore || seeds == EDT_SEED_BOUNDARY, "an ignore plane is read by seeds == 2 (boundary) alone");
    STCD_CHECK(edt_aligned(index, 4) && edt_aligned(d2, 4) && edt_aligned(scratch, 16), "index and d2 must be 4-byte and scratch 16-byte aligned");
    STCD_CHECK(scratch_bytes >= edt_bytes(height, width), "scratch too small (stcd_edt_nearest_scratch_bytes)");
    EdtEpi ep = {};
    ep.d2 = d2; ep.index = index;
    ep.vec = width % 4 == 0 && edt_aligned(index, 16) && edt_aligned(d2, 16);
    STCD_HIP(edt_run<EDT_EPI_INDEX>(edt_src(mask, ignore, height, width, seeds), ep, scratch, (hipStream_t)hip_stream));
    return 0;
}

int stcd_edt_gather(const uint8_t* mask, int height, int width, int seeds, int q, const int32_t* values, int32_t* out, void* scratch,
                    int64_t scratch_bytes, void* hip_stream) {
    STCD_CHECK(mask && values && out && scratch, "null pointer argument");
    STCD_CHECK(edt_shape_ok(height, width), "height and width must be in [1, 16384]");
    STCD_CHECK(seeds >= EDT_SEED_UNSET && seeds <= EDT_SEED_BOUNDARY, "seeds must be 0 (unset), 1 (set) or 2 (boundary)");
    STCD_CHECK(q >= 0, "q must be >= 0");
    const int64_t px = (int64_t)height * width;
    STCD_CHECK(!edt_overlap(mask, px, out, 4 * px), "out must not overlap mask");
    STCD_CHECK(!edt_overlap(values, 4 * px, out, 4 * px), "out must not overlap values");
    STCD_CHECK(edt_aligned(values, 4) && edt_aligned(out, 4) && edt_aligned(scratch, 16), "values and out must be 4-byte and scratch 16-byte aligned");
    STCD_CHECK(scratch_bytes >= edt_bytes(height, width), "scratch too small (stcd_edt_nearest_scratch_bytes)");
    EdtEpi ep = {};
    ep.values = values; ep.gathered = out; ep.q = q < EDT_NO_SEED ? q : EDT_NO_SEED - 1;       // "no seed" is within no q
    ep.vec = width % 4 == 0 && edt_aligned(out, 16);
    STCD_HIP(edt_run<EDT_EPI_GATHER>(edt_src(mask, nullptr, height, width, seeds), ep, scratch, (hipStream_t)hip_stream));
    return 0;
}

}  // extern "C"
