// kernels_objects.hip -- change objects on the device: connected components of a binary mask, their table (area, bounding box,
// overlap with a second mask) and the area / hole filter of the pseudo-label (gfx950), with their C-ABI entries.
//
// No counterpart in the reference: it continues the pseudo-label cleaning (stcd_mask_close, train_stcd.py:186-188) from pixels to
// objects.  As in kernels_scene_round.hip every kernel reads and writes bytes and integers only: no float arithmetic, no float
// atomics, so every output is a pure function of the input; pixel offsets are 64-bit, pixel INDICES (the labels) are int32
// (height * width < 2^31 is checked by the entries); byte loads and stores, no alignment demand on masks or width.
//
// The equivalence forest.  parent[p] is -1 for an unset pixel, else the index of a pixel of the same component with
// parent[p] <= p; a root (parent[p] == p) is the smallest pixel index of its set, i.e. the component's first pixel in raster
// order.  Every find / union loop therefore walks strictly decreasing indices and ends; each still carries an iteration cap
// (the pixel count) and sets the status word on reaching it, which would be a bug and never an input property.  No block waits
// for another block: each phase is its own launch.
//
//   k_obj_tile     one block per OBJ_TILE^2 tile: the tile as a bit image in LDS (one __ballot per 64 pixels), every pixel starts
//                  at the first pixel of its row run, runs of neighbouring rows are united by atomicMin in an LDS forest (one
//                  union per overlap of two runs, the diagonal contacts of 8-connectivity only where no direct contact exists),
//                  then parent[p] = global index of the local root.  Reads the tile's bytes once, writes 4 B per pixel.
//   k_obj_seam     one thread per pixel on the first row / column of a tile: unites it with its set neighbours across the tile
//                  edge (3 of them with 8-connectivity: that covers the diagonal pairs where four tiles meet) by atomicMin in
//                  the global forest.
//   k_obj_flatten_count / _measure   one full find per set pixel, parent[p] = root.  count: roots per OBJ_CHUNK pixels for the
//                  scan.  measure: a wave's 64 consecutive pixels are cut into runs of one root; one atomicAdd of the run length
//                  (and one atomicOr of the border flag, bit 31) per run into stat[root], and one per BLOCK for the block's
//                  smallest root (Guideline 12: not one atomic per pixel).
//   k_obj_scan_sums / k_obj_rank / k_obj_relabel   the plain three-launch prefix sum over the root flags: chunk sums (from the
//                  flatten), one block scans the sums, every chunk numbers its roots 1..n in raster order; then labels[p] =
//                  rank[parent[p]].
//   k_obj_select   the keep decision per pixel from stat[parent[p]]: the area filter, the hole fill, or the plain binarisation.
//   k_obj_table    per run of one label inside one row of a wave's 64 pixels: one 64-bit integer atomicAdd of the area, four
//                  atomicMin / atomicMax of the box, two adds of the overlap counts.
#include <algorithm>
#include <climits>

#include "common.h"

namespace stcd {

#define OBJ_TILE 64                            // tile height and width: one 64-bit word per row
#define OBJ_CHUNK 4096                         // pixels per block of the linear passes: 256 threads x 16
#define OBJ_BORDER 0x80000000u                 // stat[root]: bit 31 = the component touches the scene border, bits 0..30 = its area

__device__ __forceinline__ int ob_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ob_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------------------------------------ the forest in LDS (one tile)
__device__ __forceinline__ int ob_find_lds(const int* lab, int a, int* status) {
    for (int n = 0; n <= OBJ_TILE * OBJ_TILE; ++n) {
        const int pa = __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (pa == a || pa < 0) return a;
        a = pa;
    }
    atomicOr(status, 1);
    return a;
}
__device__ __forceinline__ void ob_union_lds(int* lab, int a, int b, int* status) {
    for (int n = 0; n <= OBJ_TILE * OBJ_TILE; ++n) {
        a = ob_find_lds(lab, a, status);
        b = ob_find_lds(lab, b, status);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                  // a > b: the larger root is hung under the smaller
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;                                                       // a was no root any more: old < a is of its set, unite that with b
    }
    atomicOr(status, 1);
}

// ------------------------------------------------------------------------------------------------ the forest in global memory
__device__ __forceinline__ int ob_find(const int* parent, int a, int cap, int* status) {
    for (int n = 0; n <= cap; ++n) {
        const int pa = ob_load(parent + a);
        if (pa == a || pa < 0) return a;
        a = pa;
    }
    atomicOr(status, 1);
    return a;
}
__device__ __forceinline__ void ob_union(int* parent, int a, int b, int cap, int* status) {
    for (int n = 0; n <= cap; ++n) {
        a = ob_find(parent, a, cap, status);
        b = ob_find(parent, b, cap, status);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
    atomicOr(status, 2);
}

// ------------------------------------------------------------------------------------------------ 1. tile pass
template <bool ZERO_STAT>
__global__ void __launch_bounds__(256)
k_obj_tile(const uint8_t* __restrict__ in, int H, int W, int conn8, int invert, int tiles_x, int* __restrict__ parent,
           uint32_t* __restrict__ stat, int* __restrict__ status) {
    __shared__ unsigned long long bits[OBJ_TILE];
    __shared__ int lab[OBJ_TILE * OBJ_TILE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int gy0 = by * OBJ_TILE, gx0 = bx * OBJ_TILE;
    const int gx = gx0 + lane;
    // stage: bit (r, lane) = pixel (gy0 + r, gx0 + lane) belongs to the labelled class; outside the scene: not
    for (int r = wave; r < OBJ_TILE; r += 4) {
        const int gy = gy0 + r;
        const bool set = gy < H && gx < W && ((in[(int64_t)gy * W + gx] != 0) != (invert != 0));
        const unsigned long long word = __ballot(set);
        if (lane == 0) bits[r] = word;
    }
    __syncthreads();
    // every pixel starts at the first pixel of its row run: the unions along a row are done
    for (int r = wave; r < OBJ_TILE; r += 4) {
        const unsigned long long w = bits[r];
        int v = -1;
        if ((w >> lane) & 1ull) {
            const unsigned long long below = ~w & ((1ull << lane) - 1ull);                 // unset pixels left of this one
            v = r * OBJ_TILE + (below ? 64 - __clzll((long long)below) : 0);
        }
        lab[r * OBJ_TILE + lane] = v;
    }
    __syncthreads();
    // unite the runs of row r with those of row r - 1: one union per stretch of columns where both rows are set; with
    // 8-connectivity also across a diagonal, but only where neither of the two direct contacts beside it exists (they would join
    // the same two runs)
    for (int r = wave; r < OBJ_TILE; r += 4) {
        if (r == 0) continue;                                          // uniform over the wave
        const unsigned long long w = bits[r], u = bits[r - 1];
        const unsigned long long t = w & u, lead = t & ~(t << 1);
        const int me = r * OBJ_TILE + lane, up = me - OBJ_TILE;
        if ((lead >> lane) & 1ull) ob_union_lds(lab, me, up, status);
        if (conn8) {
            const unsigned long long dl = w & (u << 1) & ~u & ~(w << 1);                   // up-left set, up unset, left unset
            const unsigned long long dr = w & (u >> 1) & ~u & ~(w >> 1);                   // up-right set, up unset, right unset
            if ((dl >> lane) & 1ull) ob_union_lds(lab, me, up - 1, status);                // bit lane of u << 1 set: lane >= 1
            if ((dr >> lane) & 1ull) ob_union_lds(lab, me, up + 1, status);                // bit lane of u >> 1 set: lane <= 62
        }
    }
    __syncthreads();
    // parent = global index of the local root (the tile's raster order is the scene's: the smallest local index is the smallest
    // global one)
    for (int r = wave; r < OBJ_TILE; r += 4) {
        const int gy = gy0 + r;
        if (gy >= H || gx >= W) continue;
        const int64_t p = (int64_t)gy * W + gx;
        int v = -1;
        if ((bits[r] >> lane) & 1ull) {
            const int a = ob_find_lds(lab, r * OBJ_TILE + lane, status);
            v = (int)((int64_t)(gy0 + (a >> 6)) * W + gx0 + (a & 63));
        }
        parent[p] = v;
        if (ZERO_STAT) stat[p] = 0u;
    }
}

// ------------------------------------------------------------------------------------------------ 2. seam pass
// items [0, seams_y * W): pixel (64 (s + 1), x) against row 64 (s + 1) - 1; then [.., + seams_x * H): pixel (y, 64 (s + 1)) against
// column 64 (s + 1) - 1
__global__ void __launch_bounds__(256)
k_obj_seam(int* __restrict__ parent, int H, int W, int conn8, int64_t items_h, int64_t items, int cap, int* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    if (i < items_h) {
        const int s = (int)(i / W), x = (int)(i - (int64_t)s * W), y = (s + 1) * OBJ_TILE;
        const int p = (int)((int64_t)y * W + x);
        if (ob_load(parent + p) < 0) return;
        // neighbours along the seam that lie in the same tile are united already: a pair is skipped where the pair beside it
        // joins the same two sets (as in the tile pass), so a straight contact of n pixels costs one union per tile, not n
        const bool up = ob_load(parent + p - W) >= 0;
        const bool tl = x % OBJ_TILE != 0, tr = (x + 1) % OBJ_TILE != 0 && x + 1 < W;      // x - 1 / x + 1 is in this tile column
        const bool left = tl && ob_load(parent + p - 1) >= 0, right = tr && ob_load(parent + p + 1) >= 0;
        const bool upl = x > 0 && ob_load(parent + p - W - 1) >= 0, upr = x + 1 < W && ob_load(parent + p - W + 1) >= 0;
        if (up && !(left && upl)) ob_union(parent, p, p - W, cap, status);
        if (conn8) {
            if (upl && !(tl && (up || left))) ob_union(parent, p, p - W - 1, cap, status);
            if (upr && !(tr && (up || right))) ob_union(parent, p, p - W + 1, cap, status);
        }
    } else {
        const int64_t j = i - items_h;
        const int s = (int)(j / H), y = (int)(j - (int64_t)s * H), x = (s + 1) * OBJ_TILE;
        const int p = (int)((int64_t)y * W + x);
        if (ob_load(parent + p) < 0) return;
        const bool lf = ob_load(parent + p - 1) >= 0;
        const bool ta = y % OBJ_TILE != 0, tb = (y + 1) % OBJ_TILE != 0 && y + 1 < H;      // y - 1 / y + 1 is in this tile row
        const bool above = ta && ob_load(parent + p - W) >= 0, below = tb && ob_load(parent + p + W) >= 0;
        const bool lfa = y > 0 && ob_load(parent + p - W - 1) >= 0, lfb = y + 1 < H && ob_load(parent + p + W - 1) >= 0;
        if (lf && !(above && lfa)) ob_union(parent, p, p - 1, cap, status);
        if (conn8) {
            if (lfa && !(ta && (lf || above))) ob_union(parent, p, p - W - 1, cap, status);
            if (lfb && !(tb && (lf || below))) ob_union(parent, p, p + W - 1, cap, status);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 3. flatten, count or measure
// bits [lo, hi) of a 64-bit word, 0 <= lo < hi <= 64
__device__ __forceinline__ unsigned long long ob_range(int lo, int hi) {
    const unsigned long long upto = hi >= 64 ? ~0ull : (1ull << hi) - 1ull;
    return upto & ~((1ull << lo) - 1ull);
}
// the end (exclusive) of the run that starts at `lane`: the next run head or unset lane above it
__device__ __forceinline__ int ob_run_end(unsigned long long heads, unsigned long long set, int lane) {
    const unsigned long long above = lane >= 63 ? 0ull : ~((2ull << lane) - 1ull);
    const unsigned long long stop = (heads | ~set) & above;
    return stop ? __ffsll((long long)stop) - 1 : 64;
}
// the root of pixel i (-1: unset or past the scene), written back to parent[i]
__device__ __forceinline__ int ob_flatten(int* parent, int64_t i, int64_t HW, int cap, int* status) {
    if (i >= HW) return -1;
    const int pa = ob_load(parent + i);
    if (pa < 0) return -1;
    const int r = ob_find(parent, pa, cap, status);
    if (r != pa) ob_store(parent + i, r);                              // readers that pass through i see the old ancestor or the root
    return r;
}

// flatten and count the roots of every OBJ_CHUNK pixels for the scan (a root stays a root from the seam pass on)
__global__ void __launch_bounds__(256)
k_obj_flatten_count(int* __restrict__ parent, int64_t HW, int cap, int* __restrict__ sums, int* __restrict__ status) {
    __shared__ int wsum[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * OBJ_CHUNK;
    int nroot = 0;
    for (int k = 0; k < OBJ_CHUNK / 256; ++k) {                        // uniform: every lane reaches the ballot
        const int64_t i = base + k * 256 + threadIdx.x;
        const int r = ob_flatten(parent, i, HW, cap, status);
        nroot += __popcll(__ballot(r >= 0 && (int64_t)r == i));
    }
    if (lane == 0) wsum[wave] = nroot;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// flatten and measure: stat[root] += area, |= OBJ_BORDER.  The smallest root of the block's pixels is its key: a component that
// reaches this chunk from far above (the scene's background in the hole step, a large object) has a smaller root than what starts
// inside the chunk; the key's pixels are counted per wave with one ballot, summed in LDS and added with ONE atomic per block, so
// the one address every block shares sees blocks, not runs.  Every other run of one root within a wave's 64 pixels takes one
// atomicAdd of its length (Guideline 12).
__global__ void __launch_bounds__(256)
k_obj_flatten_measure(int* __restrict__ parent, int64_t HW, int H, int W, int cap, uint32_t* __restrict__ stat, int* __restrict__ status) {
    constexpr int PER = OBJ_CHUNK / 256;
    __shared__ int s_key;
    __shared__ uint32_t s_area, s_border;
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * OBJ_CHUNK;
    if (threadIdx.x == 0) { s_key = INT_MAX; s_area = 0u; s_border = 0u; }
    __syncthreads();
    int r[PER], least = INT_MAX;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        r[k] = ob_flatten(parent, base + k * 256 + threadIdx.x, HW, cap, status);
        if (r[k] >= 0) least = min(least, r[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) least = min(least, __shfl_xor(least, o, 64));
    if (lane == 0 && least != INT_MAX) atomicMin(&s_key, least);
    __syncthreads();
    const int key = s_key;                                             // INT_MAX: no set pixel in this chunk
#pragma unroll
    for (int k = 0; k < PER; ++k) {                                    // uniform: every lane reaches the ballots
        const int64_t i = base + k * 256 + threadIdx.x;
        const bool set = r[k] >= 0, keyed = set && r[k] == key, other = set && !keyed;
        const int prev = __shfl_up(r[k], 1, 64);
        const bool head = other && (lane == 0 || prev != r[k]);
        bool border = false;
        if (set) {
            const int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);        // i < 2^31
            border = y == 0 || y == H - 1 || x == 0 || x == W - 1;
        }
        const unsigned long long K = __ballot(keyed), S = __ballot(other), Hd = __ballot(head), Bd = __ballot(border);
        if (lane == 0 && K) {
            atomicAdd(&s_area, (uint32_t)__popcll(K));
            if (Bd & K) atomicOr(&s_border, 1u);
        }
        if (head) {
            const int end = ob_run_end(Hd, S, lane);
            atomicAdd(stat + r[k], (uint32_t)(end - lane));
            if (Bd & ob_range(lane, end)) atomicOr(stat + r[k], OBJ_BORDER);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_area) {
        atomicAdd(stat + key, s_area);
        if (s_border) atomicOr(stat + key, OBJ_BORDER);
    }
}

// ------------------------------------------------------------------------------------------------ 4. compaction
// one block: sums[b] becomes the number of roots before chunk b, *count their total
__global__ void __launch_bounds__(256)
k_obj_scan_sums(int* __restrict__ sums, int nb, int* __restrict__ count) {
    __shared__ int ws[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int carry = 0;
    for (int base = 0; base < nb; base += 256) {                       // uniform
        const int i = base + threadIdx.x;
        const int v = i < nb ? sums[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) before += ws[w]; total += ws[w]; }
        if (i < nb) sums[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();                                               // ws is written again
    }
    if (threadIdx.x == 0) *count = carry;
}

// rank[p] = 1-based number of the root p in raster order
__global__ void __launch_bounds__(256)
k_obj_rank(const int* __restrict__ parent, int64_t HW, const int* __restrict__ sums, uint32_t* __restrict__ rank) {
    __shared__ int ws[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * OBJ_CHUNK;
    int run = sums[blockIdx.x];
    for (int k = 0; k < OBJ_CHUNK / 256; ++k) {                        // uniform
        const int64_t i = base + k * 256 + threadIdx.x;
        const bool root = i < HW && (int64_t)parent[i] == i;
        const unsigned long long b = __ballot(root);
        if (lane == 0) ws[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) before += ws[w]; total += ws[w]; }
        if (root) rank[i] = (uint32_t)(run + before + __popcll(b & ((1ull << lane) - 1ull)) + 1);
        run += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_obj_relabel(int* __restrict__ labels, int64_t HW, const uint32_t* __restrict__ rank) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const int pa = labels[i];
    labels[i] = pa < 0 ? 0 : (int)rank[pa];
}

// ------------------------------------------------------------------------------------------------ 5. select
enum { OBJ_SEL_BINARY = 0, OBJ_SEL_MIN_AREA = 1, OBJ_SEL_HOLE = 2 };
// BINARY:   out = src != 0
// MIN_AREA: out = src != 0 and area(component of the pixel) >= limit          (parent labels the set pixels of src)
// HOLE:     out = src != 0 or (area <= limit and the component touches no border)   (parent labels the unset pixels of src)
template <int SEL>
__global__ void __launch_bounds__(256)
k_obj_select(const uint8_t* __restrict__ src, int64_t HW, const int* __restrict__ parent, const uint32_t* __restrict__ stat,
             uint32_t limit, uint32_t value, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    bool keep = src[i] != 0;
    if (SEL == OBJ_SEL_MIN_AREA) {
        if (keep) { const int r = parent[i]; keep = r >= 0 && (stat[r] & ~OBJ_BORDER) >= limit; }
    } else if (SEL == OBJ_SEL_HOLE) {
        if (!keep) { const int r = parent[i]; keep = r >= 0 && stat[r] <= limit; }         // the border flag is above every limit
    }
    out[i] = (uint8_t)(keep ? value : 0u);
}

// ------------------------------------------------------------------------------------------------ the object table
__global__ void __launch_bounds__(256)
k_obj_table_init(int n, unsigned long long* __restrict__ area, int* __restrict__ bbox, unsigned long long* __restrict__ overlap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    area[i] = 0ull;
    bbox[4 * (int64_t)i] = INT_MAX; bbox[4 * (int64_t)i + 1] = INT_MAX; bbox[4 * (int64_t)i + 2] = -1; bbox[4 * (int64_t)i + 3] = -1;
    if (overlap) { overlap[2 * (int64_t)i] = 0ull; overlap[2 * (int64_t)i + 1] = 0ull; }
}

__global__ void __launch_bounds__(256)
k_obj_table(const int* __restrict__ labels, int64_t HW, int W, int n, const uint8_t* __restrict__ overlay,
            unsigned long long* __restrict__ area, int* __restrict__ bbox, unsigned long long* __restrict__ overlap) {
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * OBJ_CHUNK;
    for (int k = 0; k < OBJ_CHUNK / 256; ++k) {                        // uniform
        const int64_t i = base + k * 256 + threadIdx.x;
        int lab = 0, y = 0, x = 0;
        bool counted = false, hit = false;
        if (i < HW) {
            lab = labels[i];
            if (lab < 1 || lab > n) lab = 0;                           // never index past the table
            if (lab) {
                y = (int)((uint32_t)i / (uint32_t)W); x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);             // i < 2^31
                if (overlay) { const uint8_t o = overlay[i]; counted = o != 255; hit = counted && o != 0; }
            }
        }
        const int prev = __shfl_up(lab, 1, 64);
        const bool set = lab != 0, head = set && (lane == 0 || prev != lab || x == 0);     // a run stays inside one row
        const unsigned long long S = __ballot(set), Hd = __ballot(head), Cn = __ballot(counted), Ht = __ballot(hit);
        if (head) {
            const int end = ob_run_end(Hd, S, lane), len = end - lane;
            const int64_t o = lab - 1;
            atomicAdd(area + o, (unsigned long long)len);
            atomicMin(bbox + 4 * o, y); atomicMin(bbox + 4 * o + 1, x);
            atomicMax(bbox + 4 * o + 2, y); atomicMax(bbox + 4 * o + 3, x + len - 1);
            if (overlay) {
                const unsigned long long m = ob_range(lane, end);
                const int c = __popcll(Cn & m), h = __popcll(Ht & m);
                if (c) atomicAdd(overlap + 2 * o, (unsigned long long)c);
                if (h) atomicAdd(overlap + 2 * o + 1, (unsigned long long)h);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ launch sequences
namespace {

struct ObjScratch {                                                    // the layout of the scratch buffer
    int64_t parent, stat, sums, mid, tail, bytes;                      // byte offsets; tail: 8 bytes, count slot then status word
};
inline int64_t obj_chunks(int64_t hw) { return (hw + OBJ_CHUNK - 1) / OBJ_CHUNK; }
inline ObjScratch obj_layout(int64_t hw) {
    ObjScratch s;
    s.parent = 0;
    s.stat = s.parent + 4 * hw;
    s.sums = s.stat + 4 * hw;
    s.mid = s.sums + 4 * obj_chunks(hw);
    s.tail = (s.mid + hw + 7) / 8 * 8;
    s.bytes = s.tail + 8;
    return s;
}
inline unsigned obj_grid(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// tile pass and seam pass: the forest of the set (invert: unset) pixels of `in` in `parent`
void obj_forest(const uint8_t* in, int H, int W, int conn8, int invert, int* parent, uint32_t* stat, int* status, hipStream_t s) {
    const int tiles_x = (W + OBJ_TILE - 1) / OBJ_TILE, tiles_y = (H + OBJ_TILE - 1) / OBJ_TILE;
    const unsigned tiles = (unsigned)((int64_t)tiles_x * tiles_y);
    if (stat) k_obj_tile<true><<<tiles, 256, 0, s>>>(in, H, W, conn8, invert, tiles_x, parent, stat, status);
    else      k_obj_tile<false><<<tiles, 256, 0, s>>>(in, H, W, conn8, invert, tiles_x, parent, stat, status);
    const int64_t items_h = (int64_t)(tiles_y - 1) * W, items = items_h + (int64_t)(tiles_x - 1) * H;
    if (items > 0) k_obj_seam<<<obj_grid(items, 256), 256, 0, s>>>(parent, H, W, conn8, items_h, items, (int)((int64_t)H * W), status);
}

inline bool obj_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
    return x == y || (x < y ? y - x < a_bytes : x - y < b_bytes);
}
inline bool obj_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace
}  // namespace stcd

using namespace stcd;

extern "C" {

int64_t stcd_objects_scratch_bytes(int height, int width) {
    if (height < 0 || width < 0 || (int64_t)height * width >= ((int64_t)1 << 31)) return 0;
    return obj_layout((int64_t)height * width).bytes;
}

int stcd_objects_label(const uint8_t* mask, int height, int width, int connectivity, int invert, int32_t* labels, int32_t* count,
                       void* scratch, int64_t scratch_bytes, void* hip_stream) {
    STCD_CHECK(mask && labels && count && scratch, "null pointer argument");
    STCD_CHECK(height >= 0 && width >= 0, "bad shape");
    STCD_CHECK((int64_t)height * width < ((int64_t)1 << 31), "height * width must be below 2^31 (int32 labels)");
    STCD_CHECK(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
    STCD_CHECK(invert == 0 || invert == 1, "invert must be 0 or 1");
    STCD_CHECK(obj_aligned(labels, 4) && obj_aligned(count, 4) && obj_aligned(scratch, 8), "labels and count must be 4-byte, scratch 8-byte aligned");
    const int64_t hw = (int64_t)height * width;
    const ObjScratch L = obj_layout(hw);
    STCD_CHECK(scratch_bytes >= L.bytes && scratch_bytes % 4 == 0, "scratch too small (stcd_objects_scratch_bytes) or no multiple of 4 bytes");
    if (height == 0 || width == 0) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    char* base = (char*)scratch;
    uint32_t* rank = (uint32_t*)(base + L.stat);
    int* sums = (int*)(base + L.sums);
    int* status = (int*)(base + scratch_bytes - 4);
    STCD_HIP(hipMemsetAsync(status, 0, 4, s));
    obj_forest(mask, height, width, connectivity == 8, invert, labels, nullptr, status, s);
    const unsigned chunks = (unsigned)obj_chunks(hw);
    k_obj_flatten_count<<<chunks, 256, 0, s>>>(labels, hw, (int)hw, sums, status);
    k_obj_scan_sums<<<1, 256, 0, s>>>(sums, (int)chunks, count);
    k_obj_rank<<<chunks, 256, 0, s>>>(labels, hw, sums, rank);
    k_obj_relabel<<<obj_grid(hw, 256), 256, 0, s>>>(labels, hw, rank);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_objects_table(const int32_t* labels, int height, int width, int n, const uint8_t* overlay, int64_t* area, int32_t* bbox,
                       int64_t* overlap, void* hip_stream) {
    STCD_CHECK(labels != nullptr, "null pointer argument");
    STCD_CHECK(height >= 0 && width >= 0, "bad shape");
    STCD_CHECK((int64_t)height * width < ((int64_t)1 << 31), "height * width must be below 2^31 (int32 labels)");
    STCD_CHECK(n >= 0 && (int64_t)n <= (int64_t)height * width, "n must be in [0, height * width]");
    STCD_CHECK(n == 0 || (area && bbox), "null pointer argument");
    STCD_CHECK((overlay != nullptr) == (overlap != nullptr) || n == 0, "overlay and overlap go together");
    STCD_CHECK(obj_aligned(labels, 4) && obj_aligned(bbox, 4) && obj_aligned(area, 8) && obj_aligned(overlap, 8), "misaligned table pointer");
    if (height == 0 || width == 0 || n == 0) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    const int64_t hw = (int64_t)height * width;
    unsigned long long* ar = (unsigned long long*)area;
    unsigned long long* ov = (unsigned long long*)overlap;
    k_obj_table_init<<<obj_grid(n, 256), 256, 0, s>>>(n, ar, bbox, ov);
    k_obj_table<<<(unsigned)obj_chunks(hw), 256, 0, s>>>(labels, hw, width, n, overlay, ar, bbox, ov);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_mask_filter_objects(const uint8_t* in, int height, int width, int connectivity, int64_t min_area, int64_t max_hole,
                             int mask_value, uint8_t* out, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    STCD_CHECK(in && out && scratch, "null pointer argument");
    STCD_CHECK(height >= 0 && width >= 0, "bad shape");
    STCD_CHECK((int64_t)height * width < ((int64_t)1 << 31), "height * width must be below 2^31 (int32 labels)");
    STCD_CHECK(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
    STCD_CHECK(max_hole >= 0, "max_hole must be >= 0");
    STCD_CHECK(mask_value >= 1 && mask_value <= 255, "mask_value must be in [1, 255]");
    STCD_CHECK(obj_aligned(scratch, 8), "scratch must be 8-byte aligned");
    const int64_t hw = (int64_t)height * width;
    const ObjScratch L = obj_layout(hw);
    STCD_CHECK(scratch_bytes >= L.bytes && scratch_bytes % 4 == 0, "scratch too small (stcd_objects_scratch_bytes) or no multiple of 4 bytes");
    STCD_CHECK(!obj_overlap(in, (uint64_t)hw, out, (uint64_t)hw), "out must not overlap in");
    STCD_CHECK(!obj_overlap(in, (uint64_t)hw, scratch, (uint64_t)scratch_bytes) && !obj_overlap(out, (uint64_t)hw, scratch, (uint64_t)scratch_bytes),
               "scratch must not overlap in or out");
    if (height == 0 || width == 0) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    char* base = (char*)scratch;
    int* parent = (int*)(base + L.parent);
    uint32_t* stat = (uint32_t*)(base + L.stat);
    uint8_t* mid = (uint8_t*)(base + L.mid);
    int* status = (int*)(base + scratch_bytes - 4);
    const bool conn8 = connectivity == 8;
    const unsigned chunks = (unsigned)obj_chunks(hw), px = obj_grid(hw, 256);
    const uint32_t value = (uint32_t)mask_value;
    STCD_HIP(hipMemsetAsync(status, 0, 4, s));
    const bool hole = max_hole > 0;
    const uint8_t* src = in;                                           // what step 2 works on
    if (min_area > 1) {                                                // step 1: set components below min_area are cleared
        const uint32_t limit = (uint32_t)std::min<int64_t>(min_area, (int64_t)1 << 31);    // an area is below 2^31
        uint8_t* dst = hole ? mid : out;
        obj_forest(in, height, width, conn8, 0, parent, stat, status, s);
        k_obj_flatten_measure<<<chunks, 256, 0, s>>>(parent, hw, height, width, (int)hw, stat, status);
        k_obj_select<OBJ_SEL_MIN_AREA><<<px, 256, 0, s>>>(in, hw, parent, stat, limit, hole ? 1u : value, dst);
        src = dst;
    }
    if (hole) {                                                        // step 2: unset components of at most max_hole off the border are set
        const uint32_t limit = (uint32_t)std::min<int64_t>(max_hole, ((int64_t)1 << 31) - 1);
        obj_forest(src, height, width, !conn8, 1, parent, stat, status, s);
        k_obj_flatten_measure<<<chunks, 256, 0, s>>>(parent, hw, height, width, (int)hw, stat, status);
        k_obj_select<OBJ_SEL_HOLE><<<px, 256, 0, s>>>(src, hw, parent, stat, limit, value, out);
    } else if (src == in) {
        k_obj_select<OBJ_SEL_BINARY><<<px, 256, 0, s>>>(in, hw, nullptr, nullptr, 0u, value, out);
    }
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
