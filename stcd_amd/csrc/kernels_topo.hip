// kernels_topo.hip -- change polygons on the device: which edges of a ring set conflict, and the repair loop that makes the
// Douglas-Peucker rings of kernels_simplify.hip topology-safe (gfx950), with their C-ABI entries.  tests/topology_spec.py states
// every output in plain Python and include/stcd_hip.h the rule set.  Integers only: an orientation is below 2^30, a key is that of
// kernels_simplify.hip, so every output is a pure function of the input.
//
// The state of the repair loop is the keep byte per input vertex that the simplify count phase left, the list kv of the kept
// vertices (one CURRENT EDGE starts at each and ends at the next kept vertex of its ring) and twice the area of every ring's kept
// vertices, which a restore updates by the triangle it adds.  One detection pass:
//     k_topo_sum / k_topo_scan / k_topo_excl   the keep bytes to places (the scan pattern of the simplify write phase)
//     k_topo_compact / k_topo_cur              kv, and per current edge its two ends (packed) and the length of its chain
//     k_topo_gcount / (scan) / k_topo_gfill    every edge into the cells of a uniform grid its segment passes through: a row walk
//                                              with exact floor / ceil columns per row, never the cells of the bounding box
//     k_topo_pairs     a block per non-empty cell (grid-stride): the cell's edges staged in LDS in tiles of TP_TILE, every lane tests
//                      its own edge against the tile and sets ITS OWN flag with a plain byte store: no atomics, no pair list
//     k_topo_pockets   a wavefront per current edge with dropped vertices: the box of its chain, the first vertices of the other
//                      rings in the grid rows of that box (entered once, by k_topo_points), on-or-inside with the lanes striding
//                      over the chain, which is read from global memory whatever its length
//     k_topo_tally     the flagged edges and pocket hits, one atomic per wavefront
// and, where the round restores:
//     k_topo_restore   a wavefront per flagged edge with dropped vertices: arg-max of the key over the chain, lowest index on ties
//     k_topo_check / k_topo_ringfix   the sign rule on every ring whose mask changed, and the counts for the host
// No thread walks a ring; a thread does walk the grid rows of ONE edge.  Nothing here allocates, synchronises or copies to the host.
#include <algorithm>
#include <climits>

#include "common.h"
#include "ring_scan.h"

namespace stcd {

void sm_state_of(void* scratch, int64_t n_rings, int64_t n_vertices, uint8_t** keep, long long** area, int** status);   // kernels_simplify.hip

#define TP_TILE 256                            // TOPO_TILE of stcd_amd/objects.py: edges of a cell staged in LDS at a time
#define TP_CHUNK 4096                          // elements per block of the scans: 256 threads x 16
#define TP_COORD_MAX 16384
#define TP_CELL_DEFAULT 16
#define TP_PAIR_GRID 16384                     // blocks of the grid-stride pass over the cells

enum { TP_ST_RANGE = 1, TP_ST_ROUNDS = 2, TP_ST_OFFSETS = 4, TP_ST_MISMATCH = 8, TP_ST_CAPACITY = 16 };

struct TpHeader {                              // the first 64 bytes of the scratch buffer
    long long rings, vertices, edges;          // edges: the current edges (kept vertices)
    int status, pad_;
    long long entries, restored, flagged, hits; // of the pass under way
};

__device__ __forceinline__ int tp_pack(int y, int x) { return (y << 16) | x; }
__device__ __forceinline__ int tp_y(int p) { return p >> 16; }
__device__ __forceinline__ int tp_x(int p) { return p & 0xffff; }
__device__ __forceinline__ int tp_orient(int a, int b, int c) {
    return (tp_y(b) - tp_y(a)) * (tp_x(c) - tp_x(a)) - (tp_x(b) - tp_x(a)) * (tp_y(c) - tp_y(a));
}
__device__ __forceinline__ bool tp_in_box(int p, int a, int b) {
    return min(tp_y(a), tp_y(b)) <= tp_y(p) && tp_y(p) <= max(tp_y(a), tp_y(b)) && min(tp_x(a), tp_x(b)) <= tp_x(p) && tp_x(p) <= max(tp_x(a), tp_x(b));
}
// rule CONFLICT of tests/topology_spec.py
__device__ __forceinline__ bool tp_conflict(int a, int b, int c, int d) {
    if (a == b || c == d) return false;
    if (max(tp_y(a), tp_y(b)) < min(tp_y(c), tp_y(d)) || max(tp_y(c), tp_y(d)) < min(tp_y(a), tp_y(b)) ||
        max(tp_x(a), tp_x(b)) < min(tp_x(c), tp_x(d)) || max(tp_x(c), tp_x(d)) < min(tp_x(a), tp_x(b)))
        return false;                                                  // closed segments that share a point have boxes that share one
    const int o1 = tp_orient(a, b, c), o2 = tp_orient(a, b, d), o3 = tp_orient(c, d, a), o4 = tp_orient(c, d, b);
    if ((o1 | o2 | o3 | o4) == 0) {
        const bool ony = tp_y(a) != tp_y(b);
        const int a0 = ony ? tp_y(a) : tp_x(a), b0 = ony ? tp_y(b) : tp_x(b), c0 = ony ? tp_y(c) : tp_x(c), d0 = ony ? tp_y(d) : tp_x(d);
        return min(max(a0, b0), max(c0, d0)) - max(min(a0, b0), min(c0, d0)) > 0;
    }
    if (a == c || a == d || b == c || b == d) return false;
    if (((o1 < 0 && o2 > 0) || (o2 < 0 && o1 > 0)) && ((o3 < 0 && o4 > 0) || (o4 < 0 && o3 > 0))) return true;
    return (o1 == 0 && tp_in_box(c, a, b)) || (o2 == 0 && tp_in_box(d, a, b)) || (o3 == 0 && tp_in_box(a, c, d)) || (o4 == 0 && tp_in_box(b, c, d));
}
// the key of kernels_simplify.hip (rule 1 there)
__device__ __forceinline__ unsigned long long tp_key(int p, int a, int b) {
    const long long ey = tp_y(p) - tp_y(a), ex = tp_x(p) - tp_x(a), dy = tp_y(b) - tp_y(a), dx = tp_x(b) - tp_x(a);
    const long long L = dy * dy + dx * dx, e2 = ey * ey + ex * ex;
    if (L == 0) return (unsigned long long)e2;
    const long long t = ey * dy + ex * dx;
    if (t <= 0) return (unsigned long long)(e2 * L);
    if (t >= L) { const long long fy = tp_y(p) - tp_y(b), fx = tp_x(p) - tp_x(b); return (unsigned long long)((fy * fy + fx * fx) * L); }
    const long long c = ey * dx - ex * dy;
    return (unsigned long long)(c * c);
}
__device__ __forceinline__ long long tp_side(int t, int h) { return (long long)tp_x(t) * tp_y(h) - (long long)tp_x(h) * tp_y(t); }
__device__ __forceinline__ int tp_floordiv(int n, int d) {             // d > 0
    const int q = n / d;
    return q - ((n % d) < 0);
}
__device__ __forceinline__ int tp_load_xy(const int2* __restrict__ vertices, long long v) {
    const int2 p = vertices[v];
    return tp_pack(p.x, p.y);                                          // int2.x is the first of the pair: y
}

// f(cell) for every cell of the grid (side 1 << sh, G cells a row) the closed segment (a, b) passes through: per cell row, the
// columns from the floor of the least x to the ceiling of the largest x of the segment within that row's closed slab.
template <class F>
__device__ __forceinline__ void tp_walk(int a, int b, int sh, int G, F f) {
    if (tp_y(a) > tp_y(b)) { const int t = a; a = b; b = t; }
    const int ay = tp_y(a), ax = tp_x(a), by = tp_y(b), bx = tp_x(b), dy = by - ay, dx = bx - ax;
    for (int r = ay >> sh; r <= (by >> sh); ++r) {
        int xlo = min(ax, bx), xhi = max(ax, bx);
        if (dy != 0) {
            const int n0 = (max(ay, r << sh) - ay) * dx, n1 = (min(by, (r + 1) << sh) - ay) * dx;     // at most 2^28
            const int f0 = tp_floordiv(n0, dy), f1 = tp_floordiv(n1, dy);
            const int c0 = f0 + (n0 % dy != 0), c1 = f1 + (n1 % dy != 0);
            xlo = ax + min(f0, f1); xhi = ax + max(c0, c1);
        }
        for (int cx = xlo >> sh; cx <= (xhi >> sh); ++cx) f(r * G + cx);
    }
}

__device__ __forceinline__ bool tp_dead(const TpHeader* hdr) { return hdr->status != 0; }

// ------------------------------------------------------------------------------------------------ validation and per-vertex tables
__global__ void __launch_bounds__(256)
k_topo_validate(const int* __restrict__ vertices, const long long* __restrict__ offsets, long long R, long long V, TpHeader* __restrict__ hdr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int st = 0;
    if (i < V) {
        const int y = vertices[2 * i], x = vertices[2 * i + 1];
        if ((unsigned)y > (unsigned)TP_COORD_MAX || (unsigned)x > (unsigned)TP_COORD_MAX) st |= TP_ST_RANGE;
    }
    if (i < R) {
        const long long o0 = offsets[i], o1 = offsets[i + 1];
        if (o0 < 0 || o1 < o0 || o1 > V || (i == 0 && o0 != 0) || (i == R - 1 && o1 != V)) st |= TP_ST_OFFSETS;
    }
    if (i == 0 && R == 0 && (V != 0 || offsets[0] != 0)) st |= TP_ST_OFFSETS;
    if (st) atomicOr(&hdr->status, st);
    if (i == 0) { hdr->rings = R; hdr->vertices = V; }
}

// rid[v]: the ring of vertex v (the last r with offsets[r] <= v); ain[r]: twice the signed area of the input ring
__global__ void __launch_bounds__(256)
k_topo_rid(const int2* __restrict__ vertices, const long long* __restrict__ offsets, long long R, long long V, const TpHeader* __restrict__ hdr,
           int* __restrict__ rid, unsigned long long* __restrict__ ain) {
    if (tp_dead(hdr)) return;
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    long long lo = 0, hi = R;                                          // the first t in [0, R] with offsets[t] > v: offsets[R] == V > v
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (offsets[mid] > v) hi = mid; else lo = mid + 1;
    }
    const long long r = lo - 1;
    rid[v] = (int)r;
    if (ain) {
        const long long nx = v + 1 < offsets[r + 1] ? v + 1 : offsets[r];
        atomicAdd(ain + r, (unsigned long long)tp_side(tp_load_xy(vertices, v), tp_load_xy(vertices, nx)));
    }
}

// every edge of the ring set as it stands (stcd_rings_conflicts)
__global__ void __launch_bounds__(256)
k_topo_all(const int2* __restrict__ vertices, const long long* __restrict__ offsets, long long V, TpHeader* __restrict__ hdr,
           const int* __restrict__ rid, int* __restrict__ ea, int* __restrict__ eb) {
    if (tp_dead(hdr)) return;
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v == 0) hdr->edges = V;
    if (v >= V) return;
    const long long r = rid[v];
    const long long nx = v + 1 < offsets[r + 1] ? v + 1 : offsets[r];
    ea[v] = tp_load_xy(vertices, v);
    eb[v] = tp_load_xy(vertices, nx);
}

// ------------------------------------------------------------------------------------------------ scans (of bytes and of counts)
template <typename T>
__global__ void __launch_bounds__(256)
k_topo_sum(const T* __restrict__ in, long long n, const TpHeader* __restrict__ hdr, long long* __restrict__ sums) {
    __shared__ long long wsum[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * TP_CHUNK + threadIdx.x;
    long long s = 0;
    if (!tp_dead(hdr))
        for (int k = 0; k < TP_CHUNK / 256; ++k)
            if (first + k * 256 < n) s += (long long)in[first + k * 256];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// which: 0 the kept vertices (hdr->edges, checked against n_expect), 1 the grid entries (hdr->entries, checked against the capacity)
__global__ void __launch_bounds__(256)
k_topo_scan(long long* __restrict__ sums, int64_t nb, TpHeader* __restrict__ hdr, int which, long long limit, int* __restrict__ last,
            const int* __restrict__ round0) {
    __shared__ long long ws[4];
    const long long total = rg_block_scan(sums, nb, 1, ws);
    if (threadIdx.x == 0 && !tp_dead(hdr)) {
        if (round0) hdr->status |= *round0 & (TP_ST_RANGE | TP_ST_ROUNDS | TP_ST_OFFSETS);      // what the simplify count phase found
        if (which == 0) {
            hdr->edges = total;
            if (limit >= 0 && total != limit) hdr->status |= TP_ST_MISMATCH;
            if (last) *last = (int)total;                              // pos[V]
        } else {
            hdr->entries = total;
            if (total > limit) hdr->status |= TP_ST_CAPACITY;
        }
    }
}

// out[i] = the sum of in[0 .. i-1]; in place where out == in (each element is read, then written, by one thread)
template <typename T>
__global__ void __launch_bounds__(256)
k_topo_excl(const T* in, long long n, const TpHeader* __restrict__ hdr, const long long* __restrict__ sums, int* out) {
    __shared__ int ws[4];
    if (tp_dead(hdr)) return;                                          // uniform over the grid
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * TP_CHUNK + threadIdx.x;
    long long run = sums[blockIdx.x];
    for (int k = 0; k < TP_CHUNK / 256; ++k) {                         // uniform
        const int64_t i = first + k * 256;
        const int f = i < n ? (int)in[i] : 0;
        const int inc = (int)rg_wave_scan((long long)f, lane);
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) before += ws[w]; total += ws[w]; }
        if (i < n) out[i] = (int)(run + before + inc - f);
        run += total;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ the current edges
__global__ void __launch_bounds__(256)
k_topo_compact(const uint8_t* __restrict__ keep, const int* __restrict__ pos, long long V, const TpHeader* __restrict__ hdr, int* __restrict__ kv) {
    if (tp_dead(hdr)) return;
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V && (keep[v] & 1)) kv[pos[v]] = (int)v;                   // pos[v] < hdr->edges <= V
}

__global__ void __launch_bounds__(256)
k_topo_cur(const int2* __restrict__ vertices, const long long* __restrict__ offsets, const TpHeader* __restrict__ hdr, const int* __restrict__ rid,
           const int* __restrict__ kv, int* __restrict__ ea, int* __restrict__ eb, int* __restrict__ len) {
    if (tp_dead(hdr)) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, E = hdr->edges;
    if (e >= E) return;
    const int v = kv[e], r = rid[v];
    const bool inner = e + 1 < E && rid[kv[e + 1]] == r;               // the next kept vertex is this ring's
    const long long head = inner ? kv[e + 1] : offsets[r];
    ea[e] = tp_load_xy(vertices, v);
    eb[e] = tp_load_xy(vertices, head);
    len[e] = (int)((inner ? (long long)kv[e + 1] : offsets[r + 1]) - v);     // j - i
}

// ------------------------------------------------------------------------------------------------ the grid
__global__ void __launch_bounds__(256)
k_topo_gcount(const int* __restrict__ ea, const int* __restrict__ eb, const TpHeader* __restrict__ hdr, int sh, int G, int* __restrict__ count) {
    if (tp_dead(hdr)) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= hdr->edges) return;
    const int a = ea[e], b = eb[e];
    if (a == b) return;                                                // a zero-length edge conflicts with nothing
    tp_walk(a, b, sh, G, [&](int cell) { atomicAdd(count + cell, 1); });
}

// start[c] is the place of cell c's first entry and becomes the place after its last: cell c is [c ? start[c - 1] : 0, start[c])
__global__ void __launch_bounds__(256)
k_topo_gfill(const int* __restrict__ ea, const int* __restrict__ eb, const TpHeader* __restrict__ hdr, int sh, int G, int* __restrict__ start,
             int* __restrict__ entries, long long cap) {
    if (tp_dead(hdr)) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= hdr->edges) return;
    const int a = ea[e], b = eb[e];
    if (a == b) return;
    tp_walk(a, b, sh, G, [&](int cell) {
        const int at = atomicAdd(start + cell, 1);
        if (at >= 0 && at < cap) entries[at] = (int)e;
    });
}

// the first vertex of every ring that has one, as a point of the same grid
__global__ void __launch_bounds__(256)
k_topo_points(const int2* __restrict__ vertices, const long long* __restrict__ offsets, long long R, const TpHeader* __restrict__ hdr, int sh, int G,
              int* __restrict__ pstart, int* __restrict__ pent, int fill) {
    if (tp_dead(hdr)) return;
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R || offsets[r + 1] == offsets[r]) return;
    const int2 p = vertices[offsets[r]];
    const int cell = (p.x >> sh) * G + (p.y >> sh);
    const int at = atomicAdd(pstart + cell, 1);
    if (fill && at >= 0 && at < R) pent[at] = (int)r;
}

__global__ void __launch_bounds__(TP_TILE)
k_topo_pairs(const int* __restrict__ ea, const int* __restrict__ eb, const TpHeader* __restrict__ hdr, const int* __restrict__ start,
             const int* __restrict__ entries, long long ncells, uint8_t* __restrict__ flags) {
    __shared__ int te[TP_TILE], ta[TP_TILE], tb[TP_TILE];
    if (tp_dead(hdr)) return;
    const long long E = hdr->edges, N = hdr->entries;
    const int tid = threadIdx.x;
    for (long long c = blockIdx.x; c < ncells; c += gridDim.x) {       // uniform over the block
        const long long lo = c ? start[c - 1] : 0, hi = start[c];
        if (lo < 0 || hi > N || hi - lo < 2) continue;
        const int m = (int)(hi - lo);
        for (int bi = 0; bi < m; bi += TP_TILE) {
            const bool mine = bi + tid < m;
            const int e = mine ? entries[lo + bi + tid] : -1;
            const bool ok = mine && e >= 0 && e < E;                   // an index is checked before it is used
            const int a = ok ? ea[e] : 0, b = ok ? eb[e] : 0;
            bool hit = false;
            for (int bj = 0; bj < m; bj += TP_TILE) {
                __syncthreads();
                if (bj + tid < m) {
                    const int f = entries[lo + bj + tid];
                    const bool fk = f >= 0 && f < E;
                    te[tid] = fk ? f : -1; ta[tid] = fk ? ea[f] : 0; tb[tid] = fk ? eb[f] : 0;     // a == b conflicts with nothing
                }
                __syncthreads();
                const int cnt = min(TP_TILE, m - bj);
                if (ok && !hit)
                    for (int k = 0; k < cnt; ++k)
                        if (te[k] != e && tp_conflict(a, b, ta[k], tb[k])) { hit = true; break; }
            }
            if (hit) flags[e] = 1;
        }
        __syncthreads();
    }
}

// what the lanes of a wavefront share about current edge e
struct TpChain { int v0, r, len; long long base, n; };
__device__ __forceinline__ bool tp_chain(long long e, const TpHeader* hdr, const long long* __restrict__ offsets, const int* __restrict__ rid,
                                         const int* __restrict__ kv, const int* __restrict__ len, TpChain& c) {
    if (e >= hdr->edges) return false;
    c.len = len[e];
    if (c.len < 2) return false;
    c.v0 = kv[e]; c.r = rid[c.v0]; c.base = offsets[c.r]; c.n = offsets[c.r + 1] - c.base;
    return c.v0 + (long long)c.len <= c.base + c.n;                    // the chain stays within its ring
}
// vertex k of the pocket P[i .. j % n], 0 <= k <= len
__device__ __forceinline__ int tp_chain_xy(const int2* __restrict__ vertices, const TpChain& c, int k) {
    const long long v = (long long)c.v0 + k;
    return tp_load_xy(vertices, v < c.base + c.n ? v : c.base);
}

__global__ void __launch_bounds__(256)
k_topo_pockets(const int2* __restrict__ vertices, const long long* __restrict__ offsets, long long R, const TpHeader* __restrict__ hdr,
               const int* __restrict__ rid, const int* __restrict__ kv, const int* __restrict__ len, int sh, int G, const int* __restrict__ pstart,
               const int* __restrict__ pent, uint8_t* __restrict__ pflags) {
    if (tp_dead(hdr)) return;
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);      // uniform over the wavefront, as is all control flow below
    TpChain c;
    if (!tp_chain(e, hdr, offsets, rid, kv, len, c)) return;
    const int m = c.len + 1;                                           // the pocket's vertices, and its sides
    int y0 = INT_MAX, y1 = -1, x0 = INT_MAX, x1 = -1;
    for (int k = lane; k < m; k += 64) {
        const int p = tp_chain_xy(vertices, c, k);
        y0 = min(y0, tp_y(p)); y1 = max(y1, tp_y(p)); x0 = min(x0, tp_x(p)); x1 = max(x1, tp_x(p));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        y0 = min(y0, __shfl_xor(y0, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
        x0 = min(x0, __shfl_xor(x0, o, 64)); x1 = max(x1, __shfl_xor(x1, o, 64));
    }
    for (int cy = y0 >> sh; cy <= (y1 >> sh); ++cy) {
        const long long c0 = (long long)cy * G + (x0 >> sh), c1 = (long long)cy * G + (x1 >> sh);
        const long long lo = c0 ? pstart[c0 - 1] : 0, hi = pstart[c1];       // the cells of a row follow each other
        if (lo < 0 || hi > R) continue;
        for (long long base = lo; base < hi; base += 64) {
            int p = 0;
            bool cand = false;
            if (base + lane < hi) {
                const long long s = pent[base + lane];
                if (s >= 0 && s < R && s != c.r) {
                    p = tp_load_xy(vertices, offsets[s]);
                    cand = tp_y(p) >= y0 && tp_y(p) <= y1 && tp_x(p) >= x0 && tp_x(p) <= x1;
                }
            }
            unsigned long long todo = __ballot(cand);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int q = __shfl(p, l, 64);
                bool on = false, odd = false;
                for (int k = lane; k < m; k += 64) {
                    int u = tp_chain_xy(vertices, c, k), v = tp_chain_xy(vertices, c, k + 1 == m ? 0 : k + 1);
                    if (tp_orient(u, v, q) == 0 && tp_in_box(q, u, v)) on = true;
                    if (tp_y(u) == tp_y(v)) continue;
                    if (tp_y(u) > tp_y(v)) { const int t = u; u = v; v = t; }
                    if (tp_y(u) <= tp_y(q) && tp_y(q) < tp_y(v) &&
                        (tp_x(v) - tp_x(u)) * (tp_y(q) - tp_y(u)) > (tp_x(q) - tp_x(u)) * (tp_y(v) - tp_y(u)))
                        odd = !odd;
                }
                if (__ballot(on) != 0 || (__popcll(__ballot(odd)) & 1)) {
                    if (lane == 0) pflags[e] = 1;
                    return;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256)
k_topo_tally(TpHeader* __restrict__ hdr, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ pflags) {
    if (tp_dead(hdr)) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = e < hdr->edges;
    const int f = __popcll(__ballot(in && flags[e])), h = __popcll(__ballot(in && pflags && pflags[e]));
    if ((threadIdx.x & 63) == 0) {
        if (f) atomicAdd((unsigned long long*)&hdr->flagged, (unsigned long long)f);
        if (h) atomicAdd((unsigned long long*)&hdr->hits, (unsigned long long)h);
    }
}

__global__ void __launch_bounds__(256)
k_topo_restore(const int2* __restrict__ vertices, const long long* __restrict__ offsets, TpHeader* __restrict__ hdr, const int* __restrict__ rid,
               const int* __restrict__ kv, const int* __restrict__ len, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ pflags,
               uint8_t* __restrict__ keep, unsigned long long* __restrict__ area, int* __restrict__ changed) {
    if (tp_dead(hdr)) return;
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    TpChain c;
    if (!tp_chain(e, hdr, offsets, rid, kv, len, c)) return;
    if (!(flags[e] | pflags[e])) return;
    const int a = tp_chain_xy(vertices, c, 0), b = tp_chain_xy(vertices, c, c.len);
    unsigned long long bk = 0;
    int bi = INT_MAX;
    for (int k = 1 + lane; k < c.len; k += 64) {                       // ascending: a lane keeps its lowest
        const unsigned long long v = tp_key(tp_chain_xy(vertices, c, k), a, b);
        if (bi == INT_MAX || v > bk) { bk = v; bi = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(bk, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != INT_MAX && (bi == INT_MAX || ok > bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; }
    }
    if (lane == 0) {                                                   // 1 <= bi < len
        const int w = tp_chain_xy(vertices, c, bi);
        keep[c.v0 + bi] = 1;
        atomicAdd(area + c.r, (unsigned long long)(tp_side(a, w) + tp_side(w, b) - tp_side(a, b)));
        changed[c.r] = 1;
        atomicAdd((unsigned long long*)&hdr->restored, 1ull);
    }
}

// rule 4 of the repair loop: a changed ring whose kept area is 0 or has the other sign keeps all of its vertices
__device__ __forceinline__ bool tp_bad(long long a, long long a_in) { return a == 0 || (a > 0) != (a_in > 0); }

__global__ void __launch_bounds__(256)
k_topo_check(long long V, TpHeader* __restrict__ hdr, const int* __restrict__ rid, const int* __restrict__ changed, const long long* __restrict__ area,
             const long long* __restrict__ ain, uint8_t* __restrict__ keep) {
    if (tp_dead(hdr)) return;
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    bool add = false;
    if (v < V) {
        const int r = rid[v];
        add = changed[r] && tp_bad(area[r], ain[r]) && !(keep[v] & 1);
        if (add) keep[v] = 1;
    }
    const int n = __popcll(__ballot(add));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd((unsigned long long*)&hdr->restored, (unsigned long long)n);
}

__global__ void __launch_bounds__(256)
k_topo_ringfix(long long R, const TpHeader* __restrict__ hdr, int* __restrict__ changed, long long* __restrict__ area, const long long* __restrict__ ain) {
    if (tp_dead(hdr)) return;
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R || !changed[r]) return;
    if (tp_bad(area[r], ain[r])) area[r] = ain[r];
    changed[r] = 0;
}

// a round starts: the capacity and mismatch bits are those of one call, the counters those of one pass
__global__ void k_topo_reset(TpHeader* __restrict__ hdr) {
    hdr->status &= ~(TP_ST_CAPACITY | TP_ST_MISMATCH);
    hdr->entries = hdr->restored = hdr->flagged = hdr->hits = 0;
}

// counts: (status, current edges, grid entries, restored, flagged edges, pocket hits, 0, 0)
__global__ void k_topo_counts(const TpHeader* __restrict__ hdr, long long* __restrict__ counts) {
    const int st = hdr->status;
    counts[0] = st; counts[1] = hdr->edges; counts[2] = hdr->entries; counts[3] = hdr->restored;
    counts[4] = st ? -1 : hdr->flagged; counts[5] = st ? -1 : hdr->hits; counts[6] = counts[7] = 0;
}

__global__ void __launch_bounds__(256)
k_topo_wverts(TpHeader* __restrict__ hdr, long long R, long long V, long long n_out, const int2* __restrict__ vertices, const int* __restrict__ kv,
              int2* __restrict__ out) {
    const bool ok = hdr->status == 0 && hdr->rings == R && hdr->vertices == V && hdr->edges == n_out;
    if (!ok) {                                                         // uniform over the grid: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&hdr->status, TP_ST_MISMATCH);
        return;
    }
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_out) return;
    const int v = kv[e];
    if (v >= 0 && v < V) out[e] = vertices[v];
}

__global__ void __launch_bounds__(256)
k_topo_wrings(const TpHeader* __restrict__ hdr, long long R, long long V, long long n_out, const long long* __restrict__ offsets,
              const int* __restrict__ pos, const long long* __restrict__ area, long long* __restrict__ out_offsets, long long* __restrict__ out_area2) {
    if ((hdr->status & ~TP_ST_MISMATCH) != 0 || hdr->rings != R || hdr->vertices != V || hdr->edges != n_out) return;
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r > R) return;
    const long long o = offsets[r];
    out_offsets[r] = o >= 0 && o < V ? (long long)pos[o] : n_out;
    if (r < R) out_area2[r] = area[r];
}

// ------------------------------------------------------------------------------------------------ launch sequences
namespace {

struct TpScratch {                                                     // byte offsets into the scratch buffer
    int64_t sums, ain, area, changed, rid, kv, ea, eb, len, pos, pent, gstart, pstart, flags, pflags, simplify, bytes;
};
inline int64_t tp_chunks(int64_t n) { return std::max<int64_t>(1, (n + TP_CHUNK - 1) / TP_CHUNK); }
inline int64_t tp_even(int64_t n) { return (n + 1) / 2 * 2; }
inline int tp_shift(int cell) {                                        // log2 of the cell's side, -1 for a side that is refused
    if (cell == 0) cell = TP_CELL_DEFAULT;
    for (int sh = 3; sh <= 8; ++sh)
        if (cell == (1 << sh)) return sh;
    return -1;
}
inline int64_t tp_cells(int sh) { const int64_t G = (TP_COORD_MAX >> sh) + 1; return G * G; }
inline TpScratch tp_layout(int64_t R, int64_t V, int sh) {
    TpScratch s;
    const int64_t NC = tp_cells(sh);
    int64_t o = (int64_t)sizeof(TpHeader);
    s.sums = o; o += 8 * tp_chunks(std::max(V, NC));
    s.ain = o; o += 8 * R;
    s.area = o; o += 8 * R;
    s.changed = o; o += 4 * tp_even(R);
    int64_t* per[] = {&s.rid, &s.kv, &s.ea, &s.eb, &s.len};
    for (int64_t* p : per) { *p = o; o += 4 * tp_even(V); }
    s.pos = o; o += 4 * tp_even(V + 1);
    s.pent = o; o += 4 * tp_even(R);
    s.gstart = o; o += 4 * tp_even(NC);
    s.pstart = o; o += 4 * tp_even(NC);
    s.flags = o; o += (V + 7) / 8 * 8;
    s.pflags = o; o += (V + 7) / 8 * 8;
    s.simplify = o; o += stcd_rings_simplify_scratch_bytes(R, V);
    s.bytes = (o + 7) / 8 * 8;
    return s;
}
inline bool tp_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool tp_sizes_ok(int64_t R, int64_t V) { return R >= 0 && V >= 0 && R < ((int64_t)1 << 31) && V < ((int64_t)1 << 31); }
inline unsigned tp_blocks(int64_t n, int per = 256) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

// the scan of n ints at a, in place, with the total checked by k_topo_scan (which == 1) -- three launches
inline void tp_scan_counts(int* a, int64_t n, TpHeader* hdr, long long* sums, long long cap, hipStream_t s) {
    const unsigned nb = (unsigned)tp_chunks(n);
    k_topo_sum<int><<<nb, 256, 0, s>>>(a, n, hdr, sums);
    k_topo_scan<<<1, 256, 0, s>>>(sums, nb, hdr, 1, cap, nullptr, nullptr);
    k_topo_excl<int><<<nb, 256, 0, s>>>(a, n, hdr, sums, a);
}

// the edges ea / eb (hdr->edges of them, at most n_edges) into the grid and against each other: flags[e] = 1 where e conflicts
inline int tp_detect(char* b, const TpScratch& L, int sh, int64_t n_edges, uint8_t* flags, int* entries, int64_t max_entries, hipStream_t s) {
    TpHeader* hdr = (TpHeader*)b;
    const int G = (TP_COORD_MAX >> sh) + 1;
    const int64_t NC = tp_cells(sh);
    int* gstart = (int*)(b + L.gstart);
    const int* ea = (const int*)(b + L.ea);
    const int* eb = (const int*)(b + L.eb);
    if (hipMemsetAsync(gstart, 0, 4 * NC, s) != hipSuccess || hipMemsetAsync(flags, 0, n_edges, s) != hipSuccess) return 1;
    k_topo_gcount<<<tp_blocks(n_edges), 256, 0, s>>>(ea, eb, hdr, sh, G, gstart);
    tp_scan_counts(gstart, NC, hdr, (long long*)(b + L.sums), max_entries, s);
    k_topo_gfill<<<tp_blocks(n_edges), 256, 0, s>>>(ea, eb, hdr, sh, G, gstart, entries, max_entries);
    k_topo_pairs<<<(unsigned)std::min<int64_t>(NC, TP_PAIR_GRID), TP_TILE, 0, s>>>(ea, eb, hdr, gstart, entries, NC, flags);
    return 0;
}

}  // namespace
}  // namespace stcd

using namespace stcd;

#define TP_CHECK_COMMON()                                                                                                         \
    STCD_CHECK(vertices && offsets && scratch && counts, "null pointer argument");                                                \
    STCD_CHECK(n_rings >= 0 && n_vertices >= 0, "n_rings and n_vertices must be >= 0");                                           \
    STCD_CHECK(tp_sizes_ok(n_rings, n_vertices), "n_rings and n_vertices must be below 2^31");                                    \
    STCD_CHECK(tp_shift(cell) >= 0, "cell must be 0 or a power of two from 8 to 256");                                            \
    STCD_CHECK(tp_aligned(vertices, 8) && tp_aligned(offsets, 8) && tp_aligned(scratch, 8) && tp_aligned(counts, 8),              \
               "vertices, offsets, counts and scratch must be 8-byte aligned");                                                   \
    STCD_CHECK(scratch_bytes >= tp_layout(n_rings, n_vertices, tp_shift(cell)).bytes, "scratch too small (stcd_rings_topo_scratch_bytes)")

#define TP_CHECK_ENTRIES()                                                                                                        \
    STCD_CHECK(max_entries >= 0 && max_entries < ((int64_t)1 << 31), "max_entries must be in [0, 2^31)");                         \
    STCD_CHECK(max_entries == 0 || entries, "null pointer argument");                                                             \
    STCD_CHECK(tp_aligned(entries, 4), "entries must be 4-byte aligned")

extern "C" {

int64_t stcd_rings_topo_scratch_bytes(int64_t n_rings, int64_t n_vertices, int cell) {
    if (!tp_sizes_ok(n_rings, n_vertices) || tp_shift(cell) < 0) return 0;
    return tp_layout(n_rings, n_vertices, tp_shift(cell)).bytes;
}

int stcd_rings_conflicts(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int cell, uint8_t* flags,
                         int64_t* counts, int32_t* entries, int64_t max_entries, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    TP_CHECK_COMMON();
    TP_CHECK_ENTRIES();
    STCD_CHECK(n_vertices == 0 || flags, "null pointer argument");
    hipStream_t s = (hipStream_t)hip_stream;
    const int sh = tp_shift(cell);
    const TpScratch L = tp_layout(n_rings, n_vertices, sh);
    char* b = (char*)scratch;
    TpHeader* hdr = (TpHeader*)b;
    const long long R = n_rings, V = n_vertices;
    STCD_HIP(hipMemsetAsync(hdr, 0, sizeof(TpHeader), s));
    k_topo_validate<<<tp_blocks(std::max(R, V)), 256, 0, s>>>((const int*)vertices, (const long long*)offsets, R, V, hdr);
    if (V > 0) {
        k_topo_rid<<<tp_blocks(V), 256, 0, s>>>((const int2*)vertices, (const long long*)offsets, R, V, hdr, (int*)(b + L.rid), nullptr);
        k_topo_all<<<tp_blocks(V), 256, 0, s>>>((const int2*)vertices, (const long long*)offsets, V, hdr, (const int*)(b + L.rid), (int*)(b + L.ea),
                                                (int*)(b + L.eb));
        STCD_CHECK(tp_detect(b, L, sh, V, flags, entries, max_entries, s) == 0, "hipMemsetAsync failed");
        k_topo_tally<<<tp_blocks(V), 256, 0, s>>>(hdr, flags, nullptr);
    }
    k_topo_counts<<<1, 1, 0, s>>>(hdr, (long long*)counts);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_rings_safe_begin(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t q, int cell,
                          int64_t* counts, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    TP_CHECK_COMMON();
    STCD_CHECK(q >= 0 && q < ((int64_t)1 << 31), "q must be in [0, 2^31)");
    hipStream_t s = (hipStream_t)hip_stream;
    const int sh = tp_shift(cell);
    const TpScratch L = tp_layout(n_rings, n_vertices, sh);
    char* b = (char*)scratch;
    TpHeader* hdr = (TpHeader*)b;
    const long long R = n_rings, V = n_vertices;
    const int G = (TP_COORD_MAX >> sh) + 1;
    const int64_t NC = tp_cells(sh);
    STCD_HIP(hipMemsetAsync(hdr, 0, sizeof(TpHeader), s));
    k_topo_validate<<<tp_blocks(std::max(R, V)), 256, 0, s>>>((const int*)vertices, (const long long*)offsets, R, V, hdr);
    if (R > 0 && V > 0) {
        // round 0: the simplify count phase on its own part of the scratch buffer; its keep bytes and areas are the state from here on
        const int64_t sm_bytes = stcd_rings_simplify_scratch_bytes(R, V);
        if (stcd_rings_simplify_count(vertices, offsets, R, V, q, counts, b + L.simplify, sm_bytes, hip_stream) != 0) return 1;
        uint8_t* keep; long long* area; int* round0;
        sm_state_of(b + L.simplify, R, V, &keep, &area, &round0);
        STCD_HIP(hipMemsetAsync(b + L.ain, 0, 8 * R, s));
        STCD_HIP(hipMemsetAsync(b + L.changed, 0, 4 * R, s));
        STCD_HIP(hipMemsetAsync(b + L.pstart, 0, 4 * NC, s));
        k_topo_rid<<<tp_blocks(V), 256, 0, s>>>((const int2*)vertices, (const long long*)offsets, R, V, hdr, (int*)(b + L.rid),
                                                (unsigned long long*)(b + L.ain));
        STCD_HIP(hipMemcpyAsync(b + L.area, area, 8 * R, hipMemcpyDeviceToDevice, s));
        int* pstart = (int*)(b + L.pstart);
        k_topo_points<<<tp_blocks(R), 256, 0, s>>>((const int2*)vertices, (const long long*)offsets, R, hdr, sh, G, pstart, nullptr, 0);
        tp_scan_counts(pstart, NC, hdr, (long long*)(b + L.sums), R, s);
        k_topo_points<<<tp_blocks(R), 256, 0, s>>>((const int2*)vertices, (const long long*)offsets, R, hdr, sh, G, pstart, (int*)(b + L.pent), 1);
        const unsigned nb = (unsigned)tp_chunks(V);
        k_topo_sum<uint8_t><<<nb, 256, 0, s>>>(keep, V, hdr, (long long*)(b + L.sums));
        k_topo_scan<<<1, 256, 0, s>>>((long long*)(b + L.sums), nb, hdr, 0, -1, nullptr, round0);
    }
    k_topo_counts<<<1, 1, 0, s>>>(hdr, (long long*)counts);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_rings_safe_round(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int cell, int64_t n_edges,
                          int restore, int64_t* counts, int32_t* entries, int64_t max_entries, void* scratch, int64_t scratch_bytes,
                          void* hip_stream) {
    TP_CHECK_COMMON();
    TP_CHECK_ENTRIES();
    STCD_CHECK(n_edges >= 0 && n_edges <= n_vertices, "n_edges must be in [0, n_vertices]");
    hipStream_t s = (hipStream_t)hip_stream;
    const int sh = tp_shift(cell);
    const TpScratch L = tp_layout(n_rings, n_vertices, sh);
    char* b = (char*)scratch;
    TpHeader* hdr = (TpHeader*)b;
    const long long R = n_rings, V = n_vertices, E = n_edges;
    const int G = (TP_COORD_MAX >> sh) + 1;
    if (R > 0 && V > 0) {
        uint8_t* keep; long long* area0; int* round0;
        sm_state_of(b + L.simplify, R, V, &keep, &area0, &round0);
        const int2* vx = (const int2*)vertices;
        const long long* off = (const long long*)offsets;
        int *rid = (int*)(b + L.rid), *kv = (int*)(b + L.kv), *len = (int*)(b + L.len), *pos = (int*)(b + L.pos);
        uint8_t *flags = (uint8_t*)(b + L.flags), *pflags = (uint8_t*)(b + L.pflags);
        long long* sums = (long long*)(b + L.sums);
        // the capacity bit of an earlier call of this round is forgotten, the counters of the pass start at 0
        k_topo_reset<<<1, 1, 0, s>>>(hdr);
        const unsigned nb = (unsigned)tp_chunks(V);
        k_topo_sum<uint8_t><<<nb, 256, 0, s>>>(keep, V, hdr, sums);
        k_topo_scan<<<1, 256, 0, s>>>(sums, nb, hdr, 0, E, pos + V, nullptr);
        k_topo_excl<uint8_t><<<nb, 256, 0, s>>>(keep, V, hdr, sums, pos);
        k_topo_compact<<<tp_blocks(V), 256, 0, s>>>(keep, pos, V, hdr, kv);
        k_topo_cur<<<tp_blocks(E), 256, 0, s>>>(vx, off, hdr, rid, kv, (int*)(b + L.ea), (int*)(b + L.eb), len);
        STCD_CHECK(tp_detect(b, L, sh, E, flags, entries, max_entries, s) == 0, "hipMemsetAsync failed");
        STCD_HIP(hipMemsetAsync(pflags, 0, E, s));
        k_topo_pockets<<<tp_blocks(E, 4), 256, 0, s>>>(vx, off, R, hdr, rid, kv, len, sh, G, (const int*)(b + L.pstart), (const int*)(b + L.pent), pflags);
        k_topo_tally<<<tp_blocks(E), 256, 0, s>>>(hdr, flags, pflags);
        if (restore) {
            k_topo_restore<<<tp_blocks(E, 4), 256, 0, s>>>(vx, off, hdr, rid, kv, len, flags, pflags, keep, (unsigned long long*)(b + L.area),
                                                           (int*)(b + L.changed));
            k_topo_check<<<tp_blocks(V), 256, 0, s>>>(V, hdr, rid, (const int*)(b + L.changed), (const long long*)(b + L.area),
                                                      (const long long*)(b + L.ain), keep);
            k_topo_ringfix<<<tp_blocks(R), 256, 0, s>>>(R, hdr, (int*)(b + L.changed), (long long*)(b + L.area), (const long long*)(b + L.ain));
        }
    }
    k_topo_counts<<<1, 1, 0, s>>>(hdr, (long long*)counts);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_rings_safe_write(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int cell, int64_t n_out,
                          int32_t* out_vertices, int64_t* out_offsets, int64_t* out_area2, int64_t* counts, void* scratch, int64_t scratch_bytes,
                          void* hip_stream) {
    TP_CHECK_COMMON();
    STCD_CHECK(out_offsets != nullptr, "null pointer argument");
    STCD_CHECK(n_out >= 0 && n_out <= n_vertices, "n_out must be in [0, n_vertices]");
    STCD_CHECK((n_out == 0 || out_vertices) && (n_rings == 0 || out_area2), "null pointer argument");
    STCD_CHECK(tp_aligned(out_vertices, 8) && tp_aligned(out_offsets, 8) && tp_aligned(out_area2, 8), "misaligned output pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const TpScratch L = tp_layout(n_rings, n_vertices, tp_shift(cell));
    char* b = (char*)scratch;
    TpHeader* hdr = (TpHeader*)b;
    const long long R = n_rings, V = n_vertices;
    k_topo_wverts<<<tp_blocks(n_out), 256, 0, s>>>(hdr, R, V, n_out, (const int2*)vertices, (const int*)(b + L.kv), (int2*)out_vertices);
    k_topo_wrings<<<tp_blocks(R + 1), 256, 0, s>>>(hdr, R, V, n_out, (const long long*)offsets, (const int*)(b + L.pos), (const long long*)(b + L.area),
                                                   (long long*)out_offsets, (long long*)out_area2);
    k_topo_counts<<<1, 1, 0, s>>>(hdr, (long long*)counts);
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
