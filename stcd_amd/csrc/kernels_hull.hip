// kernels_hull.hip -- change polygons on the device: the convex hull of every ring of kernels_rings.hip by QuickHull over index
// intervals, and the minimum-area rectangle of every hull (gfx950), with their C-ABI entries.  tests/hull_spec.py states every
// output in plain Python and include/stcd_hip.h the rule set.  Integers only: a cross product of coordinates in [0, 16384] is
// below 2^30, a box area times an edge length below 2^90 (compared in 128 bits), so every output is a pure function of the input.
//
// The hull has the structure of kernels_simplify.hip: a ring of n vertices is worked on by a TEAM of threads, every ring iterates
// its own levels inside one kernel, no thread walks a chain, there is no device recursion, no launch and no host read per level,
// and no block waits for another block.  The anchors are the lexicographic minimum and maximum of (x, y), lowest index each (one
// 64-bit atomicMin / atomicMax of (x, y, index)); the state is kept in TRAVEL POSITIONS u = (v - i0) mod n, i0 the lower anchor, so
// that the two chains are [0, A] and [A, n] and "first in travel order" is "lowest u".  Per position: xy, pv / nx (a dropped
// vertex: the kept ones round it, pv == -1 once it lies on or inside its chord and is out of the game; a kept vertex: pv == u and
// nx the next kept one; n stands for position 0 at the ring's end) and, at the slots of kept vertices, bk: the largest
// (cross << 32 | ~u) of the chain that starts there.  One round is
//     A  every dropped vertex still in the game: strictly outside its chord, 64-bit atomicMax of (cross, ~u) at bk[pv]; else out
//     B  every such chain splits at its winner: the winner becomes kept, the others move pv or nx to it
//     C  the slots are cleared; the ring is done when the round split nothing (n rounds at the most: status bit 2)
// with the block's barrier between the steps.  "Outside" is decided by the sign of the ring's own area2, recomputed from the
// vertices.  Then one keep byte per vertex and the area2 of the kept ones.
//
//   k_hull_wave    4 rings per 256-thread block, one wavefront each, for rings of at most HL_WAVE_MAX vertices, state in an LDS
//                  slice; checks the offsets of every ring and lists the longer rings.
//   k_hull_block   one block per listed ring (grid-stride over the list): state in LDS up to HL_LDS_MAX vertices, in the scratch
//                  buffer above that (the slots then read and cleared with agent-scope atomic loads and stores).
//   k_hull_sum / k_hull_scan / k_hull_wverts / k_hull_wrings   the keep bytes counted and scanned (ring_scan.h) and the write phase,
//                  as in kernels_simplify.hip.
//   k_hull_boxes   4 hulls per block: a wavefront takes a hull of up to BX_WAVE_MAX vertices, the block then takes each longer one
//                  of its four; a lane takes an edge at a time and scans the hull's vertices (in LDS up to BX_LDS_MAX, from global
//                  memory above); the lanes' best edges are reduced with the exact comparison and the lowest-index rule.
#include <algorithm>
#include <climits>

#include "common.h"
#include "ring_scan.h"

namespace stcd {

#define HL_WAVE_MAX 64                         // HULL_WAVE_MAX of stcd_amd/objects.py: longest ring one wavefront takes
#define HL_LDS_MAX 2048                        // HULL_LDS_MAX: longest ring whose state fits the block's LDS (20 bytes a vertex)
#define HL_CHUNK 4096                          // vertices per block of the scan: 256 threads x 16
#define HL_BLOCK_GRID 1024                     // blocks of the grid-stride pass over the listed rings
#define HL_COORD_MAX 16384
#define BX_WAVE_MAX 64                         // BOX_WAVE_MAX: longest hull one wavefront boxes
#define BX_LDS_MAX 1024                        // BOX_LDS_MAX: longest hull the block holds in LDS

enum { HL_ST_RANGE = 1, HL_ST_ROUNDS = 2, HL_ST_OFFSETS = 4, HL_ST_MISMATCH = 8 };

struct HlHeader {                              // the first 48 bytes of the scratch buffer, kept from the count to the write phase
    long long rings, vertices, vout;
    int status, nlist;                         // nlist: rings longer than HL_WAVE_MAX
    long long pad_[2];
};

struct HlState { int *xy, *pv, *nx; unsigned long long* bk; };          // n entries each, in LDS or in the scratch buffer

template <int TEAMS>
struct HlControl {                             // in LDS, per team
    unsigned long long lo[TEAMS], hi[TEAMS];   // (x, y, index) of the lowest, (x, y, ~index) of the highest vertex
    unsigned long long area[TEAMS][2];         // twice the signed area of the input ring, of the kept vertices
    int flag[2][TEAMS];                        // round r split a chain: flag[r & 1]
};

// x in the high half: packed vertices compare as (x, y)
__device__ __forceinline__ int hl_pack(int y, int x) { return (x << 16) | y; }
__device__ __forceinline__ long long hl_x(int p) { return p >> 16; }
__device__ __forceinline__ long long hl_y(int p) { return p & 0xffff; }
// the packed vertex v of a ring, clamped into range (bit 1 is raised for it where the ring is first read)
__device__ __forceinline__ int hl_read(const int* __restrict__ in, int v, bool& range) {
    int y = in[2 * (int64_t)v], x = in[2 * (int64_t)v + 1];
    if ((unsigned)y > (unsigned)HL_COORD_MAX || (unsigned)x > (unsigned)HL_COORD_MAX) {
        range = true;
        y = min(max(y, 0), HL_COORD_MAX); x = min(max(x, 0), HL_COORD_MAX);
    }
    return hl_pack(y, x);
}
// x_t * y_h - x_h * y_t of the side from t to h
__device__ __forceinline__ long long hl_side(int t, int h) { return hl_x(t) * hl_y(h) - hl_x(h) * hl_y(t); }
// > 0 where p lies left of a -> b with x to the right and y up: the side the interior of a ring of positive area2 is on
__device__ __forceinline__ long long hl_cross(int a, int b, int p) {
    return (hl_x(b) - hl_x(a)) * (hl_y(p) - hl_y(a)) - (hl_y(b) - hl_y(a)) * (hl_x(p) - hl_x(a));
}

// the slots: written by atomics, so read and cleared past the vector L1 when they live in global memory
template <typename T> __device__ __forceinline__ T hl_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void hl_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One ring per team of TEAM threads (t: the thread within the team), 256 / TEAM teams per block; EVERY thread of the block calls
// this with its team's ring, n == 0 for a team without one: the barriers are the block's.  in: the ring's n input vertices.
template <int TEAM>
__device__ __forceinline__ void hl_ring(const int* __restrict__ in, const int n, const HlState s, uint8_t* __restrict__ keep,
                                        long long* __restrict__ area_out, int* __restrict__ status, HlControl<256 / TEAM>& c,
                                        const int team, const int t) {
    constexpr int TEAMS = 256 / TEAM;
    if (t == 0) {
        c.lo[team] = ~0ull; c.hi[team] = 0ull;
        c.area[team][0] = c.area[team][1] = 0; c.flag[0][team] = c.flag[1][team] = 0;
    }
    __syncthreads();
    // the anchors
    bool range = false;
    if (n > 0) {
        unsigned long long lo = ~0ull, hi = 0ull;
        for (int v = t; v < n; v += TEAM) {
            const unsigned long long p = (unsigned long long)(unsigned)hl_read(in, v, range) << 32;
            lo = min(lo, p | (unsigned)v);
            hi = max(hi, p | (0xffffffffu - (unsigned)v));
        }
        if (t < n) { atomicMin(&c.lo[team], lo); atomicMax(&c.hi[team], hi); }
    }
    if (range) atomicOr(status, HL_ST_RANGE);
    __syncthreads();
    int i0 = 0, A = 0;                                                 // position u is vertex (u + i0) mod n; the other anchor is position A
    if (n > 0) {
        const int a = (int)(unsigned)c.lo[team], b = (int)(0xffffffffu - (unsigned)c.hi[team]);       // both below n
        i0 = min(a, b); A = max(a, b) - i0;
    }
    for (int u = t; u < n; u += TEAM) {
        const int v = u + i0 < n ? u + i0 : u + i0 - n;
        bool again = false;
        s.xy[u] = hl_read(in, v, again);
        s.pv[u] = u == 0 || u == A ? u : u < A ? 0 : A;
        s.nx[u] = u < A ? A : n;
        hl_store(s.bk + u, 0ull);
    }
    __syncthreads();
    if (n > 0) {
        long long a = 0;
        for (int u = t; u < n; u += TEAM) a += hl_side(s.xy[u], s.xy[u + 1 == n ? 0 : u + 1]);
        atomicAdd(&c.area[team][0], (unsigned long long)a);
    }
    __syncthreads();
    const bool hole = (long long)c.area[team][0] < 0;
    bool active = n > 0;
    for (int round = 0;; ++round) {                                    // uniform over the block
        if (active)
            for (int u = t; u < n; u += TEAM) {
                const int p = s.pv[u];
                if (p == u || p < 0) continue;
                const int h = s.nx[u];
                const long long x = hl_cross(s.xy[p], s.xy[h == n ? 0 : h], s.xy[u]);
                const long long out = hole ? x : -x;                   // below 2^30
                if (out <= 0) s.pv[u] = -1;                            // on or inside a chord between hull vertices: never a hull vertex
                else atomicMax(s.bk + p, ((unsigned long long)out << 32) | (0xffffffffu - (unsigned)u));
            }
        __syncthreads();
        if (active) {
            bool split = false;
            for (int u = t; u < n; u += TEAM) {
                const int p = s.pv[u];
                if (p == u || p < 0) continue;
                const int w = (int)(0xffffffffu - (unsigned)hl_load(s.bk + p));   // p < w < nx[u]: u's own key is in the slot at the least
                if (w <= p || w >= s.nx[u]) { s.pv[u] = -1; continue; }           // an index is checked before it is used
                split = true;
                if (u == w) { s.pv[u] = u; s.nx[p] = u; }              // p is kept: nobody reads or writes its nx in this step
                else if (u < w) s.nx[u] = w;
                else s.pv[u] = w;
            }
            if (split) c.flag[round & 1][team] = 1;
        }
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int k = 0; k < TEAMS; ++k) any = any || c.flag[round & 1][k];
        if (active) {
            const bool go = c.flag[round & 1][team];
            for (int u = t; u < n; u += TEAM)
                if (s.pv[u] == u) hl_store(s.bk + u, 0ull);
            if (go && round + 1 >= n) atomicOr(status, HL_ST_ROUNDS);  // a splitting round keeps a vertex: n - 2 of them at the most
            active = go && round + 1 < n;
        }
        if (t == 0) c.flag[~round & 1][team] = 0;
        __syncthreads();
        if (!any) break;
    }
    if (n > 0) {
        long long a = 0;
        for (int u = t; u < n; u += TEAM) {
            const bool kept = s.pv[u] == u;
            keep[u + i0 < n ? u + i0 : u + i0 - n] = kept;
            if (kept) {
                const int h = s.nx[u];
                a += hl_side(s.xy[u], s.xy[h <= 0 || h >= n ? 0 : h]);
            }
        }
        atomicAdd(&c.area[team][1], (unsigned long long)a);
    }
    __syncthreads();
    if (t == 0 && area_out) *area_out = (long long)c.area[team][1];
    __syncthreads();                                                   // the state is another ring's after this
}

// the ring's first vertex and length, 0 where the offsets are no ring's (status bit 4: nothing of that ring is read)
__device__ __forceinline__ int hl_ring_range(const long long* __restrict__ offsets, long long r, long long R, long long V, long long& off, int* status) {
    const long long o0 = offsets[r], o1 = offsets[r + 1];
    off = 0;
    if (o0 < 0 || o1 < o0 || o1 > V || (r == 0 && o0 != 0) || (r == R - 1 && o1 != V)) { atomicOr(status, HL_ST_OFFSETS); return 0; }
    off = o0;
    return (int)(o1 - o0);                                             // V is below 2^31
}

__global__ void __launch_bounds__(256)
k_hull_wave(const int* __restrict__ vertices, const long long* __restrict__ offsets, long long R, long long V, HlHeader* __restrict__ hdr,
            int* __restrict__ list, uint8_t* __restrict__ keep, long long* __restrict__ area) {
    constexpr int TEAMS = 256 / 64;
    __shared__ int xy[TEAMS * HL_WAVE_MAX], pv[TEAMS * HL_WAVE_MAX], nx[TEAMS * HL_WAVE_MAX];
    __shared__ unsigned long long bk[TEAMS * HL_WAVE_MAX];
    __shared__ HlControl<TEAMS> c;
    const int team = threadIdx.x >> 6, t = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * TEAMS + team;
    long long off = 0;
    int n = 0;
    bool listed = false;
    if (r < R) {
        n = hl_ring_range(offsets, r, R, V, off, &hdr->status);
        listed = n > HL_WAVE_MAX;
        if (listed) {
            if (t == 0) list[atomicAdd(&hdr->nlist, 1)] = (int)r;      // at most R entries
            n = 0;
        }
    }
    const int o = team * HL_WAVE_MAX;
    const HlState s = {xy + o, pv + o, nx + o, bk + o};
    hl_ring<64>(vertices + 2 * off, n, s, keep + off, r < R && !listed ? area + r : nullptr, &hdr->status, c, team, t);
}

__global__ void __launch_bounds__(256)
k_hull_block(const int* __restrict__ vertices, const long long* __restrict__ offsets, long long R, long long V, HlHeader* __restrict__ hdr,
             const int* __restrict__ list, uint8_t* __restrict__ keep, long long* __restrict__ area, const HlState g) {
    __shared__ int xy[HL_LDS_MAX], pv[HL_LDS_MAX], nx[HL_LDS_MAX];
    __shared__ unsigned long long bk[HL_LDS_MAX];
    __shared__ HlControl<1> c;
    const int count = (int)min((long long)hdr->nlist, R);
    for (int i = blockIdx.x; i < count; i += gridDim.x) {              // uniform over the block
        const long long r = list[i];
        if (r < 0 || r >= R) continue;                                 // an index is checked before it is used
        long long off = 0;
        const int n = hl_ring_range(offsets, r, R, V, off, &hdr->status);
        if (n <= HL_LDS_MAX) {
            const HlState s = {xy, pv, nx, bk};
            hl_ring<256>(vertices + 2 * off, n, s, keep + off, area + r, &hdr->status, c, 0, (int)threadIdx.x);
        } else {
            const HlState s = {g.xy + off, g.pv + off, g.nx + off, g.bk + off};
            hl_ring<256>(vertices + 2 * off, n, s, keep + off, area + r, &hdr->status, c, 0, (int)threadIdx.x);
        }
    }
}

__global__ void __launch_bounds__(256)
k_hull_sum(const uint8_t* __restrict__ keep, long long V, long long* __restrict__ sums) {
    __shared__ int wsum[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * HL_CHUNK + threadIdx.x;
    int n = 0;
    for (int k = 0; k < HL_CHUNK / 256; ++k)
        if (first + k * 256 < V) n += keep[first + k * 256] & 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (long long)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

__global__ void __launch_bounds__(256)
k_hull_scan(long long* __restrict__ sums, int64_t nb, const long long* __restrict__ offsets, long long R, long long V,
            HlHeader* __restrict__ hdr, long long* __restrict__ counts) {
    __shared__ long long ws[4];
    const long long total = rg_block_scan(sums, nb, 1, ws);
    if (threadIdx.x == 0) {
        if (R == 0 && (V != 0 || offsets[0] != 0)) hdr->status |= HL_ST_OFFSETS;           // no ring launch has looked at them
        hdr->rings = R; hdr->vertices = V; hdr->vout = total;
        counts[0] = total; counts[1] = (long long)hdr->status;
    }
}

// the header is the count phase's own, on rings of these sizes, and n_out is what it left (bit 8 of an earlier write call aside)
__device__ __forceinline__ bool hl_write_ok(const HlHeader* __restrict__ hdr, long long R, long long V, long long n_out) {
    return (hdr->status & ~HL_ST_MISMATCH) == 0 && hdr->rings == R && hdr->vertices == V && hdr->vout == n_out;
}

__global__ void __launch_bounds__(256)
k_hull_wverts(HlHeader* __restrict__ hdr, long long R, long long V, long long n_out, const int2* __restrict__ vertices,
              const uint8_t* __restrict__ keep, const long long* __restrict__ sums, int* __restrict__ pos, int2* __restrict__ out) {
    __shared__ int ws[4];
    if (!hl_write_ok(hdr, R, V, n_out)) {                              // uniform over the grid: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&hdr->status, HL_ST_MISMATCH);
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * HL_CHUNK + threadIdx.x;
    long long run = sums[blockIdx.x];
    for (int k = 0; k < HL_CHUNK / 256; ++k) {                         // uniform
        const int64_t v = first + k * 256;
        const int f = v < V ? keep[v] & 1 : 0;
        const int inc = (int)rg_wave_scan((long long)f, lane);
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) before += ws[w]; total += ws[w]; }
        const long long at = run + before + inc - f;                   // the kept vertices before v
        if (v < V) pos[v] = (int)at;
        if (f && at < n_out) out[at] = vertices[v];
        run += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_hull_wrings(const HlHeader* __restrict__ hdr, long long R, long long V, long long n_out, const long long* __restrict__ offsets,
              const int* __restrict__ pos, const long long* __restrict__ area, long long* __restrict__ out_offsets,
              long long* __restrict__ out_area2) {
    if (!hl_write_ok(hdr, R, V, n_out)) return;                        // k_hull_wverts has set bit 8
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r > R) return;
    const long long o = offsets[r];                                    // the count phase found 0 <= o <= V; an index is checked before it is used
    out_offsets[r] = o >= 0 && o < V ? (long long)pos[o] : n_out;
    if (r < R) out_area2[r] = area[r];
}

// ------------------------------------------------------------------------------------------------ oriented boxes
struct BxBest { unsigned long long area; unsigned len; int edge, dmin, dmax, z; };        // area = W |Z|, len = L; edge -1: none

// a's box is the smaller one, or as small on a lower edge: area_a / len_a < area_b / len_b, exactly
__device__ __forceinline__ bool bx_better(const BxBest& a, const BxBest& b) {
    if (a.edge < 0) return false;
    if (b.edge < 0) return true;
    const unsigned __int128 pa = (unsigned __int128)a.area * b.len, pb = (unsigned __int128)b.area * a.len;
    return pa < pb || (pa == pb && a.edge < b.edge);
}

__device__ __forceinline__ BxBest bx_wave_best(BxBest m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        BxBest b;
        b.area = __shfl_xor(m.area, o, 64); b.len = __shfl_xor(m.len, o, 64); b.edge = __shfl_xor(m.edge, o, 64);
        b.dmin = __shfl_xor(m.dmin, o, 64); b.dmax = __shfl_xor(m.dmax, o, 64); b.z = __shfl_xor(m.z, o, 64);
        if (bx_better(b, m)) m = b;
    }
    return m;
}

// the best of the edges t, t + TEAM, ... of a hull of h >= 3 vertices: xy its packed vertices in LDS, or nullptr to read `in`
template <int TEAM>
__device__ __forceinline__ BxBest bx_edges(const int* xy, const int* __restrict__ in, const int h, const int t) {
    BxBest m = {0ull, 0u, -1, 0, 0, 0};
    bool range = false;                                                // raised by the caller's own pass over the hull
    for (int i = t; i < h; i += TEAM) {
        const int i1 = i + 1 == h ? 0 : i + 1;
        const int a = xy ? xy[i] : hl_read(in, i, range), b = xy ? xy[i1] : hl_read(in, i1, range);
        const int ey = (int)(hl_y(b) - hl_y(a)), ex = (int)(hl_x(b) - hl_x(a));
        const unsigned L = (unsigned)(ey * ey + ex * ex);              // at most 2^29
        if (L == 0) continue;
        int dmin = 0, dmax = 0, zmin = 0, zmax = 0;                    // vertex i itself has d = z = 0
        for (int j = 0; j < h; ++j) {
            const int p = xy ? xy[j] : hl_read(in, j, range);
            const int py = (int)(hl_y(p) - hl_y(a)), px = (int)(hl_x(p) - hl_x(a));
            const int d = py * ey + px * ex, z = ex * py - ey * px;    // both within 2^29
            dmin = min(dmin, d); dmax = max(dmax, d); zmin = min(zmin, z); zmax = max(zmax, z);
        }
        BxBest e;
        e.z = zmax >= -zmin ? zmax : zmin;
        e.area = (unsigned long long)(dmax - dmin) * (unsigned long long)(e.z < 0 ? -e.z : e.z);
        e.len = L; e.edge = i; e.dmin = dmin; e.dmax = dmax;
        if (bx_better(e, m)) m = e;
    }
    return m;
}

__device__ __forceinline__ void bx_write(const BxBest& m, const int* xy, const int* __restrict__ in, int h, long long r,
                                         int* __restrict__ out_edge, int* __restrict__ out_origin, int* __restrict__ out_dir,
                                         long long* __restrict__ out_extent) {
    int oy = 0, ox = 0, ey = 0, ex = 0;
    if (m.edge >= 0 && m.edge < h) {
        bool range = false;
        const int i1 = m.edge + 1 == h ? 0 : m.edge + 1;
        const int a = xy ? xy[m.edge] : hl_read(in, m.edge, range), b = xy ? xy[i1] : hl_read(in, i1, range);
        oy = (int)hl_y(a); ox = (int)hl_x(a); ey = (int)(hl_y(b) - hl_y(a)); ex = (int)(hl_x(b) - hl_x(a));
    }
    out_edge[r] = m.edge;
    out_origin[2 * r] = oy; out_origin[2 * r + 1] = ox;
    out_dir[2 * r] = ey; out_dir[2 * r + 1] = ex;
    out_extent[3 * r] = m.dmin; out_extent[3 * r + 1] = m.dmax; out_extent[3 * r + 2] = m.z;
}

__global__ void __launch_bounds__(256)
k_hull_boxes(const int* __restrict__ vertices, const long long* __restrict__ offsets, long long R, long long V, int* __restrict__ status,
             int* __restrict__ out_edge, int* __restrict__ out_origin, int* __restrict__ out_dir, long long* __restrict__ out_extent) {
    constexpr int TEAMS = 256 / 64;
    __shared__ int xy[BX_LDS_MAX];                                     // 4 slices of BX_WAVE_MAX, then one long hull
    __shared__ int len[TEAMS];
    __shared__ long long first[TEAMS];
    __shared__ BxBest best[TEAMS];
    static_assert(TEAMS * BX_WAVE_MAX <= BX_LDS_MAX, "the wavefronts' slices fit the block's array");
    const int team = threadIdx.x >> 6, t = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * TEAMS + team;
    long long off = 0;
    int h = 0;
    if (r < R) h = hl_ring_range(offsets, r, R, V, off, status);
    if (t == 0) { len[team] = r < R ? h : -1; first[team] = off; }
    bool range = false;
    int* mine = xy + team * BX_WAVE_MAX;
    if (h <= BX_WAVE_MAX && t < h) mine[t] = hl_read(vertices + 2 * off, t, range);
    __syncthreads();
    if (r < R && h <= BX_WAVE_MAX) {
        BxBest m = {0ull, 0u, -1, 0, 0, 0};
        if (h >= 3) m = bx_wave_best(bx_edges<64>(mine, nullptr, h, t));
        if (t == 0) bx_write(m, mine, nullptr, h, r, out_edge, out_origin, out_dir, out_extent);
    }
    __syncthreads();                                                   // the slices are read: the array is the block's now
    for (int k = 0; k < TEAMS; ++k) {                                  // uniform over the block
        const int hk = len[k];
        if (hk <= BX_WAVE_MAX) continue;
        const long long rk = (long long)blockIdx.x * TEAMS + k;
        const int* in = vertices + 2 * first[k];
        const int* lds = hk <= BX_LDS_MAX ? xy : nullptr;
        for (int j = threadIdx.x; j < hk; j += 256) {
            const int p = hl_read(in, j, range);
            if (lds) xy[j] = p;
        }
        __syncthreads();
        const BxBest m = bx_wave_best(bx_edges<256>(lds, in, hk, (int)threadIdx.x));
        if (t == 0) best[team] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            BxBest b = best[0];
            for (int w = 1; w < TEAMS; ++w)
                if (bx_better(best[w], b)) b = best[w];
            bx_write(b, lds, in, hk, rk, out_edge, out_origin, out_dir, out_extent);
        }
        __syncthreads();                                               // xy and best are written again
    }
    if (range) atomicOr(status, HL_ST_RANGE);
}

// ------------------------------------------------------------------------------------------------ launch sequences
namespace {

struct HlScratch {                                                     // byte offsets into the scratch buffer
    int64_t sums, area, bk, list, pos, xy, pv, nx, keep, bytes;
};
inline int64_t hl_chunks(int64_t n) { return std::max<int64_t>(1, (n + HL_CHUNK - 1) / HL_CHUNK); }
inline HlScratch hl_layout(int64_t R, int64_t V) {
    HlScratch s;
    int64_t o = (int64_t)sizeof(HlHeader);
    s.sums = o; o += 8 * hl_chunks(V);
    s.area = o; o += 8 * R;
    s.bk = o; o += 8 * V;
    s.list = o; o += 4 * ((R + 1) / 2 * 2);
    int64_t* per[] = {&s.pos, &s.xy, &s.pv, &s.nx};
    for (int64_t* p : per) { *p = o; o += 4 * ((V + 1) / 2 * 2); }
    s.keep = o; o += V;
    s.bytes = (o + 7) / 8 * 8;
    return s;
}
inline bool hl_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool hl_sizes_ok(int64_t R, int64_t V) { return R >= 0 && V >= 0 && R < ((int64_t)1 << 31) && V < ((int64_t)1 << 31); }

}  // namespace
}  // namespace stcd

using namespace stcd;

// what both hull entries check before anything else
#define HL_CHECK_COMMON()                                                                                                         \
    STCD_CHECK(vertices && offsets && scratch, "null pointer argument");                                                          \
    STCD_CHECK(n_rings >= 0 && n_vertices >= 0, "n_rings and n_vertices must be >= 0");                                           \
    STCD_CHECK(hl_sizes_ok(n_rings, n_vertices), "n_rings and n_vertices must be below 2^31");                                    \
    STCD_CHECK(hl_aligned(vertices, 8) && hl_aligned(offsets, 8) && hl_aligned(scratch, 8), "vertices, offsets and scratch must be 8-byte aligned"); \
    STCD_CHECK(scratch_bytes >= hl_layout(n_rings, n_vertices).bytes, "scratch too small (stcd_rings_hull_scratch_bytes)")

extern "C" {

int64_t stcd_rings_hull_scratch_bytes(int64_t n_rings, int64_t n_vertices) {
    if (!hl_sizes_ok(n_rings, n_vertices)) return 0;
    return hl_layout(n_rings, n_vertices).bytes;
}

int stcd_rings_hull_count(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t* counts, void* scratch,
                          int64_t scratch_bytes, void* hip_stream) {
    HL_CHECK_COMMON();
    STCD_CHECK(counts != nullptr, "null pointer argument");
    STCD_CHECK(hl_aligned(counts, 8), "counts must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const HlScratch L = hl_layout(n_rings, n_vertices);
    char* b = (char*)scratch;
    HlHeader* hdr = (HlHeader*)b;
    long long* sums = (long long*)(b + L.sums);
    long long* area = (long long*)(b + L.area);
    int* list = (int*)(b + L.list);
    uint8_t* keep = (uint8_t*)(b + L.keep);
    const HlState g = {(int*)(b + L.xy), (int*)(b + L.pv), (int*)(b + L.nx), (unsigned long long*)(b + L.bk)};
    const long long R = n_rings, V = n_vertices;
    const unsigned chunks = (unsigned)hl_chunks(V);
    STCD_HIP(hipMemsetAsync(hdr, 0, sizeof(HlHeader), s));
    if (R > 0) {
        k_hull_wave<<<(unsigned)((R + 3) / 4), 256, 0, s>>>((const int*)vertices, (const long long*)offsets, R, V, hdr, list, keep, area);
        k_hull_block<<<(unsigned)std::min<int64_t>(R, HL_BLOCK_GRID), 256, 0, s>>>((const int*)vertices, (const long long*)offsets, R, V, hdr, list,
                                                                                   keep, area, g);
    }
    k_hull_sum<<<chunks, 256, 0, s>>>(keep, R > 0 ? V : 0, sums);
    k_hull_scan<<<1, 256, 0, s>>>(sums, (int64_t)chunks, (const long long*)offsets, R, V, hdr, (long long*)counts);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_rings_hull_write(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t n_out,
                          int32_t* out_vertices, int64_t* out_offsets, int64_t* out_area2, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    HL_CHECK_COMMON();
    STCD_CHECK(out_offsets != nullptr, "null pointer argument");
    STCD_CHECK(n_out >= 0 && n_out <= n_vertices, "n_out must be in [0, n_vertices]");
    STCD_CHECK((n_out == 0 || out_vertices) && (n_rings == 0 || out_area2), "null pointer argument");
    STCD_CHECK(hl_aligned(out_vertices, 8) && hl_aligned(out_offsets, 8) && hl_aligned(out_area2, 8), "misaligned output pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const HlScratch L = hl_layout(n_rings, n_vertices);
    char* b = (char*)scratch;
    HlHeader* hdr = (HlHeader*)b;
    const long long R = n_rings, V = n_vertices;
    k_hull_wverts<<<(unsigned)hl_chunks(V), 256, 0, s>>>(hdr, R, V, n_out, (const int2*)vertices, (const uint8_t*)(b + L.keep),
                                                         (const long long*)(b + L.sums), (int*)(b + L.pos), (int2*)out_vertices);
    k_hull_wrings<<<(unsigned)((R + 256) / 256), 256, 0, s>>>(hdr, R, V, n_out, (const long long*)offsets, (const int*)(b + L.pos),
                                                              (const long long*)(b + L.area), (long long*)out_offsets, (long long*)out_area2);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_rings_boxes(const int32_t* hull_vertices, const int64_t* hull_offsets, int64_t n_rings, int64_t n_vertices, int32_t* out_edge,
                     int32_t* out_origin, int32_t* out_dir, int64_t* out_extent, int32_t* status, void* hip_stream) {
    STCD_CHECK(hull_offsets && status, "null pointer argument");
    STCD_CHECK(n_rings >= 0 && n_vertices >= 0, "n_rings and n_vertices must be >= 0");
    STCD_CHECK(hl_sizes_ok(n_rings, n_vertices), "n_rings and n_vertices must be below 2^31");
    STCD_CHECK(n_vertices == 0 || hull_vertices, "null pointer argument");
    STCD_CHECK(n_rings == 0 || (out_edge && out_origin && out_dir && out_extent), "null pointer argument");
    STCD_CHECK(hl_aligned(hull_vertices, 4) && hl_aligned(hull_offsets, 8) && hl_aligned(out_edge, 4) && hl_aligned(out_origin, 4) &&
                   hl_aligned(out_dir, 4) && hl_aligned(out_extent, 8) && hl_aligned(status, 4),
               "misaligned pointer (8 bytes for hull_offsets and out_extent, 4 for the others)");
    hipStream_t s = (hipStream_t)hip_stream;
    STCD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_rings > 0)
        k_hull_boxes<<<(unsigned)((n_rings + 3) / 4), 256, 0, s>>>((const int*)hull_vertices, (const long long*)hull_offsets, (long long)n_rings,
                                                                  (long long)n_vertices, (int*)status, (int*)out_edge, (int*)out_origin, (int*)out_dir,
                                                                  (long long*)out_extent);
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
