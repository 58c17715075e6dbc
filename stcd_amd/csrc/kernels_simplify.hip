// kernels_simplify.hip -- change polygons on the device: Douglas-Peucker over the rings of kernels_rings.hip (gfx950), with its C-ABI
// entries.  tests/simplify_spec.py states every output in plain Python and include/stcd_hip.h the rule set.  Integers only: a key is
// d^2 * L' (at most 2^58 for coordinates in [0, 16384]), compared as 4 * key > q * L' in 64 bits, so every output is a pure function
// of the input.  Every ring iterates its own levels inside one kernel: no thread walks a chain, there is no device recursion, no
// launch and no host read per level, and no block waits for another block.
//
// A ring of n vertices is worked on by a TEAM of threads, vertex v by thread v % TEAM.  Per vertex: xy (the packed coordinates),
// pv / nx (a dropped vertex: the kept vertices round it; a kept vertex: pv == v and nx the next kept one; n stands for P[0] at the
// chain's end) and, used at the slots of kept vertices only, bk / bi: the largest key of the segment that starts there and the
// lowest index that has it.  One round is
//     A  every dropped vertex: 64-bit atomicMax of its key at bk[pv]
//     B  every dropped vertex whose key is that maximum: atomicMin of its index at bi[pv]
//     C  where 4 * bk > q * L' the segment splits: the winner becomes kept, the others move pv or nx to it
//     D  the slots are cleared; the ring is done when the round split nothing (n rounds at the most: status bit 2)
// with the block's barrier between the steps.  The anchors (rule 2) and the triangle rule (rule 4) use the same two atomics at slot 0.
// Then, still per ring: the area of the kept vertices and of the input ring, the sign rule (rule 5), one keep byte per vertex and
// the ring's area2.
//
//   k_simplify_wave   4 rings per 256-thread block, one wavefront each, for rings of at most SM_WAVE_MAX vertices, state in an LDS
//                     slice; checks the offsets of every ring and lists the longer rings.
//   k_simplify_block  one block per listed ring (grid-stride over the list, whatever the ring's place in the input): state in LDS up
//                     to SM_LDS_MAX vertices, in the scratch buffer above that; the slots are then read and cleared with agent-scope
//                     atomic loads and stores, as the atomics that write them go to L2.
//   k_simplify_sum / k_simplify_scan   the keep bytes summed per SM_CHUNK vertices, the chunk sums scanned by one block
//                     (rg_block_scan of ring_scan.h): V' and the status word for the host.
//   k_simplify_wverts / k_simplify_wrings   the write phase: the place of a kept vertex is the number of kept vertices before it,
//                     as rings follow each other in the input; offsets[r] is the place of the ring's first vertex.
#include <algorithm>
#include <climits>

#include "common.h"
#include "ring_scan.h"

namespace stcd {

#define SM_WAVE_MAX 64                         // SIMPLIFY_WAVE_MAX of stcd_amd/objects.py: longest ring one wavefront takes
#define SM_LDS_MAX 2048                        // SIMPLIFY_LDS_MAX: longest ring whose state fits the block's LDS (24 bytes a vertex)
#define SM_CHUNK 4096                          // vertices per block of the scan: 256 threads x 16
#define SM_BLOCK_GRID 1024                     // blocks of the grid-stride pass over the listed rings (Guideline 11)
#define SM_COORD_MAX 16384

enum { SM_ST_RANGE = 1, SM_ST_ROUNDS = 2, SM_ST_OFFSETS = 4, SM_ST_MISMATCH = 8 };

struct SmHeader {                              // the first 48 bytes of the scratch buffer, kept from the count to the write phase
    long long rings, vertices, vout;
    int status, nlist;                         // nlist: rings longer than SM_WAVE_MAX
    long long pad_[2];
};

struct SmState { int *xy, *pv, *nx, *bi; unsigned long long* bk; };     // n entries each, in LDS or in the scratch buffer

template <int TEAMS>
struct SmControl {                             // in LDS, per team
    unsigned long long area[TEAMS][2];         // twice the signed area of the input ring, of the kept vertices
    int flag[2][TEAMS];                        // round r split a segment: flag[r & 1]
    int kept[TEAMS];
};

__device__ __forceinline__ int sm_pack(int y, int x) { return (y << 16) | x; }
__device__ __forceinline__ long long sm_y(int p) { return p >> 16; }
__device__ __forceinline__ long long sm_x(int p) { return p & 0xffff; }
__device__ __forceinline__ unsigned long long sm_dist2(int p, int a) {
    const long long ey = sm_y(p) - sm_y(a), ex = sm_x(p) - sm_x(a);
    return (unsigned long long)(ey * ey + ex * ex);
}
__device__ __forceinline__ unsigned long long sm_len(int a, int b) {          // L'
    const unsigned long long L = sm_dist2(b, a);
    return L ? L : 1ull;
}
// rule 1: d^2 * L' with d the distance of p from the segment (a, b)
__device__ __forceinline__ unsigned long long sm_key(int p, int a, int b) {
    const long long ey = sm_y(p) - sm_y(a), ex = sm_x(p) - sm_x(a), dy = sm_y(b) - sm_y(a), dx = sm_x(b) - sm_x(a);
    const long long L = dy * dy + dx * dx, e2 = ey * ey + ex * ex;
    if (L == 0) return (unsigned long long)e2;
    const long long t = ey * dy + ex * dx;
    if (t <= 0) return (unsigned long long)(e2 * L);
    if (t >= L) return sm_dist2(p, b) * (unsigned long long)L;
    const long long c = ey * dx - ex * dy;
    return (unsigned long long)(c * c);
}
// x_t * y_h - x_h * y_t of the side from t to h
__device__ __forceinline__ long long sm_side(int t, int h) { return sm_x(t) * sm_y(h) - sm_x(h) * sm_y(t); }

// the slots: written by atomics, so read and cleared past the vector L1 when they live in global memory
template <typename T> __device__ __forceinline__ T sm_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void sm_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One ring per team of TEAM threads (t: the thread within the team), 256 / TEAM teams per block; EVERY thread of the block calls
// this with its team's ring, n == 0 for a team without one: the barriers are the block's.  in: the ring's n input vertices.
template <int TEAM>
__device__ __forceinline__ void sm_ring(const int* __restrict__ in, const int n, const unsigned long long q, const SmState s,
                                        uint8_t* __restrict__ keep, long long* __restrict__ area_out, int* __restrict__ status,
                                        SmControl<256 / TEAM>& c, const int team, const int t) {
    constexpr int TEAMS = 256 / TEAM;
    bool active = n >= 4;                                              // rule 5: a shorter ring is copied whole
    bool range = false;
    for (int v = t; v < n; v += TEAM) {
        int y = in[2 * (int64_t)v], x = in[2 * (int64_t)v + 1];
        if ((unsigned)y > (unsigned)SM_COORD_MAX || (unsigned)x > (unsigned)SM_COORD_MAX) {
            range = true;                                              // the keys stay within 64 bits whatever the input
            y = min(max(y, 0), SM_COORD_MAX); x = min(max(x, 0), SM_COORD_MAX);
        }
        s.xy[v] = sm_pack(y, x);
        sm_store(s.bk + v, 0ull); sm_store(s.bi + v, INT_MAX);
    }
    if (range) atomicOr(status, SM_ST_RANGE);
    if (t == 0) { c.area[team][0] = c.area[team][1] = 0; c.flag[0][team] = c.flag[1][team] = 0; c.kept[team] = 0; }
    __syncthreads();
    // rule 2: the vertex farthest from P[0], lowest index on ties (vertex 0 itself where every distance is 0); the input's area
    if (n > 0) {
        const int p0 = s.xy[0];
        unsigned long long far = 0;
        long long a = 0;
        for (int v = t; v < n; v += TEAM) {
            const int p = s.xy[v];
            far = max(far, sm_dist2(p, p0));
            a += sm_side(p, s.xy[v + 1 == n ? 0 : v + 1]);
        }
        if (active) atomicMax(s.bk, far);
        atomicAdd(&c.area[team][0], (unsigned long long)a);
    }
    __syncthreads();
    if (active) {
        const int p0 = s.xy[0];
        const unsigned long long far = sm_load(s.bk);
        for (int v = t; v < n; v += TEAM)
            if (sm_dist2(s.xy[v], p0) == far) { atomicMin(s.bi, v); break; }       // the thread's lowest
    }
    __syncthreads();
    const int a1 = active ? sm_load(s.bi) : 0;
    __syncthreads();                                                   // slot 0 is cleared below
    if (active) {
        for (int v = t; v < n; v += TEAM) {
            s.pv[v] = v == 0 || v == a1 ? v : v < a1 ? 0 : a1;
            s.nx[v] = v < a1 ? a1 : n;
        }
        if (t == 0) { sm_store(s.bk, 0ull); sm_store(s.bi, INT_MAX); }
    }
    __syncthreads();
    // rule 3, level by level
    for (int round = 0;; ++round) {                                    // uniform over the block
        if (active)
            for (int v = t; v < n; v += TEAM) {
                const int p = s.pv[v];
                if (p == v) continue;
                const int h = s.nx[v];
                atomicMax(s.bk + p, sm_key(s.xy[v], s.xy[p], s.xy[h == n ? 0 : h]));
            }
        __syncthreads();
        if (active)
            for (int v = t; v < n; v += TEAM) {
                const int p = s.pv[v];
                if (p == v) continue;
                const int h = s.nx[v];
                if (sm_key(s.xy[v], s.xy[p], s.xy[h == n ? 0 : h]) == sm_load(s.bk + p)) atomicMin(s.bi + p, v);
            }
        __syncthreads();
        if (active) {
            bool split = false;
            for (int v = t; v < n; v += TEAM) {
                const int p = s.pv[v];
                if (p == v) continue;
                const int h = s.nx[v];
                if (4ull * sm_load(s.bk + p) > q * sm_len(s.xy[p], s.xy[h == n ? 0 : h])) {
                    const int w = sm_load(s.bi + p);                   // p < w < h
                    split = true;
                    if (v == w) { s.pv[v] = v; s.nx[p] = v; }          // p is kept: nobody reads or writes its nx in this step
                    else if (v < w) s.nx[v] = w;
                    else s.pv[v] = w;
                }
            }
            if (split) c.flag[round & 1][team] = 1;
        }
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int k = 0; k < TEAMS; ++k) any = any || c.flag[round & 1][k];
        if (active) {
            const bool go = c.flag[round & 1][team];
            for (int v = t; v < n; v += TEAM)
                if (s.pv[v] == v) { sm_store(s.bk + v, 0ull); sm_store(s.bi + v, INT_MAX); }
            if (go && round + 1 >= n) atomicOr(status, SM_ST_ROUNDS);  // a splitting round keeps a vertex: n - 2 of them at the most
            active = go && round + 1 < n;
        }
        if (t == 0) c.flag[~round & 1][team] = 0;
        __syncthreads();
        if (!any) break;
    }
    // rule 4: nothing but the anchors was kept
    const bool ranked = n >= 4;
    if (ranked) {
        int k = 0;
        for (int v = t; v < n; v += TEAM) k += s.pv[v] == v;
        if (k) atomicAdd(&c.kept[team], k);
    }
    __syncthreads();
    const bool triangle = ranked && c.kept[team] == (a1 == 0 ? 1 : 2);
    if (triangle) {
        const int p0 = s.xy[0], p1 = s.xy[a1];
        unsigned long long best = 0;
        for (int v = t; v < n; v += TEAM)
            if (v != 0 && v != a1) best = max(best, sm_key(s.xy[v], p0, p1));
        atomicMax(s.bk, best);
    }
    __syncthreads();
    if (triangle) {
        const int p0 = s.xy[0], p1 = s.xy[a1];
        const unsigned long long best = sm_load(s.bk);
        for (int v = t; v < n; v += TEAM)
            if (v != 0 && v != a1 && sm_key(s.xy[v], p0, p1) == best) { atomicMin(s.bi, v); break; }
    }
    __syncthreads();
    const int third = triangle ? sm_load(s.bi) : -1;
    // rule 5: the area of the kept vertices against the input's
    if (ranked) {
        if (triangle) {
            if (t == 0) {
                const int i1 = min(a1, third), i2 = max(a1, third);
                const int p0 = s.xy[0], p1 = s.xy[i1], p2 = s.xy[i2];
                c.area[team][1] = (unsigned long long)(sm_side(p0, p1) + sm_side(p1, p2) + sm_side(p2, p0));
            }
        } else {
            long long a = 0;
            for (int v = t; v < n; v += TEAM)
                if (s.pv[v] == v) {
                    const int h = s.nx[v];
                    a += sm_side(s.xy[v], s.xy[h == n ? 0 : h]);
                }
            atomicAdd(&c.area[team][1], (unsigned long long)a);
        }
    }
    __syncthreads();
    const long long a_in = (long long)c.area[team][0], a_out = (long long)c.area[team][1];
    const bool whole = !ranked || a_out == 0 || (a_out > 0) != (a_in > 0);
    for (int v = t; v < n; v += TEAM) keep[v] = whole || s.pv[v] == v || v == third;
    if (t == 0 && area_out) *area_out = whole ? a_in : a_out;
    __syncthreads();                                                   // the state is another ring's after this
}

// the ring's first vertex and length, 0 where the offsets are no ring's (status bit 4: nothing of that ring is read)
__device__ __forceinline__ int sm_ring_range(const long long* __restrict__ offsets, long long r, long long R, long long V, long long& off, int* status) {
    const long long o0 = offsets[r], o1 = offsets[r + 1];
    off = 0;
    if (o0 < 0 || o1 < o0 || o1 > V || (r == 0 && o0 != 0) || (r == R - 1 && o1 != V)) { atomicOr(status, SM_ST_OFFSETS); return 0; }
    off = o0;
    return (int)(o1 - o0);                                             // V is below 2^31
}

__global__ void __launch_bounds__(256)
k_simplify_wave(const int* __restrict__ vertices, const long long* __restrict__ offsets, long long R, long long V, unsigned long long q,
                SmHeader* __restrict__ hdr, int* __restrict__ list, uint8_t* __restrict__ keep, long long* __restrict__ area) {
    constexpr int TEAMS = 256 / 64;
    __shared__ int xy[TEAMS * SM_WAVE_MAX], pv[TEAMS * SM_WAVE_MAX], nx[TEAMS * SM_WAVE_MAX], bi[TEAMS * SM_WAVE_MAX];
    __shared__ unsigned long long bk[TEAMS * SM_WAVE_MAX];
    __shared__ SmControl<TEAMS> c;
    const int team = threadIdx.x >> 6, t = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * TEAMS + team;
    long long off = 0;
    int n = 0;
    bool listed = false;
    if (r < R) {
        n = sm_ring_range(offsets, r, R, V, off, &hdr->status);
        listed = n > SM_WAVE_MAX;
        if (listed) {
            if (t == 0) list[atomicAdd(&hdr->nlist, 1)] = (int)r;      // at most R entries
            n = 0;
        }
    }
    const int o = team * SM_WAVE_MAX;
    const SmState s = {xy + o, pv + o, nx + o, bi + o, bk + o};
    sm_ring<64>(vertices + 2 * off, n, q, s, keep + off, r < R && !listed ? area + r : nullptr, &hdr->status, c, team, t);
}

__global__ void __launch_bounds__(256)
k_simplify_block(const int* __restrict__ vertices, const long long* __restrict__ offsets, long long R, long long V, unsigned long long q,
                 SmHeader* __restrict__ hdr, const int* __restrict__ list, uint8_t* __restrict__ keep, long long* __restrict__ area,
                 const SmState g) {
    __shared__ int xy[SM_LDS_MAX], pv[SM_LDS_MAX], nx[SM_LDS_MAX], bi[SM_LDS_MAX];
    __shared__ unsigned long long bk[SM_LDS_MAX];
    __shared__ SmControl<1> c;
    const int count = (int)min((long long)hdr->nlist, R);
    for (int i = blockIdx.x; i < count; i += gridDim.x) {              // uniform over the block
        const long long r = list[i];
        if (r < 0 || r >= R) continue;                                 // an index is checked before it is used
        long long off = 0;
        const int n = sm_ring_range(offsets, r, R, V, off, &hdr->status);
        if (n <= SM_LDS_MAX) {
            const SmState s = {xy, pv, nx, bi, bk};
            sm_ring<256>(vertices + 2 * off, n, q, s, keep + off, area + r, &hdr->status, c, 0, (int)threadIdx.x);
        } else {
            const SmState s = {g.xy + off, g.pv + off, g.nx + off, g.bi + off, g.bk + off};
            sm_ring<256>(vertices + 2 * off, n, q, s, keep + off, area + r, &hdr->status, c, 0, (int)threadIdx.x);
        }
    }
}

__global__ void __launch_bounds__(256)
k_simplify_sum(const uint8_t* __restrict__ keep, long long V, long long* __restrict__ sums) {
    __shared__ int wsum[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * SM_CHUNK + threadIdx.x;
    int n = 0;
    for (int k = 0; k < SM_CHUNK / 256; ++k)
        if (first + k * 256 < V) n += keep[first + k * 256] & 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (long long)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

__global__ void __launch_bounds__(256)
k_simplify_scan(long long* __restrict__ sums, int64_t nb, const long long* __restrict__ offsets, long long R, long long V,
                SmHeader* __restrict__ hdr, long long* __restrict__ counts) {
    __shared__ long long ws[4];
    const long long total = rg_block_scan(sums, nb, 1, ws);
    if (threadIdx.x == 0) {
        if (R == 0 && (V != 0 || offsets[0] != 0)) hdr->status |= SM_ST_OFFSETS;           // no ring launch has looked at them
        hdr->rings = R; hdr->vertices = V; hdr->vout = total;
        counts[0] = total; counts[1] = (long long)hdr->status;
    }
}

// the header is the count phase's own, on rings of these sizes, and n_out is what it left (bit 8 of an earlier write call aside)
__device__ __forceinline__ bool sm_write_ok(const SmHeader* __restrict__ hdr, long long R, long long V, long long n_out) {
    return (hdr->status & ~SM_ST_MISMATCH) == 0 && hdr->rings == R && hdr->vertices == V && hdr->vout == n_out;
}

__global__ void __launch_bounds__(256)
k_simplify_wverts(SmHeader* __restrict__ hdr, long long R, long long V, long long n_out, const int2* __restrict__ vertices,
                  const uint8_t* __restrict__ keep, const long long* __restrict__ sums, int* __restrict__ pos, int2* __restrict__ out) {
    __shared__ int ws[4];
    if (!sm_write_ok(hdr, R, V, n_out)) {                              // uniform over the grid: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&hdr->status, SM_ST_MISMATCH);
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * SM_CHUNK + threadIdx.x;
    long long run = sums[blockIdx.x];
    for (int k = 0; k < SM_CHUNK / 256; ++k) {                         // uniform
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
k_simplify_wrings(const SmHeader* __restrict__ hdr, long long R, long long V, long long n_out, const long long* __restrict__ offsets,
                  const int* __restrict__ pos, const long long* __restrict__ area, long long* __restrict__ out_offsets,
                  long long* __restrict__ out_area2) {
    if (!sm_write_ok(hdr, R, V, n_out)) return;                        // k_simplify_wverts has set bit 8
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r > R) return;
    const long long o = offsets[r];                                    // the count phase found 0 <= o <= V; an index is checked before it is used
    out_offsets[r] = o >= 0 && o < V ? (long long)pos[o] : n_out;
    if (r < R) out_area2[r] = area[r];
}

// ------------------------------------------------------------------------------------------------ launch sequences
namespace {

struct SmScratch {                                                     // byte offsets into the scratch buffer
    int64_t sums, area, bk, list, pos, xy, pv, nx, bi, keep, bytes;
};
inline int64_t sm_chunks(int64_t n) { return std::max<int64_t>(1, (n + SM_CHUNK - 1) / SM_CHUNK); }
inline SmScratch sm_layout(int64_t R, int64_t V) {
    SmScratch s;
    int64_t o = (int64_t)sizeof(SmHeader);
    s.sums = o; o += 8 * sm_chunks(V);
    s.area = o; o += 8 * R;
    s.bk = o; o += 8 * V;
    s.list = o; o += 4 * ((R + 1) / 2 * 2);
    int64_t* per[] = {&s.pos, &s.xy, &s.pv, &s.nx, &s.bi};
    for (int64_t* p : per) { *p = o; o += 4 * ((V + 1) / 2 * 2); }
    s.keep = o; o += V;
    s.bytes = (o + 7) / 8 * 8;
    return s;
}
inline bool sm_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool sm_sizes_ok(int64_t R, int64_t V) { return R >= 0 && V >= 0 && R < ((int64_t)1 << 31) && V < ((int64_t)1 << 31); }

}  // namespace

// for kernels_topo.hip, whose repair loop goes on from the count phase's state: where the keep bytes, the areas and the status word lie
void sm_state_of(void* scratch, int64_t n_rings, int64_t n_vertices, uint8_t** keep, long long** area, int** status) {
    const SmScratch L = sm_layout(n_rings, n_vertices);
    *keep = (uint8_t*)scratch + L.keep;
    *area = (long long*)((char*)scratch + L.area);
    *status = &((SmHeader*)scratch)->status;
}
}  // namespace stcd

using namespace stcd;

// what both entries check before anything else
#define SM_CHECK_COMMON()                                                                                                         \
    STCD_CHECK(vertices && offsets && scratch, "null pointer argument");                                                          \
    STCD_CHECK(n_rings >= 0 && n_vertices >= 0, "n_rings and n_vertices must be >= 0");                                           \
    STCD_CHECK(sm_sizes_ok(n_rings, n_vertices), "n_rings and n_vertices must be below 2^31");                                    \
    STCD_CHECK(q >= 0 && q < ((int64_t)1 << 31), "q must be in [0, 2^31)");                                                       \
    STCD_CHECK(sm_aligned(vertices, 8) && sm_aligned(offsets, 8) && sm_aligned(scratch, 8), "vertices, offsets and scratch must be 8-byte aligned"); \
    STCD_CHECK(scratch_bytes >= sm_layout(n_rings, n_vertices).bytes, "scratch too small (stcd_rings_simplify_scratch_bytes)")

extern "C" {

int64_t stcd_rings_simplify_scratch_bytes(int64_t n_rings, int64_t n_vertices) {
    if (!sm_sizes_ok(n_rings, n_vertices)) return 0;
    return sm_layout(n_rings, n_vertices).bytes;
}

int stcd_rings_simplify_count(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t q, int64_t* counts,
                              void* scratch, int64_t scratch_bytes, void* hip_stream) {
    SM_CHECK_COMMON();
    STCD_CHECK(counts != nullptr, "null pointer argument");
    STCD_CHECK(sm_aligned(counts, 8), "counts must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const SmScratch L = sm_layout(n_rings, n_vertices);
    char* b = (char*)scratch;
    SmHeader* hdr = (SmHeader*)b;
    long long* sums = (long long*)(b + L.sums);
    long long* area = (long long*)(b + L.area);
    int* list = (int*)(b + L.list);
    uint8_t* keep = (uint8_t*)(b + L.keep);
    const SmState g = {(int*)(b + L.xy), (int*)(b + L.pv), (int*)(b + L.nx), (int*)(b + L.bi), (unsigned long long*)(b + L.bk)};
    const long long R = n_rings, V = n_vertices;
    const unsigned chunks = (unsigned)sm_chunks(V);
    STCD_HIP(hipMemsetAsync(hdr, 0, sizeof(SmHeader), s));
    if (R > 0) {
        k_simplify_wave<<<(unsigned)((R + 3) / 4), 256, 0, s>>>((const int*)vertices, (const long long*)offsets, R, V, (unsigned long long)q, hdr, list,
                                                                keep, area);
        k_simplify_block<<<(unsigned)std::min<int64_t>(R, SM_BLOCK_GRID), 256, 0, s>>>((const int*)vertices, (const long long*)offsets, R, V,
                                                                                      (unsigned long long)q, hdr, list, keep, area, g);
    }
    k_simplify_sum<<<chunks, 256, 0, s>>>(keep, R > 0 ? V : 0, sums);
    k_simplify_scan<<<1, 256, 0, s>>>(sums, (int64_t)chunks, (const long long*)offsets, R, V, hdr, (long long*)counts);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_rings_simplify_write(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t q, int64_t n_out,
                              int32_t* out_vertices, int64_t* out_offsets, int64_t* out_area2, void* scratch, int64_t scratch_bytes,
                              void* hip_stream) {
    SM_CHECK_COMMON();
    STCD_CHECK(out_offsets != nullptr, "null pointer argument");
    STCD_CHECK(n_out >= 0 && n_out <= n_vertices, "n_out must be in [0, n_vertices]");
    STCD_CHECK((n_out == 0 || out_vertices) && (n_rings == 0 || out_area2), "null pointer argument");
    STCD_CHECK(sm_aligned(out_vertices, 8) && sm_aligned(out_offsets, 8) && sm_aligned(out_area2, 8), "misaligned output pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const SmScratch L = sm_layout(n_rings, n_vertices);
    char* b = (char*)scratch;
    SmHeader* hdr = (SmHeader*)b;
    const long long R = n_rings, V = n_vertices;
    k_simplify_wverts<<<(unsigned)sm_chunks(V), 256, 0, s>>>(hdr, R, V, n_out, (const int2*)vertices, (const uint8_t*)(b + L.keep),
                                                             (const long long*)(b + L.sums), (int*)(b + L.pos), (int2*)out_vertices);
    k_simplify_wrings<<<(unsigned)((R + 256) / 256), 256, 0, s>>>(hdr, R, V, n_out, (const long long*)offsets, (const int*)(b + L.pos),
                                                                  (const long long*)(b + L.area), (long long*)out_offsets, (long long*)out_area2);
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
