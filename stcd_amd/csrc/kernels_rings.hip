// kernels_rings.hip -- change polygons on the device: the boundary rings of the objects of a label image (gfx950), with their C-ABI
// entries.  Continues kernels_objects.hip from numbered objects to vector data; tests/rings_spec.py states every output in plain
// Python.  Integers only: no float arithmetic and no float atomics, so every output is a pure function of the input; pixel and
// vertex offsets are 64-bit, corner ids are int32 (the corner capacity is below 2^31); the labels are read with 4-byte loads and
// no demand on the width.  Every phase is its own launch, no block waits for another block, and no thread walks a ring.
//
// Lattice: vertex (y, x), 0 <= y <= H, 0 <= x <= W; the four pixels round it are quad[0] = (y-1, x-1), quad[1] = (y-1, x),
// quad[2] = (y, x-1), quad[3] = (y, x), read as 0 outside the scene.  The directed unit edge that leaves the vertex in direction t
// (0 east, 1 south, 2 west, 3 north) is owned by quad[P(t)] and exists where that pixel is labelled and quad[Q(t)], across the
// edge, carries another label.  The edge that arrives straight from behind is owned by quad[R(t)] with quad[S(t)] across it: an
// existing edge continues a straight run iff quad[R(t)] has the owner's label and quad[S(t)] has not, and is a CORNER otherwise
// (a turn of the ring, both edges of a saddle included).  So corners are detected from the 2 x 2 neighbourhood of a vertex alone.
//
//   k_ring_count / k_ring_scan / k_ring_emit   the three-launch prefix sum of kernels_objects.hip over the corner counts (0..4)
//                  of the vertices: per RG_CHUNK vertices, one block scans the chunk sums, then every vertex with a corner stores
//                  the id of its first one and every corner its (y, x, dir).  Ids are numbered in key order (y, x, dir), so the
//                  smallest id of a ring is the ring's start.
//   k_ring_link    one thread per corner: the straight run to the next vertex where the ring turns (at most max(H, W) unit steps,
//                  two label loads each, under an iteration cap), the turn from the two pixels ahead (left at a saddle under
//                  connectivity 8, right under 4), and the id of that corner from the vertex's first id: next[id].
//   k_ring_jump    pointer jumping, one launch per round with ping-pong buffers (nothing is read and written in one launch): after
//                  round r every corner knows the smallest id m among its 2^(r+1) successors-or-self and its distance d to the
//                  first of them.  ceil(log2 V) rounds are needed; the host launches ceil(log2 capacity) and a launch past the
//                  device's own round count returns at once.
//   k_ring_starts  a corner with m == id starts a ring: one 64-bit integer atomicAdd of the count per block.
//   k_ring_wsum / k_ring_wscan / k_ring_wrings  the same prefix sum over the starts (ring number) and their ring lengths
//                  (offsets), then object, offsets and a zeroed area2 per ring.
//   k_ring_wverts  one thread per corner: its place is offsets[ring] + (length - d) % length; twice the signed area is summed per
//                  run of one ring within a wave's 64 consecutive corners and added with one 64-bit integer atomicAdd per run
//                  (Guideline 12: not one atomic per vertex).
#include <algorithm>
#include <climits>

#include "common.h"
#include "ring_scan.h"                         // rg_wave_scan, rg_block_scan

namespace stcd {

#define RG_CHUNK 4096                         // vertices (corners in the write phase) per block of the scans: 256 threads x 16
#define RG_MAX_GRID 2048                       // blocks of the grid-stride passes over the corners (Guideline 11)

enum { RG_ST_WALK = 1, RG_ST_LINK = 2, RG_ST_CAPACITY = 4, RG_ST_MISMATCH = 8 };

struct RgHeader {                              // the first 32 bytes of the scratch buffer, kept from the count to the write phase
    long long rings, corners;
    int rounds, status;
    int bad, pad_;                             // bad: the write phase found R / V to disagree and writes nothing
};

// quad index of the owner of the edge of direction t, of the pixel across it, and of the two pixels behind the tail
__host__ __device__ constexpr int rg_p(int t) { return (0x1023 >> (4 * t)) & 3; }
__host__ __device__ constexpr int rg_q(int t) { return (0x0231 >> (4 * t)) & 3; }
__host__ __device__ constexpr int rg_r(int t) { return (0x3102 >> (4 * t)) & 3; }
__host__ __device__ constexpr int rg_s(int t) { return (0x2310 >> (4 * t)) & 3; }

__device__ __forceinline__ int rg_at(const int* __restrict__ lab, int H, int W, int y, int x) {
    if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0;
    const int l = lab[(int64_t)y * W + x];
    return l > 0 ? l : 0;
}
// pixel quad[i] of vertex (y, x)
__device__ __forceinline__ int rg_quad_at(const int* __restrict__ lab, int H, int W, int y, int x, int i) {
    return rg_at(lab, H, W, y - 1 + (i >> 1), x - 1 + (i & 1));
}
__device__ __forceinline__ unsigned rg_corners(const int* __restrict__ lab, int H, int W, int y, int x) {
    int q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = rg_quad_at(lab, H, W, y, x, i);
    unsigned m = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = q[rg_p(t)];
        if (p != 0 && p != q[rg_q(t)] && !(q[rg_r(t)] == p && q[rg_s(t)] != p)) m |= 1u << t;
    }
    return m;
}

// the vertex of linear index i (one 64-bit division per thread) and the step of 256 vertices
struct RgCursor { int y, x, qy, rx; };
__device__ __forceinline__ RgCursor rg_cursor(int64_t i, int Wp) {
    RgCursor c;
    c.y = (int)(i / Wp); c.x = (int)(i - (int64_t)c.y * Wp);
    c.qy = 256 / Wp; c.rx = 256 - c.qy * Wp;
    return c;
}
__device__ __forceinline__ void rg_advance(RgCursor& c, int Wp) {
    c.y += c.qy; c.x += c.rx;
    if (c.x >= Wp) { c.x -= Wp; ++c.y; }
}

// ------------------------------------------------------------------------------------------------ count phase: numbering
__global__ void __launch_bounds__(256)
k_ring_count(const int* __restrict__ lab, int H, int W, int64_t NV, long long* __restrict__ sums) {
    __shared__ int wsum[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * RG_CHUNK + threadIdx.x;
    RgCursor c = rg_cursor(first, W + 1);
    int n = 0;
    for (int k = 0; k < RG_CHUNK / 256; ++k) {
        if (first + k * 256 < NV) n += __popc(rg_corners(lab, H, W, c.y, c.x));
        rg_advance(c, W + 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (long long)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

__global__ void __launch_bounds__(256)
k_ring_scan(long long* __restrict__ sums, int64_t nb, long long cap, RgHeader* __restrict__ hdr) {
    __shared__ long long ws[4];
    const long long V = rg_block_scan(sums, nb, 1, ws);
    if (threadIdx.x == 0) {
        hdr->corners = V;
        int rounds = 0;
        while (rounds < 31 && (1ll << rounds) < V) ++rounds;           // ceil(log2 V): 2^rounds covers the longest ring
        hdr->rounds = rounds;
        if (V > cap) hdr->status |= RG_ST_CAPACITY;                    // nothing below this launch touches a corner then
    }
}

__global__ void __launch_bounds__(256)
k_ring_emit(const int* __restrict__ lab, int H, int W, int64_t NV, const long long* __restrict__ sums, const RgHeader* __restrict__ hdr,
            long long cap, int* __restrict__ base, int* __restrict__ cy, int* __restrict__ cx, uint8_t* __restrict__ cdir) {
    __shared__ int ws[4];
    if (hdr->corners > cap) return;                                    // uniform over the grid
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * RG_CHUNK + threadIdx.x;
    RgCursor c = rg_cursor(first, W + 1);
    long long run = sums[blockIdx.x];
    for (int k = 0; k < RG_CHUNK / 256; ++k) {                         // uniform
        const int64_t i = first + k * 256;
        const unsigned m = i < NV ? rg_corners(lab, H, W, c.y, c.x) : 0u;
        const int cnt = __popc(m);
        const int inc = (int)rg_wave_scan((long long)cnt, lane);
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) before += ws[w]; total += ws[w]; }
        if (m) {
            long long id = run + before + inc - cnt;                   // < corners <= cap < 2^31
            base[i] = (int)id;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if ((m >> t) & 1u) {
                    if (id < cap) { cy[id] = c.y; cx[id] = c.x; cdir[id] = (uint8_t)t; }
                    ++id;
                }
        }
        run += total;
        rg_advance(c, W + 1);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ count phase: links
__global__ void __launch_bounds__(256)
k_ring_link(const int* __restrict__ lab, int H, int W, int conn8, RgHeader* __restrict__ hdr, long long cap, const int* __restrict__ base,
            const int* __restrict__ cy, const int* __restrict__ cx, const uint8_t* __restrict__ cdir, int* __restrict__ next,
            int* __restrict__ jump, int* __restrict__ m, int* __restrict__ d) {
    const long long V = hdr->corners;
    if (V > cap) return;
    const int steps = max(H, W) + 1;
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < V; id += (int64_t)gridDim.x * 256) {
        int y = cy[id], x = cx[id];
        const int t = cdir[id];
        const int k = rg_quad_at(lab, H, W, y, x, (0x1023 >> (4 * t)) & 3);
        const int sy = (t == 1) - (t == 3), sx = (t == 0) - (t == 2);
        const int pi = (0x1023 >> (4 * t)) & 3, qi = (0x0231 >> (4 * t)) & 3;
        int nt = -1;
        for (int n = 0; n < steps; ++n) {                              // leaves the scene at the latest: the pixels ahead read 0 there
            y += sy; x += sx;
            const bool ahead = rg_quad_at(lab, H, W, y, x, pi) == k, across = rg_quad_at(lab, H, W, y, x, qi) == k;
            if (ahead && !across) continue;                            // the run goes on
            nt = ahead ? (t + 3) & 3 : (across && conn8) ? (t + 3) & 3 : (t + 1) & 3;
            break;
        }
        int to = (int)id;                                              // a bug below leaves a ring of one corner: every index stays valid
        if (k == 0 || nt < 0 || (unsigned)y > (unsigned)H || (unsigned)x > (unsigned)W) atomicOr(&hdr->status, RG_ST_WALK);
        else {
            const unsigned mk = rg_corners(lab, H, W, y, x);
            const long long tid = (mk >> nt) & 1u ? (long long)base[(int64_t)y * (W + 1) + x] + __popc(mk & ((1u << nt) - 1u)) : -1;
            if (tid < 0 || tid >= V) atomicOr(&hdr->status, RG_ST_LINK);
            else to = (int)tid;
        }
        next[id] = to; jump[id] = to; m[id] = (int)id; d[id] = 0;
    }
}

// round r: (jump, m, d) of the source buffers -> the destination buffers.  m: the smallest id among the corner and its 2^(r+1) - 1
// successors; d: the distance to the FIRST of them (on a tie the nearer half wins, so d stays below the ring's length)
__global__ void __launch_bounds__(256)
k_ring_jump(int r, const RgHeader* __restrict__ hdr, long long cap, const int* __restrict__ js, const int* __restrict__ ms,
            const int* __restrict__ ds, int* __restrict__ jd, int* __restrict__ md, int* __restrict__ dd) {
    const long long V = hdr->corners;
    if (V > cap || r >= hdr->rounds) return;
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < V; id += (int64_t)gridDim.x * 256) {
        const int j = js[id];
        const int m1 = ms[id], m2 = ms[j];
        const bool far = m2 < m1;
        md[id] = far ? m2 : m1;
        dd[id] = far ? (1 << r) + ds[j] : ds[id];
        jd[id] = js[j];
    }
}

__global__ void __launch_bounds__(256)
k_ring_starts(RgHeader* __restrict__ hdr, long long cap, const int* __restrict__ mA, const int* __restrict__ mB) {
    __shared__ int wsum[4];
    const long long V = hdr->corners;
    if (V > cap) return;
    const int* __restrict__ m = (hdr->rounds & 1) ? mB : mA;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int n = 0;
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < V; id += (int64_t)gridDim.x * 256) n += m[id] == (int)id;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (threadIdx.x == 0 && total) atomicAdd((unsigned long long*)&hdr->rings, (unsigned long long)total);
}

__global__ void k_ring_publish(const RgHeader* __restrict__ hdr, long long* __restrict__ counts) {
    if (threadIdx.x == 0) { counts[0] = hdr->rings; counts[1] = hdr->corners; counts[2] = (long long)hdr->status; }
}

// ------------------------------------------------------------------------------------------------ write phase
// csum[2 b], csum[2 b + 1]: the starts of corner chunk b and the sum of their ring lengths (length = d[next[start]] + 1)
__global__ void __launch_bounds__(256)
k_ring_wsum(const RgHeader* __restrict__ hdr, long long V, const int* __restrict__ next, const int* __restrict__ mA, const int* __restrict__ mB,
            const int* __restrict__ dA, const int* __restrict__ dB, long long* __restrict__ csum) {
    __shared__ long long ws[8];
    const bool odd = hdr->rounds & 1;
    const int* __restrict__ m = odd ? mB : mA;
    const int* __restrict__ d = odd ? dB : dA;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long lim = hdr->status == 0 && hdr->corners == V ? V : 0;                   // nothing but what the count phase wrote
    long long n = 0, len = 0;
    for (int k = 0; k < RG_CHUNK / 256; ++k) {
        const int64_t id = (int64_t)blockIdx.x * RG_CHUNK + k * 256 + threadIdx.x;
        if (id < lim && m[id] == (int)id) {
            const int nx = next[id];
            if ((long long)(unsigned)nx < V) { ++n; len += d[nx] + 1; }                    // an index is checked before it is used
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n += __shfl_xor(n, o, 64); len += __shfl_xor(len, o, 64); }
    if (lane == 0) { ws[wave] = n; ws[4 + wave] = len; }
    __syncthreads();
    if (threadIdx.x == 0) {
        csum[2 * (int64_t)blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
        csum[2 * (int64_t)blockIdx.x + 1] = ws[4] + ws[5] + ws[6] + ws[7];
    }
}

__global__ void __launch_bounds__(256)
k_ring_wscan(long long* __restrict__ csum, int64_t nb, long long R, long long V, RgHeader* __restrict__ hdr) {
    __shared__ long long ws[4];
    const long long rings = rg_block_scan(csum, nb, 2, ws);
    const long long verts = rg_block_scan(csum + 1, nb, 2, ws);
    if (threadIdx.x == 0) {
        const bool ok = hdr->status == 0 && R == hdr->rings && V == hdr->corners && rings == R && verts == V;
        hdr->bad = ok ? 0 : 1;
        if (!ok) hdr->status |= RG_ST_MISMATCH;
    }
}

__global__ void __launch_bounds__(256)
k_ring_wrings(const int* __restrict__ lab, int H, int W, const RgHeader* __restrict__ hdr, long long R, long long V,
              const long long* __restrict__ csum, const int* __restrict__ cy, const int* __restrict__ cx, const uint8_t* __restrict__ cdir,
              const int* __restrict__ next, int* __restrict__ mA, int* __restrict__ mB, const int* __restrict__ dA, const int* __restrict__ dB,
              long long* __restrict__ offsets, int* __restrict__ object, long long* __restrict__ area2) {
    __shared__ long long ws[8];
    if (hdr->bad) return;
    const bool odd = hdr->rounds & 1;
    const int* __restrict__ m = odd ? mB : mA;
    const int* __restrict__ d = odd ? dB : dA;
    int* __restrict__ ridx = odd ? mA : mB;                            // the idle buffer: ridx[start] = the ring's number
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[R] = V;
    long long run_r = csum[2 * (int64_t)blockIdx.x], run_v = csum[2 * (int64_t)blockIdx.x + 1];
    for (int k = 0; k < RG_CHUNK / 256; ++k) {                         // uniform
        const int64_t id = (int64_t)blockIdx.x * RG_CHUNK + k * 256 + threadIdx.x;
        const int nx = id < V ? next[id] : -1;
        const bool start = id < V && m[id] == (int)id && (long long)(unsigned)nx < V;
        const long long len = start ? d[nx] + 1 : 0;
        const unsigned long long b = __ballot(start);
        const long long inc = rg_wave_scan(len, lane);
        if (lane == 63) { ws[wave] = __popcll(b); ws[4 + wave] = inc; }
        __syncthreads();
        long long before_r = 0, before_v = 0, total_r = 0, total_v = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) { before_r += ws[w]; before_v += ws[4 + w]; }
            total_r += ws[w]; total_v += ws[4 + w];
        }
        const long long ring = run_r + before_r + __popcll(b & ((1ull << lane) - 1ull));             // < R: the scan's totals agreed
        if (start && ring < R) {
            ridx[id] = (int)ring;
            offsets[ring] = run_v + before_v + inc - len;
            object[ring] = rg_quad_at(lab, H, W, cy[id], cx[id], (0x1023 >> (4 * cdir[id])) & 3);
            area2[ring] = 0;
        }
        run_r += total_r; run_v += total_v;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_ring_wverts(const RgHeader* __restrict__ hdr, long long V, const int* __restrict__ cy, const int* __restrict__ cx, const int* __restrict__ next,
              const int* __restrict__ mA, const int* __restrict__ mB, const int* __restrict__ dA, const int* __restrict__ dB,
              const long long* __restrict__ offsets, int* __restrict__ vertices, unsigned long long* __restrict__ area2) {
    if (hdr->bad) return;
    const bool odd = hdr->rounds & 1;
    const int* __restrict__ m = odd ? mB : mA;
    const int* __restrict__ d = odd ? dB : dA;
    const int* __restrict__ ridx = odd ? mA : mB;
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < V; base += (int64_t)gridDim.x * 256) {      // uniform over the block
        const int64_t id = base + threadIdx.x;
        bool live = id < V;
        int start = -1, ring = 0;
        long long term = 0;
        const long long R = hdr->rings;
        if (live) {
            start = m[id];
            const int nx = next[id];
            live = (long long)(unsigned)start < V && (long long)(unsigned)nx < V;
            if (live) ring = ridx[start];
            live = live && (long long)(unsigned)ring < R;
            if (!live) start = -1;                                     // what no count phase wrote: an index is checked before it is used
        }
        if (live) {
            const long long off = offsets[ring], len = offsets[ring + 1] - off;
            const int dist = d[id];
            const long long pos = off + (dist ? len - dist : 0);
            const int y = cy[id], x = cx[id], nx = next[id];
            if (pos >= 0 && pos < V) { vertices[2 * pos] = y; vertices[2 * pos + 1] = x; }
            term = (long long)x * cy[nx] - (long long)cx[nx] * y;
        }
        // one atomic per run of one ring among the wave's 64 consecutive corners
        const int prev = __shfl_up(start, 1, 64);
        const bool head = live && (lane == 0 || prev != start);
        const unsigned long long S = __ballot(live), Hd = __ballot(head);
        const long long inc = rg_wave_scan(term, lane);
        int last = lane;
        if (head) {
            const unsigned long long above = lane >= 63 ? 0ull : ~((2ull << lane) - 1ull);
            const unsigned long long stop = (Hd | ~S) & above;
            last = (stop ? __ffsll((long long)stop) - 1 : 64) - 1;
        }
        const long long upto = __shfl(inc, last, 64);
        if (head) atomicAdd(area2 + ring, (unsigned long long)(upto - (inc - term)));
    }
}

// ------------------------------------------------------------------------------------------------ launch sequences
namespace {

struct RgScratch {                                                     // byte offsets into the scratch buffer
    int64_t base, sums, csum, cy, cx, next, jump[2], m[2], d[2], cdir, bytes;
};
inline int64_t rg_chunks(int64_t n) { return (n + RG_CHUNK - 1) / RG_CHUNK; }
inline RgScratch rg_layout(int64_t H, int64_t W, int64_t cap) {
    const int64_t nv = (H + 1) * (W + 1);
    RgScratch s;
    int64_t o = (int64_t)sizeof(RgHeader);
    s.sums = o; o += 8 * rg_chunks(nv);
    s.csum = o; o += 16 * (rg_chunks(cap) + 1);
    s.base = o; o += 4 * nv;
    int64_t* per[] = {&s.cy, &s.cx, &s.next, &s.jump[0], &s.m[0], &s.d[0], &s.jump[1], &s.m[1], &s.d[1]};
    for (int64_t* p : per) { *p = o; o += 4 * cap; }
    s.cdir = o; o += cap;
    s.bytes = (o + 7) / 8 * 8;
    return s;
}
inline unsigned rg_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, RG_MAX_GRID)); }
inline bool rg_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace
}  // namespace stcd

using namespace stcd;

// what both entries check before anything else
#define RG_CHECK_COMMON()                                                                                                        \
    STCD_CHECK(labels && scratch, "null pointer argument");                                                                      \
    STCD_CHECK(height >= 0 && width >= 0 && height < INT_MAX && width < INT_MAX, "bad shape");                                   \
    STCD_CHECK((int64_t)height * width < ((int64_t)1 << 31), "height * width must be below 2^31 (int32 labels)");                \
    STCD_CHECK(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");                                           \
    STCD_CHECK(max_corners >= 0 && max_corners < ((int64_t)1 << 31), "max_corners must be in [0, 2^31)");                         \
    STCD_CHECK(rg_aligned(labels, 4) && rg_aligned(scratch, 8), "labels must be 4-byte, scratch 8-byte aligned");                 \
    STCD_CHECK(scratch_bytes >= rg_layout(height, width, max_corners).bytes, "scratch too small (stcd_rings_scratch_bytes)")

extern "C" {

int64_t stcd_rings_scratch_bytes(int height, int width, int64_t max_corners) {
    if (height < 0 || width < 0 || height == INT_MAX || width == INT_MAX || (int64_t)height * width >= ((int64_t)1 << 31) || max_corners < 0 || max_corners >= ((int64_t)1 << 31)) return 0;
    return rg_layout(height, width, max_corners).bytes;
}

int stcd_rings_count(const int32_t* labels, int height, int width, int connectivity, int64_t max_corners, int64_t* counts, void* scratch,
                     int64_t scratch_bytes, void* hip_stream) {
    RG_CHECK_COMMON();
    STCD_CHECK(counts != nullptr, "null pointer argument");
    STCD_CHECK(rg_aligned(counts, 8), "counts must be 8-byte aligned");
    if (height == 0 || width == 0) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    const RgScratch L = rg_layout(height, width, max_corners);
    char* b = (char*)scratch;
    RgHeader* hdr = (RgHeader*)b;
    long long* sums = (long long*)(b + L.sums);
    int *base = (int*)(b + L.base), *cy = (int*)(b + L.cy), *cx = (int*)(b + L.cx), *next = (int*)(b + L.next);
    int* jump[2] = {(int*)(b + L.jump[0]), (int*)(b + L.jump[1])};
    int* m[2] = {(int*)(b + L.m[0]), (int*)(b + L.m[1])};
    int* d[2] = {(int*)(b + L.d[0]), (int*)(b + L.d[1])};
    uint8_t* cdir = (uint8_t*)(b + L.cdir);
    const int64_t nv = ((int64_t)height + 1) * ((int64_t)width + 1);
    const unsigned chunks = (unsigned)rg_chunks(nv), grid = rg_grid(max_corners);
    const long long cap = max_corners;
    STCD_HIP(hipMemsetAsync(hdr, 0, sizeof(RgHeader), s));
    k_ring_count<<<chunks, 256, 0, s>>>(labels, height, width, nv, sums);
    k_ring_scan<<<1, 256, 0, s>>>(sums, (int64_t)chunks, cap, hdr);
    k_ring_emit<<<chunks, 256, 0, s>>>(labels, height, width, nv, sums, hdr, cap, base, cy, cx, cdir);
    k_ring_link<<<grid, 256, 0, s>>>(labels, height, width, connectivity == 8, hdr, cap, base, cy, cx, cdir, next, jump[0], m[0], d[0]);
    int rounds = 0;
    while (((int64_t)1 << rounds) < max_corners) ++rounds;             // ceil(log2 capacity) >= the device's ceil(log2 V)
    for (int r = 0; r < rounds; ++r)
        k_ring_jump<<<grid, 256, 0, s>>>(r, hdr, cap, jump[r & 1], m[r & 1], d[r & 1], jump[~r & 1], m[~r & 1], d[~r & 1]);
    k_ring_starts<<<grid, 256, 0, s>>>(hdr, cap, m[0], m[1]);
    k_ring_publish<<<1, 64, 0, s>>>(hdr, (long long*)counts);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_rings_write(const int32_t* labels, int height, int width, int connectivity, int64_t max_corners, int64_t n_rings, int64_t n_vertices,
                     int32_t* vertices, int64_t* offsets, int32_t* object, int64_t* area2, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    RG_CHECK_COMMON();
    STCD_CHECK(offsets != nullptr, "null pointer argument");
    STCD_CHECK(n_rings >= 0 && n_vertices >= 0, "n_rings and n_vertices must be >= 0");
    STCD_CHECK(n_vertices <= max_corners, "n_vertices is above max_corners: the count phase did not complete (status bit 4)");
    STCD_CHECK(n_vertices >= 4 * n_rings && n_vertices % 2 == 0 && (n_rings == 0) == (n_vertices == 0),
               "n_rings / n_vertices are no result of the count phase (every ring has an even number >= 4 of vertices)");
    STCD_CHECK(n_vertices <= 4 * (((int64_t)height + 1) * ((int64_t)width + 1)), "n_vertices is above four per lattice vertex");
    STCD_CHECK(n_rings == 0 || (vertices && object && area2), "null pointer argument");
    STCD_CHECK(rg_aligned(vertices, 4) && rg_aligned(object, 4) && rg_aligned(offsets, 8) && rg_aligned(area2, 8), "misaligned output pointer");
    if (height == 0 || width == 0) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    const RgScratch L = rg_layout(height, width, max_corners);
    char* b = (char*)scratch;
    RgHeader* hdr = (RgHeader*)b;
    long long* csum = (long long*)(b + L.csum);
    int *cy = (int*)(b + L.cy), *cx = (int*)(b + L.cx), *next = (int*)(b + L.next);
    int *mA = (int*)(b + L.m[0]), *mB = (int*)(b + L.m[1]), *dA = (int*)(b + L.d[0]), *dB = (int*)(b + L.d[1]);
    uint8_t* cdir = (uint8_t*)(b + L.cdir);
    const long long R = n_rings, V = n_vertices;
    const unsigned chunks = (unsigned)std::max<int64_t>(1, rg_chunks(V));
    k_ring_wsum<<<chunks, 256, 0, s>>>(hdr, V, next, mA, mB, dA, dB, csum);
    k_ring_wscan<<<1, 256, 0, s>>>(csum, (int64_t)chunks, R, V, hdr);
    k_ring_wrings<<<chunks, 256, 0, s>>>(labels, height, width, hdr, R, V, csum, cy, cx, cdir, next, mA, mB, dA, dB, (long long*)offsets, object,
                                         (long long*)area2);
    k_ring_wverts<<<rg_grid(V), 256, 0, s>>>(hdr, V, cy, cx, next, mA, mB, dA, dB, (const long long*)offsets, vertices, (unsigned long long*)area2);
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
