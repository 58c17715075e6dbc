// kernels_conv_tile.hip -- 3x3 stride-1 convolutions with Ci % 64 == 0 on SMALL maps (forward, data gradient, stride-1 transposed):
// k_conv_res's tile, fragment image, accumulation order and epilogue, with the staging done by LDS-DMA
// (`buffer_load_dwordx4 ... lds`) so that everything a tile needs is requested before the first multiplication.
//
//   * block = 4 waves, output tile 16 rows x 16 columns x NT n-tiles of 16 channels; wave w owns rows 4w .. 4w + 3.  Blocks are
//     persistent over the tiles bl, bl + P, ... of their BatchNorm group, exactly as k_conv_res's.
//   * the filter slice (mode-A fragment image of conv_mfma_plan, CiB = 64; LDS order [32-ch chunk][tap][NT][64 lanes][16 B]) goes to
//     LDS once per block, one DMA instruction per 1-KB fragment: the image is lane-linear per fragment.
//   * the 18 x 18 halo is staged in PARTS of 64 channels (128-B pixel rows; the 16-B chunk index XOR-swizzled by (column >> 1) & 7
//     -- on the per-lane SOURCE address, a DMA's LDS image is lane-linear -- and read back with the same XOR).  A part is 41 DMA
//     instructions of 8 pixels x 8 chunks; every wave issues 11 (an index past the part repeats instruction 40: the same bytes to
//     the same place), so all waves count alike.  Pixels outside the image get an offset past num_records and land as zeros.
//   * NBUF = min(Ci / 64, 2) part buffers.  The block walks the steps (tile, part) in order; the first NBUF steps are requested
//     at entry behind the filter, step s + NBUF is requested into the buffer of step s right behind the barrier that ends step s's
//     MFMAs.  So for Ci <= 128 the WHOLE K of a tile is requested before its first MFMA and the next tile's parts fly under this
//     tile's; for Ci = 256 two parts are in flight while one multiplies.  No VGPR destination: nothing for the compiler to
//     serialise.  A step = [counted s_waitcnt vmcnt, s_barrier] [216 * NT / 3 ... MFMAs out of LDS, no global wait] [lgkmcnt(0),
//     s_barrier] [request] [epilogue of the tile behind its last part].
//   * the counted wait: vmcnt counts DMAs and stores together, in issue order.  Younger than step s's DMAs are the requests of the
//     steps still ahead (11 instructions each) and, when a tile ended within the last NBUF steps, that tile's output stores -- always
//     exactly 4 * NT per wave: the epilogue stores unconditionally and drops what lies outside the map by the range check.
//   * accumulation order of every output element: 32-channel chunk ascending, then column shift, then row shift, weights as the
//     MFMA's A operand -- k_conv_res's order, so the stored outputs are bit-identical to its.
//   * epilogue: bias, bf16 NHWC store (ldo >= co), optional per-channel sums into the int64 accumulators (k_conv_res's code).
//   * MEASURED (MI355X, per op with the repack launch): 9 - 17 % faster than k_conv_res on the fourteen
//     64- to 256-channel shapes of the 64^2 / 32^2 levels (32 x 32^2 x 128 -> 128: 24.8 -> 22.0 us; 32 x 64^2 x 64 -> 64: 24.9 -> 20.6 us);
//     the SiamUnet_diff step 2.108 -> 2.074 ms.  Its waves live 29.7 k cycles for 9.2 k cycles of MFMAs (conv42): the fragment reads
//     take the LDS port as long as the MFMAs take the matrix units.
#include <algorithm>

#include "common.h"

namespace stcd {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

struct ConvTileArgs {
    stcd_conv_geom g;
    const bf16* in;
    const bf16* wf;        // mode-A fragment image of conv_mfma_plan (CiB = 64): [Ci/64][tap][2][NTtot][64][8]
    const float* bias;     // nullable
    bf16* out;
    int NTtot;             // n-tiles of the image
    int nparts, nbuf;      // Ci / 64; part buffers in LDS
    int nslices, P, groups;
    int tiles_x, tiles_y, ntiles;
    int filt_bytes;
    long long* stat_acc;   // nullable: see ConvResArgs
    int cpad, stat_c0;
    float s1_scale, s2_scale;
    unsigned in_bytes, wf_bytes, out_bytes;
    int8_t tix[3][3];      // tap index of every (row shift, column shift)
};

constexpr int TL_HW = 18;                      // halo edge of the 16 x 16 output tile
constexpr int TL_NDMA = 41;                    // DMA instructions of a part: 324 pixels, 8 per instruction
constexpr int TL_PART = TL_NDMA * 1024;        // LDS bytes of a part
constexpr int TL_NI = 11;                      // DMA instructions per wave and part
#define TL_LDS(P_) ((__attribute__((address_space(3))) void*)(P_))
#define TL_WAIT(N_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory")

template <int NT>
__global__ void __launch_bounds__(256, NT == 4 ? 1 : 2)
k_conv_tile(const ConvTileArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, r = lane & 15;
    const int P = a.P;
    const int bl = blockIdx.x % P, rest = blockIdx.x / P, slice = rest % a.nslices, grp = rest / a.nslices;
    char* const filt = smem;                                  // [32-ch chunk][tap][NT][64 lanes][16 B]
    char* const halo0 = smem + a.filt_bytes;                  // nbuf parts, TL_PART apart
    const int nparts = a.nparts, nbuf = a.nbuf;

    // the descriptor of X starts one row + one pixel BEFORE the tensor: offsets relative to a halo's corner are never negative
    const int64_t lead = ((int64_t)a.g.wi + 1) * a.g.ldi * 2;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(a.in)) - lead, (short)0, (int)(a.in_bytes + (unsigned)lead), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(a.wf)), (short)0, (int)a.wf_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<char*>(a.out), (short)0, (int)a.out_bytes, 0x00020000);

    // ---- bias first (ordinary loads: waited for before any DMA is in flight)
    float bv[NT][4];
#pragma unroll
    for (int t2 = 0; t2 < NT; ++t2) {
        const int cb = (slice * NT + t2) * 16 + 4 * q;        // (the plan requires co % 16 == 0: always a whole float4)
        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.bias) b4 = *reinterpret_cast<const float4*>(a.bias + cb);
        bv[t2][0] = b4.x; bv[t2][1] = b4.y; bv[t2][2] = b4.z; bv[t2][3] = b4.w;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- the block's filter slice: wave w requests fragments w, w + 4, ... (an index past the slice repeats the last fragment)
    {
        const int nfrag = nparts * 2 * 9 * NT;
        for (int f0 = wid; f0 < nfrag + wid; f0 += 4) {
            const int f = min(f0, nfrag - 1);
            const int ntl = f % NT, ft = f / NT, t = ft % 9, c32 = ft / 9;
            const int src = (((c32 >> 1) * 9 + t) * 2 + (c32 & 1)) * a.NTtot + slice * NT + ntl;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, TL_LDS(filt + f * 1024), 16, lane * 16,
                                                     __builtin_amdgcn_readfirstlane(src * 1024), 0, 0);
        }
    }

    // ---- halo staging plan: instruction i of this wave moves pixels (min(wid + 4 i, 40)) * 8 + (lane >> 3), LDS slot lane & 7
    int pyx[TL_NI], poff[TL_NI];
#pragma unroll
    for (int i = 0; i < TL_NI; ++i) {
        const int pix = min(wid + 4 * i, TL_NDMA - 1) * 8 + (lane >> 3);
        const int hx = pix % TL_HW, hy = pix / TL_HW;
        const int ch = (lane & 7) ^ ((hx >> 1) & 7);
        pyx[i] = pix < TL_HW * TL_HW ? (((hy - 1) << 16) | ((hx - 1) & 0xffff)) : (0x4000 << 16);     // past the halo: far outside every image
        poff[i] = ((hy * a.g.wi + hx) * a.g.ldi + ch * 8) * 2;        // bytes past the halo's top-left pixel
    }

    // tile walk inside the group: tiles bl, bl + P, ...
    const int tpg = a.ntiles / a.groups;
    const int tiles_img = a.tiles_x * a.tiles_y;
    const int dn = P / tiles_img, drem = P - dn * tiles_img, dty = drem / a.tiles_x, dtx = drem - dty * a.tiles_x;
    const int tile0 = grp * tpg + bl;
    const int tile_end = (grp + 1) * tpg;
    struct Pos { int tile, n, y, x, c; };
#define TL_ADV(P_)                                                                                                     \
    do {                                                                                                               \
        if (++(P_).c == nparts) {                                                                                      \
            (P_).c = 0; (P_).tile += P;                                                                                \
            (P_).x += dtx; if ((P_).x >= a.tiles_x) { (P_).x -= a.tiles_x; ++(P_).y; }                                 \
            (P_).y += dty; if ((P_).y >= a.tiles_y) { (P_).y -= a.tiles_y; ++(P_).n; }                                 \
            (P_).n += dn;                                                                                              \
        }                                                                                                              \
    } while (0)
#define TL_REQ(P_, BUF_)                                                                                               \
    do {                                                                                                               \
        const int gy0_ = (P_).y * 16, gx0_ = (P_).x * 16;                                                               \
        const int soff_ = __builtin_amdgcn_readfirstlane(                                                              \
            (int)(((((int64_t)(P_).n * a.g.hi + gy0_) * a.g.wi + gx0_) * a.g.ldi + (P_).c * 64) * 2));                 \
        char* const dst_ = halo0 + (BUF_) * TL_PART;                                                                   \
        _Pragma("unroll") for (int i = 0; i < TL_NI; ++i) {                                                            \
            const int hy_ = pyx[i] >> 16, hx_ = (int)(short)(pyx[i] & 0xffff);                                         \
            const bool ok_ = (unsigned)(gy0_ + hy_) < (unsigned)a.g.hi && (unsigned)(gx0_ + hx_) < (unsigned)a.g.wi;   \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, TL_LDS(dst_ + min(wid + 4 * i, TL_NDMA - 1) * 1024), 16,     \
                                                     ok_ ? poff[i] : (int)0x80000000u, soff_, 0, 0);                   \
        }                                                                                                              \
    } while (0)

    Pos cur{tile0, 0, 0, 0, 0};
    cur.n = tile0 / tiles_img;
    { const int trem = tile0 - cur.n * tiles_img; cur.y = trem / a.tiles_x; cur.x = trem - cur.y * a.tiles_x; }
    Pos rq = cur;
    int inflight = 0;                                  // steps requested and not yet waited for
    for (int k = 0; k < nbuf; ++k)
        if (rq.tile < tile_end) { TL_REQ(rq, k); TL_ADV(rq); ++inflight; }

    float s1[NT][4], s2[NT][4];
#pragma unroll
    for (int t2 = 0; t2 < NT; ++t2)
#pragma unroll
        for (int j = 0; j < 4; ++j) s1[t2][j] = s2[t2][j] = 0.f;
    f32x4 acc[4][NT];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int t2 = 0; t2 < NT; ++t2) acc[m][t2] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-lane halo read offsets: row 4 * wid + hr, column r + dx, 16-B chunk ks * 4 + q (swizzled by the column)
    int aoff[2][3];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
            aoff[ks][dx] = (((4 * wid) * TL_HW + r + dx) * 8 + ((ks * 4 + q) ^ (((r + dx) >> 1) & 7))) * 16;

    const bool want_stats = a.stat_acc != nullptr;
    int buf = 0;
    bool stored = false;                               // a tile's output stores have been issued
    while (cur.tile < tile_end) {
        // ---- step (cur.tile, cur.c) has landed: all but the requests of the steps ahead and the stores behind its own request
        {
            const int ny = inflight - 1;
            const bool st = stored && cur.c < nbuf;
            if (ny == 0) { if (st) TL_WAIT(4 * NT); else TL_WAIT(0); }
            else { if (st) TL_WAIT(TL_NI + 4 * NT); else TL_WAIT(TL_NI); }
            --inflight;
        }
        __builtin_amdgcn_s_barrier();
        const char* hb = halo0 + buf * TL_PART;
        {
            // the (32-channel chunk, column shift) stages of the part, software-pipelined over two fragment sets as k_conv_res<.., PIPE>
            bf16x8 ab[2][6], wb[2][3][NT];
            const char* const fb0 = filt + (cur.c * 2) * (9 * NT * 1024) + lane * 16;
#define TL_LOAD_STAGE(S_, B_)                                                                                         \
            do {                                                                                                      \
                constexpr int ks_ = (S_) / 3, dx_ = (S_) % 3;                                                         \
                _Pragma("unroll") for (int hr = 0; hr < 6; ++hr)                                                      \
                    ab[B_][hr] = *reinterpret_cast<const bf16x8*>(hb + aoff[ks_][dx_] + hr * (TL_HW * 128));          \
                _Pragma("unroll") for (int dy = 0; dy < 3; ++dy)                                                      \
                    _Pragma("unroll") for (int t2 = 0; t2 < NT; ++t2)                                                 \
                        wb[B_][dy][t2] = *reinterpret_cast<const bf16x8*>(fb0 + ks_ * (9 * NT * 1024) + a.tix[dy][dx_] * (NT * 1024) + t2 * 1024); \
            } while (0)
#define TL_MMA_STAGE(B_)                                                                                              \
            do {                                                                                                      \
                _Pragma("unroll") for (int dy = 0; dy < 3; ++dy)                                                      \
                    _Pragma("unroll") for (int t2 = 0; t2 < NT; ++t2)                                                 \
                        _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                 \
                            acc[m][t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[B_][dy][t2], ab[B_][m + dy], acc[m][t2], 0, 0, 0); \
            } while (0)
            TL_LOAD_STAGE(0, 0);
            TL_LOAD_STAGE(1, 1); __builtin_amdgcn_sched_barrier(0);
            TL_MMA_STAGE(0);
            TL_LOAD_STAGE(2, 0); __builtin_amdgcn_sched_barrier(0);
            TL_MMA_STAGE(1);
            TL_LOAD_STAGE(3, 1); __builtin_amdgcn_sched_barrier(0);
            TL_MMA_STAGE(0);
            TL_LOAD_STAGE(4, 0); __builtin_amdgcn_sched_barrier(0);
            TL_MMA_STAGE(1);
            TL_LOAD_STAGE(5, 1); __builtin_amdgcn_sched_barrier(0);
            TL_MMA_STAGE(0);
            TL_MMA_STAGE(1);
#undef TL_LOAD_STAGE
#undef TL_MMA_STAGE
        }
        barrier_lds();                                 // every wave's reads of this buffer have returned: it may be refilled
        if (rq.tile < tile_end) { TL_REQ(rq, buf); TL_ADV(rq); ++inflight; }
        if (cur.c == nparts - 1) {
            // ---- epilogue of this tile: lane (q, r) holds channels 4q .. 4q + 3 of n-tile t2 at row 4 * wid + m, column r.
            //      Exactly 4 * NT store instructions per wave (the counted waits above rely on it).
            const int mx = cur.x * 16 + r;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int my = cur.y * 16 + wid * 4 + m;
                const bool inside = my < a.g.hm && mx < a.g.wm;
                const unsigned obyte = (unsigned)(((((int64_t)cur.n * a.g.ho + my) * a.g.wo + mx) * a.g.ldo + slice * NT * 16 + 4 * q) * 2);
#pragma unroll
                for (int t2 = 0; t2 < NT; ++t2) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = acc[m][t2][j] + bv[t2][j];
                    acc[m][t2] = f32x4{0.f, 0.f, 0.f, 0.f};
                    u32x2 pk;
                    pk[0] = pack_bf16x2(v[0], v[1]);
                    pk[1] = pack_bf16x2(v[2], v[3]);
                    __builtin_amdgcn_raw_buffer_store_b64(pk, ors, inside ? (int)(obyte + t2 * 32) : (int)0x80000000u, 0, 0);
                    if (want_stats && inside) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float rv = round_as<bf16>(v[j]);
                            s1[t2][j] += rv;
                            s2[t2][j] += rv * rv;
                        }
                    }
                }
            }
            stored = true;
        }
        TL_ADV(cur);
        buf = buf + 1 == nbuf ? 0 : buf + 1;
    }
#undef TL_ADV
#undef TL_REQ

    // ---- fused per-channel sums: one atomic add per (channel, sum) and block; slices cover disjoint channel ranges
    if (a.stat_acc) {
        float* red = reinterpret_cast<float*>(smem);     // [4 waves][NT][4 q][4 j][2]  (the filter is dead by now)
        __syncthreads();
#pragma unroll
        for (int t2 = 0; t2 < NT; ++t2)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = s1[t2][j], y = s2[t2][j];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { x += __shfl_xor(x, o, 64); y += __shfl_xor(y, o, 64); }
                if (r == 0) {
                    red[(((wid * NT + t2) * 4 + q) * 4 + j) * 2] = x;
                    red[(((wid * NT + t2) * 4 + q) * 4 + j) * 2 + 1] = y;
                }
            }
        __syncthreads();
        for (int i = tid; i < NT * 16 * 2; i += 256) {
            const int which = i / (NT * 16), c = i - which * NT * 16;
            const int t2 = c >> 4, qq = (c >> 2) & 3, j = c & 3;
            float acc_ = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) acc_ += red[(((w * NT + t2) * 4 + qq) * 4 + j) * 2 + which];
            const int chn = slice * NT * 16 + c - a.stat_c0;
            if (chn >= 0 && chn < a.cpad) bn_acc_add(a.stat_acc, bl, a.groups, a.cpad, grp, which, chn, acc_, which ? a.s2_scale : a.s1_scale);
        }
    }
}

ConvTilePlan conv_tile_plan(const stcd_conv_geom& g, const ConvMfmaPlan& p, int groups) {
    ConvTilePlan tp;
    if (!p.ok || p.modeB || p.CiB != 64 || g.ntaps != 9 || g.in_stride != 1 || g.out_stride != 1 || g.oy0 != 0 || g.ox0 != 0) return tp;
    if (g.ci % 64 != 0 || g.co % 16 != 0 || g.ldi % 8 != 0 || g.ldo % 4 != 0 || g.hm > g.hi || g.wm > g.wi) return tp;
    if (g.hm > g.ho || g.wm > g.wo) return tp;
    if (g.hi >= 16384 || g.wi >= 16384) return tp;                                        // packed halo coordinates
    if (groups < 1 || g.n % groups != 0) return tp;
    if (((int64_t)g.n * g.hi + 2) * g.wi * g.ldi * 2 >= ((int64_t)1 << 31)) return tp;     // 32-bit buffer offsets, X
    if ((int64_t)g.n * g.ho * g.wo * g.ldo * 2 >= ((int64_t)1 << 31)) return tp;           // ... and the output stores
    if ((int64_t)p.wf_elems * 2 >= ((int64_t)1 << 31)) return tp;
    bool seen[9] = {false};
    for (int t = 0; t < 9; ++t) {
        if (g.dy[t] < -1 || g.dy[t] > 1 || g.dx[t] < -1 || g.dx[t] > 1) return tp;
        seen[(g.dy[t] + 1) * 3 + g.dx[t] + 1] = true;
    }
    for (int t = 0; t < 9; ++t) if (!seen[t]) return tp;
    const int nparts = g.ci / 64, nbuf = std::min(nparts, 2), ntr = g.co / 16, cap = 160 * 1024 - 1024;
    auto lds_of = [&](int nt) { return nparts * 2 * 9 * nt * 1024 + nbuf * TL_PART; };
    // widest output-channel slice beside the part buffers; where two blocks per CU fit with half of it (Ci = 64), those: one block's
    // requests then fly under the other's MFMAs
    int NT = 0;
    for (int nt = 4; nt >= 1 && !NT; nt >>= 1)
        if (ntr % nt == 0 && lds_of(nt) <= cap) NT = nt;
    if (!NT) return tp;
    if (NT == 4 && 2 * lds_of(2) <= cap) NT = 2;
    const int64_t tiles_x = (g.wm + 15) / 16, tiles_y = (g.hm + 15) / 16, ntiles = (int64_t)g.n * tiles_x * tiles_y;
    if (ntiles >= ((int64_t)1 << 24)) return tp;
    // fewer (tile, slice) pairs than CUs: narrower slices, until every CU has a block
    while (NT > 1 && ntiles * (ntr / NT) < 256) NT >>= 1;
    tp.NT = NT; tp.nparts = nparts; tp.nbuf = nbuf; tp.nslices = ntr / NT;
    tp.filt_bytes = nparts * 2 * 9 * NT * 1024;
    tp.lds_bytes = lds_of(NT);
    tp.ntiles = (int)ntiles;
    const int64_t tpg = ntiles / groups;
    const int per_cu = std::max(1, std::min(2, cap / tp.lds_bytes));
    const int64_t slots = (int64_t)per_cu * 256;
    const int64_t P = std::max<int64_t>(1, slots / ((int64_t)groups * tp.nslices));
    tp.P = (int)std::min<int64_t>(P, tpg);
    tp.blocks = tp.P * tp.nslices * groups;
    tp.ok = true;
    return tp;
}

int launch_conv_tile(const stcd_conv_geom& g, const ConvMfmaPlan& p, const ConvTilePlan& tp, const ConvArgs& c) {
    const int groups = c.groups;
    const hipStream_t s = c.s;
    if (!tp.ok || groups < 1 || tp.blocks != tp.P * tp.nslices * groups) return 1;
    ConvTileArgs a;
    a.g = g;
    a.in = (const bf16*)c.in; a.wf = (const bf16*)c.wf; a.bias = c.bias; a.out = (bf16*)c.out;
    a.NTtot = p.NTtot; a.nparts = tp.nparts; a.nbuf = tp.nbuf;
    a.nslices = tp.nslices; a.P = tp.P; a.groups = groups;
    a.tiles_x = (g.wm + 15) / 16; a.tiles_y = (g.hm + 15) / 16; a.ntiles = g.n * a.tiles_x * a.tiles_y;
    a.filt_bytes = tp.filt_bytes;
    a.stat_acc = c.sums.acc; a.cpad = c.sums.C; a.stat_c0 = c.sums.c0; a.s1_scale = c.sums.s1; a.s2_scale = c.sums.s2;
    a.in_bytes = (unsigned)((int64_t)g.n * g.hi * g.wi * g.ldi * 2);
    a.wf_bytes = (unsigned)(p.wf_elems * 2);
    a.out_bytes = (unsigned)((int64_t)g.n * g.ho * g.wo * g.ldo * 2);
    for (int t = 0; t < 9; ++t) a.tix[g.dy[t] + 1][g.dx[t] + 1] = (int8_t)t;
#define LAUNCH_TILE(N_)                                                                                           \
    do {                                                                                                          \
        static bool attr_set = false;                                                                             \
        if (!attr_set) {                                                                                          \
            (void)hipFuncSetAttribute((const void*)k_conv_tile<N_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
            attr_set = true;                                                                                      \
        }                                                                                                         \
        k_conv_tile<N_><<<(unsigned)tp.blocks, 256, (size_t)tp.lds_bytes, s>>>(a);                                \
    } while (0)
    switch (tp.NT) {
        case 1: LAUNCH_TILE(1); break;
        case 2: LAUNCH_TILE(2); break;
        default: LAUNCH_TILE(4); break;
    }
#undef LAUNCH_TILE
    return 0;
}

}  // namespace stcd
