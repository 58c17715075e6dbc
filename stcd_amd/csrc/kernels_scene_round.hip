// kernels_scene_round.hip -- the self-training round on whole scenes: per-cell agreement counts and the closing of the pseudo-label (gfx950).
//
// What this replaces in the reference (semantics, not code):
//   metric.addBatch(preds[i], preds[-1]) per pre-cut 256 x 256 crop and checkpoint      train_stcd.py:118-125
//   cv2.morphologyEx(pred, cv2.MORPH_CLOSE, np.ones((5, 5))) of the pseudo-label        train_stcd.py:186-188
// Both kernels read and write bytes and integer counts only: no float arithmetic, no float atomics, so every output is a pure
// function of the inputs.  Pixel offsets are 64-bit (height * width may pass 2^31).
//
// k_scene_cell_agree.  The scene is cut into non-overlapping cell x cell squares (edge cells are cut off at the border); a work item
// is (cell, segment of its rows), so a 256-pixel cell gives four blocks and a 4096^2 scene 1024.  A block of 256 threads is laid out
// as TY rows x TX columns (TX a power of two the launcher picks from the cell width) and walks its rows; a thread reads 16 pixels
// of every mask with one 16-byte load (VEC: width % 16 == 0, cell % 16 == 0 and every base pointer 16-byte aligned, which makes every
// row start, cell start and cell width a multiple of 16) or one pixel with a byte load otherwise (an arbitrary-width scene has
// unaligned rows and a cell boundary may fall inside a 16-byte group).  "Non-zero byte" is formed four pixels at a time in a 32-bit
// word.  Per earlier model three sums are kept (|pred_i|, |pred_i & last|, |last| once) and four for the label matrix; registers
// -> wave (shuffles) -> block (LDS) -> one 64-bit integer atomic per block and non-zero counter, as kernels_selftrain.hip does.
//   block reads : its rows of its cell in each of the n_models masks (and the label), once
//   block writes: at most 4 * (n_models - 1) + 4 atomic adds into agree[cell] / cm[cell]
//
// k_mask_close.  One launch; dilation and erosion with the (2 r + 1)^2 square are separable, and a row of 64 pixels is one 64-bit
// word of bits, so the four passes are shifts, ORs and ANDs on a bit image that never leaves the LDS.
//   block reads : the CLOSE_ROWS x 256 window of `in` around its tile: the tile and a halo of CLOSE_HALO = 8 >= 2 r pixels on
//                 every side, one byte per lane and one __ballot per 64 pixels; positions outside the scene stage as unset
//   on chip     : bit image A[CLOSE_ROWS][4] (2 KiB) and a second one B: rows dilate A -> B, columns dilate B -> A with every
//                 position outside the scene forced to SET (the erosion's border rule), rows erode A -> B, columns erode B -> A.
//                 Each pass is wrong within r of the window's border (the window's outside reads as unset in the dilation and
//                 set in the erosion, which is not the scene's rule); after four passes the error has travelled 2 r <= 8 pixels,
//                 so the tile is exact
//   block writes: its CLOSE_TH x CLOSE_TW = 48 x 240 tile of `out` inside the scene, one byte per lane; nothing else
// The window is read 1.42 x per output pixel (neighbouring blocks share halo rows through L2); byte loads and stores keep the kernel
// free of any alignment requirement on `in`, `out` and the width.
#include <algorithm>

#include "common.h"

namespace stcd {

// ------------------------------------------------------------------------------------------------ per-cell agreement
#define CELL_MAX_BLOCKS 65536      // grid-stride over the work items above this: 256 blocks per CU
#define CELL_COUNTERS (2 * (STCD_SELFTRAIN_MAX_MODELS - 1) + 2 + 4)
// counter slots: [2 i] = |pred_i|, [2 i + 1] = |pred_i & last| for the earlier models i, then |last|, the pixel count, and for the
// label matrix: non-ignored pixels, |label|, |last| and |label & last| among those
enum { CA_LAST = 2 * (STCD_SELFTRAIN_MAX_MODELS - 1), CA_PIX = CA_LAST + 1, CA_CM = CA_LAST + 2 };

__device__ __forceinline__ unsigned long long ca_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// bit 7 of every non-zero byte of w
__device__ __forceinline__ uint32_t ca_nonzero(uint32_t w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }

template <bool VEC>
__global__ void __launch_bounds__(256)
k_scene_cell_agree(SceneMaskPtrs mk, int nm, int H, int W, int cell, int cells_x, int64_t cells, int segs, int seg_rows, int txlog,
                   const uint8_t* __restrict__ label, unsigned long long* __restrict__ agree, unsigned long long* __restrict__ cm) {
    constexpr int MAXM = STCD_SELFTRAIN_MAX_MODELS;
    constexpr int UNIT = VEC ? 16 : 1;                                 // pixels a thread takes per step
    constexpr int NW = VEC ? 4 : 1;                                    // ... in 32-bit words of four bytes (scalar: the low byte of one)
    constexpr uint32_t SEEN = VEC ? 0x80808080u : 0x80u;
    __shared__ unsigned long long part[4][CELL_COUNTERS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = threadIdx.x & ((1 << txlog) - 1), ty = threadIdx.x >> txlog, TX = 1 << txlog, TY = 256 >> txlog;
    const int64_t items = cells * segs;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {       // uniform over the block: the barriers below are safe
        const int64_t c = it / segs;
        const int seg = (int)(it - c * segs);
        const int cy = (int)(c / cells_x), cx = (int)(c - (int64_t)cy * cells_x);
        const int64_t x0 = (int64_t)cx * cell, y0 = (int64_t)cy * cell + (int64_t)seg * seg_rows;
        const int cw = (int)std::min<int64_t>(cell, W - x0);           // >= 1: cells_x == ceil(W / cell)
        const int64_t y1 = std::min<int64_t>(std::min<int64_t>(y0 + seg_rows, ((int64_t)cy + 1) * cell), H);
        unsigned int np[MAXM - 1], nb[MAXM - 1], nlast = 0, npix = 0, lv = 0, ll = 0, lp = 0, lb = 0;
#pragma unroll
        for (int i = 0; i < MAXM - 1; ++i) np[i] = nb[i] = 0;
        for (int64_t y = y0 + ty; y < y1; y += TY) {
            const int64_t row = y * W + x0;
            for (int u = tx * UNIT; u < cw; u += TX * UNIT) {          // VEC: cw % 16 == 0, the 16 bytes lie inside the cell
                uint32_t pred[MAXM][NW], last[NW] = {};
#pragma unroll
                for (int k = 0; k < MAXM; ++k) {
                    if (k >= nm) continue;                             // nm is uniform
                    const uint8_t* q = mk.p[k] + row + u;
                    if constexpr (VEC) {
                        const uint4 a = *reinterpret_cast<const uint4*>(q);
                        pred[k][0] = ca_nonzero(a.x); pred[k][1] = ca_nonzero(a.y); pred[k][2] = ca_nonzero(a.z); pred[k][3] = ca_nonzero(a.w);
                    } else {
                        pred[k][0] = *q ? 0x80u : 0u;
                    }
                    if (k == nm - 1) {                                 // no run-time index into the register array
#pragma unroll
                        for (int j = 0; j < NW; ++j) last[j] = pred[k][j];
                    }
                }
#pragma unroll
                for (int j = 0; j < NW; ++j) {
#pragma unroll
                    for (int i = 0; i < MAXM - 1; ++i) {
                        if (i >= nm - 1) continue;
                        np[i] += __popc(pred[i][j]);
                        nb[i] += __popc(pred[i][j] & last[j]);
                    }
                    nlast += __popc(last[j]);
                }
                npix += UNIT;
                if (label) {
                    uint32_t lw[NW];
                    if constexpr (VEC) {
                        const uint4 a = *reinterpret_cast<const uint4*>(label + row + u);
                        lw[0] = a.x; lw[1] = a.y; lw[2] = a.z; lw[3] = a.w;
                    } else {
                        lw[0] = label[row + u];                        // only the low byte is looked at (SEEN)
                    }
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        const uint32_t valid = ca_nonzero(~lw[j]) & SEEN;                  // a byte of 255 is ignored
                        const uint32_t lab = ca_nonzero(lw[j]) & valid, pr = last[j] & valid;
                        lv += __popc(valid); ll += __popc(lab); lp += __popc(pr); lb += __popc(lab & pr);
                    }
                }
            }
        }
        // this work item's counts: wave sums, then the block's through LDS
#pragma unroll
        for (int i = 0; i < MAXM - 1; ++i) {
            if (i >= nm - 1) continue;
            const unsigned long long a = ca_wave_sum(np[i]), b = ca_wave_sum(nb[i]);
            if (lane == 0) { part[wave][2 * i] = a; part[wave][2 * i + 1] = b; }
        }
        {
            const unsigned long long a = ca_wave_sum(nlast), b = ca_wave_sum(npix);
            if (lane == 0) { part[wave][CA_LAST] = a; part[wave][CA_PIX] = b; }
        }
        if (label) {                                                   // uniform
            const unsigned long long a = ca_wave_sum(lv), b = ca_wave_sum(ll), d = ca_wave_sum(lp), e = ca_wave_sum(lb);
            if (lane == 0) { part[wave][CA_CM] = a; part[wave][CA_CM + 1] = b; part[wave][CA_CM + 2] = d; part[wave][CA_CM + 3] = e; }
        }
        __syncthreads();
        if ((int)threadIdx.x < nm - 1) {
            const int i = threadIdx.x;
            unsigned long long P = 0, B = 0, L = 0, N = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { P += part[w][2 * i]; B += part[w][2 * i + 1]; L += part[w][CA_LAST]; N += part[w][CA_PIX]; }
            unsigned long long* a = agree + (c * (nm - 1) + i) * 4;    // a[2 * last + pred_i]
            const unsigned long long c00 = N - P - L + B, c01 = P - B, c10 = L - B;
            if (c00) atomicAdd(a + 0, c00);
            if (c01) atomicAdd(a + 1, c01);
            if (c10) atomicAdd(a + 2, c10);
            if (B) atomicAdd(a + 3, B);
        }
        if (label && threadIdx.x == 64) {                              // another wave than the agreement's
            unsigned long long V = 0, L = 0, P = 0, B = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { V += part[w][CA_CM]; L += part[w][CA_CM + 1]; P += part[w][CA_CM + 2]; B += part[w][CA_CM + 3]; }
            unsigned long long* a = cm + c * 4;                        // a[2 * label + pred_last]
            const unsigned long long c00 = V - L - P + B, c01 = P - B, c10 = L - B;
            if (c00) atomicAdd(a + 0, c00);
            if (c01) atomicAdd(a + 1, c01);
            if (c10) atomicAdd(a + 2, c10);
            if (B) atomicAdd(a + 3, B);
        }
        __syncthreads();                                               // part is written again for the block's next work item
    }
}

static inline bool sr_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

void launch_scene_cell_agree(const SceneMaskPtrs& mk, int n_models, int height, int width, int cell, int cells_x, int cells_y,
                             const uint8_t* label, int64_t* agree, int64_t* cm, hipStream_t s) {
    if (height == 0 || width == 0) return;
    bool vec = width % 16 == 0 && cell % 16 == 0 && (!label || sr_aligned(label, 16));
    for (int k = 0; k < n_models; ++k) vec = vec && sr_aligned(mk.p[k], 16);
    // a block takes about 16 Ki pixels of a cell: a thread counts in 32 bits and a 256-pixel cell still gives four blocks
    const int cw = std::min(cell, width), ch = std::min(cell, height);
    const int seg_rows = std::max(1, std::min(ch, 16384 / cw));
    const int segs = (ch + seg_rows - 1) / seg_rows;
    const int units = vec ? cw / 16 : cw;                              // steps a row of a full cell takes with one thread per step
    int txlog = 0;
    while (txlog < 8 && (1 << txlog) < units) ++txlog;
    const int64_t cells = (int64_t)cells_x * cells_y;
    const unsigned grid = (unsigned)std::min<int64_t>(cells * segs, CELL_MAX_BLOCKS);
    unsigned long long* ag = (unsigned long long*)agree;
    unsigned long long* cmu = (unsigned long long*)cm;
    if (vec) k_scene_cell_agree<true><<<grid, 256, 0, s>>>(mk, n_models, height, width, cell, cells_x, cells, segs, seg_rows, txlog, label, ag, cmu);
    else     k_scene_cell_agree<false><<<grid, 256, 0, s>>>(mk, n_models, height, width, cell, cells_x, cells, segs, seg_rows, txlog, label, ag, cmu);
}

// ------------------------------------------------------------------------------------------------ binary closing
#define CLOSE_ROWS 64                          // staged rows
#define CLOSE_WORDS 4                          // staged columns / 64
#define CLOSE_HALO 8                           // >= 2 * radius for radius <= 4
#define CLOSE_TH (CLOSE_ROWS - 2 * CLOSE_HALO)
#define CLOSE_TW (64 * CLOSE_WORDS - 2 * CLOSE_HALO)

int64_t mask_close_tiles(int height, int width) {
    return (((int64_t)height + CLOSE_TH - 1) / CLOSE_TH) * (((int64_t)width + CLOSE_TW - 1) / CLOSE_TW);
}

// the word of row `r` at word column `c` of a bit image, `fill` outside the window
__device__ __forceinline__ unsigned long long cl_word(const unsigned long long (*img)[CLOSE_WORDS], int r, int c, unsigned long long fill) {
    return (r >= 0 && r < CLOSE_ROWS && c >= 0 && c < CLOSE_WORDS) ? img[r][c] : fill;
}

__global__ void __launch_bounds__(256)
k_mask_close(const uint8_t* __restrict__ in, int H, int W, int radius, uint32_t mask_value, int tiles_x, uint8_t* __restrict__ out) {
    __shared__ unsigned long long A[CLOSE_ROWS][CLOSE_WORDS], B[CLOSE_ROWS][CLOSE_WORDS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int64_t gy0 = (int64_t)by * CLOSE_TH - CLOSE_HALO, gx0 = (int64_t)bx * CLOSE_TW - CLOSE_HALO;       // the window's origin in the scene
    // stage: bit (r, 64 c + lane) of A = pixel (gy0 + r, gx0 + 64 c + lane) is non-zero; outside the scene: unset
    for (int r = wave; r < CLOSE_ROWS; r += 4) {
        const int64_t gy = gy0 + r;
        const bool row_in = gy >= 0 && gy < H;                         // uniform over the wave
#pragma unroll
        for (int c = 0; c < CLOSE_WORDS; ++c) {
            const int64_t gx = gx0 + 64 * c + lane;
            const bool set = row_in && gx >= 0 && gx < W && in[gy * W + gx] != 0;
            const unsigned long long word = __ballot(set);
            if (lane == 0) A[r][c] = word;
        }
    }
    __syncthreads();
    const int r = threadIdx.x >> 2, c = threadIdx.x & 3;               // one word per thread: CLOSE_ROWS * CLOSE_WORDS == 256
    {                                                                  // rows, dilate: A -> B (bit j of a word is column j: << moves right)
        const unsigned long long x = A[r][c], xl = cl_word(A, r, c - 1, 0), xr = cl_word(A, r, c + 1, 0);
        unsigned long long d = x;
        for (int s = 1; s <= radius; ++s) d |= (x << s) | (xl >> (64 - s)) | (x >> s) | (xr << (64 - s));
        B[r][c] = d;
    }
    __syncthreads();
    {                                                                  // columns, dilate: B -> A, then the outside of the scene reads as set
        unsigned long long d = B[r][c];
        for (int s = 1; s <= radius; ++s) d |= cl_word(B, r - s, c, 0) | cl_word(B, r + s, c, 0);
        const int64_t gy = gy0 + r, gx = gx0 + 64 * c;                 // columns gx .. gx + 63
        unsigned long long outside = 0;
        if (gy < 0 || gy >= H) outside = ~0ull;
        else {
            if (gx < 0) outside |= gx <= -64 ? ~0ull : (1ull << (int)(-gx)) - 1ull;
            if (gx + 63 >= W) outside |= gx >= W ? ~0ull : ~((1ull << (int)(W - gx)) - 1ull);
        }
        A[r][c] = d | outside;
    }
    __syncthreads();
    {                                                                  // rows, erode: A -> B
        const unsigned long long x = A[r][c], xl = cl_word(A, r, c - 1, ~0ull), xr = cl_word(A, r, c + 1, ~0ull);
        unsigned long long e = x;
        for (int s = 1; s <= radius; ++s) e &= ((x << s) | (xl >> (64 - s))) & ((x >> s) | (xr << (64 - s)));
        B[r][c] = e;
    }
    __syncthreads();
    {                                                                  // columns, erode: B -> A
        unsigned long long e = B[r][c];
        for (int s = 1; s <= radius; ++s) e &= cl_word(B, r - s, c, ~0ull) & cl_word(B, r + s, c, ~0ull);
        A[r][c] = e;                                                   // A was last read before the previous barrier
    }
    __syncthreads();
    // write the tile: rows and columns CLOSE_HALO .. window - CLOSE_HALO of the window, inside the scene
    for (int rr = CLOSE_HALO + wave; rr < CLOSE_ROWS - CLOSE_HALO; rr += 4) {
        const int64_t gy = gy0 + rr;
        if (gy >= H) break;                                            // uniform over the wave; gy >= 0 for a tile row
#pragma unroll
        for (int cc = 0; cc < CLOSE_WORDS; ++cc) {
            const int col = 64 * cc + lane;
            const int64_t gx = gx0 + col;
            if (col >= CLOSE_HALO && col < 64 * CLOSE_WORDS - CLOSE_HALO && gx < W)
                out[gy * W + gx] = (uint8_t)(((A[rr][cc] >> lane) & 1ull) * mask_value);
        }
    }
}

void launch_mask_close(const uint8_t* in, int height, int width, int radius, int mask_value, uint8_t* out, hipStream_t s) {
    if (height == 0 || width == 0) return;
    const int tiles_x = (width + CLOSE_TW - 1) / CLOSE_TW;
    k_mask_close<<<(unsigned)mask_close_tiles(height, width), 256, 0, s>>>(in, height, width, radius, (uint32_t)mask_value, tiles_x, out);
}

}  // namespace stcd
