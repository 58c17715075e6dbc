// ops_abi.hip -- per-op C-ABI entry points of the normalisation / pooling / fusion kernels and every stcd_scene_* entry
// (include/stcd_hip.h).
//
// These run EXACTLY the launch sequences the engine runs for one layer (statistics -> finalize -> apply, ...), on
// caller-provided NHWC tensors, so the parity tests can pin every elementwise kernel against the reference's per-op
// vectors (tests/golden/g1_ops.npz) and the plain-C oracle at per-op tolerance.  Reference semantics:
//   BatchNorm2d + ReLU + Dropout2d   /root/reference/models/SiamUnet_diff.py:19-20, applied :99
//   F.max_pool2d(2,2)                /root/reference/models/SiamUnet_diff.py:101
//   |T1-T2| / T2-T1 skip fusion      SiamUnet_diff.py:150 / SiamUnet_sub.py:150
//   ReplicationPad2d                 SiamUnet_diff.py:149
#include <algorithm>

#include "common.h"

using namespace stcd;

namespace {

int check_map(const stcd_map_geom* g) {
    STCD_CHECK(g != nullptr, "geometry is null");
    STCD_CHECK(g->n >= 1 && g->h >= 1 && g->w >= 1, "bad sizes");
    STCD_CHECK(g->c >= 8 && g->c % 8 == 0 && g->c <= 2048 && (g->c & (g->c - 1)) == 0, "channels must be a power of two in [8, 2048]");
    STCD_CHECK(g->groups >= 1 && g->groups <= 2 && g->n % g->groups == 0, "groups must be 1 or 2 and divide n");
    STCD_CHECK((int64_t)g->n * g->h * g->w * (g->c / 8) < ((int64_t)1 << 31), "tensor too large for 32-bit indexing");
    return 0;
}

int64_t acc_bytes(const stcd_map_geom& g) { return bn_acc_bytes(g.groups, g.c); }

}  // namespace

extern "C" {

int64_t stcd_op_ew_scratch_bytes(const stcd_map_geom* g) {
    if (!g || g->c < 8 || g->groups < 1) return 0;
    return acc_bytes(*g) + 256;
}

int stcd_op_bn_act(int dtype, const stcd_map_geom* g, const void* y, int ldy, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, const float* mask, int relu, int training, void* a, int lda,
                   void* pool, int ldp, float* stat, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(dtype == STCD_DTYPE_F32 || dtype == STCD_DTYPE_BF16, "unknown dtype");
    STCD_CHECK(y && gamma && beta && running_mean && running_var && a && stat && scratch, "null pointer argument");
    STCD_CHECK(ldy >= g->c && lda >= g->c && ldy % 8 == 0 && lda % 8 == 0 && (!pool || (ldp >= g->c && ldp % 8 == 0)), "bad pixel stride");
    STCD_CHECK(scratch_bytes >= stcd_op_ew_scratch_bytes(g), "scratch too small");
    hipStream_t s = (hipStream_t)hip_stream;
    const int npg = g->n / g->groups;
    const int64_t ppg = (int64_t)npg * g->h * g->w;
    long long* acc = (long long*)scratch;
    BnActArgs aa;
    if (training) {
        STCD_HIP(hipMemsetAsync(acc, 0, (size_t)acc_bytes(*g), s));
        launch_bn_stats(dtype, y, ldy, g->c, g->groups, ppg, acc, s);
        aa.facc = acc; aa.gamma = gamma; aa.beta = beta; aa.running_mean = running_mean; aa.running_var = running_var;
    } else {
        launch_bn_eval_prepare(g->c, g->groups, gamma, beta, running_mean, running_var, stat, 1e-5f, s);
    }
    aa.Y = y; aa.ldy = ldy; aa.A = a; aa.lda = lda; aa.a_group_off = ppg * lda;
    aa.P = pool; aa.ldp = ldp; aa.stat = stat; aa.mask = mask;
    aa.C = g->c; aa.groups = g->groups; aa.npg = npg; aa.H = g->h; aa.W = g->w; aa.relu = relu ? 1 : 0;
    launch_bn_act(dtype, aa, s);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_bn_act_pair(int dtype, const stcd_map_geom* g, const void* y, int ldy, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, const float* mask, int fuse_mode, void* a, int lda, void* pool,
                        int ldp, void* fused, int ldf, float* stat, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(dtype == STCD_DTYPE_F32 || dtype == STCD_DTYPE_BF16, "unknown dtype");
    STCD_CHECK(g->groups == 2, "the pair kernel handles the two dates of a pair: groups must be 2");
    STCD_CHECK(y && gamma && beta && running_mean && running_var && fused && stat && scratch, "null pointer argument");
    STCD_CHECK(fuse_mode == 0 || fuse_mode == 1, "fuse_mode must be 0 (|a1-a2|) or 1 (a2-a1)");
    STCD_CHECK(scratch_bytes >= stcd_op_ew_scratch_bytes(g), "scratch too small");
    hipStream_t s = (hipStream_t)hip_stream;
    const int npg = g->n / 2;
    const int64_t ppg = (int64_t)npg * g->h * g->w;
    long long* acc = (long long*)scratch;
    STCD_HIP(hipMemsetAsync(acc, 0, (size_t)acc_bytes(*g), s));
    launch_bn_stats(dtype, y, ldy, g->c, 2, ppg, acc, s);
    BnActArgs aa;
    aa.facc = acc; aa.gamma = gamma; aa.beta = beta; aa.running_mean = running_mean; aa.running_var = running_var;
    aa.Y = y; aa.ldy = ldy; aa.A = a; aa.lda = lda; aa.a_group_off = ppg * lda;
    aa.P = pool; aa.ldp = ldp; aa.stat = stat; aa.mask = mask;
    aa.C = g->c; aa.groups = 2; aa.npg = npg; aa.H = g->h; aa.W = g->w; aa.relu = 1;
    launch_bn_act_pair(dtype, aa, fused, ldf, fuse_mode, s);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_bn_act_bwd(int dtype, const stcd_map_geom* g, const void* da, int ldda, const void* y, int ldy, const float* stat,
                       const float* mask, int relu, void* dy, int lddy, float* dgamma, float* dbeta, void* scratch,
                       int64_t scratch_bytes, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(dtype == STCD_DTYPE_F32 || dtype == STCD_DTYPE_BF16, "unknown dtype");
    STCD_CHECK(da && y && stat && dy && dgamma && dbeta && scratch, "null pointer argument");
    STCD_CHECK(scratch_bytes >= stcd_op_ew_scratch_bytes(g), "scratch too small");
    hipStream_t s = (hipStream_t)hip_stream;
    const int npg = g->n / g->groups;
    const int64_t HW = (int64_t)g->h * g->w, ppg = npg * HW;
    long long* acc = (long long*)scratch;
    STCD_HIP(hipMemsetAsync(acc, 0, (size_t)acc_bytes(*g), s));
    launch_bn_bwd_reduce(dtype, da, ldda, ppg * ldda, y, ldy, stat, mask, g->c, g->groups, npg, HW, relu ? 1 : 0, acc, s);
    launch_bn_bwd_apply(dtype, da, ldda, ppg * ldda, dy, lddy, y, ldy, stat, acc, dgamma, dbeta, mask, g->c, g->groups, npg, HW,
                        relu ? 1 : 0, s);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_maxpool(int dtype, const stcd_map_geom* g, const void* a, int lda, void* pool, int ldp, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(a && pool, "null pointer argument");
    launch_maxpool(dtype, a, lda, pool, ldp, g->n, g->h, g->w, g->c, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_maxpool_bwd(int dtype, const stcd_map_geom* g, const void* a, int lda, const void* dpool, int ldp, void* da, int ldda,
                        int accumulate, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(a && dpool && da, "null pointer argument");
    const int npg = g->n / g->groups;
    const int64_t ppg = (int64_t)npg * g->h * g->w;
    launch_pool_bwd(dtype, a, lda, ppg * lda, dpool, ldp, da, ldda, ppg * ldda, g->groups, npg, g->h, g->w, g->c, accumulate ? 1 : 0,
                    (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

/* 3x3 stride-2 padding-1 max-pool of the ResNet stem (F.max_pool2d(x, 3, 2, 1), models/resnet.py:176) and its gradient through the
 * recorded winners.  g: the INPUT map (h, w even); pool / dpool: [n, h/2, w/2, c]; idx: n*(h/2)*(w/2)*c bytes. */
int stcd_op_maxpool3(int dtype, const stcd_map_geom* g, const void* a, int lda, void* pool, int ldp, void* idx, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(a && pool && g->h % 2 == 0 && g->w % 2 == 0, "null pointer argument or odd size");
    launch_maxpool3(dtype, a, lda, pool, ldp, g->n, g->h, g->w, g->c, (hipStream_t)hip_stream, (unsigned char*)idx);
    STCD_HIP(hipGetLastError());
    return 0;
}
int stcd_op_maxpool3_bwd(int dtype, const stcd_map_geom* g, const void* idx, const void* dpool, int ldp, void* da, int ldda, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(idx && dpool && da && g->h % 2 == 0 && g->w % 2 == 0, "null pointer argument or odd size");
    launch_maxpool3_bwd(dtype, (const unsigned char*)idx, dpool, ldp, da, ldda, g->n, g->h, g->w, g->c, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_fuse(int dtype, int mode, const stcd_map_geom* g, const void* a, int lda, void* d, int ldd, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(g->groups == 2 && (mode == 0 || mode == 1) && a && d, "bad argument (groups must be 2, mode 0 or 1)");
    const int b = g->n / 2;
    const int64_t HW = (int64_t)g->h * g->w;
    launch_fuse(dtype, mode, a, lda, (int64_t)b * HW * lda, d, ldd, b, HW, g->c, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int64_t stcd_op_pairdw_scratch_bytes(const stcd_map_geom* g) {
    if (!g || g->n < 2 || g->c < 8) return 0;
    return pairdw_partial_floats(g->n / 2, g->h, g->w, g->c) * 4 + 256;
}
int stcd_op_pairdw(int dtype, const stcd_map_geom* g, const void* a, int lda, const float* w, const float* b, void* out, int ldo,
                   void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(g->groups == 2 && a && w && out, "bad argument (groups must be 2: the two dates stacked in the batch dimension)");
    const int n = g->n / 2;
    launch_pairdw_fwd(dtype, a, lda, (int64_t)n * g->h * g->w * lda, out, ldo, w, b, n, g->h, g->w, g->c, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}
int stcd_op_pairdw_bwd(int dtype, const stcd_map_geom* g, const void* a, int lda, const void* dout, int lddo, const float* w, void* da,
                       int ldda, float* dw, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(g->groups == 2 && a && dout && w && da && dw && scratch, "bad argument (groups must be 2)");
    STCD_CHECK(scratch_bytes >= stcd_op_pairdw_scratch_bytes(g), "scratch too small");
    const int n = g->n / 2;
    launch_pairdw_bwd_data(dtype, dout, lddo, da, ldda, (int64_t)n * g->h * g->w * ldda, w, n, g->h, g->w, g->c, (hipStream_t)hip_stream);
    launch_pairdw_bwd_filter(dtype, a, lda, (int64_t)n * g->h * g->w * lda, dout, lddo, dw, (float*)scratch, n, g->h, g->w, g->c,
                             (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_fuse_bwd(int dtype, int mode, const stcd_map_geom* g, const void* a, int lda, const void* dd, int ldd, void* da, int ldda,
                     void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(g->groups == 2 && (mode == 0 || mode == 1) && a && dd && da, "bad argument (groups must be 2, mode 0 or 1)");
    const int b = g->n / 2;
    const int64_t HW = (int64_t)g->h * g->w;
    launch_fuse_bwd(dtype, mode, a, lda, (int64_t)b * HW * lda, dd, ldd, da, ldda, (int64_t)b * HW * ldda, b, HW, g->c,
                    (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_rep_pad(int dtype, const stcd_map_geom* g, void* d, int ld, int h0, int w0, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(d && h0 >= 1 && w0 >= 1 && h0 <= g->h && w0 <= g->w, "bad argument");
    launch_rep_pad(dtype, d, ld, g->n, g->h, g->w, h0, w0, g->c, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_rep_pad_bwd(int dtype, const stcd_map_geom* g, void* dd, int ld, int h0, int w0, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(dd && h0 >= 1 && w0 >= 1 && h0 <= g->h && w0 <= g->w, "bad argument");
    launch_rep_pad_bwd(dtype, dd, ld, g->n, g->h, g->w, h0, w0, g->c, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_op_skip_bwd(int dtype, int mode, const stcd_map_geom* g, const void* a, int lda, const void* y, int ldy, const void* dd,
                     int ldd, const void* dpool, int ldp, const float* stat, const float* mask, void* da, int ldda, void* dy,
                     int lddy, float* dgamma, float* dbeta, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    if (check_map(g)) return 1;
    STCD_CHECK(g->groups == 2 && (mode == 0 || mode == 1), "groups must be 2, mode 0 or 1");
    STCD_CHECK(y && dd && dpool && stat && da && dy && dgamma && dbeta && scratch, "null pointer argument");
    STCD_CHECK(scratch_bytes >= stcd_op_ew_scratch_bytes(g), "scratch too small");
    hipStream_t s = (hipStream_t)hip_stream;
    const int b = g->n / 2;
    STCD_CHECK(a || skip_pair_supported(b, g->h, g->w, g->c), "a == NULL (recompute the activations from y): unsupported shape");
    const int64_t HW = (int64_t)g->h * g->w, ppg = b * HW;
    long long* acc = (long long*)scratch;
    STCD_HIP(hipMemsetAsync(acc, 0, (size_t)acc_bytes(*g), s));
    if (a)
        launch_skip_bwd(dtype, mode, a, lda, ppg * lda, y, ldy, dd, ldd, dpool, ldp, da, ldda, ppg * ldda, stat, mask, b, g->h, g->w,
                        g->c, acc, s);
    else        // the engine's default plan: the forward stored no activations, k_skip_bwd_pair recomputes them from y
        launch_skip_bwd_pair(dtype, mode, y, ldy, dd, ldd, dpool, ldp, da, ldda, ppg * ldda, stat, mask, b, g->h, g->w, g->c, acc, s);
    launch_bn_bwd_apply(dtype, da, ldda, ppg * ldda, dy, lddy, y, ldy, stat, acc, dgamma, dbeta, mask, g->c, 2, b, HW, 1, s);
    STCD_HIP(hipGetLastError());
    return 0;
}

// ---- whole-scene inference (kernels_scene.hip): every gather entry is scene_gather and every stitch entry scene_stitch, so each
//      check stands once and reports under the entry's name.  d4 is checked first; the entries without the argument pass 0, the
//      upright view.
// pair: two scenes into x1 and x2; otherwise scene_b and x2 are not looked at and scene_a alone goes into x1
static int scene_gather(const char* entry, bool pair, const uint8_t* scene_a, const uint8_t* scene_b, int height, int width, int tile,
                        int stride, int tiles_x, int first_tile, int n_tiles, const float* mean3, const float* std3, float* x1, float* x2,
                        int d4, void* hip_stream) {
    STCD_CHECK_AS(entry, d4 >= 0 && d4 <= 7, "d4 must be in [0, 7]");
    STCD_CHECK_AS(entry, scene_a && (!pair || (scene_b && x2)) && mean3 && std3 && x1, "null pointer argument");
    if (check_scene_grid(height, width, tile, stride, tiles_x, stride >= 1 && tile >= 1 ? scene_tiles(height, tile, stride) : 0, first_tile, n_tiles))
        return 1;
    STCD_CHECK_AS(entry, std3[0] > 0.f && std3[1] > 0.f && std3[2] > 0.f, "std must be positive");
    launch_scene_gather_d4(scene_a, pair ? scene_b : nullptr, height, width, tile, stride, tiles_x, first_tile, n_tiles, mean3, std3, x1,
                           pair ? x2 : nullptr, d4, (hipStream_t)hip_stream);
    const hipError_t err = hipGetLastError();
    STCD_CHECK_AS(entry, err == hipSuccess, std::string("hipGetLastError(): ") + hipGetErrorString(err));
    return 0;
}
// logits: host array of n_heads device pointers; the single-head entries pass the address of their one pointer, or NULL if that is NULL
static int scene_stitch(const char* entry, const float* const* logits, int n_heads, int classes, int height, int width, int tile, int stride,
                        int tiles_x, int tiles_y, int first_tile, int n_tiles, const float* window, float* acc, float* wsum, int d4,
                        void* hip_stream) {
    STCD_CHECK_AS(entry, d4 >= 0 && d4 <= 7, "d4 must be in [0, 7]");
    STCD_CHECK_AS(entry, logits && acc && wsum, "null pointer argument");
    STCD_CHECK_AS(entry, n_heads >= 1 && n_heads <= STCD_SCENE_MAX_HEADS, "n_heads must be in [1, 3]");
    SceneHeadPtrs lg{};
    for (int h = 0; h < n_heads; ++h) {
        STCD_CHECK_AS(entry, logits[h] != nullptr, "a logits pointer is null");
        lg.p[h] = logits[h];
    }
    STCD_CHECK_AS(entry, classes == 1 || classes == 2, "classes must be 1 or 2");
    if (check_scene_grid(height, width, tile, stride, tiles_x, tiles_y, first_tile, n_tiles)) return 1;
    launch_scene_stitch_heads_d4(lg, n_heads, classes, height, width, tile, stride, tiles_x, tiles_y, first_tile, n_tiles, window, acc, wsum,
                                 d4, (hipStream_t)hip_stream);
    const hipError_t err = hipGetLastError();
    STCD_CHECK_AS(entry, err == hipSuccess, std::string("hipGetLastError(): ") + hipGetErrorString(err));
    return 0;
}

int stcd_scene_gather(const uint8_t* scene_a, const uint8_t* scene_b, int height, int width, int tile, int stride, int tiles_x,
                      int first_tile, int n_tiles, const float* mean3, const float* std3, float* x1, float* x2, void* hip_stream) {
    return scene_gather(__func__, true, scene_a, scene_b, height, width, tile, stride, tiles_x, first_tile, n_tiles, mean3, std3, x1, x2, 0,
                        hip_stream);
}
int stcd_scene_gather_d4(const uint8_t* scene_a, const uint8_t* scene_b, int height, int width, int tile, int stride, int tiles_x,
                         int first_tile, int n_tiles, const float* mean3, const float* std3, float* x1, float* x2, int d4,
                         void* hip_stream) {
    return scene_gather(__func__, true, scene_a, scene_b, height, width, tile, stride, tiles_x, first_tile, n_tiles, mean3, std3, x1, x2, d4,
                        hip_stream);
}
int stcd_scene_gather_one_d4(const uint8_t* scene, int height, int width, int tile, int stride, int tiles_x, int first_tile, int n_tiles,
                             const float* mean3, const float* std3, float* x, int d4, void* hip_stream) {
    return scene_gather(__func__, false, scene, nullptr, height, width, tile, stride, tiles_x, first_tile, n_tiles, mean3, std3, x, nullptr,
                        d4, hip_stream);
}
int stcd_scene_stitch(const float* logits, int classes, int height, int width, int tile, int stride, int tiles_x, int tiles_y,
                      int first_tile, int n_tiles, const float* window, float* acc, float* wsum, void* hip_stream) {
    return scene_stitch(__func__, logits ? &logits : nullptr, 1, classes, height, width, tile, stride, tiles_x, tiles_y, first_tile, n_tiles,
                        window, acc, wsum, 0, hip_stream);
}
int stcd_scene_stitch_d4(const float* logits, int classes, int height, int width, int tile, int stride, int tiles_x, int tiles_y,
                         int first_tile, int n_tiles, const float* window, float* acc, float* wsum, int d4, void* hip_stream) {
    return scene_stitch(__func__, logits ? &logits : nullptr, 1, classes, height, width, tile, stride, tiles_x, tiles_y, first_tile, n_tiles,
                        window, acc, wsum, d4, hip_stream);
}
int stcd_scene_stitch_heads_d4(const float* const* logits, int n_heads, int classes, int height, int width, int tile, int stride, int tiles_x,
                               int tiles_y, int first_tile, int n_tiles, const float* window, float* acc, float* wsum, int d4,
                               void* hip_stream) {
    return scene_stitch(__func__, logits, n_heads, classes, height, width, tile, stride, tiles_x, tiles_y, first_tile, n_tiles, window, acc,
                        wsum, d4, hip_stream);
}
int stcd_scene_finalize(const float* acc, const float* wsum, int classes, int height, int width, float threshold, const uint8_t* label,
                        uint8_t* mask, float* prob, int64_t* cm, void* hip_stream) {
    STCD_CHECK(acc && wsum && mask, "null pointer argument");
    STCD_CHECK(classes == 1 || classes == 2, "classes must be 1 or 2");
    STCD_CHECK(height >= 1 && width >= 1, "bad shape");
    STCD_CHECK((label != nullptr) == (cm != nullptr), "label and cm go together");
    launch_scene_finalize(acc, wsum, classes, height, width, threshold, label, mask, prob, cm, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}
int stcd_scene_finalize_seg(const float* acc, const float* wsum, int classes, int height, int width, float seg_threshold,
                            float change_threshold, const uint8_t* label_a, const uint8_t* label_b, const uint8_t* label_c, uint8_t* seg_a,
                            uint8_t* seg_b, uint8_t* change, uint8_t* gated, float* prob, int64_t* cm, void* hip_stream) {
    STCD_CHECK(acc && wsum && seg_a && seg_b && change, "null pointer argument");
    STCD_CHECK(classes == 1 || classes == 2, "classes must be 1 or 2");
    STCD_CHECK(height >= 1 && width >= 1, "bad shape");
    STCD_CHECK((label_a || label_b || label_c) == (cm != nullptr), "cm goes with at least one label");
    launch_scene_finalize_seg(acc, wsum, classes, height, width, seg_threshold, change_threshold, label_a, label_b, label_c, seg_a, seg_b,
                              change, gated, prob, cm, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

// ---- the round on whole scenes (kernels_scene_round.hip)
int stcd_scene_cell_agree(const uint8_t* const* masks, int n_models, int height, int width, int cell, int cells_x, int cells_y,
                          const uint8_t* label, int64_t* agree, int64_t* cm, void* hip_stream) {
    STCD_CHECK(masks != nullptr, "null pointer argument");
    STCD_CHECK(n_models >= 1 && n_models <= STCD_SELFTRAIN_MAX_MODELS, "n_models must be in [1, 8]");
    SceneMaskPtrs mk{};
    for (int k = 0; k < n_models; ++k) {
        STCD_CHECK(masks[k] != nullptr, "a mask pointer is null");
        mk.p[k] = masks[k];
    }
    STCD_CHECK(height >= 0 && width >= 0, "bad shape");
    STCD_CHECK(cell >= 1, "cell must be >= 1");
    STCD_CHECK(cells_x == (int)(((int64_t)width + cell - 1) / cell), "cells_x is not ceil(width / cell)");
    STCD_CHECK(cells_y == (int)(((int64_t)height + cell - 1) / cell), "cells_y is not ceil(height / cell)");
    STCD_CHECK((agree == nullptr) == (n_models == 1), "agree is NULL if and only if n_models == 1");
    STCD_CHECK((label != nullptr) == (cm != nullptr), "label and cm go together");
    STCD_CHECK(n_models > 1 || label != nullptr, "one model and no label: nothing to compute");
    if (height == 0 || width == 0) return 0;
    launch_scene_cell_agree(mk, n_models, height, width, cell, cells_x, cells_y, label, agree, cm, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
