// engine.hip -- network plans, workspace layout and the C ABI (include/stcd_hip.h) of the stcd engine.
//
// The engine owns the *graph* of the FC-Siam family (and SNUNet, engine_snunet.hip): buffers are carved out of
// one caller-provided workspace at stcd_configure() time, forward/backward are straight-line launch sequences
// on the caller's stream (no allocation, no sync -> hipGraph-capturable).  Data layout in HBM:
//   activations  NHWC, bf16 (or fp32 in parity mode), T1 images then T2 images in one batch of 2B for the
//                shared encoder (BN statistics stay per date: "groups"),
//   concat       never materialised by a copy: producers write channel slices of the decoder's input buffer,
//   parameters   caller's flat fp32 buffer in the reference's layouts; repacked per call into [tap][K][N],
//   gradients    caller's flat fp32 buffer, same layout as parameters.
// Layer tables restate /root/reference/models/SiamUnet_diff.py:13-92 (+ SiamUnet_conc.py:54-87); the forward
// order follows SiamUnet_diff.py:94-181.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <array>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"

namespace stcd {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

enum ConvKind { K_CONV3 = 0, K_CONVT3_S1 = 1, K_UPCONV = 2, K_CONV1 = 3, K_CONVT2 = 4, K_CONV3_S2 = 5, K_CONV1_S2 = 6, K_STEM7 = 7 };

struct TRef { int64_t off = -1; int ld = 0; };                 // byte offset in workspace, pixel stride (elements)
struct GRef { int64_t off = -1; int ld = 0; int64_t goff = 0; }; // grouped view (see common.h)

static inline int round8(int c) { return (c + 7) & ~7; }

struct ConvW {
    std::string name;
    int kind = 0, cin = 0, cout = 0;
    int kin_p = 0, nout_p = 0;       // padded K (input channels incl. zero pad) and N
    int64_t w_off = 0, b_off = 0;    // into flat params (elements)
    PackSpec fwd{}, dgrad{};         // dgrad.ntaps == 0: no data gradient needed
    int64_t wpk_fwd = -1, wpk_dgrad = -1, dwe = -1;   // workspace byte offsets
    int64_t dwe_floats = 0;
};
struct BnP {
    std::string name;
    int C = 0, calls = 1;
    int64_t g_off = 0, b_off = 0;    // gamma/beta in flat params
    int64_t run_off = 0;             // running mean (var at +C) in flat bn buffer
};
struct DropP { std::string name; int rows = 0, C = 0; int64_t off = 0; };

// one conv-shaped launch, fully bound at configure time
struct ConvOp {
    stcd_conv_geom g{};
    int conv = -1; bool dgrad = false;   // which packed filter of which ConvW
    int tap0 = 0;                        // first tap inside that filter's PackSpec (sub-pixel phases)
    int kreal = 0, nreal = 0;            // un-padded channels (algorithmic work accounting)
    double flops = 0.0, bytes = 0.0;     // ... of the launch, as its profile record reports it (Binder: conv_work; the stem's own)
    ConvMfmaPlan plan; int64_t wf = -1;  // MFMA path: plan + fragment-order weight image (workspace offset)
    bool small = false;                  // eligible for the small-channel persistent kernel
    ConvResPlan res; int res_groups = 1; // resident-filter persistent kernel (3x3 stride 1, Ci % 32 == 0)
    ConvGemmPlan gemm;                    // 1x1 convs with Ci % 64 == 0, Co % 64 == 0: tiled GEMM
    ConvDmaPlan dma;                      // wide layers on large maps: 256 x 256 implicit-GEMM tile staged by LDS-DMA (kernels_conv_dma.hip)
    ConvHaloPlan halo;                    // wide 3x3 layers on large maps: resident halo, streamed filter (opt-in, STCD_HALO_KERNEL=1)
    ConvTilePlan tile;                    // k_conv_res layers with Ci % 64 == 0 on small maps: LDS-DMA staged tile kernel (pick_tile, FC-Siam only)
};
struct WgradOp {
    stcd_conv_geom g{};
    int conv = -1, tap0 = 0, kreal = 0, nreal = 0;
    WgradMfmaPlan plan;
    int64_t slab = -1;                   // this launch's own K-split slabs (reduced in one batched launch per stage)
    int stage = 0;
    int64_t in_off = -1, dout_off = -1;  // workspace offsets of X and dY (grouped launch at the end of the stage)
    int group = -1;                      // index of its WgradGroup inside e.wgroups[stage] (form_wgroups); -1: a launch of its own
    WgradXf xf;                          // X is a virtual activation (the producer's raw conv output, transformed while staged: XfSrc); xf.C == 0: plain
    bool own_taps = false;               // filter taps (ky, kx) of this launch given here instead of conv.fwd.ky/kx[tap0 + t]
    int8_t oky[9] = {0}, okx[9] = {0};   // (the 7x7 stem: 49 taps spread over 7 launches)
};
struct WgradGroup {                      // all launches of one kernel in one backward stage
    WgradKernel kernel;
    std::vector<WgradJob> jobs;
    int total_blocks = 0, lds_bytes = 0;
    int64_t table_off = -1;
    double flops = 0.0, bytes = 0.0;
};
// What a backward call changes on the weight-gradient path; the plan above is read-only after configure.  WgradScope resets it.
struct WgradRun {
    struct Group { int seen = 0; bool launched = false; };      // members whose operands exist so far; the group's grid went out
    std::vector<Group> groups[2];        // per stage, as e.wgroups (sized by build_wgrad_jobs: a step allocates nothing)
    bool early = false;                  // exec_wgrad sends a group out with its last member
    hipStream_t side = nullptr;          // ... on this stream, when there is one
    bool rj_early_done = false, final_on_main = false;      // stage 1's split reduce table (rj_split)
    bool failed = false;                 // a launch of this path was refused or a HIP call failed (set_error has the text): stage_tail returns 1
};

struct Cbrd {                         // conv -> BN -> ReLU -> Dropout2d [-> pool]
    ConvOp fwd, dgr; WgradOp wg;
    int conv = -1, bn = -1, drop = -1;
    int N = 0, H = 0, W = 0, groups = 1, npg = 0;
    TRef in; int K = 0;               // input view and its channel count
    TRef Y; GRef A; TRef P; TRef dPool; bool pool = false;
    GRef dA; TRef dY; TRef dIn; bool has_dIn = false;
    int64_t stat = -1;
    int64_t facc = -1, bacc = -1;     // BatchNorm accumulators (forward statistics / backward sums), see common.h
    const Cbrd* dgr_bwd = nullptr;    // this layer's data-gradient launch also forms the BatchNorm-backward sums of THAT layer (BwdSum)
    bool bwd_sums_fused = false;      // ... and that layer then skips its k_bn_reduce launch
    int64_t dgr_sum_acc = -1; int dgr_sum_c0 = 0, dgr_sum_C = 0;   // the data-gradient launch also sums a channel slice of its
                                                                    // output (bias gradient of the transposed conv feeding it)
    TRef fuse_dst;                    // skip layers of diff / sub: the decoder's concat slice that receives |a1-a2| / a2-a1
    // "virtual activation" (round 4): virt = this layer's A is never written -- its ONE consumer (the next conv of the stage: forward
    // launch and weight gradient) reads Y and applies scale / shift / ReLU / Dropout2d while staging (no k_bn_act launch, one tensor
    // pass less); xsrc = the producer whose raw output this layer reads that way (nullptr: a materialised input)
    bool virt = false; const Cbrd* xsrc = nullptr;
};
struct XConc {                        // cross_conc skip block of SiamUnet_cross_conc (SiamUnet_crossconc.py:11-33): pairwise depthwise
    int level = 0, C = 0;             // conv -> BN -> ReLU, then conv3x3 C -> C -> BN -> ReLU (the Cbrd `res`, no dropout) into the concat slice
    int64_t w_off = 0, b_off = 0;     // diff.0 weight [C][2][3][3] / bias in the flat parameters
    int bn1 = -1;
    TRef G, dG, R, dR;                // pairwise-conv output (+ gradient), its BN + ReLU (+ gradient)
    int64_t stat1 = -1, facc1 = -1, bacc1 = -1, part = -1;
    Cbrd res;
};
struct UpConv {
    int conv = -1, level = 0;
    int N = 0, h = 0, w = 0, Ho = 0, Wo = 0, C = 0;   // input h x w, concat buffer Ho x Wo
    TRef in, out, dOut, dIn;
    ConvOp fwd[4], dgr; WgradOp wg[4];
    int64_t bias_acc = -1; bool bias_fused = false;
};

// ---- optional event instrumentation: one hipEvent pair around every launch of a kernel class (bench.py's live
//      roofline measurement; off by default, adds nothing to the normal path)
enum ProfClass { PC_CONV = 0, PC_WGRAD = 1, PC_BN_STATS = 2, PC_BN_ACT = 3, PC_BN_BWD_REDUCE = 4, PC_BN_BWD_APPLY = 5,
                 PC_POOL_FUSE = 6, PC_PACK = 7, PC_COUNT = 8 };
struct ProfRec { hipEvent_t a, b; int klass; int name_id; double flops, bytes; };
struct Prof {
    bool on = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
    std::vector<std::string> names;      // kernel names as rocprofv3 prints them (substring), interned
    size_t used = 0;
    int intern(const std::string& n) {
        for (size_t i = 0; i < names.size(); ++i)
            if (names[i] == n) return (int)i;
        names.push_back(n);
        return (int)names.size() - 1;
    }
    hipEvent_t get() {
        if (used == pool.size()) { hipEvent_t ev; (void)hipEventCreate(&ev); pool.push_back(ev); }
        return pool[used++];
    }
    ~Prof() { for (auto ev : pool) (void)hipEventDestroy(ev); }
};

// ---- SegCD plan: one generic layer = conv (1x1 / 3x3 / strided / the 7x7 stem) -> BatchNorm [-> + residual] [-> ReLU]
struct ViewRef { int64_t off = 0; int ld = 0; int64_t goff = 0; int gmask = 1; };    // workspace-relative SliceViews entry
struct GLayer {
    std::string name;
    int conv = -1, bn = -1, kind = K_CONV3;
    int N = 0, Hi = 0, Wi = 0, Ho = 0, Wo = 0, K = 0, C = 0, groups = 2, npg = 0;
    bool relu = true;
    TRef in, Y, A, res;                   // res.off < 0: no residual
    TRef dA, dIn, dRes;                   // dA: summed gradient of A (dY is formed in place); dIn: this layer's contribution to
    bool has_dIn = true;                  // d(in); dRes: gated gradient of the residual branch (dZout), off < 0: none
    std::vector<ViewRef> extra_dst;       // decoder concat slices that also receive A
    std::vector<ViewRef> grad_src;        // gradient contributions gathered into dA by the BatchNorm-backward reduction
    bool grad_base = true;                // dA already holds a contribution when the backward of this layer starts
    ConvOp fwd, dgr[4]; int ndgr = 0; WgradOp wg[8]; int nwg = 0;
    int64_t stat = -1, coef = -1, facc = -1, bacc = -1;
    int g_first = 0;                      // BatchNorm group the reference normalises first (running-statistic update order)
};
enum GStepKind { GS_LAYER = 0, GS_MAXPOOL = 1, GS_UPSAMPLE = 2, GS_ABSDIFF = 3, GS_BCONV = 4, GS_ABSPAIR = 5, GS_BILINEAR = 6,
                 GS_TOKENIZE = 7, GS_TOKENENC = 8, GS_TOKENDEC = 9 };
// GS_ABSDIFF (FFCTLCD): images [2B, 3B) of `src` (C channels of a [3B, h, w, ld] tensor) = |date 0 - date 1|; backward: the
// gradient of that third group (dsrc) becomes a [2B, h, w, C] contribution buffer (ddst) the producer of the two dates gathers
// base_resnet tail (dsrc / ddst: gradients of src / dst): GS_BCONV = conv_pred, a biased 3x3 conv without BatchNorm over the 2B images
// of src; GS_ABSPAIR: dst [B] = |date 0 - date 1| of src [2B]; GS_BILINEAR: dst [N, 4h, 4w] = bilinear x4 of src (align_corners = False)
// BIT token path between GS_BCONV and GS_ABSPAIR (kernels_bit.hip; state in stcd_engine_impl::bit): GS_TOKENIZE: tokens of the 2B images of
// src (its backward adds the tokenizer's data gradient to the decoder's and writes conv_pred's ddst = dsrc); GS_TOKENENC: the
// token-encoder layer per pair; GS_TOKENDEC: dst = the decoder over src with the encoded tokens (backward: ddst -> bit.dec_din)
struct GStep { int kind = GS_LAYER; int layer = -1; TRef src, dst, dsrc, ddst; int N = 0, h = 0, w = 0, C = 0; };

// ---- SNUNet-ECAM plan (SNUNet.py:63-152)
struct SrcSlice { TRef src; TRef dsrc; int C = 0; int prod = -1; int grp = -1; };   // a producer's output inside a consumer's concat
struct NBlock {                                              // conv_block_nested (SNUNet.py:8-26)
    std::string name;
    int c1 = -1, bn1 = -1, c2 = -1, bn2 = -1;
    int N = 0, H = 0, W = 0, groups = 1, npg = 0, Cin = 0, C = 0;
    TRef in, dIn;                                            // (concat) input and its gradient; dIn.off < 0: no data gradient
    std::vector<SrcSlice> srcs;                              // prefix slices copied in; the up-sampled tail is written in place
    int up = -1;
    TRef Y1, A1, Y2, Out, P, dOut, dP, dZ2, dA1;
    TRef dbg_dOut;                                           // stcd_set_debug bit 0: copy of the gathered dOut (bn2's backward overwrites it)
    bool pool = false;
    int64_t stat1 = -1, stat2 = -1;
    int64_t facc1 = -1, bacc1 = -1, facc2 = -1, bacc2 = -1;
    int64_t d1_sum_acc = -1; int d1_sum_c0 = 0, d1_sum_C = 0;
    std::vector<ViewRef> extra_dst;                          // consumers' concat slices that receive Out (forward)
    std::vector<ViewRef> grad_src;                           // consumers' concat-gradient slices (+ up-sampling paths) summed into dOut
    bool grad_base = false;                                  // dOut already holds a gradient (max-pool / ECAM) before the sum
    ConvOp f1, f2, d1, d2; WgradOp w1, w2;
};
struct SnUp {                                                // up: ConvTranspose2d(C, C, 2, stride=2) (SNUNet.py:29-43)
    int conv = -1, N = 0, h = 0, w = 0, C = 0;
    TRef src, dsrc, out, dOut, tmp;                          // out/dOut: tail slice of the consumer's concat buffers
    ConvOp fwd[4], dgr; WgradOp wg[4];
    int64_t bias_acc = -1; bool bias_fused = false; int coff = 0;
};

struct CfPlan;                                                  // ChangeFormer plan (engine_cf.inl)
struct stcd_engine_impl {
    Prof prof;
    std::shared_ptr<CfPlan> cf;
    std::vector<NBlock> sn_blocks;
    std::vector<SnUp> sn_ups;
    std::vector<int> sn_order;                               // forward order of blocks (index into sn_blocks)
    std::vector<XConc> xc;                                   // SiamUnet_cross_conc: one block per level (index = level 0..3)
    int sn_final = -1;
    int64_t sn_w[4] = {0, 0, 0, 0};                          // ca.fc1, ca.fc2, ca1.fc1, ca1.fc2 offsets in the flat params
    TRef snE, sndE, snZ, sndZ;
    TRef sn_dbg_dE;                                          // stcd_set_debug bit 0: copy of the head's data gradient sndE
    int64_t sn_pool = -1, sn_argm = -1, sn_att = -1, sn_hid = -1, sn_sums = -1, sn_dpool = -1, sn_part = -1;
    int64_t sn_dout_begin = -1, sn_dout_end = -1;
    ConvOp sn_final_fwd, sn_final_dgr; WgradOp sn_final_wg;
    // Siam_NestedUNet_Conc (SNUNet.py:155-243): final1..4 / conv_final offsets in the flat params (weight, bias), head scratch
    int64_t snc_w[5] = {0, 0, 0, 0, 0}, snc_b[5] = {0, 0, 0, 0, 0}, snc_scratch = -1;
    // ---- SegCD (ResNet-50 UNet) plan
    std::vector<GLayer> g_layers;                            // every conv + BatchNorm (+ residual) (+ ReLU) layer, forward order
    std::vector<GStep> g_fwd;                                // forward program (the backward walks it in reverse)
    int g_stem = -1, g_head_conv = -1;
    int debug_flags = 0;
    std::vector<stcd_ws_tensor> ws_tensors;
    std::vector<std::array<int, 4>> g_blocks;                // per residual block: (L1, L2, L3, Ld or -1) bottleneck; (L1, -1, L2, Ld or -1) basic
    int seg_x = 4, seg_layers[4] = {3, 4, 6, 3};             // block expansion (4: Bottleneck, 1: BasicBlock) and blocks per stage
    int seg_dates = 2;                                       // 2: SegCD (both dates batched, per-date BatchNorm groups); 1: UnetSeg
    bool seg_ffc = false;                                    // FFCTLCD: the decoder also runs on |f1 - f2| (a third group)
    TRef g_pool_idc;                                         // identity-branch contribution of layer1.0 to d(max-pool output)
    std::vector<std::array<int, 2>> g_dec;                   // (conv1, conv2) per decoder block
    TRef gP0, gdP0, gX3, gdX3, gFuseTmp;
    int64_t g_pool_idx = -1;                                  // winners of the stem's 3x3 max-pool (bytes)
    int64_t g_stem_part = -1;                                 // k_stem_wgrad's per-chunk partial filters (fp32 / non-MFMA path: fixed-order finish)
    int64_t g_raw3 = -1, g_draw3 = -1;
    ConvOp g_head_fwd, g_head_dgr; WgradOp g_head_wg;
    // ---- base_resnet (the BIT family's CNN baseline): SegCD's BasicBlock trunk at stride (1,2,1,1) + the tail above
    bool bres = false; int seg_nstage = 4;                   // residual stages the forward runs (3: resnet_stages_num == 4)
    int g_head_c = 16;                                       // input channels of the head conv
    int g_cls = -1, g_pred_conv = -1;                        // classifier.0 + classifier.1 (one BatchNorm group); conv_pred
    ConvOp g_pred_fwd, g_pred_dgr; WgradOp g_pred_wg;
    int64_t g_pred_bias_acc = -1;
    // ---- BIT (BASE_Transformer): the token path between conv_pred and the differencing
    struct BitPlan {
        bool on = false; int L = 1, dh = 64;                 // decoder depth, decoder dim_head (the encoder: one layer, dim_head 64)
        int64_t pos_off = 0, wa_off = 0, enc_off = 0, dec_off = 0;      // flat parameter offsets (elements)
        int64_t tok_in = -1, tok_out = -1, dtok_out = -1, dtok_in = -1, stat = -1, AP = -1, dAP = -1, xs = -1, dG = -1, dec_part = -1,
                dmh = -1, dm = -1, enc_part = -1, tok_part = -1;        // workspace byte offsets
        TRef dec_din;
    } bit;
    int arch = 0, in_ch = 3, label = 2, dt = F32;
    int64_t min_bn_count = 0;                                // fewest values per channel any BatchNorm layer of the current plan sees
    float drop_p = 0.2f;
    std::vector<stcd_tensor_info> params;
    int64_t param_floats = 0, enc_param_end = 0;
    std::vector<ConvW> convs;
    std::vector<BnP> bns;
    int64_t bn_floats = 0;
    // shape-bound plan
    bool configured = false, fwd_training = false;
    int B = 0, H = 0, W = 0;
    std::vector<DropP> drops;
    int64_t drop_floats = 0;
    int64_t ws_bytes = 0;
    std::vector<Cbrd> enc, dec;
    std::vector<UpConv> ups;
    int final_conv = -1;
    ConvOp final_fwd, final_dgr; WgradOp final_wg;
    const Cbrd* final_dgr_bwd = nullptr;                // the last decoder layer, when final_dgr also forms its BatchNorm-backward sums
    const Cbrd* final_xsrc = nullptr;   // conv11d reads conv12d's raw output (virtual activation)
    int use_virt = 0;                   // STCD_VIRT_ACT=1: virtual activations (round 4: built, bit-identical, MEASURED 2-3 % SLOWER on the
                                        // headline step -- DESIGN.md section 4 -- so every activation is materialised by default)
    int fc_virt_layers = 0;             // layers of the current FC-Siam plan whose activation is virtual
    std::vector<ConvOp*> conv_ops;      // every ConvOp of the plan (weight-image packing walks this)
    int64_t slab = -1, slab_floats = 0;
    std::vector<WgradOp*> wgrad_ops;                    // every WgradOp of the plan
    std::vector<WgradGroup> wgroups[2];                 // per backward stage: grouped weight-gradient launches
    std::vector<ReduceJob> rjobs[2];                    // per backward stage
    int64_t rjobs_total[2] = {0, 0}, rjobs_off[2] = {-1, -1};
    // FC-Siam, stage 1: the reduce table is split by weight-gradient group.  Jobs [0, rj_split) belong to the groups that go out
    // before the stage's last one (wg_final_group: the group of wg_last_op, conv11's weight gradient, the backward's last launch)
    // and are reduced right behind the last of them; jobs [rj_split, n) are the final group's, reduced on the tail.  Each part's
    // `start`s count from 0.  rj_split == 0: one launch on the tail for the whole table.
    const WgradOp* wg_last_op = nullptr;
    int rj_split = 0, wg_final_group = -1;
    int64_t rj_total_early = 0, rj_total_final = 0;
    WgradRun wrun;
    int last_tail = 0;      // what the last stage-1 tail found: bit 0 the early part was reduced behind its groups, bit 1 the final group ran on the caller's stream
    // batched filter repacking: [0] = forward-only job list (eval), [1] = forward + data-gradient filters (training)
    std::vector<PackJob> jobs[2];
    int64_t jobs_total[2] = {0, 0}, jobs_off[2] = {-1, -1};
    const void* jobs_uploaded_ws = nullptr;
    uint64_t weights_tag = 0, packed_tag = 0;      // stcd_set_weights_tag: skip the repack while the caller vouches for the weights
    const void* packed_ws = nullptr; const void* packed_params = nullptr; int packed_level = -1;
    TRef X0, G, finalIn, dFinalIn;
    int Hs[5] = {0}, Ws[5] = {0};
    TRef D[4], dD[4], P[4], dP[4];
    int64_t zero_begin = -1, zero_end = -1;          // everything a step needs zeroed (accumulators, ...): ONE memset per forward
    int64_t final_bias_acc = -1;
    std::vector<BiasJob> bias_jobs; int64_t bias_jobs_off = -1;
    int64_t masks = -1, dwe_begin = -1, dwe_end = -1, scratch8 = -1;
    int use_mfma = 1, use_small = 1, use_wgroup = 1, use_res = 1, use_skip_fused = 1, use_act_fuse = 1, use_gemm = 1, use_skip_recompute = 1, use_bwdsum = 1, use_bwdsum_res = 0, use_tile = 1, use_halo = 0;
    // FC-Siam backward: the decoder's grouped weight gradients (+ slab reduce, bias finish) run on a low-priority side stream beside
    // the encoder's backward chain on the caller's stream; their grids get 1 / WG_SIDE_DIV of the planner's block budget so that the
    // chain's blocks find free slots (wgrad_side_stream)
    int wg_side_on = 1;
    static constexpr int WG_SIDE_DIV = 4;                // share of the planner's block budget for stage 0's grouped grids: 1 / div
    static constexpr int WGROUP_ROUNDS = 1, WGROUP_MIN_TILES = 8;      // split_tile_group: resident rounds of a group's blocks, fewest tiles per block
    hipStream_t wg_side = nullptr; hipEvent_t wg_fork = nullptr, wg_join = nullptr; int wg_side_dev = -1;
};

}  // namespace stcd

using namespace stcd;
struct stcd_engine : stcd_engine_impl {};

namespace stcd {

// ------------------------------------------------------------------------------------------ model tables
static const int ENC_STAGE_CONVS[4] = {2, 2, 3, 3};
static const int ENC_C[4] = {16, 32, 64, 128};
static const int SKIP_IDX[4] = {1, 3, 6, 9};           // the encoder layer whose activation is level s's skip connection

static void add_param(stcd_engine& e, const std::string& name, std::initializer_list<int64_t> shape, int64_t* off_out) {
    stcd_tensor_info ti;
    memset(&ti, 0, sizeof(ti));
    snprintf(ti.name, sizeof(ti.name), "%s", name.c_str());
    ti.ndim = (int)shape.size();
    int64_t n = 1;
    int i = 0;
    for (auto s : shape) { ti.shape[i++] = s; n *= s; }
    ti.numel = n;
    ti.offset = e.param_floats;
    *off_out = ti.offset;
    e.param_floats += (n + 3) & ~(int64_t)3;   // keep every tensor 16-B aligned in the flat buffer
    e.params.push_back(ti);
}

static void make_specs(ConvW& c, bool need_dgrad) {
    if (c.kind == K_STEM7) {      // dedicated kernels read / write the reference layout directly: nothing to pack
        c.fwd = PackSpec{}; c.dgrad = PackSpec{};
        c.fwd.ks = 7; c.fwd.K = c.cin; c.fwd.N = c.cout; c.fwd.kpad = c.kin_p; c.fwd.wld = c.nout_p;
        return;
    }
    if (c.kind == K_CONV3_S2) {   // Conv2d(k3, s2, p1): forward = stride-2 gather; data gradient = 4 sub-pixel phases (as K_UPCONV's forward)
        PackSpec& f = c.fwd;
        f.ks = 3; f.K = c.cin; f.N = c.cout; f.kpad = c.kin_p; f.wld = c.nout_p; f.ntaps = 9; f.kn_major = 0;
        {   // taps grouped by the PARITY PLANE of the input pixel they read (row 2m + ky - 1: ky == 1 -> even rows, else odd), planes
            // (0,0),(0,1),(1,0),(1,1) with 1+2+2+4 taps: the weight gradient runs as four stride-1 launches over plane views
            int t = 0;
            for (int py = 0; py < 2; ++py)
                for (int px = 0; px < 2; ++px)
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx)
                            if ((ky != 1) == (py == 1) && (kx != 1) == (px == 1)) { f.ky[t] = ky; f.kx[t] = kx; ++t; }
        }
        PackSpec& d = c.dgrad;
        d.ks = 3; d.K = c.cout; d.N = c.cin; d.kpad = c.nout_p; d.wld = round8(c.cin); d.ntaps = need_dgrad ? 9 : 0; d.kn_major = 1;
        int t = 0;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px)
                for (int dy = 0; dy <= py; ++dy)
                    for (int dx = 0; dx <= px; ++dx) { d.ky[t] = py + 1 - 2 * dy; d.kx[t] = px + 1 - 2 * dx; ++t; }
        return;
    }
    if (c.kind == K_CONV1 || c.kind == K_CONVT2 || c.kind == K_CONV1_S2) {
        const int ks = c.kind == K_CONVT2 ? 2 : 1;
        PackSpec& f = c.fwd;
        f.ks = ks; f.K = c.cin; f.N = c.cout; f.kpad = c.kin_p; f.wld = c.nout_p;
        f.ntaps = ks * ks;
        f.kn_major = c.kind == K_CONVT2;              // ConvTranspose2d weights are [Cin][Cout][k][k]
        for (int t = 0; t < f.ntaps; ++t) { f.ky[t] = t / ks; f.kx[t] = t % ks; }   // K_CONVT2: tap = output phase (py,px)
        PackSpec& d = c.dgrad;
        d.ks = ks; d.K = c.cout; d.N = c.cin; d.kpad = c.nout_p; d.wld = round8(c.cin);
        d.ntaps = need_dgrad ? ks * ks : 0;
        d.kn_major = c.kind != K_CONVT2;
        for (int t = 0; t < ks * ks; ++t) { d.ky[t] = t / ks; d.kx[t] = t % ks; }   // K_CONVT2: tap (dy,dx) of the stride-2 gather
        return;
    }
    PackSpec& f = c.fwd;
    f.ks = 3;
    f.K = c.cin; f.N = c.cout; f.kpad = c.kin_p; f.wld = c.nout_p;
    PackSpec& d = c.dgrad;
    d.ks = 3;
    d.K = c.cout; d.N = c.cin; d.kpad = c.nout_p; d.wld = round8(c.cin);
    d.ntaps = 0;
    if (c.kind == K_CONV3 || c.kind == K_CONVT3_S1) {
        f.ntaps = 9;
        f.kn_major = c.kind == K_CONVT3_S1;       // ConvTranspose2d weights are [Cin][Cout][3][3]
        for (int t = 0; t < 9; ++t) {
            int dy = t / 3 - 1, dx = t % 3 - 1;
            f.ky[t] = c.kind == K_CONV3 ? dy + 1 : 1 - dy;
            f.kx[t] = c.kind == K_CONV3 ? dx + 1 : 1 - dx;
        }
        if (need_dgrad) {
            d.ntaps = 9;
            d.kn_major = c.kind == K_CONV3;
            for (int t = 0; t < 9; ++t) {
                int dy = t / 3 - 1, dx = t % 3 - 1;
                d.ky[t] = c.kind == K_CONV3 ? 1 - dy : 1 + dy;
                d.kx[t] = c.kind == K_CONV3 ? 1 - dx : 1 + dx;
            }
        }
    } else {  // K_UPCONV: 4 sub-pixel phases, 1+2+2+4 taps, stored in phase order (py,px) = (0,0),(0,1),(1,0),(1,1)
        f.ntaps = 9;
        f.kn_major = 1;
        int t = 0;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px)
                for (int dy = 0; dy <= py; ++dy)
                    for (int dx = 0; dx <= px; ++dx) {
                        f.ky[t] = py + 1 - 2 * dy;
                        f.kx[t] = px + 1 - 2 * dx;
                        ++t;
                    }
        if (need_dgrad) {   // stride-2 3x3 conv over dOut
            d.ntaps = 9;
            d.kn_major = 0;
            for (int k = 0; k < 9; ++k) { d.ky[k] = k / 3; d.kx[k] = k % 3; }
        }
    }
}

static int add_conv(stcd_engine& e, const std::string& name, int kind, int cin, int cout, bool need_dgrad, bool bias = true) {
    ConvW c;
    c.name = name; c.kind = kind; c.cin = cin; c.cout = cout;
    c.kin_p = round8(cin); c.nout_p = round8(cout);
    if (kind == K_CONV3 || kind == K_CONV3_S2) add_param(e, name + ".weight", {cout, cin, 3, 3}, &c.w_off);
    else if (kind == K_CONV1 || kind == K_CONV1_S2) add_param(e, name + ".weight", {cout, cin, 1, 1}, &c.w_off);
    else if (kind == K_STEM7) add_param(e, name + ".weight", {cout, cin, 7, 7}, &c.w_off);
    else if (kind == K_CONVT2) add_param(e, name + ".weight", {cin, cout, 2, 2}, &c.w_off);
    else add_param(e, name + ".weight", {cin, cout, 3, 3}, &c.w_off);
    c.b_off = -1;
    if (bias) add_param(e, name + ".bias", {cout}, &c.b_off);
    make_specs(c, need_dgrad);
    e.convs.push_back(c);
    return (int)e.convs.size() - 1;
}
static int add_bn(stcd_engine& e, const std::string& name, int C, int calls) {
    BnP b;
    b.name = name; b.C = C; b.calls = calls;
    add_param(e, name + ".weight", {C}, &b.g_off);
    add_param(e, name + ".bias", {C}, &b.b_off);
    b.run_off = e.bn_floats;
    e.bn_floats += 2 * C;
    e.bns.push_back(b);
    return (int)e.bns.size() - 1;
}

struct DecSpec { const char* up; int C; int n; const char* sfx[3]; int cout[3]; };
static const DecSpec DEC[4] = {
    {"upconv4", 128, 3, {"43d", "42d", "41d"}, {128, 128, 64}},
    {"upconv3", 64, 3, {"33d", "32d", "31d"}, {64, 64, 32}},
    {"upconv2", 32, 2, {"22d", "21d", nullptr}, {32, 16, 0}},
    {"upconv1", 16, 2, {"12d", "11d", nullptr}, {16, -1, 0}},   // 11d -> label_nbr, no BN
};

// FC-EF (`Unet`, models/Unet.py:93-154): the FC-Siam-conc plan with ONE encoder stream over cat(x1, x2) -- every encoder tensor holds
// B images in one BatchNorm group, the skips are the stream's own activations, written straight into the concat buffers
static inline int fc_dates(const stcd_engine& e) { return e.arch == STCD_ARCH_FCEF ? 1 : 2; }
static inline bool fc_concat_skips(const stcd_engine& e) { return e.arch == STCD_ARCH_CONC || e.arch == STCD_ARCH_FCEF; }
static inline bool fc_cross(const stcd_engine& e) { return e.arch == STCD_ARCH_XCONC; }
// Siam_NestedUNet_Conc shares the trunk (tables, plan, block order); only the tail differs (kernels_snhead.hip)
static inline bool is_snconc(int arch) { return arch == STCD_ARCH_SNUNET_CONC || arch == STCD_ARCH_SNUNET_CONC_DS; }
static inline bool is_snunet(int arch) { return arch == STCD_ARCH_SNUNET || is_snconc(arch); }
static inline int sn_out_maps(int arch) { return arch == STCD_ARCH_SNUNET_CONC_DS ? 5 : 1; }
// skip layers of diff / sub whose activations are never stored: the forward writes only the pooled map and the fused skip,
// the backward (k_skip_bwd_pair) recomputes them from Y
static inline bool skip_recomputed(const stcd_engine& e, const Cbrd& L) {
    return e.use_skip_recompute && e.use_act_fuse && e.use_skip_fused && L.pool && L.fuse_dst.off >= 0 && L.groups == 2 &&
           skip_pair_supported(L.npg, L.H, L.W, e.convs[L.conv].cout);
}
static inline bool fc_family(const stcd_engine& e) {      // the engines backward_fcsiam runs
    return e.arch == STCD_ARCH_DIFF || e.arch == STCD_ARCH_CONC || e.arch == STCD_ARCH_SUB || e.arch == STCD_ARCH_FCEF || e.arch == STCD_ARCH_XCONC;
}

static void build_fcsiam_tables(stcd_engine& e) {
    // registration order of SiamUnet_*.__init__ (SiamUnet_diff.py:18-90): conv, bn per layer; upconv before its stage
    for (int s = 0; s < 4; ++s)
        for (int j = 0; j < ENC_STAGE_CONVS[s]; ++j) {
            std::string sfx = std::to_string(s + 1) + std::to_string(j + 1);
            int cin = j == 0 ? (s == 0 ? (e.arch == STCD_ARCH_FCEF ? 2 * e.in_ch : e.in_ch) : ENC_C[s - 1]) : ENC_C[s];
            add_conv(e, "conv" + sfx, K_CONV3, cin, ENC_C[s], !(s == 0 && j == 0));
            add_bn(e, "bn" + sfx, ENC_C[s], fc_dates(e));
        }
    e.enc_param_end = e.param_floats;
    for (int k = 0; k < 4; ++k) {
        const DecSpec& d = DEC[k];
        add_conv(e, d.up, K_UPCONV, d.C, d.C, true);
        int skipc = e.arch == STCD_ARCH_CONC ? 2 * d.C : d.C;
        int cin = d.C + skipc;
        for (int j = 0; j < d.n; ++j) {
            int cout = d.cout[j] < 0 ? e.label : d.cout[j];
            add_conv(e, std::string("conv") + d.sfx[j], K_CONVT3_S1, cin, cout, true);
            if (d.cout[j] >= 0) add_bn(e, std::string("bn") + d.sfx[j], cout, 1);
            cin = cout;
        }
    }
    if (fc_cross(e)) {      // SiamUnet_crossconc.py:119-122: cross_conc1..4 registered after the decoder, each diff.0 / diff.1 / conv_res.0 / conv_res.1
        e.xc.assign(4, XConc());
        for (int l = 0; l < 4; ++l) {
            XConc& X = e.xc[l];
            const std::string n = "cross_conc" + std::to_string(l + 1);
            X.level = l; X.C = ENC_C[l];
            add_param(e, n + ".diff.0.weight", {X.C, 2, 3, 3}, &X.w_off);
            add_param(e, n + ".diff.0.bias", {X.C}, &X.b_off);
            X.bn1 = add_bn(e, n + ".diff.1", X.C, 1);
            X.res.conv = add_conv(e, n + ".conv_res.0", K_CONV3, X.C, X.C, true);
            X.res.bn = add_bn(e, n + ".conv_res.1", X.C, 1);
        }
    }
}

// ------------------------------------------------------------------------------------------ workspace plan
struct Planner;
static void build_wgrad_jobs(stcd_engine& e, Planner& ws);
static void build_filter_pack_jobs(stcd_engine& e, Planner& ws);
// The workspace planner every configure_* builds its plan with: a bump allocator over the caller's workspace (256-byte slices, in
// the order of the calls -- each family keeps its own sequence), the named tensors of the test introspection, the bias jobs and
// the tail all four families share.
struct Planner {
    stcd_engine& e;
    const int64_t T;                     // bytes per activation element
    int64_t cur = 0;
    explicit Planner(stcd_engine& e_) : e(e_), T((int64_t)dsize(e_.dt)) {}
    int64_t take(int64_t bytes) {
        int64_t o = cur;
        cur += (bytes + 255) & ~(int64_t)255;
        e.ws_bytes = cur;                // the plan's size is whatever has been taken so far (SNUNet takes its debug copies after tables())
        return o;
    }
    TRef plain(int n, int h, int w, int c) { TRef t; t.off = take((int64_t)n * h * w * c * T); t.ld = c; return t; }
    // test introspection (stcd_ws_tensor_*): a named [n, h, w, c] tensor at `off` with pixel stride ld; a tensor the plan does not hold
    // (off < 0) is not listed.  dtype < 0: the engine's activation type (BIT's tokens are fp32 in either mode)
    void tensor(const std::string& name, int64_t off, int ld, int n, int h, int w, int c, int dtype = -1) {
        if (off < 0) return;
        stcd_ws_tensor r;
        memset(&r, 0, sizeof(r));
        snprintf(r.name, sizeof(r.name), "%s", name.c_str());
        r.offset_bytes = off; r.n = n; r.h = h; r.w = w; r.c = c; r.ld = ld; r.dtype = dtype < 0 ? e.dt : dtype;
        e.ws_tensors.push_back(r);
    }
    void tensor(const std::string& name, const TRef& t, int n, int h, int w, int c) { tensor(name, t.off, t.ld, n, h, w, c); }
    // a bias gradient summed in the integer accumulator at acc_off (C channels, `valid` of them real): k_bias_finish converts it
    void bias_job(int64_t acc_off, int conv, int C, int valid) {
        BiasJob jb{}; jb.acc_off = acc_off; jb.out_off = e.convs[conv].b_off; jb.C = C; jb.valid = valid; jb.scale = BN_BS;
        e.bias_jobs.push_back(jb);
    }
    // the tail of every plan: the bias-job table, then the slab / reduce / weight-gradient / repack job tables
    void tables() {
        e.bias_jobs_off = take((int64_t)e.bias_jobs.size() * sizeof(BiasJob) + 16);
        build_wgrad_jobs(e, *this);
        build_filter_pack_jobs(e, *this);
        e.jobs_uploaded_ws = nullptr;
    }
};

static int conv_index(const stcd_engine& e, const std::string& name) {
    for (size_t i = 0; i < e.convs.size(); ++i)
        if (e.convs[i].name == name) return (int)i;
    return -1;
}
static int bn_index(const stcd_engine& e, const std::string& name) {
    for (size_t i = 0; i < e.bns.size(); ++i)
        if (e.bns[i].name == name) return (int)i;
    return -1;
}

// ------------------------------------------------------------------------------------------ conv geometries
// Every stcd_conv_geom the engine binds is built by one of these (the per-op ABI checks the caller's own: check_geom).  A wrong
// hi or ldo here is an out-of-bounds access, not a failing assert -- so each shape is written once.  Tap lists that follow a filter
// layout are derived from the PackSpec that orders the filter image: (ky, kx) -> (dy, dx) cannot drift from the packed taps.
static stcd_conv_geom geom_base(int n, int hi, int wi, int ci, int ldi, int hm, int wm, int in_stride,
                                int ho, int wo, int out_stride, int oy0, int ox0, int co, int ldo) {
    stcd_conv_geom g;
    memset(&g, 0, sizeof(g));
    g.n = n; g.hi = hi; g.wi = wi; g.ci = ci; g.ldi = ldi;
    g.hm = hm; g.wm = wm; g.in_stride = in_stride;
    g.ho = ho; g.wo = wo; g.out_stride = out_stride; g.oy0 = oy0; g.ox0 = ox0;
    g.co = co; g.ldo = ldo;
    return g;
}
// stride-1 3x3 (padding 1) over the whole map
static stcd_conv_geom geom3(int N, int H, int W, int K, int ldi, int co, int ldo) {
    stcd_conv_geom g = geom_base(N, H, W, K, ldi, H, W, 1, H, W, 1, 0, 0, co, ldo);
    g.ntaps = 9;
    for (int t = 0; t < 9; ++t) { g.dy[t] = (int8_t)(t / 3 - 1); g.dx[t] = (int8_t)(t % 3 - 1); }
    return g;
}
// stride-1 1x1 (dy / dx[1..8] keep geom3's values: no kernel reads past ntaps)
static stcd_conv_geom geom1(int N, int H, int W, int K, int ldi, int co, int ldo) {
    stcd_conv_geom g = geom3(N, H, W, K, ldi, co, ldo);
    g.ntaps = 1; g.dy[0] = 0; g.dx[0] = 0;
    return g;
}
// stride-2 gather: output (m, n) of an hm x wm map reads input (2m + ky - pad, 2n + kx - pad) for every tap (ky, kx) of `ps` -- a
// strided Conv2d's forward, a stride-2 ConvTranspose2d's data gradient.  (hi, wi) are the BUFFER dims (row pitch): the taps reach
// row 2 hm - 1 / column 2 wm - 1 at most, so the replication-padded rows / columns of an odd-sized concat buffer are never read.
static stcd_conv_geom geom_gather2(int n, int hi, int wi, int ci, int ldi, int hm, int wm, int co, int ldo, const PackSpec& ps, int pad) {
    stcd_conv_geom g = geom_base(n, hi, wi, ci, ldi, hm, wm, 2, hm, wm, 1, 0, 0, co, ldo);
    g.ntaps = ps.ntaps;
    for (int t = 0; t < ps.ntaps; ++t) { g.dy[t] = (int8_t)(ps.ky[t] - pad); g.dx[t] = (int8_t)(ps.kx[t] - pad); }
    return g;
}
// sub-pixel phase ph = 2 py + px of a stride-2 scatter (a ConvTranspose2d's forward, a strided Conv2d's data gradient) as a
// stride-1 launch that writes every second pixel of the ho x wo buffer:  out(2m + py, 2n + px) = sum_t in(m + dy_t, n + dx_t) W[ky_t][kx_t]
// over the taps [tap0, tap0 + ntaps) of `ps` that land on this phase, dy = (py + pad - ky) / 2 (likewise dx).
static stcd_conv_geom geom_phase(int n, int h, int w, int ci, int ldi, int ho, int wo, int co, int ldo, int ph, const PackSpec& ps, int pad,
                                 int tap0, int ntaps) {
    const int py = ph >> 1, px = ph & 1;
    stcd_conv_geom g = geom_base(n, h, w, ci, ldi, h, w, 1, ho, wo, 2, py, px, co, ldo);
    g.ntaps = ntaps;
    for (int t = 0; t < ntaps; ++t) { g.dy[t] = (int8_t)((py + pad - ps.ky[tap0 + t]) / 2); g.dx[t] = (int8_t)((px + pad - ps.kx[tap0 + t]) / 2); }
    return g;
}
// 3x3 stride 2 padding 1 sorts its nine taps by phase / parity plane (0,0), (0,1), (1,0), (1,1): 1 + 2 + 2 + 4 (make_specs); phase
// ph owns the taps [PHASE3_TAP0[ph], PHASE3_TAP0[ph + 1])
static const int PHASE3_TAP0[5] = {0, 1, 3, 5, 9};
// ... e.g. ConvTranspose2d(k3,s2,p1,op1): out(2m+py, 2n+px) = sum_{dy<=py, dx<=px} in(m+dy, n+dx) W[py+1-2dy][px+1-2dx]
static stcd_conv_geom geom_phase3(int n, int h, int w, int ci, int ldi, int ho, int wo, int co, int ldo, int ph, const PackSpec& ps, int* tap0) {
    *tap0 = PHASE3_TAP0[ph];
    return geom_phase(n, h, w, ci, ldi, ho, wo, co, ldo, ph, ps, 1, *tap0, PHASE3_TAP0[ph + 1] - *tap0);
}
// weight gradient of a stride-2 layer over the parity plane (py, px) of its input: input pixel (2m + ky - pad, 2n + kx - pad) lies in
// the plane at plane coordinates (m + dy, n + dx), dy = (ky - pad - py) / 2 for the taps of that parity.  A plane is a VIEW of the
// NHWC tensor [n, Hi, Wi, ld] starting at pixel (py, px): pixel stride 2 * ld and a virtual row of Wi pixels (= two real rows), of
// which the first Wi / 2 exist (the launch's wi_valid) -- one stride-1 launch per plane (and per <= 9 of its taps).
static stcd_conv_geom geom_plane(int n, int Hi, int Wi, int ci, int ld, int ho, int wo, int co, int ldo, int ph, int pad, int ntaps,
                                 const int8_t* ky, const int8_t* kx) {
    const int py = ph >> 1, px = ph & 1;
    stcd_conv_geom g = geom_base(n, Hi / 2, Wi, ci, 2 * ld, ho, wo, 1, ho, wo, 1, 0, 0, co, ldo);
    g.ntaps = ntaps;
    for (int t = 0; t < ntaps; ++t) { g.dy[t] = (int8_t)((ky[t] - pad - py) / 2); g.dx[t] = (int8_t)((kx[t] - pad - px) / 2); }
    return g;
}
// the 7x7 stride-2 stem's forward on the tap-list GEMM kernel: tap = filter row ky, and the 7 filter columns x 8 (padded) channels
// of a row are 112 contiguous bytes of the NHWC8 input -- one 64-"channel" row of 8 pixels starting 3 pixels to the left
static stcd_conv_geom geom_stem_rows(int n, int Hi, int Wi, int ldi, int ho, int wo, int co, int ldo) {
    stcd_conv_geom g = geom_base(n, Hi, Wi, 64, ldi, ho, wo, 2, ho, wo, 1, 0, 0, co, ldo);
    g.ntaps = 7;
    for (int t = 0; t < 7; ++t) { g.dy[t] = (int8_t)(t - 3); g.dx[t] = -3; }
    return g;
}

static void conv_work(const stcd_engine& e, const stcd_conv_geom& g, int kreal, int nreal, double* flops, double* bytes);

// the tap-list GEMM kernel takes what the resident-filter kernel cannot, and -- for ChangeFormer -- what the resident kernel would
// run in 16-channel output slices, i.e. re-read X once per 16 output channels
static void pick_gemm_or_res(const stcd_engine& e, ConvOp& op, const stcd_conv_geom& g, int groups) {
    if (!e.use_gemm || op.small) return;
    // (ChangeFormer's 256-channel decoder convolutions get 16-channel output slices from the resident-filter kernel, i.e. X is
    //  re-read 16 times through L2: the GEMM kernel's 128 x 128 tile measured 8.3 vs 9.5 ms per step there; a tie elsewhere)
    if (op.res.ok && !(e.cf && op.res.NT == 1)) return;
    op.gemm = conv_gemm_plan(g, op.plan, groups);
    if (!op.gemm.ok) return;
    op.res = ConvResPlan();
    // the LDS-DMA kernel takes the layers it fits once they fill the chip with 256-position tiles (ChangeFormer's decoder head)
    if ((int64_t)g.n * g.hm * g.wm >= 256 * 192) op.dma = conv_dma_plan(g, op.plan);
    // opt-in (measured 0.93 - 1.03 of k_conv_gemm on ChangeFormer's 256 -> 256 layers): layers that take the GEMM kernel,
    // carry no fused BatchNorm statistics (groups == 1 callers that pass none) and fill the chip with 16 x 16 tiles
    if (e.use_halo && (int64_t)g.n * ((g.hm + 15) / 16) * ((g.wm + 15) / 16) >= 512) op.halo = conv_halo_plan(g, op.plan);
}

// The LDS-DMA tile kernel takes a resident-filter layer (same tile, same results) where the launch is a short chain of steps per
// block: Ci % 64 == 0 and at most TILE_MAX_TILES 16 x 16 tiles, i.e. each block of k_conv_res would walk only a few (tile, chunk)
// steps and wait out a memory round trip in each.  Measured per shape in DESIGN.md section 4; STCD_NO_TILE_KERNEL=1 turns it off.
constexpr int TILE_MAX_TILES = 512;
static void pick_tile(const stcd_engine& e, ConvOp& op, const stcd_conv_geom& g, int groups) {
    if (!e.use_tile || !op.res.ok || op.gemm.ok || op.small) return;
    const ConvTilePlan tp = conv_tile_plan(g, op.plan, groups);
    if (tp.ok && tp.ntiles <= TILE_MAX_TILES) op.tile = tp;
}

// weight-gradient plan of one launch: the GEMM kernel for one-tap launches with >= 64 channels on both sides, else the tile kernel
static WgradMfmaPlan pick_wgrad_plan(const stcd_engine& e, const stcd_conv_geom& g, int kpad, int wld) {
    // (a GEMM group is one more launch of the stage: only layers with >= 0.8 GFLOP go there -- FC-Siam's two one-tap up-conv
    //  phases, 0.54 GFLOP each, stay in the tile kernel's grid: measured +2 % on the diff step otherwise)
    if (e.use_gemm && e.use_wgroup && 2.0 * g.n * g.hm * g.wm * (double)g.ci * g.co >= 0.8e9) {
        WgradMfmaPlan p = wgrad_gemm_plan(g, kpad, wld);
        if (p.ok) return p;
    }
    // (64 x 32 tile: SNUNet everywhere; ChangeFormer for its 3x3 layers only -- measured 5.0 vs 5.4 ms there, but 2.7 vs 2.1 ms on the
    //  4-tap phases of its transposed convs)
    // ChangeFormer's 256 -> 256 3x3 layers on 256^2 / 512^2 maps: the LDS-DMA kernel (measured: DESIGN.md section 4)
    if (e.use_wgroup && (g.ntaps == 9 || (e.cf && g.ntaps == 4)) && (int64_t)g.n * g.hm * g.wm >= 65536) {
        WgradMfmaPlan p = wgrad_dma_plan(g, kpad, wld);
        if (p.ok) return p;
    }
    return wgrad_mfma_plan(g, kpad, wld, is_snunet(e.arch) || (e.cf && g.ntaps == 9));
}

// plans of every kernel that may take the bf16 launch op.g (conv_kernel chooses among them per call); with_tile: FC-Siam alone
static void plan_conv(const stcd_engine& e, ConvOp& op, int groups, bool with_tile) {
    op.plan = conv_mfma_plan(op.g);
    op.small = conv_small_ok(op.g, op.plan);
    if (e.use_res && !op.small) op.res = conv_res_plan(op.g, op.plan, groups);
    pick_gemm_or_res(e, op, op.g, groups);
    if (with_tile) pick_tile(e, op, op.g, groups);
}
// the launches of the reference kernel: no bf16 MFMA plan, or no fragment image.  build_filter_pack_jobs packs the fp32 filter image for
// exactly these, and conv_kernel sends exactly these there.
static bool conv_on_ref(bool mfma, const ConvOp& op) { return !(mfma && op.plan.ok && op.wf >= 0); }
// ---- the binder: every conv-shaped launch and every weight gradient of every family is bound here, at configure time.  Both start
//      from a value-initialised op (a re-configure at another shape reuses the objects) and keep only what the caller passes.
struct Binder {
    stcd_engine& e; Planner& ws;
    bool with_tile = false;      // k_conv_tile is a candidate (FC-Siam)
    void conv(ConvOp& op, const stcd_conv_geom& g, int conv, bool dgrad, int tap0, int kreal, int nreal, int groups = 1) const {
        op = ConvOp();
        op.g = g; op.conv = conv; op.dgrad = dgrad; op.tap0 = tap0; op.kreal = kreal; op.nreal = nreal; op.res_groups = groups;
        conv_work(e, g, kreal, nreal, &op.flops, &op.bytes);
        if (e.dt == BF16) plan_conv(e, op, groups, with_tile);
        if (op.plan.ok) op.wf = ws.take(op.plan.wf_elems * 2);
        e.conv_ops.push_back(&op);
    }
    // the 7x7 stem's forward with its plan forced: the tap-list GEMM kernel over 8-pixel rows (g.ci = 64 "channels" = 8 pixels x 8
    // padded channels), or not bound at all -- the dedicated fp32 kernel then runs it
    void stem(ConvOp& op, const stcd_conv_geom& g, int conv, int groups) const {
        op = ConvOp();
        op.g = g; op.conv = conv; op.kreal = e.convs[conv].cin; op.nreal = g.co; op.res_groups = groups;
        op.flops = 2.0 * g.n * g.ho * g.wo * 49.0 * op.kreal * op.nreal;      // the whole 7x7 filter, not the 7 row taps of g
        op.plan = conv_mfma_plan(g);
        if (g.ldi == 8 && g.co % 64 == 0) op.gemm = conv_gemm_plan(g, op.plan, groups);
        op.gemm.pix_chunks = 1;
        if (!op.gemm.ok) return;
        op.wf = ws.take(op.plan.wf_elems * 2);
        e.conv_ops.push_back(&op);
    }
    // own_ky / own_kx: the filter taps of this launch given here instead of conv.fwd.ky / kx[tap0 + t] (the 7x7 stem)
    void wgrad(WgradOp& op, const stcd_conv_geom& g, int conv, int64_t in_off, int64_t dout_off, int stage = 0, int tap0 = 0,
               int wi_valid = 0, const int8_t* own_ky = nullptr, const int8_t* own_kx = nullptr) const {
        const ConvW& cv = e.convs[conv];
        op = WgradOp();
        op.g = g; op.conv = conv; op.tap0 = tap0; op.kreal = cv.cin; op.nreal = cv.cout;
        op.in_off = in_off; op.dout_off = dout_off; op.stage = stage;
        op.own_taps = own_ky != nullptr;
        for (int t = 0; t < g.ntaps && op.own_taps; ++t) { op.oky[t] = own_ky[t]; op.okx[t] = own_kx[t]; }
        if (e.dt == BF16) { op.plan = pick_wgrad_plan(e, g, cv.fwd.kpad, cv.fwd.wld); op.plan.wi_valid = wi_valid; }
        e.wgrad_ops.push_back(&op);
    }
};
// the fp32 filter images of the reference kernels and the fp64 accumulators of the reference weight-gradient path
static void take_ref_images(stcd_engine& e, Planner& ws, bool with_dwe = true) {
    for (auto& c : e.convs) {
        c.wpk_fwd = ws.take((int64_t)c.fwd.ntaps * c.fwd.kpad * c.fwd.wld * 4);
        if (c.dgrad.ntaps) c.wpk_dgrad = ws.take((int64_t)c.dgrad.ntaps * c.dgrad.kpad * c.dgrad.wld * 4);
    }
    e.dwe_begin = ws.cur;
    for (auto& c : e.convs) {
        c.dwe_floats = (int64_t)c.fwd.ntaps * c.fwd.kpad * c.fwd.wld;
        c.dwe = with_dwe ? ws.take(c.dwe_floats * 8) : -1;
    }
    e.dwe_end = ws.cur;
}


// STCD_CF_SIDE=0: ChangeFormer's single-call backward keeps its grouped weight gradients on the caller's stream
static bool cf_side_on() { static const bool on = env_flag("STCD_CF_SIDE", true); return on; }

// ---- the weight-gradient plan of a configure (build_wgrad_jobs): groups, their K splits, slabs and job tables, reduce tables
// floats of ONE K-split slab of a launch, [tap][kpad][wld]
static int64_t wgrad_slab_floats(const stcd_engine& e, const WgradOp& op) { return (int64_t)op.g.ntaps * e.convs[op.conv].fwd.kpad * e.convs[op.conv].fwd.wld; }
// the 8 x 16-position tiles the tile kernel walks
static int64_t wgrad_ntiles(const stcd_conv_geom& g) { return (int64_t)g.n * ((g.wm + 15) / 16) * ((g.hm + 7) / 8); }
// the filter taps (ky, kx) a launch forms: its own table, or its part of the conv's
static void wgrad_taps(const stcd_engine& e, const WgradOp& op, int8_t* ky, int8_t* kx) {
    const PackSpec& f = e.convs[op.conv].fwd;
    for (int t = 0; t < op.g.ntaps; ++t) {
        ky[t] = op.own_taps ? op.oky[t] : f.ky[op.tap0 + t];
        kx[t] = op.own_taps ? op.okx[t] : f.kx[op.tap0 + t];
    }
}
static WgradJob wgrad_job_of(const stcd_engine& e, const WgradKernel& k, const WgradOp& op, int64_t in_off, int64_t dout_off, int64_t slab_off) {
    const PackSpec& f = e.convs[op.conv].fwd;
    return wgrad_job(k, op.g, op.plan, in_off, dout_off, slab_off, f.kpad, f.wld, &op.xf);
}

// step 1: one group per (stage, kernel); every launch with a plan joins the group of its kernel
static void form_wgroups(stcd_engine& e) {
    for (WgradOp* op : e.wgrad_ops) {
        if (!op->plan.ok) continue;
        const WgradKernel k = wgrad_kernel_of(op->plan, op->g, op->xf.C > 0);
        std::vector<WgradGroup>& gs = e.wgroups[op->stage];
        size_t gi = 0;
        while (gi < gs.size() && !(gs[gi].kernel == k)) ++gi;
        if (gi == gs.size()) { gs.emplace_back(); gs.back().kernel = k; }
        op->group = (int)gi;
    }
}

// step 2: the K split (gx) of every member, chosen for the GROUP; one function per kind
// one block per CU and ONE round: the smallest split length (in 64-position K-tiles) whose blocks -- (split, tap, channel tile) over all
// layers of the group -- fit the 256 CUs; every block then walks about the same K
static void split_dma_group(const stcd_engine& e, const std::vector<WgradOp*>& ops) {
    auto positions = [](const WgradOp* op) { return (int64_t)op->g.n * op->g.hi * op->g.wi; };
    auto blocks_at = [&](int64_t kt) {
        int64_t b = 0;
        for (const WgradOp* op : ops) b += ((positions(op) + kt * 64 - 1) / (kt * 64)) * op->plan.gy * op->plan.gz;
        return b;
    };
    int64_t lo = 1, hi = 1;
    // (fewer than one block per CU leaves whole CUs to the kernels of the backward chain the group runs beside -- its
    //  blocks fill the register file of the CUs they sit on)
    // 192 when the group runs on the side stream (single-call backwards): measured 26.9 -> 26.3 ms; 256 gains nothing there
    const int dma_blocks = e.wg_side_on && cf_side_on() ? 192 : 256;
    while (blocks_at(hi) > dma_blocks) hi *= 2;
    while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (blocks_at(mid) <= dma_blocks) hi = mid; else lo = mid + 1; }
    for (WgradOp* op : ops) {
        const PackSpec& f = e.convs[op->conv].fwd;
        int64_t S = (positions(op) + lo * 64 - 1) / (lo * 64);
        S = std::min<int64_t>(S, std::max<int64_t>(1, ((int64_t)64 << 20) / (wgrad_slab_floats(e, *op) * 4)));
        wgrad_dma_set_split(op->plan, op->g, (int)S, f.kpad, f.wld);
    }
}
// about WGROUP_ROUNDS resident rounds of blocks over all the group's layers, each block owning at least WGROUP_MIN_TILES tiles, so
// deep layers get few slabs and the prologue / slab epilogue is amortised
static void split_tile_group(const stcd_engine& e, int stage, const WgradGroup& G, const std::vector<WgradOp*>& ops) {
    int64_t W = 0;
    for (const WgradOp* op : ops) W += wgrad_ntiles(op->g) * op->plan.gy * op->plan.gz;
    int slots = wgrad_variant_slots(G.kernel, G.lds_bytes);
    // stage 0 of the FC-Siam family runs beside stage 1's chain on a side stream: its grids leave room for the chain's blocks
    // (stage 1's groups keep the full budget: half cost 2 %, a quarter 7 %)
    if (stage == 0 && e.wg_side_on && fc_family(e)) slots = std::max(64, slots / stcd_engine_impl::WG_SIDE_DIV);
    const int64_t rounds = stcd_engine_impl::WGROUP_ROUNDS;
    const int64_t tpb = std::max<int64_t>(stcd_engine_impl::WGROUP_MIN_TILES, (W + rounds * slots - 1) / (rounds * slots));
    for (WgradOp* op : ops) {
        const int64_t slab = wgrad_slab_floats(e, *op);
        int64_t gx = std::max<int64_t>(1, (wgrad_ntiles(op->g) + tpb - 1) / tpb);
        gx = std::min<int64_t>(gx, std::max<int64_t>(1, ((int64_t)32 << 20) / (slab * 4)));
        op->plan.gx = (int)gx;
        op->plan.slab_floats = gx * slab;
    }
}
static void choose_wgroup_splits(stcd_engine& e) {
    for (int st = 0; st < 2; ++st)
        for (size_t gi = 0; gi < e.wgroups[st].size(); ++gi) {
            WgradGroup& G = e.wgroups[st][gi];
            std::vector<WgradOp*> ops;      // its members, in wgrad_ops order
            for (WgradOp* op : e.wgrad_ops)
                if (op->stage == st && op->group == (int)gi) ops.push_back(op);
            for (const WgradOp* op : ops)      // LDS need of the group = max over its jobs
                G.lds_bytes = std::max(G.lds_bytes, wgrad_job_of(e, G.kernel, *op, 0, 0, 0).lds_bytes);
            if (G.kernel.kind == WgradKernel::DMA) split_dma_group(e, ops);
            else if (G.kernel.kind == WgradKernel::TILE) split_tile_group(e, st, G, ops);      // (GEMM: gx is fixed by wgrad_gemm_plan)
        }
}

// step 3: every launch's slabs, in wgrad_ops order, and the job of every grouped launch in its group's table
static void take_wgrad_slabs(stcd_engine& e, Planner& ws) {
    for (WgradOp* op : e.wgrad_ops) {
        if (!op->plan.ok) continue;
        op->slab = ws.take(op->plan.slab_floats * 4);
        if (op->group < 0) continue;
        WgradGroup& G = e.wgroups[op->stage][op->group];
        WgradJob j = wgrad_job_of(e, G.kernel, *op, op->in_off, op->dout_off, op->slab);
        j.start = G.total_blocks;
        G.total_blocks += j.gx * j.gy * j.gz;
        G.jobs.push_back(j);
        double fl, by;
        conv_work(e, op->g, op->kreal, op->nreal, &fl, &by);
        G.flops += fl; G.bytes += by;
    }
}

// step 4: the slab sum of one launch (its `start` is the table's to set), and the table of each stage
static ReduceJob reduce_job_of(const stcd_engine& e, const WgradOp& op) {
    const ConvW& cv = e.convs[op.conv];
    ReduceJob j{};
    j.slab_off = op.slab; j.out_off = cv.w_off;
    j.slab_stride = wgrad_slab_floats(e, op);
    j.gx = op.plan.gx; j.ntaps = op.g.ntaps; j.K = cv.cin; j.N = cv.cout; j.kpad = cv.fwd.kpad; j.wld = cv.fwd.wld;
    j.ks = cv.fwd.ks; j.kn_major = cv.fwd.kn_major;
    wgrad_taps(e, op, j.ky, j.kx);
    j.tiled = (int64_t)j.ntaps * j.K * j.N >= 512 * 1024;     // measured: the tiled form pays from ~0.5 M weights per launch
    if (!j.tiled) {   // index space: blocks of (256 / parts) outputs x parts threads; <= 32 slabs per part where 64 parts allow
        const int64_t outs = (int64_t)j.ntaps * j.K * j.N;
        int parts = 1;
        while (parts < 64 && parts * 32 < j.gx) parts *= 2;
        j.parts = (int8_t)parts;
        const int64_t OUTS = 256 / parts;
        j.count = ((outs + OUTS - 1) / OUTS) * 256;
    } else {   // index space: one block (256 threads) per tile of 32 co x TK ci x taps, all slabs (>= 0.5 M weights: the 32 / 64 MB
        const int TK = j.ntaps == 1 ? 32 : 16;                 // slab caps leave <= 32 of them): see k_reduce_jobs
        const int64_t ntiles = (int64_t)((j.N + 31) / 32) * ((j.K + TK - 1) / TK);
        j.parts = 1;
        j.count = ntiles * 256;
    }
    return j;
}
static int64_t append_reduce_job(std::vector<ReduceJob>& table, int64_t total, ReduceJob j) {
    j.start = total;
    table.push_back(j);
    return total + ((j.count + 255) & ~(int64_t)255);     // block-aligned: one job per block
}
static void build_reduce_tables(stcd_engine& e) {
    for (const WgradOp* op : e.wgrad_ops)
        if (op->plan.ok) e.rjobs_total[op->stage] = append_reduce_job(e.rjobs[op->stage], e.rjobs_total[op->stage], reduce_job_of(e, *op));
}

// step 5: stage 1's table by group: the final group's jobs last, each part counting from 0 (the order of summation of every output is
// its job's own; the split only partitions jobs across launches).  stcd_set_debug bit 1: one table, one launch on the tail.
static void split_reduce_final(stcd_engine& e) {
    const WgradOp* last = e.wg_last_op;
    if (!last || !last->plan.ok || last->group < 0 || last->stage != 1 || (e.debug_flags & 2)) return;
    std::vector<ReduceJob> part[2];
    int64_t tot[2] = {0, 0};
    for (const WgradOp* op : e.wgrad_ops) {      // (the order build_reduce_tables appended them in)
        if (!op->plan.ok || op->stage != 1) continue;
        if (op->group < 0) return;               // a launch of its own: no split
        const int k = op->group == last->group ? 1 : 0;
        tot[k] = append_reduce_job(part[k], tot[k], e.rjobs[1][part[0].size() + part[1].size()]);
    }
    if (part[0].empty() || part[1].empty()) return;
    e.rjobs[1] = part[0];
    e.rjobs[1].insert(e.rjobs[1].end(), part[1].begin(), part[1].end());
    e.rj_split = (int)part[0].size(); e.wg_final_group = last->group;
    e.rj_total_early = tot[0]; e.rj_total_final = tot[1];
}

static void build_wgrad_jobs(stcd_engine& e, Planner& ws) {
    for (int st = 0; st < 2; ++st) { e.rjobs[st].clear(); e.rjobs_total[st] = 0; e.wgroups[st].clear(); }
    e.rj_split = 0; e.wg_final_group = -1; e.rj_total_early = e.rj_total_final = 0;
    if (e.dt == BF16 && e.use_mfma) {
        if (e.use_wgroup) { form_wgroups(e); choose_wgroup_splits(e); }
        take_wgrad_slabs(e, ws);
        build_reduce_tables(e);
        split_reduce_final(e);
        for (int st = 0; st < 2; ++st) {
            e.rjobs_off[st] = ws.take((int64_t)e.rjobs[st].size() * sizeof(ReduceJob) + 16);
            for (WgradGroup& G : e.wgroups[st]) G.table_off = ws.take((int64_t)G.jobs.size() * sizeof(WgradJob) + 16);
        }
    }
    for (int st = 0; st < 2; ++st) e.wrun.groups[st].assign(e.wgroups[st].size(), WgradRun::Group());
}

// one repack launch per forward: the filter job tables (uploaded to the workspace on first use)
static void build_filter_pack_jobs(stcd_engine& e, Planner& ws) {
    for (int with_dgrad = 0; with_dgrad < 2; ++with_dgrad) {
        std::vector<PackJob>& jobs = e.jobs[with_dgrad];
        jobs.clear();
        int64_t cur = 0;
        // every job starts on a 256-element boundary: a block then belongs to ONE job and finds it with scalar loads
        auto push = [&](PackJob j) { j.start = cur; cur += (j.count + 255) & ~(int64_t)255; jobs.push_back(j); };
        const bool mfma = e.dt == BF16 && e.use_mfma;
        if (!mfma) {
            for (auto& cv : e.convs)
                for (int d = 0; d <= with_dgrad; ++d) {
                    const PackSpec& ps = d ? cv.dgrad : cv.fwd;
                    if (!ps.ntaps) continue;
                    PackJob j{};
                    j.kind = 0; j.ps = ps; j.src_off = cv.w_off; j.dst_off = d ? cv.wpk_dgrad : cv.wpk_fwd;
                    j.count = (int64_t)ps.ntaps * ps.kpad * ps.wld;
                    push(j);
                }
        } else {
            for (const ConvOp* op : e.conv_ops) {
                if (op->dgrad && !with_dgrad) continue;
                const ConvW& cv = e.convs[op->conv];
                const PackSpec& full = op->dgrad ? cv.dgrad : cv.fwd;
                PackJob j{};
                j.ps = full;
                j.ps.ntaps = op->g.ntaps;
                for (int t = 0; t < op->g.ntaps; ++t) { j.ps.ky[t] = full.ky[op->tap0 + t]; j.ps.kx[t] = full.kx[op->tap0 + t]; }
                j.src_off = cv.w_off;
                if (cv.kind == K_STEM7) {          // the stem's forward as a 7-tap GEMM over 8-pixel rows (configure_segcd)
                    j.kind = 2; j.dst_off = op->wf; j.count = op->plan.wf_elems;
                    j.Co = cv.cout; j.NTtot = op->plan.NTtot; j.aux = cv.cin;
                    push(j);
                    continue;
                }
                if (!conv_on_ref(true, *op)) {
                    j.kind = 1; j.dst_off = op->wf;
                    j.count = op->plan.modeB ? op->plan.wf_elems : op->plan.wf_elems / op->g.ntaps;      // mode A: one thread per (ci, co), all taps
                    j.Ci = op->g.ci; j.Co = op->g.co; j.CiB = op->plan.CiB; j.nchunks = op->plan.nchunks; j.KS = op->plan.KS;
                    j.NTtot = op->plan.NTtot; j.modeB = op->plan.modeB;
                } else {   // no MFMA plan for this launch: it runs on the reference kernel (conv_kernel) and needs the fp32 image
                    j.kind = 0;
                    j.dst_off = (op->dgrad ? cv.wpk_dgrad : cv.wpk_fwd) + (int64_t)op->tap0 * full.kpad * full.wld * 4;
                    j.count = (int64_t)j.ps.ntaps * full.kpad * full.wld;
                }
                push(j);
            }
        }
        e.jobs_total[with_dgrad] = cur;
        e.jobs_off[with_dgrad] = ws.take((int64_t)jobs.size() * sizeof(PackJob) + 16);
    }
}

static int configure_fcsiam(stcd_engine& e, int B, int H, int W) {
    const int64_t T = (int64_t)dsize(e.dt);
    const int ND = fc_dates(e);            // encoder streams (dates) stacked in the batch dimension
    e.Hs[0] = H; e.Ws[0] = W;
    for (int s = 0; s < 4; ++s) { e.Hs[s + 1] = e.Hs[s] / 2; e.Ws[s + 1] = e.Ws[s] / 2; }
    Planner ws(e);
    auto add_drop = [&](const std::string& name, int rows, int C) {
        DropP d; d.name = name; d.rows = rows; d.C = C; d.off = e.drop_floats;
        e.drop_floats += (int64_t)rows * C;
        e.drops.push_back(d);
        return (int)e.drops.size() - 1;
    };

    e.X0 = ws.plain(ND * B, H, W, 8);
    // concat buffers first (conc keeps its skips inside them)
    for (int s = 0; s < 4; ++s) {
        int Cd = ENC_C[s] + (e.arch == STCD_ARCH_CONC ? 2 : 1) * ENC_C[s];
        e.D[s] = ws.plain(B, e.Hs[s], e.Ws[s], Cd);
        e.dD[s] = ws.plain(B, e.Hs[s], e.Ws[s], Cd);
        e.P[s] = ws.plain(ND * B, e.Hs[s + 1], e.Ws[s + 1], ENC_C[s]);
        e.dP[s] = ws.plain(ND * B, e.Hs[s + 1], e.Ws[s + 1], ENC_C[s]);
    }
    // ---- zero arena, directly behind dP[3] (whose date-0 half must read as zero: the reference's T1 bottleneck pool is
    //      dead work, SiamUnet_diff.py:119 overwritten at :143; the date-1 half is rewritten by upconv4's data gradient):
    //      BatchNorm accumulators of every layer (forward + backward) and the bias-gradient accumulators.
    //      ONE walk over the model tables hands out the slices, in slice order: it runs here from offset 0 to size the arena (the
    //      layers do not exist yet, nothing is assigned) and again from the arena's offset once they do -- a slice the first run
    //      did not count cannot be handed out by the second.
    auto r256 = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    auto zero_arena = [&](int64_t at, bool assign) {
        auto acc = [&](int groups, int C) { const int64_t o = at; at += r256(bn_acc_bytes(groups, C)); return o; };
        for (int s = 0; s < 4 && fc_cross(e); ++s) {      // two BatchNorms per cross_conc block
            const int C = ENC_C[s];
            const int64_t a[4] = {acc(1, C), acc(1, C), acc(1, C), acc(1, C)};
            if (assign) { XConc& X = e.xc[s]; X.facc1 = a[0]; X.bacc1 = a[1]; X.res.facc = a[2]; X.res.bacc = a[3]; }
        }
        size_t li = 0;
        for (int s = 0; s < 4; ++s)
            for (int j = 0; j < ENC_STAGE_CONVS[s]; ++j, ++li) {
                const int64_t a[2] = {acc(ND, ENC_C[s]), acc(ND, ENC_C[s])};
                if (assign) { e.enc[li].facc = a[0]; e.enc[li].bacc = a[1]; }
            }
        li = 0;
        for (int k = 0; k < 4; ++k)
            for (int j = 0; j < DEC[k].n; ++j) {
                if (DEC[k].cout[j] < 0) continue;
                const int64_t a[2] = {acc(1, DEC[k].cout[j]), acc(1, DEC[k].cout[j])};
                if (assign) { e.dec[li].facc = a[0]; e.dec[li].bacc = a[1]; }
                ++li;
            }
        for (int k = 0; k < 4; ++k) {
            const int64_t a = acc(1, DEC[k].C);
            if (assign) e.ups[k].bias_acc = a;
        }
        const int64_t a = acc(1, 8);
        if (assign) e.final_bias_acc = a;
        return at;
    };
    int64_t arena_bytes = zero_arena(0, false);
    // (FC-EF's one encoder stream has one BatchNorm group per layer; its arena is sized like the two-date families', the slack at its
    //  end -- the size tests/golden/plan_layout.json records)
    for (int s = 0; s < 4; ++s) arena_bytes += 2 * ENC_STAGE_CONVS[s] * (r256(bn_acc_bytes(2, ENC_C[s])) - r256(bn_acc_bytes(ND, ENC_C[s])));
    e.zero_begin = e.dP[3].off;
    const int64_t arena_off = ws.take(arena_bytes);
    e.zero_end = arena_off + arena_bytes;
    // ---- encoder
    for (int s = 0; s < 4; ++s) {
        const int C = ENC_C[s], h = e.Hs[s], w = e.Ws[s];
        for (int j = 0; j < ENC_STAGE_CONVS[s]; ++j) {
            std::string sfx = std::to_string(s + 1) + std::to_string(j + 1);
            Cbrd L;
            L.conv = conv_index(e, "conv" + sfx);
            L.bn = bn_index(e, "bn" + sfx);
            L.drop = add_drop("do" + sfx, ND * B, C);
            L.N = ND * B; L.H = h; L.W = w; L.groups = ND; L.npg = B;
            const bool first = j == 0, last = j == ENC_STAGE_CONVS[s] - 1;
            if (first && s == 0) { L.in = e.X0; L.K = 8; }
            else if (first) { L.in = e.P[s - 1]; L.K = ENC_C[s - 1]; }
            else { L.in.off = e.enc.back().A.off; L.in.ld = C; L.K = C; }
            L.Y = ws.plain(ND * B, h, w, C);
            if (last && fc_concat_skips(e)) {
                L.A.off = e.D[s].off + C * T; L.A.ld = e.D[s].ld; L.A.goff = C;
                L.dA.off = e.dD[s].off + C * T; L.dA.ld = e.dD[s].ld; L.dA.goff = C;
                L.dY = ws.plain(ND * B, h, w, C);
            } else {
                TRef a = ws.plain(ND * B, h, w, C), da = ws.plain(ND * B, h, w, C);
                L.A.off = a.off; L.A.ld = C; L.A.goff = (int64_t)B * h * w * C;
                L.dA.off = da.off; L.dA.ld = C; L.dA.goff = L.A.goff;
                L.dY = da;   // in place
            }
            if (last) { L.pool = true; L.P = e.P[s]; L.dPool = e.dP[s]; }
            if (last && !fc_concat_skips(e) && !fc_cross(e)) { L.fuse_dst.off = e.D[s].off + C * T; L.fuse_dst.ld = e.D[s].ld; }
            if (first && s == 0) L.has_dIn = false;
            else if (first) { L.has_dIn = true; L.dIn = e.dP[s - 1]; }
            else { L.has_dIn = true; L.dIn.off = e.enc.back().dA.off; L.dIn.ld = C; }
            L.stat = ws.take((int64_t)2 * 4 * C * 4);
            e.enc.push_back(L);
        }
    }
    // ---- decoder
    // T2 half of the last pool (FC-EF: the one stream's)
    TRef prevA = {e.P[3].off + (int64_t)(fc_dates(e) - 1) * B * e.Hs[4] * e.Ws[4] * ENC_C[3] * T, ENC_C[3]};
    TRef prevdA = {e.dP[3].off + (int64_t)(fc_dates(e) - 1) * B * e.Hs[4] * e.Ws[4] * ENC_C[3] * T, ENC_C[3]};
    for (int k = 0; k < 4; ++k) {
        const DecSpec& d = DEC[k];
        const int s = 3 - k, h = e.Hs[s], w = e.Ws[s];
        UpConv U;
        U.conv = conv_index(e, d.up); U.level = s; U.N = B; U.h = e.Hs[s + 1]; U.w = e.Ws[s + 1]; U.Ho = h; U.Wo = w; U.C = d.C;
        U.in = prevA; U.dIn = prevdA;
        U.out = e.D[s]; U.dOut = e.dD[s];
        e.ups.push_back(U);
        TRef in = e.D[s], dIn = e.dD[s];
        int K = e.D[s].ld;
        for (int j = 0; j < d.n; ++j) {
            if (d.cout[j] < 0) {   // conv11d: no BN, writes the logits
                e.final_conv = conv_index(e, "conv11d");
                e.finalIn = in; e.dFinalIn = dIn;
                break;
            }
            Cbrd L;
            L.conv = conv_index(e, std::string("conv") + d.sfx[j]);
            L.bn = bn_index(e, std::string("bn") + d.sfx[j]);
            L.drop = add_drop(std::string("do") + d.sfx[j], B, d.cout[j]);
            const int C = d.cout[j];
            L.N = B; L.H = h; L.W = w; L.groups = 1; L.npg = B;
            L.in = in; L.K = K;
            L.Y = ws.plain(B, h, w, C);
            TRef a = ws.plain(B, h, w, C), da = ws.plain(B, h, w, C);
            L.A.off = a.off; L.A.ld = C; L.A.goff = 0;
            L.dA.off = da.off; L.dA.ld = C; L.dA.goff = 0;
            L.dY = da;
            L.has_dIn = true; L.dIn = dIn;
            L.stat = ws.take((int64_t)4 * C * 4);
            e.dec.push_back(L);
            in = a; dIn = da; K = C;
            prevA = a; prevdA = da;
        }
    }
    if (fc_cross(e)) {      // the cross_conc block of every level: pairwise depthwise conv + BN + ReLU, then a dropout-free Cbrd whose
        for (int s = 0; s < 4; ++s) {       // activation IS the skip slice of the level's concat buffer
            XConc& X = e.xc[s];
            const int C = ENC_C[s], h = e.Hs[s], w = e.Ws[s];
            X.G = ws.plain(B, h, w, C); X.dG = ws.plain(B, h, w, C); X.R = ws.plain(B, h, w, C); X.dR = ws.plain(B, h, w, C);
            X.stat1 = ws.take((int64_t)4 * C * 4);
            X.part = ws.take(pairdw_partial_floats(B, h, w, C) * 4);
            Cbrd& L = X.res;
            L.drop = -1; L.N = B; L.H = h; L.W = w; L.groups = 1; L.npg = B;
            L.in = X.R; L.K = C;
            L.Y = ws.plain(B, h, w, C);
            L.A.off = e.D[s].off + C * T; L.A.ld = e.D[s].ld; L.A.goff = 0;
            L.dA.off = e.dD[s].off + C * T; L.dA.ld = e.dD[s].ld; L.dA.goff = 0;
            L.dY = ws.plain(B, h, w, C);
            L.has_dIn = true; L.dIn = X.dR;
            L.stat = ws.take((int64_t)4 * C * 4);
        }
    }
    e.G = ws.plain(B, H, W, 8);
    zero_arena(arena_off, true);
    e.scratch8 = ws.take(256);
    e.masks = ws.take(e.drop_floats * 4);
    take_ref_images(e, ws);

    // ---- bind every conv-shaped launch (geometry, filter, MFMA plan); the layer vectors are final from here on
    const Binder bind{e, ws, true};
    auto wg_stage = [&](int conv) { return e.convs[conv].w_off < e.enc_param_end ? 1 : 0; };     // encoder filters are finalised by stage 1
    auto bind_cbrd = [&](Cbrd& L) {
        const ConvW& cv = e.convs[L.conv];
        bind.conv(L.fwd, geom3(L.N, L.H, L.W, L.K, L.in.ld, cv.cout, L.Y.ld), L.conv, false, 0, cv.cin, cv.cout, L.groups);
        bind.wgrad(L.wg, geom3(L.N, L.H, L.W, L.K, L.in.ld, cv.cout, L.dY.ld), L.conv, L.in.off, L.dY.off, wg_stage(L.conv));
        if (L.has_dIn)      // (tiles partitioned by the layer's BatchNorm groups: its data gradient may carry the previous layer's backward sums)
            bind.conv(L.dgr, geom3(L.N, L.H, L.W, cv.dgrad.kpad, L.dY.ld, cv.cin, L.dIn.ld), L.conv, true, 0, cv.cout, cv.cin,
                      (e.use_bwdsum && e.use_bwdsum_res) ? L.groups : 1);
    };
    for (auto& L : e.enc) bind_cbrd(L);
    for (auto& L : e.dec) bind_cbrd(L);
    for (auto& X : e.xc) bind_cbrd(X.res);
    for (auto& U : e.ups) {
        const ConvW& cv = e.convs[U.conv];
        for (int ph = 0; ph < 4; ++ph) {
            int tap0;
            const stcd_conv_geom g = geom_phase3(U.N, U.h, U.w, U.C, U.in.ld, U.Ho, U.Wo, U.C, U.out.ld, ph, cv.fwd, &tap0);
            bind.conv(U.fwd[ph], g, U.conv, false, tap0, U.C, U.C);
            bind.wgrad(U.wg[ph], g, U.conv, U.in.off, U.dOut.off, wg_stage(U.conv), tap0);
        }
        // data gradient: 3x3 stride-2 conv over dOut, whose buffer may carry replication-padded rows / columns (geom_gather2)
        bind.conv(U.dgr, geom_gather2(U.N, U.Ho, U.Wo, cv.dgrad.kpad, U.dOut.ld, U.h, U.w, U.C, U.dIn.ld, cv.dgrad, 1), U.conv, true, 0, U.C, U.C);
    }
    {
        const ConvW& cv = e.convs[e.final_conv];
        bind.conv(e.final_fwd, geom3(B, H, W, cv.kin_p, e.finalIn.ld, e.label, e.label), e.final_conv, false, 0, cv.cin, e.label);
        bind.wgrad(e.final_wg, geom3(B, H, W, cv.kin_p, e.finalIn.ld, e.label, 8), e.final_conv, e.finalIn.off, e.G.off, wg_stage(e.final_conv));
        bind.conv(e.final_dgr, geom3(B, H, W, cv.dgrad.kpad, 8, cv.cin, e.dFinalIn.ld), e.final_conv, true, 0, e.label, cv.cin);
    }
    e.slab = ws.take(e.slab_floats * 4);

    // ---- BatchNorm-backward sums inside the data gradient that produces dA (k_conv_small<.., BWD>): layer N's data gradient writes
    //      dA of layer P (plain buffer, same map, 16 channels); P then skips its k_bn_reduce launch.  Level-1 layers only (the
    //      small-channel kernel): conv12 -> conv11, conv11d -> conv12d, the final conv -> conv11d.
    for (auto& L : e.enc) { L.dgr_bwd = nullptr; L.bwd_sums_fused = false; }
    for (auto& L : e.dec) { L.dgr_bwd = nullptr; L.bwd_sums_fused = false; }
    e.final_dgr_bwd = nullptr;
    if (e.use_bwdsum && e.dt == BF16 && e.use_mfma && e.use_small && !e.use_virt) {
        // STCD_BWDSUM_RES=1: also the layers behind a k_conv_res data gradient (k_conv_res<.., BWD>, one or two n-tiles).  Measured: eight
        // more launches gone (114 -> 106), bn_bwd_reduce 0.150 -> 0.055 ms, conv 0.970 -> 1.052 ms: the step 2.094 -> 2.114 ms (diff), conc
        // 2.433 -> 2.475 -- the resident-filter kernel pays more for 56 extra registers and the Y loads than the small launches cost.  Opt-in.
        const int res_too = e.use_bwdsum_res;
        auto dest_ok = [&](const Cbrd& P, const ConvOp& dgr, int64_t dIn_off, int dIn_ld, int N) {
            const bool kern = (dgr.small && conv_small_bwdsum_ok(dgr.g)) ||
                              (res_too && !dgr.small && !dgr.gemm.ok && e.use_res && dgr.res.ok && dgr.res_groups == P.groups &&
                               conv_res_bwdsum_ok(dgr.g, dgr.res));
            return !P.pool && P.fuse_dst.off < 0 && !P.virt && kern && dgr.wf >= 0 && dIn_off == P.dA.off && dIn_ld == P.dA.ld &&
                   e.convs[P.conv].cout == dgr.g.co && P.N == N && N % P.groups == 0 &&
                   (P.groups == 1 || P.dA.goff == (int64_t)P.npg * P.H * P.W * P.dA.ld);
        };
        auto scan = [&](std::vector<Cbrd>& v) {
            for (size_t i = 1; i < v.size(); ++i) {
                Cbrd& N = v[i]; Cbrd& P = v[i - 1];
                if (N.has_dIn && N.dgr_sum_acc < 0 && dest_ok(P, N.dgr, N.dIn.off, N.dIn.ld, N.N)) { N.dgr_bwd = &P; P.bwd_sums_fused = true; }
            }
        };
        scan(e.enc); scan(e.dec);
        if (!e.dec.empty() && dest_ok(e.dec.back(), e.final_dgr, e.dFinalIn.off, e.dFinalIn.ld, e.dec.back().N)) {
            e.final_dgr_bwd = &e.dec.back(); e.dec.back().bwd_sums_fused = true;
        }
    }

    // ---- virtual activations: a non-skip layer whose ONLY reader is the next conv of its stage hands that conv its raw output Y;
    //      the conv's forward launch (k_conv_small / k_conv_res, XF variants) and its weight gradient (k_wgrad_group, job.xf_*)
    //      apply BN-affine + ReLU + Dropout2d while staging.  Eligibility mirrors exec_conv / exec_wgrad's kernel choice, which is
    //      fixed at configure time (the switches are read at stcd_create).
    e.final_xsrc = nullptr; e.fc_virt_layers = 0;
    for (auto& L : e.enc) { L.virt = false; L.xsrc = nullptr; }
    for (auto& L : e.dec) { L.virt = false; L.xsrc = nullptr; }
    if (e.use_virt && e.dt == BF16 && e.use_mfma && e.use_wgroup && !fc_cross(e)) {
        auto fwd_ok = [&](const ConvOp& op, bool nchw) {
            if (op.wf < 0 || (op.gemm.ok && !nchw)) return false;
            if (op.small && e.use_small) return true;
            return op.res.ok && !nchw && !op.res.single_halo;
        };
        auto wg_ok = [&](const WgradOp& op) { return op.plan.ok && wgrad_kernel_takes_xf(wgrad_kernel_of(op.plan, op.g, true)); };
        auto link = [&](Cbrd& P, ConvOp& cf, WgradOp& cw, bool nchw) {
            if (P.pool || P.fuse_dst.off >= 0) return false;
            if (!fwd_ok(cf, nchw) || !wg_ok(cw)) return false;
            P.virt = true; ++e.fc_virt_layers;
            cw.in_off = P.Y.off;
            cw.xf = WgradXf{P.stat, (P.drop >= 0) ? e.masks + e.drops[P.drop].off * 4 : -1, e.convs[P.conv].cout, P.groups, P.npg};
            return true;
        };
        for (size_t i = 0; i + 1 < e.enc.size(); ++i) {
            Cbrd& P = e.enc[i]; Cbrd& Cn = e.enc[i + 1];
            if (Cn.in.off != P.A.off) continue;                       // (the next layer reads the pooled map: P is a skip layer)
            if (link(P, Cn.fwd, Cn.wg, false)) { Cn.xsrc = &P; Cn.in.off = P.Y.off; Cn.in.ld = P.Y.ld; }
        }
        for (size_t i = 0; i < e.dec.size(); ++i) {
            Cbrd& P = e.dec[i];
            if (i + 1 < e.dec.size() && e.dec[i + 1].in.off == P.A.off) {
                Cbrd& Cn = e.dec[i + 1];
                if (link(P, Cn.fwd, Cn.wg, false)) { Cn.xsrc = &P; Cn.in.off = P.Y.off; Cn.in.ld = P.Y.ld; }
            } else if (e.finalIn.off == P.A.off) {
                if (link(P, e.final_fwd, e.final_wg, true)) { e.final_xsrc = &P; e.finalIn.off = P.Y.off; e.finalIn.ld = P.Y.ld; }
            }
        }
    }

    // ---- bias gradients without a pass of their own: the transposed conv of stage k wrote channels [0, C) of the concat
    //      buffer, so its bias gradient is the per-channel sum of that slice of d(concat) -- which the data-gradient launch
    //      of the stage's first conv produces.  When that launch runs on the resident-filter kernel it sums the slice in its
    //      epilogue (integer accumulators, as the BatchNorm statistics); one k_bias_finish launch per backward converts.
    {
        size_t di = 0;
        for (int k = 0; k < 4; ++k) {
            UpConv& U = e.ups[k];
            Cbrd& L = e.dec[di];
            int nb = 0;
            for (int j = 0; j < DEC[k].n; ++j) nb += DEC[k].cout[j] >= 0;
            di += nb;
            U.bias_fused = false;
            const bool even = 2 * U.h == U.Ho && 2 * U.w == U.Wo;
            if (e.dt == BF16 && e.use_mfma && nb > 0 && L.has_dIn && L.dIn.off == U.dOut.off && L.dgr.res.ok && L.dgr.wf >= 0 && even) {
                U.bias_fused = true;
                L.dgr_sum_acc = U.bias_acc; L.dgr_sum_c0 = 0; L.dgr_sum_C = U.C;
            }
            // fused or not, the bf16 path sums the bias gradient in the integer accumulator (deterministic)
            if (e.dt == BF16) ws.bias_job(U.bias_acc, U.conv, U.C, U.C);
        }
        ws.bias_job(e.final_bias_acc, e.final_conv, 8, e.label);
    }

    // test introspection (stcd_ws_tensor_*): input, conv output, activation (per date: the two halves may sit in different
    // buffers) and output gradient of every conv + BN layer, as they stand after a forward / backward
    auto rec_layer = [&](const Cbrd& L) {
        const ConvW& cv = e.convs[L.conv];
        // "in.virt": the input is the producer's RAW conv output (virtual activation); the producer then records no A
        ws.tensor(cv.name + (L.xsrc ? ".in.virt" : ".in"), L.in, L.N, L.H, L.W, L.K);
        ws.tensor(cv.name + ".Y", L.Y, L.N, L.H, L.W, cv.cout);
        for (int g = 0; g < L.groups && !L.virt && !skip_recomputed(e, L); ++g)
            ws.tensor(cv.name + ".A.g" + std::to_string(g), L.A.off + g * L.A.goff * T, L.A.ld, L.npg, L.H, L.W, cv.cout);
        ws.tensor(cv.name + ".dY", L.dY, L.N, L.H, L.W, cv.cout);
    };
    for (const Cbrd& L : e.enc) rec_layer(L);
    for (const Cbrd& L : e.dec) rec_layer(L);
    for (const XConc& X : e.xc) {      // cross_conc block: the pairwise conv as a layer of its own (Y = G, A = R, dY = dG), then conv_res
        const std::string n = "cross_conc" + std::to_string(X.level + 1) + ".diff.0.";
        const Cbrd& R = X.res;
        ws.tensor(n + "Y", X.G, R.N, R.H, R.W, X.C); ws.tensor(n + "A.g0", X.R, R.N, R.H, R.W, X.C); ws.tensor(n + "dY", X.dG, R.N, R.H, R.W, X.C);
        rec_layer(R);
    }

    e.wg_last_op = &e.enc[0].wg;      // conv11's weight gradient: the last launch the backward chain makes ready
    ws.tables();
    // k_step_prologue writes the masks, the filter images, the zero range and the packed input from one grid, in no order: the four
    // outputs must not overlap (byte ranges of the workspace)
    {
        struct Rng { int64_t a, b; const char* what; };
        std::vector<Rng> out;
        out.push_back({e.X0.off, e.X0.off + (int64_t)ND * B * H * W * 8 * T, "packed input"});
        out.push_back({e.zero_begin, e.zero_end, "zero range"});
        if (e.drop_floats > 0) out.push_back({e.masks, e.masks + e.drop_floats * 4, "dropout masks"});
        const size_t fixed = out.size();
        for (const PackJob& j : e.jobs[1]) {
            const int64_t bytes = pack_job_bytes(j);
            if (bytes < 0) { set_error("internal: a filter pack job of a kind pack_job_bytes does not size"); return 1; }
            out.push_back({j.dst_off, j.dst_off + bytes, "filter image"});
        }
        for (size_t i = 0; i < fixed; ++i)
            for (size_t k = i + 1; k < out.size(); ++k)
                if (out[i].a < out[k].b && out[k].a < out[i].b) {
                    set_error(std::string("internal: the step prologue's outputs overlap (") + out[i].what + " / " + out[k].what + ")");
                    return 1;
                }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ execution helpers
struct Ctx {
    stcd_engine& e;
    char* ws;
    const float* params;
    float* grads;
    hipStream_t s;
    template <typename P = void> P* at(int64_t off) const { return (P*)(ws + off); }
};

struct ProfScope {
    Prof& p; hipStream_t s; bool on; hipEvent_t b;
    ProfScope(const Ctx& c, int klass, double flops, double bytes, const char* kernel = nullptr);
    ~ProfScope() { if (on) (void)hipEventRecord(b, s); }
};

ProfScope::ProfScope(const Ctx& c, int klass, double flops, double bytes, const char* kernel)
    : p(c.e.prof), s(c.s), on(c.e.prof.on), b(nullptr) {
    if (!on) return;
    static const char* DEF[PC_COUNT] = {"k_conv", "k_wgrad", "k_bn_reduce<T, 0>", "k_bn_act", "k_bn_reduce<T, 1>", "k_bn_bwd_apply",
                                        "k_pool_bwd|k_fuse|k_slice", "k_pack_jobs|k_reduce_dw"};
    ProfRec r;
    r.a = p.get(); r.b = p.get(); r.klass = klass; r.flops = flops; r.bytes = bytes;
    r.name_id = p.intern(kernel ? kernel : DEF[klass]);
    b = r.b;
    p.recs.push_back(r);
    (void)hipEventRecord(r.a, s);
}

// algorithmic work of one conv-like launch: flops = 2 MACs over real channels,
// bytes = (input + output + weights) * sizeof(T), each tensor counted once.
static void conv_work(const stcd_engine& e, const stcd_conv_geom& g, int kreal, int nreal, double* flops, double* bytes) {
    double pos = (double)g.n * g.hm * g.wm;
    *flops = 2.0 * pos * g.ntaps * kreal * nreal;
    double in_px = g.in_stride == 1 ? pos : (double)g.n * (2.0 * g.hm) * (2.0 * g.wm);
    *bytes = (in_px * kreal + pos * nreal + (double)g.ntaps * kreal * nreal) * (double)dsize(e.dt);
}

static bool mfma_on(const stcd_engine& e) { return e.dt == BF16 && e.use_mfma; }

// ---- which kernel a conv-shaped launch runs on.  The CHOICE is made here and nowhere else, and the one switch that launches the
//      answer is launch_conv below: exec_conv and the per-op ABI (stcd_op_conv, stcd_op_conv_fused) all go through it, and a launcher
//      that then rejects is an error, not a reason to try the next kernel.  The plans conv_kernel reads were made by plan_conv at
//      configure time; the precedence is the table in DESIGN.md section 3, and where it depends on what a kernel can take, that is
//      read from conv_caps (common.h): a kernel without fused sums or NCHW output is passed over by a call that needs them.
//      (A ConvEpi does not steer the choice: exec_conv reports it as not fused and the caller runs it element-wise.)
constexpr unsigned conv_kernel_bit(ConvKernel k) { return 1u << (int)k; }
// tile groups of a k_conv_small launch: the destination layer's for a BwdSum; a virtual input partitions the tiles by the PRODUCER's
// BatchNorm groups, statistics or not (eval mode has none); else the groups of the BatchNorm statistics it sums
static int conv_small_groups(const ConvArgs& a, int co) {
    return a.bs ? a.bs->groups : a.xf_on() ? a.xf->groups : (a.sums.acc && a.bn_form(co)) ? a.sums.groups : 1;
}
// allowed: conv_kernel_bit mask of the kernels the caller can run
static ConvKernel conv_kernel(bool mfma, bool use_small, const ConvOp& op, const ConvArgs& a, unsigned allowed = ~0u) {
    auto may = [&](ConvKernel x) { return (allowed & conv_kernel_bit(x)) != 0; };
    auto takes = [](ConvKernel x, unsigned need) { return (need & ~conv_caps(x)) == 0; };
    if (conv_on_ref(mfma, op)) return ConvKernel::REF;
    const unsigned nchw = a.nchw ? CAP_NCHW : 0, sums = a.sums.acc ? CAP_SUMS : 0, xf = a.xf_on() ? CAP_XF : 0;
    const unsigned grp = op.res_groups > 1 ? CAP_GROUPS : 0;
    const bool small = op.small && use_small;
    if (a.bs) return small ? ConvKernel::SMALL : ConvKernel::RES;
    if (op.gemm.ok && takes(ConvKernel::GEMM, nchw)) {
        if (op.dma.ok && takes(ConvKernel::DMA, grp | sums) && may(ConvKernel::DMA)) return ConvKernel::DMA;
        if (op.halo.ok && takes(ConvKernel::HALO, sums) && may(ConvKernel::HALO)) return ConvKernel::HALO;
        return ConvKernel::GEMM;
    }
    if (small && conv_small_call_ok(op.g, conv_small_groups(a, op.g.co), a.xf)) return ConvKernel::SMALL;
    if (op.res.ok && takes(ConvKernel::RES, nchw) && !small) {
        if (op.tile.ok && takes(ConvKernel::TILE, xf) && may(ConvKernel::TILE)) return ConvKernel::TILE;
        if (!xf || conv_res_xf_ok(op.g, op.res, op.res_groups, *a.xf)) return ConvKernel::RES;
    }
    return ConvKernel::MFMA;
}
// the name rocprofv3 prints for the choice (bench.py and the committed profile tables key on these strings)
static void conv_kernel_name(ConvKernel kern, const ConvOp& op, bool bwd, char (&kname)[64]) {
    switch (kern) {
        case ConvKernel::DMA: snprintf(kname, sizeof(kname), "k_conv_dma"); break;
        case ConvKernel::HALO: snprintf(kname, sizeof(kname), "k_conv_halo"); break;
        case ConvKernel::GEMM:
            if (op.gemm.pix_chunks) snprintf(kname, sizeof(kname), "k_conv_gemm<stem>");
            else snprintf(kname, sizeof(kname), "k_conv_gemm<%d>", op.gemm.W);
            break;
        case ConvKernel::TILE: snprintf(kname, sizeof(kname), "k_conv_tile<%d>", op.tile.NT); break;
        case ConvKernel::RES:
            if (bwd) snprintf(kname, sizeof(kname), "k_conv_res<bwd>");
            else snprintf(kname, sizeof(kname), "k_conv_res<%d, %d, %s>", op.res.NT, op.res.CW, op.res.single_halo ? "true" : "false");
            break;
        case ConvKernel::SMALL:
            if (bwd) snprintf(kname, sizeof(kname), "k_conv_small<bwd>");
            else snprintf(kname, sizeof(kname), "k_conv_small<1, %d>", (op.g.ntaps * op.g.ci + 31) / 32 <= 5 ? 5 : 9);
            break;
        case ConvKernel::MFMA: snprintf(kname, sizeof(kname), "k_conv_mfma<%d>", op.plan.NT); break;
        case ConvKernel::REF: snprintf(kname, sizeof(kname), "k_conv_ref"); break;
    }
}

// THE switch that launches a chosen kernel: `a` as the kernel is to run it (a.wf its filter image, a.groups its tile groups).
// 1: the kernel cannot deliver something `a` asks (conv_refusal) or its launcher rejected the plan / shape; nothing was launched.
static int launch_conv(ConvKernel kern, const ConvOp& op, const ConvArgs& args) {
    if (conv_refusal(kern, args, op.g.co)) return 1;
    ConvArgs a = args;
    if (!a.sums.acc) { a.sums = StatReq(); a.sums.C = op.g.co; }      // (what the kernels' argument structs hold without a request)
    switch (kern) {
        case ConvKernel::DMA: return launch_conv_dma(op.g, op.plan, op.dma, a);
        case ConvKernel::HALO: return launch_conv_halo(op.g, op.plan, op.halo, a);
        case ConvKernel::GEMM: return launch_conv_gemm(op.g, op.plan, op.gemm, a);
        case ConvKernel::SMALL: return launch_conv_small(op.g, a);
        case ConvKernel::TILE: return launch_conv_tile(op.g, op.plan, op.tile, a);
        case ConvKernel::RES: return launch_conv_res(op.g, op.plan, op.res, a);
        case ConvKernel::MFMA: return launch_conv_mfma(op.g, op.plan, a);
        case ConvKernel::REF: break;      // (reads the fp32 filter image, not a.wf: exec_conv, stcd_op_conv)
    }
    return 1;
}

// What exec_conv delivered of what the caller asked to have fused; the caller runs the separate pass for the rest.  The rules:
//   sums: by a kernel with CAP_SUMS, and only when the request's groups equal the launch's -- the plan's (res_groups), or for
//         k_conv_small its own rule (conv_small_groups); k_conv_small sums only full-channel BatchNorm-form requests (no
//         CAP_SUM_SLICE).  With a BwdSum the launch sums the backward terms instead (their scales, all channels): not delivered.
//   epi:  by a kernel with CAP_EPI.
struct ConvDone { bool sums = false, epi = false; };
static ConvArgs conv_args(const void* in, void* out, const float* bias = nullptr, bool nchw = false) {
    ConvArgs a;
    a.in = in; a.out = out; a.bias = bias; a.nchw = nchw;
    return a;
}
// args: in / bias / out / nchw and the features asked for; wf, groups and the stream are filled in here
static ConvDone exec_conv(const Ctx& c, const ConvOp& op, const ConvArgs& args) {
    const ConvW& cv = c.e.convs[op.conv];
    const ConvKernel kern = conv_kernel(mfma_on(c.e), c.e.use_small, op, args);
    const unsigned caps = conv_caps(kern);
    char kname[64];
    conv_kernel_name(kern, op, args.bs != nullptr, kname);
    ProfScope prof(c, PC_CONV, op.flops, op.bytes + (args.bs ? (double)op.g.n * op.g.ho * op.g.wo * op.g.co * 2.0 : 0.0), kname);
    ConvDone done;
    if (args.xf_on() && !(caps & CAP_XF)) {
        // planned at configure time for a kernel that applies the transform: no other can (and none may run on raw Y)
        set_error("internal: a virtual-activation input reached a convolution kernel without the staging transform");
        return done;
    }
    ConvArgs a = args;
    a.s = c.s;
    if (kern == ConvKernel::REF) {
        const PackSpec& ps = op.dgrad ? cv.dgrad : cv.fwd;
        const float* w = c.at<float>(op.dgrad ? cv.wpk_dgrad : cv.wpk_fwd) + (int64_t)op.tap0 * ps.kpad * ps.wld;
        launch_conv_ref(c.e.dt, op.g, a.in, w, ps.kpad, ps.wld, a.bias, a.out, a.nchw, a.s);
        return done;
    }
    a.wf = op.wf >= 0 ? c.at(op.wf) : nullptr;
    a.groups = !(caps & CAP_GROUPS) ? 1 : kern == ConvKernel::SMALL ? conv_small_groups(a, op.g.co) : op.res_groups;
    done.sums = a.sums.acc && !a.bs && conv_sums_ok(caps, a, op.g.co) && a.sums.groups == a.groups;
    done.epi = a.epi && (caps & CAP_EPI);
    if (!done.sums) a.sums = StatReq();
    if (!done.epi) a.epi = nullptr;
    if (launch_conv(kern, op, a) != 0)
        set_error(a.bs ? std::string("fused BatchNorm-backward sums: the data-gradient launch of ") + cv.name + " does not fit " + kname
                       : std::string("internal: ") + kname + " rejected the " + (op.dgrad ? "data-gradient" : "forward") + " launch of " +
                             cv.name + " it was chosen for");
    return done;
}

// the four sub-pixel phases of a stride-2 transposed convolution as one launch; false: not applicable (caller loops)
static bool exec_conv_x4(const Ctx& c, const ConvOp ops[4], const void* in, const float* bias, void* out) {
    if (!mfma_on(c.e)) return false;
    stcd_conv_geom g[4]; ConvMfmaPlan p[4]; const void* wf[4];
    double fl = 0.0, by = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (!ops[k].plan.ok || ops[k].wf < 0) return false;
        g[k] = ops[k].g; p[k] = ops[k].plan; wf[k] = c.at(ops[k].wf);
        fl += ops[k].flops; by += ops[k].bytes;
    }
    if (!conv_mfma_x4_ok(g, p)) return false;
    char kname[64];
    snprintf(kname, sizeof(kname), "k_conv_mfma_x4<%d>", p[0].NT);
    ProfScope prof(c, PC_CONV, fl, by, kname);
    if (launch_conv_mfma_x4(g, p, in, wf, bias, out, c.s) != 0) set_error(std::string("internal: ") + kname + " rejected the launch it was chosen for");
    return true;
}

// what comes before the pack launch: uploads the job tables on first use of a workspace, then says whether the filter images must be
// (re)packed -- and books them as packed, so the caller launches the pack (on its own or inside k_step_prologue) when *need is set
static int pack_prepare(const Ctx& c, bool with_dgrad, bool* need) {
    stcd_engine& e = c.e;
    *need = false;
    if (e.jobs_uploaded_ws != (const void*)c.ws) {      // first use of this workspace: upload both job tables
        for (int k = 0; k < 2; ++k) {
            if (!e.jobs[k].empty())
                STCD_HIP(hipMemcpyAsync(c.at(e.jobs_off[k]), e.jobs[k].data(), e.jobs[k].size() * sizeof(PackJob),
                                        hipMemcpyHostToDevice, c.s));
            if (!e.rjobs[k].empty())
                STCD_HIP(hipMemcpyAsync(c.at(e.rjobs_off[k]), e.rjobs[k].data(), e.rjobs[k].size() * sizeof(ReduceJob),
                                        hipMemcpyHostToDevice, c.s));
            for (WgradGroup& G : e.wgroups[k])
                STCD_HIP(hipMemcpyAsync(c.at(G.table_off), G.jobs.data(), G.jobs.size() * sizeof(WgradJob), hipMemcpyHostToDevice, c.s));
        }
        if (!e.bias_jobs.empty())
            STCD_HIP(hipMemcpyAsync(c.at(e.bias_jobs_off), e.bias_jobs.data(), e.bias_jobs.size() * sizeof(BiasJob), hipMemcpyHostToDevice, c.s));
        e.jobs_uploaded_ws = c.ws;
    }
    const int k = with_dgrad ? 1 : 0;
    // the caller declared the weights constant under this tag (stcd_set_weights_tag): the images packed into THIS workspace from
    // THIS parameter buffer under the same tag are still valid (the forward-only image set is a subset of the training one)
    // Training forwards always repack and never vouch for the next call (an optimizer step follows them).
    if (k == 0 && e.weights_tag != 0 && e.weights_tag == e.packed_tag && e.packed_ws == (const void*)c.ws && e.packed_params == (const void*)c.params)
        return 0;
    e.packed_tag = k == 0 ? e.weights_tag : 0; e.packed_ws = c.ws; e.packed_params = c.params; e.packed_level = k;
    *need = true;
    return 0;
}
static int pack_all_weights(const Ctx& c, bool with_dgrad) {
    stcd_engine& e = c.e;
    bool need = false;
    if (pack_prepare(c, with_dgrad, &need)) return 1;
    if (!need) return 0;
    const int k = with_dgrad ? 1 : 0;
    ProfScope prof(c, PC_PACK, 0.0, 0.0);
    launch_pack_jobs(c.at<PackJob>(e.jobs_off[k]), (int)e.jobs[k].size(), e.jobs_total[k], c.params, c.ws, c.s);
    return 0;
}

// ---- weight gradients at run time.  What a call changes is in e.wrun (WgradScope); the plan is only read.  A refusal or a failed HIP
//      call keeps the first such text of the call and sets wrun.failed, which stage_tail turns into the backward's return value.
static void wgrad_fail(const Ctx& c, const std::string& msg) {
    if (!c.e.wrun.failed) set_error(msg);
    c.e.wrun.failed = true;
}

static void launch_wgroup(const Ctx& c, int stage, int group) {
    const WgradGroup& G = c.e.wgroups[stage][group];
    char kname[64];
    wgrad_kernel_name(G.kernel, true, kname);
    ProfScope prof(c, PC_WGRAD, G.flops, G.bytes, kname);
    c.e.wrun.groups[stage][group].launched = true;
    if (launch_wgrad_jobs(G.kernel, c.at<WgradJob>(G.table_off), (int)G.jobs.size(), G.total_blocks, G.lds_bytes, c.ws, c.s) != 0)
        wgrad_fail(c, "grouped weight-gradient launch exceeds the LDS budget");
}

// A backward with early launches (wrun.early): a member's operands (X stored by the forward, dY final) exist when the chain
// calls exec_wgrad for it; the group's grid goes out with its LAST member -- on the side stream, behind an event of the chain's
// stream, when there is one -- instead of at the end of the stage
// stage 1 with a split reduce table: once every group but the final one has gone out, their slabs are summed right behind them (on the
// stream they went out on), under the chain's last kernels instead of on the tail
static void reduce_early_if_due(const Ctx& c) {
    stcd_engine& e = c.e;
    if (e.rj_split <= 0 || e.wrun.rj_early_done) return;
    if (e.prof.on) return;      // instrumented steps run serially on one stream: both parts go out on the tail, timed as one record
    for (size_t g = 0; g < e.wgroups[1].size(); ++g)
        if ((int)g != e.wg_final_group && !e.wrun.groups[1][g].launched) return;
    launch_reduce_jobs(c.at<ReduceJob>(e.rjobs_off[1]), e.rj_split, e.rj_total_early, c.ws, c.grads, c.s);
    e.wrun.rj_early_done = true;
}
static void wgroup_member_ready(const Ctx& c, const WgradOp& op) {
    stcd_engine& e = c.e;
    WgradRun& run = e.wrun;
    WgradRun::Group& rg = run.groups[op.stage][op.group];
    if (++rg.seen < (int)e.wgroups[op.stage][op.group].jobs.size() || rg.launched) return;
    // stage 1's final group (conv11, conv12) becomes ready when the chain has nothing left to run beside it: it goes out on the
    // caller's stream, and its slab reduce and the optimizer behind it need no cross-stream hand-off (stage_tail; measured in
    // DESIGN.md section 4, "Step seams")
    const bool final_group = op.stage == 1 && e.rj_split > 0 && op.group == e.wg_final_group;
    if (run.side && !final_group) {
        if (hipEventRecord(e.wg_fork, c.s) != hipSuccess || hipStreamWaitEvent(run.side, e.wg_fork, 0) != hipSuccess) { wgrad_fail(c, "side-stream fork failed"); return; }
        Ctx cs{e, c.ws, c.params, c.grads, run.side};
        launch_wgroup(cs, op.stage, op.group);
        if (op.stage == 1) reduce_early_if_due(cs);
    } else {
        launch_wgroup(c, op.stage, op.group);
        if (final_group && run.side) run.final_on_main = true;
        else if (op.stage == 1) reduce_early_if_due(c);
    }
}

// weight gradient of one launch, delivered straight into the reference-layout gradient tensor
static void exec_wgrad(const Ctx& c, const WgradOp& op, const void* in, const void* dout) {
    const ConvW& cv = c.e.convs[op.conv];
    if (mfma_on(c.e) && op.plan.ok && op.group >= 0) {          // runs in the stage's grouped launch (reduce_stage, or early: wgroup_member_ready)
        if (c.e.wrun.early) wgroup_member_ready(c, op);
        return;
    }
    double fl, by;
    conv_work(c.e, op.g, op.kreal, op.nreal, &fl, &by);
    if (mfma_on(c.e) && op.plan.ok) {
        char kname[64];
        wgrad_kernel_name(wgrad_kernel_of(op.plan, op.g, false), false, kname);
        ProfScope prof(c, PC_WGRAD, fl, by, kname);
        if (launch_wgrad_mfma(op.g, op.plan, in, dout, c.at<float>(op.slab), cv.fwd.kpad, cv.fwd.wld, c.s) == 0)
            return;                // the slabs are summed by the stage's batched reduce launch (reduce_stage)
    }
    if (op.own_taps) { wgrad_fail(c, "internal: no reference fallback for a launch with its own tap table"); return; }
    PackSpec sub = cv.fwd;                 // this launch's taps of the filter
    sub.ntaps = op.g.ntaps;
    wgrad_taps(c.e, op, sub.ky, sub.kx);
    double* dwe = c.at<double>(cv.dwe) + (int64_t)op.tap0 * sub.kpad * sub.wld;
    if (mfma_on(c.e)) {   // the bulk memset of the reference path's accumulators is skipped in MFMA mode
        const hipError_t err = hipMemsetAsync(dwe, 0, (size_t)sub.ntaps * sub.kpad * sub.wld * 8, c.s);
        if (err != hipSuccess) { wgrad_fail(c, std::string("exec_wgrad: hipMemsetAsync: ") + hipGetErrorString(err)); return; }
    }
    {
        ProfScope prof(c, PC_WGRAD, fl, by, "k_wgrad_ref");
        launch_wgrad_ref_f64(c.e.dt, op.g, in, dout, dwe, sub.kpad, sub.wld, c.s);
    }
    launch_unpack_dw(sub, dwe, c.grads + cv.w_off, c.s);
}

// the stage's groups that have not gone out yet, then the batched slab reduction
static void reduce_stage(const Ctx& c, int stage) {
    stcd_engine& e = c.e;
    for (size_t g = 0; g < e.wgroups[stage].size(); ++g)
        if (!e.wrun.groups[stage][g].launched) launch_wgroup(c, stage, (int)g);
    if (e.rjobs[stage].empty()) return;
    ProfScope prof(c, PC_PACK, 0.0, 0.0, "k_reduce_jobs");
    if (stage == 1 && e.rj_split > 0) {      // split table: whatever of the early part is still open, then the final group's jobs
        if (!e.wrun.rj_early_done) launch_reduce_jobs(c.at<ReduceJob>(e.rjobs_off[1]), e.rj_split, e.rj_total_early, c.ws, c.grads, c.s);
        e.last_tail = (e.wrun.rj_early_done ? 1 : 0) | (e.wrun.final_on_main ? 2 : 0);      // (stcd_seam_plan)
        launch_reduce_jobs(c.at<ReduceJob>(e.rjobs_off[1]) + e.rj_split, (int)e.rjobs[1].size() - e.rj_split, e.rj_total_final, c.ws, c.grads, c.s);
        return;
    }
    launch_reduce_jobs(c.at<ReduceJob>(e.rjobs_off[stage]), (int)e.rjobs[stage].size(), e.rjobs_total[stage], c.ws, c.grads, c.s);
}

// the Dropout2d factors of drop entry `drop` (nullptr: the layer has none, or dropout is off)
static const float* drop_mask(const Ctx& c, int drop, bool on = true) {
    return (on && c.e.drop_p > 0.f && drop >= 0) ? c.at<float>(c.e.masks) + c.e.drops[drop].off : nullptr;
}
// the BatchNorm fields of an activation launch: it derives scale / shift itself, from the accumulators `facc` in training mode,
// from the running statistics in eval mode (facc == nullptr) -- no finalize / prepare launch either way
static void bn_fields(BnActArgs& a, const Ctx& c, const BnP& bn, int C, float* bn_running, long long* facc) {
    a.facc = facc;
    a.gamma = c.params + bn.g_off; a.beta = c.params + bn.b_off;
    a.running_mean = bn_running + bn.run_off; a.running_var = bn_running + bn.run_off + C;
}
// conv, then the BatchNorm statistics of its output Y in `facc` (nullptr: eval, none): summed by the conv kernel where it delivers
// them (exec_conv), else by the separate pass
static void exec_conv_stats(const Ctx& c, const ConvOp& op, ConvArgs a, long long* facc, int groups, int C, const TRef& Y, int64_t ppg,
                            double act_bytes) {
    a.sums.acc = facc; a.sums.groups = groups; a.sums.C = C;
    if (exec_conv(c, op, a).sums || !facc) return;
    ProfScope ps(c, PC_BN_STATS, 0.0, act_bytes);
    launch_bn_stats(c.e.dt, c.at(Y.off), Y.ld, C, groups, ppg, facc, c.s);
}

// the producer P as its consumer's staging transform sees it (XfSrc, common.h): training -> batch statistics from P's accumulators,
// the consumer's block 0 publishes P.stat and updates the running statistics; eval -> the running statistics, nothing written
static XfSrc xf_source(const Ctx& c, const Cbrd& P, float* bn_running, bool training) {
    stcd_engine& e = c.e;
    const BnP& bn = e.bns[P.bn];
    XfSrc x;
    x.C = e.convs[P.conv].cout; x.groups = P.groups; x.npg = P.npg; x.ppg = (long long)P.npg * P.H * P.W;
    x.facc = training ? c.at<long long>(P.facc) : nullptr;
    x.gamma = c.params + bn.g_off; x.beta = c.params + bn.b_off;
    x.rmean = bn_running + bn.run_off; x.rvar = bn_running + bn.run_off + x.C;
    x.stat = c.at<float>(P.stat);
    x.mask = drop_mask(c, P.drop, training);
    x.publish = training ? 1 : 0;
    x.on = 1;
    return x;
}

static void cbrd_forward(const Ctx& c, const Cbrd& L, float* bn_running, bool training) {
    stcd_engine& e = c.e;
    const ConvW& cv = e.convs[L.conv];
    const BnP& bn = e.bns[L.bn];
    const int C = cv.cout;
    const int64_t ppg = (int64_t)L.npg * L.H * L.W;
    const double act_bytes = (double)L.N * L.H * L.W * C * (double)dsize(e.dt);
    long long* const facc = training ? c.at<long long>(L.facc) : nullptr;
    XfSrc xf;                // (on == 0: a materialised input)
    if (L.xsrc) xf = xf_source(c, *L.xsrc, bn_running, training);
    ConvArgs ca = conv_args(c.at(L.in.off), c.at(L.Y.off), c.params + cv.b_off);
    ca.xf = &xf;
    exec_conv_stats(c, L.fwd, ca, facc, L.groups, C, L.Y, ppg, act_bytes);
    float* stat = c.at<float>(L.stat);
    if (L.virt) return;      // the consumer applies scale / shift / ReLU / Dropout2d while staging Y (and publishes the statistics)
    BnActArgs a;
    a.Y = c.at(L.Y.off); a.ldy = L.Y.ld;
    a.A = skip_recomputed(e, L) ? nullptr : c.at(L.A.off); a.lda = L.A.ld; a.a_group_off = L.A.goff;
    a.P = L.pool ? c.at(L.P.off) : nullptr; a.ldp = L.P.ld;
    a.stat = stat;
    a.mask = drop_mask(c, L.drop, training);
    a.C = C; a.groups = L.groups; a.npg = L.npg; a.H = L.H; a.W = L.W; a.relu = 1;
    bn_fields(a, c, bn, C, bn_running, facc);
    if (L.fuse_dst.off >= 0 && e.use_act_fuse && L.groups == 2) {
        ProfScope ps(c, PC_BN_ACT, 0.0, act_bytes * (a.A ? 2.75 : 1.75), "k_bn_act_pair");
        launch_bn_act_pair(e.dt, a, c.at(L.fuse_dst.off), L.fuse_dst.ld, e.arch == STCD_ARCH_DIFF ? 0 : 1, c.s);
        return;
    }
    ProfScope ps(c, PC_BN_ACT, 0.0, act_bytes * (L.pool ? 2.25 : 2.0));
    launch_bn_act(e.dt, a, c.s);
}

// the BatchNorm-backward sums of layer P as a data-gradient launch forms them (BwdSum, common.h)
static BwdSum bwd_sum_of(const Ctx& c, const Cbrd& P) {
    stcd_engine& e = c.e;
    BwdSum b;
    b.Y = c.at(P.Y.off); b.ldy = P.Y.ld; b.stat = c.at<float>(P.stat);
    b.mask = drop_mask(c, P.drop);
    b.acc = c.at<long long>(P.bacc); b.groups = P.groups;
    return b;
}

// skip_chunks > 0: dA and the BN partial sums were already produced by launch_skip_bwd (that many rows per date)
static void cbrd_backward(const Ctx& c, const Cbrd& L, int skip_chunks = 0) {
    stcd_engine& e = c.e;
    const ConvW& cv = e.convs[L.conv];
    const BnP& bn = e.bns[L.bn];
    const int C = cv.cout;
    const int64_t HW = (int64_t)L.H * L.W, ppg = (int64_t)L.npg * HW;
    const float* stat = c.at<float>(L.stat);
    const float* mask = drop_mask(c, L.drop);
    long long* bacc = c.at<long long>(L.bacc);
    const double act_bytes = (double)L.N * HW * C * (double)dsize(e.dt);
    (void)ppg;
    if (!skip_chunks && !L.bwd_sums_fused) {
        ProfScope ps(c, PC_BN_BWD_REDUCE, 0.0, 2.0 * act_bytes);
        launch_bn_bwd_reduce(e.dt, c.at(L.dA.off), L.dA.ld, L.dA.goff, c.at(L.Y.off), L.Y.ld, stat, mask, C, L.groups, L.npg, HW, 1,
                             bacc, c.s);
    }
    {
        ProfScope ps(c, PC_BN_BWD_APPLY, 0.0, 3.0 * act_bytes);
        launch_bn_bwd_apply(e.dt, c.at(L.dA.off), L.dA.ld, L.dA.goff, c.at(L.dY.off), L.dY.ld, c.at(L.Y.off), L.Y.ld, stat, bacc,
                            c.grads + bn.g_off, c.grads + bn.b_off, mask, C, L.groups, L.npg, HW, 1, c.s);
    }
    // weight gradient (the conv bias feeds only a train-mode BN: its gradient is exactly zero and stays zero)
    exec_wgrad(c, L.wg, c.at(L.in.off), c.at(L.dY.off));
    if (L.has_dIn) {
        ConvArgs a = conv_args(c.at(L.dY.off), c.at(L.dIn.off));
        if (L.dgr_sum_acc >= 0) a.sums = StatReq{c.at<long long>(L.dgr_sum_acc), 1, L.dgr_sum_c0, L.dgr_sum_C, BN_BS, BN_BS};
        BwdSum bs;
        if (L.dgr_bwd) { bs = bwd_sum_of(c, *L.dgr_bwd); a.bs = &bs; }
        exec_conv(c, L.dgr, a);
    }
}

static void upconv_forward(const Ctx& c, const UpConv& U) {
    stcd_engine& e = c.e;
    const ConvW& cv = e.convs[U.conv];
    if (!exec_conv_x4(c, U.fwd, c.at(U.in.off), c.params + cv.b_off, c.at(U.out.off)))
        for (int ph = 0; ph < 4; ++ph) exec_conv(c, U.fwd[ph], conv_args(c.at(U.in.off), c.at(U.out.off), c.params + cv.b_off));
    launch_rep_pad(e.dt, c.at(U.out.off), U.out.ld, U.N, U.Ho, U.Wo, 2 * U.h, 2 * U.w, U.C, c.s);
}

static void upconv_backward(const Ctx& c, const UpConv& U) {
    stcd_engine& e = c.e;
    const ConvW& cv = e.convs[U.conv];
    launch_rep_pad_bwd(e.dt, c.at(U.dOut.off), U.dOut.ld, U.N, U.Ho, U.Wo, 2 * U.h, 2 * U.w, U.C, c.s);
    // bias gradient over the un-padded 2h x 2w region == all phases' positions
    if (U.bias_fused && mfma_on(e)) {
        // summed by the data-gradient launch that produced dOut; converted by k_bias_finish at the end of the stage
    } else if (2 * U.h == U.Ho && 2 * U.w == U.Wo) {
        launch_bias_grad(e.dt, c.at(U.dOut.off), U.dOut.ld, (int64_t)U.N * U.Ho * U.Wo, U.C, c.grads + cv.b_off, c.s,
                         e.dt == BF16 ? c.at<long long>(U.bias_acc) : nullptr);
    } else {
        const int64_t T = (int64_t)dsize(e.dt);
        for (int n = 0; n < U.N; ++n)
            for (int y = 0; y < 2 * U.h; ++y)
                launch_bias_grad(e.dt, c.at<char>(U.dOut.off) + ((int64_t)(n * U.Ho + y) * U.Wo) * U.dOut.ld * T, U.dOut.ld,
                                 2 * U.w, U.C, c.grads + cv.b_off, c.s, e.dt == BF16 ? c.at<long long>(U.bias_acc) : nullptr);
    }
    for (int ph = 0; ph < 4; ++ph) exec_wgrad(c, U.wg[ph], c.at(U.in.off), c.at(U.dOut.off));
    exec_conv(c, U.dgr, conv_args(c.at(U.dOut.off), c.at(U.dIn.off)));
}

// cross_conc block (SiamUnet_crossconc.py:24-33): skip slice of the level's concat buffer = relu(bn(conv(relu(bn(pairdw(x1, x2))))))
static void xconc_forward(const Ctx& c, const XConc& X, const Cbrd& skip, float* bn_running, bool training) {
    stcd_engine& e = c.e;
    const BnP& bn = e.bns[X.bn1];
    const int C = X.C, B = X.res.N, h = X.res.H, w = X.res.W;
    {
        ProfScope ps(c, PC_POOL_FUSE, 0.0, 3.0 * B * h * w * C * (double)dsize(e.dt), "k_pairdw_fwd");
        launch_pairdw_fwd(e.dt, c.at(skip.A.off), skip.A.ld, skip.A.goff, c.at(X.G.off), X.G.ld, c.params + X.w_off, c.params + X.b_off, B, h, w, C, c.s);
    }
    if (training) launch_bn_stats(e.dt, c.at(X.G.off), X.G.ld, C, 1, (int64_t)B * h * w, c.at<long long>(X.facc1), c.s);
    BnActArgs a;
    a.Y = c.at(X.G.off); a.ldy = X.G.ld;
    a.A = c.at(X.R.off); a.lda = X.R.ld; a.a_group_off = 0;
    a.P = nullptr; a.ldp = 0;
    a.stat = c.at<float>(X.stat1);
    a.mask = nullptr;
    a.C = C; a.groups = 1; a.npg = B; a.H = h; a.W = w; a.relu = 1;
    bn_fields(a, c, bn, C, bn_running, training ? c.at<long long>(X.facc1) : nullptr);
    launch_bn_act(e.dt, a, c.s);
    cbrd_forward(c, X.res, bn_running, training);
}
// its backward: writes the gradient of BOTH dates' skip activations (the pool gradient is accumulated onto them in the encoder stage)
static void xconc_backward(const Ctx& c, const XConc& X, const Cbrd& skip) {
    stcd_engine& e = c.e;
    const BnP& bn = e.bns[X.bn1];
    const int C = X.C, B = X.res.N, h = X.res.H, w = X.res.W;
    const int64_t HW = (int64_t)h * w;
    cbrd_backward(c, X.res);                       // BN-backward of conv_res, its weight gradient, data gradient -> dR
    launch_bn_bwd_reduce(e.dt, c.at(X.dR.off), X.dR.ld, 0, c.at(X.G.off), X.G.ld, c.at<float>(X.stat1), nullptr, C, 1, B, HW, 1,
                         c.at<long long>(X.bacc1), c.s);
    launch_bn_bwd_apply(e.dt, c.at(X.dR.off), X.dR.ld, 0, c.at(X.dG.off), X.dG.ld, c.at(X.G.off), X.G.ld, c.at<float>(X.stat1),
                        c.at<long long>(X.bacc1), c.grads + bn.g_off, c.grads + bn.b_off, nullptr, C, 1, B, HW, 1, c.s);
    ProfScope ps(c, PC_POOL_FUSE, 0.0, 6.0 * B * h * w * C * (double)dsize(e.dt), "k_pairdw_bwd");
    launch_pairdw_bwd_data(e.dt, c.at(X.dG.off), X.dG.ld, c.at(skip.dA.off), skip.dA.ld, skip.dA.goff, c.params + X.w_off, B, h, w, C, c.s);
    launch_pairdw_bwd_filter(e.dt, c.at(skip.A.off), skip.A.ld, skip.A.goff, c.at(X.dG.off), X.dG.ld, c.grads + X.w_off, c.at<float>(X.part),
                             B, h, w, C, c.s);
    // (diff.0's bias sits in front of a train-mode BatchNorm: its gradient is exactly zero and stays zero)
}

static int forward_fcsiam(stcd_engine& e, const float* x1, const float* x2, const float* params, float* bn_running,
                          const float* masks, uint64_t seed, int training, float* logits, void* workspace, hipStream_t s) {
    Ctx c{e, (char*)workspace, params, nullptr, s};
    const int B = e.B, dt = e.dt;
    const int64_t T = (int64_t)dsize(dt);
    // ---- the step's entry: dropout masks, filter images, the zero arena, the packed input.  They write disjoint buffers
    //      (configure_fcsiam checks it) and read only the caller's tensors: ONE launch (k_step_prologue) with a block range each;
    //      stcd_set_debug bit 1: the four launches they were.  Explicit masks are copied in either way.
    float gen_p = -1.f;                                  // >= 0: masks from the counter hash with this p
    if (training && e.drop_p > 0.f) {
        if (masks) STCD_HIP(hipMemcpyAsync(c.at(e.masks), masks, e.drop_floats * 4, hipMemcpyDeviceToDevice, s));
        else gen_p = e.drop_p;
    } else if (training && e.fc_virt_layers > 0) {
        // p == 0 with virtual activations: the weight-gradient job table addresses the mask buffer unconditionally (it is built at
        // configure time), so the buffer must read as all ones (k_dropout_gen with p = 0 writes 1 / (1 - 0) everywhere)
        gen_p = 0.f;
    }
    const int in_dates = e.arch == STCD_ARCH_FCEF ? 0 : 2;      // 0: cat(x1, x2) along the channels
    if (e.debug_flags & 2) {
        if (gen_p >= 0.f) launch_dropout_gen(c.at<float>(e.masks), e.drop_floats, seed, gen_p, s);
        if (pack_all_weights(c, training != 0)) return 1;
        if (training) STCD_HIP(hipMemsetAsync(c.at(e.zero_begin), 0, e.zero_end - e.zero_begin, s));   // the step's ONE workspace memset
        launch_in_pack(dt, x1, x2, c.at(e.X0.off), B, e.in_ch, e.H, e.W, s, in_dates);
    } else {
        StepPrologue a{};
        if (gen_p >= 0.f) { a.mask = c.at<float>(e.masks); a.drop_n = e.drop_floats; a.seed = seed; a.p = gen_p; }
        bool need_pack = false;
        if (pack_prepare(c, training != 0, &need_pack)) return 1;
        if (need_pack) {
            const int k = training ? 1 : 0;
            a.jobs = c.at<PackJob>(e.jobs_off[k]); a.njobs = (int)e.jobs[k].size(); a.pack_total = e.jobs_total[k];
            a.params = params; a.ws = c.ws;
        }
        if (training) {
            if (zero_fill_ok(c.at(e.zero_begin), e.zero_end - e.zero_begin)) { a.zero_p = c.at<char>(e.zero_begin); a.zero_bytes = e.zero_end - e.zero_begin; }
            else STCD_HIP(hipMemsetAsync(c.at(e.zero_begin), 0, e.zero_end - e.zero_begin, s));      // (a workspace the 16-byte stores cannot take)
        }
        a.x1 = x1; a.x2 = x2; a.X = c.at(e.X0.off); a.B = B; a.cin = e.in_ch; a.HW = (int64_t)e.H * e.W;
        a.concat = in_dates == 0 ? 1 : 0;
        a.in_total = (int64_t)(a.concat ? 1 : in_dates) * B * a.HW;
        int rc;
        if (need_pack) {      // instrumented steps: the launch stands where the pack launch stood, in its class and under its name
            ProfScope prof(c, PC_PACK, 0.0, 0.0);
            rc = launch_step_prologue(dt, a, s);
        } else {
            rc = launch_step_prologue(dt, a, s);
        }
        STCD_CHECK(rc == 0, "the step prologue's grid exceeds 2^31 - 1 blocks");
    }
    for (auto& L : e.enc) cbrd_forward(c, L, bn_running, training != 0);
    size_t di = 0;
    for (int k = 0; k < 4; ++k) {
        const UpConv& U = e.ups[k];
        const int s_ = U.level, C = ENC_C[s_];
        upconv_forward(c, U);
        const Cbrd& skip = e.enc[SKIP_IDX[s_]];
        if (fc_cross(e)) xconc_forward(c, e.xc[s_], skip, bn_running, training != 0);
        else if (!fc_concat_skips(e) && !(e.use_act_fuse && skip.fuse_dst.off >= 0)) {
            ProfScope ps(c, PC_POOL_FUSE, 0.0, 3.0 * B * e.Hs[s_] * e.Ws[s_] * C * (double)T);
            launch_fuse(dt, e.arch == STCD_ARCH_DIFF ? 0 : 1, c.at(skip.A.off), skip.A.ld, skip.A.goff,
                        c.at<char>(e.D[s_].off) + C * T, e.D[s_].ld, B, (int64_t)e.Hs[s_] * e.Ws[s_], C, s);
        }
        for (int j = 0; j < DEC[k].n; ++j) {
            if (DEC[k].cout[j] < 0) break;
            cbrd_forward(c, e.dec[di++], bn_running, training != 0);
        }
    }
    {
        XfSrc xf;                // (on == 0: a materialised input)
        if (e.final_xsrc) xf = xf_source(c, *e.final_xsrc, bn_running, training != 0);
        ConvArgs a = conv_args(c.at(e.finalIn.off), logits, params + e.convs[e.final_conv].b_off, true);
        a.xf = &xf;
        exec_conv(c, e.final_fwd, a);
    }
    STCD_HIP(hipGetLastError());
    return 0;
}

// The side stream of the decoder's weight gradients (FC-Siam family, both backward stages in one call): created on first use, lowest
// priority.  nullptr: switched off (STCD_WGRAD_SIDE=0), or the caller's stream is being captured into a graph (a captured step stays on
// one stream).  MEASURED (MI355X, SiamUnet_diff 16 x 256^2): serial 2.281-2.289 ms; side stream with the planner's full grids 2.265
// (the grouped launches fill every CU: the chain's kernels queue behind them); with a quarter of the block budget for stage 0's
// groups (fewer, longer blocks: fewer slabs too) 2.223-2.235 ms.  A CU-masked stream (hipExtStreamCreateWithCUMask, any mask
// including all CUs) cost 0.8-1.7 ms per step on this stack and was dropped.
static hipStream_t wgrad_side_stream(stcd_engine& e, hipStream_t s) {
    if (!e.wg_side_on || !e.use_wgroup || !mfma_on(e)) return nullptr;
    if (e.prof.on) return nullptr;                      // instrumented steps (stcd_profile_enable) time every kernel ALONE: same plan, one stream
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (cap != hipStreamCaptureStatusNone) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (e.wg_side && e.wg_side_dev == dev) return e.wg_side;
    if (e.wg_side) return nullptr;                      // created on another device: stay serial there
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);      // (least, greatest)
    hipStream_t st = nullptr;
    if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio_lo) != hipSuccess) { (void)hipGetLastError(); e.wg_side_on = 0; return nullptr; }
    if (hipEventCreateWithFlags(&e.wg_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e.wg_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError(); (void)hipStreamDestroy(st); e.wg_side_on = 0; return nullptr;
    }
    e.wg_side = st; e.wg_side_dev = dev;
    return st;
}

static void finish_biases(const Ctx& c) {
    launch_bias_finish(c.at<BiasJob>(c.e.bias_jobs_off), (int)c.e.bias_jobs.size(), c.ws, c.grads, c.s);
}

// The tail of a backward stage: the stage's groups that have not gone out and its slab reduction (reduce_stage), then `extra` (column
// sums, bias finish).  With a side stream all of it runs there, behind an event of the caller's stream, and wg_join is recorded; the
// caller's stream waits on it only where wait_join says so (the last stage of a call: an earlier stage's tail runs beside the next
// stage's chain, and the side stream's order carries it to the last join).
// Returns 1 when a HIP call here fails or the call's weight-gradient path has failed (wrun.failed).
template <typename Extra>
static int stage_tail(const Ctx& c, int stage, hipStream_t side, bool wait_join, Extra extra) {
    stcd_engine& e = c.e;
    if (!side) { reduce_stage(c, stage); extra(c); return e.wrun.failed; }
    if (stage == 1 && e.wrun.final_on_main && e.wrun.rj_early_done) {
        // the stage's final group went out on the caller's stream, and everything the side stream holds went out long ago (the earlier
        // stage's tail, the early groups, their reduce): join it first, then the final group's reduce follows that group on this stream
        STCD_HIP(hipEventRecord(e.wg_join, side));
        STCD_HIP(hipStreamWaitEvent(c.s, e.wg_join, 0));
        reduce_stage(c, stage);
        extra(c);
        return e.wrun.failed;
    }
    STCD_HIP(hipEventRecord(e.wg_fork, c.s));
    STCD_HIP(hipStreamWaitEvent(side, e.wg_fork, 0));
    Ctx cs{e, c.ws, c.params, c.grads, side};
    reduce_stage(cs, stage);
    extra(cs);
    STCD_HIP(hipEventRecord(e.wg_join, side));
    if (wait_join) STCD_HIP(hipStreamWaitEvent(c.s, e.wg_join, 0));
    return e.wrun.failed;
}

// Every backward entry opens with this: e.wrun is reset for the stages the call runs (stage < 0: both) and set up for the call, and
// is clean again when the call ends, however it ends.  early: exec_wgrad sends a group out with its last member, on `side` if set.
// last_tail (stcd_seam_plan) is the stage-1 tail's to write and outlives the call.
struct WgradScope {
    stcd_engine& e;
    WgradScope(stcd_engine& e_, int stage, bool early, hipStream_t side) : e(e_) {
        reset(stage);
        e.wrun.early = early; e.wrun.side = side;
        if (stage != 0) e.last_tail = 0;
    }
    ~WgradScope() { reset(-1); }
    void reset(int stage) {
        WgradRun& r = e.wrun;
        for (int st = 0; st < 2; ++st)
            if (stage < 0 || stage == st) std::fill(r.groups[st].begin(), r.groups[st].end(), WgradRun::Group());
        r.early = false; r.side = nullptr;
        r.rj_early_done = r.final_on_main = r.failed = false;
    }
};

static int backward_fcsiam(stcd_engine& e, const float* grad_logits, const float* params, float* grads, void* workspace,
                           int stage, hipStream_t s) {
    Ctx c{e, (char*)workspace, params, grads, s};
    // both stages in one call (no gradient all-reduce between them): stage 0's weight gradients only read stored tensors and write
    // their own slabs / gradient entries, so they can run beside stage 1's chain
    hipStream_t side = stage < 0 ? wgrad_side_stream(e, s) : nullptr;
    WgradScope wgrad_scope(e, stage, mfma_on(e) && e.use_wgroup, side);
    const int B = e.B, dt = e.dt;
    const int64_t T = (int64_t)dsize(dt);
    if (stage <= 0) {
        // the gradient buffer is cleared by extra blocks of the pack launch (every writer of it follows in stream order; the zeros
        // stay in the biases in front of a train-mode BatchNorm); stcd_set_debug bit 1: by a memset of its own, as it was
        // (or the caller's buffer is one the 16-byte stores cannot take)
        const bool sep = (e.debug_flags & 2) != 0 || !zero_fill_ok(grads, e.param_floats * 4);
        if (sep) STCD_HIP(hipMemsetAsync(grads, 0, e.param_floats * 4, s));
        if (!mfma_on(e)) STCD_HIP(hipMemsetAsync(c.at(e.dwe_begin), 0, e.dwe_end - e.dwe_begin, s));
        // (the date-0 half of dP[3] and every accumulator were zeroed by the forward's arena memset)
        // conv11d: its bias gradient = per-channel sum of d(logits), formed while the gradient is packed
        if (launch_gout_pack(dt, grad_logits, c.at(e.G.off), B, e.label, e.H, e.W, s, c.at<long long>(e.final_bias_acc),
                             sep ? nullptr : grads, e.param_floats * 4)) {
            set_error("internal: k_gout_pack rejected the gradient buffer's zero-fill");
            return 1;
        }
        exec_wgrad(c, e.final_wg, c.at(e.finalIn.off), c.at(e.G.off));
        {
            ConvArgs a = conv_args(c.at(e.G.off), c.at(e.dFinalIn.off));
            BwdSum bs;
            if (e.final_dgr_bwd) { bs = bwd_sum_of(c, *e.final_dgr_bwd); a.bs = &bs; }
            exec_conv(c, e.final_dgr, a);
        }
        int di = (int)e.dec.size() - 1;
        for (int k = 3; k >= 0; --k) {
            int nb = 0;
            for (int j = 0; j < DEC[k].n; ++j) nb += DEC[k].cout[j] >= 0;
            for (int j = 0; j < nb; ++j) cbrd_backward(c, e.dec[di--]);
            const UpConv& U = e.ups[k];
            const int s_ = U.level, C = ENC_C[s_];
            upconv_backward(c, U);
            const Cbrd& skip = e.enc[SKIP_IDX[s_]];
            if (fc_cross(e)) xconc_backward(c, e.xc[s_], skip);
            else if (!fc_concat_skips(e) && !e.use_skip_fused) {
                ProfScope ps(c, PC_POOL_FUSE, 0.0, (e.arch == STCD_ARCH_DIFF ? 5.0 : 3.0) * B * e.Hs[s_] * e.Ws[s_] * C * (double)T);
                launch_fuse_bwd(dt, e.arch == STCD_ARCH_DIFF ? 0 : 1, c.at(skip.A.off), skip.A.ld, skip.A.goff,
                                c.at<char>(e.dD[s_].off) + C * T, e.dD[s_].ld, c.at(skip.dA.off), skip.dA.ld, skip.dA.goff, B,
                                (int64_t)e.Hs[s_] * e.Ws[s_], C, s);
            }
        }
        if (stage_tail(c, 0, side, false, finish_biases)) return 1;      // (stage 1's join below is the one the caller's stream waits on)
    }
    if (stage < 0 || stage == 1) {
        for (int li = (int)e.enc.size() - 1; li >= 0; --li) {
            const Cbrd& L = e.enc[li];
            int skip_chunks = 0;
            if (L.pool && !fc_concat_skips(e) && !fc_cross(e) && e.use_skip_fused) {
                // pool gradient + skip-fusion gradient + BN partial sums of the level's last conv in one pass
                const int C = e.convs[L.conv].cout;
                int lvl = 0;
                while (lvl < 4 && SKIP_IDX[lvl] != li) ++lvl;
                const float* mk = drop_mask(c, L.drop);
                if (skip_recomputed(e, L)) {
                    ProfScope ps(c, PC_POOL_FUSE, 0.0, 2.75 * L.N * L.H * L.W * C * (double)T, "k_skip_bwd_pair");
                    launch_skip_bwd_pair(dt, e.arch == STCD_ARCH_DIFF ? 0 : 1, c.at(L.Y.off), L.Y.ld, c.at<char>(e.dD[lvl].off) + C * T,
                                         e.dD[lvl].ld, c.at(L.dPool.off), L.dPool.ld, c.at(L.dA.off), L.dA.ld, L.dA.goff,
                                         c.at<float>(L.stat), mk, L.npg, L.H, L.W, C, c.at<long long>(L.bacc), s);
                } else {
                ProfScope ps(c, PC_POOL_FUSE, 0.0, 4.75 * L.N * L.H * L.W * C * (double)T, "k_skip_bwd");
                launch_skip_bwd(dt, e.arch == STCD_ARCH_DIFF ? 0 : 1, c.at(L.A.off), L.A.ld, L.A.goff, c.at(L.Y.off), L.Y.ld,
                                c.at<char>(e.dD[lvl].off) + C * T, e.dD[lvl].ld, c.at(L.dPool.off), L.dPool.ld, c.at(L.dA.off), L.dA.ld,
                                L.dA.goff, c.at<float>(L.stat), mk, L.npg, L.H, L.W, C, c.at<long long>(L.bacc), s);
                }
                skip_chunks = 1;
            } else if (L.pool) {  // dA_skip += gradient routed back through the 2x2 max-pool
                const int C = e.convs[L.conv].cout;
                ProfScope ps(c, PC_POOL_FUSE, 0.0, 3.25 * L.N * L.H * L.W * C * (double)T);
                launch_pool_bwd(dt, c.at(L.A.off), L.A.ld, L.A.goff, c.at(L.dPool.off), L.dPool.ld, c.at(L.dA.off), L.dA.ld,
                                L.dA.goff, L.groups, L.npg, L.H, L.W, C, 1, s);
            }
            cbrd_backward(c, L, skip_chunks);
        }
        if (stage_tail(c, 1, side, true, [](const Ctx&) {})) return 1;
    }
    STCD_HIP(hipGetLastError());
    return 0;
}

// ================================================================================================ SNUNet-ECAM, Siam_NestedUNet_Conc
static const int SN_F[5] = {32, 64, 128, 256, 512};

static int add_block_params(stcd_engine& e, const std::string& name, int cin, int c, int calls, bool need_dgrad1, NBlock* b) {
    b->name = name; b->Cin = cin; b->C = c;
    b->c1 = add_conv(e, name + ".conv1", K_CONV3, cin, c, need_dgrad1);
    b->bn1 = add_bn(e, name + ".bn1", c, calls);
    b->c2 = add_conv(e, name + ".conv2", K_CONV3, c, c, true);
    b->bn2 = add_bn(e, name + ".bn2", c, calls);
    return 0;
}

// registration order of SNUNet_ECAM.__init__ (SNUNet.py:73-106)
static void build_snunet_tables(stcd_engine& e) {
    const int* f = SN_F;
    e.sn_blocks.clear(); e.sn_ups.clear();
    auto blk = [&](const std::string& n, int cin, int c, int calls, bool dg) {
        NBlock b; add_block_params(e, n, cin, c, calls, dg, &b); e.sn_blocks.push_back(b);
    };
    auto up = [&](const std::string& n, int c) {
        SnUp u; u.C = c; u.conv = add_conv(e, n + ".up", K_CONVT2, c, c, true); e.sn_ups.push_back(u);
    };
    blk("conv0_0", e.in_ch, f[0], 2, false);
    blk("conv1_0", f[0], f[1], 2, true); up("Up1_0", f[1]);
    blk("conv2_0", f[1], f[2], 2, true); up("Up2_0", f[2]);
    blk("conv3_0", f[2], f[3], 2, true); up("Up3_0", f[3]);
    blk("conv4_0", f[3], f[4], 1, true); up("Up4_0", f[4]);
    blk("conv0_1", f[0] * 2 + f[1], f[0], 1, true);
    blk("conv1_1", f[1] * 2 + f[2], f[1], 1, true); up("Up1_1", f[1]);
    blk("conv2_1", f[2] * 2 + f[3], f[2], 1, true); up("Up2_1", f[2]);
    blk("conv3_1", f[3] * 2 + f[4], f[3], 1, true); up("Up3_1", f[3]);
    blk("conv0_2", f[0] * 3 + f[1], f[0], 1, true);
    blk("conv1_2", f[1] * 3 + f[2], f[1], 1, true); up("Up1_2", f[1]);
    blk("conv2_2", f[2] * 3 + f[3], f[2], 1, true); up("Up2_2", f[2]);
    blk("conv0_3", f[0] * 4 + f[1], f[0], 1, true);
    blk("conv1_3", f[1] * 4 + f[2], f[1], 1, true); up("Up1_3", f[1]);
    blk("conv0_4", f[0] * 5 + f[1], f[0], 1, true);
    const int c4 = f[0] * 4, c1 = f[0];
    e.enc_param_end = 0;      // one backward stage: every gradient is final when stage 0 returns
    if (is_snconc(e.arch)) {      // registration order of Siam_NestedUNet_Conc.__init__ (SNUNet.py:195-199)
        const int L = e.label;
        for (int i = 0; i < 4; ++i) {
            const std::string n = std::string("final") + char('1' + i);
            add_param(e, n + ".weight", {L, c1, 1, 1}, &e.snc_w[i]);
            add_param(e, n + ".bias", {L}, &e.snc_b[i]);
        }
        add_param(e, "conv_final.weight", {L, 4 * L, 1, 1}, &e.snc_w[4]);
        add_param(e, "conv_final.bias", {L}, &e.snc_b[4]);
        e.sn_final = -1;
        return;
    }
    add_param(e, "ca.fc1.weight", {c4 / 16, c4, 1, 1}, &e.sn_w[0]);
    add_param(e, "ca.fc2.weight", {c4, c4 / 16, 1, 1}, &e.sn_w[1]);
    add_param(e, "ca1.fc1.weight", {c1 / 4, c1, 1, 1}, &e.sn_w[2]);
    add_param(e, "ca1.fc2.weight", {c1, c1 / 4, 1, 1}, &e.sn_w[3]);
    e.sn_final = add_conv(e, "conv_final", K_CONV1, c4, e.label, true);
}

static int sn_block_index(const stcd_engine& e, const std::string& name) {
    for (size_t i = 0; i < e.sn_blocks.size(); ++i)
        if (e.sn_blocks[i].name == name) return (int)i;
    return -1;
}
static int sn_up_index(const stcd_engine& e, const std::string& name) {
    for (size_t i = 0; i < e.sn_ups.size(); ++i)
        if (e.convs[e.sn_ups[i].conv].name == name + ".up") return (int)i;
    return -1;
}

static int configure_snunet(stcd_engine& e, int B, int H, int W) {
    const int64_t T = (int64_t)dsize(e.dt);
    const int* f = SN_F;
    Planner ws(e);
    int hs[5], wsz[5];
    hs[0] = H; wsz[0] = W;
    for (int l = 0; l < 4; ++l) { hs[l + 1] = hs[l] / 2; wsz[l + 1] = wsz[l] / 2; }
    auto B_ = [&](const char* n) -> NBlock& { return e.sn_blocks[sn_block_index(e, n)]; };

    const bool conc = is_snconc(e.arch);       // no ECAM: no gated copy of E, no packed output gradient (kernels_snhead.hip)
    e.X0 = ws.plain(2 * B, H, W, 8);
    if (!conc) e.G = ws.plain(B, H, W, 8);
    const int c4 = f[0] * 4;
    e.snE = ws.plain(B, H, W, c4);
    if (!conc) { e.snZ = ws.plain(B, H, W, c4); e.sndZ = ws.plain(B, H, W, c4); }

    // ---- activation buffers of every block.  dOut buffers are allocated back to back: one memset per backward.
    e.sn_dout_begin = ws.cur;
    e.sndE = ws.plain(B, H, W, c4);
    for (auto& b : e.sn_blocks) {
        const int lvl = b.name[4] - '0', j = b.name[6] - '0';
        const bool enc = j == 0;
        b.H = hs[lvl]; b.W = wsz[lvl];
        b.N = (enc && lvl < 4) ? 2 * B : B;
        b.groups = (enc && lvl < 4) ? 2 : 1;
        b.npg = B;
        if (lvl == 0 && j >= 1) {            // x0_1..x0_4 live directly in the ECAM input (one copy less)
            b.dOut.off = e.sndE.off + (int64_t)(j - 1) * f[0] * T; b.dOut.ld = c4;
        } else {
            b.dOut = ws.plain(b.N, b.H, b.W, b.C);
        }
    }
    e.sn_dout_end = ws.cur;
    for (auto& b : e.sn_blocks) {
        const int lvl = b.name[4] - '0', j = b.name[6] - '0';
        const bool enc = j == 0;
        if (lvl == 0 && j >= 1) { b.Out.off = e.snE.off + (int64_t)(j - 1) * f[0] * T; b.Out.ld = c4; }
        else b.Out = ws.plain(b.N, b.H, b.W, b.C);
        b.Y1 = ws.plain(b.N, b.H, b.W, b.C); b.A1 = ws.plain(b.N, b.H, b.W, b.C); b.Y2 = ws.plain(b.N, b.H, b.W, b.C);
        b.dZ2 = ws.plain(b.N, b.H, b.W, b.C); b.dA1 = ws.plain(b.N, b.H, b.W, b.C);
        b.pool = enc && lvl < 4;
        if (b.pool) { b.P = ws.plain(b.N, b.H / 2, b.W / 2, b.C); b.dP = ws.plain(b.N, b.H / 2, b.W / 2, b.C); }
        b.stat1 = ws.take((int64_t)b.groups * 4 * b.C * 4);
        b.stat2 = ws.take((int64_t)b.groups * 4 * b.C * 4);
    }
    e.zero_begin = ws.cur;
    for (auto& b : e.sn_blocks) {
        b.facc1 = ws.take(bn_acc_bytes(b.groups, b.C)); b.facc2 = ws.take(bn_acc_bytes(b.groups, b.C));
        b.bacc1 = ws.take(bn_acc_bytes(b.groups, b.C)); b.bacc2 = ws.take(bn_acc_bytes(b.groups, b.C));
    }
    for (auto& u : e.sn_ups) u.bias_acc = ws.take(bn_acc_bytes(1, u.C));
    if (!conc) e.final_bias_acc = ws.take(bn_acc_bytes(1, 8));
    e.zero_end = ws.cur;
    // ---- inputs
    for (auto& b : e.sn_blocks) {
        const int lvl = b.name[4] - '0', j = b.name[6] - '0';
        b.srcs.clear(); b.up = -1;
        if (j == 0) {
            if (lvl == 0) { b.in = e.X0; b.Cin = 8; b.dIn.off = -1; }
            else {
                NBlock& prev = e.sn_blocks[sn_block_index(e, std::string("conv") + char('0' + lvl - 1) + "_0")];
                b.in = prev.P; b.dIn = prev.dP; b.Cin = prev.C;
                if (lvl == 4) {             // only the B date goes one level deeper (SNUNet.py:123 is commented out)
                    const int64_t half = (int64_t)B * (prev.H / 2) * (prev.W / 2) * prev.C * T;
                    b.in.off += half; b.dIn.off += half;
                }
            }
            continue;
        }
        b.in = ws.plain(b.N, b.H, b.W, b.Cin); b.dIn = ws.plain(b.N, b.H, b.W, b.Cin);
        NBlock& enc = e.sn_blocks[sn_block_index(e, std::string("conv") + char('0' + lvl) + "_0")];
        const int64_t half = (int64_t)B * enc.H * enc.W * enc.C * T;
        int coff = 0;
        auto add_src = [&](TRef src, TRef dsrc, int C, int prod, int grp) {
            SrcSlice s_; s_.src = src; s_.dsrc = dsrc; s_.C = C; s_.prod = prod; s_.grp = grp; b.srcs.push_back(s_); coff += C;
        };
        const int enc_i = sn_block_index(e, std::string("conv") + char('0' + lvl) + "_0");
        add_src(enc.Out, enc.dOut, enc.C, enc_i, 0);                                                      // x{lvl}_0A
        add_src(TRef{enc.Out.off + half, enc.Out.ld}, TRef{enc.dOut.off + half, enc.dOut.ld}, enc.C, enc_i, 1);   // x{lvl}_0B
        for (int k = 1; k < j; ++k) {
            const int di = sn_block_index(e, std::string("conv") + char('0' + lvl) + "_" + char('0' + k));
            NBlock& d = e.sn_blocks[di];
            add_src(d.Out, d.dOut, d.C, di, -1);
        }
        // up-sampled tail: Up{lvl+1}_{j-1}( x{lvl+1}_{j-1} ), the B date for j == 1
        const std::string upname = std::string("Up") + char('0' + lvl + 1) + "_" + char('0' + j - 1);
        b.up = sn_up_index(e, upname);
        SnUp& u = e.sn_ups[b.up];
        NBlock& lower = e.sn_blocks[sn_block_index(e, std::string("conv") + char('0' + lvl + 1) + "_" + char('0' + j - 1))];
        u.N = B; u.h = lower.H; u.w = lower.W;
        u.src = lower.Out; u.dsrc = lower.dOut;
        if (j == 1 && lvl + 1 < 4) {        // encoder output of both dates: take the B half
            const int64_t lh = (int64_t)B * lower.H * lower.W * lower.C * T;
            u.src.off += lh; u.dsrc.off += lh;
        }
        u.out = TRef{b.in.off + (int64_t)coff * T, b.Cin};
        u.dOut = TRef{b.dIn.off + (int64_t)coff * T, b.Cin};
        u.coff = coff;
        u.tmp = ws.plain(B, u.h, u.w, u.C);
    }
    // ---- dense concatenation without copy kernels: every producer writes its output straight into its consumers' concat
    //      slices (extra destinations of its last activation kernel), and gathers its gradient from their concat-gradient
    //      slices (extra sources of its BatchNorm-backward reduction).  The two dates of an encoder level sit side by side
    //      in a consumer (A at coff, B at coff + C): one view with a per-date channel offset.
    for (auto& b : e.sn_blocks) { b.extra_dst.clear(); b.grad_src.clear(); }
    for (auto& b : e.sn_blocks) {
        int coff = 0;
        for (auto& s_ : b.srcs) {
            if (s_.grp != 1) {       // (the date-1 slice of an encoder level rides on its date-0 view)
                NBlock& P = e.sn_blocks[s_.prod];
                ViewRef v; v.ld = b.in.ld; v.off = b.in.off + (int64_t)coff * T;
                if (s_.grp == 0) { v.gmask = 3; v.goff = s_.C; } else { v.gmask = 1; v.goff = 0; }
                P.extra_dst.push_back(v);
                ViewRef gv = v; gv.off = b.dIn.off + (int64_t)coff * T; gv.ld = b.dIn.ld;
                P.grad_src.push_back(gv);
            }
            coff += s_.C;
        }
    }
    for (auto& b : e.sn_blocks) {
        const int lvl = b.name[4] - '0', j = b.name[6] - '0';
        b.grad_base = (b.pool) || (lvl == 0 && j >= 1);          // max-pool gradient / ECAM gradient is written first
        if (b.up >= 0) {        // gradient arriving through the transposed conv that up-samples the LOWER block's output
            SnUp& u = e.sn_ups[b.up];
            NBlock& lower = e.sn_blocks[sn_block_index(e, std::string("conv") + char('0' + lvl + 1) + "_" + char('0' + j - 1))];
            ViewRef v; v.off = u.tmp.off; v.ld = u.tmp.ld; v.goff = 0;
            v.gmask = (lower.groups == 2) ? 2 : 1;               // an encoder level feeds its date-1 half only (SNUNet.py:127-142)
            lower.grad_src.push_back(v);
        }
    }
    for (auto& b : e.sn_blocks)
        if ((int)b.extra_dst.size() > MAX_VIEWS || (int)b.grad_src.size() > MAX_VIEWS) { set_error("internal: too many concat views"); return 1; }

    // ---- forward order (SNUNet.py:119-142)
    static const char* ORDER[] = {"conv0_0", "conv1_0", "conv2_0", "conv3_0", "conv4_0", "conv0_1", "conv1_1", "conv0_2", "conv2_1",
                                  "conv1_2", "conv0_3", "conv3_1", "conv2_2", "conv1_3", "conv0_4"};
    for (auto n : ORDER) e.sn_order.push_back(sn_block_index(e, n));

    e.scratch8 = ws.take(256);
    e.masks = ws.take(256);
    if (conc) {
        e.snc_scratch = ws.take(snhead_scratch_floats(B, (int64_t)H * W, e.label, sn_out_maps(e.arch) > 1) * 4);
    } else {
        e.sn_pool = ws.take((int64_t)B * 4 * c4 * 4); e.sn_argm = ws.take((int64_t)B * 2 * c4 * 8);
        e.sn_att = ws.take((int64_t)B * 2 * c4 * 4); e.sn_hid = ws.take((int64_t)B * 2 * 2 * 16 * 4);
        e.sn_sums = ws.take((int64_t)B * 2 * c4 * 4); e.sn_dpool = ws.take((int64_t)B * 4 * c4 * 4);
        e.sn_part = ws.take(ecam_part_floats(B, c4) * 4);
    }
    take_ref_images(e, ws);

    const Binder bind{e, ws};
    for (auto& b : e.sn_blocks) {
        const ConvW& c1 = e.convs[b.c1];
        const ConvW& c2 = e.convs[b.c2];
        bind.conv(b.f1, geom3(b.N, b.H, b.W, b.Cin, b.in.ld, b.C, b.Y1.ld), b.c1, false, 0, c1.cin, b.C, b.groups);
        bind.wgrad(b.w1, geom3(b.N, b.H, b.W, b.Cin, b.in.ld, b.C, b.dA1.ld), b.c1, b.in.off, b.dA1.off);
        if (b.dIn.off >= 0) bind.conv(b.d1, geom3(b.N, b.H, b.W, c1.dgrad.kpad, b.dA1.ld, c1.cin, b.dIn.ld), b.c1, true, 0, b.C, c1.cin);
        bind.conv(b.f2, geom3(b.N, b.H, b.W, b.C, b.A1.ld, b.C, b.Y2.ld), b.c2, false, 0, b.C, b.C, b.groups);
        bind.wgrad(b.w2, geom3(b.N, b.H, b.W, b.C, b.A1.ld, b.C, b.dOut.ld), b.c2, b.A1.off, b.dOut.off);
        bind.conv(b.d2, geom3(b.N, b.H, b.W, c2.dgrad.kpad, b.dOut.ld, b.C, b.dA1.ld), b.c2, true, 0, b.C, b.C);
    }
    for (auto& u : e.sn_ups) {
        if (u.N == 0) continue;
        const ConvW& cv = e.convs[u.conv];
        for (int ph = 0; ph < 4; ++ph) {      // ConvTranspose2d(k2, s2): phase ph is the one tap ph, out(2m + py, 2n + px) = in(m, n) W[py][px]
            const stcd_conv_geom g = geom_phase(u.N, u.h, u.w, u.C, u.src.ld, 2 * u.h, 2 * u.w, u.C, u.out.ld, ph, cv.fwd, 0, ph, 1);
            bind.conv(u.fwd[ph], g, u.conv, false, ph, u.C, u.C);
            bind.wgrad(u.wg[ph], g, u.conv, u.src.off, u.dOut.off, 0, ph);
        }
        // data gradient: the four taps (dy, dx) of a stride-2 gather over dOut
        bind.conv(u.dgr, geom_gather2(u.N, 2 * u.h, 2 * u.w, cv.dgrad.kpad, u.dOut.ld, u.h, u.w, u.C, u.tmp.ld, cv.dgrad, 0), u.conv, true, 0, u.C, u.C);
    }
    if (!conc) {
        const ConvW& cv = e.convs[e.sn_final];
        bind.conv(e.sn_final_fwd, geom1(B, H, W, c4, e.snZ.ld, e.label, e.label), e.sn_final, false, 0, c4, e.label);
        bind.wgrad(e.sn_final_wg, geom1(B, H, W, c4, e.snZ.ld, e.label, 8), e.sn_final, e.snZ.off, e.G.off);
        bind.conv(e.sn_final_dgr, geom1(B, H, W, cv.dgrad.kpad, 8, c4, e.sndZ.ld), e.sn_final, true, 0, e.label, c4);
    }
    e.slab = ws.take(e.slab_floats * 4);
    // bias gradients of the transposed convs: summed by the consumer block's conv1 data gradient (see configure_fcsiam)
    for (auto& b : e.sn_blocks) {
        b.d1_sum_acc = -1;
        if (b.up < 0) continue;
        SnUp& u = e.sn_ups[b.up];
        u.bias_fused = false;
        if (e.dt == BF16 && e.use_mfma && b.dIn.off >= 0 && b.d1.res.ok && b.d1.wf >= 0) {
            u.bias_fused = true;
            b.d1_sum_acc = u.bias_acc; b.d1_sum_c0 = u.coff; b.d1_sum_C = u.C;
        }
        if (e.dt == BF16) ws.bias_job(u.bias_acc, u.conv, u.C, u.C);
    }
    if (!conc) ws.bias_job(e.final_bias_acc, e.sn_final, 8, e.label);
    ws.tables();

    // test introspection (stcd_ws_tensor_*): every tensor a block, a transposed conv or the head stores, as it stands after a
    // forward / backward.  Two values do not survive the backward -- the gathered dOut (bn2's backward runs in place) and the head's
    // data gradient (it is the base term of conv0_1..conv0_4's dOut): debug bit 0 keeps a copy of each in a buffer of its own at the
    // END of the workspace, so that the plan without the bit is byte for byte the plan it was.
    const bool dbg = (e.debug_flags & 1) != 0;
    for (auto& b : e.sn_blocks) {
        b.dbg_dOut = dbg ? ws.plain(b.N, b.H, b.W, b.C) : TRef{};
        ws.tensor(b.name + ".in", b.in, b.N, b.H, b.W, b.Cin);
        ws.tensor(b.name + ".Y1", b.Y1, b.N, b.H, b.W, b.C); ws.tensor(b.name + ".A1", b.A1, b.N, b.H, b.W, b.C);
        ws.tensor(b.name + ".Y2", b.Y2, b.N, b.H, b.W, b.C); ws.tensor(b.name + ".Out", b.Out, b.N, b.H, b.W, b.C);
        if (b.pool) { ws.tensor(b.name + ".P", b.P, b.N, b.H / 2, b.W / 2, b.C); ws.tensor(b.name + ".dP", b.dP, b.N, b.H / 2, b.W / 2, b.C); }
        ws.tensor(b.name + ".dOut", b.dbg_dOut, b.N, b.H, b.W, b.C);
        ws.tensor(b.name + ".dZ2", b.dZ2, b.N, b.H, b.W, b.C);
        ws.tensor(b.name + ".dY2", b.dOut, b.N, b.H, b.W, b.C);          // the dOut buffer after bn2's backward
        ws.tensor(b.name + ".dY1", b.dA1, b.N, b.H, b.W, b.C);           // the dA1 buffer after bn1's backward
        ws.tensor(b.name + ".dIn", b.dIn, b.N, b.H, b.W, b.Cin);
    }
    for (const auto& u : e.sn_ups) {
        if (u.N == 0) continue;
        const std::string& cn = e.convs[u.conv].name;              // "UpL_J.up"
        const std::string un = cn.substr(0, cn.size() - 3);
        ws.tensor(un + ".in", u.src, u.N, u.h, u.w, u.C); ws.tensor(un + ".Y", u.out, u.N, 2 * u.h, 2 * u.w, u.C);
        ws.tensor(un + ".dY", u.dOut, u.N, 2 * u.h, 2 * u.w, u.C); ws.tensor(un + ".dIn", u.tmp, u.N, u.h, u.w, u.C);
    }
    e.sn_dbg_dE = dbg ? ws.plain(B, H, W, c4) : TRef{};
    if (conc) {
        ws.tensor("head.in", e.snE, B, H, W, c4); ws.tensor("head.dIn", e.sn_dbg_dE, B, H, W, c4);
    } else {
        ws.tensor("ecam.in", e.snE, B, H, W, c4); ws.tensor("ecam.Y", e.snZ, B, H, W, c4); ws.tensor("ecam.dY", e.sndZ, B, H, W, c4);
        ws.tensor("ecam.dIn", e.sn_dbg_dE, B, H, W, c4); ws.tensor("conv_final.dY", e.G, B, H, W, 8);
    }
    return 0;
}

static void sn_block_forward(const Ctx& c, const NBlock& b, float* bn_running, bool training) {
    stcd_engine& e = c.e;
    const int64_t T = (int64_t)dsize(e.dt), px = (int64_t)b.N * b.H * b.W, ppg = (int64_t)b.npg * b.H * b.W;
    const double act_bytes = (double)px * b.C * (double)T;
    (void)px; (void)T;      // (the concat prefix of b.in was written by the producers: NBlock::extra_dst)
    BnActArgs a;
    auto bn_stage = [&](const ConvOp& f, const void* in, int conv, int bni, const TRef& Y, int64_t facc_off) {
        long long* const facc = training ? c.at<long long>(facc_off) : nullptr;
        exec_conv_stats(c, f, conv_args(in, c.at(Y.off), c.params + e.convs[conv].b_off), facc, b.groups, b.C, Y, ppg, act_bytes);
        bn_fields(a, c, e.bns[bni], b.C, bn_running, facc);
    };
    bn_stage(b.f1, c.at(b.in.off), b.c1, b.bn1, b.Y1, b.facc1);
    a.Y = c.at(b.Y1.off); a.ldy = b.Y1.ld; a.A = c.at(b.A1.off); a.lda = b.A1.ld; a.a_group_off = ppg * b.A1.ld;
    a.P = nullptr; a.ldp = 0; a.stat = c.at<float>(b.stat1); a.mask = nullptr;
    a.C = b.C; a.groups = b.groups; a.npg = b.npg; a.H = b.H; a.W = b.W; a.relu = 1;
    {
        ProfScope ps(c, PC_BN_ACT, 0.0, 2.0 * act_bytes);
        launch_bn_act(e.dt, a, c.s);
    }
    bn_stage(b.f2, c.at(b.A1.off), b.c2, b.bn2, b.Y2, b.facc2);
    a.Y = c.at(b.Y2.off); a.ldy = b.Y2.ld; a.A = c.at(b.Out.off); a.lda = b.Out.ld; a.a_group_off = ppg * b.Out.ld;
    a.P = b.pool ? c.at(b.P.off) : nullptr; a.ldp = b.P.ld; a.stat = c.at<float>(b.stat2);
    a.res = c.at(b.Y1.off); a.ldres = b.Y1.ld;        // identity = conv1's raw output (SNUNet.py:19,25)
    a.extra.n = (int)b.extra_dst.size();
    for (int k = 0; k < a.extra.n; ++k) {
        a.extra.p[k] = c.at(b.extra_dst[k].off); a.extra.ld[k] = b.extra_dst[k].ld; a.extra.goff[k] = b.extra_dst[k].goff;
        a.extra.gmask[k] = b.extra_dst[k].gmask;
    }
    {
        ProfScope ps(c, PC_BN_ACT, 0.0, (b.pool ? 3.25 : 3.0) * act_bytes);
        launch_bn_act(e.dt, a, c.s);
    }
}

static void sn_block_backward(const Ctx& c, const NBlock& b) {
    stcd_engine& e = c.e;
    const int64_t T = (int64_t)dsize(e.dt), HW = (int64_t)b.H * b.W, px = (int64_t)b.N * HW, ppg = (int64_t)b.npg * HW;
    const double act_bytes = (double)px * b.C * (double)T;
    const BnP& bn1 = e.bns[b.bn1];
    const BnP& bn2 = e.bns[b.bn2];
    (void)ppg;
    const int64_t goff_out = ppg * b.dOut.ld, goff_a1 = ppg * b.dA1.ld;
    // out = relu(bn2(y2) + y1): gate on z2 + y1; dZ2 (gated) is also the gradient of the identity branch
    {
        ProfScope ps(c, PC_BN_BWD_REDUCE, 0.0, 3.0 * act_bytes);
        SliceViews xs;
        xs.n = (int)b.grad_src.size();
        for (int k = 0; k < xs.n; ++k) {
            xs.p[k] = c.at(b.grad_src[k].off); xs.ld[k] = b.grad_src[k].ld; xs.goff[k] = b.grad_src[k].goff; xs.gmask[k] = b.grad_src[k].gmask;
        }
        launch_bn_bwd_reduce(e.dt, c.at(b.dOut.off), b.dOut.ld, goff_out, c.at(b.Y2.off), b.Y2.ld, c.at<float>(b.stat2), nullptr, b.C,
                             b.groups, b.npg, HW, 1, c.at<long long>(b.bacc2), c.s, c.at(b.Y1.off), b.Y1.ld, &xs, b.grad_base ? 1 : 0,
                             c.at(b.dOut.off));
    }
    if (b.dbg_dOut.off >= 0)         // debug bit 0: keep the gathered sum, which the launch below overwrites in place
        (void)hipMemcpy2DAsync(c.at(b.dbg_dOut.off), (size_t)b.dbg_dOut.ld * T, c.at(b.dOut.off), (size_t)b.dOut.ld * T, (size_t)b.C * T,
                               (size_t)px, hipMemcpyDeviceToDevice, c.s);
    {
        ProfScope ps(c, PC_BN_BWD_APPLY, 0.0, 5.0 * act_bytes);
        launch_bn_bwd_apply(e.dt, c.at(b.dOut.off), b.dOut.ld, goff_out, c.at(b.dOut.off), b.dOut.ld, c.at(b.Y2.off), b.Y2.ld,
                            c.at<float>(b.stat2), c.at<long long>(b.bacc2), c.grads + bn2.g_off, c.grads + bn2.b_off, nullptr, b.C,
                            b.groups, b.npg, HW, 1, c.s, c.at(b.Y1.off), b.Y1.ld, c.at(b.dZ2.off), b.dZ2.ld, nullptr, 0,
                            c.grads + e.convs[b.c1].b_off);
    }
    exec_wgrad(c, b.w2, c.at(b.A1.off), c.at(b.dOut.off));                   // dOut now holds dY2
    exec_conv(c, b.d2, conv_args(c.at(b.dOut.off), c.at(b.dA1.off)));
    {
        ProfScope ps(c, PC_BN_BWD_REDUCE, 0.0, 2.0 * act_bytes);
        launch_bn_bwd_reduce(e.dt, c.at(b.dA1.off), b.dA1.ld, goff_a1, c.at(b.Y1.off), b.Y1.ld, c.at<float>(b.stat1), nullptr, b.C,
                             b.groups, b.npg, HW, 1, c.at<long long>(b.bacc1), c.s);
    }
    {
        ProfScope ps(c, PC_BN_BWD_APPLY, 0.0, 4.0 * act_bytes);
        launch_bn_bwd_apply(e.dt, c.at(b.dA1.off), b.dA1.ld, goff_a1, c.at(b.dA1.off), b.dA1.ld, c.at(b.Y1.off), b.Y1.ld,
                            c.at<float>(b.stat1), c.at<long long>(b.bacc1), c.grads + bn1.g_off, c.grads + bn1.b_off, nullptr, b.C,
                            b.groups, b.npg, HW, 1, c.s, nullptr, 0, nullptr, 0, c.at(b.dZ2.off), b.dZ2.ld);
    }
    // conv1's bias reaches the loss only through the identity branch (its BN path has zero gradient): db1 = sum dZ2,
    // and dZ2 is exactly the gated gradient whose per-channel sum bn2's backward already formed as d(beta2): bn2's apply
    // kernel wrote it to both places (a 128-byte hipMemcpyAsync cost three copy kernels per block, 44 launches per step)
    exec_wgrad(c, b.w1, c.at(b.in.off), c.at(b.dA1.off));                   // dA1 now holds dY1
    if (b.dIn.off >= 0) {
        ConvArgs a = conv_args(c.at(b.dA1.off), c.at(b.dIn.off));
        if (b.d1_sum_acc >= 0) a.sums = StatReq{c.at<long long>(b.d1_sum_acc), 1, b.d1_sum_c0, b.d1_sum_C, BN_BS, BN_BS};
        exec_conv(c, b.d1, a);
    }
}

static void sn_up_forward(const Ctx& c, const SnUp& u) {
    const ConvW& cv = c.e.convs[u.conv];
    if (exec_conv_x4(c, u.fwd, c.at(u.src.off), c.params + cv.b_off, c.at(u.out.off))) return;
    for (int ph = 0; ph < 4; ++ph) exec_conv(c, u.fwd[ph], conv_args(c.at(u.src.off), c.at(u.out.off), c.params + cv.b_off));
}
static void sn_up_backward(const Ctx& c, const SnUp& u) {
    stcd_engine& e = c.e;
    const ConvW& cv = e.convs[u.conv];
    const int64_t T = (int64_t)dsize(e.dt);
    if (!(u.bias_fused && mfma_on(e)))
        launch_bias_grad(e.dt, c.at(u.dOut.off), u.dOut.ld, (int64_t)u.N * 4 * u.h * u.w, u.C, c.grads + cv.b_off, c.s,
                         e.dt == BF16 ? c.at<long long>(u.bias_acc) : nullptr);
    for (int ph = 0; ph < 4; ++ph) exec_wgrad(c, u.wg[ph], c.at(u.src.off), c.at(u.dOut.off));
    exec_conv(c, u.dgr, conv_args(c.at(u.dOut.off), c.at(u.tmp.off)));     // summed into the lower block's dOut by ITS reduction
    (void)T;
}

static SnHeadParams sn_head_params(const stcd_engine& e, const float* params) {
    SnHeadParams p;
    for (int i = 0; i < 4; ++i) { p.w[i] = params + e.snc_w[i]; p.b[i] = params + e.snc_b[i]; }
    p.wf = params + e.snc_w[4]; p.bf = params + e.snc_b[4];
    p.L = e.label; p.ds = sn_out_maps(e.arch) > 1;
    return p;
}

static int forward_snunet(stcd_engine& e, const float* x1, const float* x2, const float* params, float* bn_running, int training,
                          float* logits, void* workspace, hipStream_t s) {
    Ctx c{e, (char*)workspace, params, nullptr, s};
    if (pack_all_weights(c, training != 0)) return 1;
    if (training) STCD_HIP(hipMemsetAsync(c.at(e.zero_begin), 0, e.zero_end - e.zero_begin, s));
    launch_in_pack(e.dt, x1, x2, c.at(e.X0.off), e.B, e.in_ch, e.H, e.W, s);
    for (int bi : e.sn_order) {
        const NBlock& b = e.sn_blocks[bi];
        if (b.up >= 0) sn_up_forward(c, e.sn_ups[b.up]);
        sn_block_forward(c, b, bn_running, training != 0);
    }
    if (is_snconc(e.arch)) {
        ProfScope ps(c, PC_CONV, 2.0 * e.B * e.H * e.W * 128.0 * sn_out_maps(e.arch) * e.label,
                     (double)e.B * e.H * e.W * (128.0 * dsize(e.dt) + 4.0 * sn_out_maps(e.arch) * e.label), "k_snhead_fwd");
        launch_snhead_forward(e.dt, c.at(e.snE.off), e.snE.ld, sn_head_params(e, params), logits, e.B, (int64_t)e.H * e.W, s);
        STCD_HIP(hipGetLastError());
        return 0;
    }
    const int c4 = SN_F[0] * 4;
    launch_ecam_forward(e.dt, c.at(e.snE.off), e.snE.ld, c.at(e.snZ.off), e.snZ.ld, e.B, (int64_t)e.H * e.W, c4, params + e.sn_w[0],
                        params + e.sn_w[1], params + e.sn_w[2], params + e.sn_w[3], c.at<float>(e.sn_pool), c.at<int64_t>(e.sn_argm),
                        c.at<float>(e.sn_att), c.at<float>(e.sn_hid), c.at<float>(e.sn_part), s);
    exec_conv(c, e.sn_final_fwd, conv_args(c.at(e.snZ.off), logits, params + e.convs[e.sn_final].b_off, true));
    STCD_HIP(hipGetLastError());
    return 0;
}

static int backward_snunet(stcd_engine& e, const float* grad_logits, const float* params, float* grads, void* workspace, int stage,
                           hipStream_t s) {
    if (stage == 1) return 0;            // single-stage plan: everything is final after stage 0 / -1
    Ctx c{e, (char*)workspace, params, grads, s};
    // single call, no gradient hook: the grouped weight gradients go out with their last member on the engine's side stream (the
    // groups whose members all sit deep in the backward order -- the GEMM groups, the 32 x 32 tile group -- run beside the rest of
    // the chain: 13.22 -> 12.80 ms; cutting the groups into buckets of the backward order, or smaller grids, added nothing)
    hipStream_t side = stage < 0 ? wgrad_side_stream(e, s) : nullptr;
    WgradScope wgrad_scope(e, stage, mfma_on(e) && e.use_wgroup, side);
    const int dt = e.dt, B = e.B;
    const int64_t T = (int64_t)dsize(dt);
    const int c4 = SN_F[0] * 4;
    STCD_HIP(hipMemsetAsync(grads, 0, e.param_floats * 4, s));
    if (!mfma_on(e)) STCD_HIP(hipMemsetAsync(c.at(e.dwe_begin), 0, e.dwe_end - e.dwe_begin, s));
    // (no bulk zeroing of the dOut buffers: each is fully written -- max-pool / ECAM gradient, or the gathered sum)
    for (auto& b : e.sn_blocks)          // pooled gradients of the A half of conv3_0 never get written (x4_0A does not exist)
        if (b.pool && b.name == "conv3_0") STCD_HIP(hipMemsetAsync(c.at(b.dP.off), 0, (int64_t)B * (b.H / 2) * (b.W / 2) * b.C * T, s));
    if (is_snconc(e.arch)) {
        const double px = (double)B * e.H * e.W, no = (double)sn_out_maps(e.arch) * e.label;
        ProfScope ps(c, PC_CONV, 4.0 * px * 128.0 * no, px * (256.0 * (double)T + 4.0 * no), "k_snhead_bwd|k_snhead_reduce|k_snhead_chain");
        SnHeadGrads hg;
        for (int i = 0; i < 4; ++i) { hg.w[i] = grads + e.snc_w[i]; hg.b[i] = grads + e.snc_b[i]; }
        hg.wf = grads + e.snc_w[4]; hg.bf = grads + e.snc_b[4];
        launch_snhead_backward(dt, c.at(e.snE.off), e.snE.ld, sn_head_params(e, params), hg, grad_logits, c.at(e.sndE.off), e.sndE.ld,
                               c.at<float>(e.snc_scratch), B, (int64_t)e.H * e.W, s);
    } else {
        launch_gout_pack(dt, grad_logits, c.at(e.G.off), B, e.label, e.H, e.W, s, c.at<long long>(e.final_bias_acc));
        exec_wgrad(c, e.sn_final_wg, c.at(e.snZ.off), c.at(e.G.off));
        exec_conv(c, e.sn_final_dgr, conv_args(c.at(e.G.off), c.at(e.sndZ.off)));
        launch_ecam_backward(dt, c.at(e.snE.off), e.snE.ld, c.at(e.sndZ.off), e.sndZ.ld, c.at(e.sndE.off), e.sndE.ld, B, (int64_t)e.H * e.W, c4,
                             params + e.sn_w[0], params + e.sn_w[1], params + e.sn_w[2], params + e.sn_w[3], grads + e.sn_w[0],
                             grads + e.sn_w[1], grads + e.sn_w[2], grads + e.sn_w[3], c.at<float>(e.sn_pool), c.at<int64_t>(e.sn_argm),
                             c.at<float>(e.sn_att), c.at<float>(e.sn_hid), c.at<float>(e.sn_sums), c.at<float>(e.sn_dpool), c.at<float>(e.sn_part), s);
    }
    if (e.sn_dbg_dE.off >= 0)        // debug bit 0: the head's data gradient, before conv0_1..conv0_4 gather into it
        STCD_HIP(hipMemcpyAsync(c.at(e.sn_dbg_dE.off), c.at(e.sndE.off), (int64_t)B * e.H * e.W * c4 * T, hipMemcpyDeviceToDevice, s));
    for (int oi = (int)e.sn_order.size() - 1; oi >= 0; --oi) {
        const NBlock& b = e.sn_blocks[e.sn_order[oi]];
        if (b.pool) {    // gradient coming back through the 2x2 max-pool of this encoder output
            ProfScope ps(c, PC_POOL_FUSE, 0.0, 3.25 * b.N * b.H * b.W * b.C * (double)T);
            const int64_t goff = (int64_t)b.npg * b.H * b.W;
            launch_pool_bwd(dt, c.at(b.Out.off), b.Out.ld, goff * b.Out.ld, c.at(b.dP.off), b.dP.ld, c.at(b.dOut.off), b.dOut.ld,
                            goff * b.dOut.ld, b.groups, b.npg, b.H, b.W, b.C, 0, s);
        }
        sn_block_backward(c, b);       // (its concat gradient b.dIn is gathered by the producers' reductions later on)
        if (b.up >= 0) sn_up_backward(c, e.sn_ups[b.up]);
    }
    if (stage_tail(c, 0, side, true, finish_biases)) return 1;
    STCD_HIP(hipGetLastError());
    return 0;
}


// ================================================================================================ SegCD (ResNet-50 UNet)
// smp.SegCD(encoder_name="resnet50"): the model the reference's scripts train (train_pse_cd.py:419-427, train_stcd.py:631-638).
//   SegCD.forward            /root/reference/segmentation_models_pytorch/decoders/unet/model.py:316-332
//   ResNet-50 encoder        /root/reference/segmentation_models_pytorch/encoders/resnet.py:37-70, /root/reference/models/resnet.py:78-190
//   UnetDecoder              /root/reference/segmentation_models_pytorch/decoders/unet/decoder.py:8-123
// Both dates run as ONE batch of 2B images through the shared encoder + decoder (every BatchNorm keeps per-date statistics:
// the modules are called once per date); only the head combines them.  Gradients of tensors with several consumers
// (identity branches, decoder skips) are never accumulated by extra kernels: every consumer writes its own contribution
// buffer and the producer's BatchNorm-backward reduction gathers them (SliceViews).
static const int RS_PLANES[4] = {64, 128, 256, 512};
static bool is_unetseg(int arch) { return arch >= STCD_ARCH_UNETSEG && arch <= STCD_ARCH_UNETSEG + 4; }
static bool is_ffctlcd(int arch) { return arch >= STCD_ARCH_FFCTLCD && arch <= STCD_ARCH_FFCTLCD + 4; }
static bool is_bit(int arch) { return arch >= STCD_ARCH_BIT && arch <= STCD_ARCH_BIT + 2; }
static bool is_bres(int arch) { return (arch >= STCD_ARCH_BASE_RESNET && arch <= STCD_ARCH_BASE_RESNET + 3) || is_bit(arch); }
static bool is_segcd(int arch) { return (arch >= STCD_ARCH_SEGCD && arch <= STCD_ARCH_SEGCD_R152) || is_unetseg(arch) || is_ffctlcd(arch) || is_bres(arch); }
// stride of block b of residual stage li: (1,2,2,2); base_resnet (replace_stride_with_dilation=[False,True,True] on BasicBlock, which
// keeps dilation 1: models/resnet.py:47-48) stays at 1/8 resolution: (1,2,1,1)
static int seg_stride(const stcd_engine& e, int li, int b) { return (b == 0 && (e.bres ? li == 1 : li > 0)) ? 2 : 1; }

static const int SEG_DEC[5] = {256, 128, 64, 32, 16};

static int add_glayer(stcd_engine& e, const std::string& conv_name, const std::string& bn_name, int kind, int cin, int cout, bool relu,
                      bool need_dgrad, int bn_calls = 0) {
    GLayer L;
    L.name = conv_name; L.kind = kind; L.relu = relu; L.has_dIn = need_dgrad;
    L.conv = add_conv(e, conv_name, kind, cin, cout, need_dgrad, false);
    L.bn = add_bn(e, bn_name, cout, bn_calls ? bn_calls : e.seg_dates);
    e.g_layers.push_back(L);
    return (int)e.g_layers.size() - 1;
}

// encoders/resnet.py:126-171: block type and depths of the plain ResNet registry entries
static void segcd_encoder_cfg(stcd_engine& e) {
    static const int L18[4] = {2, 2, 2, 2}, L34[4] = {3, 4, 6, 3}, L101[4] = {3, 4, 23, 3}, L152[4] = {3, 8, 36, 3};
    const int* l = L34;
    e.seg_x = 4;
    e.seg_dates = is_unetseg(e.arch) ? 1 : 2;
    e.seg_ffc = is_ffctlcd(e.arch);
    e.bres = is_bres(e.arch); e.seg_nstage = 4; e.g_head_c = 16;
    if (e.bres) {      // STCD_ARCH_BASE_RESNET + k: (resnet18, resnet34) x (5, 4 stages); STCD_ARCH_BIT + k: resnet18, 4 stages
        e.bit.on = is_bit(e.arch);
        if (e.bit.on) { e.bit.L = e.arch == STCD_ARCH_BIT ? 1 : 8; e.bit.dh = e.arch == STCD_ARCH_BIT + 2 ? 8 : 64; }
        const int k = e.bit.on ? 1 : e.arch - STCD_ARCH_BASE_RESNET;
        e.seg_x = 1; e.seg_nstage = (k & 1) ? 3 : 4; e.g_head_c = 32;
        for (int i = 0; i < 4; ++i) e.seg_layers[i] = (k >> 1) ? L34[i] : L18[i];
        return;
    }
    switch (is_unetseg(e.arch) ? e.arch - STCD_ARCH_UNETSEG + STCD_ARCH_SEGCD
            : is_ffctlcd(e.arch) ? e.arch - STCD_ARCH_FFCTLCD + STCD_ARCH_SEGCD : e.arch) {      // same encoder order in every id range
        case STCD_ARCH_SEGCD_R18: e.seg_x = 1; l = L18; break;
        case STCD_ARCH_SEGCD_R34: e.seg_x = 1; l = L34; break;
        case STCD_ARCH_SEGCD_R101: l = L101; break;
        case STCD_ARCH_SEGCD_R152: l = L152; break;
        default: break;                                                // resnet50: Bottleneck, [3, 4, 6, 3]
    }
    for (int i = 0; i < 4; ++i) e.seg_layers[i] = l[i];
}

static void build_segcd_tables(stcd_engine& e) {
    segcd_encoder_cfg(e);
    const int X = e.seg_x;
    e.g_layers.clear(); e.g_blocks.clear(); e.g_dec.clear();
    const std::string enc = e.bres ? "resnet." : "encoder.";
    if (e.bit.on) add_param(e, "pos_embedding", {1, 8, 32}, &e.bit.pos_off);      // a parameter of the root module: first in named_parameters()
    e.g_stem = add_glayer(e, enc + "conv1", enc + "bn1", K_STEM7, e.in_ch, 64, true, false);
    int inpl = 64;
    for (int li = 0; li < 4; ++li)
        for (int b = 0; b < e.seg_layers[li]; ++b) {
            const int w = RS_PLANES[li], stride = seg_stride(e, li, b);
            const std::string pre = enc + "layer" + std::to_string(li + 1) + "." + std::to_string(b);
            // ResNet._make_layer (models/resnet.py:165-187): a down-sample where the stride or the width changes
            const bool down = b == 0 && (stride != 1 || inpl != w * X);
            if (li >= e.seg_nstage) {      // base_resnet with 4 stages: layer4 stays in the state_dict and is never run -- parameters
                int64_t off;               // only (no layer, no BatchNorm buffer of the engine), their gradient stays zero
                add_param(e, pre + ".conv1.weight", {w, inpl, 3, 3}, &off);
                add_param(e, pre + ".bn1.weight", {w}, &off); add_param(e, pre + ".bn1.bias", {w}, &off);
                add_param(e, pre + ".conv2.weight", {w, w, 3, 3}, &off);
                add_param(e, pre + ".bn2.weight", {w}, &off); add_param(e, pre + ".bn2.bias", {w}, &off);
                if (down) {
                    add_param(e, pre + ".downsample.0.weight", {w, inpl, 1, 1}, &off);
                    add_param(e, pre + ".downsample.1.weight", {w}, &off); add_param(e, pre + ".downsample.1.bias", {w}, &off);
                }
                inpl = w;
                continue;
            }
            std::array<int, 4> blk;
            if (X == 4) {      // Bottleneck (models/resnet.py:78-124): 1x1, 3x3 (carries the stride), 1x1
                blk[0] = add_glayer(e, pre + ".conv1", pre + ".bn1", K_CONV1, inpl, w, true, true);
                blk[1] = add_glayer(e, pre + ".conv2", pre + ".bn2", stride == 2 ? K_CONV3_S2 : K_CONV3, w, w, true, true);
                blk[2] = add_glayer(e, pre + ".conv3", pre + ".bn3", K_CONV1, w, 4 * w, true, true);
            } else {           // BasicBlock (models/resnet.py:37-75): 3x3 (carries the stride), 3x3
                blk[0] = add_glayer(e, pre + ".conv1", pre + ".bn1", stride == 2 ? K_CONV3_S2 : K_CONV3, inpl, w, true, true);
                blk[1] = -1;
                blk[2] = add_glayer(e, pre + ".conv2", pre + ".bn2", K_CONV3, w, w, true, true);
            }
            blk[3] = down ? add_glayer(e, pre + ".downsample.0", pre + ".downsample.1", stride == 2 ? K_CONV1_S2 : K_CONV1, inpl, X * w, false, true) : -1;
            e.g_blocks.push_back(blk);
            inpl = X * w;
        }
    if (e.bres) {      // registration order of ResNet.__init__ (models/networks.py:231-262): resnet (with its unused fc), classifier, conv_pred
        int64_t off;
        add_param(e, "resnet.fc.weight", {1000, 512}, &off);
        add_param(e, "resnet.fc.bias", {1000}, &off);
        // TwoLayerConv2d (models/help_funcs.py): conv3x3 without bias, BatchNorm2d, ReLU, conv3x3 with bias; called once per forward
        e.g_cls = add_glayer(e, "classifier.0", "classifier.1", K_CONV3, 32, 32, true, true, 1);
        e.g_head_conv = add_conv(e, "classifier.3", K_CONV3, 32, e.label, true, true);
        e.g_pred_conv = add_conv(e, "conv_pred", K_CONV3, RS_PLANES[e.seg_nstage - 1], 32, true, true);
        e.enc_param_end = 0;
        if (e.bit.on) {      // BASE_Transformer.__init__ (models/networks.py:324-357): conv_a, transformer, transformer_decoder
            int64_t off;
            add_param(e, "conv_a.weight", {4, 32, 1, 1}, &e.bit.wa_off);
            auto layer = [&](const std::string& pre, int I, bool cross) {      // the block kernels_bit.hip's bit_off() describes
                int64_t first;
                add_param(e, pre + "0.fn.norm.weight", {32}, &first); add_param(e, pre + "0.fn.norm.bias", {32}, &off);
                if (cross) {
                    add_param(e, pre + "0.fn.fn.to_q.weight", {I, 32}, &off); add_param(e, pre + "0.fn.fn.to_k.weight", {I, 32}, &off);
                    add_param(e, pre + "0.fn.fn.to_v.weight", {I, 32}, &off);
                } else add_param(e, pre + "0.fn.fn.to_qkv.weight", {3 * I, 32}, &off);
                add_param(e, pre + "0.fn.fn.to_out.0.weight", {32, I}, &off); add_param(e, pre + "0.fn.fn.to_out.0.bias", {32}, &off);
                add_param(e, pre + "1.fn.norm.weight", {32}, &off); add_param(e, pre + "1.fn.norm.bias", {32}, &off);
                add_param(e, pre + "1.fn.fn.net.0.weight", {64, 32}, &off); add_param(e, pre + "1.fn.fn.net.0.bias", {64}, &off);
                add_param(e, pre + "1.fn.fn.net.3.weight", {32, 64}, &off); add_param(e, pre + "1.fn.fn.net.3.bias", {32}, &off);
                return first;
            };
            e.bit.enc_off = layer("transformer.layers.0.", 512, false);
            for (int l = 0; l < e.bit.L; ++l) {
                const int64_t o = layer("transformer_decoder.layers." + std::to_string(l) + ".", 8 * e.bit.dh, true);
                if (l == 0) e.bit.dec_off = o;
            }
        }
        return;
    }
    const int ENC_OUT[5] = {512 * X, 256 * X, 128 * X, 64 * X, 64};
    int cin = ENC_OUT[0];
    for (int i = 0; i < 5; ++i) {
        const int cskip = i < 4 ? ENC_OUT[i + 1] : 0, cout = SEG_DEC[i];
        const std::string pre = "decoder.blocks." + std::to_string(i);
        std::array<int, 2> d;
        // FFCTLCD (model.py:407-423) runs the decoder three times per forward: |f1 - f2| first, then date 1, then date 2
        d[0] = add_glayer(e, pre + ".conv1.0", pre + ".conv1.1", K_CONV3, cin + cskip, cout, true, true, e.seg_ffc ? 3 : 0);
        d[1] = add_glayer(e, pre + ".conv2.0", pre + ".conv2.1", K_CONV3, cout, cout, true, true, e.seg_ffc ? 3 : 0);
        e.g_dec.push_back(d);
        cin = cout;
    }
    e.g_head_conv = add_conv(e, "segmentation_head.0", K_CONV3, SEG_DEC[4], e.label, true, true);
    e.enc_param_end = 0;      // one backward stage
}

static int configure_segcd(stcd_engine& e, int B, int H, int W) {
    const int64_t T = (int64_t)dsize(e.dt);
    const int D = e.seg_dates, N = D * B;
    Planner ws(e);
    auto view = [&](const TRef& t, int coff, int ld, int h, int w) {       // both dates of a plain [2B,h,w,ld] tensor, channel offset coff
        ViewRef v; v.off = t.off + (int64_t)coff * T; v.ld = ld; v.goff = D == 2 ? (int64_t)B * h * w * ld : 0; v.gmask = D == 2 ? 3 : 1; return v;
    };
    for (auto& L : e.g_layers) { L.extra_dst.clear(); L.grad_src.clear(); L.grad_base = true; L.res = TRef(); L.dRes = TRef(); L.ndgr = 0; }
    e.X0 = ws.plain(N, H, W, 8);
    // ---- shapes + activation buffers, forward order
    auto shape = [&](GLayer& L, const TRef& in, int K, int hi, int wi, int stride, int ng = 0) {
        const ConvW& cv = e.convs[L.conv];
        if (ng == 0) ng = D;
        const int n = ng * B;
        L.N = n; L.groups = ng; L.npg = B; L.in = in; L.K = K; L.Hi = hi; L.Wi = wi; L.Ho = hi / stride; L.Wo = wi / stride; L.C = cv.cout;
        L.Y = ws.plain(n, L.Ho, L.Wo, L.C); L.A = ws.plain(n, L.Ho, L.Wo, L.C); L.dA = ws.plain(n, L.Ho, L.Wo, L.C);
        L.stat = ws.take((int64_t)std::max(2, ng) * 4 * L.C * 4); L.coef = ws.take((int64_t)std::max(2, ng) * 5 * L.C * 4);
        L.g_first = 0;
    };
    GLayer& S = e.g_layers[e.g_stem];
    shape(S, e.X0, 8, H, W, 2);
    S.has_dIn = false;
    { GStep st; st.kind = GS_LAYER; st.layer = e.g_stem; e.g_fwd.push_back(st); }
    e.gP0 = ws.plain(N, H / 4, W / 4, 64); e.gdP0 = ws.plain(N, H / 4, W / 4, 64);
    e.g_pool_idx = ws.take((int64_t)N * (H / 4) * (W / 4) * 64);
    e.g_stem_part = ws.take(stem_wgrad_part_floats(N, H, W, e.in_ch, 64) * 4);
    { GStep st; st.kind = GS_MAXPOOL; st.src = S.A; st.dst = e.gP0; st.dsrc = S.dA; st.ddst = e.gdP0; st.N = N; st.h = H / 2; st.w = W / 2; st.C = 64; e.g_fwd.push_back(st); }
    TRef cur = e.gP0; int curC = 64, h = H / 4, w = W / 4, prev_out = -1;      // prev_out: layer whose A is `cur` (-1: the max-pool)
    std::vector<int> stage_out;                                               // L3 of the last block of layer1..4
    size_t bi = 0;
    for (int li = 0; li < e.seg_nstage; ++li)
        for (int b = 0; b < e.seg_layers[li]; ++b, ++bi) {
            const std::array<int, 4>& blk = e.g_blocks[bi];
            const int stride = seg_stride(e, li, b);
            const int ho = h / stride, wo = w / stride;
            GLayer& L1 = e.g_layers[blk[0]]; GLayer& L3 = e.g_layers[blk[2]];
            GLayer* L2 = blk[1] >= 0 ? &e.g_layers[blk[1]] : nullptr;
            if (L2) {          // Bottleneck: the 3x3 in the middle carries the stride
                shape(L1, cur, curC, h, w, 1);
                shape(*L2, L1.A, L1.C, h, w, stride);
            } else {           // BasicBlock: the first 3x3 carries it
                shape(L1, cur, curC, h, w, stride);
            }
            if (blk[3] >= 0) { GLayer& Ld = e.g_layers[blk[3]]; shape(Ld, cur, curC, h, w, stride); }
            GLayer& Lm = L2 ? *L2 : L1;                                        // producer of the last conv's input
            shape(L3, Lm.A, Lm.C, ho, wo, 1);
            L3.res = blk[3] >= 0 ? e.g_layers[blk[3]].A : cur;
            // gradient wiring: single-consumer tensors are written in place, the block input gets contribution buffers
            if (e.debug_flags & 1) {
                if (L2) { L2->dIn = ws.plain(N, h, w, L1.C); L1.grad_base = false; L1.grad_src.push_back(view(L2->dIn, 0, L1.C, h, w)); }
                L3.dIn = ws.plain(N, ho, wo, Lm.C); Lm.grad_base = false; Lm.grad_src.push_back(view(L3.dIn, 0, Lm.C, ho, wo));
            } else { if (L2) L2->dIn = L1.dA; L3.dIn = Lm.dA; }
            L1.dIn = (prev_out < 0) ? e.gdP0 : ws.plain(N, h, w, curC);
            TRef idc;                                                          // identity-branch contribution to d(cur)
            if (blk[3] >= 0) { GLayer& Ld = e.g_layers[blk[3]]; L3.dRes = Ld.dA; Ld.dIn = ws.plain(N, h, w, curC); idc = Ld.dIn; }
            else { L3.dRes = ws.plain(N, h, w, curC); idc = L3.dRes; }
            if (prev_out >= 0) {
                GLayer& Pv = e.g_layers[prev_out];
                Pv.grad_base = false;
                Pv.grad_src.push_back(view(L1.dIn, 0, curC, h, w));
                Pv.grad_src.push_back(view(idc, 0, curC, h, w));
            } else e.g_pool_idc = idc;
            { GStep st; st.layer = blk[0]; e.g_fwd.push_back(st); }
            if (L2) { GStep st; st.layer = blk[1]; e.g_fwd.push_back(st); }
            if (blk[3] >= 0) { GStep st; st.layer = blk[3]; e.g_fwd.push_back(st); }
            { GStep st; st.layer = blk[2]; e.g_fwd.push_back(st); }
            cur = L3.A; curC = L3.C; h = ho; w = wo; prev_out = blk[2];
            if (b == e.seg_layers[li] - 1) stage_out.push_back(blk[2]);
        }
    if (e.bres) {
        // ---- base_resnet tail (models/networks.py:267-304): per date nearest x2 + conv_pred, |x1 - x2|, bilinear x4, classifier
        GLayer& X = e.g_layers[stage_out.back()];
        X.grad_base = true;                                                                 // the up-sampling gradient alone
        const int Ct = X.C, h4 = 2 * X.Ho, w4 = 2 * X.Wo;
        GStep up; up.kind = GS_UPSAMPLE; up.src = X.A; up.dsrc = X.dA; up.dst = ws.plain(N, h4, w4, Ct); up.ddst = ws.plain(N, h4, w4, Ct);
        up.N = N; up.h = X.Ho; up.w = X.Wo; up.C = Ct; e.g_fwd.push_back(up);
        GStep cp; cp.kind = GS_BCONV; cp.src = up.dst; cp.dsrc = up.ddst; cp.dst = ws.plain(N, h4, w4, 32); cp.ddst = ws.plain(N, h4, w4, 32);
        cp.N = N; cp.h = h4; cp.w = w4; cp.C = Ct; e.g_fwd.push_back(cp);
        TRef pair_src = cp.dst, pair_dsrc = cp.ddst;      // what |x1 - x2| reads and where its backward writes
        if (e.bit.on) {      // tokenizer -> token encoder -> decoder; the differencing then reads the decoder's output
            auto& b = e.bit;
            const int n = h4 * w4, L = b.L;
            b.tok_in = ws.take((int64_t)N * 128 * 4); b.tok_out = ws.take((int64_t)N * 128 * 4);
            b.dtok_out = ws.take((int64_t)N * 128 * 4); b.dtok_in = ws.take((int64_t)N * 128 * 4);
            b.stat = ws.take((int64_t)N * 8 * 4);
            b.AP = ws.take((int64_t)L * N * 2048 * 4); b.dAP = ws.take((int64_t)L * N * 2048 * 4);
            b.xs = ws.take((int64_t)std::max(1, L - 1) * N * n * 32 * T);
            b.dG = ws.take((int64_t)N * n * 32 * 4);
            b.dec_part = ws.take(bit_dec_part_floats(n, N, L) * 4);
            b.dmh = ws.take((int64_t)L * N * 8 * 128 * 4); b.dm = ws.take((int64_t)L * N * 128 * 4);
            b.enc_part = ws.take(bit_enc_part_floats(B, 64) * 4);
            b.tok_part = ws.take((int64_t)N * 128 * 4);
            b.dec_din = ws.plain(N, h4, w4, 32);
            GStep tk; tk.kind = GS_TOKENIZE; tk.src = cp.dst; tk.dsrc = cp.ddst; tk.N = N; tk.h = h4; tk.w = w4; tk.C = 32; e.g_fwd.push_back(tk);
            GStep te; te.kind = GS_TOKENENC; te.N = N; e.g_fwd.push_back(te);
            GStep td; td.kind = GS_TOKENDEC; td.src = cp.dst; td.dsrc = b.dec_din; td.dst = ws.plain(N, h4, w4, 32); td.ddst = ws.plain(N, h4, w4, 32);
            td.N = N; td.h = h4; td.w = w4; td.C = 32; e.g_fwd.push_back(td);
            pair_src = td.dst; pair_dsrc = td.ddst;      // the differencing reads the decoder's output, not conv_pred's
        }
        GStep ab; ab.kind = GS_ABSPAIR; ab.src = pair_src; ab.dsrc = pair_dsrc; ab.dst = ws.plain(B, h4, w4, 32); ab.ddst = ws.plain(B, h4, w4, 32);
        ab.N = B; ab.h = h4; ab.w = w4; ab.C = 32; e.g_fwd.push_back(ab);
        GStep bl; bl.kind = GS_BILINEAR; bl.src = ab.dst; bl.dsrc = ab.ddst; bl.dst = ws.plain(B, H, W, 32); bl.ddst = ws.plain(B, H, W, 32);
        bl.N = B; bl.h = h4; bl.w = w4; bl.C = 32; e.g_fwd.push_back(bl);
        GLayer& CL = e.g_layers[e.g_cls];
        shape(CL, bl.dst, 32, H, W, 1, 1);
        CL.dIn = bl.ddst; CL.grad_base = true;                                              // dA: the head's data gradient
        { GStep st; st.layer = e.g_cls; e.g_fwd.push_back(st); }
        e.gX3 = CL.A; e.gdX3 = CL.dA;
        e.G = ws.plain(B, H, W, 8);
    } else {
    // ---- decoder: x = f5; block i: nearest x2 into cat_i[:, :Cx], skip (written by its encoder producer) in cat_i[:, Cx:]
    const int skip_layer[4] = {stage_out[2], stage_out[1], stage_out[0], e.g_stem};          // f4, f3, f2, f1
    int xl = stage_out[3];                                                                  // layer producing x
    e.g_layers[xl].grad_base = true;                                                        // f5: the up-sampling gradient alone
    const bool ffc = e.seg_ffc;
    const int DG = ffc ? 3 : D, ND = DG * B;                                                // decoder groups / images
    auto absdiff = [&](const TRef& val, const TRef& grad, int coff, int C, int h_, int w_, GLayer& producer) {
        // third group of `val` (channels [coff, coff + C)) = |date 0 - date 1|; its gradient returns to `producer` as a contribution
        TRef tmp = ws.plain(N, h_, w_, C);
        GStep st; st.kind = GS_ABSDIFF; st.N = B; st.h = h_; st.w = w_; st.C = C;
        st.src = val; st.src.off += (int64_t)coff * T; st.dsrc = grad; st.dsrc.off += (int64_t)coff * T; st.ddst = tmp;
        e.g_fwd.push_back(st);
        producer.grad_src.push_back(view(tmp, 0, C, h_, w_));
    };
    if (ffc) {      // x = [f5(date 0); f5(date 1); |f5 - f5|]: the last encoder layer writes the two dates into a 3B-image tensor
        GLayer& X = e.g_layers[xl];
        X.A = ws.plain(ND, X.Ho, X.Wo, X.C); X.dA = ws.plain(ND, X.Ho, X.Wo, X.C);
        absdiff(X.A, X.dA, 0, X.C, X.Ho, X.Wo, X);
    }
    for (int i = 0; i < 5; ++i) {
        GLayer& X = e.g_layers[xl];
        const int Cx = X.C, hh = 2 * X.Ho, ww = 2 * X.Wo;
        const int Cs = i < 4 ? e.g_layers[skip_layer[i]].C : 0;
        TRef cat = ws.plain(ND, hh, ww, Cx + Cs), dcat = ws.plain(ND, hh, ww, Cx + Cs);
        { GStep st; st.kind = GS_UPSAMPLE; st.src = X.A; st.dst = cat; st.dsrc = X.dA; st.ddst = dcat; st.N = ND; st.h = X.Ho; st.w = X.Wo; st.C = Cx; e.g_fwd.push_back(st); }
        if (i < 4) {
            GLayer& Sk = e.g_layers[skip_layer[i]];
            Sk.extra_dst.push_back(view(cat, Cx, Cx + Cs, hh, ww));
            Sk.grad_src.push_back(view(dcat, Cx, Cx + Cs, hh, ww));
            if (ffc) absdiff(cat, dcat, Cx, Cs, hh, ww, Sk);
        }
        GLayer& D1 = e.g_layers[e.g_dec[i][0]]; GLayer& D2 = e.g_layers[e.g_dec[i][1]];
        shape(D1, cat, Cx + Cs, hh, ww, 1, DG);
        shape(D2, D1.A, D1.C, hh, ww, 1, DG);
        if (ffc) D1.g_first = D2.g_first = 2;          // model.py:413-419: decoder(|f1 - f2|) runs before decoder(f1), decoder(f2)
        D1.dIn = dcat;
        if (e.debug_flags & 1) {
            D2.dIn = ws.plain(ND, hh, ww, D1.C); D1.grad_base = false;
            ViewRef v = view(D2.dIn, 0, D1.C, hh, ww);
            if (ffc) v.gmask = 7;
            D1.grad_src.push_back(v);
        } else D2.dIn = D1.dA;
        for (int k : {e.g_dec[i][0], e.g_dec[i][1]}) { GStep st; st.layer = k; e.g_fwd.push_back(st); }
        xl = e.g_dec[i][1];
    }
    // ---- head: X3 = [d1; d2; |d1 - d2|] (3B images), one conv launch; the last decoder layer writes d1, d2 straight into X3
    //      (UnetSeg: X3 = d, B images, the head's output is the network's)
    GLayer& DL = e.g_layers[xl];
    const int nhead = D == 2 ? 3 * B : B;
    e.gX3 = ws.plain(nhead, H, W, 16); e.gdX3 = ws.plain(nhead, H, W, 16);
    DL.A = e.gX3; DL.dA = e.gdX3;
    DL.grad_base = true;
    if (D == 2) {
        if (!ffc) {      // FFCTLCD's last decoder layer already holds [d(f1); d(f2); d(|f1 - f2|)]: the head reads it as it is
            e.gFuseTmp = ws.plain(N, H, W, 16);
            DL.grad_src.push_back(view(e.gFuseTmp, 0, 16, H, W));
        }
        e.g_raw3 = ws.take((int64_t)3 * B * e.label * H * W * 4); e.g_draw3 = ws.take((int64_t)3 * B * e.label * H * W * 4);
    }
    e.G = ws.plain(nhead, H, W, 8);
    }
    for (auto& L : e.g_layers)
        if ((int)L.extra_dst.size() > MAX_VIEWS || (int)L.grad_src.size() > MAX_VIEWS) { set_error("internal: too many views"); return 1; }
    // ---- zero arena: accumulators, tickets-free (consumer-side tables), bias accumulator of the head
    e.zero_begin = ws.cur;
    for (auto& L : e.g_layers) { L.facc = ws.take(bn_acc_bytes(std::max(2, L.groups), L.C)); L.bacc = ws.take(bn_acc_bytes(std::max(2, L.groups), L.C)); }
    e.final_bias_acc = ws.take(bn_acc_bytes(1, 8));
    if (e.bres) e.g_pred_bias_acc = ws.take(bn_acc_bytes(1, 32));
    e.zero_end = ws.cur;
    e.scratch8 = ws.take(256);
    e.masks = ws.take(256);
    take_ref_images(e, ws);
    // ---- bind every conv-shaped launch
    const Binder bind{e, ws};
    // weight gradient of a stride-2 layer over parity plane ph of its input (geom_plane): nt taps (ky, kx) of that parity
    auto bind_plane = [&](WgradOp& op, const GLayer& L, int ci, int ph, int pad, int tap0, int nt, const int8_t* ky, const int8_t* kx, bool own_taps) {
        const stcd_conv_geom gw = geom_plane(L.N, L.Hi, L.Wi, ci, L.in.ld, L.Ho, L.Wo, e.convs[L.conv].cout, L.dA.ld, ph, pad, nt, ky, kx);
        bind.wgrad(op, gw, L.conv, L.in.off + ((int64_t)(ph >> 1) * L.Wi + (ph & 1)) * L.in.ld * T, L.dA.off, 0, tap0, L.Wi / 2,
                   own_taps ? ky : nullptr, own_taps ? kx : nullptr);
    };
    for (auto& L : e.g_layers) {
        if (L.kind == K_STEM7) {
            // 7x7 stride-2 weight gradient on the MFMA path: row 2y + ky - 3 lies in parity plane py = (ky + 1) & 1 at plane row
            // y + (ky - 3 - py) / 2; per plane 3x3 / 3x4 / 4x3 / 4x4 taps, run as stride-1 launches of <= 9 taps over plane views
            // (geom_plane).  fp32 mode (and any plan that does not fit) keeps the dedicated fp32 kernel.
            L.nwg = 0;
            L.fwd = ConvOp();
            if (e.dt == BF16 && e.use_mfma && e.use_gemm)      // forward on the tap-list GEMM kernel over 8-pixel rows
                bind.stem(L.fwd, geom_stem_rows(L.N, L.Hi, L.Wi, L.in.ld, L.Ho, L.Wo, e.convs[L.conv].cout, L.Y.ld), L.conv, L.groups);
            if (!(e.dt == BF16 && e.use_mfma && e.use_wgroup)) continue;
            bool all_ok = true;
            int nops = 0;
            for (int ph = 0; ph < 4 && all_ok; ++ph) {
                const int py = ph >> 1, px = ph & 1;
                std::vector<std::pair<int, int>> taps;
                for (int ky = 0; ky < 7; ++ky)
                    for (int kx = 0; kx < 7; ++kx)
                        if (((ky + 1) & 1) == py && ((kx + 1) & 1) == px) taps.push_back({ky, kx});
                const int nchunk = ((int)taps.size() + 8) / 9, per = ((int)taps.size() + nchunk - 1) / nchunk;
                for (int c0 = 0; c0 < (int)taps.size(); c0 += per) {
                    const int nt = std::min(per, (int)taps.size() - c0);
                    int8_t oky[9], okx[9];
                    for (int t = 0; t < nt; ++t) { oky[t] = (int8_t)taps[c0 + t].first; okx[t] = (int8_t)taps[c0 + t].second; }
                    bind_plane(L.wg[nops], L, 8, ph, 3, 0, nt, oky, okx, true);
                    all_ok = all_ok && L.wg[nops].plan.ok;
                    ++nops;
                }
            }
            if (all_ok) L.nwg = nops;
            else for (int k = 0; k < nops; ++k) e.wgrad_ops.pop_back();
            continue;
        }
        const ConvW& cv = e.convs[L.conv];
        const int stride = L.Hi / L.Ho;
        const bool k3 = L.kind == K_CONV3 || L.kind == K_CONV3_S2;
        // forward (ldo: the conv output's) and, at stride 1, the weight gradient's (ldo: dY's) geometry; stride 2: a gather (3x3 p1 or 1x1)
        auto geom_fwd = [&](int ldo) {
            return stride == 2 ? geom_gather2(L.N, L.Hi, L.Wi, L.K, L.in.ld, L.Ho, L.Wo, cv.cout, ldo, cv.fwd, k3 ? 1 : 0)
                               : k3 ? geom3(L.N, L.Hi, L.Wi, L.K, L.in.ld, cv.cout, ldo) : geom1(L.N, L.Hi, L.Wi, L.K, L.in.ld, cv.cout, ldo);
        };
        bind.conv(L.fwd, geom_fwd(L.Y.ld), L.conv, false, 0, cv.cin, cv.cout, L.groups);
        if (stride == 1) {
            bind.wgrad(L.wg[0], geom_fwd(L.dA.ld), L.conv, L.in.off, L.dA.off);
            L.nwg = 1;
        } else {      // one launch per parity plane of the input: the 1 + 2 + 2 + 4 taps of a 3x3, the one plane (0, 0) of a 1x1
            L.nwg = k3 ? 4 : 1;
            for (int ph = 0; ph < L.nwg; ++ph) {
                const int tap0 = k3 ? PHASE3_TAP0[ph] : 0, nt = k3 ? PHASE3_TAP0[ph + 1] - tap0 : 1;
                bind_plane(L.wg[ph], L, L.K, ph, k3 ? 1 : 0, tap0, nt, cv.fwd.ky + tap0, cv.fwd.kx + tap0, false);
            }
        }
        if (!L.has_dIn) continue;
        if (stride == 1) {
            bind.conv(L.dgr[0], k3 ? geom3(L.N, L.Ho, L.Wo, cv.dgrad.kpad, L.dA.ld, cv.cin, L.dIn.ld)
                                   : geom1(L.N, L.Ho, L.Wo, cv.dgrad.kpad, L.dA.ld, cv.cin, L.dIn.ld), L.conv, true, 0, cv.cout, cv.cin);
            L.ndgr = 1;
        } else if (k3) {      // d(in)(2m+py, 2n+px) = sum_{dy<=py, dx<=px} dY(m+dy, n+dx) W[.][.][py+1-2dy][px+1-2dx]
            for (int ph = 0; ph < 4; ++ph) {
                int tap0;
                const stcd_conv_geom gd = geom_phase3(L.N, L.Ho, L.Wo, cv.dgrad.kpad, L.dA.ld, L.Hi, L.Wi, cv.cin, L.dIn.ld, ph, cv.dgrad, &tap0);
                bind.conv(L.dgr[ph], gd, L.conv, true, tap0, cv.cout, cv.cin);
            }
            L.ndgr = 4;
        } else {              // 1x1 stride 2: only the even positions receive a gradient (the rest is zeroed)
            bind.conv(L.dgr[0], geom_phase(L.N, L.Ho, L.Wo, cv.dgrad.kpad, L.dA.ld, L.Hi, L.Wi, cv.cin, L.dIn.ld, 0, cv.dgrad, 0, 0, 1), L.conv, true, 0, cv.cout, cv.cin);
            L.ndgr = 1;
        }
    }
    {
        const ConvW& cv = e.convs[e.g_head_conv];
        const int nhead = (D == 2 && !e.bres) ? 3 * B : B, hc = e.g_head_c;
        bind.conv(e.g_head_fwd, geom3(nhead, H, W, hc, hc, e.label, e.label), e.g_head_conv, false, 0, hc, e.label);
        bind.wgrad(e.g_head_wg, geom3(nhead, H, W, hc, hc, e.label, 8), e.g_head_conv, e.gX3.off, e.G.off);
        bind.conv(e.g_head_dgr, geom3(nhead, H, W, cv.dgrad.kpad, 8, hc, hc), e.g_head_conv, true, 0, e.label, hc);
    }
    for (const GStep& st : e.g_fwd) {
        if (st.kind != GS_BCONV) continue;
        const ConvW& cv = e.convs[e.g_pred_conv];
        bind.conv(e.g_pred_fwd, geom3(st.N, st.h, st.w, st.C, st.src.ld, 32, st.dst.ld), e.g_pred_conv, false, 0, st.C, 32);
        bind.wgrad(e.g_pred_wg, geom3(st.N, st.h, st.w, st.C, st.src.ld, 32, st.ddst.ld), e.g_pred_conv, st.src.off, st.ddst.off);
        bind.conv(e.g_pred_dgr, geom3(st.N, st.h, st.w, cv.dgrad.kpad, st.ddst.ld, st.C, st.dsrc.ld), e.g_pred_conv, true, 0, 32, st.C);
    }
    for (const auto& L : e.g_layers) {
        ws.tensor(L.name + ".in", L.in, L.N, L.Hi, L.Wi, L.K);
        ws.tensor(L.name + ".Y", L.Y, L.N, L.Ho, L.Wo, L.C);
        ws.tensor(L.name + ".A", L.A, L.N, L.Ho, L.Wo, L.C);
        ws.tensor(L.name + ".dY", L.dA, L.N, L.Ho, L.Wo, L.C);
        if (L.has_dIn) ws.tensor(L.name + ".dIn", L.dIn, L.N, L.Hi, L.Wi, L.K);
        ws.tensor(L.name + ".res", L.res, L.N, L.Ho, L.Wo, L.C);
    }
    for (const GStep& st : e.g_fwd) {      // the base_resnet steps that are no layer
        if (st.kind != GS_BCONV && st.kind != GS_BILINEAR) continue;
        const bool cp = st.kind == GS_BCONV;
        const int ho = cp ? st.h : 4 * st.h, wo = cp ? st.w : 4 * st.w;
        const std::string n = cp ? "conv_pred." : "upsamplex4.";
        ws.tensor(n + "in", st.src, st.N, st.h, st.w, st.C); ws.tensor(n + "Y", st.dst, st.N, ho, wo, 32);
        ws.tensor(n + "dY", st.ddst, st.N, ho, wo, 32); ws.tensor(n + "dIn", st.dsrc, st.N, st.h, st.w, st.C);
    }
    for (const GStep& st : e.g_fwd) {      // the BIT token path: the decoder's maps and the tokens around the encoder (fp32)
        if (st.kind != GS_TOKENDEC) continue;
        ws.tensor("bit.dec.in", st.src.off, 32, st.N, st.h, st.w, 32); ws.tensor("bit.dec.Y", st.dst.off, 32, st.N, st.h, st.w, 32);
        ws.tensor("bit.dec.dY", st.ddst.off, 32, st.N, st.h, st.w, 32); ws.tensor("bit.dec.dIn", st.dsrc.off, 32, st.N, st.h, st.w, 32);
        ws.tensor("bit.tokens.in", e.bit.tok_in, 32, st.N, 1, 4, 32, F32); ws.tensor("bit.tokens.Y", e.bit.tok_out, 32, st.N, 1, 4, 32, F32);
        ws.tensor("bit.tokens.dY", e.bit.dtok_out, 32, st.N, 1, 4, 32, F32); ws.tensor("bit.tokens.dIn", e.bit.dtok_in, 32, st.N, 1, 4, 32, F32);
    }
    e.slab = ws.take(e.slab_floats * 4);
    ws.bias_job(e.final_bias_acc, e.g_head_conv, 8, e.label);
    // conv_pred's bias gradient: summed in the integer accumulator (launch_bias_grad), converted at the end
    if (e.bres && e.dt == BF16) ws.bias_job(e.g_pred_bias_acc, e.g_pred_conv, 32, 32);
    ws.tables();
    return 0;
}

static SliceViews to_views(const Ctx& c, const std::vector<ViewRef>& v) {
    SliceViews xs;
    xs.n = (int)v.size();
    for (int k = 0; k < xs.n; ++k) { xs.p[k] = c.at(v[k].off); xs.ld[k] = v[k].ld; xs.goff[k] = v[k].goff; xs.gmask[k] = v[k].gmask; }
    return xs;
}

static void glayer_forward(const Ctx& c, GLayer& L, float* bn_running, bool training) {
    stcd_engine& e = c.e;
    const ConvW& cv = e.convs[L.conv];
    const BnP& bn = e.bns[L.bn];
    const int64_t ppg = (int64_t)L.npg * L.Ho * L.Wo;
    float* stat = c.at<float>(L.stat);
    long long* const facc = training ? c.at<long long>(L.facc) : nullptr;
    bool fused = false;
    if (L.kind == K_STEM7 && conv_on_ref(mfma_on(e), L.fwd)) {      // an unbound stem (Binder::stem): the dedicated fp32 kernel
        ProfScope ps(c, PC_CONV, 2.0 * L.N * L.Ho * L.Wo * 49.0 * cv.cin * cv.cout, 0.0, "k_stem_fwd");
        launch_stem_fwd(e.dt, c.at(L.in.off), c.params + cv.w_off, c.at(L.Y.off), L.N, L.Hi, L.Wi, cv.cin, cv.cout, c.s);
    } else {
        ConvArgs ca = conv_args(c.at(L.in.off), c.at(L.Y.off));
        ca.sums.acc = facc; ca.sums.groups = L.groups; ca.sums.C = L.C;
        fused = exec_conv(c, L.fwd, ca).sums;
    }
    // (the separate pass carries no profile record here, so this is not exec_conv_stats)
    if (facc && !fused) launch_bn_stats(e.dt, c.at(L.Y.off), L.Y.ld, L.C, L.groups, ppg, facc, c.s);
    BnActArgs a;
    bn_fields(a, c, bn, L.C, bn_running, facc);
    a.Y = c.at(L.Y.off); a.ldy = L.Y.ld; a.A = c.at(L.A.off); a.lda = L.A.ld; a.a_group_off = ppg * L.A.ld;
    a.P = nullptr; a.ldp = 0; a.stat = stat; a.mask = nullptr;
    a.C = L.C; a.groups = L.groups; a.npg = L.npg; a.H = L.Ho; a.W = L.Wo; a.relu = L.relu ? 1 : 0;
    if (L.res.off >= 0) { a.res = c.at(L.res.off); a.ldres = L.res.ld; }
    a.extra = to_views(c, L.extra_dst);
    a.g_first = L.g_first;
    ProfScope ps(c, PC_BN_ACT, 0.0, 2.0 * L.N * L.Ho * L.Wo * L.C * (double)dsize(e.dt));
    launch_bn_act(e.dt, a, c.s);
}

static void glayer_backward(const Ctx& c, GLayer& L) {
    stcd_engine& e = c.e;
    const ConvW& cv = e.convs[L.conv];
    const BnP& bn = e.bns[L.bn];
    const int64_t HW = (int64_t)L.Ho * L.Wo, ppg = (int64_t)L.npg * HW;
    const float* stat = c.at<float>(L.stat);
    const void* res = L.res.off >= 0 ? c.at(L.res.off) : nullptr;
    const double act_bytes = (double)L.N * HW * L.C * (double)dsize(e.dt);
    {
        ProfScope ps(c, PC_BN_BWD_REDUCE, 0.0, 2.0 * act_bytes);
        const SliceViews xs = to_views(c, L.grad_src);
        launch_bn_bwd_reduce(e.dt, c.at(L.dA.off), L.dA.ld, ppg * L.dA.ld, c.at(L.Y.off), L.Y.ld, stat, nullptr, L.C, L.groups, L.npg, HW,
                             L.relu ? 1 : 0, c.at<long long>(L.bacc), c.s, res, L.res.ld, &xs, L.grad_base ? 1 : 0, c.at(L.dA.off));
    }
    {
        ProfScope ps(c, PC_BN_BWD_APPLY, 0.0, 3.0 * act_bytes);
        launch_bn_bwd_apply(e.dt, c.at(L.dA.off), L.dA.ld, ppg * L.dA.ld, c.at(L.dA.off), L.dA.ld, c.at(L.Y.off), L.Y.ld, stat,
                            c.at<long long>(L.bacc), c.grads + bn.g_off, c.grads + bn.b_off, nullptr, L.C, L.groups, L.npg, HW, L.relu ? 1 : 0,
                            c.s, res, L.res.ld, L.dRes.off >= 0 ? c.at(L.dRes.off) : nullptr, L.dRes.ld);
    }
    if (L.kind == K_STEM7 && L.nwg > 0) {
        for (int k = 0; k < L.nwg; ++k) exec_wgrad(c, L.wg[k], c.at(L.wg[k].in_off), c.at(L.dA.off));
        return;
    }
    if (L.kind == K_STEM7) {
        ProfScope ps(c, PC_WGRAD, 2.0 * L.N * HW * 49.0 * cv.cin * cv.cout, 0.0, "k_stem_wgrad");
        launch_stem_wgrad(e.dt, c.at(L.in.off), c.at(L.dA.off), c.grads + cv.w_off, L.N, L.Hi, L.Wi, cv.cin, cv.cout, c.s, c.at<float>(e.g_stem_part));
        return;
    }
    for (int k = 0; k < L.nwg; ++k) exec_wgrad(c, L.wg[k], c.at(L.wg[k].in_off), c.at(L.dA.off));
    if (!L.has_dIn) return;
    if (L.kind == K_CONV1_S2)
        (void)hipMemsetAsync(c.at(L.dIn.off), 0, (size_t)L.N * L.Hi * L.Wi * L.dIn.ld * dsize(e.dt), c.s);
    if (L.ndgr == 4) {
        if (!exec_conv_x4(c, L.dgr, c.at(L.dA.off), nullptr, c.at(L.dIn.off)))
            for (int ph = 0; ph < 4; ++ph) exec_conv(c, L.dgr[ph], conv_args(c.at(L.dA.off), c.at(L.dIn.off)));
    } else {
        exec_conv(c, L.dgr[0], conv_args(c.at(L.dA.off), c.at(L.dIn.off)));
    }
}

static int forward_segcd(stcd_engine& e, const float* x1, const float* x2, const float* params, float* bn_running, int training,
                         float* logits, void* workspace, hipStream_t s) {
    Ctx c{e, (char*)workspace, params, nullptr, s};
    const int B = e.B, dt = e.dt;
    const int64_t T = (int64_t)dsize(dt), HW = (int64_t)e.H * e.W;
    if (pack_all_weights(c, training != 0)) return 1;
    if (training) STCD_HIP(hipMemsetAsync(c.at(e.zero_begin), 0, e.zero_end - e.zero_begin, s));
    launch_in_pack(dt, x1, x2, c.at(e.X0.off), B, e.in_ch, e.H, e.W, s, e.seg_dates);
    for (const GStep& st : e.g_fwd) {
        if (st.kind == GS_LAYER) glayer_forward(c, e.g_layers[st.layer], bn_running, training != 0);
        else if (st.kind == GS_MAXPOOL) launch_maxpool3(dt, c.at(st.src.off), st.src.ld, c.at(st.dst.off), st.dst.ld, st.N, st.h, st.w, st.C, s,
                                                        training ? c.at<unsigned char>(e.g_pool_idx) : nullptr);
        else if (st.kind == GS_ABSDIFF) {
            const int64_t hw = (int64_t)st.h * st.w;
            launch_fuse(dt, 0, c.at(st.src.off), st.src.ld, (int64_t)st.N * hw * st.src.ld,
                        c.at<char>(st.src.off) + (int64_t)2 * st.N * hw * st.src.ld * T, st.src.ld, st.N, hw, st.C, s);
        } else if (st.kind == GS_BCONV)
            exec_conv(c, e.g_pred_fwd, conv_args(c.at(st.src.off), c.at(st.dst.off), params + e.convs[e.g_pred_conv].b_off));
        else if (st.kind == GS_ABSPAIR) {
            ProfScope ps(c, PC_POOL_FUSE, 0.0, 3.0 * st.N * st.h * st.w * st.C * (double)T, "k_fuse");
            launch_fuse(dt, 0, c.at(st.src.off), st.src.ld, (int64_t)st.N * st.h * st.w * st.src.ld, c.at(st.dst.off), st.dst.ld, st.N,
                        (int64_t)st.h * st.w, st.C, s);
        } else if (st.kind == GS_TOKENIZE) {
            ProfScope ps(c, PC_POOL_FUSE, 16.0 * 32 * st.N * st.h * st.w, 2.0 * st.N * st.h * st.w * 32 * (double)T, "k_bit_tok_fwd");
            launch_bit_tok_fwd(dt, c.at(st.src.off), params + e.bit.wa_off, c.at<float>(e.bit.tok_in), c.at<float>(e.bit.stat), st.N, st.h * st.w, s);
        } else if (st.kind == GS_TOKENENC) {
            { ProfScope ps(c, PC_POOL_FUSE, 2.0 * B * 8 * (4.0 * 512 * 32 + 2.0 * 32 * 64), 4.0 * bit_layer_floats(64), "k_bit_enc<false>");
            launch_bit_enc_fwd(c.at<float>(e.bit.tok_in), params + e.bit.pos_off, params + e.bit.enc_off, c.at<float>(e.bit.tok_out), B, 64, s); }
            ProfScope ps(c, PC_POOL_FUSE, 2.0 * e.bit.L * st.N * 4.0 * 8 * e.bit.dh * 32 * 4, 4.0 * e.bit.L * (bit_layer_floats(e.bit.dh) + st.N * 2048.0), "k_bit_dec_fold");
            launch_bit_dec_fold(c.at<float>(e.bit.tok_out), params + e.bit.dec_off, c.at<float>(e.bit.AP), st.N, e.bit.L, e.bit.dh, s);
        } else if (st.kind == GS_TOKENDEC) {
            const double rows = (double)st.N * st.h * st.w;
            ProfScope ps(c, PC_POOL_FUSE, 12288.0 * e.bit.L * rows, (training ? e.bit.L + 1.0 : 2.0) * rows * 32 * (double)T, "k_bit_dec_fwd");
            launch_bit_dec_fwd(dt, c.at(st.src.off), c.at(st.dst.off), training ? c.at(e.bit.xs) : nullptr, c.at<float>(e.bit.AP),
                               params + e.bit.dec_off, st.h * st.w, st.N, e.bit.L, e.bit.dh, s);
        } else if (st.kind == GS_BILINEAR) {
            ProfScope ps(c, PC_POOL_FUSE, 0.0, 17.0 * st.N * st.h * st.w * st.C * (double)T, "k_bilinear");
            launch_bilinear(dt, c.at(st.src.off), st.src.ld, c.at(st.dst.off), st.dst.ld, st.N, st.h, st.w, 4 * st.h, 4 * st.w, st.C, 0, s);
        } else if (e.bres) {
            ProfScope ps(c, PC_POOL_FUSE, 0.0, 5.0 * st.N * st.h * st.w * st.C * (double)T, "k_upsample2");
            launch_upsample2(dt, c.at(st.src.off), st.src.ld, c.at(st.dst.off), st.dst.ld, st.N, st.h, st.w, st.C, s);
        }
        else launch_upsample2(dt, c.at(st.src.off), st.src.ld, c.at(st.dst.off), st.dst.ld, st.N, st.h, st.w, st.C, s);
    }
    if (e.seg_dates == 1 || e.bres) {      // UnetSeg: masks = head(decoder output); base_resnet: logits = classifier.3(classifier's ReLU)
        exec_conv(c, e.g_head_fwd, conv_args(c.at(e.gX3.off), logits, params + e.convs[e.g_head_conv].b_off, true));
        STCD_HIP(hipGetLastError());
        return 0;
    }
    // head: X3[2B:3B] = |d1 - d2| ; raw = conv(X3) = [m1; m2; diffea] ; logits = [m1; m2; min(diffea, |m1 - m2|)]
    // (FFCTLCD: X3[2B:3B] is the decoder's output on |f1 - f2|, already in place)
    if (!e.seg_ffc) launch_fuse(dt, 0, c.at(e.gX3.off), 16, (int64_t)B * HW * 16, c.at<char>(e.gX3.off) + (int64_t)2 * B * HW * 16 * T, 16, B, HW, 16, s);
    exec_conv(c, e.g_head_fwd, conv_args(c.at(e.gX3.off), c.at(e.g_raw3), params + e.convs[e.g_head_conv].b_off, true));
    launch_segcd_combine(c.at<float>(e.g_raw3), logits, (int64_t)B * e.label * HW, s);
    STCD_HIP(hipGetLastError());
    return 0;
}

static int backward_segcd(stcd_engine& e, const float* grad_logits, const float* params, float* grads, void* workspace, int stage,
                          hipStream_t s) {
    if (stage == 1) return 0;
    Ctx c{e, (char*)workspace, params, grads, s};
    WgradScope wgrad_scope(e, stage, false, nullptr);      // (the groups go out on the tail)
    const int B = e.B, dt = e.dt;
    const int64_t T = (int64_t)dsize(dt), HW = (int64_t)e.H * e.W;
    STCD_HIP(hipMemsetAsync(grads, 0, e.param_floats * 4, s));
    if (!mfma_on(e)) STCD_HIP(hipMemsetAsync(c.at(e.dwe_begin), 0, e.dwe_end - e.dwe_begin, s));
    if (e.seg_dates == 1 || e.bres) {
        launch_gout_pack(dt, grad_logits, c.at(e.G.off), B, e.label, e.H, e.W, s, c.at<long long>(e.final_bias_acc));
        exec_wgrad(c, e.g_head_wg, c.at(e.gX3.off), c.at(e.G.off));
        exec_conv(c, e.g_head_dgr, conv_args(c.at(e.G.off), c.at(e.gdX3.off)));
    } else {
        launch_segcd_combine_bwd(c.at<float>(e.g_raw3), grad_logits, c.at<float>(e.g_draw3), (int64_t)B * e.label * HW, s);
        launch_gout_pack(dt, c.at<float>(e.g_draw3), c.at(e.G.off), 3 * B, e.label, e.H, e.W, s, c.at<long long>(e.final_bias_acc));
        exec_wgrad(c, e.g_head_wg, c.at(e.gX3.off), c.at(e.G.off));
        exec_conv(c, e.g_head_dgr, conv_args(c.at(e.G.off), c.at(e.gdX3.off)));
        // d(d1), d(d2) += -/+ sign(d1 - d2) * d|d1 - d2| : written to a contribution buffer the last decoder layer gathers
        if (!e.seg_ffc) launch_fuse_bwd(dt, 0, c.at(e.gX3.off), 16, (int64_t)B * HW * 16, c.at<char>(e.gdX3.off) + (int64_t)2 * B * HW * 16 * T, 16,
                        c.at(e.gFuseTmp.off), 16, (int64_t)B * HW * 16, B, HW, 16, s);
    }
    for (int k = (int)e.g_fwd.size() - 1; k >= 0; --k) {
        const GStep& st = e.g_fwd[k];
        if (st.kind == GS_LAYER) glayer_backward(c, e.g_layers[st.layer]);
        else if (st.kind == GS_UPSAMPLE)
            launch_upsample2_bwd(dt, c.at(st.ddst.off), st.ddst.ld, c.at(st.dsrc.off), st.dsrc.ld, st.N, st.h, st.w, st.C, s);
        else if (st.kind == GS_ABSDIFF) {
            const int64_t hw = (int64_t)st.h * st.w;
            launch_fuse_bwd(dt, 0, c.at(st.src.off), st.src.ld, (int64_t)st.N * hw * st.src.ld,
                            c.at<char>(st.dsrc.off) + (int64_t)2 * st.N * hw * st.dsrc.ld * T, st.dsrc.ld,
                            c.at(st.ddst.off), st.ddst.ld, (int64_t)st.N * hw * st.ddst.ld, st.N, hw, st.C, s);
        }
        else if (st.kind == GS_TOKENDEC) {
            auto& b = e.bit;
            const int n = st.h * st.w;
            const double rows = (double)st.N * n;
            {   // recompute + backward: 3 x the forward's products; reads the layer inputs and the gradient, the gradient travels in fp32
                ProfScope ps(c, PC_POOL_FUSE, 3.0 * 12288.0 * b.L * rows, rows * 32 * ((b.L + 2.0) * (double)T + 8.0 * (b.L - 1)), "k_bit_dec_bwd");
                if (launch_bit_dec_bwd(dt, c.at(st.src.off), c.at(b.xs), c.at(st.ddst.off), c.at<float>(b.dG), c.at(st.dsrc.off), c.at<float>(b.AP),
                                       params + b.dec_off, c.at<float>(b.dec_part), n, st.N, b.L, b.dh, s)) return 1;
            }
            // partial sums, unfold of dA / dP into the projection gradients, d(memory): bytes = the partials read once
            ProfScope ps(c, PC_POOL_FUSE, 2.0 * b.L * st.N * 6.0 * 8 * b.dh * 32 * 4, 4.0 * (double)bit_dec_part_floats(n, st.N, b.L), "k_bit_sum_parts|k_bit_dec_unfold|k_bit_dec_mfinish");
            launch_bit_dec_finish(c.at<float>(b.dec_part), c.at<float>(b.dAP), c.at<float>(b.tok_out), params + b.dec_off, grads + b.dec_off,
                                  c.at<float>(b.dmh), c.at<float>(b.dm), c.at<float>(b.dtok_out), n, st.N, b.L, b.dh, s);
        } else if (st.kind == GS_TOKENENC) {
            auto& b = e.bit;
            ProfScope ps(c, PC_POOL_FUSE, 6.0 * B * 8 * (4.0 * 512 * 32 + 2.0 * 32 * 64), 4.0 * (double)bit_enc_part_floats(B, 64) * 2, "k_bit_enc<true>");
            launch_bit_enc_bwd(c.at<float>(b.tok_in), params + b.pos_off, params + b.enc_off, c.at<float>(b.dtok_out), c.at<float>(b.dtok_in),
                               c.at<float>(b.enc_part), grads + b.enc_off, grads + b.pos_off, B, 64, s);
        } else if (st.kind == GS_TOKENIZE) {
            auto& b = e.bit;
            ProfScope ps(c, PC_POOL_FUSE, 48.0 * 32 * st.N * st.h * st.w, 4.0 * st.N * st.h * st.w * 32 * (double)T, "k_bit_tok_bwd");
            launch_bit_tok_bwd(dt, c.at(st.src.off), params + b.wa_off, c.at<float>(b.stat), c.at<float>(b.dtok_in), c.at(b.dec_din.off),
                               c.at(st.dsrc.off), c.at<float>(b.tok_part), grads + b.wa_off, st.N, st.h * st.w, s);
        }
        else if (st.kind == GS_BILINEAR) {
            ProfScope ps(c, PC_POOL_FUSE, 0.0, 17.0 * st.N * st.h * st.w * st.C * (double)T, "k_bilinear_bwd");
            launch_bilinear_bwd(dt, c.at(st.ddst.off), st.ddst.ld, c.at(st.dsrc.off), st.dsrc.ld, st.N, st.h, st.w, 4 * st.h, 4 * st.w, st.C, 0, s);
        } else if (st.kind == GS_ABSPAIR) {      // d(x1), d(x2) = +/- sign(x1 - x2) * d|x1 - x2|; sign(0) = 0 as torch.abs
            const int64_t hw = (int64_t)st.h * st.w;
            ProfScope ps(c, PC_POOL_FUSE, 0.0, 5.0 * st.N * hw * st.C * (double)T, "k_fuse_bwd");
            launch_fuse_bwd(dt, 0, c.at(st.src.off), st.src.ld, (int64_t)st.N * hw * st.src.ld, c.at(st.ddst.off), st.ddst.ld,
                            c.at(st.dsrc.off), st.dsrc.ld, (int64_t)st.N * hw * st.dsrc.ld, st.N, hw, st.C, s);
        } else if (st.kind == GS_BCONV) {
            { ProfScope ps(c, PC_POOL_FUSE, 0.0, (double)st.N * st.h * st.w * 32 * (double)T, "k_bias_grad");
            launch_bias_grad(dt, c.at(st.ddst.off), st.ddst.ld, (int64_t)st.N * st.h * st.w, 32, grads + e.convs[e.g_pred_conv].b_off, s,
                             dt == BF16 ? c.at<long long>(e.g_pred_bias_acc) : nullptr); }
            exec_wgrad(c, e.g_pred_wg, c.at(st.src.off), c.at(st.ddst.off));
            exec_conv(c, e.g_pred_dgr, conv_args(c.at(st.ddst.off), c.at(st.dsrc.off)));
        }
        else {      // max-pool: d(P0) = conv1 contribution (written in place) + identity-branch contribution of layer1.0 (its
                    // down-sample's data gradient for Bottleneck encoders, the gated residual gradient itself for BasicBlock ones)
            launch_slice(dt, c.at(st.ddst.off), st.ddst.ld, c.at(e.g_pool_idc.off), e.g_pool_idc.ld, (int64_t)st.N * (st.h / 2) * (st.w / 2), st.C, 1, s);
            launch_maxpool3_bwd(dt, c.at<unsigned char>(e.g_pool_idx), c.at(st.ddst.off), st.ddst.ld, c.at(st.dsrc.off), st.dsrc.ld, st.N, st.h, st.w, st.C, s);
        }
    }
    if (stage_tail(c, 0, nullptr, false, finish_biases)) return 1;
    STCD_HIP(hipGetLastError());
    return 0;
}

#include "engine_cf.inl"

// The shape-bound state every configure_* rebuilds from empty, reset in ONE place (stcd_configure) -- a vector left out here lets a
// table grow with every re-configure (tests/test_lifecycle_cpu.py).  Per-layer fields of the table-time vectors (sn_blocks, g_layers,
// xc) are reset by their family's own loops; build_wgrad_jobs and build_filter_pack_jobs clear the job tables they own.
static void reset_plan(stcd_engine& e) {
    e.enc.clear(); e.dec.clear(); e.ups.clear();
    e.drops.clear(); e.drop_floats = 0;
    e.conv_ops.clear(); e.wgrad_ops.clear(); e.slab_floats = 0; e.wg_last_op = nullptr;
    e.ws_tensors.clear(); e.bias_jobs.clear();
    e.g_fwd.clear(); e.sn_order.clear();
    if (e.cf) cf_reset_plan(*e.cf);
}

}  // namespace stcd

// ================================================================================================ C ABI
extern "C" {

const char* stcd_last_error(void) { return stcd::g_err.c_str(); }
int stcd_abi_version(void) { return STCD_ABI_VERSION; }

static void engine_env_switches(stcd_engine* e) {       // read at every stcd_create*
    e->use_mfma = !env_flag("STCD_FORCE_REF_KERNELS", false);
    e->use_small = !env_flag("STCD_NO_SMALL_KERNEL", false);
    e->use_gemm = !env_flag("STCD_NO_GEMM_KERNEL", false);
    e->use_res = !env_flag("STCD_NO_RES_KERNEL", false);
    e->use_halo = env_flag("STCD_HALO_KERNEL", false);                      // 1: k_conv_halo where it fits (opt-in, pick_gemm_or_res)
    e->use_tile = !env_flag("STCD_NO_TILE_KERNEL", false);                  // 1: the small-map Ci % 64 == 0 layers of FC-Siam stay on k_conv_res
    e->use_wgroup = !env_flag("STCD_NO_WGRAD_GROUPS", false);
    e->use_act_fuse = !env_flag("STCD_NO_ACT_FUSE", false);
    e->use_skip_fused = !env_flag("STCD_NO_SKIP_FUSED", false);
    e->use_skip_recompute = !env_flag("STCD_NO_SKIP_RECOMPUTE", false);     // 1: the skip layers of diff / sub store their activations again
    e->use_bwdsum = !env_flag("STCD_NO_BWDSUM_FUSE", false);                // 1: every layer runs its own k_bn_reduce (no sums in k_conv_small data gradients)
    e->use_bwdsum_res = env_flag("STCD_BWDSUM_RES", false);                 // 1: also the layers behind a k_conv_res data gradient (measured slower, see configure_fcsiam)
    e->use_virt = env_int("STCD_VIRT_ACT", e->use_virt) != 0;               // 1: virtual activations (opt-in); 0 / unset: k_bn_act per layer
    e->wg_side_on = env_int("STCD_WGRAD_SIDE", e->wg_side_on) != 0;         // 0: the decoder's weight gradients stay on the caller's stream
}

int stcd_cf_default_config(stcd_cf_config* cfg) {
    STCD_CHECK(cfg != nullptr, "cfg is null");
    static const int E[4] = {64, 128, 320, 512}, DP[4] = {3, 3, 4, 3}, HD[4] = {1, 2, 4, 8}, SR[4] = {8, 4, 2, 1};
    memset(cfg, 0, sizeof(*cfg));
    cfg->in_ch = 3; cfg->out_ch = 2;
    for (int i = 0; i < 4; ++i) { cfg->embed_dims[i] = E[i]; cfg->depths[i] = DP[i]; cfg->num_heads[i] = HD[i]; cfg->sr_ratios[i] = SR[i]; }
    cfg->mlp_ratio = 4; cfg->embedding_dim = 256; cfg->patch1 = 7; cfg->patch = 7;
    cfg->drop_rate = 0.1f; cfg->attn_drop = 0.1f; cfg->drop_path_rate = 0.1f; cfg->diff_drop = 0.6f;
    return 0;
}

int stcd_create_changeformer(const stcd_cf_config* cfg, int dtype, stcd_engine** out) {
    STCD_CHECK(out != nullptr && cfg != nullptr, "null argument");
    STCD_CHECK(cfg->in_ch >= 1 && cfg->in_ch <= 8, "in_ch must be in [1,8]");
    STCD_CHECK(cfg->out_ch >= 1 && cfg->out_ch <= 8, "out_ch must be in [1,8]");
    STCD_CHECK(dtype == STCD_DTYPE_F32 || dtype == STCD_DTYPE_BF16, "unknown dtype");
    STCD_CHECK(cfg->mlp_ratio >= 1 && cfg->embedding_dim >= 8 && cfg->embedding_dim % 8 == 0, "embedding_dim must be a positive multiple of 8");
    STCD_CHECK((cfg->embedding_dim & (cfg->embedding_dim - 1)) == 0, "embedding_dim must be a power of two (BatchNorm kernels)");
    STCD_CHECK((cfg->patch1 & 1) && (cfg->patch & 1) && cfg->patch1 >= 3 && cfg->patch >= 3, "patch sizes must be odd and >= 3");
    for (int i = 0; i < 4; ++i) {
        STCD_CHECK(cfg->embed_dims[i] >= 8 && cfg->embed_dims[i] % 8 == 0 && cfg->embed_dims[i] <= 1024, "embed_dims must be multiples of 8, <= 1024");
        STCD_CHECK(cfg->depths[i] >= 1 && cfg->num_heads[i] >= 1 && cfg->sr_ratios[i] >= 1, "depths, num_heads and sr_ratios must be >= 1");
        STCD_CHECK(cfg->embed_dims[i] % cfg->num_heads[i] == 0, "embed_dims must be divisible by num_heads");
    }
    for (float p : {cfg->drop_rate, cfg->attn_drop, cfg->drop_path_rate, cfg->diff_drop}) STCD_CHECK(p >= 0.f && p < 1.f, "drop rates must be in [0,1)");
    std::unique_ptr<stcd_engine> e(new stcd_engine());
    e->arch = STCD_ARCH_CHANGEFORMER; e->in_ch = cfg->in_ch; e->label = cfg->out_ch; e->dt = dtype;
    engine_env_switches(e.get());
    e->cf = std::make_shared<CfPlan>();
    CfPlan& P = *e->cf;
    for (int i = 0; i < 4; ++i) { P.E[i] = cfg->embed_dims[i]; P.depths[i] = cfg->depths[i]; P.heads[i] = cfg->num_heads[i]; P.srs[i] = cfg->sr_ratios[i]; }
    P.mlp_ratio = cfg->mlp_ratio; P.D = cfg->embedding_dim; P.patch1 = cfg->patch1; P.patch = cfg->patch;
    P.drop = cfg->drop_rate; P.attn_drop = cfg->attn_drop; P.drop_path = cfg->drop_path_rate; P.diff_drop = cfg->diff_drop;
    build_cf_tables(*e);
    *out = e.release();
    return 0;
}

int stcd_cf_num_sites(const stcd_engine* e) { return e && e->cf && e->configured ? (int)e->cf->sites.size() : 0; }
int stcd_cf_site_get(const stcd_engine* e, int i, stcd_cf_site* out) {
    STCD_CHECK(e && e->cf && e->configured && out && i >= 0 && i < (int)e->cf->sites.size(), "bad argument");
    memset(out, 0, sizeof(*out));
    const CfPlan::Site& s = e->cf->sites[i];
    snprintf(out->name, sizeof(out->name), "%s", s.name.c_str());
    out->ndim = s.nd;
    for (int k = 0; k < s.nd; ++k) out->dims[k] = s.dims[k];
    out->p = s.p;
    return 0;
}
uint32_t stcd_cf_site_seed(uint64_t seed, int site) { return cf_site_seed(seed, site); }
int stcd_cf_set_aux_backward(stcd_engine* e, int on) {
    STCD_CHECK(e && e->cf, "not a ChangeFormer engine");
    if (e->cf->aux_bwd != (on != 0)) e->configured = false;      // the heads' backward launches and scratch are part of the plan
    e->cf->aux_bwd = on != 0;
    return 0;
}
int stcd_set_wgrad_side(stcd_engine* e, int on) {
    STCD_CHECK(e, "null engine");
    if ((e->wg_side_on != 0) != (on != 0)) e->configured = false;        // the block budget of stage 0's grouped grids is part of the plan
    e->wg_side_on = on != 0;
    return 0;
}
int stcd_cf_set_drop_rates(stcd_engine* e, float drop_rate, float attn_drop, float diff_drop) {
    STCD_CHECK(e && e->cf, "not a ChangeFormer engine");
    for (float p : {drop_rate, attn_drop, diff_drop}) STCD_CHECK(p >= 0.f && p < 1.f, "drop rates must be in [0,1)");
    e->cf->drop = drop_rate; e->cf->attn_drop = attn_drop; e->cf->diff_drop = diff_drop;
    e->configured = false;      // the site table is rebuilt by the next stcd_configure
    return 0;
}
int64_t stcd_output_floats(const stcd_engine* e) {
    if (!e || !e->configured) return 0;
    if (e->cf) return e->cf->out_floats;
    const int maps = (is_segcd(e->arch) && !is_unetseg(e->arch) && !is_bres(e->arch)) ? 3 : sn_out_maps(e->arch);
    return (int64_t)maps * e->B * e->label * e->H * e->W;
}
int stcd_cf_output_info(const stcd_engine* e, int i, int64_t* offset, int* height, int* width) {
    STCD_CHECK(e && e->cf && e->configured && offset && height && width && i >= 0 && i < 5, "bad argument");
    if (i < 4) { *offset = e->cf->df[i].out_off; *height = e->cf->df[i].h; *width = e->cf->df[i].w; }
    else { *offset = e->cf->cp_off; *height = e->H; *width = e->W; }
    return 0;
}

int stcd_create(int arch, int in_ch, int label_ch, int dtype, stcd_engine** out) {
    STCD_CHECK(out != nullptr, "out is null");
    if (is_cf(arch)) {
        stcd_cf_config cfg;
        stcd_cf_default_config(&cfg);
        cfg.in_ch = in_ch; cfg.out_ch = label_ch;
        return stcd_create_changeformer(&cfg, dtype, out);
    }
    STCD_CHECK((arch >= STCD_ARCH_DIFF && arch <= STCD_ARCH_SEGCD_R152) || arch == STCD_ARCH_FCEF || arch == STCD_ARCH_XCONC || is_snconc(arch) || is_unetseg(arch) || is_ffctlcd(arch) || is_bres(arch), "unknown arch");
    STCD_CHECK(!is_bres(arch) || in_ch == 3, "base_resnet: in_ch must be 3 (the reference's resnet.conv1 always takes 3 channels, models/networks.py:234)");
    STCD_CHECK(arch != STCD_ARCH_FCEF || in_ch <= 4, "FC-EF concatenates the two dates along the channels: in_ch must be <= 4");
    STCD_CHECK(in_ch >= 1 && in_ch <= 8, "in_ch must be in [1,8]");
    STCD_CHECK(label_ch >= 1 && label_ch <= 8, "label_ch must be in [1,8]");
    STCD_CHECK(dtype == STCD_DTYPE_F32 || dtype == STCD_DTYPE_BF16, "unknown dtype");
    STCD_CHECK(arch != STCD_ARCH_SNUNET_CONC_DS || label_ch <= 2, "Siam_NestedUNet_Conc with deep supervision: label_ch must be <= 2 (five maps of label_ch rows each in one pass of the head kernels)");
    std::unique_ptr<stcd_engine> e(new stcd_engine());
    e->arch = arch; e->in_ch = in_ch; e->label = label_ch; e->dt = dtype;
    engine_env_switches(e.get());
    if (is_snunet(arch)) build_snunet_tables(*e);
    else if (is_segcd(arch)) build_segcd_tables(*e);
    else build_fcsiam_tables(*e);
    *out = e.release();
    return 0;
}
void stcd_destroy(stcd_engine* e) {
    if (e && e->wg_side) { (void)hipStreamSynchronize(e->wg_side); (void)hipStreamDestroy(e->wg_side); (void)hipEventDestroy(e->wg_fork); (void)hipEventDestroy(e->wg_join); }
    delete e;
}

int stcd_num_params(const stcd_engine* e) { return e ? (int)e->params.size() : 0; }
int stcd_param_info(const stcd_engine* e, int i, stcd_tensor_info* info) {
    STCD_CHECK(e && info && i >= 0 && i < (int)e->params.size(), "bad argument");
    *info = e->params[i];
    return 0;
}
int64_t stcd_param_floats(const stcd_engine* e) { return e ? e->param_floats : 0; }
int stcd_num_bn(const stcd_engine* e) { return e ? (int)e->bns.size() : 0; }
int stcd_bn_info_get(const stcd_engine* e, int i, stcd_bn_info* info) {
    STCD_CHECK(e && info && i >= 0 && i < (int)e->bns.size(), "bad argument");
    memset(info, 0, sizeof(*info));
    snprintf(info->name, sizeof(info->name), "%s", e->bns[i].name.c_str());
    info->channels = e->bns[i].C;
    info->calls_per_forward = e->bns[i].calls;
    info->offset = e->bns[i].run_off;
    return 0;
}
int64_t stcd_bn_floats(const stcd_engine* e) { return e ? e->bn_floats : 0; }

int stcd_configure(stcd_engine* e, int batch, int height, int width) {
    STCD_CHECK(e != nullptr, "engine is null");
    STCD_CHECK(batch >= 1, "batch must be >= 1");
    STCD_CHECK(height >= 16 && width >= 16, "height and width must be >= 16 (four 2x2 pools)");
    STCD_CHECK((int64_t)2 * batch * height * width * 16 < ((int64_t)1 << 31), "tensor too large for 32-bit pixel indexing");
    e->configured = false;
    e->packed_tag = 0; e->packed_ws = nullptr; e->packed_level = -1;
    e->B = batch; e->H = height; e->W = width;
    reset_plan(*e);
    if (is_cf(e->arch)) {
        STCD_CHECK(height % 32 == 0 && width % 32 == 0, "ChangeFormer needs height and width divisible by 32 (stride-4 patch embedding, sr_ratio 8)");
        if (configure_cf(*e, batch, height, width)) return 1;
    } else if (is_snunet(e->arch)) {
        STCD_CHECK(height % 16 == 0 && width % 16 == 0, "SNUNet needs height and width divisible by 16 (the reference's cat of up-sampled maps fails otherwise)");
        if (configure_snunet(*e, batch, height, width)) return 1;
    } else if (is_segcd(e->arch)) {
        STCD_CHECK(!is_bres(e->arch) || (height % 32 == 0 && width % 32 == 0), "base_resnet needs height and width divisible by 32 (the engine's rule: 1/8-resolution trunk, row tiles of 4 pixels at that level)");
        STCD_CHECK(height % 32 == 0 && width % 32 == 0, "SegCD needs height and width divisible by 32 (five stride-2 stages; the reference's cat of the x2 up-sampled maps fails otherwise)");
        STCD_CHECK((int64_t)3 * batch * height * width * 16 < ((int64_t)1 << 31), "tensor too large for 32-bit pixel indexing");
        if (configure_segcd(*e, batch, height, width)) return 1;
    } else if (configure_fcsiam(*e, batch, height, width)) return 1;
    // torch's BatchNorm2d refuses a training forward with one value per channel ("Expected more than 1 value per channel when
    // training"): remember the smallest per-channel sample count of the plan, stcd_forward checks it
    e->min_bn_count = INT64_MAX;
    for (const auto& L : e->enc) e->min_bn_count = std::min<int64_t>(e->min_bn_count, (int64_t)L.npg * L.H * L.W);
    for (const auto& L : e->dec) e->min_bn_count = std::min<int64_t>(e->min_bn_count, (int64_t)L.npg * L.H * L.W);
    for (const auto& b : e->sn_blocks) e->min_bn_count = std::min<int64_t>(e->min_bn_count, (int64_t)b.npg * b.H * b.W);
    for (const auto& L : e->g_layers) e->min_bn_count = std::min<int64_t>(e->min_bn_count, (int64_t)L.npg * L.Ho * L.Wo);
    if (e->cf) e->min_bn_count = std::min<int64_t>(e->min_bn_count, (int64_t)batch * (height / 32) * (width / 32));
    e->configured = true;
    e->fwd_training = false;
    return 0;
}
int64_t stcd_workspace_bytes(const stcd_engine* e) { return e && e->configured ? e->ws_bytes : 0; }
int stcd_num_dropout(const stcd_engine* e) { return e && e->configured ? (int)e->drops.size() : 0; }
int stcd_dropout_info_get(const stcd_engine* e, int i, stcd_dropout_info* info) {
    STCD_CHECK(e && e->configured && info && i >= 0 && i < (int)e->drops.size(), "bad argument");
    memset(info, 0, sizeof(*info));
    snprintf(info->name, sizeof(info->name), "%s", e->drops[i].name.c_str());
    info->rows = e->drops[i].rows;
    info->channels = e->drops[i].C;
    info->offset = e->drops[i].off;
    return 0;
}
int64_t stcd_dropout_floats(const stcd_engine* e) { return e && e->configured ? e->drop_floats : 0; }
int stcd_set_dropout_p(stcd_engine* e, float p) {
    STCD_CHECK(e != nullptr, "engine is null");
    STCD_CHECK(p >= 0.f && p < 1.f, "p must be in [0,1)");
    e->drop_p = p;
    return 0;
}

int stcd_forward(stcd_engine* e, const float* x1, const float* x2, const float* params, float* bn_running,
                 const float* dropout_masks, uint64_t dropout_seed, int training, float* logits, void* workspace,
                 void* hip_stream) {
    STCD_CHECK(e && e->configured, "engine not configured");
    STCD_CHECK(x1 && x2 && params && bn_running && logits && workspace, "null pointer argument");
    STCD_CHECK(!(training && e->min_bn_count <= 1), "Expected more than 1 value per channel when training: a BatchNorm layer of this network sees "
               "one value per channel at this batch / image size (torch.nn.BatchNorm2d raises the same)");
    e->fwd_training = false;
    int rc = is_cf(e->arch)
                 ? forward_cf(*e, x1, x2, params, bn_running, dropout_masks, dropout_seed, training, logits, workspace, (hipStream_t)hip_stream)
             : is_snunet(e->arch)
                 ? forward_snunet(*e, x1, x2, params, bn_running, training, logits, workspace, (hipStream_t)hip_stream)
                 : is_segcd(e->arch)
                       ? forward_segcd(*e, x1, x2, params, bn_running, training, logits, workspace, (hipStream_t)hip_stream)
                       : forward_fcsiam(*e, x1, x2, params, bn_running, dropout_masks, dropout_seed, training, logits, workspace,
                                        (hipStream_t)hip_stream);
    if (rc == 0) e->fwd_training = training != 0;
    return rc;
}

int stcd_backward(stcd_engine* e, const float* grad_logits, const float* params, float* grads, void* workspace, int stage,
                  void* hip_stream) {
    STCD_CHECK(e && e->configured, "engine not configured");
    STCD_CHECK(e->fwd_training, "backward requires a preceding training-mode forward on this engine that no backward has consumed "
               "(one backward per forward: it overwrites the stored activations in place)");
    STCD_CHECK(grad_logits && params && grads && workspace, "null pointer argument");
    STCD_CHECK(stage >= -1 && stage <= 1, "stage must be -1, 0 or 1");
    // the backward kernels overwrite the stored activations / output gradients in place: one backward per forward.  Stage 0 leaves
    // the encoder half pending (stage 1 follows it); the whole backward and stage 1 consume the forward
    if (stage != 0) e->fwd_training = false;
    if (is_cf(e->arch)) return backward_cf(*e, grad_logits, params, grads, workspace, stage, (hipStream_t)hip_stream);
    if (is_snunet(e->arch)) return backward_snunet(*e, grad_logits, params, grads, workspace, stage, (hipStream_t)hip_stream);
    if (is_segcd(e->arch)) return backward_segcd(*e, grad_logits, params, grads, workspace, stage, (hipStream_t)hip_stream);
    return backward_fcsiam(*e, grad_logits, params, grads, workspace, stage, (hipStream_t)hip_stream);
}

int stcd_set_weights_tag(stcd_engine* e, uint64_t tag) {
    STCD_CHECK(e != nullptr, "engine is null");
    e->weights_tag = tag;
    return 0;
}
int stcd_set_debug(stcd_engine* e, int flags) {
    STCD_CHECK(e != nullptr, "engine is null");
    e->debug_flags = flags;
    e->configured = false;      // takes effect at the next stcd_configure
    return 0;
}
int stcd_seam_plan(const stcd_engine* e, int* entry_fused, int* reduce_early_jobs, int* reduce_final_jobs, int* last_tail) {
    STCD_CHECK(e && entry_fused && reduce_early_jobs && reduce_final_jobs && last_tail, "null argument");
    STCD_CHECK(e->configured, "stcd_configure first");
    *entry_fused = (fc_family(*e) && !(e->debug_flags & 2)) ? 1 : 0;
    *reduce_early_jobs = e->rj_split;
    *reduce_final_jobs = e->rj_split > 0 ? (int)e->rjobs[1].size() - e->rj_split : 0;
    *last_tail = e->last_tail;
    return 0;
}
int stcd_ws_tensor_count(const stcd_engine* e) { return e ? (int)e->ws_tensors.size() : 0; }
int stcd_ws_tensor_get(const stcd_engine* e, int index, stcd_ws_tensor* out) {
    STCD_CHECK(e != nullptr && out != nullptr, "null argument");
    STCD_CHECK(index >= 0 && index < (int)e->ws_tensors.size(), "tensor index out of range");
    *out = e->ws_tensors[index];
    return 0;
}

int stcd_grad_stage_range(const stcd_engine* e, int stage, int64_t* begin, int64_t* end) {
    STCD_CHECK(e && begin && end, "bad argument");
    STCD_CHECK(stage == 0 || stage == 1, "stage must be 0 or 1");
    if (stage == 0) { *begin = e->enc_param_end; *end = e->param_floats; }
    else { *begin = 0; *end = e->enc_param_end; }
    return 0;
}

int stcd_profile_enable(stcd_engine* e, int on) {
    STCD_CHECK(e != nullptr, "engine is null");
    e->prof.on = on != 0;
    e->prof.recs.clear();
    e->prof.names.clear();
    e->prof.used = 0;
    return 0;
}
int stcd_profile_read(stcd_engine* e, int klass, double* total_ms, int64_t* launches, double* flops, double* bytes) {
    STCD_CHECK(e && total_ms && launches && flops && bytes, "bad argument");
    STCD_CHECK(klass >= 0 && klass < PC_COUNT, "unknown kernel class");
    *total_ms = 0.0; *launches = 0; *flops = 0.0; *bytes = 0.0;
    for (auto& r : e->prof.recs) {
        if (r.klass != klass) continue;
        STCD_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        STCD_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        *total_ms += ms; *launches += 1; *flops += r.flops; *bytes += r.bytes;
    }
    return 0;
}

int stcd_profile_num_kernels(const stcd_engine* e) { return e ? (int)e->prof.names.size() : 0; }
int stcd_profile_kernel(stcd_engine* e, int i, char* name, int name_cap, double* total_ms, int64_t* launches, double* flops,
                        double* bytes) {
    STCD_CHECK(e && name && total_ms && launches && flops && bytes && name_cap > 0, "bad argument");
    STCD_CHECK(i >= 0 && i < (int)e->prof.names.size(), "kernel index out of range");
    snprintf(name, (size_t)name_cap, "%s", e->prof.names[i].c_str());
    *total_ms = 0.0; *launches = 0; *flops = 0.0; *bytes = 0.0;
    for (auto& r : e->prof.recs) {
        if (r.name_id != i) continue;
        STCD_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        STCD_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        *total_ms += ms; *launches += 1; *flops += r.flops; *bytes += r.bytes;
    }
    return 0;
}

int64_t stcd_loss_scratch_bytes(void) { return loss_scratch_bytes(); }
int stcd_loss_ce(const float* logits, const int64_t* target, int batch, int classes, int64_t hw, int ignore_index,
                 float* loss_out, float* dlogits, void* scratch, void* hip_stream) {
    STCD_CHECK(logits && target && loss_out && scratch, "null pointer argument");
    STCD_CHECK(batch >= 1 && classes >= 2 && classes <= 16 && hw >= 1, "bad shape");
    launch_loss_ce(logits, target, batch, classes, hw, ignore_index, loss_out, dlogits, scratch, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}
int stcd_loss_bce_dice(const float* logits, const float* target, int64_t numel, int from_logits, float* loss_out,
                       float* dlogits, void* scratch, void* hip_stream) {
    STCD_CHECK(logits && target && loss_out && scratch, "null pointer argument");
    STCD_CHECK(numel >= 1, "bad shape");
    launch_loss_bce_dice(logits, target, numel, from_logits, loss_out, dlogits, scratch, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}
int stcd_loss_contrastive(const float* pred, const int64_t* cd_label, const int64_t* pse_label, int64_t numel_half, float* loss_out,
                          float* dpred, void* scratch, void* hip_stream) {
    STCD_CHECK(pred && cd_label && pse_label && loss_out && scratch, "null pointer argument");
    STCD_CHECK(numel_half >= 1, "bad shape");
    launch_loss_contrastive(pred, cd_label, pse_label, numel_half, loss_out, dpred, scratch, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}
int64_t stcd_loss_iou_scratch_bytes(int batch, int classes, int64_t hw) {
    if (batch < 1 || classes < 2 || classes > 16 || hw < 1) return 0;
    return iou_scratch_bytes(batch, classes, hw);
}
int stcd_loss_focal(const float* x, const int64_t* target, int batch, int classes, int64_t hw, const float* alpha, float gamma,
                    float smooth, int flags, float* loss_out, float* dx, void* scratch, void* hip_stream) {
    STCD_CHECK(x && target && loss_out && scratch, "null pointer argument");
    STCD_CHECK(classes >= 2 && classes <= 16, "classes must be in [2, 16]");
    STCD_CHECK(batch >= 1 && hw >= 1, "bad shape");
    STCD_CHECK(smooth >= 0.f && smooth <= 1.f, "smooth must be in [0, 1]");
    STCD_CHECK(flags >= 0 && flags <= 3, "flags: bit 0 = softmax fused, bit 1 = sum instead of mean");
    launch_loss_focal(x, target, batch, classes, hw, alpha, gamma, smooth, flags, loss_out, dx, scratch, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}
int stcd_loss_iou(const float* logits, const int64_t* target, int batch, int classes, int64_t hw, const float* weight, int mode,
                  float* loss_out, float* dlogits, void* scratch, void* hip_stream) {
    STCD_CHECK(logits && target && loss_out && scratch, "null pointer argument");
    STCD_CHECK(classes >= 2 && classes <= 16, "classes must be in [2, 16]");
    STCD_CHECK(batch >= 1 && hw >= 1, "bad shape");
    STCD_CHECK(mode == 0 || mode == 1, "mode must be 0 (mIoU) or 1 (min-max IoU)");
    launch_loss_iou(logits, target, batch, classes, hw, weight, mode, loss_out, dlogits, scratch, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}
int stcd_confusion_update(const float* logits, const int64_t* target, int batch, int classes, int64_t hw, int64_t* cm,
                          void* hip_stream) {
    STCD_CHECK(logits && target && cm, "null pointer argument");
    STCD_CHECK(batch >= 1 && (classes == 1 || classes == 2) && hw >= 1, "bad shape (classes must be 1 or 2)");
    launch_confusion(logits, target, batch, classes, hw, cm, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel, int64_t step, double lr,
                   double beta1, double beta2, double eps, double weight_decay, int decoupled, void* hip_stream) {
    STCD_CHECK(params && grads && exp_avg && exp_avg_sq, "null pointer argument");
    STCD_CHECK(numel >= 1 && step >= 1, "numel and step must be >= 1");
    STCD_CHECK(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
               "buffers must be 16-byte aligned");
    // scalars are formed in double like torch's Python floats, then rounded once to fp32
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    launch_adam(params, grads, exp_avg, exp_avg_sq, numel, (float)lr, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                (float)eps, (float)weight_decay, decoupled ? 1 : 0, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)),
                (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_adam_hyper(int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, float* hyper_host8) {
    STCD_CHECK(hyper_host8 != nullptr && step >= 1, "bad argument");
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    hyper_host8[0] = (float)lr; hyper_host8[1] = (float)(1.0 - beta1); hyper_host8[2] = (float)beta2; hyper_host8[3] = (float)(1.0 - beta2);
    hyper_host8[4] = (float)eps; hyper_host8[5] = (float)weight_decay; hyper_host8[6] = (float)(lr / bc1); hyper_host8[7] = (float)(1.0 / sqrt(bc2));
    return 0;
}
int stcd_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel, const float* hyper_dev8,
                       int decoupled, void* hip_stream) {
    STCD_CHECK(params && grads && exp_avg && exp_avg_sq && hyper_dev8, "null pointer argument");
    STCD_CHECK(numel >= 1, "numel must be >= 1");
    launch_adam_dev(params, grads, exp_avg, exp_avg_sq, numel, hyper_dev8, decoupled ? 1 : 0, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_pseudo_pair(const uint8_t* img_a, const uint8_t* donor, const uint8_t* mask, const uint8_t* change, const float* alpha,
                     const int32_t* erase_xywh, uint64_t seed, int batch, int height, int width, const float* mean3,
                     const float* std3, float* x1, float* x2, int64_t* c_label, int64_t* s_label_a, int64_t* s_label_b,
                     void* hip_stream) {
    STCD_CHECK(img_a && donor && mask && change && x1 && x2 && c_label && mean3 && std3, "null pointer argument");
    STCD_CHECK(batch >= 1 && height >= 1 && width >= 1, "bad shape");
    STCD_CHECK(std3[0] > 0.f && std3[1] > 0.f && std3[2] > 0.f, "std must be positive");
    launch_pseudo_pair(img_a, donor, mask, change, alpha, erase_xywh, seed, batch, height, width, mean3, std3, x1, x2, c_label,
                       s_label_a, s_label_b, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int64_t stcd_augment_scratch_bytes(int n_images, int height, int width) {
    return (n_images >= 1 && height >= 1 && width >= 1) ? augment_scratch_bytes(n_images, height, width) : 0;
}
int stcd_augment(const float* x, const float* params, int n_images, int height, int width, const float* mean3, const float* std3,
                 float* out, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    STCD_CHECK(x && params && mean3 && std3 && out && scratch, "null pointer argument");
    STCD_CHECK(n_images >= 1 && n_images <= 65535 && height >= 1 && width >= 1, "bad shape");
    STCD_CHECK(std3[0] > 0.f && std3[1] > 0.f && std3[2] > 0.f, "std must be positive");
    STCD_CHECK(scratch_bytes >= augment_scratch_bytes(n_images, height, width), "scratch too small");
    STCD_CHECK(x != out, "in-place augmentation is not supported (the blur reads neighbours)");
    launch_augment(x, params, n_images, height, width, mean3, std3, out, scratch, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_selftrain_score(const float* const* logits, int n_models, int batch, int classes, int64_t hw, float threshold, const uint8_t* label,
                         int mask_value, uint8_t* mask, int64_t* agree, int64_t* cm, void* hip_stream) {
    STCD_CHECK(logits && mask, "null pointer argument");
    STCD_CHECK(n_models >= 1 && n_models <= STCD_SELFTRAIN_MAX_MODELS, "n_models must be in [1, 8]");
    SelftrainPtrs lg{};
    for (int k = 0; k < n_models; ++k) {
        STCD_CHECK(logits[k] != nullptr, "a logits pointer is null");
        lg.p[k] = logits[k];
    }
    STCD_CHECK(classes == 1 || classes == 2, "classes must be 1 or 2");
    STCD_CHECK(batch >= 0 && hw >= 0, "bad shape");
    STCD_CHECK(mask_value >= 1 && mask_value <= 255, "mask_value must be in [1, 255]");
    STCD_CHECK((agree == nullptr) == (n_models == 1), "agree is NULL if and only if n_models == 1");
    STCD_CHECK((label != nullptr) == (cm != nullptr), "label and cm go together");
    if (batch == 0 || hw == 0) return 0;
    launch_selftrain_score(lg, n_models, batch, classes, hw, threshold, label, mask_value, mask, agree, cm, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

int stcd_mask_close(const uint8_t* in, int height, int width, int radius, int mask_value, uint8_t* out, void* hip_stream) {
    STCD_CHECK(in && out, "null pointer argument");
    STCD_CHECK(height >= 0 && width >= 0, "bad shape");
    STCD_CHECK(radius >= 1 && radius <= 4, "radius must be in [1, 4]");
    STCD_CHECK(mask_value >= 1 && mask_value <= 255, "mask_value must be in [1, 255]");
    const uint64_t bytes = (uint64_t)height * (uint64_t)width, a = (uint64_t)(uintptr_t)in, b = (uint64_t)(uintptr_t)out;
    STCD_CHECK(a != b && (a < b ? b - a >= bytes : a - b >= bytes), "out must not overlap in (the passes read neighbours)");
    STCD_CHECK(mask_close_tiles(height, width) < ((int64_t)1 << 31), "more than 2^31 tiles");
    if (height == 0 || width == 0) return 0;
    launch_mask_close(in, height, width, radius, mask_value, out, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

static int check_geom(const stcd_conv_geom* g) {
    STCD_CHECK(g != nullptr, "geometry is null");
    STCD_CHECK(g->ntaps >= 1 && g->ntaps <= 9, "ntaps must be in [1,9]");
    STCD_CHECK(g->ci >= 8 && g->ci % 8 == 0 && g->ldi >= g->ci && g->ldi % 8 == 0, "ci/ldi must be multiples of 8");
    STCD_CHECK(g->co >= 1 && g->ldo >= g->co, "bad co/ldo");
    STCD_CHECK(g->in_stride >= 1 && g->out_stride >= 1 && g->n >= 1 && g->hm >= 1 && g->wm >= 1, "bad sizes");
    STCD_CHECK((g->hm - 1) * g->out_stride + g->oy0 < g->ho && (g->wm - 1) * g->out_stride + g->ox0 < g->wo,
               "output positions exceed the output buffer");
    return 0;
}
// split count of a stand-alone k_wgrad_dma launch (stcd_op_wgrad impl 7): one round of blocks over the 256 CUs, >= 8 K-tiles per block
static int op_dma_splits(const stcd_conv_geom& g, const WgradMfmaPlan& p) {
    const int64_t M = (int64_t)g.n * g.hi * g.wi;
    return (int)std::max<int64_t>(1, std::min<int64_t>(256 / std::max(1, p.gy * p.gz), M / 512));
}
int64_t stcd_op_scratch_bytes(const stcd_conv_geom* g) {
    if (!g) return 0;
    ConvMfmaPlan p = conv_mfma_plan(*g);
    WgradMfmaPlan w = wgrad_mfma_plan(*g, g->ci, g->co), ww = wgrad_mfma_plan(*g, g->ci, g->co, true);
    WgradMfmaPlan wg = wgrad_gemm_plan(*g, g->ci, g->co);
    WgradMfmaPlan wd = wgrad_dma_plan(*g, g->ci, g->co);
    if (wd.ok) wgrad_dma_set_split(wd, *g, op_dma_splits(*g, wd), g->ci, g->co);
    return std::max<int64_t>(p.wf_elems * 2, std::max(std::max(std::max(w.slab_floats, ww.slab_floats), wg.ok ? wg.slab_floats : 0), wd.ok ? wd.slab_floats : 0) * 4) + 1024;
}
int stcd_op_conv(int dtype, int impl, const stcd_conv_geom* g, const void* in, const float* w, const float* bias,
                 void* out, void* scratch, int64_t scratch_bytes, void* hip_stream) {
    if (check_geom(g)) return 1;
    STCD_CHECK(in && w && out, "null pointer argument");
    if (impl == 1 || impl == 2 || impl == 3 || impl == 6 || impl == 8) {
        STCD_CHECK(dtype == STCD_DTYPE_BF16, "the MFMA implementation is bf16 only");
        ConvOp op;      // the planners' answers for this geometry
        op.g = *g;
        op.plan = conv_mfma_plan(*g);
        const ConvMfmaPlan& p = op.plan;
        STCD_CHECK(p.ok, "geometry not supported by the MFMA kernel");
        STCD_CHECK(scratch && scratch_bytes >= p.wf_elems * 2, "scratch too small for the fragment-order filter");
        launch_pack_frag(*g, p, w, g->ci, g->co, scratch, (hipStream_t)hip_stream);
        ConvArgs a;      // one group, no statistics, no epilogue, NHWC; the filter image is `scratch`
        a.in = in; a.wf = scratch; a.bias = bias; a.out = out; a.s = (hipStream_t)hip_stream;
        ConvKernel kern = ConvKernel::MFMA;      // impl 2
        const char* const fail = impl == 2 ? "LDS budget exceeded" : impl == 1 ? "the chosen kernel rejected the geometry" : "launch failed";
        if (impl == 3) {      // resident-halo / streamed-filter kernel of the wide 3x3 layers (Ci % 64 == 0, Co % 128 == 0)
            op.halo = conv_halo_plan(*g, p);
            STCD_CHECK(op.halo.ok, "geometry not supported by the resident-halo kernel (3x3 stride 1, Ci % 64 == 0, Co % 128 == 0)");
            kern = ConvKernel::HALO;
        } else if (impl == 6) {      // 256 x 256 implicit-GEMM tile staged by LDS-DMA (Ci % 64 == 0, Co % 256 == 0, an even number >= 4 of K-tiles)
            op.dma = conv_dma_plan(*g, p);
            STCD_CHECK(op.dma.ok, "geometry not supported by the LDS-DMA kernel (Ci % 64 == 0, Co % 256 == 0, (Ci / 64) * taps even and >= 4)");
            kern = ConvKernel::DMA;
        } else if (impl == 8) {      // k_conv_res's tile staged by LDS-DMA (3x3 stride 1, Ci % 64 == 0, Co % 16 == 0; the engine's choice on small maps)
            op.tile = conv_tile_plan(*g, p, 1);
            STCD_CHECK(op.tile.ok, "geometry not supported by the LDS-DMA tile kernel (3x3 stride 1 over the full map, Ci % 64 == 0, Co % 16 == 0)");
            kern = ConvKernel::TILE;
        } else if (impl == 1) {
            // the engine's plans and the engine's choice with a fresh engine's switches; the kernels with an impl number of their own
            // (3 halo, 6 dma, 8 tile) stay behind those numbers
            stcd_engine sw;
            sw.dt = BF16;
            engine_env_switches(&sw);
            plan_conv(sw, op, 1, false);
            op.wf = 0;      // (not the reference kernel's launch: there is an image)
            kern = conv_kernel(true, sw.use_small, op, a,
                               ~(conv_kernel_bit(ConvKernel::DMA) | conv_kernel_bit(ConvKernel::HALO) | conv_kernel_bit(ConvKernel::TILE)));
        }
        STCD_CHECK(launch_conv(kern, op, a) == 0, fail);
        STCD_HIP(hipGetLastError());
        return 0;
    }
    STCD_CHECK(impl == 0, "impl must be 0 (reference FMA), 1 (MFMA, auto-selected kernel), 2 (generic MFMA kernel), 3 (resident-halo kernel), 6 (LDS-DMA kernel) or 8 (LDS-DMA tile kernel)");
    launch_conv_ref(dtype, *g, in, w, g->ci, g->co, bias, out, false, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}
// One named kernel with what the engine fuses into it (exec_conv's arguments, spelled out by the caller).  Everything is validated
// with the kernel's own planner and its launcher's own predicates BEFORE the filter is packed, so a refused combination launches
// nothing; the out-values are written as soon as the plan stands.
int stcd_op_conv_fused(const stcd_conv_geom* g, stcd_conv_fused* f, const void* in, const float* w, const float* bias, void* out,
                       void* scratch, int64_t scratch_bytes, void* hip_stream) {
    if (check_geom(g)) return 1;
    STCD_CHECK(f != nullptr, "the fused-features request is null");
    f->blocks = f->tiles_per_group = f->blocks_per_group = f->tile_m = 0;
    f->bn_rep = BN_REP;
    STCD_CHECK(in && w && out, "null pointer argument");
    STCD_CHECK(f->kernel >= STCD_CONV_SMALL && f->kernel <= STCD_CONV_DMA, "kernel must be one of STCD_CONV_*");
    const int groups = f->groups;
    STCD_CHECK(groups >= 1 && g->n % groups == 0, "groups must be >= 1 and divide n (whole images per BatchNorm group)");
    static const ConvKernel OF_ID[] = {ConvKernel::SMALL, ConvKernel::RES, ConvKernel::TILE,      // STCD_CONV_* -> ConvKernel, here alone
                                       ConvKernel::GEMM, ConvKernel::HALO, ConvKernel::DMA};
    static_assert(STCD_CONV_SMALL == 0 && STCD_CONV_RES == 1 && STCD_CONV_TILE == 2 && STCD_CONV_GEMM == 3 && STCD_CONV_HALO == 4 && STCD_CONV_DMA == 5, "OF_ID");
    const ConvKernel kern = OF_ID[f->kernel];
    const bool sums = f->sum_acc != nullptr, epi_on = f->use_epi != 0, bwd = f->bw_acc != nullptr;
    ConvEpi epi;
    BwdSum bs;
    ConvArgs a;      // the filter image is `scratch`
    a.in = in; a.wf = scratch; a.bias = bias; a.out = out; a.groups = groups; a.s = (hipStream_t)hip_stream;
    if (sums) a.sums = StatReq{(long long*)f->sum_acc, groups, f->sum_c0, f->sum_c, f->sum_scale1, f->sum_scale2};
    if (epi_on) a.epi = &epi;
    if (bwd) a.bs = &bs;
    const char* const refused = conv_refusal(kern, a, g->co);      // what the capability table says of this kernel
    STCD_CHECK(!refused, std::string(conv_kernel_str(kern)) + " does not take " + (refused ? refused : ""));
    if (sums) {
        STCD_CHECK(f->sum_c0 >= 0 && f->sum_c >= 1 && f->sum_c0 + f->sum_c <= g->co, "the summed channel slice lies outside the output channels");
        STCD_CHECK(f->sum_scale1 > 0.f && f->sum_scale2 > 0.f, "the sum scales must be positive");
    }
    if (epi_on) {
        STCD_CHECK(!f->gate || (f->ldg >= g->co && f->ldg % 8 == 0), "gate: the pixel stride must be a multiple of 8 and >= co");
        STCD_CHECK(!f->res || (f->ldr >= g->co && f->ldr % 8 == 0), "res: the pixel stride must be a multiple of 8 and >= co");
        STCD_CHECK(f->res || (f->alpha == 1.f && f->beta == 1.f), "alpha / beta combine the output with a residual: without one they must be 1");
        epi.relu = f->relu ? 1 : 0;
        epi.gate = f->gate; epi.ldg = f->ldg; epi.res = f->res; epi.ldr = f->ldr; epi.alpha = f->alpha; epi.beta = f->beta;
    }
    if (bwd) {
        STCD_CHECK(f->bw_y && f->bw_stat, "BatchNorm-backward sums need the layer's conv output and its statistics");
        STCD_CHECK(f->bw_ldy >= g->co && f->bw_ldy % 4 == 0, "bw_y: the pixel stride must be a multiple of 4 and >= co");
        bs.Y = f->bw_y; bs.ldy = f->bw_ldy; bs.stat = f->bw_stat; bs.mask = f->bw_mask; bs.acc = (long long*)f->bw_acc; bs.groups = groups;
    }
    ConvOp op;      // the named kernel's own plan for the requested groups
    op.g = *g;
    op.plan = conv_mfma_plan(*g);
    const ConvMfmaPlan& p = op.plan;
    STCD_CHECK(p.ok, "geometry not supported by the MFMA kernels");
    STCD_CHECK(scratch && scratch_bytes >= p.wf_elems * 2, "scratch too small for the fragment-order filter");
    const int64_t tiles16 = (int64_t)g->n * ((g->hm + 15) / 16) * ((g->wm + 15) / 16);
    if (kern == ConvKernel::SMALL) {
        STCD_CHECK(conv_small_ok(*g, p) && conv_small_call_ok(*g, groups, nullptr), "geometry not supported by k_conv_small (one n-tile, <= 5 k-steps)");
        STCD_CHECK(!bwd || conv_small_bwdsum_ok(*g), "k_conv_small forms BatchNorm-backward sums for 16 channels out, whole 8 x 16 tiles, 3 or 5 k-steps");
        f->blocks = conv_small_blocks(*g, groups);
        f->blocks_per_group = f->blocks / groups;
        f->tiles_per_group = (int)((int64_t)g->n * ((g->hm + 7) / 8) * ((g->wm + 15) / 16) / groups);
    } else if (kern == ConvKernel::RES) {
        op.res = conv_res_plan(*g, p, groups);
        STCD_CHECK(op.res.ok, "geometry not supported by k_conv_res (3x3 stride 1, Ci % 32 == 0)");
        STCD_CHECK(!bwd || conv_res_bwdsum_ok(*g, op.res), "this k_conv_res plan forms no BatchNorm-backward sums (slices of one or two n-tiles, double halo)");
        f->blocks = op.res.blocks; f->blocks_per_group = op.res.P; f->tiles_per_group = (int)(tiles16 / groups);
    } else if (kern == ConvKernel::TILE) {
        op.tile = conv_tile_plan(*g, p, groups);
        STCD_CHECK(op.tile.ok, "geometry not supported by k_conv_tile (3x3 stride 1 over the full map, Ci % 64 == 0, Co % 16 == 0)");
        f->blocks = op.tile.blocks; f->blocks_per_group = op.tile.P; f->tiles_per_group = (int)(tiles16 / groups);
    } else if (kern == ConvKernel::GEMM) {
        op.gemm = conv_gemm_plan(*g, p, groups);
        STCD_CHECK(op.gemm.ok, "geometry not supported by k_conv_gemm (Ci % 64 == 0, Co % 64 == 0)");
        f->blocks = op.gemm.blocks; f->blocks_per_group = op.gemm.tiles_m; f->tiles_per_group = op.gemm.tiles_m; f->tile_m = 32 * op.gemm.W;
    } else if (kern == ConvKernel::HALO) {
        op.halo = conv_halo_plan(*g, p);
        STCD_CHECK(op.halo.ok, "geometry not supported by k_conv_halo (3x3 stride 1, Ci % 128 == 0, Co % 128 == 0)");
        f->blocks = op.halo.blocks; f->blocks_per_group = op.halo.P; f->tiles_per_group = (int)tiles16;
    } else {
        op.dma = conv_dma_plan(*g, p);
        STCD_CHECK(op.dma.ok, "geometry not supported by k_conv_dma (Ci % 64 == 0, Co % 256 == 0, (Ci / 64) * taps even and >= 4)");
        f->blocks = op.dma.blocks; f->blocks_per_group = std::min(op.dma.blocks, op.dma.tiles_m); f->tiles_per_group = op.dma.tiles_m;
    }
    launch_pack_frag(*g, p, w, g->ci, g->co, scratch, a.s);
    STCD_CHECK(launch_conv(kern, op, a) == 0, "the named kernel's launcher rejected the combination");
    STCD_HIP(hipGetLastError());
    return 0;
}
int stcd_op_wgrad(int dtype, int impl, const stcd_conv_geom* g, const void* in, const void* dout, float* dw, void* scratch,
                  int64_t scratch_bytes, void* hip_stream) {
    if (check_geom(g)) return 1;
    STCD_CHECK(in && dout && dw, "null pointer argument");
    if (impl == 1 || impl == 4 || impl == 5) {      // 4: the tile kernel with its 64 x 32-channel tile allowed (the SNUNet engine's choice); 5: 64 x 64
        STCD_CHECK(dtype == STCD_DTYPE_BF16, "the MFMA implementation is bf16 only");
        WgradMfmaPlan p = wgrad_mfma_plan(*g, g->ci, g->co, impl >= 4, impl == 5 ? 1 : 0);
        STCD_CHECK(p.ok, "geometry not supported by the MFMA kernel");
        STCD_CHECK(scratch && scratch_bytes >= p.slab_floats * 4, "scratch too small for the partial slabs");
        STCD_CHECK(launch_wgrad_mfma(*g, p, in, dout, (float*)scratch, g->ci, g->co, (hipStream_t)hip_stream) == 0, "LDS budget exceeded");
        launch_reduce_dw((const float*)scratch, p.gx, *g, g->ci, g->co, g->ci, g->co, nullptr, dw, (hipStream_t)hip_stream);
        STCD_HIP(hipGetLastError());
        return 0;
    }
    // 7: the LDS-DMA kernel, 256 x 256 channel tile per (position split, tap) block (ChangeFormer's 256 -> 256 3x3 layers)
    // 3: one-tap launches on the position-GEMM kernel (the engine's choice for Ci, Co >= 64)
    // either as a grouped launch of one job: `scratch` holds the slabs, then the job table
    if (impl == 3 || impl == 7) {
        STCD_CHECK(dtype == STCD_DTYPE_BF16, "the MFMA implementation is bf16 only");
        WgradMfmaPlan p = impl == 7 ? wgrad_dma_plan(*g, g->ci, g->co) : wgrad_gemm_plan(*g, g->ci, g->co);
        STCD_CHECK(p.ok, impl == 7 ? "geometry not supported by the LDS-DMA weight-gradient kernel (stride 1, full map >= 64 wide, Ci % 256 == 0, Co % 256 == 0)"
                                   : "geometry not supported by the GEMM weight-gradient kernel (one tap, Ci >= 64, Co >= 64)");
        if (impl == 7) wgrad_dma_set_split(p, *g, op_dma_splits(*g, p), g->ci, g->co);
        const int64_t table = (p.slab_floats * 4 + 255) & ~(int64_t)255;
        STCD_CHECK(scratch && scratch_bytes >= table + (int64_t)sizeof(WgradJob), "scratch too small for the partial slabs + job table");
        const WgradKernel k = wgrad_kernel_of(p, *g, false);
        const WgradJob j = wgrad_job(k, *g, p, (int64_t)(intptr_t)in, (int64_t)(intptr_t)dout, (int64_t)(intptr_t)scratch, g->ci, g->co);
        STCD_HIP(hipMemcpyAsync((char*)scratch + table, &j, sizeof(j), hipMemcpyHostToDevice, (hipStream_t)hip_stream));
        STCD_HIP(hipStreamSynchronize((hipStream_t)hip_stream));       // `j` is a stack object
        STCD_CHECK(launch_wgrad_jobs(k, (const WgradJob*)((char*)scratch + table), 1, p.gx * p.gy * p.gz, j.lds_bytes, nullptr, (hipStream_t)hip_stream) == 0, "LDS budget exceeded");
        launch_reduce_dw((const float*)scratch, p.gx, *g, g->ci, g->co, g->ci, g->co, nullptr, dw, (hipStream_t)hip_stream);
        STCD_HIP(hipGetLastError());
        return 0;
    }
    STCD_CHECK(impl == 0, "impl must be 0 (reference FMA), 1 / 4 (MFMA tile kernel, 4: wide tile allowed), 3 (MFMA position-GEMM kernel) or 7 (LDS-DMA kernel)");
    STCD_HIP(hipMemsetAsync(dw, 0, (size_t)g->ntaps * g->ci * g->co * 4, (hipStream_t)hip_stream));
    launch_wgrad_ref(dtype, *g, in, dout, dw, g->ci, g->co, (hipStream_t)hip_stream);
    STCD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
