/* stcd_hip.h -- C ABI of the MI355X (gfx950) bi-temporal change-detection engine.
 *
 * The reference (VCISwang/STCD) has NO native interface: its hot path sits behind a Python
 * torch.nn.Module duck-type built by a factory:
 *     define_G(args)            /root/reference/models/networks.py:138-215
 *     Module(input_nbr,label_nbr).forward(x1,x2) -> logits
 *                               /root/reference/models/SiamUnet_diff.py:13,94-181
 *                               /root/reference/models/SiamUnet_conc.py:94-181
 *                               /root/reference/models/SiamUnet_sub.py:94-180
 *                               /root/reference/models/SNUNet.py:63-152
 *     loss(logits,label)        /root/reference/models/losses.py:6-21 (cross_entropy), :24-34 (cd_loss)
 * This header is the boundary a maintainer would bind instead (ctypes stub: INTEGRATION.md): plain
 * pointers and sizes, no torch types.  All pointers are DEVICE pointers unless a parameter says "host".
 * Every entry point returns 0 on success; on failure it returns non-zero and stcd_last_error() gives
 * the reason (thread-local).  No exceptions cross the ABI.  An engine handle is not thread-safe: one
 * handle per process / per GPU (the reference pins nn.DataParallel to one device,
 * /root/reference/train_pse_cd.py:405-417).
 *
 * Ownership: the caller owns inputs, parameters, gradients, outputs and the workspace; the engine borrows
 * them for the duration of one call, enqueued on the caller's HIP stream.  The engine allocates no device
 * memory and never synchronises the device.
 */
#ifndef STCD_HIP_H
#define STCD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STCD_ABI_VERSION 2

/* network family: replaces the class chosen by define_G (networks.py:145-169) */
#define STCD_ARCH_DIFF 0   /* "SiamUnet_abs"  -> SiamUnet_diff  */
#define STCD_ARCH_CONC 1   /* "SiamUnet_conc" -> SiamUnet_conc  */
#define STCD_ARCH_SUB 2    /* "SiamUnet_sub"  -> SiamUnet_sub   */
#define STCD_ARCH_SNUNET 3 /* "SNUNet"        -> SNUNet_ECAM    */
#define STCD_ARCH_SEGCD 4  /* smp.SegCD(encoder_name="resnet50"): the model the scripts train (train_pse_cd.py:419-427,
                            * segmentation_models_pytorch/decoders/unet/model.py:267-332).  Its forward returns THREE maps
                            * (mask_t1, mask_t2, change): `logits` / `grad_logits` of stcd_forward / stcd_backward hold
                            * [3*batch, label_ch, H, W] floats in that order; H and W must be divisible by 32. */
/* the same class over the other plain ResNet encoders of the reference's registry
 * (segmentation_models_pytorch/encoders/resnet.py:126-171; blocks: models/resnet.py:37-75 BasicBlock, :78-124 Bottleneck) */
#define STCD_ARCH_SEGCD_R18 5  /* encoder_name="resnet18":  BasicBlock  [2, 2, 2, 2]  */
#define STCD_ARCH_SEGCD_R34 6  /* encoder_name="resnet34":  BasicBlock  [3, 4, 6, 3]  */
#define STCD_ARCH_SEGCD_R101 7 /* encoder_name="resnet101": Bottleneck  [3, 4, 23, 3] */
#define STCD_ARCH_SEGCD_R152 8 /* encoder_name="resnet152": Bottleneck  [3, 8, 36, 3] */
/* "Unet" -> Unet, the FC-EF network of the same paper (models/Unet.py:10-154; define_G name "Unet", models/networks.py:144-145): ONE
 * encoder stream over cat(x1, x2) (conv11 takes 2 * in_ch channels, in_ch <= 4), skips = the stream's own activations, decoder and
 * state_dict layout of SiamUnet_diff; forward returns the logits tensor. */
#define STCD_ARCH_FCEF 9
/* "SiamUnet_cross_conc" -> SiamUnet_cross_conc (models/SiamUnet_crossconc.py:35-212; define_G name, models/networks.py:152-153): the
 * FC-Siam encoder / decoder with a cross_conc block on every skip (:11-33: the two dates' channels interleaved into a grouped 3x3
 * conv (C groups of 2 -> 1), BatchNorm, ReLU, a 3x3 conv C -> C, BatchNorm, ReLU); forward returns [logits]. */
#define STCD_ARCH_XCONC 10
/* Siam_NestedUNet_Conc, "SNUNet-CD without attention" (models/SNUNet.py:155-243; no define_G name in the reference): the trunk
 * and state_dict layout of SNUNet_ECAM without ca / ca1, then final1..final4 (Conv2d(32, label_ch, 1) on x0_1..x0_4) and
 * conv_final (Conv2d(4 * label_ch, label_ch, 1)) over their concat.  H and W must be divisible by 16.  The head runs as one
 * composed 1x1 conv 128 -> label_ch over cat(x0_1..x0_4), streamed once per direction by kernels of its own that read / write the
 * fp32 NCHW maps directly (no packed output gradient, no output_1..4 in memory); both ids take that path. */
#define STCD_ARCH_SNUNET_CONC 11 /* forward returns the fused map: logits [batch, label_ch, H, W] */
/* the same network with deep supervision (models/SNUNet.py:155-243 computes output1..4 and drops them; models/trainer.py:300-309
 * trains on a list): `logits` / `grad_logits` hold FIVE maps, map-major, [5*batch, label_ch, H, W] = output1, output2, output3,
 * output4, output (the [3*batch, ...] convention of STCD_ARCH_SEGCD); the last map equals STCD_ARCH_SNUNET_CONC's output bit for
 * bit.  label_ch <= 2. */
#define STCD_ARCH_SNUNET_CONC_DS 12
/* smp.UnetSeg (decoders/unet/model.py:109-171), the single-image ResNet UNet train_sup.py:303 trains: the same encoder /
 * decoder / head on ONE image batch (x2 of stcd_forward is ignored; BatchNorm over the whole batch; logits [batch, label_ch,
 * H, W]).  STCD_ARCH_UNETSEG + k, k = 0..4: resnet50, resnet18, resnet34, resnet101, resnet152 (the order of the ids above). */
#define STCD_ARCH_UNETSEG 16
/* smp.FFCTLCD (decoders/unet/model.py:335-423; the commented alternative of train_pse_cd.py:419 / train_stcd.py:637): shared
 * encoder on both dates, the shared decoder + head on |f1 - f2| (feature level), f1 and f2 -- three decoder passes with their
 * own BatchNorm batch statistics, in that order --, change = min(head(dec(|f1 - f2|)), |mask_t1 - mask_t2|).  Same outputs as
 * STCD_ARCH_SEGCD ([3*batch, label_ch, H, W] = mask_t1, mask_t2, change).  STCD_ARCH_FFCTLCD + k, k as above. */
#define STCD_ARCH_FFCTLCD 32
/* "base_resnet18" -> ResNet, the CNN baseline of the BIT family (models/networks.py:223-304; define_G name, :172-173): a BasicBlock
 * ResNet trunk that stays at 1/8 resolution (layer3 / layer4 run at stride 1, dilation 1: models/resnet.py:47-48) shared by both
 * dates with per-date BatchNorm statistics, nearest x2, conv_pred (3x3, bias, -> 32), |x1 - x2|, bilinear x4 (align_corners =
 * False), classifier (conv3x3 32 -> 32, BatchNorm over the batch, ReLU, conv3x3 32 -> label_ch with bias); logits [batch,
 * label_ch, H, W].  STCD_ARCH_BASE_RESNET + k: k = 0 resnet18 / resnet_stages_num 5, 1 resnet18 / 4 (the trunk stops after
 * layer3), 2 resnet34 / 5, 3 resnet34 / 4.  Every tensor of the class's state_dict is a parameter of the engine, also the ones
 * no output depends on (resnet.fc.*, resnet.layer4.* at 4 stages): their gradient is exactly zero.  H and W must be divisible
 * by 32; in_ch must be 3. */
#define STCD_ARCH_BASE_RESNET 48
/* BIT: BASE_Transformer (models/networks.py:307-441) = the trunk above (resnet18, resnet_stages_num 4) with the token path between
 * conv_pred and |x1 - x2|: semantic tokenizer (conv_a 1x1 32 -> 4 without bias, softmax over the positions of an image, 4 tokens per
 * date), one token-encoder layer over the 8 tokens of a pair (+ pos_embedding; 8 heads, dim_head 64), and a cross-attention decoder
 * over every pixel of each date with that date's 4 tokens as memory.  Both attentions scale by dim ** -0.5 = 32 ** -0.5.
 * STCD_ARCH_BIT + k: k = 0 dec_depth 1 / decoder_dim_head 64 ("base_transformer_pos_s4"), 1: 8 / 64 ("..._dd8"), 2: 8 / 8
 * ("..._dd8_dedim8").  The parameter table is in named_parameters() order: pos_embedding first (flat offset 0), then the trunk's
 * tensors, conv_a.weight, transformer.layers.0.*, transformer_decoder.layers.*.  logits [batch, label_ch, H, W]. */
#define STCD_ARCH_BIT 52

/* ChangeFormerV6 (/root/reference/models/ChangeFormer.py:1669-1701; define_G name "ChangeFormerV6", models/networks.py:195-196;
 * BASELINE.json configs[4]): hierarchical transformer encoder shared by both dates + MLP / conv-difference decoder.  Its forward
 * returns FIVE maps [p_c4, p_c3, p_c2, p_c1, cp] (ChangeFormer.py:1578-1622): `logits` of stcd_forward holds them back to back
 * (stcd_cf_output_info gives offset / size of each; stcd_output_floats the total), `grad_logits` of stcd_backward has the same
 * layout and only the gradient of the LAST map (cp) is propagated (the reference's loss uses G_pred[-1], models/trainer.py:311).
 * H and W must be divisible by 32.  stcd_create(STCD_ARCH_CHANGEFORMER, ...) builds the V6 configuration with embed_dim 256;
 * stcd_create_changeformer takes any configuration of the same class family. */
#define STCD_ARCH_CHANGEFORMER 64

/* arithmetic / storage type of activations. Parameters, gradients, BN statistics, logits: always fp32. */
#define STCD_DTYPE_F32 0  /* parity mode: fp32 storage, fp32 FMA */
#define STCD_DTYPE_BF16 1 /* production: bf16 storage, MFMA with fp32 accumulation */

typedef struct stcd_engine stcd_engine;

typedef struct stcd_tensor_info {
    char name[64];    /* reference state_dict key, e.g. "conv43d.weight" */
    int32_t ndim;
    int64_t shape[4]; /* reference shape, e.g. (256,128,3,3) */
    int64_t offset;   /* element offset into the flat fp32 parameter / gradient buffer */
    int64_t numel;
} stcd_tensor_info;

typedef struct stcd_bn_info {
    char name[64];           /* module name, e.g. "bn11": buffers are name.running_mean / name.running_var */
    int32_t channels;
    int32_t calls_per_forward; /* 2 for the shared encoder (T1 then T2), 1 otherwise: num_batches_tracked increment */
    int64_t offset;          /* running_mean at offset, running_var at offset+channels, in the flat BN buffer */
} stcd_bn_info;

typedef struct stcd_dropout_info {
    char name[64];   /* module name, e.g. "do11" */
    int32_t rows;    /* 2*batch for encoder layers (T1 rows then T2 rows), batch for decoder layers */
    int32_t channels;
    int64_t offset;  /* element offset into the flat fp32 mask buffer; mask[row*channels + c] in {0, 1/(1-p)} */
} stcd_dropout_info;

/* ChangeFormerV6.__init__ / EncoderTransformer_v3.__init__ arguments (ChangeFormer.py:1671-1691, 1344-1348) */
typedef struct stcd_cf_config {
    int32_t in_ch, out_ch;          /* input_nc, output_nc */
    int32_t embed_dims[4];          /* [64, 128, 320, 512] */
    int32_t depths[4];              /* [3, 3, 4, 3] */
    int32_t num_heads[4];           /* [1, 2, 4, 8] */
    int32_t sr_ratios[4];           /* [8, 4, 2, 1] */
    int32_t mlp_ratio;              /* 4 */
    int32_t embedding_dim;          /* embed_dim = 256: decoder width */
    int32_t patch1, patch;          /* patch_embed1: k7 s4; patch_embed2..4: k = patch_size = 7, s2 */
    float drop_rate, attn_drop, drop_path_rate;   /* 0.1, 0.1, 0.1 */
    float diff_drop;                /* conv_diff's nn.Dropout(p=0.6), ChangeFormer.py:1143 */
} stcd_cf_config;

/* one Dropout / DropPath site of the configured ChangeFormer engine: masks are never stored -- element i of the site (linear index
 * over dims, the engine's NHWC / [image, head, query, key] order; encoder sites hold both dates: 2*batch images, date 1 first)
 * is kept iff (fmix32(i * 0x9E3779B1 + stcd_cf_site_seed(seed, site)) >> 8) >= floor(p * 2^24), and scaled by 1 / (1 - p). */
typedef struct stcd_cf_site {
    char name[96];                  /* e.g. "Tenc_x2.block1.0.attn.attn_drop", "TDec_x2.diff_c4.3" */
    int32_t ndim;
    int32_t dims[4];
    float p;
} stcd_cf_site;

const char* stcd_last_error(void);
int stcd_abi_version(void);

/* ---- engine lifecycle: replaces Module.__init__ (SiamUnet_diff.py:13-92, SNUNet.py:65-113) ---- */
int stcd_create(int arch, int in_ch, int label_ch, int dtype, stcd_engine** out);
int stcd_cf_default_config(stcd_cf_config* cfg);                     /* the ChangeFormerV6 values above */
int stcd_create_changeformer(const stcd_cf_config* cfg, int dtype, stcd_engine** out);
void stcd_destroy(stcd_engine* e);
/* floats of the `logits` / `grad_logits` buffers for the current configuration (every family) */
int64_t stcd_output_floats(const stcd_engine* e);
/* ChangeFormer: output map i (0..4 = p_c4, p_c3, p_c2, p_c1, cp), each [batch, out_ch, height, width] fp32 NCHW at `offset` floats */
int stcd_cf_output_info(const stcd_engine* e, int i, int64_t* offset, int* height, int* width);
int stcd_cf_num_sites(const stcd_engine* e);
int stcd_cf_site_get(const stcd_engine* e, int i, stcd_cf_site* out);
uint32_t stcd_cf_site_seed(uint64_t seed, int site);
/* change the element-wise dropout rates of a ChangeFormer engine (re-run stcd_configure afterwards); DropPath rates are fixed at
 * creation (they are a per-block schedule) */
int stcd_cf_set_drop_rates(stcd_engine* e, float drop_rate, float attn_drop, float diff_drop);
/* multi_scale_train (models/trainer.py:300-309: the loss is a weighted sum over ALL five predictions): on != 0 makes stcd_backward
 * propagate the gradients of the four auxiliary maps too -- `grad_logits` then carries d(loss)/d(p_c4 ... p_c1, cp) in the output
 * layout of stcd_cf_output_info (make_prediction, models/ChangeFormer.py:1151-1157: conv - ReLU - BatchNorm - conv per scale).  Off
 * (the default, multi_scale_train == "False", trainer.py:311): only cp's gradient is read and the heads' backward launches are not
 * part of the plan.  Changing the setting invalidates the plan: call stcd_configure (and re-query stcd_workspace_bytes) afterwards. */
int stcd_cf_set_aux_backward(stcd_engine* e, int on);
/* FC-Siam family (SiamUnet_diff / _conc / _sub / _cross_conc, Unet), SNUNet_ECAM and ChangeFormerV6: with the whole backward in ONE stcd_backward call
 * (stage -1) the grouped weight gradients go out as soon as their last operand exists, on a low-priority side stream of the engine
 * beside the rest of the backward chain, and are joined before the call's work on `hip_stream` ends; the FC-Siam decoder's grids and
 * ChangeFormer's LDS-DMA group are planned smaller for that.  on == 0 plans and runs them on the caller's
 * stream -- what a data-parallel caller wants, which calls stage 0 and stage 1 separately to all-reduce the decoder's gradients
 * (nn.DataParallel's role in /root/reference/models/networks.py:85-116) in between (staged calls never use the side stream).  Default on
 * (environment STCD_WGRAD_SIDE=0: off).  Changing the setting invalidates the plan: call stcd_configure afterwards. */
int stcd_set_wgrad_side(stcd_engine* e, int on);

/* ---- parameter / buffer enumeration in the reference's registration order (state_dict compatibility,
 *      /root/reference/models/trainer.py:138,183; basic_model.py:35) ---- */
int stcd_num_params(const stcd_engine* e);
int stcd_param_info(const stcd_engine* e, int i, stcd_tensor_info* info);
int64_t stcd_param_floats(const stcd_engine* e);
int stcd_num_bn(const stcd_engine* e);
int stcd_bn_info_get(const stcd_engine* e, int i, stcd_bn_info* info);
int64_t stcd_bn_floats(const stcd_engine* e);

/* ---- shape binding: batch = image PAIRS per call; height/width as the reference accepts (any >= 16;
 *      ReplicationPad2d branch, SiamUnet_diff.py:149, for sizes not divisible by 16) ---- */
int stcd_configure(stcd_engine* e, int batch, int height, int width);
int64_t stcd_workspace_bytes(const stcd_engine* e);
int stcd_num_dropout(const stcd_engine* e);
int stcd_dropout_info_get(const stcd_engine* e, int i, stcd_dropout_info* info);
int64_t stcd_dropout_floats(const stcd_engine* e);
/* Dropout2d probability (reference: 0.2, SiamUnet_diff.py:20); 0 disables dropout in training mode. */
int stcd_set_dropout_p(stcd_engine* e, float p);

/* ---- forward: replaces Module.forward(x1,x2) (SiamUnet_diff.py:94-181) ----
 * x1,x2      fp32 NCHW [batch,in_ch,H,W]
 * params     flat fp32 parameters (layout: stcd_param_info)
 * bn_running flat fp32 running stats (layout: stcd_bn_info_get); updated in place when training != 0
 * dropout_masks  nullable; when given (training only) these masks are used verbatim (parity tests);
 *            when NULL and training, masks are drawn on-device from (dropout_seed) by a counter hash
 * logits     fp32 NCHW [batch,label_ch,H,W]
 */
int stcd_forward(stcd_engine* e, const float* x1, const float* x2, const float* params, float* bn_running,
                 const float* dropout_masks, uint64_t dropout_seed, int training, float* logits,
                 void* workspace, void* hip_stream);

/* ---- backward: replaces autograd through the module (loss.backward(), trainer.py:313) ----
 * Must follow a training-mode stcd_forward on the same workspace.  grads (flat fp32, layout of params) is
 * OVERWRITTEN with d loss / d param.  stage: -1 = whole backward; 0 = decoder half (its gradients are final
 * when it returns, so a data-parallel caller may start reducing them), 1 = encoder half.
 * ONE backward per forward: the backward kernels overwrite the stored activations and output gradients in place, so stage -1 and
 * stage 1 consume the forward -- a further stcd_backward (any stage) fails until the next training-mode stcd_forward.  Stage 0
 * does not consume it: stage 0 followed by stage 1 is the staged form of one backward.
 */
int stcd_backward(stcd_engine* e, const float* grad_logits, const float* params, float* grads,
                  void* workspace, int stage, void* hip_stream);
/* Inference loops: every stcd_forward repacks the filters from `params` into the workspace (the optimizer rewrites them each
 * training step).  A caller that KNOWS the parameters are unchanged declares it with a non-zero tag: while the tag, the workspace
 * and the parameter pointer stay the same the repack is skipped (0.3 ms of a 3.5 ms SegCD eval forward).  tag 0 (default): always
 * repack.  Changing the parameters without changing the tag is the caller's error. */
int stcd_set_weights_tag(stcd_engine* e, uint64_t tag);
/* [begin,end) element range of the flat gradient buffer that stage 0 finalises (the rest belongs to stage 1). */
int stcd_grad_stage_range(const stcd_engine* e, int stage, int64_t* begin, int64_t* end);

/* ---- test introspection: the named activation / gradient tensors of the CURRENT configuration inside the workspace, so a
 *      parity test can check every layer of a deep network IN PLACE (layer output against a convolution of the layer's own
 *      stored input, weight gradient against the stored input and output gradient ...) at per-op tolerance, independent of how
 *      rounding differences grow through the depth.  Filled for the STCD_ARCH_SEGCD* families ("<conv name>.in|.Y|.A|.dY|.dIn|.res")
 *      (STCD_ARCH_BASE_RESNET also: "conv_pred.in|.Y|.dY|.dIn", no BatchNorm; "upsamplex4.in|.Y|.dY|.dIn", the bilinear step;
 *      STCD_ARCH_BIT also, always fp32 for the tokens: "bit.tokens.in|.Y|.dY|.dIn" [2*batch, 1, 4, 32], the tokens before / after the
 *      encoder and their gradients, and "bit.dec.in|.Y|.dY|.dIn", the decoder's maps -- conv_pred.dY = bit.dec.dIn + the tokenizer's
 *      data gradient)
 *      and the FC-Siam families ("<conv name>.in|.Y|.A.g0|.A.g1|.dY"; the activation per date),
 *      and the three SNUNet ids: per block "convL_J.in|.Y1|.A1|.Y2|.Out|.dZ2|.dY2|.dY1|.dIn" (both dates of an encoder level in one
 *      tensor, date 0 first; ".P|.dP" for the pooled encoder blocks; no ".dIn" for conv0_0; ".dY2" / ".dY1" are the dOut / dA1
 *      buffers as the backward leaves them; conv0_1..conv0_4's ".Out" is a channel slice, ld = 128, of the head's input), per
 *      transposed conv "UpL_J.in|.Y|.dY|.dIn" (".in": the lower block's ".Out", its date-1 half below an encoder level; ".Y" / ".dY":
 *      the tail slice of the consumer's ".in" / ".dIn"), and the head: "ecam.in|.Y|.dY" + "conv_final.dY" (the packed 8-channel
 *      gradient), or "head.in" for the two Conc ids.
 *      NHWC: element (n, y, x, ch) at offset_bytes + (((n*h + y)*w + x)*ld + ch) * elem_size.
 *      stcd_set_debug bit 0 (before stcd_configure): every layer writes its input gradient to a buffer of its own (the
 *      producer gathers it) instead of in place into the producer's gradient tensor, so ".dIn" survives the backward.
 *      SNUNet: the bit adds copies of the two values its backward overwrites, in buffers of their own at the end of the
 *      workspace -- "convL_J.dOut", the gathered output gradient before bn2's backward runs in place on it, and "ecam.dIn" /
 *      "head.dIn", the head's data gradient before conv0_1..conv0_4 gather into it; without the bit neither exists.
 *      stcd_set_debug bit 1 (value 2; FC-Siam family, for tests and A/B runs): the step's entry work goes out as the separate
 *      launches it was before they were merged -- dropout masks, weight pack, arena memset and input pack in front of the forward
 *      (otherwise one k_step_prologue launch), the memset of the gradient buffer in front of the backward (otherwise extra blocks
 *      of the k_gout_pack launch), and ONE slab-reduce launch for all of stage 1's weight gradients behind the last of them, on the
 *      side stream (otherwise the reduce of the groups that go out early follows them there, and the last group and its reduce run
 *      on the caller's stream).  Same workspace layout, same bits in every result. */
typedef struct stcd_ws_tensor {
    char name[96];
    int64_t offset_bytes;
    int n, h, w, c, ld;
    int dtype;
} stcd_ws_tensor;
int stcd_set_debug(stcd_engine* e, int flags);
/* Test introspection of the step's entry and tail, as the last stcd_configure planned them and the last backward ran them:
 *   entry_fused        1: the forward opens with one k_step_prologue launch and the backward's k_gout_pack clears the gradient buffer
 *                      (FC-Siam family without stcd_set_debug bit 1); 0: separate launches
 *   reduce_early_jobs, reduce_final_jobs   slab-reduce jobs of backward stage 1 that are summed behind the groups that go out early /
 *                      behind the final group; both 0: one reduce launch for the stage (debug bit 1, other families, no MFMA plan)
 *   last_tail          the last backward's stage-1 tail: bit 0 the early part went out behind its groups, bit 1 the final group and its
 *                      reduce ran on the caller's stream (single-call backward with the side stream); 0 before any backward */
int stcd_seam_plan(const stcd_engine* e, int* entry_fused, int* reduce_early_jobs, int* reduce_final_jobs, int* last_tail);
int stcd_ws_tensor_count(const stcd_engine* e);
int stcd_ws_tensor_get(const stcd_engine* e, int index, stcd_ws_tensor* out);

/* ---- measurement aid (bench.py): when enabled, every launch of the engine's kernel classes is bracketed by a
 *      hipEvent pair on the caller's stream; stcd_profile_read sums one class (it synchronises those events) and
 *      reports the ALGORITHMIC work of the same launches (each tensor counted once).
 *      Classes: 0 conv/dgrad  1 wgrad  2 bn-stats  3 bn+relu+dropout(+pool)  4 bn-backward reduce
 *               5 bn-backward apply  6 pool/fusion backward  7 packing. */
#define STCD_PROFILE_CLASSES 8
int stcd_profile_enable(stcd_engine* e, int on);
int stcd_profile_read(stcd_engine* e, int klass, double* total_ms, int64_t* launches, double* flops, double* bytes);
/* the same records grouped by kernel NAME (a substring of the name rocprofv3 prints, e.g. "k_conv_mfma<4>") */
int stcd_profile_num_kernels(const stcd_engine* e);
int stcd_profile_kernel(stcd_engine* e, int i, char* name, int name_cap, double* total_ms, int64_t* launches, double* flops,
                        double* bytes);

/* ---- losses, fused forward+backward: replace cross_entropy (losses.py:6-21) and
 *      cd_loss(sigmoid(x),y) == BCE_DICE (losses.py:24-34; train_pse_cd.py:227-228,436-462) ----
 * loss_out: one fp32 on the device.  dlogits nullable.  scratch: >= stcd_loss_scratch_bytes() bytes.
 */
int64_t stcd_loss_scratch_bytes(void);
int stcd_loss_ce(const float* logits, const int64_t* target, int batch, int classes, int64_t hw, int ignore_index,
                 float* loss_out, float* dlogits, void* scratch, void* hip_stream);
/* from_logits bit 0 set: x are logits, the loss is cd_loss(sigmoid(x), y) and dx is d loss / d logits (fused form used by
 * the script-shaped loop); clear: x are probabilities, exactly cd_loss(x, y) with dx = d loss / d probability.
 * bit 1 set: the Dice term alone (class Dice, train_pse_cd.py:436-447), without the BCE term. */
int stcd_loss_bce_dice(const float* x, const float* target, int64_t numel, int from_logits, float* loss_out, float* dx,
                       void* scratch, void* hip_stream);
/* contrastive loss of the semi-supervised stage (replaces contrastive_loss, /root/reference/train_stcd.py:334-385):
 * pred fp32 [2*numel_half] PROBABILITIES, first half = change prediction of the real pairs (cd), second half = of the
 * pseudo pairs (pse); labels int64 [numel_half] each.  loss = masked MSE(pse, cd) over (cd_label == pse_label) + masked
 * MSE(pse, |cd - 1|) over the rest, each divided by (count + 1e-8); dpred (nullable) = d loss / d pred, both halves. */
int stcd_loss_contrastive(const float* pred, const int64_t* cd_label, const int64_t* pse_label, int64_t numel_half, float* loss_out,
                          float* dpred, void* scratch, void* hip_stream);
/* focal loss (replaces FocalLoss, reference models/losses.py:70-160): x fp32 NCHW [batch, classes, hw], target int64
 * [batch*hw], alpha fp32 [classes] on the device (NULL: ones).  flags bit 0: x are logits and the softmax is fused (apply_nonlin =
 * softmax_helper, dx = d loss / d logits); clear: x are probabilities (dx = d loss / d x).  bit 1: sum instead of mean
 * (size_average=False).  k = one-hot(label) clamped to [smooth/(classes-1), 1-smooth] (no clamp at smooth == 0),
 * pt = sum k p + smooth, loss = -alpha[label] (1-pt)^gamma log pt.  Label 225 counts as class 0 (:136); any other label outside
 * [0, classes) makes the loss and that pixel's gradient NaN.  2 <= classes <= 16.  scratch: >= stcd_loss_scratch_bytes(). */
int stcd_loss_focal(const float* x, const int64_t* target, int batch, int classes, int64_t hw, const float* alpha, float gamma,
                    float smooth, int flags, float* loss_out, float* dx, void* scratch, void* hip_stream);
/* mIoU / min-max IoU (replace mIoULoss :170-206 and mmIoULoss :208-242): p = softmax(logits), t = one-hot(label); per (n, c)
 * iou = sum p t / (sum (p + t - p t) + 1e-8).  mode 0: loss = -mean(weight_c iou) (weight fp32 [classes] on the device, NULL:
 * ones); mode 1: loss = -min(iou) - mean(iou), the min's gradient split evenly among tied entries.  A label outside [0, classes)
 * makes the loss NaN.  2 <= classes <= 16.  scratch: >= stcd_loss_iou_scratch_bytes(batch, classes, hw) bytes (0 for a shape
 * outside the supported range). */
int64_t stcd_loss_iou_scratch_bytes(int batch, int classes, int64_t hw);
int stcd_loss_iou(const float* logits, const int64_t* target, int batch, int classes, int64_t hw, const float* weight, int mode,
                  float* loss_out, float* dlogits, void* scratch, void* hip_stream);
/* ---- metric: replaces SegmentationMetric.genConfusionMatrix (train_pse_cd.py:361-368) without the
 *      per-step .cpu() sync (train_pse_cd.py:231).  cm[2*label+pred] += count; cm is 4 int64 on the device.
 *      pred = argmax over classes (classes==2) or logit > 0 (classes==1, i.e. sigmoid > 0.5). */
int stcd_confusion_update(const float* logits, const int64_t* target, int batch, int classes, int64_t hw,
                          int64_t* cm, void* hip_stream);

/* ---- optimizer: one launch of torch.optim.Adam (decoupled == 0: weight decay added to the gradient) or
 *      torch.optim.AdamW (decoupled != 0) over the flat parameter / gradient buffers, amsgrad off
 *      (replaces optimizer_G.step(): models/trainer.py:46-50,312-314; train_pse_cd.py:431,239).
 *      step = 1-based update count (bias correction); exp_avg / exp_avg_sq: fp32 state, zero-initialised. */
int stcd_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel, int64_t step,
                   double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, void* hip_stream);

/* The same update for a CAPTURED training step (hipGraph): the step-dependent scalars come from device memory, so one captured launch
 * serves every replay.  stcd_adam_hyper fills a HOST array of 8 floats for (step, lr, ...) with exactly the scalars stcd_adam_step
 * forms (the caller keeps it in pinned memory and makes its copy to hyper_dev8 part of the graph); stcd_adam_step_dev reads them. */
int stcd_adam_hyper(int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, float* hyper_host8);
int stcd_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel, const float* hyper_dev8,
                       int decoupled, void* hip_stream);

/* ---- pseudo-change pair synthesis on the device (replaces the file-based assembly of data/dataset.py:468-482 plus
 *      ToTensor/Normalize :499-500 and the paired cutout :24-57; the reference holds NO generator arithmetic, so the
 *      blend below is this library's own specification -- oracle/pseudo_ref.py restates it, parity is unpinned).
 *      img_a, donor: uint8 [B,H,W,3] (HWC, device); mask: uint8 [B,H,W] (>= 1 means building); change: uint8 [B]
 *      (tile is in the change list); alpha: nullable fp32 [B] blend strength (NULL = 1: donor replaces A inside the
 *      mask, as the reference's in-painted file does); erase_xywh: nullable int32 [B,4] cutout rectangle (w == 0: none),
 *      filled with per-pixel uniform values from `seed`, identical in A and B, label 255 there (host mean3/std3).
 *      x1, x2: fp32 [B,3,H,W] normalised; c_label / s_label_a / s_label_b: int64 [B,H,W] (the last two nullable). */
int stcd_pseudo_pair(const uint8_t* img_a, const uint8_t* donor, const uint8_t* mask, const uint8_t* change, const float* alpha,
                     const int32_t* erase_xywh, uint64_t seed, int batch, int height, int width, const float* mean3,
                     const float* std3, float* x1, float* x2, int64_t* c_label, int64_t* s_label_a, int64_t* s_label_b,
                     void* hip_stream);

/* ---- photometric augmentation on the device: counterpart of the host-side PIL/torchvision path of the datasets
 *      (/root/reference/data/dataset.py:488-495 ColorJitter(0.5,0.5,0.5,0.25) w.p. 0.5, RandomGrayscale(0.2), blur() :120-124)
 *      on normalised fp32 NCHW images [n_images,3,H,W] already on the device (e.g. the x1/x2 of stcd_pseudo_pair).
 *      params: device fp32 [n_images][8] = {jitter_on, brightness, contrast, saturation, hue, gray_on, sigma (0: no blur), 0};
 *      torchvision's float functional formulas, fixed order brightness -> contrast -> saturation -> hue, then grayscale, then a
 *      separable Gaussian (radius ceil(3 sigma), replicated edges).  The reference holds no device arithmetic for this:
 *      parity is unpinned beyond the per-op formulas (oracle/pseudo_ref.py restates them; tests pin them to PIL).
 *      out must not alias x; scratch >= stcd_augment_scratch_bytes() bytes. */
int64_t stcd_augment_scratch_bytes(int n_images, int height, int width);
int stcd_augment(const float* x, const float* params, int n_images, int height, int width, const float* mean3, const float* std3,
                 float* out, void* scratch, int64_t scratch_bytes, void* hip_stream);

/* ---- whole-scene inference: tile two co-registered uint8 scenes, run the network on the tiles, put the logits back together.
 *      Three entries that share one regular tile grid: scene height x width, tile edge T, stride S (1 <= S <= T),
 *      tiles_y = max(0, ceil((height - T) / S)) + 1, likewise tiles_x; tile k has ky = k / tiles_x, kx = k % tiles_x and origin
 *      (ky * S, kx * S).  A tile may reach past the bottom / right edge and a scene may be smaller than one tile.  Every entry
 *      works on the tiles [first_tile, first_tile + n_tiles) (n_tiles == 0: nothing is launched); tiles_x / tiles_y must be the
 *      values above.  All indices are 64-bit inside: classes * height * width may pass 2^31. */
/* Replaces the offline 256-pixel crops of split.py:17-46 and the host ToTensor + Normalize of data/dataset.py:499-500.
 * scene_a, scene_b: uint8 [height,width,3] (HWC, device) -> x1, x2: fp32 [n_tiles,3,T,T] normalised, ready for the forward.
 * A tile pixel outside the scene reads the scene by mirror reflection without repeating the edge sample
 * (m = 2*(L-1); i = ((i % m) + m) % m; i = i >= L ? m - i : i; L == 1 -> 0): the reference pads nothing, this is the library's
 * own rule.  Value arithmetic is stcd_pseudo_pair's: (u * (1.f/255.f) - mean[c]) * (1.f/std[c]) (host mean3 / std3). */
int stcd_scene_gather(const uint8_t* scene_a, const uint8_t* scene_b, int height, int width, int tile, int stride, int tiles_x,
                      int first_tile, int n_tiles, const float* mean3, const float* std3, float* x1, float* x2, void* hip_stream);
/* The overlap blend; the reference has none (it scores crops one by one), so this is the library's own specification.
 * logits: fp32 [n_tiles,classes,T,T] (classes 1 or 2) of tiles [first_tile, first_tile + n_tiles) are added into acc fp32
 * [classes,height,width] and wsum fp32 [height,width], both zeroed by the caller before the first call.  window: nullable
 * fp32 [T] (NULL = all ones); pixel weight w = window[ty] * window[tx]; tile pixels outside the scene are dropped.
 * A gather over scene pixels, without float atomics: each pixel adds its covering tiles of this call in ASCENDING tile index,
 * acc = fmaf(w, logit, acc), wsum += w (as one fused multiply-add of the two window factors: the product is not rounded first).  Hence the same inputs give the same bits on every run, and acc / wsum do not depend
 * on how the tiles were split into calls as long as the calls come in ascending first_tile. */
int stcd_scene_stitch(const float* logits, int classes, int height, int width, int tile, int stride, int tiles_x, int tiles_y,
                      int first_tile, int n_tiles, const float* window, float* acc, float* wsum, void* hip_stream);
/* Replaces the arg-max / threshold of models/trainer.py:197-203 and, with a label, SegmentationMetric.genConfusionMatrix
 * (train_pse_cd.py:361-368) on the whole scene.  mask: uint8 [height,width].  classes == 2: acc[1] > acc[0] (a tie is class 0,
 * as torch.argmax takes the first maximum).  classes == 1: acc[0] > threshold * wsum, i.e. the blended raw output above
 * `threshold`: 0 is "sigmoid > 0.5" (stcd_confusion_update, train_pse_cd.py); 0.5 is CDTrainer's n_class == 1 rule on the raw
 * output (trainer.py:200-203) EXCEPT that the reference compares with >= and this entry with >: a value exactly on the
 * threshold is class 0 here.  The mask needs no division; every pixel must have wsum > 0 (true after all tiles were stitched
 * with a positive window).  prob: nullable fp32 [height,width], softmax class 1 (classes == 2) or sigmoid (classes == 1) of
 * acc / wsum.  label: nullable uint8 [height,width] (>= 1 is change, 255 is ignored) together with cm: int64 [4] on the
 * device, cm[2*label+pred] += count as stcd_confusion_update does; both or neither. */
int stcd_scene_finalize(const float* acc, const float* wsum, int classes, int height, int width, float threshold,
                        const uint8_t* label, uint8_t* mask, float* prob, int64_t* cm, void* hip_stream);
/* Test-time augmentation over the eight symmetries of the square, without a host permutation of tiles or logits.
 * d4 in 0..7: bit 0 mirrors columns, bit 1 mirrors rows, bit 2 transposes, the transpose applied last.  For an upright tile
 * X[c,p,q] the view is Xd[c,i,j] = X[c,p,q] with (a,b) = (d4 & 4) ? (j,i) : (i,j), p = (d4 & 2) ? T-1-a : a,
 * q = (d4 & 1) ? T-1-b : b.  Any other d4 is an error reported before any HIP call; d4 == 0 gives the bits of the entries above.
 * The other arguments and their checks are those of stcd_scene_gather / stcd_scene_stitch.
 * gather_d4: x1, x2 = view d4 of the tiles stcd_scene_gather writes, bit-equal to that entry followed by the index permutation
 * (reflection past the edges and the value arithmetic are unchanged).
 * stitch_d4: logits are the network's outputs FOR view d4 of the tiles; the logit of the upright tile pixel (p,q) is read at
 * Ld[c,i,j] with a = (d4 & 2) ? T-1-p : p, b = (d4 & 1) ? T-1-q : q, (i,j) = (d4 & 4) ? (b,a) : (a,b).  The weight is
 * window[p] * window[q] in upright coordinates, and tile order and the chain acc = fmaf(w, logit, acc), wsum += w are those of
 * stcd_scene_stitch: the result is bit-equal to un-transforming the logits and calling that entry.  Views and models are
 * therefore further links of one chain: stitch every view of every model into the same acc / wsum (each view's tiles in
 * ascending order) and stcd_scene_finalize blends the wsum-weighted mean; the bits depend on the order of views and models
 * but not on how a view's tiles were split into calls.  No float atomics. */
int stcd_scene_gather_d4(const uint8_t* scene_a, const uint8_t* scene_b, int height, int width, int tile, int stride, int tiles_x,
                         int first_tile, int n_tiles, const float* mean3, const float* std3, float* x1, float* x2, int d4,
                         void* hip_stream);
int stcd_scene_stitch_d4(const float* logits, int classes, int height, int width, int tile, int stride, int tiles_x, int tiles_y,
                         int first_tile, int n_tiles, const float* window, float* acc, float* wsum, int d4, void* hip_stream);
/* ---- whole scenes for the models the reference's scripts train: UnetSeg (one image in, train_sup.py:303) and SegCD, whose forward
 *      returns (mask_t1, mask_t2, change) (decoders/unet/model.py:316-332).  Grid, views and checks are those of the entries above. */
/* One scene: x fp32 [n_tiles,3,T,T] is bit-equal to the x1 that stcd_scene_gather_d4(scene, scene, ...) writes (same reflection,
 * same value arithmetic, same views) without reading a second scene or writing a second batch. */
int stcd_scene_gather_one_d4(const uint8_t* scene, int height, int width, int tile, int stride, int tiles_x, int first_tile,
                             int n_tiles, const float* mean3, const float* std3, float* x, int d4, void* hip_stream);
/* Several heads of one forward in one launch.  logits: HOST array of n_heads device pointers (1 <= n_heads <= STCD_SCENE_MAX_HEADS;
 * the kernel takes them by value, as stcd_selftrain_score takes its models), each fp32 [n_tiles,classes,T,T], classes 1 or 2.
 * acc: fp32 [n_heads*classes,height,width], head h in planes h*classes ..; ONE wsum fp32 [height,width].  For every head the
 * planes of acc, and wsum, are bit-equal to what stcd_scene_stitch_d4 leaves when called on that head alone with its own acc and
 * wsum: ascending tile order per pixel, the same fmaf chain, upright weights, for all eight views and any split of the tiles
 * into calls.  The covering tiles, the window weight and the read-modify-write of wsum are worked out once per pixel, not once
 * per head; the transposing views stage one head at a time, so LDS does not grow with n_heads.  No float atomics. */
#define STCD_SCENE_MAX_HEADS 3
int stcd_scene_stitch_heads_d4(const float* const* logits, int n_heads, int classes, int height, int width, int tile, int stride,
                               int tiles_x, int tiles_y, int first_tile, int n_tiles, const float* window, float* acc, float* wsum,
                               int d4, void* hip_stream);
/* stcd_scene_finalize for SegCD's three stitched heads in one pass: acc fp32 [3*classes,height,width] in the forward's order
 * (t1, t2, change) over one wsum.  seg_a, seg_b, change: uint8 [height,width], each bit-equal to stcd_scene_finalize on that head
 * (classes == 2: acc[1] > acc[0], a tie is class 0; classes == 1: acc > threshold * wsum with seg_threshold for the two building
 * maps and change_threshold for the change map; NaN is class 0).  gated: nullable uint8 [height,width],
 * change & (seg_a != seg_b): the decision-level gate min(|pred_B - pred_A|, change_prediction) sketched in train_stcd.py:170-176.
 * prob: nullable fp32 [3,height,width], each plane bit-equal to that entry's prob.  label_a, label_b, label_c: each nullable
 * uint8 [height,width] (>= 1 is set, 255 is ignored).  cm: int64 [4][4] on the device, ADDED to; row 0 seg_a vs label_a, row 1
 * seg_b vs label_b, row 2 change vs label_c, row 3 gated vs label_c, each cm[row][2*label+pred]; required iff any label is given.
 * The row of an absent label is left untouched, and so is row 3 when gated is NULL.  Counts are integers, reduced per wave and
 * block before one 64-bit integer atomic per block and counter.  One pass: 3*classes + 1 fp32 planes in, 3 or 4 bytes a pixel out. */
int stcd_scene_finalize_seg(const float* acc, const float* wsum, int classes, int height, int width, float seg_threshold,
                            float change_threshold, const uint8_t* label_a, const uint8_t* label_b, const uint8_t* label_c,
                            uint8_t* seg_a, uint8_t* seg_b, uint8_t* change, uint8_t* gated, float* prob, int64_t* cm,
                            void* hip_stream);

/* ---- the self-training round: K checkpoints of one network score the same pairs.  Replaces, per pair and checkpoint, the sigmoid,
 *      the compare, the .int(), the .cpu() and the host bincount of train_stcd.py:111-125 (reliability split) and :155-177
 *      (pseudo-label writer) by one launch that reads every logit once and writes one byte per pixel.
 * logits: HOST array of n_models device pointers (1 <= n_models <= STCD_SELFTRAIN_MAX_MODELS; the kernel takes them by value),
 * each fp32 [batch,classes,hw]: the raw change output of one checkpoint for the same `batch` pairs; classes 1 or 2.
 * Prediction of model k at a pixel: classes == 1: x > threshold (0 is the reference's "sigmoid > 0.5", the rule of
 * stcd_confusion_update and stcd_scene_finalize; a value exactly on the threshold is class 0); classes == 2: x[1] > x[0] (a tie
 * is class 0, as torch.argmax takes the first maximum).  NaN compares false: class 0.
 * mask: uint8 [batch,hw], the LAST model's prediction: mask_value (1..255) where change, else 0.
 * agree: int64 [batch][n_models-1][4] on the device, agree[b][i][2*last + pred_i] += count over the pixels of pair b: the matrix the
 * reference forms with metric.addBatch(preds[i], preds[-1]) (:120; the later checkpoint plays the label).  NULL iff n_models == 1.
 * label / cm: both or neither; label uint8 [batch,hw] (>= 1 is change, 255 is ignored), cm int64 [4] on the device,
 * cm[2*label + pred_last] += count as stcd_confusion_update does.
 * Counts are integers, reduced per wave and block before one 64-bit atomic per block and cell: every output is a pure function of
 * the inputs.  16-byte loads when hw % 4 == 0 and the pointers allow it, a scalar path otherwise; 64-bit indices inside
 * (batch * classes * hw may pass 2^31).  batch == 0 or hw == 0 launches nothing.  Arguments are checked before any HIP call. */
#define STCD_SELFTRAIN_MAX_MODELS 8
int stcd_selftrain_score(const float* const* logits, int n_models, int batch, int classes, int64_t hw, float threshold,
                         const uint8_t* label, int mask_value, uint8_t* mask, int64_t* agree, int64_t* cm, void* hip_stream);

/* ---- the self-training round on whole scenes: the stitched masks of K checkpoints (stcd_scene_finalize) become a reliability
 *      grid and a cleaned pseudo-label without leaving the device.  All outputs are integers or bytes: pure functions of the
 *      inputs, no float arithmetic, no float atomics, 64-bit indices inside (height * width may pass 2^31).  Arguments are
 *      checked before any HIP call. */
/* Replaces metric.addBatch(preds[i], preds[-1]) per pre-cut crop and checkpoint, train_stcd.py:118-125, by one launch over the
 * scene.  masks: HOST array of n_models device pointers (1 <= n_models <= STCD_SELFTRAIN_MAX_MODELS, taken by value), each uint8
 * [height,width]; any non-zero byte is change; the LAST mask plays the label (preds[-1], :119-122).
 * Cells: cell >= 1, cells_x == ceil(width / cell), cells_y == ceil(height / cell) (anything else is an error); non-overlapping
 * cell x cell squares, c = cy * cells_x + cx; edge cells are cut off at the scene border and counted over their real pixels.
 * agree: int64 [cells][n_models-1][4] on the device, agree[c][i][2*last + pred_i] += count over the pixels of cell c; NULL iff
 * n_models == 1.  label / cm: both or neither; label uint8 [height,width] (>= 1 is change, 255 is ignored), cm int64 [cells][4],
 * cm[c][2*label + pred_last] += count.  n_models == 1 without a label computes nothing: an error.  Counts are ADDED to what the
 * buffers hold, reduced per wave and block before one 64-bit integer atomic per block and counter.  16-byte loads when
 * width % 16 == 0, cell % 16 == 0 and every pointer is 16-byte aligned, a scalar path otherwise.  height == 0 or width == 0
 * launches nothing. */
int stcd_scene_cell_agree(const uint8_t* const* masks, int n_models, int height, int width, int cell, int cells_x, int cells_y,
                          const uint8_t* label, int64_t* agree, int64_t* cm, void* hip_stream);
/* Binary morphological closing with the (2*radius+1)^2 square, dilation then erosion: at radius 2 the
 * cv2.morphologyEx(img, cv2.MORPH_CLOSE, np.ones((5, 5))) of train_stcd.py:186-188.  in: uint8 [height,width], any non-zero byte
 * is set; out: uint8 [height,width], mask_value (1..255) where set, else 0; radius in 1..4.  out must not overlap in.
 * Border rule (OpenCV's default): a pixel outside the scene never contributes -- the dilation reads it as unset, the erosion
 * reads every position outside the scene as set.  One launch: a block stages a 64 x 256 window as bits, runs the four separable
 * passes in LDS and writes its 48 x 240 tile; no alignment is required of in, out or width. */
int stcd_mask_close(const uint8_t* in, int height, int width, int radius, int mask_value, uint8_t* out, void* hip_stream);

/* ---- change objects: connected components of a binary mask, their table and the area / hole filter of the pseudo-label.  No
 *      counterpart in the reference: the cleaning of train_stcd.py:186-188 one level up, from pixels to objects.  Bytes and
 *      integers only: every output is a pure function of the input.  height * width must be below 2^31 (labels are int32);
 *      connectivity is 4 or 8; no alignment is required of a mask or of the width.  Arguments are checked before any HIP call;
 *      height == 0 or width == 0 launches nothing.  Every phase is its own launch: no block ever waits for another block, and
 *      every find / union loop walks strictly decreasing pixel indices under an iteration cap (the pixel count); a thread that
 *      reaches the cap sets the status word, the LAST 4 BYTES of the scratch buffer (zeroed at the start of a call), which
 *      reports a bug and never a property of the input. */
/* Bytes of the scratch buffer of the two entries below (8-byte aligned, a multiple of 4 bytes); 0 for a shape they refuse. */
int64_t stcd_objects_scratch_bytes(int height, int width);
/* labels: int32 [height,width] on the device: 0 is background, 1..n the components of the non-zero (invert == 1: the zero)
 * pixels of mask (uint8 [height,width]), numbered in raster order of each component's first pixel: scipy.ndimage.label's numbering
 * with the cross (4) or the full 3 x 3 structure (8).  count: one int32 on the device, n (it may be the 4 bytes before the
 * status word, so that one 8-byte copy reads both).  Launches: tile pass (a 64 x 64 tile labelled in LDS), seam pass (atomicMin
 * across tile edges), flatten, a three-launch prefix sum over the roots, relabel. */
int stcd_objects_label(const uint8_t* mask, int height, int width, int connectivity, int invert, int32_t* labels, int32_t* count,
                       void* scratch, int64_t scratch_bytes, void* hip_stream);
/* The table of the objects 1..n of a label image (a label outside 1..n is skipped): area int64 [n]; bbox int32 [n,4] =
 * (y0, x0, y1, x1), inclusive; with an overlay (uint8 [height,width], >= 1 is set, 255 is ignored; NULL together with overlap)
 * overlap int64 [n,2] = (pixels of the object that are not ignored, those of them where the overlay is set).  The table is
 * overwritten, not added to; one integer atomic per run of a label within 64 pixels of a row.  n == 0 launches nothing. */
int stcd_objects_table(const int32_t* labels, int height, int width, int n, const uint8_t* overlay, int64_t* area, int32_t* bbox,
                       int64_t* overlap, void* hip_stream);
/* The object filter of a mask in one call with no host read inside.  Step 1: every component of non-zero pixels (connectivity
 * 4 or 8) with area < min_area is cleared.  Step 2, on the result of step 1: every component of unset pixels, taken with the
 * complementary connectivity (4 when objects use 8 and the reverse), of area <= max_hole that touches no scene border is set.
 * min_area <= 1 skips step 1, max_hole == 0 skips step 2 (both: out is the binarised input); max_hole < 0 is an error.
 * out: uint8 [height,width], mask_value (1..255) where set, else 0; it must not overlap in, and neither may overlap scratch. */
int stcd_mask_filter_objects(const uint8_t* in, int height, int width, int connectivity, int64_t min_area, int64_t max_hole,
                             int mask_value, uint8_t* out, void* scratch, int64_t scratch_bytes, void* hip_stream);

/* ---- change polygons: the boundary rings of the objects of a label image (labels int32 [height,width]: <= 0 is background, as
 *      stcd_objects_label numbers them or any other labelling).  tests/rings_spec.py states every output.  Lattice: vertex (y, x)
 *      with 0 <= y <= height, 0 <= x <= width; pixel (i, j) is the unit square between (i, j) and (i + 1, j + 1) and owns one
 *      directed unit edge per side whose neighbour carries another label: top east, right south, bottom west, left north, so an
 *      outer ring runs (i,j), (i,j+1), (i+1,j+1), (i+1,j).  The successor of an edge is the edge of the same label that leaves its
 *      head; where two diagonal pixels of a label meet (the other two carrying other labels) the ring crosses to the other pixel
 *      under connectivity 8 and stays with its own pixel under connectivity 4.  The cycles of that map are the rings; only their
 *      corners are kept (the tails of the edges whose predecessor has another direction), in travel order from the ring's smallest
 *      edge in (tail y, tail x, direction) order; rings are ordered by that edge, i.e. in raster order of their first vertex.
 *      Two phases with one host read between them: the count entry leaves R (rings), V (vertices) and a status word on the device;
 *      the caller reads them, allocates, and hands R and V to the write entry.  The scratch buffer carries the state from the one
 *      to the other.  Integers only, every output a pure function of the input; neither entry allocates, copies to the host or
 *      synchronises; height * width must be below 2^31 and connectivity be 4 or 8; height == 0 or width == 0 launches nothing.
 *      No thread walks a ring: corners are found from the 2 x 2 pixels round a vertex, numbered by a three-launch prefix sum, linked
 *      to the next corner along the straight run (at most max(height, width) unit steps, under an iteration cap), and the ring's
 *      first corner and every corner's rank come from pointer jumping, one launch per round.
 *      max_corners (below 2^31) is the capacity of the per-corner part of the scratch buffer: R cannot be known before the rings
 *      are ranked, so the caller sizes that part before V is known.  If V exceeds it the count entry still writes the exact V, sets
 *      status bit 4 and computes nothing else; the caller repeats the call with max_corners >= V.
 *      Status word: 0, or bits 1 / 2: an iteration cap or an impossible link (a bug, never a property of the input), 4: V is above
 *      max_corners, 8 (write entry, in the scratch header only): R / V are not what the count phase left. ---- */
/* Bytes of the scratch buffer of the two entries below (8-byte aligned): 32 + 4 per lattice vertex ((height + 1) * (width + 1), about
 * 4 per pixel) + 8 per 4096 vertices + 37 per corner of capacity (+ 16 per 4096 of them); 0 for arguments they refuse. */
int64_t stcd_rings_scratch_bytes(int height, int width, int64_t max_corners);
/* counts: int64 [3] on the device = (R, V, status).  Launches: the three-launch prefix sum over the corners, the links,
 * ceil(log2 max_corners) pointer-jumping rounds (a round past ceil(log2 V) returns at once), the count of the ring starts. */
int stcd_rings_count(const int32_t* labels, int height, int width, int connectivity, int64_t max_corners, int64_t* counts, void* scratch,
                     int64_t scratch_bytes, void* hip_stream);
/* After stcd_rings_count on the same labels, shape, connectivity, max_corners and scratch, with the R and V it left:
 * vertices int32 [V,2] = (y, x), the first vertex of a ring not repeated; offsets int64 [R+1], ring r is vertices[offsets[r] ..
 * offsets[r+1]); object int32 [R], the ring's label; area2 int64 [R] = sum over consecutive vertices of x_t * y_h - x_h * y_t, twice
 * the area: positive for an outer ring, negative for a hole (one 64-bit integer atomic per run of a ring within 64 consecutive
 * corners).  Refused before any launch: n_vertices above max_corners, or an (n_rings, n_vertices) pair no count phase can leave
 * (negative, n_vertices odd or below 4 * n_rings, one of them 0 alone).  A pair that passes those checks but is not the one in
 * the scratch header is found on the device: nothing is written and bit 8 of the header's status word (scratch byte 20) is set.
 * n_rings == 0 writes offsets[0] = 0 alone. */
int stcd_rings_write(const int32_t* labels, int height, int width, int connectivity, int64_t max_corners, int64_t n_rings, int64_t n_vertices,
                     int32_t* vertices, int64_t* offsets, int32_t* object, int64_t* area2, void* scratch, int64_t scratch_bytes, void* hip_stream);

/* ---- ring simplification: Douglas-Peucker over rings in the layout above (vertices int32 [V,2] = (y, x), offsets int64 [R+1]),
 *      on the device, with exact integer arithmetic.  tests/simplify_spec.py states every output.  The tolerance travels as
 *      q = floor(4 * tolerance^2), 0 <= q < 2^31 (tolerances 1.0, 1.5, 2.0: q = 4, 9, 16); coordinates must lie in [0, 16384], so
 *      that every key below is at most 2^58.  For one ring P[0..n-1], P[n] = P[0]:
 *        1. key(p, a, b) = d^2 * L', d the distance of p from the SEGMENT (a, b), L = |b - a|^2, L' = L or 1 when L == 0: with
 *           e = p - a, d = b - a, t = e.d:  t <= 0: |p - a|^2 * L;  t >= L: |p - b|^2 * L;  else cross(e, d)^2;  L == 0: |p - a|^2.
 *        2. anchors: vertex 0 and the vertex a1 of largest |P - P[0]|^2 (lowest index on ties); chains [0, a1] and [a1, n].
 *        3. on a chain [i, j] with j - i >= 2 the interior vertex k of largest key against (P[i], P[j]), lowest index on ties, is
 *           kept if 4 * key > q * L', and [i, k] and [k, j] are treated the same way; otherwise every interior vertex is dropped.
 *        4. if nothing but the anchors was kept, the vertex of largest key against (P[0], P[a1]) among all others (lowest index on
 *           ties) is kept too, whatever its key: at least a triangle.
 *        5. area2 (the formula of stcd_rings_write) of the kept vertices is 0, or differs in sign from that of the input ring as
 *           recomputed from its vertices: the ring is copied whole.  So a hole stays a hole and an outer ring an outer ring.  Rings
 *           of fewer than 4 vertices are copied whole.
 *      The result keeps the ring count and order, every ring a subsequence of its input in travel order with the first vertex still
 *      first; q == 0 drops only vertices that lie on the segment between their kept neighbours (none on a traced ring).  Topology
 *      is NOT protected: a simplified hole may touch or cross its exterior and two objects' polygons may overlap by up to the
 *      tolerance; stcd_rings_safe_begin / _round / _write below repair that and stcd_rings_conflicts reports it.
 *      Every ring iterates the levels of step 3 inside one kernel (a wavefront per ring up to 64 vertices, a block per longer
 *      ring, its state in LDS up to 2048 vertices and in the scratch buffer above): no launch and no host read per level, no
 *      thread walks a chain.  Two phases with one host read between them, as for the rings; the scratch buffer carries the state.
 *      Neither entry allocates, copies to the host or synchronises.
 *      Status word: 0, or bits 1: a coordinate outside [0, 16384], 2: a ring reached the round cap of n (a bug, never a property
 *      of the input), 4: offsets that do not start at 0, do not ascend or do not end at n_vertices (nothing of such a ring is read),
 *      8 (write entry, in the scratch header only, scratch byte 24): n_out is not what the count phase left. ---- */
/* Bytes of the scratch buffer of the two entries below (8-byte aligned): 48 + 29 per vertex + 12 per ring + 8 per 4096 vertices; 0
 * for arguments they refuse (negative, or 2^31 and above). */
int64_t stcd_rings_simplify_scratch_bytes(int64_t n_rings, int64_t n_vertices);
/* counts: int64 [2] on the device = (V', status): the vertices that remain.  Refused before any launch: null pointers, negative
 * counts or counts of 2^31 and above, q outside [0, 2^31), misaligned pointers (8 bytes), a scratch buffer that is too small. */
int stcd_rings_simplify_count(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t q,
                              int64_t* counts, void* scratch, int64_t scratch_bytes, void* hip_stream);
/* After stcd_rings_simplify_count on the same rings and scratch, with the V' it left as n_out: out_vertices int32 [n_out,2],
 * out_offsets int64 [R+1], out_area2 int64 [R], recomputed from the vertices that remain.  Refused before any launch: what the
 * count entry refuses, n_out < 0 and n_out > n_vertices.  An n_out that passes those checks but is not the count phase's own (or a
 * count phase that left a status, or other ring sizes) is found on the device: nothing is written and bit 8 is set. */
int stcd_rings_simplify_write(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t q, int64_t n_out,
                              int32_t* out_vertices, int64_t* out_offsets, int64_t* out_area2, void* scratch, int64_t scratch_bytes,
                              void* hip_stream);

/* ---- topology of ring sets: which edges conflict, and Douglas-Peucker with its topology repaired; rings in the layout above
 *      (vertices int32 [V,2] = (y, x) in [0, 16384], offsets int64 [R+1]), on the device, with exact integer arithmetic.
 *      tests/topology_spec.py states every output.  Edge k of ring r with n vertices runs from P[k] to P[(k+1) % n] and has the
 *      global index offsets[r] + k.  orient(a, b, c) = (b.y - a.y)(c.x - a.x) - (b.x - a.x)(c.y - a.y), below 2^30 in magnitude.
 *      CONFLICT of two distinct edges (a, b), (c, d), of one ring or of two:
 *        1. a zero-length edge conflicts with nothing.
 *        2. all four orientations 0 (collinear): iff their overlap along the axis in which a and b differ has positive length.
 *        3. otherwise no endpoint value may be common to both (a != c, a != d, b != c, b != d) and the closed segments must share a
 *           point: both orientation sign products negative, or one orientation 0 and that point in the other edge's bounding box.
 *      So proper crossings, a vertex inside another edge, collinear overlaps and spikes conflict; contact at a vertex of both does
 *      not (consecutive edges, pinch corners), and the rings of stcd_rings_write have no conflict.  Known limit: a crossing exactly
 *      through a vertex that both rings share is not seen.
 *      POCKET HIT: a current edge from kept vertex i to the next kept vertex j (j = n for the edge that closes the ring; vertex 0 is
 *      always kept) with j - i >= 2 has the pocket P[i], ..., P[j % n], a closed polygon; the edge is hit iff the first vertex p of
 *      any OTHER ring lies on one of the pocket's sides (orientation 0 and within the side's bounding box) or inside: the sides
 *      (u, v), taken with u.y < v.y, with u.y <= p.y < v.y (the half-open row rule of stcd_rings_raster) and
 *      (v.x - u.x)(p.y - u.y) > (p.x - u.x)(v.y - u.y) are odd in number.
 *      TOPOLOGY-SAFE SIMPLIFICATION at q:
 *        1. round 0 is stcd_rings_simplify_count (rules 1 to 5 there): a keep mask over the input vertices.
 *        2. a round flags every current edge that conflicts with another current edge or whose pocket is hit.
 *        3. every flagged edge with dropped vertices restores the vertex of largest key (rule 1 of the simplification) against
 *           (P[i], P[j % n]) among i+1 .. j-1, lowest index on ties: the one Douglas-Peucker would split at next.  All at once.
 *        4. every ring whose mask changed: kept area2 0 or of another sign than the input's -> all of its vertices are kept.
 *        5. repeat from 2 until a round restores nothing.  Masks only grow, so this ends; at the end a flagged edge is an input
 *           edge, so conflict-free input gives a conflict-free result in which every ring winds round every other ring's first
 *           vertex as often, mod 2, as in the input.  Input that conflicts already still ends; what is left is counted.
 *      Candidate pairs come from a uniform grid of cell x cell pixels, cell a power of two from 8 to 256 (0: 16): every edge is
 *      entered into the cells its segment passes through (a walk over the cell rows it spans with exact floor / ceiling columns per
 *      row, not the cells of its bounding box) by count, prefix sum and fill; one block per non-empty cell stages the cell's edges
 *      in LDS in tiles of 256 and every lane tests its own edge against the tile and sets its own flag with a plain byte store (no
 *      atomics, no pair list; a pair that shares several cells is tested in each).  No output depends on cell.  The first vertices
 *      of all rings lie in the same grid; a wavefront per current edge with dropped vertices takes the box of its chain, the points
 *      in the grid rows of that box and runs on-or-inside with its lanes striding over the chain, and another one the arg-max of
 *      the restore.  No thread walks a ring.  No entry allocates, synchronises or copies to the host; all run on hip_stream.
 *      counts: int64 [8] on the device = (status, current edges, grid entries, vertices restored by this call, conflicting edges,
 *      pocket hits, 0, 0); the last two of the named ones are -1 where the status is set.  Status word: 0, or bits 1: a coordinate
 *      outside [0, 16384], 2: a ring reached its round cap in round 0 (a bug, never a property of the input), 4: offsets that do not
 *      start at 0, do not ascend or do not end at n_vertices, 8: n_edges / n_out is not the device's own count, 16: the grid has more
 *      entries than max_entries (counts[2] says how many; nothing was flagged or restored).  With a status set the kernels that
 *      follow do nothing.  Bits 8 and 16 are those of one call, the others stay. ---- */
/* Bytes of the scratch buffer of the entries below (8-byte aligned): 64 + 26 per vertex + 24 per ring + 8 per cell of the grid
 * ((16384 / cell + 1)^2 of them) + the scan's 8 per 4096 of the larger of the two + stcd_rings_simplify_scratch_bytes; 0 for arguments
 * they refuse. */
int64_t stcd_rings_topo_scratch_bytes(int64_t n_rings, int64_t n_vertices, int cell);
/* flags uint8 [n_vertices]: 1 where the edge that starts at that vertex conflicts with any other edge of the ring set, else 0;
 * counts as above (current edges = n_vertices).  entries: int32 [max_entries], the grid's (cell, edge) entries; 4 * n_vertices + 4096
 * is enough for traced rings.  Refused before any launch: null pointers, negative counts or counts of 2^31 and above, a cell that is
 * not 0 or a power of two from 8 to 256, max_entries outside [0, 2^31), misaligned pointers (8 bytes, entries 4), a scratch buffer
 * that is too small.  n_vertices == 0 launches the validation and the counts alone.  Otherwise 11 kernel launches and 3 memsets whatever
 * the data: validation, the ring of every vertex, the edges, the grid (count, 3 of the scan, fill), the pairs, the tally, the counts. */
int stcd_rings_conflicts(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int cell, uint8_t* flags,
                         int64_t* counts, int32_t* entries, int64_t max_entries, void* scratch, int64_t scratch_bytes, void* hip_stream);
/* Round 0 of the safe simplification: stcd_rings_simplify_count on a part of the scratch buffer, then the ring of every vertex, the
 * input areas and the grid of first vertices.  counts[1] is the number of kept vertices, which is the number of current edges.
 * Refused before any launch: as above, and q outside [0, 2^31).  The launches of stcd_rings_simplify_count, then 10 kernel launches, 4
 * memsets and one device-to-device copy of 8 bytes per ring. */
int stcd_rings_safe_begin(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t q, int cell,
                          int64_t* counts, void* scratch, int64_t scratch_bytes, void* hip_stream);
/* One round after stcd_rings_safe_begin on the same rings, cell and scratch: the detection pass (rule 2) over the n_edges current
 * edges and, with restore != 0, rules 3 and 4.  n_edges is counts[1] of the begin entry plus every counts[3] since (bit 8 if not).
 * counts[3] == 0 ends the loop; counts[4] is then the number of conflicting edges of the result.  With restore == 0 nothing changes:
 * the pass a round cap ends with.  After bit 16 the same call is repeated with max_entries >= counts[2].  Refused before any launch:
 * as stcd_rings_conflicts, and n_edges outside [0, n_vertices].  15 kernel launches and 3 memsets per round whatever the data, 3 launches
 * more with restore != 0. */
int stcd_rings_safe_round(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int cell, int64_t n_edges,
                          int restore, int64_t* counts, int32_t* entries, int64_t max_entries, void* scratch, int64_t scratch_bytes,
                          void* hip_stream);
/* After a round that restored nothing (or ran with restore == 0), with its n_edges as n_out: out_vertices int32 [n_out,2],
 * out_offsets int64 [R+1], out_area2 int64 [R] of the kept vertices.  Refused before any launch: as the begin entry, n_out outside
 * [0, n_vertices], null or misaligned outputs.  An n_out that is not the device's own is found there: nothing is written, bit 8. */
int stcd_rings_safe_write(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int cell, int64_t n_out,
                          int32_t* out_vertices, int64_t* out_offsets, int64_t* out_area2, int64_t* counts, void* scratch,
                          int64_t scratch_bytes, void* hip_stream);

/* ---- convex hulls and oriented boxes: rings in the layout above (vertices int32 [V,2] = (y, x) in [0, 16384], offsets int64 [R+1]),
 *      on the device, with exact integer arithmetic.  tests/hull_spec.py states every output.
 *      Hull of one ring P[0..n-1]:
 *        1. a coordinate that occurs more than once counts at its lowest index only.
 *        2. the hull ring is the subsequence of P, in input order, of the STRICT extreme points of the convex hull of the point set
 *           (a point collinear with its hull neighbours is not one); it starts at the hull vertex of lowest input index.
 *        3. area2 (the formula of stcd_rings_write) is recomputed from the kept vertices; ring count and order are unchanged.
 *        4. 0, 1 or 2 distinct points, or points all on one line, give 0, 1 or 2 vertices and area2 0.
 *      Found by QuickHull over index intervals: the anchors are the lexicographic minimum and maximum of (x, y), the two chains
 *      between them are intervals in travel order, on a chain the vertex strictly outside the chord with the largest |cross|
 *      (below 2^30; the first in travel order on ties) is kept and the chain splits there; "outside" is decided by the sign of the
 *      ring's own area2 as recomputed from its vertices.  That equals rules 1 to 4 on every ring that does not cross itself (the
 *      rings of stcd_rings_write, pinches included).  On a ring that crosses itself, or repeats a hull vertex, the entries end, stay
 *      in bounds and return a subsequence that holds the two anchors; which other vertices it holds is unspecified.
 *      Every ring iterates its levels inside one kernel (a wavefront per ring up to 64 vertices, a block per longer ring, its state
 *      in LDS up to 2048 vertices and in the scratch buffer above): no launch and no host read per level.  Two phases with one host
 *      read between them, as for the simplification; the scratch buffer carries the state.  Neither entry allocates, copies to the
 *      host or synchronises.
 *      Status word: 0, or bits 1: a coordinate outside [0, 16384], 2: a ring reached the round cap of n (a bug, never a property
 *      of the input), 4: offsets that do not start at 0, do not ascend or do not end at n_vertices (nothing of such a ring is read),
 *      8 (write entry, in the scratch header only, scratch byte 24): n_out is not what the count phase left.
 *      Oriented box of one hull H[0..h-1] (stcd_rings_boxes):
 *        5. h < 3: edge -1 and zeros.
 *        6. for edge i from H[i] to H[(i + 1) % h]: e = (ey, ex), L = ey^2 + ex^2; for every j: d_j = (H[j] - H[i]) . e and
 *           z_j = ex (y_j - y_i) - ey (x_j - x_i).  W = max d - min d; Z = max z if max z >= -min z, else min z (on a convex hull
 *           all z_j have one sign).  The box on edge i has area W |Z| / L.  An edge with L == 0 (no hull has one) is passed over.
 *        7. the chosen edge has the smallest area, compared exactly in 128 bits (W_i |Z_i| L_b < W_b |Z_b| L_i; the products stay
 *           below 2^90), the lowest i on ties; no edge with L > 0: edge -1 and zeros.
 *        8. the box: origin H[i], dir e, extent (min d, max d, Z).  With n = (ex, -ey) a point H[i] + a e + b n has d = a L and
 *           z = b L: the corners are (a, b) = (dmin / L, 0), (dmax / L, 0), (dmax / L, Z / L), (dmin / L, Z / L).
 *      One launch: a wavefront per hull of up to 64 vertices, the block for each longer one (in LDS up to 1024 vertices), a lane
 *      per edge over all vertices, O(h^2) per hull by design: hulls of digital shapes are short. ---- */
/* Bytes of the scratch buffer of the two hull entries (8-byte aligned): 48 + 25 per vertex + 12 per ring + 8 per 4096 vertices; 0
 * for arguments they refuse (negative, or 2^31 and above). */
int64_t stcd_rings_hull_scratch_bytes(int64_t n_rings, int64_t n_vertices);
/* counts: int64 [2] on the device = (V', status): the hull vertices.  Refused before any launch: null pointers, negative counts or
 * counts of 2^31 and above, misaligned pointers (8 bytes), a scratch buffer that is too small. */
int stcd_rings_hull_count(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t* counts, void* scratch,
                          int64_t scratch_bytes, void* hip_stream);
/* After stcd_rings_hull_count on the same rings and scratch, with the V' it left as n_out: out_vertices int32 [n_out,2], out_offsets
 * int64 [R+1], out_area2 int64 [R].  Refused before any launch: what the count entry refuses, n_out < 0 and n_out > n_vertices.  An
 * n_out that passes those checks but is not the count phase's own (or a count phase that left a status, or other ring sizes) is
 * found on the device: nothing is written and bit 8 is set. */
int stcd_rings_hull_write(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int64_t n_out,
                          int32_t* out_vertices, int64_t* out_offsets, int64_t* out_area2, void* scratch, int64_t scratch_bytes, void* hip_stream);
/* out_edge int32 [R], out_origin int32 [R,2] = (y, x), out_dir int32 [R,2] = (ey, ex), out_extent int64 [R,3] = (dmin, dmax, Z), all
 * on the device; status: one int32 on the device, cleared by the entry, then 0 or bits 1 and 4 as above (bit 1: the coordinate is
 * clamped; bit 4: the ring gets edge -1); where it is set the boxes are not valid.  The rules ask for no convexity: any rings in the layout above are taken.  Refused before any launch:
 * null pointers, negative counts or counts of 2^31 and above, misaligned pointers.  Needs no scratch buffer, allocates nothing and
 * reads nothing back. */
int stcd_rings_boxes(const int32_t* hull_vertices, const int64_t* hull_offsets, int64_t n_rings, int64_t n_vertices, int32_t* out_edge,
                     int32_t* out_origin, int32_t* out_dir, int64_t* out_extent, int32_t* status, void* hip_stream);

/* ---- ring rasterization: rings in the layout above (vertices int32 [V,2] = (y, x) lattice corners in [0, 16384], offsets int64
 *      [R+1], ring r closed implicitly: edges from vertex k to vertex k + 1 mod n) back to a uint8 mask of height x width pixels at
 *      the origin, 1 <= height, width <= 16384, on the device, with exact integer arithmetic.  tests/raster_spec.py states every
 *      output.  Pixel (i, j) is the unit square between (i, j) and (i + 1, j + 1), sampled at its centre (i + 1/2, j + 1/2).
 *        1. an edge with y0 == y1 contributes nothing.  Another edge is taken with y0 < y1, dy = y1 - y0, and sign s = +1 if it ran
 *           north as stored (y1 < y0 before the swap), else -1.  It touches row i iff y0 <= i < y1 and 0 <= i < height: a row's
 *           centre line never passes through a lattice vertex, so there are no vertex cases.
 *        2. in row i it toggles column j* = floor((num + dy - 1) / (2 dy)), num = 2 x0 dy + (x1 - x0) (2 i + 1 - 2 y0) (twice dy
 *           times the x of the crossing, 0 <= num <= 2^29): the first j with j + 1/2 >= crossing, so a centre ON an edge counts as
 *           right of it; j* is clamped to [0, width], and column `width` is outside the frame.  delta[i][j*] += s.
 *        3. the winding number w[i][j] is the sum of delta[i][0..j]: for the rings of stcd_rings_write (outer ring area2 > 0, hole
 *           < 0) it is 1 inside an object and 0 elsewhere.
 *        4. rule 0 (positive): a pixel is set iff w > 0, the union of overlapping polygons with holes subtracted; rule 1 (evenodd):
 *           iff w is odd, for foreign rings whose orientation means nothing.
 *      So parts of a ring beyond the frame are clipped exactly, a ring of fewer than 3 vertices or one that runs out and back along
 *      a line cancels itself, and two polygons that share an edge partition the pixels along it.
 *      One clear (hipMemsetAsync of the scratch buffer, on every call) and two kernels on the caller's stream; the entry neither
 *      allocates nor reads anything back.  k_raster_edges: a thread per edge finds its ring by binary search in offsets, clips the
 *      row span to [0, height) before any loop and adds s with a 32-bit integer atomic that returns nothing; a lane walks its own
 *      edge up to 32 rows, longer edges are collected per wavefront and its 64 lanes stride over the rows of each; no thread walks a
 *      ring.  k_raster_scan: a wavefront per row sums delta in chunks of 1024 columns with a carried sum, applies the rule, writes
 *      the mask (16-byte stores when width % 16 == 0 and mask / overlay are 16-byte aligned, bytes otherwise) and counts cm.
 *      Integer atomics are order-free: every output is a pure function of the input.
 *      Status word, the FIRST 4 bytes of the scratch buffer: 0, or bits 1: a coordinate outside [0, 16384] (the edge is skipped),
 *      4: offsets that do not start at 0, do not ascend or do not end at n_vertices (nothing of such a ring is read).  Where it is
 *      set the mask contents are unspecified. ---- */
/* Bytes of the scratch buffer of the entry below (8-byte aligned): 16 (the header) + 4 * height * (width + 1) (the delta plane,
 * int32 [height][width + 1]), rounded up to a multiple of 8; 0 for a height or width outside [1, 16384]. */
int64_t stcd_rings_raster_scratch_bytes(int height, int width);
/* mask: uint8 [height,width] on the device, mask_value (1..255) where set, else 0.  overlay / cm: both or neither; overlay uint8
 * [height,width] (>= 1 is set, 255 is ignored), cm int64 [4] on the device, cm[2 * overlay_set + raster_set] += count over the
 * pixels that are not ignored: counts are ADDED to what cm holds, reduced per wave and block before one 64-bit integer atomic per
 * block and counter.  Refused before any HIP call: null pointers (overlay and cm aside, and vertices when n_vertices == 0), overlay without cm or cm without overlay,
 * negative counts or counts of 2^31 and above, height / width outside [1, 16384], a rule other than 0 / 1, mask_value outside
 * [1, 255], vertices / offsets / cm / scratch not 8-byte aligned, a scratch buffer that is too small.  n_rings == 0 or
 * n_vertices == 0 writes an all-zero mask (and still counts cm).  mask and cm must not overlap scratch. */
int stcd_rings_raster(const int32_t* vertices, const int64_t* offsets, int64_t n_rings, int64_t n_vertices, int height, int width,
                      int rule, int mask_value, const uint8_t* overlay, int64_t* cm, uint8_t* mask, void* scratch, int64_t scratch_bytes,
                      void* hip_stream);

/* ---- distance transform: the exact squared Euclidean distance transform of a uint8 mask [height,width], 1 <= height, width <=
 *      16384, on the device, and what is read off it: the int32 plane (scipy.ndimage.distance_transform_edt, squared and exact),
 *      the disc buffers (scipy.ndimage.binary_dilation / binary_erosion with a disc of any radius; the square window of
 *      stcd_mask_close stays what it is) and the boundary match of two masks (boundary precision / recall at a pixel tolerance and
 *      the Hausdorff distance, today .cpu() plus scipy).  tests/edt_spec.py states every output; all quantities are integers.
 *        - A pixel is set iff its byte is non-zero.  Pixel (i, j) is a lattice point; the squared distance of two pixels is
 *          (i - i')^2 + (j - j')^2.
 *        - d2[i][j] is the minimum squared distance from (i, j) to a SEED pixel inside the frame, 0 on a seed.  With no seed in the
 *          frame every value is NO_SEED = 2^30; the largest real value is 2 * 16383^2 < 2^30.  Nothing outside the frame is a
 *          seed.  Only the distance is returned, never the nearest pixel: ties between seeds do not matter.
 *        - seeds: 0 (unset) the zero pixels, scipy's convention; 1 (set) the object pixels; 2 (boundary) the boundary pixels.
 *        - boundary: an optional plane `ignore` marks VOID pixels, byte 255 (the label's "ignored" byte).  p is a boundary pixel
 *          of mask M iff p is set in M, p is not void, and at least one 4-neighbour of p inside the frame is unset in M and not
 *          void.  So the frame edge is no boundary, a void pixel is never a boundary pixel and never makes its neighbour one: a tile
 *          cut from a scene and a label with an ignored margin grow no false outlines.
 *        - buffer: q = floor(radius^2), computed once on the host.  Dilation by the disc sets p iff d2_set[p] <= q; erosion keeps p
 *          iff d2_unset[p] > q, and does not eat in from the frame edge.  Closing is dilate then erode, opening erode then dilate:
 *          close >= mask >= open as sets, radius 0 is the identity.
 *        - boundary match of pred against label, the label's byte 255 void for both masks; up to 8 tolerances t as q_t =
 *          floor(t^2).  Bp, Bl: the two boundary sets.  counts[s] = (n, max_d2, within[0..T-1]) for side 0 (Bp measured against
 *          Bl) and side 1 (Bl against Bp): n the boundary pixels of that side, max_d2 the largest d2 among them to the other
 *          side's boundary (0 if n == 0, NO_SEED if the other side is empty and n > 0), within[t] how many have d2 <= q_t.
 *          precision_t = within0[t] / n0, recall_t = within1[t] / n1, hausdorff2 = max of the two max_d2, on the host.
 *      Separable: a column pass leaves g, the distance along the column to its nearest seed, as uint16; the row pass takes
 *      min_k (j - k)^2 + g[i][k]^2.  Four launches per transform on the caller's stream, whatever the data: k_edt_col_seeds (a thread
 *      per chunk of 64 rows and 4 columns evaluates the seed predicate in its loader and tables the chunk's first and last seed
 *      row), k_edt_col_carry (a thread per column carries them across the chunks), k_edt_col_dist (the loader again, g from the
 *      chunk's 64 seed bits and the table), k_edt_row (a block per row; the cost is Monge, so the leftmost argmin is monotone: the
 *      middle column first, then the middles of the halves within the argmins of their neighbours, log2 levels inside the kernel
 *      with the row resident in LDS; O(W log W) per row, independent of the data).  The epilogue of the row pass is chosen by the
 *      entry: the plane, the threshold, or the match counts.  No entry allocates, reads anything back or synchronises; there is no
 *      atomic on the d2 path, and the match counts meet in integer atomics: every output is a pure function of the input. ---- */
/* Bytes of the scratch buffer of the three entries below (16-byte aligned): 2 per pixel of the frame with its width rounded up to
 * 4 (g), rounded up to 16, plus 4 per column of that width and chunk of 64 rows (the table); 0 for a height or width outside
 * [1, 16384]. */
int64_t stcd_edt_scratch_bytes(int height, int width);
/* d2: int32 [height,width] on the device.  ignore: NULL, or with seeds == 2 a uint8 [height,width] plane whose byte 255 is void.
 * Refused before any HIP call: null pointers, a shape outside [1, 16384], seeds outside 0..2, an ignore plane with seeds 0 or 1,
 * d2 not 4-byte or scratch not 16-byte aligned, a scratch buffer that is too small.  16-byte stores when width % 4 == 0 and d2 is
 * 16-byte aligned; mask rows are read as 32-bit words when width % 4 == 0 and the planes are 4-byte aligned, as bytes otherwise. */
int stcd_edt(const uint8_t* mask, const uint8_t* ignore, int height, int width, int seeds, int32_t* d2, void* scratch, int64_t scratch_bytes,
             void* hip_stream);
/* One half of an opening or closing, no d2 plane written: out [height,width] = mask_value (1..255) where d2 <= q (keep_above == 0:
 * with seeds == 1 the dilation) or where d2 > q (keep_above == 1: with seeds == 0 the erosion), else 0; q >= 0.  out must not
 * overlap mask, and neither may overlap scratch.  Refusals as above. */
int stcd_mask_buffer(const uint8_t* mask, int height, int width, int seeds, int q, int keep_above, int mask_value, uint8_t* out, void* scratch,
                     int64_t scratch_bytes, void* hip_stream);
/* counts: int64 [2][2 + n_q] on the device as defined above, cleared by the entry itself (one hipMemsetAsync).  q: n_q (0..8)
 * integers >= 0 on the HOST, copied into the kernel arguments.  Two transforms, no d2 plane: each row pass measures the boundary
 * pixels of the other mask in its epilogue, reduced per wave and block before one 64-bit integer atomic per block and counter.
 * Refused before any HIP call: null pointers, a shape outside [1, 16384], n_q outside [0, 8], a negative q, counts not 8-byte or
 * scratch not 16-byte aligned, a scratch buffer that is too small. */
int stcd_boundary_match(const uint8_t* pred, const uint8_t* label, int height, int width, const int32_t* q, int n_q, int64_t* counts,
                        void* scratch, int64_t scratch_bytes, void* hip_stream);

/* ---- nearest-seed (feature) transform: the distance transform above with the seed it found, what
 *      scipy.ndimage.distance_transform_edt(return_indices=True) gives as a linear index, and what is read off it: Voronoi growth of
 *      a label plane (skimage.segmentation.expand_labels) and the distance-transform split of merged objects.
 *      tests/nearest_spec.py states every output; all quantities are integers.  Seeds, modes and the ignore plane are stcd_edt's.
 *        - index[i][j] = y * width + x of the seed (y, x) that minimises (i - y)^2 + (j - x)^2; among equal distances the smallest
 *          column x wins, then the smallest row y.  A seed's nearest seed is itself.  With no seed in the frame every index is -1
 *          (and d2 NO_SEED).  height * width <= 2^28, so the index fits int32.  d2, where asked for, is stcd_edt's to the bit.
 *        - gather: out[p] = values[index[p]] where d2[p] <= q, else 0.  With mask = (labels != 0), values = labels and q =
 *          floor(distance^2) that is expand_labels(labels, distance) under the tie rule above; q = 0 returns the labels.
 *        - split (stcd_objects_split_cut), from mask M, its components L0 (`labels`), the components Lc of a core mask
 *          (`core_labels`: M eroded by a disc, small cores dropped) and index, the nearest-seed transform of the core mask, mode 1:
 *          owner[p] = Lc[index[p]] if p is set in M, index[p] >= 0 and L0[index[p]] == L0[p], else 0.  A set pixel with owner 0 is
 *          an ORPHAN: its nearest core belongs to another component, or there is no core.  A set pixel p is CUT (out byte 0) iff
 *          owner[p] != 0 and one of its neighbours right, down-left, down, down-right inside the frame has a non-zero owner other
 *          than owner[p]; every other set pixel becomes mask_value, every unset pixel 0.  Of two 8-adjacent pixels with different
 *          owners the earlier in raster order is cut, so a component of out (4- or 8-connected) holds two owners only where
 *          orphans join them.  Orphans never cut and are never cut.
 *      The tie rule is the one the kernels imply: the row pass takes the leftmost argmin column, and along a column the seed above
 *      wins a tie with the seed below.  The column pass's third launch, k_edt_col_near, writes g with bit 15 set where the column's
 *      nearer seed is strictly below (g <= 16383 leaves the bit free; 0xFFFF stays "no seed"), so the scratch buffer is that of
 *      stcd_edt; the row pass strips the bit into a side line of LDS (a byte per four columns) as it loads the row, searches the
 *      argmins as before and rebuilds the seed row of column arg[j] in its epilogue.  Four launches per transform, no atomics. ---- */
/* Bytes of the scratch buffer of the two entries below (16-byte aligned): those of stcd_edt_scratch_bytes. */
int64_t stcd_edt_nearest_scratch_bytes(int height, int width);
/* index: int32 [height,width] on the device; d2: NULL, or int32 [height,width].  Refused before any HIP call: null pointers (d2 and
 * ignore aside), a shape outside [1, 16384], seeds outside 0..2, an ignore plane with seeds 0 or 1, index / d2 not 4-byte or scratch
 * not 16-byte aligned, a scratch buffer that is too small.  16-byte stores when width % 4 == 0 and index (and d2) are 16-byte
 * aligned. */
int stcd_edt_nearest(const uint8_t* mask, const uint8_t* ignore, int height, int width, int seeds, int32_t* d2, int32_t* index,
                     void* scratch, int64_t scratch_bytes, void* hip_stream);
/* out: int32 [height,width] on the device = values[index] where d2 <= q, else 0; values: int32 [height,width]; q >= 0.  Neither
 * index nor d2 is written.  Refused before any HIP call: null pointers, a shape outside [1, 16384], seeds outside 0..2, q < 0,
 * values / out not 4-byte or scratch not 16-byte aligned, a scratch buffer that is too small, out overlapping mask or values. */
int stcd_edt_gather(const uint8_t* mask, int height, int width, int seeds, int q, const int32_t* values, int32_t* out, void* scratch,
                    int64_t scratch_bytes, void* hip_stream);
/* One pass, one launch: out uint8 [height,width] as defined above; owner: NULL, or int32 [height,width]; counts: int64 [2] on the
 * device = (cut pixels, orphan pixels), cleared by the entry itself (one hipMemsetAsync), reduced per wave and block before one
 * 64-bit integer atomic per block and counter.  labels, core_labels, index: int32 [height,width]; an index outside [-1, height *
 * width) counts as -1.  Refused before any HIP call: null pointers (owner aside), a shape outside [1, 16384], mask_value outside
 * [1, 255], int32 planes not 4-byte or counts not 8-byte aligned, out overlapping mask.  Needs no scratch buffer. */
int stcd_objects_split_cut(const uint8_t* mask, const int32_t* labels, const int32_t* core_labels, const int32_t* index, int height,
                           int width, int mask_value, uint8_t* out, int32_t* owner, int64_t* counts, void* hip_stream);

/* ---- per-op entry points (NHWC, activation dtype per `dtype`); used by the parity tests.
 *      Geometry is the engine's generic "tap list" convolution: see DESIGN.md section 3. ---- */
typedef struct stcd_conv_geom {
    int32_t n, hi, wi, ci, ldi;         /* input: images, spatial, channels (K per tap), pixel stride (elements) */
    int32_t hm, wm, in_stride;          /* output-position grid per image; input pixel = m*in_stride + tap */
    int32_t ho, wo, out_stride, oy0, ox0; /* output buffer dims; output pixel = m*out_stride + (oy0,ox0) */
    int32_t co, ldo;                    /* output channels, output pixel stride (elements) */
    int32_t ntaps;
    int8_t dy[9], dx[9];
    int8_t pad_[2];
} stcd_conv_geom;

/* w: fp32 [ntaps][ci][co]; bias: fp32 [co] or NULL; impl: 0 = reference FMA kernel, 1 = MFMA, the kernel the engine would
 * pick (bf16 only: small-channel persistent kernel, resident-filter kernel, tap-list GEMM kernel, else the generic one),
 * 2 = generic MFMA kernel, 3 = resident-halo kernel (wide 3x3 layers, opt-in in the engine), 6 = LDS-DMA kernel (Ci % 64 == 0,
 * Co % 256 == 0, an even number >= 4 of (64-channel chunk, tap) K-tiles: 256 positions x 256 channels per persistent 8-wave block,
 * `buffer_load ... lds` staging with counted vmcnt -- what the engine runs for ChangeFormer's 256 -> 256 decoder-head layers,
 * /root/reference/models/ChangeFormerBaseNetworks.py:85-120), 8 = LDS-DMA tile kernel (3x3 stride 1 over the full map, Ci % 64 == 0,
 * Co % 16 == 0: the resident-filter kernel's 16 x 16 tile with the filter slice and the halo of all input channels requested by
 * `buffer_load ... lds` before the first MFMA -- what the engine runs for FC-Siam's 64- to 256-channel layers on 64^2 / 32^2 maps;
 * outputs bit-identical to impl 1's) */
int stcd_op_conv(int dtype, int impl, const stcd_conv_geom* g, const void* in, const float* w, const float* bias,
                 void* out, void* scratch, int64_t scratch_bytes, void* hip_stream);
/* One NAMED bf16 conv kernel with the features the engine fuses into it (stcd_op_conv launches the kernels with one group and
 * none of them): per-channel sums of the rounded output, the ConvEpi epilogue, BatchNorm-backward sums of a data gradient.
 * The filter is packed as stcd_op_conv packs it and the plan is the kernel's own planner's for `groups`; a combination the named
 * kernel's planner or launcher does not take is an error -- no other kernel runs in its place, and nothing is launched.
 * Images are ordered group by group (n % groups == 0: date-0 images first, then date-1 images). */
enum { STCD_CONV_SMALL = 0, STCD_CONV_RES = 1, STCD_CONV_TILE = 2, STCD_CONV_GEMM = 3, STCD_CONV_HALO = 4, STCD_CONV_DMA = 5 };
typedef struct stcd_conv_fused {
    int32_t kernel;                 /* STCD_CONV_*: k_conv_small / _res / _tile / _gemm / _halo / _dma */
    int32_t groups;                 /* BatchNorm groups the tiles are partitioned by (1 for halo / dma) */
    /* sums (small, res, tile, gemm), or sum_acc == NULL: int64 [bn_rep][groups][2][sum_c] += sum(y) * sum_scale1 and
     * sum(y^2) * sum_scale2 of the stored (rounded; gemm: ReLU'd and rounded, before gate / residual) output channels
     * [sum_c0, sum_c0 + sum_c).  The kernels ADD.  k_conv_small: sum_c0 = 0, sum_c = co, scales 2^26 and 2^18 only. */
    void* sum_acc;
    int32_t sum_c0, sum_c;
    float sum_scale1, sum_scale2;
    /* epilogue (gemm, halo, dma), or use_epi == 0:  v = conv + bias; relu: v = max(v, 0); v = round_bf16(v);
     * gate: v = gate > 0 ? v : 0; res: out = round_bf16(alpha * v + beta * res).  gate / res: bf16 tensors of the OUTPUT buffer's
     * geometry [n][ho][wo] with pixel strides ldg / ldr (multiples of 8, >= co), nullable; without res alpha = beta = 1. */
    int32_t use_epi, relu;
    const void* gate;
    const void* res;
    int32_t ldg, ldr;
    float alpha, beta;
    /* BatchNorm-backward sums (small, res), or bw_acc == NULL: the launch is a data gradient writing dA of a conv -> BN -> ReLU ->
     * Dropout2d layer whose conv output is bw_y (bf16, output geometry, pixel stride bw_ldy); bw_stat: fp32 [groups][4][co] (mean,
     * invstd, scale, shift), bw_mask: fp32 [n][co] or NULL.  bw_acc: int64 [bn_rep][groups][2][co] += 2^36 * sum(dz) and
     * 2^36 * sum(dz * (y - mean) * invstd), dz = round_bf16(dA) * mask * (y * scale + shift > 0). */
    const void* bw_y;
    const float* bw_stat;
    const float* bw_mask;
    void* bw_acc;
    int32_t bw_ldy;
    /* out (filled in as soon as the plan stands, before anything is launched): blocks of the grid; tiles (gemm / dma: M-tiles) one
     * group walks; blocks that share them, i.e. the adds one accumulator entry receives; replicas of the accumulator */
    int32_t blocks, tiles_per_group, blocks_per_group, bn_rep;
    int32_t tile_m;                 /* gemm: positions per M-tile (128 or 64); 0 otherwise */
} stcd_conv_fused;
/* w: fp32 [ntaps][ci][co]; bias: fp32 [co] or NULL; scratch: stcd_op_scratch_bytes(g) */
int stcd_op_conv_fused(const stcd_conv_geom* g, stcd_conv_fused* f, const void* in, const float* w, const float* bias, void* out,
                       void* scratch, int64_t scratch_bytes, void* hip_stream);
/* dw: fp32 [ntaps][ci][co], overwritten; impl: 0 = reference FMA kernel, 1 = MFMA tile kernel (4: its 64 x 32-channel tile
 * allowed for Ci >= 64, as the SNUNet engine runs it; 5: its 64 x 64-channel tile, an opt-in variant), 3 = MFMA position-GEMM kernel
 * (one tap, Ci >= 64, Co >= 64: what the engine runs for 1x1 convs and the phases of 2x2 stride-2 transposed convs),
 * 7 = LDS-DMA kernel (stride-1 full-map tap lists with Ci % 256 == 0, Co % 256 == 0, maps >= 64 wide; dY plain or one sub-pixel
 * phase of a map twice as large: block = (position split, tap, 256 x 256 channel tile) -- ChangeFormer's decoder-head layers) */
int stcd_op_wgrad(int dtype, int impl, const stcd_conv_geom* g, const void* in, const void* dout, float* dw,
                  void* scratch, int64_t scratch_bytes, void* hip_stream);
int64_t stcd_op_scratch_bytes(const stcd_conv_geom* g);

/* ---- per-op entry points of the normalisation / pooling / fusion kernels (NHWC, activation dtype per `dtype`,
 *      channels a power of two >= 8); each runs exactly the launch sequence the engine runs for that layer step.
 *      n = images (date-0 images first, then date-1 images when groups == 2: BatchNorm statistics stay per date,
 *      /root/reference/models/SiamUnet_diff.py:99 and :123 call the same bn module once per date). ---- */
typedef struct stcd_map_geom {
    int32_t n, h, w, c, groups;
} stcd_map_geom;
int64_t stcd_op_ew_scratch_bytes(const stcd_map_geom* g);
/* a = dropout_mask * relu(BatchNorm2d(y)) (nn.BatchNorm2d + F.relu + nn.Dropout2d, SiamUnet_diff.py:19-20,99), optional
 * pool = F.max_pool2d(a, 2, 2) (:101).  training != 0: batch statistics per group, running stats updated in place
 * (momentum 0.1, unbiased variance; group 0 then group 1); else running statistics.  mask: nullable fp32 [n][c].
 * stat (out): fp32 [groups][4][c] = mean, 1/sqrt(var+eps), scale, shift -- what the backward needs. */
int stcd_op_bn_act(int dtype, const stcd_map_geom* g, const void* y, int ldy, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, const float* mask, int relu, int training, void* a, int lda,
                   void* pool, int ldp, float* stat, void* scratch, int64_t scratch_bytes, void* hip_stream);
/* the same for the last conv of an encoder level (groups == 2, training, ReLU), both dates in one pass, also writing the
 * bi-temporal skip fused = |a1 - a2| (fuse_mode 0, SiamUnet_diff.py:150) or a2 - a1 (1, SiamUnet_sub.py:150): [n/2] images.
 * a == NULL: the activations themselves are not written (only pool and fused; see stcd_op_skip_bwd) */
int stcd_op_bn_act_pair(int dtype, const stcd_map_geom* g, const void* y, int ldy, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, const float* mask, int fuse_mode, void* a, int lda, void* pool,
                        int ldp, void* fused, int ldf, float* stat, void* scratch, int64_t scratch_bytes, void* hip_stream);
/* backward of stcd_op_bn_act (training): da -> dy (may alias da), dgamma, dbeta summed over the groups */
int stcd_op_bn_act_bwd(int dtype, const stcd_map_geom* g, const void* da, int ldda, const void* y, int ldy, const float* stat,
                       const float* mask, int relu, void* dy, int lddy, float* dgamma, float* dbeta, void* scratch,
                       int64_t scratch_bytes, void* hip_stream);
int stcd_op_maxpool(int dtype, const stcd_map_geom* g, const void* a, int lda, void* pool, int ldp, void* hip_stream);
/* da (+)= dpool routed to the first maximum of each 2x2 window (torch's tie rule) */
int stcd_op_maxpool_bwd(int dtype, const stcd_map_geom* g, const void* a, int lda, const void* dpool, int ldp, void* da, int ldda,
                        int accumulate, void* hip_stream);
/* skip fusion of the two dates (groups == 2): d[n/2 images] = |a1 - a2| (mode 0) or a2 - a1 (mode 1), and its gradient */
/* F.max_pool2d(x, 3, 2, 1) of the ResNet stem (models/resnet.py:176) and its gradient (SegCD): g describes the INPUT map (h, w even);
 * pool / dpool are [n, h/2, w/2, c]; idx (n*(h/2)*(w/2)*c bytes) receives / provides the winning window position of every element */
int stcd_op_maxpool3(int dtype, const stcd_map_geom* g, const void* a, int lda, void* pool, int ldp, void* idx, void* hip_stream);
int stcd_op_maxpool3_bwd(int dtype, const stcd_map_geom* g, const void* idx, const void* dpool, int ldp, void* da, int ldda, void* hip_stream);
/* cross_conc's grouped 3x3 convolution (models/SiamUnet_crossconc.py:14-18,24-29: the two dates' channels interleaved, one group per
 * channel pair) on the two dates as they sit stacked in the batch dimension (g->groups == 2, a: [2 * n, h, w, c]; out / dout: [n, h, w, c];
 * w: the reference tensor [c][2][3][3], b: [c] or NULL); the backward writes both dates' gradients (da like a) and dw. */
int64_t stcd_op_pairdw_scratch_bytes(const stcd_map_geom* g);
int stcd_op_pairdw(int dtype, const stcd_map_geom* g, const void* a, int lda, const float* w, const float* b, void* out, int ldo,
                   void* hip_stream);
int stcd_op_pairdw_bwd(int dtype, const stcd_map_geom* g, const void* a, int lda, const void* dout, int lddo, const float* w, void* da,
                       int ldda, float* dw, void* scratch, int64_t scratch_bytes, void* hip_stream);
int stcd_op_fuse(int dtype, int mode, const stcd_map_geom* g, const void* a, int lda, void* d, int ldd, void* hip_stream);
int stcd_op_fuse_bwd(int dtype, int mode, const stcd_map_geom* g, const void* a, int lda, const void* dd, int ldd, void* da, int ldda,
                     void* hip_stream);
/* nn.ReplicationPad2d((0, w - w0, 0, h - h0)) in place on a [n,h,w] map whose valid region is h0 x w0
 * (SiamUnet_diff.py:149), and its gradient (the replicas' gradients fold into the edge pixel) */
int stcd_op_rep_pad(int dtype, const stcd_map_geom* g, void* d, int ld, int h0, int w0, void* hip_stream);
int stcd_op_rep_pad_bwd(int dtype, const stcd_map_geom* g, void* dd, int ld, int h0, int w0, void* hip_stream);
/* backward of an encoder level's last conv in one pass (groups == 2): da = max-pool gradient of dpool + skip-fusion
 * gradient of dd, then the BatchNorm backward of it: dy, dgamma, dbeta.  a == NULL: the activations were not stored
 * (stcd_op_bn_act_pair with a == NULL; the engine's default plan for diff / sub) and are recomputed from y, stat and mask with
 * the forward's arithmetic -- channels a multiple of 8 and a power of two <= 256 */
int stcd_op_skip_bwd(int dtype, int mode, const stcd_map_geom* g, const void* a, int lda, const void* y, int ldy, const void* dd,
                     int ldd, const void* dpool, int ldp, const float* stat, const float* mask, void* da, int ldda, void* dy,
                     int lddy, float* dgamma, float* dbeta, void* scratch, int64_t scratch_bytes, void* hip_stream);

/* ---- per-op entry points of the ChangeFormer kernels (contiguous tensors: tokens [rows, c] / maps [n, h, w, c] NHWC, activation dtype
 *      per `dtype`); each runs the launch sequence the engine runs for that step.  Dropout inside an op: site 0 of `seed`
 *      (stcd_cf_site above; DropPath of stcd_op_cf_resid_drop: site 1), p == 0 disables it. ---- */
int64_t stcd_op_cf_scratch_bytes(int64_t rows, int channels, int n, int q_tokens, int kv_tokens);
/* OverlapPatchEmbed.proj / Attention.sr as GEMMs (ChangeFormer.py:207-208, 315): col [n*ho*wo, ldc], column ci*k*k + ky*k + kx */
int stcd_op_cf_im2col(int dtype, const void* x, void* col, int ldc, int n, int h, int w, int c, int k, int stride, int pad, void* hip_stream);
int stcd_op_cf_col2im(int dtype, const void* dcol, int ldc, void* dx, int n, int h, int w, int c, int k, int stride, int pad, int accumulate,
                      void* hip_stream);
/* nn.LayerNorm(c, eps) per row (ChangeFormer.py:209,317,478,486); stats fp32 [rows][2] = mean, 1/sqrt(var + eps) */
int stcd_op_cf_layernorm(int dtype, const void* x, void* y, const float* gamma, const float* beta, float* stats, int64_t rows, int c, float eps,
                         void* hip_stream);
/* dx = [add] + LayerNorm-backward(dy [+ dy2]); dgamma, dbeta fp32 [c] overwritten */
int stcd_op_cf_layernorm_bwd(int dtype, const void* dy, const void* dy2, const void* x, const float* stats, const float* gamma, const void* add,
                             void* dx, float* dgamma, float* dbeta, void* scratch, int64_t rows, int c, void* hip_stream);
int stcd_op_cf_colsum(int dtype, const void* x, int64_t rows, int c, float* out, void* scratch, void* hip_stream);
/* Attention.forward between the q / kv projections and proj (ChangeFormer.py:347-354): q [n, q_tokens, heads*d], kv [n, kv_tokens, 2*heads*d]
 * (k then v, head-major channels), out [n, q_tokens, heads*d], lse fp32 [n, heads, q_tokens]; scale = d^-0.5; attn_drop probability p */
int stcd_op_cf_attention(int dtype, const void* q, const void* kv, void* out, float* lse, int n, int q_tokens, int kv_tokens, int heads, int d,
                         float p, uint64_t seed, void* hip_stream);
int64_t stcd_op_cf_attention_scratch_bytes(int n, int q_tokens, int kv_tokens, int heads, int d);
int stcd_op_cf_attention_bwd(int dtype, const void* q, const void* kv, const void* out, const void* dout, const float* lse, void* dq, void* dkv,
                             void* scratch, int n, int q_tokens, int kv_tokens, int heads, int d, float p, uint64_t seed, void* hip_stream);
/* Mlp between fc1 and fc2 (ChangeFormer.py:289-292, 517-523): u = depthwise3x3(h) + b, a = dropout(GELU(u)); w = [ch][1][3][3] */
int stcd_op_cf_dwgelu(int dtype, const void* h, void* u, void* a, const float* w, const float* b, int n, int height, int width, int ch, float p,
                      uint64_t seed, void* hip_stream);
int64_t stcd_op_cf_dwgelu_scratch_bytes(int n, int height, int width, int ch);
/* da is overwritten with the gated gradient; dh = d(h); dw [ch][9], db [ch] overwritten */
int stcd_op_cf_dwgelu_bwd(int dtype, const void* h, const void* u, void* da, void* dh, const float* w, float* dw, float* db, void* scratch, int n,
                          int height, int width, int ch, float p, uint64_t seed, void* hip_stream);
/* Block.forward's x + drop_path(dropout(y)) (ChangeFormer.py:505-509) over [n, rows_per_img, c]; backward != 0: out = d(y) from y = d(out) */
int stcd_op_cf_resid_drop(int dtype, const void* x, const void* y, void* out, int n, int64_t rows_per_img, int c, float p, float path_p,
                          uint64_t seed, int backward, void* hip_stream);
/* F.interpolate(mode="bilinear", align_corners=False) (ChangeFormer.py:1585,1591) [n,h,w,c] -> [n,out_h,out_w,c]; backward != 0: src is the
 * gradient of the large map, dst receives the gradient of the small one; accumulate != 0: dst += */
int stcd_op_cf_bilinear(int dtype, const void* src, void* dst, int n, int h, int w, int out_h, int out_w, int c, int accumulate, int backward,
                        void* hip_stream);
/* op: 0 PReLU(x; alpha[0]) | 1 x * dropout(p) | 2 relu(x) | 3 x * [y > 0] | 4 alpha_f * x + beta_f * y (y nullable) */
int stcd_op_cf_elementwise(int dtype, int op, const void* x, const void* y, void* out, int64_t rows, int c, const float* alpha, float alpha_f,
                           float beta_f, float p, uint64_t seed, void* hip_stream);
/* dy = dz * (y > 0 ? 1 : alpha[0]); dalpha[0] = sum dz * y * [y <= 0] */
int stcd_op_cf_prelu_bwd(int dtype, const void* dz, const void* y, void* dy, const float* alpha, float* dalpha, void* scratch, int64_t rows, int c,
                         void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* STCD_HIP_H */
