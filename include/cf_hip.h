/* cf_hip.h - C ABI of libcfhip.so: the MI355X (gfx950) kernels of the CenterFusion forward path.
 *
 * The reference (HengWeiBin/CenterFusionDetect3D) is pure Python on PyTorch; its "FFI" for this
 * path is the set of ATen / torchvision operators its modules dispatch to.  Each entry point below
 * names the reference interface it replaces (paths relative to /root/reference/src/lib).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory unless marked "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); launches are asynchronous;
 *   - no hidden allocation, no host synchronisation, re-entrant per stream (graph-capturable);
 *   - return value: 0 on success, negative CF_E* code on failure (never throws across the ABI);
 *     cf_last_error() returns a static host string describing the last failure of this thread.
 *   - activations between kernels are NHWC fp32 ("channels-last"); the module boundary tensors
 *     (images in, head maps out) are NCHW fp32 as in the reference.
 */
#ifndef CF_HIP_H
#define CF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_ABI_VERSION 7 /* 2: cf_dcn_args.mask_activated, cf_nchw_to_nhwc, cf_spin_us; 3: cf_conv3x3_root_f16x3, stride 2 in cf_conv3x3_f16x3; 4: cf_head_fused_args.mx / first_scale, cf_pack_feat_mx, cf_dcn_args.out_mx; 5: cf_conv3x3_proj_f16x3, cf_stem_args.out_pool, cf_pack_conv_f16x3, cf_pack_dcn_f16; 6: in_scale (per-layer activation pre-scale of the f16x3 kernels) in cf_conv_args / cf_dcn_args / cf_stem_args, cf_dcn_args.mx_scale, cf_pack_feat_mx_scaled, cf_absmax_f32, cf_checksum64, cf_topk_peaks_if_changed, cf_topk_frustum; 7: the exports cf_conv2d_bf16x3 and cf_head_tail (CF_EINVAL stubs since ABI 6) removed, with CF_LAYOUT_NHWC_SPLIT_BF16 (an out_layout only the former took); nothing else changed */

#define CF_OK 0
#define CF_EINVAL (-22)
#define CF_ELAUNCH (-5)

#define CF_MAX_SRC 4
#define CF_MAX_GROUPS 4 /* layers per cf_conv3x3_f16x3_grouped / cf_dcn_v2_f16x3_grouped launch */

/* activation / epilogue modes of cf_conv2d_fused and cf_dcn_v2_fused */
#define CF_ACT_NONE 0
#define CF_ACT_RELU 1
#define CF_ACT_SIGMOID_CLAMP 2 /* clamp(sigmoid(x), 1e-4, 1-1e-4)  (networks/detectHeads.py:21-23) */
#define CF_ACT_RAW_AND_SIGDEPTH 3 /* out = x, out2 = 1/(sigmoid(x)+1e-6)-1 (model/utils.py:131-141) */

#define CF_LAYOUT_NHWC 0
#define CF_LAYOUT_NCHW 1

/* One 16-byte K-slot of the implicit GEMM: 4 consecutive channels of one source at one tap. */
typedef struct cf_slot {
  int32_t src;   /* index into cf_conv_args.src (uniform inside a 32-wide K chunk); -1: zero chunk */
  int32_t dy;    /* tap row offset relative to ho*stride (already includes -pad)                    */
  int32_t dx;    /* tap col offset relative to wo*stride                                            */
  int32_t c_off; /* first channel inside the source row; <0: zero padding slot                      */
} cf_slot;

/* cf_conv2d_fused: implicit-GEMM convolution on the fp32 MFMA pipe with a fused epilogue
 *   out = act( conv(cat(src...), W) + bias [+ residual] )
 * replaces aten::conv2d + aten::batch_norm(eval, folded into W/bias) + add_ + relu_ of
 *   model/networks/dla.py:21-41 (Root: the channel concat is never materialised - up to 4 sources),
 *   dla.py:124-161 (BasicBlock), dla.py:177-192,250-269 (stem/level0/level1), dla.py:98-103 (project),
 *   dla.py:426-433 (conv_offset_mask), model/networks/detectHeads.py:59-98 (head convs) and
 *   model/networks/fusionModules.py:18-35 (ConcateCombiner: feat || pc_hm as two sources).
 * GEMM view: M = B*Ho*Wo, N = n_out, K = 4 * n_slots, weights pre-packed [N_pad][K_pad]
 * (K contiguous, BN folded) in slot order by the host (centerfusiondetect3d_amd/packing.py). */
typedef struct cf_conv_args {
  const float* src[CF_MAX_SRC]; /* NHWC sources sharing B,H,W                                        */
  int32_t src_c[CF_MAX_SRC];    /* channel stride (floats per pixel) of each source                  */
  int32_t n_src;
  int32_t B, H, W;              /* input geometry                                                     */
  int32_t Ho, Wo;               /* output geometry                                                    */
  int32_t stride;               /* spatial stride                                                     */
  const float* weight;          /* [N_pad][K_pad]                                                     */
  const cf_slot* slots;         /* [K_pad/4]                                                          */
  const float* bias;            /* [N_pad]                                                            */
  int32_t K_pad;                /* multiple of 32                                                     */
  int32_t N;                    /* real output channels                                               */
  int32_t N_pad;                /* multiple of 32, >= N                                               */
  const float* residual;        /* optional NHWC [M][res_stride], added before the activation         */
  int32_t res_stride;
  float* out;                   /* NHWC: [M][out_stride] ; NCHW: [B][N][Ho*Wo]                        */
  float* out2;                  /* second output for CF_ACT_RAW_AND_SIGDEPTH (same layout) or NULL    */
  int32_t out_stride;           /* floats per pixel of the NHWC destination (>= N)                    */
  int32_t out_layout;           /* CF_LAYOUT_*                                                        */
  int32_t act;                  /* CF_ACT_*                                                           */
  int32_t precise;              /* !=0: two-level (per-32-K-chunk) fp32 summation, see cf_gemm.hip    */
  float out_scale;              /* f16x3 kernels only: 2^-s / in_scale, s = weight scale exponent (2^-(s+4) at the
                                   default in_scale)                                                   */
  float in_scale;               /* (ABI 6) f16x3 kernels only: the power of two every source value (and, in the fused
                                   Root / projection forms, every operand of that GEMM) is multiplied by before
                                   the split into fp16 hi + lo.  0 = the default 16.  |x| * in_scale must stay
                                   below 65504: larger values are CLAMPED (see "Dynamic range" below)  */
} cf_conv_args;
int cf_conv2d_fused(const cf_conv_args* a, void* stream);

/* cf_stem_fused: the DLA-34 stem in one launch - base_layer 7x7 (C -> 16), level0 3x3 (16 -> 16) and
 * level1 3x3 stride 2 (16 -> 32), each followed by its folded BatchNorm and ReLU
 * (model/networks/dla.py:237-262: DLA.base_layer, level0, level1) - straight from the NCHW image batch
 * to the half-resolution fp32 NHWC level1 map; the full-resolution intermediates stay in LDS
 * (cf_stem.hip).  f16x3 arithmetic (fp32-level accuracy).  Weights: MFMA 16x16x32 fragment order as
 * produced by packing.pack_stem; scale_* = 2^-(s+4) of the layer. */
typedef struct cf_stem_args {
  const float* x;                 /* images, fp32 NCHW (B, C, H, W), C <= 3                    */
  int32_t B, C, H, W;             /* H, W even                                                 */
  const void* w_base;   const float* b_base;   float scale_base;
  const void* w_level0; const float* b_level0; float scale_level0;
  const void* w_level1; const float* b_level1; float scale_level1;
  float* out;                     /* fp32 NHWC (B, H/2, W/2, 32)                               */
  float* out_pool;                /* (ABI 5) optional: MaxPool2d(2, 2) of `out`, fp32 NHWC (B, H/4, W/4, 32) - the level-2
                                     Tree's downsample (dla.py:96), written from the same registers; NULL = not written */
  float in_scale[3];              /* (ABI 6) activation pre-scale (power of two, 0 = 16) of the image, of base_layer's output
                                     and of level0's output; scale_* = 2^-s / in_scale[i] of the layer that reads it */
} cf_stem_args;
int cf_stem_fused(const cf_stem_args* a, void* stream);

/* cf_stem_fused_early: cf_stem_fused for EARLY radar fusion (MODEL.FUSION_STRATEGY = "early"): base_layer has six input channels,
 * [image 0-2 | radar map 3-5], the radar map nearest-upsampled x4 from the output size to the image size.  replaces
 * model/networks/fusionModules.py:18-35 (ConcateCombiner: F.interpolate + torch.cat) + model/networks/dla.py:250-262 (the stem
 * on the six-channel image).  The six-channel image is never written: a workgroup reads the map at (y >> 2, x >> 2) into a second
 * plane of its LDS patch and runs the radar taps as 13 further k-steps into the base layer's accumulators, behind the image's
 * (with all-zero radar weights the outputs are cf_stem_fused's, bit for bit).  Everything behind base_layer is cf_stem_fused.
 * `stem` is that entry point's block (x: the image, C <= 3; in_scale[0] pre-scales the radar values too: |v| * in_scale[0] above
 * 65504 is clamped); w_base / w_base_radar / scale_base come from packing.pack_stem_early (ONE 2^s for all six channels).
 * H and W must be multiples of 4 and the map exactly (H/4, W/4): anything else returns CF_EINVAL.  (added under ABI 7) */
typedef struct cf_stem_early_args {
  cf_stem_args stem;
  const float* pc;                /* radar map, fp32 NCHW (B, 3, pc_h, pc_w): read only                */
  int32_t pc_h, pc_w;             /* must be H / 4, W / 4                                              */
  const void* w_base_radar;       /* [13 k-steps][2][64 lanes][8 f16]: w_base's layout, channels 3-5   */
} cf_stem_early_args;
int cf_stem_fused_early(const cf_stem_early_args* a, void* stream);

/* cf_conv2d_f16x3: cf_conv2d_fused semantics (fp32 NHWC sources / residual / output, bias, ReLU) with
 * the products evaluated on the f16 MFMA pipe from split operands (x = hi + lo fp16 after a
 * power-of-two scale): fp32-level accuracy at ~3x the fp32-MFMA rate (cf_gemm_f16.hip).  Differences
 * in the argument block: one slot = 8 channels (src_c multiples of 8, K_pad = 8 * n_slots, multiple
 * of 32); weight = fragment-packed fp16 hi/lo planes of 2^s * W (packing.pack_conv_f16);
 * out_scale = 2^-(s+4); N_pad is 32 or a multiple of 64; output layout NHWC only; act NONE / RELU. */
int cf_conv2d_f16x3(const cf_conv_args* a, void* stream);

/* cf_conv3x3_f16x3: the 3x3 / stride 1 / pad 1 / single-source case of cf_conv2d_f16x3 with LDS patch
 * reuse (cf_conv3x3_f16.hip): each 16-channel slice of the input rows a pixel tile needs is fetched
 * and split once and serves all 9 taps.  Same argument block and same result as cf_conv2d_f16x3 for
 * weights packed slice-major (k = (16-channel slice, tap, channel): K_pad = 144 * C/16 rounded up to
 * 32; the slot table lists that order, so it is only read when the call falls back).  Feature maps too
 * wide for the patch (about W > 250) are forwarded to cf_conv2d_f16x3.  Carries the BasicBlock
 * convolutions (model/networks/dla.py:42-62) and DeformConv.conv_offset_mask (dla.py:406-414). */
int cf_conv3x3_f16x3(const cf_conv_args* a, void* stream);
/* (ABI 3) also the 3x3 / stride 2 / pad 1 case - the BasicBlock conv1 that opens a DLA level (dla.py:124-145): odd / even
 * input columns as two planes of the LDS patch; same packing, same result as cf_conv2d_f16x3. */

/* cf_conv3x3_root_f16x3: BasicBlock.conv2 (+ residual + ReLU; dla.py:33-41) of a one-level Tree's tree2 and the Tree's
 * Root (1x1 convolution + BN + ReLU over cat(x2, x1, *children); dla.py:105-118, 81-96) in ONE launch:
 *   x2 = ReLU(conv3x3(t, W2) + b2 + x1);  out = act(W_root . [x2; x1] + b_root)
 * `conv` is conv2's argument block as for cf_conv3x3_f16x3 (residual = x1, act = RELU; `out` = a buffer for x2, written
 * only when the call falls back); `root` is the Root's block as for cf_conv2d_f16x3 with src[0] = conv->out,
 * src[1] = conv->residual and, behind them, the Tree's children (dla.py:109-117; level_root's pooled input, earlier
 * tree outputs); `root_channels[i]` (host array, n_src entries) = the channels the Root reads from source i.  Where a workgroup holds every channel of its pixels (64 / 128 / 256-channel layers) x2 never leaves the
 * chip: it is split to fp16 hi / lo into LDS as the B operand of the Root's GEMM, whose products and order are those of
 * cf_conv2d_f16x3 - so the result equals the two launches bit for bit, which is what runs for every other shape. */
int cf_conv3x3_root_f16x3(const cf_conv_args* conv, const cf_conv_args* root, const int32_t* root_channels, void* stream);

/* (ABI 5) cf_conv3x3_proj_f16x3: BasicBlock.conv2 of the sub-tree that opens a DLA level TOGETHER WITH the Tree's `project`
 * (1x1 convolution + BN of the 2x2-max-pooled level input), which the reference computes as a tensor and hands to the
 * block as its residual (model/networks/dla.py:96-107 Tree.forward: bottom = downsample(x); residual = project(bottom);
 * x1 = tree1(x, residual); dla.py:56-62 BasicBlock: out = bn2(conv2(.)) + residual; relu):
 *   out = act( conv3x3(src[0], W2) + W_p . src[1] + (b2 + b_p) )
 * One argument block as for cf_conv3x3_f16x3 with n_src = 2: src[0] = the 3x3 input, src[1] = the pooled tensor (same
 * B, H, W as the output), weights = packing.pack_conv_f16(proj=...) - the projection's k-steps (slots: source 1, tap
 * (0, 0)) behind the slice-major 3x3 part, both scaled by one 2^s, bias = the sum.  `src_channels` (host array, 2
 * entries) = the real channels of the two sources (multiples of 32).  The projection's products go into the same
 * accumulators, last: no residual tensor, one launch less per DLA level.  A geometry no patch tiling fits runs
 * cf_conv2d_f16x3 on the same slot table (the same products in the same order; the same bits wherever the patch tiling
 * does not split K over waves - maps of at most 512 pixels with 256+ channels do, as in cf_conv3x3_f16x3). */
int cf_conv3x3_proj_f16x3(const cf_conv_args* a, const int32_t* src_channels, void* stream);

/* cf_conv3x3_f16x3_grouped (added within ABI 7: nothing existing changed): n_groups (1 .. CF_MAX_GROUPS) DeformConv.conv_offset_mask
 * convolutions (dla.py:406-414; N_pad = 32) of ONE geometry on independent inputs as one launch - the projections of an IDA
 * level (dla.py:518-524) depend neither on each other nor on the node chain.  `groups` (host array) holds one argument block
 * per layer as for cf_conv3x3_f16x3: src[0], weight, bias, in_scale and out_scale are the layer's own; B, H, W, src_c[0], K_pad,
 * N, N_pad, out_stride and act must agree; no residual; group g's `out` must be group 0's + g * B*H*W * out_stride floats (one
 * buffer, rows [g M, (g + 1) M)).  A workgroup serves one group: group g's rows are bit for bit those of cf_conv3x3_f16x3 on
 * block g.  n_groups = 1 is that call.  Anything else (n_groups outside the range, a null block, another N_pad) -> CF_EINVAL,
 * nothing is launched. */
int cf_conv3x3_f16x3_grouped(const cf_conv_args* const* groups, int32_t n_groups, void* stream);
/* ... and the tiling that launch takes, form[6] = {WC, WP, WK, patch units per thread, tiled patch, 32-pixel column tiles per
 * wave} (the template arguments of conv3x3_f16x3_kernel_grouped): host arithmetic only, chosen by the launcher's own code. */
int cf_conv3x3_grouped_form(const cf_conv_args* const* groups, int32_t n_groups, int32_t* form);

/* cf_conv3x3_tile_form (added within ABI 7: nothing existing changed): what a call of one of the four cf_conv3x3_* entry points
 * would launch, from the argument blocks that call takes - the launchers' own rule (cf_conv3x3_f16.hip: conv3_pick), host
 * arithmetic only: no stream, nothing launched, the HIP runtime is not touched.  `entry` names the entry point:
 *   CF_CONV3_ENTRY_PLAIN    blocks[0] = the block of cf_conv3x3_f16x3 (stride 1 or 2), n_blocks = 1, channels = NULL
 *   CF_CONV3_ENTRY_ROOT     blocks[0] = conv, blocks[1] = root, n_blocks = 2, channels = root_channels
 *   CF_CONV3_ENTRY_PROJ     blocks[0] = the block of cf_conv3x3_proj_f16x3, n_blocks = 1, channels = src_channels
 *   CF_CONV3_ENTRY_GROUPED  blocks = groups, n_blocks = n_groups, channels = NULL (one group: the answer for cf_conv3x3_f16x3)
 * The blocks are validated as the launch validates them: what it refuses returns CF_EINVAL here.  form[CF_CONV3_FORM_INTS]:
 *   [0]  1: the LDS-patch kernel runs; 0: the call is forwarded to cf_conv2d_f16x3 (a stride-2 block with a residual is
 *        forwarded before the rest of its validation, which is then that entry point's) - entries 2.. are -1
 *   [1]  ROOT entry: 1 = conv2 and the Root run as ONE launch; 0 = two launches, and the answer describes conv2's
 *   [2..14]  the kernel's template arguments WC, WP, WK, RT, NU, DB, MINB, T2, CT, S2, ROOT, PROJ, GRP
 *   [15..22] workgroups in x (per group: a grouped launch has n_groups times as many), gridDim.y, threads, dynamic LDS bytes,
 *        patch rows PR, tiles_x, tiles_y (tiled patches, else 0), rounds of the slice loop */
#define CF_CONV3_ENTRY_PLAIN 0
#define CF_CONV3_ENTRY_ROOT 1
#define CF_CONV3_ENTRY_PROJ 2
#define CF_CONV3_ENTRY_GROUPED 3
#define CF_CONV3_FORM_INTS 23
int cf_conv3x3_tile_form(int32_t entry, const cf_conv_args* const* blocks, int32_t n_blocks, const int32_t* channels, int32_t* form);

/* ---- (ABI 5) host-side weight preparation: SURVEY 8(b) "cf_pack_weights" (one-time BN fold + layout) -------------------------
 * Pure CPU functions (no stream, no device memory): HOST pointers in, HOST buffers out; the caller copies the results to the
 * device once.  They do what centerfusiondetect3d_amd/packing.py does for the Python host - the same arithmetic operation for
 * operation, the same bytes (tests/test_cabi.py) - so a host in any language can feed the f16x3 operators.  Reference: the
 * eval-mode BatchNorm the reference runs as its own op behind every convolution (model/networks/dla.py:29, 36-39, 151-159;
 * DeformConv: dla.py:399-404) is folded here; the heads / stem / upsample packers stay in packing.py. */
typedef struct cf_pack_src {
  int32_t channels;   /* real channels this source contributes to the convolution's Cin                  */
  int32_t stride;     /* floats per pixel of the NHWC tensor holding it (multiple of 8)                  */
  int32_t c_base;     /* first channel inside that tensor (multiple of 8)                                */
} cf_pack_src;
typedef struct cf_pack_bn {        /* eval-mode BatchNorm to fold (per output channel); gamma == NULL: none */
  const float* gamma; const float* beta; const float* mean; const float* var;
  float eps;
} cf_pack_bn;
typedef struct cf_pack_conv_desc {
  const float* weight;             /* (cout, sum of src channels, kh, kw), fp32, host                       */
  const float* bias;               /* (cout) or NULL                                                        */
  cf_pack_bn bn;
  int32_t cout, kh, kw, stride;
  int32_t pad;                     /* < 0: (kh - 1) / 2 * dilation                                          */
  int32_t dilation;
  const cf_pack_src* src; int32_t n_src;
  const float* proj_weight;        /* optional (cout, proj.channels) 1x1 projection summed into the same    */
  const float* proj_bias;          /*   accumulators (cf_conv3x3_proj_f16x3), with its own BatchNorm        */
  cf_pack_bn proj_bn;
  cf_pack_src proj;
} cf_pack_conv_desc;
typedef struct cf_pack_info {
  int32_t n_pad, k_pad;            /* cf_conv_args.N_pad / K_pad (cf_dcn_args: N_pad; K = 9 * C)            */
  int32_t n_slots;                 /* entries of the slot table (k_pad / 8); 0 for the DCN                  */
  int32_t patch;                   /* slice-major 3x3 packing: cf_conv3x3_f16x3 / _root / _proj may run it  */
  float out_scale;                 /* 2^-(s+4): cf_conv_args.out_scale / cf_dcn_args.out_scale              */
  size_t weight_bytes;             /* size of the packed weight buffer                                      */
} cf_pack_info;
/* sizes first (out_scale is not known before the weights are read: 0 here) ... */
int cf_pack_conv_f16x3_info(const cf_pack_conv_desc* d, cf_pack_info* info);
/* ... then the packing: weight_out (weight_bytes), slots_out (n_slots), bias_out (n_pad floats), all host memory */
int cf_pack_conv_f16x3(const cf_pack_conv_desc* d, void* weight_out, cf_slot* slots_out, float* bias_out, cf_pack_info* info);
/* DeformConv main weights (cout, cin, 3, 3) -> cf_dcn_v2_f16x3's layout (K order tap-major, fp16 hi / lo fragments) */
int cf_pack_dcn_f16_info(int32_t cout, int32_t cin, cf_pack_info* info);
int cf_pack_dcn_f16(const float* weight, const float* bias, const cf_pack_bn* bn, int32_t cout, int32_t cin,
                    void* weight_out, float* bias_out, cf_pack_info* info);

/* cf_split_bf16: fp32 NHWC [M][in_stride] (C used) -> split-bf16 [M][2][Cs], channels C..Cs-1 zero.  "split-bf16": every
 * value is carried as two bf16 numbers x = hi + lo (hi = rne(x), lo = rne(x - hi), 16 significant bits together; per pixel
 * [Cs hi][Cs lo], the same bytes as fp32) - the operand format of cf_head_fused, whose products are evaluated as
 * a*b ~= a_lo*b_hi + a_hi*b_lo + a_hi*b_hi with fp32 accumulation (<= ~2^-17 relative error per product). */
int cf_split_bf16(const float* x, void* out, long M, int C, int in_stride, int Cs, void* stream);

/* cf_head_tail_args: the `tail` member of cf_head_fused_args - the layers behind a head group's first 3x3 convolution, for up
 * to CF_MAX_HEADS sibling heads:  x -> [ReLU(W x + b)] x n_hidden -> W_out x + b_out (+ head activation), hidden width 256
 * (the 1x1 layers of model/networks/detectHeads.py:64-71, 80-90).  There is no stand-alone launch for it: x / x_stride /
 * c_base are not read (the hidden tile is produced in LDS by the fused launch and never written to HBM).
 * w_hidden / w_out: weights in the fragment order of v_mfma_f32_16x16x32_bf16 (centerfusiondetect3d_amd/packing.py:
 * pack_fragments16): [row tile of 16][k step of 32][hi,lo][lane 64][8 bf16]; w_hidden[][] is [16 tiles][8 k steps], w_out
 * one row tile (n_out <= 16, zero padded); b_out has 32 floats. */
#define CF_MAX_HEADS 12
typedef struct cf_head_tail_args {
  const void* x;                           /* not read */
  int32_t x_stride;                        /* not read */
  int32_t B, H, W;
  int32_t n_heads;
  int32_t n_hidden;                        /* 0..2 hidden 256->256 layers per head */
  const void* w_hidden[CF_MAX_HEADS][2];
  const float* b_hidden[CF_MAX_HEADS][2];
  const void* w_out[CF_MAX_HEADS];
  const float* b_out[CF_MAX_HEADS];
  float* out[CF_MAX_HEADS];                /* fp32 NCHW (B, n_out, H, W) */
  float* out2[CF_MAX_HEADS];               /* second output of CF_ACT_RAW_AND_SIGDEPTH heads, else NULL */
  int32_t c_base[CF_MAX_HEADS];            /* not read */
  int32_t n_out[CF_MAX_HEADS];
  int32_t act[CF_MAX_HEADS];
} cf_head_tail_args;

/* cf_head_fused: a whole head group in one launch: 3x3 conv (sources -> 256) + ReLU, then the layers of `tail`, on the bf16
 * MFMA pipe with split operands.  Only the (B, n_out, H, W) fp32 NCHW maps are written.  replaces
 * model/networks/detectHeads.py:59-98 end to end (one launch instead of 2 per primary / 4 per secondary head, and no
 * hidden-map round trips through HBM).
 * src[]: split-bf16 NHWC sources (feat, 64 channels [, pc_hm, 8 channels]); w_first[i]: 16x16x32 fragments
 * [256/16][K_pad/32] of head i in the canonical 3x3 slot order (packing.pack_conv_bf16); b_first[i]: 256 floats.
 * The pc_hm source (3 real channels) takes ONE k-step behind the 18 of the feature channels, k = 3 tap + channel (27 real,
 * k = 27..31 zero weights): the kernel gathers the matching operand rows from the pc_hm planes of its LDS patch.  A workgroup
 * whose pc_hm patch (tile + 1-pixel frame) holds only +-0 leaves that k-step out - it would add exact zeros;
 * cf_head_fused_with(a, -1, 0, stream) runs it everywhere (results are the same bits).  (layout of that k-step changed
 * within ABI 7: the argument block and the exports did not; w_first[] is whatever packing.py of the same tree writes)
 * ONE form runs: layout3x3 = 1 with mfma16 = 1 (mx = 0 or 1).  The fields can still spell the forms of earlier kernels
 * (layout3x3 = 0: an arbitrary slot table; mfma16 = 0: 32x32x16 fragments): those calls return CF_EINVAL. */
typedef struct cf_head_fused_args {
  cf_head_tail_args tail;
  const void* src[2];
  int32_t src_c[2];
  int32_t n_src;
  const cf_slot* slots;                    /* mx = 0: validated as before (non-NULL; 8-channel slots), not read by the kernel */
  int32_t K_pad;                           /* mx = 0: validated as before - a multiple of 64, <= 2048, >= 576 (608 with pc_hm: 18 + 1 k-steps) */
  const void* w_first[CF_MAX_HEADS];
  const float* b_first[CF_MAX_HEADS];
  int32_t layout3x3;                       /* must be 1: the slot order is the canonical one - src[0] (64 channels): 9 taps
                                              x 8 slots, then src[1] (8 channels, 3 real): one dense 32-deep chunk, k = 3 tap +
                                              channel (its 4 slots are padding entries) - which the 2-D patch kernel implies
                                              (no slot table reads)                                                       */
  const void* w_out_perm[CF_MAX_HEADS];    /* n_hidden == 0: w_out as ONE 16-row tile whose k position (step ks, group g, j) holds
                                              hidden channel 64 (ks >> 1) + 16 (2 (ks & 1) + (j >> 2)) + 4 g + (j & 3) - the order of
                                              an accumulator register group (packing.pack_fragments16(acc_order=True))    */
  int32_t mfma16;                          /* must be 1: w_first[], w_out_perm[], tail.w_hidden[][] and tail.w_out[] are packed for
                                              v_mfma_f32_16x16x32_bf16 - [16-row tile][k step of 32][hi,lo][lane 64][8 bf16],
                                              lane l = row l & 15, k 8 (l >> 4) + j (packing.pack_fragments16); n_out <= 16 */
  int32_t mx;                              /* != 0: the FIRST layer runs as "fp16 main term + block-scaled FP6
                                              cross terms" (v_mfma_f32_16x16x32_f16 + v_mfma_scale_f32_16x16x128_f8f6f4, 1.5 passes per
                                              product instead of 3): src[0] is the 272-byte-per-pixel image cf_pack_feat_mx writes
                                              (src_c[0] = 64), w_first[i] the operand stream of packing.pack_head_first_mx (slots / K_pad
                                              are not read; 4 * 9 * 14592 bytes of (wave, tap) slabs, then with src[1] 4 * 3 * 4 * 2048 bytes:
                                              the pc_hm weights per tap as before, with the dense pc_hm k-step threaded through that layout's
                                              padding - packing.pack_head_first_mx), src[1] (optional) the
                                              split-bf16 pc_hm planes as before; the tail layers are unchanged.  ABI 4 */
  float first_scale[CF_MAX_HEADS];         /* mx: 2^-(s+4) of head i's first layer (applied where b_first is added) */
} cf_head_fused_args;
int cf_head_fused(const cf_head_fused_args* a, void* stream);
/* cf_head_fused with the launcher's two result-neutral choices forced: tile = 0 (8 x 16) / 1 (16 x 8) / -1 (the rule's own);
   pc_skip = 0 / 1 / -1 likewise.  For tests and measurement tools; the bits do not depend on either.  Any other value is
   CF_EINVAL, before any launch.  cf_head_fused(a, s) is cf_head_fused_with(a, -1, -1, s).  (added under ABI 7) */
int cf_head_fused_with(const cf_head_fused_args* a, int tile, int pc_skip, void* stream);

/* cf_head_fused_at: cf_head_fused at LISTED pixels only (no new struct, ABI 7): the same argument block, evaluated on n_tiles
 * "virtual tiles" of 18 pixels each.  slot_pixels: [n_tiles][18] int32 in device memory, each entry a flat pixel
 * b * H * W + y * W + x of the (B, ., H, W) maps, or anything outside [0, B * H * W) (-1 by convention) for an empty slot.
 * For every listed pixel the launch writes, into `out[]` / `out2[]`, exactly the bits cf_head_fused writes there (the 3x3
 * neighbourhood of the pixel is gathered from src[], zero outside its image); no other element of the maps is touched.
 * Duplicates are allowed (the same bits are then written twice).  Grid: n_tiles x head groups - a launch far below one
 * round of workgroups.  Forms: mx = 0 with or without hidden layers and pc_hm source; mx = 1 without both or with both.
 * cf_head_slot_tables: one launch that builds such tables from up to two (B, K) lists of pixel indices in [0, H * W)
 * (cf_topk_peaks' `inds`): table_ab [B][ceil(2K / 18)][18] from list_a (entries 0..K-1 of an image; NULL: empty) followed by
 * list_b (entries K..2K-1), table_b [B][ceil(K / 18)][18] from list_b alone.  Either table may be NULL.  Every entry in
 * [0, HW) gets a slot, entries outside get -1, the padding up to a whole tile is -1.  No reference counterpart: the
 * reference evaluates every head at every pixel (model/networks/detectHeads.py:117-191) and reads them at the peaks. */
#define CF_HEAD_AT_SLOTS 18                /* listed pixels per virtual tile */
int cf_head_fused_at(const cf_head_fused_args* a, const int32_t* slot_pixels, int n_tiles, void* stream);
int cf_head_slot_tables(const int32_t* list_a, const int32_t* list_b, int B, int K, int HW, int32_t* table_ab,
                        int32_t* table_b, void* stream);

/* cf_pack_feat_mx: fp32 NHWC feature map [M][in_stride] (64 channels used) -> [M][272] bytes for cf_head_fused with mx = 1:
 * per pixel four 64-byte segments g = 0..3 - [8 fp16: hi channels 8g..8g+7][8 fp16: hi channels 32+8g..32+8g+7][FP6 block g:
 * 32 e2m3 fields (element j in bits 6j..6j+5, 24 B) + 8 B zero], block 0 / 1 = lo channels 0-31 / 32-63, block 2 / 3 = hi
 * channels 0-31 / 32-63, where hi = fp16(clamp(16 x)), lo = 16 x - hi - then [4 E8M0 scale bytes, block order][12 B zero].
 * A block's scale is 2^e with e the smallest integer such that max|.| <= 7.5 * 2^e.
 * replaces: nothing in the reference - it is the operand preparation of model/networks/detectHeads.py:64-79 on this path
 * (the fp32 -> split conversion the bf16x3 heads take from cf_split_bf16 / the DCN epilogue).  ABI 4 */
int cf_pack_feat_mx(const float* x, int in_stride, void* rows, long M, void* stream);
/* (ABI 6) the same rows with hi = fp16(clamp(scale x)), lo = scale x - hi for a power-of-two `scale` (cf_pack_feat_mx: 16); the
 * head launch that reads them gets first_scale = 2^-s / scale.  For feature maps whose values exceed 65504 / 16 / 2. */
int cf_pack_feat_mx_scaled(const float* x, int in_stride, void* rows, long M, float scale, void* stream);

/* cf_dcn_v2_fused: modulated deformable 3x3 convolution (stride 1, pad 1, dil 1, groups 1) with
 * the bilinear gather fused into the GEMM A-tile staging, + bias(BN folded) + ReLU.
 * replaces torchvision.ops.deform_conv2d + BN + ReLU of model/networks/dla.py:456-472.
 * `offmask` is the raw output of conv_offset_mask, NHWC with `om_stride` floats per pixel:
 * channels 2k / 2k+1 = dy / dx of tap k, channels 18+k = mask logit of tap k (sigmoid applied
 * here unless mask_activated) - the chunk/cat of dla.py:457-459 is the identity on the first 18 channels. */
typedef struct cf_dcn_args {
  const float* x;       /* NHWC [B][H][W][C]                    */
  const float* offmask; /* NHWC [B][H][W][om_stride], 27 used   */
  int32_t om_stride;
  int32_t B, H, W, C;   /* C multiple of 32                     */
  const float* weight;  /* [N_pad][9*C], k = tap*C + c          */
  const float* bias;    /* [N_pad]                              */
  int32_t N, N_pad;
  float* out;           /* NHWC [B][H][W][out_stride]           */
  int32_t out_stride;
  int32_t act;
  int32_t precise;      /* as cf_conv_args.precise              */
  float out_scale;      /* cf_dcn_v2_f16x3 only: 2^-s / in_scale (2^-(s+4) at the default in_scale) */
  void* out_split_bf16; /* cf_dcn_v2_f16x3 only, optional: the same result additionally as split-bf16 NHWC
                           [B][H][W][2 (hi, lo)][split_stride] - what the head kernels read (saves cf_split_bf16) */
  int32_t split_stride; /* channels per plane of out_split_bf16 (>= N, multiple of 8) */
  void* workspace;      /* cf_dcn_v2_f16x3 only, optional: cf_dcn_v2_workspace_bytes(...) bytes.  With it, small
                           maps (<= 2048 pixels per image) split K over 2-4 workgroups per tile and a second
                           launch adds the partial sums in fixed order; without it K is never split */
  size_t workspace_bytes; /* size of `workspace`; checked against cf_dcn_v2_workspace_bytes(...) when K is split */
  int32_t mask_activated; /* 0: offmask channels 18..26 are mask LOGITS, sigmoid applied here (the fused DeformConv of
                             the module path); != 0: they already are the modulation factors, used as they are - the
                             contract of torchvision.ops.deform_conv2d(mask=...) (dla.py:460: the caller's sigmoid) */
  void* out_mx;           /* cf_dcn_v2_f16x3 only, optional, N = N_pad = 64, not on K-split maps: the same result additionally
                             as the [B*H*W][272] byte rows of cf_pack_feat_mx (bit-identical to packing `out`): the operand
                             format of cf_head_fused with mx = 1 - saves that pass over the feature map.  ABI 4 */
  float in_scale;         /* (ABI 6) cf_dcn_v2_f16x3 only: power of two the sampled values are multiplied by (through the
                             modulation factor) before the fp16 split; 0 = 16; as cf_conv_args.in_scale */
  float mx_scale;         /* (ABI 6) with out_mx: the rows' pre-scale (cf_pack_feat_mx_scaled's `scale`); 0 = 16 */
} cf_dcn_args;
int cf_dcn_v2_fused(const cf_dcn_args* a, void* stream);

/* cf_dcn_v2_f16x3: cf_dcn_v2_fused with the main GEMM on the f16 MFMA pipe from split operands (see
 * cf_conv2d_f16x3); weight = fragment-packed fp16 hi/lo planes of 2^s * W in (tap, channel) K order
 * (packing.pack_dcn_f16), out_scale = 2^-(s+4).  x / offmask / out stay fp32 NHWC. */
int cf_dcn_v2_f16x3(const cf_dcn_args* a, void* stream);
size_t cf_dcn_v2_workspace_bytes(int B, int H, int W, int C, int N_pad);

/* cf_dcn_v2_f16x3_grouped (added within ABI 7: nothing existing changed): the deformable convolutions of n_groups
 * (1 .. CF_MAX_GROUPS) same-shape layers as one launch (and, on K-split maps, ONE reduction over all groups' rows).  `groups`
 * (host array): one block per layer as for cf_dcn_v2_f16x3; x, weight, bias, in_scale and out_scale are the layer's own (two
 * groups may read the same x); the geometry, N, N_pad, strides, act and mask_activated must agree; `offmask` and `out` of
 * group g must be group 0's + g * B*H*W rows; the workspace is group 0's (n_groups x cf_dcn_v2_workspace_bytes(...), or null: no K
 * split).  out_split_bf16 / out_mx are refused (CF_EINVAL) when n_groups > 1.  Group g's rows equal cf_dcn_v2_f16x3 on block g
 * (same workspace choice) bit for bit: same descriptors, same K order, same K split, partial sums added in the same order. */
int cf_dcn_v2_f16x3_grouped(const cf_dcn_args* const* groups, int32_t n_groups, void* stream);
/* ... and what that call (one group: cf_dcn_v2_f16x3 on groups[0]) would launch, by the launchers' own rule (cf_gemm_f16.hip:
 * dcn_pick; K split: dcn_k_split, taken only when the block carries a workspace) - validated as the launch, host arithmetic
 * only, the HIP runtime is not touched (added within ABI 7).  form[CF_DCN_FORM_INTS] = {WC, WP, RT, COAL, CT: the template
 * arguments of dcn_f16x3_kernel (two or more groups: dcn_f16x3_kernel_grouped); gridDim.x, gridDim.y, K parts (gridDim.z;
 * above 1 a reduction launch follows); workgroups in x per group} */
#define CF_DCN_FORM_INTS 9
int cf_dcn_v2_f16x3_form(const cf_dcn_args* const* groups, int32_t n_groups, int32_t* form);

/* What cf_conv2d_fused (dcn = 0) / cf_dcn_v2_fused (dcn = 1) launches for M output pixels: *kind 0 = the 32x32x2 tile
 * kernel, 1 = the 16-channel kernel; *bm x *bn its tile.  Host arithmetic only, nothing is launched.  The launchers
 * choose through the same function, so a test can prove which template instantiation a shape reaches (added within
 * ABI 7: nothing existing changed). */
int cf_gemm_tile_form(long M, int N, int N_pad, int out_layout, int act, int precise, int dcn,
                      int32_t* kind, int32_t* bm, int32_t* bn);

/* Backward of the deformable convolution, for autograd behind the operator-level drop-in (ops.deform_conv2d; added
 * within ABI 7: nothing existing changed).  Replaces the backward torchvision.ops.deform_conv2d registers with autograd
 * (model/networks/dla.py:461-470 under training).  Everything is fp32 NHWC in the forward's layouts and the forward's one
 * configuration (3x3, stride 1, pad 1, dil 1, one group, one offset group, C a multiple of 32, any N <= 1024); the
 * sampling rule is the forward's, floor held constant (at an integer position the offset gradient is the right-hand
 * derivative).  Products on the exact fp32-input MFMA: no range to guard, nothing clamped. */
typedef struct cf_dcn_bwd_args {
  const float* gout;    /* NHWC [B][H][W][N]: gradient of the output                                         */
  const float* weight;  /* RAW weight [N][C][3][3] (cf_dcn_v2_bwd_data only)                                  */
  const float* x;       /* NHWC [B][H][W][C]                                                                  */
  const float* offmask; /* NHWC [B][H][W][32]: dy / dx of tap k in 2k / 2k+1, the ACTIVATED mask in 18..26    */
  int32_t B, H, W, C, N;
  float* gx;            /* cf_dcn_v2_bwd_data: NHWC [B][H][W][C], ZEROED by the caller (float atomics add into it:
                           the last bits can differ from run to run); may be NULL                              */
  float* gom;           /* cf_dcn_v2_bwd_data: NHWC [B][H][W][32] in offmask's channel order (the mask gradient is
                           with respect to the activated mask), channels 27..31 zero; plain stores; may be NULL */
  float* gw;            /* cf_dcn_v2_bwd_weight: [N][C][3][3]; may be NULL                                     */
  float* gbias;         /* cf_dcn_v2_bwd_weight: [N], the sum of gout over the pixels; may be NULL             */
  void* workspace;      /* cf_dcn_v2_bwd_weight: cf_dcn_v2_bwd_workspace_bytes(...) bytes - the pixel dimension is
                           split into slabs whose partial sums a second launch adds in slab order, so gw and gbias
                           are bitwise reproducible (no float atomics)                                         */
  size_t workspace_bytes;
} cf_dcn_bwd_args;
/* gx and gom; a launch whose two outputs are NULL succeeds and does nothing */
int cf_dcn_v2_bwd_data(const cf_dcn_bwd_args* a, void* stream);
/* gw and gbias; a launch whose two outputs are NULL succeeds and does nothing */
int cf_dcn_v2_bwd_weight(const cf_dcn_bwd_args* a, void* stream);
size_t cf_dcn_v2_bwd_workspace_bytes(int B, int H, int W, int C, int N);

/* Training kernels of the neck's DeformConv block (conv_offset_mask -> sigmoid -> DCN -> BatchNorm -> ReLU,
 * model/networks/dla.py:456-472) and of the IDA upsample (added within ABI 7: nothing existing changed).  All tensors
 * fp32 NHWC.  Every parameter gradient is a sum of slab partials that a second launch adds in slab order: bitwise
 * reproducible, no float atomics.  Products through MFMA use the exact fp32-input MFMA: no range to guard.
 *
 * cf_conv3x3_bwd_weight / cf_conv3x3_bwd_data: backward of the offset convolution (3x3, stride 1, zero padding 1,
 * C -> 27; C a multiple of 32, at most 512).  gom [B][H][W][32] is cf_dcn_v2_bwd_data's: channels 18..26 are the
 * gradient with respect to the ACTIVATED mask m, which offmask [B][H][W][32] holds; both kernels multiply them by
 * m (1 - m) as they load them (the gradient with respect to the logits the convolution produced), channels 27..31 are
 * ignored.  _weight: gw [27][C][3][3] and gbias [27], either may be NULL (both: nothing runs); x [B][H][W][C] is the
 * convolution's input.  _data ADDS the input gradient into gx [B][H][W][C] (plain read-modify-write, each pixel row
 * owned by one workgroup: run it on the stream of, and behind, cf_dcn_v2_bwd_data, which fills gx); weight is the raw
 * [27][C][3][3]. */
/* cf_offmask_activate: channels 18..26 of an offmask buffer [M][32] in place, logit -> sigmoid: the forward of the block keeps
 * the ACTIVATED mask (cf_dcn_args.mask_activated = 1), which the backward kernels read. */
int cf_offmask_activate(float* offmask, long M, void* stream);
size_t cf_conv3x3_bwd_workspace_bytes(int B, int H, int W, int C);
int cf_conv3x3_bwd_weight(const float* gom, const float* offmask, const float* x, int B, int H, int W, int C, float* gw,
                          float* gbias, void* workspace, size_t workspace_bytes, void* stream);
int cf_conv3x3_bwd_data(const float* gom, const float* offmask, const float* weight, int B, int H, int W, int C, float* gx,
                        void* stream);

/* cf_bn_relu_train_forward: y = relu(gamma (x - mean) invstd + beta) on an [M][C] map (M = B*H*W rows; C a multiple of
 * 4, at most 1024).  training != 0: mean and the biased variance of the batch - per slab of rows the mean about a
 * pivot row and the sum of squares about that mean (two passes), the slabs merged in slab order in float64 - and
 * running_mean / running_var (either may be NULL) updated with `momentum`, the latter with the unbiased M / (M - 1)
 * variance; M = 1 is refused.  training == 0: mean / invstd of the running statistics.  save_mean / save_invstd [C]
 * are written for the backward.  cf_bn_relu_backward: from gy, the same x (the pre-BN map), gamma, beta and the saved
 * statistics: gz [M][C], ggamma [C], gbeta [C]; each may be NULL.  The ReLU mask is recomputed with the forward's own
 * expression.  The workspace of both is cf_bn_relu_workspace_bytes(M, C). */
size_t cf_bn_relu_workspace_bytes(long M, int C);
int cf_bn_relu_train_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             int training, float momentum, float eps, long M, int C, float* y, float* save_mean,
                             float* save_invstd, void* workspace, size_t workspace_bytes, void* stream);
int cf_bn_relu_backward(const float* gy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                        const float* save_invstd, int training, long M, int C, float* gz, float* ggamma, float* gbeta,
                        void* workspace, size_t workspace_bytes, void* stream);

/* cf_upsample_dw_bwd: backward of cf_upsample_dw for f = 2 or 4 (k = 2f).  gout [B][H*f][W*f][C]; gx [B][H][W][C] is
 * gathered from the k x k block of gout each input pixel fed; gweight in the packed [k][k][C] order (x is read for it
 * only).  Either output may be NULL.  The skip input's gradient is gout itself. */
size_t cf_upsample_dw_bwd_workspace_bytes(int B, int H, int W, int C, int f);
int cf_upsample_dw_bwd(const float* gout, const float* x, const float* weight, int B, int H, int W, int C, int f, float* gx,
                       float* gweight, void* workspace, size_t workspace_bytes, void* stream);

/* Training kernels of the DLA-34 base, levels 2-5 (added within ABI 7: nothing existing changed).  One block shape covers
 * them: convolution (no bias) -> BatchNorm -> [+ residual] -> [ReLU] (model/networks/dla.py:44-118, 121-161).  All
 * tensors fp32 NHWC; products through the exact fp32-input MFMA: no range to guard, nothing is clamped.  No float
 * atomics: every output is bitwise reproducible.
 *
 * Geometry of the two convolution kernels: k = 1 or 3, padding (k - 1) / 2, stride 1 or 2 (2 with k = 3 only),
 * Ho = (H + 2 pad - k) / stride + 1 (odd H, W are fine under stride 2); C and N multiples of 32, C <= 1280, N <= 512.
 * x [B][H][W][C] is the convolution's input, gz [B][Ho][Wo][N] the gradient of its output, weight the raw torch
 * [N][C][k][k] (no host packing on the backward path).
 * cf_conv_bwd_weight: gw [N][C][k][k].  The output pixels are split into slabs whose partial sums (workspace:
 * cf_conv_bwd_workspace_bytes(...)) a second launch adds in slab order.
 * cf_conv_bwd_data: gx [B][H][W][C], plain stores of every element (no accumulate-into form); each pixel row of gx is
 * owned by one workgroup.  Under stride 2 a workgroup's pixels share their row / column parity and its tap loop walks
 * the taps of that parity alone (no zero-stuffed gz). */
size_t cf_conv_bwd_workspace_bytes(int B, int H, int W, int C, int N, int k, int stride);
int cf_conv_bwd_weight(const float* gz, const float* x, int B, int H, int W, int C, int N, int k, int stride, float* gw,
                       void* workspace, size_t workspace_bytes, void* stream);
int cf_conv_bwd_data(const float* gz, const float* weight, int B, int H, int W, int C, int N, int k, int stride,
                     float* gx, void* stream);

/* cf_bn_act_train_forward: y = act(gamma (x - mean) invstd + beta [+ residual]) on an [M][C] map; residual NULL or
 * [M][C], relu 0 or 1 (act = ReLU or nothing).  Statistics, running-statistics update, the float64 slab merge and the
 * workspace are cf_bn_relu_train_forward's (the same kernels): with residual == NULL and relu == 1 the results equal
 * cf_bn_relu_* bit for bit.  cf_bn_act_backward: gz [M][C] (the pre-BN map's gradient), gres [M][C] (the residual's:
 * gy under the ReLU mask), ggamma [C], gbeta [C]; each may be NULL.  The ReLU mask is recomputed from the forward's
 * own expression, residual included; the per-channel sums are slab partials added in slab order. */
size_t cf_bn_act_workspace_bytes(long M, int C);
int cf_bn_act_train_forward(const float* x, const float* gamma, const float* beta, const float* residual, int relu,
                            float* running_mean, float* running_var, int training, float momentum, float eps, long M,
                            int C, float* y, float* save_mean, float* save_invstd, void* workspace,
                            size_t workspace_bytes, void* stream);
int cf_bn_act_backward(const float* gy, const float* x, const float* gamma, const float* beta, const float* residual,
                       int relu, const float* save_mean, const float* save_invstd, int training, long M, int C,
                       float* gz, float* gres, float* ggamma, float* gbeta, void* workspace, size_t workspace_bytes,
                       void* stream);

/* cf_maxpool2x2_bwd: backward of cf_maxpool2x2.  gout [B][H/2][W/2][C], x [B][H][W][C] the pooled map, gx [B][H][W][C]:
 * the whole gradient goes to the first maximum of each window in row-major order (what aten does on a tie); every
 * element of gx is written, zeros included.  C a multiple of 4; no workspace. */
int cf_maxpool2x2_bwd(const float* gout, const float* x, int B, int H, int W, int C, float* gx, void* stream);

/* Training kernels of the DLA-34 stem (added within ABI 7: nothing existing changed): the narrow convolutions of
 * base.base_layer (7x7, 3 or 6 -> 16), level0 (3x3, 16 -> 16) and level1 (3x3 stride 2, 16 -> 32), padding (k - 1) / 2,
 * no bias, exact fp32, no float atomics (bitwise reproducible), 64-bit element offsets.  BatchNorm + ReLU on top of them
 * are cf_bn_act_train_forward / cf_bn_act_backward (any C that is a multiple of 4).
 *
 * Geometry: k = 7 with stride 1 and Cin <= 8, or k = 3 with stride 1 or 2 and Cin = 16; Cout = 16 or 32;
 * Ho = (H + 2 pad - k) / stride + 1.  weight is the raw torch [Cout][Cin][k][k]; z and gz are [B][Ho][Wo][Cout] NHWC.
 * k = 7: x is the caller's NCHW image [B][Cin or Cin - 3][H][W]; radar NULL, or the [B][3][H/4][W/4] map that supplies
 * the last three input channels, sampled at (y >> 2, x >> 2) inside the kernel (H, W multiples of 4).  k = 3: x is
 * [B][H][W][16] NHWC and radar must be NULL.
 * cf_stem_conv_forward: z, the pre-BN map.
 * cf_stem_conv_bwd_weight: gw [Cout][Cin][k][k]; the output pixels are split into slabs whose partial sums (workspace:
 * cf_stem_conv_bwd_workspace_bytes(...), 0 for a geometry outside the family) a second launch adds in slab order.
 * cf_stem_conv_bwd_data: gx [B][H][W][16] of the 3x3 layers, plain stores of every element; under stride 2 a workgroup's
 * pixels share their row / column parity.  The 7x7 layer has no input gradient (k = 7 is refused). */
size_t cf_stem_conv_bwd_workspace_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride);
int cf_stem_conv_forward(const float* x, const float* radar, const float* weight, int B, int H, int W, int Cin, int Cout,
                         int k, int stride, float* z, void* stream);
int cf_stem_conv_bwd_weight(const float* gz, const float* x, const float* radar, int B, int H, int W, int Cin, int Cout,
                            int k, int stride, float* gw, void* workspace, size_t workspace_bytes, void* stream);
int cf_stem_conv_bwd_data(const float* gz, const float* weight, int B, int H, int W, int Cin, int Cout, int k, int stride,
                          float* gx, void* stream);

/* cf_upsample_dw: depthwise transposed conv (k = 2f, stride f, pad f/2, groups = C, no bias),
 * optionally fused with the IDA skip add:  out = convT(x) [+ skip].
 * replaces aten::conv_transpose2d + add of model/networks/dla.py:502-511, 518-524.
 * weight is repacked [k][k][C]; all tensors NHWC; output is (H*f, W*f). */
int cf_upsample_dw(const float* x, const float* weight, const float* skip, float* out, int B,
                   int H, int W, int C, int f, void* stream);

/* cf_maxpool2x2: 2x2 stride-2 max pooling, NHWC.  replaces aten::max_pool2d of dla.py:96,107. */
int cf_maxpool2x2(const float* x, float* out, int B, int H, int W, int C, void* stream);

/* cf_nchw_to_nhwc4: (B,3,H,W) NCHW image -> (B,H,W,4) NHWC with a zero 4th channel (stem input). */
int cf_nchw_to_nhwc4(const float* x, float* out, int B, int C, int H, int W, void* stream);

/* cf_nhwc_to_nchw: generic layout change used to hand NHWC intermediates back in NCHW. */
int cf_nhwc_to_nchw(const float* x, float* out, int B, int H, int W, int C, int c_stride,
                    void* stream);

/* cf_nchw_to_nhwc: (B,C,H,W) -> NHWC with `out_stride` floats per pixel, written at channel `out_offset`
 * (the other channels of the destination are left alone).  Entry side of the operator-level deform_conv2d
 * drop-in (ops.deform_conv2d: NCHW input / offset / mask of dla.py:461-470 -> the NHWC buffers of cf_dcn_v2_*). */
int cf_nchw_to_nhwc(const float* x, float* out, int B, int C, int H, int W, int out_stride, int out_offset,
                    void* stream);

/* cf_radar_ingest: raw radar sweeps -> what cf_pillar_expand consumes (detector.py:257-283,
 * datasets/nuscenes.py:171-199, utils/pointcloud.py:17-49): depth <= max_dist
 * (if > 0), y -= z_offset, pinhole projection with the 3x3 intrinsic and division by the projected z,
 * keep depth > 0 and 1 < u < img_w - 1 and 1 < v < img_h - 1, order by depth (ties: original index;
 * descending = exact reverse).  pc (B, n_rows, max_n) f64 padded sweeps with counts_in (B) points each
 * (rows 0..2 = x, y, z in the camera frame); intrinsics (B, 3, 3) f64.  Outputs: pc_2d (B, 3, max_n)
 * [u, v, depth], pc_3d (B, n_rows, max_n) (row 1 carries the offset y), counts_out (B); padding zeroed. */
int cf_radar_ingest(const double* pc, const int32_t* counts_in, int B, int n_rows, int max_n,
                    const double* intrinsics, int img_w, int img_h, double max_dist, double z_offset,
                    int descending, double* pc_2d, double* pc_3d, int32_t* counts_out, void* stream);

/* cf_preprocess_images: the image side of Detector.pre_process (detector.py:226-234; SURVEY §8(f)
 * rank 2): cv2.warpAffine(INTER_LINEAR, border 0) of uint8 HWC camera frames to the network input
 * size in OpenCV's fixed-point arithmetic, ((v / 255 - mean) / std) evaluated in float64, fp32 NCHW out.
 * src (B, Hs, Ws, 3) uint8 on the device; map_dst_to_src, mean, stdv: HOST pointers (six doubles: the
 * already inverted 2x3 matrix, as cv::warpAffine forms it; three floats each). */
int cf_preprocess_images(const uint8_t* src, int B, int Hs, int Ws, const double* map_dst_to_src,
                         const float* mean, const float* stdv, int Hd, int Wd, float* out, void* stream);

/* cf_augment_images: the image side of a TRAINING item (dataset/generic_dataset.py:159-190, 414-439): per frame
 *   1. v = the 8-bit cv2.warpAffine(INTER_LINEAR, border 0) of cf_preprocess_images, with frame b's own dst -> src map; with
 *      flip[b] != 0 the source is read as img[:, ::-1, :] (the tap column j is fetched from stored column Ws-1-j; coordinates,
 *      weights and the validity test are unchanged);
 *   2. t = (float)v / 255.0f;
 *   3. if `colour`: for k in order[b] (0 brightness, 1 contrast, 2 saturation: the reference's ColorJitter list), with
 *      r = factor[b][k], q = (float)(1.0 - (double)r), blend(a, o) = clamp(r*a + q*o, 0, 1) (mul, mul, add, each rounded):
 *      brightness t = blend(t, 0); saturation t = blend(t, g), g = (0.2989f*t0 + 0.587f*t1) + 0.114f*t2 of this pixel (the
 *      channels in stored order, no reordering: cv2.imread leaves BGR and ToTensor keeps it); contrast t = blend(t, m), m = the
 *      mean of g over all Hd*Wd pixels of the frame as they stand at that point (border zeros included), summed in float64 in
 *      a fixed order and rounded once to fp32.  Then t += lighting[b][c], unclamped;
 *   4. out = (t - mean[c]) / std[c] in fp32 (the dataset's fp32 path, not cf_preprocess_images' float64 one).
 * src (B,Hs,Ws,3) uint8, map_dst_to_src (B,6) f64, flip (B) u8 (a torch.bool tensor), order (B,3) i32, factor (B,3) f32, lighting (B,3) f32: DEVICE;
 * order / factor / lighting may be NULL without `colour`.  mean, stdv: HOST pointers, three floats.  out (B,3,Hd,Wd) f32.
 * With `colour` the caller hands in cf_augment_workspace_bytes(B, Hd, Wd) bytes of device memory, 8-byte aligned (per-block
 * partial sums and the warped bytes); without it workspace may be NULL.  Two launches with colour, one without; no allocation,
 * no host synchronisation, no atomics: the same input gives the same bits on every run and in every batch.
 * Limits (refused with CF_EINVAL): every size < 32768, B * ceil(Hd*Wd / 1024) <= 2^31 - 1, std[c] != 0.  An `order` entry
 * outside 0..2 is skipped (the Python side validates the table on the host). */
size_t cf_augment_workspace_bytes(int B, int Hd, int Wd);
int cf_augment_images(const uint8_t* src, int B, int Hs, int Ws, const double* map_dst_to_src, const uint8_t* flip,
                      const int32_t* order, const float* factor, const float* lighting, const float* mean, const float* stdv,
                      int colour, int Hd, int Wd, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* cf_topk_peaks: per-image top-K over a (B,C,H,W) NCHW score map, optionally after the 3x3
 * equality NMS, ordered by (score desc, class asc, pixel asc).
 * replaces model/utils.py:6-38 (topk) [+ model/utils.py:112-128 (nms) when nms != 0].
 * outputs: scores (B,K) f32, inds (B,K) i32 pixel index in [0,H*W), classes (B,K) i32.
 * workspace: cf_topk_workspace_bytes(B, K) bytes of device memory (per-slice candidate keys). */
size_t cf_topk_workspace_bytes(int B, int K);
/* nms == 2: the same result as nms == 1, but the suppressed map is first written by its own fully
 * parallel pass into scratch memory behind the keys - workspace must then hold
 * cf_topk_workspace_bytes_nms(B, C, H, W, K) bytes.  (nms == 1 suppresses on the fly, no scratch.) */
size_t cf_topk_workspace_bytes_nms(int B, int C, int H, int W, int K);
/* (ABI 6) cf_checksum64: a position-weighted checksum of a device buffer read as 32-bit words, as CF_CHECKSUM_PARTS partial sums
 * over a fixed partition of the words: parts[b] = sum of word[i] * w(i) mod 2^64, w(i) = ((uint32)i * 2654435761) | 1 (exact
 * integer arithmetic: the same bits give the same parts; one launch, no atomics, nothing to zero).
 * cf_topk_peaks_if_changed: the guard of peaks computed earlier - sums = [expected parts | actual parts] (2 x
 * CF_CHECKSUM_PARTS words in device memory, compared ON THE DEVICE: no host sync).  All equal: the launch does nothing and
 * scores / inds / classes keep what they hold.  Any part differs: it computes cf_topk_peaks(heat, nms) into them - one
 * workgroup per image, ~0.3 ms: the rare path.  nms = 1 or 2 (same result); workspace: cf_topk_workspace_bytes(B, K) bytes.
 * Together they let the host keep the peaks the forward computed beside its own launches (model.py: heads_lanes) and still
 * honour ANY later change of the heat map - also one made through `tensor.data`, which no version counter sees - as the
 * reference's fusionDecode would (model/decode.py:38-57: it always reads the map it is given).  No reference counterpart. */
#define CF_CHECKSUM_PARTS 256
int cf_checksum64(const void* x, long n_words, unsigned long long* parts, void* stream);
int cf_topk_peaks_if_changed(const float* heat, int B, int C, int H, int W, int K, int nms, float* scores, int32_t* inds,
                             int32_t* classes, void* workspace, const unsigned long long* sums, void* stream);
int cf_topk_peaks(const float* heat, int B, int C, int H, int W, int K, int nms, float* scores,
                  int32_t* inds, int32_t* classes, void* workspace, void* stream);
/* (added under ABI 7) cf_topk_peaks_fused: the index pass of a forward whose heads run at the peaks, in TWO launches: the
 * NMS'd peaks of cf_topk_peaks(heat, nms = 2) in scores / inds / classes and - optional, all three or none - the raw peaks of
 * cf_topk_peaks(heat, nms = 0) in raw_scores / raw_inds / raw_classes, both from one read of the map (the 3x3 equality NMS is
 * applied inside the slice kernel: no suppressed map), one merge launch for both - which also writes, if not NULL, the
 * tables cf_head_slot_tables(raw_inds, inds, B, K, H * W, table_ab, table_b) would write (same shapes, same entries; without
 * the raw peaks table_ab holds -1 where they would stand).  Bit for bit the results of those calls.  Maps whose slices do not
 * fit the register-cached kernel (more than 16 x 16,384 elements per image) take cf_topk_peaks' own slice passes in front of
 * the one merge.  workspace: cf_topk_peaks_fused_workspace_bytes(B, C, H, W, K) bytes.  Meant for a stream with nothing
 * beside it: its 1024-thread workgroups do not fit next to a head launch's. */
size_t cf_topk_peaks_fused_workspace_bytes(int B, int C, int H, int W, int K);
int cf_topk_peaks_fused(const float* heat, int B, int C, int H, int W, int K, float* raw_scores, int32_t* raw_inds,
                        int32_t* raw_classes, float* scores, int32_t* inds, int32_t* classes, int32_t* table_ab,
                        int32_t* table_b, void* workspace, void* stream);

/* cf_frustum_assoc: radar frustum association for K peaks per image.
 * replaces utils/pointcloud.py:331-394 (getPcFrustumHeatmap, after its topk) and 397-481
 * (cvtPcDepthToHeatmap) incl. get_alpha / cvtAlphaToYaw / get3DCorners / getDistanceThresh
 * (pointcloud.py:195-328).  All maps NCHW fp32.  pc_hm (B,3,H,W) is fully written (zero where
 * nothing is painted); pc_hm_nhwc4 (B,H,W,4) fp32 and pc_hm_split8 (B,H,W,2,8) split-bf16, if not
 * NULL, receive the same data channels-last for the secondary-head convolution. */
int cf_frustum_assoc(const int32_t* inds, int K, const float* depth, const float* wh,
                     const float* dim, const float* rot, const float* calib, const float* pc_dep,
                     int B, int H, int W, float max_pc_dist, float* pc_hm, float* pc_hm_nhwc4,
                     void* pc_hm_split8, void* stream);

/* (ABI 6) cf_topk_frustum: cf_topk_peaks(heat, nms = 0) followed by cf_frustum_assoc on its peaks - the chain between the
 * primary and the secondary head launches (utils/pointcloud.py:347-392: topk of the un-NMS'd heat map, then the association
 * loop) - as TWO launches instead of three: the slice top-K, then the association kernel, which merges the slices' sorted
 * lists in its prologue.  heat (B,C,H,W); workspace: cf_topk_workspace_bytes(B, K) bytes; scores / inds / classes (B,K):
 * optional (all three or none) - the peaks as cf_topk_peaks would return them.  Same results as the two calls, bit for bit. */
int cf_topk_frustum(const float* heat, int C, int K, const float* depth, const float* wh, const float* dim,
                    const float* rot, const float* calib, const float* pc_dep, int B, int H, int W, float max_pc_dist,
                    float* pc_hm, float* pc_hm_nhwc4, void* pc_hm_split8, float* scores, int32_t* inds, int32_t* classes,
                    void* workspace, void* stream);

/* cf_pc_hm_direct: middle fusion WITHOUT frustum association (MODEL.FRUSTUM = False): the radar map itself is the
 * secondary heads' pc_hm.  replaces model/networks/base_model.py:69-79 (the in-place normalisation of the caller's pc_dep).
 * pc_dep (B,3,H,W) fp32 NCHW: channel 0 is rewritten IN PLACE as 1 - x / max_pc_dist (fp32 division, then the subtraction:
 * an empty pixel becomes 1.0), channels 1 and 2 are read only.  pc_hm_nhwc4 (B,H,W,4) fp32 and pc_hm_split8 (B,H,W,2,8)
 * split-bf16, if not NULL (16-byte aligned), receive the three channels channels-last as cf_frustum_assoc writes them.  One pass. */
int cf_pc_hm_direct(float* pc_dep, int B, int H, int W, float max_pc_dist, float* pc_hm_nhwc4, void* pc_hm_split8,
                    void* stream);

/* cf_pillar_expand: radar points -> pc_dep (B,3,H,W) by pillar expansion (fp64 geometry).
 * replaces dataset/generic_dataset.py:738-942 (processPointCloud / transformPointCloud /
 * getPcPillarsSize) + dataset/datasets/nuscenes.py:221-263 (getDepthMap / drawPcHeat).
 * pc_2d: (B, 3, max_n) f64 [u, v, depth] in source-image pixels, depth-ascending per frame;
 * pc_3d: (B, n_rows>=10, max_n) f64 camera-frame radar rows (row 8 = vx, row 9 = vz);
 * counts: (B) i32 valid points per frame; calib (B,3,4) f64; trans (B,2,3) f64 (source image ->
 * output map affine); pillar = (h, w, l) metres.  keep_mask (B,max_n) u8 and xy_out (B,2,max_n)
 * f64 may be NULL; they receive the transformPointCloud filter mask / transformed coordinates. */
int cf_pillar_expand(const double* pc_2d, const double* pc_3d, const int32_t* counts, int B,
                     int max_n, int n_rows, const double* calib, const double* trans, int H, int W,
                     double pillar_h, double pillar_w, double pillar_l, float* pc_dep,
                     uint8_t* keep_mask, double* xy_out, void* stream);

/* cf_radar_roi_expand: cf_pillar_expand's inputs and outputs for the other two DATASET.PC_ROI_METHOD values.
 * method 1 = "points": replaces dataset/datasets/nuscenes.py:265-294 (drawPcPoints) - one pixel per kept point at the
 *   truncated transformed coordinates; of several points on one pixel the last in order stays.
 * method 2 = "heatmap": replaces dataset/generic_dataset.py:811-818 + utils/image.py:145-176 (getGaussianRadius, float64):
 *   the square of radius int(gaussian_radius(250 / depth + 5)) around the truncated centre, clipped to the map; painted
 *   in point order (later points overwrite earlier ones), as for pillars. */
int cf_radar_roi_expand(const double* pc_2d, const double* pc_3d, const int32_t* counts, int B, int max_n,
                        int n_rows, const double* calib, const double* trans, int H, int W, int method,
                        float* pc_dep, uint8_t* keep_mask, double* xy_out, void* stream);

/* cf_decode_gather: from K (index, class, score) peaks produce the 33-float detection rows of
 * model/decode.py:10-174 (fusionDecode): [score, classId, cx_n, cy_n, x1, y1, x2, y2, rot8, dim3,
 * amodal2, att8, vel3, depth].  Any map pointer may be NULL (its columns are zero-filled; reg NULL
 * means the +0.5 centre of decode.py:139-141).  det: (B,K,33) f32. */
typedef struct cf_decode_args {
  const float* scores;  /* (B,K) */
  const int32_t* inds;  /* (B,K) */
  const int32_t* classes;
  const float *reg, *wh, *depth, *rot, *dim, *amodal, *att, *vel; /* NCHW maps */
  int32_t B, K, H, W;
  int32_t out_h, out_w; /* outputSize */
  int32_t norm2d;
  float* det;           /* (B,K,33) */
} cf_decode_args;
int cf_decode_gather(const cf_decode_args* a, void* stream);

/* cf_post_process: 2D -> 3D post-processing of decoded detections, replaces utils/postProcess.py:13-85
 * (+ utils/ddd.py:8-23,122-199, utils/pointcloud.py:195-296) for the inference case.
 * det (B,K,33) as written by cf_decode_gather; calib (B,3,4) f32; trans_inv (2,3) f32 device = the
 * output-map -> source-image affine (getAffineTransform(..., inverse=True)); out (B,K,54) f32:
 * [score, classId+1, centre xy (source px), bbox x1 y1 x2 y2 (source px), depth, alpha, dim hwl,
 *  amodal_offset xy, nuscenes_att 8, velocity 3 (re-projected on the heading), location xyz, yaw,
 *  8 box corners xyz (all zero when a dimension is <= 0)]. */
int cf_post_process(const float* det, const float* calib, const float* trans_inv, int B, int K,
                    int out_h, int out_w, float* out, void* stream);

/* cf_decode_post: cf_decode_gather and cf_post_process in ONE launch (the 33-float row never leaves
 * registers): model/decode.py:10-174 followed by utils/postProcess.py:13-85, as Detector.process +
 * Detector.post_process chain them (detector.py:343-349, 397-426) and as the evaluation loop does
 * (model/progressBar.py:95-110).  post (B,K,54) as cf_post_process writes it; a->det (B,K,33) is
 * optional (NULL: only the final rows).  Bit-identical to the two separate calls. */
int cf_decode_post(const cf_decode_args* a, const float* calib, const float* trans_inv, float* post,
                   void* stream);

/* cf_decode_gather_unc / cf_decode_post_unc: cf_decode_gather / cf_decode_post for a model with the `uncertainty`
 * head (TRAIN.UNCERTAINTY_LOSS: config/utils.py:100-102).  uncertainty: the head's (B,1,H,W) f32 NCHW map.  The score
 * written to column 0 of the (B,K,33) and (B,K,54) rows is score * exp(-exp(u)) with u read at the peak pixel
 * (model/decode.py:80-85; precise expf, fp32).  a->scores is only read and the rows keep the order of the K peaks (the
 * reference does not sort again either); every other column is what the plain call writes.  The plain calls ARE these
 * kernels with a NULL map. */
int cf_decode_gather_unc(const cf_decode_args* a, const float* uncertainty, void* stream);
int cf_decode_post_unc(const cf_decode_args* a, const float* uncertainty, const float* calib, const float* trans_inv,
                       float* post, void* stream);

/* cf_depth_maps: the normalised uint8 maps of Detector.post_process (detector.py:381-393; `ret["depthmaps"]` of
 * Detector.run) for n_maps (<= CF_DEPTH_MAPS_MAX) maps of one batch in ONE launch.  maps: HOST array of n_maps device
 * pointers, each a (B,1,H,W) f32 map whose images are contiguous H*W planes batch_strides[m] floats apart (HOST array; NULL:
 * H*W - a channel-0 view of a (B,C,H,W) tensor passes C*H*W); out (n_maps,B,H,W) uint8.  Per image: row 0 and column 0 of image 0 (only) count
 * as 0, then ((x - min) / (max - min)) * 255 truncated, each operation rounded in fp32 - numpy's bytes.  A flat image
 * (0 / 0, whose cast numpy leaves undefined) gives 0. */
#define CF_DEPTH_MAPS_MAX 8
int cf_depth_maps(const float* const* maps, const long* batch_strides, int n_maps, int B, int H, int W, uint8_t* out,
                  void* stream);

/* cf_serialize_nuscenes: post-processed detections -> the numeric content of the nuScenes result
 * file, replaces dataset/datasets/nuscenes.py:416-482 (getEvalFormatItem) and the per-sample merge +
 * top-500 of nuscenes.py:536-553 (convert_eval_format); SURVEY §8(f) rank 4.
 *   rows (B*K, 12) f32: [translation xyz = trans_matrix @ (location - (0, h, 0), 1), size (w, l, h),
 *                        velocity xy = (velocity_matrix @ (v, 0))[:2], score, class index 0..9,
 *                        attribute id 0..8 (0 = ""), keep = score > -1 && all dimensions > 0]
 *   rotation (B*K, 4) f64 (optional): pose_rot * cs_rot * R_y(yaw), (w, x, y, z); NULL cs/pose: R_y(yaw)
 *   order (n_samples, max_per_sample) i32: row indices (b*K + k) of each sample's best rows, best first,
 *     -1 padded; counts (n_samples).  A sample's frames are sample_frames[sample_ptr[s] .. sample_ptr[s+1])
 *     in image order (CSR); at most cf_serialize_max_candidates() kept rows per sample take part.
 * The strings of the file (sample_token, detection_name, attribute_name) are joined on the host. */
typedef struct cf_serialize_args {
  const float* post;             /* (B,K,54) from cf_post_process / cf_decode_post                */
  int32_t B, K;
  const float* trans_matrix;     /* (B,4,4) f32 camera -> global (image_info["trans_matrix"])     */
  const float* velocity_matrix;  /* (B,4,4) f32 (image_info["velocity_trans_matrix"])             */
  const double* cs_rot;          /* (B,4) f64 calibrated-sensor quaternion, or NULL               */
  const double* pose_rot;        /* (B,4) f64 ego-pose quaternion, or NULL                        */
  float* rows;                   /* (B*K,12)                                                      */
  double* rotation;              /* (B*K,4) or NULL                                               */
  int32_t n_samples;             /* 0: rows only                                                  */
  const int32_t* sample_ptr;     /* (n_samples+1)                                                 */
  const int32_t* sample_frames;  /* (sample_ptr[n_samples]) frame indices                         */
  int32_t max_per_sample;        /* 500 in the reference                                          */
  int32_t* order;                /* (n_samples, max_per_sample)                                   */
  int32_t* counts;               /* (n_samples)                                                   */
} cf_serialize_args;
int cf_serialize_nuscenes(const cf_serialize_args* a, void* stream);
int cf_serialize_max_candidates(void);

/* The criterion: GenericLoss of model/genericLoss.py over one output layer, forward and backward, with no host sync
 * (added within ABI 7: nothing existing changed).  replaces: the ~1,300 aten calls and ~20 device-to-host branches of
 * genericLoss.py:60-302 + losses.py (FastFocalLoss, RegWeightedL1Loss, BinRotLoss, WeightedBCELoss,
 * UncertaintyDepthLoss) behind modelWithLoss.py:43-55.  Every map is fp32 NCHW, read in place (no NHWC copy).
 *
 * Per object row r = b*M + m:  layer mask lm = (wh[r][0] * wh[r][1]) / out_area > 0; where lm is false every per-object
 * field counts as 0 (pixel 0, mask 0, class 0, targets 0, rotbin 0, attribute mask 0).  Pixel = int(cy) * w + int(cx) from
 * `centers`, CLAMPED into [0, h*w) (the reference raises on a centre outside the map).
 *
 * Head kinds (value = what goes into `losses`; the total adds weight * value unless stated):
 *   CF_LOSS_L1      sum_c |pred*m - target*m| / (channels * sum m)            (divisor 1e7 when sum m == 0)
 *   CF_LOSS_L1_UNC  one channel; u = clamp(unc, -10, 10) at the pixel; value = mean of |d| over the rows with m != 0; the
 *                   TOTAL takes mean of (|d| e^-u + u) over those rows instead (over all B*M rows when none has m != 0)
 *   CF_LOSS_BINROT  eight channels; two 2-way cross-entropies averaged over the rows with m != 0, plus smooth-L1 on
 *                   (sin, cos) of rotres averaged over the rows with rotbin[k] != 0 whatever their m; 0 when sum m == 0
 *   CF_LOSS_BCE     sum mask * bce_with_logits(pred, target) / sum mask        (divisor 1e7 when sum mask == 0)
 * The heat-map term is FastFocalLoss: -(pos + neg) / sum m, or -neg when sum m == 0. */
#define CF_LOSS_MAX_HEADS 16
#define CF_LOSS_L1 0
#define CF_LOSS_L1_UNC 1
#define CF_LOSS_BINROT 2
#define CF_LOSS_BCE 3
#define CF_LOSS_STATS (4 + 4 * CF_LOSS_MAX_HEADS) /* floats in cf_loss_args.stats */

typedef struct cf_loss_head {
  int32_t kind;          /* CF_LOSS_*                                                                          */
  int32_t channels;      /* L1_UNC: 1, BINROT: 8                                                               */
  const float* map;      /* [B][channels][h][w]                                                                */
  const float* target;   /* [B][M][channels]; BINROT: rotres [B][M][2]                                         */
  const float* mask;     /* BCE: [B][M][channels]; the other kinds use cf_loss_args.mask                       */
  const int64_t* rotbin; /* BINROT: [B][M][2]                                                                  */
  const float* unc;      /* L1_UNC: the uncertainty map [B][1][h][w]                                           */
  float weight;          /* of this term in the total                                                          */
  float* gmap;           /* backward: gradient of `map`, ZEROED by the caller (float atomics add into it), or NULL */
  float* gunc;           /* backward, L1_UNC: gradient of `unc`, zeroed by the caller (heads may share it), or NULL */
} cf_loss_head;

typedef struct cf_loss_args {
  const float* heat;     /* [B][C][h][w] probabilities (after the clamped sigmoid)                             */
  const float* heat_gt;  /* [B][C][h][w]                                                                       */
  const float* centers;  /* [B][M][2] (x, y) on the output map                                                 */
  const float* wh;       /* [B][M][2]: the layer mask comes from its product                                   */
  const float* mask;     /* [B][M]                                                                             */
  const int64_t* cls;    /* [B][M], clamped into [0, C)                                                        */
  int32_t B, C, h, w, M;
  int32_t n_heads;       /* <= CF_LOSS_MAX_HEADS                                                               */
  float out_area;        /* MODEL.OUTPUT_SIZE[0] * MODEL.OUTPUT_SIZE[1]                                        */
  float heat_weight;
  cf_loss_head head[CF_LOSS_MAX_HEADS];
  float* losses;         /* forward out [n_heads + 3]: heat-map term, head 0 .. n_heads-1, total, 0.0          */
  float* total;          /* forward out: the total once more, in a buffer of its own; may be NULL             */
  uint8_t* layer_mask;   /* forward out [B][M]: lm as 0 / 1; may be NULL                                       */
  float* stats;          /* [CF_LOSS_STATS]: counts and normalisers, written by forward, read by backward      */
  void* workspace;       /* forward: cf_loss_workspace_bytes(...) bytes (the per-workgroup partial sums)       */
  size_t workspace_bytes;
  const float* grad_out; /* backward: ONE float on the device, the gradient arriving at the total              */
  float* gheat;          /* backward: gradient of `heat`, every element written (no zeroing needed), or NULL   */
} cf_loss_args;
/* Two launches: a grid-stride pass over heat / heat_gt (16-byte loads when both are 16-byte aligned) that leaves one
 * partial sum per workgroup in `workspace`, then one workgroup over the B*M objects that gathers every head's prediction,
 * adds the partials in a fixed order, resolves the zero-count branches on the device and writes losses / total / stats.
 * No float atomics, no memset: the values are bitwise reproducible from call to call. */
int cf_loss_forward(const cf_loss_args* a, void* stream);
/* Up to two launches: a dense pass that writes gheat from heat, heat_gt and stats, then a pass over the objects that
 * adds the positive focal terms into gheat and scatters each head's gradient into gmap / gunc with float atomic adds
 * (<= B*M*(sum channels + 1) adds; a pixel hit by three or more objects may differ in its last bits from run to run).
 * Everything is scaled by *grad_out.  Outputs that are NULL are skipped; with all of them NULL nothing is launched. */
int cf_loss_backward(const cf_loss_args* a, void* stream);
size_t cf_loss_workspace_bytes(int B, int C, int h, int w);

/* Training path of ONE detection head on a frozen trunk (csrc/cf_heads_bwd.hip; added under ABI 7; replaces torch autograd over
 * the nn.Sequential of detectHeads.py:59-98): conv3x3(Cin -> 256) + bias -> ReLU -> [conv1x1(256 -> 256) + bias -> ReLU] x
 * n_hidden -> conv1x1(256 -> n_out) + bias, from the RAW fp32 weights, exact fp32-input MFMA products, fp32 accumulation.
 * Cin = c_x + c_x2: the channels of `x` followed by those of the optional second source `x2` (the radar channels of the secondary
 * heads: the concatenation is never materialised).  The hidden maps are not kept: both directions work through a list of pixels in
 * chunks of `chunk_px` rows held in the workspace, and the backward recomputes the hidden maps with the forward's own kernel (its
 * ReLU mask is the forward's bit for bit; ReLU'(0) = 0).  The gradient with respect to x / x2 is produced by cf_head_backward_dx
 * only; cf_head_backward serves a frozen trunk and does nothing for it. */
#define CF_HEAD_TRAIN_MAX_HIDDEN 2
typedef struct cf_head_train_args {
  const float* x;        /* NHWC [B][h][w][x_stride], channels 0 .. c_x-1 read                                     */
  const float* x2;       /* NHWC [B][h][w][x2_stride], channels 0 .. c_x2-1 read; NULL with c_x2 = 0               */
  int32_t x_stride, c_x, x2_stride, c_x2;
  int32_t B, h, w;
  int32_t n_hidden;      /* 1x1 hidden layers, 0 .. CF_HEAD_TRAIN_MAX_HIDDEN                                       */
  int32_t hidden;        /* width of every hidden map: 256                                                         */
  int32_t n_out;         /* 1 .. 16                                                                                */
  int32_t chunk_px;      /* list positions per chunk, a multiple of 64; 0 = the default (32768), capped by B*h*w   */
  const float* weight[CF_HEAD_TRAIN_MAX_HIDDEN + 2]; /* raw torch layouts in layer order: [256][Cin][3][3], [256][256].., [n_out][256] */
  const float* bias[CF_HEAD_TRAIN_MAX_HIDDEN + 2];
  float* y;              /* forward out: NCHW [B][n_out][h][w], every element written                              */
  const float* gy;       /* backward in: NCHW [B][n_out][h][w], arbitrary                                          */
  float* gw[CF_HEAD_TRAIN_MAX_HIDDEN + 2];      /* backward out, in w's layouts; zeroed by the call                */
  float* gb[CF_HEAD_TRAIN_MAX_HIDDEN + 2];
  void* workspace;       /* 16-byte aligned; cf_head_train_workspace_bytes / cf_head_bwd_workspace_bytes           */
  size_t workspace_bytes;
} cf_head_train_args;
/* 2 + n_hidden launches per chunk of the B*h*w pixels behind one weight re-layout per layer; bitwise reproducible. */
int cf_head_train_forward(const cf_head_train_args* a, void* stream);
/* A first pass compacts the pixels where any channel of gy is non-zero (a NaN counts) into a device-side list + count; the
 * recompute, the chain and the weight-gradient launches then run per chunk of that list - grids come from the shapes, the work
 * loops read the count, the host never waits; chunks behind the end of the list cost an empty launch each.  An all-zero gy gives
 * exact zeros.  gw / gb are summed with float atomics and the list order comes from an atomic counter: the last bits can differ
 * from run to run. */
int cf_head_backward(const cf_head_train_args* a, void* stream);
size_t cf_head_train_workspace_bytes(int B, int h, int w, int Cin, int n_hidden, int chunk_px);
size_t cf_head_bwd_workspace_bytes(int B, int h, int w, int Cin, int n_hidden, int chunk_px);
/* the chunk length those calls use for this geometry and chunk_px (0: the default) */
int cf_head_bwd_chunk_px(int B, int h, int w, int chunk_px);
/* cf_head_backward - the same checks, launches, gw and gb - plus the gradient of the sources (added under ABI 7, nothing existing
 * changed): gx NHWC [B][h][w][gx_stride >= c_x] takes the columns of x, gx2 NHWC [B][h][w][gx2_stride >= c_x2] those of x2; either
 * may be NULL (its columns are skipped), both NULL is CF_ERR_ARG, as are a stride below the channel count and gx2 without x2.
 *   dX[b][y][x][c] = sum over taps (dy,dx) and o < 256 of G0[b][y-dy][x-dx][o] * W0[o][c][1+dy][1+dx]
 * with G0 the masked gradient of the first layer's pre-activation.  The call zeroes gx / gx2 whole (padding channels included),
 * once; one launch per chunk of the list then scatters 32 positions x 32 channels per wave to the nine neighbours of each pixel
 * with float atomics (neighbours outside the image receive nothing): like gw / gb, the last bits can differ from run to run; an
 * all-zero gy gives exact zeros.  The workspace holds a second packed copy of W0 behind cf_head_backward's regions. */
int cf_head_backward_dx(const cf_head_train_args* a, float* gx, int gx_stride, float* gx2, int gx2_stride, void* stream);
size_t cf_head_bwd_dx_workspace_bytes(int B, int h, int w, int Cin, int n_hidden, int chunk_px);

/* Training targets: the collated batch of the reference's dataset for B images, built on the device from packed annotation
 * tables (csrc/cf_targets.hip; added under ABI 7, nothing existing changed).  replaces: the loop over annotations of
 * dataset/generic_dataset.py:206-228, initReturn / transformBbox / addInstance / processAlpha (generic_dataset.py:441-708),
 * nuScenes.initReturn (dataset/datasets/nuscenes.py:348-391), getGaussianRadius / getGaussianMatrix / ellip_gaussian2D /
 * drawGaussianHeatRegion (utils/image.py:145-256), get3dBox (utils/ddd.py:8-23), and, on numpy inputs, cvtAlphaToYaw /
 * get3DCorners / getDistanceThresh / cvtPcDepthToHeatmap (utils/pointcloud.py:214-328, 397-481).  One pyramid layer.
 *
 * Arithmetic follows numpy's dtypes operation by operation (float64 where numpy promotes, fp32 where it stores; a Python
 * scalar next to an fp32 value stays fp32).  Rows are indexed by annotation: a skipped annotation (class id > C or <= -999,
 * height or width <= 0 after the clip, index >= counts[b]) leaves a zero row.  Every element of every output is written; no
 * output needs zeroing.  Optional outputs may be NULL (a head the configuration lacks). */
#define CF_TARGETS_MAX_OBJS 128
#define CF_TARGETS_F 20        /* float64 per annotation, see cf_targets_args.ann                                       */
#define CF_TARGETS_DESC_BYTES 112 /* workspace bytes per (image, annotation)                                            */
/* presence bits of the optional annotation keys (iann[..][2]) */
#define CF_TARGETS_HAS_AMODAL 1
#define CF_TARGETS_HAS_ATTRIBUTES 2
#define CF_TARGETS_HAS_VELOCITY 4
#define CF_TARGETS_HAS_ALPHA 8
#define CF_TARGETS_HAS_DEPTH 16
#define CF_TARGETS_HAS_DIMENSION 32
#define CF_TARGETS_HAS_LOCATION 64
#define CF_TARGETS_HAS_YAW 128
/* cf_targets_args.flags */
#define CF_TARGETS_REP3D 1       /* DATASET.HEATMAP_REP == "3d" (generic_dataset.py:581-588)                            */
#define CF_TARGETS_NORM2D 2      /* MODEL.NORM_2D (generic_dataset.py:621-629)                                          */
#define CF_TARGETS_WRITE_DEPTH 4 /* "depth" or "depth2" among the heads (generic_dataset.py:660)                        */
#define CF_TARGETS_WRITE_ROT 8   /* "rotation" among the heads (generic_dataset.py:647)                                 */
#define CF_TARGETS_FRUSTUM 16    /* DATASET.RADAR_PC and MODEL.FRUSTUM (generic_dataset.py:673-687)                     */

typedef struct cf_targets_args {
  const double* ann;     /* [B][M][CF_TARGETS_F]: bbox x, y, w, h (source pixels) | truncated | amodal_center x, y |
                            velocity_cam[0..2], min(velocity_cam) | alpha | depth | dimension h, w, l | location x, y, z |
                            yaw; an absent key is 0 with its presence bit clear                                        */
  const int32_t* iann;   /* [B][M][3]: class id after the class map (1-based), attributes, presence bits              */
  const int32_t* counts; /* [B]: annotations of the image that are looked at (<= M)                                    */
  const double* trans;   /* [B][2][3]: source image -> output map (generic_dataset.py:182-187)                         */
  const float* calib;    /* [B][3][4]; FRUSTUM only                                                                    */
  const double* scale;   /* [B]: the augmentation's scale factor (depth * scale, generic_dataset.py:661)               */
  const float* pc_dep;   /* [B][3][h][w] radar map, read only; FRUSTUM only                                            */
  int32_t B, M, C, h, w; /* M <= CF_TARGETS_MAX_OBJS; (h, w) = MODEL.OUTPUT_SIZE                                       */
  int32_t flags;         /* CF_TARGETS_*                                                                               */
  float max_pc_dist;     /* DATASET.MAX_PC_DIST; FRUSTUM only                                                          */
  float* heat;           /* [B][C][h][w]  heatmap0                                                                     */
  int64_t* cls;          /* [B][M]        classIds (zero-based)                                                        */
  float* mask;           /* [B][M]                                                                                     */
  float* trunc_mask;     /* [B][M]                                                                                     */
  float* wh;             /* [B][M][2]     widthHeight                                                                  */
  float* reg;            /* [B][M][2]     or NULL                                                                      */
  float* amodal_offset;  /* [B][M][2]     or NULL                                                                      */
  float* dimension;      /* [B][M][3]     or NULL                                                                      */
  float* depth;          /* [B][M][1]     or NULL                                                                      */
  int64_t* rotbin;       /* [B][M][2]     or NULL; rotbin, rotres and t_rotation come together                         */
  float* rotres;         /* [B][M][2]                                                                                  */
  float* att;            /* [B][M][8]     nuscenes_att, or NULL; att and att_mask come together                        */
  float* att_mask;       /* [B][M][8]     nuscenes_att_mask                                                            */
  float* velocity;       /* [B][M][3]     or NULL                                                                      */
  float* pc_hm;          /* [B][3][h][w]  FRUSTUM only: zero where no box paints                                       */
  float* t_bboxes;       /* [B][M][4]     target.bboxes (x1, y1, x2, y2 on the output map)                             */
  float* t_scores;       /* [B][M]        target.scores: zeros, as the reference leaves them                           */
  float* t_centers;      /* [B][M][2]     target.centers                                                               */
  float* t_heat_centers; /* [B][M][2]     target.heatCenters                                                           */
  float* t_bboxes3d;     /* [B][M][8][3]  target.bboxes3d                                                              */
  float* t_rotation;     /* [B][M][8]     target.rotation, or NULL                                                     */
  float* t_att;          /* [B][M][8]     target.nuscenes_att: zeros (the reference never fills it), or NULL           */
  float* t_velocity;     /* [B][M][3]     target.velocity: zeros, or NULL                                              */
  void* workspace;       /* cf_targets_workspace_bytes(B, M) bytes, 8-byte aligned: the per-object descriptors         */
  size_t workspace_bytes;
} cf_targets_args;
/* Three launches of 256 threads on `stream`, no host sync, bitwise reproducible:
 *   objects   one thread per (image, annotation): every per-object row, plus a descriptor (class, integer centre, radii and
 *             2 sigma^2, clipped Gaussian window, frustum ROI, paint rectangle, depth gate) in the workspace;
 *   heat map  one workgroup per (16-row band, image): descriptors staged in LDS, those missing the band culled; each element
 *             is the maximum over the objects of its class of the float64 Gaussian rounded to fp32, or 0;
 *   frustum   (CF_TARGETS_FRUSTUM) one workgroup per (band, image): a wave per box whose paint rectangle reaches the band
 *             finds the first row-major minimum among the non-zero radar pixels of its ROI with lo < v < hi; each pixel takes
 *             v / max_pc_dist (fp32) and the two velocity channels of the LAST such box in annotation order that covers it. */
int cf_targets_build(const cf_targets_args* a, void* stream);
size_t cf_targets_workspace_bytes(int B, int M);

/* cf_optim_adamw / cf_optim_sgd: the parameter update of a training step over ANY number of fp32 tensors in one launch
 * (replaces torch.optim.AdamW / torch.optim.SGD as model/modelWithLoss.py:66-76 constructs them: on the order of a hundred
 * foreach launches per step there).  Two DEVICE tables describe the work; they hold pointers and sizes only, so a host rebuilds
 * them only when the set of (parameter, gradient) pointers changes:
 *   tensors  [n_tensors] cf_optim_tensor: one record per parameter;
 *   chunks   [n_chunks]  cf_optim_chunk: (tensor index, element offset); ONE workgroup of 256 threads owns one chunk of at most
 *            CF_OPTIM_CHUNK elements of one tensor.  cf_optim_plan (host side) writes the list.
 * Everything that changes from step to step travels by value in cf_optim_args.  A tensor's own step count is
 * step - step_base (>= 1): torch keeps one count per parameter, and a parameter that receives its first gradient later starts at 1
 * there - here its record carries the optimizer's count at the moment it joined.  No workgroup reads what another workgroup of
 * the launch writes (no device-side counter), no LDS, no scratch.  16-byte accesses when all of a tensor's pointers are 16-byte
 * aligned, 4-byte accesses otherwise and for the last numel % 4 elements.
 * fp32 arithmetic in the order and with the roundings of torch's single-tensor CPU implementations (fma = one rounding, where
 * torch's lerp_ / addcmul_ / add_(alpha) kernels fuse; every other operation rounds on its own):
 *   AdamW  p *= decay (= 1 - lr * wd, rounded from double by the host);  m = fma(g - m, 1 - beta1, m);
 *          v = fma((1 - beta2) * g, g, v * beta2);  bc1 = 1 - beta1^s, bc2 = 1 - beta2^s in double;
 *          p += (-float(lr / bc1) * m) / (sqrt(v) / float(sqrt(bc2)) + eps)
 *   SGD    g' = fma(wd, p, g);  buf = g' at the tensor's first step (s == 1), else momentum * buf + g';  p = fma(-lr, buf, p)
 *          (no dampening, no Nesterov; state1 NULL = no momentum buffer: p = fma(-lr, g', p)). */
#define CF_OPTIM_CHUNK 4096 /* elements per workgroup; a multiple of 4, so a chunk keeps its tensor's 16-byte alignment */
typedef struct cf_optim_tensor {
  float* param;
  const float* grad;
  float* state1;     /* AdamW: exp_avg;    SGD: momentum_buffer or NULL */
  float* state2;     /* AdamW: exp_avg_sq; SGD: NULL                    */
  int64_t numel;
  int32_t step_base; /* the optimizer's step count before this tensor's first update */
  int32_t reserved;  /* 0 */
} cf_optim_tensor;
typedef struct cf_optim_chunk {
  int64_t offset;    /* first element of the chunk inside its tensor: a multiple of CF_OPTIM_CHUNK */
  int32_t tensor;    /* index into the tensor table */
  int32_t reserved;  /* 0 */
} cf_optim_chunk;
typedef struct cf_optim_args {
  const cf_optim_tensor* tensors; /* device */
  const cf_optim_chunk* chunks;   /* device */
  int32_t n_tensors, n_chunks;
  double lr;                      /* AdamW: divided by the bias correction in double, then rounded; SGD: rounded to fp32 */
  double beta1, beta2, eps;       /* AdamW; 1 - beta is formed in double, then rounded, as Python does for torch */
  double wd, momentum;            /* SGD */
  float decay;                    /* AdamW: 1 - lr * wd, formed in double by the host */
  int32_t step;                   /* the optimizer's step count INCLUDING this launch (>= 1) */
} cf_optim_args;
/* host side, no device access: the chunk list of `tensors` (HOST copy of the table: only numel is read) in table order, tensors
 * with numel == 0 contributing none.  chunks == NULL: count only.  -> CF_OK with the number of chunks in *n_chunks; CF_EINVAL
 * for a NULL table or n_chunks, n <= 0, a negative numel, or a `capacity` (entries of `chunks`) below the count. */
int cf_optim_plan(const cf_optim_tensor* tensors, int n, cf_optim_chunk* chunks, int64_t capacity, int64_t* n_chunks);
/* one launch each on `stream`; CF_EINVAL for NULL args / tables, n_tensors <= 0, n_chunks <= 0, step <= 0 */
int cf_optim_adamw(const cf_optim_args* a, void* stream);
int cf_optim_sgd(const cf_optim_args* a, void* stream);
int cf_optim_chunk_elems(void); /* CF_OPTIM_CHUNK of the library */

/* Weight packing runs once per load_state_dict (BatchNorm fold, slot tables, split hi / lo planes, MFMA fragment order).
 * For the f16x3 convolution and DCN operators it is part of this ABI (cf_pack_conv_f16x3, cf_pack_dcn_f16 above: host-side C,
 * byte-identical to the Python packers); the heads', the stem's and the upsample's weights are packed by
 * centerfusiondetect3d_amd/packing.py only (the reference's own host side is Python).  The layouts the kernels expect
 * are documented at each argument block above and in DESIGN.md section 3. */

/* Dynamic range of the f16x3 / mx kernels.  They evaluate fp32 products from operands split into two fp16 values after a
 * power-of-two pre-scale: weights per layer (chosen by the packer from max|W|), activations by `in_scale` (default 16).  An
 * activation with |x| * in_scale > 65504 is CLAMPED to +-65504 / in_scale - silently, the kernels carry no overflow flag.
 * The reference's fp32 convolutions accept any magnitude (model/networks/dla.py:124-159), so a caller must either know
 * its activations stay below 65504 / in_scale (4094 at the default) or measure them - cf_absmax_f32 on the source buffers -
 * and pass a smaller in_scale (out_scale = 2^-s / in_scale).  The Python host does exactly that: DLASeg.check_ranges /
 * calibrate / activation_ranges (centerfusiondetect3d_amd/model.py), Detector(range_policy=...).
 *
 * cf_absmax_f32: out[0] = max |x[m][c]| over m < M, c < C of an fp32 buffer with `stride` floats per row, as a float
 * (NaN if any element is NaN, +inf if any is infinite).  `out` (device, one float) is zeroed by the call (hipMemsetAsync on
 * `stream`) before the reduction; M = 0 leaves 0 there.  replaces: nothing in the reference (range guard of this path). */
int cf_absmax_f32(const float* x, long M, int C, int stride, float* out, void* stream);

/* cf_spin_us: diagnostic - ONE 64-thread workgroup that stays resident for `microseconds` (<= 100000) of the
 * constant 100 MHz clock and then exits.  Two of them on two streams finish in ~1x the time when the streams run
 * concurrently and in ~2x when HIP has put them on one hardware queue: the host's one-time stream-pair probe
 * (centerfusiondetect3d_amd/model.py, _side_streams).  No reference counterpart (the reference leaves stream
 * placement to PyTorch: it never forks streams). */
int cf_spin_us(int microseconds, void* stream);

const char* cf_last_error(void);
int cf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CF_HIP_H */
