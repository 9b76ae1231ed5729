// Whole detection heads in one launch on the bf16 MFMA pipe with SPLIT operands ("bf16x3"):
//
//     3x3 conv (64 [+3] -> 256) + ReLU  ->  [ReLU(W_l x + b_l)] x n_hidden  ->  W_out x + b_out (+ head activation)
//
// replaces the per-layer launches of model/networks/detectHeads.py:59-98 (3x3 first layer, 1x1 256->256 + ReLU
// layers, 1x1 256->n_out) whose only HBM-visible result is the small NCHW head map: the hidden maps never reach HBM.
//
// Split operands: every fp32 value x is carried as two bf16 numbers x = hi + lo (hi = rne(x), lo = rne(x - hi), 16
// significant bits together) and a product is evaluated as a*b ~= a_lo*b_hi + a_hi*b_lo + a_hi*b_hi (fp32 accumulate,
// a_lo*b_lo dropped): three v_mfma_f32_16x16x32_bf16 per 32-deep k-step, relative error per product <= ~2^-17.  Used
// for the heads only: they sit behind the DCN neck, so their rounding is not amplified (DESIGN.md section 4 "Numerics").
// "split-bf16 NHWC" = a pixel is [C hi][C lo] bf16, the same HBM bytes as fp32 (cf_split_bf16, the DCN epilogue).
//
// GEMM orientation is SWAPPED with respect to the conv kernels: MFMA A-operand = weights
// (rows = output channels), B-operand = activations (columns = pixels).  Consequences:
//   * weights never touch LDS: they are pre-packed on the host in MFMA fragment order, so a wave's
//     A fragment of one 32-deep k-step is ONE fully coalesced 1 KiB global load (L2-resident);
//   * no barrier inside a layer - only one between layers, when the tile is rewritten in place;
//   * the accumulator has pixels on lanes, so the final NCHW store is coalesced along pixels.
// In the hidden layers wave w of the 4 owns output channels [64w, 64w+64) x the 64 pixels of a half tile (4x4 16x16
// accumulators) whose [64 px][256 ch] hi and lo planes (66 KiB) stay in LDS for the whole chain; in the output layer
// the 4 waves split K instead and their partial sums are reduced through LDS.
#include <string>
#include "cf_common.h"
#include "cf_mx.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 hf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int HT_PX = 64;            // pixels per workgroup
constexpr int HT_C = 256;            // hidden width
constexpr int HT_ROWB = HT_C * 2 + 16;  // LDS bytes per pixel row per plane (528: odd multiple of 16)
constexpr int HT_PLANE = HT_PX * HT_ROWB;
constexpr int HT_LDS = 2 * HT_PLANE;    // 67,584 B

struct HeadTailK {
  const unsigned char* x;   // split-bf16 NHWC [M][2][x_stride]
  int x_stride;
  int M, HW;
  int n_heads;
  int n_hidden;             // 256->256 layers per head (0..2)
  const unsigned char* w_hidden[CF_MAX_HEADS][2];  // fragment-packed 256x256
  const float* b_hidden[CF_MAX_HEADS][2];          // 256 floats
  const unsigned char* w_out[CF_MAX_HEADS];        // fragment-packed 32x256
  const float* b_out[CF_MAX_HEADS];                // 32 floats (padded)
  float* out[CF_MAX_HEADS];                        // NCHW fp32 (B, n_out, H, W)
  float* out2[CF_MAX_HEADS];                       // RAW_AND_SIGDEPTH second output or null
  int c_base[CF_MAX_HEADS];                        // first hidden channel of the head inside x
  int n_out[CF_MAX_HEADS];
  int act[CF_MAX_HEADS];
};

__device__ __forceinline__ float bf16_rne(float a) { return (float)(__bf16)a; }
__device__ __forceinline__ unsigned pack2(float a, float b) {
  return ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)b) << 16) |
         __builtin_bit_cast(unsigned short, (__bf16)a);
}

// fragment-packed weights: [row tile][k step][plane][lane][8 bf16]  -> byte offset of a wave's fragment
__device__ __forceinline__ const bf16x8* wfrag(const unsigned char* w, int rt, int ks, int plane, int n_ks, int lane) {
  // (tile base) + 16 * lane: with a wave-uniform rt / ks the base is scalar arithmetic (see wfrag16, cf_f16x3.h)
  const unsigned char* base = w + ((size_t)rt * n_ks + ks) * 2048 + plane * 1024;
  return reinterpret_cast<const bf16x8*>(base + (unsigned)lane * 16u);
}

// 16x16 accumulators of one 64-pixel half tile (v_mfma_f32_16x16x32_bf16: lane = pixel ct*16 + (l & 15), reg r = channel
// 64w + 16rt + 4(l >> 4) + r) -> ReLU(acc + b) -> split bf16 -> LDS tile [plane][px][528 B]
// CTS: bit ct set = column tile ct (16 pixels) is stored (default: all four; the AT kernels keep the tile rows with a centre)
template <bool SCALED = false, int CTS = 0xF>
__device__ __forceinline__ void store_hidden_tile16(unsigned char* xt, const f32x4 (&acc)[4][4], const float* bias,
                                                    int wave, int lane, float sc = 1.0f, int pxcol = -1) {
  const int g = lane >> 4, c16 = pxcol < 0 ? (lane & 15) : pxcol;   // pxcol: the pixel column this lane's accumulators hold
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    const int ch = wave * 64 + rt * 16 + 4 * g;
    const f32x4 bb = *reinterpret_cast<const f32x4*>(bias + ch);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      if (!((CTS >> ct) & 1)) continue;
      float v[4], hi[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = fmaxf(SCALED ? __builtin_fmaf(acc[rt][ct][e], sc, bb[e]) : acc[rt][ct][e] + bb[e], 0.0f);
        hi[e] = bf16_rne(v[e]);
      }
      unsigned char* o = xt + (ct * 16 + c16) * HT_ROWB + ch * 2;
      const u32x2 ph = {pack2(hi[0], hi[1]), pack2(hi[2], hi[3])};
      const u32x2 pl = {pack2(v[0] - hi[0], v[1] - hi[1]), pack2(v[2] - hi[2], v[3] - hi[3])};
      *reinterpret_cast<u32x2*>(o) = ph;
      *reinterpret_cast<u32x2*>(o + HT_PLANE) = pl;
    }
  }
}

// pixel index inside a 64-pixel tile -> (image, pixel inside the image); false = outside
struct TileMap {       // 64 pixels of a tile at (y0, x0) of image b: 4 rows of 16 (sh = 4) or 8 rows of 8 (sh = 3)
  int b, y0, x0, H, W, sh = 4;
  __device__ __forceinline__ bool operator()(int px, int& bb, int& pix) const {
    const int y = y0 + (px >> sh), x = x0 + (px & ((1 << sh) - 1));
    if (y >= H || x >= W) return false;
    bb = b;
    pix = y * W + x;
    return true;
  }
};

// Virtual tiles (head_patch16_kernel<.., AT>): the 8 x 16 tile holds 3 x 6 disjoint 3x3 neighbourhoods whose centres - tile pixels
// (row 0 / 3 / 6, column 0 / 3 / .. / 15) - are the slots of a per-tile table of flat map pixels b * HW + y * W + x (-1: empty)
constexpr int AT_SLOTS = CF_HEAD_AT_SLOTS;
__device__ __forceinline__ int at_slot_of(int ty, int tx) { return (ty % 3 == 0 && tx % 3 == 0) ? (ty / 3) * 6 + tx / 3 : -1; }
struct SlotMap {       // 64 pixels of one half of a virtual tile: only the centres of non-empty slots are written
  const int* slots;
  int M, HW, half;
  __device__ __forceinline__ bool operator()(int px, int& bb, int& pix) const {
    const int t = half * 64 + px, sl = at_slot_of(t >> 4, t & 15);
    if (sl < 0) return false;
    const int s = slots[sl];
    if ((unsigned)s >= (unsigned)M) return false;
    bb = s / HW;
    pix = s - bb * HW;
    return true;
  }
};

// Hidden layers + output layer on a pixel tile that is already in LDS (xt).  All 256 threads.  Weights packed by
// pack_fragments16: w_hidden [16 rt][8 ks], w_out one 16-row tile; wave w owns channels [64w, 64w+64) x 64 pixels as
// 4 x 4 accumulators of 16 x 16; a k-step is 32 deep.
// CTS: the column tiles (bit ct) that are computed and whose pixels pm may accept (default: all four)
template <class PixMap, int CTS = 0xF>
__device__ __forceinline__ void head_tail_from_lds16(const HeadTailK& p, unsigned char* xt, int head, const PixMap& pm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  for (int l = 0; l < p.n_hidden; ++l) {
    const unsigned char* w = p.w_hidden[head][l];
    const float* bias = p.b_hidden[head][l];
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.0f;
    bf16x8 wh[2][4], wl[2][4];               // one k-step ahead: set ks & 1
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      wh[0][rt] = *wfrag(w, wave * 4 + rt, 0, 0, 8, lane);
      wl[0][rt] = *wfrag(w, wave * 4 + rt, 0, 1, 8, lane);
    }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      if (ks + 1 < 8) {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
          wh[(ks + 1) & 1][rt] = *wfrag(w, wave * 4 + rt, ks + 1, 0, 8, lane);
          wl[(ks + 1) & 1][rt] = *wfrag(w, wave * 4 + rt, ks + 1, 1, 8, lane);
        }
      }
      bf16x8 xh[4], xl[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        if (!((CTS >> ct) & 1)) continue;
        const unsigned char* row = xt + (ct * 16 + c16) * HT_ROWB + (ks * 32 + g * 8) * 2;
        xh[ct] = *reinterpret_cast<const bf16x8*>(row);
        xl[ct] = *reinterpret_cast<const bf16x8*>(row + HT_PLANE);
      }
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if ((CTS >> ct) & 1) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[ks & 1][rt], xh[ct], acc[rt][ct], 0, 0, 0);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if ((CTS >> ct) & 1) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks & 1][rt], xl[ct], acc[rt][ct], 0, 0, 0);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if ((CTS >> ct) & 1) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks & 1][rt], xh[ct], acc[rt][ct], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // every wave has read the whole tile: rewrite it in place
    store_hidden_tile16<false, CTS>(xt, acc, bias, wave, lane);
    __syncthreads();
  }

  // ---- output layer: wave w takes k in [64w, 64w+64) = 2 k-steps
  f32x4 oacc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) oacc[b][r] = 0.0f;
  {
    const unsigned char* w = p.w_out[head];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int ks = wave * 2 + s2;
      const bf16x8 ah = *wfrag(w, 0, ks, 0, 8, lane), al = *wfrag(w, 0, ks, 1, 8, lane);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        if (!((CTS >> ct) & 1)) continue;
        const unsigned char* row = xt + (ct * 16 + c16) * HT_ROWB + (ks * 32 + g * 8) * 2;
        const bf16x8 xh = *reinterpret_cast<const bf16x8*>(row);
        const bf16x8 xl = *reinterpret_cast<const bf16x8*>(row + HT_PLANE);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, xh, oacc[ct], 0, 0, 0);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xl, oacc[ct], 0, 0, 0);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xh, oacc[ct], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // tile no longer needed: reuse LDS for the 4 partial sums [wave][n 16][px 64]
  float* red = reinterpret_cast<float*>(xt);
  const int n_out = p.n_out[head], act = p.act[head];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 4 * g + r;
      if (((CTS >> ct) & 1) && n < n_out) red[(wave * 16 + n) * HT_PX + ct * 16 + c16] = oacc[ct][r];
    }
  __syncthreads();
  const float* bo = p.b_out[head];
  float* out = p.out[head];
  float* out2 = p.out2[head];
  const int px = tid & 63;
  int b, pix;
  if (pm(px, b, pix)) {
    for (int n = tid >> 6; n < n_out; n += 4) {
      const float raw = red[n * HT_PX + px] + red[(16 + n) * HT_PX + px] + red[(32 + n) * HT_PX + px] +
                        red[(48 + n) * HT_PX + px] + bo[n];
      const size_t o = ((size_t)b * n_out + n) * p.HW + pix;
      float v = raw;
      if (act == CF_ACT_RELU) v = fmaxf(raw, 0.0f);
      else if (act == CF_ACT_SIGMOID_CLAMP) v = fminf(fmaxf(cf_sigmoid(raw), 1e-4f), 1.0f - 1e-4f);
      out[o] = v;
      if (act == CF_ACT_RAW_AND_SIGDEPTH) out2[o] = 1.0f / (cf_sigmoid(raw) + 1e-6f) - 1.0f;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Whole head on a 2-D PATCH: one workgroup owns an 8 x 16 (or 16 x 8) pixel tile (128 px) of one image.  The
// (8+2) x (16+2) input patch - all 64 feature channels (and the 8-channel pc_hm plane pair) in split-bf16 - is copied
// to LDS once, zero-filled outside the image, and all 9 taps read their B fragments from it at compile-time offsets:
// no slot table, no barrier and no staging inside the K loop.  A wave owns 64 hidden channels x 128 pixels as 4 x 8
// accumulators of 16 x 16 (v_mfma_f32_16x16x32_bf16); a k-step is 32 deep = half the channels of one tap (or ALL nine
// taps x 3 channels of the pc_hm plane pair, k = 3 tap + channel, read from an operand image built once per workgroup
// behind the patch - and left out by a workgroup whose pc_hm patch is all zero).  Under the chip's power management a
// dense MFMA loop on random data holds a higher
// clock with the 16x16x32 shape than with 32x32x16 at equal cycles per FLOP: measured on this part 1.72 vs 1.51
// PFLOP/s with every operand re-read from LDS (tools/micro/mfma_shape.hip, MI355X_MICROARCH.md "DVFS give-back"
// item 7) - and this kernel is bound by exactly that loop.  Weights come as [16-row tile][k32 step][hi|lo][lane][8]
// fragments (packing.pack_fragments16), one k-step ahead in registers.  With n_hidden == 0 the 256 -> n_out layer
// runs straight from the accumulator registers: ReLU(acc + b) split to bf16 IS a B fragment - two stacked 16 x 16
// tiles give a lane 4 + 4 channels of one pixel - if w_out is packed in that k order
// (pack_fragments16(acc_order=True)); the four waves' partial sums meet in LDS; n_out <= 16.
// ---------------------------------------------------------------------------------------------
constexpr int HP_ROWS = (8 + 2) * (16 + 2);    // 180 patch rows (either tile orientation)
constexpr int HP_PX = 8 * 16;                  // 128 pixels per tile
constexpr int HP16_RED = 4 * 16 * HP_PX * 4;   // partial sums [wave][16][128] BEHIND the patch
constexpr int hp16_patch_bytes(bool pc) { return HP_ROWS * (4 * 64 + (pc ? 32 : 0) + 16); }   // 48,960 / 54,720
// pc_hm source: behind the patch, the four waves' "my part of the pc_hm patch is non-zero" words (16 B) and the OPERAND IMAGE
// of the radar k-step, [128 px][hi, lo][32 bf16: k = 3 tap + channel, 27 real] at a row pitch of 80 B (odd multiple of 16)
constexpr int HP_PCIMG_ROWB = 32 * 2 + 16;
constexpr int HP_PCIMG = HP_PX * 2 * HP_PCIMG_ROWB;            // 20,480 B
constexpr int hp16_pc_extra(bool pc) { return pc ? 16 + HP_PCIMG : 0; }
// without pc_hm: 48,960 + 32,768 = 81,728 B <= half of the CU's 160 KiB: still two workgroups per CU.  With pc_hm and hidden
// layers: 54,720 + 16 + 20,480 = 75,216 B (the chain's 67,584 B tile reuses it afterwards): two per CU; with pc_hm and no
// hidden layers 107,984 B: one per CU, as before the image (87,488 B)
constexpr int hp16_lds(bool pc, bool hidden) {
  return hidden ? (HT_LDS > hp16_patch_bytes(pc) + hp16_pc_extra(pc) ? HT_LDS : hp16_patch_bytes(pc) + hp16_pc_extra(pc))
                : hp16_patch_bytes(pc) + hp16_pc_extra(pc) + HP16_RED;
}

struct HeadPatchK {
  HeadTailK t;
  const unsigned char* src[2];               // split-bf16 NHWC sources of the 3x3 layer (feat or its mx rows, pc_hm)
  int src_c[2];
  int H, W, tiles_x, tiles_y, n_ks;
  int pc_skip;                               // != 0: a workgroup whose pc_hm patch is all (+-) zero leaves the pc_hm taps out
  int hloop;                                 // consecutive heads one workgroup walks on its patch
  const unsigned char* w_first[CF_MAX_HEADS];
  const float* b_first[CF_MAX_HEADS];
  const unsigned char* w_out_perm[CF_MAX_HEADS];
  float first_scale[CF_MAX_HEADS];           // MX kernel: 2^-(s+4) of head i's first layer
  const int* slot_pixels;                    // AT kernels: [tiles_x virtual tiles][AT_SLOTS] flat map pixels (-1: empty slot)
};

// MX = true: the FIRST layer on "fp16 main term + block-scaled FP6 cross terms" (1.5 MFMA passes per product instead of the 3
// of bf16x3; numerics and the gate that confines the scheme to the first layer: packing.pack_head_first_mx).  The
// feature source is the 272-byte-per-pixel image cf_pack_feat_mx writes - four 64-byte segments g = 0..3, each [8 fp16: channels
// 8g..8g+7 of 16 x][8 fp16: channels 32+8g..][32 FP6 e2m3 fields (24 B) + 8 B pad: block g of q6(xl) channels 0-31, 32-63,
// q6(xh) channels 0-31, 32-63], then one E8M0 scale byte per block and padding - which IS the LDS patch row: lane group g of
// every B fragment reads inside segment g (bank-conflict-free ds_read_b128, see colperm below).  Per tap: 2 k-steps of v_mfma_f32_16x16x32_f16 (weights' fp16 hi) and ONE v_mfma_scale_f32_16x16x128_f8f6f4
// whose four 32-deep K blocks are q6(Wh) . q6(xl) (two 32-channel halves) and q6(Wl) . q6(xh): lane g = l >> 4 of either operand
// holds K block g, with the block's scale byte in its lane.  Weights stream from L2 in (wave, tap) slabs, two items (of
// main / main / cross) ahead.  pc_hm stays on bf16x3 (one dense k-step, pc_kstep below) with its weights pre-multiplied by
// 2^(s+4); the accumulators are scaled by
// first_scale = 2^-(s+4) where the bias is added.  Hidden and output layers: unchanged bf16x3.
// HID: -1 = n_hidden decided at run time (the bf16x3 instantiations); 0 / 1 = compiled for heads without / with hidden layers
// (the MX instantiations: the register allocator then sees one of the two epilogues, not both).
// AT = true ("at the listed pixels"): the tile is a VIRTUAL one - 18 listed pixels of any images with their 3x3 neighbourhoods
// gathered into the patch (SlotMap above; q.tiles_x tiles, q.tiles_y = 1) - and only those pixels of the maps are written.  Every
// step between the patch fill and the output writes works per pixel column of the MFMA tile, so a pixel gets the bits the dense
// form gives it.
template <int NS, bool PC, bool TP, bool MX = false, int HID = -1, bool AT = false>
__global__ __launch_bounds__(256, 2) void head_patch16_kernel(HeadPatchK q) {
  static_assert(NS == 4, "64 feature channels");
  static_assert(!AT || !TP, "virtual tiles are laid out on the flat 8 x 16 tile");
  constexpr int MX_SLAB = 14592, PC_OFF = MX ? 272 : NS * 64;      // (wave, tap) weight slab bytes; pc_hm planes inside a patch row
  // TP: the 128-pixel tile stands upright (16 rows x 8 columns) instead of 8 x 16 - same patch size (18 x 10 rows), chosen by
  // the host when it covers the map with fewer tiles (112 x 200: 7 x 25 = 175 exact tiles instead of 14 x 13 = 182)
  constexpr int TSH = TP ? 3 : 4, TMASK = (1 << TSH) - 1;          // pixel index -> (row = px >> TSH, column = px & TMASK)
  constexpr int T_H = TP ? 16 : 8, T_W = TP ? 8 : 16, P_W = T_W + 2;
  static_assert((T_H + 2) * P_W == HP_ROWS, "both tile shapes have the same patch size");
  constexpr int ROWB = NS * 64 + (PC ? 32 : 0) + 16;     // odd multiple of 16 B
  constexpr int NKF = 9 * NS / 2;                        // k32-steps of the feature channels
  constexpr int NK = NKF + (PC ? 1 : 0);               // + the radar taps: ONE k-step, k = 3 tap + channel (27 real of 32)
  extern __shared__ __attribute__((aligned(16))) unsigned char xt[];
  const HeadTailK& p = q.t;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: scalar weight tile addressing)
  const int g = lane >> 4;
  // MX, flat tile: lane l & 15 holds pixel COLUMN colperm(l & 15) of the 16-pixel tile row, not column l & 15.  A ds_read_b128 is
  // served in groups of 16 lanes made of 8 lanes of one K group g and 8 of g + 1 ({0-3, 12-15, 20-27}, ...); with the K groups
  // of a patch row 64 B apart and the row pitch = 16 B (mod 256 B), the 16 lanes of a group hit 16 different 16-byte bank
  // quads iff the columns of lanes {4..11} form a set invariant under +4: {0,4,8,12,1,5,9,13} (the others get the rest).
  const int c16 = (MX && !TP) ? ((lane & 12) == 4 || (lane & 12) == 8 ? (((lane & 15) - 4) & 3) * 4 + (((lane & 15) - 4) >> 2)
                                                                      : (lane & 3) * 4 + 2 + ((lane & 15) >> 3))
                              : (lane & 15);
  const int per_img = q.tiles_x * q.tiles_y;
  const int per_head = AT ? per_img : per_img * (p.M / p.HW);
  // grid = (head range, tile): a workgroup keeps its patch in LDS and walks q.hloop consecutive heads on it (heads
  // without hidden layers only: the hidden chain rewrites the patch area).  Head-range-major order, so the
  // workgroups in flight work on the same few heads and their first-layer weights stay hot in L2, while the patch
  // is read from HBM once per range instead of once per head.
  const int hg = blockIdx.x / per_head;
  // within a head range consecutive tiles run on ONE XCD: neighbouring patches share their halo rows in that XCD's L2
  int rem = cf_xcd_remap(blockIdx.x - hg * per_head, per_head);
  const int head0 = hg * q.hloop, head1 = min(head0 + q.hloop, p.n_heads);
  const int b = rem / per_img;
  rem -= b * per_img;
  const int y0 = (rem / q.tiles_x) * T_H, x0 = (rem % q.tiles_x) * T_W;
  // AT: this workgroup's slots; patch row (pr, pc) of the 10 x 18 patch is neighbour (pr % 3 - 1, pc % 3 - 1) of slot (pr / 3, pc / 3)
  // -> its flat map pixel, or -1 = a zero row (outside the image, an empty slot, the unused 10th patch row)
  const int* const at_slots = AT ? q.slot_pixels + (size_t)rem * AT_SLOTS : nullptr;
  // AT: on the flat tile a column tile ct is tile ROW ct, and only rows 0, 3 and 6 hold a centre (at_slot_of): every loop over
  // column tiles below leaves the other five out - at compile time, inside the unrolled loops, so their accumulators and
  // fragment reads do not exist.  (MFMA accumulator columns are independent: a written pixel keeps its bits.)
  constexpr auto live = [](int ct) { return !AT || ct % 3 == 0; };
  auto at_src = [&](int row) -> int {
    const int pr = row / P_W, pc = row % P_W;
    if (pr >= 9) return -1;
    const int s = at_slots[(pr / 3) * 6 + pc / 3];
    if ((unsigned)s >= (unsigned)p.M) return -1;
    const int bb = s / p.HW, pix = s - bb * p.HW;
    const int y = pix / q.W + pr % 3 - 1, x = pix % q.W + pc % 3 - 1;
    if ((unsigned)y >= (unsigned)q.H || (unsigned)x >= (unsigned)q.W) return -1;
    return bb * p.HW + y * q.W + x;
  };
  if constexpr (AT) {                         // (workgroup-uniform) a tile without a listed pixel writes nothing
    int any = 0;
    for (int i = 0; i < AT_SLOTS; ++i) any |= (unsigned)at_slots[i] < (unsigned)p.M ? 1 : 0;
    if (!any) return;
  }

  // ---- patch -> LDS (one pass, every load in flight before the first LDS write)
  if constexpr (MX) {
    constexpr int UPR = 17;                                // 16-byte units of a 272-byte mx row: the LDS row image itself
    constexpr int NIT = (HP_ROWS * UPR + 255) / 256;
    u32x4 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + it * 256;
      const int row = idx / UPR, u = idx % UPR;
      const int y = y0 - 1 + row / P_W, x = x0 - 1 + row % P_W;
      v[it] = u32x4{0u, 0u, 0u, 0u};                       // outside the image: zero fields with scale byte 0 (2^-127): exact zeros
      if constexpr (AT) {
        const int s = row < HP_ROWS ? at_src(row) : -1;
        if (s >= 0) v[it] = *reinterpret_cast<const u32x4*>(q.src[0] + (size_t)s * 272 + u * 16);
      } else
      if (row < HP_ROWS && (unsigned)y < (unsigned)q.H && (unsigned)x < (unsigned)q.W)
        v[it] = *reinterpret_cast<const u32x4*>(q.src[0] + (size_t)(b * p.HW + y * q.W + x) * 272 + u * 16);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + it * 256;
      const int row = idx / UPR, u = idx % UPR;
      if (row < HP_ROWS) *reinterpret_cast<u32x4*>(xt + row * ROWB + u * 16) = v[it];
    }
  } else {
    constexpr int UPR = NS * 4;                            // 16-byte units per row: hi plane then lo plane
    constexpr int NIT = (HP_ROWS * UPR + 255) / 256;
    u32x4 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + it * 256;
      const int row = idx / UPR, u = idx % UPR;
      const int y = y0 - 1 + row / P_W, x = x0 - 1 + row % P_W;
      v[it] = u32x4{0u, 0u, 0u, 0u};
      if constexpr (AT) {
        const int s = row < HP_ROWS ? at_src(row) : -1;
        if (s >= 0) v[it] = *reinterpret_cast<const u32x4*>(q.src[0] + ((size_t)s * 2 * q.src_c[0]) * 2 +
                                                             (u / (NS * 2)) * q.src_c[0] * 2 + (u % (NS * 2)) * 16);
      } else
      if (row < HP_ROWS && (unsigned)y < (unsigned)q.H && (unsigned)x < (unsigned)q.W)
        v[it] = *reinterpret_cast<const u32x4*>(q.src[0] + ((size_t)(b * p.HW + y * q.W + x) * 2 * q.src_c[0]) * 2 +
                                                (u / (NS * 2)) * q.src_c[0] * 2 + (u % (NS * 2)) * 16);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + it * 256;
      const int row = idx / UPR, u = idx % UPR;
      const int plane = u / (NS * 2), uu = u % (NS * 2);
      if (row < HP_ROWS) *reinterpret_cast<u32x4*>(xt + row * ROWB + (uu >> 1) * 64 + plane * 32 + (uu & 1) * 16) = v[it];
    }
  }
  // pc_hm is zero outside the boxes the frustum association painted: a patch (tile + frame) without a non-zero value adds
  // exact zeros to the accumulators.  Every thread ORs the words it copies (sign bits off: -0 is zero); a wave leaves its
  // verdict in one word BEHIND the patch (in front of the partial sums / inside the chain's tile, which is written only
  // after every wave is done with the patch), and the barrier that completes the patch publishes the four words.
  unsigned* const pc_flags = reinterpret_cast<unsigned*>(xt + hp16_patch_bytes(PC));
  if (PC) {
    unsigned nz = 0u;
    for (int idx = tid; idx < HP_ROWS * 2; idx += 256) {
      const int row = idx >> 1, plane = idx & 1;
      const int y = y0 - 1 + row / P_W, x = x0 - 1 + row % P_W;
      u32x4 w = {0u, 0u, 0u, 0u};
      if constexpr (AT) {
        const int s = at_src(row);
        if (s >= 0) w = *reinterpret_cast<const u32x4*>(q.src[1] + ((size_t)s * 2 + plane) * q.src_c[1] * 2);
      } else
      if ((unsigned)y < (unsigned)q.H && (unsigned)x < (unsigned)q.W)
        w = *reinterpret_cast<const u32x4*>(q.src[1] + ((size_t)(b * p.HW + y * q.W + x) * 2 + plane) * q.src_c[1] * 2);
      *reinterpret_cast<u32x4*>(xt + row * ROWB + PC_OFF + plane * 16) = w;
      nz |= (w[0] | w[1] | w[2] | w[3]) & 0x7fff7fffu;
    }
    const bool wave_nz = __builtin_amdgcn_ballot_w64(nz != 0u) != 0ull;
    if (lane == 0) pc_flags[wave] = (wave_nz || !q.pc_skip) ? 1u : 0u;
  }

  // B fragment of a 16x16x32 MFMA: lane (g = l >> 4, c = l & 15) holds 8 consecutive channels 8g .. 8g+7 of the
  // k-step's 32 for pixel column c of the 16-pixel tile row
  int rowb[8];                               // LDS byte offset of this lane's pixel in tile row ct (tap (-1,-1))
#pragma unroll
  for (int ct = 0; ct < 8; ++ct)          // pixel ct * 16 + c16: a compile-time stride per ct (immediate offsets of the ds_reads)
    rowb[ct] = ((c16 >> TSH) * P_W + (c16 & TMASK)) * ROWB + ct * ((16 >> TSH) * P_W * ROWB);
  const int koff = (g >> 1) * 64 + (g & 1) * 16;         // 8-channel group inside a 32-channel half (hi plane; lo at +32)
  // radar k-step: the same lane reads k = 8g .. 8g+7 of pixel ct * 16 + c16 from the operand image (hi; lo one row on)
  unsigned char* const pcimg = xt + hp16_patch_bytes(PC) + 16;
  const int imgb = c16 * (2 * HP_PCIMG_ROWB) + g * 16;
  __syncthreads();                           // the patch is complete
  bool pc_live = false;                      // workgroup-uniform: the pc_hm taps contribute
  if (PC) {
    const u32x4 f = *reinterpret_cast<const u32x4*>(pc_flags);
    pc_live = __builtin_amdgcn_readfirstlane((int)(f[0] | f[1] | f[2] | f[3])) != 0;
  }
  if (PC && pc_live) {
    // the operand image, once per workgroup: thread = (pixel, plane) gathers channels 0-2 of its 9 taps from the patch's
    // pc_hm planes (outside the image: the patch's zeros) into one row, k = 3 tap + channel, k = 27..31 zero
    const int ipx = tid & (HP_PX - 1), plane = tid >> 7;
    const unsigned char* sp = xt + ((ipx >> TSH) * P_W + (ipx & TMASK)) * ROWB + PC_OFF + plane * 16;
    unsigned e[32];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const u32x2 w = *reinterpret_cast<const u32x2*>(sp + ((t / 3) * P_W + t % 3) * ROWB);
      e[3 * t] = w[0] & 0xffffu;
      e[3 * t + 1] = w[0] >> 16;
      e[3 * t + 2] = w[1] & 0xffffu;
    }
#pragma unroll
    for (int k = 27; k < 32; ++k) e[k] = 0u;
    unsigned char* dp = pcimg + (ipx * 2 + plane) * HP_PCIMG_ROWB;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<u32x4*>(dp + j * 16) = u32x4{e[8 * j] | (e[8 * j + 1] << 16), e[8 * j + 2] | (e[8 * j + 3] << 16),
                                                     e[8 * j + 4] | (e[8 * j + 5] << 16), e[8 * j + 6] | (e[8 * j + 7] << 16)};
    __syncthreads();                         // (workgroup-uniform branch) the image is complete
  }
  // the radar k-step on bf16x3 (cross, cross, main as everywhere): 4 row tiles x 8 pixel tiles x 3 = 96 MFMAs
  auto pc_kstep = [&](const bf16x8 (&ah)[4], const bf16x8 (&al)[4], f32x4 (&acc)[4][8]) __attribute__((always_inline)) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      bf16x8 xh[4], xl[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        if (!live(4 * hf + ct)) continue;
        const unsigned char* r = pcimg + imgb + (4 * hf + ct) * (16 * 2 * HP_PCIMG_ROWB);
        xh[ct] = *reinterpret_cast<const bf16x8*>(r);
        xl[ct] = *reinterpret_cast<const bf16x8*>(r + HP_PCIMG_ROWB);
      }
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (live(4 * hf + ct))
            acc[rt][4 * hf + ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[rt], xh[ct], acc[rt][4 * hf + ct], 0, 0, 0);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (live(4 * hf + ct))
            acc[rt][4 * hf + ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[rt], xl[ct], acc[rt][4 * hf + ct], 0, 0, 0);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (live(4 * hf + ct))
            acc[rt][4 * hf + ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[rt], xh[ct], acc[rt][4 * hf + ct], 0, 0, 0);
    }
  };
  auto first_layer = [&](int head, f32x4 (&acc)[4][8]) __attribute__((always_inline)) {
  if constexpr (MX) {
    const unsigned char* wb = q.w_first[head] + (size_t)wave * (9 * MX_SLAB);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][c][r] = 0.0f;
    hf16x8 am[2][4];                         // fp16 hi fragments of the tap's two k-steps
    u32x4 ax0[4];                            // FP6 fragments of the tap's cross term: 24 B per lane and row tile
    u32x2 ax1[4];
    int sa;                                  // their E8M0 scale bytes, byte rt
    // buffer loads: a scalar resource per (wave, tap) slab + a per-lane 32-bit offset + small constants - no 64-bit address
    // arithmetic and no address register pairs in a loop that has every register in use
    auto slab = [&](int tap) {
      return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(wb + tap * MX_SLAB), 0, MX_SLAB, 0x00020000);
    };
    const int l16 = lane * 16, l8 = lane * 8, l4 = lane * 4;
    // radar k-step (PC): behind the slabs the pc_hm weights x 2^s x feat_scale lie in the container [wv 4][ks 3][rt 4][hi, lo][lane 64]
    // [8 bf16] of the per-tap layout; the dense k-step (k = 3 tap + channel, lane group G = k >> 3) is threaded through its
    // padding - group 0 in the g = 0 lanes of k-step 0, groups 1-3 in the g = 1..3 lanes of k-step 2 (packing.pack_head_first_mx) -
    // so a lane's fragment is at lane * 16 (+ two k-steps for G > 0).  With hidden layers (HID == 1, the model's radar heads) the 8
    // fragments are requested inside tap 8, where a tap 9's main fragments would be: those registers are free by then, and no L2
    // latency is exposed in front of the k-step.  Without hidden layers the epilogue's addresses are live across the head loop
    // and the early request costs scratch: requested where they are used.
    bf16x8 ph[4], pl[4];
    auto ldp = [&](bf16x8 (&d)[4], int plane) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<unsigned char*>(q.w_first[head] + (size_t)4 * 9 * MX_SLAB), 0, 4 * 3 * 4 * 2048, 0x00020000);
      const int lo = l16 + (g ? 2 * 4 * 2048 : 0);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        d[rt] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, lo, wave * (3 * 4 * 2048) + rt * 2048 + plane * 1024, 0));
    };
    auto ldm = [&](hf16x8 (&d)[4], int tap, int ks2) {
      const __amdgpu_buffer_rsrc_t rs = slab(tap);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        d[rt] = __builtin_bit_cast(hf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, l16, (rt * 2 + ks2) * 1024, 0));
    };
    auto ldx = [&](int tap) {
      const __amdgpu_buffer_rsrc_t rs = slab(tap);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        ax0[rt] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, l16, 8192 + rt * 1536, 0));
        ax1[rt] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, l8, 8192 + rt * 1536 + 1024, 0));
      }
      sa = (int)__builtin_amdgcn_raw_buffer_load_b32(rs, l4, 14336, 0);
    };
    // one half (tile rows 4 hf .. 4 hf + 3) of a main k-step / one pair (tile rows 2 pr, 2 pr + 1) of a cross step
    auto main_half = [&](const hf16x8 (&A)[4], int off, int hf) {
      hf16x8 xb[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (live(4 * hf + ct)) xb[ct] = *reinterpret_cast<const hf16x8*>(xt + rowb[4 * hf + ct] + off);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (live(4 * hf + ct))
            acc[rt][4 * hf + ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[rt], xb[ct], acc[rt][4 * hf + ct], 0, 0, 0);
    };
    auto cross_pair = [&](int toff, int pr) {
      i32x8 xb[2];
      int sb[2];
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        if (!live(2 * pr + c2)) continue;                  // (AT: pair 2 goes entirely, pairs 0, 1 and 3 keep one tile row each)
        const unsigned char* r = xt + rowb[2 * pr + c2] + toff;
        const u32x4 b0 = *reinterpret_cast<const u32x4*>(r + 64 * g + 32);
        const u32x2 b1 = *reinterpret_cast<const u32x2*>(r + 64 * g + 48);
        xb[c2] = i32x8{(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], 0, 0};
        sb[c2] = (int)(*reinterpret_cast<const unsigned*>(r + 256) >> (8 * g));     // this lane's block: byte g -> byte 0
      }
#define CF_MX_ROW(RT)                                                                                                   \
      {                                                                                                                 \
        const i32x8 a6 = {(int)ax0[RT][0], (int)ax0[RT][1], (int)ax0[RT][2], (int)ax0[RT][3], (int)ax1[RT][0],          \
                          (int)ax1[RT][1], 0, 0};                                                                       \
        _Pragma("unroll") for (int c2 = 0; c2 < 2; ++c2) if (live(2 * pr + c2))                                         \
          acc[RT][2 * pr + c2] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a6, xb[c2], acc[RT][2 * pr + c2],    \
                                                                                  2, 2, RT, sa, 0, sb[c2]);             \
      }
      CF_MX_ROW(0) CF_MX_ROW(1) CF_MX_ROW(2) CF_MX_ROW(3)
#undef CF_MX_ROW
    };
    ldm(am[0], 0, 0);
    ldm(am[1], 0, 1);
    ldx(0);
    // Items per tap: main k-step 0, main k-step 1, cross.  The operands of the item two behind are requested in the MIDDLE
    // of an item (their buffer was freed by the item before), with the only sched_barrier of the item right behind the
    // requests: they cannot sink to their first use, while the LDS reads of the NEXT item's first half may rise above the
    // second half's MFMAs.  (An explicit software pipeline of the B fragments - two buffers, one barrier per 16 MFMAs - was
    // built and measured at the same time, 904 vs 897 us, for 16 more registers: docs/experiments/r5_heads_mx_kernel.md.)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = ((tap / 3) * P_W + tap % 3) * ROWB;
      const int o0 = toff + g * 64, o1 = toff + g * 64 + 16;   // channels 0-31 / 32-63: lane group g holds 8 g .. 8 g + 7 of them
      main_half(am[0], o0, 0);
      if (tap > 0) ldx(tap);                               // (cross operands of THIS tap: freed by the item before)
      __builtin_amdgcn_sched_barrier(0);
      main_half(am[0], o0, 1);
      main_half(am[1], o1, 0);
      if (tap + 1 < 9) ldm(am[0], tap + 1, 0);
      else if (PC && HID == 1) ldp(ph, 0);
      __builtin_amdgcn_sched_barrier(0);
      main_half(am[1], o1, 1);
      cross_pair(toff, 0);
      cross_pair(toff, 1);
      if (tap + 1 < 9) ldm(am[1], tap + 1, 1);
      else if (PC && HID == 1) ldp(pl, 1);
      __builtin_amdgcn_sched_barrier(0);
      cross_pair(toff, 2);
      cross_pair(toff, 3);
    }
    __builtin_amdgcn_sched_barrier(0);       // (the epilogue's loads stay behind the last item)
    if (PC) {
      if (pc_live) {                         // (an all-zero pc_hm patch would add exact zeros)
        if constexpr (HID != 1) { ldp(ph, 0); ldp(pl, 1); }
        pc_kstep(ph, pl, acc);
      }
    }
    return;
  }
  const unsigned char* w1 = q.w_first[head];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][c][r] = 0.0f;

  bf16x8 wh[2][4], wl[2][4];                 // weight fragments one k-step ahead: set ks & 1
  auto load_w = [&](bf16x8 (&dh)[4], bf16x8 (&dl)[4], int ks) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      dh[rt] = *wfrag(w1, wave * 4 + rt, ks, 0, q.n_ks, lane);
      dl[rt] = *wfrag(w1, wave * 4 + rt, ks, 1, q.n_ks, lane);
    }
  };
  load_w(wh[0], wl[0], 0);

#pragma unroll
  for (int ks = 0; ks < NKF; ++ks) {
    if (ks + 1 < NK) load_w(wh[(ks + 1) & 1], wl[(ks + 1) & 1], ks + 1);
    const int tap = ks / (NS / 2), half = ks % (NS / 2);
    const int off = ((tap / 3) * P_W + tap % 3) * ROWB + half * 128 + koff, lo = 32;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {         // tile rows 0-3, then 4-7: half of the B fragments live at a time
      bf16x8 xh[4], xl[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        if (!live(4 * hf + ct)) continue;
        xh[ct] = *reinterpret_cast<const bf16x8*>(xt + rowb[4 * hf + ct] + off);
        xl[ct] = *reinterpret_cast<const bf16x8*>(xt + rowb[4 * hf + ct] + off + lo);
      }
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (live(4 * hf + ct))
            acc[rt][4 * hf + ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[ks & 1][rt], xh[ct], acc[rt][4 * hf + ct], 0, 0, 0);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (live(4 * hf + ct))
            acc[rt][4 * hf + ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks & 1][rt], xl[ct], acc[rt][4 * hf + ct], 0, 0, 0);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (live(4 * hf + ct))
            acc[rt][4 * hf + ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks & 1][rt], xh[ct], acc[rt][4 * hf + ct], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (PC) {                                  // the radar k-step, or (all-zero pc_hm patch: exact zeros) nothing - see the MX form
    if (pc_live) pc_kstep(wh[NKF & 1], wl[NKF & 1], acc);
  }
  };

  if (HID < 0 ? p.n_hidden > 0 : HID == 1) {   // (the host launches these with hloop == 1)
    const int head = head0;
    f32x4 acc[4][8];
    first_layer(head, acc);
    // hidden layers need all 256 channels of a pixel: the two 64-pixel halves of the tile go through
    // the LDS-resident chain (head_tail_from_lds16) one after the other (LDS stays at 66 KiB: 2 workgroups/CU)
    __syncthreads();                         // every wave is done with the patch
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x4 a2[4][4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) a2[rt][ct] = acc[rt][4 * half + ct];
      // AT: the tile rows with a centre - 0 and 3 of half 0, 6 (local 2) of half 1; the chain's other rows are neither written nor read
      if constexpr (AT) {
        if (half == 0) store_hidden_tile16<MX, 0x9>(xt, a2, q.b_first[head], wave, lane, MX ? q.first_scale[head] : 1.0f, c16);
        else store_hidden_tile16<MX, 0x4>(xt, a2, q.b_first[head], wave, lane, MX ? q.first_scale[head] : 1.0f, c16);
      } else
      store_hidden_tile16<MX>(xt, a2, q.b_first[head], wave, lane, MX ? q.first_scale[head] : 1.0f, c16);
      if constexpr (MX) __builtin_amdgcn_sched_barrier(0);     // (the chain's first weight loads stay behind the tile stores)
      __syncthreads();
      if constexpr (AT) {
        if (half == 0) head_tail_from_lds16<SlotMap, 0x9>(p, xt, head, SlotMap{at_slots, p.M, p.HW, half});
        else head_tail_from_lds16<SlotMap, 0x4>(p, xt, head, SlotMap{at_slots, p.M, p.HW, half});
      }
      else head_tail_from_lds16(p, xt, head, TileMap{b, y0 + (64 >> TSH) * half, x0, q.H, q.W, TSH});
      __syncthreads();
    }
    return;
  }
  if constexpr (HID == 1) return;

  for (int head = head0; head < head1; ++head) {
  f32x4 acc[4][8];
  first_layer(head, acc);
  // ---- output layer from registers: this wave's 64 hidden channels = 2 k-steps of 32
  f32x4 oacc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) oacc[c][r] = 0.0f;
  {
    const float* b1 = q.b_first[head] + wave * 64 + 4 * g;
    const unsigned char* wo = q.w_out_perm[head];
    const float fsc = MX ? q.first_scale[head] : 1.0f;
    (void)fsc;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int ks2 = wave * 2 + s2;
      const bf16x8 ah = *wfrag(wo, 0, ks2, 0, 8, lane), al = *wfrag(wo, 0, ks2, 1, 8, lane);
      const f32x4 ba = *reinterpret_cast<const f32x4*>(b1 + 32 * s2);
      const f32x4 bb = *reinterpret_cast<const f32x4*>(b1 + 32 * s2 + 16);
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        if (!live(ct)) continue;
        float v[8], hi[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float bj = j < 4 ? ba[j] : bb[j - 4];
          v[j] = fmaxf(MX ? __builtin_fmaf(acc[2 * s2 + (j >> 2)][ct][j & 3], fsc, bj) : acc[2 * s2 + (j >> 2)][ct][j & 3] + bj, 0.0f);
          hi[j] = bf16_rne(v[j]);
        }
        const u32x4 ph = {pack2(hi[0], hi[1]), pack2(hi[2], hi[3]), pack2(hi[4], hi[5]), pack2(hi[6], hi[7])};
        const u32x4 pl = {pack2(v[0] - hi[0], v[1] - hi[1]), pack2(v[2] - hi[2], v[3] - hi[3]),
                          pack2(v[4] - hi[4], v[5] - hi[5]), pack2(v[6] - hi[6], v[7] - hi[7])};
        const bf16x8 xh = __builtin_bit_cast(bf16x8, ph), xl = __builtin_bit_cast(bf16x8, pl);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, xh, oacc[ct], 0, 0, 0);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xl, oacc[ct], 0, 0, 0);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xh, oacc[ct], 0, 0, 0);
      }
    }
  }
  const int n_out = p.n_out[head], act = p.act[head];
  float* red = reinterpret_cast<float*>(xt + hp16_patch_bytes(PC) + hp16_pc_extra(PC));   // [wave][n 16][px 128], BEHIND the patch (which the next head reuses)
#pragma unroll
  for (int ct = 0; ct < 8; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 4 * g + r;
      if (live(ct) && n < n_out) red[(wave * 16 + n) * HP_PX + ct * 16 + c16] = oacc[ct][r];
    }
  __syncthreads();
  {
    const int px = tid & (HP_PX - 1);
    const int y = y0 + (px >> TSH), x = x0 + (px & TMASK);
    // this thread's pixel of the map: (image ob, pixel opix) - dense: the tile's own; AT: the slot's, for the centre pixels of
    // non-empty slots
    bool valid = y < q.H && x < q.W;
    int ob = b;
    size_t opix = (size_t)y * q.W + x;
    if constexpr (AT) {
      const int sl = at_slot_of(px >> 4, px & 15);
      const int s = sl >= 0 ? at_slots[sl] : -1;
      valid = (unsigned)s < (unsigned)p.M;
      ob = s / p.HW;
      opix = (size_t)(s - ob * p.HW);
    }
    if (valid) {
      const float* bo = p.b_out[head];
      float* out = p.out[head];
      float* out2 = p.out2[head];
      for (int n = tid >> 7; n < n_out; n += 2) {
        const float raw = red[n * HP_PX + px] + red[(16 + n) * HP_PX + px] + red[(32 + n) * HP_PX + px] +
                          red[(48 + n) * HP_PX + px] + bo[n];
        const size_t o = ((size_t)ob * n_out + n) * p.HW + opix;
        float v = raw;
        if (act == CF_ACT_RELU) v = fmaxf(raw, 0.0f);
        else if (act == CF_ACT_SIGMOID_CLAMP) v = fminf(fmaxf(cf_sigmoid(raw), 1e-4f), 1.0f - 1e-4f);
        out[o] = v;
        if (act == CF_ACT_RAW_AND_SIGDEPTH) out2[o] = 1.0f / (cf_sigmoid(raw) + 1e-6f) - 1.0f;
      }
    }
  }
  __syncthreads();                           // the partial sums are consumed: the next head may overwrite them
  }                                          // head loop
}

// ---------------------------------------------------------------------------------------------
// fp32 NHWC feature map -> the 272-byte mx rows head_patch16_kernel<.., MX> stages (layout: there).  One thread per
// (pixel, 32-channel block); the arithmetic is cf_mx.h: mx_pack_block (shared with the DCN epilogue).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_feat_mx_kernel(const float* __restrict__ x, int in_stride,
                                                           unsigned char* __restrict__ rows, long M, float scale) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long m = t >> 1;
  const int blk = (int)(t & 1);
  if (m >= M) return;
  const f32x4* src = reinterpret_cast<const f32x4*>(x + m * in_stride + 32 * blk);
  float v[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4 q = src[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * i + e] = q[e];
  }
  mx_pack_block(v, rows + m * 272, blk, scale);
}

}  // namespace

extern "C" int cf_pack_feat_mx_scaled(const float* x, int in_stride, void* rows, long M, float scale, void* stream) {
  CF_REQUIRE(x && rows && M > 0, "cf_pack_feat_mx: null tensor or M=%ld", M);
  const float sc = cf_resolve_in_scale(scale);
  CF_REQUIRE(sc > 0.0f, "cf_pack_feat_mx_scaled: scale must be 0 (= 16) or a power of two");
  CF_REQUIRE(in_stride >= 64 && in_stride % 4 == 0, "cf_pack_feat_mx: in_stride=%d (64 channels, 16-byte aligned rows)", in_stride);
  CF_REQUIRE(M < (1L << 30), "cf_pack_feat_mx: M=%ld too large", M);
  const long threads = 2 * M;
  hipLaunchKernelGGL(pack_feat_mx_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     in_stride, static_cast<unsigned char*>(rows), M, sc);
  return cf_check_launch("cf_pack_feat_mx");
}

extern "C" int cf_pack_feat_mx(const float* x, int in_stride, void* rows, long M, void* stream) {
  return cf_pack_feat_mx_scaled(x, in_stride, rows, M, 16.0f, stream);
}

// the tail member of the argument block -> kernel arguments (tail.x / x_stride / c_base are not read: the hidden tile is born in LDS)
static int fill_tail(const cf_head_tail_args* a, HeadTailK& k) {
  CF_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cf_head_fused: bad geometry");
  CF_REQUIRE(a->n_heads >= 1 && a->n_heads <= CF_MAX_HEADS, "cf_head_fused: n_heads=%d", a->n_heads);
  CF_REQUIRE(a->n_hidden >= 0 && a->n_hidden <= 2, "cf_head_fused: n_hidden=%d", a->n_hidden);
  const long M = (long)a->B * a->H * a->W;
  CF_REQUIRE(M < (1L << 31), "cf_head_fused: tensor too large");
  k.x = reinterpret_cast<const unsigned char*>(a->x);
  k.x_stride = a->x_stride;
  k.M = (int)M;
  k.HW = a->H * a->W;
  k.n_heads = a->n_heads;
  k.n_hidden = a->n_hidden;
  for (int i = 0; i < a->n_heads; ++i) {
    for (int l = 0; l < a->n_hidden; ++l) {
      CF_REQUIRE(a->w_hidden[i][l] && a->b_hidden[i][l], "cf_head_fused: head %d layer %d weights missing", i, l);
      k.w_hidden[i][l] = reinterpret_cast<const unsigned char*>(a->w_hidden[i][l]);
      k.b_hidden[i][l] = a->b_hidden[i][l];
    }
    CF_REQUIRE(a->w_out[i] && a->b_out[i] && a->out[i], "cf_head_fused: head %d output layer missing", i);
    CF_REQUIRE(a->n_out[i] >= 1 && a->n_out[i] <= 32, "cf_head_fused: head %d n_out=%d", i, a->n_out[i]);
    CF_REQUIRE(a->act[i] != CF_ACT_RAW_AND_SIGDEPTH || a->out2[i], "cf_head_fused: head %d needs out2", i);
    k.w_out[i] = reinterpret_cast<const unsigned char*>(a->w_out[i]);
    k.b_out[i] = a->b_out[i];
    k.out[i] = a->out[i];
    k.out2[i] = a->out2[i];
    k.c_base[i] = a->c_base[i];
    k.n_out[i] = a->n_out[i];
    k.act[i] = a->act[i];
  }
  return CF_OK;
}

// The one form that runs: the canonical 3x3 slot order (layout3x3 = 1) over a 64-channel first source [and an 8-channel
// pc_hm source] with every weight packed as 16x16x32 fragments (mfma16 = 1).  The argument block can still spell the
// forms of the earlier kernels (32x32x16 fragments, an arbitrary slot table): those are refused, never reinterpreted.
constexpr int HEAD_MAX_K_PAD = 2048;   // bound of cf_head_fused_args.K_pad (64 chunks of 32)
#define CF_HEAD_FORMS "cf_head_fused runs layout3x3 = 1 (64-channel first source [, 8-channel second]) with mfma16 = 1 " \
                      "(16x16x32 fragments, n_out <= 16) only"

// slot_pixels == nullptr: the dense launch over the whole map; else n_tiles virtual tiles (cf_head_fused_at).
// tile / pc_skip: 0 or 1 forces that choice, -1 leaves it to the rule (cf_head_fused_with)
static int head_fused_launch(const cf_head_fused_args* a, const int* slot_pixels, int n_tiles, int tile, int pc_skip, void* stream) {
  const bool at = slot_pixels != nullptr;
  HeadPatchK hp{};
  hp.slot_pixels = slot_pixels;
  const int rc = fill_tail(&a->tail, hp.t);
  if (rc != CF_OK) return rc;
  CF_REQUIRE(a->n_src >= 1 && a->n_src <= 2, "cf_head_fused: n_src=%d", a->n_src);
  for (int i = 0; i < a->n_src; ++i) {
    CF_REQUIRE(a->src[i] && a->src_c[i] > 0 && a->src_c[i] % 8 == 0, "cf_head_fused: source %d invalid", i);
    hp.src[i] = reinterpret_cast<const unsigned char*>(a->src[i]);
    hp.src_c[i] = a->src_c[i];
  }
  const bool mx = a->mx != 0;                // first layer: fp16 main + FP6 cross terms on the mx feature rows
  if (mx) {                                  // the mx operand stream has no slot table
    CF_REQUIRE(a->layout3x3 && a->mfma16 && a->src_c[0] == 64 && (a->n_src == 1 || a->src_c[1] == 8),
               "cf_head_fused: mx = 1 needs layout3x3 = 1, mfma16 = 1, a 64-channel mx source [and an 8-channel pc_hm source]");
  } else {
    CF_REQUIRE(a->slots && a->K_pad > 0 && a->K_pad % 64 == 0, "cf_head_fused: K_pad=%d must be a multiple of 64", a->K_pad);
    CF_REQUIRE(a->K_pad <= HEAD_MAX_K_PAD, "cf_head_fused: K_pad=%d exceeds %d", a->K_pad, HEAD_MAX_K_PAD);
  }
  const int n_heads = a->tail.n_heads, H = a->tail.H, W = a->tail.W;
  for (int i = 0; i < n_heads; ++i) {
    CF_REQUIRE(a->w_first[i] && a->b_first[i], "cf_head_fused: head %d first layer missing", i);
    hp.w_first[i] = reinterpret_cast<const unsigned char*>(a->w_first[i]);
    hp.b_first[i] = a->b_first[i];
  }
  if (!(a->layout3x3 && a->src_c[0] == 64 && (a->n_src == 1 || a->src_c[1] == 8))) {
    // nothing but the 3x3 patch kernel reads 16x16x32 fragments
    CF_REQUIRE(a->mfma16 == 0, "cf_head_fused: mfma16 fragments need the 3x3 patch layout (layout3x3 = 1, 64-channel first "
                               "source [, 8-channel second]); this launch would run on the 32x32x16 slot-table kernel");
    cf_set_error(CF_HEAD_FORMS ": there is no slot-table kernel (layout3x3 = 0)");
    return CF_EINVAL;
  }
  // K order = 9 taps x 64 feature channels [, then ONE k-step of the pc_hm taps: k = 3 tap + channel]
  const bool m16 = a->mfma16 != 0;           // fragments packed for v_mfma_f32_16x16x32_bf16 (k-steps of 32)
  hp.H = H; hp.W = W;
  hp.n_ks = a->K_pad / 32;
  CF_REQUIRE(mx || a->K_pad / 16 >= (a->n_src == 2 ? 38 : 36), "cf_head_fused: K_pad=%d too small for the 3x3 layout", a->K_pad);
  for (int i = 0; i < n_heads; ++i) {
    CF_REQUIRE(!mx || (a->first_scale[i] > 0.0f && a->first_scale[i] < 1e30f), "cf_head_fused: head %d: first_scale missing (mx)", i);
    hp.first_scale[i] = a->first_scale[i];
  }
  if (m16) {
    CF_REQUIRE(mx || (a->K_pad % 32 == 0 && a->K_pad / 32 >= (a->n_src == 2 ? 19 : 18)), "cf_head_fused: K_pad=%d (16x16x32 fragments)", a->K_pad);
    for (int i = 0; i < n_heads; ++i)
      CF_REQUIRE(a->tail.n_out[i] <= 16, "cf_head_fused: head %d: n_out=%d > 16 (the 16x16x32 kernels produce ONE 16-row output tile, with or without hidden layers)", i, a->tail.n_out[i]);
  }
  for (int i = 0; i < n_heads; ++i) {
    CF_REQUIRE(a->tail.n_hidden > 0 || a->w_out_perm[i], "cf_head_fused: head %d: w_out_perm missing", i);
    hp.w_out_perm[i] = reinterpret_cast<const unsigned char*>(a->w_out_perm[i]);
  }
  // tile orientation: 8 x 16 or 16 x 8 pixels, whichever covers the map with fewer tiles (results do not depend on it)
  const long t_land = (long)((W + 15) / 16) * ((H + 7) / 8), t_port = (long)((W + 7) / 8) * ((H + 15) / 16);
  CF_REQUIRE(t_land * a->tail.B * n_heads < (1L << 31), "cf_head_fused: grid too large");   // (bounds either orientation's grid)
  CF_REQUIRE(m16, CF_HEAD_FORMS ": nothing reads 32x32x16 fragments (mfma16 = 0)");
  bool portrait = tile < 0 ? t_port < t_land : tile != 0;
  if (at) portrait = false;                  // (virtual tiles are flat)
  // workgroups whose pc_hm patch is all zero leave the pc_hm taps out (results do not depend on it)
  hp.pc_skip = pc_skip != 0;
  hp.tiles_x = portrait ? (W + 7) / 8 : (W + 15) / 16;
  hp.tiles_y = portrait ? (H + 15) / 16 : (H + 7) / 8;
  const int n_img = at ? 1 : a->tail.B;      // virtual tiles are not per image: the table holds flat pixels of the batch
  if (at) { hp.tiles_x = n_tiles; hp.tiles_y = 1; }
  // heads without hidden layers: a workgroup walks several heads on one patch (chosen below).  With hidden layers the
  // chain rewrites the patch: one head per workgroup.
  int hloop = 1;
  if (a->tail.n_hidden == 0) {
    // heads per workgroup: 1, 2 or half of them, whichever needs the fewest rounds of (2 workgroups per CU) x (heads +
    // a quarter of a head's time for the patch) - small batches want many short workgroups (bs=1: 103 vs 123 us with
    // 1 vs 4 heads), bs=16 the long ones (1307 vs 1331 us).  The results do not depend on it.
    static const int slots = [] {
      int dev = 0, cus = 256;
      if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
      return 2 * (cus > 0 ? cus : 256);
    }();
    const long tiles = (long)hp.tiles_x * hp.tiles_y * n_img;
    const int n = n_heads, cand[3] = {1, 2, (n + 1) / 2};
    double best = 0.0;
    for (int i = 0; i < 3; ++i) {
      const int h = cand[i] < 1 ? 1 : (cand[i] > n ? n : cand[i]);
      const double cost = (double)((tiles * ((n + h - 1) / h) + slots - 1) / slots) * (h + 0.25);
      if (i == 0 || cost < best - 1e-9) { best = cost; hloop = h; }
    }
  }
  hp.hloop = hloop;
  const long blocks = (long)hp.tiles_x * hp.tiles_y * n_img * ((n_heads + hloop - 1) / hloop);
  CF_REQUIRE(blocks < (1L << 31), "%s: grid too large", at ? "cf_head_fused_at" : "cf_head_fused");
  const bool hidden = a->tail.n_hidden > 0;
  const bool pc = a->n_src == 2;
  const int lds = hp16_lds(pc, hidden);
  auto launch = [&](auto kernel, CfLdsLimit& lim) {
    lim.ensure(kernel, lds, hp16_lds(pc, false));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, hp);
  };
  static CfLdsLimit lim16[4], limx[4], limxh[2], lim_at[4];
  if (at) {
    // the forms of the dense launch on virtual tiles (these instantiations may use scratch: a launch is one workgroup's
    // lifetime long, not a throughput loop)
    CF_REQUIRE(!mx || hidden == pc, "cf_head_fused_at: mx = 1 runs without hidden layers and pc_hm source, or with both (the forms "
                                    "the model's head groups take); pack other heads for bf16x3");
    if (mx && hidden) launch(head_patch16_kernel<4, true, false, true, 1, true>, lim_at[3]);
    else if (mx) launch(head_patch16_kernel<4, false, false, true, 0, true>, lim_at[2]);
    else if (pc) launch(head_patch16_kernel<4, true, false, false, -1, true>, lim_at[1]);
    else launch(head_patch16_kernel<4, false, false, false, -1, true>, lim_at[0]);
    return cf_check_launch("cf_head_fused_at");
  }
  if (mx && hidden) {
    // (hidden layers behind an mx first layer WITHOUT the pc_hm source: that instantiation does not fit 256 registers
    //  without scratch, and no configuration of the reference has such heads - its packing stays bf16x3)
    CF_REQUIRE(pc, "cf_head_fused: mx = 1 with hidden layers needs the pc_hm source (n_src = 2); pack such heads for bf16x3");
    if (portrait) launch(head_patch16_kernel<4, true, true, true, 1>, limxh[1]);
    else launch(head_patch16_kernel<4, true, false, true, 1>, limxh[0]);
  } else if (mx) {
    if (pc && portrait) launch(head_patch16_kernel<4, true, true, true, 0>, limx[3]);
    else if (pc) launch(head_patch16_kernel<4, true, false, true, 0>, limx[2]);
    else if (portrait) launch(head_patch16_kernel<4, false, true, true, 0>, limx[1]);
    else launch(head_patch16_kernel<4, false, false, true, 0>, limx[0]);
  } else {
    if (pc && portrait) launch(head_patch16_kernel<4, true, true>, lim16[3]);
    else if (pc) launch(head_patch16_kernel<4, true, false>, lim16[2]);
    else if (portrait) launch(head_patch16_kernel<4, false, true>, lim16[1]);
    else launch(head_patch16_kernel<4, false, false>, lim16[0]);
  }
  return cf_check_launch("cf_head_fused");
}

extern "C" int cf_head_fused_with(const cf_head_fused_args* a, int tile, int pc_skip, void* stream) {
  CF_REQUIRE(a != nullptr, "cf_head_fused: null args (a)");
  CF_REQUIRE(tile >= -1 && tile <= 1, "cf_head_fused_with: tile=%d is not 0 (8 x 16), 1 (16 x 8) or -1 (the rule's own)", tile);
  CF_REQUIRE(pc_skip >= -1 && pc_skip <= 1, "cf_head_fused_with: pc_skip=%d is not 0, 1 or -1 (the rule's own)", pc_skip);
  return head_fused_launch(a, nullptr, 0, tile, pc_skip, stream);
}

extern "C" int cf_head_fused(const cf_head_fused_args* a, void* stream) { return cf_head_fused_with(a, -1, -1, stream); }

extern "C" int cf_head_fused_at(const cf_head_fused_args* a, const int32_t* slot_pixels, int n_tiles, void* stream) {
  CF_REQUIRE(a != nullptr, "cf_head_fused_at: null args");
  CF_REQUIRE(slot_pixels != nullptr && n_tiles > 0, "cf_head_fused_at: slot table missing or n_tiles=%d", n_tiles);
  const int rc = head_fused_launch(a, slot_pixels, n_tiles, -1, -1, stream);
  if (rc == CF_EINVAL) {                     // (the shared checks name cf_head_fused: say which entry point was called)
    const std::string why = cf_last_error();
    cf_set_error("cf_head_fused_at: %s", why.c_str());
  }
  return rc;
}

// ---------------------------------------------------------------------------------------------
// The slot tables of cf_head_fused_at from up to two (B, K) lists of pixel indices (the frustum chain's top-K, the decoder's
// NMS peaks).  One thread per table entry.
// ---------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void head_slot_tables_kernel(const int* __restrict__ tk, const int* __restrict__ pk, int B, int K,
                                                               int HW, int* __restrict__ tp, int* __restrict__ ts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int per_p = (2 * K + AT_SLOTS - 1) / AT_SLOTS * AT_SLOTS, per_s = (K + AT_SLOTS - 1) / AT_SLOTS * AT_SLOTS;
  if (tp && i < B * per_p) {
    const int b = i / per_p, j = i - b * per_p;
    int v = -1;
    if (j < K) v = tk ? tk[b * K + j] : -1;
    else if (j < 2 * K) v = pk ? pk[b * K + j - K] : -1;
    tp[i] = (unsigned)v < (unsigned)HW ? b * HW + v : -1;
  }
  if (ts && i < B * per_s) {
    const int b = i / per_s, j = i - b * per_s;
    const int v = (j < K && pk) ? pk[b * K + j] : -1;
    ts[i] = (unsigned)v < (unsigned)HW ? b * HW + v : -1;
  }
}
}  // namespace

extern "C" int cf_head_slot_tables(const int32_t* list_a, const int32_t* list_b, int B, int K, int HW, int32_t* table_ab,
                                   int32_t* table_b, void* stream) {
  CF_REQUIRE(B > 0 && K > 0 && HW > 0, "cf_head_slot_tables: B=%d K=%d HW=%d", B, K, HW);
  CF_REQUIRE((long)B * HW < (1L << 31), "cf_head_slot_tables: B * HW must stay below 2^31 (flat pixels are int32)");
  CF_REQUIRE((long)B * (2L * K + AT_SLOTS) < (1L << 31), "cf_head_slot_tables: B * K too large");
  CF_REQUIRE(list_a || list_b, "cf_head_slot_tables: no list");
  CF_REQUIRE(table_ab || table_b, "cf_head_slot_tables: no table");
  CF_REQUIRE(!table_b || list_b, "cf_head_slot_tables: table_b is built from list_b");
  const long n = (long)B * ((2 * K + AT_SLOTS - 1) / AT_SLOTS * AT_SLOTS);   // (the larger table)
  hipLaunchKernelGGL(head_slot_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, list_a,
                     list_b, B, K, HW, table_ab, table_b);
  return cf_check_launch("cf_head_slot_tables");
}
