// 3x3 / stride 1 / pad 1 convolution on the f16x3 scheme (fp32 storage, split-fp16 products - see the
// numerics note in cf_gemm_f16.hip) with PATCH REUSE: the generic slot kernel re-gathers and re-splits
// every input element once per tap (9x); here a workgroup owns R = 64*WP consecutive pixels of the
// flattened (B*H*W) index space and, per 16-channel slice, stages the flat row range
//     [m0 - W - 1, m0 + R + W + 1)
// ONCE - fp32 rows -> fp16 hi/lo -> LDS.  All 9 taps then read their B fragments from that patch at
// row offset (dy+1)*W + (dx+1); a lane whose tap leaves the image (or the batch element) is pointed
// at an all-zero row instead, so borders cost one select per fragment address.  Per slice that is one
// barrier and one operand split for 9 k-steps of MFMA work, and (R + 2W + 2)/R <= 2.6x input
// traffic instead of 9x.
//
// K order is SLICE-MAJOR: k-step index ks = slice * 9 + tap (packing.pack_conv_f16(slice_major=True)
// emits the slot table in that order, so the generic kernel cf_conv2d_f16x3 computes the same sums
// from the same packed weights - it is the fallback for feature maps too wide for the LDS patch).
//
// Workgroup = 4 waves as WC (32*RT-channel groups) x WP (64-pixel groups) x WK (slices in flight:
// the patch then carries 16*WK channels per round and wave wk multiplies slice wk; partial sums are
// added in fixed wave order through LDS at the end).  WK > 1 is for small feature maps with many
// input channels (the 14x25 / 28x50 offset convolutions), where pixel tiles alone cannot fill 256 CUs.
//
// STRIDE 2 (S2, tiled form only; the four BasicBlock conv1 layers that open levels 2-5, dla.py:124-145): an output tile of
// TH x 16 pixels needs the (2 TH + 1) x 33 input pixels around it.  The patch keeps each input row as two PLANES - the
// 17 odd columns 2 (x0 + j) - 1, then the 16 even columns 2 (x0 + j) - so that tap (dy, dx) of output pixel (py, px) sits
// at row 2 py + dy, entry {px, 17 + px, px + 1}[dx]: a compile-time offset per tap, exactly as in the stride-1 tile.  Every
// input element is fetched and split ~1.1 times instead of the slot kernel's 2.25.
//
// Replaces the 3x3 convolutions of model/networks/dla.py:42-62, 124-145 (BasicBlock conv1/conv2) and
// the conv_offset_mask of model/networks/dla.py:406-414 (DeformConv) on the device.
//
// LAUNCH CHOICE, host side, in four steps that every entry point walks and nothing else decides:
//   Conv3Form       the kernel's template parameters as a value
//   conv3_fits      form + geometry -> grid, threads, LDS bytes, patch rows, rounds - or "does not fit"
//   conv3_pick      THE rule: launch variant + geometry -> the first fitting form of an ordered candidate list
//   conv3_dispatch  CF_CONV3_TILES, the one list of instantiated forms: picked form -> its kernel instantiation
// cf_conv3x3_tile_form reports the pick without touching the HIP runtime (tests/test_f16x3_forms_cpu.py sweeps it).
#include "cf_f16x3.h"

namespace {

#define CF_MFMA_F16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)

struct Conv3F {
  const float* x;               // fp32 NHWC, first channel of the source
  const unsigned char* weight;  // [N_pad/32][n_ks][2][64][8 f16]
  const float* bias;
  const float* residual;
  float* out;
  int x_stride, H, W, HW, M, N, n_rt, n_ks, n_rounds, res_stride, out_stride, act, PR;   // H, W, HW, M: the OUTPUT map
  int tiles_x, tiles_y;         // T2 only
  int Hi, Wi, HWi;              // S2 only: the input map (H, W are then the output's)
  // ROOT only: the Tree's 1x1 Root over (this convolution's output x2, its residual x1) run from the epilogue
  const unsigned char* root_w;  // [2][8 k-steps][2][64][8 f16]: K = (x2 channels 0..63, x1 channels 0..63)
  const float* root_bias;
  float* root_out;
  int root_out_stride, root_act;
  float root_scale;
  // ... and the Root's further sources (the Tree's children: dla.py:109-117), K order behind x2 and x1
  const float* root_xsrc[2];
  int root_xsrc_c[2], root_xsrc_ch[2];   // floats per pixel, channels (multiples of 64)
  int root_nks;                          // k-steps of the whole Root: (2 N + children's channels) / 16
  float out_scale;
  float in_scale;        // activation pre-scale of this convolution's operands (patch rows, projected rows)
  float root_in_scale;   // ROOT only: ... and of the Root GEMM's operands (x2, x1, the children)
  // PROJ only: a 1x1 convolution of a second tensor (same map as the output) summed into the same accumulators
  const float* proj_x;
  int proj_c, proj_ch, proj_nks, proj_ks0;   // floats per pixel, channels (multiple of 32), k-steps, first k-step in the stream
};

// GROUPED form (cf_conv3x3_f16x3_grouped): n_groups convolutions of ONE geometry (H, W, M, N, strides, k-steps) on independent
// inputs with their own weights as one grid of n_groups x tiles workgroups - the IDA projections' offset convolutions, which
// each sit on the ~32 us launch floor.  Workgroup b belongs to group b / n_tiles and is tile
// b % n_tiles OF THAT GROUP: every index below (m0, the patch rows' range test, m < M) stays group-local, so a tile never
// reaches into the next group's rows; only the operand pointers and the first output row are the group's.
constexpr int CF_GROUPS = 4;
struct Conv3G {
  int n_tiles;                                  // workgroups (gridDim.x) per group
  const float* x[CF_GROUPS];
  const unsigned char* weight[CF_GROUPS];
  const float* bias[CF_GROUPS];
  float in_scale[CF_GROUPS], out_scale[CF_GROUPS];
};

// T2: the R pixels are an (R/16) x 16 tile of ONE image instead of a flat run: the patch is the tile
// plus a one-pixel frame, (R/16 + 2) x 18 rows, zero-filled outside the image - so no tap needs a
// validity select and the tap offsets are compile-time constants.  Pays on wide maps (W = 200: 1.3x
// input traffic instead of 2.6x) whenever W is close to a multiple of 16.
// CT = 32-pixel column tiles per wave: 2 (64 x 64 wave tiles, two waves per SIMD at 256 registers each) or 1 (half-size
// tiles for small grids, below).  The kernel is generic in CT; the one-wave-per-SIMD form CT = 4 (MINB = 1, 512 registers:
// both accumulator sets of a 64-channel x 128-pixel tile in AGPRs) measured slower and is not instantiated: DESIGN.md section 9.
// ROOT (BasicBlock conv2 of a one-level Tree without children, dla.py:105-118, 33-41; N = 64 WC channels, all of them in
// this workgroup): the Tree's Root - ReLU(W_root . [x2; x1] + b), x2 = this convolution's output, x1 = its residual -
// runs from the epilogue.  Every wave splits its 64 channels of x2 (bias, residual, ReLU applied) and of x1 to fp16
// hi / lo into its two LDS regions, which ARE pieces of the B operand of the 1x1 GEMM; after a barrier (WC > 1: the WC
// waves of a pixel group read each other's pieces) 8 WC k-steps of MFMAs follow in the slot kernel's order, each wave
// producing its own 64 output channels.  Only the Root's output goes to HBM: x2 is never written (unless p.out is
// given), x1 is read once for both uses, one launch less.
// PROJ (BasicBlock conv2 of the sub-tree that opens a DLA level: its residual is the Tree's `project` - 1x1 convolution
// + BN - of the 2x2-max-pooled level input, dla.py:96-107, 56-62): the projection's k-steps run behind the 3x3 part, into
// the same accumulators, so the residual never exists as a tensor and its launch is gone.  B tiles of 32 pixels x 64 channels:
// the WC x WK waves of a pixel group each fetch one 64-channel piece of the pooled rows from HBM (whole rows), split it
// to fp16 hi / lo into their LDS region, and after the group's barrier every wave multiplies the round's pieces in K
// order (WK > 1: piece i goes to K-split wave i % WK).  The regions are the patch buffers' memory (dead by then).
#define CF_CONV3_GROUPED 0
#include "cf_conv3x3_f16_kernel.h"   // conv3x3_f16x3_kernel
#undef CF_CONV3_GROUPED
#define CF_CONV3_GROUPED 1
#include "cf_conv3x3_f16_kernel.h"   // conv3x3_f16x3_kernel_grouped
#undef CF_CONV3_GROUPED

// ---- 1. the template parameters of conv3x3_f16x3_kernel / _grouped as a value
struct Conv3Form {
  int WC, WP, WK, RT, NU;
  bool DB;
  int MINB;
  bool T2;
  int CT;
  bool S2, ROOT, PROJ, GRP;   // the launch variant: at most one of them
};

// The tile shapes that are instantiated, and for which launch variants: the ONE list conv3_pick names its candidates from
// and conv3_dispatch maps a picked form to its kernel through.  Named c<channels per workgroup>_<pixel tile>: flat<R> = a
// flat run of R pixels, <TH>x16 = a tiled patch (T2); k<WK> = K split over WK waves; w8 = eight waves.
//   X(name, WC, WP, WK, RT, NU, DB, MINB, T2, CT, variants)
enum { V_PLAIN = 1, V_PROJ = 2, V_ROOT = 4, V_GRP = 8, V_S2 = 16 };
#define CF_CONV3_TILES(X)                                                        \
  /* N_pad = 32: the offset convolutions, alone or grouped */                    \
  X(c32_8x16, 1, 4, 1, 1, 4, true, 2, true, 1, V_PLAIN | V_GRP)                  \
  X(c32_16x16, 1, 4, 1, 1, 6, true, 2, true, 2, V_PLAIN | V_GRP)                 \
  X(c32_flat256, 1, 4, 1, 1, 8, true, 2, false, 2, V_PLAIN | V_GRP)              \
  X(c32_flat256_wide, 1, 4, 1, 1, 12, true, 1, false, 2, V_PLAIN | V_GRP)        \
  X(c32_flat64_k4, 1, 1, 4, 1, 8, true, 2, false, 2, V_PLAIN | V_GRP)            \
  X(c32_flat64_k4_wide, 1, 1, 4, 1, 12, true, 2, false, 2, V_PLAIN | V_GRP)      \
  X(c32_flat128_k2, 1, 2, 2, 1, 12, true, 2, false, 2, V_PLAIN | V_GRP)          \
  /* 64+ channels, with or without the projection k-steps or the fused Root */   \
  X(c64_8x16, 1, 4, 1, 2, 4, true, 2, true, 1, V_PLAIN | V_PROJ | V_ROOT)        \
  X(c64_16x16, 1, 4, 1, 2, 6, true, 2, true, 2, V_PLAIN | V_PROJ | V_ROOT)       \
  X(c64_flat256, 1, 4, 1, 2, 6, true, 2, false, 2, V_PLAIN | V_PROJ | V_ROOT)    \
  X(c128_8x16, 2, 2, 1, 2, 4, true, 2, true, 2, V_PLAIN | V_PROJ | V_ROOT)       \
  X(c128_flat128, 2, 2, 1, 2, 6, true, 2, false, 2, V_PLAIN | V_PROJ | V_ROOT)   \
  X(c128_flat32_k2, 2, 1, 2, 2, 4, true, 2, false, 1, V_PLAIN | V_PROJ)          \
  X(c128_flat64_k2, 2, 1, 2, 2, 4, true, 2, false, 2, V_PLAIN | V_PROJ)          \
  X(c256_flat32, 4, 1, 1, 2, 4, true, 2, false, 1, V_PLAIN | V_PROJ | V_ROOT)    \
  X(c256_flat128_w8, 4, 2, 1, 2, 2, true, 1, false, 2, V_PLAIN | V_PROJ)         \
  X(c256_8x16_w8, 4, 2, 1, 2, 2, true, 1, true, 2, V_PLAIN | V_PROJ)             \
  X(c256_flat64, 4, 1, 1, 2, 4, true, 2, false, 2, V_PLAIN | V_PROJ | V_ROOT)    \
  X(c256_4x16, 4, 1, 1, 2, 2, true, 2, true, 2, V_PLAIN | V_PROJ | V_ROOT)       \
  /* stride 2 */                                                                 \
  X(c64_s2_8x16, 1, 4, 1, 2, 9, false, 2, true, 1, V_S2)                         \
  X(c128_s2_4x16, 2, 2, 1, 2, 5, true, 2, true, 1, V_S2)                         \
  X(c256_s2_2x16, 4, 1, 1, 2, 3, true, 2, true, 1, V_S2)                         \
  X(c256_s2_4x16, 4, 1, 1, 2, 5, true, 2, true, 2, V_S2)

#define X(name, WC, WP, WK, RT, NU, DB, MINB, T2, CT, V) constexpr Conv3Form name{WC, WP, WK, RT, NU, DB, MINB, T2, CT, false, false, false, false};
CF_CONV3_TILES(X)
#undef X

constexpr int conv3_variant(const Conv3Form& f) { return f.S2 ? V_S2 : f.ROOT ? V_ROOT : f.PROJ ? V_PROJ : f.GRP ? V_GRP : V_PLAIN; }

constexpr Conv3Form conv3_as(Conv3Form f, int variant) {
  f.S2 = variant == V_S2; f.ROOT = variant == V_ROOT; f.PROJ = variant == V_PROJ; f.GRP = variant == V_GRP;
  return f;
}

// ---- 2. does a form fit a launch, and with which launch parameters
struct Conv3Geo {
  int B, H, W;          // the INPUT map (stride 2: the output is Ho x Wo; otherwise the same)
  int Ho, Wo, N_pad;
  int slices;           // 16-channel slices of the 3x3 input
  long M() const { return (long)B * Ho * Wo; }
};

struct Conv3Launch {
  long blocks;          // gridDim.x (per group of a grouped launch)
  int grid_y, threads;
  size_t lds;           // dynamic LDS bytes
  int PR, tiles_x, tiles_y, n_rounds;   // Conv3F's fields of the same names
};

bool conv3_fits(const Conv3Form& f, const Conv3Geo& g, int n_groups, Conv3Launch* L) {
  if (g.slices % f.WK != 0) return false;
  const int R = 32 * f.CT * f.WP, ROWB = 64 * f.WK + 16, NT = 64 * f.WC * f.WP * f.WK;
  *L = Conv3Launch{};
  if (f.T2) {
    L->PR = f.S2 ? (2 * (R / 16) + 1) * 33 : (R / 16 + 2) * 18;
    L->tiles_x = (g.Wo + 15) / 16;
    L->tiles_y = (g.Ho + R / 16 - 1) / (R / 16);
    L->blocks = (long)L->tiles_x * L->tiles_y * g.B;
  } else {
    L->PR = R + 2 * g.Wo + 2;
    L->blocks = (g.M() + R - 1) / R;
  }
  const long units = (long)L->PR * 4 * f.WK;
  if (units > (long)NT * f.NU || L->blocks >= (1L << 31) || L->blocks * n_groups >= (1L << 31)) return false;
  size_t dyn = (size_t)(f.DB ? 2 : 1) * (L->PR + 1) * ROWB;
  const size_t wk_min = (size_t)4 * f.RT * f.CT * 16 * 64 * 4;               // WK > 1: the partial sums' exchange
  if (f.WK > 1 && dyn < wk_min) dyn = wk_min;
  const size_t epi = (size_t)(NT / 64) * 32 * (f.RT * 128 + 16);             // the waves' transposition tiles
  if (f.WK == 1 && NT == 256 && dyn < epi) dyn = epi;
  if (dyn > 160 * 1024) return false;
  if (f.S2 && f.MINB >= 2 && dyn > 80 * 1024) return false;
  if (f.ROOT) {
    const size_t root_lds = (size_t)4 * 2 * 9216;   // four waves x two regions
    if (dyn < root_lds) dyn = root_lds;
    if (dyn > 80 * 1024) return false;
  }
  if (f.PROJ) {
    const size_t proj_lds = (size_t)(NT / 64) * 9216;   // one B-tile region per wave
    if (dyn < proj_lds) dyn = proj_lds;
  }
  L->lds = dyn;
  L->threads = NT;
  L->grid_y = (g.N_pad / 32 + f.WC * f.RT - 1) / (f.WC * f.RT);
  L->n_rounds = g.slices / f.WK;
  return true;
}

// 16 x 16 tiles cover the map with at most ~6 % of the tile area outside it
bool tiles_fit(int H, int W) {
  const long covered = (long)((H + 15) / 16) * 16 * ((W + 15) / 16) * 16;
  return covered * 100 <= (long)H * W * 106;
}

// ---- 3. THE rule: the first fitting form of the variant's ordered candidate list; false = none.  variant: V_PLAIN, V_S2,
// V_ROOT (the fused conv2 + Root launch only: none = run the V_PLAIN pick and the Root as its own launch), V_PROJ, V_GRP
// (n_groups convolutions as one grid: the N_pad = 32 list of V_PLAIN, whose one-round count sees the whole grid).
struct Conv3Pick {
  Conv3Form form;
  Conv3Launch launch;
};

bool conv3_pick(int variant, const Conv3Geo& g, int n_groups, Conv3Pick* pick) {
  const Conv3Form* cand[8];
  int n = 0;
  auto add = [&](bool cond, const Conv3Form& f) { if (cond) cand[n++] = &f; };
  const long HW = (long)g.H * g.W, M = g.M();
  const bool big = HW >= 4096;                    // (never a function of the batch size: WK changes the
                                                  //  summation order, and a shard of a batch has to
                                                  //  reproduce the full batch bit for bit)
  const bool t2 = big && tiles_fit(g.H, g.W);
  // SMALL GRIDS (small batches): while a launch of half-size pixel tiles (CT = 1: 32 pixels per wave) still fits the chip
  // in one round - at most one workgroup per CU - it is a third faster than the default tile, whose handful of
  // workgroups each walk twice the MFMAs per round on an otherwise empty chip (bs=1, 128 -> 128 at 56x100: 16.6 vs
  // 25.8 us; 256 -> 256 at 28x50: 27.5 vs 41.2 us; 512 -> 512 at 14x25: 31.8 vs 43.2 us; at 262 workgroups the gain is
  // gone).  The tile shape changes no sum (same K order, same WK): results are bit-identical, so this MAY depend on the
  // batch size; the patch is tiled (8 x 16) whatever the map - tile quantisation costs nothing on an empty chip.
  const long tiles8x16 = (long)((g.H + 7) / 8) * ((g.W + 15) / 16) * g.B;
  const long runs32 = (M + 31) / 32;
  auto one_round = [](long wgs) { return wgs <= 256; };
  if (variant == V_ROOT) {
    // small launches (latency chains of bs = 1 ... 4): the half-height tiles of the unfused path, fused - one launch less
    // where the whole chain is a handful of under-filled launches
    if (g.N_pad == 64 && one_round(tiles8x16)) {
      add(true, c64_8x16);
    } else if (g.N_pad == 256 && HW > 512 && one_round(runs32)) {
      add(true, c256_flat32);
    } else if (g.N_pad == 64) {
      add(t2, c64_16x16); add(true, c64_flat256);
    } else if (g.N_pad == 128 && !one_round(2 * tiles8x16)) {
      add(t2, c128_8x16); add(true, c128_flat128); add(true, c128_8x16);
    } else if (g.N_pad == 256 && HW > 512) {
      add(true, c256_flat64); add(true, c256_4x16);
    }
  } else if (variant == V_S2) {
    // stride 2: 4 x 16 or 8 x 16 output tiles by output width; a geometry the patch does not fit goes to the slot kernel
    if (g.N_pad == 64) add(true, c64_s2_8x16);
    else if (g.N_pad == 128) add(true, c128_s2_4x16);
    else if (g.N_pad >= 256) {
      // half-height tiles (2 x 16) while that grid still fits the chip in one round (level 5 of a bs <= 8 launch: 34.5 vs
      // 47.9 us); same sums whatever the tile, so this may depend on the batch size (as the stride-1 small-grid rule)
      const long half_tiles = (long)((g.Ho + 1) / 2) * ((g.Wo + 15) / 16) * g.B * ((g.N_pad + 255) / 256);
      add(true, one_round(half_tiles) ? c256_s2_2x16 : c256_s2_4x16);
    }
  } else if (g.N_pad == 32) {
    if (big) {
      add(one_round(tiles8x16 * n_groups), c32_8x16);
      add(t2, c32_16x16); add(true, c32_flat256); add(true, c32_flat256_wide);
    } else {
      add(true, c32_flat64_k4); add(true, c32_flat64_k4_wide); add(true, c32_flat128_k2); add(true, c32_flat256_wide);
    }
  } else if (g.N_pad == 64) {
    add(one_round(tiles8x16), c64_8x16); add(t2, c64_16x16); add(true, c64_flat256);
  } else if (g.N_pad == 128) {
    // (the one-wave-per-SIMD form - CT = 4, 64-channel x 128-pixel wave tiles, accumulators in AGPRs - was bit-identical
    //  and measured 97-123 us against 76-92 us here: DESIGN.md section 9)
    // wide maps (3x896x1600: level 3 is 112 x 200): 8 x 16 tiles with a frame - the flat run's patch (R + 2W + 2 rows)
    // no longer fits, and falling back to the slot kernel re-gathers every input 9 times
    add(one_round(2 * tiles8x16), c64_8x16);   // (64 channels per workgroup)
    add(t2, c128_8x16); add(true, c128_flat128);
    add(true, c128_8x16);                      // (8 waves x 256 pixels measured 4 % slower here)
  } else {
    // 256+ channels: every 64-pixel tile streams the whole weight matrix from L2, which bounds these
    // layers - with enough tiles to go round, 8 waves (two pixel groups per channel group, 128 pixels)
    // halve that stream (the second group's fragment loads hit L1)
    const long tiles128 = (M + 127) / 128 * ((g.N_pad + 255) / 256);
    // smallest maps (level5, 14x25): 128 channels x 64 pixels per workgroup with K split over wave pairs
    // doubles the workgroup count and halves every wave's round chain (per-image rule, see above)
    if (HW <= 512) {
      add(one_round(runs32 * ((g.N_pad + 127) / 128)), c128_flat32_k2); add(true, c128_flat64_k2);
    }
    add(one_round(runs32 * ((g.N_pad + 255) / 256)), c256_flat32);
    // (the tiled forms behind the flat ones: maps wider than ~60 / ~95 pixels, e.g. level 4 of a 3x896x1600 input)
    add(tiles128 >= 160, c256_flat128_w8); add(tiles128 >= 160, c256_8x16_w8);
    add(true, c256_flat64); add(true, c256_4x16);
  }
  for (int i = 0; i < n; ++i) {
    pick->form = conv3_as(*cand[i], variant);
    if (conv3_fits(pick->form, g, n_groups, &pick->launch)) return true;
  }
  return false;
}

// ---- 4. picked form -> its instantiation (each with its own CfLdsLimit); a form CF_CONV3_TILES does not list is an error
template <int WC, int WP, int WK, int RT, int NU, bool DB, int MINB, bool T2, int CT, bool S2, bool ROOT, bool PROJ, bool GRP>
void conv3_launch(const Conv3F& k, const Conv3Launch& L, const Conv3G* grp, int n_groups, hipStream_t st) {
  static CfLdsLimit lds_limit;                // (one per template instantiation)
  const dim3 grid((unsigned)(L.blocks * n_groups), (unsigned)L.grid_y);
  if constexpr (GRP) {
    Conv3G g = *grp;
    g.n_tiles = (int)L.blocks;
    auto kernel = conv3x3_f16x3_kernel_grouped<WC, WP, WK, RT, NU, DB, MINB, T2, CT>;
    lds_limit.ensure(kernel, L.lds, 65536);
    hipLaunchKernelGGL(kernel, grid, dim3(L.threads), L.lds, st, k, g);
  } else {
    auto kernel = conv3x3_f16x3_kernel<WC, WP, WK, RT, NU, DB, MINB, T2, CT, S2, ROOT, PROJ>;
    lds_limit.ensure(kernel, L.lds, 65536);
    hipLaunchKernelGGL(kernel, grid, dim3(L.threads), L.lds, st, k);
  }
}

template <int V, int WC, int WP, int WK, int RT, int NU, bool DB, int MINB, bool T2, int CT, typename... A>
bool conv3_launch_if(const Conv3Form& f, const A&... args) {
  if (f.WC != WC || f.WP != WP || f.WK != WK || f.RT != RT || f.NU != NU || f.DB != DB || f.MINB != MINB || f.T2 != T2 || f.CT != CT ||
      !(conv3_variant(f) & V))
    return false;
  const int v = conv3_variant(f);
  if constexpr ((V & V_PLAIN) != 0) if (v == V_PLAIN) conv3_launch<WC, WP, WK, RT, NU, DB, MINB, T2, CT, false, false, false, false>(args...);
  if constexpr ((V & V_PROJ) != 0) if (v == V_PROJ) conv3_launch<WC, WP, WK, RT, NU, DB, MINB, T2, CT, false, false, true, false>(args...);
  if constexpr ((V & V_ROOT) != 0) if (v == V_ROOT) conv3_launch<WC, WP, WK, RT, NU, DB, MINB, T2, CT, false, true, false, false>(args...);
  if constexpr ((V & V_GRP) != 0) if (v == V_GRP) conv3_launch<WC, WP, WK, RT, NU, DB, MINB, T2, CT, false, false, false, true>(args...);
  if constexpr ((V & V_S2) != 0) if (v == V_S2) conv3_launch<WC, WP, WK, RT, NU, DB, MINB, T2, CT, true, false, false, false>(args...);
  return true;
}

int conv3_dispatch(const Conv3Pick& p, Conv3F k, const Conv3G* grp, int n_groups, hipStream_t st, const char* who) {
  const Conv3Form& f = p.form;
  k.PR = p.launch.PR; k.tiles_x = p.launch.tiles_x; k.tiles_y = p.launch.tiles_y; k.n_rounds = p.launch.n_rounds;
#define X(name, WC, WP, WK, RT, NU, DB, MINB, T2, CT, V) \
  if (conv3_launch_if<V, WC, WP, WK, RT, NU, DB, MINB, T2, CT>(f, k, p.launch, grp, n_groups, st)) return cf_check_launch(who);
  CF_CONV3_TILES(X)
#undef X
  CF_REQUIRE(false, "%s: the picked form <%d, %d, %d, %d, %d, %d, %d, %d, %d; S2 %d ROOT %d PROJ %d GRP %d> is not instantiated", who, f.WC, f.WP,
             f.WK, f.RT, f.NU, f.DB, f.MINB, f.T2, f.CT, f.S2, f.ROOT, f.PROJ, f.GRP);
}

// cf_conv3x3_tile_form's answer: {patch kernel runs (0: forwarded to cf_conv2d_f16x3), conv2 + Root fused, the 13 fields of
// Conv3Form, the 8 of Conv3Launch}; without a patch launch the 21 form / launch entries are -1
void conv3_report(int32_t* out, const Conv3Pick* p) {
  for (int i = 0; i < CF_CONV3_FORM_INTS; ++i) out[i] = -1;
  out[0] = p != nullptr;
  out[1] = p != nullptr && p->form.ROOT;
  if (!p) return;
  const Conv3Form& f = p->form;
  const Conv3Launch& L = p->launch;
  const int32_t v[21] = {f.WC, f.WP, f.WK, f.RT, f.NU, f.DB, f.MINB, f.T2, f.CT, f.S2, f.ROOT, f.PROJ, f.GRP,
                         (int32_t)L.blocks, L.grid_y, L.threads, (int32_t)L.lds, L.PR, L.tiles_x, L.tiles_y, L.n_rounds};
  for (int i = 0; i < 21; ++i) out[2 + i] = v[i];
}

}  // namespace

// A geometry that fits no patch configuration is forwarded to cf_conv2d_f16x3 (same packed weights).
// root != nullptr (cf_conv3x3_root_f16x3, already validated): try the fused conv2 + Root launch first; *fused says whether it ran.
// proj_ch != nullptr (cf_conv3x3_proj_f16x3, already validated): src[1] is the 1x1 projection's source, proj_ch = the real
// channels of (the 3x3 source, the projection's source).
// report != nullptr (cf_conv3x3_tile_form): validate and pick as the launch does, write the answer, touch no runtime.
static int conv3x3_impl(const cf_conv_args* a, const cf_conv_args* root, const int32_t* root_ch, bool* fused, void* stream,
                        const int32_t* proj_ch = nullptr, int32_t* report = nullptr) {
  CF_REQUIRE(a != nullptr, "cf_conv3x3_f16x3: null args");
  CF_REQUIRE(a->n_src == (proj_ch ? 2 : 1) && a->src[0] && a->src_c[0] > 0 && a->src_c[0] % 4 == 0, "cf_conv3x3_f16x3: one fp32 NHWC source");
  const bool s2 = a->stride == 2;
  CF_REQUIRE((a->stride == 1 && a->Ho == a->H && a->Wo == a->W) ||
             (s2 && a->Ho == (a->H - 1) / 2 + 1 && a->Wo == (a->W - 1) / 2 + 1), "cf_conv3x3_f16x3: 3x3, pad 1, stride 1 or 2");
  if (s2 && a->residual) {   // (the stride-2 tile has no residual epilogue: same weights, slot kernel - which validates the block itself)
    if (report) return conv3_report(report, nullptr), CF_OK;
    return cf_conv2d_f16x3(a, stream);
  }
  CF_REQUIRE(a->K_pad > 0 && a->K_pad % 32 == 0, "cf_conv3x3_f16x3: K_pad=%d not a multiple of 32", a->K_pad);
  CF_REQUIRE(a->N > 0 && a->N_pad >= a->N && (a->N_pad == 32 || a->N_pad % 64 == 0), "cf_conv3x3_f16x3: N=%d N_pad=%d", a->N, a->N_pad);
  CF_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cf_conv3x3_f16x3: bad geometry");
  CF_REQUIRE(a->weight && a->bias && a->out, "cf_conv3x3_f16x3: null buffer");
  CF_REQUIRE(a->out_layout == CF_LAYOUT_NHWC && a->out_stride >= a->N && a->out_stride % 4 == 0,
             "cf_conv3x3_f16x3: output must be fp32 NHWC with a stride that is a multiple of 4");
  CF_REQUIRE(a->act == CF_ACT_NONE || a->act == CF_ACT_RELU, "cf_conv3x3_f16x3: act=%d unsupported", a->act);
  CF_REQUIRE(a->out_scale > 0.0f, "cf_conv3x3_f16x3: out_scale must be the 2^-(s+4) the weights were packed with");
  CF_REQUIRE(!a->residual || a->res_stride % 4 == 0, "cf_conv3x3_f16x3: residual stride must be a multiple of 4");
  // K_pad = 16 * 9 * slices, rounded up to a multiple of 32 (+ the projection's channels behind it)
  const int slices = proj_ch ? proj_ch[0] / 16 : a->K_pad / 144;
  if (proj_ch)
    CF_REQUIRE(slices >= 2 && slices % 2 == 0 && a->K_pad == slices * 144 + proj_ch[1],
               "cf_conv3x3_proj_f16x3: K_pad=%d is not a slice-major 3x3 packing of %d channels + %d projected ones", a->K_pad, proj_ch[0], proj_ch[1]);
  else
  CF_REQUIRE(slices >= 1 && (a->K_pad == slices * 144 || a->K_pad == slices * 144 + 16),
             "cf_conv3x3_f16x3: K_pad=%d is not a slice-major 3x3 packing", a->K_pad);
  CF_REQUIRE(slices * 16 <= a->src_c[0], "cf_conv3x3_f16x3: %d input channels exceed the source width %d", slices * 16, a->src_c[0]);
  const long M = (long)a->B * a->Ho * a->Wo;
  CF_REQUIRE((long)a->B * a->H * a->W * a->src_c[0] < (1L << 31) && M < (1L << 31), "cf_conv3x3_f16x3: tensor too large");
  Conv3F k{};
  k.x = a->src[0];
  k.weight = reinterpret_cast<const unsigned char*>(a->weight);
  k.bias = a->bias; k.residual = a->residual; k.out = a->out;
  k.x_stride = a->src_c[0];
  k.H = a->Ho; k.W = a->Wo; k.HW = a->Ho * a->Wo; k.M = (int)M; k.N = a->N;
  k.Hi = a->H; k.Wi = a->W; k.HWi = a->H * a->W;
  k.n_rt = a->N_pad / 32; k.n_ks = a->K_pad / 16;
  k.res_stride = a->res_stride; k.out_stride = a->out_stride; k.act = a->act;
  k.out_scale = a->out_scale;
  k.in_scale = cf_resolve_in_scale(a->in_scale);
  CF_REQUIRE(k.in_scale > 0.0f, "cf_conv3x3_f16x3: in_scale must be 0 (= 16) or a power of two");
  if (proj_ch) {
    k.proj_x = a->src[1];
    k.proj_c = a->src_c[1];
    k.proj_ch = proj_ch[1];
    k.proj_nks = proj_ch[1] / 16;
    k.proj_ks0 = slices * 9;                 // the projection's k-steps sit behind the 3x3 part
  }
  hipStream_t st = (hipStream_t)stream;
  const Conv3Geo geo{a->B, a->H, a->W, a->Ho, a->Wo, a->N_pad, slices};
  Conv3Pick pick;
  if (root && !s2) {
    Conv3F kr = k;
    kr.out = nullptr;                        // x2 stays on the chip
    kr.root_w = reinterpret_cast<const unsigned char*>(root->weight);
    kr.root_bias = root->bias;
    kr.root_out = root->out;
    kr.root_out_stride = root->out_stride;
    kr.root_act = root->act;
    kr.root_scale = root->out_scale;
    kr.root_in_scale = cf_resolve_in_scale(root->in_scale);
    CF_REQUIRE(kr.root_in_scale > 0.0f, "cf_conv3x3_root_f16x3: the Root's in_scale must be 0 (= 16) or a power of two");
    kr.root_nks = root->K_pad / 16;
    for (int i = 0; i < 2; ++i) {
      kr.root_xsrc[i] = i + 2 < root->n_src ? root->src[i + 2] : nullptr;
      kr.root_xsrc_c[i] = i + 2 < root->n_src ? root->src_c[i + 2] : 0;
      kr.root_xsrc_ch[i] = i + 2 < root->n_src ? root_ch[i + 2] : 0;
    }
    if (conv3_pick(V_ROOT, geo, 1, &pick)) {
      *fused = true;
      if (report) return conv3_report(report, &pick), CF_OK;
      return conv3_dispatch(pick, kr, nullptr, 1, st, "cf_conv3x3_root_f16x3");
    }
  }
  const bool found = conv3_pick(s2 ? V_S2 : proj_ch ? V_PROJ : V_PLAIN, geo, 1, &pick);
  if (report) return conv3_report(report, found ? &pick : nullptr), CF_OK;
  if (!found) return cf_conv2d_f16x3(a, stream);
  return conv3_dispatch(pick, k, nullptr, 1, st, "cf_conv3x3_f16x3");
}

extern "C" int cf_conv3x3_f16x3(const cf_conv_args* a, void* stream) { return conv3x3_impl(a, nullptr, nullptr, nullptr, stream); }

// BasicBlock conv2 whose residual is the Tree's `project` (1x1 convolution + BN of the pooled level input, dla.py:96-107):
// src[1] = the pooled tensor, its k-steps packed behind the 3x3 part (packing.pack_conv_f16(proj=...)); one launch, the
// residual tensor never exists.  Geometries no patch tiling fits run the slot kernel on the same table.
static int conv3x3_proj_impl(const cf_conv_args* a, const int32_t* src_channels, void* stream, int32_t* report) {
  CF_REQUIRE(a != nullptr && src_channels != nullptr, "cf_conv3x3_proj_f16x3: null args");
  CF_REQUIRE(a->n_src == 2 && a->src[0] && a->src[1], "cf_conv3x3_proj_f16x3: two sources (3x3 input, projected tensor)");
  CF_REQUIRE(a->stride == 1 && a->N_pad >= 64, "cf_conv3x3_proj_f16x3: stride 1, 64+ output channels");
  CF_REQUIRE(src_channels[0] >= 32 && src_channels[0] % 32 == 0 && src_channels[0] <= a->src_c[0] && a->src_c[0] % 8 == 0,
             "cf_conv3x3_proj_f16x3: %d channels of the 3x3 source (width %d)", src_channels[0], a->src_c[0]);
  CF_REQUIRE(src_channels[1] >= 32 && src_channels[1] % 32 == 0 && src_channels[1] <= a->src_c[1] && a->src_c[1] % 8 == 0,
             "cf_conv3x3_proj_f16x3: %d channels of the projected source (width %d)", src_channels[1], a->src_c[1]);
  CF_REQUIRE((long)a->B * a->H * a->W * a->src_c[1] < (1L << 31), "cf_conv3x3_proj_f16x3: tensor too large");
  CF_REQUIRE(a->slots != nullptr, "cf_conv3x3_proj_f16x3: the slot table is needed (fallback)");
  return conv3x3_impl(a, nullptr, nullptr, nullptr, stream, src_channels, report);
}

extern "C" int cf_conv3x3_proj_f16x3(const cf_conv_args* a, const int32_t* src_channels, void* stream) {
  return conv3x3_proj_impl(a, src_channels, stream, nullptr);
}

// BasicBlock conv2 (+ residual + ReLU) and the Tree's Root over (conv2's output, conv2's residual) as ONE launch where
// a workgroup holds every channel of its pixels (64-channel layers); everything else runs the two launches.  Same
// bits either way (the Root's products and their order are the slot kernel's).
static int conv3x3_root_impl(const cf_conv_args* a, const cf_conv_args* r, const int32_t* root_channels, void* stream, int32_t* report) {
  CF_REQUIRE(a != nullptr && r != nullptr && root_channels != nullptr, "cf_conv3x3_root_f16x3: null args");
  CF_REQUIRE(a->out && a->residual && a->act == CF_ACT_RELU && a->stride == 1,
             "cf_conv3x3_root_f16x3: conv2 needs its output buffer (fallback), a residual and ReLU");
  CF_REQUIRE(r->n_src >= 2 && r->n_src <= CF_MAX_SRC && r->src[0] == a->out && r->src[1] == a->residual &&
                 r->src_c[0] == a->out_stride && r->src_c[1] == a->res_stride,
             "cf_conv3x3_root_f16x3: the Root's first sources must be (conv2's output, conv2's residual)");
  CF_REQUIRE(r->B == a->B && r->H == a->Ho && r->W == a->Wo && r->Ho == r->H && r->Wo == r->W && r->stride == 1,
             "cf_conv3x3_root_f16x3: the Root is a 1x1 convolution on conv2's output map");
  CF_REQUIRE(r->weight && r->bias && r->out && !r->residual && r->out_scale > 0.0f &&
                 (r->act == CF_ACT_NONE || r->act == CF_ACT_RELU) && r->out_layout == CF_LAYOUT_NHWC &&
                 r->out_stride >= r->N && r->out_stride % 4 == 0,
             "cf_conv3x3_root_f16x3: bad Root argument block");
  int k_sum = 0;
  bool pieces_ok = root_channels[0] == a->N && root_channels[1] == a->N;
  for (int i = 0; i < r->n_src; ++i) {
    CF_REQUIRE(r->src[i] && root_channels[i] > 0 && root_channels[i] <= r->src_c[i], "cf_conv3x3_root_f16x3: source %d invalid", i);
    k_sum += root_channels[i];
    if (i >= 2) pieces_ok = pieces_ok && root_channels[i] % 64 == 0 && r->src_c[i] % 4 == 0;
  }
  CF_REQUIRE(k_sum <= r->K_pad, "cf_conv3x3_root_f16x3: the sources' channels (%d) exceed K_pad = %d", k_sum, r->K_pad);
  bool fused = false;
  const bool fusable = (a->N == 64 || a->N == 128 || a->N == 256) && a->N_pad == a->N && r->N == a->N &&
                       r->N_pad == a->N && pieces_ok && r->K_pad == k_sum && a->res_stride % 4 == 0 && r->out_stride % 4 == 0;
  const int rc = conv3x3_impl(a, fusable ? r : nullptr, root_channels, &fused, stream, nullptr, report);
  if (rc != CF_OK || fused || report) return rc;
  return cf_conv2d_f16x3(r, stream);
}

extern "C" int cf_conv3x3_root_f16x3(const cf_conv_args* a, const cf_conv_args* r, const int32_t* root_channels, void* stream) {
  return conv3x3_root_impl(a, r, root_channels, stream, nullptr);
}

// ---- grouped form: the offset convolutions (N_pad = 32) of up to CF_MAX_GROUPS same-shape layers as ONE launch.  Every block is
// validated as cf_conv3x3_f16x3 validates it; the tiling is conv3_pick's V_GRP answer - the N_pad = 32 rule of the ungrouped
// launch on the per-image geometry, its one-round count seeing the whole grid - so group g's rows carry the bits of the
// ungrouped call on block g.  report as in conv3x3_impl; always_grouped (cf_conv3x3_grouped_form): answer for the grouped
// kernel even with one group, which launches as the ungrouped call.
static int conv3x3_grouped_impl(const cf_conv_args* const* gs, int n_groups, void* stream, int32_t* report = nullptr, bool always_grouped = false) {
  CF_REQUIRE(gs != nullptr && n_groups >= 1 && n_groups <= CF_MAX_GROUPS, "cf_conv3x3_f16x3_grouped: n_groups=%d outside 1..%d", n_groups, CF_MAX_GROUPS);
  for (int g = 0; g < n_groups; ++g) CF_REQUIRE(gs[g] != nullptr, "cf_conv3x3_f16x3_grouped: group %d is null", g);
  const cf_conv_args* a = gs[0];
  CF_REQUIRE(a->stride == 1 && a->Ho == a->H && a->Wo == a->W && a->B > 0 && a->H > 0 && a->W > 0, "cf_conv3x3_f16x3_grouped: 3x3, pad 1, stride 1");
  CF_REQUIRE(a->N > 0 && a->N_pad == 32 && a->N <= 32, "cf_conv3x3_f16x3_grouped: the grouped form is built for N_pad = 32 (offset convolutions), got N=%d N_pad=%d", a->N, a->N_pad);
  CF_REQUIRE(a->K_pad > 0 && a->K_pad % 32 == 0, "cf_conv3x3_f16x3_grouped: K_pad=%d not a multiple of 32", a->K_pad);
  const int slices = a->K_pad / 144;
  CF_REQUIRE(slices >= 1 && (a->K_pad == slices * 144 || a->K_pad == slices * 144 + 16), "cf_conv3x3_f16x3_grouped: K_pad=%d is not a slice-major 3x3 packing", a->K_pad);
  CF_REQUIRE(a->out && a->out_layout == CF_LAYOUT_NHWC && a->out_stride >= a->N && a->out_stride % 4 == 0,
             "cf_conv3x3_f16x3_grouped: output must be fp32 NHWC with a stride that is a multiple of 4");
  CF_REQUIRE(a->act == CF_ACT_NONE || a->act == CF_ACT_RELU, "cf_conv3x3_f16x3_grouped: act=%d unsupported", a->act);
  const long M = (long)a->B * a->H * a->W;
  CF_REQUIRE(M * n_groups < (1L << 31), "cf_conv3x3_f16x3_grouped: tensor too large");
  Conv3G grp{};
  for (int g = 0; g < n_groups; ++g) {
    const cf_conv_args* b = gs[g];
    CF_REQUIRE(b->n_src == 1 && b->src[0] && b->weight && b->bias, "cf_conv3x3_f16x3_grouped: group %d: one fp32 NHWC source, weight and bias", g);
    CF_REQUIRE(!b->residual && !b->out2, "cf_conv3x3_f16x3_grouped: group %d: no residual / second output in the grouped form", g);
    CF_REQUIRE(b->src_c[0] == a->src_c[0] && b->src_c[0] % 4 == 0 && slices * 16 <= b->src_c[0] && b->B == a->B && b->H == a->H && b->W == a->W &&
                   b->Ho == a->Ho && b->Wo == a->Wo && b->stride == 1 && b->K_pad == a->K_pad && b->N == a->N && b->N_pad == a->N_pad &&
                   b->out_stride == a->out_stride && b->out_layout == a->out_layout && b->act == a->act,
               "cf_conv3x3_f16x3_grouped: group %d differs from group 0 in geometry", g);
    CF_REQUIRE(b->out == a->out + (size_t)g * M * a->out_stride, "cf_conv3x3_f16x3_grouped: group %d must write rows [g M, (g + 1) M) of group 0's buffer", g);
    CF_REQUIRE((long)M * b->src_c[0] < (1L << 31), "cf_conv3x3_f16x3_grouped: tensor too large");
    CF_REQUIRE(b->out_scale > 0.0f, "cf_conv3x3_f16x3_grouped: out_scale must be the 2^-(s+4) the weights were packed with");
    grp.x[g] = b->src[0];
    grp.weight[g] = reinterpret_cast<const unsigned char*>(b->weight);
    grp.bias[g] = b->bias;
    grp.in_scale[g] = cf_resolve_in_scale(b->in_scale);
    grp.out_scale[g] = b->out_scale;
    CF_REQUIRE(grp.in_scale[g] > 0.0f, "cf_conv3x3_f16x3_grouped: in_scale must be 0 (= 16) or a power of two");
  }
  if (n_groups == 1 && !always_grouped) return conv3x3_impl(a, nullptr, nullptr, nullptr, stream, nullptr, report);   // (one group: the ungrouped launch itself)
  Conv3F k{};
  k.x = a->src[0];
  k.weight = reinterpret_cast<const unsigned char*>(a->weight);
  k.bias = a->bias; k.out = a->out;
  k.x_stride = a->src_c[0];
  k.H = a->H; k.W = a->W; k.HW = a->H * a->W; k.M = (int)M; k.N = a->N;
  k.Hi = a->H; k.Wi = a->W; k.HWi = a->H * a->W;
  k.n_rt = 1; k.n_ks = a->K_pad / 16;
  k.out_stride = a->out_stride; k.act = a->act;
  k.out_scale = a->out_scale;
  k.in_scale = grp.in_scale[0];
  Conv3Pick pick;
  const bool found = conv3_pick(V_GRP, Conv3Geo{a->B, a->H, a->W, a->H, a->W, a->N_pad, slices}, n_groups, &pick);
  CF_REQUIRE(found, "cf_conv3x3_f16x3_grouped: %d x %d map with %d channels fits no patch tiling (run the layers one by one)", a->H, a->W, slices * 16);
  if (report) return conv3_report(report, &pick), CF_OK;
  return conv3_dispatch(pick, k, &grp, n_groups, (hipStream_t)stream, "cf_conv3x3_f16x3_grouped");
}

extern "C" int cf_conv3x3_f16x3_grouped(const cf_conv_args* const* groups, int32_t n_groups, void* stream) {
  return conv3x3_grouped_impl(groups, n_groups, stream);
}

extern "C" int cf_conv3x3_grouped_form(const cf_conv_args* const* groups, int32_t n_groups, int32_t* form) {
  CF_REQUIRE(form != nullptr, "cf_conv3x3_grouped_form: null output");
  int32_t r[CF_CONV3_FORM_INTS];
  const int rc = conv3x3_grouped_impl(groups, n_groups, nullptr, r, true);
  if (rc != CF_OK) return rc;
  const int32_t f[6] = {r[2], r[3], r[4], r[6], r[9], r[10]};   // {WC, WP, WK, NU, T2, CT}
  for (int i = 0; i < 6; ++i) form[i] = f[i];
  return CF_OK;
}

extern "C" int cf_conv3x3_tile_form(int32_t entry, const cf_conv_args* const* blocks, int32_t n_blocks, const int32_t* channels, int32_t* form) {
  CF_REQUIRE(blocks != nullptr && form != nullptr, "cf_conv3x3_tile_form: null args");
  switch (entry) {
    case CF_CONV3_ENTRY_PLAIN:
      CF_REQUIRE(n_blocks == 1, "cf_conv3x3_tile_form: cf_conv3x3_f16x3 takes one block, got %d", n_blocks);
      return conv3x3_impl(blocks[0], nullptr, nullptr, nullptr, nullptr, nullptr, form);
    case CF_CONV3_ENTRY_ROOT:
      CF_REQUIRE(n_blocks == 2, "cf_conv3x3_tile_form: cf_conv3x3_root_f16x3 takes two blocks (conv2, Root), got %d", n_blocks);
      return conv3x3_root_impl(blocks[0], blocks[1], channels, nullptr, form);
    case CF_CONV3_ENTRY_PROJ:
      CF_REQUIRE(n_blocks == 1, "cf_conv3x3_tile_form: cf_conv3x3_proj_f16x3 takes one block, got %d", n_blocks);
      return conv3x3_proj_impl(blocks[0], channels, nullptr, form);
    case CF_CONV3_ENTRY_GROUPED:
      return conv3x3_grouped_impl(blocks, n_blocks, nullptr, form);
    default:
      CF_REQUIRE(false, "cf_conv3x3_tile_form: entry=%d is none of CF_CONV3_ENTRY_*", entry);
  }
}
