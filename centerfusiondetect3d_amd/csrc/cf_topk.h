// Peak top-K: what its kernels (cf_topk.hip) and the frustum kernel, which merges the slice lists in its prologue
// (cf_frustum.hip), share - constants, the 64-bit keys, the steps both slice kernels take, the ordering and merge helpers and
// the host-side launcher of the slice pass.
//
// A key = order-preserving score bits << 32 | ~flat_index: descending keys are ordered by (score desc, flat index asc)
// == (score desc, class asc, pixel asc), and keys are unique over an image.
#pragma once
#include "cf_common.h"

// Checks the top-K geometry and runs the slice pass over `heat` (B,C,H,W): workspace[0 .. B * TOPK_SLICES * K) receives the
// sorted key lists of every slice.  nms: 0 = plain, 1 = 3x3 equality NMS on the fly, 2 = the NMS as a pass of its own into the
// scratch behind the keys (cf_topk_workspace_bytes_nms), then the plain slice pass over it.  `who` names the entry point in
// messages.  Defined in cf_topk.hip: a kernel can only be launched from its own translation unit.
int topk_launch_slices(const char* who, const float* heat, int B, int C, int H, int W, int K, int nms, void* workspace,
                       hipStream_t stream);

namespace {
typedef uint32_t u32x4p __attribute__((ext_vector_type(4)));

constexpr int TOPK_THREADS = 256;   // slice kernel
constexpr int TOPK_MERGE_THREADS = 1024;
constexpr int TOPK_CAP = 4096;      // candidate keys kept in LDS (32 KiB)
constexpr int TOPK_SLICES = 16;     // workgroups per image in the slice pass (32: slice pass 43 -> 26 us, but the merge of
                                    // twice as many lists 12 -> 35 us)
constexpr int TOPK_MAXK = 256;      // K <= number of threads of the slice kernel
constexpr int TOPK_RT = 1024;       // register-cached slice kernel: threads,
constexpr int TOPK_RE = 16;         // elements per thread
constexpr int CK_PARTS = CF_CHECKSUM_PARTS;

// dynamic LDS of a merge (merge_sorted_lists): TOPK_SLICES * K keys + TOPK_SLICES / 2 * K of scratch; 48 KB at K = 256
constexpr size_t topk_merge_lds_bytes(int K) { return (size_t)(TOPK_SLICES + TOPK_SLICES / 2) * K * sizeof(uint64_t); }

__device__ __forceinline__ uint32_t f2u(float f) {  // order-preserving float -> uint (-0 and +0 tie, as they compare)
  uint32_t u = __float_as_uint(f);
  u = (u == 0x80000000u) ? 0u : u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float u2f(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__device__ __forceinline__ uint64_t pack_key(uint32_t u, int i) { return ((uint64_t)u << 32) | (uint32_t)(~(uint32_t)i); }
__device__ __forceinline__ void unpack_key(uint64_t key, int HW, float& score, int& pix, int& cls) {
  const uint32_t idx = ~(uint32_t)key;
  cls = (int)(idx / (uint32_t)HW);
  pix = (int)(idx - (uint32_t)cls * HW);
  score = u2f((uint32_t)(key >> 32));
}

// Descending bitonic sort of P (power of two) 64-bit keys in LDS; whole workgroup participates.
__device__ inline void bitonic_sort_desc(uint64_t* keys, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t a = keys[i], b = keys[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) {
            keys[i] = b;
            keys[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

// keys[0..n) unique, n <= blockDim.x * 4: out[r] = the key of rank r (descending) for r < K.
__device__ __forceinline__ void rank_select_desc(const uint64_t* keys, int n, int K, uint64_t* __restrict__ out) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const uint64_t mine = keys[i];
    int rank = 0;
    int j = 0;
    for (; j + 8 <= n; j += 8) {                                    // eight reads in flight (same address across the wave: LDS broadcast)
      uint64_t o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = keys[j + e];
#pragma unroll
      for (int e = 0; e < 8; ++e) rank += o[e] > mine ? 1 : 0;
    }
    for (; j < n; ++j) rank += keys[j] > mine ? 1 : 0;
    if (rank < K) out[rank] = mine;
  }
}

// ---- steps both slice kernels take (THREADS = the workgroup's size; keys / hist / s_sel / wave_cnt = its LDS)

// A tiny slice, n <= K elements from flat index lo: everything is a candidate.  value(i) = the order-preserving score of
// flat element i.
template <int THREADS, typename Value>
__device__ __forceinline__ void topk_tiny_slice(uint64_t* keys, int lo, int n, int K, uint64_t* __restrict__ out, Value value) {
  const int tid = threadIdx.x;
  for (int i = tid; i < TOPK_MAXK; i += THREADS) keys[i] = i < n ? pack_key(value(lo + i), lo + i) : 0ull;
  __syncthreads();
  bitonic_sort_desc(keys, TOPK_MAXK);
  for (int j = tid; j < K; j += THREADS) out[j] = keys[j];
}

// The exact K-th largest value of the slice by a 4 x 8-bit radix select (the rare path: more than TOPK_CAP elements above
// the bound): fewer than K elements are strictly greater than the result.  visit(f) calls f(u) for every order-preserving
// value u of this thread's share of the slice - from memory or from registers.
template <int THREADS, typename Visit>
__device__ __forceinline__ uint32_t topk_radix_select(uint32_t* hist, uint32_t* s_sel, int K, Visit visit) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0, mask = 0, need = K;
  for (int pass = 3; pass >= 0; --pass) {
    const int shift = pass * 8;
    for (int i = tid; i < 256; i += THREADS) hist[i] = 0;
    __syncthreads();
    visit([&](uint32_t u) {
      if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
    });
    __syncthreads();
    if (tid == 0) {
      uint32_t acc = 0;
      int bin = 255;
      for (; bin > 0; --bin) {
        if (acc + hist[bin] >= need) break;
        acc += hist[bin];
      }
      s_sel[0] = (uint32_t)bin;
      s_sel[1] = need - acc;
    }
    __syncthreads();
    prefix |= s_sel[0] << shift;
    mask |= 255u << shift;
    need = s_sel[1];
    __syncthreads();
  }
  return prefix;
}

// One round of the index-ordered tie selection (threads in index order, `eq` = this thread's element ties with the bound):
// -> the number of tying threads before this one; all = the round's count.  One barrier; the caller places one more before
// the next round reuses wave_cnt.
template <int THREADS>
__device__ __forceinline__ int topk_tie_round(bool eq, uint32_t* wave_cnt, int& all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(eq);
  if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  int wave_off = 0;
  all = 0;
  for (int w = 0; w < THREADS / 64; ++w) {
    const int cw = (int)wave_cnt[w];
    if (w < wave) wave_off += cw;
    all += cw;
  }
  return wave_off + __popcll(bal & ((1ull << lane) - 1ull));
}

// Merge of the TOPK_SLICES sorted key lists of one image (keys[] in LDS, list o at keys + o * K; descending, keys unique
// over the image - zero padding of tiny slices excepted, which ties only with itself) as a TREE of pairwise merges that each
// keep the top K: 16 -> 8 -> 4 -> 2 -> 1 lists, ping-pong between keys[0 .. 16 K) and tmp[0 .. 8 K).  An element's rank in
// the merge of its pair = its position + the number of the partner's keys above it (one 7-step binary search): 3,000
// searches over the four levels instead of the 24,000 of ranking every key against all 15 other lists at once (11.5 us as
// its own launch).  -> pointer to the K merged keys (in keys[] or tmp[]).  Whole workgroup; ends with a barrier.
__device__ __forceinline__ const uint64_t* merge_sorted_lists(uint64_t* keys, uint64_t* tmp, int K) {
  uint64_t* src = keys;
  uint64_t* dst = tmp;
  for (int lists = TOPK_SLICES; lists > 1; lists >>= 1) {
    const int total = lists * K;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int sl = i / K, pos = i - sl * K;
      const uint64_t mine = src[i];
      const uint64_t* lst = src + (sl ^ 1) * K;          // the partner list
      int lo = 0, hi = K;                                // first position whose key is NOT above mine
      // (equal keys exist only as zero padding; the odd list of a pair counts them as above, so a tie takes two ranks)
      const bool ge = (sl & 1) != 0;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint64_t o = lst[mid];
        if (o > mine || (ge && o == mine)) lo = mid + 1; else hi = mid;
      }
      const int rank = pos + lo;
      if (rank < K) dst[(sl >> 1) * K + rank] = mine;
    }
    __syncthreads();
    uint64_t* t = src; src = dst; dst = t;
  }
  return src;
}
}  // namespace
