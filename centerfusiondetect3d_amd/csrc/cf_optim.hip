// Multi-tensor optimizer update (cf_optim_adamw, cf_optim_sgd): ONE launch walks every parameter of a group.
// A streaming kernel: grid = number of chunks, a workgroup of 256 threads owns one chunk (<= CF_OPTIM_CHUNK elements) of one
// tensor, 16 B per lane and access when the tensor's pointers allow it, no LDS, no scratch, nothing shared between workgroups.
// Built with -ffp-contract=off: the compiler fuses nothing on its own, so the fp32 roundings are the ones written below - those
// of torch's single-tensor CPU implementations the tests compare against (the kernel is bandwidth-bound: 28 B per parameter
// for AdamW, 20 B for SGD with momentum).
#include "cf_common.h"

namespace {

constexpr int kThreads = 256;
static_assert(CF_OPTIM_CHUNK % 4 == 0 && CF_OPTIM_CHUNK % (4 * kThreads) == 0, "a chunk is whole float4 rounds of the workgroup");
constexpr int kRounds = CF_OPTIM_CHUNK / (4 * kThreads);

// what one launch needs beyond the tables, already in the form the element update uses
struct Scalars {
  float decay, w1, b2, w2, eps;   // AdamW
  float wd, mu, lr;               // SGD
  double lr_d, beta1_d, beta2_d;  // AdamW bias corrections (per tensor: they depend on its own step)
  int step;
};

__device__ __forceinline__ double ipow(double b, int e) {   // b^e, e >= 1, by squaring (<= 31 rounds, once per thread)
  double r = 1.0;
  while (e) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

// The roundings are those of torch's CPU kernels (lerp_, addcmul_, addcdiv_, add_ with alpha), which fuse exactly the
// multiply-adds written as fmaf here and nothing else.
struct AdamStep {
  float decay, w1, b2, w2, eps, neg_step_size, bc2_sqrt;
  __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
    p = p * decay;
    m = fmaf(g - m, w1, m);
    v = fmaf(w2 * g, g, v * b2);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p + (neg_step_size * m) / denom;
  }
};

struct SgdStep {
  float wd, mu, neg_lr;
  bool first, has_buf;
  __device__ __forceinline__ void operator()(float& p, float g, float& buf, float&) const {
    const float gp = fmaf(wd, p, g);
    float b = gp;
    if (has_buf) {
      if (!first) b = mu * buf + gp;
      buf = b;
    }
    p = fmaf(neg_lr, b, p);
  }
};

template <typename Step, bool S1, bool S2>
__device__ __forceinline__ void update_chunk(const Step& st, float* __restrict__ p, const float* __restrict__ g,
                                             float* __restrict__ s1, float* __restrict__ s2, int n, bool vec) {
  // p, g, s1, s2 point at the chunk; n <= CF_OPTIM_CHUNK elements of it exist
  const int tid = threadIdx.x;
  int done = 0;
  if (vec) {
    const int nvec = n >> 2;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int i = r * kThreads + tid;
      if (i < nvec) {
        f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
        if (S1) av = reinterpret_cast<const f32x4*>(s1)[i];
        if (S2) bv = reinterpret_cast<const f32x4*>(s2)[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // (compile-time component index: registers, no scratch)
          float pe = pv[c], a = av[c], b = bv[c];
          st(pe, gv[c], a, b);
          pv[c] = pe;
          av[c] = a;
          bv[c] = b;
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        if (S1) reinterpret_cast<f32x4*>(s1)[i] = av;
        if (S2) reinterpret_cast<f32x4*>(s2)[i] = bv;
      }
    }
    done = nvec << 2;   // the last n % 4 elements follow one by one
  }
  for (int i = done + tid; i < n; i += kThreads) {
    float pe = p[i], a = 0.f, b = 0.f;
    const float ge = g[i];
    if (S1) a = s1[i];
    if (S2) b = s2[i];
    st(pe, ge, a, b);
    p[i] = pe;
    if (S1) s1[i] = a;
    if (S2) s2[i] = b;
  }
}

template <bool ADAM>
__global__ __launch_bounds__(kThreads) void optim_kernel(const cf_optim_tensor* __restrict__ tensors,
                                                         const cf_optim_chunk* __restrict__ chunks, int n_tensors, Scalars sc) {
  const cf_optim_chunk ck = chunks[blockIdx.x];
  if (ck.tensor < 0 || ck.tensor >= n_tensors) return;
  const cf_optim_tensor t = tensors[ck.tensor];
  if (ck.offset < 0 || ck.offset >= t.numel) return;
  const int64_t left = t.numel - ck.offset;
  const int n = left < (int64_t)CF_OPTIM_CHUNK ? (int)left : CF_OPTIM_CHUNK;
  const int step = sc.step - t.step_base;   // this tensor's own count (>= 1)
  const uintptr_t bits = (uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.state1 | (uintptr_t)t.state2;
  const bool vec = (bits & 15) == 0;        // (a NULL state pointer counts as aligned; chunk offsets are multiples of 4 elements)
  float* p = t.param + ck.offset;
  const float* g = t.grad + ck.offset;
  if (ADAM) {
    const int s = step < 1 ? 1 : step;
    const double bc1 = 1.0 - ipow(sc.beta1_d, s), bc2 = 1.0 - ipow(sc.beta2_d, s);
    const AdamStep st = {sc.decay, sc.w1, sc.b2, sc.w2, sc.eps, -(float)(sc.lr_d / bc1), (float)sqrt(bc2)};
    update_chunk<AdamStep, true, true>(st, p, g, t.state1 + ck.offset, t.state2 + ck.offset, n, vec);
  } else {
    const SgdStep st = {sc.wd, sc.mu, -sc.lr, step <= 1, t.state1 != nullptr};
    if (t.state1)
      update_chunk<SgdStep, true, false>(st, p, g, t.state1 + ck.offset, nullptr, n, vec);
    else
      update_chunk<SgdStep, false, false>(st, p, g, nullptr, nullptr, n, vec);
  }
}

int check_args(const char* what, const cf_optim_args* a) {
  CF_REQUIRE(a != nullptr, "%s: null args (a)", what);
  CF_REQUIRE(a->tensors != nullptr && a->chunks != nullptr, "%s: null table (tensors, chunks)", what);
  CF_REQUIRE(a->n_tensors > 0 && a->n_chunks > 0, "%s: n_tensors=%d, n_chunks=%d must be positive", what, a->n_tensors, a->n_chunks);
  CF_REQUIRE(a->step > 0, "%s: step=%d must count this launch (>= 1)", what, a->step);
  return CF_OK;
}

template <bool ADAM>
int launch(const char* what, const cf_optim_args* a, void* stream) {
  const int rc = check_args(what, a);
  if (rc != CF_OK) return rc;
  Scalars sc;
  sc.decay = a->decay;
  sc.w1 = (float)(1.0 - a->beta1);
  sc.b2 = (float)a->beta2;
  sc.w2 = (float)(1.0 - a->beta2);
  sc.eps = (float)a->eps;
  sc.wd = (float)a->wd;
  sc.mu = (float)a->momentum;
  sc.lr = (float)a->lr;
  sc.lr_d = a->lr;
  sc.beta1_d = a->beta1;
  sc.beta2_d = a->beta2;
  sc.step = a->step;
  hipLaunchKernelGGL(optim_kernel<ADAM>, dim3((unsigned)a->n_chunks), dim3(kThreads), 0, (hipStream_t)stream, a->tensors, a->chunks,
                     a->n_tensors, sc);
  return cf_check_launch(what);
}

}  // namespace

extern "C" int cf_optim_plan(const cf_optim_tensor* tensors, int n, cf_optim_chunk* chunks, int64_t capacity, int64_t* n_chunks) {
  CF_REQUIRE(tensors != nullptr && n_chunks != nullptr, "cf_optim_plan: null table (tensors) or n_chunks");
  CF_REQUIRE(n > 0, "cf_optim_plan: n=%d must be positive", n);
  int64_t count = 0;
  for (int i = 0; i < n; ++i) {
    CF_REQUIRE(tensors[i].numel >= 0, "cf_optim_plan: tensor %d has numel=%lld", i, (long long)tensors[i].numel);
    count += (tensors[i].numel + CF_OPTIM_CHUNK - 1) / CF_OPTIM_CHUNK;
  }
  CF_REQUIRE(count <= 0x7fffffff, "cf_optim_plan: %lld chunks exceed one launch's grid", (long long)count);
  *n_chunks = count;
  if (chunks == nullptr) return CF_OK;
  CF_REQUIRE(capacity >= count, "cf_optim_plan: capacity=%lld below the %lld chunks needed", (long long)capacity, (long long)count);
  int64_t k = 0;
  for (int i = 0; i < n; ++i)
    for (int64_t off = 0; off < tensors[i].numel; off += CF_OPTIM_CHUNK) {
      chunks[k].offset = off;
      chunks[k].tensor = i;
      chunks[k].reserved = 0;
      ++k;
    }
  return CF_OK;
}

extern "C" int cf_optim_adamw(const cf_optim_args* a, void* stream) { return launch<true>("cf_optim_adamw", a, stream); }

extern "C" int cf_optim_sgd(const cf_optim_args* a, void* stream) { return launch<false>("cf_optim_sgd", a, stream); }

extern "C" int cf_optim_chunk_elems(void) { return CF_OPTIM_CHUNK; }
