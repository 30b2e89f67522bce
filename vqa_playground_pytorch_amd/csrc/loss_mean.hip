// The reference driver's other two criteria, forward and gradient in one pass over the logits, each with an optional
// count of the target's top-k hits from the same pass (as kld_hits_rows_kernel, metrics.hip, does for the KLD sum):
//
//   BCE (train.py:522-534): nn.BCELoss()(nn.Sigmoid()(z), a), a mean over all B*C elements of soft targets a in [0,1]:
//     loss    = scale * sum_{b,c} a * min(softplus(-z), 100) + (1 - a) * min(softplus(z), 100)
//     dL/dz   = scale * (sigmoid(z) - a)
//     softplus(z) = max(z, 0) + log1p(exp(-|z|)) = -log(1 - sigmoid(z)) and softplus(-z) = softplus(z) - z = -log(sigmoid(z))
//     without ever forming 1 - sigmoid(z) (which cancels in fp32 from |z| ~ 9 on); the two min() are BCELoss's clamp of
//     its log terms at -100.  Finite for every finite z.
//   CE (train.py:519-520): nn.CrossEntropyLoss()(z, label), a mean over the B rows of sampled answer indices:
//     loss    = scale * sum_b (logsumexp(z_b) - z_b[label_b])
//     dL/dz   = scale * (softmax(z) - onehot(label))
//     a label outside [0, C) is the caller's error (ops.py rejects it); the kernel clamps the index and stays in bounds.
//
// `scale` is a launch argument: 1 / (B_global * C) for BCE and 1 / B_global for CE, so that the SUM all-reduce of the
// data-parallel step adds up to the reference's mean over the global batch (trainer.py).
//
// Same shape as loss.hip / metrics.hip: one workgroup per row (C <= 4096 values in registers, wave64 DPP reductions,
// unconditional loads from a clamped column), the B row losses -- and, with hits, the B ranks -- combined by ONE workgroup
// in a fixed order: no atomics, no memset.  The target column is argmax(a) (first index of the largest value) for BCE and
// the label itself for CE (train.py:30-32); "beats" is metrics.hip's order (NaN above every number, ties to the lower
// column).  The hits instances run the same loss / gradient arithmetic in the same order: bitwise the same loss and d_logits.
// HBM-bound: BCE reads z and a and writes dz (3 * B * C * 4 bytes), CE reads z and writes dz (2 * B * C * 4 bytes).
#include <climits>

#include "common.hpp"

namespace vqa {
namespace meanloss {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;  // C <= 4096
constexpr int kMaxK = 16;
enum { kBce = 0, kCe = 1 };

// a beats b (the order documented at the top of metrics.hip)
__device__ __forceinline__ bool beats(float va, int ia, float vb, int ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}

// best (value, column) pair of the wave under `beats`, wave-uniform (the DPP steps of wave_sum, then four readlanes)
__device__ __forceinline__ void wave_best(float& v, int& i) {
#define VQA_BEST_STEP(CTRL)                                   \
  {                                                           \
    const float ov = dpp_mov<CTRL>(v);                        \
    const int oi = dpp_mov_i<CTRL>(i);                        \
    if (beats(ov, oi, v, i)) { v = ov; i = oi; }              \
  }
  VQA_BEST_STEP(0xB1)
  VQA_BEST_STEP(0x4E)
  VQA_BEST_STEP(0x141)
  VQA_BEST_STEP(0x140)
#undef VQA_BEST_STEP
  const int vi = __float_as_int(v);
  float bv = __int_as_float(__builtin_amdgcn_readlane(vi, 0));
  int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
  for (int r = 16; r < 64; r += 16) {
    const float ov = __int_as_float(__builtin_amdgcn_readlane(vi, r));
    const int oi = __builtin_amdgcn_readlane(i, r);
    if (beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  v = bv;
  i = bi;
}

__device__ __forceinline__ int wave_sum_i(int x) {
  x += dpp_mov_i<0xB1>(x);
  x += dpp_mov_i<0x4E>(x);
  x += dpp_mov_i<0x141>(x);
  x += dpp_mov_i<0x140>(x);
  return __builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
         __builtin_amdgcn_readlane(x, 48);
}

__device__ __forceinline__ int block_sum_i(int x, int* red_s) {
  x = wave_sum_i(x);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red_s[wave] = x;
  __syncthreads();
  return red_s[0] + red_s[1] + red_s[2] + red_s[3];
}
__device__ __forceinline__ float block_sum(float x, float* red_s) {
  x = wave_sum(x);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red_s[wave] = x;
  __syncthreads();
  return red_s[0] + red_s[1] + red_s[2] + red_s[3];
}
__device__ __forceinline__ float block_max(float x, float* red_s) {
  x = wave_max(x);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red_s[wave] = x;
  __syncthreads();
  return fmaxf(fmaxf(red_s[0], red_s[1]), fmaxf(red_s[2], red_s[3]));
}

// One row.  LOSS = kBce: `target` is the row-major [B,C] soft target; kCe: `labels` is int64 [B].  HITS: also the rank of the
// target column among the logits (row_rank[b] = #{c < C : z_c beats z_t}).
template <int LOSS, bool HITS>
__global__ __launch_bounds__(kThreads) void mean_rows_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                             const int64_t* __restrict__ labels, float* __restrict__ row_loss,
                                                             int* __restrict__ row_rank, float* __restrict__ d_logits,
                                                             float scale, int C) {
  __shared__ float red_s[4];
  __shared__ float bv_s[4], zt_s;
  __shared__ int bi_s[4], ired_s[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (size_t)b * C;
  float zv[kPerThread], av[kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = tid + i * kThreads;
    const int cc = min(c, C - 1);  // unconditional loads from a clamped column
    const float zt = z[cc];
    zv[i] = c < C ? zt : -INFINITY;
    if (LOSS == kBce) {
      const float at = target[(size_t)b * C + cc];
      av[i] = c < C ? at : 0.f;
    }
  }
  // the target column
  int t = 0;
  if (LOSS == kCe) {
    const int64_t l = labels[b];
    t = (int)(l < 0 ? 0 : (l > C - 1 ? C - 1 : l));
  } else if (HITS) {
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int c = tid + i * kThreads;
      if (c < C && beats(av[i], c, bv, bi)) { bv = av[i]; bi = c; }
    }
    wave_best(bv, bi);
    if ((tid & 63) == 0) {
      bv_s[tid >> 6] = bv;
      bi_s[tid >> 6] = bi;
    }
    __syncthreads();
    bv = bv_s[0];
    bi = bi_s[0];
#pragma unroll
    for (int w = 1; w < kThreads / kWave; ++w)
      if (beats(bv_s[w], bi_s[w], bv, bi)) { bv = bv_s[w]; bi = bi_s[w]; }
    t = bi;  // C >= 1: always a real column
  }
  float zt = 0.f;
  if (LOSS == kCe || HITS) {
#pragma unroll
    for (int i = 0; i < kPerThread; ++i)
      if (tid + i * kThreads == t) zt_s = zv[i];
    __syncthreads();
    zt = zt_s;
  }
  if (HITS) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int c = tid + i * kThreads;
      n += (c < C && beats(zv[i], c, zt, t)) ? 1 : 0;
    }
    n = block_sum_i(n, ired_s);
    if (tid == 0) row_rank[b] = n;
  }
  if (LOSS == kBce) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int c = tid + i * kThreads;
      const float x = zv[i], a = av[i];
      const float e = expf(-fabsf(x));                  // in (0, 1]; 0 for the padded columns
      const float l1p = log1pf(e);
      const float sp = fmaxf(x, 0.f) + l1p;             // softplus(z)  = -log(1 - sigmoid(z))
      const float sn = fmaxf(-x, 0.f) + l1p;            // softplus(-z) = -log(sigmoid(z))
      const float term = a * fminf(sn, 100.f) + (1.f - a) * fminf(sp, 100.f);
      s += c < C ? term : 0.f;
      const float r = 1.f / (1.f + e);
      zv[i] = ((x >= 0.f ? r : e * r) - a) * scale;     // (sigmoid(z) - a) * scale
    }
    s = block_sum(s, red_s);
    if (tid == 0) row_loss[b] = s * scale;
  } else {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) m = fmaxf(m, zv[i]);
    m = block_max(m, red_s);
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const float e = expf(zv[i] - m);  // exp(-inf) = 0 for the padded columns
      se += e;
      zv[i] = e;
    }
    se = block_sum(se, red_s);
    // logsumexp(z) - z_t = log se - (z_t - m)
    if (tid == 0) row_loss[b] = (logf(se) - (zt - m)) * scale;
    const float k = scale / se;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) zv[i] = tid + i * kThreads == t ? fmaf(zv[i], k, -scale) : zv[i] * k;
  }
  if (d_logits != nullptr) {
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int c = tid + i * kThreads;
      if (c < C) d_logits[(size_t)b * C + c] = zv[i];
    }
  }
}

// one workgroup: loss[0] = the row losses added in kld_total_kernel's order and, given ranks, hits[j] = #{b : row_rank[b] <= j}
// for j < kmax.  The hits and no-hits entry points both total their rows here: the same sum either way.
__global__ __launch_bounds__(kThreads) void mean_total_kernel(const float* __restrict__ row_loss, float* __restrict__ loss,
                                                              const int* __restrict__ row_rank, int* __restrict__ hits, int kmax,
                                                              int B) {
  __shared__ float red_s[4];
  __shared__ int ired_s[4];
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += kThreads) s += row_loss[b];
  s = block_sum(s, red_s);
  if (threadIdx.x == 0) loss[0] = s;
  if (row_rank == nullptr) return;  // uniform: every thread leaves
  int n[kMaxK];
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) n[j] = 0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const int r = row_rank[b];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) n[j] += r <= j ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) {
    if (j < kmax) {  // kmax is uniform: the barriers inside are reached by every thread or none
      const int c = block_sum_i(n[j], ired_s);
      if (threadIdx.x == 0) hits[j] = c;
    }
  }
}

static int check_sizes(const char* what, int B, int C, float scale) {
  VQA_REQUIRE(B > 0 && C > 0, VQA_E_BADARG, "%s: bad sizes B=%d C=%d", what, B, C);
  VQA_REQUIRE(scale == scale && scale > 0.f && scale <= 3.0e38f, VQA_E_BADARG, "%s: scale must be positive and finite", what);
  VQA_REQUIRE(C <= kThreads * kPerThread, VQA_E_UNSUPPORTED, "%s: C=%d exceeds %d", what, C, kThreads * kPerThread);
  return VQA_OK;
}

template <int LOSS>
static int launch(const char* what, const float* logits, const float* target, const int64_t* labels, float* loss, float* d_logits,
                  int* hits, int kmax, bool want_hits, float scale, void* workspace, size_t workspace_bytes, int B, int C,
                  vqa_stream_t stream) {
  VQA_REQUIRE(logits && (LOSS == kBce ? (const void*)target : (const void*)labels) && loss && workspace && (hits || !want_hits),
              VQA_E_BADARG, "%s: null pointer", what);
  const int rc = check_sizes(what, B, C, scale);
  if (rc != VQA_OK) return rc;
  if (want_hits)
    VQA_REQUIRE(kmax >= 1 && kmax <= kMaxK && kmax <= C, VQA_E_BADARG, "%s: k=%d outside [1, min(%d, C=%d)]", what, kmax, kMaxK, C);
  const size_t need = (size_t)B * (want_hits ? sizeof(float) + sizeof(int) : sizeof(float));
  VQA_REQUIRE(workspace_bytes >= need, VQA_E_BADARG, "%s: workspace of %zu B is too small", what, workspace_bytes);
  VQA_REQUIRE(aligned(workspace, 4) && (LOSS == kBce || aligned(labels, 8)), VQA_E_UNSUPPORTED, "%s: misaligned labels or workspace",
              what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* row_loss = static_cast<float*>(workspace);
  int* row_rank = want_hits ? reinterpret_cast<int*>(row_loss + B) : nullptr;
  if (want_hits)
    VQA_LAUNCH((mean_rows_kernel<LOSS, true>), dim3(B), dim3(kThreads), 0, s, logits, target, labels, row_loss, row_rank, d_logits,
               scale, C);
  else
    VQA_LAUNCH((mean_rows_kernel<LOSS, false>), dim3(B), dim3(kThreads), 0, s, logits, target, labels, row_loss, row_rank, d_logits,
               scale, C);
  VQA_LAUNCH(mean_total_kernel, dim3(1), dim3(kThreads), 0, s, row_loss, loss, (const int*)row_rank, hits, kmax, B);
  return check_launch(what);
}

}  // namespace meanloss
}  // namespace vqa

using namespace vqa;
using namespace vqa::meanloss;

extern "C" size_t vqa_mean_loss_workspace_bytes(int B) { return B > 0 ? (size_t)B * sizeof(float) : 0; }
extern "C" size_t vqa_mean_loss_hits_workspace_bytes(int B, int kmax) {
  (void)kmax;
  return B > 0 ? (size_t)B * (sizeof(float) + sizeof(int)) : 0;
}

extern "C" int vqa_bce_mean_loss(const float* logits, const float* target, float* loss, float* d_logits, float scale,
                                 void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  return launch<kBce>("bce_mean_loss", logits, target, nullptr, loss, d_logits, nullptr, 0, false, scale, workspace,
                      workspace_bytes, B, C, stream);
}

extern "C" int vqa_bce_mean_loss_hits(const float* logits, const float* target, float* loss, float* d_logits, int* hits,
                                      int kmax, float scale, void* workspace, size_t workspace_bytes, int B, int C,
                                      vqa_stream_t stream) {
  return launch<kBce>("bce_mean_loss_hits", logits, target, nullptr, loss, d_logits, hits, kmax, true, scale, workspace,
                      workspace_bytes, B, C, stream);
}

extern "C" int vqa_ce_mean_loss(const float* logits, const int64_t* labels, float* loss, float* d_logits, float scale,
                                void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  return launch<kCe>("ce_mean_loss", logits, nullptr, labels, loss, d_logits, nullptr, 0, false, scale, workspace, workspace_bytes,
                     B, C, stream);
}

extern "C" int vqa_ce_mean_loss_hits(const float* logits, const int64_t* labels, float* loss, float* d_logits, int* hits, int kmax,
                                     float scale, void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  return launch<kCe>("ce_mean_loss_hits", logits, nullptr, labels, loss, d_logits, hits, kmax, true, scale, workspace,
                     workspace_bytes, B, C, stream);
}
