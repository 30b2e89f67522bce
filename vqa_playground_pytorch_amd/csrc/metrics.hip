// What the reference's loops REPORT from the logits: top-k hits of the train step, and the predictions of test() / visu.py.
//
//   accuracy(output, a, topk=(1, 5)) (train.py:22-38, called at :70-72): target class = torch.max(a, 1) (the FIRST index of
//     the row's largest target value), a top-k hit when the target is among output.topk(k) -- counted here without a sort:
//     the target's rank r = #{c : z_c > z_t} (order below) is a top-k hit iff r < k;
//   test() (train.py:110-191): OpenEnded = output.max(1), MultipleChoice = the best-scoring column among the a_mc_idx candidates;
//   visu.py:188-194: the top-5 columns and their softmax probabilities over the whole row.
//
// ONE order everywhere ("a beats b"): NaN ranks above every number (torch's topk / sort / max treat NaN as largest), otherwise
// the larger value, ties to the lower column index.  It is a total order on (value, column) pairs, so the j-th pick of a top-k
// is the best element beaten by the (j-1)-th pick: k block-wide arg-max rounds over a row held in registers, no sort, no state.
//
// All kernels are HBM-bound row kernels: one workgroup per row (C <= 4096 values in registers, as kld_rows_kernel), wave64
// DPP reductions of (value, column) pairs.  Per-row ranks go to a workspace; one workgroup turns them into hit counts in a
// fixed order -- no atomics, no memset (a memset node replays wrongly inside a hipGraph on this ROCm: see api.hip).
#include <climits>

#include "common.hpp"

namespace vqa {
namespace metrics {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;  // C <= 4096
constexpr int kMaxK = 16;
constexpr int kMaxCand = 256;

// a beats b (see the top of the file)
__device__ __forceinline__ bool beats(float va, int ia, float vb, int ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}

// best (value, column) pair of the wave under `beats`, wave-uniform: the four DPP steps of wave_sum (quad_perm x2,
// row_half_mirror, row_mirror) leave every lane with the best of its 16-lane row; four readlanes combine the rows
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

// block-wide best pair; bv_s / bi_s [4] are this round's LDS slots (callers alternate two sets, so one barrier per round)
__device__ __forceinline__ void block_best(float& v, int& i, float* bv_s, int* bi_s) {
  wave_best(v, i);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    bv_s[wave] = v;
    bi_s[wave] = i;
  }
  __syncthreads();
  v = bv_s[0];
  i = bi_s[0];
#pragma unroll
  for (int w = 1; w < kThreads / kWave; ++w)
    if (beats(bv_s[w], bi_s[w], v, i)) { v = bv_s[w]; i = bi_s[w]; }
}

__device__ __forceinline__ int block_sum_i(int x, int* red_s) {
  x = wave_sum_i(x);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red_s[wave] = x;
  __syncthreads();
  return red_s[0] + red_s[1] + red_s[2] + red_s[3];
}

// the same two reductions as loss.hip's (the KLD arithmetic below must stay bitwise equal to kld_rows_kernel's)
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

// Rank of the row's target column: t = first index of the largest target value, rank = #{c < C : z_c beats z_t}.
// zv / tv hold the row (column tid + i * kThreads); columns >= C are excluded by index.
__device__ __forceinline__ int target_rank(const float (&zv)[kPerThread], const float (&tv)[kPerThread], int C, float* bv_s,
                                           int* bi_s, float* zt_s, int* red_s) {
  const int tid = threadIdx.x;
  float bv = -INFINITY;
  int bi = INT_MAX;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = tid + i * kThreads;
    if (c < C && beats(tv[i], c, bv, bi)) { bv = tv[i]; bi = c; }
  }
  block_best(bv, bi, bv_s, bi_s);
  const int t = bi;  // C >= 1: always a real column
#pragma unroll
  for (int i = 0; i < kPerThread; ++i)
    if (tid + i * kThreads == t) *zt_s = zv[i];
  __syncthreads();
  const float zt = *zt_s;
  int n = 0;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = tid + i * kThreads;
    n += (c < C && beats(zv[i], c, zt, t)) ? 1 : 0;
  }
  return block_sum_i(n, red_s);
}

// kld_rows_kernel (loss.hip) + the target's rank: the same loads, the same loss / gradient arithmetic in the same order
__global__ __launch_bounds__(kThreads) void kld_hits_rows_kernel(const float* __restrict__ logits,
                                                                 const float* __restrict__ target,
                                                                 float* __restrict__ row_loss, int* __restrict__ row_rank,
                                                                 float* __restrict__ d_logits, int C) {
  __shared__ float red_s[4];
  __shared__ float bv_s[4], zt_s;
  __shared__ int bi_s[4], ired_s[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (size_t)b * C;
  const float* a = target + (size_t)b * C;
  float zv[kPerThread], av[kPerThread];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = tid + i * kThreads;
    const int cc = min(c, C - 1);  // unconditional loads from a clamped column
    const float zt = z[cc], at = a[cc];
    zv[i] = c < C ? zt : -INFINITY;
    av[i] = c < C ? at : 0.f;
    m = fmaxf(m, zv[i]);
  }
  const int rank = target_rank(zv, av, C, bv_s, bi_s, &zt_s, ired_s);
  if (tid == 0) row_rank[b] = rank;
  m = block_max(m, red_s);
  float se = 0.f, sa = 0.f, saz = 0.f, sal = 0.f;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const float e = expf(zv[i] - m);  // exp(-inf) = 0 for the padded columns
    se += e;
    sa += av[i];
    if (av[i] > 0.f) {
      saz = fmaf(av[i], zv[i] - m, saz);
      sal = fmaf(av[i], logf(av[i]), sal);
    }
    zv[i] = e;
  }
  se = block_sum(se, red_s);
  sa = block_sum(sa, red_s);
  saz = block_sum(saz, red_s);
  sal = block_sum(sal, red_s);
  // sum_c a (log a - (z - m - log se)) = sal - saz + sa * log se
  if (tid == 0) row_loss[b] = sal - saz + sa * logf(se);
  if (d_logits != nullptr) {
    const float k = sa / se;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int c = tid + i * kThreads;
      if (c < C) d_logits[(size_t)b * C + c] = fmaf(zv[i], k, -av[i]);
    }
  }
}

// one workgroup: hits[j] = #{b : row_rank[b] <= j} for j < kmax, and (row_loss != nullptr) loss[0] = the row losses added in
// kld_total_kernel's order (bitwise the same total)
__global__ __launch_bounds__(kThreads) void hits_total_kernel(const int* __restrict__ row_rank, int* __restrict__ hits, int kmax,
                                                              const float* __restrict__ row_loss, float* __restrict__ loss,
                                                              int B) {
  __shared__ float red_s[4];
  __shared__ int ired_s[4];
  if (row_loss != nullptr) {
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += kThreads) s += row_loss[b];
    s = block_sum(s, red_s);
    if (threadIdx.x == 0) loss[0] = s;
  }
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
      const int s = block_sum_i(n[j], ired_s);
      if (threadIdx.x == 0) hits[j] = s;
    }
  }
}

// one row: the k best columns in order (top_idx int64), their softmax probability over the whole row (top_prob, optional),
// and the target's rank (row_rank, when a target is given)
__global__ __launch_bounds__(kThreads) void topk_rows_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                             int64_t* __restrict__ top_idx, float* __restrict__ top_prob,
                                                             int* __restrict__ row_rank, int k, int C) {
  __shared__ float red_s[4];
  __shared__ float bv_s[2][4], zt_s;
  __shared__ int bi_s[2][4], ired_s[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (size_t)b * C;
  float zv[kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = tid + i * kThreads;
    const float x = z[min(c, C - 1)];  // unconditional loads from a clamped column
    zv[i] = c < C ? x : -INFINITY;
  }
  if (target != nullptr) {
    const float* a = target + (size_t)b * C;
    float tv[kPerThread];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) tv[i] = a[min(tid + i * kThreads, C - 1)];
    const int rank = target_rank(zv, tv, C, bv_s[1], bi_s[1], &zt_s, ired_s);
    if (tid == 0) row_rank[b] = rank;
  }
  float m = 0.f, se = 1.f;
  if (top_prob != nullptr) {
    m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) m = fmaxf(m, zv[i]);  // fmaxf skips NaN; a NaN in the row makes se NaN (as torch)
    m = block_max(m, red_s);
    se = 0.f;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) se += expf(zv[i] - m);
    se = block_sum(se, red_s);
  }
  // round j: the best pair beaten by pick j-1 -- (NaN, -1) beats every pair, so round 0 takes the row's best
  float pv = __int_as_float(0x7FC00000);
  int pi = -1;
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int c = tid + i * kThreads;
      if (c < C && beats(pv, pi, zv[i], c) && beats(zv[i], c, bv, bi)) { bv = zv[i]; bi = c; }
    }
    block_best(bv, bi, bv_s[j & 1], bi_s[j & 1]);
    if (tid == 0) {
      top_idx[(size_t)b * k + j] = bi;
      if (top_prob != nullptr) top_prob[(size_t)b * k + j] = expf(bv - m) / se;
    }
    pv = bv;
    pi = bi;
  }
}

// one wave per row: the candidate column (0 <= cand < C) with the best logit, -1 when the row has none
__global__ __launch_bounds__(kThreads) void candidates_kernel(const float* __restrict__ logits, const int64_t* __restrict__ cand,
                                                              int64_t* __restrict__ pred, int B, int C, int M) {
  const int b = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;  // whole waves leave: no barrier below
  float bv = -INFINITY;
  int bi = INT_MAX;
  for (int j = lane; j < M; j += kWave) {
    const int64_t c = cand[(size_t)b * M + j];
    if (c >= 0 && c < C) {
      const float v = logits[(size_t)b * C + c];
      if (beats(v, (int)c, bv, bi)) { bv = v; bi = (int)c; }
    }
  }
  wave_best(bv, bi);
  if (lane == 0) pred[b] = bi == INT_MAX ? -1 : bi;
}

}  // namespace metrics
}  // namespace vqa

using namespace vqa;
using namespace vqa::metrics;

extern "C" size_t vqa_kld_sum_loss_hits_workspace_bytes(int B, int kmax) {
  (void)kmax;
  return B > 0 ? (size_t)B * (sizeof(float) + sizeof(int)) : 0;
}

static int check_k(const char* what, int B, int C, int k) {
  VQA_REQUIRE(B > 0 && C > 0, VQA_E_BADARG, "%s: bad sizes B=%d C=%d", what, B, C);
  VQA_REQUIRE(C <= kThreads * kPerThread, VQA_E_UNSUPPORTED, "%s: C=%d exceeds %d", what, C, kThreads * kPerThread);
  VQA_REQUIRE(k >= 1 && k <= kMaxK && k <= C, VQA_E_BADARG, "%s: k=%d outside [1, min(%d, C=%d)]", what, k, kMaxK, C);
  return VQA_OK;
}

extern "C" int vqa_kld_sum_loss_hits(const float* logits, const float* target, float* loss, float* d_logits, int* hits, int kmax,
                                     void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  VQA_REQUIRE(logits && target && loss && hits && workspace, VQA_E_BADARG, "kld_sum_loss_hits: null pointer");
  const int rc = check_k("kld_sum_loss_hits", B, C, kmax);
  if (rc != VQA_OK) return rc;
  VQA_REQUIRE(workspace_bytes >= vqa_kld_sum_loss_hits_workspace_bytes(B, kmax), VQA_E_BADARG,
              "kld_sum_loss_hits: workspace of %zu B is too small", workspace_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* row_loss = static_cast<float*>(workspace);
  int* row_rank = reinterpret_cast<int*>(row_loss + B);
  VQA_LAUNCH(kld_hits_rows_kernel, dim3(B), dim3(kThreads), 0, s, logits, target, row_loss, row_rank, d_logits, C);
  VQA_LAUNCH(hits_total_kernel, dim3(1), dim3(kThreads), 0, s, row_rank, hits, kmax, row_loss, loss, B);
  return check_launch("kld_sum_loss_hits");
}

extern "C" size_t vqa_predict_topk_workspace_bytes(int B, int k) {
  (void)k;
  return B > 0 ? (size_t)B * sizeof(int) : 0;
}

extern "C" int vqa_predict_topk(const float* logits, const float* target, int64_t* top_idx, float* top_prob, int* hits, int k,
                                void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  VQA_REQUIRE(logits && top_idx, VQA_E_BADARG, "predict_topk: null pointer");
  const int rc = check_k("predict_topk", B, C, k);
  if (rc != VQA_OK) return rc;
  VQA_REQUIRE(target == nullptr || (hits != nullptr && workspace != nullptr), VQA_E_BADARG,
              "predict_topk: a target needs hits and a workspace");
  VQA_REQUIRE(target == nullptr || workspace_bytes >= vqa_predict_topk_workspace_bytes(B, k), VQA_E_BADARG,
              "predict_topk: workspace of %zu B is too small", workspace_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* row_rank = target != nullptr ? static_cast<int*>(workspace) : nullptr;
  VQA_LAUNCH(topk_rows_kernel, dim3(B), dim3(kThreads), 0, s, logits, target, top_idx, top_prob, row_rank, k, C);
  if (target != nullptr)
    VQA_LAUNCH(hits_total_kernel, dim3(1), dim3(kThreads), 0, s, row_rank, hits, k, (const float*)nullptr, (float*)nullptr, B);
  return check_launch("predict_topk");
}

extern "C" int vqa_predict_candidates(const float* logits, const int64_t* cand, int64_t* pred, int B, int C, int M,
                                      vqa_stream_t stream) {
  VQA_REQUIRE(logits && cand && pred, VQA_E_BADARG, "predict_candidates: null pointer");
  VQA_REQUIRE(B > 0 && C > 0 && M > 0, VQA_E_BADARG, "predict_candidates: bad sizes B=%d C=%d M=%d", B, C, M);
  VQA_REQUIRE(M <= kMaxCand, VQA_E_UNSUPPORTED, "predict_candidates: M=%d exceeds %d", M, kMaxCand);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rows = kThreads / kWave;
  VQA_LAUNCH(candidates_kernel, dim3((B + rows - 1) / rows), dim3(kThreads), 0, s, logits, cand, pred, B, C, M);
  return check_launch("predict_candidates");
}
