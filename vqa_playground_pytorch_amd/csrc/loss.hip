// Everything the train step and the evaluator compute from a [B,C] row of logits: the three criteria of the reference
// driver (forward and gradient in one pass), the target's top-k hits, and the predictions of test() / visu.py.
//
//   KLD (train.py:536-544): KLDivLoss(size_average=False)(F.log_softmax(z), a), a sum over soft targets a:
//     loss    = sum_{b,c} a * (log a - log_softmax(z))                      (0 * log 0 = 0)
//     dL/dz   = softmax(z) * sum_c a - a
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
//   `scale` is a launch argument: 1 / (B_global * C) for BCE and 1 / B_global for CE, so that the SUM all-reduce of the
//   data-parallel step adds up to the reference's mean over the global batch (trainer.py).  KLD has none.
//
//   accuracy(output, a, topk=(1, 5)) (train.py:22-38, called at :70-72): target class = torch.max(a, 1) (the FIRST index of
//     the row's largest target value; for CE the label itself), a top-k hit when the target is among output.topk(k) -- counted
//     here without a sort: the target's rank r = #{c : z_c beats z_t} (order below) is a top-k hit iff r < k;
//   test() (train.py:110-191): OpenEnded = output.max(1), MultipleChoice = the best-scoring column among the a_mc_idx candidates;
//   visu.py:188-194: the top-5 columns and their softmax probabilities over the whole row.
//
// ONE order everywhere ("a beats b"): NaN ranks above every number (torch's topk / sort / max treat NaN as largest), otherwise
// the larger value, ties to the lower column index.  It is a total order on (value, column) pairs, so the j-th pick of a top-k
// is the best element beaten by the (j-1)-th pick: k block-wide arg-max rounds over a row held in registers, no sort, no state.
//
// ONE shape everywhere: one workgroup per row (C <= 4096 values in registers, unconditional loads from a clamped column,
// wave64 DPP reductions); the per-row losses and ranks go to a workspace and ONE workgroup totals them in a fixed order --
// bitwise reproducible, no atomics, no memset (torch's own [B,C] -> scalar sum zeroes its semaphores with a memset node, which
// replays wrongly inside a hipGraph on this ROCm: see api.hip).  The three criteria are instances of one row body, with and
// without the rank, so counting the hits cannot change a bit of the loss or the gradient.
// HBM-bound: KLD and BCE read z and a and write dz (3 * B * C * 4 bytes), CE reads z and writes dz (2 * B * C * 4 bytes).
#include <climits>

#include "common.hpp"

namespace vqa {
namespace rows {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;  // C <= 4096
constexpr int kMaxK = 16;
constexpr int kMaxCand = 256;
enum { kBce = 0, kCe = 1, kKld = 2 };  // (0 and 1 are mean_rows_kernel's first template argument)

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

// block-wide sums and maximum over one LDS slot set red_s[4]; the four waves are combined in a fixed order
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

// A row in registers: v[i] is column threadIdx.x + i * kThreads; columns >= C are excluded by index.
// The target column: the first index of the row's largest target value (C >= 1: always a real column).
__device__ __forceinline__ int first_largest(const float (&tv)[kPerThread], int C, float* bv_s, int* bi_s) {
  float bv = -INFINITY;
  int bi = INT_MAX;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = threadIdx.x + i * kThreads;
    if (c < C && beats(tv[i], c, bv, bi)) { bv = tv[i]; bi = c; }
  }
  block_best(bv, bi, bv_s, bi_s);
  return bi;
}
// The logit at column t (block-uniform, 0 <= t < C), handed to every thread through *zt_s.
__device__ __forceinline__ float logit_at(const float (&zv)[kPerThread], int t, float* zt_s) {
#pragma unroll
  for (int i = 0; i < kPerThread; ++i)
    if ((int)threadIdx.x + i * kThreads == t) *zt_s = zv[i];
  __syncthreads();
  return *zt_s;
}
// The rank of column t among the logits: #{c < C : z_c beats z_t}.
__device__ __forceinline__ int column_rank(const float (&zv)[kPerThread], int C, float zt, int t, int* red_s) {
  int n = 0;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = threadIdx.x + i * kThreads;
    n += (c < C && beats(zv[i], c, zt, t)) ? 1 : 0;
  }
  return block_sum_i(n, red_s);
}

// One row of one criterion.  kKld / kBce: `target` is the row-major [B,C] soft target; kCe: `labels` is int64 [B].
// HITS: also row_rank[b] = the rank of the target column among the logits.  d_logits may be null (loss only).
template <int LOSS, bool HITS>
__device__ __forceinline__ void loss_row(const float* __restrict__ logits, const float* __restrict__ target,
                                         const int64_t* __restrict__ labels, float* __restrict__ row_loss,
                                         int* __restrict__ row_rank, float* __restrict__ d_logits, float scale, int C) {
  __shared__ float red_s[4];
  __shared__ float bv_s[4], zt_s;
  __shared__ int bi_s[4], ired_s[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (size_t)b * C;
  const float* a = LOSS != kCe ? target + (size_t)b * C : nullptr;
  float zv[kPerThread], av[kPerThread];
  // KLD takes its row maximum here and CE in a loop of its own below, and KLD forms its gradient where it is stored: the
  // compiler's schedule follows these placements (with one loop for both maxima after the loads, KLD issued 2 of its 32 loads
  // before the first wait), and with them each instance compiles to the code it had as a kernel of its own.
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = tid + i * kThreads;
    const int cc = min(c, C - 1);  // unconditional loads from a clamped column
    const float zt = z[cc];
    zv[i] = c < C ? zt : -INFINITY;
    if constexpr (LOSS != kCe) {
      const float at = a[cc];
      av[i] = c < C ? at : 0.f;
    }
    if constexpr (LOSS == kKld) m = fmaxf(m, zv[i]);
  }
  // the target column, its logit and its rank
  int t = 0;
  float zt = 0.f;
  if constexpr (LOSS == kCe) {
    const int64_t l = labels[b];
    t = (int)(l < 0 ? 0 : (l > C - 1 ? C - 1 : l));
  } else if constexpr (HITS) {
    t = first_largest(av, C, bv_s, bi_s);
  }
  if constexpr (LOSS == kCe || HITS) zt = logit_at(zv, t, &zt_s);
  if constexpr (HITS) {
    const int rank = column_rank(zv, C, zt, t, ired_s);
    if (tid == 0) row_rank[b] = rank;
  }
  // the loss of the row; zv becomes the row of d_logits (KLD: of softmax's numerators, scaled by k at the store)
  float k = 0.f;
  if constexpr (LOSS == kBce) {
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
  } else {  // KLD and CE: over the softmax of the row
    if constexpr (LOSS == kCe) {
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) m = fmaxf(m, zv[i]);
    }
    m = block_max(m, red_s);
    float se = 0.f, sa = 0.f, saz = 0.f, sal = 0.f;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const float e = expf(zv[i] - m);  // exp(-inf) = 0 for the padded columns
      se += e;
      if constexpr (LOSS == kKld) {
        sa += av[i];
        if (av[i] > 0.f) {
          saz = fmaf(av[i], zv[i] - m, saz);
          sal = fmaf(av[i], logf(av[i]), sal);
        }
      }
      zv[i] = e;
    }
    se = block_sum(se, red_s);
    if constexpr (LOSS == kKld) {
      sa = block_sum(sa, red_s);
      saz = block_sum(saz, red_s);
      sal = block_sum(sal, red_s);
      // sum_c a (log a - (z - m - log se)) = sal - saz + sa * log se
      if (tid == 0) row_loss[b] = sal - saz + sa * logf(se);
      k = sa / se;
    } else {
      // logsumexp(z) - z_t = log se - (z_t - m)
      if (tid == 0) row_loss[b] = (logf(se) - (zt - m)) * scale;
      const float ks = scale / se;
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) zv[i] = tid + i * kThreads == t ? fmaf(zv[i], ks, -scale) : zv[i] * ks;
    }
  }
  if (d_logits != nullptr) {
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int c = tid + i * kThreads;
      if (c < C) d_logits[(size_t)b * C + c] = LOSS == kKld ? fmaf(zv[i], k, -av[i]) : zv[i];
    }
  }
}

template <int LOSS, bool HITS>  // LOSS: kBce or kCe
__global__ __launch_bounds__(kThreads) void mean_rows_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                             const int64_t* __restrict__ labels, float* __restrict__ row_loss,
                                                             int* __restrict__ row_rank, float* __restrict__ d_logits,
                                                             float scale, int C) {
  loss_row<LOSS, HITS>(logits, target, labels, row_loss, row_rank, d_logits, scale, C);
}

// one workgroup totals the rows: given row losses, loss[0] = their sum (stride kThreads over b, then block_sum: the same
// total whoever asks); given ranks, hits[j] = #{b : row_rank[b] <= j} for j < kmax
__global__ __launch_bounds__(kThreads) void rows_total_kernel(const float* __restrict__ row_loss, float* __restrict__ loss,
                                                              const int* __restrict__ row_rank, int* __restrict__ hits, int kmax,
                                                              int B) {
  __shared__ float red_s[4];
  __shared__ int ired_s[4];
  if (row_loss != nullptr) {
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += kThreads) s += row_loss[b];
    s = block_sum(s, red_s);
    if (threadIdx.x == 0) loss[0] = s;
  }
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
    const int t = first_largest(tv, C, bv_s[1], bi_s[1]);
    const float zt = logit_at(zv, t, &zt_s);
    const int rank = column_rank(zv, C, zt, t, ired_s);
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

}  // namespace rows

// The KLD instances live in vqa itself, outside rows: the benchmark's counter tables look the step's loss kernel up as
// vqa::kld_rows_kernel.
template <bool HITS>
__global__ __launch_bounds__(rows::kThreads) void kld_rows_kernel(const float* __restrict__ logits,
                                                                  const float* __restrict__ target,
                                                                  float* __restrict__ row_loss, int* __restrict__ row_rank,
                                                                  float* __restrict__ d_logits, int C) {
  rows::loss_row<rows::kKld, HITS>(logits, target, nullptr, row_loss, row_rank, d_logits, 1.f, C);
}

namespace rows {

static int check_sizes(const char* what, int B, int C, float scale) {
  VQA_REQUIRE(B > 0 && C > 0, VQA_E_BADARG, "%s: bad sizes B=%d C=%d", what, B, C);
  VQA_REQUIRE(scale == scale && scale > 0.f && scale <= 3.0e38f, VQA_E_BADARG, "%s: scale must be positive and finite", what);
  VQA_REQUIRE(C <= kThreads * kPerThread, VQA_E_UNSUPPORTED, "%s: C=%d exceeds %d", what, C, kThreads * kPerThread);
  return VQA_OK;
}
static int check_k(const char* what, int k, int C) {
  VQA_REQUIRE(k >= 1 && k <= kMaxK && k <= C, VQA_E_BADARG, "%s: k=%d outside [1, min(%d, C=%d)]", what, k, kMaxK, C);
  return VQA_OK;
}

static size_t loss_workspace_bytes(int B, bool want_hits) {  // row_loss float[B], then row_rank int[B]
  return B > 0 ? (size_t)B * (want_hits ? sizeof(float) + sizeof(int) : sizeof(float)) : 0;
}

// the six loss entry points: checks, the row kernel of LOSS with or without the ranks, the totalling kernel
template <int LOSS>
static int launch_loss(const char* what, const float* logits, const float* target, const int64_t* labels, float* loss,
                       float* d_logits, int* hits, int kmax, bool want_hits, float scale, void* workspace, size_t bytes, int B,
                       int C, vqa_stream_t stream) {
  VQA_REQUIRE(logits && (LOSS == kCe ? (const void*)labels : (const void*)target) && loss && workspace && (hits || !want_hits),
              VQA_E_BADARG, "%s: null pointer", what);
  int rc = check_sizes(what, B, C, scale);
  if (rc == VQA_OK && want_hits) rc = check_k(what, kmax, C);
  if (rc != VQA_OK) return rc;
  VQA_REQUIRE(bytes >= loss_workspace_bytes(B, want_hits), VQA_E_BADARG, "%s: workspace of %zu B is too small", what, bytes);
  // (the KLD entry points have never refused a misaligned workspace; they keep their return codes)
  VQA_REQUIRE(LOSS == kKld || (aligned(workspace, 4) && (LOSS == kBce || aligned(labels, 8))), VQA_E_UNSUPPORTED,
              "%s: misaligned labels or workspace", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* row_loss = static_cast<float*>(workspace);
  int* row_rank = want_hits ? reinterpret_cast<int*>(row_loss + B) : nullptr;
  if constexpr (LOSS == kKld) {
    if (want_hits)
      VQA_LAUNCH(kld_rows_kernel<true>, dim3(B), dim3(kThreads), 0, s, logits, target, row_loss, row_rank, d_logits, C);
    else
      VQA_LAUNCH(kld_rows_kernel<false>, dim3(B), dim3(kThreads), 0, s, logits, target, row_loss, row_rank, d_logits, C);
  } else {
    if (want_hits)
      VQA_LAUNCH((mean_rows_kernel<LOSS, true>), dim3(B), dim3(kThreads), 0, s, logits, target, labels, row_loss, row_rank,
                 d_logits, scale, C);
    else
      VQA_LAUNCH((mean_rows_kernel<LOSS, false>), dim3(B), dim3(kThreads), 0, s, logits, target, labels, row_loss, row_rank,
                 d_logits, scale, C);
  }
  VQA_LAUNCH(rows_total_kernel, dim3(1), dim3(kThreads), 0, s, (const float*)row_loss, loss, (const int*)row_rank, hits, kmax, B);
  return check_launch(what);
}

}  // namespace rows
}  // namespace vqa

using namespace vqa;
using namespace vqa::rows;

extern "C" size_t vqa_kld_sum_loss_workspace_bytes(int B) { return loss_workspace_bytes(B, false); }
extern "C" size_t vqa_mean_loss_workspace_bytes(int B) { return loss_workspace_bytes(B, false); }
extern "C" size_t vqa_kld_sum_loss_hits_workspace_bytes(int B, int kmax) {
  (void)kmax;
  return loss_workspace_bytes(B, true);
}
extern "C" size_t vqa_mean_loss_hits_workspace_bytes(int B, int kmax) {
  (void)kmax;
  return loss_workspace_bytes(B, true);
}
extern "C" size_t vqa_predict_topk_workspace_bytes(int B, int k) {
  (void)k;
  return B > 0 ? (size_t)B * sizeof(int) : 0;
}

extern "C" int vqa_kld_sum_loss(const float* logits, const float* target, float* loss, float* d_logits, void* workspace,
                                size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  return launch_loss<kKld>("kld_sum_loss", logits, target, nullptr, loss, d_logits, nullptr, 0, false, 1.f, workspace,
                           workspace_bytes, B, C, stream);
}

extern "C" int vqa_kld_sum_loss_hits(const float* logits, const float* target, float* loss, float* d_logits, int* hits, int kmax,
                                     void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  return launch_loss<kKld>("kld_sum_loss_hits", logits, target, nullptr, loss, d_logits, hits, kmax, true, 1.f, workspace,
                           workspace_bytes, B, C, stream);
}

extern "C" int vqa_bce_mean_loss(const float* logits, const float* target, float* loss, float* d_logits, float scale,
                                 void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  return launch_loss<kBce>("bce_mean_loss", logits, target, nullptr, loss, d_logits, nullptr, 0, false, scale, workspace,
                           workspace_bytes, B, C, stream);
}

extern "C" int vqa_bce_mean_loss_hits(const float* logits, const float* target, float* loss, float* d_logits, int* hits,
                                      int kmax, float scale, void* workspace, size_t workspace_bytes, int B, int C,
                                      vqa_stream_t stream) {
  return launch_loss<kBce>("bce_mean_loss_hits", logits, target, nullptr, loss, d_logits, hits, kmax, true, scale, workspace,
                           workspace_bytes, B, C, stream);
}

extern "C" int vqa_ce_mean_loss(const float* logits, const int64_t* labels, float* loss, float* d_logits, float scale,
                                void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  return launch_loss<kCe>("ce_mean_loss", logits, nullptr, labels, loss, d_logits, nullptr, 0, false, scale, workspace,
                          workspace_bytes, B, C, stream);
}

extern "C" int vqa_ce_mean_loss_hits(const float* logits, const int64_t* labels, float* loss, float* d_logits, int* hits, int kmax,
                                     float scale, void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  return launch_loss<kCe>("ce_mean_loss_hits", logits, nullptr, labels, loss, d_logits, hits, kmax, true, scale, workspace,
                          workspace_bytes, B, C, stream);
}

extern "C" int vqa_predict_topk(const float* logits, const float* target, int64_t* top_idx, float* top_prob, int* hits, int k,
                                void* workspace, size_t workspace_bytes, int B, int C, vqa_stream_t stream) {
  VQA_REQUIRE(logits && top_idx, VQA_E_BADARG, "predict_topk: null pointer");
  int rc = check_sizes("predict_topk", B, C, 1.f);
  if (rc == VQA_OK) rc = check_k("predict_topk", k, C);
  if (rc != VQA_OK) return rc;
  VQA_REQUIRE(target == nullptr || (hits != nullptr && workspace != nullptr), VQA_E_BADARG,
              "predict_topk: a target needs hits and a workspace");
  VQA_REQUIRE(target == nullptr || workspace_bytes >= vqa_predict_topk_workspace_bytes(B, k), VQA_E_BADARG,
              "predict_topk: workspace of %zu B is too small", workspace_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* row_rank = target != nullptr ? static_cast<int*>(workspace) : nullptr;
  VQA_LAUNCH(topk_rows_kernel, dim3(B), dim3(kThreads), 0, s, logits, target, top_idx, top_prob, row_rank, k, C);
  if (target != nullptr)
    VQA_LAUNCH(rows_total_kernel, dim3(1), dim3(kThreads), 0, s, (const float*)nullptr, (float*)nullptr, (const int*)row_rank, hits,
               k, B);
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
