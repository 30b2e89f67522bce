// The three criteria of loss.hip on a SPARSE answer target: the (answer id, probability) pairs of the reference's wire format
// (a_10_idx, at most ten per question) as they come from the feed, instead of the dense [B,C] row the host would build of them.
//
//   a_idx int32 [B,K], a_val fp32 [B,K], 1 <= K <= 16.  Entry j of a row is LIVE iff 0 <= a_idx[j] < C and no later entry of the
//   row has the same id; padding is a_idx = -1.  The row means exactly the dense row of datasets.py:963-969,
//       a[:] = 0; for j in order: a[a_idx[j]] = a_val[j]                (the last pair of a duplicated id wins)
//   Domain: finite a_val >= 0.
//
//   KLD (sum):  sa = sum_live a, loss_b = sum_live a * (log a - (z - m - log se)) with the terms of a > 0 only;
//               dL/dz = softmax(z) * sa - a.  A row without a live pair: loss 0, gradient 0.
//   BCE (mean): loss_b = scale * [ sum_c min(softplus(z_c), 100) + sum_live a * (min(softplus(-z), 100) - min(softplus(z), 100)) ],
//               dL/dz = scale * (sigmoid(z) - a): loss.hip's softplus form and clamp, with the target's terms gathered over the pairs.
//   CE (mean) with a DRAWN label (the reference samples it on the host per item, datasets.py:952-959:
//               np.random.choice(choice_id, p=choice_prob)): label_b = the id of the first live pair whose running sum of a_val
//               exceeds u_b * sum_live a_val, u_b = (mask_word(row_offset + b, seed) >> 8) * 2^-24 in [0, 1) -- the library's counter
//               hash under the dropout kernels' seed convention (host seed, or *seed_ptr + seed read on the device, so a replayed
//               graph draws fresh labels every step).  Pairs with a_val = 0 are never drawn.  labels_out int64 [B]; loss and
//               gradient are CE's with that label.  A row with no live positive pair: label -1, loss 0, gradient 0.
//   HITS:       the rank of the target column among the logits under loss.hip's order ("beats": NaN above every number, then the
//               larger value, ties to the lower column).  KLD / BCE: the lowest id among the live pairs holding the row's largest
//               value if that value is > 0, else column 0 (torch.max(a, 1) of the dense row); CE: the drawn label, and rank C
//               (never a hit) for label -1.  Counting the hits changes no bit of the loss or the gradient.
//
// The shape is loss.hip's: one 256-thread workgroup per row, C <= 4096 logits in registers, unconditional loads from a clamped
// column, wave64 DPP reductions, row losses and ranks to a workspace that one workgroup totals in a fixed order (no atomics, no
// memset).  The K pairs of a row go through LDS once; liveness is O(K^2) work of the first K threads.  A pair's value reaches
// the gradient through its owning thread's register slot (unrolled selects inside a branch that only the owner's wave takes: the
// register row is never indexed dynamically), its logit goes back through LDS, and the per-pair terms of the loss are computed by
// thread j and added in pair order -- the sums over the target need no block reduction.
// HBM-bound: z is read and dz written (2 * B * C * 4 bytes, against the dense kernels' 3) plus 8 * K bytes of pairs per row.
// (loss.hip stays byte for byte what its counter tables were measured on, so the row helpers it shares are restated here.)
#include "common.hpp"

namespace vqa {
namespace sparse {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;  // C <= 4096
constexpr int kMaxK = 16;       // top-k hit counts
constexpr int kMaxPairs = 16;   // pairs per row
enum { kBce = 0, kCe = 1, kKld = 2 };

// a beats b (loss.hip's order)
__device__ __forceinline__ bool beats(float va, int ia, float vb, int ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ int wave_sum_i(int x) {
  x += dpp_mov_i<0xB1>(x);
  x += dpp_mov_i<0x4E>(x);
  x += dpp_mov_i<0x141>(x);
  x += dpp_mov_i<0x140>(x);
  return __builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
         __builtin_amdgcn_readlane(x, 48);
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

struct DrawCfg {  // CE: where u_b comes from (the dropout kernels' seed convention) and where the labels go
  uint64_t seed;
  const uint64_t* seed_ptr;
  uint64_t row_offset;
  int64_t* labels_out;
};

// One row of one criterion on the pairs a_idx / a_val [B,K].  HITS: also row_rank[b].  d_logits may be null (loss only).
template <int LOSS, bool HITS>
__global__ __launch_bounds__(kThreads) void sparse_loss_rows_kernel(const float* __restrict__ logits, const int* __restrict__ a_idx,
                                                                    const float* __restrict__ a_val, float* __restrict__ row_loss,
                                                                    int* __restrict__ row_rank, float* __restrict__ d_logits,
                                                                    DrawCfg draw, float scale, int C, int K) {
  __shared__ float red_s[4];
  __shared__ int ired_s[4];
  __shared__ int raw_s[kMaxPairs], id_s[kMaxPairs];       // a pair's id as given / as it counts (-1: not live)
  __shared__ float val_s[kMaxPairs], z_s[kMaxPairs];      // its value and the logit of its column
  __shared__ float t1_s[kMaxPairs], t2_s[kMaxPairs];      // its terms of the loss
  __shared__ float z0_s;                                  // the logit of column 0 (the target column of an all-zero row)
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (size_t)b * C;
  float zv[kPerThread], av[kPerThread];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int c = tid + i * kThreads;
    const float zt = z[min(c, C - 1)];  // unconditional loads from a clamped column
    zv[i] = c < C ? zt : -INFINITY;
    av[i] = 0.f;
    if constexpr (LOSS != kBce) m = fmaxf(m, zv[i]);
  }
  // the pairs of the row: through LDS once; thread j decides whether pair j is live
  if (tid < K) {
    raw_s[tid] = a_idx[(size_t)b * K + tid];
    val_s[tid] = a_val[(size_t)b * K + tid];
  }
  if (tid == 0) z0_s = zv[0];
  __syncthreads();
  if (tid < K) {
    const int id = raw_s[tid];
    bool live = id >= 0 && id < C;
    for (int j = tid + 1; j < K; ++j) live = live && raw_s[j] != id;
    id_s[tid] = live ? id : -1;
  }
  __syncthreads();
  // a live pair's value into its owning thread's slot, its logit into LDS (K is uniform; only the owner's wave enters the branch)
  for (int j = 0; j < K; ++j) {
    const int id = id_s[j];
    if (id >= 0 && (id & (kThreads - 1)) == tid) {
      const int slot = id >> 8;
      const float v = val_s[j];
      float zj = 0.f;
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) {
        if (i == slot) {
          zj = zv[i];
          if constexpr (LOSS != kCe) av[i] = v;
        }
      }
      z_s[j] = zj;
    }
  }
  __syncthreads();
  // what every thread needs of the pairs, in pair order (LDS broadcast reads, block-uniform results): the target's sum, the
  // target column of the hits, CE's drawn label
  float sa = 0.f;
  if constexpr (LOSS != kBce) {
    for (int j = 0; j < K; ++j) sa += id_s[j] >= 0 ? val_s[j] : 0.f;
  }
  int t = 0;         // the target column ...
  float zt = 0.f;    // ... and its logit
  bool none = false; // CE: no label could be drawn
  if constexpr (LOSS == kCe) {
    const uint32_t w = mask_word(draw.row_offset + (uint64_t)b, draw.seed_ptr != nullptr ? draw.seed_ptr[0] + draw.seed : draw.seed);
    const float thr = (float)(w >> 8) * 0x1p-24f * sa;
    float run = 0.f;
    int pick = -1, last = -1;
    for (int j = 0; j < K; ++j) {
      if (id_s[j] >= 0 && val_s[j] > 0.f) {
        run += val_s[j];
        last = j;
        if (pick < 0 && run > thr) pick = j;
      }
    }
    if (pick < 0) pick = last;  // (unreachable for finite values: the running sum ends at sa > thr; kept so a label is always live)
    none = pick < 0;
    t = none ? 0 : id_s[pick];
    zt = none ? 0.f : z_s[pick];
    if (tid == 0) draw.labels_out[b] = none ? -1 : t;
  } else if constexpr (HITS) {
    float bv = 0.f;
    int bj = -1;
    for (int j = 0; j < K; ++j) {
      const int id = id_s[j];
      const float v = val_s[j];
      if (id >= 0 && (v > bv || (v == bv && bj >= 0 && id < t))) { bv = v; bj = j; t = id; }
    }
    zt = bj >= 0 ? z_s[bj] : z0_s;
    if (bj < 0) t = 0;
  }
  if constexpr (HITS) {
    int rank = column_rank(zv, C, zt, t, ired_s);
    if (LOSS == kCe && none) rank = C;
    if (tid == 0) row_rank[b] = rank;
  }
  // the loss of the row; zv becomes the row of d_logits (KLD: of softmax's numerators, scaled by k at the store)
  float k = 0.f;
  if constexpr (LOSS == kBce) {
    if (tid < K) {  // pair j's term: a * (min(softplus(-z), 100) - min(softplus(z), 100))
      const float x = z_s[tid], a = val_s[tid];
      const float l1p = log1pf(expf(-fabsf(x)));
      const float sp = fmaxf(x, 0.f) + l1p, sn = fmaxf(-x, 0.f) + l1p;
      t1_s[tid] = id_s[tid] >= 0 ? a * (fminf(sn, 100.f) - fminf(sp, 100.f)) : 0.f;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int c = tid + i * kThreads;
      const float x = zv[i];
      const float e = expf(-fabsf(x));                  // in (0, 1]; 0 for the padded columns
      const float sp = fmaxf(x, 0.f) + log1pf(e);       // softplus(z)  = -log(1 - sigmoid(z))
      s += c < C ? fminf(sp, 100.f) : 0.f;
      const float r = 1.f / (1.f + e);
      zv[i] = ((x >= 0.f ? r : e * r) - av[i]) * scale; // (sigmoid(z) - a) * scale
    }
    s = block_sum(s, red_s);  // (its barriers also publish t1_s)
    if (tid == 0) {
      for (int j = 0; j < K; ++j) s += t1_s[j];
      row_loss[b] = s * scale;
    }
  } else {  // KLD and CE: over the softmax of the row
    m = block_max(m, red_s);
    if constexpr (LOSS == kKld) {
      if (tid < K) {  // pair j's terms: a * (z - m) and a * log a, for a > 0 (0 log 0 = 0)
        const float a = val_s[tid];
        const bool on = id_s[tid] >= 0 && a > 0.f;
        t1_s[tid] = on ? a * (z_s[tid] - m) : 0.f;
        t2_s[tid] = on ? a * logf(a) : 0.f;
      }
    }
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const float e = expf(zv[i] - m);  // exp(-inf) = 0 for the padded columns
      se += e;
      zv[i] = e;
    }
    se = block_sum(se, red_s);  // (its barriers also publish t1_s / t2_s)
    if constexpr (LOSS == kKld) {
      if (tid == 0) {
        float saz = 0.f, sal = 0.f;
        for (int j = 0; j < K; ++j) {
          saz += t1_s[j];
          sal += t2_s[j];
        }
        // sum_live a (log a - (z - m - log se)) = sal - saz + sa * log se
        row_loss[b] = sal - saz + sa * logf(se);
      }
      k = sa / se;
    } else {
      // logsumexp(z) - z_t = log se - (z_t - m)
      if (tid == 0) row_loss[b] = none ? 0.f : (logf(se) - (zt - m)) * scale;
      const float ks = none ? 0.f : scale / se, hot = none ? 0.f : scale;
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) zv[i] = tid + i * kThreads == t ? fmaf(zv[i], ks, -hot) : zv[i] * ks;
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

// one workgroup totals the rows (loss.hip's rows_total_kernel): loss[0] = the sum of the row losses (stride kThreads over b, then
// block_sum); given ranks, hits[j] = #{b : row_rank[b] <= j} for j < kmax
__global__ __launch_bounds__(kThreads) void sparse_rows_total_kernel(const float* __restrict__ row_loss, float* __restrict__ loss,
                                                                     const int* __restrict__ row_rank, int* __restrict__ hits,
                                                                     int kmax, int B) {
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

static size_t workspace_bytes(int B, bool want_hits) {  // row_loss float[B], then row_rank int[B]
  return B > 0 ? (size_t)B * (want_hits ? sizeof(float) + sizeof(int) : sizeof(float)) : 0;
}

// the six entry points: checks (nothing is launched when one fails), the row kernel, the totalling kernel
template <int LOSS>
static int launch(const char* what, const float* logits, const int32_t* a_idx, const float* a_val, float* loss, float* d_logits,
                  int* hits, int kmax, bool want_hits, float scale, DrawCfg draw, void* workspace, size_t bytes, int B, int C, int K,
                  vqa_stream_t stream) {
  VQA_REQUIRE(logits && a_idx && a_val && loss && workspace && (hits || !want_hits) && (LOSS != kCe || draw.labels_out),
              VQA_E_BADARG, "%s: null pointer", what);
  VQA_REQUIRE(B > 0 && C > 0, VQA_E_BADARG, "%s: bad sizes B=%d C=%d", what, B, C);
  VQA_REQUIRE(K >= 1 && K <= kMaxPairs, VQA_E_BADARG, "%s: K=%d pairs per row outside [1, %d]", what, K, kMaxPairs);
  VQA_REQUIRE(scale == scale && scale > 0.f && scale <= 3.0e38f, VQA_E_BADARG, "%s: scale must be positive and finite", what);
  VQA_REQUIRE(C <= kThreads * kPerThread, VQA_E_UNSUPPORTED, "%s: C=%d exceeds %d", what, C, kThreads * kPerThread);
  VQA_REQUIRE(!want_hits || (kmax >= 1 && kmax <= kMaxK && kmax <= C), VQA_E_BADARG, "%s: k=%d outside [1, min(%d, C=%d)]", what,
              kmax, kMaxK, C);
  VQA_REQUIRE(bytes >= workspace_bytes(B, want_hits), VQA_E_BADARG, "%s: workspace of %zu B is too small", what, bytes);
  VQA_REQUIRE(aligned(workspace, 4) && aligned(a_idx, 4) && aligned(a_val, 4) && aligned(draw.labels_out, 8) &&
                  aligned(draw.seed_ptr, 8),
              VQA_E_UNSUPPORTED, "%s: misaligned pairs, labels, seed word or workspace", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* row_loss = static_cast<float*>(workspace);
  int* row_rank = want_hits ? reinterpret_cast<int*>(row_loss + B) : nullptr;
  if (want_hits)
    VQA_LAUNCH((sparse_loss_rows_kernel<LOSS, true>), dim3(B), dim3(kThreads), 0, s, logits, a_idx, a_val, row_loss, row_rank,
               d_logits, draw, scale, C, K);
  else
    VQA_LAUNCH((sparse_loss_rows_kernel<LOSS, false>), dim3(B), dim3(kThreads), 0, s, logits, a_idx, a_val, row_loss, row_rank,
               d_logits, draw, scale, C, K);
  VQA_LAUNCH(sparse_rows_total_kernel, dim3(1), dim3(kThreads), 0, s, (const float*)row_loss, loss, (const int*)row_rank, hits, kmax,
             B);
  return check_launch(what);
}

}  // namespace sparse
}  // namespace vqa

using namespace vqa;
using namespace vqa::sparse;

extern "C" size_t vqa_sparse_loss_workspace_bytes(int B, int kmax) { return workspace_bytes(B, kmax > 0); }

extern "C" int vqa_kld_sum_loss_sparse(const float* logits, const int32_t* a_idx, const float* a_val, float* loss, float* d_logits,
                                       void* workspace, size_t workspace_bytes, int B, int C, int K, vqa_stream_t stream) {
  return launch<kKld>("kld_sum_loss_sparse", logits, a_idx, a_val, loss, d_logits, nullptr, 0, false, 1.f, DrawCfg{}, workspace,
                      workspace_bytes, B, C, K, stream);
}

extern "C" int vqa_kld_sum_loss_sparse_hits(const float* logits, const int32_t* a_idx, const float* a_val, float* loss,
                                            float* d_logits, int32_t* hits, int kmax, void* workspace, size_t workspace_bytes, int B,
                                            int C, int K, vqa_stream_t stream) {
  return launch<kKld>("kld_sum_loss_sparse_hits", logits, a_idx, a_val, loss, d_logits, hits, kmax, true, 1.f, DrawCfg{}, workspace,
                      workspace_bytes, B, C, K, stream);
}

extern "C" int vqa_bce_mean_loss_sparse(const float* logits, const int32_t* a_idx, const float* a_val, float* loss, float* d_logits,
                                        float scale, void* workspace, size_t workspace_bytes, int B, int C, int K,
                                        vqa_stream_t stream) {
  return launch<kBce>("bce_mean_loss_sparse", logits, a_idx, a_val, loss, d_logits, nullptr, 0, false, scale, DrawCfg{}, workspace,
                      workspace_bytes, B, C, K, stream);
}

extern "C" int vqa_bce_mean_loss_sparse_hits(const float* logits, const int32_t* a_idx, const float* a_val, float* loss,
                                             float* d_logits, int32_t* hits, int kmax, float scale, void* workspace,
                                             size_t workspace_bytes, int B, int C, int K, vqa_stream_t stream) {
  return launch<kBce>("bce_mean_loss_sparse_hits", logits, a_idx, a_val, loss, d_logits, hits, kmax, true, scale, DrawCfg{},
                      workspace, workspace_bytes, B, C, K, stream);
}

extern "C" int vqa_ce_mean_loss_sampled(const float* logits, const int32_t* a_idx, const float* a_val, int64_t* labels_out,
                                        float* loss, float* d_logits, float scale, uint64_t seed, const uint64_t* seed_ptr,
                                        uint64_t row_offset, void* workspace, size_t workspace_bytes, int B, int C, int K,
                                        vqa_stream_t stream) {
  return launch<kCe>("ce_mean_loss_sampled", logits, a_idx, a_val, loss, d_logits, nullptr, 0, false, scale,
                     DrawCfg{seed, seed_ptr, row_offset, labels_out}, workspace, workspace_bytes, B, C, K, stream);
}

extern "C" int vqa_ce_mean_loss_sampled_hits(const float* logits, const int32_t* a_idx, const float* a_val, int64_t* labels_out,
                                             float* loss, float* d_logits, int32_t* hits, int kmax, float scale, uint64_t seed,
                                             const uint64_t* seed_ptr, uint64_t row_offset, void* workspace, size_t workspace_bytes,
                                             int B, int C, int K, vqa_stream_t stream) {
  return launch<kCe>("ce_mean_loss_sampled_hits", logits, a_idx, a_val, loss, d_logits, hits, kmax, true, scale,
                     DrawCfg{seed, seed_ptr, row_offset, labels_out}, workspace, workspace_bytes, B, C, K, stream);
}
