// K3 with a region count per sample -- softmax over the first len_b regions of sample b + pooling of those rows.
//
// Adaptive bottom-up features carry 10..100 boxes per image, zero-padded to N.  The `_len_` entry points are the `_drop`
// entry points of attention_pool.hip applied to the rows n < len_b of sample b:
//
//   forward : the same (sample, 4*NT-wide feature chunk) ownership and prefetch-before-prologue as the unmasked kernel;
//             the softmax runs over n < len_b (logits beyond are never read), alpha is written 0 beyond, and the stream
//             stops at len_b.
//   backward: a workgroup owns (sample, kRows region rows) over ALL D columns, so every dot product <d_pooled_g, v_n>
//             is complete inside its workgroup: no accumulator to zero, no float atomics, one fixed summation order at
//             every shape.  Small batches: one such chunk per workgroup (a long sample is spread over ceil(len_b / kRows)
//             workgroups and its short neighbours return at once; workgroups past len_b only write the zero rows of d_v),
//             the dot products land in d_logits with plain stores and a second tiny kernel closes the softmax backward on
//             [len_b][G] in place and zero-fills the rest.  Batches that give every CU a workgroup: one workgroup walks all
//             chunks of its sample and closes the softmax itself (one launch).
//
// HBM-bound like K3: len_b * D elements per sample each way instead of N * D.
// lens is read by the kernels (never by the host): a replayed graph sees the current counts.  The kernels use
// min(max(lens[b], 1), N), so no value can index out of bounds or divide by zero; validation belongs to the host.
#include <cstdlib>

#include "common.hpp"

namespace vqa {

constexpr int kMaxG = 8;
constexpr int kRows = 16;   // region rows a backward workgroup owns

__device__ __forceinline__ int region_count(const int32_t* __restrict__ lens, int b, int N) {
  return min(max(lens[b], 1), N);
}

// softmax over n < L for every glimpse; logits_b -> alpha_s (LDS, [L][G]).  Called by all NT threads.
template <int NT>
__device__ __forceinline__ void block_softmax_first_regions(const float* __restrict__ logits_b, float* alpha_s, float* stat_s,
                                                            int L, int G) {
  const int tid = threadIdx.x;
  const int LG = L * G;
  for (int t = tid; t < LG; t += NT) alpha_s[t] = logits_b[t];
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int g = wave; g < G; g += NT / 64) {
    float m = -INFINITY;
    for (int n = lane; n < L; n += 64) m = fmaxf(m, alpha_s[n * G + g]);
    m = wave_max(m);
    float s = 0.f;
    for (int n = lane; n < L; n += 64) s += expf(alpha_s[n * G + g] - m);
    s = wave_sum(s);
    if (lane == 0) {
      stat_s[g] = m;
      stat_s[kMaxG + g] = 1.f / s;
    }
  }
  __syncthreads();
  for (int t = tid; t < LG; t += NT) {
    const int g = t % G;
    alpha_s[t] = expf(alpha_s[t] - stat_s[g]) * stat_s[kMaxG + g];
  }
  __syncthreads();
}

template <typename T, int NT, int G>
__global__ __launch_bounds__(NT) void attention_pool_len_fwd_kernel(const float* __restrict__ logits, const T* __restrict__ v,
                                                                    const int32_t* __restrict__ lens, float* __restrict__ alpha,
                                                                    float* __restrict__ pooled, float* __restrict__ first,
                                                                    int N, int D, DropCfg dc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* alpha_s = reinterpret_cast<float*>(smem);  // [N][G] (the first L rows are used)
  float* stat_s = alpha_s + N * G;                  // [2*kMaxG]
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int L = region_count(lens, b, N);
  const int d = (blockIdx.x * NT + tid) * 4;
  const bool active = d < D;
  const T* vb = v + (size_t)b * N * D + d;

  // start the first rows of the stream before the softmax prologue so HBM latency overlaps it
  constexpr int PF = 4;
  float4 pf[PF];
#pragma unroll
  for (int i = 0; i < PF; ++i) pf[i] = (active && i < L) ? ld4(vb + (size_t)i * D) : make_float4(0.f, 0.f, 0.f, 0.f);

  block_softmax_first_regions<NT>(logits + (size_t)b * N * G, alpha_s, stat_s, L, G);
  if (blockIdx.x == 0)
    for (int t = tid; t < N * G; t += NT) alpha[(size_t)b * N * G + t] = t < L * G ? alpha_s[t] : 0.0f;
  if (!active) return;

  float4 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < PF; ++i) {
    if (i < L) {
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = fma4(alpha_s[i * G + g], pf[i], acc[g]);
    }
  }
#pragma unroll 8
  for (int n = PF; n < L; ++n) {
    const float4 x = ld4(vb + (size_t)n * D);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = fma4(alpha_s[n * G + g], x, acc[g]);
  }
  if (first != nullptr) st4(first + (size_t)b * D + d, acc[0]);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const size_t e = ((size_t)b * G + g) * D + d;      // the unmasked kernel's dropout counter: element of [B,G,D]
    float4 o = acc[g];
    if (dc.p8 > 0) o = mul4(o, drop_quad((uint32_t)e, dc));
    st4(pooled + e, o);
  }
}

// d_logits = alpha (dal - sum_{n < L} alpha dal) on the first L rows of one sample, 0 beyond.  dal_b: the dot products
// <d_pooled_g, v_n> (+ ext_b: the gradient arriving on alpha directly, whose rows n >= L are never read) -- LDS, or the
// sample's rows of d_logits itself (then every element is read before the barrier and overwritten after it).
template <int NT>
__device__ __forceinline__ void close_softmax_first_regions(const float* __restrict__ alpha_b, const float* dal_b,
                                                            const float* __restrict__ ext_b, float* out_b, float* inner_s, int L,
                                                            int N, int G) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int gI = wave; gI < G; gI += NT / 64) {
    float s = 0.f;
    for (int n = lane; n < L; n += 64) {
      const int i = n * G + gI;
      s += alpha_b[i] * (dal_b[i] + (ext_b != nullptr ? ext_b[i] : 0.f));
    }
    s = wave_sum(s);
    if (lane == 0) inner_s[gI] = s;
  }
  __syncthreads();
  for (int t = tid; t < N * G; t += NT) {
    float o = 0.0f;
    if (t < L * G) o = alpha_b[t] * (dal_b[t] + (ext_b != nullptr ? ext_b[t] : 0.f) - inner_s[t % G]);
    out_b[t] = o;
  }
}

// Backward, the streaming kernel.  A workgroup works on chunks of kRows region rows over ALL D columns: every lane keeps CG
// float4 columns of the G rows of d_pooled (mask and d_first applied) in registers; 4 NT CG columns per pass, D in as many
// passes as it takes.  RB = 16 / G rows per batch: the RB G dot products of a batch go through ONE butterfly reduce-scatter
// over the 16 lanes of a DPP row, the four rows of the wave are added (rows_sum), every wave stores to its OWN LDS slot and
// the slots are added in wave order.
//   WHOLE = false: grid (ceil(N / kRows), B), one chunk per workgroup.  out [B,N,G] is d_logits used as dal: rows n < len_b
//                  receive <d_pooled_g, v_n>, attention_softmax_len_bwd_kernel closes the softmax in a second launch.
//   WHOLE = true : grid (1, B), the workgroup walks all chunks of its sample, keeps dal in LDS (N G floats) and closes the
//                  softmax itself: one launch, d_pooled read once per sample.
template <typename T, int NT, int G, bool WHOLE>
__global__ __launch_bounds__(NT) void attention_pool_len_bwd_kernel(const float* __restrict__ alpha, const T* __restrict__ v,
                                                                    const int32_t* __restrict__ lens,
                                                                    const float* __restrict__ d_pooled,
                                                                    const float* __restrict__ d_first,
                                                                    const float* __restrict__ d_alpha_ext, float* __restrict__ out,
                                                                    T* __restrict__ d_v, int N, int D, DropCfg dc) {
  constexpr int CG = 2, RB = 16 / G, W = NT / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dal_s = reinterpret_cast<float*>(smem);     // WHOLE: [N][G]
  __shared__ float alpha_s[kRows * G];
  __shared__ float red_s[kRows * G];
  __shared__ float part_s[W][kRows * G];
  __shared__ float inner_s[kMaxG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int L = region_count(lens, b, N);
  const T* vb = v + (size_t)b * N * D;
  T* dvb = d_v ? d_v + (size_t)b * N * D : nullptr;
  const int my_k = (lane & 15) / G, my_g = (lane & 15) % G;
  const bool one_pass = D <= CG * NT * 4;            // then the registers hold d_pooled for every chunk of the sample
  float4 p[CG][G];
  int dcol[CG];
  bool active[CG];
  auto load_p = [&](int d0) {
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      const int d = d0 + (c * NT + tid) * 4;
      active[c] = d < D;
      dcol[c] = active[c] ? d : 0;
#pragma unroll
      for (int gI = 0; gI < G; ++gI) {
        const size_t e = ((size_t)b * G + gI) * D + dcol[c];
        float4 t = ld4(d_pooled + e);
        if (dc.p8 > 0) t = mul4(t, drop_quad((uint32_t)e, dc));   // the forward's dropout of `pooled`
        if (gI == 0 && d_first != nullptr) t = add4(t, ld4(d_first + (size_t)b * D + dcol[c]));
        p[c][gI] = active[c] ? t : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  if (one_pass) load_p(0);
  // (every bound below is uniform over the workgroup)
  for (int n_lo = WHOLE ? 0 : blockIdx.x * kRows; n_lo < N; n_lo += WHOLE ? kRows : N) {
    const int n_top = min(n_lo + kRows, N);
    if (dvb != nullptr) {                            // the absent rows of this chunk
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int n = max(n_lo, L); n < n_top; ++n)
        for (int c = tid * 4; c < D; c += NT * 4) st4(dvb + (size_t)n * D + c, z);
    }
    if (n_lo >= L) {
      if (dvb == nullptr) break;                     // nothing left to write
      continue;
    }
    const int rows = min(n_top, L) - n_lo;           // 1 .. kRows
    const int RG = rows * G;
    for (int t = tid; t < RG; t += NT) {
      alpha_s[t] = alpha[((size_t)b * N + n_lo) * G + t];
      red_s[t] = 0.f;
    }
    for (int d0 = 0; d0 < D; d0 += CG * NT * 4) {
      if (!one_pass) load_p(d0);
      __syncthreads();    // alpha_s / red_s are set (first pass); part_s of the pass or chunk before has been read
      for (int r0 = 0; r0 < rows; r0 += RB) {
        float4 x[CG][RB];
#pragma unroll
        for (int c = 0; c < CG; ++c)
#pragma unroll
          for (int k = 0; k < RB; ++k) x[c][k] = ld4(vb + (size_t)(n_lo + min(r0 + k, rows - 1)) * D + dcol[c]);
        float val[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) val[i] = 0.f;
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          const int r = r0 + k;
#pragma unroll
          for (int gI = 0; gI < G; ++gI) {
            float t = 0.f;
#pragma unroll
            for (int c = 0; c < CG; ++c) t += dot4(x[c][k], p[c][gI]);     // (p = 0 in inactive columns)
            val[k * G + gI] = t;
          }
          if (dvb != nullptr && r < rows) {
#pragma unroll
            for (int c = 0; c < CG; ++c)
              if (active[c]) {
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int gI = 0; gI < G; ++gI) o = fma4(alpha_s[r * G + gI], p[c][gI], o);
                st4(dvb + (size_t)(n_lo + r) * D + dcol[c], o);
              }
          }
        }
        const float s1 = rows_sum(row_reduce_scatter16(val, lane));
        const int r = r0 + my_k;
        if (lane < 16 && my_k < RB && r < rows) part_s[wave][r * G + my_g] = s1;
      }
      __syncthreads();
      for (int t = tid; t < RG; t += NT) {
        float sum = part_s[0][t];
#pragma unroll
        for (int w = 1; w < W; ++w) sum += part_s[w][t];
        red_s[t] += sum;                              // (thread t owns element t in every pass and chunk)
      }
    }
    for (int t = tid; t < RG; t += NT) {
      if constexpr (WHOLE) dal_s[n_lo * G + t] = red_s[t];
      else out[((size_t)b * N + n_lo) * G + t] = red_s[t];
    }
  }
  if constexpr (WHOLE) {
    __syncthreads();
    const size_t base = (size_t)b * N * G;
    close_softmax_first_regions<NT>(alpha + base, dal_s, d_alpha_ext != nullptr ? d_alpha_ext + base : nullptr, out + base, inner_s,
                                    L, N, G);
  }
}

// Backward, second launch of the WHOLE = false form: closes the softmax in place over d_logits.
__global__ __launch_bounds__(256) void attention_softmax_len_bwd_kernel(const float* __restrict__ alpha,
                                                                        const int32_t* __restrict__ lens,
                                                                        const float* __restrict__ d_alpha_ext,
                                                                        float* __restrict__ d_logits, int N, int G) {
  __shared__ float inner_s[kMaxG];
  const int b = blockIdx.x;
  const size_t base = (size_t)b * N * G;
  close_softmax_first_regions<256>(alpha + base, d_logits + base, d_alpha_ext != nullptr ? d_alpha_ext + base : nullptr,
                                   d_logits + base, inner_s, region_count(lens, b, N), N, G);
}

template <typename T, int G>
static int launch_len_fwd(const float* logits, const T* v, const int32_t* lens, float* alpha, float* pooled, float* first,
                          const DropCfg& dc, int B, int N, int D, hipStream_t s) {
  constexpr int NT = 256;
  const size_t lds = ((size_t)N * G + 2 * kMaxG) * sizeof(float);     // 32 832 bytes at N = 1024, G = 8
  dim3 grid((D / 4 + NT - 1) / NT, B);
  VQA_LAUNCH((attention_pool_len_fwd_kernel<T, NT, G>), grid, dim3(NT), lds, s, logits, v, lens, alpha, pooled, first, N, D, dc);
  return check_launch("softmax_attention_pool_len_fwd");
}

template <typename T, int G>
static int launch_len_bwd(const float* alpha, const T* v, const int32_t* lens, const float* d_pooled, const float* d_first,
                          const float* d_alpha_ext, float* d_logits, T* d_v, const DropCfg& dc, int B, int N, int D, hipStream_t s) {
  constexpr int NT = 256;
  // One workgroup per sample from a batch that gives every CU one on (256 CUs): one launch, d_pooled read once per sample;
  // several workgroups per CU even out the samples' unequal lengths.  A smaller batch spreads every sample over
  // ceil(N / kRows) workgroups, so that a long sample does not run on one CU while the others idle.
  // (VQA_K3_LEN_WHOLE_MIN_B: the smallest batch that takes the one-launch form; tests set 1, a huge value keeps the other)
  const char* env = vqa::option("VQA_K3_LEN_WHOLE_MIN_B");
  const int min_b = env != nullptr ? std::atoi(env) : 256;
  if (B >= min_b) {
    VQA_LAUNCH((attention_pool_len_bwd_kernel<T, NT, G, true>), dim3(1, B), dim3(NT), (size_t)N * G * sizeof(float), s, alpha, v,
               lens, d_pooled, d_first, d_alpha_ext, d_logits, d_v, N, D, dc);     // (32 KiB of dynamic LDS at most)
    return check_launch("softmax_attention_pool_len_bwd");
  }
  VQA_LAUNCH((attention_pool_len_bwd_kernel<T, NT, G, false>), dim3((N + kRows - 1) / kRows, B), dim3(NT), 0, s, alpha, v, lens,
             d_pooled, d_first, nullptr, d_logits, d_v, N, D, dc);
  VQA_LAUNCH(attention_softmax_len_bwd_kernel, dim3(B), dim3(256), 0, s, alpha, lens, d_alpha_ext, d_logits, N, G);
  return check_launch("softmax_attention_pool_len_bwd");
}

template <typename T>
static int pool_len_fwd_impl(const char* who, const float* logits, const T* v, const int32_t* lens, float* alpha, float* pooled,
                      float* first, float p_drop, uint64_t seed, const uint64_t* seed_ptr, int B, int N, int D, int G,
                      vqa_stream_t stream) {
  constexpr size_t kAlign = 4 * sizeof(T);
  VQA_REQUIRE(logits && v && lens && alpha && pooled, VQA_E_BADARG, "%s: null pointer", who);
  VQA_REQUIRE(B > 0 && N > 0 && D > 0 && G > 0, VQA_E_BADARG, "%s: bad sizes B=%d N=%d D=%d G=%d", who, B, N, D, G);
  VQA_REQUIRE(G <= kMaxG && N <= 1024, VQA_E_UNSUPPORTED, "%s: needs G <= 8 and N <= 1024 (G=%d N=%d)", who, G, N);
  VQA_REQUIRE(D % 4 == 0 && aligned(v, kAlign) && aligned(pooled, 16) && aligned(lens, 4), VQA_E_UNSUPPORTED,
              "%s: needs D %% 4 == 0, %zu-byte aligned v, 16-byte aligned pooled and 4-byte aligned lens (D=%d)", who, kAlign, D);
  VQA_REQUIRE(B <= 65535, VQA_E_UNSUPPORTED, "%s: B=%d exceeds 65535", who, B);
  VQA_REQUIRE(p_drop >= 0.f && p_drop < 1.f, VQA_E_BADARG, "%s: p_drop=%f outside [0,1)", who, (double)p_drop);
  VQA_REQUIRE(p_drop == 0.f || (size_t)B * G * D < (1ull << 32), VQA_E_UNSUPPORTED, "%s: dropout needs B*G*D < 2^32", who);
  VQA_REQUIRE(first == nullptr || aligned(first, 16), VQA_E_UNSUPPORTED, "%s: first is not 16-byte aligned", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const DropCfg dc = make_drop(p_drop, seed, seed_ptr);
#define CALL_FWD(G_) launch_len_fwd<T, G_>(logits, v, lens, alpha, pooled, first, dc, B, N, D, s)
  switch (G) {
    case 1: return CALL_FWD(1);
    case 2: return CALL_FWD(2);
    case 3: return CALL_FWD(3);
    case 4: return CALL_FWD(4);
    case 5: return CALL_FWD(5);
    case 6: return CALL_FWD(6);
    case 7: return CALL_FWD(7);
    default: return CALL_FWD(8);
  }
#undef CALL_FWD
}

template <typename T>
static int pool_len_bwd_impl(const char* who, const float* alpha, const T* v, const int32_t* lens, const float* d_pooled,
                      const float* d_first, const float* d_alpha_ext, float* d_logits, T* d_v, float p_drop, uint64_t seed,
                      const uint64_t* seed_ptr, int B, int N, int D, int G, vqa_stream_t stream) {
  constexpr size_t kAlign = 4 * sizeof(T);
  VQA_REQUIRE(alpha && v && lens && d_pooled && d_logits, VQA_E_BADARG, "%s: null pointer", who);
  VQA_REQUIRE(B > 0 && N > 0 && D > 0 && G > 0, VQA_E_BADARG, "%s: bad sizes B=%d N=%d D=%d G=%d", who, B, N, D, G);
  VQA_REQUIRE(G <= kMaxG && N <= 1024, VQA_E_UNSUPPORTED, "%s: needs G <= 8 and N <= 1024 (G=%d N=%d)", who, G, N);
  VQA_REQUIRE(D % 4 == 0 && aligned(v, kAlign) && aligned(d_pooled, 16) && (d_v == nullptr || aligned(d_v, kAlign)) &&
                  aligned(lens, 4),
              VQA_E_UNSUPPORTED, "%s: needs D %% 4 == 0, 16-byte aligned d_pooled, %zu-byte aligned v/d_v and 4-byte aligned lens (D=%d)",
              who, kAlign, D);
  VQA_REQUIRE(B <= 65535, VQA_E_UNSUPPORTED, "%s: B=%d exceeds 65535", who, B);
  VQA_REQUIRE(p_drop >= 0.f && p_drop < 1.f, VQA_E_BADARG, "%s: p_drop=%f outside [0,1)", who, (double)p_drop);
  VQA_REQUIRE(p_drop == 0.f || (size_t)B * G * D < (1ull << 32), VQA_E_UNSUPPORTED, "%s: dropout needs B*G*D < 2^32", who);
  VQA_REQUIRE(d_first == nullptr || aligned(d_first, 16), VQA_E_UNSUPPORTED, "%s: d_first is not 16-byte aligned", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const DropCfg dc = make_drop(p_drop, seed, seed_ptr);
#define CALL_BWD(G_) launch_len_bwd<T, G_>(alpha, v, lens, d_pooled, d_first, d_alpha_ext, d_logits, d_v, dc, B, N, D, s)
  switch (G) {
    case 1: return CALL_BWD(1);
    case 2: return CALL_BWD(2);
    case 3: return CALL_BWD(3);
    case 4: return CALL_BWD(4);
    case 5: return CALL_BWD(5);
    case 6: return CALL_BWD(6);
    case 7: return CALL_BWD(7);
    default: return CALL_BWD(8);
  }
#undef CALL_BWD
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_softmax_attention_pool_len_fwd(const float* logits, const float* v, const int32_t* lens, float* alpha,
                                                  float* pooled, float* first, float p_drop, uint64_t seed,
                                                  const uint64_t* seed_ptr, int B, int N, int D, int G, vqa_stream_t stream) {
  return pool_len_fwd_impl<float>("softmax_attention_pool_len_fwd", logits, v, lens, alpha, pooled, first, p_drop, seed, seed_ptr,
                                  B, N, D, G, stream);
}

extern "C" int vqa_softmax_attention_pool_len_fwd_bf16(const float* logits, const vqa_bf16_t* v, const int32_t* lens,
                                                       float* alpha, float* pooled, float* first, float p_drop, uint64_t seed,
                                                       const uint64_t* seed_ptr, int B, int N, int D, int G,
                                                       vqa_stream_t stream) {
  return pool_len_fwd_impl<bf16>("softmax_attention_pool_len_fwd_bf16", logits, reinterpret_cast<const bf16*>(v), lens, alpha,
                                 pooled, first, p_drop, seed, seed_ptr, B, N, D, G, stream);
}

extern "C" int vqa_softmax_attention_pool_len_bwd(const float* alpha, const float* v, const int32_t* lens, const float* d_pooled,
                                                  const float* d_first, const float* d_alpha_ext, float* d_logits, float* d_v,
                                                  float p_drop, uint64_t seed, const uint64_t* seed_ptr, int B, int N, int D,
                                                  int G, vqa_stream_t stream) {
  return pool_len_bwd_impl<float>("softmax_attention_pool_len_bwd", alpha, v, lens, d_pooled, d_first, d_alpha_ext, d_logits, d_v,
                                  p_drop, seed, seed_ptr, B, N, D, G, stream);
}

extern "C" int vqa_softmax_attention_pool_len_bwd_bf16(const float* alpha, const vqa_bf16_t* v, const int32_t* lens,
                                                       const float* d_pooled, const float* d_first, const float* d_alpha_ext,
                                                       float* d_logits, vqa_bf16_t* d_v, float p_drop, uint64_t seed,
                                                       const uint64_t* seed_ptr, int B, int N, int D, int G,
                                                       vqa_stream_t stream) {
  return pool_len_bwd_impl<bf16>("softmax_attention_pool_len_bwd_bf16", alpha, reinterpret_cast<const bf16*>(v), lens, d_pooled,
                                 d_first, d_alpha_ext, d_logits, reinterpret_cast<bf16*>(d_v), p_drop, seed, seed_ptr, B, N, D, G,
                                 stream);
}
