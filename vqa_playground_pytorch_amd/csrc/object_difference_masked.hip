// K2 with per-sample region counts -- object-difference attention logits over the first n_b regions of every sample.
//
// The unmasked kernels (object_difference.hip) treat all N rows of vl[b] as regions.  A padded batch of adaptive features
// (10..36 boxes, zero-padded to N) has n_b = lens[b] real rows per sample; here
//
//   logits[b,i,g] = bias[g] + sum_{j < n_b, d} w[g,j*L+d] * keep(b,i,j,d) * (T[b,i,d] - T[b,j,d])   for i < n_b,   T = vl * ql
//   logits[b,i,g] = 0                                                                              for i >= n_b
//
// and the backward is its exact transpose: d_vl is 0 on the padding, d_ql / d_bias sum over the real rows, the filter slot
// w[g,j,:] receives nothing from a sample with n_b <= j.  lens is a DEVICE int32 [B] read by the kernels (a replayed graph
// sees the current counts) and clamped as the masked K3 kernels clamp it: n_b = min(max(lens[b], 1), N).
//
// keep() is the unmasked kernels' function of (seed, b, i, j, d): the same hash, the same two counter layouts, counters
// built from N and never from n_b -- whether an element is kept does not depend on the counts, and
// vqa_object_difference_dropout_mask stays the oracle.  The layout decision (oda_bits_mode, VQA_K2_BYTE_MASK) is restated
// below because object_difference.hip is a pinned file; nothing is moved out of it.
//
// Padding is never READ: no row i >= n_b of vl[b] or d_logits[b] is loaded, not even to keep a lane busy -- a NaN there
// cannot reach an output.  Loops over i and j stop at n_b (rounded up to the kernel's own group of four regions); no kernel
// walks N x N pairs and zeroes afterwards.  No float atomics, every sum in a fixed order: two runs give the same bits.
//
// Two families, chosen as the unmasked path chooses (oda_mfma_ok and oda_bits_mode, restated at the dispatch):
//   * G <= 4, N <= 36, p = 0 or the one-bit p = 0.5 mask: the unmasked path's DEFAULT kernels stopped at n_b -- the 4x4-MFMA
//     forward (packed subtracts), the staged 4x4-MFMA weight gradient with two sample slots per group, and the data gradient
//     (one-bit split / one-bit / plain form under the unmasked dispatch conditions).  Same accumulation order: with every
//     lens[b] = N they return the unmasked entry points' bits.
//   * everything else within the limits (N > 36, G > 4, any other rate, VQA_K2_MFMA=0, VQA_K2_BYTE_MASK=1): a general VALU
//     family (forward, data gradient, weight-gradient slabs), lane <-> feature d, one hash word per four regions i in either
//     layout.  No bit equality with the unmasked kernels is promised there.
// Both end in the slab reduce and a bias gradient over the real rows.  Knobs: VQA_K2_MFMA and VQA_K2_BYTE_MASK are honoured
// (they decide the mask layout and the path's eligibility); the A/B knobs VQA_K2_PK, VQA_K2_WSTAGE, VQA_K2_FUSED and
// VQA_K2_DATA_SPLIT are not read -- the forms they select lost their measurements and have no masked twins.
#include <cstdlib>

#include <type_traits>
#include <utility>

#include "gemm_f32_rt.hpp"

namespace vqa {

constexpr int kLenMaxG = 8;
constexpr int kLenIC = 12;   // regions i (forward, data gradient) or j (weight gradient) in registers per pass: three quads

// mask layouts (template parameter MODE)
constexpr int kLenPlain = 0;   // p = 0
constexpr int kLenByte = 1;    // one byte per element: word ((b*NQ + i/4)*N + j)*L + d (64-bit counter), byte i%4, keep iff >= p8
constexpr int kLenBit = 2;     // p = 0.5: one bit per element: word ((b*NI + i/32)*N + j)*L + d (32-bit counter), bit i%32

__device__ __forceinline__ int len_of(const int32_t* __restrict__ lens, int b, int N) { return min(max(lens[b], 1), N); }

struct LenMask {
  uint32_t key;        // bit layout
  uint64_t seed_eff;   // byte layout
  uint32_t p8;
  float scale;
  int NQ, NI;
};
__device__ __forceinline__ LenMask len_mask(const DropCfg& dc, int N) {
  return LenMask{drop_key(dc), dc.effective(), dc.p8, dc.scale, (N + 3) >> 2, (N + 31) >> 5};
}
// the hash word of regions 4 iq .. 4 iq + 3 of one (b, j, d), region 4 iq + k in bit k (bit layout) or byte k (byte layout)
template <int MODE>
__device__ __forceinline__ uint32_t len_word(const LenMask& m, int b, int iq, int j, int d, int N, int L) {
  if constexpr (MODE == kLenBit) {
    const uint32_t cnt = (((uint32_t)b * (uint32_t)m.NI + (uint32_t)(iq >> 3)) * (uint32_t)N + (uint32_t)j) * (uint32_t)L + (uint32_t)d;
    return mask_word32(cnt, m.key) >> ((iq & 7) * 4);
  } else if constexpr (MODE == kLenByte) {
    return mask_word((((uint64_t)b * m.NQ + iq) * N + j) * L + d, m.seed_eff);
  } else {
    return 0u;
  }
}
// keep / (1 - p) of region 4 iq + k
template <int MODE>
__device__ __forceinline__ float len_keep(const LenMask& m, uint32_t word, int k) {
  if constexpr (MODE == kLenBit) return ((word >> k) & 1u) != 0u ? m.scale : 0.f;
  else if constexpr (MODE == kLenByte) return ((word >> (8 * k)) & 255u) >= m.p8 ? m.scale : 0.f;
  else return 1.f;
}
// T = vl * ql as a ROUNDED product on both sides of T_i - T_j (no fma contraction): T_i - T_i is exactly zero
__device__ __forceinline__ float len_T(float v, float q) {
  float t = v * q;
  asm("" : "+v"(t));
  return t;
}

// ------------------------------------------------------------------------------------------ forward
// grid (ceil(N/kLenIC), B); block = round_up(min(L,1024), 64) threads, lane <-> feature d.  A workgroup whose chunk of
// regions i starts at or behind n_b writes its zeros and leaves.
template <int G, int MODE>
__global__ void oda_len_fwd_kernel(const float* __restrict__ vl, const float* __restrict__ ql, const float* __restrict__ w,
                                   const float* __restrict__ bias, const int32_t* __restrict__ lens,
                                   float* __restrict__ logits, DropCfg dc, int N, int L) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red_s = reinterpret_cast<float*>(smem);  // [nwaves][kLenIC*G]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int b = blockIdx.y, i0 = blockIdx.x * kLenIC;
  const int nb = len_of(lens, b, N);
  float* out = logits + ((size_t)b * N + i0) * G;
  const int rows = min(kLenIC, N - i0);
  if (i0 >= nb) {
    for (int t = tid; t < rows * G; t += blockDim.x) out[t] = 0.f;
    return;
  }
  const LenMask m = len_mask(dc, N);
  const float* vlb = vl + (size_t)b * N * L;
  const int nq = (min(kLenIC, nb - i0) + 3) >> 2;      // quads of regions i of this chunk with a real row
  float acc[kLenIC][G];
#pragma unroll
  for (int ic = 0; ic < kLenIC; ++ic)
#pragma unroll
    for (int g = 0; g < G; ++g) acc[ic][g] = 0.f;

  for (int d = tid; d < L; d += blockDim.x) {
    const float qd = ql[(size_t)b * L + d];
    float Ti[kLenIC];
#pragma unroll
    for (int ic = 0; ic < kLenIC; ++ic) Ti[ic] = (i0 + ic < nb) ? len_T(vlb[(size_t)(i0 + ic) * L + d], qd) : 0.f;
    for (int j = 0; j < nb; ++j) {
      const float Tj = len_T(vlb[(size_t)j * L + d], qd);
      float wv[G];
#pragma unroll
      for (int g = 0; g < G; ++g) wv[g] = w[((size_t)g * N + j) * L + d];
#pragma unroll
      for (int q = 0; q < kLenIC / 4; ++q) {
        if (q < nq) {                                    // (workgroup-uniform)
          const uint32_t word = len_word<MODE>(m, b, (i0 >> 2) + q, j, d, N, L);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int ic = q * 4 + k;
            float val = Ti[ic] - Tj;                     // (a region of the quad behind n_b: finite, and its sum is dropped)
            if (MODE != kLenPlain) val *= len_keep<MODE>(m, word, k);
#pragma unroll
            for (int g = 0; g < G; ++g) acc[ic][g] = fmaf(wv[g], val, acc[ic][g]);
          }
        }
      }
    }
  }
  // reduce over d: wave64 DPP sums, then across waves through LDS in wave order
#pragma unroll
  for (int ic = 0; ic < kLenIC; ++ic)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float r = wave_sum(acc[ic][g]);
      if (lane == 0) red_s[wave * (kLenIC * G) + ic * G + g] = r;
    }
  __syncthreads();
  for (int t = tid; t < rows * G; t += blockDim.x) {
    const int ic = t / G, g = t % G;
    float s = 0.f;
    if (i0 + ic < nb) {
      s = bias[g];
      for (int wv = 0; wv < nwaves; ++wv) s += red_s[wv * (kLenIC * G) + t];
    }
    out[t] = s;
  }
}

// ----------------------------------------------------------------------------- backward: d_vl, d_ql
// One workgroup per sample, lane <-> feature d.  dT[n][d], n < n_b, is accumulated in an LDS column private to the lane:
//   dT[i] += sum_j keep U[i,j],  dT[j] -= sum_i keep U[i,j],  U[i,j,d] = sum_g dS[i,g] w[g,j,d]   (i, j < n_b).
template <int G, int MODE>
__global__ void oda_len_bwd_data_kernel(const float* __restrict__ vl, const float* __restrict__ ql,
                                        const float* __restrict__ w, const float* __restrict__ dS,
                                        const int32_t* __restrict__ lens, float* __restrict__ d_vl,
                                        float* __restrict__ d_ql, DropCfg dc, int N, int L, int gate) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dT_s = reinterpret_cast<float*>(smem);        // [N][blockDim]
  float* dS_s = dT_s + (size_t)N * blockDim.x;          // [N + kLenIC][G], zero from row n_b on
  const int tid = threadIdx.x, nt = blockDim.x;
  const int b = blockIdx.x;
  const int nb = len_of(lens, b, N);
  const LenMask m = len_mask(dc, N);
  const float* vlb = vl + (size_t)b * N * L;
  for (int t = tid; t < (N + kLenIC) * G; t += nt) dS_s[t] = t < nb * G ? dS[(size_t)b * N * G + t] : 0.f;
  __syncthreads();
  for (int d = tid; d < L; d += nt) {
    for (int n = 0; n < nb; ++n) dT_s[n * nt + tid] = 0.f;
    for (int i0 = 0; i0 < nb; i0 += kLenIC) {
      const int nq = (min(kLenIC, nb - i0) + 3) >> 2;
      float ds[kLenIC][G], dTi[kLenIC];
#pragma unroll
      for (int ic = 0; ic < kLenIC; ++ic) {
        dTi[ic] = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) ds[ic][g] = dS_s[(i0 + ic) * G + g];      // (zero rows behind n_b)
      }
      for (int j = 0; j < nb; ++j) {
        float wv[G];
#pragma unroll
        for (int g = 0; g < G; ++g) wv[g] = w[((size_t)g * N + j) * L + d];
        float pj = 0.f;
#pragma unroll
        for (int q = 0; q < kLenIC / 4; ++q) {
          if (q < nq) {
            const uint32_t word = len_word<MODE>(m, b, (i0 >> 2) + q, j, d, N, L);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int ic = q * 4 + k;
              float u = 0.f;
#pragma unroll
              for (int g = 0; g < G; ++g) u = fmaf(ds[ic][g], wv[g], u);
              if (MODE != kLenPlain) u *= len_keep<MODE>(m, word, k);
              dTi[ic] += u;
              pj += u;
            }
          }
        }
        dT_s[j * nt + tid] -= pj;
      }
#pragma unroll
      for (int ic = 0; ic < kLenIC; ++ic)
        if (i0 + ic < nb) dT_s[(i0 + ic) * nt + tid] += dTi[ic];
    }
    const float qd = ql[(size_t)b * L + d];
    float dq = 0.f;
    for (int n = 0; n < nb; ++n) {
      const float t = dT_s[n * nt + tid];
      const float vn = vlb[(size_t)n * L + d];
      d_vl[((size_t)b * N + n) * L + d] = (gate != 0 && !(vn > 0.f)) ? 0.f : t * qd;   // gate: relu gradient of vl's producer
      dq = fmaf(t, vn, dq);
    }
    for (int n = nb; n < N; ++n) d_vl[((size_t)b * N + n) * L + d] = 0.f;
    d_ql[(size_t)b * L + d] = dq;
  }
}

// --------------------------------------------------------------------------------- backward: d_w slabs
// grid (ceil(N/kLenIC) j-chunks, SG sample groups); lane <-> d (blockDim >= L); dw[jc][g] of the chunk lives in registers
// across the group's samples, taken in ascending b:  dw[g,j,d] += sum_{i < n_b} dS[b,i,g] keep(b,i,j,d) (T_i[d] - T_j[d])
// for j < n_b.  A sample whose n_b lies at or below the chunk's first region is skipped whole.
template <int G, int MODE>
__global__ void oda_len_bwd_weight_kernel(const float* __restrict__ vl, const float* __restrict__ ql,
                                          const float* __restrict__ dS, const int32_t* __restrict__ lens,
                                          float* __restrict__ slab, DropCfg dc, int B, int N, int L,
                                          int samples_per_group) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dS_s = reinterpret_cast<float*>(smem);  // [N + 3][G] (zero from row n_b to the end of its quad)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int j0 = blockIdx.x * kLenIC, sg = blockIdx.y;
  const LenMask m = len_mask(dc, N);
  const int b_lo = sg * samples_per_group, b_hi = min(B, b_lo + samples_per_group);
  const int d = tid;
  const bool active = d < L;
  float dw[kLenIC][G];
#pragma unroll
  for (int jc = 0; jc < kLenIC; ++jc)
#pragma unroll
    for (int g = 0; g < G; ++g) dw[jc][g] = 0.f;
  for (int b = b_lo; b < b_hi; ++b) {
    const int nb = len_of(lens, b, N);
    if (j0 >= nb) continue;                              // (workgroup-uniform: every lane skips the barriers below together)
    const int nqb = (nb + 3) >> 2;
    __syncthreads();
    for (int t = tid; t < nqb * 4 * G; t += nt) dS_s[t] = (t < nb * G) ? dS[(size_t)b * N * G + t] : 0.f;
    __syncthreads();
    if (!active) continue;
    const float* vlb = vl + (size_t)b * N * L;
    const float qd = ql[(size_t)b * L + d];
    float Tj[kLenIC];
#pragma unroll
    for (int jc = 0; jc < kLenIC; ++jc) Tj[jc] = (j0 + jc < nb) ? len_T(vlb[(size_t)(j0 + jc) * L + d], qd) : 0.f;
    for (int iq = 0; iq < nqb; ++iq) {
      float Ti[4], ds[4][G];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = iq * 4 + k;
        Ti[k] = (i < nb) ? len_T(vlb[(size_t)i * L + d], qd) : 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) ds[k][g] = dS_s[i * G + g];  // zero rows behind n_b
      }
#pragma unroll
      for (int jc = 0; jc < kLenIC; ++jc) {
        if (j0 + jc < nb) {                              // (uniform) a slot behind n_b receives nothing from this sample
          const uint32_t word = len_word<MODE>(m, b, iq, j0 + jc, d, N, L);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float val = Ti[k] - Tj[jc];
            if (MODE != kLenPlain) val *= len_keep<MODE>(m, word, k);
#pragma unroll
            for (int g = 0; g < G; ++g) dw[jc][g] = fmaf(ds[k][g], val, dw[jc][g]);
          }
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int jc = 0; jc < kLenIC; ++jc)
    if (j0 + jc < N)
#pragma unroll
      for (int g = 0; g < G; ++g) slab[(((size_t)sg * G + g) * N + j0 + jc) * L + d] = dw[jc][g];
}

// d_w[e] = sum_sg slab[sg][e], e over G*N*L: 256 lanes = 64 elements x 4 quarters of the slab list, eight loads in flight per
// lane, the quarters added in order through LDS (the unmasked oda_reduce_kernel, restated)
__global__ __launch_bounds__(256) void oda_len_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                             size_t n, int S) {
  __shared__ float part[3][64];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const size_t e = (size_t)blockIdx.x * 64 + c;
  const size_t ec = e < n ? e : n - 1;
  const int per = (S + 3) / 4, s_lo = q * per, s_hi = min(S, s_lo + per);
  float a = 0.f;
  for (int s0 = s_lo; s0 < s_hi; s0 += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = slab[(size_t)min(s0 + k, S - 1) * n + ec];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (s0 + k < s_hi) a += v[k];
  }
  if (q > 0) part[q - 1][c] = a;
  __syncthreads();
  if (q == 0 && e < n) out[e] = ((a + part[0][c]) + part[1][c]) + part[2][c];
}

// d_bias[g] = sum_b sum_{i < n_b} dS[b,i,g]; one workgroup of 1024 lanes, fixed order: a lane takes every 1024th row of [B*N] in
// ascending order and skips the padded ones (never loaded: such a slot reads region 0 of its sample and drops it).  Eight rows (8*G independent loads) in flight as in the unmasked
// kernel -- the tensor is tiny and the kernel a chain of load latencies; the counts a row's load depends on are fetched one
// round ahead, so a round still costs one latency and not two.
template <int G>
__global__ __launch_bounds__(1024) void oda_len_dbias_kernel(const float* __restrict__ dS, const int32_t* __restrict__ lens,
                                                             float* __restrict__ d_bias, int rows, int N) {
  __shared__ float part[16][G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0.f;
  // (row index, or -1 behind the end; region of the row; row of its sample's region 0; count of its sample)
  auto counts_of = [&](int r0, int (&row)[8], int (&reg)[8], int (&first)[8], int (&cnt)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = r0 + 1024 * k;
      const int rc = min(r, rows - 1);
      const int b = rc / N;
      row[k] = r < rows ? rc : -1;
      reg[k] = rc - b * N;
      first[k] = b * N;
      cnt[k] = len_of(lens, b, N);
    }
  };
  int row[8], reg[8], first[8], cnt[8];
  counts_of(tid, row, reg, first, cnt);
  for (int r0 = tid; r0 < rows; r0 += 8 * 1024) {
    float v[8][G];
    bool real[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      real[k] = row[k] >= 0 && reg[k] < cnt[k];
      // (unconditional loads -- a guarded load is a branch and a wait of its own: 20 us against 5 --; a padded row reads its
      //  sample's region 0 instead, which is always real, and the value is dropped)
      const int rs = real[k] ? row[k] : first[k];
#pragma unroll
      for (int g = 0; g < G; ++g) v[k][g] = dS[(size_t)rs * G + g];
    }
    int row_n[8], reg_n[8], first_n[8], cnt_n[8];
    counts_of(r0 + 8 * 1024, row_n, reg_n, first_n, cnt_n);      // (behind the end: clamped reads nobody uses)
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (real[k]) {
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] += v[k][g];
      }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      row[k] = row_n[k];
      reg[k] = reg_n[k];
      first[k] = first_n[k];
      cnt[k] = cnt_n[k];
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float a = wave_sum(acc[g]);
    if (lane == 0) part[wave][g] = a;
  }
  __syncthreads();
  if (tid < G) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += part[w][tid];
    d_bias[tid] = t;
  }
}

// ======================================================================================================================
// The default kernels of the unmasked path, stopped at n_b: the 4x4-MFMA forward and weight gradient (G <= 4, N <= 36, p = 0 or
// the one-bit mask) and the one-bit data gradients.  Same operands, same order of accumulation: with lens[b] = N they return
// the unmasked entry points' bits.  What object_difference.hip says about their layouts and schedules holds here; the comments
// below say what differs.

typedef float len_f32x2 __attribute__((ext_vector_type(2)));
typedef float len_f32x4 __attribute__((ext_vector_type(4)));
constexpr int kLenIG = 9;    // region groups of 4 (N <= 36)
constexpr int kLenTS = 40;   // floats per row of the staged tiles (36 regions + 4: rows stay 16-byte aligned)

// v & (bit K of bits ? ~0 : 0): v_bfe_i32 + v_and_b32 (keep_bit of object_difference.hip: in C the compiler makes it a select)
template <int K>
__device__ __forceinline__ float len_keep_bit(float v, uint32_t bits) {
  uint32_t m;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(bits), "n"(K));
  return __uint_as_float(__float_as_uint(v) & m);
}
// the same with the bit index in a scalar register (wave-uniform)
__device__ __forceinline__ float len_keep_bit_at(float v, uint32_t bits, int off) {
  uint32_t m;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(bits), "s"(off));
  return __uint_as_float(__float_as_uint(v) & m);
}
template <int... Is, class F>
__device__ __forceinline__ void len_static_for_impl(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void len_static_for(F&& f) {
  len_static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f));
}
template <int CTRL>
__device__ __forceinline__ uint32_t len_dpp_u32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
// f(integral_constant<int, n>) for the run-time n in 1 .. kLenIG (wave-uniform): one copy of the loop per group count
template <class F>
__device__ __forceinline__ void len_groups_switch(int n, F&& f) {
  using std::integral_constant;
  switch (n) {
    case 1: f(integral_constant<int, 1>{}); break;
    case 2: f(integral_constant<int, 2>{}); break;
    case 3: f(integral_constant<int, 3>{}); break;
    case 4: f(integral_constant<int, 4>{}); break;
    case 5: f(integral_constant<int, 5>{}); break;
    case 6: f(integral_constant<int, 6>{}); break;
    case 7: f(integral_constant<int, 7>{}); break;
    case 8: f(integral_constant<int, 8>{}); break;
    default: f(integral_constant<int, kLenIG>{}); break;
  }
}

// ---- forward on the 4x4 matrix instruction: oda_fwd_mfma_kernel<true, true> / <false> stopped at n_b ------------------------------
// block k <-> feature d = 16 ds + k, row r <-> region i = 4 ig + r, column r <-> glimpse.  The regions j run to n_b in groups of
// four (a j >= n_b of the last group multiplies a zero filter value); the lane keeps T_i of ceil(n_b / 4) region groups and only
// those are multiplied: the loop is compiled once per group count and the workgroup picks its copy.  Row indices are clamped
// to n_b - 1, not N - 1.  Workgroup = one sample, its waves share the feature sets.
template <bool MASK>
__global__ __launch_bounds__(512) void oda_len_fwd_mfma_kernel(const float* __restrict__ vl, const float* __restrict__ ql,
                                                               const float* __restrict__ w, const float* __restrict__ bias,
                                                               const int32_t* __restrict__ lens, float* __restrict__ logits,
                                                               DropCfg dc, int N, int L, int G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red_s = reinterpret_cast<float*>(smem);      // [nwaves][4 kLenIG][4]
  const int tid = threadIdx.x, lane = tid & 63, nwaves = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = lane >> 2, r = lane & 3;
  const int b = blockIdx.x;
  const int nb = __builtin_amdgcn_readfirstlane(len_of(lens, b, N));
  const int NI = (N + 31) >> 5;
  const uint32_t key = MASK ? drop_key(dc) : 0u;
  const uint32_t stride = (uint32_t)N * (uint32_t)L;
  const float* vlb = vl + (size_t)b * N * L;
  const rt::rsrc_t Vb = rt::make_rsrc(vlb, (size_t)nb * L * 4);      // (the sample's real rows: a read behind them returns 0)
  const rt::rsrc_t Wb = rt::make_rsrc(w, (size_t)G * N * L * 4);
  const int nsets = (L + 15) >> 4;
  struct SetRegs {
    float ti[kLenIG], tj[4], wv[4], qd;
  };
  auto set_offsets = [&](int ds, uint32_t& vo, uint32_t& wo, int& dcl, bool& dok) {
    const int d = 16 * min(ds, nsets - 1) + k;
    dok = d < L && ds < nsets;
    dcl = d < L ? d : 0;
    vo = (uint32_t)dcl * 4u;
    wo = ((uint32_t)min(r, G - 1) * stride + (uint32_t)dcl) * 4u;
  };
  auto load_group = [&](float (&t)[4], float (&wg)[4], uint32_t vo, uint32_t wo, int j0) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const uint32_t so = (uint32_t)min(j0 + jj, nb - 1) * (uint32_t)L * 4u;
      t[jj] = rt::ldg4(Vb, vo, so);
      wg[jj] = rt::ldg4(Wb, wo, so);
    }
  };
  len_groups_switch((nb + 3) >> 2, [&](auto nig_) {
    constexpr int NIG = decltype(nig_)::value;
    len_f32x4 acc[NIG];
#pragma unroll
    for (int ig = 0; ig < NIG; ++ig) acc[ig] = len_f32x4{0.f, 0.f, 0.f, 0.f};
    auto load_set = [&](SetRegs& sr, int ds) {
      uint32_t vo, wo;
      int dcl;
      bool dok;
      set_offsets(ds, vo, wo, dcl, dok);
      sr.qd = ql[(size_t)b * L + dcl];
#pragma unroll
      for (int ig = 0; ig < NIG; ++ig) sr.ti[ig] = rt::ldg4(Vb, vo + (uint32_t)min(4 * ig + r, nb - 1) * (uint32_t)L * 4u, 0u);
      load_group(sr.tj, sr.wv, vo, wo, 0);
    };
    SetRegs nx;
    if (wave < nsets) load_set(nx, wave);
    for (int ds = wave; ds < nsets; ds += nwaves) {
      uint32_t vo, wo;
      int dcl;
      bool dok;
      set_offsets(ds, vo, wo, dcl, dok);
      const float qd = dok ? nx.qd : 0.f;
      float Ti[NIG], tj[4], wv[4];
#pragma unroll
      for (int ig = 0; ig < NIG; ++ig) Ti[ig] = 4 * ig + r < nb ? nx.ti[ig] * qd : 0.f;      // (qd = 0 beyond L)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        tj[jj] = nx.tj[jj];
        wv[jj] = nx.wv[jj];
      }
      load_set(nx, ds + nwaves);                               // (past the last set: a clamped reload nobody uses)
      const bool gok = dok && r < G;
      const uint32_t cnt_d = (uint32_t)b * (uint32_t)NI * stride + (uint32_t)dcl;   // + j L (+ stride for the second word)
      for (int j0 = 0; j0 < nb; j0 += 4) {
        float tn[4], wn[4];
        load_group(tn, wn, vo, wo, min(j0 + 4, nb - 1));
        uint32_t hw0 = 0u, hw1 = 0u;
        if constexpr (MASK) {
          const uint32_t cnt = cnt_d + (uint32_t)min(j0 + r, N - 1) * (uint32_t)L;    // (a counter, not an address: built from N)
          hw0 = mask_word32(cnt, key);
          if (NI > 1) hw1 = mask_word32(cnt + stride, key);
        }
        len_static_for<4>([&](auto jj_) {
          constexpr int jj = decltype(jj_)::value;
          constexpr int kCtrl = jj * 0x55;                     // quad_perm [jj, jj, jj, jj]
          const uint32_t b0 = len_dpp_u32<kCtrl>(hw0) >> r, b1 = len_dpp_u32<kCtrl>(hw1) >> r;   // bit 4 ig <-> region 4 ig + r
          const float Tj = tj[jj] * qd;
          const float wg = (gok && j0 + jj < nb) ? wv[jj] : 0.f;                              // (a region beyond n_b adds nothing)
          // the differences as the unmasked default forms write them, so that the compiler contracts (or not) alike: packed
          // pairs under the mask (oda_fwd_mfma_kernel<true, true>), one subtraction each without (oda_fwd_mfma_kernel<false>)
          float x[NIG];
          if constexpr (MASK) {
            const len_f32x2 tj2 = len_f32x2{Tj, Tj};
#pragma unroll
            for (int h = 0; h < NIG / 2; ++h) {
              const len_f32x2 d2 = len_f32x2{Ti[2 * h], Ti[2 * h + 1]} - tj2;
              x[2 * h] = d2[0];
              x[2 * h + 1] = d2[1];
            }
            if constexpr (NIG & 1) x[NIG - 1] = Ti[NIG - 1] - Tj;
          } else {
#pragma unroll
            for (int ig = 0; ig < NIG; ++ig) x[ig] = Ti[ig] - Tj;
          }
          len_static_for<NIG>([&](auto ig_) {
            constexpr int ig = decltype(ig_)::value;
            if constexpr (MASK) x[ig] = ig < 8 ? len_keep_bit<(4 * ig) & 31>(x[ig], b0) : len_keep_bit<0>(x[ig], b1);
          });
          __builtin_amdgcn_sched_group_barrier(0x002, MASK ? 3 * NIG + 6 : NIG + 2, 0);
          len_static_for<NIG>([&](auto ig_) {
            constexpr int ig = decltype(ig_)::value;
            acc[ig] = __builtin_amdgcn_mfma_f32_4x4x1f32(x[ig], wg, acc[ig], 0, 0, 0);
          });
          __builtin_amdgcn_sched_group_barrier(0x008, NIG, 0);
        });
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          tj[jj] = tn[jj];
          wv[jj] = wn[jj];
        }
      }
    }
    // the 16 blocks of the wave: blocks 0..3 of a 16-lane row by two rotations, the four rows lane-wise
#pragma unroll
    for (int ig = 0; ig < NIG; ++ig)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float v = acc[ig][t];
        v += dpp_mov<0x124>(v);      // row_ror:4
        v += dpp_mov<0x128>(v);      // row_ror:8
        v = rows_sum(v);
        if (lane < 4) red_s[(wave * 4 * kLenIG + 4 * ig + t) * 4 + lane] = v;       // region 4 ig + t, glimpse lane
      }
  });
  __syncthreads();
  for (int t = tid; t < N * G; t += blockDim.x) {
    const int i = t / G, g = t % G;
    float out = 0.f;                                          // exactly 0 on the padding
    if (i < nb) {
      float sum = 0.f;
      for (int wv_ = 0; wv_ < nwaves; ++wv_) sum += red_s[(wv_ * 4 * kLenIG + i) * 4 + g];
      out = fmaf(MASK ? dc.scale : 1.f, sum, bias[g]);        // the kept values' factor 2
    }
    logits[((size_t)b * N + i) * G + g] = out;
  }
}

// ---- weight gradient on the 4x4 matrix instruction: oda_bwd_weight_mfma_staged_kernel<MASK, 1> stopped at n_b -------------------
// block k <-> feature d, row r <-> glimpse (A = dS[b][i][r]), column r <-> region j = 4 jg + r (B = the masked difference of the
// lane's own j).  Per sample: the regions i run to n_b in passes of four (dS rows >= n_b are staged as zeros); a lane's region
// j >= n_b is silenced through its mask words -- zeroed, so that the bit picked per i is 0 -- and with p = 0 the same AND is
// handed an all-ones or all-zeros word per j; the region groups jg >= ceil(n_b / 4) are not multiplied at all (one copy of
// the region loop per group count).  Their accumulators stay 0 and the slab gets exact zeros.  Summation order: per sample,
// regions i ascending, two sample slots per group meeting in LDS -- the unmasked kernel's.
template <bool MASK>
__global__ __launch_bounds__(512) void oda_len_bwd_weight_mfma_kernel(const float* __restrict__ vl, const float* __restrict__ ql,
                                                                      const float* __restrict__ dS,
                                                                      const int32_t* __restrict__ lens, float* __restrict__ slab,
                                                                      DropCfg dc, int B, int N, int L, int G,
                                                                      int samples_per_group) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ex_s = reinterpret_cast<float*>(smem);            // [2][nwaves][4 kLenIG][64]: the odd slot's accumulators of a set
  const int tid = threadIdx.x, lane = tid & 63, nwaves = blockDim.x / 128;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = wid % nwaves, sw = (wid / nwaves) & 1;
  const int k = lane >> 2, r = lane & 3;
  float* Tw = ex_s + (size_t)2 * nwaves * (4 * kLenIG) * 64 + (size_t)wid * (20 * kLenTS);   // [16][kLenTS], wave-private
  float* Sw = Tw + 16 * kLenTS;                                                               // [4][kLenTS]
  const int sg = blockIdx.x;
  const int NI = (N + 31) >> 5;
  const uint32_t key = MASK ? drop_key(dc) : 0u;
  const uint32_t stride = (uint32_t)N * (uint32_t)L;
  const int b_lo = sg * samples_per_group, b_hi = min(B, b_lo + samples_per_group);
  const rt::rsrc_t Vb = rt::make_rsrc(vl, (size_t)B * N * L * 4);
  const rt::rsrc_t Sb = rt::make_rsrc(dS, (size_t)B * N * G * 4);
  const rt::rsrc_t Qb = rt::make_rsrc(ql, (size_t)B * L * 4);
  const rt::rsrc_t Wb = rt::make_rsrc(slab + (size_t)sg * G * N * L, (size_t)G * N * L * 4);   // this group's slab
  const int nsets = (L + 15) >> 4;
  const int nb = (b_hi - b_lo - sw + 1) / 2;                  // samples b_lo + sw, b_lo + sw + 2, ... of this slot
  const int max_sets = (nsets + nwaves - 1) / nwaves;         // every wave runs the same number of set rounds (barriers inside)
  struct Raw {
    float v[kLenIG], s[3], q;
  };
  auto fetch = [&](Raw& o, int si, int bi) {
    const int ds = wave + si * nwaves;
    const int d = 16 * ds + k;
    const uint32_t vo = (uint32_t)((ds < nsets && d < L) ? d : 0) * 4u;
    const int b = b_lo + sw + 2 * bi;
    const int nr = len_of(lens, b, N);                        // rows behind it are never read: clamped to n_b - 1
    const uint32_t row0 = (uint32_t)b * stride * 4u;
#pragma unroll
    for (int jg = 0; jg < kLenIG; ++jg) o.v[jg] = rt::ldg4(Vb, vo + (uint32_t)min(4 * jg + r, nr - 1) * (uint32_t)L * 4u, row0);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int e = lane + 64 * t, i = e >> 2, g = e & 3;
      const float a = rt::ldg4(Sb, (uint32_t)(min(i, nr - 1) * G + min(g, G - 1)) * 4u, (uint32_t)b * (uint32_t)(N * G) * 4u);
      o.s[t] = (i < nr && g < G) ? a : 0.f;
    }
    o.q = rt::ldg4(Qb, vo, (uint32_t)b * (uint32_t)L * 4u);
  };
  auto arrived = [&](Raw& o) {
#pragma unroll
    for (int jg = 0; jg < kLenIG; ++jg) asm volatile("" : "+v"(o.v[jg]));
    asm volatile("" : "+v"(o.s[0]), "+v"(o.s[1]), "+v"(o.s[2]), "+v"(o.q));
  };
  Raw cur;
  if (nb > 0 && wave < nsets) {
    fetch(cur, 0, 0);
    arrived(cur);
  }
  len_f32x4 acc[kLenIG];
  for (int si = 0; si < max_sets; ++si) {
    const int ds = wave + si * nwaves;
    const int d = 16 * ds + k;
    const bool set_ok = ds < nsets;
    const bool dok = set_ok && d < L;
    const int dcl = dok ? d : 0;
#pragma unroll
    for (int jg = 0; jg < kLenIG; ++jg) acc[jg] = len_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int bi = 0; bi < (set_ok ? nb : 0); ++bi) {
      const int b = b_lo + sw + 2 * bi;
      const int nr = __builtin_amdgcn_readfirstlane(len_of(lens, b, N));
      Raw nxt;
      {
        const bool last_b = bi + 1 >= nb;
        const int si2 = last_b ? si + 1 : si, bi2 = last_b ? 0 : bi + 1;
        if (si2 < max_sets && wave + si2 * nwaves < nsets) fetch(nxt, si2, bi2);
      }
      float Tj[kLenIG];
      uint32_t w0[kLenIG], w1[kLenIG];
#pragma unroll
      for (int jg = 0; jg < kLenIG; ++jg) {
        float t = cur.v[jg] * cur.q;
        asm("" : "+v"(t));                  // (a ROUNDED product on both sides of T_i - T_j: T_i - T_i is exactly zero)
        Tw[k * kLenTS + 4 * jg + r] = t;    // (regions beyond n_b: copies of region n_b - 1, finite, times dS = 0)
        Tj[jg] = t;
        const bool real = 4 * jg + r < nr;
        if constexpr (MASK) {
          const int j = min(4 * jg + r, N - 1);
          const uint32_t cnt = (uint32_t)b * (uint32_t)NI * stride + (uint32_t)j * (uint32_t)L + (uint32_t)dcl;
          w0[jg] = real ? mask_word32(cnt, key) : 0u;
          w1[jg] = (real && NI > 1) ? mask_word32(cnt + stride, key) : 0u;
        } else {
          w0[jg] = w1[jg] = real ? ~0u : 0u;
        }
      }
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int e = lane + 64 * t;
        if (e < 4 * 36) Sw[(e & 3) * kLenTS + (e >> 2)] = cur.s[t];      // (zeros from row n_b on, every sample anew)
      }
      // (wave-private tiles: the wave's own LDS operations complete in order, no barrier)
      len_f32x4 ta = *reinterpret_cast<const len_f32x4*>(Tw + k * kLenTS);
      len_f32x4 sa = *reinterpret_cast<const len_f32x4*>(Sw + r * kLenTS);
      __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0), once per (set, sample)
      len_groups_switch((nr + 3) >> 2, [&](auto njg_) {
        constexpr int NJ = decltype(njg_)::value;
        // four regions i0 .. i0 + 3; region i0 + ii is bit bit0 + ii of the words wv
        auto pass = [&](int i0, const uint32_t (&wv)[kLenIG], int bit0) {
          const int in = min(i0 + 4, 32);
          const len_f32x4 tn = *reinterpret_cast<const len_f32x4*>(Tw + k * kLenTS + in);
          const len_f32x4 sn = *reinterpret_cast<const len_f32x4*>(Sw + r * kLenTS + in);
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      // (the two reads FIRST)
          len_static_for<4>([&](auto ii_) {
            constexpr int ii = decltype(ii_)::value;
            const float Ti = ta[ii];
            const float av = sa[ii];          // (zero beyond n_b and G; a lane beyond L accumulates finite values nobody stores)
            float x[NJ];
            const len_f32x2 ti2 = len_f32x2{Ti, Ti};
#pragma unroll
            for (int h = 0; h < NJ / 2; ++h) {
              const len_f32x2 d2 = ti2 - len_f32x2{Tj[2 * h], Tj[2 * h + 1]};
              x[2 * h] = d2[0];
              x[2 * h + 1] = d2[1];
            }
            if constexpr (NJ & 1) x[NJ - 1] = Ti - Tj[NJ - 1];
#pragma unroll
            for (int jg = 0; jg < NJ; ++jg) x[jg] = len_keep_bit_at(x[jg], wv[jg], bit0 + ii);
            __builtin_amdgcn_sched_group_barrier(0x002, 2 * NJ + NJ / 2 + (NJ & 1), 0);
#pragma unroll
            for (int jg = 0; jg < NJ; ++jg) acc[jg] = __builtin_amdgcn_mfma_f32_4x4x1f32(av, x[jg], acc[jg], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, NJ, 0);
          });
          __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the two reads, issued a pass ago, for the compiler's bookkeeping too
          ta = tn;
          sa = sn;
        };
        const int n_lo = min(nr, 32);
        for (int i0 = 0; i0 < n_lo; i0 += 4) pass(i0, w0, i0);
        if (nr > 32) pass(32, w1, 0);
      });
      cur = nxt;
      arrived(cur);
    }
    // the two sample slots of a set meet: slot 1 hands its accumulators over, slot 0 adds and stores
    float* ex = ex_s + ((size_t)(si & 1) * nwaves + wave) * (4 * kLenIG) * 64 + lane;
    if (sw == 1) {
#pragma unroll
      for (int jg = 0; jg < kLenIG; ++jg)
#pragma unroll
        for (int t = 0; t < 4; ++t) ex[(4 * jg + t) * 64] = acc[jg][t];
    }
    __syncthreads();
    if (sw == 0 && dok) {
      const float sc = MASK ? dc.scale : 1.f;
      float e[kLenIG][4];
#pragma unroll
      for (int jg = 0; jg < kLenIG; ++jg)
#pragma unroll
        for (int t = 0; t < 4; ++t) e[jg][t] = ex[(4 * jg + t) * 64];      // (all reads in flight, then the stores)
#pragma unroll
      for (int jg = 0; jg < kLenIG; ++jg) {
        const int j = 4 * jg + r;
        if (j < N) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (t < G)
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, (acc[jg][t] + e[jg][t]) * sc), Wb,
                                                    (int)(((uint32_t)(t * N + j) * (uint32_t)L + (uint32_t)d) * 4u), 0, 0);
        }
      }
    }
    // (no second barrier: the next set hands over in the other buffer, and its barrier is behind these reads)
  }
}

// ---- data gradient, one-bit mask: oda_bwd_data_bits_kernel stopped at n_b ---------------------------------------------------
// one workgroup per sample, lane <-> feature d, chunks of kLenIC regions i against every region j < n_b
__device__ __forceinline__ uint32_t len_bits(uint32_t cnt_lo, uint32_t word_stride, int sh, bool straddle, uint32_t key) {
  uint32_t bits = mask_word32(cnt_lo, key) >> sh;
  if (straddle) bits |= mask_word32(cnt_lo + word_stride, key) << (32 - sh);   // (straddle implies sh > 0)
  return bits;
}
template <int G>
__global__ void oda_len_bwd_data_bits_kernel(const float* __restrict__ vl, const float* __restrict__ ql,
                                             const float* __restrict__ w, const float* __restrict__ dS,
                                             const int32_t* __restrict__ lens, float* __restrict__ d_vl,
                                             float* __restrict__ d_ql, DropCfg dc, int N, int L, int gate) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dT_s = reinterpret_cast<float*>(smem);        // [N][blockDim]
  float* dS_s = dT_s + (size_t)N * blockDim.x;          // [N + kLenIC][G]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int b = blockIdx.x;
  const int nb = len_of(lens, b, N);
  const int NI = (N + 31) >> 5;
  const uint32_t key = drop_key(dc);
  const uint32_t stride = (uint32_t)N * (uint32_t)L;
  const float* vlb = vl + (size_t)b * N * L;
  for (int t = tid; t < (N + kLenIC) * G; t += nt) dS_s[t] = t < nb * G ? dS[(size_t)b * N * G + t] : 0.f;   // (zero from row n_b on)
  __syncthreads();
  for (int d = tid; d < L; d += nt) {
    for (int n = 0; n < nb; ++n) dT_s[n * nt + tid] = 0.f;
    for (int i0 = 0; i0 < nb; i0 += kLenIC) {
      const int sh = i0 & 31;
      const bool straddle = ((min(i0 + kLenIC, N) - 1) >> 5) != (i0 >> 5);
      const uint32_t base = ((uint32_t)b * NI + (uint32_t)(i0 >> 5)) * stride;
      len_f32x2 ds[kLenIC / 2][G], dTi[kLenIC / 2];
#pragma unroll
      for (int ip = 0; ip < kLenIC / 2; ++ip) {
        dTi[ip] = len_f32x2{0.f, 0.f};
#pragma unroll
        for (int g = 0; g < G; ++g) ds[ip][g] = len_f32x2{dS_s[(i0 + 2 * ip) * G + g], dS_s[(i0 + 2 * ip + 1) * G + g]};
      }
      auto load_w = [&](float (&wr)[G], int j) {
        const int jc = min(j, nb - 1);
#pragma unroll
        for (int g = 0; g < G; ++g) wr[g] = w[((size_t)g * N + jc) * L + d];
      };
      auto one_j = [&](int j, const float (&wv)[G]) {
        const float dtj = dT_s[j * nt + tid];
        const uint32_t bits = len_bits(base + (uint32_t)(j * L + d), stride, sh, straddle, key);
        len_f32x2 u[kLenIC / 2];
#pragma unroll
        for (int ip = 0; ip < kLenIC / 2; ++ip) u[ip] = ds[ip][0] * len_f32x2{wv[0], wv[0]};
#pragma unroll
        for (int g = 1; g < G; ++g)
#pragma unroll
          for (int ip = 0; ip < kLenIC / 2; ++ip) u[ip] = __builtin_elementwise_fma(ds[ip][g], len_f32x2{wv[g], wv[g]}, u[ip]);
        len_f32x2 pj = len_f32x2{0.f, 0.f};
        len_static_for<kLenIC / 2>([&](auto ip_) {
          constexpr int ip = decltype(ip_)::value;
          const len_f32x2 m = len_f32x2{len_keep_bit<2 * ip>(u[ip].x, bits), len_keep_bit<2 * ip + 1>(u[ip].y, bits)};
          dTi[ip] += m;
          pj += m;
        });
        dT_s[j * nt + tid] = dtj - (pj.x + pj.y);
      };
      float wa[G], wb[G], wc[G];
      load_w(wa, 0);
      load_w(wb, 1);
      load_w(wc, 2);
      for (int j = 0; j < nb; j += 3) {
        one_j(j, wa);
        load_w(wa, j + 3);
        if (j + 1 < nb) one_j(j + 1, wb);
        load_w(wb, j + 4);
        if (j + 2 < nb) one_j(j + 2, wc);
        load_w(wc, j + 5);
      }
#pragma unroll
      for (int ip = 0; ip < kLenIC / 2; ++ip) {
        if (i0 + 2 * ip < nb) dT_s[(i0 + 2 * ip) * nt + tid] += dTi[ip].x;
        if (i0 + 2 * ip + 1 < nb) dT_s[(i0 + 2 * ip + 1) * nt + tid] += dTi[ip].y;
      }
    }
    const float qd = ql[(size_t)b * L + d] * dc.scale;      // (the kept values' factor 2 rides on q here)
    float dq = 0.f;
    for (int n = 0; n < nb; ++n) {
      const float t = dT_s[n * nt + tid];
      const float vn = vlb[(size_t)n * L + d];
      d_vl[((size_t)b * N + n) * L + d] = (gate != 0 && !(vn > 0.f)) ? 0.f : t * qd;   // gate: relu gradient of vl's producer
      dq = fmaf(t, vn, dq);
    }
    for (int n = nb; n < N; ++n) d_vl[((size_t)b * N + n) * L + d] = 0.f;
    d_ql[(size_t)b * L + d] = dq * dc.scale;
  }
}

// The same with the region chunks of a sample spread over the waves of a workgroup (oda_bwd_data_bits_split_kernel stopped at
// n_b): grid (ceil(L/64), B), wave c = chunk i0 = c kLenIC of the regions i, lane = feature d of the block.  A wave whose chunk
// starts at or behind n_b has no region loop and no plane; every wave still takes its share of the N output rows (zeros from
// row n_b on).
template <int G>
__global__ void oda_len_bwd_data_bits_split_kernel(const float* __restrict__ vl, const float* __restrict__ ql,
                                                   const float* __restrict__ w, const float* __restrict__ dS,
                                                   const int32_t* __restrict__ lens, float* __restrict__ d_vl,
                                                   float* __restrict__ d_ql, DropCfg dc, int N, int L, int gate) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NC = blockDim.x >> 6;                       // chunk waves = ceil(N / kLenIC)
  float* dT_s = reinterpret_cast<float*>(smem);         // [NC][N][64]
  float* dq_s = dT_s + (size_t)NC * N * 64;             // [NC][64]
  float* dS_s = dq_s + NC * 64;                         // [N + kLenIC][G]
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y;
  const int nb = __builtin_amdgcn_readfirstlane(len_of(lens, b, N));
  const int ncb = (nb + kLenIC - 1) / kLenIC;           // the waves with a chunk of real regions
  const int d_raw = blockIdx.x * 64 + lane;
  const bool active = d_raw < L;
  const int d = active ? d_raw : L - 1;
  const int NI = (N + 31) >> 5;
  const uint32_t key = drop_key(dc);
  const uint32_t stride = (uint32_t)N * (uint32_t)L;
  const float* vlb = vl + (size_t)b * N * L;
  for (int t = tid; t < (N + kLenIC) * G; t += blockDim.x) dS_s[t] = t < nb * G ? dS[(size_t)b * N * G + t] : 0.f;
  __syncthreads();
  float* mine = dT_s + (size_t)c * N * 64 + lane;       // this wave's plane: row n at mine[n * 64]
  float vn_pre[kLenIC], ql_pre;      // vl of the output rows this wave finishes with (n = c, c + NC, ...) and ql
  if (c < ncb) {
    const int i0 = c * kLenIC;
    const int sh = i0 & 31;
    const bool straddle = ((min(i0 + kLenIC, N) - 1) >> 5) != (i0 >> 5);
    const uint32_t base = ((uint32_t)b * NI + (uint32_t)(i0 >> 5)) * stride;
    len_f32x2 ds[kLenIC / 2][G], dTi[kLenIC / 2];
#pragma unroll
    for (int ip = 0; ip < kLenIC / 2; ++ip) {
      dTi[ip] = len_f32x2{0.f, 0.f};
#pragma unroll
      for (int g = 0; g < G; ++g) ds[ip][g] = len_f32x2{dS_s[(i0 + 2 * ip) * G + g], dS_s[(i0 + 2 * ip + 1) * G + g]};
    }
    auto load_w = [&](float (&wr)[G], int j) {
      const int jc = min(j, nb - 1);
#pragma unroll
      for (int g = 0; g < G; ++g) wr[g] = w[((size_t)g * N + jc) * L + d];
    };
    auto one_j = [&](int j, const float (&wv)[G]) {
      const uint32_t bits = len_bits(base + (uint32_t)(j * L + d), stride, sh, straddle, key);
      len_f32x2 u[kLenIC / 2];
#pragma unroll
      for (int ip = 0; ip < kLenIC / 2; ++ip) u[ip] = ds[ip][0] * len_f32x2{wv[0], wv[0]};
#pragma unroll
      for (int g = 1; g < G; ++g)
#pragma unroll
        for (int ip = 0; ip < kLenIC / 2; ++ip) u[ip] = __builtin_elementwise_fma(ds[ip][g], len_f32x2{wv[g], wv[g]}, u[ip]);
      len_f32x2 pj = len_f32x2{0.f, 0.f};
      len_static_for<kLenIC / 2>([&](auto ip_) {
        constexpr int ip = decltype(ip_)::value;
        const len_f32x2 m = len_f32x2{len_keep_bit<2 * ip>(u[ip].x, bits), len_keep_bit<2 * ip + 1>(u[ip].y, bits)};
        dTi[ip] += m;
        pj += m;
      });
      mine[j * 64] = -(pj.x + pj.y);
    };
    float wa[G], wb[G], wc[G];
    load_w(wa, 0);
    load_w(wb, 1);
    load_w(wc, 2);
#pragma unroll
    for (int q = 0; q < kLenIC; ++q) vn_pre[q] = vlb[(size_t)min(c + q * NC, nb - 1) * L + d];
    ql_pre = ql[(size_t)b * L + d];
    auto arrived = [&](float (&wr)[G]) {
#pragma unroll
      for (int g = 0; g < G; ++g) asm volatile("" : "+v"(wr[g]));
    };
    arrived(wa);
    for (int j = 0; j < nb; j += 3) {
      one_j(j, wa);
      load_w(wa, j + 3);
      if (j + 1 < nb) one_j(j + 1, wb);
      load_w(wb, j + 4);
      if (j + 2 < nb) one_j(j + 2, wc);
      load_w(wc, j + 5);
      arrived(wa);
    }
#pragma unroll
    for (int ip = 0; ip < kLenIC / 2; ++ip) {      // (the wave's own column of its own plane: written above, by this lane)
      if (i0 + 2 * ip < nb) mine[(i0 + 2 * ip) * 64] += dTi[ip].x;
      if (i0 + 2 * ip + 1 < nb) mine[(i0 + 2 * ip + 1) * 64] += dTi[ip].y;
    }
  } else {
#pragma unroll
    for (int q = 0; q < kLenIC; ++q) vn_pre[q] = vlb[(size_t)min(c + q * NC, nb - 1) * L + d];
    ql_pre = ql[(size_t)b * L + d];
  }
  __syncthreads();
  const float qd = ql_pre * dc.scale;                     // (the kept values' factor 2 rides on q here)
  float dq = 0.f;
#pragma unroll
  for (int qn = 0; qn < kLenIC; ++qn) {                   // the output rows, dealt over the waves
    const int n = c + qn * NC;
    if (n < nb) {
      float t = 0.f;
      for (int q = 0; q < ncb; ++q) t += dT_s[((size_t)q * N + n) * 64 + lane];    // fixed order, the planes that exist
      const float vn = vn_pre[qn];
      if (active) d_vl[((size_t)b * N + n) * L + d] = (gate != 0 && !(vn > 0.f)) ? 0.f : t * qd;
      dq = fmaf(t, vn, dq);
    } else if (n < N) {
      if (active) d_vl[((size_t)b * N + n) * L + d] = 0.f;
    }
  }
  dq_s[c * 64 + lane] = dq;
  __syncthreads();
  if (c == 0 && active) {
    float s = 0.f;
    for (int q = 0; q < NC; ++q) s += dq_s[q * 64 + lane];
    d_ql[(size_t)b * L + d] = s * dc.scale;
  }
}

// ---- dispatch --------------------------------------------------------------------------------------------------------------
// oda_bits_mode of object_difference.hip, restated: p = 0.5 and 32-bit element counters -> the one-bit-per-element layout
// (VQA_K2_BYTE_MASK set keeps the byte layout)
static int len_mask_mode(const DropCfg& dc, int B, int N, int L) {
  if (dc.p8 == 0) return kLenPlain;
  const bool bits = dc.p8 == kDropHalf && (size_t)B * ((N + 31) / 32) * N * L < (1ull << 32) && vqa::option("VQA_K2_BYTE_MASK") == nullptr;
  return bits ? kLenBit : kLenByte;
}
// oda_mfma_ok, restated: G <= 4 glimpses, N <= 36 regions, no dropout or the one-bit mask (VQA_K2_MFMA=0: the VALU family)
static bool len_mfma_ok(int mode, int B, int N, int L, int G) {
  const bool off = vqa::option_is("VQA_K2_MFMA", '0');
  return !off && G <= 4 && N <= 4 * kLenIG && mode != kLenByte && (size_t)B * N * L * 4 < (1ull << 32);
}
static int len_threads(int L) {
  int t = (L < 1024 ? L : 1024);
  return (t + 63) / 64 * 64;
}
static int len_groups(int B) { return B < 128 ? B : 128; }
static int len_mfma_groups(int B) { return B < 256 ? B : 256; }   // sample groups of the MFMA weight gradient

template <int G>
static int launch_len_fwd(const float* vl, const float* ql, const float* w, const float* bias, const int32_t* lens,
                          float* logits, DropCfg dc, int B, int N, int L, hipStream_t s) {
  const int nt = len_threads(L);
  const int mode = len_mask_mode(dc, B, N, L);
  if (len_mfma_ok(mode, B, N, L, G)) {
    const int nsets = (L + 15) / 16;
    const int nw = nsets < 8 ? (nsets < 4 ? nsets : 4) : 8;       // waves per sample: the unmasked forward's choice
    const size_t lds_m = (size_t)nw * 4 * kLenIG * 4 * sizeof(float);
    if (mode == kLenBit)
      VQA_LAUNCH(oda_len_fwd_mfma_kernel<true>, dim3(B), dim3(64 * nw), lds_m, s, vl, ql, w, bias, lens, logits, dc, N, L, G);
    else
      VQA_LAUNCH(oda_len_fwd_mfma_kernel<false>, dim3(B), dim3(64 * nw), lds_m, s, vl, ql, w, bias, lens, logits, dc, N, L, G);
    return check_launch("object_difference_attention_len_fwd");
  }
  const size_t lds = (size_t)(nt / 64) * kLenIC * G * sizeof(float);
  const dim3 grid((N + kLenIC - 1) / kLenIC, B);
  if (mode == kLenBit)
    VQA_LAUNCH((oda_len_fwd_kernel<G, kLenBit>), grid, dim3(nt), lds, s, vl, ql, w, bias, lens, logits, dc, N, L);
  else if (mode == kLenByte)
    VQA_LAUNCH((oda_len_fwd_kernel<G, kLenByte>), grid, dim3(nt), lds, s, vl, ql, w, bias, lens, logits, dc, N, L);
  else
    VQA_LAUNCH((oda_len_fwd_kernel<G, kLenPlain>), grid, dim3(nt), lds, s, vl, ql, w, bias, lens, logits, dc, N, L);
  return check_launch("object_difference_attention_len_fwd");
}

template <int G>
static int launch_len_bwd(const float* vl, const float* ql, const float* w, const float* dS, const int32_t* lens, float* d_vl,
                          float* d_ql, float* d_w, float* d_bias, float* slab, DropCfg dc, int B, int N, int L, int gate_dvl,
                          hipStream_t s) {
  const int nt = len_threads(L);
  const int mode = len_mask_mode(dc, B, N, L);
  {
    // the data gradient: the unmasked path's present choice among its three default forms (VQA_K2_DATA_SPLIT is not read)
    const size_t lds = ((size_t)N * nt + (size_t)(N + kLenIC) * G) * sizeof(float);     // (the unmasked backward's limit)
    VQA_REQUIRE(lds <= 160 * 1024, VQA_E_UNSUPPORTED, "object_difference_attention_len_bwd: N=%d L=%d need %zu B of LDS", N, L, lds);
    const int nc = (N + kLenIC - 1) / kLenIC;
    if (mode == kLenBit && nc <= 4 && (long)B * ((L + 63) / 64) >= 512) {
      const size_t lds_s = ((size_t)nc * N * 64 + (size_t)nc * 64 + (size_t)(N + kLenIC) * G) * sizeof(float);
      VQA_ENSURE_LDS((oda_len_bwd_data_bits_split_kernel<G>), lds_s);
      VQA_LAUNCH((oda_len_bwd_data_bits_split_kernel<G>), dim3((L + 63) / 64, B), dim3(64 * nc), lds_s, s, vl, ql, w, dS, lens,
                 d_vl, d_ql, dc, N, L, gate_dvl);
    } else if (mode == kLenBit) {
      VQA_ENSURE_LDS((oda_len_bwd_data_bits_kernel<G>), lds);
      VQA_LAUNCH((oda_len_bwd_data_bits_kernel<G>), dim3(B), dim3(nt), lds, s, vl, ql, w, dS, lens, d_vl, d_ql, dc, N, L, gate_dvl);
    } else if (mode == kLenByte) {
      VQA_ENSURE_LDS((oda_len_bwd_data_kernel<G, kLenByte>), lds);
      VQA_LAUNCH((oda_len_bwd_data_kernel<G, kLenByte>), dim3(B), dim3(nt), lds, s, vl, ql, w, dS, lens, d_vl, d_ql, dc, N, L, gate_dvl);
    } else {
      VQA_ENSURE_LDS((oda_len_bwd_data_kernel<G, kLenPlain>), lds);
      VQA_LAUNCH((oda_len_bwd_data_kernel<G, kLenPlain>), dim3(B), dim3(nt), lds, s, vl, ql, w, dS, lens, d_vl, d_ql, dc, N, L, gate_dvl);
    }
  }
  {
    int SG = len_groups(B);
    int spg = (B + SG - 1) / SG;
    if (len_mfma_ok(mode, B, N, L, G)) {
      SG = len_mfma_groups(B);
      spg = (B + SG - 1) / SG;
      SG = (B + spg - 1) / spg;
      const int nsets = (L + 15) / 16, nw = nsets < 4 ? nsets : 4;
      const size_t lds_st = (size_t)2 * nw * 4 * kLenIG * 64 * sizeof(float) + (size_t)2 * nw * 20 * kLenTS * sizeof(float);
      if (mode == kLenBit) {
        VQA_ENSURE_LDS(oda_len_bwd_weight_mfma_kernel<true>, lds_st);
        VQA_LAUNCH(oda_len_bwd_weight_mfma_kernel<true>, dim3(SG), dim3(128 * nw), lds_st, s, vl, ql, dS, lens, slab, dc, B, N, L, G, spg);
      } else {
        VQA_ENSURE_LDS(oda_len_bwd_weight_mfma_kernel<false>, lds_st);
        VQA_LAUNCH(oda_len_bwd_weight_mfma_kernel<false>, dim3(SG), dim3(128 * nw), lds_st, s, vl, ql, dS, lens, slab, dc, B, N, L, G, spg);
      }
    } else {
      const size_t lds = (size_t)(N + 3) * G * sizeof(float);
      const dim3 grid((N + kLenIC - 1) / kLenIC, SG);
      if (mode == kLenBit)
        VQA_LAUNCH((oda_len_bwd_weight_kernel<G, kLenBit>), grid, dim3(nt), lds, s, vl, ql, dS, lens, slab, dc, B, N, L, spg);
      else if (mode == kLenByte)
        VQA_LAUNCH((oda_len_bwd_weight_kernel<G, kLenByte>), grid, dim3(nt), lds, s, vl, ql, dS, lens, slab, dc, B, N, L, spg);
      else
        VQA_LAUNCH((oda_len_bwd_weight_kernel<G, kLenPlain>), grid, dim3(nt), lds, s, vl, ql, dS, lens, slab, dc, B, N, L, spg);
    }
    const size_t n = (size_t)G * N * L;
    VQA_LAUNCH(oda_len_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, slab, d_w, n, SG);
  }
  VQA_LAUNCH(oda_len_dbias_kernel<G>, dim3(1), dim3(1024), 0, s, dS, lens, d_bias, B * N, N);
  return check_launch("object_difference_attention_len_bwd");
}

}  // namespace vqa

using namespace vqa;

// the limits of the unmasked entry points
static int oda_len_check(const char* who, int B, int N, int L, int G, float p) {
  VQA_REQUIRE(B > 0 && N > 0 && L > 0 && G > 0, VQA_E_BADARG, "%s: bad sizes B=%d N=%d L=%d G=%d", who, B, N, L, G);
  VQA_REQUIRE(G <= kLenMaxG && N <= 128 && L <= 1024, VQA_E_UNSUPPORTED, "%s: needs G <= 8, N <= 128, L <= 1024 (G=%d N=%d L=%d)",
              who, G, N, L);
  VQA_REQUIRE(p >= 0.f && p < 1.f, VQA_E_BADARG, "%s: p_drop=%f outside [0,1)", who, (double)p);
  VQA_REQUIRE(B <= 65535, VQA_E_UNSUPPORTED, "%s: B=%d exceeds 65535", who, B);
  return VQA_OK;
}

#define VQA_G_SWITCH(G, CALL) \
  switch (G) {                \
    case 1: return CALL(1);   \
    case 2: return CALL(2);   \
    case 3: return CALL(3);   \
    case 4: return CALL(4);   \
    case 5: return CALL(5);   \
    case 6: return CALL(6);   \
    case 7: return CALL(7);   \
    default: return CALL(8);  \
  }

extern "C" int vqa_object_difference_attention_len_fwd(const float* vl, const float* ql, const float* w, const float* bias,
                                                       const int32_t* lens, float* logits, float p_drop, uint64_t seed,
                                                       const uint64_t* seed_ptr, int B, int N, int L, int G,
                                                       vqa_stream_t stream) {
  VQA_REQUIRE(vl && ql && w && bias && lens && logits, VQA_E_BADARG, "object_difference_attention_len_fwd: null pointer");
  int rc = oda_len_check("object_difference_attention_len_fwd", B, N, L, G, p_drop);
  if (rc != VQA_OK) return rc;
  const DropCfg dc = make_drop(p_drop, seed, seed_ptr);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define CALL(G_) launch_len_fwd<G_>(vl, ql, w, bias, lens, logits, dc, B, N, L, s)
  VQA_G_SWITCH(G, CALL)
#undef CALL
}

extern "C" size_t vqa_object_difference_attention_len_bwd_workspace_bytes(int B, int N, int L, int G) {
  if (B <= 0 || N <= 0 || L <= 0 || G <= 0) return 0;
  return (size_t)(len_mfma_groups(B) > len_groups(B) ? len_mfma_groups(B) : len_groups(B)) * G * N * L * sizeof(float);
}

extern "C" int vqa_object_difference_attention_len_bwd(const float* vl, const float* ql, const float* w,
                                                       const float* d_logits, const int32_t* lens, float* d_vl, float* d_ql,
                                                       float* d_w, float* d_bias, void* workspace, size_t workspace_bytes,
                                                       float p_drop, uint64_t seed, const uint64_t* seed_ptr, int B, int N,
                                                       int L, int G, int gate_dvl, vqa_stream_t stream) {
  VQA_REQUIRE(vl && ql && w && d_logits && lens && d_vl && d_ql && d_w && d_bias && workspace, VQA_E_BADARG,
              "object_difference_attention_len_bwd: null pointer");
  int rc = oda_len_check("object_difference_attention_len_bwd", B, N, L, G, p_drop);
  if (rc != VQA_OK) return rc;
  VQA_REQUIRE(workspace_bytes >= vqa_object_difference_attention_len_bwd_workspace_bytes(B, N, L, G), VQA_E_BADARG,
              "object_difference_attention_len_bwd: workspace of %zu B is too small", workspace_bytes);
  const DropCfg dc = make_drop(p_drop, seed, seed_ptr);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* slab = static_cast<float*>(workspace);
#define CALL(G_) launch_len_bwd<G_>(vl, ql, w, d_logits, lens, d_vl, d_ql, d_w, d_bias, slab, dc, B, N, L, gate_dvl, s)
  VQA_G_SWITCH(G, CALL)
#undef CALL
}
