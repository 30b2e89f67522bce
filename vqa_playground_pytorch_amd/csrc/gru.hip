// Gate math of the BayesianGRU question encoder (SkipThoughts' uni-skip GRU), one kernel per time step each way -- the one pair
// behind all eight vqa_gru_gates_{fwd,bwd}[_bf16][_len] entry points.
//
// Replaces, per step t of putils.BayesianGRU.forward (putils/__init__.py:704-731 with the cell of :604-646):
//     hr, hi, hn = h*m_r, h*m_i, h*m_n                     (sequence-shared dropout masks, SequentialDropout :503-539)
//     r = sigmoid(gi_r[t] + W_hr hr);  i = sigmoid(gi_i[t] + W_hi hi);  n = af(gi_n[t] + r * (W_hn hn))
//     h' = (1 - i) * n + i * h
// -- about fifteen elementwise launches around three small GEMMs, and twice that in autograd's backward.  Here the
// three recurrent GEMMs of a step are ONE batched GEMM a[g] = hm[g] W_g^T (ops.GruSequence) and everything else is this file:
//   forward : (gi[:, :, t, :], a, h) -> h', the three masked copies of h' that feed the next step's GEMM (written
//             straight into the [3,T,B,ld] history the weight-gradient GEMM reads at the end), and r, i, n, a_n saved
//   backward: dh_t = d_out[t] + carry + sum_g dhm[g]*m_g;  gate derivatives -> gz[g] (gradient at the GEMM outputs,
//             written into its [3,T,B,ld] history), d_gi[:, :, t, :], carry' = dh_t * i
// HBM-light (B*H elements, ~12 floats each).  af: 1 relu, 3 tanh.  Lane = 4 adjacent hidden units.  Vector stores only.
//
// HT: the GEMM-operand histories' type.  float: row stride ld = H.  bf16 (the mixed-precision path, csrc/gru_bf16.hip states its
// contract): rows padded to ld, hm = bf(h' * m_g) and gz = bf(dzr), bf(dzi), bf(dan) rounded once at the store; h, r, i, n, a_n and
// d_gi stay fp32 and unrounded.
//
// LEN: a per-row step count.  BayesianGRU returns the state at step len - 1 (putils/__init__.py:731-743), so a step past a
// question's end computes a value nobody reads and a gradient that is exactly zero.  With lens [B] (int32, device;
// 1 <= lens[b] <= T) row b is ACTIVE at step t iff t < lens[b]:
//   forward   active:   the instructions of LEN = false on the same operands
//             inactive: h_new = h_prev, hm_next[g] = h_prev * m_g (bf16 history: rounded as ever), so the histories stay finite;
//                       a and gi are not read, r / i / n / a_n are not written
//   backward  active:   the instructions of LEN = false, except that dhm[b] joins dh only where row b is active at t + 1 as well
//                       (the product tile that holds it may not have been computed: vqa_gemm_nt_split_batched_len)
//             inactive: gz[., t, b] = 0, d_gi[., b, t, .] = 0 exactly, carry_out = d_out_t + carry_in; dhm and the saved tensors
//                       are not read
// What an inactive row may not read is never loaded -- it is uninitialised memory and may hold NaN --, a branch per thread: one
// thread owns 4 adjacent hidden units of one row.  With LEN = false `lens` is never dereferenced.
//
// The arithmetic is fixed by the source, not by the compiler: the kernels are compiled with floating-point contraction OFF and
// spell their fused multiply-adds (n's pre-activation fma(r, a_n, gi_n); h' = fma(i, h, (1 - i) * n); tanh' = fma(-n, n, 1);
// dhm * m is a product of its own, then added) -- left to the compiler, one of four lanes of h' came out as fma(1 - i, n, i * h).
#include "common.hpp"

namespace vqa {

__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float gru_af(float z, int af) { return af == 1 ? fmaxf(z, 0.f) : tanhf(z); }
__device__ __forceinline__ float gru_af_grad(float n, int af) { return af == 1 ? (n > 0.f ? 1.f : 0.f) : fmaf(-n, n, 1.f); }

#define VQA_GRU_FOR4(EXPR)                 \
  {                                        \
    { constexpr int c = 0; EXPR; }         \
    { constexpr int c = 1; EXPR; }         \
    { constexpr int c = 2; EXPR; }         \
    { constexpr int c = 3; EXPR; }         \
  }
__device__ __forceinline__ float& f4(float4& v, int c) { return reinterpret_cast<float*>(&v)[c]; }
__device__ __forceinline__ float f4(const float4& v, int c) { return reinterpret_cast<const float*>(&v)[c]; }

// gi [3,B,T,H]; a [3,B,H]; h_prev [B,H]; masks [3,B,H] or null; h_new [B,H] (slot t of the [T,B,H] output);
// hm_next: base of slot t+1 of the [3,T,B,ld] history (group stride hist_gs, row stride ld) or null at the last step;
// saved r, i, n, an: slot t of [T,B,H] each.
template <typename HT, bool LEN>
__global__ __launch_bounds__(256) void gru_gates_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ a,
                                                            const float* __restrict__ h_prev,
                                                            const float* __restrict__ masks, float* __restrict__ h_new,
                                                            HT* __restrict__ hm_next, size_t hist_gs, int ld,
                                                            float* __restrict__ r_s, float* __restrict__ i_s,
                                                            float* __restrict__ n_s, float* __restrict__ an_s,
                                                            const int* __restrict__ lens, int B, int T, int H, int t, int af) {
#pragma clang fp contract(off)
  const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const size_t BH = (size_t)B * H;
  if (e >= BH) return;
  const size_t b = e / H, h = e % H;
  const float4 hp = ld4(h_prev + e);
  bool active = true;
  if constexpr (LEN) active = t < lens[b];
  float4 hn;
  if (active) {
    const size_t gio = (b * T + t) * H + h, gig = (size_t)B * T * H;
    const float4 gr = ld4(gi + gio), gz = ld4(gi + gig + gio), gn = ld4(gi + 2 * gig + gio);
    const float4 ar = ld4(a + e), ai = ld4(a + BH + e), an = ld4(a + 2 * BH + e);
    float4 r, i, n;
    VQA_GRU_FOR4(f4(r, c) = sigmoidf(f4(gr, c) + f4(ar, c)); f4(i, c) = sigmoidf(f4(gz, c) + f4(ai, c));
                 f4(n, c) = gru_af(fmaf(f4(r, c), f4(an, c), f4(gn, c)), af);
                 f4(hn, c) = fmaf(f4(i, c), f4(hp, c), (1.f - f4(i, c)) * f4(n, c)));
    st4(r_s + e, r);
    st4(i_s + e, i);
    st4(n_s + e, n);
    st4(an_s + e, an);
  } else {
    hn = hp;
  }
  st4(h_new + e, hn);
  if (hm_next != nullptr) {
    const size_t ho = b * (size_t)ld + h;
#pragma unroll
    for (int g = 0; g < 3; ++g) st4(hm_next + g * hist_gs + ho, masks != nullptr ? mul4(hn, ld4(masks + g * BH + e)) : hn);
  }
}

// d_out_t [B,H] or null; carry_in [B,H] or null; dhm [3,B,H] or null (both null at the last step); masks [3,B,H] or null;
// saved r, i, n, an (slot t), h_prev [B,H]; outputs gz: slot t of the [3,T,B,ld] history (group stride hist_gs, row stride ld),
// d_gi [3,B,T,H] (slot t), carry_out [B,H].
template <typename HT, bool LEN>
__global__ __launch_bounds__(256) void gru_gates_bwd_kernel(const float* __restrict__ d_out_t,
                                                            const float* __restrict__ carry_in,
                                                            const float* __restrict__ dhm, const float* __restrict__ masks,
                                                            const float* __restrict__ r_s, const float* __restrict__ i_s,
                                                            const float* __restrict__ n_s, const float* __restrict__ an_s,
                                                            const float* __restrict__ h_prev, HT* __restrict__ gz,
                                                            size_t hist_gs, int ld, float* __restrict__ d_gi,
                                                            float* __restrict__ carry_out, const int* __restrict__ lens, int B,
                                                            int T, int H, int t, int af) {
#pragma clang fp contract(off)
  const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const size_t BH = (size_t)B * H;
  if (e >= BH) return;
  const size_t b = e / H, h = e % H;
  const size_t ho = b * (size_t)ld + h;
  const size_t gio = (b * T + t) * H + h, gig = (size_t)B * T * H;
  float4 dh = d_out_t != nullptr ? ld4(d_out_t + e) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (carry_in != nullptr) dh = add4(dh, ld4(carry_in + e));
  bool next_active = true;                            // row b is active at t + 1 as well: dhm[b] was computed
  if constexpr (LEN) {
    const int len = lens[b];
    if (t >= len) {
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        st4(gz + g * hist_gs + ho, z);
        st4(d_gi + g * gig + gio, z);
      }
      st4(carry_out + e, dh);
      return;
    }
    next_active = t + 1 < len;
  }
  if (dhm != nullptr && next_active) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      float4 d = ld4(dhm + g * BH + e);
      if (masks != nullptr) {
        const float4 m = ld4(masks + g * BH + e);
        VQA_GRU_FOR4(f4(d, c) = f4(d, c) * f4(m, c));
      }
      VQA_GRU_FOR4(f4(dh, c) = f4(dh, c) + f4(d, c));
    }
  }
  const float4 r = ld4(r_s + e), i = ld4(i_s + e), n = ld4(n_s + e), an = ld4(an_s + e), hp = ld4(h_prev + e);
  float4 dzr, dzi, dzn, dan, co;
  VQA_GRU_FOR4(const float d = f4(dh, c); const float dn = d * (1.f - f4(i, c)) * gru_af_grad(f4(n, c), af);
               f4(dzn, c) = dn; f4(dan, c) = dn * f4(r, c);
               f4(dzr, c) = dn * f4(an, c) * f4(r, c) * (1.f - f4(r, c));
               f4(dzi, c) = d * (f4(hp, c) - f4(n, c)) * f4(i, c) * (1.f - f4(i, c)); f4(co, c) = d * f4(i, c));
  st4(gz + ho, dzr);
  st4(gz + hist_gs + ho, dzi);
  st4(gz + 2 * hist_gs + ho, dan);
  st4(d_gi + gio, dzr);
  st4(d_gi + gig + gio, dzi);
  st4(d_gi + 2 * gig + gio, dzn);
  st4(carry_out + e, co);
}

// every mode's limits: H % 4 for the fp32 history (its ld is H), H % 8 and the history's layout for bf16, the counts for LEN
template <typename HT, bool LEN>
static int gru_check(const char* who, const HT* hist, size_t hist_gs, int ld, const int* lens, int B, int T, int H, int t, int af) {
  constexpr bool bf = sizeof(HT) == 2;
  VQA_REQUIRE(!LEN || lens != nullptr, VQA_E_BADARG, "%s: null pointer", who);
  VQA_REQUIRE(B > 0 && T > 0 && H > 0 && t >= 0 && t < T, VQA_E_BADARG, "%s: bad sizes B=%d T=%d H=%d t=%d", who, B, T, H, t);
  VQA_REQUIRE(H % (bf ? 8 : 4) == 0, VQA_E_UNSUPPORTED, "%s: needs H %% %d == 0 (H=%d)", who, bf ? 8 : 4, H);
  VQA_REQUIRE(af == 1 || af == 3, VQA_E_BADARG, "%s: af must be 1 (relu) or 3 (tanh), got %d", who, af);
  if (bf) {
    VQA_REQUIRE(hist == nullptr || ld >= H, VQA_E_BADARG, "%s: history row stride %d < H=%d", who, ld, H);
    VQA_REQUIRE(hist == nullptr || (ld % 8 == 0 && hist_gs % 8 == 0 && aligned(hist, 16)), VQA_E_UNSUPPORTED,
                "%s: the bf16 history needs ld %% 8 == 0, a group stride %% 8 == 0 and a 16-byte aligned slot", who);
  }
  return VQA_OK;
}

// (the launches name literal instantiations so that the launch log says which one ran)
template <typename HT, bool LEN>
static int gates_fwd(const char* who, const float* gi, const float* a, const float* h_prev, const float* masks, float* h_new,
                     HT* hm_next, size_t hist_gs, int ld, float* r_s, float* i_s, float* n_s, float* an_s, const int* lens, int B, int T,
                     int H, int t, int af, vqa_stream_t stream) {
  VQA_REQUIRE(gi && a && h_prev && h_new && r_s && i_s && n_s && an_s, VQA_E_BADARG, "%s: null pointer", who);
  int rc = gru_check<HT, LEN>(who, hm_next, hist_gs, ld, lens, B, T, H, t, af);
  if (rc != VQA_OK) return rc;
  const size_t n4 = (size_t)B * H / 4;
  const dim3 grid((unsigned)((n4 + 255) / 256));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if constexpr (LEN)
    VQA_LAUNCH((gru_gates_fwd_kernel<HT, true>), grid, dim3(256), 0, s, gi, a, h_prev, masks, h_new, hm_next, hist_gs, ld, r_s, i_s, n_s,
               an_s, lens, B, T, H, t, af);
  else
    VQA_LAUNCH((gru_gates_fwd_kernel<HT, false>), grid, dim3(256), 0, s, gi, a, h_prev, masks, h_new, hm_next, hist_gs, ld, r_s, i_s, n_s,
               an_s, lens, B, T, H, t, af);
  return check_launch(who);
}

template <typename HT, bool LEN>
static int gates_bwd(const char* who, const float* d_out_t, const float* carry_in, const float* dhm, const float* masks,
                     const float* r_s, const float* i_s, const float* n_s, const float* an_s, const float* h_prev, HT* gz,
                     size_t hist_gs, int ld, float* d_gi, float* carry_out, const int* lens, int B, int T, int H, int t, int af,
                     vqa_stream_t stream) {
  VQA_REQUIRE(r_s && i_s && n_s && an_s && h_prev && gz && d_gi && carry_out, VQA_E_BADARG, "%s: null pointer", who);
  int rc = gru_check<HT, LEN>(who, gz, hist_gs, ld, lens, B, T, H, t, af);
  if (rc != VQA_OK) return rc;
  const size_t n4 = (size_t)B * H / 4;
  const dim3 grid((unsigned)((n4 + 255) / 256));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if constexpr (LEN)
    VQA_LAUNCH((gru_gates_bwd_kernel<HT, true>), grid, dim3(256), 0, s, d_out_t, carry_in, dhm, masks, r_s, i_s, n_s, an_s, h_prev, gz,
               hist_gs, ld, d_gi, carry_out, lens, B, T, H, t, af);
  else
    VQA_LAUNCH((gru_gates_bwd_kernel<HT, false>), grid, dim3(256), 0, s, d_out_t, carry_in, dhm, masks, r_s, i_s, n_s, an_s, h_prev, gz,
               hist_gs, ld, d_gi, carry_out, lens, B, T, H, t, af);
  return check_launch(who);
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_gru_gates_fwd(const float* gi, const float* a, const float* h_prev, const float* masks, float* h_new,
                                 float* hm_next, size_t hist_group_stride, float* r_s, float* i_s, float* n_s, float* an_s,
                                 int B, int T, int H, int t, int af, vqa_stream_t stream) {
  return gates_fwd<float, false>("gru_gates_fwd", gi, a, h_prev, masks, h_new, hm_next, hist_group_stride, H, r_s, i_s, n_s, an_s,
                                 nullptr, B, T, H, t, af, stream);
}

extern "C" int vqa_gru_gates_bwd(const float* d_out_t, const float* carry_in, const float* dhm, const float* masks,
                                 const float* r_s, const float* i_s, const float* n_s, const float* an_s,
                                 const float* h_prev, float* gz, size_t hist_group_stride, float* d_gi, float* carry_out,
                                 int B, int T, int H, int t, int af, vqa_stream_t stream) {
  return gates_bwd<float, false>("gru_gates_bwd", d_out_t, carry_in, dhm, masks, r_s, i_s, n_s, an_s, h_prev, gz, hist_group_stride, H,
                                 d_gi, carry_out, nullptr, B, T, H, t, af, stream);
}

extern "C" int vqa_gru_gates_fwd_bf16(const float* gi, const float* a, const float* h_prev, const float* masks, float* h_new,
                                      vqa_bf16_t* hm_next, size_t hist_group_stride, int ld, float* r_s, float* i_s, float* n_s,
                                      float* an_s, int B, int T, int H, int t, int af, vqa_stream_t stream) {
  return gates_fwd<bf16, false>("gru_gates_fwd_bf16", gi, a, h_prev, masks, h_new, reinterpret_cast<bf16*>(hm_next), hist_group_stride,
                                ld, r_s, i_s, n_s, an_s, nullptr, B, T, H, t, af, stream);
}

extern "C" int vqa_gru_gates_bwd_bf16(const float* d_out_t, const float* carry_in, const float* dhm, const float* masks,
                                      const float* r_s, const float* i_s, const float* n_s, const float* an_s,
                                      const float* h_prev, vqa_bf16_t* gz, size_t hist_group_stride, int ld, float* d_gi,
                                      float* carry_out, int B, int T, int H, int t, int af, vqa_stream_t stream) {
  return gates_bwd<bf16, false>("gru_gates_bwd_bf16", d_out_t, carry_in, dhm, masks, r_s, i_s, n_s, an_s, h_prev,
                                reinterpret_cast<bf16*>(gz), hist_group_stride, ld, d_gi, carry_out, nullptr, B, T, H, t, af, stream);
}

extern "C" int vqa_gru_gates_fwd_len(const float* gi, const float* a, const float* h_prev, const float* masks, float* h_new,
                                     float* hm_next, size_t hist_group_stride, float* r_s, float* i_s, float* n_s, float* an_s,
                                     const int32_t* lens, int B, int T, int H, int t, int af, vqa_stream_t stream) {
  return gates_fwd<float, true>("gru_gates_fwd_len", gi, a, h_prev, masks, h_new, hm_next, hist_group_stride, H, r_s, i_s, n_s, an_s,
                                lens, B, T, H, t, af, stream);
}

extern "C" int vqa_gru_gates_bwd_len(const float* d_out_t, const float* carry_in, const float* dhm, const float* masks,
                                     const float* r_s, const float* i_s, const float* n_s, const float* an_s, const float* h_prev,
                                     float* gz, size_t hist_group_stride, float* d_gi, float* carry_out, const int32_t* lens, int B,
                                     int T, int H, int t, int af, vqa_stream_t stream) {
  return gates_bwd<float, true>("gru_gates_bwd_len", d_out_t, carry_in, dhm, masks, r_s, i_s, n_s, an_s, h_prev, gz, hist_group_stride, H,
                                d_gi, carry_out, lens, B, T, H, t, af, stream);
}

extern "C" int vqa_gru_gates_fwd_bf16_len(const float* gi, const float* a, const float* h_prev, const float* masks, float* h_new,
                                          vqa_bf16_t* hm_next, size_t hist_group_stride, int ld, float* r_s, float* i_s, float* n_s,
                                          float* an_s, const int32_t* lens, int B, int T, int H, int t, int af, vqa_stream_t stream) {
  return gates_fwd<bf16, true>("gru_gates_fwd_bf16_len", gi, a, h_prev, masks, h_new, reinterpret_cast<bf16*>(hm_next), hist_group_stride,
                               ld, r_s, i_s, n_s, an_s, lens, B, T, H, t, af, stream);
}

extern "C" int vqa_gru_gates_bwd_bf16_len(const float* d_out_t, const float* carry_in, const float* dhm, const float* masks,
                                          const float* r_s, const float* i_s, const float* n_s, const float* an_s,
                                          const float* h_prev, vqa_bf16_t* gz, size_t hist_group_stride, int ld, float* d_gi,
                                          float* carry_out, const int32_t* lens, int B, int T, int H, int t, int af,
                                          vqa_stream_t stream) {
  return gates_bwd<bf16, true>("gru_gates_bwd_bf16_len", d_out_t, carry_in, dhm, masks, r_s, i_s, n_s, an_s, h_prev,
                               reinterpret_cast<bf16*>(gz), hist_group_stride, ld, d_gi, carry_out, lens, B, T, H, t, af, stream);
}
