// Mixed-precision INPUT side of the BayesianGRU question encoder (ops.EncoderInputBf16; opt-in: input_dtype=bf16): the three
// [B*T,620] -> 2400 input projections of all T steps as bf16 products with fp32 accumulation, and the fused kernels around
// them -- the embedding lookup, the sequence-shared input dropout masks, the bias, the embedding gradient.  The recurrent side
// is csrc/gru_bf16.hip; the two modes are independent switches.
//
// Arithmetic contract (bf(.) = round to nearest even to bf16; m = b*T + t a row; e[m] = table[idx[m]] or the caller's x[b,t,:];
// mx[b][g] the sequence-shared input mask of gate g in {r, i, n}, 1 without masks; putils/__init__.py:691-703):
//   weights   Wb_g = bf(W_ig): a bf16 shadow [3,2400,640] of the fp32 masters, rows zero-padded to a multiple of 64, packed once
//             per forward pass with vqa_pack_bf16 and transposed once per backward pass; a temporary, never a parameter
//   forward   xb_g[m] = bf(e[m] * mx[b][g])          the product formed in fp32, rounded once; without masks ONE plane bf(e[m])
//                                                    shared by the three gates (problem stride 0)
//             gi_g    = xb_g Wb_g^T + b_g            fp32 accumulation, the fp32 bias added after it; gi fp32 [3,B,T,H]
//   backward  d_gi arrives fp32 from the gate kernels
//             d_b_g   = column sum of the UNROUNDED fp32 d_gi_g      vqa_column_sum: fixed order
//             dgb     = bf(d_gi)                                     one vqa_pack_bf16 launch
//             dW_g    = dgb_g^T xb_g over all B*T rows               vqa_gemm_bf16_tn_ex: fp32, fixed-order slabs, no atomics,
//                                                                    the 640 padded columns cropped to 620 in its store
//             dxm_g   = dgb_g Wb_g                                   vqa_gru_gemm_bf16 against the transposed shadow, fp32
//             d_e[m]  = sum_g dxm_g[m] * mx[b][g]                    fp32, g = r, i, n in that order
//             d_table[v] = sum_{m: idx[m] = v, v != padding_idx} d_e[m]
//   The roundings are straight-through for the gradients; gi, d_gi, the biases and the master weights stay fp32.  Everything up
//   to d_e is bitwise reproducible.  The scatter into the table adds with fp32 atomics in arrival order -- as the index_add_ of
//   the fp32 path does: that one gradient is as reproducible as it is there, no more and no less.
//
// vqa_embed_pack_bf16 and vqa_embed_grad are bandwidth kernels: one thread per 8 (pack: one 16-byte bf16 store, two 16-byte
// loads) or 4 (grad: 16-byte loads, a 16-byte store or four atomics) consecutive columns of one row.  K % 4 == 0, so the last
// chunk of a pack row holds 8 or 4 columns (K = 620: 77 chunks of 8 and one of 4, an 8-byte store); columns [K, ld) are never
// written.  A token id outside [0,V) is clamped into the table (the policy of the CE label kernel): no read outside of it.
//
// vqa_gemm_bf16_nt_f32_bias is csrc/gru_bf16.hip's product (gemm_bf16_mfma.hpp's NT tile loop, 128 x 128 tiles or 64 x 128 for
// M <= 64, tiles numbered row-tile-fastest and handed out in contiguous ranges per XCD, rows past M read from the clamped last
// row into accumulator rows that are never stored) with the bias in its store and a free K >= 1: the contraction runs over the
// operand rows' zero pads up to the next multiple of 64.  A kernel of its own: gru_gemm_bf16_kernel's bits are pinned.
#include "common.hpp"
#include "gemm_bf16_mfma.hpp"

namespace vqa {

struct EncInGemmArgs {
  const bf16* a;
  long a_gs;
  int lda;
  const bf16* w;
  long w_gs;
  int ldw;
  const float* bias;     // fp32 [G] rows of N, bias_gs elements apart; or null
  long bias_gs;
  float* c;
  long c_gs;
  int ldc;
  int M, N, Kp;          // Kp: the contraction rounded up to a multiple of 64 (the operand rows' zero pads)
  int tiles_m, tiles_n;
};

template <int BM, int BN>
__global__ __launch_bounds__(kBfThreads) void gemm_bf16_nt_f32_bias_kernel(EncInGemmArgs q) {
  using T = BfTile<BM, BN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tiles = q.tiles_m * q.tiles_n;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int prob = __builtin_amdgcn_readfirstlane(lin / tiles), tile = lin - prob * tiles;
  const int m0 = (tile % q.tiles_m) * BM, n0 = (tile / q.tiles_m) * BN;
  const bf16* A = q.a + (size_t)prob * q.a_gs;
  const bf16* W = q.w + (size_t)prob * q.w_gs;
  float* C = q.c + (size_t)prob * q.c_gs;
  f32x16 acc[T::TM][T::TN];
  bf_zero_acc(acc);
  gemm_bf16_nt_tile<BM, BN>(A, q.lda, q.M, W, q.ldw, q.N, m0, n0, q.Kp, smem, acc);
  const BfAccCoord<BM, BN> cc(m0, n0);
  const unsigned lo = cc.loff(q.ldc);
#pragma unroll
  for (int tn = 0; tn < T::TN; ++tn) {
    if (cc.col(tn) >= q.N) continue;
    const float bv = q.bias != nullptr ? q.bias[(size_t)prob * q.bias_gs + cc.col(tn)] : 0.f;
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (cc.row(tm, i) < q.M) (C + cc.uoff(tm, tn, i, q.ldc))[lo] = q.bias != nullptr ? acc[tm][tn][i] + bv : acc[tm][tn][i];
  }
}

template <int BM, int BN>
static int launch_enc_in_gemm(EncInGemmArgs q, int G, hipStream_t s) {
  q.tiles_m = (q.M + BM - 1) / BM;
  q.tiles_n = (q.N + BN - 1) / BN;
  const size_t lds = BfTile<BM, BN>::kSmemBytes;
  VQA_ENSURE_LDS((gemm_bf16_nt_f32_bias_kernel<BM, BN>), lds);
  VQA_LAUNCH((gemm_bf16_nt_f32_bias_kernel<BM, BN>), dim3(q.tiles_m * q.tiles_n * G), dim3(kBfThreads), lds, s, q);
  return check_launch("gemm_bf16_nt_f32_bias");
}

__device__ __forceinline__ size_t token_row(const int64_t* __restrict__ idx, int m, int V) {
  const int64_t v = idx[m];
  return (size_t)(v < 0 ? 0 : (v >= V ? V - 1 : v));
}

// xb[g][m][col .. col+8) = bf(src[row(m)][col ..] * masks[m / T][g][col ..]); thread = one chunk of 8 columns of one row
__global__ __launch_bounds__(256) void embed_pack_bf16_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx,
                                                              const float* __restrict__ masks, bf16* __restrict__ xb,
                                                              size_t plane, int ld, int M, int K, int T, int V, int G,
                                                              int chunks) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)M * chunks) return;
  const int m = (int)(id / chunks), col = (int)(id - (size_t)m * chunks) * 8;
  const bool full = col + 8 <= K;      // else the row's last 4 columns (K % 4 == 0)
  const float* e = src + (idx != nullptr ? token_row(idx, m, V) : (size_t)m) * K + col;
  const float4 lo = ld4(e), hi = full ? ld4(e + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  bf16* out = xb + (size_t)m * ld + col;
  const int planes = masks != nullptr ? G : 1;
  for (int g = 0; g < planes; ++g) {
    float4 a = lo, b = hi;
    if (masks != nullptr) {
      const float* mk = masks + ((size_t)(m / T) * G + g) * K + col;
      a = mul4(lo, ld4(mk));
      if (full) b = mul4(hi, ld4(mk + 4));
    }
    bf16* o = out + (size_t)g * plane;
    if (full) {
      *reinterpret_cast<uint4*>(o) = make_uint4(pack_bf16(a.x, a.y), pack_bf16(a.z, a.w), pack_bf16(b.x, b.y), pack_bf16(b.z, b.w));
    } else {
      st4(o, a);
    }
  }
}

// d_e[m][col .. col+4) = sum_g dxm[g][m][col ..] * masks[m / T][g][col ..]; with idx: added into out[idx[m]] (rows of the
// padding id skipped), else stored to out[m].  thread = 4 columns of one row
__global__ __launch_bounds__(256) void embed_grad_kernel(const float* __restrict__ dxm, size_t dxm_gs, int ldx,
                                                         const float* __restrict__ masks, const int64_t* __restrict__ idx,
                                                         long padding_idx, float* __restrict__ out, int M, int K, int T, int V,
                                                         int G, int chunks) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)M * chunks) return;
  const int m = (int)(id / chunks), col = (int)(id - (size_t)m * chunks) * 4;
  if (idx != nullptr && idx[m] == (int64_t)padding_idx) return;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int g = 0; g < G; ++g) {
    const float4 d = ld4(dxm + (size_t)g * dxm_gs + (size_t)m * ldx + col);
    if (masks != nullptr) {
      const float4 k = ld4(masks + ((size_t)(m / T) * G + g) * K + col);
      acc = make_float4(fmaf(d.x, k.x, acc.x), fmaf(d.y, k.y, acc.y), fmaf(d.z, k.z, acc.z), fmaf(d.w, k.w, acc.w));
    } else {
      acc = add4(acc, d);
    }
  }
  if (idx == nullptr) {
    st4(out + (size_t)m * K + col, acc);
    return;
  }
  float* p = out + token_row(idx, m, V) * K + col;
  unsafeAtomicAdd(p, acc.x);          // (the hardware fp32 add, no return value: what index_add_ issues)
  unsafeAtomicAdd(p + 1, acc.y);
  unsafeAtomicAdd(p + 2, acc.z);
  unsafeAtomicAdd(p + 3, acc.w);
}

static int padded64(int K) { return (K + 63) / 64 * 64; }

static int embed_check(const char* who, const void* idx, const void* masks, int M, int K, int T, int V, int G) {
  VQA_REQUIRE(M >= 1 && K >= 1 && T >= 1 && G >= 1 && G <= 4096 && M % T == 0, VQA_E_BADARG,
              "%s: bad sizes M=%d K=%d T=%d G=%d (M = B * T rows)", who, M, K, T, G);
  VQA_REQUIRE(idx == nullptr || V >= 1, VQA_E_BADARG, "%s: a table of V=%d rows", who, V);
  VQA_REQUIRE(K % 4 == 0, VQA_E_UNSUPPORTED, "%s: needs K %% 4 == 0 (K=%d)", who, K);
  VQA_REQUIRE((size_t)M * ((K + 3) / 4) < (1ull << 40), VQA_E_UNSUPPORTED, "%s: M * K too large", who);
  VQA_REQUIRE(aligned(idx, 8) && aligned(masks, 16), VQA_E_UNSUPPORTED, "%s: idx must be 8-byte, masks 16-byte aligned", who);
  return VQA_OK;
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_embed_pack_bf16(const float* src, const int64_t* idx, const float* masks, vqa_bf16_t* xb, long plane_stride,
                                   int ld, int M, int K, int T, int V, int G, vqa_stream_t stream) {
  VQA_REQUIRE(src && xb, VQA_E_BADARG, "embed_pack_bf16: null pointer");
  int rc = embed_check("embed_pack_bf16", idx, masks, M, K, T, V, G);
  if (rc != VQA_OK) return rc;
  VQA_REQUIRE(ld >= K && plane_stride >= 0, VQA_E_BADARG, "embed_pack_bf16: row stride %d < K=%d", ld, K);
  VQA_REQUIRE(masks == nullptr || G == 1 || (size_t)plane_stride >= (size_t)M * ld, VQA_E_BADARG,
              "embed_pack_bf16: plane stride %ld < M * ld = %zu", plane_stride, (size_t)M * ld);
  VQA_REQUIRE(ld % 8 == 0 && plane_stride % 8 == 0 && aligned(xb, 16) && aligned(src, 16), VQA_E_UNSUPPORTED,
              "embed_pack_bf16: needs ld %% 8 == 0, a plane stride %% 8 == 0 and 16-byte aligned src / xb");
  const int chunks = (K + 7) / 8;
  const size_t n = (size_t)M * chunks;
  VQA_LAUNCH(embed_pack_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, idx,
             masks, reinterpret_cast<bf16*>(xb), (size_t)plane_stride, ld, M, K, T, V, G, chunks);
  return check_launch("embed_pack_bf16");
}

extern "C" int vqa_gemm_bf16_nt_f32_bias(const vqa_bf16_t* a, long a_gs, int lda, const vqa_bf16_t* w, long w_gs, int ldw,
                                         const float* bias, long bias_gs, float* c, long c_gs, int ldc, int G, int M, int N,
                                         int K, vqa_stream_t stream) {
  VQA_REQUIRE(a && w && c, VQA_E_BADARG, "gemm_bf16_nt_f32_bias: null pointer");
  VQA_REQUIRE(G >= 1 && G <= 4096 && M >= 1 && N >= 1 && K >= 1 && a_gs >= 0 && w_gs >= 0 && c_gs >= 0 && bias_gs >= 0,
              VQA_E_BADARG, "gemm_bf16_nt_f32_bias: bad sizes G=%d M=%d N=%d K=%d", G, M, N, K);
  const int Kp = padded64(K);
  VQA_REQUIRE(N % 8 == 0 && lda % 8 == 0 && ldw % 8 == 0 && lda >= Kp && ldw >= Kp && ldc >= N &&
                  (size_t)M * lda < (1ull << 31) && (size_t)N * ldw < (1ull << 31) && (size_t)M * ldc < (1ull << 31),
              VQA_E_UNSUPPORTED,
              "gemm_bf16_nt_f32_bias: shape outside the kernel (M=%d N=%d K=%d lda=%d ldw=%d ldc=%d): N %% 8 == 0, operand rows "
              "padded to a multiple of 64 elements (lda, ldw >= K rounded up to 64, %% 8 == 0), ldc >= N",
              M, N, K, lda, ldw, ldc);
  VQA_REQUIRE(aligned(a, 16) && aligned(w, 16) && aligned(c, 4) && aligned(bias, 4) && a_gs % 8 == 0 && w_gs % 8 == 0,
              VQA_E_UNSUPPORTED, "gemm_bf16_nt_f32_bias: a, w (and their problem strides) must be 16-byte aligned");
  const EncInGemmArgs q{reinterpret_cast<const bf16*>(a), a_gs, lda, reinterpret_cast<const bf16*>(w), w_gs, ldw, bias, bias_gs,
                        c, c_gs, ldc, M, N, Kp, 0, 0};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (M <= 64) return launch_enc_in_gemm<64, 128>(q, G, s);
  return launch_enc_in_gemm<128, 128>(q, G, s);
}

extern "C" int vqa_embed_grad(const float* dxm, long dxm_gs, int ldx, const float* masks, const int64_t* idx, long padding_idx,
                              float* out, int M, int K, int T, int V, int G, vqa_stream_t stream) {
  VQA_REQUIRE(dxm && out, VQA_E_BADARG, "embed_grad: null pointer");
  int rc = embed_check("embed_grad", idx, masks, M, K, T, V, G);
  if (rc != VQA_OK) return rc;
  VQA_REQUIRE(ldx >= K && dxm_gs >= 0 && (G == 1 || (size_t)dxm_gs >= (size_t)M * ldx), VQA_E_BADARG,
              "embed_grad: dxm row stride %d < K=%d, or plane stride %ld < M * ldx", ldx, K, dxm_gs);
  VQA_REQUIRE(ldx % 4 == 0 && dxm_gs % 4 == 0 && aligned(dxm, 16) && aligned(out, 16), VQA_E_UNSUPPORTED,
              "embed_grad: needs ldx %% 4 == 0, a plane stride %% 4 == 0 and 16-byte aligned dxm / out");
  const int chunks = K / 4;
  const size_t n = (size_t)M * chunks;
  VQA_LAUNCH(embed_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dxm,
             (size_t)dxm_gs, ldx, masks, idx, padding_idx, out, M, K, T, V, G, chunks);
  return check_launch("embed_grad");
}
