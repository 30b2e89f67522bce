// Mixed-precision recurrent path of the BayesianGRU question encoder: the per-step products of ops.GruSequence(bf16=True) as ONE
// bf16 product each (v_mfma_f32_32x32x16_bf16: bf16 operands, fp32 accumulation) instead of the split engine's six partial
// products (csrc/gru_gemm.hip).  The gate kernels are csrc/gru.hip's, instantiated for bf16 GEMM-operand histories.
//
// Arithmetic contract (bf(.) = round to nearest even to bf16; step t of putils.BayesianGRU.forward, putils/__init__.py:604-646,
// 691-731):
//   weights   Wb_g = bf(W_hg), g in {r, i, n}: a bf16 shadow packed once per forward pass from the fp32 masters, and its transpose
//             once per backward pass (vqa_pack_bf16); the masters stay fp32
//   forward   hm_t[g] = bf(h_{t-1} * m_g)            the product formed in fp32, rounded once (no masks: bf(h_{t-1}))
//             a[g]    = hm_t[g] Wb_g^T               fp32 accumulation, fp32 result
//             gates exactly as csrc/gru.hip: h, r, i, n, a_n stay fp32
//   backward  dzr, dzi, dzn, dan in fp32 as csrc/gru.hip forms them; d_gi is fp32 and unrounded
//             gzb_t[g] = bf(gz_t[g])                 the GEMM operand
//             dhm      = gzb_t[g] Wb_g               fp32 accumulation, fp32 result
//             dW_g     = sum_t gzb_t[g]^T hm_t[g]    over all T*B rows: vqa_gemm_bf16_tn, fp32, fixed-order slabs, no atomics
//   The roundings are straight-through for the gradients.  Everything is bitwise reproducible from run to run.
//
// The GEMM.  G same-shaped products per launch, c_g[m][n] = sum_k a_g[m][k] * w_g[n][k], on gemm_bf16_mfma.hpp's NT tile loop
// (two-stage LDS ring, global loads two stages ahead).  The contraction advances 64 at a time, so the caller pads operand ROWS
// to a multiple of 64 elements with zeros (2400 -> 2432) and the kernel reads the pads; rows past M (or N) are read from the
// clamped last row and reach only accumulator rows (columns) that are never stored -- an MFMA row depends on its own A row
// alone, so any M >= 1 runs and a non-finite row stays in its row.
// Tile and wave layout: 128 x 128 per workgroup, four waves 2 x 2, each wave 2 x 2 accumulators of 32 x 32.  Per 16-deep MFMA
// step a wave then reads 2 + 2 ds_read_b128 fragments for 4 MFMAs = one read per 32-cycle MFMA slot, half of the two reads per
// slot the LDS delivers for free (a third per slot would make the LDS array, not the matrix pipe, set the pace); a 64 x 64 tile
// (one accumulator per wave) sits exactly at two.  At the training shape (M = 512, N = 2400, G = 3) 128 x 128 gives
// 4 x 19 x 3 = 228 workgroups: one round on the 256 CUs at 89 % fill, where 128 x 64 or 64 x 128 need two rounds of half-sized
// tiles (456 workgroups) at a worse read-to-MFMA ratio (1.5 per slot).  M <= 64 takes 64 x 128 so that a short batch does not
// pay for 64 clamped rows.  Tiles are numbered row-tile-fastest inside a problem and handed out in contiguous ranges per XCD:
// the (at most 8) row tiles of one column tile are neighbours and share that 128-row slice of the weights in their XCD's L2.
#include "common.hpp"
#include "gemm_bf16_mfma.hpp"

namespace vqa {

struct GruBfArgs {
  const bf16* a;
  long a_gs;
  int lda;
  const bf16* w;
  long w_gs;
  int ldw;
  float* c;
  long c_gs;
  int ldc;
  int M, N, Kp;          // Kp: the contraction rounded up to a multiple of 64 (the operand rows' zero pads)
  int tiles_m, tiles_n;
  const int* lens;       // LEN instantiations only: [M] rows' step counts (device), and the step `t` of this launch
  int t;
};

// LEN (vqa_gru_gemm_bf16_len): a workgroup whose row tile holds no row with lens[row] > t returns before the tile loop and writes
// nothing -- one workgroup-uniform vote, ahead of every LDS use and every other barrier.
template <int BM, int BN, bool LEN = false>
__global__ __launch_bounds__(kBfThreads) void gru_gemm_bf16_kernel(GruBfArgs q) {
  using T = BfTile<BM, BN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tiles = q.tiles_m * q.tiles_n;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int prob = __builtin_amdgcn_readfirstlane(lin / tiles), tile = lin - prob * tiles;
  const int m0 = (tile % q.tiles_m) * BM, n0 = (tile / q.tiles_m) * BN;
  if constexpr (LEN) {
    int live = 0;
    for (int i = threadIdx.x; i < BM; i += kBfThreads) live |= (m0 + i < q.M && q.lens[m0 + i] > q.t) ? 1 : 0;
    if (!__syncthreads_or(live)) return;
  }
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
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (cc.row(tm, i) < q.M) (C + cc.uoff(tm, tn, i, q.ldc))[lo] = acc[tm][tn][i];
  }
}

template <int BM, int BN, bool LEN = false>
static int launch_gru_gemm_bf16(GruBfArgs q, int G, hipStream_t s) {
  q.tiles_m = (q.M + BM - 1) / BM;
  q.tiles_n = (q.N + BN - 1) / BN;
  const size_t lds = BfTile<BM, BN>::kSmemBytes;
  if constexpr (LEN) {
    VQA_ENSURE_LDS((gru_gemm_bf16_kernel<BM, BN, true>), lds);
    VQA_LAUNCH((gru_gemm_bf16_kernel<BM, BN, true>), dim3(q.tiles_m * q.tiles_n * G), dim3(kBfThreads), lds, s, q);
    return check_launch("gru_gemm_bf16_len");
  } else {
    VQA_ENSURE_LDS((gru_gemm_bf16_kernel<BM, BN>), lds);
    VQA_LAUNCH((gru_gemm_bf16_kernel<BM, BN>), dim3(q.tiles_m * q.tiles_n * G), dim3(kBfThreads), lds, s, q);
    return check_launch("gru_gemm_bf16");
  }
}

static int padded64(int K) { return (K + 63) / 64 * 64; }

static int gru_gemm_bf16_any(const char* who, bool len, const vqa_bf16_t* a, long a_gs, int lda, const vqa_bf16_t* w, long w_gs, int ldw,
                             float* c, long c_gs, int ldc, int G, int M, int N, int K, const int* lens, int t, hipStream_t s) {
  VQA_REQUIRE(a && w && c && (!len || lens), VQA_E_BADARG, "%s: null pointer", who);
  VQA_REQUIRE(G >= 1 && G <= 4096 && M >= 1 && N >= 1 && K >= 1 && a_gs >= 0 && w_gs >= 0 && c_gs >= 0, VQA_E_BADARG,
              "%s: bad sizes G=%d M=%d N=%d K=%d", who, G, M, N, K);
  VQA_REQUIRE(vqa_gru_gemm_bf16_supported(M, N, K, lda, ldw, ldc) == 1, VQA_E_UNSUPPORTED,
              "%s: shape outside the kernel (M=%d N=%d K=%d lda=%d ldw=%d ldc=%d): N %% 8 == 0, K %% 8 == 0, operand rows "
              "padded to a multiple of 64 elements (lda, ldw >= K rounded up to 64, %% 8 == 0), ldc >= N",
              who, M, N, K, lda, ldw, ldc);
  VQA_REQUIRE(aligned(a, 16) && aligned(w, 16) && aligned(c, 4) && a_gs % 8 == 0 && w_gs % 8 == 0, VQA_E_UNSUPPORTED,
              "%s: a, w (and their problem strides) must be 16-byte aligned", who);
  const GruBfArgs q{reinterpret_cast<const bf16*>(a), a_gs, lda, reinterpret_cast<const bf16*>(w), w_gs, ldw, c, c_gs, ldc,
                    M, N, padded64(K), 0, 0, lens, t};
  if (len) return M <= 64 ? launch_gru_gemm_bf16<64, 128, true>(q, G, s) : launch_gru_gemm_bf16<128, 128, true>(q, G, s);
  if (M <= 64) return launch_gru_gemm_bf16<64, 128>(q, G, s);
  return launch_gru_gemm_bf16<128, 128>(q, G, s);
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_gru_gemm_bf16_supported(int M, int N, int K, int lda, int ldw, int ldc) {
  if (M < 1 || N < 8 || K < 8 || N % 8 != 0 || K % 8 != 0) return 0;
  const int Kp = padded64(K);
  return (lda % 8 == 0 && ldw % 8 == 0 && lda >= Kp && ldw >= Kp && ldc >= N && (size_t)M * lda < (1ull << 31) &&
          (size_t)N * ldw < (1ull << 31) && (size_t)M * ldc < (1ull << 31)) ? 1 : 0;
}

extern "C" int vqa_gru_gemm_bf16(const vqa_bf16_t* a, long a_gs, int lda, const vqa_bf16_t* w, long w_gs, int ldw, float* c,
                                 long c_gs, int ldc, int G, int M, int N, int K, vqa_stream_t stream) {
  return gru_gemm_bf16_any("gru_gemm_bf16", false, a, a_gs, lda, w, w_gs, ldw, c, c_gs, ldc, G, M, N, K, nullptr, 0,
                           static_cast<hipStream_t>(stream));
}

extern "C" int vqa_gru_gemm_bf16_len(const vqa_bf16_t* a, long a_gs, int lda, const vqa_bf16_t* w, long w_gs, int ldw, float* c,
                                     long c_gs, int ldc, int G, int M, int N, int K, const int32_t* lens, int t, vqa_stream_t stream) {
  return gru_gemm_bf16_any("gru_gemm_bf16_len", true, a, a_gs, lda, w, w_gs, ldw, c, c_gs, ldc, G, M, N, K, lens, t,
                           static_cast<hipStream_t>(stream));
}

extern "C" int vqa_gru_gemm_bf16_tile_rows(int M) { return M <= 64 ? 64 : 128; }
