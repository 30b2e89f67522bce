// Packed (ragged) region batches -> the padded [B,N,D] tensor every region-side kernel reads.
//
// A packed batch ships only the real rows of its samples, back to back: packed [B*N, D] is a capacity-sized buffer of which the first
// R = sum_b lens[b] rows mean something, sample b's at rows off[b] .. off[b] + lens[b], off the exclusive prefix sum of lens (the
// feed: feed.store_batches(packed=True); the contract: INTEGRATION.md section 2).  This pass rebuilds
//   out[b, i, :] = packed[off[b] + i, :]   (i <  lens[b])
//   out[b, i, :] = +0.0                    (i >= lens[b])
// in one launch, fp32 -> fp32, bf16 -> bf16, or bf16 -> fp32 widened exactly (the bits of vqa_widen_bf16, which it then replaces).
//
// The prefix sum is a block reduction INSIDE this kernel: every workgroup of sample b sums clamp(lens[0..b)) itself -- thread t takes
// lens[t], lens[t + 256], ... (so B may pass one wave and one workgroup), then 256 partial sums are added in LDS.  That is at most
// B / 256 four-byte loads per thread out of L2 next to a row chunk of tens of KiB, and it needs no workspace, no second launch and
// no host value: the call is one graph node whose grid depends on (B, N, D) alone.
// Every count is clamped to 0..N before it is used, so off[b] + i < B*N for every row that is read, whatever `lens` holds.
#include "common.hpp"

namespace vqa {
namespace {

constexpr int kUnpackThreads = 256;
constexpr int kUnpackTargetWgs = 1024;   // four workgroups per CU of a 256-CU device

__device__ __forceinline__ int clamp_len(int n, int N) { return n < 0 ? 0 : (n > N ? N : n); }

// one unit = 8 consecutive elements of a row: 16 bytes of bf16, 32 bytes of fp32
template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(kUnpackThreads) void unpack_regions_kernel(const void* __restrict__ packed, const int* __restrict__ lens,
                                                                        void* __restrict__ out, int B, int N, int D8, int chunks,
                                                                        int rows_per_chunk) {
  static_assert(IN_BF16 || !OUT_BF16, "fp32 rows are never narrowed here");
  __shared__ int part[kUnpackThreads];
  const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks, t = threadIdx.x;
  int s = 0;
  for (int j = t; j < b; j += kUnpackThreads) s += clamp_len(lens[j], N);
  part[t] = s;
  __syncthreads();
#pragma unroll
  for (int w = kUnpackThreads / 2; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  const size_t off = (size_t)part[0];
  const int len = clamp_len(lens[b], N);
  const int r0 = c * rows_per_chunk;
  const int r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
  const int units = (r1 - r0) * D8;
  for (int u = t; u < units; u += kUnpackThreads) {
    const int i = r0 + u / D8, k = u - (u / D8) * D8;
    const size_t dst = (((size_t)b * N + i) * D8 + k) * 8;      // element index into out
    const size_t src = ((off + i) * D8 + k) * 8;               // element index into packed (read only when i < len)
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;             // (fp32 out: elements 0..3 and 4..7; bf16 out: lo alone)
    if (i < len) {
      if (IN_BF16) {
        const uint4 p = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(packed) + src);
        if (OUT_BF16) {
          lo = p;
        } else {
          lo = make_uint4(p.x << 16, p.x & 0xFFFF0000u, p.y << 16, p.y & 0xFFFF0000u);
          hi = make_uint4(p.z << 16, p.z & 0xFFFF0000u, p.w << 16, p.w & 0xFFFF0000u);
        }
      } else {
        lo = *reinterpret_cast<const uint4*>(static_cast<const float*>(packed) + src);
        hi = *reinterpret_cast<const uint4*>(static_cast<const float*>(packed) + src + 4);
      }
    }
    if (OUT_BF16) {
      *reinterpret_cast<uint4*>(static_cast<uint16_t*>(out) + dst) = lo;
    } else {
      *reinterpret_cast<uint4*>(static_cast<float*>(out) + dst) = lo;
      *reinterpret_cast<uint4*>(static_cast<float*>(out) + dst + 4) = hi;
    }
  }
}

bool unpack_shape_ok(int B, int N, int D) {
  return B > 0 && N > 0 && D > 0 && D % 8 == 0 && (size_t)B * (size_t)N <= 0x7FFFFFFFull;
}

}  // namespace
}  // namespace vqa

extern "C" int vqa_unpack_regions_supported(int B, int N, int D, int in_bf16, int out_bf16) {
  return vqa::unpack_shape_ok(B, N, D) && (in_bf16 != 0 || out_bf16 == 0) ? 1 : 0;
}

extern "C" int vqa_unpack_regions(const void* packed, const int* lens, void* out, int B, int N, int D, int in_bf16, int out_bf16,
                                  vqa_stream_t stream) {
  using namespace vqa;
  VQA_REQUIRE(packed && lens && out, VQA_E_BADARG, "unpack_regions: null pointer");
  VQA_REQUIRE(B > 0 && N > 0 && D > 0, VQA_E_BADARG, "unpack_regions: B = %d, N = %d, D = %d must be positive", B, N, D);
  VQA_REQUIRE(vqa_unpack_regions_supported(B, N, D, in_bf16, out_bf16), VQA_E_UNSUPPORTED,
              "unpack_regions: D = %d must be a multiple of 8, B*N below 2^31, and fp32 rows are not narrowed to bf16", D);
  VQA_REQUIRE(aligned(packed, 16) && aligned(out, 16) && aligned(lens, 16), VQA_E_UNSUPPORTED,
              "unpack_regions: packed, lens and out must be 16-byte aligned");
  // the grid: a function of (B, N, D) alone -- a sample's N rows in `chunks` row chunks, enough of them to fill the device at
  // small batches (B 128 x N 100: 8 chunks of 13 rows; B 512 x N 36: 2 of 18), one chunk once B alone does
  int chunks = (kUnpackTargetWgs + B - 1) / B;
  if (chunks > N) chunks = N;
  const int rows_per_chunk = (N + chunks - 1) / chunks;
  chunks = (N + rows_per_chunk - 1) / rows_per_chunk;
  VQA_REQUIRE((size_t)B * chunks <= 0x7FFFFFFFull, VQA_E_UNSUPPORTED, "unpack_regions: B = %d is too large", B);
  const dim3 grid((unsigned)((size_t)B * chunks)), block(kUnpackThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (in_bf16 && out_bf16)
    VQA_LAUNCH((unpack_regions_kernel<true, true>), grid, block, 0, s, packed, lens, out, B, N, D / 8, chunks, rows_per_chunk);
  else if (in_bf16)
    VQA_LAUNCH((unpack_regions_kernel<true, false>), grid, block, 0, s, packed, lens, out, B, N, D / 8, chunks, rows_per_chunk);
  else
    VQA_LAUNCH((unpack_regions_kernel<false, false>), grid, block, 0, s, packed, lens, out, B, N, D / 8, chunks, rows_per_chunk);
  return check_launch("unpack_regions");
}
