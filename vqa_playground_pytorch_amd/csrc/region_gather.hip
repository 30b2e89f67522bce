// Device-resident region store -> the padded [B,N,D] tensor every region-side kernel reads.
//
// The store lives in HBM once: rows [total_rows, D], fp32 or bf16, image i's rows at starts[i] .. starts[i] + counts[i] (a padded
// store: starts[i] = i*N; a ragged one: its offsets; counts == NULL: every image has N rows).  A batch is B image indices
// (feed.DeviceFeatureStore, feed.store_batches(resident=); the contract: INTEGRATION.md section 2).  This pass rebuilds
//   out[b, r, :] = rows[starts[i] + r, :]   (r <  c)          i = clamp(idx[b], 0, n_img - 1)
//   out[b, r, :] = +0.0                     (r >= c)          c = clamp(counts[i], 0, N)
// in one launch, fp32 -> fp32, bf16 -> bf16, or bf16 -> fp32 widened exactly (the bits of vqa_widen_bf16): the forms and the
// chunking of a sample's rows are region_unpack.hip's, the source row comes from the index instead of a prefix sum.  idx[b], starts[i] and counts[i] depend on blockIdx alone: the compiler reads them with scalar loads into SGPRs, the row
// loads and stores are plain per-lane global accesses of 16 bytes, and no descriptor is built from them (no waterfall loop).
// The index and the count are clamped HERE, whatever the device tensors hold; that starts[i] + counts[i] <= total_rows for every
// image is the store's invariant, checked once on the host when it is built (feed.DeviceFeatureStore), and relied on.
#include "common.hpp"

namespace vqa {
namespace {

constexpr int kGatherThreads = 256;
constexpr int kGatherTargetWgs = 1024;   // four workgroups per CU of a 256-CU device
constexpr int kGatherUnroll = 4;         // units per thread and pass: 4 16-byte loads in flight ahead of the stores

// One unit = 16 bytes of a store row: 8 bf16 or 4 fp32 elements; consecutive lanes take consecutive units, so every load and
// every copying store of a wave covers 1 KiB without a gap.  WIDEN = false copies a unit as it is (fp32 -> fp32 and bf16 -> bf16
// are the same kernel; the row is `upr` units long); WIDEN = true turns the unit's 8 bf16 into 8 fp32, two 16-byte stores.
template <bool WIDEN>
__device__ __forceinline__ void store_unit(uint4* __restrict__ out, size_t dst, const uint4 p) {
  if (WIDEN) {                                                    // widened exactly: the bf16 bits are the upper half of the fp32
    out[2 * dst] = make_uint4(p.x << 16, p.x & 0xFFFF0000u, p.y << 16, p.y & 0xFFFF0000u);
    out[2 * dst + 1] = make_uint4(p.z << 16, p.z & 0xFFFF0000u, p.w << 16, p.w & 0xFFFF0000u);
  } else {
    out[dst] = p;
  }
}

template <bool WIDEN>
__global__ __launch_bounds__(kGatherThreads) void gather_regions_kernel(const uint4* __restrict__ rows, const long* __restrict__ starts,
                                                                        const int* __restrict__ counts, int n_img,
                                                                        const int* __restrict__ idx, uint4* __restrict__ out,
                                                                        int* __restrict__ v_len_out, int N, int upr, int chunks,
                                                                        int rows_per_chunk) {
  constexpr int T = kGatherThreads, U = kGatherUnroll;
  const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks, t = threadIdx.x;
  int i = idx[b];                                               // blockIdx-uniform: scalar loads, SGPR values
  i = i < 0 ? 0 : (i >= n_img ? n_img - 1 : i);
  int len = counts ? counts[i] : N;
  len = len < 0 ? 0 : (len > N ? N : len);
  const size_t first = (size_t)starts[i];
  if (v_len_out && c == 0 && t == 0) v_len_out[b] = len;
  const int r0 = c * rows_per_chunk;
  const int r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
  const int units = (r1 - r0) * upr;
  const int real_units = len > r0 ? ((len < r1 ? len : r1) - r0) * upr : 0;   // the chunk's units that come from the store
  // a chunk's rows are consecutive in the store and in out: unit u of the chunk is u units behind either start
  const uint4* __restrict__ src = rows + (first + r0) * (size_t)upr;          // the chunk's first source row (read when real)
  const size_t dst0 = ((size_t)b * N + r0) * (size_t)upr;                     // the chunk's first output row, in source units
  // the real units, U per thread and pass: the loads of pass p + 1 are issued before the stores of pass p wait for theirs
  int u = t;
  if (u + (U - 1) * T < real_units) {
    uint4 cur[U], nxt[U];
#pragma unroll
    for (int k = 0; k < U; ++k) cur[k] = src[u + k * T];
    for (; u + (2 * U - 1) * T < real_units; u += U * T) {
#pragma unroll
      for (int k = 0; k < U; ++k) nxt[k] = src[u + (U + k) * T];
#pragma unroll
      for (int k = 0; k < U; ++k) store_unit<WIDEN>(out, dst0 + u + k * T, cur[k]);
#pragma unroll
      for (int k = 0; k < U; ++k) cur[k] = nxt[k];
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_unit<WIDEN>(out, dst0 + u + k * T, cur[k]);
    u += U * T;
  }
  for (; u < real_units; u += T) store_unit<WIDEN>(out, dst0 + u, src[u]);    // fewer than U passes left
  // the padding: exact +0.0 (real_units is a multiple of upr, so u starts at the thread's own first unit behind the real rows)
  for (u = real_units + t; u < units; u += T) store_unit<WIDEN>(out, dst0 + u, make_uint4(0u, 0u, 0u, 0u));
}

bool gather_shape_ok(int B, int N, int D) {
  return B > 0 && N > 0 && D > 0 && D % 8 == 0 && (size_t)B * (size_t)N <= 0x7FFFFFFFull;
}

}  // namespace
}  // namespace vqa

extern "C" int vqa_gather_regions_supported(int B, int N, int D, int in_bf16, int out_bf16) {
  return vqa::gather_shape_ok(B, N, D) && (in_bf16 != 0 || out_bf16 == 0) ? 1 : 0;
}

extern "C" int vqa_gather_regions(const void* rows, long total_rows, const long* starts, const int* counts, int n_img, const int* idx,
                                  void* out, int* v_len_out, int B, int N, int D, int in_bf16, int out_bf16, vqa_stream_t stream) {
  using namespace vqa;
  VQA_REQUIRE(rows && starts && idx && out, VQA_E_BADARG, "gather_regions: null pointer");
  VQA_REQUIRE(B > 0 && N > 0 && D > 0 && n_img > 0 && total_rows > 0, VQA_E_BADARG,
              "gather_regions: B = %d, N = %d, D = %d, n_img = %d, total_rows = %ld must be positive", B, N, D, n_img, total_rows);
  VQA_REQUIRE(vqa_gather_regions_supported(B, N, D, in_bf16, out_bf16), VQA_E_UNSUPPORTED,
              "gather_regions: D = %d must be a multiple of 8, B*N below 2^31, and fp32 rows are not narrowed to bf16", D);
  VQA_REQUIRE(aligned(rows, 16) && aligned(starts, 16) && aligned(idx, 16) && aligned(out, 16) && (!counts || aligned(counts, 16)) &&
                  (!v_len_out || aligned(v_len_out, 16)),
              VQA_E_UNSUPPORTED, "gather_regions: rows, starts, counts, idx, out and v_len_out must be 16-byte aligned");
  // the grid: region_unpack.hip's, a function of (B, N, D) alone -- a sample's N rows in `chunks` row chunks, enough of them to
  // fill the device at small batches, one chunk once B alone does
  int chunks = (kGatherTargetWgs + B - 1) / B;
  if (chunks > N) chunks = N;
  const int rows_per_chunk = (N + chunks - 1) / chunks;
  chunks = (N + rows_per_chunk - 1) / rows_per_chunk;
  VQA_REQUIRE((size_t)B * chunks <= 0x7FFFFFFFull, VQA_E_UNSUPPORTED, "gather_regions: B = %d is too large", B);
  const dim3 grid((unsigned)((size_t)B * chunks)), block(kGatherThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint4* src = static_cast<const uint4*>(rows);
  uint4* dst = static_cast<uint4*>(out);
  if (in_bf16 && !out_bf16)
    VQA_LAUNCH((gather_regions_kernel<true>), grid, block, 0, s, src, starts, counts, n_img, idx, dst, v_len_out, N, D / 8, chunks, rows_per_chunk);
  else          // a copy of 16-byte units: D / 8 of them in a bf16 row, D / 4 in an fp32 row
    VQA_LAUNCH((gather_regions_kernel<false>), grid, block, 0, s, src, starts, counts, n_img, idx, dst, v_len_out, N, in_bf16 ? D / 8 : D / 4,
               chunks, rows_per_chunk);
  return check_launch("gather_regions");
}
