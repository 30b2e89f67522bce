// Host side of the feed (no device code): the per-sample row gather of the reference's loader -- `outer.data['img']['feature'][visual_index]`
// once per sample in Inner.__getitem__ (datasets.py:912-913), collated by the DataLoader's worker processes (:975-977) -- as ONE call
// that copies the batch's rows from the memory-mapped feature store into the (pinned) staging tensor on a few threads, optionally
// rounding them to bf16 (round to nearest even; the transport format of feed.store_batches(region_dtype=bfloat16)).
// Why native: from Python the same gather is one numpy.take per worker thread, and every one of those calls takes and returns the GIL --
// next to a training loop that holds it for milliseconds at a time, a 16-thread gather of 151 MB took 9-19 ms per batch instead of the
// 2-3 ms the copies need (tools/feed_bench.py --store).  A ctypes call drops the GIL once for the whole batch.
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "common.hpp"

namespace {
inline uint16_t bf16_rne(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);   // NaN stays a (quiet) NaN
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
}  // namespace

extern "C" int vqa_host_gather_rows(const float* store, long store_rows, long row_floats, const long* idx, int n, void* out,
                                    int out_bf16, int threads) {
  VQA_REQUIRE(store && idx && out, VQA_E_BADARG, "host_gather_rows: null pointer");
  VQA_REQUIRE(store_rows > 0 && row_floats > 0 && n >= 0, VQA_E_BADARG, "host_gather_rows: bad sizes");
  for (int r = 0; r < n; ++r)
    VQA_REQUIRE(idx[r] >= 0 && idx[r] < store_rows, VQA_E_BADARG, "host_gather_rows: index %ld outside [0, %ld)", idx[r], store_rows);
  if (n == 0) return VQA_OK;
  int nt = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
  if (nt > n) nt = n;
  auto work = [=](int lo, int hi) {
    for (int r = lo; r < hi; ++r) {
      const float* src = store + (size_t)idx[r] * row_floats;
      if (out_bf16) {
        uint16_t* dst = static_cast<uint16_t*>(out) + (size_t)r * row_floats;
        for (long k = 0; k < row_floats; ++k) dst[k] = bf16_rne(src[k]);
      } else {
        std::memcpy(static_cast<float*>(out) + (size_t)r * row_floats, src, (size_t)row_floats * 4);
      }
    }
  };
  const int per = (n + nt - 1) / nt;
  std::vector<std::thread> pool;
  pool.reserve(nt);
  for (int t = 1; t < nt; ++t) pool.emplace_back(work, t * per, (t + 1) * per < n ? (t + 1) * per : n);
  work(0, per < n ? per : n);
  for (auto& th : pool) th.join();
  return VQA_OK;
}

// The ragged form (packed region batches, feed.FeatureStore.gather_packed): image idx[r] contributes its rows starts[idx[r]] ..
// starts[idx[r]] + counts[idx[r]] of the [store_rows, row_floats] array, and the batch's rows land back to back in `out`
// (capacity_rows rows): the destination prefix sum is computed once, here, and the copy is split over the threads by BYTES (equal
// shares of the R destination rows, wherever the image borders fall), not by image -- counts differ tenfold.  v_len_out[r] =
// counts[idx[r]], *total_rows = R.  Everything the call reads is range-checked before a byte is copied: the indices, every selected
// image's row range against the store, and R against the capacity.  Rows of `out` from R on are left as they are.
extern "C" int vqa_host_gather_ragged(const float* store, long store_rows, long row_floats, const long* starts, const int* counts,
                                      long n_img, const long* idx, int n, void* out, long capacity_rows, int* v_len_out,
                                      long* total_rows, int out_bf16, int threads) {
  VQA_REQUIRE(store && starts && counts && idx && out && v_len_out && total_rows, VQA_E_BADARG, "host_gather_ragged: null pointer");
  VQA_REQUIRE(store_rows > 0 && row_floats > 0 && n_img > 0 && n >= 0 && capacity_rows >= 0, VQA_E_BADARG,
              "host_gather_ragged: bad sizes");
  std::vector<long> dst((size_t)n + 1, 0);
  for (int r = 0; r < n; ++r) {
    VQA_REQUIRE(idx[r] >= 0 && idx[r] < n_img, VQA_E_BADARG, "host_gather_ragged: index %ld outside [0, %ld)", idx[r], n_img);
    const long s = starts[idx[r]], c = counts[idx[r]];
    VQA_REQUIRE(c >= 0 && s >= 0 && s <= store_rows && c <= store_rows - s, VQA_E_BADARG,
                "host_gather_ragged: image %ld holds rows %ld .. %ld + %ld of a store of %ld", idx[r], s, s, c, store_rows);
    dst[r + 1] = dst[r] + c;
    VQA_REQUIRE(dst[r + 1] <= capacity_rows, VQA_E_BADARG, "host_gather_ragged: the batch's rows pass the buffer's %ld", capacity_rows);
  }
  const long R = dst[n];
  for (int r = 0; r < n; ++r) v_len_out[r] = counts[idx[r]];
  *total_rows = R;
  if (R == 0) return VQA_OK;
  long nt = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
  if (nt > R) nt = R;
  auto work = [&dst, store, starts, idx, out, out_bf16, row_floats](long lo, long hi) {   // destination rows [lo, hi)
    int r = (int)(std::upper_bound(dst.begin(), dst.end(), lo) - dst.begin()) - 1;           // the image that holds row lo
    while (lo < hi) {
      while (dst[r + 1] <= lo) ++r;                                                           // (images without rows)
      const long end = dst[r + 1] < hi ? dst[r + 1] : hi;
      const float* src = store + (size_t)(starts[idx[r]] + (lo - dst[r])) * row_floats;
      const size_t count = (size_t)(end - lo) * row_floats;
      if (out_bf16) {
        uint16_t* d = static_cast<uint16_t*>(out) + (size_t)lo * row_floats;
        for (size_t k = 0; k < count; ++k) d[k] = bf16_rne(src[k]);
      } else {
        std::memcpy(static_cast<float*>(out) + (size_t)lo * row_floats, src, count * 4);
      }
      lo = end;
    }
  };
  std::vector<std::thread> pool;
  pool.reserve((size_t)nt);
  for (long t = 1; t < nt; ++t) pool.emplace_back(work, R * t / nt, R * (t + 1) / nt);
  work(0, R / nt);
  for (auto& th : pool) th.join();
  return VQA_OK;
}
