// pfm_delta_host.h -- host side of the packed path of pfm_values_to_host_delta (pfm_delta.hip): the changed chunks of a slab
// arrive in page-locked staging as an index list and a dense payload, and are copied to their places in the caller's value
// array.  Plain C++17, no HIP include: tests/cpp/delta_scatter_main.cpp compiles it on its own.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace pfm
{
  // host threads of the scatter: PFM_HOST_THREADS if set, else the hardware's, at most 16
  inline int delta_host_threads()
  {
    int t = (int)std::thread::hardware_concurrency();
    if (const char *e = std::getenv("PFM_HOST_THREADS"))
      t = std::atoi(e);
    return std::max(1, std::min(t, 16));
  }

  // Chunk list[i] of the slab (numbered from its first chunk, first_chunk of the block) <- payload chunk i, i < count:
  // dst[(first_chunk + list[i]) * chunk_doubles ...], clamped to the block's length block_len (the tail chunk of a block is
  // shorter).  dst and payload need 8-byte alignment only.  The chunks are split evenly over at most n_threads threads (the
  // caller's among them); a thread is only worth starting for min_bytes_per_thread of payload.
  inline void delta_scatter(double *dst, int64_t block_len, int64_t chunk_doubles, int64_t first_chunk, const uint32_t *list,
                            int64_t count, const double *payload, int n_threads, int64_t min_bytes_per_thread = 1 << 20)
  {
    if (count <= 0)
      return;
    const int64_t per = std::max<int64_t>(1, min_bytes_per_thread / (chunk_doubles * (int64_t)sizeof(double)));
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_threads, 16), count / per));
    auto work = [=](int t) {
      for (int64_t i = count * t / nt, e = count * (t + 1) / nt; i < e; ++i)
        {
          const int64_t at = (first_chunk + (int64_t)list[i]) * chunk_doubles;
          const int64_t n = std::min(chunk_doubles, block_len - at);
          if (n > 0)
            std::memcpy(dst + at, payload + i * chunk_doubles, (size_t)n * sizeof(double));
        }
    };
    std::vector<std::thread> th;
    th.reserve((size_t)nt - 1);
    for (int t = 1; t < nt; ++t)
      th.emplace_back(work, t);
    work(0);
    for (auto &x : th)
      x.join();
  }
} // namespace pfm
