// pfm_host_pool.h -- the host threads of the context build: a pool of workers kept between calls (pfm_host_pool.cpp) and the
// chunked loops on top of it.  No HIP include; the pool state exists once in the library, the templates here only wrap the
// caller's loop body for the one non-template entry (run_chunks).
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

namespace pfm
{
  // the cores this process may use (affinity mask, cgroup quota, PFM_HOST_THREADS), at most 32; read once per process
  int host_threads();
  // chunks of a loop over n items with at least `grain` items each, at most host_threads()
  int chunks_for(int64_t n, int64_t grain);
  // body(t) for t = 0 .. nt-1 on nt threads (t = 0 on the caller's), nt >= 2; an exception of a chunk is rethrown here
  void run_chunks(int nt, const std::function<void(int)> &body);

  // fn(begin, end) over [0, n) in contiguous chunks, one per thread (at least `grain` items per thread).  An exception
  // thrown by a worker (bad_alloc in a lambda that grows a vector) is carried to the caller instead of ending the
  // process in std::terminate.  parallel_chunks: the same with the chunk index, for loops that keep per-chunk results.
  template <class F>
  void parallel_chunks(int nt, F &&fn)
  {
    if (nt <= 1)
      {
        fn(0);
        return;
      }
    run_chunks(nt, std::function<void(int)>(std::ref(fn)));
  }
  template <class F>
  void parallel_for(int64_t n, F &&fn, int64_t grain = 16384)
  {
    const int nt = chunks_for(n, grain);
    if (nt <= 1)
      {
        fn((int64_t)0, n);
        return;
      }
    parallel_chunks(nt, [&fn, n, nt](int t) { fn(n * t / nt, n * (t + 1) / nt); });
  }

  // a[i] += a[i-1] ... in place (row pointers of 1e7 rows: 24 ms on one core)
  template <class T>
  void inclusive_scan_parallel(T *a, int64_t n)
  {
    const int nt = chunks_for(n, 65536);
    if (nt <= 1)
      {
        for (int64_t i = 1; i < n; ++i)
          a[i] += a[i - 1];
        return;
      }
    std::vector<T> tot((size_t)nt);
    parallel_chunks(nt, [&](int t) {
      const int64_t b = n * t / nt, e = n * (t + 1) / nt;
      T s = 0;
      for (int64_t i = b; i < e; ++i)
        {
          s += a[i];
          a[i] = s;
        }
      tot[(size_t)t] = s;
    });
    T run = 0;
    for (int t = 0; t < nt; ++t)
      {
        const T x = tot[(size_t)t];
        tot[(size_t)t] = run;
        run += x;
      }
    parallel_chunks(nt, [&](int t) {
      const T off = tot[(size_t)t];
      if (off == 0)
        return;
      const int64_t b = n * t / nt, e = n * (t + 1) / nt;
      for (int64_t i = b; i < e; ++i)
        a[i] += off;
    });
  }

  // indices i of [b, e) with pred(i), ascending (chunked over the host threads)
  template <class P>
  std::vector<int32_t> parallel_select(int64_t b, int64_t e, P &&pred)
  {
    const int64_t n = e - b;
    const int nt = chunks_for(n, 16384);
    std::vector<std::vector<int32_t>> part((size_t)nt);
    parallel_chunks(nt, [&](int t) {
      std::vector<int32_t> &out = part[(size_t)t];
      for (int64_t i = b + n * t / nt; i < b + n * (t + 1) / nt; ++i)
        if (pred(i))
          out.push_back((int32_t)i);
    });
    if (nt == 1)
      return std::move(part[0]);
    size_t total = 0;
    for (auto &q : part)
      total += q.size();
    std::vector<int32_t> out;
    out.reserve(total);
    for (auto &q : part)
      out.insert(out.end(), q.begin(), q.end());
    return out;
  }
} // namespace pfm
