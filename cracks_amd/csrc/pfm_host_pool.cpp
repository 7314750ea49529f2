// pfm_host_pool.cpp -- the worker threads behind pfm_host_pool.h: thread count, three pools kept between calls, and the one
// entry every chunked loop of the context build goes through.  Host only.
#include "pfm_host_pool.h"
#include "pfm_switches.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <mutex>
#include <string>
#include <thread>
#include <pthread.h>

namespace pfm
{
  // Host threads for the O(n_nodes) / O(n_cells) loops of the context build (setup_system of the reference runs them
  // after every refine_mesh, cracks.cc:4148): the cores this process may use (affinity mask, cgroup quota), at most 32.
  int host_threads()
  {
    static int n = 0;
    if (n)
      return n;
    unsigned hc = std::thread::hardware_concurrency();
    int t = hc ? (int)hc : 1;
    std::ifstream f("/sys/fs/cgroup/cpu.max");
    std::string q;
    double per = 0;
    if (f >> q >> per && q != "max" && per > 0)
      t = std::min(t, std::max(1, (int)(std::stod(q) / per)));
    if (switches().host_threads)
      t = switches().host_threads;
    n = std::max(1, std::min(t, 32));
    return n;
  }

  namespace
  {
    // Worker threads of the context build, kept between calls: a rebuild at 2.7e5 cells runs some twenty parallel loops of
    // 20-200 us each, and starting 16 threads costs more than such a loop.  One parallel region at a time (a second caller --
    // the colour and overlay threads of pfm_ctx_create run next to the main thread -- starts its own threads as before).
    // A forked child has none of the parent's threads: it starts over with an empty pool (pthread_atfork).
    struct HostPool
    {
      std::mutex mx, region;
      std::condition_variable cv, cv_done;
      std::vector<std::thread> th;
      const std::function<void(int)> *job = nullptr;
      std::atomic<uint64_t> gen{0};
      std::atomic<int> left{0};
      int want = 0;
      std::atomic<bool> stop{false};

      // the loops of a rebuild follow one another within microseconds: a worker (and the caller, for the end of a region) polls
      // for ~50 us before it sleeps on the condition variable (a sleep and a wake-up cost 30-50 us each with 16 threads)
      static bool spin_until(const std::function<bool()> &ready)
      {
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0;; ++i)
          {
            if (ready())
              return true;
            __builtin_ia32_pause();
            if ((i & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(50))
              return false;
          }
      }
      void worker(int id, uint64_t seen) // seen: the generation at the worker's creation (it answers the ones after it)
      {
        for (;;)
          {
            if (!spin_until([&] { return stop.load(std::memory_order_acquire) || gen.load(std::memory_order_acquire) != seen; }))
              {
                std::unique_lock<std::mutex> lk(mx);
                cv.wait(lk, [&] { return stop.load() || gen.load() != seen; });
              }
            if (stop.load())
              return;
            seen = gen.load(std::memory_order_acquire);
            // EVERY worker answers every region (those beyond `want` without running anything): want and job are then never
            // rewritten while a worker may still read them
            if (id < want)
              (*job)(id);
            if (left.fetch_sub(1, std::memory_order_acq_rel) == 1)
              {
                std::lock_guard<std::mutex> lk(mx);
                cv_done.notify_one();
              }
          }
      }
      // f(t) for t = 0 .. nt-1, t = 0 on the calling thread; false when the pool is taken (caller falls back)
      bool run(int nt, const std::function<void(int)> &f)
      {
        std::unique_lock<std::mutex> reg(region, std::try_to_lock);
        if (!reg.owns_lock())
          return false;
        while ((int)th.size() + 1 < nt)
          {
            const int id = (int)th.size() + 1;
            const uint64_t born = gen.load(std::memory_order_acquire);
            th.emplace_back([this, id, born] { worker(id, born); });
          }
        job = &f;
        want = nt;
        left.store((int)th.size(), std::memory_order_relaxed);
        gen.fetch_add(1, std::memory_order_release);
        {
          std::lock_guard<std::mutex> lk(mx); // a worker is either before its look at gen or asleep and notified below
        }
        cv.notify_all();
        f(0);
        if (!spin_until([&] { return left.load(std::memory_order_acquire) == 0; }))
          {
            std::unique_lock<std::mutex> lk(mx);
            cv_done.wait(lk, [&] { return left.load() == 0; });
          }
        job = nullptr;
        return true;
      }
      ~HostPool()
      {
        stop.store(true);
        {
          std::lock_guard<std::mutex> lk(mx);
        }
        cv.notify_all();
        for (auto &t : th)
          t.join();
      }
    };
    // Three pools: pfm_ctx_create classifies the cells (overlay) and colours them on two threads next to the one that uploads;
    // each takes the first pool that is free.
    constexpr int N_POOLS = 3;
    std::atomic<HostPool *> g_pools{nullptr};
    HostPool *host_pools()
    {
      HostPool *p = g_pools.load(std::memory_order_acquire);
      if (p)
        return p;
      static std::mutex mk;
      std::lock_guard<std::mutex> lk(mk);
      p = g_pools.load(std::memory_order_acquire);
      if (!p)
        {
          static bool hooked = false;
          if (!hooked)
            {
              hooked = true;
              pthread_atfork(nullptr, nullptr, [] { g_pools.store(nullptr, std::memory_order_release); }); // the child's copy is leaked
              atexit([] { delete[] g_pools.exchange(nullptr); });
            }
          p = new HostPool[N_POOLS];
          g_pools.store(p, std::memory_order_release);
        }
      return p;
    }
  } // namespace

  void run_chunks(int nt, const std::function<void(int)> &fn)
  {
    std::vector<std::exception_ptr> err((size_t)nt);
    const std::function<void(int)> body = [&fn, &err](int t) {
      try
        {
          fn(t);
        }
      catch (...)
        {
          err[(size_t)t] = std::current_exception();
        }
    };
    HostPool *pools = host_pools();
    bool done = false;
    for (int q = 0; q < N_POOLS && !done; ++q)
      done = pools[q].run(nt, body);
    if (!done)
      {
        std::vector<std::thread> th;
        th.reserve(nt);
        for (int t = 1; t < nt; ++t)
          th.emplace_back([&body, t] { body(t); });
        body(0);
        for (auto &x : th)
          x.join();
      }
    for (auto &e : err)
      if (e)
        std::rethrow_exception(e);
  }
  int chunks_for(int64_t n, int64_t grain) { return (int)std::min<int64_t>(host_threads(), std::max<int64_t>(1, n / std::max<int64_t>(grain, 1))); }
} // namespace pfm
