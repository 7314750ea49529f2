// pfm_transfer.cpp -- copies between the device and memory the CALLER owns (include/pfm_assemble.h): the two pinned
// staging buffers per device and the copies through them (h2d, d2h_staged), the choice between them and a DMA from
// page-locked memory (h2d_user, d2h_user, pfm_host_register / _unregister), the matrix values on their way to the host
// (pfm_values_to_host) and the synchronous host-pointer entry pfm_assemble.
#include "pfm_host.h"
#include "pfm_host_pool.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace pfm;

namespace
{
  thread_local int g_h2d_batch = 0; // the H2dBatch scopes the calling thread is inside (h2d)
  struct Stage // two pinned buffers per device: the events belong to the device that was current when they were made
  {
    static constexpr size_t CHUNK = 32u << 20;
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    int next = 0;
    bool ok = false, tried = false;
    ~Stage()
    {
      for (int i = 0; i < 2; ++i)
        {
          if (pending[i])
            (void)hipEventSynchronize(ev[i]);
          if (buf[i])
            (void)hipHostFree(buf[i]);
          if (ev[i])
            (void)hipEventDestroy(ev[i]);
        }
    }
  };
  std::mutex g_stage_mx; // one transfer at a time goes through the staging buffers (pfm_ctx_create uploads on a second thread)
  Stage g_stages[16];
  Stage *stage_of_current_device() // call with g_stage_mx held; nullptr: no pinned memory to be had
  {
    int dev = 0;
    (void)hipGetDevice(&dev);
    Stage &st = g_stages[dev & 15];
    if (!st.tried)
      {
        st.tried = true;
        st.ok = hipHostMalloc(&st.buf[0], Stage::CHUNK, hipHostMallocPortable) == hipSuccess &&
                hipHostMalloc(&st.buf[1], Stage::CHUNK, hipHostMallocPortable) == hipSuccess &&
                hipEventCreateWithFlags(&st.ev[0], hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&st.ev[1], hipEventDisableTiming) == hipSuccess;
      }
    return st.ok ? &st : nullptr;
  }

  // Device -> host copy into pageable memory of the caller through the same buffers, ordered behind the work on `s`,
  // complete on return (results the host reads right after a call: residual vectors, small matrices).
  hipError_t d2h_staged(void *h, const void *d, size_t bytes, hipStream_t s)
  {
    std::lock_guard<std::mutex> stage_lock(g_stage_mx);
    Stage *stp = stage_of_current_device();
    if (!stp)
      {
        const hipError_t e = hipStreamSynchronize(s);
        return e != hipSuccess ? e : hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost);
      }
    Stage &st = *stp;
    for (int k = 0; k < 2; ++k)
      if (st.pending[k])
        {
          st.pending[k] = false;
          const hipError_t e = hipEventSynchronize(st.ev[k]);
          if (e != hipSuccess)
            return e;
        }
    const size_t piece = Stage::CHUNK;
    size_t prev_off = 0, prev_nb = 0;
    int prev_k = -1;
    auto land = [&]() -> hipError_t { // the previous piece: wait for it, hand it to the caller's buffer
      if (prev_k < 0)
        return hipSuccess;
      const hipError_t e = hipEventSynchronize(st.ev[prev_k]);
      if (e != hipSuccess)
        return e;
      const char *src = static_cast<const char *>(st.buf[prev_k]);
      char *dst = static_cast<char *>(h) + prev_off;
      parallel_for((int64_t)prev_nb, [&](int64_t b, int64_t e2) { memcpy(dst + b, src + b, (size_t)(e2 - b)); }, 1 << 18);
      prev_k = -1;
      return hipSuccess;
    };
    for (size_t off = 0; off < bytes; off += piece)
      {
        const int k = st.next;
        st.next ^= 1;
        const size_t nb = std::min(piece, bytes - off);
        hipError_t e = hipMemcpyAsync(st.buf[k], static_cast<const char *>(d) + off, nb, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
          e = hipEventRecord(st.ev[k], s);
        if (e == hipSuccess)
          e = land();
        if (e != hipSuccess)
          return e;
        prev_k = k, prev_off = off, prev_nb = nb;
      }
    return land();
  }

  pfm_ctx::HostPin *find_pin(pfm_ctx *c, const void *p, size_t bytes)
  {
    for (auto &hp : c->host_pins)
      if (hp.p == p && hp.bytes >= bytes)
        return &hp;
    return nullptr;
  }

  // The other direction.  Page-locked: asynchronous on `s`.  Pageable and up to 64 MB (glibc serves such blocks from the
  // heap, where registered pages may have lived): through the staging buffers, complete on return.  Larger pageable arrays
  // (always mappings of their own) take the runtime's path.
  hipError_t d2h_user(pfm_ctx *c, void *h, const void *d, size_t bytes, hipStream_t s)
  {
    if (bytes == 0)
      return hipSuccess;
    if (find_pin(c, h, bytes) || bytes > ((size_t)64 << 20))
      return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s);
    return d2h_staged(h, d, bytes, s);
  }

  // matrix values of the last pfm_assemble_device -> the host's arrays, asynchronously: block 0 on the context's stream,
  // the phase-field blocks on a second stream (joined into the first before returning).  Does not synchronise.
  int values_to_host_async(pfm_ctx *c, double *const *d_values, double *const *h_values)
  {
    (void)hipSetDevice(c->device);
    if (!c->copy_stream)
      {
        if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "copy stream");
      }
    for (int b = 0; b < c->n_blocks; ++b) // (checked before the fork: no exit path leaves copy_stream unjoined)
      if (c->block_nnz(b) > 0 && (!h_values[b] || !d_values[b]))
        return fail(c, PFM_ERR_BAD_ARG, "pfm_values_to_host: null block");
    hipError_t e = hipEventRecord(c->ev_copy, c->stream);
    if (e == hipSuccess)
      e = hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0);
    for (int b = 0; b < c->n_blocks && e == hipSuccess; ++b)
      {
        const size_t bytes = sizeof(double) * (size_t)c->block_nnz(b);
        if (!bytes)
          continue;
        if (c->n_blocks == 4 && b == 1)
          {
            // (u,phi) = 0.  A registered array is ours between the calls (nobody else writes the matrix: the reference only
            // ever fills it through assemble_system): cleared once, by host threads next to the transfers, never copied.
            // An unregistered one is copied like the others (the device block holds the zeros the kernels wrote).
            pfm_ctx::HostPin *hp = find_pin(c, h_values[b], bytes);
            if (hp)
              {
                if (!hp->zeroed)
                  {
                    const int nt = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
                    std::vector<std::thread> th;
                    const size_t chunk = ((bytes / (size_t)nt) + 4095) & ~(size_t)4095;
                    for (int t = 0; t < nt; ++t)
                      {
                        const size_t lo = std::min(bytes, (size_t)t * chunk), hi = std::min(bytes, lo + chunk);
                        if (hi > lo)
                          th.emplace_back([=] { std::memset(reinterpret_cast<char *>(h_values[b]) + lo, 0, hi - lo); });
                      }
                    for (auto &t : th)
                      t.join();
                    hp->zeroed = true;
                  }
                continue;
              }
          }
        e = d2h_user(c, h_values[b], d_values[b], bytes, b == 0 ? c->stream : c->copy_stream);
      }
    if (e == hipSuccess)
      e = hipEventRecord(c->ev_copy, c->copy_stream);
    if (e == hipSuccess)
      e = hipStreamWaitEvent(c->stream, c->ev_copy, 0);
    return e == hipSuccess ? PFM_OK : hipfail(c, e, "copy back (matrix values)");
  }
} // namespace

namespace pfm
{
  H2dBatch::H2dBatch() { ++g_h2d_batch; }
  H2dBatch::~H2dBatch() { --g_h2d_batch; }

  // Host -> device copy of caller-owned (pageable) memory.  hipMemcpy from pageable memory ran at ~3.6 GB/s on the
  // test box; tables from 256 KB go through two pinned staging buffers filled by the host threads (parallel memcpy) while
  // the previous piece is on the bus.  On return the caller's buffer has been read.  The copy itself is complete as well,
  // unless the calling thread is inside an H2dBatch scope (pfm_ctx_create: some twenty uploads, one synchronisation at the
  // end, 0.1-0.3 ms each otherwise): then it is ordered on the null stream like a hipMemcpyAsync from pinned memory.
  hipError_t h2d(void *d, const void *h, size_t bytes)
  {
    if (bytes < (256u << 10))
      return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    std::lock_guard<std::mutex> stage_lock(g_stage_mx);
    Stage *stp = stage_of_current_device();
    if (!stp)
      return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    Stage &st = *stp;
    // pieces: a table of a few MB in two halves (the second is copied to the staging buffer while the first is on the bus)
    const size_t piece = bytes <= (1u << 20) ? bytes : std::min(Stage::CHUNK, ((bytes + 1) / 2 + 4095) & ~(size_t)4095);
    for (size_t off = 0; off < bytes; off += piece)
      {
        const int k = st.next;
        st.next ^= 1;
        const size_t nb = std::min(piece, bytes - off);
        if (st.pending[k])
          {
            st.pending[k] = false;
            const hipError_t e = hipEventSynchronize(st.ev[k]);
            if (e != hipSuccess)
              return e;
          }
        const char *src = static_cast<const char *>(h) + off;
        char *dst = static_cast<char *>(st.buf[k]);
        parallel_for((int64_t)nb, [&](int64_t b, int64_t e) { memcpy(dst + b, src + b, (size_t)(e - b)); }, 1 << 18);
        hipError_t e = hipMemcpyAsync(static_cast<char *>(d) + off, st.buf[k], nb, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess)
          e = hipEventRecord(st.ev[k], nullptr);
        if (e != hipSuccess)
          return e;
        st.pending[k] = true;
      }
    return g_h2d_batch > 0 ? hipSuccess : hipStreamSynchronize(nullptr);
  }

  // Host -> device copy of a buffer the CALLER owns.  Page-locked through pfm_host_register: an asynchronous DMA on `s`.
  // Anything else goes through the library's own staging buffers (h2d) and is complete on return: the runtime's path for
  // pageable memory pins the caller's pages on the fly, and on this stack that faulted intermittently ("Memory access fault by
  // GPU ... on address <host heap>") when such pages had been registered and unregistered before (tests/test_gpu_cart.py's
  // host-pointer cases followed by the 216^3 test).
  hipError_t h2d_user(pfm_ctx *c, void *d, const void *h, size_t bytes, hipStream_t s)
  {
    if (bytes == 0)
      return hipSuccess;
    if (find_pin(c, h, bytes))
      return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s);
    // the staged copy runs on the NULL stream, which does not order itself behind a hipStreamNonBlocking stream installed
    // through pfm_ctx_set_stream (torch side streams are of that kind): kernels still queued on `s` may read what this copy
    // overwrites (node_flags of an assembly in flight, the staging vectors of the last state) -- wait for them first
    const hipError_t es = hipStreamSynchronize(s);
    if (es != hipSuccess)
      return es;
    return h2d(d, h, bytes);
  }

  // d2h_user for a piece [h, h + bytes) of an array: page-locked if it lies inside a registered array
  hipError_t d2h_user_piece(pfm_ctx *c, void *h, const void *d, size_t bytes, hipStream_t s)
  {
    if (bytes == 0)
      return hipSuccess;
    const char *lo = static_cast<const char *>(h);
    for (const auto &hp : c->host_pins)
      if (lo >= static_cast<const char *>(hp.p) && lo + bytes <= static_cast<const char *>(hp.p) + hp.bytes)
        return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s);
    return d2h_user(c, h, d, bytes, s);
  }
} // namespace pfm

extern "C"
{
  // ---- host-visible outputs (the caller hands system_pde_matrix to Trilinos right after the call,
  // cracks.cc:2754, 2770, 2918).  35 GB of matrix values cross PCIe per Jacobian at 216^3: what can be done about that is
  // (1) DMA from / to page-locked memory instead of the runtime's pageable path (pfm_host_register), (2) never moving the
  // (u,phi) block, which is identically zero (cracks.cc:2333-2337; placeholders of constrained rows live on the diagonals
  // of the (u,u) and (phi,phi) blocks): 3/16 of the bytes, (3) two copy streams.
  int pfm_host_register(pfm_ctx *c, void *p, int64_t bytes)
  {
    if (!c || !p || bytes <= 0)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    for (auto &hp : c->host_pins)
      if (hp.p == p)
        {
          if (hp.bytes >= (size_t)bytes)
            return PFM_OK;
          (void)hipHostUnregister(hp.p); // the same array, grown: lock it again
          hp.p = nullptr;
        }
    c->host_pins.erase(std::remove_if(c->host_pins.begin(), c->host_pins.end(), [](const pfm_ctx::HostPin &h) { return h.p == nullptr; }),
                       c->host_pins.end());
    const hipError_t e = hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess)
      {
        (void)hipGetLastError(); // not sticky: the transfers simply take the pageable path
        return fail(c, PFM_ERR_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e) + " (the array stays pageable)");
      }
    pfm_ctx::HostPin hp;
    hp.p = p;
    hp.bytes = (size_t)bytes;
    c->host_pins.push_back(hp);
    return PFM_OK;
  }

  int pfm_host_unregister(pfm_ctx *c, void *p)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream)
      (void)hipStreamSynchronize(c->copy_stream);
    delta_forget_host(c, p);
    for (auto &hp : c->host_pins)
      if (!p || hp.p == p)
        {
          (void)hipHostUnregister(hp.p);
          hp.p = nullptr;
        }
    c->host_pins.erase(std::remove_if(c->host_pins.begin(), c->host_pins.end(), [](const pfm_ctx::HostPin &h) { return h.p == nullptr; }),
                       c->host_pins.end());
    return PFM_OK;
  }

  int pfm_values_to_host(pfm_ctx *c, double *const *d_values, double *const *h_values)
  {
    if (!c || !d_values || !h_values)
      return PFM_ERR_BAD_ARG;
    const int rc = values_to_host_async(c, d_values, h_values);
    if (rc)
      return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? PFM_OK : hipfail(c, e, "pfm_values_to_host");
  }

  int pfm_assemble(pfm_ctx *c, const double *sol, const double *old, const double *oldold,
                   int residual_only, double *const *values, double *residual_pde,
                   double *residual_total)
  {
    if (!c || !residual_pde || (residual_only && !residual_total) || (!residual_only && !values))
      return PFM_ERR_BAD_ARG;
    if (c->v.n_owned != c->v.n_nodes)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_assemble is single-rank only; use the halo entry points");
    int rc = pfm_state_set(c, sol, old, oldold, 0);
    if (rc)
      return rc;
    const size_t vb = sizeof(double) * (size_t)c->n_owned_dofs();
    for (int k = 0; k < 2; ++k)
      if (!c->d_stage_res[k])
        {
          hipError_t e = hipMalloc((void **)&c->d_stage_res[k], std::max<size_t>(vb, 8));
          if (e != hipSuccess)
            return hipfail(c, e, "hipMalloc stage residual");
          c->device_bytes += (int64_t)vb;
        }
    if (!residual_only)
      for (int b = 0; b < c->n_blocks; ++b)
        if (!c->d_stage_val[b])
          {
            const size_t bytes = sizeof(double) * (size_t)c->block_nnz(b);
            hipError_t e = hipMalloc((void **)&c->d_stage_val[b], std::max<size_t>(bytes, 8));
            if (e != hipSuccess)
              return hipfail(c, e, "hipMalloc stage values");
            c->device_bytes += (int64_t)bytes;
            if (c->n_blocks == 4 && b == 1 && bytes)
              {
                // the staging (u,phi) block is the library's own: cleared once, here, and kept (plan_assembly) -- complete
                // before any assembly on any stream; an unregistered h_values[1] keeps receiving these zeros by its copy
                e = hipMemsetAsync(c->d_stage_val[b], 0, bytes, c->stream);
                if (e == hipSuccess)
                  e = hipStreamSynchronize(c->stream);
                if (e != hipSuccess)
                  return hipfail(c, e, "clear the staged (u,phi) block");
                c->stage_up_kept = true;
              }
          }
    rc = pfm_assemble_device(c, residual_only, c->d_stage_val, c->d_stage_res[0], c->d_stage_res[1]);
    if (rc)
      return rc;
    // the residual first (the caller's Newton loop reads it at once, cracks.cc:2791-2794), then the matrix blocks
    hipError_t e = d2h_user(c, residual_pde, c->d_stage_res[0], vb, c->stream);
    if (e == hipSuccess && residual_only)
      e = d2h_user(c, residual_total, c->d_stage_res[1], vb, c->stream);
    if (e != hipSuccess)
      return hipfail(c, e, "copy back");
    if (!residual_only)
      {
        rc = values_to_host_async(c, c->d_stage_val, values);
        if (rc)
          return rc;
      }
    return pfm_sync_status(c);
  }
}
