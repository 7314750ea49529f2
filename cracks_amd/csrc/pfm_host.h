// pfm_host.h -- what the host-side files of the C ABI share: pfm_transfer.cpp (copies of caller-owned memory),
// pfm_ctx_build.cpp (pfm_ctx_create and the lazy tables), pfm_host.cpp (calls on a living context), pfm_halo.cpp (ghost
// exchange) and pfm_dispatch.cpp (assembly).  Each name is defined in the file named next to it; everything else in those
// files is local to its file.
#pragma once

#include "pfm_entry.h"

#include <algorithm>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

namespace pfm
{
  struct HipFail
  {
    hipError_t e;
    const char *what;
  };

  template <class T>
  T *dev_alloc(pfm_ctx *c, size_t n)
  {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess)
      throw HipFail{e, "hipMalloc"};
    c->allocs.push_back(p);
    c->device_bytes += (int64_t)bytes;
    return static_cast<T *>(p);
  }

  inline int hipfail(pfm_ctx *c, hipError_t e, const char *what)
  {
    return fail(c, PFM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }

  // f() behind the C ABI: what dev_alloc / dev_upload and the lazy table builders throw becomes the call's status
  // (f returns nothing, or a status)
  template <class F>
  int guarded(pfm_ctx *c, F &&f)
  {
    try
      {
        if constexpr (std::is_void<decltype(f())>::value)
          return f(), PFM_OK;
        else
          return f();
      }
    catch (const HipFail &x)
      {
        return hipfail(c, x.e, x.what);
      }
    catch (const std::bad_alloc &)
      {
        return fail(c, PFM_ERR_NOMEM, "host allocation failed");
      }
  }

  // ---- pfm_transfer.cpp
  struct H2dBatch // while one lives on the calling thread, h2d leaves its copies ordered on the null stream
  {
    H2dBatch();
    ~H2dBatch();
  };
  hipError_t h2d(void *d, const void *h, size_t bytes);
  hipError_t h2d_user(pfm_ctx *c, void *d, const void *h, size_t bytes, hipStream_t s);

  template <class T>
  T *dev_upload(pfm_ctx *c, const T *h, size_t n)
  {
    T *d = dev_alloc<T>(c, n);
    if (n)
      {
        hipError_t e = h2d(d, h, n * sizeof(T));
        if (e != hipSuccess)
          throw HipFail{e, "hipMemcpy H2D"};
      }
    return d;
  }

  // ---- pfm_ctx_build.cpp (the row tables: also for pfm_pattern_bind, which changes the order of the rows)
  void ensure_host_graph(pfm_ctx *c);
  void ensure_general_tables(pfm_ctx *c);
  void ensure_full_colours(pfm_ctx *c);
  bool row_order_tables(const pfm_ctx *c, int dim, int32_t NO, const LatticeHost &L, std::vector<uint32_t> &mask,
                        std::vector<uint8_t> &perm, bool &any_perm);
  void upload_row_tables(pfm_ctx *c, const std::vector<uint32_t> &mask, const std::vector<uint8_t> &perm, bool any_perm);

  // ---- pfm_host.cpp
  int state_set_impl(pfm_ctx *c, const double *sol, const double *old, const double *oldold, int on_device);
  bool ensure_hang_gather(pfm_ctx *c);

  // ---- pfm_halo.cpp
  enum { HALO_VALUES = 1, HALO_FLAGS = 2 };
  int halo_exchange_on(pfm_ctx *c, void *comm, const int *peer_ranks, hipStream_t st, int what = HALO_VALUES);
} // namespace pfm
