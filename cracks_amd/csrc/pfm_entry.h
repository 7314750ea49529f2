// pfm_entry.h -- host side of the device-side entries (pfm_newton.hip, pfm_postproc.hip, pfm_adapt.hip, pfm_pointstat.hip):
// the error text, the context's grow-only device buffers, the upload of the owned-cell mask and the launch of a
// `template <int dim>` kernel from the context's dimension.
#pragma once

#include "pfm_internal.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>

namespace pfm
{
  inline int fail(pfm_ctx *c, int code, const std::string &msg)
  {
    if (c)
      c->err = msg;
    return code;
  }

  constexpr size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

  // Buffer b of the context with at least `bytes` bytes (grow-only; contents undefined after growth).  It is in
  // `allocs` (freed by pfm_ctx_destroy) and counted in `device_bytes`.  Growth waits for the work queued on the
  // context's stream, which may still use the old buffer.  PFM_ERR_NOMEM leaves an empty buffer and a usable context.
  inline int dev_buf_reserve(pfm_ctx *c, DevBuf &b, size_t bytes, const char *what)
  {
    if (b.p && b.bytes >= bytes)
      return PFM_OK;
    if (b.p)
      {
        (void)hipStreamSynchronize(c->stream);
        c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), b.p), c->allocs.end());
        (void)hipFree(b.p);
        c->device_bytes -= (int64_t)b.bytes;
        b = DevBuf{};
      }
    bytes = std::max<size_t>(bytes, 256);
    if (hipMalloc(&b.p, bytes) != hipSuccess)
      {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(c, PFM_ERR_NOMEM, std::string("hipMalloc ") + what);
      }
    c->allocs.push_back(b.p);
    b.bytes = bytes;
    c->device_bytes += (int64_t)bytes;
    return PFM_OK;
  }

  // the owned-cell mask of an entry in the context's device buffer (one buffer, one stream); *d_owned = nullptr for a
  // NULL mask
  inline int upload_mask(pfm_ctx *c, const uint8_t *cell_owned, uint8_t **d_owned)
  {
    *d_owned = nullptr;
    if (!cell_owned)
      return PFM_OK;
    if (int rc = dev_buf_reserve(c, c->buf_cell_owned, (size_t)c->v.n_cells, "cell mask"))
      return rc;
    if (c->v.n_cells > 0 &&
        hipMemcpyAsync(c->buf_cell_owned.p, cell_owned, (size_t)c->v.n_cells, hipMemcpyHostToDevice, c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "cell mask upload");
    *d_owned = c->buf_cell_owned.as<uint8_t>();
    return PFM_OK;
  }
} // namespace pfm

// launches kernel<2> or kernel<3> for dim = 2 or 3: the argument list is written once
#define PFM_LAUNCH_DIM(dim, kernel, grid, block, stream, ...)                 \
  do                                                                          \
    {                                                                         \
      if ((dim) == 2)                                                         \
        hipLaunchKernelGGL(kernel<2>, grid, block, 0, stream, __VA_ARGS__);   \
      else                                                                    \
        hipLaunchKernelGGL(kernel<3>, grid, block, 0, stream, __VA_ARGS__);   \
    }                                                                         \
  while (0)
