// pfm_q1_point.h -- what the post-processing entries (pfm_postproc.hip, pfm_pointstat.hip) share.  Device: a cell's vertex
// coordinates and node state from the device view, and shape values / physical gradients / det J at a reference point.
// Host: the error text and the upload of the owned-cell mask.
#pragma once

#include "pfm_internal.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>

namespace pfm
{
  template <int dim>
  __device__ __forceinline__ void load_geometry(const DevView &v, long long cell, double x[1 << dim][dim])
  {
#pragma unroll
    for (int b = 0; b < (1 << dim); ++b)
      {
        const int n = v.conn[(long long)b * v.n_cells + cell];
#pragma unroll
        for (int d = 0; d < dim; ++d)
          x[b][d] = v.coords[(long long)d * v.n_nodes + n];
      }
  }

  template <int dim>
  __device__ __forceinline__ void load_state(const DevView &v, long long cell, double U[1 << dim][dim], double PH[1 << dim])
  {
#pragma unroll
    for (int b = 0; b < (1 << dim); ++b)
      {
        const int n = v.conn[(long long)b * v.n_cells + cell];
#pragma unroll
        for (int d = 0; d < dim; ++d)
          U[b][d] = v.u[d][n];
        PH[b] = v.phi[n];
      }
  }

  // Q1 shape values, physical gradients and det J at the reference point xi (MappingQ1)
  template <int dim>
  __device__ __forceinline__ double eval_point(const double x[1 << dim][dim], const double xi[dim], double N[1 << dim],
                                               double g[1 << dim][dim], double inv[dim][dim])
  {
    constexpr int nv = 1 << dim;
    double dNr[nv][dim];
#pragma unroll
    for (int b = 0; b < nv; ++b)
      {
        double val = 1.0;
#pragma unroll
        for (int d = 0; d < dim; ++d)
          val *= ((b >> d) & 1) ? xi[d] : (1.0 - xi[d]);
        N[b] = val;
#pragma unroll
        for (int e = 0; e < dim; ++e)
          {
            double s = 1.0;
#pragma unroll
            for (int d = 0; d < dim; ++d)
              s *= (d == e) ? (((b >> d) & 1) ? 1.0 : -1.0) : (((b >> d) & 1) ? xi[d] : (1.0 - xi[d]));
            dNr[b][e] = s;
          }
      }
    double J[dim][dim], det;
#pragma unroll
    for (int i = 0; i < dim; ++i)
#pragma unroll
      for (int j = 0; j < dim; ++j)
        {
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < nv; ++b)
            s += x[b][i] * dNr[b][j];
          J[i][j] = s;
        }
    if constexpr (dim == 2)
      {
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        const double id = 1.0 / det;
        inv[0][0] = J[1][1] * id;
        inv[0][1] = -J[0][1] * id;
        inv[1][0] = -J[1][0] * id;
        inv[1][1] = J[0][0] * id;
      }
    else
      {
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
        const double id = 1.0 / det;
        inv[0][0] = c00 * id;
        inv[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
        inv[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
        inv[1][0] = c01 * id;
        inv[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
        inv[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
        inv[2][0] = c02 * id;
        inv[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
        inv[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
      }
#pragma unroll
    for (int b = 0; b < nv; ++b)
#pragma unroll
      for (int d = 0; d < dim; ++d)
        {
          double s = 0.0;
#pragma unroll
          for (int e = 0; e < dim; ++e)
            s += inv[e][d] * dNr[b][e];
          g[b][d] = s;
        }
    return det;
  }

  // ---- host side, shared by the entries of both files

  inline int fail(pfm_ctx *c, int code, const std::string &msg)
  {
    if (c)
      c->err = msg;
    return code;
  }

  // the owned-cell mask of a functional in the context's device buffer (shared with pfm_functionals, same stream);
  // *d_owned = nullptr for a NULL mask
  inline int upload_mask(pfm_ctx *c, const uint8_t *cell_owned, uint8_t **d_owned)
  {
    *d_owned = nullptr;
    if (!cell_owned)
      return PFM_OK;
    if (!c->d_cell_owned)
      {
        if (hipMalloc((void **)&c->d_cell_owned, (size_t)std::max<long long>(c->v.n_cells, 1)) != hipSuccess)
          return fail(c, PFM_ERR_NOMEM, "hipMalloc cell mask");
        c->allocs.push_back(c->d_cell_owned);
      }
    if (c->v.n_cells > 0 &&
        hipMemcpyAsync(c->d_cell_owned, cell_owned, (size_t)c->v.n_cells, hipMemcpyHostToDevice, c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "cell mask upload");
    *d_owned = c->d_cell_owned;
    return PFM_OK;
  }
} // namespace pfm
