// pfm_q1_point.h -- the Q1 element of the device-side entries (pfm_newton.hip, pfm_postproc.hip, pfm_adapt.hip,
// pfm_pointstat.hip).  Device only: a cell's vertex coordinates and node state from the device view, the dof of a
// (node, component), QGauss(3), and shape values / physical gradients / det J at a reference point (MappingQ1).
#pragma once

#include "pfm_internal.h"

#include <hip/hip_runtime.h>

namespace pfm
{
  // dof of (node, component) in a vector of n_nodes nodes
  __device__ __forceinline__ long long dof_of(int layout, int dim, long long n_nodes, long long node, int comp)
  {
    if (layout == PFM_LAYOUT_INTERLEAVED)
      return node * (dim + 1) + comp;
    return comp < dim ? node * dim + comp : n_nodes * dim + node;
  }
  // ... in a vector over the owned nodes of the view
  template <int dim>
  __device__ __forceinline__ long long dof_of(const DevView &v, int P, int c)
  {
    return dof_of(v.layout, dim, v.n_owned, P, c);
  }

  // QGauss(3) on [0,1]
  __device__ __forceinline__ double gauss_x(int i)
  {
    return i == 0 ? 0.5 - 0.5 * 0.7745966692414834 : (i == 1 ? 0.5 : 0.5 + 0.5 * 0.7745966692414834);
  }
  __device__ __forceinline__ double gauss_w(int i) { return i == 1 ? 8.0 / 18.0 : 5.0 / 18.0; }

  // Q1 shape value of vertex b at xi
  template <int dim>
  __device__ __forceinline__ double q1_weight(int b, const double xi[dim])
  {
    double w = 1.0;
#pragma unroll
    for (int d = 0; d < dim; ++d)
      w *= ((b >> d) & 1) ? xi[d] : (1.0 - xi[d]);
    return w;
  }

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
} // namespace pfm
