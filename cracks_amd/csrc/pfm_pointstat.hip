// pfm_pointstat.hip — the two statistics of the reference that sample the solution at points (include/pfm_newton.h):
//
//   pfm_cod_buckets   compute_cod_array                              cracks.cc:3337-3449, 3323-3335
//   pfm_point_eval    compute_point_stress, compute_point_value      cracks.cc:3285-3320, 3264-3283
//
// MappingQ1 per point on any Q1 mesh, FP64 throughout, the node state of the device view (every kernel path, both layouts).
// No floating-point atomics: every sum has a fixed order, repeated calls are bitwise identical.  The bucket sums are
// reduced per bucket in wave order here (not the block reduction of pfm_reduce.h); the Q1 element is pfm_q1_point.h, the
// host helpers pfm_entry.h.
#include "pfm_entry.h"
#include "pfm_q1_point.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/pfm_newton.h"

namespace pfm
{
  namespace
  {
    // ---- pfm_cod_buckets.  Work items are (cell, slab): a slab is CB_SLAB_ROWS rows of sample points along xi_0.  A wave
    // takes a contiguous range of items; its lanes walk the rows lane, lane + 64, ... of a slab.  Along a row x, the columns
    // of J, u and the reference gradient of phi are affine in xi_0 (hoisted per row), and (u . grad phi) det J =
    // sum_e dphi/dxi_e det(J with column e replaced by u): no division per point.  A lane keeps the two sums of its current
    // bucket in registers and adds them to its private LDS column [bucket of the window][lane] when the bucket changes.
    // The bucket of x is found by comparing with the thresholds T[i] = the smallest double whose value_to_bucket is >= i
    // (computed on the host by bisection over the doubles with the reference's unfused expression, which is monotone in
    // x): exactly the reference's index without a division per point.  A cell that spans more than CB_WIN buckets is walked
    // once per window of CB_WIN buckets.  After a slab the lanes' columns are added per bucket by xor-shuffles and lane 0
    // adds the result to the wave's accumulator; the waves' accumulators go to scratch and one block adds them in wave order.
    constexpr int CB_WAVES = 4;                   // waves per workgroup
    constexpr int CB_WIN = 8;                     // buckets per window: 8 KiB of LDS columns per wave
    constexpr int CB_SLAB_ROWS = 256;             // rows of a work item (4 per lane)
    constexpr int CB_MAX_WAVES = 6144;            // waves (and partial sums) per launch: 1536 workgroups, whole rounds of the 768
                                                  // (2-D, LDS bound) or 512 (3-D, register bound) that 256 CUs hold
    constexpr long long CB_MAX_POINTS = 1LL << 32; // sample points per launch
    constexpr int CB_MAX_BUCKETS = 128, CB_MAX_SUB = 128;

    __device__ __forceinline__ void wave_sync()
    {
      // LDS traffic between the lanes of ONE wave: the hardware keeps a wave's LDS operations in order, this keeps the
      // compiler from moving them across
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }

    // bucket of x from the thresholds T[0 .. nb] (LDS): (number of T[i] <= x) - 1, in -1 .. nb
    __device__ __forceinline__ int bucket_of(const double *__restrict__ T, int nb, double x)
    {
      int lo = 0, hi = nb + 1;
      while (lo < hi)
        {
          const int mid = (lo + hi) >> 1;
          if (T[mid] <= x)
            lo = mid + 1;
          else
            hi = mid;
        }
      return lo - 1;
    }

    // The Q1 function with vertex values f[0 .. nv) restricted to the row (xi_1[, xi_2]) = eta: value A + xi_0 S and, for
    // e = 1 .. dim-1, d/dxi_e = G0[e-1] + xi_0 GS[e-1].  (d/dxi_0 = S.)
    template <int dim>
    __device__ __forceinline__ void row_coeffs(const double *__restrict__ f, const double eta[dim - 1], double &A, double &S,
                                               double G0[dim - 1], double GS[dim - 1])
    {
      if constexpr (dim == 2)
        {
          const double t = eta[0], s = 1.0 - t;
          A = f[0] * s + f[2] * t;
          const double B = f[1] * s + f[3] * t;
          S = B - A;
          G0[0] = f[2] - f[0];
          GS[0] = (f[3] - f[1]) - G0[0];
        }
      else
        {
          const double t1 = eta[0], s1 = 1.0 - t1, t2 = eta[1], s2 = 1.0 - t2;
          A = (f[0] * s1 + f[2] * t1) * s2 + (f[4] * s1 + f[6] * t1) * t2;
          const double B = (f[1] * s1 + f[3] * t1) * s2 + (f[5] * s1 + f[7] * t1) * t2;
          S = B - A;
          G0[0] = (f[2] - f[0]) * s2 + (f[6] - f[4]) * t2;
          GS[0] = ((f[3] - f[1]) * s2 + (f[7] - f[5]) * t2) - G0[0];
          G0[1] = (f[4] - f[0]) * s1 + (f[6] - f[2]) * t1;
          GS[1] = ((f[5] - f[1]) * s1 + (f[7] - f[3]) * t1) - G0[1];
        }
    }

    template <int dim>
    __global__ __launch_bounds__(64 * CB_WAVES) void k_cod_buckets(DevView v, const uint8_t *__restrict__ cell_owned, long long cell0,
                                                                   long long n_items, int slabs, long long items_per_wave,
                                                                   int n_buckets, int n_sub, const double *__restrict__ thr,
                                                                   double *__restrict__ partial /* [waves][2 n_buckets] */)
    {
      constexpr int nv = 1 << dim, NDATA = nv * (2 * dim + 1);
      __shared__ double s_col[CB_WAVES][CB_WIN][2][64];
      __shared__ double s_acc[CB_WAVES][2 * CB_MAX_BUCKETS];
      __shared__ double s_cell[CB_WAVES][NDATA]; // [coordinate d | u_c | phi][vertex]
      __shared__ double s_xi[CB_MAX_SUB];
      __shared__ double s_thr[CB_MAX_BUCKETS + 1];
      const int tid = threadIdx.x, lane = tid & 63;
      const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
      for (int i = tid; i < n_sub; i += 64 * CB_WAVES)
        s_xi[i] = ((double)i + 0.5) / (double)n_sub;
      for (int i = tid; i <= n_buckets; i += 64 * CB_WAVES)
        s_thr[i] = thr[i];
      for (int i = lane; i < 2 * n_buckets; i += 64)
        s_acc[wib][i] = 0.0;
#pragma unroll
      for (int b = 0; b < CB_WIN; ++b)
        {
          s_col[wib][b][0][lane] = 0.0;
          s_col[wib][b][1][lane] = 0.0;
        }
      __syncthreads();
      const long long wave = (long long)blockIdx.x * CB_WAVES + wib;
      const long long it0 = wave * items_per_wave, it1 = min(n_items, it0 + items_per_wave);
      const int rows_per_cell = dim == 2 ? n_sub : n_sub * n_sub;
      double weight = 1.0 / (double)n_sub;
#pragma unroll
      for (int d = 1; d < dim; ++d)
        weight = weight / (double)n_sub;
      const double inf = __builtin_huge_val();
      const double *__restrict__ cd = s_cell[wib];
      long long cur_cell = -1;
      bool active = false;
      int blo = 0, bhi = -1;
      for (long long it = it0; it < it1; ++it) // wave-uniform
        {
          const long long cl = it / slabs;
          const int slab = (int)(it - cl * slabs);
          const long long cell = cell0 + cl;
          if (cell != cur_cell)
            {
              cur_cell = cell;
              active = !cell_owned || cell_owned[cell] != 0;
              if (active)
                {
                  wave_sync(); // the previous cell's rows have read s_cell
                  if (lane < NDATA)
                    {
                      const int b = lane % nv, q = lane / nv;
                      const int n = v.conn[(long long)b * v.n_cells + cell];
                      double val;
                      if (q < dim)
                        val = v.coords[(long long)q * v.n_nodes + n];
                      else if (q < 2 * dim)
                        val = (q - dim == 0 ? v.u[0] : (q - dim == 1 ? v.u[1] : v.u[2]))[n];
                      else
                        val = v.phi[n];
                      s_cell[wib][q * nv + b] = val;
                    }
                  wave_sync();
                  // buckets the cell can touch: those of its vertices' x range, widened by far more than the rounding of
                  // the interpolated x (a few ulps of the largest |x|).  A cell wholly outside the buckets is skipped.
                  double xmin = cd[0], xmax = cd[0];
#pragma unroll
                  for (int b = 1; b < nv; ++b)
                    {
                      xmin = fmin(xmin, cd[b]);
                      xmax = fmax(xmax, cd[b]);
                    }
                  const double slack = 1e-12 * fmax(fabs(xmin), fabs(xmax));
                  blo = bucket_of(s_thr, n_buckets, xmin - slack); // -1 .. n_buckets
                  bhi = bucket_of(s_thr, n_buckets, xmax + slack);
                  active = bhi >= 0 && blo < n_buckets;
                  blo = max(blo, 0);
                  bhi = min(bhi, n_buckets - 1);
                }
            }
          if (!active)
            continue;
          const int row0 = slab * CB_SLAB_ROWS, row1 = min(rows_per_cell, row0 + CB_SLAB_ROWS);
          for (int wlo = blo; wlo <= bhi; wlo += CB_WIN)
            {
              const int nbw = min(CB_WIN, bhi - wlo + 1);
              // the lane's current bucket: its thresholds, its column in the window (-1: outside) and its two sums
              double lo_t = inf, hi_t = -inf, sv = 0.0, sd = 0.0;
              int col = -1;
              for (int r = row0 + lane; r < row1; r += 64)
                {
                  double eta[dim - 1];
                  if constexpr (dim == 2)
                    eta[0] = s_xi[r];
                  else
                    {
                      eta[0] = s_xi[r % n_sub];
                      eta[1] = s_xi[r / n_sub];
                    }
                  double xA[dim], xS[dim], xG0[dim][dim - 1], xGS[dim][dim - 1];
                  double uA[dim], uS[dim], pA, pS, pG0[dim - 1], pGS[dim - 1], dump0[dim - 1], dump1[dim - 1];
#pragma unroll
                  for (int d = 0; d < dim; ++d)
                    {
                      row_coeffs<dim>(cd + d * nv, eta, xA[d], xS[d], xG0[d], xGS[d]);
                      row_coeffs<dim>(cd + (dim + d) * nv, eta, uA[d], uS[d], dump0, dump1);
                    }
                  row_coeffs<dim>(cd + 2 * dim * nv, eta, pA, pS, pG0, pGS);
                  (void)pA;
#pragma unroll 2
                  for (int k = 0; k < n_sub; ++k)
                    {
                      const double t = s_xi[k];
                      const double x = xA[0] + t * xS[0];
                      if (!(x >= lo_t && x < hi_t))
                        {
                          if (col >= 0)
                            {
                              s_col[wib][col][0][lane] += sv;
                              s_col[wib][col][1][lane] += sd;
                            }
                          const int idx = bucket_of(s_thr, n_buckets, x);
                          lo_t = idx >= 0 ? s_thr[idx] : -inf;
                          hi_t = idx < n_buckets ? s_thr[idx + 1] : inf;
                          col = (idx >= wlo && idx < wlo + nbw) ? idx - wlo : -1;
                          sv = 0.0;
                          sd = 0.0;
                        }
                      if (col >= 0)
                        {
                          if constexpr (dim == 2)
                            {
                              const double j00 = xS[0], j10 = xS[1];
                              const double j01 = xG0[0][0] + t * xGS[0][0], j11 = xG0[1][0] + t * xGS[1][0];
                              const double u0 = uA[0] + t * uS[0], u1 = uA[1] + t * uS[1];
                              const double g1 = pG0[0] + t * pGS[0];
                              sd += j00 * j11 - j01 * j10;
                              sv += pS * (j11 * u0 - j01 * u1) + g1 * (j00 * u1 - j10 * u0);
                            }
                          else
                            {
                              double c1[3], c2[3], u[3];
#pragma unroll
                              for (int i = 0; i < 3; ++i)
                                {
                                  c1[i] = xG0[i][0] + t * xGS[i][0];
                                  c2[i] = xG0[i][1] + t * xGS[i][1];
                                  u[i] = uA[i] + t * uS[i];
                                }
                              const double g1 = pG0[0] + t * pGS[0], g2 = pG0[1] + t * pGS[1];
                              const double n0[3] = {c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2],
                                                    c1[0] * c2[1] - c1[1] * c2[0]};
                              const double n1[3] = {c2[1] * xS[2] - c2[2] * xS[1], c2[2] * xS[0] - c2[0] * xS[2],
                                                    c2[0] * xS[1] - c2[1] * xS[0]};
                              const double n2[3] = {xS[1] * c1[2] - xS[2] * c1[1], xS[2] * c1[0] - xS[0] * c1[2],
                                                    xS[0] * c1[1] - xS[1] * c1[0]};
                              sd += xS[0] * n0[0] + xS[1] * n0[1] + xS[2] * n0[2];
                              sv += u[0] * (pS * n0[0] + g1 * n1[0] + g2 * n2[0]) + u[1] * (pS * n0[1] + g1 * n1[1] + g2 * n2[1]) +
                                    u[2] * (pS * n0[2] + g1 * n1[2] + g2 * n2[2]);
                            }
                        }
                    }
                }
              if (col >= 0)
                {
                  s_col[wib][col][0][lane] += sv;
                  s_col[wib][col][1][lane] += sd;
                }
              // the lanes of every bucket of the window, in the fixed order of the xor-shuffles; lane 0 accumulates
              for (int b = 0; b < nbw; ++b)
                {
                  double a = s_col[wib][b][0][lane], c = s_col[wib][b][1][lane];
                  s_col[wib][b][0][lane] = 0.0;
                  s_col[wib][b][1][lane] = 0.0;
#pragma unroll
                  for (int off = 32; off >= 1; off >>= 1)
                    {
                      a += __shfl_xor(a, off);
                      c += __shfl_xor(c, off);
                    }
                  if (lane == 0)
                    {
                      s_acc[wib][2 * (wlo + b)] += a * weight;
                      s_acc[wib][2 * (wlo + b) + 1] += c * weight;
                    }
                }
            }
        }
      __syncthreads();
      for (int i = lane; i < 2 * n_buckets; i += 64)
        partial[wave * (2 * n_buckets) + i] = s_acc[wib][i];
    }

    // total[t] (+)= the waves' partial sums in wave order
    __global__ __launch_bounds__(256) void k_cod_buckets_reduce(const double *__restrict__ partial, int n_waves, int n2, int first,
                                                                double *__restrict__ total)
    {
      const int t = threadIdx.x;
      if (t >= n2)
        return;
      double s = first ? 0.0 : total[t];
      for (int w = 0; w < n_waves; ++w)
        s += partial[(long long)w * n2 + t];
      total[t] = s;
    }

    // ---- pfm_point_eval

    constexpr int PE_MAX_POINTS = 4096, PE_CHUNK = 256, PE_NEWTON_STEPS = 20;
    constexpr double PE_BOX_TOL = 1e-8, PE_CELL_TOL = 1e-10, PE_STEP_TOL = 1e-12;

    // Newton inverse of the Q1 map from the cell centre: true when a step became <= PE_STEP_TOL in every coordinate
    template <int dim>
    __device__ __forceinline__ bool newton_inverse(const double x[1 << dim][dim], const double p[dim], double xi[dim])
    {
      constexpr int nv = 1 << dim;
#pragma unroll
      for (int d = 0; d < dim; ++d)
        xi[d] = 0.5;
#pragma unroll 1
      for (int it = 0; it < PE_NEWTON_STEPS; ++it)
        {
          double F[dim], J[dim][dim];
#pragma unroll
          for (int i = 0; i < dim; ++i)
            {
              F[i] = -p[i];
#pragma unroll
              for (int j = 0; j < dim; ++j)
                J[i][j] = 0.0;
            }
#pragma unroll
          for (int b = 0; b < nv; ++b)
            {
              double N = 1.0, dN[dim];
#pragma unroll
              for (int d = 0; d < dim; ++d)
                N *= ((b >> d) & 1) ? xi[d] : (1.0 - xi[d]);
#pragma unroll
              for (int e = 0; e < dim; ++e)
                {
                  double s = 1.0;
#pragma unroll
                  for (int d = 0; d < dim; ++d)
                    s *= (d == e) ? (((b >> d) & 1) ? 1.0 : -1.0) : (((b >> d) & 1) ? xi[d] : (1.0 - xi[d]));
                  dN[e] = s;
                }
#pragma unroll
              for (int i = 0; i < dim; ++i)
                {
                  F[i] += x[b][i] * N;
#pragma unroll
                  for (int j = 0; j < dim; ++j)
                    J[i][j] += x[b][i] * dN[j];
                }
            }
          double dx[dim];
          if constexpr (dim == 2)
            {
              const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
              dx[0] = (J[1][1] * F[0] - J[0][1] * F[1]) / det;
              dx[1] = (J[0][0] * F[1] - J[1][0] * F[0]) / det;
            }
          else
            {
              const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
              const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
              const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
              const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
              dx[0] = (c00 * F[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * F[1] + (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * F[2]) / det;
              dx[1] = (c01 * F[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * F[1] + (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * F[2]) / det;
              dx[2] = (c02 * F[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * F[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * F[2]) / det;
            }
          double step = 0.0;
          bool finite = true;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            {
              xi[d] -= dx[d];
              finite = finite && fabs(dx[d]) <= 1e300; // false for inf and NaN
              step = fmax(step, fabs(dx[d]));
            }
          if (!finite)
            return false;
          if (step <= PE_STEP_TOL)
            return true;
        }
      return false;
    }

    // thread <-> cell, blockIdx.y <-> chunk of PE_CHUNK points (LDS): cell_of[p] = min over the cells that contain p
    template <int dim>
    __global__ __launch_bounds__(256) void k_point_find(DevView v, const uint8_t *__restrict__ cell_owned, const double *__restrict__ points,
                                                        int n_points, int32_t *__restrict__ cell_of)
    {
      constexpr int nv = 1 << dim;
      __shared__ double s_p[PE_CHUNK][dim];
      const int p0 = blockIdx.y * PE_CHUNK, np = min(PE_CHUNK, n_points - p0);
      for (int i = threadIdx.x; i < np * dim; i += 256)
        s_p[i / dim][i % dim] = points[(long long)p0 * dim + i];
      __syncthreads();
      const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
      if (cell >= v.n_cells || (cell_owned && !cell_owned[cell]))
        return;
      double x[nv][dim];
      load_geometry<dim>(v, cell, x);
      double lo[dim], hi[dim], diam = 0.0;
#pragma unroll
      for (int d = 0; d < dim; ++d)
        {
          lo[d] = hi[d] = x[0][d];
#pragma unroll
          for (int b = 1; b < nv; ++b)
            {
              lo[d] = fmin(lo[d], x[b][d]);
              hi[d] = fmax(hi[d], x[b][d]);
            }
        }
#pragma unroll
      for (int b = 0; b < nv / 2; ++b) // cell->diameter(): the longest vertex diagonal
        {
          double s = 0.0;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            {
              const double e = x[nv - 1 - b][d] - x[b][d];
              s += e * e;
            }
          diam = fmax(diam, sqrt(s));
        }
      const double tol = PE_BOX_TOL * diam;
#pragma unroll
      for (int d = 0; d < dim; ++d)
        {
          lo[d] -= tol;
          hi[d] += tol;
        }
      for (int q = 0; q < np; ++q)
        {
          bool in = true;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            in = in && s_p[q][d] >= lo[d] && s_p[q][d] <= hi[d];
          if (!in)
            continue;
          double p[dim], xi[dim];
#pragma unroll
          for (int d = 0; d < dim; ++d)
            p[d] = s_p[q][d];
          if (!newton_inverse<dim>(x, p, xi))
            continue;
          bool inside = true;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            inside = inside && xi[d] >= -PE_CELL_TOL && xi[d] <= 1.0 + PE_CELL_TOL;
          if (inside)
            atomicMin(&cell_of[p0 + q], (int32_t)cell);
        }
    }

    // thread <-> point: the Q1 interpolant and its gradient at the clamped xi of the point's cell
    template <int dim>
    __global__ __launch_bounds__(256) void k_point_values(DevView v, const double *__restrict__ points, int n_points,
                                                          int32_t *__restrict__ cell_of, double *__restrict__ values,
                                                          double *__restrict__ grads)
    {
      constexpr int nv = 1 << dim, nc = dim + 1;
      const int i = blockIdx.x * 256 + threadIdx.x;
      if (i >= n_points)
        return;
      const int32_t cell = cell_of[i];
      double val[nc], gr[nc][dim];
#pragma unroll
      for (int c = 0; c < nc; ++c)
        {
          val[c] = 0.0;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            gr[c][d] = 0.0;
        }
      if (cell == INT_MAX)
        cell_of[i] = -1;
      else
        {
          double x[nv][dim], U[nv][dim], PH[nv], p[dim], xi[dim], N[nv], g[nv][dim], inv[dim][dim];
          load_geometry<dim>(v, cell, x);
          load_state<dim>(v, cell, U, PH);
#pragma unroll
          for (int d = 0; d < dim; ++d)
            p[d] = points[(long long)i * dim + d];
          (void)newton_inverse<dim>(x, p, xi); // converged in k_point_find: the same arithmetic
#pragma unroll
          for (int d = 0; d < dim; ++d)
            xi[d] = fmin(fmax(xi[d], 0.0), 1.0); // project_to_unit_cell
          (void)eval_point<dim>(x, xi, N, g, inv);
#pragma unroll
          for (int b = 0; b < nv; ++b)
#pragma unroll
            for (int c = 0; c < nc; ++c)
              {
                const double f = c < dim ? U[b][c < dim ? c : 0] : PH[b];
                val[c] += f * N[b];
#pragma unroll
                for (int d = 0; d < dim; ++d)
                  gr[c][d] += f * g[b][d];
              }
        }
#pragma unroll
      for (int c = 0; c < nc; ++c)
        {
          values[(long long)i * nc + c] = val[c];
#pragma unroll
          for (int d = 0; d < dim; ++d)
            grads[((long long)i * nc + c) * dim + d] = gr[c][d];
        }
    }

    // value_to_bucket before its cast (cracks.cc:3327), every operation rounded on its own
    double bucket_real(double x, double x_lo, double x_hi, int n_buckets)
    {
#pragma clang fp contract(off)
      const double a = x - x_lo;
      const double b = x_hi - x_lo;
      const double q = a / b;
      const double s = q * (double)n_buckets;
      return std::floor(s + 0.5);
    }

    // the doubles in their order as unsigned integers
    uint64_t ordered_key(double d)
    {
      uint64_t u;
      std::memcpy(&u, &d, sizeof(u));
      return (u >> 63) ? ~u : (u | (1ull << 63));
    }
    double ordered_value(uint64_t k)
    {
      const uint64_t u = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
      double d;
      std::memcpy(&d, &u, sizeof(d));
      return d;
    }

    // T[i] = the smallest double x with bucket_real(x) >= i (-inf: every finite x, +inf: none); bucket_real is monotone in x
    double bucket_threshold(int i, double x_lo, double x_hi, int n_buckets)
    {
      const double big = std::numeric_limits<double>::max(), inf = std::numeric_limits<double>::infinity();
      auto pred = [&](double x) { return bucket_real(x, x_lo, x_hi, n_buckets) >= (double)i; };
      if (!pred(big))
        return inf;
      if (pred(-big))
        return -inf;
      uint64_t lo = ordered_key(-big), hi = ordered_key(big); // pred(lo) false, pred(hi) true
      while (hi - lo > 1)
        {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (pred(ordered_value(mid)))
            hi = mid;
          else
            lo = mid;
        }
      return ordered_value(hi);
    }
  } // namespace
} // namespace pfm

using namespace pfm;

extern "C"
{
  int pfm_cod_buckets(pfm_ctx *c, const uint8_t *cell_owned, int n_buckets, double x_lo, double x_hi, int n_sub, double *values,
                      double *volume)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (!values || !volume || n_buckets < 1 || n_buckets > CB_MAX_BUCKETS || n_sub < 1 || n_sub > CB_MAX_SUB || !std::isfinite(x_lo) ||
        !std::isfinite(x_hi) || !(x_lo < x_hi))
      return fail(c, PFM_ERR_BAD_ARG, "pfm_cod_buckets: bad arguments (1 <= n_buckets, n_sub <= 128, finite x_lo < x_hi, outputs)");
    if (!c->have_params)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_set_params has not been called");
    (void)hipSetDevice(c->device);
    const int dim = c->v.dim, n2 = 2 * n_buckets;
    const long long NC = c->v.n_cells;
    std::vector<double> thr((size_t)n_buckets + 1);
    for (int i = 0; i <= n_buckets; ++i)
      thr[(size_t)i] = bucket_threshold(i, x_lo, x_hi, n_buckets);
    long long pts_per_cell = 1;
    for (int d = 0; d < dim; ++d)
      pts_per_cell *= n_sub;
    const long long rows_per_cell = pts_per_cell / n_sub;
    const int slabs = (int)((rows_per_cell + CB_SLAB_ROWS - 1) / CB_SLAB_ROWS);
    const long long cells_per_launch = std::max<long long>(1, CB_MAX_POINTS / pts_per_cell);
    const size_t o_total = align256(sizeof(double) * thr.size()), o_partial = o_total + align256(sizeof(double) * (size_t)n2);
    if (int rc = dev_buf_reserve(c, c->buf_stat, o_partial + sizeof(double) * (size_t)n2 * CB_MAX_WAVES, "statistics scratch"))
      return rc;
    char *base = c->buf_stat.as<char>();
    double *d_thr = reinterpret_cast<double *>(base), *d_total = reinterpret_cast<double *>(base + o_total),
           *d_partial = reinterpret_cast<double *>(base + o_partial);
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    if (hipMemcpyAsync(d_thr, thr.data(), sizeof(double) * thr.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemsetAsync(d_total, 0, sizeof(double) * (size_t)n2, c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "pfm_cod_buckets: threshold upload");
    for (long long c0 = 0; c0 < NC; c0 += cells_per_launch)
      {
        const long long n_items = std::min(cells_per_launch, NC - c0) * slabs;
        const unsigned nb = (unsigned)((std::min<long long>(n_items, CB_MAX_WAVES) + CB_WAVES - 1) / CB_WAVES);
        const int n_waves = (int)nb * CB_WAVES;
        const long long items_per_wave = (n_items + n_waves - 1) / n_waves;
        PFM_LAUNCH_DIM(dim, k_cod_buckets, dim3(nb), dim3(64 * CB_WAVES), c->stream, c->v, d_owned, c0, n_items, slabs, items_per_wave,
                       n_buckets, n_sub, d_thr, d_partial);
        hipLaunchKernelGGL(k_cod_buckets_reduce, dim3(1), dim3(256), 0, c->stream, d_partial, n_waves, n2, c0 == 0 ? 1 : 0, d_total);
        if (hipGetLastError() != hipSuccess)
          return fail(c, PFM_ERR_HIP, "k_cod_buckets launch");
      }
    std::vector<double> h((size_t)n2);
    if (hipMemcpyAsync(h.data(), d_total, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "pfm_cod_buckets: copy");
    for (int b = 0; b < n_buckets; ++b)
      {
        values[b] = h[(size_t)2 * b];
        volume[b] = h[(size_t)2 * b + 1];
      }
    return PFM_OK;
  }

  int pfm_point_eval(pfm_ctx *c, const uint8_t *cell_owned, int n_points, const double *points, int32_t *cell, double *values,
                     double *grads)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (n_points < 0 || n_points > PE_MAX_POINTS || !points || !cell)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_point_eval: bad arguments (0 <= n_points <= 4096, points, cell)");
    if (!c->have_params)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_set_params has not been called");
    const int dim = c->v.dim, nc = dim + 1;
    for (long long i = 0; i < (long long)n_points * dim; ++i)
      if (!std::isfinite(points[i]))
        return fail(c, PFM_ERR_BAD_ARG, "pfm_point_eval: coordinate " + std::to_string(i) + " is not finite");
    if (n_points == 0)
      return PFM_OK;
    (void)hipSetDevice(c->device);
    const size_t np = (size_t)n_points;
    const size_t o_cell = align256(sizeof(double) * np * dim), o_val = o_cell + align256(sizeof(int32_t) * np),
                 o_grad = o_val + align256(sizeof(double) * np * nc), total = o_grad + align256(sizeof(double) * np * nc * dim);
    if (int rc = dev_buf_reserve(c, c->buf_stat, total, "statistics scratch"))
      return rc;
    char *base = c->buf_stat.as<char>();
    double *d_points = reinterpret_cast<double *>(base), *d_val = reinterpret_cast<double *>(base + o_val),
           *d_grad = reinterpret_cast<double *>(base + o_grad);
    int32_t *d_cell = reinterpret_cast<int32_t *>(base + o_cell);
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    if (hipMemcpyAsync(d_points, points, sizeof(double) * np * dim, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_cell), INT_MAX, np, c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "pfm_point_eval: point upload");
    const unsigned nbc = (unsigned)((c->v.n_cells + 255) / 256), nchunks = (unsigned)((n_points + PE_CHUNK - 1) / PE_CHUNK);
    if (nbc)
      PFM_LAUNCH_DIM(dim, k_point_find, dim3(nbc, nchunks), dim3(256), c->stream, c->v, d_owned, d_points, n_points, d_cell);
    const unsigned nbp = (unsigned)((n_points + 255) / 256);
    PFM_LAUNCH_DIM(dim, k_point_values, dim3(nbp), dim3(256), c->stream, c->v, d_points, n_points, d_cell, d_val, d_grad);
    if (hipGetLastError() != hipSuccess)
      return fail(c, PFM_ERR_HIP, "k_point_find launch");
    std::vector<int32_t> h_cell(np);
    std::vector<double> h_val(values ? np * nc : 0), h_grad(grads ? np * nc * dim : 0);
    bool ok = hipMemcpyAsync(h_cell.data(), d_cell, sizeof(int32_t) * np, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (values)
      ok = ok && hipMemcpyAsync(h_val.data(), d_val, sizeof(double) * h_val.size(), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (grads)
      ok = ok && hipMemcpyAsync(h_grad.data(), d_grad, sizeof(double) * h_grad.size(), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "pfm_point_eval: copy");
    std::copy(h_cell.begin(), h_cell.end(), cell);
    if (values)
      std::copy(h_val.begin(), h_val.end(), values);
    if (grads)
      std::copy(h_grad.begin(), h_grad.end(), grads);
    return PFM_OK;
  }
}
