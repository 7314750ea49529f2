// pfm_newton.hip — the other per-iteration sweeps of the Newton / active-set loop, so
// that residual_total, diag_mass and the solution never leave the device between two assemblies:
//
//   pfm_diag_mass_device    assemble_diag_mass_matrix                 cracks.cc:2514-2562
//   pfm_active_set_device   active-set predicate + cycle counter      cracks.cc:2837-2886, 2903-2909
//                           + constraints_hanging_nodes.distribute    cracks.cc:2888-2890
//   pfm_active_set_owned_device, pfm_halo_pack_flags_all / _unpack_flags_all, pfm_distribute_hanging_device
//                           the same block in the pieces of a rank with ghost peers (pfm_active_set_exchange, pfm_halo.cpp)
//   pfm_functionals         compute_energy, compute_tcv               cracks.cc:3615-3701, 3553-3611
//
// All three work on any Q1 mesh (MappingQ1 geometry per cell) with the node state / tables of the context.  The Q1
// element is pfm_q1_point.h, the fixed-order reductions are pfm_reduce.h, the host helpers pfm_entry.h.
#include "pfm_entry.h"
#include "pfm_q1_point.h"
#include "pfm_reduce.h"

#include <algorithm>

#include "../../include/pfm_newton.h"

namespace pfm
{
  namespace
  {
    // (k_diag_mass keeps its own Jacobian and determinant: through eval_point the last bits of the 3-D masses change)
    __device__ __forceinline__ double det2(const double J[2][2]) { return J[0][0] * J[1][1] - J[0][1] * J[1][0]; }
    __device__ __forceinline__ double det3(const double J[3][3])
    {
      return J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2]) +
             J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    }

    // ---- diag_mass: QGaussLobatto(2) = the vertices with weight 2^-dim; the phase-field dof of vertex a of a
    // cell receives det J(vertex a) 2^-dim.  thread <-> (cell, vertex).
    template <int dim>
    __global__ __launch_bounds__(256) void k_diag_mass(DevView v, double *__restrict__ mass)
    {
      constexpr int nv = 1 << dim;
      const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (gid >= v.n_cells * nv)
        return;
      const long long cell = gid / nv;
      const int a = (int)(gid - cell * nv);
      double x[nv][dim];
      int node_a = 0;
#pragma unroll
      for (int b = 0; b < nv; ++b)
        {
          const int n = v.conn[(long long)b * v.n_cells + cell];
          if (b == a)
            node_a = n;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            x[b][d] = v.coords[(long long)d * v.n_nodes + n];
        }
      if (node_a >= v.n_owned)
        return; // the owner of the node sums it (owner computes: its cells are all local)
      double J[dim][dim];
#pragma unroll
      for (int i = 0; i < dim; ++i)
#pragma unroll
        for (int j = 0; j < dim; ++j)
          {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < nv; ++b)
              {
                double g = 1.0;
#pragma unroll
                for (int d = 0; d < dim; ++d)
                  {
                    const double xa = (a >> d) & 1;
                    if (d == j)
                      g *= ((b >> d) & 1) ? 1.0 : -1.0;
                    else
                      g *= ((b >> d) & 1) ? xa : (1.0 - xa);
                  }
                s += x[b][i] * g;
              }
            J[i][j] = s;
          }
      double det;
      if constexpr (dim == 2)
        det = det2(J);
      else
        det = det3(J);
      unsafeAtomicAdd(&mass[node_a], det / (double)nv);
    }

    // ---- active set, thread <-> owned node
    template <int dim>
    __global__ __launch_bounds__(256) void k_active_set(DevView v, uint8_t *__restrict__ node_flags,
                                                        const double *__restrict__ residual_total,
                                                        const double *__restrict__ mass, double cconst,
                                                        double *__restrict__ solution, const double *__restrict__ old_solution,
                                                        int32_t *__restrict__ cycle_counter,
                                                        unsigned long long *__restrict__ counts)
    {
      const int P = blockIdx.x * blockDim.x + threadIdx.x;
      unsigned active_now = 0, cycling = 0, changed = 0;
      if (P < v.n_owned)
        {
          const uint8_t f = node_flags[P];
          const bool was = (f >> dim) & 1u;
          const bool hanging = v.hn_index && v.hn_index[P] >= 0; // constraints_hanging_nodes.is_constrained(idx)
          bool now = false;
          if (!hanging)
            {
              const long long idx = dof_of<dim>(v, P, dim);
              const double old_value = old_solution[idx], new_value = solution[idx];
              const double gap = new_value - old_value;
              const int cyc = cycle_counter[P];
              bool crit_le_0;
              {
                // the criterion is rounded as written (quotient, product, sum; no fma): at a tie a contracted
                // fma(c, gap, r / m) decides differently from the reference and from newton.py's numpy statement
#pragma clang fp contract(off)
                const double q = residual_total[idx] / mass[P];
                const double cg = cconst * gap;
                crit_le_0 = q + cg <= 0.0;
              }
              const bool inactive = crit_le_0 && cyc < 5; // cracks.cc:2868-2872
              if (!inactive)
                {
                  cycling = cyc >= 5;
                  now = true;
                  solution[idx] = old_value; // cracks.cc:2880
                }
            }
          if (was && !now)
            cycle_counter[P] += 1; // cracks.cc:2905-2908
          changed = was != now;
          active_now = now;
          node_flags[P] = (uint8_t)((f & ~(1u << dim)) | ((now ? 1u : 0u) << dim));
        }
      // integer counts: exact and order independent
      const unsigned long long b0 = __ballot(active_now), b1 = __ballot(cycling), b2 = __ballot(changed);
      if ((threadIdx.x & 63) == 0)
        {
          if (b0)
            atomicAdd(&counts[0], (unsigned long long)__popcll(b0));
          if (b1)
            atomicAdd(&counts[1], (unsigned long long)__popcll(b1));
          if (b2)
            atomicAdd(&counts[2], 1ull);
        }
    }

    // line k of the hanging table: sum_j hn_weights[j] * value_of(parent j), in table order -- the one expression behind
    // both distributions below, so that they leave the same bits
    template <class ValueOf>
    __device__ __forceinline__ double hanging_sum(const DevView &v, int k, ValueOf value_of)
    {
      double s = 0.0;
      for (long long j = v.hn_ptr[k]; j < v.hn_ptr[k + 1]; ++j)
        s += v.hn_weights[j] * value_of(v.hn_parents[j]);
      return s;
    }

    // constraints_hanging_nodes.distribute(solution): thread <-> (hanging node, component)
    template <int dim>
    __global__ __launch_bounds__(256) void k_distribute_hanging(DevView v, double *__restrict__ solution)
    {
      const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      const int P = (int)(gid / (dim + 1)), c = (int)(gid % (dim + 1));
      if (P >= v.n_owned || v.hn_index[P] < 0)
        return;
      solution[dof_of<dim>(v, P, c)] = hanging_sum(v, v.hn_index[P], [&](int parent) { return solution[dof_of<dim>(v, parent, c)]; });
    }

    // hn_nodes[k] = the node of line k of the hanging table (the context keeps node -> k only): thread <-> local node
    __global__ __launch_bounds__(256) void k_hanging_nodes(DevView v, int32_t *__restrict__ hn_nodes)
    {
      const int P = blockIdx.x * blockDim.x + threadIdx.x;
      if (P < v.n_nodes && v.hn_index[P] >= 0)
        hn_nodes[v.hn_index[P]] = P;
    }

    // the same distribution where a parent may be a ghost: on the node arrays of the solution, over ALL local hanging nodes
    // (a ghost one is recomputed from its parents, which are local); owned ones are also written to the dof vector.
    // thread <-> (line of the hanging table, component).  Parents never hang: the reads and the writes are disjoint.
    template <int dim>
    __global__ __launch_bounds__(256) void k_distribute_hanging_state(DevView v, const int32_t *__restrict__ hn_nodes, int n_hanging,
                                                                      double *__restrict__ solution /* or nullptr */)
    {
      const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      const int k = (int)(gid / (dim + 1)), c = (int)(gid % (dim + 1));
      if (k >= n_hanging)
        return;
      const int P = hn_nodes[k];
      if (P < 0)
        return; // a line whose node another line of the table overrides
      double *field = c == dim ? v.phi : (c == 0 ? v.u[0] : (c == 1 ? v.u[1] : v.u[2]));
      const double s = hanging_sum(v, k, [&](int parent) { return field[parent]; });
      field[P] = s;
      if (solution && P < v.n_owned)
        solution[dof_of<dim>(v, P, c)] = s;
    }

    // flag bytes of the nodes of a concatenated halo list, one byte per entry: the message of peer k starts at byte ptr[k],
    // so entry j of the list is byte j of the buffer and no peer has to be looked up (k_halo_all needs its peer for the
    // field-major layout inside a message).  UNPACK merges the active-set line of the phase field (bit dim) only.
    template <bool UNPACK>
    __global__ __launch_bounds__(256) void k_halo_flags_all(int dim, uint8_t *__restrict__ node_flags, const int32_t *__restrict__ nodes,
                                                            long long n_total, uint8_t *__restrict__ buf)
    {
      const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (j >= n_total)
        return;
      const int node = nodes[j];
      if constexpr (UNPACK)
        {
          const unsigned m = 1u << dim;
          node_flags[node] = (uint8_t)((node_flags[node] & ~m) | (buf[j] & m));
        }
      else
        buf[j] = node_flags[node];
    }

    // ---- energies and total crack volume: thread <-> cell, QGauss(3)^dim, MappingQ1; fixed-order reduction
    template <int dim>
    __global__ __launch_bounds__(256) void k_functionals(DevView v, pfm_params prm, const uint8_t *__restrict__ cell_owned,
                                                         const double *__restrict__ lam_over, const double *__restrict__ mu_over,
                                                         double *__restrict__ partial /* [gridDim.x][3] */)
    {
      constexpr int nv = 1 << dim, nq = dim == 2 ? 9 : 27;
      const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      double acc[3] = {0.0, 0.0, 0.0};
      if (cell < v.n_cells && (!cell_owned || cell_owned[cell]))
        {
          double x[nv][dim], U[nv][dim], PH[nv];
          load_geometry<dim>(v, cell, x);
          load_state<dim>(v, cell, U, PH);
          const double lam = lam_over ? lam_over[cell] : (v.cell_lambda ? v.cell_lambda[cell] : prm.lambda);
          const double mu = mu_over ? mu_over[cell] : (v.cell_mu ? v.cell_mu[cell] : prm.mu);
#pragma unroll 1
          for (int q = 0; q < nq; ++q)
            {
              const int qi[3] = {q % 3, (q / 3) % 3, q / 9};
              double xi[dim], w = 1.0;
#pragma unroll
              for (int d = 0; d < dim; ++d)
                {
                  xi[d] = gauss_x(qi[d]);
                  w *= gauss_w(qi[d]);
                }
              double N[nv], g[nv][dim], inv[dim][dim];
              const double det = eval_point<dim>(x, xi, N, g, inv);
              double gu[dim][dim], gpf[dim], uq[dim], pf = 0.0;
#pragma unroll
              for (int c = 0; c < dim; ++c)
                {
                  uq[c] = 0.0;
                  gpf[c] = 0.0;
#pragma unroll
                  for (int d = 0; d < dim; ++d)
                    gu[c][d] = 0.0;
                }
#pragma unroll
              for (int b = 0; b < nv; ++b)
                {
                  pf += PH[b] * N[b];
#pragma unroll
                  for (int c = 0; c < dim; ++c)
                    {
                      uq[c] += U[b][c] * N[b];
                      gpf[c] += PH[b] * g[b][c];
#pragma unroll
                      for (int d = 0; d < dim; ++d)
                        gu[c][d] += U[b][c] * g[b][d];
                    }
                }
              double trE = 0.0, tr_e_2 = 0.0, gg = 0.0, ug = 0.0;
#pragma unroll
              for (int a = 0; a < dim; ++a)
                {
                  trE += gu[a][a];
                  gg += gpf[a] * gpf[a];
                  ug += uq[a] * gpf[a];
#pragma unroll
                  for (int b = 0; b < dim; ++b)
                    {
                      const double e = 0.5 * (gu[a][b] + gu[b][a]);
                      tr_e_2 += e * e;
                    }
                }
              const double JxW = det * w;
              const double psi_e = 0.5 * lam * trE * trE + mu * tr_e_2;
              acc[0] += ((1 + prm.constant_k) * pf * pf + prm.constant_k) * psi_e * JxW;                               // cracks.cc:3677
              acc[1] += prm.G_c / 2.0 * ((pf - 1) * (pf - 1) / prm.alpha_eps + prm.alpha_eps * gg) * JxW;              // cracks.cc:3679-3680
              acc[2] += ug * JxW;                                                                                      // cracks.cc:3587
            }
        }
      const double r = block_reduce(acc, Sum<double>{});
      if (threadIdx.x < 3)
        partial[(long long)blockIdx.x * 3 + threadIdx.x] = r;
    }

    // ---- norms of a residual vector with the constrained lines zeroed (constraints_update.set_zero, cracks.cc:2791-2794,
    // 2947-2949): thread <-> owned node, grid-stride over a grid that depends on n_owned only; fixed-order reductions
    template <int dim>
    __global__ __launch_bounds__(256) void k_residual_norms(DevView v, const double *__restrict__ res, double *__restrict__ partial /* [gridDim.x][2] */)
    {
      double sq = 0.0, mx = 0.0;
      for (long long P = (long long)blockIdx.x * 256 + threadIdx.x; P < v.n_owned; P += (long long)gridDim.x * 256)
        {
          const unsigned f = v.node_flags[P];
          const bool hanging = v.hn_index && v.hn_index[P] >= 0;
#pragma unroll
          for (int c = 0; c <= dim; ++c)
            {
              const double r = (hanging || ((f >> c) & 1u)) ? 0.0 : res[dof_of<dim>(v, (int)P, c)];
              sq = fma(r, r, sq);
              mx = fmax(mx, fabs(r));
            }
        }
      const double acc[2] = {sq, mx};
      const double r = block_reduce(acc, SumMax{});
      if (threadIdx.x < 2)
        partial[2 * (long long)blockIdx.x + threadIdx.x] = r;
    }

    // second stage of the norms: out = (sqrt(sum), max, sum)
    __global__ __launch_bounds__(256) void k_reduce_norms(const double *__restrict__ partial, int n, double *__restrict__ out)
    {
      double acc[2];
      fold_partials(partial, n, acc, SumMax{});
      const double r = block_reduce(acc, SumMax{});
      if (threadIdx.x == 0)
        {
          out[0] = sqrt(r);
          out[2] = r;
        }
      else if (threadIdx.x == 1)
        out[1] = r;
    }
  } // namespace

  int launch_halo_flags_all(const DevView &v, const int32_t *d_nodes, int64_t n_total, uint8_t *d_buf, int unpack, hipStream_t s)
  {
    if (n_total <= 0)
      return PFM_OK;
    const unsigned nb = (unsigned)((n_total + 255) / 256);
    uint8_t *flags = const_cast<uint8_t *>(v.node_flags);
    if (unpack)
      hipLaunchKernelGGL(k_halo_flags_all<true>, dim3(nb), dim3(256), 0, s, v.dim, flags, d_nodes, (long long)n_total, d_buf);
    else
      hipLaunchKernelGGL(k_halo_flags_all<false>, dim3(nb), dim3(256), 0, s, v.dim, flags, d_nodes, (long long)n_total, d_buf);
    return hipGetLastError() == hipSuccess ? PFM_OK : PFM_ERR_HIP;
  }

  int reserve_flag_halo_buffers(pfm_ctx *c)
  {
    if (int rc = dev_buf_reserve(c, c->buf_flag_send, (size_t)c->n_send_all, "flag halo send buffer"))
      return rc;
    return dev_buf_reserve(c, c->buf_flag_recv, (size_t)c->n_recv_all, "flag halo receive buffer");
  }
} // namespace pfm

using namespace pfm;

extern "C"
{
  int pfm_diag_mass_device(pfm_ctx *c, double *d_mass)
  {
    if (!c || !d_mass)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    if (hipMemsetAsync(d_mass, 0, sizeof(double) * (size_t)c->v.n_owned, c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "diag_mass memset");
    const int nv = 1 << c->v.dim;
    const long long n = c->v.n_cells * nv;
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (nb)
      PFM_LAUNCH_DIM(c->v.dim, k_diag_mass, dim3(nb), dim3(256), c->stream, c->v, d_mass);
    return hipGetLastError() == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "k_diag_mass launch");
  }

  // k_active_set over the owned nodes; distribute: followed by k_distribute_hanging on d_solution (every parent owned)
  static int active_set_sweep(pfm_ctx *c, const double *d_residual_total, const double *d_mass, double c_const, double *d_solution,
                              const double *d_old_solution, int32_t *d_cycle_counter, int64_t *counts, bool distribute)
  {
    (void)hipSetDevice(c->device);
    if (int rc = dev_buf_reserve(c, c->buf_counts, 3 * sizeof(unsigned long long), "counts"))
      return rc;
    unsigned long long *d_counts = c->buf_counts.as<unsigned long long>();
    if (hipMemsetAsync(d_counts, 0, 3 * sizeof(unsigned long long), c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "counts memset");
    const unsigned nb = (unsigned)((c->v.n_owned + 255) / 256); // 0 on a rank that owns no node: nothing to launch
    uint8_t *flags = const_cast<uint8_t *>(c->v.node_flags);
    if (nb)
      PFM_LAUNCH_DIM(c->v.dim, k_active_set, dim3(nb), dim3(256), c->stream, c->v, flags, d_residual_total, d_mass, c_const,
                     d_solution, d_old_solution, d_cycle_counter, d_counts);
    if (distribute && c->v.hn_index && nb)
      {
        // we might have changed values of the solution, so fix the hanging nodes (cracks.cc:2888-2890)
        const long long n = (long long)c->v.n_owned * (c->v.dim + 1);
        const unsigned nbh = (unsigned)((n + 255) / 256);
        PFM_LAUNCH_DIM(c->v.dim, k_distribute_hanging, dim3(nbh), dim3(256), c->stream, c->v, d_solution);
      }
    if (hipGetLastError() != hipSuccess)
      return fail(c, PFM_ERR_HIP, "k_active_set launch");
    unsigned long long h[3];
    if (hipMemcpyAsync(h, d_counts, sizeof(h), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "counts copy");
    counts[0] = (int64_t)h[0];
    counts[1] = (int64_t)h[1];
    counts[2] = h[2] != 0; // number of waves that saw a change -> flag
    return PFM_OK;
  }

  int pfm_active_set_device(pfm_ctx *c, const double *d_residual_total, const double *d_mass, double c_const,
                            double *d_solution, const double *d_old_solution, int32_t *d_cycle_counter, int64_t *counts)
  {
    if (!c || !d_residual_total || !d_mass || !d_solution || !d_old_solution || !d_cycle_counter || !counts)
      return PFM_ERR_BAD_ARG;
    if (c->v.n_owned != c->v.n_nodes && c->v.hn_index)
      return fail(c, PFM_ERR_UNSUPPORTED, "hanging nodes on a partitioned mesh");
    return active_set_sweep(c, d_residual_total, d_mass, c_const, d_solution, d_old_solution, d_cycle_counter, counts, true);
  }

  int pfm_active_set_owned_device(pfm_ctx *c, const double *d_residual_total, const double *d_mass, double c_const,
                                  double *d_solution, const double *d_old_solution, int32_t *d_cycle_counter, int64_t *counts)
  {
    if (!c || !d_residual_total || !d_mass || !d_solution || !d_old_solution || !d_cycle_counter || !counts)
      return PFM_ERR_BAD_ARG;
    return active_set_sweep(c, d_residual_total, d_mass, c_const, d_solution, d_old_solution, d_cycle_counter, counts, false);
  }

  int pfm_halo_pack_flags_all(pfm_ctx *c, uint8_t *d_buf_all)
  {
    if (!c || (!d_buf_all && c->n_send_all))
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    const int rc = launch_halo_flags_all(c->v, c->d_send_all, c->n_send_all, d_buf_all, 0, c->stream);
    return rc ? fail(c, rc, "k_halo_flags_all launch") : PFM_OK;
  }

  int pfm_halo_unpack_flags_all(pfm_ctx *c, const uint8_t *d_buf_all)
  {
    if (!c || (!d_buf_all && c->n_recv_all))
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    const int rc = launch_halo_flags_all(c->v, c->d_recv_all, c->n_recv_all, const_cast<uint8_t *>(d_buf_all), 1, c->stream);
    return rc ? fail(c, rc, "k_halo_flags_all launch") : PFM_OK;
  }

  int pfm_distribute_hanging_device(pfm_ctx *c, double *d_solution)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (!c->v.hn_index || c->n_hanging <= 0)
      return PFM_OK;
    (void)hipSetDevice(c->device);
    if (!c->hn_nodes_ready)
      {
        if (int rc = dev_buf_reserve(c, c->buf_hn_nodes, sizeof(int32_t) * (size_t)c->n_hanging, "hanging nodes"))
          return rc;
        if (hipMemsetAsync(c->buf_hn_nodes.p, 0xff, sizeof(int32_t) * (size_t)c->n_hanging, c->stream) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "hanging nodes memset");
        hipLaunchKernelGGL(k_hanging_nodes, dim3((unsigned)((c->v.n_nodes + 255) / 256)), dim3(256), 0, c->stream, c->v,
                           c->buf_hn_nodes.as<int32_t>());
        if (hipGetLastError() != hipSuccess)
          return fail(c, PFM_ERR_HIP, "k_hanging_nodes launch");
        c->hn_nodes_ready = true;
      }
    const long long n = (long long)c->n_hanging * (c->v.dim + 1);
    PFM_LAUNCH_DIM(c->v.dim, k_distribute_hanging_state, dim3((unsigned)((n + 255) / 256)), dim3(256), c->stream, c->v,
                   c->buf_hn_nodes.as<int32_t>(), (int)c->n_hanging, d_solution);
    return hipGetLastError() == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "k_distribute_hanging_state launch");
  }

  int pfm_get_constraints(pfm_ctx *c, uint8_t *node_flags)
  {
    if (!c || !node_flags)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    if (hipMemcpyAsync(node_flags, c->v.node_flags, (size_t)c->v.n_nodes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "get_constraints");
    return PFM_OK;
  }


  int pfm_residual_norms(pfm_ctx *c, const double *d_residual, double *out)
  {
    if (!c || !out || (!d_residual && c->v.n_owned > 0))
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    const long long nbl = ((long long)c->v.n_owned + 255) / 256;
    const unsigned nb = (unsigned)std::min<long long>(nbl, NORM_BLOCKS_MAX);
    if (int rc = dev_buf_reserve(c, c->buf_norm_partial, sizeof(double) * (2 * (size_t)NORM_BLOCKS_MAX + 4), "norm partial sums"))
      return rc;
    double *d_partial = c->buf_norm_partial.as<double>(), *d_out = d_partial + 2 * (size_t)NORM_BLOCKS_MAX;
    if (nb)
      PFM_LAUNCH_DIM(c->v.dim, k_residual_norms, dim3(nb), dim3(256), c->stream, c->v, d_residual, d_partial);
    hipLaunchKernelGGL(k_reduce_norms, dim3(1), dim3(256), 0, c->stream, d_partial, (int)nb, d_out);
    if (hipGetLastError() != hipSuccess)
      return fail(c, PFM_ERR_HIP, "k_residual_norms launch");
    if (hipMemcpyAsync(out, d_out, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "residual norms copy");
    return PFM_OK;
  }

  int pfm_functionals(pfm_ctx *c, const uint8_t *cell_owned, double *out)
  {
    return pfm_functionals_material(c, cell_owned, nullptr, nullptr, out);
  }

  int pfm_functionals_material(pfm_ctx *c, const uint8_t *cell_owned, const double *cell_lambda, const double *cell_mu,
                               double *out)
  {
    if (!c || !out || ((cell_lambda == nullptr) != (cell_mu == nullptr)))
      return PFM_ERR_BAD_ARG;
    if (!c->have_params)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_set_params has not been called");
    (void)hipSetDevice(c->device);
    const unsigned nb = (unsigned)((c->v.n_cells + 255) / 256);
    if (int rc = dev_buf_reserve(c, c->buf_partial, sizeof(double) * 3 * ((size_t)nb + 1), "partial sums"))
      return rc;
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    double *d_lam = nullptr, *d_mu = nullptr;
    if (cell_lambda && c->v.n_cells > 0)
      {
        if (int rc = dev_buf_reserve(c, c->buf_func_mat, 2 * sizeof(double) * (size_t)c->v.n_cells, "material override"))
          return rc;
        d_lam = c->buf_func_mat.as<double>();
        d_mu = d_lam + c->v.n_cells;
        if (hipMemcpyAsync(d_lam, cell_lambda, sizeof(double) * (size_t)c->v.n_cells, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_mu, cell_mu, sizeof(double) * (size_t)c->v.n_cells, hipMemcpyHostToDevice, c->stream) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "material override upload");
      }
    double *d_partial = c->buf_partial.as<double>(), *d_out = d_partial + 3 * (size_t)nb;
    if (nb)
      PFM_LAUNCH_DIM(c->v.dim, k_functionals, dim3(nb), dim3(256), c->stream, c->v, c->prm, d_owned, d_lam, d_mu, d_partial);
    hipLaunchKernelGGL((k_reduce_final<double, 3, Sum<double>>), dim3(1), dim3(256), 0, c->stream, d_partial, (long long)nb, d_out);
    if (hipGetLastError() != hipSuccess)
      return fail(c, PFM_ERR_HIP, "k_functionals launch");
    if (hipMemcpyAsync(out, d_out, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "functionals copy");
    return PFM_OK;
  }
}
