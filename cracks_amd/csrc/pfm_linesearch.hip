// pfm_linesearch.hip — the Newton line search with the vectors on the device (include/pfm_newton.h):
//
//   pfm_line_search_advance / _retreat   the vector statements of cracks.cc:2944, 2955-2956 and 3050, 3059-3061
//   pfm_line_search_device               the loop around pfm_assemble_nl_residual_device and the norm stage
//   pfm_project_back_device              project_back_phase_field, cracks.cc:3111-3137
//
// The vector kernels are streams over the owned dofs: 16-byte accesses where all their vectors are 16-byte aligned, 8-byte
// ones otherwise, a scalar tail for an odd length.  Every operation is rounded on its own (no fused multiply-add; contract(off)
// as in k_active_set): the results equal an unfused host statement bit for bit.  The norm stage is k_residual_norms of
// pfm_newton.hip with the maximum kept per block of the solution: same grid, same order of every sum.
#include "pfm_entry.h"
#include "pfm_q1_point.h"
#include "pfm_reduce.h"

#include <algorithm>
#include <cmath>

#include "../../include/pfm_newton.h"

namespace pfm
{
  namespace
  {
    constexpr int LS_BLOCKS_MAX = 512; // blocks of 256 threads of a vector statement; longer vectors are walked grid-stride

    // the statements on one entry
    struct Pair
    {
      double sol, upd;
    };
    __device__ __forceinline__ double ls_advance(double s, double u)
    {
#pragma clang fp contract(off)
      return s + u;
    }
    // base = saved (SAVED) or the current solution (SUBTRACT); returns the new (solution, update)
    template <bool subtract, bool advance>
    __device__ __forceinline__ Pair ls_retreat(double base, double u, double damping)
    {
#pragma clang fp contract(off)
      Pair r;
      const double s = subtract ? base - u : base;
      r.upd = u * damping;
      r.sol = advance ? s + r.upd : s;
      return r;
    }

    // saved = solution; solution = solution + update.  wide: the vectors are 16-byte aligned and walked in pairs, the last
    // entry of an odd length by one thread on its own
    template <bool wide>
    __global__ __launch_bounds__(256) void k_ls_advance(double *__restrict__ sol, const double *__restrict__ upd, double *__restrict__ saved,
                                                        long long n)
    {
      const long long first = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
      if constexpr (wide)
        {
          double2 *sol2 = reinterpret_cast<double2 *>(sol), *saved2 = reinterpret_cast<double2 *>(saved);
          const double2 *upd2 = reinterpret_cast<const double2 *>(upd);
#pragma unroll 2
          for (long long i = first; i < n / 2; i += stride)
            {
              const double2 s = sol2[i], u = upd2[i];
              if (saved)
                saved2[i] = s;
              sol2[i] = make_double2(ls_advance(s.x, u.x), ls_advance(s.y, u.y));
            }
        }
      for (long long i = wide ? (n & ~1ll) + first : first; i < n; i += stride)
        {
          const double s = sol[i];
          if (saved)
            saved[i] = s;
          sol[i] = ls_advance(s, upd[i]);
        }
    }

    template <bool wide, bool subtract, bool advance>
    __global__ __launch_bounds__(256) void k_ls_retreat(double *__restrict__ sol, double *__restrict__ upd, const double *__restrict__ saved,
                                                        double damping, long long n)
    {
      const long long first = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
      if constexpr (wide)
        {
          double2 *sol2 = reinterpret_cast<double2 *>(sol), *upd2 = reinterpret_cast<double2 *>(upd);
          const double2 *saved2 = reinterpret_cast<const double2 *>(saved);
#pragma unroll 2
          for (long long i = first; i < n / 2; i += stride)
            {
              const double2 b = subtract ? sol2[i] : saved2[i], u = upd2[i];
              const Pair p0 = ls_retreat<subtract, advance>(b.x, u.x, damping), p1 = ls_retreat<subtract, advance>(b.y, u.y, damping);
              sol2[i] = make_double2(p0.sol, p1.sol);
              upd2[i] = make_double2(p0.upd, p1.upd);
            }
        }
      for (long long i = wide ? (n & ~1ll) + first : first; i < n; i += stride)
        {
          const Pair p = ls_retreat<subtract, advance>(subtract ? sol[i] : saved[i], upd[i], damping);
          sol[i] = p.sol;
          upd[i] = p.upd;
        }
    }

    // project_back_phase_field: thread <-> owned node
    template <int dim>
    __global__ __launch_bounds__(256) void k_project_back(DevView v, double *__restrict__ sol)
    {
      const int P = blockIdx.x * 256 + threadIdx.x;
      if (P >= v.n_owned)
        return;
      const long long idx = dof_of<dim>(v, P, dim);
      const double x = sol[idx];
      const double m = (1.0 < x) ? 1.0 : x;  // std::min(x, 1.0)
      sol[idx] = (0.0 < m) ? m : 0.0;        // std::max(0.0, m): NaN, -0.0 -> +0.0
    }

    // ---- norm stage: k_residual_norms (pfm_newton.hip) with the maximum kept apart for the displacement and the phase-field
    // dofs.  Component 0 is its sum of squares -- the same grid, the same fma chain per thread, the same block_reduce -- and
    // fmax(component 1, component 2) its maximum (a maximum does not depend on the order).
    struct SumMaxMax
    {
      static __device__ __forceinline__ double init(int) { return 0.0; }
      __device__ __forceinline__ double operator()(double a, double b, int k) const { return k == 0 ? a + b : fmax(a, b); }
    };
    template <int dim>
    __global__ __launch_bounds__(256) void k_ls_norms(DevView v, const double *__restrict__ res, double *__restrict__ partial /* [gridDim.x][3] */)
    {
      double sq = 0.0, mx_u = 0.0, mx_phi = 0.0;
      for (long long P = (long long)blockIdx.x * 256 + threadIdx.x; P < v.n_owned; P += (long long)gridDim.x * 256)
        {
          const unsigned f = v.node_flags[P];
          const bool hanging = v.hn_index && v.hn_index[P] >= 0;
#pragma unroll
          for (int c = 0; c <= dim; ++c)
            {
              const double r = (hanging || ((f >> c) & 1u)) ? 0.0 : res[dof_of<dim>(v, (int)P, c)];
              sq = fma(r, r, sq);
              if (c < dim)
                mx_u = fmax(mx_u, fabs(r));
              else
                mx_phi = fmax(mx_phi, fabs(r));
            }
        }
      const double acc[3] = {sq, mx_u, mx_phi};
      const double r = block_reduce(acc, SumMaxMax{});
      if (threadIdx.x < 3)
        partial[3 * (long long)blockIdx.x + threadIdx.x] = r;
    }

    // second stage: out = (sqrt(sum), max, sum, max over u, max over phi)
    __global__ __launch_bounds__(256) void k_ls_reduce_norms(const double *__restrict__ partial, int n, double *__restrict__ out)
    {
      double acc[3];
      fold_partials(partial, n, acc, SumMaxMax{});
      const double r = block_reduce(acc, SumMaxMax{});
      const double r_phi = __shfl(r, 2); // (threads 1 and 2 sit in one wave)
      if (threadIdx.x == 0)
        {
          out[0] = sqrt(r);
          out[2] = r;
        }
      else if (threadIdx.x == 1)
        {
          out[1] = fmax(r, r_phi);
          out[3] = r;
        }
      else if (threadIdx.x == 2)
        out[4] = r;
    }

    inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
    inline unsigned ls_grid(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, LS_BLOCKS_MAX); }

    int launch_advance(pfm_ctx *c, double *sol, const double *upd, double *saved)
    {
      const long long n = c->n_owned_dofs();
      if (n == 0)
        return PFM_OK;
      (void)hipSetDevice(c->device);
      if (aligned16(sol) && aligned16(upd) && aligned16(saved))
        hipLaunchKernelGGL(k_ls_advance<true>, dim3(ls_grid((n + 1) / 2)), dim3(256), 0, c->stream, sol, upd, saved, n);
      else
        hipLaunchKernelGGL(k_ls_advance<false>, dim3(ls_grid(n)), dim3(256), 0, c->stream, sol, upd, saved, n);
      return hipGetLastError() == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "k_ls_advance launch");
    }

    template <bool wide>
    void launch_retreat_w(hipStream_t s, bool subtract, bool advance, double *sol, double *upd, const double *saved, double damping, long long n)
    {
      const dim3 grid(ls_grid(wide ? (n + 1) / 2 : n)), block(256);
      if (subtract && advance)
        hipLaunchKernelGGL((k_ls_retreat<wide, true, true>), grid, block, 0, s, sol, upd, saved, damping, n);
      else if (subtract)
        hipLaunchKernelGGL((k_ls_retreat<wide, true, false>), grid, block, 0, s, sol, upd, saved, damping, n);
      else if (advance)
        hipLaunchKernelGGL((k_ls_retreat<wide, false, true>), grid, block, 0, s, sol, upd, saved, damping, n);
      else
        hipLaunchKernelGGL((k_ls_retreat<wide, false, false>), grid, block, 0, s, sol, upd, saved, damping, n);
    }

    int launch_retreat(pfm_ctx *c, bool subtract, double damping, double *sol, double *upd, const double *saved, bool advance)
    {
      const long long n = c->n_owned_dofs();
      if (n == 0)
        return PFM_OK;
      (void)hipSetDevice(c->device);
      if (subtract)
        saved = nullptr; // not read
      if (aligned16(sol) && aligned16(upd) && aligned16(saved))
        launch_retreat_w<true>(c->stream, subtract, advance, sol, upd, saved, damping, n);
      else
        launch_retreat_w<false>(c->stream, subtract, advance, sol, upd, saved, damping, n);
      return hipGetLastError() == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "k_ls_retreat launch");
    }

    constexpr size_t LS_NORM_BYTES = sizeof(double) * (3 * (size_t)NORM_BLOCKS_MAX + 8);

    // the norm stage of one trial: h[0..2] = pfm_residual_norms, h[3], h[4] = linf of the displacement / phase-field dofs.
    // Synchronous.  The scratch is the one of pfm_residual_norms, reserved by the caller.
    int ls_norms(pfm_ctx *c, const double *d_residual, double h[5])
    {
      const long long nbl = ((long long)c->v.n_owned + 255) / 256;
      const unsigned nb = (unsigned)std::min<long long>(nbl, NORM_BLOCKS_MAX); // the grid of pfm_residual_norms
      double *d_partial = c->buf_norm_partial.as<double>(), *d_out = d_partial + 3 * (size_t)NORM_BLOCKS_MAX;
      if (nb)
        PFM_LAUNCH_DIM(c->v.dim, k_ls_norms, dim3(nb), dim3(256), c->stream, c->v, d_residual, d_partial);
      hipLaunchKernelGGL(k_ls_reduce_norms, dim3(1), dim3(256), 0, c->stream, d_partial, (int)nb, d_out);
      if (hipGetLastError() != hipSuccess)
        return fail(c, PFM_ERR_HIP, "k_ls_norms launch");
      if (hipMemcpyAsync(h, d_out, 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
          hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, PFM_ERR_HIP, "line search norms copy");
      return PFM_OK;
    }
  } // namespace
} // namespace pfm

using namespace pfm;

extern "C"
{
  int pfm_line_search_advance(pfm_ctx *c, double *d_solution, const double *d_update, double *d_saved)
  {
    if (!c || !d_solution || !d_update)
      return PFM_ERR_BAD_ARG;
    return launch_advance(c, d_solution, d_update, d_saved);
  }

  int pfm_line_search_retreat(pfm_ctx *c, int restore, double damping, double *d_solution, double *d_update, const double *d_saved,
                              int advance)
  {
    if (!c || !d_solution || !d_update || (restore != PFM_LS_RESTORE_SAVED && restore != PFM_LS_RESTORE_SUBTRACT) ||
        !std::isfinite(damping) || (restore == PFM_LS_RESTORE_SAVED && !d_saved))
      return PFM_ERR_BAD_ARG;
    return launch_retreat(c, restore == PFM_LS_RESTORE_SUBTRACT, damping, d_solution, d_update, d_saved, advance != 0);
  }

  int pfm_line_search_device(pfm_ctx *c, const pfm_line_search_opts *o, double *d_solution, double *d_update, double *d_residual_pde,
                             double *d_residual_total, pfm_line_search_result *out)
  {
    if (!c || !o || !d_solution || !d_update || !d_residual_pde || !d_residual_total || !out)
      return PFM_ERR_BAD_ARG;
    if (o->max_steps < 1 || (o->norm != PFM_LS_NORM_L2 && o->norm != PFM_LS_NORM_LINF) ||
        (o->restore != PFM_LS_RESTORE_SAVED && o->restore != PFM_LS_RESTORE_SUBTRACT) || !std::isfinite(o->damping))
      return fail(c, PFM_ERR_BAD_ARG, "pfm_line_search_device: max_steps < 1, an unknown norm or restore mode, or a damping that is not finite");
    if (!c->peers.empty())
      return fail(c, PFM_ERR_BAD_ARG, "pfm_line_search_device: a rank with peers imports ghosts in every trial: it composes the loop itself");
    (void)hipSetDevice(c->device);
    // both buffers before anything is launched: PFM_ERR_NOMEM leaves the caller's vectors as they were
    const bool subtract = o->restore == PFM_LS_RESTORE_SUBTRACT;
    if (!subtract)
      if (int rc = dev_buf_reserve(c, c->buf_ls_saved, sizeof(double) * (size_t)c->n_owned_dofs(), "line search saved_solution"))
        return rc;
    if (int rc = dev_buf_reserve(c, c->buf_norm_partial, LS_NORM_BYTES, "norm partial sums"))
      return rc;
    double *d_saved = subtract ? nullptr : c->buf_ls_saved.as<double>();
    pfm_line_search_result r{};
    double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int step = 0;
    for (; step < o->max_steps; ++step)
      {
        // trial 0: saved = solution, solution += update; trial k > 0: the restore and the damping of the rejected trial and
        // the next `solution += update` in one pass
        int rc = step == 0 ? launch_advance(c, d_solution, d_update, d_saved)
                           : launch_retreat(c, subtract, o->damping, d_solution, d_update, d_saved, true);
        if (rc == PFM_OK)
          rc = pfm_assemble_nl_residual_device(c, d_solution, d_residual_pde, d_residual_total);
        if (rc == PFM_OK)
          rc = ls_norms(c, d_residual_pde, h);
        if (rc != PFM_OK)
          return rc;
        const double trial = o->norm == PFM_LS_NORM_L2 ? h[0] : h[1];
        if (trial < o->reference) // strict; false for a NaN on either side
          {
            r.accepted = 1;
            break;
          }
      }
    if (!r.accepted) // the last trial was rejected too: its restore and damping, nothing to advance to
      if (int rc = launch_retreat(c, subtract, o->damping, d_solution, d_update, d_saved, false))
        return rc;
    r.steps = step;
    for (int k = 0; k < 3; ++k)
      r.norms[k] = h[k];
    r.linf_block[0] = h[3];
    r.linf_block[1] = h[4];
    *out = r;
    return PFM_OK;
  }

  int pfm_project_back_device(pfm_ctx *c, double *d_solution)
  {
    if (!c || !d_solution)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    const unsigned nb = (unsigned)((c->v.n_owned + 255) / 256);
    if (nb)
      PFM_LAUNCH_DIM(c->v.dim, k_project_back, dim3(nb), dim3(256), c->stream, c->v, d_solution);
    return hipGetLastError() == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "k_project_back launch");
  }
}
