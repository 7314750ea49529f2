// pfm_postproc.hip — the functionals the reference computes from a converged state besides energy and TCV
// (include/pfm_newton.h):
//
//   pfm_face_load           compute_load                                   cracks.cc:3726-3790
//   pfm_cod_lines           compute_functional_values -> compute_cod       cracks.cc:3706-3724, 3453-3550
//   pfm_sneddon_phi_error   integrate_difference(ExactPhiSneddon, L2, phi)  cracks.cc:4495-4524, 418-450
//
// MappingQ1 per quadrature point on any Q1 mesh (pfm_q1_point.h), FP64 throughout.  Every sum is a fixed-order reduction
// (pfm_reduce.h; no floating-point atomics): repeated calls are bitwise identical.  Each entry returns this rank's part; the
// MPI sums, the reference's sign flips and its "/2" are the caller's.  Host helpers: pfm_entry.h.
#include "pfm_entry.h"
#include "pfm_q1_point.h"
#include "pfm_reduce.h"

#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pfm_newton.h"

namespace pfm
{
  namespace
  {
    // Point q of QGauss<dim-1>(3) on face f (deal.II numbering: axis f/2, side f%2) in cell reference coordinates,
    // QProjector's axis order: 2-D (s,t) / (t,s); 3-D faces 0/1 (s,q0,q1), 2/3 (q1,s,q0), 4/5 (q0,q1,s).
    template <int dim>
    __device__ __forceinline__ double face_point(int f, int q, double xi[dim])
    {
      const int a = f >> 1;
      const double s = (double)(f & 1);
      if constexpr (dim == 2)
        {
          xi[a] = s;
          xi[1 - a] = gauss_x(q);
          return gauss_w(q);
        }
      else
        {
          const double q0 = gauss_x(q % 3), q1 = gauss_x(q / 3);
          if (a == 0)
            {
              xi[0] = s;
              xi[1] = q0;
              xi[2] = q1;
            }
          else if (a == 1)
            {
              xi[0] = q1;
              xi[1] = s;
              xi[2] = q0;
            }
          else
            {
              xi[0] = q0;
              xi[1] = q1;
              xi[2] = s;
            }
          return gauss_w(q % 3) * gauss_w(q / 3);
        }
    }

    // outward unit normal and surface element of face f at a point with inverse Jacobian inv and det J (Nanson:
    // cof(J) n_ref = det J J^{-T} n_ref), returns |cof(J) n_ref|
    template <int dim>
    __device__ __forceinline__ double face_normal(int f, double det, const double inv[dim][dim], double n[dim])
    {
      const int a = f >> 1;
      const double sgn = (f & 1) ? 1.0 : -1.0;
      double c[dim], l2 = 0.0;
#pragma unroll
      for (int i = 0; i < dim; ++i)
        {
          c[i] = sgn * det * inv[a][i];
          l2 += c[i] * c[i];
        }
      const double len = sqrt(l2);
#pragma unroll
      for (int i = 0; i < dim; ++i)
        n[i] = c[i] / len;
      return len;
    }

    // ---- compute_load: thread <-> (cell, face), QGauss<dim-1>(3), undegraded stress with the global Lame coefficients
    template <int dim>
    __global__ __launch_bounds__(256) void k_face_load(DevView v, double lam, double mu, const int32_t *__restrict__ cells,
                                                       const uint8_t *__restrict__ faces, long long n,
                                                       double *__restrict__ partial /* [gridDim.x][3] */)
    {
      constexpr int nv = 1 << dim, nq = dim == 2 ? 3 : 9;
      const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      double acc[3] = {0.0, 0.0, 0.0};
      if (i < n)
        {
          const long long cell = cells[i];
          const int f = faces[i];
          double x[nv][dim], U[nv][dim], PH[nv];
          load_geometry<dim>(v, cell, x);
          load_state<dim>(v, cell, U, PH);
#pragma unroll 1
          for (int q = 0; q < nq; ++q)
            {
              double xi[dim], N[nv], g[nv][dim], inv[dim][dim], nrm[dim];
              const double w = face_point<dim>(f, q, xi);
              const double det = eval_point<dim>(x, xi, N, g, inv);
              const double JxW = face_normal<dim>(f, det, inv, nrm) * w;
              double gu[dim][dim];
#pragma unroll
              for (int c = 0; c < dim; ++c)
#pragma unroll
                for (int d = 0; d < dim; ++d)
                  {
                    double s = 0.0;
#pragma unroll
                    for (int b = 0; b < nv; ++b)
                      s += U[b][c] * g[b][d];
                    gu[c][d] = s;
                  }
              double trE = 0.0;
#pragma unroll
              for (int a = 0; a < dim; ++a)
                trE += gu[a][a];
#pragma unroll
              for (int r = 0; r < dim; ++r)
                {
                  double s = 0.0;
#pragma unroll
                  for (int c = 0; c < dim; ++c)
                    {
                      const double sig = (r == c ? lam * trE : 0.0) + 2.0 * mu * (0.5 * (gu[r][c] + gu[c][r]));
                      s += sig * nrm[c];
                    }
                  acc[r] += s * JxW;
                }
            }
        }
      const double r = block_reduce(acc, Sum<double>{});
      if (threadIdx.x < 3)
        partial[(long long)blockIdx.x * 3 + threadIdx.x] = r;
    }

    // ---- phi error against ExactPhiSneddon (cracks.cc:418-450, l_0 = 1): thread <-> cell, QGauss(3)^dim
    template <int dim>
    __global__ __launch_bounds__(256) void k_sneddon_phi_error(DevView v, double alpha_eps, const uint8_t *__restrict__ cell_owned,
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
              double p[dim], ph = 0.0;
#pragma unroll
              for (int d = 0; d < dim; ++d)
                p[d] = 0.0;
#pragma unroll
              for (int b = 0; b < nv; ++b)
                {
                  ph += PH[b] * N[b];
#pragma unroll
                  for (int d = 0; d < dim; ++d)
                    p[d] += x[b][d] * N[b];
                }
              double dist;
              if (p[0] < -1.0 || p[0] > 1.0)
                {
                  const double dx = p[0] - (p[0] < -1.0 ? -1.0 : 1.0);
                  double s = dx * dx;
#pragma unroll
                  for (int d = 1; d < dim; ++d)
                    s += p[d] * p[d];
                  dist = sqrt(s);
                }
              else
                {
                  double s = 0.0;
#pragma unroll
                  for (int d = 1; d < dim; ++d)
                    s += p[d] * p[d];
                  dist = sqrt(s);
                }
              const double diff = (1.0 - exp(-dist / alpha_eps)) - ph;
              acc[0] += diff * diff * (det * w);
            }
        }
      const double r = block_reduce(acc, Sum<double>{});
      if (threadIdx.x < 3)
        partial[(long long)blockIdx.x * 3 + threadIdx.x] = r;
    }

    // ---- COD, geometry pass.  Which lines does face f of an owned cell match (compute_cod, cracks.cc:3493-3513)?
    // The reference's three predicates are each monotone in the line position, so on ascending lines the matches form
    // one index range [lo, hi), found by binary searches that evaluate the reference's comparisons exactly.
    template <class P>
    __device__ __forceinline__ int first_true(int n, P pred)
    {
      int lo = 0, hi = n;
      while (lo < hi)
        {
          const int mid = (lo + hi) >> 1;
          if (pred(mid))
            hi = mid;
          else
            lo = mid + 1;
        }
      return lo;
    }

    template <int dim>
    __device__ __forceinline__ void cell_face_ranges(const DevView &v, long long cell, const double *__restrict__ lines, int n_lines,
                                                     double eps, int lo[2 * dim], int hi[2 * dim])
    {
#pragma clang fp contract(off)
      constexpr int nv = 1 << dim;
      double x[nv][dim];
      load_geometry<dim>(v, cell, x);
      // cell->center() (vertex mean) and cell->diameter() (longest vertex diagonal)
      double cx = 0.0;
#pragma unroll
      for (int b = 0; b < nv; ++b)
        cx += x[b][0];
      cx = cx / nv;
      double diam = 0.0;
#pragma unroll
      for (int b = 0; b < nv / 2; ++b)
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
      const double cmin = cx - diam, cmax = cx + diam;
      // not (cell_x - diameter > line) and not (cell_x + diameter < line)
      const int c_lo = first_true(n_lines, [&](int i) { return !(cmin > lines[i]); });
      const int c_hi = first_true(n_lines, [&](int i) { return cmax < lines[i]; });
#pragma unroll 1
      for (int f = 0; f < 2 * dim; ++f)
        {
          lo[f] = hi[f] = 0;
          if (c_lo >= c_hi)
            continue;
          double xi[dim], N[nv], g[nv][dim], inv[dim][dim], nrm[dim];
          face_point<dim>(f, 0, xi);
          const double det = eval_point<dim>(x, xi, N, g, inv);
          face_normal<dim>(f, det, inv, nrm);
          if (fabs(nrm[0]) < 0.5)
            continue; // |normal_vector(0) * e_x| < 0.5
          double q0x = 0.0;
#pragma unroll
          for (int b = 0; b < nv; ++b)
            q0x += x[b][0] * N[b];
          // q0x < line + eps  and  q0x > line - eps
          const int f_lo = first_true(n_lines, [&](int i) { return q0x < lines[i] + eps; });
          const int f_hi = first_true(n_lines, [&](int i) { return !(q0x > lines[i] - eps); });
          lo[f] = max(c_lo, f_lo);
          hi[f] = max(lo[f], min(c_hi, f_hi));
        }
    }

    template <int dim>
    __global__ __launch_bounds__(256) void k_cod_count(DevView v, const uint8_t *__restrict__ cell_owned, const double *__restrict__ lines,
                                                       int n_lines, double eps, int *__restrict__ count /* [n_cells] */)
    {
      const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (cell >= v.n_cells)
        return;
      int total = 0;
      if (!cell_owned || cell_owned[cell])
        {
          int lo[2 * dim], hi[2 * dim];
          cell_face_ranges<dim>(v, cell, lines, n_lines, eps, lo, hi);
#pragma unroll
          for (int f = 0; f < 2 * dim; ++f)
            total += hi[f] - lo[f];
        }
      count[cell] = total;
    }

    // entries of a cell from its offset on, in (face, line) order; the stable sort by line then yields (line, cell, face)
    template <int dim>
    __global__ __launch_bounds__(256) void k_cod_fill(DevView v, const uint8_t *__restrict__ cell_owned, const double *__restrict__ lines,
                                                      int n_lines, double eps, const long long *__restrict__ offset,
                                                      int32_t *__restrict__ key, long long *__restrict__ entry)
    {
      const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (cell >= v.n_cells || (cell_owned && !cell_owned[cell]))
        return;
      long long o = offset[cell];
      if (o == offset[cell + 1])
        return;
      int lo[2 * dim], hi[2 * dim];
      cell_face_ranges<dim>(v, cell, lines, n_lines, eps, lo, hi);
      for (int f = 0; f < 2 * dim; ++f)
        for (int l = lo[f]; l < hi[f]; ++l, ++o)
          {
            key[o] = l;
            entry[o] = cell * (2 * dim) + f;
          }
    }

    // line_ptr[l] = first entry of line l (lower bound in the sorted keys), l = 0 .. n_lines
    __global__ __launch_bounds__(256) void k_cod_line_ptr(const int32_t *__restrict__ key, long long n, int n_lines,
                                                          long long *__restrict__ line_ptr)
    {
      const int l = blockIdx.x * blockDim.x + threadIdx.x;
      if (l > n_lines)
        return;
      long long lo = 0, hi = n;
      while (lo < hi)
        {
          const long long mid = (lo + hi) >> 1;
          if (key[mid] >= l)
            hi = mid;
          else
            lo = mid + 1;
        }
      line_ptr[l] = lo;
    }

    // ---- COD, value pass: one wave per line; lane k sums the line's entries k, k + 64, ... in order, then the wave adds the
    // lanes by xor-shuffles (fixed order).  cod[l] = sum 0.5 u . grad phi JxW over the line's faces (cracks.cc:3517-3532)
    template <int dim>
    __global__ __launch_bounds__(256) void k_cod_values(DevView v, const long long *__restrict__ line_ptr, const long long *__restrict__ entry,
                                                        int n_lines, double *__restrict__ cod)
    {
      constexpr int nv = 1 << dim, nq = dim == 2 ? 3 : 9;
      const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
      const int lane = threadIdx.x & 63;
      if (l >= n_lines) // uniform per wave: no block-wide barrier below
        return;
      double acc = 0.0;
      for (long long j = line_ptr[l] + lane; j < line_ptr[l + 1]; j += 64)
        {
          const long long cf = entry[j];
          const long long cell = cf / (2 * dim);
          const int f = (int)(cf - cell * (2 * dim));
          double x[nv][dim], U[nv][dim], PH[nv];
          load_geometry<dim>(v, cell, x);
          load_state<dim>(v, cell, U, PH);
          double face = 0.0;
#pragma unroll 1
          for (int q = 0; q < nq; ++q)
            {
              double xi[dim], N[nv], g[nv][dim], inv[dim][dim], nrm[dim];
              const double w = face_point<dim>(f, q, xi);
              const double det = eval_point<dim>(x, xi, N, g, inv);
              const double JxW = face_normal<dim>(f, det, inv, nrm) * w;
              double ug = 0.0;
#pragma unroll
              for (int c = 0; c < dim; ++c)
                {
                  double uq = 0.0, gp = 0.0;
#pragma unroll
                  for (int b = 0; b < nv; ++b)
                    {
                      uq += U[b][c] * N[b];
                      gp += PH[b] * g[b][c];
                    }
                  ug += uq * gp;
                }
              face += 0.5 * ug * JxW;
            }
          acc += face;
        }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        acc += __shfl_xor(acc, off);
      if (lane == 0)
        cod[l] = acc;
    }

    // device buffer in the context's allocation list (freed by pfm_ctx_destroy); `old` is released first
    template <class T>
    int realloc_owned(pfm_ctx *c, T *&p, size_t n)
    {
      if (p)
        {
          (void)hipStreamSynchronize(c->stream);
          c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void *)p), c->allocs.end());
          (void)hipFree(p);
          p = nullptr;
        }
      if (hipMalloc((void **)&p, sizeof(T) * std::max<size_t>(n, 1)) != hipSuccess)
        {
          p = nullptr;
          return PFM_ERR_NOMEM;
        }
      c->allocs.push_back(p);
      return PFM_OK;
    }

    // block partials of the 3-wide reductions: [nb][3] + the 3 results (shared with pfm_functionals, same stream)
    int ensure_partial(pfm_ctx *c, unsigned nb)
    {
      return dev_buf_reserve(c, c->buf_partial, sizeof(double) * 3 * ((size_t)nb + 1), "partial sums");
    }

    // second stage + copy of `width` results to the host; synchronous
    int finish_reduce3(pfm_ctx *c, unsigned nb, double *out, int width, const char *what)
    {
      double *d_partial = c->buf_partial.as<double>(), *d_out = d_partial + 3 * (size_t)nb;
      hipLaunchKernelGGL((k_reduce_final<double, 3, Sum<double>>), dim3(1), dim3(256), 0, c->stream, d_partial, (long long)nb, d_out);
      if (hipGetLastError() != hipSuccess)
        return fail(c, PFM_ERR_HIP, std::string(what) + " launch");
      double h[3];
      if (hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
          hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, PFM_ERR_HIP, std::string(what) + " copy");
      for (int k = 0; k < width; ++k)
        out[k] = h[k];
      return PFM_OK;
    }

    // geometry pass of pfm_cod_lines: (line, cell, face) list into c->cod
    int build_cod_list(pfm_ctx *c, const uint8_t *cell_owned, int n_lines, const double *lines, double eps)
    {
      auto &cc = c->cod;
      cc.valid = false;
      const long long NC = c->v.n_cells;
      const int dim = c->v.dim;
      uint8_t *d_owned = nullptr;
      if (int rc = upload_mask(c, cell_owned, &d_owned))
        return rc;
      double *d_lines = nullptr;
      int *d_count = nullptr;
      long long *d_offset = nullptr;
      int32_t *d_key = nullptr, *d_key_sorted = nullptr;
      long long *d_entry = nullptr;
      void *d_tmp = nullptr;
      auto cleanup = [&]() {
        (void)hipStreamSynchronize(c->stream);
        for (void *p : {(void *)d_lines, (void *)d_count, (void *)d_offset, (void *)d_key, (void *)d_key_sorted, (void *)d_entry, d_tmp})
          if (p)
            (void)hipFree(p);
      };
      auto bad = [&](int code, const char *msg) {
        cleanup();
        return fail(c, code, msg);
      };
      if (hipMalloc((void **)&d_lines, sizeof(double) * (size_t)n_lines) != hipSuccess ||
          hipMalloc((void **)&d_count, sizeof(int) * (size_t)(NC + 1)) != hipSuccess ||
          hipMalloc((void **)&d_offset, sizeof(long long) * (size_t)(NC + 1)) != hipSuccess)
        return bad(PFM_ERR_NOMEM, "hipMalloc cod geometry scratch");
      if (hipMemcpyAsync(d_lines, lines, sizeof(double) * (size_t)n_lines, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
          hipMemsetAsync(d_count, 0, sizeof(int) * (size_t)(NC + 1), c->stream) != hipSuccess)
        return bad(PFM_ERR_HIP, "cod lines upload");
      const unsigned nbc = (unsigned)((NC + 255) / 256);
      if (nbc)
        PFM_LAUNCH_DIM(dim, k_cod_count, dim3(nbc), dim3(256), c->stream, c->v, d_owned, d_lines, n_lines, eps, d_count);
      // offsets: exclusive sum over the n_cells + 1 counts (the last one is 0) -> offset[NC] = number of entries
      size_t tb_scan = 0;
      if (hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, d_count, d_offset, (int)(NC + 1), c->stream) != hipSuccess)
        return bad(PFM_ERR_HIP, "cod scan size");
      if (hipMalloc(&d_tmp, std::max<size_t>(tb_scan, 16)) != hipSuccess)
        return bad(PFM_ERR_NOMEM, "hipMalloc cod scan scratch");
      if (hipcub::DeviceScan::ExclusiveSum(d_tmp, tb_scan, d_count, d_offset, (int)(NC + 1), c->stream) != hipSuccess)
        return bad(PFM_ERR_HIP, "cod scan");
      long long n_entries = 0;
      if (hipMemcpyAsync(&n_entries, d_offset + NC, sizeof(long long), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
          hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess)
        return bad(PFM_ERR_HIP, "cod count");
      if (n_entries > INT_MAX)
        return bad(PFM_ERR_UNSUPPORTED, "more than 2^31 (line, face) matches");
      (void)hipFree(d_tmp);
      d_tmp = nullptr;
      if (realloc_owned(c, cc.d_entry, (size_t)n_entries) != PFM_OK || realloc_owned(c, cc.d_line_ptr, (size_t)n_lines + 1) != PFM_OK)
        return bad(PFM_ERR_NOMEM, "hipMalloc cod list");
      if (n_entries > 0)
        {
          if (hipMalloc((void **)&d_key, sizeof(int32_t) * (size_t)n_entries) != hipSuccess ||
              hipMalloc((void **)&d_key_sorted, sizeof(int32_t) * (size_t)n_entries) != hipSuccess ||
              hipMalloc((void **)&d_entry, sizeof(long long) * (size_t)n_entries) != hipSuccess)
            return bad(PFM_ERR_NOMEM, "hipMalloc cod sort scratch");
          PFM_LAUNCH_DIM(dim, k_cod_fill, dim3(nbc), dim3(256), c->stream, c->v, d_owned, d_lines, n_lines, eps, d_offset, d_key, d_entry);
          int end_bit = 1;
          while (end_bit < 31 && (1LL << end_bit) < (long long)n_lines)
            ++end_bit;
          size_t tb_sort = 0;
          if (hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, d_key, d_key_sorted, d_entry, cc.d_entry, (int)n_entries, 0, end_bit,
                                                 c->stream) != hipSuccess ||
              hipMalloc(&d_tmp, std::max<size_t>(tb_sort, 16)) != hipSuccess)
            return bad(PFM_ERR_NOMEM, "cod sort scratch");
          if (hipcub::DeviceRadixSort::SortPairs(d_tmp, tb_sort, d_key, d_key_sorted, d_entry, cc.d_entry, (int)n_entries, 0, end_bit,
                                                 c->stream) != hipSuccess)
            return bad(PFM_ERR_HIP, "cod sort");
        }
      hipLaunchKernelGGL(k_cod_line_ptr, dim3((unsigned)((n_lines + 1 + 255) / 256)), dim3(256), 0, c->stream, d_key_sorted,
                         n_entries, n_lines, cc.d_line_ptr);
      if (hipGetLastError() != hipSuccess)
        return bad(PFM_ERR_HIP, "cod geometry launch");
      cleanup(); // synchronises the stream
      cc.lines.assign(lines, lines + n_lines);
      cc.eps = eps;
      cc.masked = cell_owned != nullptr;
      if (cell_owned)
        cc.mask.assign(cell_owned, cell_owned + NC);
      else
        cc.mask.clear();
      cc.n_entries = n_entries;
      cc.valid = true;
      return PFM_OK;
    }

    bool cod_cache_hit(const pfm_ctx *c, const uint8_t *cell_owned, int n_lines, const double *lines, double eps)
    {
      const auto &cc = c->cod;
      if (!cc.valid || cc.eps != eps || cc.masked != (cell_owned != nullptr) || cc.lines.size() != (size_t)n_lines)
        return false;
      if (n_lines && std::memcmp(cc.lines.data(), lines, sizeof(double) * (size_t)n_lines) != 0)
        return false;
      return !cell_owned || c->v.n_cells == 0 || std::memcmp(cc.mask.data(), cell_owned, (size_t)c->v.n_cells) == 0;
    }
  } // namespace
} // namespace pfm

using namespace pfm;

extern "C"
{
  int pfm_face_load(pfm_ctx *c, int64_t n_faces, const int32_t *cells, const uint8_t *faces, double *out)
  {
    if (!c || !out || n_faces < 0 || (n_faces > 0 && (!cells || !faces)))
      return c ? fail(c, PFM_ERR_BAD_ARG, "pfm_face_load: bad arguments") : PFM_ERR_BAD_ARG;
    if (!c->have_params)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_set_params has not been called");
    const int dim = c->v.dim;
    for (int64_t i = 0; i < n_faces; ++i)
      if (cells[i] < 0 || cells[i] >= c->v.n_cells || faces[i] >= 2 * dim)
        return fail(c, PFM_ERR_BAD_ARG, "pfm_face_load: cell or face out of range at entry " + std::to_string(i));
    (void)hipSetDevice(c->device);
    const unsigned nb = (unsigned)((n_faces + 255) / 256);
    if (int rc = ensure_partial(c, nb))
      return rc;
    if (n_faces > 0)
      {
        if (int rc = dev_buf_reserve(c, c->buf_face_cells, sizeof(int32_t) * (size_t)n_faces, "face list"))
          return rc;
        if (int rc = dev_buf_reserve(c, c->buf_face_ids, (size_t)n_faces, "face list"))
          return rc;
        int32_t *d_cells = c->buf_face_cells.as<int32_t>();
        uint8_t *d_ids = c->buf_face_ids.as<uint8_t>();
        if (hipMemcpyAsync(d_cells, cells, sizeof(int32_t) * (size_t)n_faces, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_ids, faces, (size_t)n_faces, hipMemcpyHostToDevice, c->stream) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "face list upload");
        PFM_LAUNCH_DIM(dim, k_face_load, dim3(nb), dim3(256), c->stream, c->v, c->prm.lambda, c->prm.mu, d_cells, d_ids,
                       (long long)n_faces, c->buf_partial.as<double>());
      }
    return finish_reduce3(c, nb, out, dim, "k_face_load");
  }

  int pfm_cod_lines(pfm_ctx *c, const uint8_t *cell_owned, int n_lines, const double *lines, double eps, double *cod,
                    int64_t *n_faces)
  {
    if (!c || n_lines < 0 || (n_lines > 0 && (!lines || !cod || !n_faces)) || !std::isfinite(eps) || eps < 0.0)
      return c ? fail(c, PFM_ERR_BAD_ARG, "pfm_cod_lines: bad arguments") : PFM_ERR_BAD_ARG;
    if (!c->have_params)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_set_params has not been called");
    for (int i = 0; i < n_lines; ++i)
      if (!std::isfinite(lines[i]) || (i > 0 && !(lines[i - 1] < lines[i])))
        return fail(c, PFM_ERR_BAD_ARG, "pfm_cod_lines: lines must be finite and strictly ascending");
    if (n_lines == 0)
      return PFM_OK;
    (void)hipSetDevice(c->device);
    if (!cod_cache_hit(c, cell_owned, n_lines, lines, eps))
      if (int rc = build_cod_list(c, cell_owned, n_lines, lines, eps))
        return rc;
    if (int rc = ensure_partial(c, (unsigned)((n_lines + 2) / 3)))
      return rc;
    double *d_cod = c->buf_partial.as<double>(); // the partial-sum buffer holds 3 ((n_lines + 2) / 3 + 1) >= n_lines doubles
    const unsigned nb = (unsigned)((n_lines + 3) / 4);
    PFM_LAUNCH_DIM(c->v.dim, k_cod_values, dim3(nb), dim3(256), c->stream, c->v, c->cod.d_line_ptr, c->cod.d_entry, n_lines, d_cod);
    if (hipGetLastError() != hipSuccess)
      return fail(c, PFM_ERR_HIP, "k_cod_values launch");
    std::vector<long long> ptr((size_t)n_lines + 1);
    if (hipMemcpyAsync(cod, d_cod, sizeof(double) * (size_t)n_lines, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(ptr.data(), c->cod.d_line_ptr, sizeof(long long) * ptr.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "cod copy");
    for (int i = 0; i < n_lines; ++i)
      n_faces[i] = (int64_t)(ptr[i + 1] - ptr[i]);
    return PFM_OK;
  }

  int pfm_sneddon_phi_error(pfm_ctx *c, const uint8_t *cell_owned, double *sum_sq)
  {
    if (!c || !sum_sq)
      return c ? fail(c, PFM_ERR_BAD_ARG, "pfm_sneddon_phi_error: NULL output") : PFM_ERR_BAD_ARG;
    if (!c->have_params)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_set_params has not been called");
    (void)hipSetDevice(c->device);
    const unsigned nb = (unsigned)((c->v.n_cells + 255) / 256);
    if (int rc = ensure_partial(c, nb))
      return rc;
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    if (nb)
      PFM_LAUNCH_DIM(c->v.dim, k_sneddon_phi_error, dim3(nb), dim3(256), c->stream, c->v, c->prm.alpha_eps, d_owned,
                     c->buf_partial.as<double>());
    return finish_reduce3(c, nb, sum_sq, 1, "k_sneddon_phi_error");
  }
}
