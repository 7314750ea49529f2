// pfm_adapt.hip — the sweeps of the reference's refine_mesh() around the context rebuild (include/pfm_newton.h, "mesh
// adaptation"):
//
//   pfm_refine_flags        refinement indicator + level limit             cracks.cc:3902-4116
//   pfm_min_cell_diameter   determine_mesh_dependent_parameters, 1st half  cracks.cc:3824-3835
//   pfm_state_transfer      SolutionTransfer::interpolate (refinement)     cracks.cc:4137-4159
//
// All three are memory-bound gathers over the vertex-major cell table.  Counts and minima are fixed-order two-stage
// reductions, the transfer's weights are powers of two added in a fixed order and every node has one writer: repeated
// calls are bitwise identical.
#include "pfm_internal.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <string>

#include "../../include/pfm_newton.h"

namespace pfm
{
  namespace
  {
    constexpr int XFER_MAX_VECTORS = 8;

    struct RefineCrit // pfm_refine_criteria by value
    {
      double thr;
      double lo[3], hi[3];
      int use_box, max_level;
    };

    struct XferVecs
    {
      const double *src[XFER_MAX_VECTORS];
      double *dst[XFER_MAX_VECTORS];
      int n;
    };

    // ---- refinement indicator: thread <-> cell.  partial[block] = flagged cells of the block
    template <int dim>
    __global__ __launch_bounds__(256) void k_refine_flags(DevView v, RefineCrit cr, const uint8_t *__restrict__ cell_owned,
                                                          const uint8_t *__restrict__ cell_level, uint8_t *__restrict__ flags,
                                                          unsigned long long *__restrict__ partial)
    {
      constexpr int nv = 1 << dim;
      __shared__ unsigned s_cnt[4];
      const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      int f = 0;
      if (cell < v.n_cells && (!cell_owned || cell_owned[cell]))
        {
#pragma unroll
          for (int b = 0; b < nv; ++b)
            {
              const int n = v.conn[(long long)b * v.n_cells + cell];
              if (v.phi[n] < cr.thr) // false for a NaN on either side
                f = 1;
              if (cr.use_box)
                {
                  bool inside = true;
#pragma unroll
                  for (int d = 0; d < dim; ++d)
                    {
                      const double x = v.coords[(long long)d * v.n_nodes + n];
                      inside = inside && x >= cr.lo[d] && x <= cr.hi[d];
                    }
                  if (inside)
                    f = 1;
                }
            }
          if (f && cr.max_level >= 0 && (int)cell_level[cell] == cr.max_level)
            f = 0;
        }
      if (cell < v.n_cells)
        flags[cell] = (uint8_t)f;
      const unsigned long long m = __ballot(f);
      if ((threadIdx.x & 63) == 0)
        s_cnt[threadIdx.x >> 6] = (unsigned)__popcll(m);
      __syncthreads();
      if (threadIdx.x == 0)
        partial[blockIdx.x] = (unsigned long long)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }

    __global__ __launch_bounds__(256) void k_sum_counts(const unsigned long long *__restrict__ partial, long long n,
                                                        unsigned long long *__restrict__ out)
    {
      __shared__ unsigned long long s[256];
      unsigned long long r = 0;
      for (long long i = threadIdx.x; i < n; i += 256)
        r += partial[i];
      s[threadIdx.x] = r;
      __syncthreads();
      for (int w = 128; w >= 1; w >>= 1)
        {
          if ((int)threadIdx.x < w)
            s[threadIdx.x] += s[threadIdx.x + w];
          __syncthreads();
        }
      if (threadIdx.x == 0)
        out[0] = s[0];
    }

    // square of cell->diameter(): the largest of the 2^(dim-1) vertex diagonals, every operation rounded on its own
    template <int dim>
    __device__ __forceinline__ double diameter_sq(const double x[1 << dim][dim])
    {
#pragma clang fp contract(off)
      constexpr int nv = 1 << dim;
      double best = 0.0;
#pragma unroll
      for (int b = 0; b < nv / 2; ++b)
        {
          double s = 0.0;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            {
              const double e = x[b][d] - x[nv - 1 - b][d];
              s += e * e;
            }
          best = fmax(best, s);
        }
      return best;
    }

    template <int dim>
    __device__ __forceinline__ void load_vertices(const DevView &v, long long cell, double x[1 << dim][dim])
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

    // ---- minimum of diameter^2 over the masked cells (the root is taken once, on the host)
    template <int dim>
    __global__ __launch_bounds__(256) void k_min_diameter_sq(DevView v, const uint8_t *__restrict__ cell_owned, double *__restrict__ partial)
    {
      __shared__ double s_min[4];
      const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      double r = HUGE_VAL;
      if (cell < v.n_cells && (!cell_owned || cell_owned[cell]))
        {
          double x[1 << dim][dim];
          load_vertices<dim>(v, cell, x);
          r = diameter_sq<dim>(x);
        }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        r = fmin(r, __shfl_xor(r, off));
      if ((threadIdx.x & 63) == 0)
        s_min[threadIdx.x >> 6] = r;
      __syncthreads();
      if (threadIdx.x == 0)
        partial[blockIdx.x] = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
    }

    __global__ __launch_bounds__(256) void k_min_reduce(const double *__restrict__ partial, long long n, double *__restrict__ out)
    {
      __shared__ double s_min[4];
      double r = HUGE_VAL;
      for (long long i = threadIdx.x; i < n; i += 256)
        r = fmin(r, partial[i]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        r = fmin(r, __shfl_xor(r, off));
      if ((threadIdx.x & 63) == 0)
        s_min[threadIdx.x >> 6] = r;
      __syncthreads();
      if (threadIdx.x == 0)
        out[0] = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
    }

    // reference coordinate of vertex vtx of a dst cell inside its parent: (child bit d + vertex bit d) / 2, or the vertex
    // itself where the cell is identical to its parent (child == 255)
    __device__ __forceinline__ double xfer_xi(int child, int vtx, int d)
    {
      const int vb = (vtx >> d) & 1;
      return child == 255 ? (double)vb : 0.5 * (double)(((child >> d) & 1) + vb);
    }

    template <int dim>
    __device__ __forceinline__ double q1_weight(int b, const double xi[dim])
    {
      double w = 1.0;
#pragma unroll
      for (int d = 0; d < dim; ++d)
        w *= ((b >> d) & 1) ? xi[d] : (1.0 - xi[d]);
      return w;
    }

    // ---- transfer, pass 1: thread <-> dst cell.  Checks the relation against the coordinates (bad[0] = 1 on a mismatch)
    // and leaves the lowest incident dst cell of every dst node in owner[]
    template <int dim>
    __global__ __launch_bounds__(256) void k_xfer_check(DevView s, DevView d, const int32_t *__restrict__ parent,
                                                        const uint8_t *__restrict__ child, int32_t *__restrict__ owner,
                                                        int *__restrict__ bad)
    {
      constexpr int nv = 1 << dim;
      const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (c >= d.n_cells)
        return;
      const long long p = parent[c];
      const int ch = child[c];
      if (p < 0 || p >= s.n_cells || (ch != 255 && ch >= nv))
        {
          bad[0] = 1;
          return;
        }
      double xs[nv][dim];
      load_vertices<dim>(s, p, xs);
      const double tol = 1e-10 * sqrt(diameter_sq<dim>(xs));
      bool ok = true;
#pragma unroll
      for (int vtx = 0; vtx < nv; ++vtx)
        {
          const int n = d.conn[(long long)vtx * d.n_cells + c];
          atomicMin(&owner[n], (int32_t)c);
          double xi[dim], img[dim];
#pragma unroll
          for (int k = 0; k < dim; ++k)
            {
              xi[k] = xfer_xi(ch, vtx, k);
              img[k] = 0.0;
            }
#pragma unroll
          for (int b = 0; b < nv; ++b)
            {
              const double w = q1_weight<dim>(b, xi);
#pragma unroll
              for (int k = 0; k < dim; ++k)
                img[k] += w * xs[b][k];
            }
          double dist = 0.0;
#pragma unroll
          for (int k = 0; k < dim; ++k)
            {
              const double e = d.coords[(long long)k * d.n_nodes + n] - img[k];
              dist += e * e;
            }
          ok = ok && (sqrt(dist) <= tol); // a NaN fails
        }
      if (!ok)
        bad[0] = 1;
    }

    __device__ __forceinline__ long long dof_of(int layout, int dim, long long n_nodes, long long node, int comp)
    {
      if (layout == PFM_LAYOUT_INTERLEAVED)
        return node * (dim + 1) + comp;
      return comp < dim ? node * dim + comp : n_nodes * dim + node;
    }

    // ---- transfer, pass 2: thread <-> (vertex, dst cell) in the order of the cell table; the thread of the node's owner
    // cell writes every component of every vector
    template <int dim>
    __global__ __launch_bounds__(256) void k_xfer_write(DevView s, DevView d, const int32_t *__restrict__ parent,
                                                        const uint8_t *__restrict__ child, const int32_t *__restrict__ owner,
                                                        XferVecs vecs)
    {
#pragma clang fp contract(off)
      constexpr int nv = 1 << dim;
      const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (i >= d.n_cells * nv)
        return;
      const int vtx = (int)(i / d.n_cells);
      const long long c = i - (long long)vtx * d.n_cells;
      const int n = d.conn[i];
      if ((long long)owner[n] != c)
        return;
      for (int a = 0; a < vtx; ++a) // a degenerate cell that lists the node twice: its first vertex writes
        if (d.conn[(long long)a * d.n_cells + c] == n)
          return;
      const long long p = parent[c];
      const int ch = child[c];
      double xi[dim], w[nv];
      int ns[nv];
#pragma unroll
      for (int k = 0; k < dim; ++k)
        xi[k] = xfer_xi(ch, vtx, k);
#pragma unroll
      for (int b = 0; b < nv; ++b)
        {
          w[b] = q1_weight<dim>(b, xi);
          ns[b] = w[b] != 0.0 ? s.conn[(long long)b * s.n_cells + p] : 0;
        }
      for (int k = 0; k < vecs.n; ++k)
        {
          const double *__restrict__ src = vecs.src[k];
          double *__restrict__ dst = vecs.dst[k];
#pragma unroll
          for (int comp = 0; comp <= dim; ++comp)
            {
              double val = 0.0;
              bool first = true;
#pragma unroll
              for (int b = 0; b < nv; ++b)
                if (w[b] != 0.0)
                  {
                    const double t = w[b] * src[dof_of(s.layout, dim, s.n_nodes, ns[b], comp)];
                    val = first ? t : val + t;
                    first = false;
                  }
              dst[dof_of(d.layout, dim, d.n_nodes, n, comp)] = val;
            }
        }
    }

    int fail(pfm_ctx *c, int code, const std::string &msg)
    {
      if (c)
        c->err = msg;
      return code;
    }

    // the context's adaptation scratch, at least `bytes` large (grow-only; contents undefined)
    int adapt_scratch(pfm_ctx *c, size_t bytes, char **p)
    {
      if (!c->d_adapt || c->adapt_bytes < bytes)
        {
          if (c->d_adapt)
            {
              (void)hipStreamSynchronize(c->stream);
              c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), c->d_adapt), c->allocs.end());
              (void)hipFree(c->d_adapt);
              c->d_adapt = nullptr;
              c->adapt_bytes = 0;
            }
          if (hipMalloc(&c->d_adapt, std::max<size_t>(bytes, 256)) != hipSuccess)
            {
              c->d_adapt = nullptr;
              return fail(c, PFM_ERR_NOMEM, "hipMalloc adaptation scratch");
            }
          c->allocs.push_back(c->d_adapt);
          c->adapt_bytes = std::max<size_t>(bytes, 256);
        }
      *p = static_cast<char *>(c->d_adapt);
      return PFM_OK;
    }

    constexpr size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

    int upload_mask(pfm_ctx *c, const uint8_t *cell_owned, uint8_t **d_owned)
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
  } // namespace
} // namespace pfm

using namespace pfm;

extern "C"
{
  int pfm_refine_flags(pfm_ctx *c, const pfm_refine_criteria *crit, const uint8_t *cell_owned, const uint8_t *cell_level,
                       uint8_t *flags, int64_t *n_flagged)
  {
    if (!c || !crit || !n_flagged)
      return c ? fail(c, PFM_ERR_BAD_ARG, "pfm_refine_flags: NULL criteria or output") : PFM_ERR_BAD_ARG;
    const long long NC = c->v.n_cells;
    if ((NC > 0 && !flags) || (crit->max_level >= 0 && NC > 0 && !cell_level))
      return fail(c, PFM_ERR_BAD_ARG, "pfm_refine_flags: NULL flags, or a level limit without cell levels");
    if (crit->max_level > 255)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_refine_flags: max_level does not fit the level bytes");
    RefineCrit cr{};
    cr.thr = crit->phi_threshold;
    cr.use_box = crit->use_box != 0;
    cr.max_level = crit->max_level;
    for (int d = 0; d < 3; ++d)
      {
        cr.lo[d] = crit->box_lo[d];
        cr.hi[d] = crit->box_hi[d];
      }
    (void)hipSetDevice(c->device);
    const unsigned nb = (unsigned)((NC + 255) / 256);
    // scratch: flags [NC] | levels [NC] | block counts [nb] + the total
    const size_t o_level = align256((size_t)NC), o_part = o_level + align256((size_t)NC);
    char *base = nullptr;
    if (int rc = adapt_scratch(c, o_part + sizeof(unsigned long long) * ((size_t)nb + 1), &base))
      return rc;
    uint8_t *d_flags = reinterpret_cast<uint8_t *>(base), *d_level = nullptr;
    unsigned long long *d_part = reinterpret_cast<unsigned long long *>(base + o_part);
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    if (crit->max_level >= 0 && NC > 0)
      {
        d_level = reinterpret_cast<uint8_t *>(base + o_level);
        if (hipMemcpyAsync(d_level, cell_level, (size_t)NC, hipMemcpyHostToDevice, c->stream) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "cell level upload");
      }
    if (nb)
      {
        if (c->v.dim == 2)
          hipLaunchKernelGGL(k_refine_flags<2>, dim3(nb), dim3(256), 0, c->stream, c->v, cr, d_owned, d_level, d_flags, d_part);
        else
          hipLaunchKernelGGL(k_refine_flags<3>, dim3(nb), dim3(256), 0, c->stream, c->v, cr, d_owned, d_level, d_flags, d_part);
      }
    hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(256), 0, c->stream, d_part, (long long)nb, d_part + nb);
    if (hipGetLastError() != hipSuccess)
      return fail(c, PFM_ERR_HIP, "k_refine_flags launch");
    unsigned long long total = 0;
    if ((NC > 0 && hipMemcpyAsync(flags, d_flags, (size_t)NC, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipMemcpyAsync(&total, d_part + nb, sizeof(total), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "refine flags copy");
    *n_flagged = (int64_t)total;
    return PFM_OK;
  }

  int pfm_min_cell_diameter(pfm_ctx *c, const uint8_t *cell_owned, double *h_min)
  {
    if (!c || !h_min)
      return c ? fail(c, PFM_ERR_BAD_ARG, "pfm_min_cell_diameter: NULL output") : PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    const unsigned nb = (unsigned)((c->v.n_cells + 255) / 256);
    char *base = nullptr;
    if (int rc = adapt_scratch(c, sizeof(double) * ((size_t)nb + 1), &base))
      return rc;
    double *d_part = reinterpret_cast<double *>(base);
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    if (nb)
      {
        if (c->v.dim == 2)
          hipLaunchKernelGGL(k_min_diameter_sq<2>, dim3(nb), dim3(256), 0, c->stream, c->v, d_owned, d_part);
        else
          hipLaunchKernelGGL(k_min_diameter_sq<3>, dim3(nb), dim3(256), 0, c->stream, c->v, d_owned, d_part);
      }
    hipLaunchKernelGGL(k_min_reduce, dim3(1), dim3(256), 0, c->stream, d_part, (long long)nb, d_part + nb);
    if (hipGetLastError() != hipSuccess)
      return fail(c, PFM_ERR_HIP, "k_min_diameter_sq launch");
    double sq = 0.0;
    if (hipMemcpyAsync(&sq, d_part + nb, sizeof(sq), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "min diameter copy");
    *h_min = std::sqrt(sq); // sqrt is monotone and correctly rounded: min of the roots = root of the min
    return PFM_OK;
  }

  int pfm_state_transfer(pfm_ctx *src, pfm_ctx *dst, const int32_t *parent_cell, const uint8_t *child, int n_vectors,
                         const double *const *d_src, double *const *d_dst)
  {
    if (!src || !dst)
      return dst ? fail(dst, PFM_ERR_BAD_ARG, "pfm_state_transfer: NULL context") : PFM_ERR_BAD_ARG;
    if (n_vectors < 1 || !d_src || !d_dst || (dst->v.n_cells > 0 && (!parent_cell || !child)))
      return fail(dst, PFM_ERR_BAD_ARG, "pfm_state_transfer: bad arguments");
    if (n_vectors > XFER_MAX_VECTORS)
      return fail(dst, PFM_ERR_UNSUPPORTED, "pfm_state_transfer: more than 8 vectors in one call");
    XferVecs vecs{};
    vecs.n = n_vectors;
    for (int k = 0; k < n_vectors; ++k)
      {
        if (!d_src[k] || !d_dst[k])
          return fail(dst, PFM_ERR_BAD_ARG, "pfm_state_transfer: NULL vector");
        vecs.src[k] = d_src[k];
        vecs.dst[k] = d_dst[k];
      }
    if (src->v.n_owned != src->v.n_nodes || dst->v.n_owned != dst->v.n_nodes)
      return fail(dst, PFM_ERR_UNSUPPORTED, "pfm_state_transfer: partitioned context (the transfer across a repartition is the host's)");
    if (src->device != dst->device || src->v.dim != dst->v.dim || src->v.layout != dst->v.layout)
      return fail(dst, PFM_ERR_UNSUPPORTED, "pfm_state_transfer: contexts differ in device, dimension or layout");
    const long long NC = dst->v.n_cells;
    if (NC > INT_MAX || src->v.n_cells > INT_MAX)
      return fail(dst, PFM_ERR_UNSUPPORTED, "pfm_state_transfer: more than 2^31 cells");
    if (NC == 0)
      return PFM_OK;
    (void)hipSetDevice(dst->device);
    const int dim = dst->v.dim, nv = 1 << dim;
    // scratch of dst: parent [NC] int32 | owner [n_nodes] int32 | child [NC] | mismatch word
    const size_t o_owner = align256(sizeof(int32_t) * (size_t)NC);
    const size_t o_child = o_owner + align256(sizeof(int32_t) * (size_t)dst->v.n_nodes);
    const size_t o_bad = o_child + align256((size_t)NC);
    char *base = nullptr;
    if (int rc = adapt_scratch(dst, o_bad + 256, &base))
      return rc;
    int32_t *d_parent = reinterpret_cast<int32_t *>(base), *d_owner = reinterpret_cast<int32_t *>(base + o_owner);
    uint8_t *d_child = reinterpret_cast<uint8_t *>(base + o_child);
    int *d_bad = reinterpret_cast<int *>(base + o_bad);
    // the source vectors were written on src's stream
    if (src->stream != dst->stream && hipStreamSynchronize(src->stream) != hipSuccess)
      return fail(dst, PFM_ERR_HIP, "pfm_state_transfer: source stream");
    hipStream_t st = dst->stream;
    if (hipMemcpyAsync(d_parent, parent_cell, sizeof(int32_t) * (size_t)NC, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_child, child, (size_t)NC, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetD32Async((hipDeviceptr_t)d_owner, INT_MAX, (size_t)dst->v.n_nodes, st) != hipSuccess ||
        hipMemsetAsync(d_bad, 0, sizeof(int), st) != hipSuccess)
      return fail(dst, PFM_ERR_HIP, "pfm_state_transfer: relation upload");
    const unsigned nbc = (unsigned)((NC + 255) / 256);
    if (dim == 2)
      hipLaunchKernelGGL(k_xfer_check<2>, dim3(nbc), dim3(256), 0, st, src->v, dst->v, d_parent, d_child, d_owner, d_bad);
    else
      hipLaunchKernelGGL(k_xfer_check<3>, dim3(nbc), dim3(256), 0, st, src->v, dst->v, d_parent, d_child, d_owner, d_bad);
    if (hipGetLastError() != hipSuccess)
      return fail(dst, PFM_ERR_HIP, "k_xfer_check launch");
    int bad = 0;
    if (hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return fail(dst, PFM_ERR_HIP, "pfm_state_transfer: check copy");
    if (bad)
      return fail(dst, PFM_ERR_BAD_ARG,
                  "pfm_state_transfer: the (parent_cell, child) relation does not match the meshes (index or child number out of "
                  "range, or a vertex off the Q1 image of its parent)");
    const long long n_threads = NC * nv;
    const unsigned nbw = (unsigned)((n_threads + 255) / 256);
    if (dim == 2)
      hipLaunchKernelGGL(k_xfer_write<2>, dim3(nbw), dim3(256), 0, st, src->v, dst->v, d_parent, d_child, d_owner, vecs);
    else
      hipLaunchKernelGGL(k_xfer_write<3>, dim3(nbw), dim3(256), 0, st, src->v, dst->v, d_parent, d_child, d_owner, vecs);
    if (hipGetLastError() != hipSuccess)
      return fail(dst, PFM_ERR_HIP, "k_xfer_write launch");
    return PFM_OK;
  }
}
