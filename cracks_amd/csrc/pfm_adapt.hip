// pfm_adapt.hip — the sweeps of the reference's refine_mesh() around the context rebuild (include/pfm_newton.h, "mesh
// adaptation"):
//
//   pfm_refine_flags        refinement indicator + level limit             cracks.cc:3902-4116
//   pfm_min_cell_diameter   determine_mesh_dependent_parameters, 1st half  cracks.cc:3824-3835
//   pfm_state_transfer      SolutionTransfer::interpolate (refinement)     cracks.cc:4137-4159
//   pfm_kelly_indicator     KellyErrorEstimator::estimate                  cracks.cc:4074-4083
//   pfm_indicator_select    the threshold of refine_and_coarsen_fixed_number (and pfm_indicator_count for a distributed host)
//   pfm_refine_flags_mix    RefinementStrategy::mix                        cracks.cc:4043-4116
//
// The first three are memory-bound gathers over the vertex-major cell table.  Counts and minima are the two-stage
// reductions of pfm_reduce.h, the transfer's weights are powers of two added in a fixed order and every node has one writer:
// repeated calls are bitwise identical.  Cell geometry, q1_weight and dof_of are pfm_q1_point.h, the host helpers pfm_entry.h.
#include "pfm_entry.h"
#include "pfm_q1_point.h"
#include "pfm_reduce.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
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

    RefineCrit make_crit(const pfm_refine_criteria &crit, int max_level)
    {
      RefineCrit cr{};
      cr.thr = crit.phi_threshold;
      cr.use_box = crit.use_box != 0;
      cr.max_level = max_level;
      for (int d = 0; d < 3; ++d)
        {
          cr.lo[d] = crit.box_lo[d];
          cr.hi[d] = crit.box_hi[d];
        }
      return cr;
    }

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
      const unsigned long long total = block_count(f);
      if (threadIdx.x == 0)
        partial[blockIdx.x] = total;
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

    // ---- minimum of diameter^2 over the masked cells (the root is taken once, on the host)
    template <int dim>
    __global__ __launch_bounds__(256) void k_min_diameter_sq(DevView v, const uint8_t *__restrict__ cell_owned, double *__restrict__ partial)
    {
      const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      double r[1] = {HUGE_VAL};
      if (cell < v.n_cells && (!cell_owned || cell_owned[cell]))
        {
          double x[1 << dim][dim];
          load_geometry<dim>(v, cell, x);
          r[0] = diameter_sq<dim>(x);
        }
      const double m = block_reduce(r, Min{});
      if (threadIdx.x == 0)
        partial[blockIdx.x] = m;
    }

    // reference coordinate of vertex vtx of a dst cell inside its parent: (child bit d + vertex bit d) / 2, or the vertex
    // itself where the cell is identical to its parent (child == 255)
    __device__ __forceinline__ double xfer_xi(int child, int vtx, int d)
    {
      const int vb = (vtx >> d) & 1;
      return child == 255 ? (double)vb : 0.5 * (double)(((child >> d) & 1) + vb);
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
      load_geometry<dim>(s, p, xs);
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

    // =================================================================================================================
    // RefinementStrategy::mix (cracks.cc:4043-4103): face-neighbour table, Kelly indicator, exact top-k selection
    // =================================================================================================================

    // ---- face-neighbour table.  A face is thread t = f * n_cells + cell (coalesced reads of the vertex-major cell table);
    // its key is the ascending list of its 2^(dim-1) nodes.  Build: every face enters an open-addressing table (two occupants
    // per key: integer compare-and-swap, the relation that comes out does not depend on who came first); a face with two
    // occupants has a neighbour of its own level; an unmatched face with a hanging vertex looks up the union of its other
    // vertices and the parents of the hanging ones -- the face of the coarser neighbour, which in turn collects its fine
    // faces in a side list (sorted by fine cell afterwards).
    constexpr uint32_t FT_EMPTY = 0xffffffffu, FT_MULTI = 0xfffffffeu;
    enum
    {
      REL_NONE = 0,  // no neighbour among the local cells: boundary, slit lip, cell of another rank
      REL_SAME = 1,  // nbr = the cell of the same level across the face
      REL_FINE = 2,  // nbr = the coarser cell; this face is one subface of its face
      REL_COARSE = 3 // nbr = entry of the side list: 2^(dim-1) fine faces, cell * 2 dim + face, ascending (FT_EMPTY: not local)
    };

    __device__ __forceinline__ void sort2(int &a, int &b)
    {
      const int lo = min(a, b), hi = max(a, b);
      a = lo;
      b = hi;
    }

    template <int dim>
    __device__ __forceinline__ void sort_key(int key[1 << (dim - 1)])
    {
      sort2(key[0], key[1]);
      if (dim == 3)
        {
          sort2(key[2], key[3]);
          sort2(key[0], key[2]);
          sort2(key[1], key[3]);
          sort2(key[1], key[2]);
        }
    }

    // nodes of face f of a cell: its vertices with bit f / 2 equal to f % 2, then sorted
    template <int dim>
    __device__ __forceinline__ void face_key(const DevView &v, long long cell, int f, int key[1 << (dim - 1)])
    {
      constexpr int nfv = 1 << (dim - 1);
      const int ax = f >> 1, side = f & 1;
#pragma unroll
      for (int j = 0; j < nfv; ++j)
        {
          const int lo = j & ((1 << ax) - 1);
          const int b = lo | (side << ax) | ((j >> ax) << (ax + 1));
          key[j] = v.conn[(long long)b * v.n_cells + cell];
        }
      sort_key<dim>(key);
    }

    template <int dim>
    __device__ __forceinline__ unsigned long long hash_key(const int key[1 << (dim - 1)])
    {
      unsigned long long h = 0x9E3779B97F4A7C15ull;
#pragma unroll
      for (int j = 0; j < (1 << (dim - 1)); ++j)
        {
          h ^= (unsigned long long)(unsigned)key[j];
          h *= 0xff51afd7ed558ccdull;
          h ^= h >> 29;
        }
      return h;
    }

    template <int dim>
    __device__ __forceinline__ bool same_key(const int a[1 << (dim - 1)], const int b[1 << (dim - 1)])
    {
      bool eq = true;
#pragma unroll
      for (int j = 0; j < (1 << (dim - 1)); ++j)
        eq = eq && a[j] == b[j];
      return eq;
    }

    template <int dim>
    __global__ __launch_bounds__(256) void k_ft_insert(DevView v, uint32_t *__restrict__ occ_a, uint32_t *__restrict__ occ_b, unsigned long long cap_mask)
    {
      constexpr int nfv = 1 << (dim - 1);
      const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (t >= v.n_cells * 2 * dim)
        return;
      int key[nfv], other[nfv];
      face_key<dim>(v, t % v.n_cells, (int)(t / v.n_cells), key);
      for (unsigned long long s = hash_key<dim>(key) & cap_mask;; s = (s + 1) & cap_mask)
        {
          const uint32_t cur = atomicCAS(&occ_a[s], FT_EMPTY, (uint32_t)t);
          if (cur == FT_EMPTY)
            return;
          face_key<dim>(v, cur % v.n_cells, (int)(cur / v.n_cells), other);
          if (same_key<dim>(key, other))
            {
              if (atomicCAS(&occ_b[s], FT_EMPTY, (uint32_t)t) != FT_EMPTY)
                atomicExch(&occ_b[s], FT_MULTI); // three cells at one face: not a manifold mesh, nobody gets a neighbour
              return;
            }
        }
    }

    // slot of a key, or ~0 when the key is not in the table
    template <int dim>
    __device__ __forceinline__ unsigned long long ft_find(const DevView &v, const uint32_t *__restrict__ occ_a, unsigned long long cap_mask,
                                                          const int key[1 << (dim - 1)])
    {
      int other[1 << (dim - 1)];
      for (unsigned long long s = hash_key<dim>(key) & cap_mask;; s = (s + 1) & cap_mask)
        {
          const uint32_t cur = occ_a[s];
          if (cur == FT_EMPTY)
            return ~0ull;
          face_key<dim>(v, cur % v.n_cells, (int)(cur / v.n_cells), other);
          if (same_key<dim>(key, other))
            return s;
        }
    }

    template <int dim>
    __global__ __launch_bounds__(256) void k_ft_match(DevView v, const uint32_t *__restrict__ occ_a, const uint32_t *__restrict__ occ_b,
                                                      unsigned long long cap_mask, int32_t *__restrict__ nbr, uint8_t *__restrict__ rel)
    {
      constexpr int nfv = 1 << (dim - 1);
      const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (t >= v.n_cells * 2 * dim)
        return;
      int key[nfv];
      face_key<dim>(v, t % v.n_cells, (int)(t / v.n_cells), key);
      const unsigned long long s = ft_find<dim>(v, occ_a, cap_mask, key);
      int32_t n = -1;
      if (s != ~0ull)
        {
          const uint32_t a = occ_a[s], b = occ_b[s];
          if (b != FT_EMPTY && b != FT_MULTI)
            n = (int32_t)((a == (uint32_t)t ? b : a) % v.n_cells);
        }
      nbr[t] = n;
      rel[t] = n >= 0 ? REL_SAME : REL_NONE;
    }

    // unmatched faces with a hanging vertex: find the coarser neighbour's face.  coarse_of[t] = that face (thread number)
    template <int dim>
    __global__ __launch_bounds__(256) void k_ft_hanging(DevView v, const uint32_t *__restrict__ occ_a, const uint32_t *__restrict__ occ_b,
                                                        unsigned long long cap_mask, int32_t *__restrict__ nbr, uint8_t *__restrict__ rel,
                                                        uint32_t *__restrict__ coarse_of)
    {
      constexpr int nfv = 1 << (dim - 1);
      const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (t >= v.n_cells * 2 * dim)
        return;
      coarse_of[t] = FT_EMPTY;
      if (rel[t] == REL_SAME)
        return;
      int key[nfv], uni[nfv];
      face_key<dim>(v, t % v.n_cells, (int)(t / v.n_cells), key);
      int n_uni = 0;
      bool hangs = false, ok = true;
      auto add = [&](int node) {
        bool have = false;
#pragma unroll
        for (int j = 0; j < nfv; ++j)
          have = have || (j < n_uni && uni[j] == node);
        if (have)
          return;
        if (n_uni == nfv)
          {
            ok = false;
            return;
          }
#pragma unroll
        for (int j = 0; j < nfv; ++j)
          if (j == n_uni)
            uni[j] = node;
        ++n_uni;
      };
#pragma unroll
      for (int j = 0; j < nfv; ++j)
        {
          const int k = v.hn_index[key[j]];
          if (k < 0)
            add(key[j]);
          else
            {
              hangs = true;
              for (long long e = v.hn_ptr[k]; e < v.hn_ptr[k + 1]; ++e)
                add(v.hn_parents[e]);
            }
        }
      if (!hangs || !ok || n_uni != nfv)
        return;
      sort_key<dim>(uni);
      if (same_key<dim>(uni, key))
        return;
      const unsigned long long s = ft_find<dim>(v, occ_a, cap_mask, uni);
      if (s == ~0ull || occ_b[s] != FT_EMPTY)
        return;
      const uint32_t cf = occ_a[s];
      nbr[t] = (int32_t)(cf % v.n_cells);
      rel[t] = REL_FINE;
      rel[cf] = REL_COARSE; // every subface stores the same byte
      coarse_of[t] = cf;
    }

    __global__ __launch_bounds__(256) void k_ft_number_coarse(long long n_faces, const uint8_t *__restrict__ rel, int32_t *__restrict__ nbr,
                                                              unsigned *__restrict__ counter)
    {
      const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (t < n_faces && rel[t] == REL_COARSE)
        nbr[t] = (int32_t)atomicAdd(counter, 1u);
    }

    __global__ __launch_bounds__(256) void k_ft_fill_sub(long long n_cells, int n_cell_faces, int n_sub, const uint8_t *__restrict__ rel,
                                                         const int32_t *__restrict__ nbr, const uint32_t *__restrict__ coarse_of,
                                                         uint32_t *__restrict__ sub)
    {
      const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (t >= n_cells * n_cell_faces || rel[t] != REL_FINE)
        return;
      const uint32_t code = (uint32_t)((t % n_cells) * n_cell_faces + t / n_cells);
      uint32_t *slot = sub + (long long)nbr[coarse_of[t]] * n_sub;
      for (int j = 0; j < n_sub; ++j)
        if (atomicCAS(&slot[j], FT_EMPTY, code) == FT_EMPTY)
          return;
    }

    __global__ __launch_bounds__(256) void k_ft_sort_sub(long long n_lists, int n_sub, uint32_t *__restrict__ sub)
    {
      const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (i >= n_lists)
        return;
      uint32_t *s = sub + i * n_sub;
      for (int a = 1; a < n_sub; ++a) // insertion sort of 2 or 4 entries (FT_EMPTY last)
        for (int b = a; b > 0 && s[b - 1] > s[b]; --b)
          {
            const uint32_t x = s[b];
            s[b] = s[b - 1];
            s[b - 1] = x;
          }
    }

    struct FaceTab
    {
      const int32_t *nbr;  // [2 dim][n_cells]
      const uint8_t *rel;  // [2 dim][n_cells]
      const uint32_t *sub; // [n_coarse faces][2^(dim-1)]
    };

    // ---- Kelly indicator
    template <int dim>
    struct KCell // vertices, coordinates and the selected nodal components of one cell
    {
      int n[1 << dim];
      double X[1 << dim][dim];
      double U[1 << dim][dim + 1];
    };

    template <int dim>
    __device__ __forceinline__ void load_kcell(const DevView &v, long long cell, unsigned mask, KCell<dim> &k)
    {
#pragma unroll
      for (int b = 0; b < (1 << dim); ++b)
        {
          const int n = v.conn[(long long)b * v.n_cells + cell];
          k.n[b] = n;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            {
              k.X[b][d] = v.coords[(long long)d * v.n_nodes + n];
              k.U[b][d] = (mask >> d) & 1u ? v.u[d][n] : 0.0;
            }
          k.U[b][dim] = (mask >> dim) & 1u ? v.phi[n] : 0.0;
        }
    }

    // d N_b / d xi_d of the Q1 shape functions
    template <int dim>
    __device__ __forceinline__ double q1_dweight(int b, int d, const double xi[dim])
    {
      double w = ((b >> d) & 1) ? 1.0 : -1.0;
#pragma unroll
      for (int e = 0; e < dim; ++e)
        if (e != d)
          w *= ((b >> e) & 1) ? xi[e] : (1.0 - xi[e]);
      return w;
    }

    // J = the Jacobian of the Q1 map of the cell at xi and (nrm != nullptr) m = J^-1 nrm
    template <int dim>
    __device__ __forceinline__ void jac_solve(const KCell<dim> &k, const double xi[dim], const double nrm[dim], double m[dim],
                                              double J[dim][dim])
    {
#pragma unroll
      for (int i = 0; i < dim; ++i)
#pragma unroll
        for (int d = 0; d < dim; ++d)
          J[i][d] = 0.0;
#pragma unroll
      for (int b = 0; b < (1 << dim); ++b)
#pragma unroll
        for (int d = 0; d < dim; ++d)
          {
            const double w = q1_dweight<dim>(b, d, xi);
#pragma unroll
            for (int i = 0; i < dim; ++i)
              J[i][d] += k.X[b][i] * w;
          }
      if (!nrm)
        return;
      if constexpr (dim == 2)
        {
          const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
          m[0] = (J[1][1] * nrm[0] - J[0][1] * nrm[1]) / det;
          m[1] = (J[0][0] * nrm[1] - J[1][0] * nrm[0]) / det;
        }
      else
        {
          // rows of the cofactor matrix: J^-1 = adj / det
          const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
          const double c01 = J[0][2] * J[2][1] - J[0][1] * J[2][2];
          const double c02 = J[0][1] * J[1][2] - J[0][2] * J[1][1];
          const double c10 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
          const double c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0];
          const double c12 = J[0][2] * J[1][0] - J[0][0] * J[1][2];
          const double c20 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
          const double c21 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
          const double c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
          const double det = J[0][0] * c00 + J[1][0] * c01 + J[2][0] * c02;
          m[0] = (c00 * nrm[0] + c01 * nrm[1] + c02 * nrm[2]) / det;
          m[1] = (c10 * nrm[0] + c11 * nrm[1] + c12 * nrm[2]) / det;
          m[2] = (c20 * nrm[0] + c21 * nrm[1] + c22 * nrm[2]) / det;
        }
    }

    // n . grad u_c at xi: sum_d m_d sum_b dN_b/dxi_d U[b][c]
    template <int dim>
    __device__ __forceinline__ void normal_derivative(const KCell<dim> &k, const double xi[dim], const double m[dim], double out[dim + 1])
    {
#pragma unroll
      for (int c = 0; c <= dim; ++c)
        out[c] = 0.0;
#pragma unroll
      for (int b = 0; b < (1 << dim); ++b)
        {
          double a = 0.0;
#pragma unroll
          for (int d = 0; d < dim; ++d)
            a += m[d] * q1_dweight<dim>(b, d, xi);
#pragma unroll
          for (int c = 0; c <= dim; ++c)
            out[c] += a * k.U[b][c];
        }
    }

    // int over face f of cell A of sum_c (n . grad u_c|_A - n . grad u_c|_B)^2 dA with QGauss<dim-1>(3).  The point of B under
    // a face point is the (bi)linear image of the reference corners the vertices of A's face have in B -- through the
    // hanging weights where a vertex hangs on B's face: both cells restrict the same face map, no inversion.
    template <int dim>
    __device__ __forceinline__ double face_jump_integral(const DevView &v, const KCell<dim> &A, int f, const KCell<dim> &B)
    {
      constexpr int nv = 1 << dim;
      const int ax = f >> 1, side = f & 1;
      double xiB[nv][dim]; // reference point in B of vertex b of A (the face's vertices only; 0 elsewhere)
      bool ok = true;
#pragma unroll
      for (int b = 0; b < nv; ++b)
        {
#pragma unroll
          for (int d = 0; d < dim; ++d)
            xiB[b][d] = 0.0;
          if (((b >> ax) & 1) != side)
            continue;
          int corner = -1;
#pragma unroll
          for (int k = nv - 1; k >= 0; --k)
            if (B.n[k] == A.n[b])
              corner = k;
          if (corner >= 0)
            {
#pragma unroll
              for (int d = 0; d < dim; ++d)
                xiB[b][d] = (double)((corner >> d) & 1);
              continue;
            }
          const int hk = v.hn_index ? v.hn_index[A.n[b]] : -1;
          if (hk < 0)
            {
              ok = false;
              continue;
            }
          for (long long e = v.hn_ptr[hk]; e < v.hn_ptr[hk + 1]; ++e)
            {
              const int p = v.hn_parents[e];
              const double w = v.hn_weights[e];
              int pc = -1;
#pragma unroll
              for (int k = nv - 1; k >= 0; --k)
                if (B.n[k] == p)
                  pc = k;
              if (pc < 0)
                ok = false;
#pragma unroll
              for (int d = 0; d < dim; ++d)
                xiB[b][d] += w * (double)((pc >> d) & 1);
            }
        }
      if (!ok)
        return 0.0;
      const double g = 0.3872983346207417; // sqrt(0.6) / 2
      const double gp[3] = {0.5 - g, 0.5, 0.5 + g}, gw[3] = {5.0 / 18.0, 8.0 / 18.0, 5.0 / 18.0};
      constexpr int nq = dim == 2 ? 3 : 9;
      double total = 0.0;
#pragma unroll 1
      for (int q = 0; q < nq; ++q)
        {
          const int q0 = q % 3, q1 = q / 3;
          const double p0 = q0 == 0 ? gp[0] : (q0 == 1 ? gp[1] : gp[2]), w0 = q0 == 1 ? gw[1] : gw[0];
          const double p1 = q1 == 0 ? gp[0] : (q1 == 1 ? gp[1] : gp[2]), w1 = dim == 2 ? 1.0 : (q1 == 1 ? gw[1] : gw[0]);
          // the face's free axes o0 < o1 take p0, p1 (selects, no runtime-indexed arrays)
          const int o0 = ax == 0 ? 1 : 0, o1 = ax == 2 ? 1 : 2;
          double xi[dim];
#pragma unroll
          for (int d = 0; d < dim; ++d)
            xi[d] = d == ax ? (double)side : (d == o0 ? p0 : p1);
          double JA[dim][dim], JB[dim][dim], nrm[dim], mA[dim], mB[dim];
          jac_solve<dim>(A, xi, nullptr, mA, JA);
          // normal from the face tangents (its sign cancels in the square)
          double t0[dim], t1[dim];
#pragma unroll
          for (int i = 0; i < dim; ++i)
            {
              t0[i] = o0 == 0 ? JA[i][0] : JA[i][1];
              t1[i] = o1 == 1 ? JA[i][1] : JA[i][dim - 1];
            }
          if constexpr (dim == 2)
            {
              nrm[0] = t0[1];
              nrm[1] = -t0[0];
            }
          else
            {
              nrm[0] = t0[1] * t1[2] - t0[2] * t1[1];
              nrm[1] = t0[2] * t1[0] - t0[0] * t1[2];
              nrm[2] = t0[0] * t1[1] - t0[1] * t1[0];
            }
          double len = 0.0;
#pragma unroll
          for (int i = 0; i < dim; ++i)
            len += nrm[i] * nrm[i];
          len = sqrt(len);
#pragma unroll
          for (int i = 0; i < dim; ++i)
            nrm[i] /= len;
          jac_solve<dim>(A, xi, nrm, mA, JA);
          double xb[dim];
#pragma unroll
          for (int d = 0; d < dim; ++d)
            xb[d] = 0.0;
#pragma unroll
          for (int b = 0; b < nv; ++b)
            {
              const double w = q1_weight<dim>(b, xi); // 0 off the face
#pragma unroll
              for (int d = 0; d < dim; ++d)
                xb[d] += w * xiB[b][d];
            }
          jac_solve<dim>(B, xb, nrm, mB, JB);
          double dA_[dim + 1], dB_[dim + 1];
          normal_derivative<dim>(A, xi, mA, dA_);
          normal_derivative<dim>(B, xb, mB, dB_);
          double s = 0.0;
#pragma unroll
          for (int c = 0; c <= dim; ++c)
            {
              const double j = dA_[c] - dB_[c];
              s += j * j;
            }
          total += s * (w0 * w1 * len);
        }
      return total;
    }

    // thread <-> cell: every cell evaluates all its faces itself (the subfaces of a face against finer cells from the fine
    // cells' side, in the order of the side list); nothing is added into another cell's entry
    template <int dim>
    __global__ __launch_bounds__(128) void k_kelly(DevView v, FaceTab ft, const uint8_t *__restrict__ cell_owned, unsigned mask,
                                                   double *__restrict__ eta)
    {
      constexpr int n_sub = 1 << (dim - 1);
      const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (cell >= v.n_cells)
        return;
      if (cell_owned && !cell_owned[cell])
        {
          eta[cell] = 0.0;
          return;
        }
      KCell<dim> me, other;
      load_kcell<dim>(v, cell, mask, me);
      double sum = 0.0;
#pragma unroll 1
      for (int f = 0; f < 2 * dim; ++f)
        {
          const long long t = (long long)f * v.n_cells + cell;
          const int rel = ft.rel[t];
          if (rel == REL_NONE)
            continue;
          const int32_t n = ft.nbr[t];
          if (rel == REL_COARSE)
            {
#pragma unroll 1
              for (int j = 0; j < n_sub; ++j)
                {
                  const uint32_t code = ft.sub[(long long)n * n_sub + j];
                  if (code == FT_EMPTY)
                    continue;
                  load_kcell<dim>(v, code / (2 * dim), mask, other);
                  sum += face_jump_integral<dim>(v, other, (int)(code % (2 * dim)), me);
                }
            }
          else
            {
              load_kcell<dim>(v, n, mask, other);
              sum += face_jump_integral<dim>(v, me, f, other);
            }
        }
      eta[cell] = sqrt(sqrt(diameter_sq<dim>(me.X)) / 24.0 * sum);
    }

    // ---- exact selection on the order-preserving 64-bit key of a double: -0.0 = 0.0, a NaN below every number (key 0)
    __device__ __host__ inline unsigned long long select_key(double x)
    {
      if (x != x)
        return 0ull;
      unsigned long long b;
      memcpy(&b, &x, 8);
      if ((b << 1) == 0ull) // -0.0 is 0.0
        b = 0ull;
      return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }

    inline double select_value(unsigned long long k)
    {
      if (k == 0ull)
        return std::numeric_limits<double>::quiet_NaN();
      const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
      double x;
      memcpy(&x, &b, 8);
      return x;
    }

    // state of the radix select (device): the key prefix found so far and the rank still looked for among the values that
    // share it
    struct SelectState
    {
      unsigned long long prefix, k;
    };

    // one pass: histogram of the byte at `shift` over the masked values whose higher bytes equal the prefix.  LDS histogram
    // per workgroup, merged with integer adds (exact: the order of the adds does not matter)
    __global__ __launch_bounds__(256) void k_select_hist(const double *__restrict__ x, const uint8_t *__restrict__ owned, long long n,
                                                         const SelectState *__restrict__ st, int shift, unsigned long long *__restrict__ hist)
    {
      __shared__ unsigned s_hist[256];
      s_hist[threadIdx.x] = 0;
      __syncthreads();
      const unsigned long long prefix = st->prefix;
      for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        {
          if (owned && !owned[i])
            continue;
          const unsigned long long key = select_key(x[i]);
          if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)))
            atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
        }
      __syncthreads();
      if (s_hist[threadIdx.x])
        atomicAdd(&hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
    }

    // ... and the byte that holds rank k, counted from the largest byte down
    __global__ void k_select_pick(SelectState *st, int shift, unsigned long long *hist)
    {
      if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
      unsigned long long k = st->k;
      int digit = 0;
      for (int b = 255; b >= 0; --b)
        {
          if (hist[b] >= k)
            {
              digit = b;
              break;
            }
          k -= hist[b];
        }
      st->k = k;
      st->prefix |= (unsigned long long)digit << shift;
      for (int b = 0; b < 256; ++b)
        hist[b] = 0;
    }

    // counts[0] = masked values above the key, counts[1] = equal to it; counts[2]: the smallest key above key(0.0), i.e. of a
    // positive value (integer minimum)
    __global__ __launch_bounds__(256) void k_select_count(const double *__restrict__ x, const uint8_t *__restrict__ owned, long long n,
                                                          const SelectState *__restrict__ st, unsigned long long key_in,
                                                          unsigned long long *__restrict__ counts)
    {
      __shared__ unsigned long long s_above[4], s_equal[4], s_min[4];
      const unsigned long long t = st ? st->prefix : key_in, zero = 0x8000000000000000ull;
      unsigned long long above = 0, equal = 0, mn = ~0ull;
      for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        {
          if (owned && !owned[i])
            continue;
          const unsigned long long key = select_key(x[i]);
          above += key > t;
          equal += key == t;
          if (key > zero && key < mn)
            mn = key;
        }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        {
          above += __shfl_xor(above, off);
          equal += __shfl_xor(equal, off);
          const unsigned long long o = __shfl_xor(mn, off);
          mn = o < mn ? o : mn;
        }
      if ((threadIdx.x & 63) == 0)
        {
          s_above[threadIdx.x >> 6] = above;
          s_equal[threadIdx.x >> 6] = equal;
          s_min[threadIdx.x >> 6] = mn;
        }
      __syncthreads();
      if (threadIdx.x == 0)
        {
          atomicAdd(&counts[0], s_above[0] + s_above[1] + s_above[2] + s_above[3]);
          atomicAdd(&counts[1], s_equal[0] + s_equal[1] + s_equal[2] + s_equal[3]);
          unsigned long long m = s_min[0];
          for (int w = 1; w < 4; ++w)
            m = s_min[w] < m ? s_min[w] : m;
          atomicMin(&counts[2], m);
        }
    }

    __global__ __launch_bounds__(256) void k_count_mask(const uint8_t *__restrict__ owned, long long n, unsigned long long *__restrict__ out)
    {
      unsigned long long r = 0;
      for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        r += owned[i] != 0;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        r += __shfl_xor(r, off);
      if ((threadIdx.x & 63) == 0 && r)
        atomicAdd(out, r);
    }

    // mix, step (b): the indicator of the cells the phase field has flagged is dropped (cracks.cc:4085-4095)
    __global__ __launch_bounds__(256) void k_mix_zero_flagged(long long n, const uint8_t *__restrict__ flags, double *__restrict__ eta)
    {
      const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (i < n && flags[i])
        eta[i] = 0.0;
    }

    // mix, steps (c) and (d): flag eta >= t, clear the flags at max_level, count
    __global__ __launch_bounds__(256) void k_mix_flags(long long n, const double *__restrict__ eta, double t, int max_level,
                                                       const uint8_t *__restrict__ cell_level, uint8_t *__restrict__ flags,
                                                       unsigned long long *__restrict__ partial)
    {
      const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
      int f = 0;
      if (i < n)
        {
          f = flags[i] || eta[i] >= t; // t > 0: a zero or NaN indicator never flags
          if (f && max_level >= 0 && (int)cell_level[i] == max_level)
            f = 0;
          flags[i] = (uint8_t)f;
        }
      const unsigned long long total = block_count(f);
      if (threadIdx.x == 0)
        partial[blockIdx.x] = total;
    }

    unsigned stride_grid(long long n) { return (unsigned)std::min<long long>(std::max<long long>((n + 255) / 256, 1), 2048); }

    // the face-neighbour table of the context, built on first use.  PFM_ERR_NOMEM leaves the context as it was
    int ensure_face_table(pfm_ctx *c)
    {
      if (c->face_table_ready)
        return PFM_OK;
      const long long NC = c->v.n_cells;
      const int dim = c->v.dim, nf = 2 * dim, n_sub = 1 << (dim - 1);
      const long long n_faces = NC * nf;
      if (n_faces >= (long long)FT_MULTI)
        return fail(c, PFM_ERR_UNSUPPORTED, "face-neighbour table: more than 2^32 faces");
      unsigned long long cap = 1024;
      while (cap < (unsigned long long)n_faces + (unsigned long long)n_faces / 2)
        cap <<= 1;
      const bool hanging = c->v.hn_index != nullptr;
      int32_t *nbr = nullptr;
      uint8_t *rel = nullptr;
      uint32_t *sub = nullptr, *occ = nullptr, *coarse_of = nullptr;
      unsigned *counter = nullptr;
      unsigned n_coarse = 0;
      auto cleanup = [&](bool all) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(occ);
        (void)hipFree(coarse_of);
        (void)hipFree(counter);
        if (all)
          {
            (void)hipFree(nbr);
            (void)hipFree(rel);
            (void)hipFree(sub);
          }
      };
      const size_t nbr_bytes = sizeof(int32_t) * (size_t)std::max<long long>(n_faces, 1), rel_bytes = (size_t)std::max<long long>(n_faces, 1);
      if (hipMalloc((void **)&nbr, nbr_bytes) != hipSuccess || hipMalloc((void **)&rel, rel_bytes) != hipSuccess ||
          hipMalloc((void **)&occ, sizeof(uint32_t) * 2 * cap) != hipSuccess || hipMalloc((void **)&counter, 256) != hipSuccess ||
          (hanging && hipMalloc((void **)&coarse_of, sizeof(uint32_t) * (size_t)std::max<long long>(n_faces, 1)) != hipSuccess))
        {
          (void)hipGetLastError();
          cleanup(true);
          return fail(c, PFM_ERR_NOMEM, "hipMalloc face-neighbour table");
        }
      hipStream_t st = c->stream;
      uint32_t *occ_a = occ, *occ_b = occ + cap;
      const unsigned nb = (unsigned)((n_faces + 255) / 256);
      bool ok = hipMemsetAsync(occ, 0xff, sizeof(uint32_t) * 2 * cap, st) == hipSuccess && hipMemsetAsync(counter, 0, 256, st) == hipSuccess;
      if (ok && nb)
        {
          PFM_LAUNCH_DIM(dim, k_ft_insert, dim3(nb), dim3(256), st, c->v, occ_a, occ_b, cap - 1);
          PFM_LAUNCH_DIM(dim, k_ft_match, dim3(nb), dim3(256), st, c->v, occ_a, occ_b, cap - 1, nbr, rel);
          if (hanging)
            {
              PFM_LAUNCH_DIM(dim, k_ft_hanging, dim3(nb), dim3(256), st, c->v, occ_a, occ_b, cap - 1, nbr, rel, coarse_of);
              hipLaunchKernelGGL(k_ft_number_coarse, dim3(nb), dim3(256), 0, st, n_faces, rel, nbr, counter);
            }
          ok = hipGetLastError() == hipSuccess;
        }
      ok = ok && hipMemcpyAsync(&n_coarse, counter, sizeof(unsigned), hipMemcpyDeviceToHost, st) == hipSuccess &&
           hipStreamSynchronize(st) == hipSuccess;
      if (!ok)
        {
          cleanup(true);
          return fail(c, PFM_ERR_HIP, "face-neighbour table build");
        }
      const size_t sub_bytes = sizeof(uint32_t) * (size_t)std::max<unsigned>(n_coarse, 1) * n_sub;
      if (hipMalloc((void **)&sub, sub_bytes) != hipSuccess)
        {
          (void)hipGetLastError();
          cleanup(true);
          return fail(c, PFM_ERR_NOMEM, "hipMalloc face-neighbour side list");
        }
      ok = hipMemsetAsync(sub, 0xff, sub_bytes, st) == hipSuccess;
      if (ok && n_coarse)
        {
          hipLaunchKernelGGL(k_ft_fill_sub, dim3(nb), dim3(256), 0, st, NC, nf, n_sub, rel, nbr, coarse_of, sub);
          hipLaunchKernelGGL(k_ft_sort_sub, dim3((n_coarse + 255) / 256), dim3(256), 0, st, (long long)n_coarse, n_sub, sub);
          ok = hipGetLastError() == hipSuccess;
        }
      ok = ok && hipStreamSynchronize(st) == hipSuccess;
      cleanup(!ok);
      if (!ok)
        return fail(c, PFM_ERR_HIP, "face-neighbour side list build");
      c->d_face_nbr = nbr;
      c->d_face_rel = rel;
      c->d_face_sub = sub;
      c->allocs.push_back(nbr);
      c->allocs.push_back(rel);
      c->allocs.push_back(sub);
      c->device_bytes += (int64_t)(nbr_bytes + rel_bytes + sub_bytes);
      c->face_table_ready = true;
      return PFM_OK;
    }

    int launch_kelly(pfm_ctx *c, const uint8_t *d_owned, unsigned mask, double *d_eta)
    {
      const long long NC = c->v.n_cells;
      if (NC == 0)
        return PFM_OK;
      const FaceTab ft{c->d_face_nbr, c->d_face_rel, c->d_face_sub};
      const unsigned nb = (unsigned)((NC + 127) / 128);
      PFM_LAUNCH_DIM(c->v.dim, k_kelly, dim3(nb), dim3(128), c->stream, c->v, ft, d_owned, mask, d_eta);
      return hipGetLastError() == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "k_kelly launch");
    }

    // device words of a selection: the state, counts[3], the histogram
    constexpr size_t SELECT_WORK_BYTES = sizeof(SelectState) + sizeof(unsigned long long) * (3 + 256);

    // k-th largest (1 <= k <= number of masked values, checked by the caller) of x[0, n) on the context's stream; synchronous
    int run_select(pfm_ctx *c, const double *d_x, const uint8_t *d_owned, long long n, long long k, char *work, double *threshold,
                   int64_t counts[2], double *min_positive)
    {
      SelectState *st = reinterpret_cast<SelectState *>(work);
      unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(work + sizeof(SelectState)), *d_hist = d_counts + 3;
      const SelectState init{0ull, (unsigned long long)k};
      const unsigned long long init_counts[3] = {0ull, 0ull, ~0ull};
      hipStream_t s = c->stream;
      if (hipMemcpyAsync(st, &init, sizeof(init), hipMemcpyHostToDevice, s) != hipSuccess ||
          hipMemcpyAsync(d_counts, init_counts, sizeof(init_counts), hipMemcpyHostToDevice, s) != hipSuccess ||
          hipMemsetAsync(d_hist, 0, sizeof(unsigned long long) * 256, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(c, PFM_ERR_HIP, "selection set-up"); // (the sources are on this stack frame)
      const unsigned nb = stride_grid(n);
      if (k >= 1)
        for (int shift = 56; shift >= 0; shift -= 8)
          {
            hipLaunchKernelGGL(k_select_hist, dim3(nb), dim3(256), 0, s, d_x, d_owned, n, st, shift, d_hist);
            hipLaunchKernelGGL(k_select_pick, dim3(1), dim3(64), 0, s, st, shift, d_hist);
          }
      hipLaunchKernelGGL(k_select_count, dim3(nb), dim3(256), 0, s, d_x, d_owned, n, (const SelectState *)st, 0ull, d_counts);
      if (hipGetLastError() != hipSuccess)
        return fail(c, PFM_ERR_HIP, "selection launch");
      SelectState out{};
      unsigned long long h_counts[3] = {0, 0, 0};
      if (hipMemcpyAsync(&out, st, sizeof(out), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipMemcpyAsync(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess)
        return fail(c, PFM_ERR_HIP, "selection copy");
      *threshold = select_value(out.prefix);
      counts[0] = (int64_t)h_counts[0];
      counts[1] = (int64_t)h_counts[1];
      if (min_positive)
        *min_positive = h_counts[2] == ~0ull ? HUGE_VAL : select_value(h_counts[2]);
      return PFM_OK;
    }

    int count_masked(pfm_ctx *c, const uint8_t *d_owned, long long n, char *work, long long *n_masked)
    {
      *n_masked = n;
      if (!d_owned || n == 0)
        return PFM_OK;
      unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(work), h = 0;
      if (hipMemsetAsync(d_cnt, 0, sizeof(h), c->stream) != hipSuccess)
        return fail(c, PFM_ERR_HIP, "mask count");
      hipLaunchKernelGGL(k_count_mask, dim3(stride_grid(n)), dim3(256), 0, c->stream, d_owned, n, d_cnt);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
          hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, PFM_ERR_HIP, "mask count");
      *n_masked = (long long)h;
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
    const RefineCrit cr = make_crit(*crit, crit->max_level);
    (void)hipSetDevice(c->device);
    const unsigned nb = (unsigned)((NC + 255) / 256);
    // scratch: flags [NC] | levels [NC] | block counts [nb] + the total
    const size_t o_level = align256((size_t)NC), o_part = o_level + align256((size_t)NC);
    if (int rc = dev_buf_reserve(c, c->buf_adapt, o_part + sizeof(unsigned long long) * ((size_t)nb + 1), "adaptation scratch"))
      return rc;
    char *base = c->buf_adapt.as<char>();
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
      PFM_LAUNCH_DIM(c->v.dim, k_refine_flags, dim3(nb), dim3(256), c->stream, c->v, cr, d_owned, d_level, d_flags, d_part);
    hipLaunchKernelGGL((k_reduce_final<unsigned long long, 1, Sum<unsigned long long>>), dim3(1), dim3(256), 0, c->stream, d_part,
                       (long long)nb, d_part + nb);
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
    if (int rc = dev_buf_reserve(c, c->buf_adapt, sizeof(double) * ((size_t)nb + 1), "adaptation scratch"))
      return rc;
    double *d_part = c->buf_adapt.as<double>();
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    if (nb)
      PFM_LAUNCH_DIM(c->v.dim, k_min_diameter_sq, dim3(nb), dim3(256), c->stream, c->v, d_owned, d_part);
    hipLaunchKernelGGL((k_reduce_final<double, 1, Min>), dim3(1), dim3(256), 0, c->stream, d_part, (long long)nb, d_part + nb);
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
    if (int rc = dev_buf_reserve(dst, dst->buf_adapt, o_bad + 256, "adaptation scratch"))
      return rc;
    char *base = dst->buf_adapt.as<char>();
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
    PFM_LAUNCH_DIM(dim, k_xfer_check, dim3(nbc), dim3(256), st, src->v, dst->v, d_parent, d_child, d_owner, d_bad);
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
    PFM_LAUNCH_DIM(dim, k_xfer_write, dim3(nbw), dim3(256), st, src->v, dst->v, d_parent, d_child, d_owner, vecs);
    if (hipGetLastError() != hipSuccess)
      return fail(dst, PFM_ERR_HIP, "k_xfer_write launch");
    return PFM_OK;
  }

  int pfm_kelly_indicator(pfm_ctx *c, const uint8_t *cell_owned, unsigned component_mask, double *d_eta)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (component_mask == 0 || (component_mask >> (c->v.dim + 1)) != 0)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_kelly_indicator: component mask empty or with a bit above dim");
    if (c->v.n_cells > 0 && !d_eta)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_kelly_indicator: NULL output");
    (void)hipSetDevice(c->device);
    if (int rc = ensure_face_table(c))
      return rc;
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    return launch_kelly(c, d_owned, component_mask, d_eta);
  }

  int pfm_indicator_select(pfm_ctx *c, const double *d_ind, const uint8_t *cell_owned, int64_t k, double *threshold, int64_t counts[2])
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    const long long NC = c->v.n_cells;
    if (!d_ind || !threshold || !counts || k < 1 || k > NC)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_indicator_select: NULL array or output, or k outside [1, n_cells]");
    (void)hipSetDevice(c->device);
    if (int rc = dev_buf_reserve(c, c->buf_adapt, SELECT_WORK_BYTES, "adaptation scratch"))
      return rc;
    char *work = c->buf_adapt.as<char>();
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    long long n_masked = NC;
    if (int rc = count_masked(c, d_owned, NC, work, &n_masked))
      return rc;
    if (k > n_masked)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_indicator_select: k above the number of masked cells");
    return run_select(c, d_ind, d_owned, NC, k, work, threshold, counts, nullptr);
  }

  int pfm_indicator_count(pfm_ctx *c, const double *d_ind, const uint8_t *cell_owned, double t, int64_t counts[2])
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    const long long NC = c->v.n_cells;
    if ((NC > 0 && !d_ind) || !counts)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_indicator_count: NULL array or output");
    (void)hipSetDevice(c->device);
    if (int rc = dev_buf_reserve(c, c->buf_adapt, SELECT_WORK_BYTES, "adaptation scratch"))
      return rc;
    char *work = c->buf_adapt.as<char>();
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(work), h[3] = {0, 0, 0};
    if (hipMemsetAsync(d_counts, 0, sizeof(h), c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "pfm_indicator_count: clear");
    hipLaunchKernelGGL(k_select_count, dim3(stride_grid(NC)), dim3(256), 0, c->stream, d_ind, d_owned, NC, (const SelectState *)nullptr,
                       select_key(t), d_counts);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, d_counts, sizeof(h), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "pfm_indicator_count");
    counts[0] = (int64_t)h[0];
    counts[1] = (int64_t)h[1];
    return PFM_OK;
  }

  int pfm_refine_flags_mix(pfm_ctx *c, const pfm_refine_criteria *crit, double top_fraction, unsigned component_mask,
                           const uint8_t *cell_owned, const uint8_t *cell_level, uint8_t *flags, int64_t *n_flagged, double *threshold)
  {
    if (!c || !crit || !n_flagged || !threshold)
      return c ? fail(c, PFM_ERR_BAD_ARG, "pfm_refine_flags_mix: NULL criteria or output") : PFM_ERR_BAD_ARG;
    const long long NC = c->v.n_cells;
    if ((NC > 0 && !flags) || (crit->max_level >= 0 && NC > 0 && !cell_level) || crit->max_level > 255)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_refine_flags_mix: NULL flags, a level limit without cell levels, or one above 255");
    if (!(top_fraction >= 0.0 && top_fraction <= 1.0))
      return fail(c, PFM_ERR_BAD_ARG, "pfm_refine_flags_mix: top_fraction outside [0, 1]");
    if (component_mask == 0 || (component_mask >> (c->v.dim + 1)) != 0)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_refine_flags_mix: component mask empty or with a bit above dim");
    if (c->v.n_owned != c->v.n_nodes)
      return fail(c, PFM_ERR_UNSUPPORTED,
                  "pfm_refine_flags_mix: partitioned context (the fraction is of the global cell count: compose pfm_refine_flags, "
                  "pfm_kelly_indicator and pfm_indicator_count)");
    const RefineCrit cr = make_crit(*crit, -1); // (a): without the level limit; (d) applies it at the end
    (void)hipSetDevice(c->device);
    if (int rc = ensure_face_table(c))
      return rc;
    const unsigned nb = (unsigned)((NC + 255) / 256);
    // scratch: flags [NC] | levels [NC] | eta [NC] | block counts [nb] + the total | selection words
    const size_t o_level = align256((size_t)NC), o_eta = o_level + align256((size_t)NC);
    const size_t o_part = o_eta + align256(sizeof(double) * (size_t)NC);
    const size_t o_sel = o_part + align256(sizeof(unsigned long long) * ((size_t)nb + 1));
    if (int rc = dev_buf_reserve(c, c->buf_adapt, o_sel + SELECT_WORK_BYTES, "adaptation scratch"))
      return rc;
    char *base = c->buf_adapt.as<char>();
    uint8_t *d_flags = reinterpret_cast<uint8_t *>(base), *d_level = nullptr;
    double *d_eta = reinterpret_cast<double *>(base + o_eta);
    unsigned long long *d_part = reinterpret_cast<unsigned long long *>(base + o_part);
    uint8_t *d_owned = nullptr;
    if (int rc = upload_mask(c, cell_owned, &d_owned))
      return rc;
    hipStream_t st = c->stream;
    if (crit->max_level >= 0 && NC > 0)
      {
        d_level = reinterpret_cast<uint8_t *>(base + o_level);
        if (hipMemcpyAsync(d_level, cell_level, (size_t)NC, hipMemcpyHostToDevice, st) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "cell level upload");
      }
    const long long k = (long long)(top_fraction * (double)NC); // the reference's static_cast
    double t = HUGE_VAL;
    if (nb)
      {
        PFM_LAUNCH_DIM(c->v.dim, k_refine_flags, dim3(nb), dim3(256), st, c->v, cr, d_owned, (const uint8_t *)nullptr, d_flags, d_part);
        if (hipGetLastError() != hipSuccess)
          return fail(c, PFM_ERR_HIP, "k_refine_flags launch");
        if (k >= 1)
          {
            if (int rc = launch_kelly(c, d_owned, component_mask, d_eta))
              return rc;
            hipLaunchKernelGGL(k_mix_zero_flagged, dim3(nb), dim3(256), 0, st, NC, d_flags, d_eta);
            int64_t counts[2];
            double min_positive = HUGE_VAL;
            if (int rc = run_select(c, d_eta, nullptr, NC, k, base + o_sel, &t, counts, &min_positive))
              return rc;
            if (!(t > 0.0)) // refine(): a zero threshold becomes the smallest positive indicator; +inf where there is none
              t = min_positive;
          }
        else if (hipMemsetAsync(d_eta, 0, sizeof(double) * (size_t)NC, st) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "indicator clear");
        hipLaunchKernelGGL(k_mix_flags, dim3(nb), dim3(256), 0, st, NC, d_eta, t, (int)crit->max_level, d_level, d_flags, d_part);
      }
    hipLaunchKernelGGL((k_reduce_final<unsigned long long, 1, Sum<unsigned long long>>), dim3(1), dim3(256), 0, st, d_part, (long long)nb,
                       d_part + nb);
    if (hipGetLastError() != hipSuccess)
      return fail(c, PFM_ERR_HIP, "k_mix_flags launch");
    unsigned long long total = 0;
    if ((NC > 0 && hipMemcpyAsync(flags, d_flags, (size_t)NC, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipMemcpyAsync(&total, d_part + nb, sizeof(total), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "refine flags copy");
    *n_flagged = (int64_t)total;
    *threshold = t;
    return PFM_OK;
  }
}
