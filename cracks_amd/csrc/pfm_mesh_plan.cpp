// pfm_mesh_plan.cpp -- see pfm_mesh_plan.h.  Host only: no HIP call, no context.
#include "pfm_mesh_plan.h"
#include "pfm_host_pool.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace pfm
{
  using Lattice = LatticeHost;

  // bounding box of the node coordinates (chunked over the host threads; min and max are exact)
  void bounding_box(const pfm_mesh_desc *m, double (&lo)[3], double (&hi)[3])
  {
    const int dim = m->dim;
    const int64_t N = m->n_nodes;
    const int nt = chunks_for(N, 16384);
    std::vector<double> part((size_t)nt * 6);
    parallel_chunks(nt, [&](int t) {
      const int64_t nb = N * t / nt, ne = N * (t + 1) / nt;
      double a[3], b[3]; // (locals: the chunks' slots of `part` share cache lines)
      for (int d = 0; d < dim; ++d)
        a[d] = b[d] = m->coords[(size_t)nb * dim + d];
      for (int64_t n = nb; n < ne; ++n)
        for (int d = 0; d < dim; ++d)
          {
            const double x = m->coords[(size_t)n * dim + d];
            a[d] = std::min(a[d], x);
            b[d] = std::max(b[d], x);
          }
      for (int d = 0; d < dim; ++d)
        {
          part[(size_t)t * 6 + d] = a[d];
          part[(size_t)t * 6 + 3 + d] = b[d];
        }
    });
    for (int d = 0; d < 3; ++d)
      lo[d] = hi[d] = 0;
    for (int d = 0; d < dim; ++d)
      {
        lo[d] = part[d];
        hi[d] = part[3 + d];
        for (int t = 1; t < nt; ++t)
          {
            lo[d] = std::min(lo[d], part[(size_t)t * 6 + d]);
            hi[d] = std::max(hi[d], part[(size_t)t * 6 + 3 + d]);
          }
      }
  }

  bool detect_lattice(const pfm_mesh_desc *m, Lattice &L)
  {
    const int dim = m->dim, nv = 1 << dim;
    if (m->n_hanging > 0)
      return false;
    int nc[3] = {m->box_cells[0], m->box_cells[1], dim == 3 ? m->box_cells[2] : 1};
    if (nc[0] <= 0 || nc[1] <= 0 || nc[2] <= 0)
      return false;
    const int NX = nc[0] + 1, NY = nc[1] + 1, NZ = dim == 3 ? nc[2] + 1 : 1;
    const int64_t nn = (int64_t)NX * NY * NZ;
    if (nn != m->n_nodes || (int64_t)nc[0] * nc[1] * nc[2] != m->n_cells)
      return false;
    const int32_t N = m->n_nodes;
    double x0[3], x1[3], h[3] = {1, 1, 1};
    bounding_box(m, x0, x1);
    for (int d = 0; d < dim; ++d)
      {
        h[d] = (x1[d] - x0[d]) / nc[d];
        if (!(h[d] > 0))
          return false;
      }
    pfm::raw_vector<int32_t> local_of_box((size_t)nn); // every entry is written below or the mesh is rejected
    pfm::raw_vector<int32_t> box_of_local((size_t)N);
    std::atomic<bool> ok{true};
    parallel_for(N, [&](int64_t nb, int64_t ne) {
      for (int64_t n = nb; n < ne; ++n)
        {
          int64_t idx[3] = {0, 0, 0};
          for (int d = 0; d < dim; ++d)
            {
              const double t = (m->coords[(size_t)n * dim + d] - x0[d]) / h[d];
              idx[d] = llround(t);
              if (std::abs(t - (double)idx[d]) > 1e-9 || idx[d] < 0 || idx[d] > nc[d])
                {
                  ok = false;
                  return;
                }
            }
          box_of_local[n] = (int32_t)(idx[0] + (int64_t)NX * (idx[1] + (int64_t)NY * idx[2]));
        }
    });
    if (!ok)
      return false;
    // N = nn nodes on nn positions: a bijection unless two nodes share one (duplicated coordinates, e.g. a slit) -- then
    // one of the two does not find itself at its position (racing writers of one entry: either value shows the clash)
    parallel_for(N, [&](int64_t nb, int64_t ne) {
      for (int64_t n = nb; n < ne; ++n)
        __atomic_store_n(&local_of_box[(size_t)box_of_local[n]], (int32_t)n, __ATOMIC_RELAXED);
    });
    parallel_for(N, [&](int64_t nb, int64_t ne) {
      for (int64_t n = nb; n < ne; ++n)
        if (local_of_box[(size_t)box_of_local[n]] != (int32_t)n)
          {
            ok = false;
            return;
          }
    });
    if (!ok)
      return false;
    // every lattice cell must be present exactly once, vertices in deal.II order
    pfm::raw_vector<uint8_t> seen((size_t)m->n_cells);
    parallel_for(m->n_cells, [&](int64_t b, int64_t e) { std::fill(seen.begin() + b, seen.begin() + e, (uint8_t)0); }, 1 << 20);
    parallel_for(m->n_cells, [&](int64_t cb, int64_t ce) {
      for (int64_t cell = cb; cell < ce; ++cell)
        {
          const int64_t b0 = box_of_local[m->cell_nodes[cell * nv]];
          const int64_t i = b0 % NX, j = (b0 / NX) % NY, k = b0 / ((int64_t)NX * NY);
          if (i >= nc[0] || j >= nc[1] || (dim == 3 && k >= nc[2]))
            {
              ok = false;
              return;
            }
          for (int a = 0; a < nv; ++a)
            {
              const int64_t b = (i + (a & 1)) + (int64_t)NX * ((j + ((a >> 1) & 1)) + (int64_t)NY * (k + ((a >> 2) & 1)));
              if (local_of_box[b] != m->cell_nodes[cell * nv + a])
                {
                  ok = false;
                  return;
                }
            }
          seen[i + (int64_t)nc[0] * (j + (int64_t)nc[1] * k)] = 1; // distinct cells write distinct bytes unless duplicated
        }
    });
    if (!ok)
      return false;
    parallel_for(m->n_cells, [&](int64_t cb, int64_t ce) {
      for (int64_t cell = cb; cell < ce; ++cell)
        if (!seen[cell])
          {
            ok = false; // n_cells matches the box, so a missing cell means another one is present twice
            return;
          }
    });
    if (!ok)
      return false;
    L.NX = NX;
    L.NY = NY;
    L.NZ = NZ;
    for (int d = 0; d < 3; ++d)
      {
        L.nc[d] = nc[d];
        L.h[d] = h[d];
      }
    L.local_of_box.swap(local_of_box);
    L.box_of_local.swap(box_of_local);
    return true;
  }

  // neighbours of owned lattice node n in lattice-offset order; returns their number, mask bit o = offset o exists
  int lattice_row(const Lattice &L, int dim, int64_t n, int32_t (&q)[27], uint32_t &mask)
  {
    const int NX = L.NX, NY = L.NY, NZ = L.NZ, no = dim == 3 ? 27 : 9;
    const int64_t b = L.box_of_local[n];
    const int i = (int)(b % NX), j = (int)((b / NX) % NY), k = (int)(b / ((int64_t)NX * NY));
    int deg = 0;
    mask = 0;
    for (int o = 0; o < no; ++o)
      {
        const int ii = i + (o % 3) - 1, jj = j + ((o / 3) % 3) - 1, kk = k + (dim == 3 ? (o / 9) - 1 : 0);
        if (ii < 0 || ii >= NX || jj < 0 || jj >= NY || kk < 0 || kk >= NZ)
          continue;
        mask |= 1u << o;
        q[deg++] = L.local_of_box[ii + (int64_t)NX * (jj + (int64_t)NY * kk)];
      }
    return deg;
  }

  // class of a cell in the tables the colourings fill: one of the plain classes, the last (atomic) class, or not listed
  constexpr uint8_t NONE = 255, ATOMIC = 254;
  // the cells by class, ascending within a class, the atomic class as class nk - 1: a counting sort, chunked over the host
  // threads.  out.ptr [nk + 1], out.order (one entry when no cell is listed).
  void sort_by_class(const uint8_t *col, int64_t NC, int nk, Colours &out)
  {
    out.ptr.assign((size_t)nk + 1, 0);
    const int nt = chunks_for(NC, 65536);
    std::vector<long long> hist((size_t)nt * nk, 0);
    parallel_chunks(nt, [&](int t) {
      long long *hh = hist.data() + (size_t)t * nk;
      for (int64_t cell = NC * t / nt; cell < NC * (t + 1) / nt; ++cell)
        if (col[cell] != NONE)
          ++hh[col[cell] == ATOMIC ? nk - 1 : col[cell]];
    });
    for (int k = 0; k < nk; ++k)
      {
        long long at = out.ptr[k];
        for (int t = 0; t < nt; ++t)
          {
            const long long cnt = hist[(size_t)t * nk + k];
            hist[(size_t)t * nk + k] = at;
            at += cnt;
          }
        out.ptr[(size_t)k + 1] = at;
      }
    out.order.resize((size_t)std::max<long long>(out.ptr.back(), 1));
    out.order[0] = 0;
    parallel_chunks(nt, [&](int t) {
      long long *fill = hist.data() + (size_t)t * nk;
      for (int64_t cell = NC * t / nt; cell < NC * (t + 1) / nt; ++cell)
        if (col[cell] != NONE)
          out.order[(size_t)fill[col[cell] == ATOMIC ? nk - 1 : col[cell]]++] = (int32_t)cell;
    });
  }

  int resolved_nodes(int64_t cell, int nv, CellView node_of, const int32_t *hn_index, const int64_t *hn_ptr, const int32_t *hn_parents, int32_t *out,
                     int max_nodes)
  {
    int R = 0;
    for (int a = 0; a < nv; ++a)
      {
        const int32_t A = node_of(cell, a);
        const int32_t k = hn_index ? hn_index[A] : -1;
        const int64_t rb = k < 0 ? 0 : hn_ptr[k], re = k < 0 ? 1 : hn_ptr[k + 1];
        for (int64_t r = rb; r < re; ++r)
          {
            const int32_t P = k < 0 ? A : hn_parents[r];
            bool known = false;
            for (int t = 0; t < R; ++t)
              known = known || out[t] == P;
            if (known)
              continue;
            if (R == max_nodes)
              return max_nodes + 1;
            out[R++] = P;
          }
      }
    return R;
  }

  void greedy_colours(int64_t NC, int nv, int32_t N, CellView node_of, const int32_t *hn_index, const uint8_t *subset, const std::atomic<bool> *cancel,
                      Colours &out, const int64_t *hn_ptr, const int32_t *hn_parents)
  {
    pfm::raw_vector<uint8_t> col((size_t)NC);
    pfm::raw_vector<uint64_t> used((size_t)N);
    parallel_for(N, [&](int64_t b, int64_t e) { std::fill(used.begin() + b, used.begin() + e, (uint64_t)0); });
    int n_col = 0;
    for (int64_t cell = 0; cell < NC; ++cell)
      {
        if (subset && !subset[cell])
          {
            col[cell] = NONE;
            continue;
          }
        if ((cell & 4095) == 0 && cancel && cancel->load(std::memory_order_relaxed))
          {
            out.cancelled = true;
            return;
          }
        uint64_t mask = 0;
        bool hanging = false;
        int32_t nd[16];
        int nn = nv;
        for (int a = 0; a < nv; ++a)
          {
            nd[a] = node_of(cell, a);
            hanging = hanging || (hn_index && hn_index[nd[a]] >= 0);
          }
        bool colourable = !hanging;
        if (hanging && hn_ptr)
          {
            nn = resolved_nodes(cell, nv, node_of, hn_index, hn_ptr, hn_parents, nd, 16);
            colourable = nn <= 16;
          }
        if (colourable)
          for (int a = 0; a < nn; ++a)
            mask |= used[nd[a]];
        int k = 63;
        if (colourable && ~mask != 0)
          k = __builtin_ctzll(~mask);
        if (k < 62)
          {
            for (int a = 0; a < nn; ++a)
              used[nd[a]] |= 1ull << k;
            n_col = std::max(n_col, k + 1);
            col[cell] = (uint8_t)k;
          }
        else
          {
            col[cell] = ATOMIC;
            out.overflow = out.overflow || !hanging || (hn_ptr && colourable); // a cell that should have had a colour and found none
          }
      }
    sort_by_class(col.data(), NC, n_col + 1, out);
  }

  bool ring_cells(int64_t NC, int nv, int32_t N, CellView node_of, const int32_t *hn_index, const int64_t *hn_ptr, const int32_t *hn_parents,
                  std::vector<uint8_t> &ring, bool hanging_coloured)
  {
    ring.clear();
    if (!hn_index)
      return false;
    pfm::raw_vector<uint8_t> touched((size_t)N), at_hanging((size_t)NC);
    parallel_for(N, [&](int64_t b, int64_t e) { std::fill(touched.begin() + b, touched.begin() + e, (uint8_t)0); });
    std::atomic<bool> any_atomic{false}, any_ring{false};
    parallel_for(NC, [&](int64_t cb, int64_t ce) {
      bool mine = false;
      for (int64_t cell = cb; cell < ce; ++cell)
        {
          bool hanging = false;
          for (int a = 0; a < nv; ++a)
            hanging = hanging || hn_index[node_of(cell, a)] >= 0;
          if (hanging && hanging_coloured)
            {
              // (greedy_colours: such a cell sits in a plain class unless it has more than 16 resolved nodes)
              int32_t tmp[16];
              hanging = resolved_nodes(cell, nv, node_of, hn_index, hn_ptr, hn_parents, tmp, 16) > 16;
            }
          at_hanging[cell] = hanging ? 1 : 0;
          if (!hanging)
            continue;
          mine = true;
          for (int a = 0; a < nv; ++a)
            {
              const int32_t n = node_of(cell, a);
              touched[n] = 1; // (bytes; racing writers store the same value)
              const int32_t k = hn_index[n];
              if (k >= 0)
                for (long long j = hn_ptr[k]; j < hn_ptr[k + 1]; ++j)
                  touched[hn_parents[j]] = 1;
            }
        }
      if (mine)
        any_atomic = true;
    });
    if (!any_atomic)
      return false;
    ring.resize((size_t)NC);
    parallel_for(NC, [&](int64_t cb, int64_t ce) {
      bool mine = false;
      for (int64_t cell = cb; cell < ce; ++cell)
        {
          bool r = false;
          if (!at_hanging[cell])
            for (int a = 0; a < nv; ++a)
              r = r || touched[node_of(cell, a)] != 0;
          ring[cell] = r ? 1 : 0;
          mine = mine || r;
        }
      if (mine)
        any_ring = true;
    });
    if (!any_ring)
      ring.clear();
    return any_ring;
  }

  // Every loop below runs over cells, nodes or blocks in chunks on the host threads (HostPool): the classification is part of
  // the context rebuild after every refine_mesh.  Tables that several cells write (the cell of which a node is vertex a, the
  // node at a lattice position) are filled with compare-and-swap: a second claimant marks the entry instead of racing.
  PatchPlan plan_patches2d(const pfm_mesh_desc *m, const std::vector<int32_t> &hn_index)
  {
    PatchPlan pl;
    const int32_t N = m->n_nodes, NO = m->n_owned_nodes;
    const int64_t NC = m->n_cells;
    if (m->dim != 2 || NC == 0 || Switches::no_patch())
      return pl;
    // PFM_CTX_TIMING=1: the phases of this classification on stderr (it runs on a thread of its own)
    PhaseClock clk("[pfm_ctx_create]     plan: %-22s %6.2f ms\n");
    const double *X = m->coords;
    double lo[3], hi[3];
    bounding_box(m, lo, hi);
    const double xmin = lo[0], ymin = lo[1], xmax = hi[0], ymax = hi[1];
    const double tol = 1e-9 * std::max(xmax - xmin, ymax - ymin);
    clk.mark("bounds");
    // level of a cell (by its size), lattice position of its lower-left vertex
    struct Level
    {
      double hx, hy;
      long long ix0, iy0, ix1, iy1; // cell index range
    };
    struct Size
    {
      double hx, hy;
    };
    // the size of an EXACT axis-parallel rectangle in deal.II's vertex order (the patch kernel takes J = diag(hx, hy));
    // any other cell stays with the general family
    auto cell_size = [&](int64_t k, double &hx, double &hy, double &x0, double &y0) {
      const int32_t *cn = m->cell_nodes + 4 * k;
      x0 = X[2 * cn[0]], y0 = X[2 * cn[0] + 1];
      const double x1 = X[2 * cn[1]], y1 = X[2 * cn[1] + 1];
      const double x2 = X[2 * cn[2]], y2 = X[2 * cn[2] + 1], x3 = X[2 * cn[3]], y3 = X[2 * cn[3] + 1];
      hx = x1 - x0, hy = y2 - y0;
      return hx > tol && hy > tol && y1 == y0 && x2 == x0 && x3 == x1 && y3 == y2;
    };
    auto same_size = [](const Size &a, double hx, double hy) { return std::fabs(a.hx - hx) <= 1e-9 * hx && std::fabs(a.hy - hy) <= 1e-9 * hy; };
    const int ntc = chunks_for(NC, 8192);
    std::vector<Level> levels;
    {
      // the sizes that occur, in the order of their first cell: per chunk, then merged in chunk order
      std::vector<std::vector<Size>> found((size_t)ntc);
      parallel_chunks(ntc, [&](int t) {
        std::vector<Size> &mine = found[(size_t)t];
        for (int64_t k = NC * t / ntc; k < NC * (t + 1) / ntc; ++k)
          {
            double hx, hy, x0, y0;
            if (!cell_size(k, hx, hy, x0, y0))
              continue;
            bool known = false;
            for (const Size &q : mine)
              known = known || same_size(q, hx, hy);
            if (!known && mine.size() < 100)
              mine.push_back(Size{hx, hy});
          }
      });
      for (const auto &mine : found)
        for (const Size &q : mine)
          {
            bool known = false;
            for (const Level &l : levels)
              known = known || same_size(Size{l.hx, l.hy}, q.hx, q.hy);
            if (!known && levels.size() < 100)
              levels.push_back(Level{q.hx, q.hy, LLONG_MAX, LLONG_MAX, LLONG_MIN, LLONG_MIN});
          }
    }
    if (levels.empty())
      return pl;
    const int NL = (int)levels.size();
    clk.mark("levels");
    pfm::raw_vector<int8_t> cell_level((size_t)NC); // (written by the loop below: the pages are first touched by its threads)
    pfm::raw_vector<int32_t> cix((size_t)NC), ciy((size_t)NC);
    {
      std::vector<Level> part((size_t)ntc * NL);
      std::atomic<bool> too_far{false};
      parallel_chunks(ntc, [&](int t) {
        Level *mine = part.data() + (size_t)t * NL;
        for (int l = 0; l < NL; ++l)
          mine[l] = Level{0, 0, LLONG_MAX, LLONG_MAX, LLONG_MIN, LLONG_MIN};
        for (int64_t k = NC * t / ntc; k < NC * (t + 1) / ntc; ++k)
          {
            cell_level[k] = -1;
            double hx, hy, x0, y0;
            if (!cell_size(k, hx, hy, x0, y0))
              continue;
            int L = -1;
            for (int l = 0; l < NL; ++l)
              if (same_size(Size{levels[l].hx, levels[l].hy}, hx, hy))
                L = l;
            if (L < 0)
              continue;
            const double fx = (x0 - xmin) / levels[L].hx, fy = (y0 - ymin) / levels[L].hy;
            const long long ix = std::llround(fx), iy = std::llround(fy);
            if (std::fabs(fx - (double)ix) > 1e-6 || std::fabs(fy - (double)iy) > 1e-6)
              continue; // off the level's lattice
            if (ix > (1 << 30) || iy > (1 << 30))
              {
                too_far = true;
                continue;
              }
            cell_level[k] = (int8_t)L;
            cix[k] = (int32_t)ix;
            ciy[k] = (int32_t)iy;
            Level &lv = mine[L];
            lv.ix0 = std::min(lv.ix0, ix);
            lv.iy0 = std::min(lv.iy0, iy);
            lv.ix1 = std::max(lv.ix1, ix);
            lv.iy1 = std::max(lv.iy1, iy);
          }
      });
      (void)too_far; // such cells keep level -1: general family
      for (int t = 0; t < ntc; ++t)
        for (int l = 0; l < NL; ++l)
          {
            const Level &q = part[(size_t)t * NL + l];
            Level &lv = levels[l];
            lv.ix0 = std::min(lv.ix0, q.ix0);
            lv.iy0 = std::min(lv.iy0, q.iy0);
            lv.ix1 = std::max(lv.ix1, q.ix1);
            lv.iy1 = std::max(lv.iy1, q.iy1);
          }
    }
    // incident cells per node: inc[4 n + a] = the cell of which n is vertex a (-1 none, -2 two cells claim the corner)
    clk.mark("cell levels");
    pfm::raw_vector<int32_t> inc((size_t)N * 4);
    parallel_for((int64_t)N * 4, [&](int64_t b, int64_t e) { std::fill(inc.begin() + b, inc.begin() + e, -1); });
    parallel_for(NC, [&](int64_t cb, int64_t ce) {
      for (int64_t k = cb; k < ce; ++k)
        for (int a = 0; a < 4; ++a)
          {
            int32_t *slot = &inc[(size_t)m->cell_nodes[4 * k + a] * 4 + a];
            int32_t expect = -1;
            if (!__atomic_compare_exchange_n(slot, &expect, (int32_t)k, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED))
              __atomic_store_n(slot, -2, __ATOMIC_RELAXED);
          }
    }, 8192);
    pfm::raw_vector<uint8_t> is_parent((size_t)N), dup((size_t)N);
    pfm::raw_vector<int8_t> node_level((size_t)N); // of regular nodes: the common level of their four cells
    std::vector<uint8_t> regular((size_t)N); // (handed over to the plan)
    parallel_for(N, [&](int64_t b, int64_t e) {
      std::fill(is_parent.begin() + b, is_parent.begin() + e, (uint8_t)0);
      std::fill(dup.begin() + b, dup.begin() + e, (uint8_t)0);
      std::fill(node_level.begin() + b, node_level.begin() + e, (int8_t)-1);
      std::fill(regular.begin() + b, regular.begin() + e, (uint8_t)0);
    });
    if (m->n_hanging > 0)
      for (int64_t j = 0; j < m->hn_ptr[m->n_hanging]; ++j)
        is_parent[m->hn_parents[j]] = 1;
    // two nodes at one lattice position (the lips of a slit, meshes/unit_slit.inp): neither they nor their neighbours are
    // regular.  One table per level (node at a lattice position), all in one array.
    {
      std::vector<long long> off((size_t)NL + 1, 0), Wn((size_t)NL, 0);
      for (int L = 0; L < NL; ++L)
        {
          const Level &lv = levels[L];
          long long sz = 0;
          if (lv.ix0 <= lv.ix1)
            {
              const long long W = lv.ix1 - lv.ix0 + 2, Hh = lv.iy1 - lv.iy0 + 2;
              if ((double)W * (double)Hh <= 4.0e8)
                {
                  sz = W * Hh;
                  Wn[L] = W;
                }
            }
          off[(size_t)L + 1] = off[L] + sz;
        }
      pfm::raw_vector<int32_t> node_at((size_t)off[NL]);
      parallel_for(off[NL], [&](int64_t b, int64_t e) { std::fill(node_at.begin() + b, node_at.begin() + e, -1); });
      parallel_for(NC, [&](int64_t cb, int64_t ce) {
        for (int64_t k = cb; k < ce; ++k)
          {
            const int L = cell_level[k];
            if (L < 0 || Wn[L] == 0)
              continue;
            const Level &lv = levels[L];
            for (int a = 0; a < 4; ++a)
              {
                const int32_t n = m->cell_nodes[4 * k + a];
                int32_t *slot = &node_at[(size_t)(off[L] + (ciy[k] - lv.iy0 + (a >> 1)) * Wn[L] + (cix[k] - lv.ix0 + (a & 1)))];
                int32_t seen = -1;
                if (!__atomic_compare_exchange_n(slot, &seen, n, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED) && seen != n)
                  dup[n] = dup[seen] = 1; // (bytes, racing writers store the same value)
              }
          }
      }, 8192);
    }
    auto hanging = [&](int32_t n) { return (!hn_index.empty() && hn_index[n] >= 0) || dup[n] != 0; };
    clk.mark("incident cells, duplicates");
    int64_t n_regular = 0;
    {
      const int nt = chunks_for(NO, 8192);
      std::vector<int64_t> cnt((size_t)nt, 0);
      parallel_chunks(nt, [&](int t) {
        int64_t mine = 0;
        for (int64_t n = (int64_t)NO * t / nt; n < (int64_t)NO * (t + 1) / nt; ++n)
          {
            if (hanging((int32_t)n) || is_parent[n])
              continue;
            const int32_t k0 = inc[(size_t)n * 4 + 0], k1 = inc[(size_t)n * 4 + 1], k2 = inc[(size_t)n * 4 + 2], k3 = inc[(size_t)n * 4 + 3];
            if (k0 < 0 || k1 < 0 || k2 < 0 || k3 < 0)
              continue; // not exactly four cells, one at each corner
            const int8_t L = cell_level[k0];
            if (L < 0 || cell_level[k1] != L || cell_level[k2] != L || cell_level[k3] != L)
              continue;
            bool ok = true;
            for (const int32_t k : {k0, k1, k2, k3})
              for (int b = 0; b < 4; ++b)
                ok = ok && !hanging(m->cell_nodes[4 * k + b]);
            // the four cells really are the 2 x 2 cells around n on the level's lattice
            ok = ok && cix[k2] == cix[k3] + 1 && ciy[k2] == ciy[k3] && cix[k1] == cix[k3] && ciy[k1] == ciy[k3] + 1 && cix[k0] == cix[k3] + 1 &&
                 ciy[k0] == ciy[k3] + 1;
            if (ok)
              {
                regular[n] = 1;
                node_level[n] = L;
                ++mine;
              }
          }
        cnt[(size_t)t] = mine;
      });
      for (const int64_t q : cnt)
        n_regular += q;
    }
    if (n_regular == 0)
      return pl;
    clk.mark("regular nodes");
    // blocks: block (bx, by) of a level owns the lattice nodes [7 bx, 7 bx + 6] x [7 by, 7 by + 6] and holds the cells
    // [7 bx - 1, 7 bx + 6] x [7 by - 1, 7 by + 6]; node (i, j) of the lattice = upper-right vertex of cell (i - 1, j - 1)
    pfm::raw_vector<int32_t> blk_cells, blk_nodes;
    for (int L = 0; L < NL; ++L)
      {
        const Level &lv = levels[L];
        if (lv.ix0 > lv.ix1)
          continue;
        const long long W = lv.ix1 - lv.ix0 + 1, Hh = lv.iy1 - lv.iy0 + 1;
        if ((double)W * (double)Hh > 4.0e8)
          continue; // a level whose bounding box is mostly empty: not worth a dense table
        pfm::raw_vector<int32_t> at((size_t)(W * Hh));
        parallel_for(W * Hh, [&](int64_t b, int64_t e) { std::fill(at.begin() + b, at.begin() + e, -1); });
        parallel_for(NC, [&](int64_t cb, int64_t ce) {
          for (int64_t k = cb; k < ce; ++k)
            if (cell_level[k] == (int8_t)L)
              at[(size_t)((ciy[k] - lv.iy0) * W + (cix[k] - lv.ix0))] = (int32_t)k;
        });
        auto cell_at = [&](long long i, long long j) -> int32_t {
          return (i < lv.ix0 || i > lv.ix1 || j < lv.iy0 || j > lv.iy1) ? -1 : at[(size_t)((j - lv.iy0) * W + (i - lv.ix0))];
        };
        auto floordiv = [](long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
        const long long bx0 = floordiv(lv.ix0, 7), bx1 = floordiv(lv.ix1 + 1, 7), by0 = floordiv(lv.iy0, 7), by1 = floordiv(lv.iy1 + 1, 7);
        const long long nbx = bx1 - bx0 + 1, nblk = nbx * (by1 - by0 + 1);
        const int nt = chunks_for(nblk, 64);
        std::vector<std::vector<int32_t>> pc((size_t)nt), pn((size_t)nt);
        parallel_chunks(nt, [&](int t) {
          for (long long q = nblk * t / nt; q < nblk * (t + 1) / nt; ++q)
            {
              const long long by = by0 + q / nbx, bx = bx0 + q % nbx;
              int32_t cells[64], nodes[81];
              bool any = false;
              for (int i = 0; i < 81; ++i)
                nodes[i] = -1;
              for (int cy = 0; cy < 8; ++cy)
                for (int cx = 0; cx < 8; ++cx)
                  {
                    const int32_t k = cell_at(7 * bx - 1 + cx, 7 * by - 1 + cy);
                    cells[cy * 8 + cx] = k;
                    if (k >= 0)
                      for (int a = 0; a < 4; ++a)
                        nodes[(cx + (a & 1)) + 9 * (cy + (a >> 1))] = m->cell_nodes[4 * k + a];
                  }
              for (int hy = 1; hy <= 7; ++hy)
                for (int hx = 1; hx <= 7; ++hx)
                  {
                    const int32_t n = nodes[hx + 9 * hy];
                    any = any || (n >= 0 && n < NO && regular[n] && node_level[n] == (int8_t)L);
                  }
              if (!any)
                continue;
              // a regular node of ANOTHER level may sit at a position of this block (coinciding lattices): it is not ours
              for (int hy = 1; hy <= 7; ++hy)
                for (int hx = 1; hx <= 7; ++hx)
                  {
                    const int32_t n = nodes[hx + 9 * hy];
                    if (n >= 0 && n < NO && regular[n] && node_level[n] != (int8_t)L)
                      nodes[hx + 9 * hy] = -1;
                  }
              pc[(size_t)t].insert(pc[(size_t)t].end(), cells, cells + 64);
              pn[(size_t)t].insert(pn[(size_t)t].end(), nodes, nodes + 81);
            }
        });
        {
          // the chunks' pieces behind one another, copied by the chunks' threads
          std::vector<size_t> oc((size_t)nt + 1, blk_cells.size()), on((size_t)nt + 1, blk_nodes.size());
          for (int t = 0; t < nt; ++t)
            {
              oc[(size_t)t + 1] = oc[(size_t)t] + pc[(size_t)t].size();
              on[(size_t)t + 1] = on[(size_t)t] + pn[(size_t)t].size();
            }
          blk_cells.resize(oc[(size_t)nt]);
          blk_nodes.resize(on[(size_t)nt]);
          parallel_chunks(nt, [&](int t) {
            std::copy(pc[(size_t)t].begin(), pc[(size_t)t].end(), blk_cells.begin() + (std::ptrdiff_t)oc[(size_t)t]);
            std::copy(pn[(size_t)t].begin(), pn[(size_t)t].end(), blk_nodes.begin() + (std::ptrdiff_t)on[(size_t)t]);
          });
        }
      }
    const int n_blocks = (int)(blk_cells.size() / 64);
    clk.mark("blocks");
    if (n_blocks == 0)
      return pl;
    // only the rows some block really writes are the patch kernel's (a level without a table above keeps its rows general)
    {
      std::vector<uint8_t> covered((size_t)N);
      parallel_for(N, [&](int64_t b, int64_t e) { std::fill(covered.begin() + b, covered.begin() + e, (uint8_t)0); });
      const int nt = chunks_for(n_blocks, 64);
      std::vector<int64_t> cnt((size_t)nt, 0);
      parallel_chunks(nt, [&](int t) {
        int64_t mine = 0;
        for (int64_t b = (int64_t)n_blocks * t / nt; b < (int64_t)n_blocks * (t + 1) / nt; ++b)
          for (int hy = 1; hy <= 7; ++hy)
            for (int hx = 1; hx <= 7; ++hx)
              {
                const int32_t n = blk_nodes[(size_t)b * 81 + hx + 9 * hy];
                if (n >= 0 && n < NO && regular[n] && !__atomic_exchange_n(&covered[n], (uint8_t)1, __ATOMIC_RELAXED))
                  ++mine;
              }
        cnt[(size_t)t] = mine;
      });
      n_regular = 0;
      for (const int64_t q : cnt)
        n_regular += q;
      regular.swap(covered);
    }
    // the rows of the general family (zeroed before every Jacobian; the patch kernel stores its rows whole)
    clk.mark("covered");
    std::vector<int32_t> rows_general = parallel_select(0, NO, [&](int64_t n) { return !regular[n]; });
    pl.hang.resize((size_t)N);
    parallel_for(N, [&](int64_t nb, int64_t ne) {
      for (int64_t n = nb; n < ne; ++n)
        pl.hang[n] = hanging((int32_t)n) ? 1 : 0;
    });
    pl.regular.swap(regular);
    pl.blk_cells.swap(blk_cells);
    pl.blk_nodes.swap(blk_nodes);
    pl.rows_general.swap(rows_general);
    clk.mark("rows, flags");
    pl.n_regular = n_regular;
    pl.n_blocks = n_blocks;
    return pl;
  }

  PatchPlan3 plan_patches3d(const pfm_mesh_desc *m, const std::vector<int32_t> &hn_index)
  {
    PatchPlan3 pl;
    const int32_t N = m->n_nodes, NO = m->n_owned_nodes;
    const int64_t NC = m->n_cells;
    if (m->dim != 3 || NC == 0 || Switches::no_patch())
      return pl;
    const double *X = m->coords;
    double xmin[3], xmax[3];
    bounding_box(m, xmin, xmax);
    const double tol = 1e-9 * std::max(xmax[0] - xmin[0], std::max(xmax[1] - xmin[1], xmax[2] - xmin[2]));
    double amax = 0.0;
    for (int d = 0; d < 3; ++d)
      amax = std::max(amax, std::max(std::fabs(xmin[d]), std::fabs(xmax[d])));
    const double geo_tol = 16.0 * 2.220446049250313e-16 * amax;
    struct Lv
    {
      double h[3];
      long long clo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, chi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN}; // box of its cells' positions
    };
    std::vector<Lv> lv;
    std::vector<int8_t> cell_level((size_t)NC, -1);
    std::vector<long long> cpos((size_t)NC * 3, 0);
    for (int64_t k = 0; k < NC; ++k)
      {
        const int32_t *cn = m->cell_nodes + 8 * k;
        const double *p0 = X + 3 * (size_t)cn[0], *p7 = X + 3 * (size_t)cn[7];
        const double h[3] = {p7[0] - p0[0], p7[1] - p0[1], p7[2] - p0[2]};
        bool box = h[0] > tol && h[1] > tol && h[2] > tol;
        // an axis-parallel box in deal.II's vertex order, up to the rounding of the vertex positions (the kernels take
        // J = diag(h)): the midpoints a refinement creates are means of 2, 4 or 8 parents and agree only to a few ulp
        // unless the coordinates are dyadic
        for (int a = 0; a < 8 && box; ++a)
          {
            const double *pa = X + 3 * (size_t)cn[a];
            box = std::fabs(pa[0] - ((a & 1) ? p7[0] : p0[0])) <= geo_tol && std::fabs(pa[1] - ((a & 2) ? p7[1] : p0[1])) <= geo_tol &&
                  std::fabs(pa[2] - ((a & 4) ? p7[2] : p0[2])) <= geo_tol;
          }
        if (!box)
          continue;
        int L = -1;
        for (size_t l = 0; l < lv.size(); ++l)
          if (std::fabs(lv[l].h[0] - h[0]) <= 1e-9 * h[0] && std::fabs(lv[l].h[1] - h[1]) <= 1e-9 * h[1] && std::fabs(lv[l].h[2] - h[2]) <= 1e-9 * h[2])
            L = (int)l;
        if (L < 0)
          {
            if (lv.size() >= 100)
              continue;
            lv.push_back(Lv{});
            for (int d = 0; d < 3; ++d)
              lv.back().h[d] = h[d];
            L = (int)lv.size() - 1;
          }
        bool on = true;
        for (int d = 0; d < 3; ++d)
          {
            const double f = (p0[d] - xmin[d]) / lv[L].h[d];
            const long long i = std::llround(f);
            on = on && std::fabs(f - (double)i) <= 1e-6;
            cpos[3 * (size_t)k + d] = i;
          }
        if (on)
          {
            cell_level[k] = (int8_t)L;
            for (int d = 0; d < 3; ++d)
              {
                lv[L].clo[d] = std::min(lv[L].clo[d], cpos[3 * (size_t)k + d]);
                lv[L].chi[d] = std::max(lv[L].chi[d], cpos[3 * (size_t)k + d]);
              }
          }
      }
    if (lv.empty())
      return pl;
    // incident cells per node: count, common level, the 8 cells by the vertex the node is of them
    std::vector<uint8_t> n_inc((size_t)N, 0), is_parent((size_t)N, 0);
    std::vector<int8_t> node_level((size_t)N, -2);
    std::vector<int32_t> inc((size_t)N * 8, -1);
    for (int64_t k = 0; k < NC; ++k)
      for (int a = 0; a < 8; ++a)
        {
          const int32_t n = m->cell_nodes[8 * k + a];
          if (n_inc[n] < 255)
            ++n_inc[n];
          const int8_t L = cell_level[k];
          node_level[n] = (node_level[n] == -2) ? L : (node_level[n] == L ? L : (int8_t)-1);
          inc[(size_t)n * 8 + a] = (inc[(size_t)n * 8 + a] == -1) ? (int32_t)k : -2;
        }
    if (m->n_hanging > 0)
      for (int64_t j = 0; j < m->hn_ptr[m->n_hanging]; ++j)
        is_parent[m->hn_parents[j]] = 1;
    auto hanging = [&](int32_t n) { return !hn_index.empty() && hn_index[n] >= 0; };
    std::vector<uint8_t> regular((size_t)N, 0);
    std::vector<long long> npos((size_t)N * 3, 0);
    // Regular: every cell around the node that the level's box has room for exists, is of the node's level and has no
    // hanging vertex.  A cell position OUTSIDE the box of the level's cells may be missing: the node then lies on a face of the
    // level lattice -- for a level that reaches the boundary of the domain, on that boundary -- and the row-owner kernels
    // treat it like a face node of a uniform box (fewer than 27 neighbours, cells from index ranges).
    for (int32_t n = 0; n < NO; ++n)
      {
        if (n_inc[n] == 0 || node_level[n] < 0 || hanging(n) || is_parent[n])
          continue;
        const Lv &l = lv[(size_t)node_level[n]];
        bool ok = true;
        long long pn[3] = {0, 0, 0};
        bool have = false;
        for (int a = 0; a < 8 && !have; ++a)
          {
            const int32_t k = inc[(size_t)n * 8 + a];
            if (k >= 0)
              {
                have = true; // the cell of which n is vertex a lies at pn - (a_x, a_y, a_z)
                pn[0] = cpos[3 * (size_t)k] + (a & 1), pn[1] = cpos[3 * (size_t)k + 1] + ((a >> 1) & 1), pn[2] = cpos[3 * (size_t)k + 2] + (a >> 2);
              }
          }
        ok = have;
        for (int a = 0; a < 8 && ok; ++a)
          {
            const int32_t k = inc[(size_t)n * 8 + a];
            const long long cp[3] = {pn[0] - (a & 1), pn[1] - ((a >> 1) & 1), pn[2] - (a >> 2)};
            if (k == -1)
              {
                bool outside = false;
                for (int d = 0; d < 3; ++d)
                  outside = outside || cp[d] < l.clo[d] || cp[d] > l.chi[d];
                ok = outside;
                continue;
              }
            ok = k >= 0 && cpos[3 * (size_t)k] == cp[0] && cpos[3 * (size_t)k + 1] == cp[1] && cpos[3 * (size_t)k + 2] == cp[2];
            for (int b = 0; b < 8 && ok; ++b)
              ok = !hanging(m->cell_nodes[8 * (size_t)k + b]);
          }
        if (ok)
          {
            regular[n] = 1;
            for (int d = 0; d < 3; ++d)
              npos[3 * (size_t)n + d] = pn[d];
          }
      }
    // per level: the lattice of the box of its cells, the tables
    const long long max_table = Switches::overlay3_max_table(), min_rows = Switches::overlay3_min_rows();
    for (size_t L = 0; L < lv.size(); ++L)
      {
        long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, hi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
        int64_t cnt = 0;
        for (int32_t n = 0; n < NO; ++n)
          if (regular[n] && node_level[n] == (int8_t)L)
            {
              ++cnt;
              for (int d = 0; d < 3; ++d)
                {
                  lo[d] = std::min(lo[d], npos[3 * (size_t)n + d]);
                  hi[d] = std::max(hi[d], npos[3 * (size_t)n + d]);
                }
            }
        for (int d = 0; d < 3 && cnt; ++d) // the lattice of the level: the nodes of the box of its cells
          {
            lo[d] = lv[L].clo[d];
            hi[d] = lv[L].chi[d] + 1;
          }
        const double vol = cnt ? (double)(hi[0] - lo[0] + 1) * (double)(hi[1] - lo[1] + 1) * (double)(hi[2] - lo[2] + 1) : 0.0;
        if (cnt < min_rows || vol > (double)max_table || vol > 64.0 * (double)cnt)
          {
            // too few rows, or a box that is mostly empty (a thin refined band): these rows stay with the general family
            for (int32_t n = 0; n < NO; ++n)
              if (regular[n] && node_level[n] == (int8_t)L)
                regular[n] = 0;
            continue;
          }
        Level3 lev;
        for (int d = 0; d < 3; ++d)
          {
            lev.h[d] = lv[L].h[d];
            lev.lo[d] = lo[d];
            lev.dims[d] = (int)(hi[d] - lo[d] + 1);
          }
        const long long NX = lev.dims[0], NY = lev.dims[1], NZ = lev.dims[2];
        lev.node_at.assign((size_t)(NX * NY * NZ), -1);
        lev.row_at.assign((size_t)(NX * NY * NZ), -1);
        const bool het = m->cell_lambda && m->cell_mu;
        if (het)
          {
            lev.lam.assign((size_t)((NX - 1) * (NY - 1) * (NZ - 1)), 0.0);
            lev.mu.assign((size_t)((NX - 1) * (NY - 1) * (NZ - 1)), 0.0);
          }
        bool clash = false;
        for (int64_t k = 0; k < NC; ++k)
          if (cell_level[k] == (int8_t)L)
            {
              const long long ci = cpos[3 * (size_t)k] - lev.lo[0], cj = cpos[3 * (size_t)k + 1] - lev.lo[1], ck = cpos[3 * (size_t)k + 2] - lev.lo[2];
              if (ci < 0 || ci >= NX - 1 || cj < 0 || cj >= NY - 1 || ck < 0 || ck >= NZ - 1)
                continue;
              for (int a = 0; a < 8; ++a)
                {
                  int32_t &slot = lev.node_at[(size_t)((ci + (a & 1)) + NX * ((cj + ((a >> 1) & 1)) + NY * (ck + (a >> 2))))];
                  const int32_t n = m->cell_nodes[8 * (size_t)k + a];
                  if (slot == -1)
                    slot = n;
                  else if (slot != n)
                    clash = true; // two nodes at one lattice position (a slit): not a mesh for this overlay
                }
              if (het)
                {
                  lev.lam[(size_t)(ci + (NX - 1) * (cj + (NY - 1) * ck))] = m->cell_lambda[k];
                  lev.mu[(size_t)(ci + (NX - 1) * (cj + (NY - 1) * ck))] = m->cell_mu[k];
                }
            }
        if (clash)
          {
            for (int32_t n = 0; n < NO; ++n)
              if (regular[n] && node_level[n] == (int8_t)L)
                regular[n] = 0;
            continue;
          }
        for (int32_t n = 0; n < NO; ++n)
          if (regular[n] && node_level[n] == (int8_t)L)
            {
              const long long i = npos[3 * (size_t)n] - lev.lo[0], j = npos[3 * (size_t)n + 1] - lev.lo[1], kk = npos[3 * (size_t)n + 2] - lev.lo[2];
              lev.row_at[(size_t)(i + NX * (j + NY * kk))] = n;
              ++lev.n_rows;
            }
        pl.levels.push_back(std::move(lev));
      }
    if (pl.levels.empty())
      return pl;
    for (int32_t n = 0; n < NO; ++n)
      {
        pl.n_regular += regular[n];
        if (!regular[n])
          pl.rows_general.push_back(n);
      }
    pl.hang.assign((size_t)N, 0);
    for (int32_t n = 0; n < N; ++n)
      pl.hang[n] = hanging(n) ? 1 : 0;
    pl.regular.swap(regular);
    return pl;
  }
  const char *hanging_index(const pfm_mesh_desc *m, std::vector<int32_t> &hn_index)
  {
    const int32_t N = m->n_nodes;
    hn_index.clear();
    if (m->n_hanging > 0)
      {
        hn_index.assign(N, -1);
        for (int32_t k = 0; k < m->n_hanging; ++k)
          {
            if (m->hn_nodes[k] < 0 || m->hn_nodes[k] >= N)
              return "hn_nodes out of range";
            hn_index[m->hn_nodes[k]] = k;
          }
        for (int64_t j = 0; j < m->hn_ptr[m->n_hanging]; ++j)
          if (m->hn_parents[j] < 0 || m->hn_parents[j] >= N || hn_index[m->hn_parents[j]] >= 0)
            return "hanging table must be closed (parents unconstrained)";
      }
    return nullptr;
  }

  bool hanging_cells(const pfm_mesh_desc *m, const int32_t *hn_idx, int max_parents, std::vector<int32_t> &hcells, raw_vector<int32_t> &hcell)
  {
    const int nv = 1 << m->dim;
    const int64_t NC = m->n_cells;
    hcells.clear();
    hcell.clear();
    bool fits = true;
    for (int32_t k = 0; k < m->n_hanging; ++k)
      fits = fits && m->hn_ptr[k + 1] - m->hn_ptr[k] <= max_parents;
    if (!fits)
      return false;
    hcells = parallel_select(0, NC, [&](int64_t cell) {
      bool h = false;
      for (int a = 0; a < nv; ++a)
        h = h || hn_idx[m->cell_nodes[cell * nv + a]] >= 0;
      return h;
    });
    if (hcells.empty())
      return false;
    hcell.resize((size_t)NC);
    parallel_for(NC, [&](int64_t b, int64_t e) { std::fill(hcell.begin() + b, hcell.begin() + e, -1); });
    parallel_for((int64_t)hcells.size(), [&](int64_t b, int64_t e) {
      for (int64_t i = b; i < e; ++i)
        hcell[(size_t)hcells[(size_t)i]] = (int32_t)i;
    });
    return true;
  }

  void lattice_colours(const pfm_mesh_desc *m, const LatticeHost &lattice, Colours &full)
  {
    const int dim = m->dim, nv = 1 << dim;
    const int64_t NC = m->n_cells;
    const int64_t NX = lattice.NX, NY = lattice.NY;
    pfm::raw_vector<uint8_t> col((size_t)NC);
    parallel_for(NC, [&](int64_t cb, int64_t ce) {
      for (int64_t cell = cb; cell < ce; ++cell)
        {
          const int64_t b0 = lattice.box_of_local[m->cell_nodes[cell * nv]];
          const int64_t i = b0 % NX, j = (b0 / NX) % NY, k = b0 / (NX * NY);
          col[cell] = (uint8_t)((i & 1) + 2 * (j & 1) + 4 * (k & 1));
        }
    });
    sort_by_class(col.data(), NC, (dim == 3 ? 8 : 4) + 1, full); // (the last class, of the cells that add atomically, is empty)
  }

  bool hang_gather_lists(const uint8_t *records, int64_t nh, int nv, int kcmp, int32_t n_owned, HangGatherLists &out)
  {
    out = HangGatherLists{};
    const int32_t NO = n_owned;
    std::vector<int32_t> cnt((size_t)NO + 1, 0);
    std::vector<long long> off((size_t)nh + 1, 0);
    for (int64_t hc = 0; hc < nh; ++hc)
      {
        const uint8_t *r = records + (size_t)hc * PFM_CRES_BYTES;
        const int R = r[PFM_CRES_R];
        if (R > 16)
          return false;
        off[(size_t)hc + 1] = off[(size_t)hc] + (long long)R * R * kcmp;
        const int32_t *node = reinterpret_cast<const int32_t *>(r), *hv = reinterpret_cast<const int32_t *>(r + PFM_CRES_HV);
        for (int i = 0; i < R; ++i)
          if (node[i] >= 0 && node[i] < NO)
            ++cnt[(size_t)node[i]];
        for (int a = 0; a < nv; ++a)
          if (hv[a] >= 0 && hv[a] < NO)
            ++cnt[(size_t)hv[a]];
      }
    std::vector<int32_t> row_of((size_t)NO, -1);
    out.ptr.assign(1, 0);
    for (int32_t n = 0; n < NO; ++n)
      if (cnt[(size_t)n])
        {
          row_of[(size_t)n] = (int32_t)out.rows.size();
          out.rows.push_back(n);
          out.ptr.push_back(out.ptr.back() + cnt[(size_t)n]);
        }
    out.list.resize((size_t)out.ptr.back());
    std::vector<long long> fill(out.ptr.begin(), out.ptr.end() - 1);
    for (int64_t hc = 0; hc < nh; ++hc)
      {
        const uint8_t *r = records + (size_t)hc * PFM_CRES_BYTES;
        const int R = r[PFM_CRES_R];
        const int32_t *node = reinterpret_cast<const int32_t *>(r), *hv = reinterpret_cast<const int32_t *>(r + PFM_CRES_HV);
        for (int i = 0; i < R; ++i)
          if (node[i] >= 0 && node[i] < NO)
            out.list[(size_t)fill[(size_t)row_of[(size_t)node[i]]]++] = HgEntry{(int32_t)(hc * 32 + i), R, off[(size_t)hc] + (long long)i * R * kcmp};
        for (int a = 0; a < nv; ++a)
          if (hv[a] >= 0 && hv[a] < NO)
            out.list[(size_t)fill[(size_t)row_of[(size_t)hv[a]]]++] = HgEntry{(int32_t)(hc * 32 + 16 + a), R, 0};
      }
    out.off.swap(off);
    return true;
  }
} // namespace pfm
