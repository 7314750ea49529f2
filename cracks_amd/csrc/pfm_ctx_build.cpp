// pfm_ctx_build.cpp -- pfm_ctx_create (include/pfm_assemble.h) and the tables a context builds later, on first use.
//
// What the reference does with deal.II objects before/after the cell loop
// (cracks.cc:2133-2160, 2439-2475) becomes table look-ups prepared here once per
// setup_system() (cracks.cc:1579-1680):
//   * the sparsity pattern of make_sparsity_pattern (cracks.cc:1644-1654) is the node
//     graph of the constraint-resolved mesh (x) full component coupling; its CSR offsets
//     are arithmetic in (node-graph offset, component), so no column search is needed
//     at assembly time;
//   * cell->get_dof_indices + the Trilinos column search (cracks.cc:2439-2463) become a
//     one-byte-per-vertex-pair slot table.
// The mesh analysis itself (lattice detection, colour classes, overlay plans) is host-only code: pfm_mesh_plan.cpp.
#include "pfm_host.h"
#include "pfm_host_pool.h"
#include "pfm_mesh_plan.h"

#include <algorithm>
#include <atomic>
#include <csignal>
#include <exception>
#include <execinfo.h>
#include <fcntl.h>
#include <mutex>
#include <new>
#include <thread>
#include <unistd.h>
#include <vector>

using namespace pfm;

namespace
{
  using Lattice = pfm::LatticeHost;
  // Node graph of a lattice mesh, rows = owned nodes, columns ascending by local node id (the canonical order of the
  // ABI, what a host CSR sorted by local column id has).  Arithmetic instead of the generic cell-incidence build: the
  // neighbours of lattice node (i,j,k) are the lattice offsets that stay inside the local box (every cell of the box
  // is local, detect_lattice).  Also fills the host copies of the cartesian row tables (row_order_tables).
  void lattice_host_ptr(pfm_ctx *c, int32_t NO, const Lattice &L)
  {
    const int NX = L.NX, NY = L.NY, NZ = L.NZ;
    auto &ptr = c->h_nadj_ptr;
    ptr.resize((size_t)NO + 1);
    ptr[0] = 0;
    parallel_for(NO, [&](int64_t nb, int64_t ne) {
      for (int64_t n = nb; n < ne; ++n)
        {
          const int64_t b = L.box_of_local[n];
          const int i = (int)(b % NX), j = (int)((b / NX) % NY), k = (int)(b / ((int64_t)NX * NY));
          const int cx = 1 + (i > 0) + (i < NX - 1), cy = 1 + (j > 0) + (j < NY - 1), cz = 1 + (k > 0) + (k < NZ - 1);
          ptr[n + 1] = cx * cy * cz;
        }
    });
    inclusive_scan_parallel(ptr.data() + 1, NO);
  }
  void lattice_graph(pfm_ctx *c, int dim, int32_t NO, const Lattice &L)
  {
    (void)dim;
    // a box without ghost nodes, node n at lattice position n: the row lengths are a function of n alone -- the row pointers
    // are made on the device (launch_lattice_row_ptr) and on the host only when a pattern query asks for them
    std::atomic<bool> positional{(int64_t)NO == (int64_t)L.box_of_local.size()};
    if (positional)
      parallel_for(NO, [&](int64_t nb, int64_t ne) {
        for (int64_t n = nb; n < ne; ++n)
          if (L.box_of_local[n] != (int32_t)n)
            {
              positional = false;
              return;
            }
      });
    c->graph_positional = positional;
    c->h_nadj_ptr.clear();
    if (positional)
      {
        auto span = [](int n) { return n <= 1 ? 1LL : 3LL * n - 2; }; // sum over a line of (1 + left + right)
        c->nadj_total = span(L.NX) * span(L.NY) * span(L.NZ);
      }
    else
      lattice_host_ptr(c, NO, L);
    c->h_nadj.clear();
    c->graph_lazy = true; // rows are materialised by ensure_host_graph
  }
} // namespace

namespace pfm
{
  // the canonical rows (ascending local node id) of a lattice context whose host graph has not been materialised
  void ensure_host_graph(pfm_ctx *c)
  {
    if (c->graph_dev_only)
      {
        // general mesh: rows and row pointers were built on the device (pfm_graph.hip); the host copy is a cache for pattern queries
        (void)hipSetDevice(c->device);
        if (c->h_nadj_ptr.empty())
          {
            c->h_nadj_ptr.resize((size_t)c->v.n_owned + 1);
            if (hipMemcpy(c->h_nadj_ptr.data(), c->v.nadj_ptr, sizeof(long long) * c->h_nadj_ptr.size(), hipMemcpyDeviceToHost) != hipSuccess)
              {
                c->h_nadj_ptr.clear();
                throw HipFail{hipGetLastError(), "node graph D2H"};
              }
          }
        if (c->h_nadj.empty() && c->h_nadj_ptr.back() > 0)
          {
            c->h_nadj.resize((size_t)c->h_nadj_ptr.back());
            if (hipMemcpy(c->h_nadj.data(), c->v.nadj, sizeof(int32_t) * c->h_nadj.size(), hipMemcpyDeviceToHost) != hipSuccess)
              {
                c->h_nadj.clear();
                throw HipFail{hipGetLastError(), "node graph D2H"};
              }
          }
        return;
      }
    if (!c->graph_lazy)
      return;
    const int32_t NO = c->v.n_owned;
    const int dim = c->v.dim;
    if (c->h_nadj_ptr.empty())
      lattice_host_ptr(c, NO, c->lat);
    const auto &ptr = c->h_nadj_ptr;
    c->h_nadj.resize((size_t)ptr[NO]);
    parallel_for(NO, [&](int64_t nb, int64_t ne) {
      int32_t q[27];
      uint32_t mask;
      for (int64_t n = nb; n < ne; ++n)
        {
          const int deg = lattice_row(c->lat, dim, n, q, mask);
          int32_t *row = c->h_nadj.data() + ptr[n];
          std::copy(q, q + deg, row);
          if (!std::is_sorted(row, row + deg))
            std::sort(row, row + deg);
        }
    });
    c->graph_lazy = false;
  }

  // device copy of the node graph + slot table of the general cell kernel (lattice contexts: on first use)
  void ensure_general_tables(pfm_ctx *c)
  {
    if (c->general_ready)
      return;
    ensure_host_graph(c);
    DevView &v = c->v;
    if (c->colours_lazy)
      {
        int32_t *d_order = dev_alloc<int32_t>(c, (size_t)std::max<int64_t>(v.n_cells, 1));
        const int32_t *d_box = c->graph_positional ? nullptr : dev_upload(c, c->lat.box_of_local.data(), c->lat.box_of_local.size());
        if (launch_lattice_colour_order(d_order, v.conn, d_box, v.n_cells, c->lat.NX, c->lat.NY, nullptr) != PFM_OK)
          throw HipFail{hipGetLastError(), "colour lists"};
        v.color_cells = d_order;
        c->colours_lazy = false;
      }
    v.nadj = dev_upload(c, c->h_nadj.data(), c->h_nadj.size());
    v.cslot = dev_alloc<uint8_t>(c, (size_t)v.n_cells * (size_t)(1 << v.dim) * (size_t)(1 << v.dim));
    if (launch_build_cslot(v, nullptr) != PFM_OK || hipDeviceSynchronize() != hipSuccess)
      throw HipFail{hipGetLastError(), "cslot kernel"};
    c->general_ready = true;
  }

  // Cartesian row tables from the CURRENT order of the node-graph rows (pfm_ctx_create: ascending local id;
  // pfm_pattern_bind: the caller's order): nbr_mask[n] bit o = lattice offset o exists; the CSR slot of offset o is its
  // rank among the existing offsets when the row is in lattice order, else row_perm[nadj_ptr[n] + rank] (bit 31 of the
  // mask set).  Returns false when a row is not a lattice row (cannot happen for meshes detect_lattice accepts).
  bool row_order_tables(const pfm_ctx *c, int dim, int32_t NO, const Lattice &L, std::vector<uint32_t> &mask,
                        std::vector<uint8_t> &perm, bool &any_perm)
  {
    const int NX = L.NX, NY = L.NY, NZ = L.NZ, no = dim == 3 ? 27 : 9;
    mask.assign((size_t)NO, 0u);
    perm.clear();
    std::vector<uint8_t> flagged((size_t)NO, 0);
    std::atomic<bool> ok{true};
    parallel_for(NO, [&](int64_t nb, int64_t ne) {
      for (int64_t n = nb; n < ne; ++n)
        {
          const int64_t b = L.box_of_local[n];
          const int i = (int)(b % NX), j = (int)((b / NX) % NY), k = (int)(b / ((int64_t)NX * NY));
          const int deg = (int)(c->h_nadj_ptr[n + 1] - c->h_nadj_ptr[n]);
          int32_t canon[27];
          const int32_t *row = canon;
          if (c->graph_lazy) // canonical order = ascending local id, not materialised
            {
              uint32_t m0;
              const int dg = lattice_row(L, dim, n, canon, m0);
              if (!std::is_sorted(canon, canon + dg))
                std::sort(canon, canon + dg);
            }
          else
            row = c->h_nadj.data() + c->h_nadj_ptr[n];
          uint32_t mk = 0;
          int rank = 0;
          bool lattice_order = true;
          for (int o = 0; o < no; ++o)
            {
              const int ii = i + (o % 3) - 1, jj = j + ((o / 3) % 3) - 1, kk = k + (dim == 3 ? (o / 9) - 1 : 0);
              if (ii < 0 || ii >= NX || jj < 0 || jj >= NY || kk < 0 || kk >= NZ)
                continue;
              const int32_t q = L.local_of_box[ii + (int64_t)NX * (jj + (int64_t)NY * kk)];
              mk |= 1u << o;
              if (rank >= deg || row[rank] != q)
                lattice_order = false;
              ++rank;
            }
          if (rank != deg)
            ok = false;
          mask[n] = mk | (lattice_order ? 0u : 0x80000000u);
          flagged[n] = !lattice_order;
        }
    });
    if (!ok)
      return false;
    any_perm = false;
    for (int32_t n = 0; n < NO && !any_perm; ++n)
      any_perm = flagged[n] != 0;
    if (!any_perm)
      return true;
    perm.assign((size_t)c->h_nadj_ptr[NO], 0);
    parallel_for(NO, [&](int64_t nb, int64_t ne) {
      for (int64_t n = nb; n < ne; ++n)
        {
          if (!flagged[n])
            continue;
          const int64_t b = L.box_of_local[n];
          const int i = (int)(b % NX), j = (int)((b / NX) % NY), k = (int)(b / ((int64_t)NX * NY));
          const int deg = (int)(c->h_nadj_ptr[n + 1] - c->h_nadj_ptr[n]);
          int32_t canon[27];
          const int32_t *row = canon;
          if (c->graph_lazy)
            {
              uint32_t m0;
              const int dg = lattice_row(L, dim, n, canon, m0);
              std::sort(canon, canon + dg);
            }
          else
            row = c->h_nadj.data() + c->h_nadj_ptr[n];
          int rank = 0;
          for (int o = 0; o < no; ++o)
            {
              const int ii = i + (o % 3) - 1, jj = j + ((o / 3) % 3) - 1, kk = k + (dim == 3 ? (o / 9) - 1 : 0);
              if (ii < 0 || ii >= NX || jj < 0 || jj >= NY || kk < 0 || kk >= NZ)
                continue;
              const int32_t q = L.local_of_box[ii + (int64_t)NX * (jj + (int64_t)NY * kk)];
              const int32_t *p = std::find(row, row + deg, q);
              if (p == row + deg)
                ok = false;
              perm[(size_t)c->h_nadj_ptr[n] + rank] = (uint8_t)(p - row);
              ++rank;
            }
        }
    });
    return ok;
  }

  // upload (or replace) the device copies of the cartesian row tables
  void upload_row_tables(pfm_ctx *c, const std::vector<uint32_t> &mask, const std::vector<uint8_t> &perm, bool any_perm)
  {
    CartView &cv = c->cv;
    if (!cv.nbr_mask)
      cv.nbr_mask = dev_alloc<uint32_t>(c, mask.size());
    if (!mask.empty() && h2d(const_cast<uint32_t *>(cv.nbr_mask), mask.data(), mask.size() * sizeof(uint32_t)) != hipSuccess)
      throw HipFail{hipGetLastError(), "hipMemcpy nbr_mask"};
    if (any_perm)
      {
        if (!c->d_row_perm)
          c->d_row_perm = dev_alloc<uint8_t>(c, perm.size());
        if (h2d(c->d_row_perm, perm.data(), perm.size()) != hipSuccess)
          throw HipFail{hipGetLastError(), "hipMemcpy row_perm"};
      }
    cv.row_perm = any_perm ? c->d_row_perm : nullptr;
  }

  // The colour lists of the general family over ALL cells, for a context whose overlay made them unnecessary at pfm_ctx_create
  // (full_colours_lazy): from the device copies of the cell table and the hanging-node index, when that family is first run
  // without the overlay (pfm_ctx_force_path, a stress-split assembly of a 3-D overlay context)
  void ensure_full_colours(pfm_ctx *c)
  {
    if (!c->full_colours_lazy)
      return;
    DevView &v = c->v;
    const int64_t NC = v.n_cells;
    const int nv = 1 << v.dim;
    (void)hipSetDevice(c->device);
    pfm::raw_vector<int32_t> conn((size_t)NC * nv), hn;
    if (NC > 0 && hipMemcpy(conn.data(), v.conn, sizeof(int32_t) * conn.size(), hipMemcpyDeviceToHost) != hipSuccess)
      throw HipFail{hipGetLastError(), "cell table D2H"};
    if (v.hn_index)
      {
        hn.resize((size_t)v.n_nodes);
        if (hipMemcpy(hn.data(), v.hn_index, sizeof(int32_t) * hn.size(), hipMemcpyDeviceToHost) != hipSuccess)
          throw HipFail{hipGetLastError(), "hanging index D2H"};
      }
    pfm::raw_vector<long long> hp;
    pfm::raw_vector<int32_t> hpar;
    if (c->hanging_coloured && v.hn_index && c->n_hanging > 0)
      {
        hp.resize((size_t)c->n_hanging + 1);
        if (hipMemcpy(hp.data(), v.hn_ptr, sizeof(long long) * hp.size(), hipMemcpyDeviceToHost) != hipSuccess)
          throw HipFail{hipGetLastError(), "hanging table D2H"};
        hpar.resize((size_t)hp.back());
        if (!hpar.empty() && hipMemcpy(hpar.data(), v.hn_parents, sizeof(int32_t) * hpar.size(), hipMemcpyDeviceToHost) != hipSuccess)
          throw HipFail{hipGetLastError(), "hanging table D2H"};
      }
    static_assert(sizeof(long long) == sizeof(int64_t), "hanging row pointers");
    Colours col;
    greedy_colours(NC, nv, v.n_nodes, CellView{conn.data(), 1, NC}, v.hn_index ? hn.data() : nullptr, nullptr, nullptr, col,
                   hp.empty() ? nullptr : reinterpret_cast<const int64_t *>(hp.data()), hp.empty() ? nullptr : hpar.data());
    v.color_cells = dev_upload(c, col.order.data(), col.order.size());
    c->color_ptr.swap(col.ptr);
    if (col.overflow)
      {
        // a node of more than 62 cells: every cell adds atomically (the rule of pfm_ctx_create, which
        // tests/test_gpu_topology.py reaches with fan2d_closed64 and fan3d_41)
        std::vector<uint8_t> all((size_t)NC, 1);
        v.cell_ring = dev_upload(c, all.data(), all.size());
        c->colour_overflow = true;
      }
    c->full_colours_lazy = false;
  }
} // namespace pfm

namespace
{
  // Build the fast-path tables of a lattice mesh.  Returns false (general path) whenever a
  // check fails; never an error.
  bool build_cart(pfm_ctx *c, const pfm_mesh_desc *m, const Lattice &L)
  {
    const int NX = L.NX, NY = L.NY;
    const int32_t NO = m->n_owned_nodes;
    const auto &box_of_local = L.box_of_local;
    // owned nodes must form a sub-box
    int o0[3] = {1 << 30, 1 << 30, 1 << 30}, o1[3] = {-1, -1, -1};
    {
      std::mutex mx;
      parallel_for(NO, [&](int64_t nb, int64_t ne) {
        int l0[3] = {1 << 30, 1 << 30, 1 << 30}, l1[3] = {-1, -1, -1};
        for (int64_t n = nb; n < ne; ++n)
          {
            const int64_t b = box_of_local[n];
            const int idx[3] = {(int)(b % NX), (int)((b / NX) % NY), (int)(b / ((int64_t)NX * NY))};
            for (int d = 0; d < 3; ++d)
              {
                l0[d] = std::min(l0[d], idx[d]);
                l1[d] = std::max(l1[d], idx[d]);
              }
          }
        std::lock_guard<std::mutex> lock(mx);
        for (int d = 0; d < 3; ++d)
          {
            o0[d] = std::min(o0[d], l0[d]);
            o1[d] = std::max(o1[d], l1[d]);
          }
      });
    }
    if (NO == 0)
      return false;
    if ((int64_t)(o1[0] - o0[0] + 1) * (o1[1] - o0[1] + 1) * (o1[2] - o0[2] + 1) != NO)
      return false;
    // lexicographic numbering of the owned box?
    bool owned_lex = true;
    {
      const int64_t OWX = o1[0] - o0[0] + 1, OWY = o1[1] - o0[1] + 1;
      std::atomic<bool> lex{true};
      parallel_for(NO, [&](int64_t nb, int64_t ne) {
        for (int64_t n = nb; n < ne && lex; ++n)
          {
            const int64_t b = box_of_local[n];
            const int64_t i = b % NX, j = (b / NX) % NY, k = b / ((int64_t)NX * NY);
            if ((i - o0[0]) + OWX * ((j - o0[1]) + OWY * (k - o0[2])) != n)
              lex = false;
          }
      });
      owned_lex = lex;
    }
    // Row tables.  A box without ghost nodes, numbered lexicographically, in the canonical column order (ascending local
    // id, the lazy lattice graph): every row is in lattice order, the neighbour mask is a function of the lattice
    // position alone -- one trivial kernel instead of a threaded host pass over 27 neighbours per node and a 40 MB upload
    // (55 of the 200 ms of a context rebuild at 216^3).
    const bool positional = owned_lex && NO == m->n_nodes && c->graph_lazy;
    std::vector<uint32_t> mask;
    std::vector<uint8_t> perm;
    bool any_perm = false;
    if (!positional && !row_order_tables(c, m->dim, NO, L, mask, perm, any_perm))
      return false;
    CartView &cv = c->cv;
    cv.NX = NX;
    cv.NY = NY;
    cv.NZ = L.NZ;
    for (int d = 0; d < 3; ++d)
      {
        cv.o0[d] = o0[d];
        cv.o1[d] = o1[d];
        cv.h[d] = L.h[d];
      }
    cv.local_of_box = dev_upload(c, L.local_of_box.data(), L.local_of_box.size());
    if (positional)
      {
        if (!cv.nbr_mask)
          cv.nbr_mask = dev_alloc<uint32_t>(c, (size_t)NO);
        if (launch_lattice_masks(const_cast<uint32_t *>(cv.nbr_mask), NX, NY, L.NZ, m->dim, nullptr) != PFM_OK)
          throw HipFail{hipGetLastError(), "lattice mask kernel"};
        cv.row_perm = nullptr;
      }
    else
      upload_row_tables(c, mask, perm, any_perm);
    cv.cell_lam = cv.cell_mu = nullptr;
    if (m->cell_lambda && m->cell_mu)
      {
        // heterogeneous material: the row-owner kernels address cells by lattice position
        const int nv = 1 << m->dim;
        const int64_t CX = NX - 1, CY = NY - 1;
        std::vector<double> la((size_t)m->n_cells), mu((size_t)m->n_cells);
        parallel_for(m->n_cells, [&](int64_t cb, int64_t ce) {
          for (int64_t cell = cb; cell < ce; ++cell)
            {
              const int64_t b0 = box_of_local[m->cell_nodes[cell * nv]]; // vertex 0 = lower corner (detect_lattice)
              const int64_t i = b0 % NX, j = (b0 / NX) % NY, k = b0 / ((int64_t)NX * NY);
              const int64_t at = i + CX * (j + CY * k);
              la[at] = m->cell_lambda[cell];
              mu[at] = m->cell_mu[cell];
            }
        });
        cv.cell_lam = dev_upload(c, la.data(), la.size());
        cv.cell_mu = dev_upload(c, mu.data(), mu.size());
      }
    cv.owned_lex = owned_lex ? 1 : 0;
    cv.cell_avg = nullptr;
    if (m->dim == 2)
      cv.cell_avg = dev_alloc<double>(c, (size_t)std::max<int64_t>((int64_t)(NX - 1) * (NY - 1), 1));
    return true;
  }

  // context part: reduced colour lists, uploads (after the colour classes and the node graph exist)
  void finish_patches2d(pfm_ctx *c, const pfm_mesh_desc *m, PatchPlan &pl, const int32_t *hn_index)
  {
    DevView &v = c->v;
    const int32_t N = m->n_nodes, NO = m->n_owned_nodes;
    const int64_t NC = m->n_cells;
    if (pl.n_blocks == 0)
      return;
    std::vector<uint8_t> &regular = pl.regular;
    pfm::raw_vector<int32_t> &blk_cells = pl.blk_cells, &blk_nodes = pl.blk_nodes;
    std::vector<int32_t> &rows_general = pl.rows_general;
    const int n_blocks = pl.n_blocks;
    const int64_t n_regular = pl.n_regular;
    // a regular node has the nine nodes of its 2 x 2 cells in its row and nothing else, by construction; checked against the
    // node graph, on the host or (general mesh: the graph was built there) on the device below (a violation would mean a
    // coupling this classification does not know: no overlay then)
    if (c->h_nadj_ptr.size() == (size_t)NO + 1)
      {
        std::atomic<bool> nine{true};
        parallel_for(NO, [&](int64_t nb, int64_t ne) {
          for (int64_t n = nb; n < ne; ++n)
            if (regular[n] && c->h_nadj_ptr[n + 1] - c->h_nadj_ptr[n] != 9)
              nine = false;
        });
        if (!nine)
          return;
      }
    // reduced lists of the general family: the cells that touch a row the patches do not write
    std::vector<uint8_t> need((size_t)NC);
    parallel_for(NC, [&](int64_t cb, int64_t ce) {
      for (int64_t k = cb; k < ce; ++k)
        {
          uint8_t q = 0;
          for (int a = 0; a < 4; ++a)
            {
              const int32_t n = m->cell_nodes[4 * k + a];
              if (pl.hang[n] != 0 || (n < NO && !regular[n]))
                q = 1;
            }
          need[k] = q;
        }
    });
    // its colour classes: greedy over these cells alone (the lists over all cells are made when the general family is first
    // run without the overlay, ensure_full_colours)
    Colours red;
    greedy_colours(NC, 4, N, CellView{m->cell_nodes, 4, 1}, hn_index, need.data(), nullptr, red);
    if (red.overflow)
      return; // (a node of more than 62 such cells: no overlay, the caller colours all cells)
    c->color_ptr_reduced.swap(red.ptr);
    pfm::raw_vector<int32_t> &order_red = red.order;
    c->n_general_cells = (int64_t)c->color_ptr_reduced.back();
    v.row_patch = dev_upload(c, regular.data(), regular.size());
    if (c->graph_dev_only && c->h_nadj_ptr.empty())
      {
        int bad = 1;
        if (launch_check_row_lengths(v.row_patch, v.nadj_ptr, NO, 9, v.status, nullptr) != PFM_OK ||
            hipMemcpy(&bad, v.status, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
          throw HipFail{hipGetLastError(), "row length check"};
        if (bad)
          {
            if (hipMemset(v.status, 0, sizeof(int)) != hipSuccess)
              throw HipFail{hipGetLastError(), "hipMemset"};
            v.row_patch = nullptr;
            return;
          }
      }
    c->n_rows_general = (int32_t)rows_general.size();
    if (rows_general.empty())
      rows_general.push_back(0);
    {
      // the overlay's tables in ONE device allocation (a hipMalloc costs 0.05-0.1 ms; the build made five of them here)
      auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
      const size_t b_cells = al(sizeof(int32_t) * blk_cells.size()), b_nodes = al(sizeof(int32_t) * blk_nodes.size());
      const size_t b_slots = al(sizeof(unsigned long long) * (size_t)std::max<int32_t>(NO, 1));
      const size_t b_order = al(sizeof(int32_t) * order_red.size()), b_rows = al(sizeof(int32_t) * rows_general.size());
      char *slab = dev_alloc<char>(c, b_cells + b_nodes + b_slots + b_order + b_rows);
      auto put = [&](char *d, const void *h, size_t bytes) {
        const hipError_t e = h2d(d, h, bytes);
        if (e != hipSuccess)
          throw HipFail{e, "hipMemcpy H2D"};
      };
      char *at = slab;
      put(at, blk_cells.data(), sizeof(int32_t) * blk_cells.size());
      v.patch_cells = reinterpret_cast<const int32_t *>(at);
      at += b_cells;
      put(at, blk_nodes.data(), sizeof(int32_t) * blk_nodes.size());
      v.patch_nodes = reinterpret_cast<const int32_t *>(at);
      at += b_nodes;
      c->d_node_slots = reinterpret_cast<unsigned long long *>(at);
      v.node_slots = c->d_node_slots;
      at += b_slots;
      put(at, order_red.data(), sizeof(int32_t) * order_red.size());
      c->d_color_cells_reduced = reinterpret_cast<int32_t *>(at);
      at += b_order;
      put(at, rows_general.data(), sizeof(int32_t) * rows_general.size());
      c->d_rows_general = reinterpret_cast<int32_t *>(at);
    }
    c->n_patch_blocks = n_blocks;
    c->n_patch_rows = n_regular;
    c->patch_slots_valid = false;
  }

  // context part: reduced colour lists of the general family, uploads of the level lattices
  void finish_patches3d(pfm_ctx *c, const pfm_mesh_desc *m, PatchPlan3 &pl, const int32_t *hn_index)
  {
    DevView &v = c->v;
    const int32_t NO = m->n_owned_nodes;
    const int64_t NC = m->n_cells;
    if (pl.levels.empty())
      return;
    std::vector<uint8_t> need((size_t)NC);
    parallel_for(NC, [&](int64_t cb, int64_t ce) {
      for (int64_t k = cb; k < ce; ++k)
        {
          uint8_t q = 0;
          for (int a = 0; a < 8; ++a)
            {
              const int32_t n = m->cell_nodes[8 * k + a];
              if (pl.hang[n] || (n < NO && !pl.regular[n]))
                q = 1;
            }
          need[k] = q;
        }
    });
    Colours red; // (see finish_patches2d)
    greedy_colours(NC, 8, m->n_nodes, CellView{m->cell_nodes, 8, 1}, hn_index, need.data(), nullptr, red,
                   c->hanging_coloured ? m->hn_ptr : nullptr, c->hanging_coloured ? m->hn_parents : nullptr);
    if (red.overflow)
      return;
    c->color_ptr_reduced.swap(red.ptr);
    pfm::raw_vector<int32_t> &order_red = red.order;
    c->n_general_cells = (int64_t)c->color_ptr_reduced.back();
    v.row_patch = dev_upload(c, pl.regular.data(), pl.regular.size());
    c->d_color_cells_reduced = dev_upload(c, order_red.data(), order_red.size());
    c->n_rows_general = (int32_t)pl.rows_general.size();
    if (pl.rows_general.empty())
      pl.rows_general.push_back(0);
    c->d_rows_general = dev_upload(c, pl.rows_general.data(), pl.rows_general.size());
    c->n_patch_rows = pl.n_regular;
    for (Level3 &lev : pl.levels)
      {
        pfm_ctx::OverlayLevel ol;
        CartView &cv = ol.cv;
        cv.NX = lev.dims[0];
        cv.NY = lev.dims[1];
        cv.NZ = lev.dims[2];
        for (int d = 0; d < 3; ++d)
          {
            cv.o0[d] = 0; // every node of the level lattice may own a row (CartView::row_of_box says which do)
            cv.o1[d] = lev.dims[d] - 1;
            cv.h[d] = lev.h[d];
          }
        cv.local_of_box = dev_upload(c, lev.node_at.data(), lev.node_at.size());
        cv.row_of_box = dev_upload(c, lev.row_at.data(), lev.row_at.size());
        cv.owned_lex = 0;
        cv.cell_lam = cv.cell_mu = nullptr;
        if (!lev.lam.empty())
          {
            cv.cell_lam = dev_upload(c, lev.lam.data(), lev.lam.size());
            cv.cell_mu = dev_upload(c, lev.mu.data(), lev.mu.size());
          }
        ol.d_scal = dev_alloc<unsigned char>(c, PFM_SCAL_BYTES);
        ol.n_rows = lev.n_rows;
        c->levels3.push_back(ol);
      }
    c->overlay3_rows_valid = false;
  }

  // PFM_ABORT_TRACE=<file>: a backtrace of the aborting thread into that file (debugging aid: a test runner that captures
  // stderr hides what libstdc++ or the HIP runtime say before they abort)
  void abort_trace_handler(int)
  {
    const char *path = switches().abort_trace; // (read before the handler was installed)
    const int fd = path ? open(path, O_WRONLY | O_CREAT | O_APPEND, 0644) : 2;
    void *frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, fd >= 0 ? fd : 2);
    signal(SIGABRT, SIG_DFL);
    raise(SIGABRT);
  }
  void install_abort_trace()
  {
    static std::once_flag once;
    std::call_once(once, [] {
      if (switches().abort_trace)
        {
          signal(SIGABRT, abort_trace_handler);
          signal(SIGSEGV, abort_trace_handler);
        }
    });
  }
} // namespace

extern "C"
{
  int pfm_ctx_create(pfm_ctx **out, const pfm_mesh_desc *m, int device)
  {
    install_abort_trace();
    PhaseClock clk;
    H2dBatch batch; // uploads are ordered on the null stream; the build ends with a device synchronisation
    if (!out || !m || (m->dim != 2 && m->dim != 3) ||
        (m->layout != PFM_LAYOUT_INTERLEAVED && m->layout != PFM_LAYOUT_BLOCKED) ||
        m->n_nodes <= 0 || m->n_owned_nodes < 0 || m->n_owned_nodes > m->n_nodes || m->n_cells < 0 ||
        !m->cell_nodes || !m->coords || (m->n_hanging > 0 && (!m->hn_nodes || !m->hn_ptr)))
      return PFM_ERR_BAD_ARG;
    pfm_ctx *c = new (std::nothrow) pfm_ctx;
    if (!c)
      return PFM_ERR_NOMEM;
    *out = c;
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess)
      return hipfail(c, e, "hipSetDevice");

    const int dim = m->dim, nv = 1 << dim;
    const int32_t N = m->n_nodes, NO = m->n_owned_nodes;
    const int64_t NC = m->n_cells;
    DevView &v = c->v;
    v.dim = dim;
    v.layout = m->layout;
    v.n_nodes = N;
    v.n_owned = NO;
    v.n_cells = NC;
    c->n_blocks = (m->layout == PFM_LAYOUT_BLOCKED) ? 4 : 1;

    {
      std::atomic<bool> in_range{true};
      parallel_for(NC * nv, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i)
          if (m->cell_nodes[i] < 0 || m->cell_nodes[i] >= N)
            {
              in_range = false;
              return;
            }
      });
      if (!in_range)
        return fail(c, PFM_ERR_BAD_ARG, "cell_nodes out of range");
    }

    clk.mark("argument checks");
    Lattice &lattice = c->lat;
    bool lattice_ok = false;
    // The cell table and the coordinates go to the device as the host handed them over (cell-major / node-major) and are
    // transposed to SoA by a kernel (a host transposition of 8e7 + 3e7 entries cost 0.25 s at 1e7 cells).  Large meshes: on
    // a second thread, next to the host passes below that read the same tables (lattice detection: 20 ms at 1e7 cells).
    struct MeshUpload
    {
      int32_t *raw = nullptr, *conn = nullptr;
      double *rawx = nullptr, *xs = nullptr;
      int rct = PFM_OK, rcx = PFM_OK;
      hipError_t err = hipSuccess;
      const char *what = "";
    } up;
    auto upload_mesh = [&]() {
      H2dBatch in_batch;
      auto bad = [&](hipError_t e, const char *what) {
        up.err = e;
        up.what = what;
      };
      if (hipSetDevice(device) != hipSuccess)
        return bad(hipGetLastError(), "hipSetDevice");
      const size_t cb = sizeof(int32_t) * std::max<size_t>((size_t)NC * nv, 1), xb = sizeof(double) * (size_t)N * dim;
      if (scratch_acquire((void **)&up.raw, cb) != hipSuccess || hipMalloc((void **)&up.conn, cb) != hipSuccess ||
          scratch_acquire((void **)&up.rawx, xb) != hipSuccess || hipMalloc((void **)&up.xs, xb) != hipSuccess)
        return bad(hipGetLastError(), "hipMalloc");
      hipError_t e2 = NC > 0 ? h2d(up.raw, m->cell_nodes, sizeof(int32_t) * (size_t)NC * nv) : hipSuccess;
      if (e2 != hipSuccess)
        return bad(e2, "hipMemcpy H2D");
      up.rct = launch_aos_to_soa_i32(up.raw, up.conn, NC, nv, nullptr);
      e2 = h2d(up.rawx, m->coords, xb);
      if (e2 != hipSuccess)
        return bad(e2, "hipMemcpy H2D");
      up.rcx = launch_aos_to_soa_f64(up.rawx, up.xs, N, dim, nullptr);
    };
    std::thread upload_thread;
    struct UploadJoiner // an early return or an exception must not leave the thread running, nor its buffers behind
    {
      std::thread &t;
      MeshUpload &u;
      bool taken = false;
      ~UploadJoiner()
      {
        if (t.joinable())
          t.join();
        if (!taken)
          {
            scratch_release(u.raw);
            scratch_release(u.rawx);
            for (void *q : {(void *)u.conn, (void *)u.xs})
              if (q)
                (void)hipFree(q);
          }
      }
    } upload_joiner{upload_thread, up};
    try
      {
        // constraint bytes, the nodal state and the status word: one allocation, one clear (a hipMalloc costs 0.1-3 ms)
        {
          const size_t sb = ((size_t)N * sizeof(double) + 255) & ~(size_t)255, fb = ((size_t)N + 255) & ~(size_t)255;
          const size_t total = fb + (size_t)(dim + 3) * sb + 256;
          char *slab = dev_alloc<char>(c, total);
          e = hipMemsetAsync(slab, 0, total, nullptr);
          if (e != hipSuccess)
            throw HipFail{e, "hipMemset"};
          v.node_flags = reinterpret_cast<uint8_t *>(slab);
          char *at = slab + fb;
          auto take = [&]() {
            double *q = reinterpret_cast<double *>(at);
            at += sb;
            return q;
          };
          for (int d = 0; d < 3; ++d)
            v.u[d] = (d < dim) ? take() : nullptr;
          v.phi = take();
          v.phi_old = take();
          v.phi_oldold = take();
          v.status = reinterpret_cast<int *>(at);
        }
        clk.mark("state buffers");
        if (NC > (1 << 20))
          upload_thread = std::thread(upload_mesh);
        // ---- hanging table: node -> k
        std::vector<int32_t> hn_index;
        if (const char *bad = hanging_index(m, hn_index))
          return fail(c, PFM_ERR_BAD_ARG, bad);

        // ---- node graph over the constraint-resolved cells, rows = owned nodes, columns ascending by local node id
        // (ghost nodes, numbered after the owned ones, come last: the order of a host CSR sorted by local column id).
        bool device_graph = false;
        lattice_ok = detect_lattice(m, lattice);
        clk.mark("detect_lattice");
        if (lattice_ok)
          lattice_graph(c, dim, NO, lattice);
        else
          device_graph = true; // general mesh: built on the device below, from the uploaded cell table (pfm_graph.hip)
        std::vector<int32_t> &nadj = c->h_nadj;
        clk.mark("node graph");

        // Colour classes of the general family (greedy_colours) only read host tables: on a general mesh they are computed by a
        // host thread NEXT TO the uploads and the device build of the node graph -- and given up as soon as the overlay plan
        // (below, on a thread of its own) turns out non-empty: the overlay needs the classes of the few cells it leaves to
        // the general family only (finish_patches2d / 3d), the lists over all cells are then made on first use.
        const int32_t *hn_idx = hn_index.empty() ? nullptr : hn_index.data();
        const CellView node_of{m->cell_nodes, nv, 1};
        // PFM_HANGING_COLOURED=1 (read at every pfm_ctx_create): the 3-D cells at hanging vertices in plain colour classes
        // (greedy_colours) instead of the one class with FP64 atomics -- every assembly of such a mesh is then bitwise
        // reproducible; it costs some thirty small launches per assembly (1.1e6-cell overlay mesh: Jacobian 4.45 -> 5.1 ms,
        // residual only 0.6 -> 1.3 ms), so the default keeps the atomic class.  Needs the records of DevView::cres, i.e.
        // hanging nodes with at most four parents.
        bool hanging_coloured = dim == 3 && hn_idx && !lattice_ok && Switches::hanging_coloured();
        for (int32_t k = 0; k < m->n_hanging && hanging_coloured; ++k)
          hanging_coloured = m->hn_ptr[k + 1] - m->hn_ptr[k] <= 4;
        c->hanging_coloured = hanging_coloured;
        c->n_hanging = m->n_hanging;
        const int64_t *col_hn_ptr = hanging_coloured ? m->hn_ptr : nullptr;
        const int32_t *col_hn_parents = hanging_coloured ? m->hn_parents : nullptr;
        Colours full;
        std::atomic<bool> colour_cancel{false};
        std::exception_ptr colour_err;
        auto colour_classes = [&]() {
          try
            {
              if (lattice_ok) // (2-D boxes; a 3-D box sorts its lists on the device when asked, below)
                lattice_colours(m, lattice, full);
              else
                greedy_colours(NC, nv, N, node_of, hn_idx, nullptr, &colour_cancel, full, col_hn_ptr, col_hn_parents);
            }
          catch (...)
            {
              colour_err = std::current_exception();
            }
        };
        std::thread colour_thread;
        if (!lattice_ok && NC > 65536)
          colour_thread = std::thread(colour_classes);
        // cartesian overlay of a 2-D mesh: the host classification (8 ms at 2.7e5 cells) on its own thread as well
        PatchPlan patch_plan;
        PatchPlan3 patch_plan3;
        std::exception_ptr patch_err;
        auto plan_patches = [&]() {
          try
            {
              if (dim == 2)
                patch_plan = plan_patches2d(m, hn_index);
              else if (!lattice_ok) // (a uniform 3-D box takes the cartesian family as a whole; no stress split in 3-D)
                patch_plan3 = plan_patches3d(m, hn_index);
            }
          catch (...)
            {
              patch_err = std::current_exception();
            }
        };
        std::thread patch_thread;
        if (NC > 65536)
          patch_thread = std::thread(plan_patches);
        struct Joiner
        {
          std::thread &t;
          ~Joiner()
          {
            if (t.joinable())
              t.join();
          }
        } colour_joiner{colour_thread}, patch_joiner{patch_thread}; // an exception on the way must not leave a running thread behind

        // ---- device mirrors (SoA)
        {
          if (upload_thread.joinable())
            upload_thread.join();
          else
            upload_mesh();
          upload_joiner.taken = true;
          clk.mark("  conn + coords h2d");
          int32_t *raw = up.raw, *conn = up.conn;
          double *rawx = up.rawx, *xs = up.xs;
          for (void *q : {(void *)conn, (void *)xs})
            if (q)
              c->allocs.push_back(q);
          c->device_bytes += (int64_t)(sizeof(int32_t) * (size_t)NC * nv + sizeof(double) * (size_t)N * dim);
          if (up.err != hipSuccess)
            {
              scratch_release(raw);
              scratch_release(rawx);
              throw HipFail{up.err, up.what};
            }
          const int rct = up.rct, rcx = up.rcx;
          int rcg = PFM_OK;
          v.hn_index = nullptr;
          v.hn_ptr = nullptr;
          v.hn_parents = nullptr;
          v.hn_weights = nullptr;
          try
            {
              if (m->n_hanging > 0)
                {
                  v.hn_index = dev_upload(c, hn_index.data(), hn_index.size());
                  std::vector<long long> hp(m->hn_ptr, m->hn_ptr + m->n_hanging + 1);
                  v.hn_ptr = dev_upload(c, hp.data(), hp.size());
                  v.hn_parents = dev_upload(c, m->hn_parents, (size_t)hp.back());
                  v.hn_weights = dev_upload(c, m->hn_weights, (size_t)hp.back());
                }
              clk.mark("  hanging tables");
              if (device_graph && rct == PFM_OK)
                {
                  // node graph of a general mesh on the device, from the cell table as the host handed it over
                  long long *d_ptr = dev_alloc<long long>(c, (size_t)NO + 1);
                  struct ScratchGuard // the incidence lists are freed on every way out, a throwing dev_alloc included
                  {
                    GraphScratch sc;
                    ~ScratchGuard() { graph_build_free(sc); }
                  } g;
                  long long total = 0;
                  rcg = graph_build_begin(raw, NC, nv, NO, v.hn_index, v.hn_ptr, v.hn_parents, d_ptr, g.sc, total, nullptr);
                  clk.mark("  graph rows counted");
                  if (rcg == PFM_OK)
                    {
                      int32_t *d_adj = dev_alloc<int32_t>(c, (size_t)std::max<long long>(total, 1));
                      rcg = graph_build_rows(raw, NC, nv, NO, v.hn_index, v.hn_ptr, v.hn_parents, d_ptr, d_adj, g.sc, nullptr);
                      clk.mark("  graph rows filled");
                      if (rcg == PFM_OK)
                        {
                          v.nadj_ptr = d_ptr;
                          v.nadj = d_adj;
                          c->nadj_total = total;
                          c->graph_dev_only = true; // the host copy of rows and row pointers is fetched when a pattern query asks for it
                        }
                    }
                }
            }
          catch (...)
            {
              scratch_release(raw);
              scratch_release(rawx);
              throw;
            }
          clk.mark("  row pointers to the host");
          const hipError_t es = hipDeviceSynchronize();
          clk.mark("  device synchronize");
          scratch_release(raw);
          scratch_release(rawx);
          if (rcg == PFM_ERR_UNSUPPORTED)
            return fail(c, PFM_ERR_UNSUPPORTED, "node with more than 254 neighbours");
          if (rct != PFM_OK || rcx != PFM_OK || rcg != PFM_OK || es != hipSuccess)
            throw HipFail{hipGetLastError(), "mesh table upload / node graph"};
          v.conn = conn;
          v.coords = xs;
        }
        clk.mark("conn + coords upload");
        if (patch_thread.joinable())
          patch_thread.join();
        else
          plan_patches();
        if (patch_err)
          std::rethrow_exception(patch_err);
        clk.mark("overlay plan (wait)");
        std::vector<uint8_t> ring;
        const bool any_ring = !lattice_ok && ring_cells(NC, nv, N, node_of, hn_idx, m->hn_ptr, m->hn_parents, ring, hanging_coloured);
        v.cell_ring = any_ring ? dev_upload(c, ring.data(), ring.size()) : nullptr;
        v.color_cells = nullptr;
        v.hcell = nullptr;
        v.cslot_h = nullptr;
        v.cres = nullptr;
        if (hn_idx && !lattice_ok)
          {
            // slot table of the cells at hanging vertices (DevView::cslot_h), filled next to cslot by launch_build_cslot
            const int MPH = dim == 3 ? 4 : 2;
            std::vector<int32_t> hcells;
            pfm::raw_vector<int32_t> hcell;
            if (hanging_cells(m, hn_idx, MPH, hcells, hcell))
              {
                v.hcell = dev_upload(c, hcell.data(), hcell.size());
                v.cslot_h = dev_alloc<uint8_t>(c, hcells.size() * (size_t)(nv * MPH * nv * MPH));
                // records of the reduced scatter (k_build_cres), in 2-D for PFM_HANGING_MODE_GATHER alone
                v.cres = dev_alloc<uint8_t>(c, hcells.size() * (size_t)pfm::PFM_CRES_BYTES);
                c->n_hcells = (int64_t)hcells.size();
                // round 6 default in 3-D: scratch + ordered gather instead of FP64 atomics (ensure_hang_gather, on first use);
                // PFM_HANGING_ATOMIC=1 keeps the atomic class, PFM_HANGING_COLOURED=1 the colour classes of round 5
                c->hang_gather = dim == 3 && !hanging_coloured && !Switches::hanging_atomic();
              }
            else if (dim == 2 && hanging_cells(m, hn_idx, 0x7fffffff, hcells, hcell))
              {
                // a node with more parents than the slot table holds (the atomic class searches its rows, find_slot): the
                // records take any number of parents as long as a quad resolves to 16 nodes at most
                v.hcell = dev_upload(c, hcell.data(), hcell.size());
                v.cres = dev_alloc<uint8_t>(c, hcells.size() * (size_t)pfm::PFM_CRES_BYTES);
                c->n_hcells = (int64_t)hcells.size();
              }
          }
        clk.mark("ring cells");
        finish_patches2d(c, m, patch_plan, hn_idx);
        finish_patches3d(c, m, patch_plan3, hn_idx);
        const bool overlay = c->n_patch_blocks > 0 || !c->levels3.empty();
        clk.mark("cartesian overlay");
        if (lattice_ok && dim == 3)
          {
            // uniform 3-D box: the cartesian family runs it; the lists of the general family (eight parity classes, their sizes
            // known from the box) are sorted on the device when that family is first asked for (ensure_general_tables)
            c->color_ptr.assign(10, 0);
            for (int k = 0; k < 8; ++k)
              {
                auto half = [](int n, int odd) { return (long long)(odd ? n / 2 : (n + 1) / 2); };
                c->color_ptr[(size_t)k + 1] = c->color_ptr[k] + half(lattice.nc[0], k & 1) * half(lattice.nc[1], (k >> 1) & 1) * half(lattice.nc[2], (k >> 2) & 1);
              }
            c->color_ptr[9] = c->color_ptr[8];
            c->colours_lazy = true;
          }
        else if (overlay)
          {
            colour_cancel = true; // (the thread, if it runs, stops at its next look)
            if (colour_thread.joinable())
              colour_thread.join();
            c->full_colours_lazy = true;
          }
        else
          {
            if (colour_thread.joinable())
              colour_thread.join();
            else
              colour_classes();
            if (colour_err)
              std::rethrow_exception(colour_err);
            v.color_cells = dev_upload(c, full.order.data(), full.order.size());
            c->color_ptr.swap(full.ptr);
            if (full.overflow)
              {
                // a node of more than 62 cells (tests/test_gpu_topology.py: fan2d_closed64, fan3d_41): every cell adds atomically
                ring.assign((size_t)NC, 1);
                v.cell_ring = dev_upload(c, ring.data(), ring.size());
                c->colour_overflow = true;
              }
          }
        clk.mark("colour classes");
        v.cell_lambda = v.cell_mu = nullptr;
        if (m->cell_lambda && m->cell_mu)
          {
            v.cell_lambda = dev_upload(c, m->cell_lambda, (size_t)NC);
            v.cell_mu = dev_upload(c, m->cell_mu, (size_t)NC);
          }
        if (c->graph_positional)
          {
            long long *d_ptr = dev_alloc<long long>(c, (size_t)NO + 1);
            if (launch_lattice_row_ptr(d_ptr, lattice.NX, lattice.NY, lattice.NZ, nullptr) != PFM_OK)
              throw HipFail{hipGetLastError(), "lattice row pointers"};
            v.nadj_ptr = d_ptr;
          }
        else if (!c->graph_dev_only)
          v.nadj_ptr = dev_upload(c, c->h_nadj_ptr.data(), c->h_nadj_ptr.size());
        // node graph columns + slot table of the general kernel family (position of vertex b's node in the row of
        // vertex a's node, searched on the device: 64 row searches per hex, 8 s on one host core at 1e7 cells); a
        // lattice context builds them when the general family is first used
        if (!c->graph_dev_only)
          v.nadj = nullptr;
        v.cslot = nullptr;
        c->general_ready = !c->graph_lazy;
        if (c->general_ready)
          {
            if (!c->graph_dev_only)
              v.nadj = dev_upload(c, nadj.data(), nadj.size());
            clk.mark("graph upload");
            v.cslot = dev_alloc<uint8_t>(c, (size_t)NC * nv * nv);
            if (launch_build_cslot(v, nullptr) != PFM_OK)
              throw HipFail{hipGetLastError(), "cslot kernel"};
          }
      }
    catch (const HipFail &f)
      {
        return hipfail(c, f.e, f.what);
      }
    catch (const std::bad_alloc &)
      {
        return fail(c, PFM_ERR_NOMEM, "host allocation failed");
      }
    try
      {
        clk.mark("cslot launch, state buffers");
        c->cart_ok = lattice_ok && build_cart(c, m, lattice);
        clk.mark("build_cart");
        if (!c->cart_ok)
          {
            ensure_general_tables(c); // needs the lattice tables when the graph is still lazy
            c->lat = Lattice{};       // the host lattice tables are only kept on the cartesian path
          }
        if (hipDeviceSynchronize() != hipSuccess)
          throw HipFail{hipGetLastError(), "context build"};
        c->d_scal = dev_alloc<unsigned char>(c, PFM_SCAL_BYTES);
        clk.mark("device synchronize");
      }
    catch (const HipFail &f)
      {
        return hipfail(c, f.e, f.what);
      }
    c->kernel_path = c->cart_ok ? 1 : ((c->n_patch_blocks > 0 || !c->levels3.empty()) ? 3 : 0); // 3: general family + cartesian overlay
    return PFM_OK;
  }
}
