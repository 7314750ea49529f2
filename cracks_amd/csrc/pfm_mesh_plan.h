// pfm_mesh_plan.h -- the mesh analysis of the context build (pfm_mesh_plan.cpp): lattice detection, the colour classes and
// the atomic ring of the general kernel family, the two cartesian-overlay classifiers.  It reads the caller's mesh
// description and nothing of a context, makes no HIP call and includes no HIP header, so it also builds and runs as a plain
// host program (tests/cpp/mesh_plan_main.cpp).
#pragma once
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/pfm_assemble.h"
#include "pfm_switches.h"

namespace pfm
{
  // std::vector whose resize(n) / vector(n) leaves trivially constructible elements uninitialised: tables of 1e7 entries that
  // are written once by the host threads are not cleared (and their pages not touched) by one thread first
  template <class T>
  struct default_init_allocator : std::allocator<T>
  {
    template <class U>
    struct rebind
    {
      using other = default_init_allocator<U>;
    };
    using std::allocator<T>::allocator;
    template <class U>
    void construct(U *p) noexcept(std::is_nothrow_default_constructible<U>::value)
    {
      ::new (static_cast<void *>(p)) U;
    }
    template <class U, class... A>
    void construct(U *p, A &&...a)
    {
      ::new (static_cast<void *>(p)) U(std::forward<A>(a)...);
    }
  };
  template <class T>
  using raw_vector = std::vector<T, default_init_allocator<T>>;

  // host copy of the lattice tables of a uniform box (kept for pfm_pattern_bind)
  struct LatticeHost
  {
    int NX = 0, NY = 0, NZ = 0, nc[3] = {0, 0, 0};
    double h[3] = {1, 1, 1};
    raw_vector<int32_t> local_of_box, box_of_local;
  };

  // Lattice of a uniform Cartesian box: node n <-> lattice index box_of_local[n] (x fastest), cells in deal.II
  // vertex order, every lattice cell present exactly once.  false whenever any check fails.
  bool detect_lattice(const pfm_mesh_desc *m, LatticeHost &L);
  // neighbours of owned lattice node n in lattice-offset order; returns their number, mask bit o = offset o exists
  int lattice_row(const LatticeHost &L, int dim, int64_t n, int32_t (&q)[27], uint32_t &mask);

  // the caller's cell table (cell-major) or the structure-of-arrays copy of the device: node a of a cell
  struct CellView
  {
    const int32_t *nodes;
    int64_t cell_stride, vertex_stride;
    int32_t operator()(int64_t cell, int a) const { return nodes[cell * cell_stride + a * vertex_stride]; }
  };

  // Colour classes of the general cell kernel: cells of one class share no node and are assembled by one launch with plain
  // read-modify-write (device-scope FP64 atomics run at ~3e10 /s on this chip: the scatter of a 2-D Jacobian took 1.1 of
  // 1.2 ms).  Greedy in cell order over the cells with subset[cell] != 0 (null: all cells); cells with a hanging vertex go to
  // the last class, which keeps the atomics.  order: the cells by class, ascending within a class; ptr [n_col + 2].
  struct Colours
  {
    std::vector<long long> ptr;
    pfm::raw_vector<int32_t> order;
    bool overflow = false;  // more than 62 classes were needed: such cells sit in the atomic class although no vertex hangs
    bool cancelled = false; // the caller lost interest (cancel): ptr and order are not filled
  };
  // the distinct constraint-resolved nodes of a cell (a vertex that does not hang is its own, a hanging one brings its
  // parents); returns their number, or max_nodes + 1 when there are more
  int resolved_nodes(int64_t cell, int nv, CellView node_of, const int32_t *hn_index, const int64_t *hn_ptr, const int32_t *hn_parents, int32_t *out,
                     int max_nodes);

  // hn_ptr / hn_parents != nullptr (3-D, round 5): a cell at a hanging vertex is coloured like any other, over its
  // constraint-resolved nodes -- the cell kernel reduces its element matrix and residual to those nodes before it adds
  // (K' = C^T K C, DevView::cres), so cells of one class that share no resolved node write disjoint entries and need no
  // atomics: every class adds in a fixed order and the assembly is bitwise reproducible.  Only a cell with more than 16
  // resolved nodes (or one that finds no colour) stays in the last class.
  void greedy_colours(int64_t NC, int nv, int32_t N, CellView node_of, const int32_t *hn_index, const uint8_t *subset, const std::atomic<bool> *cancel,
                      Colours &out, const int64_t *hn_ptr = nullptr, const int32_t *hn_parents = nullptr);

  // Cells of the plain classes that share a constraint-resolved node with a cell at a hanging vertex add atomically as well
  // (DevView::cell_ring): every row the atomic class touches then only ever receives atomic adds, and the class -- 68
  // latency-bound waves, 15 % of a Jacobian at 2.7e5 cells -- runs next to the others.  false: no such cell (ring empty).
  bool ring_cells(int64_t NC, int nv, int32_t N, CellView node_of, const int32_t *hn_index, const int64_t *hn_ptr, const int32_t *hn_parents,
                  std::vector<uint8_t> &ring, bool hanging_coloured = false);

  // the parity classes of a lattice mesh (the cell's lattice position), in the form of greedy_colours
  void lattice_colours(const pfm_mesh_desc *m, const LatticeHost &lattice, Colours &out);
  // hanging table: hn_index[node] = its line k, or -1 (empty when no node hangs); returns what is wrong with the table, or null
  const char *hanging_index(const pfm_mesh_desc *m, std::vector<int32_t> &hn_index);
  // The cells at hanging vertices (hcells, ascending) and each cell's place among them (hcell, -1: none), for the slot table
  // DevView::cslot_h.  false -- nothing filled -- when a node hangs on more than max_parents parents or no cell is at one.
  bool hanging_cells(const pfm_mesh_desc *m, const int32_t *hn_index, int max_parents, std::vector<int32_t> &hcells, raw_vector<int32_t> &hcell);

  // ---- ordered gather of the cells at hanging vertices (DevView::cres, DevView::hs_*, k_hanging_gather) --------------------
  // record of one such cell, built on the device (k_build_cres): int32 node[16], uint8 slot[16][16], uint8 R, int32 hv[8], int32 cell
  constexpr int PFM_CRES_SLOT = 64, PFM_CRES_R = 320, PFM_CRES_HV = 336, PFM_CRES_CELL = 368, PFM_CRES_BYTES = 376;
  struct HgEntry // one contribution to a row of the gather tables (pfm_ctx::d_hg_list)
  {
    int32_t code; // hc * 32 + index: index < 16 = resolved node i of cell hc, 16 + a = the row of the cell's hanging vertex a
    int32_t R;    // resolved nodes of the cell
    long long koff; // first double of row i of the cell's K' in DevView::hs_K
  };
  // The lists the gather runs over, from nh records: every (cell, owned resolved node) and (cell, owned hanging vertex) pair
  // under its destination row -- rows ascending, the entries of a row in ascending (cell, index) order, the order the adds take
  // -- and off[hc], the first double of cell hc's K' (R x R x kcmp each; kcmp = 7 for quads, nv = 4, and 13 for hexes, nv = 8).
  // Nodes >= n_owned (ghosts) are never listed.  false -- `out` is left empty -- when a record has more than 16 resolved nodes.
  struct HangGatherLists
  {
    std::vector<int32_t> rows;
    std::vector<long long> ptr, off;
    std::vector<HgEntry> list;
  };
  bool hang_gather_lists(const uint8_t *records, int64_t nh, int nv, int kcmp, int32_t n_owned, HangGatherLists &out);

  // ---- cartesian overlay of a general 2-D mesh (DevView::row_patch ..., pfm_kernels.hip: PATCH) -------------------------
  // Every cell that is an axis-parallel rectangle belongs to the lattice of its size (a refinement level); a node is REGULAR
  // when it is owned, neither hanging nor a parent, has exactly four incident cells, all of one level, and none of the nine
  // lattice nodes around it is hanging -- its row is then the plain 9-point row of that level, completed by one workgroup
  // of the patch kernel.  Blocks of 8 x 8 cells (7 x 7 nodes owned per block) tile each level; the general family keeps
  // the cells that touch any other row (reduced colour lists), and skips the regular rows.
  // host-only part (no context access: it runs on its own thread next to the uploads and the node graph build)
  struct PatchPlan
  {
    std::vector<uint8_t> regular, hang; // per node: row of the patch kernel; hanging or duplicated position
    pfm::raw_vector<int32_t> blk_cells, blk_nodes;
    std::vector<int32_t> rows_general;
    int64_t n_regular = 0;
    int n_blocks = 0;
  };
  PatchPlan plan_patches2d(const pfm_mesh_desc *m, const std::vector<int32_t> &hn_index);

  // ---- cartesian overlay of a general 3-D mesh (round 5) -------------------------------------------------------------------
  // The same classification as in 2-D (plan_patches2d), with the row-owner kernels of the CARTESIAN family as the "patch
  // kernel": every cell that is an exact axis-parallel box belongs to the lattice of its size (a refinement level); a node
  // is REGULAR when it is owned, neither hanging nor a parent, has exactly eight incident cells, all of one level and at
  // the eight lattice positions around it, and none of the 27 lattice nodes around it is hanging -- its rows are then the
  // plain 27-point rows of a uniform box of that level.  Per level one lattice (CartView) over the bounding box of its
  // regular nodes plus a one-node halo: node_at = the node at each lattice point (-1: none of this level), row_at = the
  // regular nodes.  k_cart_uu3 / k_cart_phi4 / k_cart_residual3 run on it as on a box and write exactly the rows of row_at;
  // cells that do not exist at a lattice position contribute only to rows that are not regular, i.e. to nothing that is
  // written.  The general family keeps the cells that touch any other row (reduced colour lists) and skips the regular rows.
  struct Level3
  {
    double h[3] = {0, 0, 0};
    long long lo[3] = {0, 0, 0}; // lattice position of the box's first node
    int dims[3] = {0, 0, 0};     // nodes of the box
    std::vector<int32_t> node_at, row_at;
    std::vector<double> lam, mu; // per lattice cell (heterogeneous material), else empty
    int64_t n_rows = 0;
  };
  struct PatchPlan3
  {
    std::vector<uint8_t> regular, hang;
    std::vector<int32_t> rows_general;
    std::vector<Level3> levels;
    int64_t n_regular = 0;
  };
  PatchPlan3 plan_patches3d(const pfm_mesh_desc *m, const std::vector<int32_t> &hn_index);

  // PFM_CTX_TIMING=1: wall time of the phases of pfm_ctx_create on stderr (tuning only); fmt takes the phase and its milliseconds
  struct PhaseClock
  {
    const char *const fmt;
    const bool on = Switches::ctx_timing();
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit PhaseClock(const char *format = "[pfm_ctx_create] %-28s %8.1f ms\n") : fmt(format) {}
    void mark(const char *what)
    {
      if (!on)
        return;
      const auto t1 = std::chrono::steady_clock::now();
      fprintf(stderr, fmt, what, std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    }
  };
} // namespace pfm
