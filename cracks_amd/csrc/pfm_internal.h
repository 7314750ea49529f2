// pfm_internal.h — the context (pfm_ctx), the device views and the launcher declarations shared by the host-side files
// of the C ABI (pfm_host.h names them) and the kernel files (*.hip).  Not part of the ABI.
#pragma once

#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <string>
#include <vector>
#include <memory>
#include <type_traits>
#include <utility>

#include "../../include/pfm_assemble.h"
#include "pfm_kernel_clock.h"
#include "pfm_mesh_plan.h"

namespace pfm
{
  // Device-side view of the static mesh tables and the node state (SoA, HBM resident).
  // (PFM_CRES_*, HgEntry: pfm_mesh_plan.h, next to the host-only builder of the gather lists)
  constexpr int PFM_HS_RD = 96; // doubles per cell of DevView::hs_RD: residual of 16 resolved nodes x 4, placeholder of 8 vertices x 4
  struct DevView
  {
    int dim, layout, n_nodes, n_owned;
    long long n_cells;
    const int32_t *conn;   // [nv][n_cells]     cell -> local node, vertex-major (coalesced per vertex)
    const double *coords;  // [dim][n_nodes]
    const double *cell_lambda, *cell_mu; // [n_cells] or nullptr
    const long long *nadj_ptr; // [n_owned+1]  node graph (rows = owned nodes, sorted columns)
    const int32_t *nadj;
    const uint8_t *cslot;      // [n_cells][nv*nv] slot of vertex b's node in the row of vertex a's node
    const int32_t *color_cells; // [n_cells] cell ids sorted by colour class (pfm_ctx::color_ptr): no two cells of a class
                                // share a node, so the general cell kernel adds into the rows without atomics
    const int32_t *hn_index;   // [n_nodes] -> k (hanging table) or -1; nullptr when the mesh is conforming
    const long long *hn_ptr;
    const int32_t *hn_parents;
    const double *hn_weights;
    // cells with a hanging vertex: hcell[cell] = their running number (-1: none hangs), cslot_h[number][a][r][b][s] = slot of
    // parent s of vertex b in the row of parent r of vertex a (r, s < 4 in 3-D, < 2 in 2-D; a vertex that does not hang is
    // its own parent 0; 0xff: no such parent, row not owned, or not in the row).  nullptr: no hanging nodes, or one with more
    // parents than that (the cell kernel then searches the row, find_slot)
    const int32_t *hcell;
    const uint8_t *cslot_h;
    // per such cell (2-D and 3-D) a record of PFM_CRES_BYTES: int32 node[16] (its distinct constraint-resolved nodes, -1 unused),
    // uint8 slot[16][16] at PFM_CRES_SLOT (slot of node j in the row of node i), uint8 R at PFM_CRES_R (0xff: more than 16).
    // The cell kernel forms C^T K C over these nodes before it adds (k_assemble_general, KRED).  nullptr: no such cells.
    const uint8_t *cres;         // (round 6: + int32 hv[8] at PFM_CRES_HV, the cell's hanging vertices' nodes (-1: does not hang),
                                 // and the cell id at PFM_CRES_CELL)
    // Round 6, the default on 3-D meshes with hanging nodes (everywhere under PFM_HANGING_MODE_GATHER): the cells at hanging
    // vertices do not add into the outputs at all.  Their kernel writes K' = C^T K C, R' = C^T R and the placeholder diagonals
    // into per-cell scratch (hs_K at hs_off[hc]: R x R x KCMP doubles, KCMP = 13 in 3-D and 7 in 2-D; hs_RD: PFM_HS_RD doubles
    // per cell, the same strides in both dimensions), and k_hanging_gather adds them row by row in a fixed order
    // (pfm_ctx::d_hg_*): no atomics, no colour classes, bitwise reproducible.  nullptr: the atomic class of round 5.
    double *hs_K;
    const long long *hs_off;
    double *hs_RD;
    const uint8_t *node_flags; // [n_nodes] bit c: dof (node,c) has a homogeneous constraint line
    const uint8_t *cell_ring;  // [n_cells] or nullptr: 1 = a cell of a plain colour class that shares a (constraint-resolved) node
                               // with a cell of the atomic class: it adds atomically too, so that the atomic class may run NEXT
                               // TO the colour classes (general family, pfm_kernels.hip)
    // node state (cracks.cc:2147-2154 after the ghost import)
    double *u[3];
    double *phi, *phi_old, *phi_oldold;
    int *status; // device error word (pfm_status)
    // pfm_assemble_nl_residual_device on a single-rank 3-D box: the residual kernel reads `solution` (owned dofs, the
    // context's layout) itself while it fills its nodal planes and writes the node state on the way -- the separate scatter
    // launch of pfm_state_set_solution (0.1 ms at 216^3) disappears.  nullptr everywhere else.
    const double *fused_solution;
    // ---- cartesian overlay of a general 2-D mesh (round 4, pfm_kernels.hip: PATCH): rows of "regular" nodes -- not hanging,
    // not a parent, exactly four incident cells of one refinement level, a plain 9-neighbour row -- are completed inside one
    // workgroup per 8 x 8 block of that level's lattice and written once; the colour classes / the atomic class only run
    // over the cells that touch another row and skip the regular ones.  nullptr: no overlay.
    const uint8_t *row_patch;            // [n_nodes] 1 = the row is written by the patch kernel
    const int32_t *patch_cells;          // [n_patch_blocks][64] cell id of lattice position (cx, cy) of the block, -1 = none
    const int32_t *patch_nodes;          // [n_patch_blocks][81] node id of the block's 9 x 9 nodes, -1 = none
    const unsigned long long *node_slots; // [n_owned] regular rows: CSR slot of lattice offset o in bits 4 o .. 4 o + 3
  };

  // Uniform Cartesian box (fast path): lattice of (NX,NY,NZ) nodes, owned nodes form the
  // sub-box [o0,o1] (inclusive, lattice coordinates); rows are addressed by local node id.
  struct CartView
  {
    int NX, NY, NZ;
    int o0[3], o1[3];
    double h[3];
    const int32_t *local_of_box; // [NX*NY*NZ] lattice index -> local node id
    const uint32_t *nbr_mask;    // [n_owned] bit o (o < 27): lattice offset o exists in the row.  Bit 31 clear: the row
                                 // is in lattice order, the CSR slot of offset o is popcount(mask & ((1 << o) - 1))
    int owned_lex;               // 1: owned node (i,j,k) has local id (i-o0x) + OWX*((j-o0y) + OWY*(k-o0z))
    const uint8_t *row_perm;     // rows whose order is not the lattice order (bit 31 of nbr_mask: e.g. ghost columns
                                 // sorted behind the owned ones): CSR slot of the r-th existing offset =
                                 // row_perm[nadj_ptr[row] + r]; nullptr when no row needs it
    const double *cell_lam, *cell_mu; // per-cell Lame coefficients (cracks.cc:2207-2216) in lattice cell order
    double *cell_avg;                 // 2-D boxes: [(NX-1)*(NY-1)] scratch, mean |diagonal| of the element matrices of the blocks with
                                      // constrained rows -- from the first launch of k_cart2d_cells to the second
                                      // ci + (NX-1) (cj + (NY-1) ck); nullptr: the scalars of pfm_params
    // pfm_assemble_overlapped, phase 2: compact launches over the tiles that read ghost nodes (lists built on first use:
    // an early-exit launch over the full grid costs ~3 ns per skipped workgroup, 0.4 ms at 1.5e5 tiles)
    const int32_t *bnd_uu3, *bnd_res3; // tile indices of k_cart_uu3 / k_cart_residual3 (the latter for its z-chunk length)
    int n_bnd_uu3, n_bnd_res3, zc_res3;
    // Deferred (u,u) placeholder patches of k_cart_phi4 (constrained displacement rows whose element diagonal vanished in
    // some cell, deal.II's mean-|diagonal| rule): when the two Jacobian kernels run next to each other the phase-field kernel
    // must not add to values the (u,u) kernel may still be writing -- it appends (index, value) here and
    // launch_cart_apply_patches adds them after the join.  nullptr: patched in place (the kernels run one after the other).
    long long *patch_idx;
    double *patch_val;
    int *patch_count;
    int patch_cap;
    // Cartesian overlay of a general 3-D mesh (round 5): the lattice is ONE refinement level's, local_of_box holds -1
    // where the level has no node, and the rows this launch writes are those of row_of_box (-1: not a row of this level's
    // launch -- hanging, parent, mixed-level or ghost nodes stay with the general family).  nullptr: every owned node of
    // the box is a row (uniform boxes).
    const int32_t *row_of_box;
    int up_block_cleared;             // blocked layout: the structurally zero (u,phi) block holds its zeros already and the kernels of
                                      // this launch leave it alone -- a kept block (pfm_values_keep_up_block), or a 2-D box whose
                                      // assembly has cleared it with a fill in front of the launch (AssemblyPlan::up_block_cleared)
    int tile_sel;                     // 0: every tile; 1: only tiles that read no ghost node ("interior"); 2: only the
                                      // others -- the two launches of pfm_assemble_overlapped, between which the ghost
                                      // import lands (cracks.cc:2147-2154 next to the cell loop instead of in front of it)
    int zc_force[4];                  // pfm_ctx_force_zchunk, per marching kernel (PFM_ZC_*): 0 = the default length
                                      // (tuning variable, else the dispatch model), > 0 = that many planes (host side only)
    const int *uu_stale;              // k_cart_uu3 into a kept (u,u) block (pfm_values_keep_uu_block): the device word that says
                                      // whether the block must be written.  Every workgroup reads it once, before its first
                                      // barrier, and returns when it is 0 (about 3 ns per skipped workgroup, as the early exits
                                      // of the overlapped assembly).  nullptr: the launch writes.
  };
  // the marching kernels of the cartesian family, indices of CartView::zc_force (pfm_ctx_force_zchunk)
  enum
  {
    PFM_ZC_UU3 = 0,  // k_cart_uu3
    PFM_ZC_PHI4 = 1, // k_cart_phi4
    PFM_ZC_RES3 = 2, // k_cart_residual3x / 3d / 3
    PFM_ZC_RES2 = 3, // k_cart_residual2m
    PFM_ZC_KERNELS = 4
  };

  // does the node range [lo, hi] (tile + one-node halo, lattice indices along `axis`) contain a ghost node?  Ghost nodes
  // are the lattice nodes outside the owned box [o0, o1].
  __host__ __device__ inline bool cart_range_has_ghost(const CartView &cv, int axis, int lo, int hi)
  {
    const int n = axis == 0 ? cv.NX : (axis == 1 ? cv.NY : cv.NZ);
    return (cv.o0[axis] > 0 && lo < cv.o0[axis]) || (cv.o1[axis] < n - 1 && hi > cv.o1[axis]);
  }
  // tile filter of the overlapped assembly: true = this launch skips the tile
  __host__ __device__ inline bool cart_tile_skipped(const CartView &cv, bool touches_ghost)
  {
    return cv.tile_sel != 0 && touches_ghost != (cv.tile_sel == 2);
  }

  struct HaloPeer
  {
    int32_t *d_send = nullptr, *d_recv = nullptr;
    int64_t n_send = 0, n_recv = 0;
  };

  // launchers implemented in pfm_kernels.hip
  // uu_stale: the word of a kept (u,u) block (pfm_ctx::uu_words) or nullptr -- set to 1 when a phi_old or phi_oldold
  // of an owned node changes its bit pattern
  int launch_state_set(const DevView &v, const double *d_sol, const double *d_old,
                       const double *d_oldold, hipStream_t s, int *uu_stale = nullptr);
  // fills v.cslot from the current order of the node-graph rows (context creation, pfm_pattern_bind)
  int launch_build_cslot(const DevView &v, hipStream_t s);
  // d_out[a * n + i] = d_in[i * w + a] (mesh tables: host AoS -> device SoA)
  int launch_aos_to_soa_i32(const int32_t *d_in, int32_t *d_out, long long n, int w, hipStream_t s);
  int launch_aos_to_soa_f64(const double *d_in, double *d_out, long long n, int w, hipStream_t s);
  int launch_check_finite(const DevView &v, const double *d, int64_t n, hipStream_t s);
  // neighbour masks of a full lexicographic lattice: bit o = lattice offset o lies inside the box (CartView::nbr_mask)
  int launch_lattice_masks(uint32_t *d_mask, int NX, int NY, int NZ, int dim, hipStream_t s);
  int launch_halo_pack(const DevView &v, const int32_t *d_nodes, int64_t n, double *d_buf, hipStream_t s);
  // all peers at once: d_nodes = concatenated lists, d_ptr[n_peers + 1] = their offsets (device)
  int launch_halo_all(const DevView &v, const int32_t *d_nodes, const long long *d_ptr, int n_peers, int64_t n_total,
                      double *d_buf, int unpack, hipStream_t s);
  int launch_halo_unpack(const DevView &v, const int32_t *d_nodes, int64_t n, const double *d_buf,
                         hipStream_t s);
  // pfm_newton.hip: the flag bytes of a concatenated halo list, one byte per entry (pfm_halo_pack_flags_all / _unpack_)
  int launch_halo_flags_all(const DevView &v, const int32_t *d_nodes, int64_t n_total, uint8_t *d_buf, int unpack, hipStream_t s);
  // pfm_ctx::buf_flag_send / buf_flag_recv for the registered lists (grow-only, counted in device_bytes)
  int reserve_flag_halo_buffers(pfm_ctx *c);
  // The launchers of the cartesian family: each carries out its part of pl = plan_cart(v, cv, p, ...) (pfm_cart_plan.h).
  // s_side: the stream the caller forked off s for the phase-field kernel of the pair or for the residual kernel, else s.
  // d_scal: the MatScal of the current parameters on the device (upload_mat_scal; by value it would pin 900 bytes of
  // SGPRs in k_cart_phi4).  clock: the context's counters, for a plan that clocks a kernel.
  struct CartPlan;
  // CartPlan::voldev_sparse: the context's buffers of one sparse full assembly, zeroed by the caller in front of it
  struct SplitSparse
  {
    uint8_t *cell_comp; // [(NX-1)(NY-1)(NZ-1)] one byte per lattice cell: 1 = a q-point of the cell is compressed (k_cart_split3_mark)
    int *tile_flag;     // [ntx nty nch of grid[PFM_ZC_UU3]] 1 = the tile-chunk owns a vertex of such a cell
    int *n_rows;        // nodes whose rows the sparse form of k_cart_split3_jac recomputed
  };
  // CartPlan::keep_uu: the device words and the saved patch list of the context's kept (u,u) block (pfm_ctx::uu_*)
  struct UuKeep
  {
    int *words;           // [0] stale: the block must be written; [1] written: the assembly in flight wrote it (k_uu_mark)
    long long *saved_idx; // entries the deferred patches of the writing assembly went to, and their values before the patch
    double *saved_val;
    int *saved_count;
  };
  int launch_assemble_cart(const CartPlan &pl, const DevView &v, const CartView &cv, const pfm_params &p, double *const *d_values,
                           double *res_pde, double *res_tot, hipStream_t s, hipStream_t s_side, void *d_scal, KernelClock *clock,
                           int *n_compressed = nullptr /* CartPlan::voldev_jac: device counter, zeroed by the caller */,
                           const SplitSparse *sparse = nullptr /* CartPlan::voldev_sparse */,
                           const UuKeep *keep = nullptr /* CartPlan::keep_uu */);
  // pfm_cart_split3.hip: the matrix values of a CartPlan::voldev_jac assembly (sparse: its rows at compressed cells alone,
  // behind launch_cart_split3_mark and the unsplit kernels)
  int launch_cart_split3_jac(const CartPlan &pl, const DevView &v, const CartView &cv, const pfm_params &p, double *const *d_values,
                             int *n_compressed, hipStream_t s, const SplitSparse *sparse = nullptr);
  int launch_cart_split3_mark(const CartPlan &pl, const DevView &v, const CartView &cv, const pfm_params &p, const SplitSparse &sparse,
                              int *n_compressed, hipStream_t s);
  int launch_cart2d(const CartPlan &pl, const DevView &v, const CartView &cv, const pfm_params &p, double *const *d_values,
                    double *res_pde, double *res_tot, hipStream_t s);
  int launch_cart_uu3(const CartPlan &pl, const DevView &v, const CartView &cv, const pfm_params &p, double *vals_uu, hipStream_t s,
                      double *res_pde, KernelClock *clock);
  int launch_cart_phi4(const CartPlan &pl, const DevView &v, const CartView &cv, double *const *d_values, hipStream_t s,
                       const void *d_scal, double *res_pde, KernelClock *clock);
  // keep (CartPlan::keep_uu): an assembly that wrote the block records the values under its patches, one that kept it
  // finds them put back (launch_uu_mark_restore) and adds as ever
  int launch_cart_apply_patches(const CartView &cv, double *vals_uu, hipStream_t s, int *status, const UuKeep *keep = nullptr);
  // behind k_cart_uu3 on its stream: written := stale, stale := 0; then, in an assembly that kept the block, the recorded
  // values go back under the patches of the last one
  int launch_uu_mark_restore(const UuKeep &keep, double *vals_uu, hipStream_t s);
  int cart_n_cu();                                 // CUs of the device (asked once)
  int cart_zchunk(CartView cv, int kernel);        // chunk length of a whole assembly of cv by marching kernel PFM_ZC_*
  // XCD-aware launch: workgroup i runs on XCD i % 8.  The kernels are launched with a grid rounded up to a multiple
  // of 8 and map blockIdx to (blockIdx % 8) * (grid / 8) + blockIdx / 8, so that every XCD works on one contiguous
  // range of tiles (neighbouring tiles share their halo in that XCD's L2) and the slow boundary tiles are spread over
  // all XCDs — with the plain mapping a tile count per row that is a multiple of 8 (e.g. the 109-node edge of an
  // 8-rank sub-box) put every boundary tile on the same two XCDs (+30 % kernel time).
  constexpr unsigned xcd_grid(unsigned n_tiles) { return ((n_tiles + 7u) / 8u) * 8u; }
  constexpr size_t PFM_SCAL_BYTES = 4096;
  // the Jacobian launchers expect the MatScal of the current parameters at d_scal (uploaded by pfm_assemble_device
  // after every pfm_set_params, pfm_ctx::scal_dirty)
  int upload_mat_scal(const pfm_params &p, const CartView &cv, void *d_scal, hipStream_t s);
  // node graph of a general mesh on the device (pfm_graph.hip)
  struct GraphScratch
  {
    int *inc_ptr = nullptr, *inc = nullptr; // incidence lists: cells around every owned node
  };
  int graph_build_begin(const int32_t *d_cells, long long NC, int nv, int32_t NO, const int32_t *d_hn_index, const long long *d_hn_ptr,
                        const int32_t *d_hn_parents, long long *d_nadj_ptr, GraphScratch &sc, long long &total, hipStream_t s);
  int graph_build_rows(const int32_t *d_cells, long long NC, int nv, int32_t NO, const int32_t *d_hn_index, const long long *d_hn_ptr,
                       const int32_t *d_hn_parents, const long long *d_nadj_ptr, int32_t *d_nadj, const GraphScratch &sc, hipStream_t s);
  void graph_build_free(GraphScratch &sc);
  // row tables (CartView::nbr_mask, row_perm) of one level lattice of the 3-D cartesian overlay, from the current row order
  // Device scratch of the context build (raw mesh tables before their transposition, incidence lists and scan space of the
  // node graph): buffers up to 32 MB are kept between builds (64 MB at most) -- a hipMalloc / hipFree pair costs 0.1-0.4 ms and
  // the free synchronises the device, a rebuild at 2.7e5 cells made eight of them.  Users run on the NULL stream, so a buffer
  // handed back while its last kernel is still queued is safe to hand out again.  Contents undefined.
  hipError_t scratch_acquire(void **p, size_t bytes);
  void scratch_release(void *p);
  int launch_lattice_row_ptr(long long *d_ptr, int NX, int NY, int NZ, hipStream_t s);
  int launch_lattice_colour_order(int32_t *d_order, const int32_t *d_vertex0, const int32_t *d_box_of_local, long long NC, int NX, int NY, hipStream_t s);
  int launch_check_row_lengths(const uint8_t *d_mark, const long long *d_ptr, int32_t NO, int want, int *d_bad, hipStream_t s);
  int launch_overlay3_rows(const int32_t *d_node_at, const int32_t *d_row_at, int NX, int NY, int NZ, const long long *d_nadj_ptr,
                           const int32_t *d_nadj, uint32_t *d_nbr_mask, uint8_t *d_row_perm, int *d_bad, hipStream_t s);
  // color_ptr[n_classes + 1]: ranges of DevView::color_cells, one launch per class; the LAST class holds the cells with
  // hanging vertices (their rows are distributed to the parents, which other vertices of the same cell may be: atomics)
  int launch_assemble_general(const DevView &v, const pfm_params &p, int residual_only,
                              double *const *d_values, double *d_res_pde, double *d_res_tot,
                              hipStream_t s, const std::vector<long long> &color_ptr, hipStream_t s_atomic = nullptr,
                              int split_model = 0 /* PFM_SPLIT_*: pfm_set_split_model */);
  // the patch kernel of the cartesian overlay (2-D): one workgroup per block of DevView::patch_cells
  int launch_assemble_patches(const DevView &v, const pfm_params &p, int residual_only, double *const *d_values, double *d_res_pde,
                              double *d_res_tot, int n_blocks, hipStream_t s);
  // fills DevView::node_slots from the current order of the node-graph rows (context creation, pfm_pattern_bind)
  // rows [0, n_rows) of the gather tables: one wave per destination row, its entries in list order (fixed): plain adds
  int launch_hanging_gather(const DevView &v, const pfm_params &p, int residual_only, double *const *d_values, double *d_res_pde, double *d_res_tot,
                            const int32_t *rows, const long long *ptr, const HgEntry *list, int64_t n_rows, hipStream_t s);
  int launch_zero_rows(const DevView &v, double *const *d_values, const int32_t *rows, int n_rows, hipStream_t s);
  int launch_patch_slots(const DevView &v, unsigned long long *d_slots, int n_blocks, hipStream_t s);

  // a grow-only device buffer of the context (dev_buf_reserve, pfm_entry.h): in pfm_ctx::allocs, counted in device_bytes
  struct DevBuf
  {
    void *p = nullptr;
    size_t bytes = 0;
    template <class T>
    T *as() const
    {
      return static_cast<T *>(p);
    }
  };

  // pfm_values_to_host_delta (pfm_delta.hip): what the library knows about the host's copy of the matrix values
  struct DeltaState
  {
    bool valid = false;                          // shadow[b] holds what h_last[b] holds
    int64_t chunk_bytes = 0, slab_bytes = 0;     // pfm_values_delta_config; 0 = the default
    DevBuf shadow[4];                            // device copy of the host's values, per block
    const void *h_last[4] = {nullptr, nullptr, nullptr, nullptr};
    // per staging slot (two slabs in flight): chunk flags, [count, payload offset], index list + packed chunks
    DevBuf flags[2], count[2], pack[2];
    void *h_pack[2] = {nullptr, nullptr};        // page-locked images of pack[]
    unsigned long long *h_count = nullptr;       // page-locked, [2][2]
    size_t h_pack_bytes = 0;
    hipEvent_t ev_cmp[2] = {nullptr, nullptr}, ev_dma[2] = {nullptr, nullptr};
  };
  // the transfer path of pfm_values_to_host for one piece of a caller-owned array (pfm_transfer.cpp: d2h_user)
  hipError_t d2h_user_piece(pfm_ctx *c, void *h, const void *d, size_t bytes, hipStream_t s);
  // pfm_host_unregister of p (nullptr: all), pfm_ctx_destroy
  void delta_forget_host(pfm_ctx *c, const void *p);
  void delta_release(pfm_ctx *c);
} // namespace pfm

struct pfm_ctx
{
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<hipStream_t> ov_streams; // 3-D overlay: one stream per level lattice (forked off `stream` in an assembly)
  std::vector<hipEvent_t> ov_events;
  hipEvent_t ov_fork = nullptr;
  hipStream_t atomic_stream = nullptr; // 3-D overlay: the general family's atomic class next to its plain classes
  hipEvent_t ev_atomic = nullptr;
  hipStream_t side_stream = nullptr;            // residual + clearing of the (u,phi) block, concurrent with the Jacobian
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  pfm::DevView v{};
  pfm_params prm{};
  bool have_params = false;
  int split_model = 0; // PFM_SPLIT_*: pfm_set_split_model
  int split_route = 0; // PFM_SPLIT_ROUTE_*: pfm_set_split_route
  pfm::DevBuf buf_compressed;     // CartPlan::voldev_jac: cells with a compressed q-point, counted by k_cart_split3_jac (one int)
  bool compressed_valid = false;  // ... of the last full assembly, which ran on that kernel (pfm_ctx_split_route_info)
  // CartPlan::voldev_sparse: cell bytes, tile-chunk flags and the row counter of k_cart_split3_mark / the sparse form of
  // k_cart_split3_jac (made on first use, emptied in front of every sparse assembly); pfm_ctx_split_sparse_info
  pfm::DevBuf buf_sparse_cells, buf_sparse_flags, buf_sparse_rows;
  int64_t sparse_tiles = 0;       // tile-chunks of the last sparse full assembly (entries of buf_sparse_flags in use)
  bool sparse_valid = false;      // the last full assembly ran sparse
  bool sparse_levels = false;     // ... on the level lattices of an overlay (OverlayLevel::buf_sparse_*; the row counter is this one)
  int n_blocks = 1;
  int kernel_path = 0;
  int force_phase = 0; // pfm_ctx_force_phase (measurement)
  bool cart_ok = false;
  pfm::CartView cv{};
  // host copies needed for pattern queries
  pfm::raw_vector<long long> h_nadj_ptr;
  long long nadj_total = -1; // entries of the node graph when its row pointers only exist on the device so far (graph_dev_only)
  std::vector<int32_t> h_nadj;
  // Lattice meshes: the 27-wide host node graph (h_nadj), its device copy (v.nadj) and the slot table of the general
  // cell kernel (v.cslot) are 1.1 + 1.1 + 0.65 GB at 1e7 cells and are only needed by pfm_pattern_get / _bind and by the
  // general family: built on first use (ensure_host_graph, ensure_general_tables in pfm_ctx_build.cpp)
  bool graph_positional = false; // uniform box, node n at lattice position n, no ghosts: row pointers and colour lists are made on the device
  bool hanging_coloured = false; // 3-D: cells at hanging vertices sit in plain colour classes (reduced scatter, no atomics)
  int32_t n_hanging = 0;
  bool full_colours_lazy = false; // overlay context: the colour lists over ALL cells are made when the general family first runs without the overlay
  bool colours_lazy = false;     // DevView::color_cells is filled when the general family is first used (ensure_general_tables)
  bool graph_lazy = false;    // h_nadj not materialised yet (h_nadj_ptr is)
  bool graph_dev_only = false; // general mesh: v.nadj was built on the device (pfm_graph.hip), h_nadj is fetched on demand
  bool general_ready = true;  // v.nadj and v.cslot exist on the device
  std::vector<long long> color_ptr; // colour classes of the general cell kernel (DevView::color_cells)
  // owned device allocations
  std::vector<void *> allocs;
  int64_t device_bytes = 0;
  // staging for host-pointer entry points
  double *d_stage_vec[3] = {nullptr, nullptr, nullptr};
  double *d_stage_res[2] = {nullptr, nullptr};
  double *d_stage_val[4] = {nullptr, nullptr, nullptr, nullptr};
  // pfm_values_keep_up_block: the caller's (u,phi) block that holds its zeros and that nobody but the library writes
  // (nullptr: no promise).  stage_up_kept: d_stage_val[1] was cleared when it was allocated; only pfm_assemble writes it
  double *kept_up_block = nullptr;
  bool stage_up_kept = false;
  // pfm_values_keep_uu_block: the caller's (u,u) block that nobody but the library writes (nullptr: no promise), the two
  // device words of pfm::UuKeep and the saved patch list (capacity CartView::patch_cap).  uu_stale_pending: an input of K_uu
  // changed on the host side, or something else wrote the block -- the next assembly that would keep it raises the word
  // first, on its stream.  prm_uu: the parameter bytes of the last pfm_set_params.  h_flags_u: the displacement bits of the
  // last pfm_set_constraints.
  double *kept_uu_block = nullptr;
  int *uu_words = nullptr;
  long long *uu_saved_idx = nullptr;
  double *uu_saved_val = nullptr;
  int *uu_saved_count = nullptr;
  int uu_saved_cap = 0;
  bool uu_stale_pending = true;
  std::vector<uint8_t> h_flags_u;
  // host arrays the caller page-locked through pfm_host_register (DMA at the link rate instead of the pageable path);
  // zeroed: the array is the (u,phi) block of a matrix and has been cleared once (pfm_values_to_host never copies it)
  struct HostPin
  {
    void *p = nullptr;
    size_t bytes = 0;
    bool zeroed = false;
  };
  std::vector<HostPin> host_pins;
  hipStream_t copy_stream = nullptr; // second device -> host stream of pfm_values_to_host
  hipEvent_t ev_copy = nullptr;
  pfm::DeltaState delta; // pfm_values_to_host_delta
  std::vector<pfm::HaloPeer> peers;
  int32_t *d_send_all = nullptr, *d_recv_all = nullptr; // concatenated halo lists and their per-peer offsets
  long long *d_send_ptr = nullptr, *d_recv_ptr = nullptr;
  int64_t n_send_all = 0, n_recv_all = 0;
  double *d_halo_send = nullptr, *d_halo_recv = nullptr; // message buffers of pfm_halo_exchange
  int64_t halo_buf_bytes = 0;                            // their share of device_bytes
  void *d_scal = nullptr; // per-launch scalar tables of the cartesian kernels (PFM_SCAL_BYTES)
  pfm::KernelClock clock; // counters of the phase clocks of k_cart_uu3 / k_cart_phi4 (profiling)
  int64_t n_flag_u = 0;   // displacement dofs with a constraint flag (capacity of the deferred patch list, CartView::patch_*)
  uint8_t *d_row_perm = nullptr; // CartView::row_perm storage (in allocs)
  bool overlap_lists_ready = false; // CartView::bnd_uu3 / bnd_res3 built
  pfm::LatticeHost lat;          // host lattice tables (cartesian path only)
  bool pattern_bound[4] = {false, false, false, false};
  bool scal_dirty = true; // d_scal does not hold the tables of the current parameters yet
  // cartesian overlay of a general 2-D mesh (DevView::row_patch ...): blocks, the reduced cell lists of the general family
  int n_patch_blocks = 0;
  int64_t n_patch_rows = 0, n_general_cells = 0;
  unsigned long long *d_node_slots = nullptr;
  bool patch_slots_valid = false;
  // cartesian overlay of a general 3-D mesh (round 5): one level lattice per refinement level with regular rows; the
  // row-owner kernels of the cartesian family (k_cart_uu3, k_cart_phi4, k_cart_residual3) run on each of them and write the
  // regular rows, the general family keeps the rest (same reduced lists as the 2-D overlay)
  struct OverlayLevel
  {
    pfm::CartView cv{};
    void *d_scal = nullptr; // the level's MatScal (its cell size)
    bool scal_dirty = true;
    int64_t n_rows = 0;
    pfm::DevBuf buf_sparse_cells, buf_sparse_flags; // CartPlan::voldev_sparse on this level lattice: as the context's, below
    int64_t sparse_tiles = 0;
  };
  std::vector<OverlayLevel> levels3;
  uint32_t *d_nbr_mask3 = nullptr;
  uint8_t *d_row_perm3 = nullptr;
  bool overlay3_rows_valid = false;
  int32_t *d_rows_general = nullptr;        // owned nodes whose rows the general family writes in an overlay assembly
  int32_t n_rows_general = 0;
  int32_t *d_color_cells_reduced = nullptr; // colour-sorted cells that touch a row the patches do not write
  std::vector<long long> color_ptr_reduced;
  uint8_t *d_cell_ring_reduced = nullptr;
  // scratch of the Newton-side sweeps (pfm_newton.hip): the 3 counts of pfm_active_set_device
  pfm::DevBuf buf_counts;
  pfm::DevBuf buf_hn_nodes;      // pfm_distribute_hanging_device: node of entry k of the hanging table (-1: none), built at its first call
  bool hn_nodes_ready = false;
  pfm::DevBuf buf_flag_send, buf_flag_recv; // message buffers of pfm_halo_exchange_flags, one byte per halo node
  // gather tables of the cells at hanging vertices (DevView::hs_*): destination rows, their entry lists (hc * 32 + index:
  // index < 16 = resolved node i of cell hc, 16 + a = the hanging vertex a's own row), ascending per row
  int32_t *d_hg_rows = nullptr;
  long long *d_hg_ptr = nullptr;
  pfm::HgEntry *d_hg_list = nullptr;
  int64_t n_hg_rows = 0;
  int64_t n_hcells = 0;           // cells at hanging vertices (records of DevView::cres)
  bool hang_gather = false;       // PFM_HANGING_MODE_DEFAULT, 3-D: decided at pfm_ctx_create (PFM_HANGING_ATOMIC=1: off)
  int hang_mode = 0;              // PFM_HANGING_MODE_*: pfm_set_hanging_mode
  bool hang_gather_failed = false; // a cell with more than 16 resolved nodes: the context keeps its atomic class in every mode
  int64_t hang_gather_bytes = 0;  // device bytes of the gather tables and the scratch (counted in device_bytes)
  bool hang_gather_ready = false; // tables and scratch exist
  bool colour_overflow = false;   // cells without a hanging vertex sit in the last class (a node of more than 62 cells)
  pfm::DevBuf buf_norm_partial; // pfm_residual_norms: [2048][2] block partials + the 3 results; pfm_line_search_device: [2048][3] + 5
  pfm::DevBuf buf_ls_saved;     // saved_solution of pfm_line_search_device (SAVED mode): one dof vector, from its first use on
  pfm::DevBuf buf_partial;      // 3-wide reductions of pfm_newton.hip / pfm_postproc.hip: [blocks][3] partials + the 3 results
  pfm::DevBuf buf_cell_owned;   // the owned-cell mask of the entry that runs (upload_mask, pfm_entry.h)
  pfm::DevBuf buf_func_mat;     // per-cell Lame override of pfm_functionals_material
  // post-processing functionals (pfm_postproc.hip): the (line, cell, face) list of pfm_cod_lines, kept for the lines, eps
  // and cell mask it was built for (the mesh geometry of a context never changes).  Device buffers are in `allocs`.
  struct CodCache
  {
    bool valid = false;
    std::vector<double> lines;
    double eps = 0.0;
    bool masked = false;
    std::vector<uint8_t> mask;
    long long *d_line_ptr = nullptr; // [n_lines + 1] entry ranges per line
    long long *d_entry = nullptr;    // [n_entries] cell * 2 dim + face, ordered by line, cell, face
    int64_t n_entries = 0;
  } cod;
  pfm::DevBuf buf_face_cells, buf_face_ids; // pfm_face_load input staging
  pfm::DevBuf buf_adapt;                    // mesh adaptation (pfm_adapt.hip): one scratch buffer
  pfm::DevBuf buf_stat;                     // pfm_cod_buckets / pfm_point_eval (pfm_pointstat.hip): one scratch buffer
  // face-neighbour table of pfm_kelly_indicator, built on first use (in allocs): neighbour cell or side-list entry and the
  // relation byte per (face, cell), and the fine faces of every face against finer cells
  int32_t *d_face_nbr = nullptr;
  uint8_t *d_face_rel = nullptr;
  uint32_t *d_face_sub = nullptr;
  bool face_table_ready = false;
  // measurement (pfm_timing_enable)
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  std::string err;

  int64_t n_owned_dofs() const { return (int64_t)v.n_owned * (v.dim + 1); }
  int64_t block_rows(int b) const;
  int64_t block_nnz(int b) const;
};
