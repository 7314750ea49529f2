// pfm_dispatch.cpp -- assembly dispatch (include/pfm_assemble.h; DESIGN.md, "Assembly dispatch"): the tables an assembly
// makes on first use, one plan per call (AssemblyPlan, plan_assembly), one routine per kernel family (assemble_box,
// assemble_overlay, assemble_general) under assemble_impl, the device entry points with the overlapped assembly and the
// force_* switches of the measurements, the timing events, and the info queries that replay the plan.
#include "pfm_host.h"
#include "pfm_cart_plan.h"

#include <algorithm>
#include <utility>
#include <vector>

using namespace pfm;

namespace
{
  // cartesian overlay: the slots of the regular rows follow the order of the node-graph rows (pfm_pattern_bind may change it);
  // v.nadj exists (ensure_tables: lattice contexts build the general tables on first use)
  int ensure_patch_ready(pfm_ctx *c)
  {
    if (c->n_patch_blocks == 0 || c->patch_slots_valid)
      return PFM_OK;
    const int rc = launch_patch_slots(c->v, c->d_node_slots, c->n_patch_blocks, c->stream);
    if (rc)
      return fail(c, rc, "patch slots");
    c->patch_slots_valid = true;
    return PFM_OK;
  }

  // 3-D overlay: neighbour masks and CSR slots of the regular rows from the current order of the node-graph rows
  int ensure_overlay3_ready(pfm_ctx *c)
  {
    if (c->levels3.empty() || c->overlay3_rows_valid)
      return PFM_OK;
    if (!c->d_nbr_mask3)
      if (const int rcg = guarded(c, [&] {
            c->d_nbr_mask3 = dev_alloc<uint32_t>(c, (size_t)std::max<int32_t>(c->v.n_owned, 1));
            c->d_row_perm3 = dev_alloc<uint8_t>(c, (size_t)std::max<long long>(c->nadj_total >= 0 ? c->nadj_total : (c->h_nadj_ptr.empty() ? 1 : c->h_nadj_ptr.back()), 1));
          }))
        return rcg;
    int *d_bad = nullptr;
    if (hipMalloc((void **)&d_bad, sizeof(int)) != hipSuccess)
      return fail(c, PFM_ERR_NOMEM, "overlay row tables");
    hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(int), c->stream);
    if (e == hipSuccess)
      e = hipMemsetAsync(c->d_nbr_mask3, 0, sizeof(uint32_t) * (size_t)std::max<int32_t>(c->v.n_owned, 1), c->stream);
    int rc = e == hipSuccess ? PFM_OK : PFM_ERR_HIP;
    for (auto &lv : c->levels3)
      if (rc == PFM_OK)
        rc = launch_overlay3_rows(lv.cv.local_of_box, lv.cv.row_of_box, lv.cv.NX, lv.cv.NY, lv.cv.NZ, c->v.nadj_ptr, c->v.nadj, c->d_nbr_mask3,
                                  c->d_row_perm3, d_bad, c->stream);
    int bad = 0;
    if (rc == PFM_OK && (hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                         hipStreamSynchronize(c->stream) != hipSuccess))
      rc = PFM_ERR_HIP;
    (void)hipFree(d_bad);
    if (rc)
      return fail(c, rc, "overlay row tables");
    if (bad != 0)
      return fail(c, PFM_ERR_INTERNAL, "3-D overlay: a regular row is not a plain 27-neighbour row of its level");
    for (auto &lv : c->levels3)
      {
        lv.cv.nbr_mask = c->d_nbr_mask3;
        lv.cv.row_perm = c->d_row_perm3;
      }
    c->overlay3_rows_valid = true;
    return PFM_OK;
  }

  // phase 2 of pfm_assemble_overlapped launches only the tiles that read ghost nodes: their indices, once per context
  int ensure_overlap_lists(pfm_ctx *c)
  {
    if (c->overlap_lists_ready || c->kernel_path != 1 || c->v.dim != 3)
      return PFM_OK;
    std::vector<int32_t> t_uu, t_res;
    pfm::CartView half2 = c->cv; // the grids of the second half, before there are lists
    half2.tile_sel = 2;
    cart_tile_grid(half2, PFM_ZC_UU3, cart_n_cu(), &t_uu);
    const int zc = cart_tile_grid(half2, PFM_ZC_RES3, cart_n_cu(), &t_res).zc;
    const int n_uu = (int)t_uu.size(), n_res = (int)t_res.size();
    if (t_uu.empty())
      t_uu.push_back(0);
    if (t_res.empty())
      t_res.push_back(0);
    if (const int rcu = guarded(c, [&] {
          c->cv.bnd_uu3 = dev_upload(c, t_uu.data(), t_uu.size());
          c->cv.bnd_res3 = dev_upload(c, t_res.data(), t_res.size());
        }))
      return rcu;
    c->cv.n_bnd_uu3 = n_uu;
    c->cv.n_bnd_res3 = n_res;
    c->cv.zc_res3 = zc;
    c->overlap_lists_ready = true;
    return PFM_OK;
  }

  // pfm_ctx_force_zchunk of the residual kernel: its list holds tiles of chunks of the old length.  Freed here, made again
  // for the new length by the next assembly that runs a half (assemble_impl)
  void drop_overlap_lists(pfm_ctx *c)
  {
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize(); // a queued launch of phase 2 may still read them
    const std::pair<const int32_t *, int> lists[2] = {{c->cv.bnd_uu3, c->cv.n_bnd_uu3}, {c->cv.bnd_res3, c->cv.n_bnd_res3}};
    for (const auto &l : lists)
      {
        auto it = std::find(c->allocs.begin(), c->allocs.end(), (void *)l.first);
        if (!l.first || it == c->allocs.end())
          continue;
        c->allocs.erase(it);
        c->device_bytes -= (int64_t)sizeof(int32_t) * std::max(l.second, 1); // (an empty list was uploaded as one entry)
        (void)hipFree((void *)l.first);
      }
    c->cv.bnd_uu3 = c->cv.bnd_res3 = nullptr;
    c->cv.n_bnd_uu3 = c->cv.n_bnd_res3 = c->cv.zc_res3 = 0;
    c->overlap_lists_ready = false;
  }

  // ---- assembly dispatch: one plan (AssemblyPlan), one routine per kernel family ("Assembly dispatch") ----
  // (the A/B switches of the dispatch: pfm_switches.h)
  // the stress split in the matrix (cracks.cc:2294): the general family has it, the row-owner kernels do not
  bool stress_split(const pfm_ctx *c) { return c->have_params && cart_scheme(c->prm).split; }
  // ... but for what plan_cart takes from the law and the route of the context (CartPlan::voldev, CartPlan::spectral)
  pfm::CartSplit cart_split(const pfm_ctx *c) { return {c->split_model, c->split_route}; }

  // Every decision of one assemble_impl call; what each means stands where it is made (plan_assembly, after_tables).
  struct AssemblyPlan
  {
    int phase = 0; // 0: the whole assembly; 1, 2: the halves of pfm_assemble_overlapped
    bool residual_only = false, split = false, cart = false, patches = false, overlay3 = false, overlay_uu = false, nothing = false;
    bool pair = false, fork = false, levels_concurrent = false, fill_up_block = false, up_block_cleared = false;
    bool keep_up_block = false; // d_values[1] is a kept (u,phi) block: nothing of this call writes it
    bool keep_uu = false;       // d_values[0] is a kept (u,u) block and the promise applies: written only when stale (CartPlan::keep_uu)
    bool gather = false, fork_general = false, atomic_stream = false; // final behind the lazy tables: after_tables
    CartPlan box;   // cart: what the launchers of the cartesian family do (plan_cart)
    CartPlan level; // overlay3: the same for the first level lattice (every level shares its scheme, law and kernels)
    void after_tables(const pfm_ctx *c, bool gather_ready);
  };

  // No side effects, no allocation: what the context, the parameters and the switches say about this call.
  AssemblyPlan plan_assembly(const pfm_ctx *c, int residual_only, int phase, double *const *d_values)
  {
    AssemblyPlan p;
    p.phase = phase;
    p.residual_only = residual_only != 0;
    p.split = stress_split(c);
    if (c->kernel_path == 1)
      p.box = plan_cart(c->v, c->cv, c->prm, residual_only, phase, cart_n_cu(), cart_split(c));
    p.cart = c->kernel_path == 1 && p.box.supported; // assemble_box
    // the general family and the overlays are not cut into interior / boundary work: everything in phase 2
    p.nothing = !p.cart && phase == 1;
    // debug: general + cart (u,u).  Path 2 implies no overlay (pfm_ctx_force_path: lattice contexts only, which have no
    // patches and no level lattices), so assemble_general alone launches the (u,u) kernel
    p.overlay_uu = c->kernel_path == 2 && !residual_only && !p.split;
    // cartesian overlay of a general mesh (AMR meshes; stress-split runs on a lattice): patch kernel (2-D) or level
    // lattices (3-D) for the regular rows, the general family for the rest (PFM_NO_PATCH=1 at context creation: general
    // family alone): assemble_overlay
    // (a split assembly keeps its level lattices where plan_cart has a kernel with the law: CartPlan::voldev, CartPlan::spectral)
    if (!p.cart && c->v.dim == 3 && !c->levels3.empty() && c->kernel_path != 0 && !p.nothing)
      p.level = plan_cart(c->v, c->levels3[0].cv, c->prm, residual_only, 0, cart_n_cu(), cart_split(c)); // (voldev_jac: bit 8 of the route)
    p.overlay3 = p.level.supported;
    p.patches = (!p.cart && c->v.dim == 2 && c->n_patch_blocks > 0 && c->kernel_path != 0 && !p.nothing) || p.overlay3;
    // cells at hanging vertices: scratch + ordered gather instead of atomics (round 6; DevView::hs_*) -- wanted.
    // PFM_HANGING_MODE_DEFAULT: 3-D only, and a split assembly keeps it under PFM_SPLIT_VOLDEV alone (under the spectral law
    // the cells at hanging vertices add with atomics, also where the level lattices take the spectral residual,
    // CartPlan::spectral: not bitwise reproducible).  PFM_HANGING_MODE_GATHER: both dimensions, every law; _ATOMIC: never.
    const bool gather_default = c->v.dim == 3 && c->hang_gather && (!p.split || c->split_model == PFM_SPLIT_VOLDEV);
    const bool gather_asked = c->hang_mode == PFM_HANGING_MODE_GATHER && c->n_hcells > 0 && c->v.cres && !c->hanging_coloured;
    p.gather = !p.cart && !p.nothing && !c->hang_gather_failed &&
               (c->hang_mode == PFM_HANGING_MODE_DEFAULT ? gather_default : gather_asked);
    // The two Jacobian kernels of a 3-D box next to each other (default): with equal LDS allocations (64 granules of 1280 B
    // each) any freed slot of a CU takes a workgroup of either kernel, the (u,u) and the phase-field workgroups mix and
    // fill each other's stalls: 14.07 -> 13.75 ms per assembly at 216^3 (PFM_JAC_SEQUENTIAL=1: one after the other).
    p.pair = p.cart && p.box.pair;
    // 2-D boxes never fork: the second launch of k_cart2d_cells (phase-field rows) reads the mean |diagonal| the first one
    // leaves in CartView::cell_avg, so it must follow it on the same stream.  (The fork was measured at 0.262 -> 0.259 ms of
    // kernel time at 1000^2 and was off by default; with an event between the launches nothing of that overlap is left.)
    p.fork = p.cart && !residual_only && phase == 0 && (p.pair || (c->v.dim != 2 && Switches::side_stream()));
    // the row-owner kernels of the cartesian family on every level lattice: each level on a stream of its own, forked
    // off the context's stream (a level lattice of 6e5 nodes fills a third of the chip's dispatch slots; the levels
    // write disjoint rows) when PFM_OVERLAY3_CONCURRENT=1 is set.  Default: one after the other on the context's
    // stream -- measured the better of the two (profiles/r05/ov3_ab.txt: 4.56 against 4.86 ms per Jacobian)
    p.levels_concurrent = p.overlay3 && c->levels3.size() > 1 && Switches::levels_concurrent();
    // 2-D box, blocked layout: the structurally zero (u,phi) block (cracks.cc:2333-2337) by a fill in front of the kernels,
    // in the whole assembly and in phase 1; phase 2 takes it as cleared by phase 1 (CartView::up_block_cleared).
    // A kept block (pfm_values_keep_up_block; the library's own staging block, cleared when pfm_assemble allocated it)
    // holds its zeros from one assembly to the next: no fill, and in both dimensions no store of any row-owner kernel
    // (k_cart2d_cells, k_cart_phi4, k_cart_split3_jac) and no memset of the general family.  Without a promise the 3-D
    // kernels write the block with their rows: 21 of the 49 store instructions of every copy-out of k_cart_phi4, 6.6 of
    // the 38 GB a 216^3 assembly writes.  Moving those stores elsewhere never paid (a fill on a third stream: 10.95 ->
    // 11.35 ms, profiles/r06/ab_up_fill.txt); not doing them at all does (profiles/keep_up_block/README.md).
    // PFM_NO_KEEP_UP_BLOCK=1: the promise is ignored.
    const double *up = (!residual_only && c->n_blocks == 4 && d_values) ? d_values[1] : nullptr;
    p.keep_up_block = up && (up == c->kept_up_block || (c->stage_up_kept && up == c->d_stage_val[1])) && Switches::keep_up_block();
    const bool blocked2 = p.cart && c->v.dim == 2 && !residual_only && c->v.layout == PFM_LAYOUT_BLOCKED;
    p.fill_up_block = blocked2 && phase <= 1 && c->n_blocks == 4 && d_values[1] && Switches::cart2d_fill() && !p.keep_up_block;
    p.up_block_cleared = p.keep_up_block || p.fill_up_block || (blocked2 && phase == 2 && Switches::cart2d_fill());
    // A kept (u,u) block (pfm_values_keep_uu_block) is left alone while it provably holds the current values.  Only where the
    // block cannot depend on `solution` and the library is the only writer of the node state: the pair of a 3-D box (blocked
    // layout, linear scheme, kappa < 0.5, homogeneous material, the whole assembly, no level lattice -- CartPlan::pair) on a
    // context without ghost nodes or peers.  Everywhere else the promise is ignored and the block is written; that assembly
    // leaves the block stale for the next one that would keep it (assemble_impl).  PFM_NO_KEEP_UU_BLOCK=1: ignored everywhere.
    const double *uu = (!residual_only && c->n_blocks == 4 && d_values) ? d_values[0] : nullptr;
    p.keep_uu = uu && uu == c->kept_uu_block && Switches::keep_uu_block() && p.pair && c->peers.empty() && c->v.n_owned == c->v.n_nodes;
    if (p.keep_uu)
      plan_keep_uu(p.box, c->v, c->cv, cart_n_cu());
    return p;
  }

  // What depends on the lazy tables (ensure_tables): the gather has its tables or the context keeps its atomic class, and
  // DevView::cell_ring exists once the colours do.
  void AssemblyPlan::after_tables(const pfm_ctx *c, bool gather_ready)
  {
    gather = gather && gather_ready;
    // general family: the atomic class (cells with hanging vertices) on the side stream next to the colour classes, behind
    // the zeroing of the outputs (DevView::cell_ring; a residual-only assembly keeps the stream order: its atomic class
    // takes 15 us, less than a fork and a join).  Overlay: the patch kernel on the stream, every class of the (small) rest
    // of the general family on the side stream.
    fork_general = !cart && !switches().general_sequential &&
                   ((!residual_only && c->v.cell_ring != nullptr) || (patches && c->n_general_cells > 0));
    // 3-D overlay Jacobian: the class of the cells at hanging vertices (FP64 atomics, 4.7 of the general family's 6 ms at
    // 1.1e6 cells) on a third stream next to the plain classes (DevView::cell_ring makes that safe).
    // (PFM_HANGING_COLOURED: a hanging cell in a plain class adds to its PARENTS' rows without atomics; should a cell with
    // more than 16 resolved nodes ever sit in the atomic class next to it, that class must not run beside the plain ones)
    atomic_stream = overlay3 && fork_general && !residual_only && (c->v.cell_ring || gather) && c->n_general_cells > 0 &&
                    !c->hanging_coloured;
  }

  // the only place that makes side_stream, ev_fork and ev_join
  int ensure_side_stream(pfm_ctx *c)
  {
    if (c->side_stream)
      return PFM_OK;
    if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "side stream");
    return PFM_OK;
  }

  // what `to` gets from here on runs behind what `from` has got so far; join_from: the same, named for the reader
  int fork_to(pfm_ctx *c, hipStream_t from, hipStream_t to, hipEvent_t ev, const char *what)
  {
    hipError_t e = hipEventRecord(ev, from);
    if (e == hipSuccess)
      e = hipStreamWaitEvent(to, ev, 0);
    return e == hipSuccess ? PFM_OK : hipfail(c, e, what);
  }
  int join_from(pfm_ctx *c, hipStream_t from, hipStream_t to, hipEvent_t ev, const char *what) { return fork_to(c, from, to, ev, what); }

  // the side stream behind what the context's stream has got so far (its join: join_from with ev_join)
  int fork_side(pfm_ctx *c, const char *what)
  {
    const int rc = ensure_side_stream(c);
    return rc ? rc : fork_to(c, c->stream, c->side_stream, c->ev_fork, what);
  }

  // the next pair of timing events; the interval opens on the context's stream
  int open_interval(pfm_ctx *c, hipEvent_t &ev0, hipEvent_t &ev1)
  {
    if (c->ev_used == c->ev_pool.size())
      {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "hipEventCreate");
        c->ev_pool.emplace_back(a, b);
      }
    ev0 = c->ev_pool[c->ev_used].first;
    ev1 = c->ev_pool[c->ev_used++].second;
    (void)hipEventRecord(ev0, c->stream);
    return PFM_OK;
  }

  // deferred placeholder patches of the pair: one entry per flagged displacement dof at most; emptied on the stream
  int ensure_patch_list(pfm_ctx *c)
  {
    if (c->cv.patch_cap < c->n_flag_u || !c->cv.patch_count)
      {
        for (void *q : {(void *)c->cv.patch_idx, (void *)c->cv.patch_val, (void *)c->cv.patch_count})
          if (q)
            (void)hipFree(q);
        c->device_bytes -= (int64_t)c->cv.patch_cap * 16 + (c->cv.patch_count ? 4 : 0);
        c->cv.patch_idx = nullptr, c->cv.patch_val = nullptr, c->cv.patch_count = nullptr;
        const size_t cap = (size_t)std::max<int64_t>(c->n_flag_u, 1);
        if (hipMalloc((void **)&c->cv.patch_idx, cap * sizeof(long long)) != hipSuccess ||
            hipMalloc((void **)&c->cv.patch_val, cap * sizeof(double)) != hipSuccess ||
            hipMalloc((void **)&c->cv.patch_count, sizeof(int)) != hipSuccess)
          return fail(c, PFM_ERR_NOMEM, "patch list");
        c->cv.patch_cap = (int)std::min<size_t>(cap, 0x7fffffff);
        c->device_bytes += (int64_t)c->cv.patch_cap * 16 + 4;
      }
    return hipMemsetAsync(c->cv.patch_count, 0, sizeof(int), c->stream) == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "patch list reset");
  }

  // AssemblyPlan::keep_uu: the saved patch list of the kept (u,u) block, as long as the patch list (behind ensure_patch_list).
  // A new one is empty and the block counts as stale.  uu_stale_pending: the word is raised here, on the assembly's stream.
  int ensure_uu_keep(pfm_ctx *c, pfm::UuKeep &keep)
  {
    if (!c->uu_words)
      return fail(c, PFM_ERR_INTERNAL, "kept (u,u) block without its device words");
    if (c->uu_saved_cap < c->cv.patch_cap || !c->uu_saved_count)
      {
        (void)hipStreamSynchronize(c->stream); // (off the hot path: a kernel in flight may still read the old list)
        for (void *q : {(void *)c->uu_saved_idx, (void *)c->uu_saved_val, (void *)c->uu_saved_count})
          if (q)
            (void)hipFree(q);
        c->device_bytes -= (int64_t)c->uu_saved_cap * 16 + (c->uu_saved_count ? 4 : 0);
        c->uu_saved_idx = nullptr, c->uu_saved_val = nullptr, c->uu_saved_count = nullptr, c->uu_saved_cap = 0;
        const size_t cap = (size_t)std::max(c->cv.patch_cap, 1);
        if (hipMalloc((void **)&c->uu_saved_idx, cap * sizeof(long long)) != hipSuccess ||
            hipMalloc((void **)&c->uu_saved_val, cap * sizeof(double)) != hipSuccess ||
            hipMalloc((void **)&c->uu_saved_count, sizeof(int)) != hipSuccess)
          return fail(c, PFM_ERR_NOMEM, "saved patch list of the kept (u,u) block");
        c->uu_saved_cap = (int)cap;
        c->device_bytes += (int64_t)c->uu_saved_cap * 16 + 4;
        if (hipMemsetAsync(c->uu_saved_count, 0, sizeof(int), c->stream) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "saved patch list reset");
        c->uu_stale_pending = true;
      }
    if (c->uu_stale_pending)
      {
        if (hipMemsetD32Async((hipDeviceptr_t)c->uu_words, 1, 1, c->stream) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "raise the stale word of the kept (u,u) block");
        c->uu_stale_pending = false;
      }
    keep = {c->uu_words, c->uu_saved_idx, c->uu_saved_val, c->uu_saved_count};
    return PFM_OK;
  }

  // the lazy tables of the plan's family; gather_ready: the gather has its tables (false: the atomic class stays)
  int ensure_tables(pfm_ctx *c, const AssemblyPlan &p, bool &gather_ready)
  {
    int rc = PFM_OK;
    if (!p.cart)
      rc = guarded(c, [&] { ensure_general_tables(c); }); // (lattice contexts build them on first use)
    if (rc == PFM_OK && p.patches)
      rc = p.overlay3 ? ensure_overlay3_ready(c) : ensure_patch_ready(c);
    else if (rc == PFM_OK && !p.cart && c->full_colours_lazy)
      rc = guarded(c, [&] { ensure_full_colours(c); }); // (a context that has only run with its overlay so far)
    if (rc == PFM_OK && p.gather)
      rc = guarded(c, [&] { gather_ready = ensure_hang_gather(c); });
    return rc;
  }

  // zero the outputs (cracks.cc:2133-2137).  The row-owner kernels write every entry exactly once -- the structurally zero
  // (u,phi) block of the blocked layout included (k_cart_phi4), unless it is a kept block (AssemblyPlan::keep_up_block), which
  // nobody writes or zeroes -- and need no zeroing pass: of a box nothing is zeroed, of an overlay the residuals and the
  // rows of the general family (launch_zero_rows and the scatter of the general family can only write or add zeros to a
  // kept block: they stay as they are).
  int zero_outputs(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot)
  {
    hipError_t e = hipSuccess;
    if (!p.cart)
      e = hipMemsetAsync(d_res_pde, 0, sizeof(double) * (size_t)c->n_owned_dofs(), c->stream);
    if (!p.cart && e == hipSuccess && p.residual_only)
      e = hipMemsetAsync(d_res_tot, 0, sizeof(double) * (size_t)c->n_owned_dofs(), c->stream);
    if (e == hipSuccess && !p.residual_only)
      for (int b = 0; b < c->n_blocks && e == hipSuccess; ++b)
        {
          if (!d_values[b] && c->block_nnz(b) > 0)
            return fail(c, PFM_ERR_BAD_ARG, "null matrix block");
          if (!p.cart && !p.patches && !(b == 1 && p.keep_up_block))
            e = hipMemsetAsync(d_values[b], 0, sizeof(double) * (size_t)c->block_nnz(b), c->stream);
        }
    if (e == hipSuccess && p.patches && !p.residual_only && c->n_rows_general > 0 &&
        launch_zero_rows(c->v, d_values, c->d_rows_general, c->n_rows_general, c->stream) != PFM_OK)
      return fail(c, PFM_ERR_HIP, "zero the rows of the general family");
    return e == hipSuccess ? PFM_OK : hipfail(c, e, "zero outputs");
  }

  // CartPlan::voldev_jac: the device counter of the cells with a compressed q-point (pfm_ctx_split_route_info), made on first
  // use; zero: emptied on the context's stream, in front of the launch (or the first of the launches) that counts
  int compressed_counter(pfm_ctx *c, bool zero, int *&n_compressed)
  {
    if (const int rc = dev_buf_reserve(c, c->buf_compressed, sizeof(int), "compressed-cell counter"))
      return rc;
    n_compressed = c->buf_compressed.as<int>();
    if (zero && hipMemsetAsync(n_compressed, 0, sizeof(int), c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "compressed-cell counter reset");
    return PFM_OK;
  }

  // CartPlan::voldev_sparse: the cell bytes, the tile-chunk flags of grid[PFM_ZC_UU3] and the row counter, made on first use
  // (grow-only: a longer lattice of flags after pfm_ctx_force_zchunk) and emptied on the context's stream in front of
  // k_cart_split3_mark
  // the row counter: one for the box, one for all level lattices of an overlay (emptied once, on the context's stream)
  int sparse_row_counter(pfm_ctx *c)
  {
    if (const int rc = dev_buf_reserve(c, c->buf_sparse_rows, sizeof(int), "row counter of the sparse split Jacobian"))
      return rc;
    return hipMemsetAsync(c->buf_sparse_rows.p, 0, sizeof(int), c->stream) == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "sparse split Jacobian: counter reset");
  }
  // the cell bytes and tile-chunk flags of lattice cv (the box, or one level lattice with buffers of its own), emptied on s
  int sparse_buffers(pfm_ctx *c, const pfm::CartView &cv, const CartPlan &pl, pfm::DevBuf &cells, pfm::DevBuf &flags, int64_t &tiles,
                     hipStream_t s, pfm::SplitSparse &sp)
  {
    const TileGrid &g = pl.grid[PFM_ZC_UU3];
    const size_t n_cells = (size_t)std::max(cv.NX - 1, 0) * (size_t)std::max(cv.NY - 1, 0) * (size_t)std::max(cv.NZ - 1, 0);
    const size_t n_tiles = (size_t)g.ntx * g.nty * g.nch;
    if (const int rc = dev_buf_reserve(c, cells, n_cells, "cell bytes of the sparse split Jacobian"))
      return rc;
    if (const int rc = dev_buf_reserve(c, flags, n_tiles * sizeof(int), "tile-chunk flags of the sparse split Jacobian"))
      return rc;
    sp = {cells.as<uint8_t>(), flags.as<int>(), c->buf_sparse_rows.as<int>()};
    if ((n_cells && hipMemsetAsync(sp.cell_comp, 0, n_cells, s) != hipSuccess) ||
        (n_tiles && hipMemsetAsync(sp.tile_flag, 0, n_tiles * sizeof(int), s) != hipSuccess))
      return fail(c, PFM_ERR_HIP, "sparse split Jacobian: buffer reset");
    tiles = (int64_t)n_tiles;
    return PFM_OK;
  }

  // Two statuses, here and in launch_levels / gather_hanging: the return value ends the call at once (its text is set);
  // `rc` (in/out) is the status of the launches, which assemble_impl reports behind the joins and the closing event.
  // cartesian box, 2-D / 3-D: the pair with its deferred placeholder patches, the fork, the fill of the (u,phi) block
  int assemble_box(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
  {
    if (p.pair)
      if (const int rcp = ensure_patch_list(c))
        return rcp;
    if (p.fork)
      if (const int rcf = fork_side(c, "fork"))
        return rcf;
    if (!p.residual_only && c->v.dim == 3 && c->scal_dirty)
      {
        // off the hot path: once per pfm_set_params, complete before any kernel of any stream may read it
        int rcs = upload_mat_scal(c->prm, c->cv, c->d_scal, c->stream);
        if (rcs == PFM_OK && hipStreamSynchronize(c->stream) != hipSuccess)
          rcs = PFM_ERR_HIP;
        if (rcs)
          return fail(c, rcs, "scalar tables");
        c->scal_dirty = false;
      }
    if (p.fill_up_block && hipMemsetAsync(d_values[1], 0, sizeof(double) * (size_t)c->block_nnz(1), c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "clear the (u,phi) block");
    pfm::CartView cv = c->cv;
    cv.up_block_cleared = p.up_block_cleared ? 1 : 0;
    if (!p.pair)
      cv.patch_idx = nullptr, cv.patch_val = nullptr, cv.patch_count = nullptr, cv.patch_cap = 0;
    int *n_compressed = nullptr;
    if (p.box.voldev_jac) // counted by the kernel of the (whole or second-half) launch
      if (const int rcc = compressed_counter(c, p.box.split3_jac(), n_compressed))
        return rcc;
    pfm::SplitSparse sparse{};
    const bool run_sparse = p.box.voldev_sparse && p.box.split3_jac();
    if (run_sparse)
      {
        if (const int rcs = sparse_row_counter(c))
          return rcs;
        if (const int rcs = sparse_buffers(c, c->cv, p.box, c->buf_sparse_cells, c->buf_sparse_flags, c->sparse_tiles, c->stream, sparse))
          return rcs;
      }
    pfm::UuKeep keep{};
    if (p.keep_uu)
      if (const int rck = ensure_uu_keep(c, keep))
        return rck;
    rc = launch_assemble_cart(p.box, c->v, cv, c->prm, d_values, d_res_pde, d_res_tot, c->stream, p.fork ? c->side_stream : c->stream,
                              c->d_scal, &c->clock, n_compressed, run_sparse ? &sparse : nullptr, p.keep_uu ? &keep : nullptr);
    if (p.box.split3_jac())
      c->compressed_valid = rc == PFM_OK;
    if (run_sparse)
      c->sparse_valid = rc == PFM_OK, c->sparse_levels = false;
    if (p.fork)
      if (const int rcj = join_from(c, c->side_stream, c->stream, c->ev_join, "join"))
        return rcj;
    if (p.pair && rc == PFM_OK)
      rc = launch_cart_apply_patches(c->cv, d_values[0], c->stream, c->v.status, p.keep_uu ? &keep : nullptr);
    return PFM_OK;
  }

  // The view the launches of the general family take.  classes: for its colour and atomic classes -- the reduced colour
  // lists next to an overlay, and either the atomic adds or the scratch of the cells at hanging vertices, never both.
  pfm::DevView general_view(const pfm_ctx *c, const AssemblyPlan &p, bool classes)
  {
    pfm::DevView vg = c->v;
    if (!p.patches)
      vg.row_patch = nullptr; // no overlay in this assembly: the general family writes every row
    if (!classes)
      return vg;
    if (p.patches)
      vg.color_cells = c->d_color_cells_reduced;
    // gather: the cells at hanging vertices only write their scratch and nobody adds atomically -- unless cells that found
    // no colour sit in the last class next to them (colour_overflow): those add to the outputs with atomics, on the side
    // stream of a Jacobian assembly, so the plain classes keep the ring and add atomically as well
    if (p.gather && !c->colour_overflow)
      vg.cell_ring = nullptr;
    if (!p.gather)
      vg.hs_K = nullptr, vg.hs_off = nullptr, vg.hs_RD = nullptr;
    return vg;
  }

  // behind every class and every level kernel (joined by the caller): the rows the hanging cells reach, in list order
  void gather_hanging(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
  {
    if (p.gather && rc == PFM_OK)
      rc = launch_hanging_gather(general_view(c, p, false), c->prm, p.residual_only, d_values, d_res_pde, d_res_tot, c->d_hg_rows, c->d_hg_ptr,
                                 c->d_hg_list, c->n_hg_rows, c->stream);
  }

  // 3-D overlay: the row-owner kernels on every level lattice, on the context's stream or (plan.levels_concurrent) each
  // level on a stream of its own between a fork and a join
  int launch_levels(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
  {
    const size_t nl = c->levels3.size();
    hipError_t e = hipSuccess;
    for (auto &lv : c->levels3)
      if (rc == PFM_OK && !p.residual_only && lv.scal_dirty)
        {
          rc = upload_mat_scal(c->prm, lv.cv, lv.d_scal, c->stream);
          lv.scal_dirty = rc != PFM_OK;
        }
    // CartPlan::voldev_jac: one counter for all levels, emptied once, in front of the first level and of the fork
    int *n_compressed = nullptr;
    if (p.level.voldev_jac)
      if (const int rcc = compressed_counter(c, true, n_compressed))
        return rcc;
    // CartPlan::voldev_sparse: likewise one row counter; the cell bytes and tile-chunk flags are the level's own (below)
    if (p.level.voldev_sparse)
      if (const int rcs = sparse_row_counter(c))
        return rcs;
    const bool par = p.levels_concurrent && rc == PFM_OK;
    if (par)
      {
        while (c->ov_streams.size() < nl)
          {
            hipStream_t st = nullptr;
            hipEvent_t ev = nullptr;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
              return fail(c, PFM_ERR_HIP, "overlay level stream");
            c->ov_streams.push_back(st);
            c->ov_events.push_back(ev);
          }
        if (!c->ov_fork && hipEventCreateWithFlags(&c->ov_fork, hipEventDisableTiming) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "overlay level event");
        e = hipEventRecord(c->ov_fork, c->stream); // one event, every level stream behind it
        for (size_t i = 0; i < nl && e == hipSuccess; ++i)
          e = hipStreamWaitEvent(c->ov_streams[i], c->ov_fork, 0);
        if (e != hipSuccess)
          return hipfail(c, e, "fork (overlay levels)");
      }
    for (size_t i = 0; i < nl && rc == PFM_OK; ++i)
      {
        hipStream_t st = par ? c->ov_streams[i] : c->stream;
        pfm_ctx::OverlayLevel &lv = c->levels3[i];
        pfm::CartView lcv = lv.cv; // one plan per level lattice
        lcv.up_block_cleared = p.keep_up_block ? 1 : 0;
        const CartPlan lpl = plan_cart(c->v, lcv, c->prm, p.residual_only, 0, cart_n_cu(), cart_split(c));
        pfm::SplitSparse sparse{};
        if (lpl.voldev_sparse) // emptied on the level's stream in front of its mark kernel
          if (const int rcs = sparse_buffers(c, lcv, lpl, lv.buf_sparse_cells, lv.buf_sparse_flags, lv.sparse_tiles, st, sparse))
            return rcs;
        rc = launch_assemble_cart(lpl, c->v, lcv, c->prm, d_values, d_res_pde, d_res_tot, st, st, lv.d_scal, &c->clock, n_compressed,
                                  lpl.voldev_sparse ? &sparse : nullptr);
      }
    if (p.level.voldev_jac)
      c->compressed_valid = rc == PFM_OK;
    if (p.level.voldev_sparse)
      c->sparse_valid = rc == PFM_OK, c->sparse_levels = true;
    for (size_t i = 0; par && i < nl; ++i)
      if (const int rcj = join_from(c, c->ov_streams[i], c->stream, c->ov_events[i], "join (overlay levels)"))
        return rcj;
    return PFM_OK;
  }

  // 2-D patch overlay / 3-D level overlay.  The patch kernel or the level kernels write every regular row once, with plain
  // stores; next to them (side stream) the general family over the cells that touch a non-regular row (it skips the
  // regular ones: DevView::row_patch), its classes one after the other, the atomic class of a 3-D Jacobian on a third stream
  int assemble_overlay(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
  {
    if (p.fork_general)
      if (const int rcf = fork_side(c, "fork (general family)"))
        return rcf;
    if (!p.overlay3)
      rc = launch_assemble_patches(c->v, c->prm, p.residual_only, d_values, d_res_pde, d_res_tot, c->n_patch_blocks, c->stream);
    else if (const int rcl = launch_levels(c, p, d_values, d_res_pde, d_res_tot, rc))
      return rcl;
    hipStream_t s_atomic = nullptr;
    if (p.atomic_stream)
      {
        int prio_lo = 0, prio_hi = 0; // (numerically lower = higher priority) the long pole gets its workgroups dispatched first
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        if (!c->atomic_stream && (hipStreamCreateWithPriority(&c->atomic_stream, hipStreamNonBlocking, prio_hi) != hipSuccess ||
                                  hipEventCreateWithFlags(&c->ev_atomic, hipEventDisableTiming) != hipSuccess))
          return fail(c, PFM_ERR_HIP, "atomic-class stream");
        const hipError_t e = hipStreamWaitEvent(c->atomic_stream, c->ev_fork, 0); // behind the fork of the side stream
        if (e != hipSuccess)
          return hipfail(c, e, "fork (atomic class)");
        s_atomic = c->atomic_stream;
      }
    if (rc == PFM_OK && c->n_general_cells > 0)
      rc = launch_assemble_general(general_view(c, p, true), c->prm, p.residual_only, d_values, d_res_pde, d_res_tot,
                                   p.fork_general ? c->side_stream : c->stream, c->color_ptr_reduced, s_atomic, c->split_model);
    if (s_atomic)
      if (const int rcj = join_from(c, s_atomic, c->stream, c->ev_atomic, "join (atomic class)"))
        return rcj;
    if (p.fork_general)
      if (const int rcj = join_from(c, c->side_stream, c->stream, c->ev_join, "join (general family)"))
        return rcj;
    gather_hanging(c, p, d_values, d_res_pde, d_res_tot, rc);
    return PFM_OK;
  }

  // general family: the colour classes on the context's stream, the atomic class next to them on the side stream, the
  // gather; kernel path 2 puts the cartesian (u,u) kernel on top
  int assemble_general(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
  {
    if (p.fork_general)
      if (const int rcf = fork_side(c, "fork (general family)"))
        return rcf;
    rc = launch_assemble_general(general_view(c, p, true), c->prm, p.residual_only, d_values, d_res_pde, d_res_tot, c->stream, c->color_ptr,
                                 (p.fork_general && !c->hanging_coloured) ? c->side_stream : nullptr, c->split_model);
    if (p.fork_general)
      if (const int rcj = join_from(c, c->side_stream, c->stream, c->ev_join, "join (general family)"))
        return rcj;
    gather_hanging(c, p, d_values, d_res_pde, d_res_tot, rc);
    if (rc == PFM_OK && p.overlay_uu && c->scal_dirty)
      {
        rc = upload_mat_scal(c->prm, c->cv, c->d_scal, c->stream);
        c->scal_dirty = rc != PFM_OK;
      }
    if (rc == PFM_OK && p.overlay_uu)
      {
        CartPlan uu = plan_cart(c->v, c->cv, c->prm, 0, 0, cart_n_cu());
        uu.rows_residual = uu.pair = false; // (the general family has written the residual)
        rc = launch_cart_uu3(uu, c->v, c->cv, c->prm, d_values[0], c->stream, nullptr, &c->clock);
      }
    return PFM_OK;
  }

  // phase 0: the whole assembly (pfm_assemble_device).  phases 1, 2: the two halves of pfm_assemble_overlapped -- 1 = what
  // reads no ghost node, 2 = the rest; timing events bracket 1..2 together.
  int assemble_impl(pfm_ctx *c, int residual_only, double *const *d_values, double *d_res_pde, double *d_res_tot, int phase)
  {
    // a rank may own nothing (empty partition piece): null buffers are fine where there is nothing to write
    const bool no_rows = c && c->n_owned_dofs() == 0;
    if (!c || (!d_res_pde && !no_rows) || (residual_only && !d_res_tot && !no_rows) || (!residual_only && !d_values))
      return PFM_ERR_BAD_ARG;
    if (!c->have_params)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_set_params has not been called");
    (void)hipSetDevice(c->device);
    if (phase != 0) // in front of the plan, whose grids of a second half are those of the lists (pfm_ctx_force_zchunk drops them)
      if (const int rcl = ensure_overlap_lists(c))
        return rcl;
    AssemblyPlan plan = plan_assembly(c, residual_only, phase, d_values);
    if (!residual_only && phase != 1 && !(plan.cart && plan.box.voldev_jac) && !(plan.overlay3 && plan.level.voldev_jac))
      c->compressed_valid = false; // pfm_ctx_split_route_info: the count belongs to the last full assembly
    if (!residual_only && phase != 1 && !(plan.cart && plan.box.voldev_sparse) && !(plan.overlay3 && plan.level.voldev_sparse))
      c->sparse_valid = false; // pfm_ctx_split_sparse_info: likewise
    if (!residual_only && d_values && c->kept_uu_block && d_values[0] == c->kept_uu_block && !plan.keep_uu)
      c->uu_stale_pending = true; // written by a path that does not record what the kept form needs (its patches stay added)
    bool gather_ready = false;
    if (const int rct = ensure_tables(c, plan, gather_ready))
      return rct;
    plan.after_tables(c, gather_ready);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (c->timing && phase == 2)
      ev1 = c->ev_pool[c->ev_used - 1].second; // opened by phase 1
    else if (c->timing)
      if (const int rco = open_interval(c, ev0, ev1))
        return rco;
    if (plan.nothing)
      return PFM_OK;
    if (const int rcz = zero_outputs(c, plan, d_values, d_res_pde, d_res_tot))
      return rcz;
    int rc = PFM_OK; // of the launches
    if (const int rcf = plan.cart      ? assemble_box(c, plan, d_values, d_res_pde, d_res_tot, rc)
                        : plan.patches ? assemble_overlay(c, plan, d_values, d_res_pde, d_res_tot, rc)
                                       : assemble_general(c, plan, d_values, d_res_pde, d_res_tot, rc))
      return rcf;
    if (phase == 1) // the interval stays open for phase 2
      return rc ? fail(c, rc, "assemble launch failed (interior tiles)") : PFM_OK;
    if (ev1)
      (void)hipEventRecord(ev1, c->stream);
    return rc ? fail(c, rc, "assemble launch failed") : PFM_OK;
  }
} // namespace

extern "C"
{
  int pfm_assemble_device(pfm_ctx *c, int residual_only, double *const *d_values, double *d_res_pde, double *d_res_tot)
  {
    if (c && c->force_phase) // measurement: one half of the overlapped assembly alone, bracketed like a whole one
      {
        const bool timing = c->timing;
        c->timing = false;
        hipEvent_t a = nullptr, b = nullptr;
        if (timing)
          if (const int rco = open_interval(c, a, b))
            return rco;
        const int rc = assemble_impl(c, residual_only, d_values, d_res_pde, d_res_tot, c->force_phase);
        if (timing)
          (void)hipEventRecord(b, c->stream);
        c->timing = timing;
        return rc;
      }
    return assemble_impl(c, residual_only, d_values, d_res_pde, d_res_tot, 0);
  }

  // assemble_nl_residual() of the line search (cracks.cc:2942-2957, 2507-2512): solution := d_solution, then the residuals.
  // On a single-rank box (2-D or 3-D lattice) the residual kernel reads d_solution itself (DevView::fused_solution); everywhere else this
  // is pfm_state_set_solution + pfm_assemble_device(residual_only).  Ranks with peers must import ghosts in between: they
  // call the two entry points themselves.
  int pfm_assemble_nl_residual_device(pfm_ctx *c, const double *d_solution, double *d_res_pde, double *d_res_tot)
  {
    if (!c || (!d_solution && c->n_owned_dofs() != 0))
      return PFM_ERR_BAD_ARG;
    if (!c->peers.empty())
      return fail(c, PFM_ERR_BAD_ARG, "pfm_assemble_nl_residual_device: a rank with peers imports ghosts between the scatter and the assembly");
    // (the residual of the box on a row-owner kernel: unsplit, or the split law on the lattice route)
    const bool fuse = c->kernel_path == 1 && (!c->have_params || plan_cart(c->v, c->cv, c->prm, 1, 0, cart_n_cu(), cart_split(c)).supported) &&
                      c->v.n_owned == c->v.n_nodes && c->v.n_owned > 0 && Switches::fused_scatter();
    if (!fuse)
      {
        const int rc = state_set_impl(c, d_solution, nullptr, nullptr, 1);
        return rc ? rc : assemble_impl(c, 1, nullptr, d_res_pde, d_res_tot, 0);
      }
    c->v.fused_solution = d_solution;
    const int rc = assemble_impl(c, 1, nullptr, d_res_pde, d_res_tot, 0);
    c->v.fused_solution = nullptr;
    return rc;
  }

  int pfm_ctx_force_phase(pfm_ctx *c, int phase)
  {
    if (!c || phase < 0 || phase > 2)
      return PFM_ERR_BAD_ARG;
    c->force_phase = phase;
    return phase ? ensure_overlap_lists(c) : PFM_OK;
  }

  int pfm_ctx_force_zchunk(pfm_ctx *c, int kernel, int planes)
  {
    if (!c || kernel < 0 || kernel >= PFM_ZC_KERNELS || planes < 0)
      return PFM_ERR_BAD_ARG;
    c->cv.zc_force[kernel] = planes;
    c->uu_stale_pending = true; // (a kept (u,u) block: written again by the tiles of the new length)
    for (auto &lv : c->levels3)
      lv.cv.zc_force[kernel] = planes;
    if (kernel == PFM_ZC_RES3 && c->overlap_lists_ready)
      drop_overlap_lists(c); // the residual's boundary list is one of chunks of its length (the (u,u) list goes with it)
    return PFM_OK;
  }

  int pfm_ctx_zchunk(const pfm_ctx *c, int kernel, int *planes)
  {
    if (!c || kernel < 0 || kernel >= PFM_ZC_KERNELS || !planes)
      return PFM_ERR_BAD_ARG;
    if (!c->cart_ok || (kernel == PFM_ZC_RES2) != (c->v.dim == 2))
      return PFM_ERR_UNSUPPORTED;
    *planes = cart_zchunk(c->cv, kernel); // the launchers' own geometry, on the context's box
    return PFM_OK;
  }

  // Ghost import NEXT TO the cell work instead of in front of it (cracks.cc:2147-2154 against 2200-2437): after the
  // caller's pfm_state_set, the exchange (pack -> RCCL -> unpack) runs on the context's side stream while the context's
  // stream assembles the tiles that read no ghost node; the stream then waits for the import and assembles the rest.
  int pfm_assemble_overlapped(pfm_ctx *c, void *comm, const int *peer_ranks, int residual_only, double *const *d_values,
                              double *d_res_pde, double *d_res_tot)
  {
    if (!c || (!c->peers.empty() && (!comm || !peer_ranks)))
      return PFM_ERR_BAD_ARG;
    if (c->peers.empty())
      return assemble_impl(c, residual_only, d_values, d_res_pde, d_res_tot, 0);
    (void)hipSetDevice(c->device);
    int rc = ensure_side_stream(c);
    if (rc == PFM_OK)
      rc = ensure_overlap_lists(c);
    // fork behind the state scatter; the pack kernel of the exchange reads the owned node state
    if (rc == PFM_OK)
      rc = fork_to(c, c->stream, c->side_stream, c->ev_fork, "fork");
    if (rc == PFM_OK)
      rc = halo_exchange_on(c, comm, peer_ranks, c->side_stream);
    if (rc)
      return rc;
    // the join in two parts around phase 1, which records neither event again: phase 1 forks nothing
    hipError_t e = hipEventRecord(c->ev_join, c->side_stream);
    if (e != hipSuccess)
      return hipfail(c, e, "join event");
    rc = assemble_impl(c, residual_only, d_values, d_res_pde, d_res_tot, 1); // interior: no ghost node is read
    if (rc)
      return rc;
    e = hipStreamWaitEvent(c->stream, c->ev_join, 0);
    if (e != hipSuccess)
      return hipfail(c, e, "join");
    return assemble_impl(c, residual_only, d_values, d_res_pde, d_res_tot, 2);
  }

  int pfm_timing_enable(pfm_ctx *c, int on)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    c->timing = on != 0;
    c->ev_used = 0;
    return PFM_OK;
  }

  int pfm_kernel_time_ms(pfm_ctx *c, double *mean_ms, int *n_launches)
  {
    if (!c || !mean_ms)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess)
      return hipfail(c, e, "kernel_time sync");
    double sum = 0.0;
    for (size_t k = 0; k < c->ev_used; ++k)
      {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, c->ev_pool[k].first, c->ev_pool[k].second);
        if (e != hipSuccess)
          return hipfail(c, e, "hipEventElapsedTime");
        sum += ms;
      }
    *mean_ms = c->ev_used ? sum / (double)c->ev_used : 0.0;
    if (n_launches)
      *n_launches = (int)c->ev_used;
    c->ev_used = 0;
    return PFM_OK;
  }

  int pfm_kernel_times_ms(pfm_ctx *c, double *ms, int capacity, int *n_launches)
  {
    if (!c || (capacity > 0 && !ms) || capacity < 0)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess)
      return hipfail(c, e, "kernel_times sync");
    const int n = (int)std::min<size_t>(c->ev_used, (size_t)capacity);
    for (int k = 0; k < n; ++k)
      {
        float t = 0.f;
        e = hipEventElapsedTime(&t, c->ev_pool[k].first, c->ev_pool[k].second);
        if (e != hipSuccess)
          return hipfail(c, e, "hipEventElapsedTime");
        ms[k] = t;
      }
    if (n_launches)
      *n_launches = (int)c->ev_used;
    return PFM_OK;
  }

  int pfm_ctx_kernel_path(const pfm_ctx *c) { return c ? c->kernel_path : -1; }

  int pfm_ctx_split_route(const pfm_ctx *c, int *route, int *lattice_residual)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (route)
      *route = c->split_route;
    if (lattice_residual)
      {
        // the plan of such an assembly, not a second copy of its conditions
        *lattice_residual = 0;
        if (c->have_params)
          {
            const AssemblyPlan p = plan_assembly(c, 1, 0, nullptr);
            *lattice_residual = ((p.cart && (p.box.voldev || p.box.spectral)) || (p.overlay3 && (p.level.voldev || p.level.spectral))) ? 1 : 0;
          }
      }
    return PFM_OK;
  }

  int pfm_ctx_split_route_info(const pfm_ctx *c, int64_t out[4])
  {
    if (!c || !out)
      return PFM_ERR_BAD_ARG;
    int lattice_residual = 0;
    (void)pfm_ctx_split_route(c, nullptr, &lattice_residual);
    out[0] = c->split_route;
    out[1] = lattice_residual;
    out[2] = 0;
    out[3] = -1;
    if (c->have_params)
      {
        // the plan of such an assembly, not a second copy of its conditions
        double *const no_values[4] = {nullptr, nullptr, nullptr, nullptr};
        const AssemblyPlan p = plan_assembly(c, 0, 0, no_values);
        out[2] = ((p.cart && p.box.voldev_jac) || (p.overlay3 && p.level.voldev_jac)) ? 1 : 0;
      }
    if (c->compressed_valid && c->buf_compressed.p)
      {
        int n = 0;
        (void)hipSetDevice(c->device);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&n, c->buf_compressed.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
          return PFM_ERR_HIP;
        out[3] = n;
      }
    return PFM_OK;
  }

  int pfm_ctx_split_sparse_info(const pfm_ctx *c, int64_t out[4])
  {
    if (!c || !out)
      return PFM_ERR_BAD_ARG;
    out[0] = 0, out[1] = -1, out[2] = -1, out[3] = 0;
    if (c->have_params)
      {
        // the plan of such an assembly, not a second copy of its conditions
        double *const no_values[4] = {nullptr, nullptr, nullptr, nullptr};
        const AssemblyPlan p = plan_assembly(c, 0, 0, no_values);
        if (p.cart && p.box.voldev_sparse)
          {
            const TileGrid &g = p.box.grid[PFM_ZC_UU3];
            out[0] = 1;
            out[3] = (int64_t)g.ntx * g.nty * g.nch;
          }
        else if (p.overlay3 && p.level.voldev_sparse) // the level lattices of an overlay: summed over the levels
          {
            out[0] = 1;
            for (const auto &lv : c->levels3)
              {
                const TileGrid g = plan_cart(c->v, lv.cv, c->prm, 0, 0, cart_n_cu(), cart_split(c)).grid[PFM_ZC_UU3];
                out[3] += (int64_t)g.ntx * g.nty * g.nch;
              }
          }
      }
    if (c->sparse_valid && c->buf_sparse_rows.p)
      {
        int n = 0;
        (void)hipSetDevice(c->device);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&n, c->buf_sparse_rows.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
          return PFM_ERR_HIP;
        int64_t flagged = 0;
        auto count = [&](const pfm::DevBuf &b, int64_t tiles) {
          std::vector<int> flags((size_t)tiles);
          if (!flags.empty() && (!b.p || hipMemcpy(flags.data(), b.p, flags.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess))
            return false;
          for (const int f : flags)
            flagged += f != 0;
          return true;
        };
        if (!c->sparse_levels && !count(c->buf_sparse_flags, c->sparse_tiles))
          return PFM_ERR_HIP;
        for (size_t i = 0; c->sparse_levels && i < c->levels3.size(); ++i)
          if (!count(c->levels3[i].buf_sparse_flags, c->levels3[i].sparse_tiles))
            return PFM_ERR_HIP;
        out[1] = n;
        out[2] = flagged;
      }
    return PFM_OK;
  }

  int pfm_ctx_hanging_info(const pfm_ctx *c, int *mode, int64_t out[5])
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (mode)
      *mode = c->hang_mode;
    if (!out)
      return PFM_OK;
    out[0] = c->n_hcells;
    out[1] = 0;
    out[2] = c->hang_gather_ready ? c->n_hg_rows : 0;
    out[3] = c->hang_gather_bytes;
    out[4] = 0;
    if (!c->have_params)
      return PFM_OK;
    // the plan of such an assembly and the view its classes would take, not a second copy of their conditions
    double *const no_values[4] = {nullptr, nullptr, nullptr, nullptr};
    const AssemblyPlan p = plan_assembly(c, 0, 0, no_values);
    out[1] = p.gather ? 1 : 0;
    if (p.cart || p.nothing)
      return PFM_OK; // the row-owner kernels: every entry written once
    // floating-point atomic adds: the atomic class (cells at hanging vertices that do not go through the gather, cells that
    // found no colour) and the ring of the plain classes
    const bool atomic_class = (c->n_hcells > 0 && !p.gather && !c->hanging_coloured) || c->colour_overflow;
    out[4] = (atomic_class || general_view(c, p, true).cell_ring != nullptr) ? 1 : 0;
    return PFM_OK;
  }

  int pfm_ctx_force_path(pfm_ctx *c, int path)
  {
    if (c)
      c->uu_stale_pending = true; // a kept (u,u) block is written again by whatever runs next
    if (path == 3 && c && !c->cart_ok && (c->n_patch_blocks > 0 || !c->levels3.empty()))
      {
        c->kernel_path = 3;
        return PFM_OK;
      }
    if (!c || path < 0 || path > 2 || (path >= 1 && !c->cart_ok) || (path == 2 && c->v.dim != 3))
      return PFM_ERR_UNSUPPORTED;
    c->kernel_path = path;
    return PFM_OK;
  }

  int pfm_ctx_overlay_info(const pfm_ctx *c, int64_t *n_patch_rows, int64_t *n_general_cells)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (n_patch_rows)
      *n_patch_rows = (c->n_patch_blocks > 0 || !c->levels3.empty()) ? c->n_patch_rows : 0;
    if (n_general_cells)
      *n_general_cells = (c->n_patch_blocks > 0 || !c->levels3.empty()) ? c->n_general_cells : c->v.n_cells;
    return PFM_OK;
  }

  int64_t pfm_ctx_device_bytes(const pfm_ctx *c) { return c ? c->device_bytes : 0; }
}
