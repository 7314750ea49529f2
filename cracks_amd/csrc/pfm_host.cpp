// pfm_host.cpp -- what a caller does to a living context (include/pfm_assemble.h): destroy, stream, parameters, split
// law and route, hanging mode, constraints, the kept (u,phi) block, pattern queries and pfm_pattern_bind, the node state,
// the gather tables of the cells at hanging vertices, the status word.
#include "pfm_host.h"
#include "pfm_host_pool.h"
#include "pfm_mesh_plan.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

using namespace pfm;

int64_t pfm_ctx::block_rows(int b) const
{
  const int dim = v.dim;
  if (v.layout == PFM_LAYOUT_INTERLEAVED)
    return (int64_t)v.n_owned * (dim + 1);
  return (b == 0 || b == 1) ? (int64_t)v.n_owned * dim : (int64_t)v.n_owned;
}

int64_t pfm_ctx::block_nnz(int b) const
{
  const int dim = v.dim;
  const int64_t g = nadj_total >= 0 ? (int64_t)nadj_total : (h_nadj_ptr.empty() ? 0 : (int64_t)h_nadj_ptr.back());
  if (v.layout == PFM_LAYOUT_INTERLEAVED)
    return g * (dim + 1) * (dim + 1);
  switch (b)
    {
      case 0:
        return g * dim * dim;
      case 1:
      case 2:
        return g * dim;
      default:
        return g;
    }
}

namespace
{
  // Adopt the caller's CSR pattern of one block.  The pattern must be the canonical one up to the order of the
  // entries within a row, and that order must keep the structure (node, component): the ncc column components of a
  // neighbour node adjacent and ascending -- what any CSR sorted by local column id has.  The node order of the rows
  // becomes the order of the context's node graph: every kernel family addresses values through it.
  int pattern_bind_impl(pfm_ctx *c, int block, const int64_t *rp64, const int32_t *rp32, const int32_t *colind)
  {
    if (!c || block < 0 || block >= c->n_blocks || (!rp64 && !rp32) || !colind)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    c->delta.valid = false; // the values move to other slots: what the host holds is not what the shadow describes
    c->uu_stale_pending = true; // ... and a kept (u,u) block is written again
    const int dim = c->v.dim;
    int ncr, ncc;
    if (c->v.layout == PFM_LAYOUT_INTERLEAVED)
      ncr = ncc = dim + 1;
    else
      {
        ncr = (block == 0 || block == 1) ? dim : 1;
        ncc = (block == 0 || block == 2) ? dim : 1;
      }
    const int32_t NO = c->v.n_owned;
    auto rp = [&](int64_t r) -> int64_t { return rp64 ? rp64[r] : (int64_t)rp32[r]; };
    if (rp(0) != 0 || rp(c->block_rows(block)) != c->block_nnz(block))
      return fail(c, PFM_ERR_BAD_ARG, "pfm_pattern_bind: row pointers do not describe this block (size mismatch)");
    if (const int rcg = guarded(c, [&] { ensure_host_graph(c); }))
      return rcg;
    std::vector<int32_t> order(c->h_nadj.size());
    std::atomic<int> bad{0}; // 1: structure, 2: column set
    std::atomic<bool> changed{false};
    parallel_for(NO, [&](int64_t nb, int64_t ne) {
      std::vector<int32_t> a, b;
      for (int64_t n = nb; n < ne && !bad; ++n)
        {
          const long long off = c->h_nadj_ptr[n];
          const int deg = (int)(c->h_nadj_ptr[n + 1] - off);
          for (int ci = 0; ci < ncr; ++ci)
            {
              const int64_t r = n * ncr + ci, b0 = rp(r);
              if (rp(r + 1) - b0 != (int64_t)deg * ncc)
                {
                  bad = 1;
                  return;
                }
              for (int sl = 0; sl < deg; ++sl)
                {
                  const int32_t col0 = colind[b0 + (int64_t)sl * ncc];
                  const int32_t q = col0 / ncc;
                  for (int d = 0; d < ncc; ++d)
                    if (colind[b0 + (int64_t)sl * ncc + d] != q * ncc + d)
                      {
                        bad = 1;
                        return;
                      }
                  if (ci == 0)
                    order[off + sl] = q;
                  else if (order[off + sl] != q)
                    {
                      bad = 1;
                      return;
                    }
                }
            }
          a.assign(order.begin() + off, order.begin() + off + deg);
          b.assign(c->h_nadj.begin() + off, c->h_nadj.begin() + off + deg);
          if (a != b)
            {
              changed = true;
              std::sort(a.begin(), a.end());
              std::sort(b.begin(), b.end());
              if (a != b)
                {
                  bad = 2;
                  return;
                }
            }
        }
    });
    if (bad == 1)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_pattern_bind: rows must keep the (node, component) structure of the canonical pattern");
    if (bad == 2)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_pattern_bind: a row couples other nodes than the mesh does (see pfm_pattern_get)");
    if (changed)
      {
        for (int b = 0; b < c->n_blocks; ++b)
          if (b != block && c->pattern_bound[b])
            return fail(c, PFM_ERR_UNSUPPORTED, "pfm_pattern_bind: all blocks must order the neighbour nodes of a row alike");
        const int rcb = guarded(c, [&]() -> int {
          c->h_nadj.swap(order);
          if (c->general_ready) // else: built from the new order when the general family is first used
            {
              if (!c->h_nadj.empty() &&
                  hipMemcpy(const_cast<int32_t *>(c->v.nadj), c->h_nadj.data(), c->h_nadj.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
                throw HipFail{hipGetLastError(), "hipMemcpy nadj"};
              c->patch_slots_valid = false; // the regular rows' slots follow the bound order
              c->overlay3_rows_valid = false;
              if (launch_build_cslot(c->v, nullptr) != PFM_OK || hipDeviceSynchronize() != hipSuccess)
                throw HipFail{hipGetLastError(), "cslot kernel"};
            }
          if (c->cart_ok)
            {
              std::vector<uint32_t> mask;
              std::vector<uint8_t> perm;
              bool any_perm = false;
              if (!row_order_tables(c, dim, NO, c->lat, mask, perm, any_perm))
                return fail(c, PFM_ERR_BAD_ARG, "pfm_pattern_bind: lattice rows inconsistent");
              upload_row_tables(c, mask, perm, any_perm);
            }
          return PFM_OK;
        });
        if (rcb)
          return rcb;
      }
    c->pattern_bound[block] = true;
    return PFM_OK;
  }
} // namespace

namespace pfm
{
  // sol / old / oldold -> node state; old == oldold == nullptr: solution only (pfm_state_set_solution)
  int state_set_impl(pfm_ctx *c, const double *sol, const double *old, const double *oldold, int on_device)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (c->n_owned_dofs() == 0)
      return PFM_OK; // a rank that owns nothing: its node state comes from the ghost import alone
    const bool sol_only = !old && !oldold;
    if (!sol || (!sol_only && (!old || !oldold)))
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    const int nvec = sol_only ? 1 : 3;
    const double *src[3] = {sol, old, oldold};
    const double *d[3] = {sol, old, oldold};
    if (!on_device)
      {
        const size_t bytes = sizeof(double) * (size_t)c->n_owned_dofs();
        for (int k = 0; k < nvec; ++k)
          {
            if (!c->d_stage_vec[k])
              {
                hipError_t e = hipMalloc((void **)&c->d_stage_vec[k], std::max<size_t>(bytes, 8));
                if (e != hipSuccess)
                  return hipfail(c, e, "hipMalloc stage");
                c->device_bytes += (int64_t)bytes;
              }
            hipError_t e = h2d_user(c, c->d_stage_vec[k], src[k], bytes, c->stream);
            if (e != hipSuccess)
              return hipfail(c, e, "state H2D");
            d[k] = c->d_stage_vec[k];
          }
      }
    int rc = launch_state_set(c->v, d[0], d[1], d[2], c->stream, c->uu_words);
    if (rc)
      return fail(c, rc, "state_set launch failed");
    if (!on_device)
      {
        hipError_t e = hipStreamSynchronize(c->stream); // host buffers are borrowed
        if (e != hipSuccess)
          return hipfail(c, e, "state sync");
      }
    return PFM_OK;
  }

  // Gather tables and scratch of the cells at hanging vertices (DevView::hs_*, pfm_ctx::d_hg_*), from the records of
  // DevView::cres (built on the device): every (cell, resolved node) and (cell, hanging vertex) pair is listed under its
  // destination row, rows ascending, the entries of a row in ascending (cell, index) order -- the order k_hanging_gather adds in.
  // false: some cell has more than 16 resolved nodes (no record): the context keeps the atomic class.
  bool ensure_hang_gather(pfm_ctx *c)
  {
    if (c->hang_gather_ready)
      return true;
    if (c->hang_gather_failed || !c->v.cres || c->n_hcells == 0)
      return false;
    (void)hipSetDevice(c->device);
    const int64_t nh = c->n_hcells;
    pfm::raw_vector<uint8_t> rec((size_t)nh * pfm::PFM_CRES_BYTES);
    if (hipMemcpy(rec.data(), c->v.cres, rec.size(), hipMemcpyDeviceToHost) != hipSuccess)
      throw HipFail{hipGetLastError(), "cres D2H"};
    const int dim = c->v.dim, kcmp = dim * dim + dim + 1; // Kuu dim x dim, Kpu dim, Kpp
    pfm::HangGatherLists L;
    if (!pfm::hang_gather_lists(rec.data(), nh, 1 << dim, kcmp, c->v.n_owned, L))
      {
        c->hang_gather = false;
        c->hang_gather_failed = true;
        return false;
      }
    const int64_t bytes0 = c->device_bytes;
    c->n_hg_rows = (int64_t)L.rows.size();
    if (L.rows.empty())
      L.rows.push_back(0);
    if (L.list.empty())
      L.list.push_back(pfm::HgEntry{0, 0, 0});
    c->d_hg_rows = dev_upload(c, L.rows.data(), L.rows.size());
    c->d_hg_ptr = dev_upload(c, L.ptr.data(), L.ptr.size());
    c->d_hg_list = dev_upload(c, L.list.data(), L.list.size());
    c->v.hs_off = dev_upload(c, L.off.data(), L.off.size());
    c->v.hs_K = dev_alloc<double>(c, (size_t)std::max<long long>(L.off.back(), 1));
    c->v.hs_RD = dev_alloc<double>(c, (size_t)nh * pfm::PFM_HS_RD);
    c->hang_gather_bytes = c->device_bytes - bytes0;
    c->hang_gather_ready = true;
    return true;
  }
} // namespace pfm

extern "C"
{
  int pfm_ctx_destroy(pfm_ctx *c)
  {
    if (!c)
      return PFM_OK;
    (void)hipSetDevice(c->device); // a failure surfaces in the next call on the stream
    (void)hipDeviceSynchronize(); // nothing of this context may still be running when its buffers go
    for (void *p : c->allocs)
      (void)hipFree(p);
    for (auto &p : c->peers)
      {
        if (p.d_send)
          (void)hipFree(p.d_send);
        if (p.d_recv)
          (void)hipFree(p.d_recv);
      }
    for (void *q : {(void *)c->d_send_all, (void *)c->d_recv_all, (void *)c->d_send_ptr, (void *)c->d_recv_ptr,
                    (void *)c->d_halo_send, (void *)c->d_halo_recv, (void *)c->cv.patch_idx, (void *)c->cv.patch_val,
                    (void *)c->cv.patch_count, (void *)c->uu_words, (void *)c->uu_saved_idx, (void *)c->uu_saved_val,
                    (void *)c->uu_saved_count})
      if (q)
        (void)hipFree(q);
    if (c->atomic_stream)
      (void)hipStreamDestroy(c->atomic_stream);
    if (c->ev_atomic)
      (void)hipEventDestroy(c->ev_atomic);
    for (hipStream_t st : c->ov_streams)
      (void)hipStreamDestroy(st);
    for (hipEvent_t ev : c->ov_events)
      (void)hipEventDestroy(ev);
    if (c->ov_fork)
      (void)hipEventDestroy(c->ov_fork);
    if (c->side_stream)
      {
        (void)hipStreamDestroy(c->side_stream);
        (void)hipEventDestroy(c->ev_fork);
        (void)hipEventDestroy(c->ev_join);
      }
    for (auto &ev : c->ev_pool)
      {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
      }
    for (auto &hp : c->host_pins) // the arrays belong to the caller; only the page lock is ours
      (void)hipHostUnregister(hp.p);
    if (c->copy_stream)
      {
        (void)hipStreamDestroy(c->copy_stream);
        (void)hipEventDestroy(c->ev_copy);
      }
    delta_release(c); // (its device buffers were in allocs)
    for (double *p : c->d_stage_vec)
      if (p)
        (void)hipFree(p);
    for (double *p : c->d_stage_res)
      if (p)
        (void)hipFree(p);
    for (double *p : c->d_stage_val)
      if (p)
        (void)hipFree(p);
    delete c;
    return PFM_OK;
  }

  const char *pfm_last_error(const pfm_ctx *c) { return c ? c->err.c_str() : "null context"; }

  int pfm_ctx_set_stream(pfm_ctx *c, void *s)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    c->stream = static_cast<hipStream_t>(s);
    return PFM_OK;
  }

  // The kept (u,phi) block (include/pfm_assemble.h; plan_assembly decides per call whether d_values[1] is it).  Off the hot
  // path: the fill is complete on return, so no later pfm_ctx_set_stream can put an assembly in front of it.
  int pfm_values_keep_up_block(pfm_ctx *c, double *d_values_up)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (c->n_blocks != 4)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_values_keep_up_block: the interleaved layout has no (u,phi) block of its own");
    if (!d_values_up)
      {
        c->kept_up_block = nullptr;
        return PFM_OK;
      }
    if (c->block_nnz(1) <= 0)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_values_keep_up_block: the (u,phi) block is empty");
    c->kept_up_block = nullptr; // no promise while the array is not known to be clear
    (void)hipSetDevice(c->device);
    hipError_t e = hipMemsetAsync(d_values_up, 0, sizeof(double) * (size_t)c->block_nnz(1), c->stream);
    if (e == hipSuccess)
      e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess)
      return hipfail(c, e, "pfm_values_keep_up_block");
    c->kept_up_block = d_values_up;
    return PFM_OK;
  }

  int pfm_values_up_block_kept(const pfm_ctx *c, const double **d_values_up)
  {
    if (!c || !d_values_up)
      return PFM_ERR_BAD_ARG;
    *d_values_up = c->kept_up_block;
    return PFM_OK;
  }

  // The kept (u,u) block (include/pfm_assemble.h; plan_assembly decides per call whether d_values[0] is it and whether the
  // promise applies).  Nothing is cleared: the block counts as stale until an assembly has written it.
  int pfm_values_keep_uu_block(pfm_ctx *c, double *d_values_uu)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    if (c->n_blocks != 4)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_values_keep_uu_block: the interleaved layout has no (u,u) block of its own");
    c->kept_uu_block = nullptr;
    c->uu_stale_pending = true;
    if (!d_values_uu)
      return PFM_OK;
    if (c->block_nnz(0) <= 0)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_values_keep_uu_block: the (u,u) block is empty");
    if (!c->uu_words)
      {
        (void)hipSetDevice(c->device);
        if (hipMalloc((void **)&c->uu_words, 2 * sizeof(int)) != hipSuccess)
          return fail(c, PFM_ERR_NOMEM, "hipMalloc device words of the kept (u,u) block");
        c->device_bytes += 2 * (int64_t)sizeof(int);
        const int init[2] = {1, 0};
        if (hipMemcpy(c->uu_words, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "pfm_values_keep_uu_block");
      }
    c->kept_uu_block = d_values_uu;
    return PFM_OK;
  }

  int pfm_values_uu_block_kept(const pfm_ctx *c, const double **d_values_uu)
  {
    if (!c || !d_values_uu)
      return PFM_ERR_BAD_ARG;
    *d_values_uu = c->kept_uu_block;
    return PFM_OK;
  }

  int pfm_set_params(pfm_ctx *c, const pfm_params *p)
  {
    if (!c || !p)
      return PFM_ERR_BAD_ARG;
    // the reference gates the split on decompose_stress_matrix alone (cracks.cc:2294): decompose_stress_rhs > 0
    // without it multiplies a zero stress_term_minus, i.e. is a plain assembly and valid in 3-D
    // (pfm_set_split_model: PFM_SPLIT_SPECTRAL and PFM_SPLIT_VOLDEV are the 3-D laws of pfm_split3.h)
    if (c->v.dim == 3 && c->split_model == PFM_SPLIT_REFERENCE && p->decompose_stress_matrix > 0 && p->timestep_number > 0)
      return fail(c, PFM_ERR_UNSUPPORTED,
                  "stress split is 2-D only in the reference (cracks.cc:1685-1690)");
    if (!c->have_params || memcmp(&c->prm, p, sizeof(pfm_params)) != 0)
      c->uu_stale_pending = true; // a kept (u,u) block (pfm_values_keep_uu_block) follows the parameters, byte by byte
    c->prm = *p;
    c->have_params = true;
    c->scal_dirty = true; // the per-launch scalar tables of the cartesian Jacobian kernels follow the parameters
    for (auto &lv : c->levels3)
      lv.scal_dirty = true;
    return PFM_OK;
  }

  int pfm_set_split_model(pfm_ctx *c, int model)
  {
    if (!c || (model != PFM_SPLIT_REFERENCE && model != PFM_SPLIT_SPECTRAL && model != PFM_SPLIT_VOLDEV))
      return c ? fail(c, PFM_ERR_BAD_ARG, "unknown split model") : PFM_ERR_BAD_ARG;
    if (model == PFM_SPLIT_SPECTRAL && c->v.dim != 3)
      return fail(c, PFM_ERR_UNSUPPORTED, "the spectral split is the 3-D law; 2-D keeps the reference's closed form");
    if (model == PFM_SPLIT_VOLDEV && c->v.dim != 3)
      return fail(c, PFM_ERR_UNSUPPORTED, "the volumetric-deviatoric split is a 3-D law; 2-D keeps the reference's closed form");
    c->split_model = model;
    c->uu_stale_pending = true;
    return PFM_OK;
  }

  int pfm_set_split_route(pfm_ctx *c, int route)
  {
    if (!c || (route != PFM_SPLIT_ROUTE_GENERAL && route != PFM_SPLIT_ROUTE_LATTICE && route != PFM_SPLIT_ROUTE_LATTICE_ANY &&
               route != PFM_SPLIT_ROUTE_LATTICE_JACOBIAN && route != PFM_SPLIT_ROUTE_LATTICE_ALL &&
               route != PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS && route != PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS &&
               route != PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE && route != PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE &&
               route != PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE && route != PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE))
      return c ? fail(c, PFM_ERR_BAD_ARG, "unknown split route") : PFM_ERR_BAD_ARG;
    if (route != PFM_SPLIT_ROUTE_GENERAL && c->v.dim != 3)
      return fail(c, PFM_ERR_UNSUPPORTED, "the lattice routes carry the 3-D split laws");
    c->split_route = route;
    c->uu_stale_pending = true;
    return PFM_OK;
  }

  int pfm_set_hanging_mode(pfm_ctx *c, int mode)
  {
    if (!c || (mode != PFM_HANGING_MODE_DEFAULT && mode != PFM_HANGING_MODE_GATHER && mode != PFM_HANGING_MODE_ATOMIC))
      return c ? fail(c, PFM_ERR_BAD_ARG, "unknown hanging mode") : PFM_ERR_BAD_ARG;
    if (mode == PFM_HANGING_MODE_GATHER && c->hanging_coloured)
      return fail(c, PFM_ERR_UNSUPPORTED, "PFM_HANGING_COLOURED=1: the cells at hanging vertices sit in the colour classes");
    c->hang_mode = mode;
    return PFM_OK;
  }

  int pfm_set_constraints(pfm_ctx *c, const uint8_t *node_flags)
  {
    if (!c || !node_flags)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipError_t e = h2d_user(c, const_cast<uint8_t *>(c->v.node_flags), node_flags, (size_t)c->v.n_nodes, c->stream);
    // capacity of the deferred patch list of the cartesian 3-D Jacobian (counted while the copy is in flight)
    if (c->cart_ok && c->v.dim == 3)
      {
        std::atomic<int64_t> nf{0};
        // a kept (u,u) block follows the displacement bits alone: the phase-field bit changes at every active-set update
        // (k_active_set writes no other bit), so the bits of the last call are what the device holds
        const bool first = c->h_flags_u.size() != (size_t)c->v.n_nodes;
        if (first)
          c->h_flags_u.assign((size_t)c->v.n_nodes, 0);
        std::atomic<bool> changed{first};
        uint8_t *const last = c->h_flags_u.data();
        parallel_for(c->v.n_nodes, [&](int64_t nb, int64_t ne) {
          int64_t k = 0;
          bool diff = false;
          for (int64_t n = nb; n < ne; ++n)
            {
              const uint8_t f = node_flags[n] & 7u;
              if (n < c->v.n_owned)
                k += __builtin_popcount(f);
              diff |= f != last[n];
              last[n] = f;
            }
          nf += k;
          if (diff)
            changed = true;
        });
        c->n_flag_u = nf;
        if (changed)
          c->uu_stale_pending = true;
      }
    else
      c->uu_stale_pending = true;
    if (e == hipSuccess)
      e = hipStreamSynchronize(c->stream); // node_flags is a borrowed host buffer
    return e == hipSuccess ? PFM_OK : hipfail(c, e, "set_constraints copy");
  }

  int pfm_pattern_size(const pfm_ctx *c, int block, int64_t *n_rows, int64_t *nnz)
  {
    if (!c || block < 0 || block >= c->n_blocks)
      return PFM_ERR_BAD_ARG;
    if (n_rows)
      *n_rows = c->block_rows(block);
    if (nnz)
      *nnz = c->block_nnz(block);
    return PFM_OK;
  }

  int pfm_pattern_get(const pfm_ctx *c, int block, int64_t *rowptr, int32_t *colind)
  {
    if (!c || block < 0 || block >= c->n_blocks || !rowptr || !colind)
      return PFM_ERR_BAD_ARG;
    const int dim = c->v.dim;
    int ncr, ncc, coff = 0; // components per node in the row / column space of this block
    bool phi_col = false;
    if (c->v.layout == PFM_LAYOUT_INTERLEAVED)
      ncr = ncc = dim + 1;
    else
      {
        ncr = (block == 0 || block == 1) ? dim : 1;
        ncc = (block == 0 || block == 2) ? dim : 1;
        phi_col = (ncc == 1);
      }
    (void)coff;
    (void)phi_col;
    try
      {
        ensure_host_graph(const_cast<pfm_ctx *>(c)); // a cache: the pattern itself does not change
      }
    catch (const std::bad_alloc &)
      {
        return PFM_ERR_NOMEM;
      }
    catch (const HipFail &)
      {
        return PFM_ERR_HIP;
      }
    int64_t pos = 0, row = 0;
    rowptr[0] = 0;
    for (int32_t n = 0; n < c->v.n_owned; ++n)
      {
        const long long b = c->h_nadj_ptr[n], e = c->h_nadj_ptr[n + 1];
        for (int ci = 0; ci < ncr; ++ci)
          {
            for (long long k = b; k < e; ++k)
              for (int d = 0; d < ncc; ++d)
                colind[pos++] = c->h_nadj[k] * ncc + d;
            rowptr[++row] = pos;
          }
      }
    return PFM_OK;
  }

  int pfm_pattern_bind(pfm_ctx *c, int block, const int64_t *rowptr, const int32_t *colind)
  {
    return pattern_bind_impl(c, block, rowptr, nullptr, colind);
  }

  int pfm_pattern_bind_i32(pfm_ctx *c, int block, const int32_t *rowptr, const int32_t *colind)
  {
    return pattern_bind_impl(c, block, nullptr, rowptr, colind);
  }

  int pfm_state_set(pfm_ctx *c, const double *sol, const double *old, const double *oldold, int on_device)
  {
    if (!c || (c->n_owned_dofs() != 0 && (!old || !oldold)))
      return PFM_ERR_BAD_ARG;
    return state_set_impl(c, sol, old, oldold, on_device);
  }

  int pfm_state_set_solution(pfm_ctx *c, const double *sol, int on_device) { return state_set_impl(c, sol, nullptr, nullptr, on_device); }

  int pfm_sync_status(pfm_ctx *c)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    int st = 0;
    hipError_t e = hipMemcpyAsync(&st, c->v.status, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
      e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess)
      return hipfail(c, e, "sync_status");
    if (st != 0)
      {
        (void)hipMemsetAsync(c->v.status, 0, sizeof(int), c->stream);
        return fail(c, st, st == PFM_ERR_NOT_ORTHOGONAL ? "eigenvectors not orthogonal (cracks.cc:1732-1736)"
                           : st == PFM_ERR_NONFINITE    ? "non-finite value (pfm_check_finite)"
                                                        : "device-side error");
      }
    return PFM_OK;
  }

  int pfm_check_finite(pfm_ctx *c, const double *d_data, int64_t n)
  {
    if (!c || n < 0 || (n > 0 && !d_data))
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    const int rc = launch_check_finite(c->v, d_data, n, c->stream);
    if (rc)
      return fail(c, rc, "check_finite launch failed");
    return pfm_sync_status(c);
  }
}
