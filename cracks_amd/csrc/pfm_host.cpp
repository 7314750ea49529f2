// pfm_host.cpp — host side of the C ABI (include/pfm_assemble.h): context build
// (node graph, CSR addressing tables, device mirrors), pattern queries, state upload,
// halo registration and the synchronous host-pointer entry point.
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
#include "pfm_internal.h"
#include "../../include/pfm_newton.h"
#include "pfm_cart_plan.h"
#include "pfm_host_pool.h"
#include "pfm_mesh_plan.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // types and constants only: the entry points are bound with dlopen (rccl() below)
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <exception>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <mutex>
#include <thread>
#include <execinfo.h>
#include <fcntl.h>
#include <csignal>
#include <unistd.h>
#include <cstdlib>
#include <chrono>

using namespace pfm;

namespace
{
  struct HipFail
  {
    hipError_t e;
    const char *what;
  };

  template <class T>
  T *dev_alloc(pfm_ctx *c, size_t n)
  {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess)
      throw HipFail{e, "hipMalloc"};
    c->allocs.push_back(p);
    c->device_bytes += (int64_t)bytes;
    return static_cast<T *>(p);
  }


  int fail(pfm_ctx *c, int code, const std::string &msg)
  {
    if (c)
      c->err = msg;
    return code;
  }

  int hipfail(pfm_ctx *c, hipError_t e, const char *what)
  {
    return fail(c, PFM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }

  // f() behind the C ABI: what dev_alloc / dev_upload and the lazy table builders throw becomes the call's status
  // (f returns nothing, or a status)
  template <class F>
  int guarded(pfm_ctx *c, F &&f)
  {
    try
      {
        if constexpr (std::is_void<decltype(f())>::value)
          return f(), PFM_OK;
        else
          return f();
      }
    catch (const HipFail &x)
      {
        return hipfail(c, x.e, x.what);
      }
    catch (const std::bad_alloc &)
      {
        return fail(c, PFM_ERR_NOMEM, "host allocation failed");
      }
  }

  // Host -> device copy of caller-owned (pageable) memory.  hipMemcpy from pageable memory ran at ~3.6 GB/s on the
  // test box; tables from 256 KB go through two pinned staging buffers filled by the host threads (parallel memcpy) while
  // the previous piece is on the bus.  On return the caller's buffer has been read.  The copy itself is complete as well,
  // unless the calling thread is inside an H2dBatch scope (pfm_ctx_create: some twenty uploads, one synchronisation at the
  // end, 0.1-0.3 ms each otherwise): then it is ordered on the null stream like a hipMemcpyAsync from pinned memory.
  thread_local int g_h2d_batch = 0;
  struct H2dBatch
  {
    H2dBatch() { ++g_h2d_batch; }
    ~H2dBatch() { --g_h2d_batch; }
  };
  struct Stage // two pinned buffers per device: the events belong to the device that was current when they were made
  {
    static constexpr size_t CHUNK = 32u << 20;
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    int next = 0;
    bool ok = false, tried = false;
    ~Stage()
    {
      for (int i = 0; i < 2; ++i)
        {
          if (pending[i])
            (void)hipEventSynchronize(ev[i]);
          if (buf[i])
            (void)hipHostFree(buf[i]);
          if (ev[i])
            (void)hipEventDestroy(ev[i]);
        }
    }
  };
  std::mutex g_stage_mx; // one transfer at a time goes through the staging buffers (pfm_ctx_create uploads on a second thread)
  Stage g_stages[16];
  Stage *stage_of_current_device() // call with g_stage_mx held; nullptr: no pinned memory to be had
  {
    int dev = 0;
    (void)hipGetDevice(&dev);
    Stage &st = g_stages[dev & 15];
    if (!st.tried)
      {
        st.tried = true;
        st.ok = hipHostMalloc(&st.buf[0], Stage::CHUNK, hipHostMallocPortable) == hipSuccess &&
                hipHostMalloc(&st.buf[1], Stage::CHUNK, hipHostMallocPortable) == hipSuccess &&
                hipEventCreateWithFlags(&st.ev[0], hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&st.ev[1], hipEventDisableTiming) == hipSuccess;
      }
    return st.ok ? &st : nullptr;
  }
  hipError_t h2d(void *d, const void *h, size_t bytes)
  {
    if (bytes < (256u << 10))
      return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    std::lock_guard<std::mutex> stage_lock(g_stage_mx);
    Stage *stp = stage_of_current_device();
    if (!stp)
      return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    Stage &st = *stp;
    // pieces: a table of a few MB in two halves (the second is copied to the staging buffer while the first is on the bus)
    const size_t piece = bytes <= (1u << 20) ? bytes : std::min(Stage::CHUNK, ((bytes + 1) / 2 + 4095) & ~(size_t)4095);
    for (size_t off = 0; off < bytes; off += piece)
      {
        const int k = st.next;
        st.next ^= 1;
        const size_t nb = std::min(piece, bytes - off);
        if (st.pending[k])
          {
            st.pending[k] = false;
            const hipError_t e = hipEventSynchronize(st.ev[k]);
            if (e != hipSuccess)
              return e;
          }
        const char *src = static_cast<const char *>(h) + off;
        char *dst = static_cast<char *>(st.buf[k]);
        parallel_for((int64_t)nb, [&](int64_t b, int64_t e) { memcpy(dst + b, src + b, (size_t)(e - b)); }, 1 << 18);
        hipError_t e = hipMemcpyAsync(static_cast<char *>(d) + off, st.buf[k], nb, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess)
          e = hipEventRecord(st.ev[k], nullptr);
        if (e != hipSuccess)
          return e;
        st.pending[k] = true;
      }
    return g_h2d_batch > 0 ? hipSuccess : hipStreamSynchronize(nullptr);
  }

  // Device -> host copy into pageable memory of the caller through the same buffers, ordered behind the work on `s`,
  // complete on return (results the host reads right after a call: residual vectors, small matrices).
  hipError_t d2h_staged(void *h, const void *d, size_t bytes, hipStream_t s)
  {
    std::lock_guard<std::mutex> stage_lock(g_stage_mx);
    Stage *stp = stage_of_current_device();
    if (!stp)
      {
        const hipError_t e = hipStreamSynchronize(s);
        return e != hipSuccess ? e : hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost);
      }
    Stage &st = *stp;
    for (int k = 0; k < 2; ++k)
      if (st.pending[k])
        {
          st.pending[k] = false;
          const hipError_t e = hipEventSynchronize(st.ev[k]);
          if (e != hipSuccess)
            return e;
        }
    const size_t piece = Stage::CHUNK;
    size_t prev_off = 0, prev_nb = 0;
    int prev_k = -1;
    auto land = [&]() -> hipError_t { // the previous piece: wait for it, hand it to the caller's buffer
      if (prev_k < 0)
        return hipSuccess;
      const hipError_t e = hipEventSynchronize(st.ev[prev_k]);
      if (e != hipSuccess)
        return e;
      const char *src = static_cast<const char *>(st.buf[prev_k]);
      char *dst = static_cast<char *>(h) + prev_off;
      parallel_for((int64_t)prev_nb, [&](int64_t b, int64_t e2) { memcpy(dst + b, src + b, (size_t)(e2 - b)); }, 1 << 18);
      prev_k = -1;
      return hipSuccess;
    };
    for (size_t off = 0; off < bytes; off += piece)
      {
        const int k = st.next;
        st.next ^= 1;
        const size_t nb = std::min(piece, bytes - off);
        hipError_t e = hipMemcpyAsync(st.buf[k], static_cast<const char *>(d) + off, nb, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
          e = hipEventRecord(st.ev[k], s);
        if (e == hipSuccess)
          e = land();
        if (e != hipSuccess)
          return e;
        prev_k = k, prev_off = off, prev_nb = nb;
      }
    return land();
  }

  template <class T>
  T *dev_upload(pfm_ctx *c, const T *h, size_t n)
  {
    T *d = dev_alloc<T>(c, n);
    if (n)
      {
        hipError_t e = h2d(d, h, n * sizeof(T));
        if (e != hipSuccess)
          throw HipFail{e, "hipMemcpy H2D"};
      }
    return d;
  }

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
} // namespace

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

} // namespace

namespace
{
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
                    (void *)c->cv.patch_count})
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

  static pfm_ctx::HostPin *find_pin(pfm_ctx *c, const void *p, size_t bytes);

  // Host -> device copy of a buffer the CALLER owns.  Page-locked through pfm_host_register: an asynchronous DMA on `s`.
  // Anything else goes through the library's own staging buffers (h2d) and is complete on return: the runtime's path for
  // pageable memory pins the caller's pages on the fly, and on this stack that faulted intermittently ("Memory access fault by
  // GPU ... on address <host heap>") when such pages had been registered and unregistered before (tests/test_gpu_cart.py's
  // host-pointer cases followed by the 216^3 test).
  static hipError_t h2d_user(pfm_ctx *c, void *d, const void *h, size_t bytes, hipStream_t s)
  {
    if (bytes == 0)
      return hipSuccess;
    if (find_pin(c, h, bytes))
      return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s);
    // the staged copy runs on the NULL stream, which does not order itself behind a hipStreamNonBlocking stream installed
    // through pfm_ctx_set_stream (torch side streams are of that kind): kernels still queued on `s` may read what this copy
    // overwrites (node_flags of an assembly in flight, the staging vectors of the last state) -- wait for them first
    const hipError_t es = hipStreamSynchronize(s);
    if (es != hipSuccess)
      return es;
    return h2d(d, h, bytes);
  }

  // The other direction.  Page-locked: asynchronous on `s`.  Pageable and up to 64 MB (glibc serves such blocks from the
  // heap, where registered pages may have lived): through the staging buffers, complete on return.  Larger pageable arrays
  // (always mappings of their own) take the runtime's path.
  static hipError_t d2h_user(pfm_ctx *c, void *h, const void *d, size_t bytes, hipStream_t s)
  {
    if (bytes == 0)
      return hipSuccess;
    if (find_pin(c, h, bytes) || bytes > ((size_t)64 << 20))
      return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s);
    return d2h_staged(h, d, bytes, s);
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
        parallel_for(c->v.n_owned, [&](int64_t nb, int64_t ne) {
          int64_t k = 0;
          for (int64_t n = nb; n < ne; ++n)
            k += __builtin_popcount(node_flags[n] & 7u);
          nf += k;
        });
        c->n_flag_u = nf;
      }
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

  // Adopt the caller's CSR pattern of one block.  The pattern must be the canonical one up to the order of the
  // entries within a row, and that order must keep the structure (node, component): the ncc column components of a
  // neighbour node adjacent and ascending -- what any CSR sorted by local column id has.  The node order of the rows
  // becomes the order of the context's node graph: every kernel family addresses values through it.
  static int pattern_bind_impl(pfm_ctx *c, int block, const int64_t *rp64, const int32_t *rp32, const int32_t *colind)
  {
    if (!c || block < 0 || block >= c->n_blocks || (!rp64 && !rp32) || !colind)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    c->delta.valid = false; // the values move to other slots: what the host holds is not what the shadow describes
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

  int pfm_pattern_bind(pfm_ctx *c, int block, const int64_t *rowptr, const int32_t *colind)
  {
    return pattern_bind_impl(c, block, rowptr, nullptr, colind);
  }

  int pfm_pattern_bind_i32(pfm_ctx *c, int block, const int32_t *rowptr, const int32_t *colind)
  {
    return pattern_bind_impl(c, block, nullptr, rowptr, colind);
  }

  // sol / old / oldold -> node state; old == oldold == nullptr: solution only (pfm_state_set_solution)
  static int state_set_impl(pfm_ctx *c, const double *sol, const double *old, const double *oldold, int on_device)
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
    int rc = launch_state_set(c->v, d[0], d[1], d[2], c->stream);
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

  int pfm_state_set(pfm_ctx *c, const double *sol, const double *old, const double *oldold, int on_device)
  {
    if (!c || (c->n_owned_dofs() != 0 && (!old || !oldold)))
      return PFM_ERR_BAD_ARG;
    return state_set_impl(c, sol, old, oldold, on_device);
  }

  int pfm_state_set_solution(pfm_ctx *c, const double *sol, int on_device) { return state_set_impl(c, sol, nullptr, nullptr, on_device); }

  // Gather tables and scratch of the cells at hanging vertices (DevView::hs_*, pfm_ctx::d_hg_*), from the records of
  // DevView::cres (built on the device): every (cell, resolved node) and (cell, hanging vertex) pair is listed under its
  // destination row, rows ascending, the entries of a row in ascending (cell, index) order -- the order k_hanging_gather adds in.
  // false: some cell has more than 16 resolved nodes (no record): the context keeps the atomic class.
  static bool ensure_hang_gather(pfm_ctx *c)
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

  static int ensure_halo_buffers(pfm_ctx *c);

  int pfm_halo_register(pfm_ctx *c, int n_peers, const int64_t *send_ptr, const int32_t *send_nodes,
                        const int64_t *recv_ptr, const int32_t *recv_nodes)
  {
    if (!c || n_peers < 0 || (n_peers > 0 && (!send_ptr || !recv_ptr)))
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    for (auto &p : c->peers)
      {
        if (p.d_send)
          (void)hipFree(p.d_send);
        if (p.d_recv)
          (void)hipFree(p.d_recv);
      }
    c->peers.assign((size_t)n_peers, HaloPeer{});
    for (int k = 0; k < n_peers; ++k)
      {
        HaloPeer &p = c->peers[k];
        p.n_send = send_ptr[k + 1] - send_ptr[k];
        p.n_recv = recv_ptr[k + 1] - recv_ptr[k];
        for (int64_t j = send_ptr[k]; j < send_ptr[k + 1]; ++j)
          if (send_nodes[j] < 0 || send_nodes[j] >= c->v.n_owned)
            return fail(c, PFM_ERR_BAD_ARG, "halo send node is not an owned node");
        for (int64_t j = recv_ptr[k]; j < recv_ptr[k + 1]; ++j)
          if (recv_nodes[j] < c->v.n_owned || recv_nodes[j] >= c->v.n_nodes)
            return fail(c, PFM_ERR_BAD_ARG, "halo recv node is not a ghost node");
        hipError_t e = hipMalloc((void **)&p.d_send, std::max<size_t>(4, sizeof(int32_t) * p.n_send));
        if (e == hipSuccess)
          e = hipMalloc((void **)&p.d_recv, std::max<size_t>(4, sizeof(int32_t) * p.n_recv));
        if (e == hipSuccess && p.n_send)
          e = hipMemcpy(p.d_send, send_nodes + send_ptr[k], sizeof(int32_t) * p.n_send, hipMemcpyHostToDevice);
        if (e == hipSuccess && p.n_recv)
          e = hipMemcpy(p.d_recv, recv_nodes + recv_ptr[k], sizeof(int32_t) * p.n_recv, hipMemcpyHostToDevice);
        if (e != hipSuccess)
          return hipfail(c, e, "halo_register");
      }
    // concatenated lists for the one-launch pack / unpack
    for (void *q : {(void *)c->d_send_all, (void *)c->d_recv_all, (void *)c->d_send_ptr, (void *)c->d_recv_ptr})
      if (q)
        (void)hipFree(q);
    c->d_send_all = c->d_recv_all = nullptr;
    c->d_send_ptr = c->d_recv_ptr = nullptr;
    for (double **q : {&c->d_halo_send, &c->d_halo_recv})
      if (*q)
        {
          (void)hipFree(*q);
          *q = nullptr;
        }
    c->device_bytes -= c->halo_buf_bytes;
    c->halo_buf_bytes = 0;
    c->n_send_all = n_peers ? send_ptr[n_peers] - send_ptr[0] : 0;
    c->n_recv_all = n_peers ? recv_ptr[n_peers] - recv_ptr[0] : 0;
    if (n_peers > 0)
      {
        std::vector<long long> sp((size_t)n_peers + 1), rp((size_t)n_peers + 1);
        for (int k = 0; k <= n_peers; ++k)
          {
            sp[k] = send_ptr[k] - send_ptr[0];
            rp[k] = recv_ptr[k] - recv_ptr[0];
          }
        hipError_t e = hipMalloc((void **)&c->d_send_all, std::max<size_t>(4, sizeof(int32_t) * c->n_send_all));
        if (e == hipSuccess)
          e = hipMalloc((void **)&c->d_recv_all, std::max<size_t>(4, sizeof(int32_t) * c->n_recv_all));
        if (e == hipSuccess)
          e = hipMalloc((void **)&c->d_send_ptr, sizeof(long long) * sp.size());
        if (e == hipSuccess)
          e = hipMalloc((void **)&c->d_recv_ptr, sizeof(long long) * rp.size());
        if (e == hipSuccess && c->n_send_all)
          e = hipMemcpy(c->d_send_all, send_nodes + send_ptr[0], sizeof(int32_t) * c->n_send_all, hipMemcpyHostToDevice);
        if (e == hipSuccess && c->n_recv_all)
          e = hipMemcpy(c->d_recv_all, recv_nodes + recv_ptr[0], sizeof(int32_t) * c->n_recv_all, hipMemcpyHostToDevice);
        if (e == hipSuccess)
          e = hipMemcpy(c->d_send_ptr, sp.data(), sizeof(long long) * sp.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess)
          e = hipMemcpy(c->d_recv_ptr, rp.data(), sizeof(long long) * rp.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess)
          return hipfail(c, e, "halo_register (concatenated lists)");
        // the message buffers of pfm_halo_exchange are allocated HERE, a local call whose outcome the ranks can agree on,
        // not inside the exchange: an allocation failing on one rank between its peers' enqueued sends and receives would
        // leave them waiting
        const int rcb = ensure_halo_buffers(c);
        if (rcb)
          return rcb;
      }
    return PFM_OK;
  }

  int pfm_halo_pack_all(pfm_ctx *c, double *d_buf_all)
  {
    if (!c || (!d_buf_all && c->n_send_all))
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    return launch_halo_all(c->v, c->d_send_all, c->d_send_ptr, (int)c->peers.size(), c->n_send_all, d_buf_all, 0, c->stream);
  }

  int pfm_halo_unpack_all(pfm_ctx *c, const double *d_buf_all)
  {
    if (!c || (!d_buf_all && c->n_recv_all))
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    return launch_halo_all(c->v, c->d_recv_all, c->d_recv_ptr, (int)c->peers.size(), c->n_recv_all,
                           const_cast<double *>(d_buf_all), 1, c->stream);
  }

  int pfm_halo_pack(pfm_ctx *c, int peer, double *d_buf)
  {
    if (!c || peer < 0 || peer >= (int)c->peers.size() || !d_buf)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    return launch_halo_pack(c->v, c->peers[peer].d_send, c->peers[peer].n_send, d_buf, c->stream);
  }

  int pfm_halo_unpack(pfm_ctx *c, int peer, const double *d_buf)
  {
    if (!c || peer < 0 || peer >= (int)c->peers.size() || !d_buf)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    return launch_halo_unpack(c->v, c->peers[peer].d_recv, c->peers[peer].n_recv, d_buf, c->stream);
  }

  // ---- ghost import over RCCL inside the library (include/pfm_assemble.h)
  static_assert(sizeof(ncclUniqueId) == PFM_COMM_ID_BYTES, "PFM_COMM_ID_BYTES must match ncclUniqueId");

  // RCCL is bound at run time: the library loads (and single-rank runs work) on hosts without librccl, and in a
  // process that already carries a copy (torch bundles one under the same SONAME) the calls go to THAT copy instead of
  // a second one with its own state.  The run-time version is checked against the header this file was compiled with
  // (same major: ncclUniqueId / ncclComm_t / the send-receive signatures are stable within a major).
  extern "C++"
  {
  namespace
  {
    struct RcclApi
    {
      ncclResult_t (*GetVersion)(int *) = nullptr;
      ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
      ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
      ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
      ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
      ncclResult_t (*GroupStart)() = nullptr;
      ncclResult_t (*GroupEnd)() = nullptr;
      ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
      ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
      const char *(*GetErrorString)(ncclResult_t) = nullptr;
      ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;    // optional (pfm_comm_info)
      ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr; // optional
      int version = 0;
      bool ok = false;
      std::string why;
    };

    const RcclApi &rccl()
    {
      static const RcclApi api = [] {
        RcclApi a;
        void *h = nullptr;
        // already in the process (torch's bundled copy, or the host application's)?
        for (const char *name : {"librccl.so.1", "librccl.so"})
          if ((h = dlopen(name, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL)))
            break;
        if (!h)
          {
            const char *rocm = getenv("ROCM_PATH");
            const std::string cand[] = {"librccl.so.1", "librccl.so", std::string(rocm ? rocm : "/opt/rocm") + "/lib/librccl.so.1",
                                        std::string(rocm ? rocm : "/opt/rocm") + "/lib/librccl.so"};
            for (const std::string &name : cand)
              if ((h = dlopen(name.c_str(), RTLD_NOW | RTLD_GLOBAL)))
                break;
          }
        if (!h)
          {
            a.why = "librccl.so not found (dlopen)";
            return a;
          }
        bool all = true;
        auto sym = [&](auto &fp, const char *name) {
          fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(h, name));
          all = all && fp != nullptr;
        };
        sym(a.GetVersion, "ncclGetVersion");
        sym(a.GetUniqueId, "ncclGetUniqueId");
        sym(a.CommInitRank, "ncclCommInitRank");
        sym(a.CommDestroy, "ncclCommDestroy");
        sym(a.CommAbort, "ncclCommAbort");
        sym(a.GroupStart, "ncclGroupStart");
        sym(a.GroupEnd, "ncclGroupEnd");
        sym(a.Send, "ncclSend");
        sym(a.Recv, "ncclRecv");
        sym(a.GetErrorString, "ncclGetErrorString");
        if (!all)
          {
            a.why = "librccl.so lacks a required symbol";
            return a;
          }
        a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(h, "ncclCommCount"));
        a.CommUserRank = reinterpret_cast<decltype(a.CommUserRank)>(dlsym(h, "ncclCommUserRank"));
        int ver = 0;
        if (a.GetVersion(&ver) != ncclSuccess || ver / 10000 != NCCL_MAJOR)
          {
            a.why = "RCCL run-time version " + std::to_string(ver) + " does not match the compiled-in major " + std::to_string(NCCL_MAJOR);
            return a;
          }
        a.version = ver;
        a.ok = true;
        return a;
      }();
      return api;
    }
  } // namespace
  } // extern "C++"

  // what a communicator handle of this ABI points to: the RCCL communicator and whether a failed exchange aborted it
  // (ncclCommAbort frees the communicator; the owner still holds the handle and must be able to destroy it)
  constexpr uint64_t PFM_COMM_MAGIC = 0x70666d636f6d6d31ull; // "pfmcomm1"
  struct PfmComm
  {
    uint64_t magic = PFM_COMM_MAGIC; // a raw ncclComm_t passed where a handle is expected is refused, not reinterpreted
    ncclComm_t cm = nullptr;
    bool aborted = false;
    bool owned = true; // false: the host's own communicator (pfm_comm_wrap), never destroyed here
    int n_ranks = 0, rank = 0;
  };

  int pfm_comm_unique_id(uint8_t id[PFM_COMM_ID_BYTES])
  {
    if (!id)
      return PFM_ERR_BAD_ARG;
    const RcclApi &R = rccl();
    if (!R.ok)
      return PFM_ERR_COMM;
    ncclUniqueId u;
    if (R.GetUniqueId(&u) != ncclSuccess)
      return PFM_ERR_COMM;
    memcpy(id, &u, sizeof(u));
    return PFM_OK;
  }

  int pfm_comm_create(void **comm, const uint8_t id[PFM_COMM_ID_BYTES], int n_ranks, int rank, int device)
  {
    if (!comm || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks)
      return PFM_ERR_BAD_ARG;
    const RcclApi &R = rccl();
    if (!R.ok)
      return PFM_ERR_COMM;
    if (hipSetDevice(device) != hipSuccess)
      return PFM_ERR_HIP;
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t cm = nullptr;
    if (R.CommInitRank(&cm, n_ranks, u, rank) != ncclSuccess)
      return PFM_ERR_COMM;
    PfmComm *h = new (std::nothrow) PfmComm;
    if (!h)
      {
        (void)R.CommAbort(cm);
        return PFM_ERR_NOMEM;
      }
    h->cm = cm;
    h->n_ranks = n_ranks;
    h->rank = rank;
    *comm = h;
    return PFM_OK;
  }

  // The handle outlives an aborted communicator (a failed exchange aborts it so that no peer waits for a message that
  // will never come): destroying it afterwards only frees the handle, using it again reports PFM_ERR_COMM.
  int pfm_comm_destroy(void *comm)
  {
    if (!comm)
      return PFM_OK;
    PfmComm *h = static_cast<PfmComm *>(comm);
    if (h->magic != PFM_COMM_MAGIC)
      return PFM_ERR_BAD_ARG; // not a handle (e.g. the host's raw ncclComm_t): nothing of it is touched
    int rc = PFM_OK;
    if (!h->aborted && h->owned)
      {
        const RcclApi &R = rccl();
        rc = (R.ok && R.CommDestroy(h->cm) == ncclSuccess) ? PFM_OK : PFM_ERR_COMM;
      }
    h->cm = nullptr;
    h->magic = 0;
    delete h;
    return rc;
  }

  int pfm_comm_wrap(void **comm, void *nccl_comm)
  {
    if (!comm || !nccl_comm)
      return PFM_ERR_BAD_ARG;
    PfmComm *h = new (std::nothrow) PfmComm;
    if (!h)
      return PFM_ERR_NOMEM;
    h->cm = static_cast<ncclComm_t>(nccl_comm);
    h->owned = false;
    *comm = h;
    return PFM_OK;
  }

  static bool comm_handle_ok(const void *comm) { return comm && static_cast<const PfmComm *>(comm)->magic == PFM_COMM_MAGIC; }
  int pfm_comm_aborted(const void *comm) { return comm_handle_ok(comm) ? (static_cast<const PfmComm *>(comm)->aborted ? 1 : 0) : 0; }

  // what RCCL itself says about the communicator behind a handle (the driver's N-GPU record can show that RCCL counted N ranks)
  int pfm_comm_info(const void *comm, int *n_ranks, int *rank, int *rccl_version)
  {
    if (!comm_handle_ok(comm))
      return PFM_ERR_BAD_ARG;
    const PfmComm *h = static_cast<const PfmComm *>(comm);
    const RcclApi &R = rccl();
    if (!R.ok || h->aborted || !h->cm)
      return PFM_ERR_COMM;
    int n = -1, r = -1;
    if (R.CommCount && R.CommCount(h->cm, &n) != ncclSuccess)
      return PFM_ERR_COMM;
    if (R.CommUserRank && R.CommUserRank(h->cm, &r) != ncclSuccess)
      return PFM_ERR_COMM;
    if (n_ranks)
      *n_ranks = n;
    if (rank)
      *rank = r;
    if (rccl_version)
      *rccl_version = R.version;
    return PFM_OK;
  }

  // both staging buffers or none: a half-allocated pair must not survive a failed call
  static int ensure_halo_buffers(pfm_ctx *c)
  {
    if (c->d_halo_send && c->d_halo_recv)
      return PFM_OK;
    const int rec = PFM_HALO_DOUBLES_PER_NODE(c->v.dim);
    if (c->d_halo_send)
      (void)hipFree(c->d_halo_send);
    if (c->d_halo_recv)
      (void)hipFree(c->d_halo_recv);
    c->d_halo_send = c->d_halo_recv = nullptr;
    double *snd = nullptr, *rcv = nullptr;
    hipError_t e = hipMalloc((void **)&snd, std::max<size_t>(8, sizeof(double) * rec * c->n_send_all));
    if (e == hipSuccess)
      e = hipMalloc((void **)&rcv, std::max<size_t>(8, sizeof(double) * rec * c->n_recv_all));
    if (e != hipSuccess)
      {
        if (snd)
          (void)hipFree(snd);
        return hipfail(c, e, "hipMalloc halo buffers");
      }
    c->d_halo_send = snd;
    c->d_halo_recv = rcv;
    c->halo_buf_bytes = (int64_t)sizeof(double) * rec * (c->n_send_all + c->n_recv_all);
    c->device_bytes += c->halo_buf_bytes;
    return PFM_OK;
  }

  // pack -> grouped send/receive -> unpack, on `st` (the context's stream, or its side stream for the overlapped form).
  // what: HALO_VALUES = the node values (pfm_halo_exchange), HALO_FLAGS = the flag bytes (pfm_halo_exchange_flags), or both
  // in one group (pfm_active_set_exchange)
  enum { HALO_VALUES = 1, HALO_FLAGS = 2 };
  static int halo_exchange_on(pfm_ctx *c, void *comm, const int *peer_ranks, hipStream_t st, int what = HALO_VALUES)
  {
    const RcclApi &R = rccl();
    if (!R.ok)
      return fail(c, PFM_ERR_COMM, "RCCL unavailable: " + R.why);
    PfmComm *h = static_cast<PfmComm *>(comm);
    if (h->magic != PFM_COMM_MAGIC)
      return fail(c, PFM_ERR_BAD_ARG, "comm is not a handle of pfm_comm_create / pfm_comm_wrap (a raw ncclComm_t must be wrapped)");
    if (h->aborted || !h->cm)
      return fail(c, PFM_ERR_COMM, "communicator was aborted by an earlier failed exchange");
    ncclComm_t cm = h->cm;
    // A rank that fails locally before its sends and receives are enqueued must not leave its peers waiting for them:
    // a communicator the library OWNS is aborted on every failure from here on (the buffers themselves come from
    // pfm_halo_register).  A wrapped communicator belongs to the host: it is never aborted or destroyed here -- the handle is
    // marked (pfm_comm_aborted() == 1, further exchanges refused) and the host decides what to do with its ncclComm_t.
    auto abort_comm = [&](int code, const std::string &msg) {
      if (h->owned)
        (void)R.CommAbort(cm);
      h->aborted = true; // the handle stays valid for pfm_comm_destroy; further exchanges on it are refused
      h->cm = nullptr;
      return fail(c, code, msg + (h->owned ? " (communicator aborted)" : " (wrapped communicator left to the host, handle disabled)"));
    };
    const bool values = what & HALO_VALUES, flags = what & HALO_FLAGS;
    int rc = values ? ensure_halo_buffers(c) : PFM_OK;
    if (rc == PFM_OK && flags)
      rc = reserve_flag_halo_buffers(c);
    if (rc)
      return abort_comm(rc, "halo buffers");
    const int rec = PFM_HALO_DOUBLES_PER_NODE(c->v.dim);
    uint8_t *f_send = c->buf_flag_send.as<uint8_t>(), *f_recv = c->buf_flag_recv.as<uint8_t>();
    if (values)
      rc = launch_halo_all(c->v, c->d_send_all, c->d_send_ptr, (int)c->peers.size(), c->n_send_all, c->d_halo_send, 0, st);
    if (rc == PFM_OK && flags)
      rc = launch_halo_flags_all(c->v, c->d_send_all, c->n_send_all, f_send, 0, st);
    if (rc)
      return abort_comm(rc, "halo pack launch failed");
    ncclResult_t r = R.GroupStart();
    int64_t so = 0, ro = 0;
    for (size_t k = 0; k < c->peers.size() && r == ncclSuccess; ++k)
      {
        const HaloPeer &p = c->peers[k];
        if (values && p.n_recv)
          r = R.Recv(c->d_halo_recv + rec * ro, (size_t)(rec * p.n_recv), ncclDouble, peer_ranks[k], cm, st);
        if (values && p.n_send && r == ncclSuccess)
          r = R.Send(c->d_halo_send + rec * so, (size_t)(rec * p.n_send), ncclDouble, peer_ranks[k], cm, st);
        if (flags && p.n_recv && r == ncclSuccess)
          r = R.Recv(f_recv + ro, (size_t)p.n_recv, ncclUint8, peer_ranks[k], cm, st);
        if (flags && p.n_send && r == ncclSuccess)
          r = R.Send(f_send + so, (size_t)p.n_send, ncclUint8, peer_ranks[k], cm, st);
        so += p.n_send;
        ro += p.n_recv;
      }
    const ncclResult_t r2 = R.GroupEnd();
    if (r == ncclSuccess)
      r = r2;
    if (r != ncclSuccess)
      {
        // work may already be enqueued on the peers: there is no safe fall-back from here -- abort the
        // communicator so that no rank waits for a message that will never come, and report
        return abort_comm(PFM_ERR_COMM, std::string("RCCL: ") + R.GetErrorString(r));
      }
    if (values)
      rc = launch_halo_all(c->v, c->d_recv_all, c->d_recv_ptr, (int)c->peers.size(), c->n_recv_all, c->d_halo_recv, 1, st);
    if (rc == PFM_OK && flags)
      rc = launch_halo_flags_all(c->v, c->d_recv_all, c->n_recv_all, f_recv, 1, st);
    if (rc)
      return fail(c, rc, "halo unpack launch failed");
    return PFM_OK;
  }

  int pfm_halo_exchange(pfm_ctx *c, void *comm, const int *peer_ranks)
  {
    if (!c || (!c->peers.empty() && (!comm || !peer_ranks)))
      return PFM_ERR_BAD_ARG;
    if (c->peers.empty())
      return PFM_OK;
    (void)hipSetDevice(c->device);
    return halo_exchange_on(c, comm, peer_ranks, c->stream);
  }

  int pfm_halo_exchange_flags(pfm_ctx *c, void *comm, const int *peer_ranks)
  {
    if (!c || (!c->peers.empty() && (!comm || !peer_ranks)))
      return PFM_ERR_BAD_ARG;
    if (c->peers.empty())
      return PFM_OK;
    (void)hipSetDevice(c->device);
    return halo_exchange_on(c, comm, peer_ranks, c->stream, HALO_FLAGS);
  }

  // cracks.cc:2826-2890 on a rank with ghost peers (include/pfm_newton.h): owned update -> scatter -> values and flags in
  // one group -> distribution of the hanging nodes, owned and ghost
  int pfm_active_set_exchange(pfm_ctx *c, void *comm, const int *peer_ranks, const double *d_residual_total, const double *d_mass,
                              double c_const, double *d_solution, const double *d_old_solution, int32_t *d_cycle_counter,
                              int64_t *counts)
  {
    if (!c || !d_residual_total || !d_mass || !d_solution || !d_old_solution || !d_cycle_counter || !counts ||
        (!c->peers.empty() && (!comm || !peer_ranks)))
      return PFM_ERR_BAD_ARG;
    int rc = pfm_active_set_owned_device(c, d_residual_total, d_mass, c_const, d_solution, d_old_solution, d_cycle_counter, counts);
    if (rc == PFM_OK)
      rc = pfm_state_set_solution(c, d_solution, 1);
    if (rc == PFM_OK && !c->peers.empty())
      rc = halo_exchange_on(c, comm, peer_ranks, c->stream, HALO_VALUES | HALO_FLAGS);
    if (rc == PFM_OK)
      rc = pfm_distribute_hanging_device(c, d_solution);
    return rc;
  }

  // cartesian overlay: the slots of the regular rows follow the order of the node-graph rows (pfm_pattern_bind may change it);
  // v.nadj exists (ensure_tables: lattice contexts build the general tables on first use)
  static int ensure_patch_ready(pfm_ctx *c)
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
  static int ensure_overlay3_ready(pfm_ctx *c)
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
  static int ensure_overlap_lists(pfm_ctx *c)
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
  static void drop_overlap_lists(pfm_ctx *c)
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
  static bool stress_split(const pfm_ctx *c) { return c->have_params && cart_scheme(c->prm).split; }
  // ... but for what plan_cart takes from the law and the route of the context (CartPlan::voldev, CartPlan::spectral)
  static pfm::CartSplit cart_split(const pfm_ctx *c) { return {c->split_model, c->split_route}; }

  // Every decision of one assemble_impl call; what each means stands where it is made (plan_assembly, after_tables).
  struct AssemblyPlan
  {
    int phase = 0; // 0: the whole assembly; 1, 2: the halves of pfm_assemble_overlapped
    bool residual_only = false, split = false, cart = false, patches = false, overlay3 = false, overlay_uu = false, nothing = false;
    bool pair = false, fork = false, levels_concurrent = false, fill_up_block = false, up_block_cleared = false;
    bool keep_up_block = false; // d_values[1] is a kept (u,phi) block: nothing of this call writes it
    bool gather = false, fork_general = false, atomic_stream = false; // final behind the lazy tables: after_tables
    CartPlan box;   // cart: what the launchers of the cartesian family do (plan_cart)
    CartPlan level; // overlay3: the same for the first level lattice (every level shares its scheme, law and kernels)
    void after_tables(const pfm_ctx *c, bool gather_ready);
  };

  // No side effects, no allocation: what the context, the parameters and the switches say about this call.
  static AssemblyPlan plan_assembly(const pfm_ctx *c, int residual_only, int phase, double *const *d_values)
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
  static int ensure_side_stream(pfm_ctx *c)
  {
    if (c->side_stream)
      return PFM_OK;
    if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "side stream");
    return PFM_OK;
  }

  // what `to` gets from here on runs behind what `from` has got so far; join_from: the same, named for the reader
  static int fork_to(pfm_ctx *c, hipStream_t from, hipStream_t to, hipEvent_t ev, const char *what)
  {
    hipError_t e = hipEventRecord(ev, from);
    if (e == hipSuccess)
      e = hipStreamWaitEvent(to, ev, 0);
    return e == hipSuccess ? PFM_OK : hipfail(c, e, what);
  }
  static int join_from(pfm_ctx *c, hipStream_t from, hipStream_t to, hipEvent_t ev, const char *what) { return fork_to(c, from, to, ev, what); }

  // the side stream behind what the context's stream has got so far (its join: join_from with ev_join)
  static int fork_side(pfm_ctx *c, const char *what)
  {
    const int rc = ensure_side_stream(c);
    return rc ? rc : fork_to(c, c->stream, c->side_stream, c->ev_fork, what);
  }

  // the next pair of timing events; the interval opens on the context's stream
  static int open_interval(pfm_ctx *c, hipEvent_t &ev0, hipEvent_t &ev1)
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
  static int ensure_patch_list(pfm_ctx *c)
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

  // the lazy tables of the plan's family; gather_ready: the gather has its tables (false: the atomic class stays)
  static int ensure_tables(pfm_ctx *c, const AssemblyPlan &p, bool &gather_ready)
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
  static int zero_outputs(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot)
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
  static int compressed_counter(pfm_ctx *c, bool zero, int *&n_compressed)
  {
    if (!c->buf_compressed.p)
      {
        if (hipMalloc(&c->buf_compressed.p, 256) != hipSuccess)
          return fail(c, PFM_ERR_NOMEM, "compressed-cell counter");
        c->buf_compressed.bytes = 256;
        c->allocs.push_back(c->buf_compressed.p);
        c->device_bytes += 256;
      }
    n_compressed = c->buf_compressed.as<int>();
    if (zero && hipMemsetAsync(n_compressed, 0, sizeof(int), c->stream) != hipSuccess)
      return fail(c, PFM_ERR_HIP, "compressed-cell counter reset");
    return PFM_OK;
  }

  // CartPlan::voldev_sparse: the cell bytes, the tile-chunk flags of grid[PFM_ZC_UU3] and the row counter, made on first use
  // (grow-only) and emptied on the context's stream in front of k_cart_split3_mark
  static int sparse_reserve(pfm_ctx *c, pfm::DevBuf &b, size_t bytes, const char *what)
  {
    if (b.p && b.bytes >= bytes)
      return PFM_OK;
    if (b.p) // (a longer lattice of flags after pfm_ctx_force_zchunk) queued work may still use the old buffer
      {
        (void)hipStreamSynchronize(c->stream);
        c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), b.p), c->allocs.end());
        (void)hipFree(b.p);
        c->device_bytes -= (int64_t)b.bytes;
        b = pfm::DevBuf{};
      }
    bytes = std::max<size_t>(bytes, 256);
    if (hipMalloc(&b.p, bytes) != hipSuccess)
      {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(c, PFM_ERR_NOMEM, what);
      }
    c->allocs.push_back(b.p);
    b.bytes = bytes;
    c->device_bytes += (int64_t)bytes;
    return PFM_OK;
  }
  // the row counter: one for the box, one for all level lattices of an overlay (emptied once, on the context's stream)
  static int sparse_row_counter(pfm_ctx *c)
  {
    if (const int rc = sparse_reserve(c, c->buf_sparse_rows, sizeof(int), "row counter of the sparse split Jacobian"))
      return rc;
    return hipMemsetAsync(c->buf_sparse_rows.p, 0, sizeof(int), c->stream) == hipSuccess ? PFM_OK : fail(c, PFM_ERR_HIP, "sparse split Jacobian: counter reset");
  }
  // the cell bytes and tile-chunk flags of lattice cv (the box, or one level lattice with buffers of its own), emptied on s
  static int sparse_buffers(pfm_ctx *c, const pfm::CartView &cv, const CartPlan &pl, pfm::DevBuf &cells, pfm::DevBuf &flags, int64_t &tiles,
                            hipStream_t s, pfm::SplitSparse &sp)
  {
    const TileGrid &g = pl.grid[PFM_ZC_UU3];
    const size_t n_cells = (size_t)std::max(cv.NX - 1, 0) * (size_t)std::max(cv.NY - 1, 0) * (size_t)std::max(cv.NZ - 1, 0);
    const size_t n_tiles = (size_t)g.ntx * g.nty * g.nch;
    if (const int rc = sparse_reserve(c, cells, n_cells, "cell bytes of the sparse split Jacobian"))
      return rc;
    if (const int rc = sparse_reserve(c, flags, n_tiles * sizeof(int), "tile-chunk flags of the sparse split Jacobian"))
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
  static int assemble_box(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
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
    rc = launch_assemble_cart(p.box, c->v, cv, c->prm, d_values, d_res_pde, d_res_tot, c->stream, p.fork ? c->side_stream : c->stream,
                              c->d_scal, &c->clock, n_compressed, run_sparse ? &sparse : nullptr);
    if (p.box.split3_jac())
      c->compressed_valid = rc == PFM_OK;
    if (run_sparse)
      c->sparse_valid = rc == PFM_OK, c->sparse_levels = false;
    if (p.fork)
      if (const int rcj = join_from(c, c->side_stream, c->stream, c->ev_join, "join"))
        return rcj;
    if (p.pair && rc == PFM_OK)
      rc = launch_cart_apply_patches(c->cv, d_values[0], c->stream, c->v.status);
    return PFM_OK;
  }

  // The view the launches of the general family take.  classes: for its colour and atomic classes -- the reduced colour
  // lists next to an overlay, and either the atomic adds or the scratch of the cells at hanging vertices, never both.
  static pfm::DevView general_view(const pfm_ctx *c, const AssemblyPlan &p, bool classes)
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
  static void gather_hanging(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
  {
    if (p.gather && rc == PFM_OK)
      rc = launch_hanging_gather(general_view(c, p, false), c->prm, p.residual_only, d_values, d_res_pde, d_res_tot, c->d_hg_rows, c->d_hg_ptr,
                                 c->d_hg_list, c->n_hg_rows, c->stream);
  }

  // 3-D overlay: the row-owner kernels on every level lattice, on the context's stream or (plan.levels_concurrent) each
  // level on a stream of its own between a fork and a join
  static int launch_levels(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
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
  static int assemble_overlay(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
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
  static int assemble_general(pfm_ctx *c, const AssemblyPlan &p, double *const *d_values, double *d_res_pde, double *d_res_tot, int &rc)
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
  static int assemble_impl(pfm_ctx *c, int residual_only, double *const *d_values, double *d_res_pde, double *d_res_tot, int phase)
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

  // ---- host-visible outputs (the caller hands system_pde_matrix to Trilinos right after the call,
  // cracks.cc:2754, 2770, 2918).  35 GB of matrix values cross PCIe per Jacobian at 216^3: what can be done about that is
  // (1) DMA from / to page-locked memory instead of the runtime's pageable path (pfm_host_register), (2) never moving the
  // (u,phi) block, which is identically zero (cracks.cc:2333-2337; placeholders of constrained rows live on the diagonals
  // of the (u,u) and (phi,phi) blocks): 3/16 of the bytes, (3) two copy streams.
  int pfm_host_register(pfm_ctx *c, void *p, int64_t bytes)
  {
    if (!c || !p || bytes <= 0)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    for (auto &hp : c->host_pins)
      if (hp.p == p)
        {
          if (hp.bytes >= (size_t)bytes)
            return PFM_OK;
          (void)hipHostUnregister(hp.p); // the same array, grown: lock it again
          hp.p = nullptr;
        }
    c->host_pins.erase(std::remove_if(c->host_pins.begin(), c->host_pins.end(), [](const pfm_ctx::HostPin &h) { return h.p == nullptr; }),
                       c->host_pins.end());
    const hipError_t e = hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess)
      {
        (void)hipGetLastError(); // not sticky: the transfers simply take the pageable path
        return fail(c, PFM_ERR_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e) + " (the array stays pageable)");
      }
    pfm_ctx::HostPin hp;
    hp.p = p;
    hp.bytes = (size_t)bytes;
    c->host_pins.push_back(hp);
    return PFM_OK;
  }

  int pfm_host_unregister(pfm_ctx *c, void *p)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream)
      (void)hipStreamSynchronize(c->copy_stream);
    delta_forget_host(c, p);
    for (auto &hp : c->host_pins)
      if (!p || hp.p == p)
        {
          (void)hipHostUnregister(hp.p);
          hp.p = nullptr;
        }
    c->host_pins.erase(std::remove_if(c->host_pins.begin(), c->host_pins.end(), [](const pfm_ctx::HostPin &h) { return h.p == nullptr; }),
                       c->host_pins.end());
    return PFM_OK;
  }

  static pfm_ctx::HostPin *find_pin(pfm_ctx *c, const void *p, size_t bytes)
  {
    for (auto &hp : c->host_pins)
      if (hp.p == p && hp.bytes >= bytes)
        return &hp;
    return nullptr;
  }

  // matrix values of the last pfm_assemble_device -> the host's arrays, asynchronously: block 0 on the context's stream,
  // the phase-field blocks on a second stream (joined into the first before returning).  Does not synchronise.
  static int values_to_host_async(pfm_ctx *c, double *const *d_values, double *const *h_values)
  {
    (void)hipSetDevice(c->device);
    if (!c->copy_stream)
      {
        if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming) != hipSuccess)
          return fail(c, PFM_ERR_HIP, "copy stream");
      }
    for (int b = 0; b < c->n_blocks; ++b) // (checked before the fork: no exit path leaves copy_stream unjoined)
      if (c->block_nnz(b) > 0 && (!h_values[b] || !d_values[b]))
        return fail(c, PFM_ERR_BAD_ARG, "pfm_values_to_host: null block");
    hipError_t e = hipEventRecord(c->ev_copy, c->stream);
    if (e == hipSuccess)
      e = hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0);
    for (int b = 0; b < c->n_blocks && e == hipSuccess; ++b)
      {
        const size_t bytes = sizeof(double) * (size_t)c->block_nnz(b);
        if (!bytes)
          continue;
        if (c->n_blocks == 4 && b == 1)
          {
            // (u,phi) = 0.  A registered array is ours between the calls (nobody else writes the matrix: the reference only
            // ever fills it through assemble_system): cleared once, by host threads next to the transfers, never copied.
            // An unregistered one is copied like the others (the device block holds the zeros the kernels wrote).
            pfm_ctx::HostPin *hp = find_pin(c, h_values[b], bytes);
            if (hp)
              {
                if (!hp->zeroed)
                  {
                    const int nt = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
                    std::vector<std::thread> th;
                    const size_t chunk = ((bytes / (size_t)nt) + 4095) & ~(size_t)4095;
                    for (int t = 0; t < nt; ++t)
                      {
                        const size_t lo = std::min(bytes, (size_t)t * chunk), hi = std::min(bytes, lo + chunk);
                        if (hi > lo)
                          th.emplace_back([=] { std::memset(reinterpret_cast<char *>(h_values[b]) + lo, 0, hi - lo); });
                      }
                    for (auto &t : th)
                      t.join();
                    hp->zeroed = true;
                  }
                continue;
              }
          }
        e = d2h_user(c, h_values[b], d_values[b], bytes, b == 0 ? c->stream : c->copy_stream);
      }
    if (e == hipSuccess)
      e = hipEventRecord(c->ev_copy, c->copy_stream);
    if (e == hipSuccess)
      e = hipStreamWaitEvent(c->stream, c->ev_copy, 0);
    return e == hipSuccess ? PFM_OK : hipfail(c, e, "copy back (matrix values)");
  }

  int pfm_values_to_host(pfm_ctx *c, double *const *d_values, double *const *h_values)
  {
    if (!c || !d_values || !h_values)
      return PFM_ERR_BAD_ARG;
    const int rc = values_to_host_async(c, d_values, h_values);
    if (rc)
      return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? PFM_OK : hipfail(c, e, "pfm_values_to_host");
  }

  int pfm_assemble(pfm_ctx *c, const double *sol, const double *old, const double *oldold,
                   int residual_only, double *const *values, double *residual_pde,
                   double *residual_total)
  {
    if (!c || !residual_pde || (residual_only && !residual_total) || (!residual_only && !values))
      return PFM_ERR_BAD_ARG;
    if (c->v.n_owned != c->v.n_nodes)
      return fail(c, PFM_ERR_BAD_ARG, "pfm_assemble is single-rank only; use the halo entry points");
    int rc = pfm_state_set(c, sol, old, oldold, 0);
    if (rc)
      return rc;
    const size_t vb = sizeof(double) * (size_t)c->n_owned_dofs();
    for (int k = 0; k < 2; ++k)
      if (!c->d_stage_res[k])
        {
          hipError_t e = hipMalloc((void **)&c->d_stage_res[k], std::max<size_t>(vb, 8));
          if (e != hipSuccess)
            return hipfail(c, e, "hipMalloc stage residual");
          c->device_bytes += (int64_t)vb;
        }
    if (!residual_only)
      for (int b = 0; b < c->n_blocks; ++b)
        if (!c->d_stage_val[b])
          {
            const size_t bytes = sizeof(double) * (size_t)c->block_nnz(b);
            hipError_t e = hipMalloc((void **)&c->d_stage_val[b], std::max<size_t>(bytes, 8));
            if (e != hipSuccess)
              return hipfail(c, e, "hipMalloc stage values");
            c->device_bytes += (int64_t)bytes;
            if (c->n_blocks == 4 && b == 1 && bytes)
              {
                // the staging (u,phi) block is the library's own: cleared once, here, and kept (plan_assembly) -- complete
                // before any assembly on any stream; an unregistered h_values[1] keeps receiving these zeros by its copy
                e = hipMemsetAsync(c->d_stage_val[b], 0, bytes, c->stream);
                if (e == hipSuccess)
                  e = hipStreamSynchronize(c->stream);
                if (e != hipSuccess)
                  return hipfail(c, e, "clear the staged (u,phi) block");
                c->stage_up_kept = true;
              }
          }
    rc = pfm_assemble_device(c, residual_only, c->d_stage_val, c->d_stage_res[0], c->d_stage_res[1]);
    if (rc)
      return rc;
    // the residual first (the caller's Newton loop reads it at once, cracks.cc:2791-2794), then the matrix blocks
    hipError_t e = d2h_user(c, residual_pde, c->d_stage_res[0], vb, c->stream);
    if (e == hipSuccess && residual_only)
      e = d2h_user(c, residual_total, c->d_stage_res[1], vb, c->stream);
    if (e != hipSuccess)
      return hipfail(c, e, "copy back");
    if (!residual_only)
      {
        rc = values_to_host_async(c, c->d_stage_val, values);
        if (rc)
          return rc;
      }
    return pfm_sync_status(c);
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

namespace pfm
{
  // d2h_user for a piece [h, h + bytes) of an array: page-locked if it lies inside a registered array
  hipError_t d2h_user_piece(pfm_ctx *c, void *h, const void *d, size_t bytes, hipStream_t s)
  {
    if (bytes == 0)
      return hipSuccess;
    const char *lo = static_cast<const char *>(h);
    for (const auto &hp : c->host_pins)
      if (lo >= static_cast<const char *>(hp.p) && lo + bytes <= static_cast<const char *>(hp.p) + hp.bytes)
        return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s);
    return d2h_user(c, h, d, bytes, s);
  }
} // namespace pfm
