// pfm_halo.cpp -- ghost import (include/pfm_assemble.h): the send / receive lists of pfm_halo_register, pack and unpack,
// RCCL bound at run time with dlopen, the communicator handles (pfm_comm_*), the exchange on a stream (halo_exchange_on)
// and the entries that run it.  The only file that sees rccl.h and dlfcn.h.
#include "pfm_host.h"
#include "../../include/pfm_newton.h"

#include <rccl/rccl.h> // types and constants only: the entry points are bound with dlopen (rccl() below)
#include <dlfcn.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

using namespace pfm;

namespace
{
  // both staging buffers or none: a half-allocated pair must not survive a failed call
  int ensure_halo_buffers(pfm_ctx *c)
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

  // ---- ghost import over RCCL inside the library (include/pfm_assemble.h)
  static_assert(sizeof(ncclUniqueId) == PFM_COMM_ID_BYTES, "PFM_COMM_ID_BYTES must match ncclUniqueId");

  // RCCL is bound at run time: the library loads (and single-rank runs work) on hosts without librccl, and in a
  // process that already carries a copy (torch bundles one under the same SONAME) the calls go to THAT copy instead of
  // a second one with its own state.  The run-time version is checked against the header this file was compiled with
  // (same major: ncclUniqueId / ncclComm_t / the send-receive signatures are stable within a major).
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

  bool comm_handle_ok(const void *comm) { return comm && static_cast<const PfmComm *>(comm)->magic == PFM_COMM_MAGIC; }
} // namespace

namespace pfm
{
  // pack -> grouped send/receive -> unpack, on `st` (the context's stream, or its side stream for the overlapped form).
  // what: HALO_VALUES = the node values (pfm_halo_exchange), HALO_FLAGS = the flag bytes (pfm_halo_exchange_flags), or both
  // in one group (pfm_active_set_exchange)
  int halo_exchange_on(pfm_ctx *c, void *comm, const int *peer_ranks, hipStream_t st, int what)
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
} // namespace pfm

extern "C"
{
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
}
