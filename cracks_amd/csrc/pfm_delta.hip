// pfm_delta.hip -- pfm_values_to_host_delta (include/pfm_assemble.h): the matrix values go to the host's CSR arrays, but only
// the chunks whose bits differ from what the host already holds cross the link ("Delta transfer").
//
// The context keeps a device copy of the host's values per block (the shadow).  A block is worked through in slabs of
// slab_bytes, two in flight:
//   stage 1 (context's stream)  k_delta_compare: one wave per chunk, new values and shadow with 16-byte loads, one
//                               wave-uniform decision (__ballot of the lanes' xor), flag[chunk]; a chunk that differs is
//                               stored to the shadow from the registers that hold it.  k_delta_scan: one workgroup, the
//                               changed chunks in ascending order and their number, which goes to the host (8 bytes).
//   stage 2 (copy stream)       nothing changed: nothing.  Most chunks changed: the slab goes d_values -> h_values as
//                               pfm_values_to_host would send it.  Else k_delta_pack gathers the changed chunks and their
//                               list into a staging buffer and ONE copy takes both to page-locked memory of the context.
//   stage 3 (host threads)      pfm_delta_host.h: a memcpy per chunk into the caller's array.
// The compare of slab k + 1, the DMA of slab k and the scatter of slab k - 1 overlap.  The packed image is a function of
// the flags alone (ordered scan, no atomics): reproducible.
#include "pfm_delta_host.h"
#include "pfm_entry.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace pfm
{
  namespace
  {
    using u64 = unsigned long long;
    constexpr int64_t DELTA_CHUNK_DEFAULT = 4096;       // bytes
    constexpr int64_t DELTA_SLAB_DEFAULT = 32ll << 20;  // bytes
    constexpr int64_t DELTA_SLAB_MAX_CHUNKS = 1 << 24;  // flags and lists are 32-bit, one scan workgroup per slab
    constexpr int CMP_WAVES = 4;                        // waves (chunks) per workgroup of the compare and pack kernels
    // a slab goes directly when more than DIRECT_NUM / DIRECT_DEN of its chunks changed: the packed path pays a host memcpy
    // per byte next to the DMA, the direct path ships the unchanged rest
    constexpr int64_t DIRECT_NUM = 3, DIRECT_DEN = 4;

    // One wave per chunk of `cd` words (a power of two >= 8; the last chunk of a block has n < cd).  W = 2: the lane's
    // pieces are 16 bytes (both bases 16-byte aligned), W = 1: 8 bytes.  ITER > 0: the chunk fits ITER pieces per lane and
    // stays in registers between the compare and the store; ITER = 0: any length, a changed chunk is read again.
    template <int ITER, int W>
    __global__ __launch_bounds__(64 * CMP_WAVES) void k_delta_compare(const u64 *__restrict__ cur, u64 *__restrict__ shadow, long long nnz,
                                                                       long long first_chunk, int n_chunks, int cd,
                                                                       unsigned *__restrict__ flags)
    {
      const int wave = (int)blockIdx.x * CMP_WAVES + ((int)threadIdx.x >> 6);
      if (wave >= n_chunks)
        return;
      const int lane = (int)threadIdx.x & 63;
      const long long base = (first_chunk + wave) * (long long)cd;
      const int n = (int)min((long long)cd, nnz - base);
      const u64 *a = cur + base;
      u64 *b = shadow + base;
      u64 diff = 0;
      if constexpr (ITER > 0)
        {
          u64 va[ITER][W];
#pragma unroll
          for (int j = 0; j < ITER; ++j)
            {
              const int i = (lane + 64 * j) * W;
              if constexpr (W == 2)
                {
                  va[j][0] = va[j][1] = 0;
                  if (i + 1 < n)
                    {
                      const ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(a + i);
                      const ulonglong2 y = *reinterpret_cast<const ulonglong2 *>(b + i);
                      va[j][0] = x.x;
                      va[j][1] = x.y;
                      diff |= (x.x ^ y.x) | (x.y ^ y.y);
                    }
                  else if (i < n)
                    {
                      va[j][0] = a[i];
                      diff |= va[j][0] ^ b[i];
                    }
                }
              else
                {
                  va[j][0] = 0;
                  if (i < n)
                    {
                      va[j][0] = a[i];
                      diff |= va[j][0] ^ b[i];
                    }
                }
            }
          const bool changed = __ballot(diff != 0) != 0ull; // wave-uniform
          if (changed)
            {
#pragma unroll
              for (int j = 0; j < ITER; ++j)
                {
                  const int i = (lane + 64 * j) * W;
                  if constexpr (W == 2)
                    {
                      if (i + 1 < n)
                        *reinterpret_cast<ulonglong2 *>(b + i) = make_ulonglong2(va[j][0], va[j][1]);
                      else if (i < n)
                        b[i] = va[j][0];
                    }
                  else if (i < n)
                    b[i] = va[j][0];
                }
            }
          if (lane == 0)
            flags[wave] = changed ? 1u : 0u;
        }
      else
        {
          for (int i = lane; i < n; i += 64)
            diff |= a[i] ^ b[i];
          const bool changed = __ballot(diff != 0) != 0ull;
          if (changed)
            for (int i = lane; i < n; i += 64)
              b[i] = a[i];
          if (lane == 0)
            flags[wave] = changed ? 1u : 0u;
        }
    }

    // list[0 .. count) = the chunks of the slab with a raised flag, ascending; *count.  One workgroup: thread t owns a
    // contiguous range of the flags, the ranges' sums are scanned in LDS.
    __global__ __launch_bounds__(1024) void k_delta_scan(const unsigned *__restrict__ flags, int n, unsigned *__restrict__ list,
                                                          u64 *__restrict__ count)
    {
      __shared__ unsigned part[1024];
      const int t = (int)threadIdx.x;
      const int per = (n + 1023) / 1024;
      const int lo = min(n, t * per), hi = min(n, lo + per);
      unsigned s = 0;
      for (int i = lo; i < hi; ++i)
        s += flags[i];
      part[t] = s;
      __syncthreads();
      for (int off = 1; off < 1024; off <<= 1)
        {
          const unsigned v = t >= off ? part[t - off] : 0u;
          __syncthreads();
          part[t] += v;
          __syncthreads();
        }
      unsigned at = part[t] - s;
      for (int i = lo; i < hi; ++i)
        if (flags[i])
          list[at++] = (unsigned)i;
      if (t == 1023)
        count[0] = part[1023];
    }

    // out = [count chunks of cd words][count list entries]: wave w copies chunk list[w] (its valid words), the first count
    // threads of the grid copy the list behind the payload
    template <int W>
    __global__ __launch_bounds__(64 * CMP_WAVES) void k_delta_pack(const u64 *__restrict__ cur, long long nnz, long long first_chunk, int cd,
                                                                    const unsigned *__restrict__ list, unsigned count, u64 *__restrict__ out)
    {
      const unsigned gt = blockIdx.x * (unsigned)(64 * CMP_WAVES) + threadIdx.x;
      const unsigned wave = gt >> 6;
      if (gt < count)
        reinterpret_cast<unsigned *>(out + (size_t)count * cd)[gt] = list[gt];
      if (wave >= count)
        return;
      const int lane = (int)threadIdx.x & 63;
      const long long base = (first_chunk + list[wave]) * (long long)cd;
      const int n = (int)min((long long)cd, nnz - base);
      const u64 *a = cur + base;
      u64 *o = out + (size_t)wave * cd;
      for (int i = lane * W; i < n; i += 64 * W)
        {
          if constexpr (W == 2)
            {
              if (i + 1 < n)
                *reinterpret_cast<ulonglong2 *>(o + i) = *reinterpret_cast<const ulonglong2 *>(a + i);
              else
                o[i] = a[i];
            }
          else
            o[i] = a[i];
        }
    }

    template <int W>
    void launch_compare_w(int iter, int blocks, hipStream_t s, const u64 *cur, u64 *shadow, long long nnz, long long first_chunk, int n_chunks,
                          int cd, unsigned *flags)
    {
      const dim3 g((unsigned)blocks), b(64 * CMP_WAVES);
      switch (iter)
        {
        case 1: hipLaunchKernelGGL((k_delta_compare<1, W>), g, b, 0, s, cur, shadow, nnz, first_chunk, n_chunks, cd, flags); break;
        case 2: hipLaunchKernelGGL((k_delta_compare<2, W>), g, b, 0, s, cur, shadow, nnz, first_chunk, n_chunks, cd, flags); break;
        case 4: hipLaunchKernelGGL((k_delta_compare<4, W>), g, b, 0, s, cur, shadow, nnz, first_chunk, n_chunks, cd, flags); break;
        case 8: hipLaunchKernelGGL((k_delta_compare<8, W>), g, b, 0, s, cur, shadow, nnz, first_chunk, n_chunks, cd, flags); break;
        default: hipLaunchKernelGGL((k_delta_compare<0, 1>), g, b, 0, s, cur, shadow, nnz, first_chunk, n_chunks, cd, flags); break;
        }
    }

    bool aligned16(const void *a, const void *b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0; }

    int64_t chunk_bytes_of(const pfm_ctx *c) { return c->delta.chunk_bytes ? c->delta.chunk_bytes : DELTA_CHUNK_DEFAULT; }
    int64_t slab_bytes_of(const pfm_ctx *c)
    {
      if (c->delta.slab_bytes)
        return c->delta.slab_bytes;
      const int64_t cb = chunk_bytes_of(c);
      return std::max(cb, DELTA_SLAB_DEFAULT / cb * cb);
    }

    void dev_buf_release(pfm_ctx *c, DevBuf &b)
    {
      if (!b.p)
        return;
      c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), b.p), c->allocs.end());
      (void)hipFree(b.p);
      c->device_bytes -= (int64_t)b.bytes;
      b = DevBuf{};
    }

    // staging of the slab pipeline (its size follows the configuration): dropped by pfm_values_delta_config
    void release_staging(pfm_ctx *c)
    {
      DeltaState &d = c->delta;
      for (int j = 0; j < 2; ++j)
        {
          dev_buf_release(c, d.flags[j]);
          dev_buf_release(c, d.count[j]);
          dev_buf_release(c, d.pack[j]);
          if (d.h_pack[j])
            (void)hipHostFree(d.h_pack[j]);
          d.h_pack[j] = nullptr;
        }
      if (d.h_count)
        (void)hipHostFree(d.h_count);
      d.h_count = nullptr;
      d.h_pack_bytes = 0;
    }

    int hipfail(pfm_ctx *c, hipError_t e, const char *what) { return fail(c, PFM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

    // streams, events, shadow and staging; PFM_ERR_NOMEM leaves nothing half-made that a later call would trust
    int ensure_resources(pfm_ctx *c, int64_t slab_chunks, int64_t chunk_bytes)
    {
      DeltaState &d = c->delta;
      if (!c->copy_stream)
        {
          if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
              hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming) != hipSuccess)
            return fail(c, PFM_ERR_HIP, "copy stream");
        }
      for (int j = 0; j < 2; ++j)
        {
          if (!d.ev_cmp[j] && hipEventCreateWithFlags(&d.ev_cmp[j], hipEventDisableTiming) != hipSuccess)
            return fail(c, PFM_ERR_HIP, "delta events");
          if (!d.ev_dma[j] && hipEventCreateWithFlags(&d.ev_dma[j], hipEventDisableTiming) != hipSuccess)
            return fail(c, PFM_ERR_HIP, "delta events");
        }
      for (int b = 0; b < c->n_blocks; ++b)
        {
          const size_t bytes = sizeof(double) * (size_t)c->block_nnz(b);
          if (bytes && (!d.shadow[b].p || d.shadow[b].bytes < bytes))
            {
              d.valid = false; // (a grown buffer has lost its contents)
              if (const int rc = dev_buf_reserve(c, d.shadow[b], bytes, "delta shadow"))
                return rc;
            }
        }
      const size_t pack_bytes = (size_t)slab_chunks * (size_t)(chunk_bytes + 4);
      for (int j = 0; j < 2; ++j)
        {
          int rc = dev_buf_reserve(c, d.flags[j], sizeof(unsigned) * 2 * (size_t)slab_chunks, "delta flags");
          if (!rc)
            rc = dev_buf_reserve(c, d.count[j], sizeof(u64), "delta count");
          if (!rc)
            rc = dev_buf_reserve(c, d.pack[j], pack_bytes, "delta staging");
          if (rc)
            return rc;
        }
      if (d.h_pack_bytes < pack_bytes || !d.h_count)
        {
          for (int j = 0; j < 2; ++j)
            {
              if (d.h_pack[j])
                (void)hipHostFree(d.h_pack[j]);
              d.h_pack[j] = nullptr;
            }
          d.h_pack_bytes = 0;
          if (!d.h_count && hipHostMalloc(reinterpret_cast<void **>(&d.h_count), 2 * sizeof(u64), hipHostMallocDefault) != hipSuccess)
            {
              (void)hipGetLastError();
              d.h_count = nullptr;
              return fail(c, PFM_ERR_NOMEM, "hipHostMalloc delta count");
            }
          for (int j = 0; j < 2; ++j)
            if (hipHostMalloc(&d.h_pack[j], pack_bytes, hipHostMallocDefault) != hipSuccess)
              {
                (void)hipGetLastError();
                d.h_pack[j] = nullptr;
                return fail(c, PFM_ERR_NOMEM, "hipHostMalloc delta staging");
              }
          d.h_pack_bytes = pack_bytes;
        }
      return PFM_OK;
    }

    pfm_ctx::HostPin *find_pin(pfm_ctx *c, const void *p, size_t bytes)
    {
      for (auto &hp : c->host_pins)
        if (hp.p == p && hp.bytes >= bytes)
          return &hp;
      return nullptr;
    }

    struct Slab // one slab on its way through the stages
    {
      int64_t first_chunk = 0, n_chunks = 0, count = 0;
      int mode = 0; // 0: nothing to ship, 1: direct, 2: packed
    };

    // blocks whose shadow holds what the host holds: the slab pipeline
    int delta_block(pfm_ctx *c, int b, const double *d_val, double *h_val, int64_t chunk_bytes, int64_t slab_chunks, int n_threads,
                    int64_t *st)
    {
      DeltaState &d = c->delta;
      const int64_t nnz = c->block_nnz(b);
      const int cd = (int)(chunk_bytes / 8);
      const int64_t n_chunks = (nnz + cd - 1) / cd, n_slabs = (n_chunks + slab_chunks - 1) / slab_chunks;
      const u64 *cur = reinterpret_cast<const u64 *>(d_val);
      u64 *shadow = d.shadow[b].as<u64>();
      const bool v16 = aligned16(cur, shadow);
      const int per_lane = (int)std::max<int64_t>(1, cd / (64 * (v16 ? 2 : 1)));
      const int iter = per_lane <= 8 ? per_lane : 0; // in registers up to 8 KiB (16-byte pieces) / 4 KiB per chunk
      Slab sl[3]; // slab k: record k % 3 (three stages), staging slot k & 1 (its buffers are free again after stage 2 of slab k + 1)
      hipError_t e = hipSuccess;
      for (int64_t k = 0; k < n_slabs + 2 && e == hipSuccess; ++k)
        {
          if (k < n_slabs) // stage 1
            {
              const int j = (int)(k & 1);
              Slab &s = sl[k % 3];
              s.first_chunk = k * slab_chunks;
              s.n_chunks = std::min(slab_chunks, n_chunks - s.first_chunk);
              s.count = 0;
              s.mode = 0;
              if (k >= 2) // the scan writes the list that the pack of slab k - 2 reads
                e = hipStreamWaitEvent(c->stream, d.ev_dma[j], 0);
              if (e != hipSuccess)
                break;
              unsigned *flags = d.flags[j].as<unsigned>(), *list = flags + slab_chunks;
              const int blocks = (int)((s.n_chunks + CMP_WAVES - 1) / CMP_WAVES);
              if (v16)
                launch_compare_w<2>(iter, blocks, c->stream, cur, shadow, nnz, s.first_chunk, (int)s.n_chunks, cd, flags);
              else
                launch_compare_w<1>(iter, blocks, c->stream, cur, shadow, nnz, s.first_chunk, (int)s.n_chunks, cd, flags);
              hipLaunchKernelGGL(k_delta_scan, dim3(1), dim3(1024), 0, c->stream, flags, (int)s.n_chunks, list, d.count[j].as<u64>());
              e = hipGetLastError();
              if (e == hipSuccess)
                e = hipMemcpyAsync(d.h_count + j, d.count[j].p, sizeof(u64), hipMemcpyDeviceToHost, c->stream);
              if (e == hipSuccess)
                e = hipEventRecord(d.ev_cmp[j], c->stream);
            }
          if (e == hipSuccess && k >= 1 && k - 1 < n_slabs) // stage 2
            {
              const int j = (int)((k - 1) & 1);
              Slab &s = sl[(k - 1) % 3];
              e = hipEventSynchronize(d.ev_cmp[j]);
              if (e != hipSuccess)
                break;
              s.count = (int64_t)d.h_count[j];
              const int64_t lo = s.first_chunk * cd, len = std::min<int64_t>(s.n_chunks * cd, nnz - lo);
              if (s.count == 0)
                s.mode = 0;
              else if (s.count == s.n_chunks || (s.count * 16 > s.n_chunks && s.count * DIRECT_DEN > s.n_chunks * DIRECT_NUM))
                {
                  s.mode = 1;
                  e = d2h_user_piece(c, h_val + lo, d_val + lo, sizeof(double) * (size_t)len, c->copy_stream);
                  st[0] += 8 * len;
                  st[4] += 1;
                }
              else
                {
                  s.mode = 2;
                  const unsigned *list = d.flags[j].as<unsigned>() + slab_chunks;
                  const int blocks = (int)((s.count + CMP_WAVES - 1) / CMP_WAVES);
                  u64 *out = d.pack[j].as<u64>();
                  if (v16)
                    hipLaunchKernelGGL(k_delta_pack<2>, dim3((unsigned)blocks), dim3(64 * CMP_WAVES), 0, c->copy_stream, cur, (long long)nnz,
                                       (long long)s.first_chunk, cd, list, (unsigned)s.count, out);
                  else
                    hipLaunchKernelGGL(k_delta_pack<1>, dim3((unsigned)blocks), dim3(64 * CMP_WAVES), 0, c->copy_stream, cur, (long long)nnz,
                                       (long long)s.first_chunk, cd, list, (unsigned)s.count, out);
                  e = hipGetLastError();
                  const size_t bytes = (size_t)s.count * (size_t)(chunk_bytes + 4);
                  if (e == hipSuccess)
                    e = hipMemcpyAsync(d.h_pack[j], out, bytes, hipMemcpyDeviceToHost, c->copy_stream);
                  st[0] += (int64_t)bytes;
                  st[5] += 1;
                }
              st[2] += s.count;
              st[6 + b] += s.count;
              if (e == hipSuccess)
                e = hipEventRecord(d.ev_dma[j], c->copy_stream);
            }
          if (e == hipSuccess && k >= 2) // stage 3
            {
              const int j = (int)(k & 1);
              const Slab &s = sl[(k - 2) % 3];
              if (s.mode == 2)
                {
                  e = hipEventSynchronize(d.ev_dma[j]);
                  if (e != hipSuccess)
                    break;
                  const double *payload = static_cast<const double *>(d.h_pack[j]);
                  const uint32_t *list = reinterpret_cast<const uint32_t *>(payload + (size_t)s.count * cd);
                  delta_scatter(h_val, nnz, cd, s.first_chunk, list, s.count, payload, n_threads);
                }
            }
        }
      return e == hipSuccess ? PFM_OK : hipfail(c, e, "pfm_values_to_host_delta (slab pipeline)");
    }
  } // namespace

  void delta_forget_host(pfm_ctx *c, const void *p)
  {
    for (int b = 0; b < 4; ++b)
      if (!p || c->delta.h_last[b] == p)
        {
          if (c->delta.h_last[b])
            c->delta.valid = false;
          c->delta.h_last[b] = nullptr;
        }
  }

  void delta_release(pfm_ctx *c)
  {
    DeltaState &d = c->delta;
    for (int j = 0; j < 2; ++j)
      {
        if (d.h_pack[j])
          (void)hipHostFree(d.h_pack[j]);
        if (d.ev_cmp[j])
          (void)hipEventDestroy(d.ev_cmp[j]);
        if (d.ev_dma[j])
          (void)hipEventDestroy(d.ev_dma[j]);
      }
    if (d.h_count)
      (void)hipHostFree(d.h_count);
    d = DeltaState{};
  }
} // namespace pfm

using namespace pfm;

extern "C"
{
  int pfm_values_to_host_delta(pfm_ctx *c, double *const *d_values, double *const *h_values, int64_t stats[10])
  {
    if (!c || !d_values || !h_values)
      return PFM_ERR_BAD_ARG;
    for (int b = 0; b < c->n_blocks; ++b) // before anything is launched or written
      if (c->block_nnz(b) > 0 && (!h_values[b] || !d_values[b]))
        return fail(c, PFM_ERR_BAD_ARG, "pfm_values_to_host_delta: null block");
    (void)hipSetDevice(c->device);
    DeltaState &d = c->delta;
    const int64_t chunk_bytes = chunk_bytes_of(c), slab_bytes = slab_bytes_of(c), slab_chunks = slab_bytes / chunk_bytes;
    const int cd = (int)(chunk_bytes / 8);
    if (const int rc = ensure_resources(c, slab_chunks, chunk_bytes))
      {
        d.valid = false;
        return rc;
      }
    int64_t st[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int n_threads = delta_host_threads();
    const bool was_valid = d.valid;
    d.valid = false; // until the call has come through: after an error the shadow may be ahead of the host
    std::vector<std::thread> clearing; // the (u,phi) block of a registered array, cleared next to the other blocks' transfers
    int rc = PFM_OK;
    hipError_t e = hipEventRecord(c->ev_copy, c->stream); // the copy stream starts behind the work that made d_values
    if (e == hipSuccess)
      e = hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0);
    // the (u,phi) block last: its clearing threads have the other blocks' time
    const int order4[4] = {0, 2, 3, 1}, order1[1] = {0};
    const int *order = c->n_blocks == 4 ? order4 : order1;
    bool clear_up = false;
    if (c->n_blocks == 4 && c->block_nnz(1) > 0 && !(was_valid && d.h_last[1] == h_values[1]))
      if (pfm_ctx::HostPin *hp = find_pin(c, h_values[1], sizeof(double) * (size_t)c->block_nnz(1)))
        {
          clear_up = true;
          if (!hp->zeroed)
            {
              const size_t bytes = sizeof(double) * (size_t)c->block_nnz(1);
              const size_t piece = ((bytes / (size_t)n_threads) + 4095) & ~(size_t)4095;
              char *h = reinterpret_cast<char *>(h_values[1]);
              for (int t = 0; t < n_threads; ++t)
                {
                  const size_t lo = std::min(bytes, (size_t)t * piece), hi = std::min(bytes, lo + piece);
                  if (hi > lo)
                    clearing.emplace_back([=] { std::memset(h + lo, 0, hi - lo); });
                }
              hp->zeroed = true;
            }
        }
    for (int ib = 0; ib < c->n_blocks && rc == PFM_OK && e == hipSuccess; ++ib)
      {
        const int b = order[ib];
        const int64_t nnz = c->block_nnz(b);
        if (!nnz)
          continue;
        const int64_t n_chunks = (nnz + cd - 1) / cd, n_slabs = (n_chunks + slab_chunks - 1) / slab_chunks;
        st[1] += 8 * nnz;
        st[3] += n_chunks;
        const bool known = was_valid && d.h_last[b] == h_values[b];
        if (!known && b == 1 && clear_up)
          {
            // the host holds zeros: so does the shadow, and the compare ships what is not +0.0 on the device
            e = hipMemsetAsync(d.shadow[b].p, 0, sizeof(double) * (size_t)nnz, c->stream);
            for (auto &t : clearing)
              t.join();
            clearing.clear();
          }
        else if (!known)
          {
            // all of the block, as pfm_values_to_host sends it; the shadow is filled on the other stream meanwhile
            hipStream_t s_link = b == 0 ? c->stream : c->copy_stream, s_dev = b == 0 ? c->copy_stream : c->stream;
            e = d2h_user_piece(c, h_values[b], d_values[b], sizeof(double) * (size_t)nnz, s_link);
            if (e == hipSuccess)
              e = hipMemcpyAsync(d.shadow[b].p, d_values[b], sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, s_dev);
            st[0] += 8 * nnz;
            st[2] += n_chunks;
            st[4] += n_slabs;
            st[6 + b] += n_chunks;
            continue;
          }
        if (e == hipSuccess)
          rc = delta_block(c, b, d_values[b], h_values[b], chunk_bytes, slab_chunks, n_threads, st);
      }
    for (auto &t : clearing)
      t.join();
    // join the copy stream, wait for everything (also after an error: nothing of this call runs on when it returns)
    hipError_t ej = hipEventRecord(c->ev_copy, c->copy_stream);
    if (ej == hipSuccess)
      ej = hipStreamWaitEvent(c->stream, c->ev_copy, 0);
    const hipError_t es = hipStreamSynchronize(c->stream), ec = hipStreamSynchronize(c->copy_stream);
    if (rc != PFM_OK)
      return rc;
    for (hipError_t x : {e, ej, es, ec})
      if (x != hipSuccess)
        return hipfail(c, x, "pfm_values_to_host_delta");
    for (int b = 0; b < 4; ++b)
      d.h_last[b] = b < c->n_blocks ? h_values[b] : nullptr;
    d.valid = true;
    if (stats)
      std::copy(st, st + 10, stats);
    return PFM_OK;
  }

  int pfm_values_delta_reset(pfm_ctx *c)
  {
    if (!c)
      return PFM_ERR_BAD_ARG;
    // the registered (u,phi) array is no longer known to hold zeros either
    if (c->n_blocks == 4 && c->delta.h_last[1])
      for (auto &hp : c->host_pins)
        if (hp.p == c->delta.h_last[1])
          hp.zeroed = false;
    c->delta.valid = false;
    for (auto &h : c->delta.h_last)
      h = nullptr;
    return PFM_OK;
  }

  int pfm_values_delta_config(pfm_ctx *c, int64_t chunk_bytes, int64_t slab_bytes)
  {
    if (!c || chunk_bytes < 0 || slab_bytes < 0)
      return PFM_ERR_BAD_ARG;
    if (chunk_bytes && (chunk_bytes < 64 || (chunk_bytes & (chunk_bytes - 1)) || chunk_bytes > (1ll << 30)))
      return fail(c, PFM_ERR_BAD_ARG, "pfm_values_delta_config: chunk_bytes must be a power of two >= 64");
    const int64_t cb = chunk_bytes ? chunk_bytes : DELTA_CHUNK_DEFAULT;
    if (slab_bytes && (slab_bytes % cb || slab_bytes / cb > DELTA_SLAB_MAX_CHUNKS))
      return fail(c, PFM_ERR_BAD_ARG, "pfm_values_delta_config: slab_bytes must be a multiple of chunk_bytes (at most 2^24 chunks)");
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    release_staging(c);
    c->delta.chunk_bytes = chunk_bytes;
    c->delta.slab_bytes = slab_bytes;
    return pfm_values_delta_reset(c);
  }

  int pfm_values_delta_info(const pfm_ctx *c, int64_t out[4])
  {
    if (!c || !out)
      return PFM_ERR_BAD_ARG;
    const DeltaState &d = c->delta;
    out[0] = chunk_bytes_of(c);
    out[1] = slab_bytes_of(c);
    out[2] = 0;
    for (int b = 0; b < 4; ++b)
      out[2] += (int64_t)d.shadow[b].bytes;
    for (int j = 0; j < 2; ++j)
      out[2] += (int64_t)(d.flags[j].bytes + d.count[j].bytes + d.pack[j].bytes);
    out[3] = d.valid ? 1 : 0;
    return PFM_OK;
  }
}
