// Stand-alone check of the host scatter of pfm_values_to_host_delta (cracks_amd/csrc/pfm_delta_host.h): built with
// -fsanitize=address,undefined by tests/test_delta_host.py.  Every case scatters a payload into a guarded destination and
// compares the whole buffer, guards included, with a reference written by a plain loop.
#include "pfm_delta_host.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace
{
  int failures = 0;

  uint64_t pattern(int64_t chunk, int64_t word) { return 0xA5A5000000000000ull ^ ((uint64_t)chunk << 20) ^ (uint64_t)word; }

  // block of block_len doubles at an offset of `shift` bytes (8-byte aligned only when shift = 8) inside a buffer with
  // guard words on both sides; list = chunks (relative to first_chunk) to overwrite
  void run_case(const char *name, int64_t block_len, int64_t cd, int64_t first_chunk, const std::vector<uint32_t> &list, int threads, int shift)
  {
    const int64_t guard = 32;
    std::vector<uint64_t> buf((size_t)(block_len + 2 * guard + 2)), ref;
    for (size_t i = 0; i < buf.size(); ++i)
      buf[i] = 0x1111111100000000ull + i;
    // a destination that is 8 mod 16: buf.data() is 16-byte aligned (operator new), so one extra word shifts it
    const int64_t lead = guard + (shift == 8 ? ((reinterpret_cast<uintptr_t>(buf.data()) & 15u) == 0 ? 1 : 0)
                                             : ((reinterpret_cast<uintptr_t>(buf.data()) & 15u) == 0 ? 0 : 1));
    ref = buf;
    const int64_t count = (int64_t)list.size();
    // payload and list as the device leaves them: count chunks, then the list
    std::vector<uint64_t> stage((size_t)(count * cd + (count + 1) / 2 + 1), 0xDEADDEADDEADDEADull);
    for (int64_t i = 0; i < count; ++i)
      for (int64_t w = 0; w < cd; ++w)
        stage[(size_t)(i * cd + w)] = pattern(first_chunk + list[(size_t)i], w);
    if (count)
      std::memcpy(stage.data() + count * cd, list.data(), (size_t)count * sizeof(uint32_t));
    for (int64_t i = 0; i < count; ++i)
      for (int64_t w = 0; w < cd; ++w)
        {
          const int64_t at = (first_chunk + list[(size_t)i]) * cd + w;
          if (at < block_len)
            ref[(size_t)(lead + at)] = pattern(first_chunk + list[(size_t)i], w);
        }
    double *dst = reinterpret_cast<double *>(buf.data() + lead);
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) != (uintptr_t)shift)
      {
        std::printf("FAIL %s: destination alignment\n", name);
        ++failures;
        return;
      }
    pfm::delta_scatter(dst, block_len, cd, first_chunk, reinterpret_cast<const uint32_t *>(stage.data() + count * cd), count,
                       reinterpret_cast<const double *>(stage.data()), threads, /*min_bytes_per_thread=*/0);
    if (std::memcmp(buf.data(), ref.data(), buf.size() * sizeof(uint64_t)) != 0)
      {
        std::printf("FAIL %s\n", name);
        ++failures;
      }
    else
      std::printf("ok   %s\n", name);
  }
} // namespace

int main()
{
  for (int threads : {1, 16})
    for (int shift : {0, 8})
      {
        // 10 chunks of 64 doubles + a tail chunk of 5: the tail chunk is listed and must be clamped
        run_case("tail chunk", 645, 64, 0, {0, 3, 10}, threads, shift);
        // second slab of a block (first_chunk > 0), every chunk of it, tail of 1 double
        run_case("whole slab with tail", 16 * 8 + 1, 8, 8, {0, 1, 2, 3, 4, 5, 6, 7, 8}, threads, shift);
        run_case("empty list", 300, 8, 0, {}, threads, shift);
        run_case("fewer chunks than threads", 4096, 64, 4, {1, 7, 30}, threads, shift);
        run_case("one chunk", 7, 8, 0, {0}, threads, shift); // block shorter than a chunk
        std::vector<uint32_t> many;
        for (uint32_t i = 0; i < 200; i += 3)
          many.push_back(i);
        run_case("many chunks", 200 * 16 - 9, 16, 0, many, threads, shift);
      }
  // the thread count follows PFM_HOST_THREADS, at most 16
  setenv("PFM_HOST_THREADS", "3", 1);
  if (pfm::delta_host_threads() != 3)
    ++failures, std::printf("FAIL PFM_HOST_THREADS=3\n");
  setenv("PFM_HOST_THREADS", "64", 1);
  if (pfm::delta_host_threads() != 16)
    ++failures, std::printf("FAIL PFM_HOST_THREADS=64\n");
  std::printf(failures ? "delta_scatter: FAILED\n" : "delta_scatter: OK\n");
  return failures ? 1 : 0;
}
