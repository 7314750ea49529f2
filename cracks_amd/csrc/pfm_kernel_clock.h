// pfm_kernel_clock.h -- device counters of the phase clocks of k_cart_uu3 and k_cart_phi4 (profiling: PFM_UU_CLK,
// PFM_PHI_CLK).  One object per context, hence per device, owns the buffer: it grows to what a launch needs and goes with
// the context.  The launcher reserves zeroed counters in front of its launch; the kernel's report reads them back behind it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <vector>

namespace pfm
{
  struct KernelClock
  {
    unsigned long long *d = nullptr;
    size_t cap = 0;
    ~KernelClock() { (void)hipFree(d); }
    unsigned long long *reserve(size_t n, hipStream_t s) // n counters, zeroed on s; nullptr: no memory
    {
      if (n > cap)
        {
          (void)hipFree(d); // (synchronises the device: no earlier launch still counts into it)
          d = nullptr, cap = 0;
          if (hipMalloc((void **)&d, n * sizeof(unsigned long long)) != hipSuccess)
            return d = nullptr;
          cap = n;
        }
      (void)hipMemsetAsync(d, 0, n * sizeof(unsigned long long), s);
      return d;
    }
    void sums(size_t n, int stride, unsigned long long *h) const // h[i] = counters i, i + stride, ... of the first n (blocks)
    {
      std::vector<unsigned long long> all(n);
      (void)hipMemcpy(all.data(), d, n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
      std::fill(h, h + stride, 0ull);
      for (size_t i = 0; i < n; ++i)
        h[i % stride] += all[i];
    }
  };
} // namespace pfm
