// pfm_reduce.h -- the one fixed-order reduction of the device-side entries (pfm_newton.hip, pfm_postproc.hip, pfm_adapt.hip).
// Device only.  A value is reduced in two stages, each by a block of 256 threads:
//
//   first stage    every thread brings one value per component; block_reduce() leaves the block's result, which the kernel
//                  writes to partial[block][component];
//   second stage   k_reduce_final, one block: thread t folds partial[t], partial[t + 256], ... in ascending order
//                  (fold_partials), then the same block_reduce().
//
// block_reduce(): the 64 lanes of a wave by xor-shuffles with offsets 32, 16, ..., 1, lane 0 of each wave writes to LDS,
// one barrier, result ((w0 op w1) op w2) op w3.  No atomics: the order of every floating-point sum is fixed by the
// launch geometry alone, so repeated calls are bitwise identical.
#pragma once

#include <hip/hip_runtime.h>

namespace pfm
{
  // largest first-stage grid of the residual norms (pfm_residual_norms and the norm stage of pfm_line_search_device, which
  // reproduces its sums bit for bit): longer vectors are walked grid-stride
  constexpr int NORM_BLOCKS_MAX = 2048;

  // operators: op(a, b, k) combines two values of component k, init(k) is the neutral element the folds start from
  template <class T>
  struct Sum
  {
    static __device__ __forceinline__ T init(int) { return T(0); }
    __device__ __forceinline__ T operator()(T a, T b, int) const { return a + b; }
  };
  struct Min
  {
    static __device__ __forceinline__ double init(int) { return HUGE_VAL; }
    __device__ __forceinline__ double operator()(double a, double b, int) const { return fmin(a, b); }
  };
  struct SumMax // component 0: a sum, component 1: the maximum of non-negative values (the norms of a residual)
  {
    static __device__ __forceinline__ double init(int) { return 0.0; }
    __device__ __forceinline__ double operator()(double a, double b, int k) const { return k == 0 ? a + b : fmax(a, b); }
  };

  // The waves' values w[0 .. N) (lane 0 of each wave counts) combined over the 4 waves of the block, which must all call
  // it.  Thread k < N returns component k (the other threads component 0).  A kernel calls one instantiation once (the
  // LDS words are not guarded for a second round).
  template <int N, class T, class Op>
  __device__ __forceinline__ T combine_waves(const T (&w)[N], Op op)
  {
    __shared__ T s_red[4][N];
    if ((threadIdx.x & 63) == 0)
      {
#pragma unroll
        for (int k = 0; k < N; ++k)
          s_red[threadIdx.x >> 6][k] = w[k];
      }
    __syncthreads();
    const int k = threadIdx.x < N ? threadIdx.x : 0;
    return op(op(op(s_red[0][k], s_red[1][k], k), s_red[2][k], k), s_red[3][k], k);
  }

  // reduction of acc[0 .. N) over the 256 threads of the block
  template <int N, class T, class Op>
  __device__ __forceinline__ T block_reduce(const T (&acc)[N], Op op)
  {
    T w[N];
#pragma unroll
    for (int k = 0; k < N; ++k)
      {
        w[k] = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
          w[k] = op(w[k], __shfl_xor(w[k], off), k);
      }
    return combine_waves(w, op);
  }

  // the number of threads of the block with `flag`: the integer sum of block_reduce, its wave stage done by a ballot
  __device__ __forceinline__ unsigned long long block_count(bool flag)
  {
    const unsigned long long w[1] = {(unsigned long long)__popcll(__ballot(flag))};
    return combine_waves(w, Sum<unsigned long long>{});
  }

  // second stage, the fold: acc[k] = init op partial[t][k] op partial[t + 256][k] op ... for thread t
  template <int N, class T, class Op>
  __device__ __forceinline__ void fold_partials(const T *__restrict__ partial, long long n, T (&acc)[N], Op op)
  {
    for (int k = 0; k < N; ++k)
      {
        T r = Op::init(k);
        for (long long i = threadIdx.x; i < n; i += 256)
          r = op(r, partial[i * N + k], k);
        acc[k] = r;
      }
  }

  // second stage of partial[n][N] into out[N]; launched with one block of 256 threads
  template <class T, int N, class Op>
  __global__ __launch_bounds__(256) void k_reduce_final(const T *__restrict__ partial, long long n, T *__restrict__ out)
  {
    T acc[N];
    fold_partials(partial, n, acc, Op{});
    const T r = block_reduce(acc, Op{});
    if (threadIdx.x < N)
      out[threadIdx.x] = r;
  }
} // namespace pfm
