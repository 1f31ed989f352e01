// sf_block.h -- workgroup primitives of the catalogue tools: plain LDS loops in a fixed order, so that every call gives
// the same bits (the fp64 sums feed kde_var and the CDF of the imputation, and tests compare bits between calls).
#pragma once
#include <hip/hip_runtime.h>

// sum of one value per thread over a workgroup of 256: halving tree from 128 (s_red: 256 words of T)
template <class T>
__device__ __forceinline__ T sf_block_sum(T v, T* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  return s_red[0];
}

// exclusive scan of one int per thread over a workgroup of NT (Hillis-Steele on s_part, NT words): returns the sum of the
// values of the threads below this one, *total = the sum of all.  (s_part is read until the return: a second scan over the
// same words needs a __syncthreads() in between.)
template <int NT>
__device__ __forceinline__ int sf_block_exscan(int v, int* s_part, int* total) {
  const int tid = threadIdx.x;
  s_part[tid] = v;
  __syncthreads();
  for (int o = 1; o < NT; o <<= 1) {
    const int u = tid >= o ? s_part[tid - o] : 0;
    __syncthreads();
    s_part[tid] += u;
    __syncthreads();
  }
  *total = s_part[NT - 1];
  return s_part[tid] - v;
}
