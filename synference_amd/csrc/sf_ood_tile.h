// sf_ood_tile.h -- the all-pairs tile shared by the out-of-distribution kernels (sf_ood.hip) and the kernel sums of the
// misspecification test (sf_mmd.hip): one thread per query with its row in registers (CP = C rounded up to 4), the base streamed
// through LDS in chunks of SF_OOD_CH rows, two rows interleaved per column so that one broadcast ds_read_b128 feeds two packed
// fp32 operations.  Squared distance, the same bits wherever it is computed:
//   acc = 0; for c ascending: t = q[c] - b[c]; acc = acc + t * t      every operation rounded to nearest in fp32, no fma
#pragma once
#include <hip/hip_runtime.h>

#define SF_OOD_CMAX 64
#define SF_OOD_CH 128     // base rows per LDS chunk

typedef float sf_f2 __attribute__((ext_vector_type(2)));
typedef float sf_f4 __attribute__((ext_vector_type(4)));

// rows [r0, r0 + SF_OOD_CH) of base[N,C] -> s_b[pair][CP][2]; rows past r1 become +inf (never under a bound), pad columns 0
template <int CP>
__device__ __forceinline__ void sf_ood_load_chunk(const float* __restrict__ base, long r0, long r1, int C, unsigned magic,
                                                  float* s_b) {
  const int nthr = blockDim.x;
  if (CP != C) {
    for (int e = threadIdx.x; e < SF_OOD_CH * CP; e += nthr) s_b[e] = 0.f;
    __syncthreads();
  }
  const int ne = SF_OOD_CH * C;
  const long left = (r1 - r0) * C;   // elements of live rows
  const float* src = base + r0 * C;
  for (int e = threadIdx.x; e < ne; e += nthr) {
    const int r = (int)(((unsigned)e * magic) >> 20);   // e / C for e < 2^14, C <= 64
    const int c = e - r * C;
    s_b[((r >> 1) * CP + c) * 2 + (r & 1)] = e < left ? src[e] : __builtin_inff();
  }
}

// squared distances of the query to the two rows of pair p
template <int CP>
__device__ __forceinline__ sf_f2 sf_ood_d2pair(const float (&q)[CP], const float* s_b, int p) {
#pragma clang fp contract(off)   // the square is not fused into the sum: the bits of the numpy model
  const sf_f4* b = (const sf_f4*)(s_b + p * CP * 2);
  sf_f2 acc = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < CP; c += 2) {
    const sf_f4 v = b[c >> 1];
    const sf_f2 q0 = {q[c], q[c]}, q1 = {q[c + 1], q[c + 1]};
    const sf_f2 b0 = {v.x, v.y}, b1 = {v.z, v.w};
    const sf_f2 t0 = q0 - b0;
    acc = acc + t0 * t0;
    const sf_f2 t1 = q1 - b1;
    acc = acc + t1 * t1;
  }
  return acc;
}

template <int CP>
__device__ __forceinline__ void sf_ood_load_query(const float* __restrict__ query, long m, bool live, int C, float (&q)[CP]) {
#pragma unroll
  for (int c = 0; c < CP; ++c) q[c] = (live && c < C) ? query[m * C + c] : 0.f;
}

// one instantiation per padded width: L<CP>::go(a...)
template <template <int> class L, class... A>
void sf_ood_dispatch(int CP, A... a) {
  switch (CP) {
    case 4: L<4>::go(a...); break;
    case 8: L<8>::go(a...); break;
    case 12: L<12>::go(a...); break;
    case 16: L<16>::go(a...); break;
    case 20: L<20>::go(a...); break;
    case 24: L<24>::go(a...); break;
    case 28: L<28>::go(a...); break;
    case 32: L<32>::go(a...); break;
    case 36: L<36>::go(a...); break;
    case 40: L<40>::go(a...); break;
    case 44: L<44>::go(a...); break;
    case 48: L<48>::go(a...); break;
    case 52: L<52>::go(a...); break;
    case 56: L<56>::go(a...); break;
    case 60: L<60>::go(a...); break;
    default: L<64>::go(a...); break;
  }
}
