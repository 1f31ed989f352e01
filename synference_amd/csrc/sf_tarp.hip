// sf_tarp.hip -- TARP coverage on the device: "Tests of Accuracy with Random Points", Lemos et al.
// 2023, "Sampling-Based Accuracy Testing of Posterior Estimators", restated from the paper; the reference reaches it
// through the third-party `tarp` package (ref: src/synference/sbi_runner.py:7090-7126, 6618-6637):
//   tarp.get_tarp_coverage(samples, y, norm=True, bootstrap=True, num_bootstrap=200)
// One pass over a row list idx[0..N) and reference points r[j,:]: with i = idx[j],
//   k_j = #{ s : dist(r_j, x[i,s,:]) < dist(r_j, theta[i,:]) }   (after the optional min/max normalisation of both)
// and the expected-coverage curve is the cumulative histogram of f_j = k_j / S.  A bootstrap call makes B such passes,
// each with its own resample of the rows (Philox stream 3) and its own reference points (stream 4).
//
// Row-major over the draws: the B*N occurrences (b, j) are grouped by the row they draw (counting sort on idx), a
// workgroup stages one row's raw draws in LDS once ([d][s] order, tiles of <= 32 KB) and its waves walk that row's
// occurrences, so the (N,S,D) draw set is read from HBM once per call and not once per pass.  Counts are int32, every
// occurrence owns its cell (plain stores), and the curve is built from integer prefix sums: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <string>

#include "sf_block.h"
#include "sf_internal.h"
#include "sf_rng.h"
#include "sf_scratch.h"

#define SF_TARP_DMAX 16
#define SF_TARP_SMAX 8192
#define SF_TARP_TILE_FLOATS 8192  // draws staged per tile: D * TS <= this (32 KB: several workgroups per CU)

// ---- 1. row resample + how often every row is drawn ---------------------------------------------------------------
// cell c = b * N + j: idx[c] = (uint64(r0) * N) >> 32 with r = philox(counter (j, 0, b, 0), key (seed, stream 3));
// boot == 0: the rows in order
__global__ void k_tarp_resample(int N, long cells, int boot, uint32_t k0, uint32_t k1, int32_t* __restrict__ idx,
                                int32_t* __restrict__ rowcnt) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) {
    const int b = (int)(c / N), j = (int)(c - (long)b * N);
    int i = j;
    if (boot) {
      uint32_t r[4];
      sf_philox4x32_10((uint32_t)j, 0u, (uint32_t)b, 0u, k0, k1, r);
      i = (int)(((uint64_t)r[0] * (uint64_t)N) >> 32);
    }
    idx[c] = i;
    atomicAdd(&rowcnt[i], 1);
  }
}

// ---- 2. exclusive scan of the row counts: sf_launch_exclusive_scan_i32 (the total is B * N < 2^31) ----------------------

// ---- 3. occurrence list grouped by row (rowcnt counts down to 0; the order inside a row does not matter) -----------
__global__ void k_tarp_scatter(long cells, const int32_t* __restrict__ idx, const int32_t* __restrict__ offs,
                               int32_t* __restrict__ rowcnt, int32_t* __restrict__ occ) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) {
    const int i = idx[c];
    occ[offs[i] + atomicSub(&rowcnt[i], 1) - 1] = (int32_t)c;
  }
}

// ---- 4. norm_axis 0: per pass and parameter, low and 1 / (high - low + 1e-10) over the resampled truths ------------
// one workgroup per pass; a NaN truth makes low / high NaN (numpy's min / max)
__global__ __launch_bounds__(256) void k_tarp_minmax(const float* __restrict__ theta, const int32_t* __restrict__ idx, int N,
                                                     int D, float* __restrict__ lowinv) {
  __shared__ float s_mn[4], s_mx[4];
  __shared__ int s_nan[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* ib = idx + (long)b * N;
  for (int d = 0; d < D; ++d) {
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int nan = 0;
    for (int j = threadIdx.x; j < N; j += 256) {
      const float v = theta[(long)ib[j] * D + d];
      nan |= (v != v) ? 1 : 0;
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      nan |= __shfl_xor(nan, o, 64);
    }
    __syncthreads();  // the previous parameter's partials have been read
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; s_nan[wave] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w) { mn = fminf(mn, s_mn[w]); mx = fmaxf(mx, s_mx[w]); nan |= s_nan[w]; }
      if (nan) mn = mx = __builtin_nanf("");
      lowinv[((long)b * D + d) * 2] = mn;
      lowinv[((long)b * D + d) * 2 + 1] = 1.0f / (mx - mn + 1e-10f);
    }
  }
}

// ---- 5. the counts -----------------------------------------------------------------------------------------------
// distance of the reference point to one (normalised) point; the truth and the draws go through the same arithmetic,
// products and sums rounded one by one.  Euclidean: the SQUARED distance (both sides of the comparison are squares).
template <int D, int METRIC>
__device__ __forceinline__ float sf_tarp_dist(const float (&v)[D], const float (&r)[D], const float (&lo)[D],
                                              const float (&inv)[D]) {
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float df = __fsub_rn(r[d], __fmul_rn(__fsub_rn(v[d], lo[d]), inv[d]));
    acc = METRIC == 0 ? __fmaf_rn(df, df, acc) : __fadd_rn(acc, fabsf(df));
  }
  return acc;
}

// one 256-thread workgroup per row i: stage a tile of the row's draws in LDS as [d][s] (row stride TSP = TS + 1 words),
// then wave w takes occurrences w, w + 4, ... of the row's list; per occurrence the reference point, low, 1 / range and
// the truth's distance are the same in every lane, per 64 draws one ballot and a population count.  A later tile adds
// to the cell its own wave wrote for the first tile.
template <int D, int METRIC>
__global__ __launch_bounds__(256) void k_tarp_count(const float* __restrict__ samples, const float* __restrict__ theta,
                                                    const float* __restrict__ refs, const float* __restrict__ lowinv,
                                                    int norm_axis, int N, int S, int TS, const int32_t* __restrict__ offs,
                                                    const int32_t* __restrict__ occ, uint32_t k0, uint32_t k1,
                                                    int32_t* __restrict__ counts) {
  extern __shared__ float sm[];
  const int i = blockIdx.x;
  const int o0 = offs[i], o1 = offs[i + 1];
  if (o0 == o1) return;  // a row no pass drew
  const int TSP = TS + 1;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float th[D];
#pragma unroll
  for (int d = 0; d < D; ++d) th[d] = theta[(long)i * D + d];
  float lo1 = 0.f, inv1 = 1.f;  // norm_axis 1: min / max of the row's own truth over the parameters
  if (norm_axis == 1) {
    float mn = th[0], mx = th[0];
    bool nan = th[0] != th[0];
#pragma unroll
    for (int d = 1; d < D; ++d) { mn = fminf(mn, th[d]); mx = fmaxf(mx, th[d]); nan = nan || th[d] != th[d]; }
    if (nan) mn = mx = __builtin_nanf("");
    lo1 = mn;
    inv1 = 1.0f / (mx - mn + 1e-10f);
  }
  for (int t0 = 0; t0 < S; t0 += TS) {
    const int ts = S - t0 < TS ? S - t0 : TS;
    __syncthreads();  // every wave has finished with the previous tile
    const float* src = samples + ((long)i * S + t0) * D;
    for (int e = threadIdx.x; e < ts * D; e += 256) {
      const int s = e / D, d = e - s * D;
      sm[d * TSP + s] = src[e];
    }
    __syncthreads();
    for (int o = o0 + wave; o < o1; o += 4) {
      const int c = occ[o];
      const int b = c / N, j = c - b * N;
      float r[D], lo[D], inv[D];
      if (refs) {
#pragma unroll
        for (int d = 0; d < D; ++d) r[d] = refs[(long)j * D + d];
      } else {
#pragma unroll
        for (int q = 0; q < (D + 3) / 4; ++q) {
          uint32_t u[4];
          sf_philox4x32_10((uint32_t)j, 0u, (uint32_t)b, (uint32_t)q, k0, k1, u);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (q * 4 + t < D) r[q * 4 + t] = sf_u01(u[t]);
        }
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {
        if (norm_axis == 0) {
          lo[d] = lowinv[((long)b * D + d) * 2];
          inv[d] = lowinv[((long)b * D + d) * 2 + 1];
        } else {
          lo[d] = lo1;
          inv[d] = inv1;
        }
      }
      const float dth = sf_tarp_dist<D, METRIC>(th, r, lo, inv);
      int cnt = 0;
      for (int s = lane; s - lane < ts; s += 64) {  // whole groups of 64: the words past ts are read and masked
        float v[D];
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = sm[d * TSP + s];
        const float ds = sf_tarp_dist<D, METRIC>(v, r, lo, inv);
        cnt += __popcll(__ballot(s < ts && ds < dth));  // a NaN draw compares false
      }
      if (lane == 0) counts[c] = t0 == 0 ? cnt : counts[c] + cnt;
    }
  }
}

// ---- 6. the coverage curve of every pass ---------------------------------------------------------------------------
// one workgroup per pass: histogram of the counts (S + 1 bins), min / max, exclusive prefix sums below[k] = #{j : k_j < k}
// (k = 0 .. S + 1), the float64 edges of np.histogram / np.linspace -- e * step + first as a multiply and an add,
// edges[n] = last -- and ecp[e] = below[k*] / N at the smallest k* with (double)k* / (double)S >= edges[e].
__global__ __launch_bounds__(256) void k_tarp_curve(const int32_t* __restrict__ counts, int N, int S, int nb, int B,
                                                    double* __restrict__ ecp, double* __restrict__ alpha) {
  extern __shared__ int h[];  // S + 2 words
  __shared__ int part[256];
  __shared__ int s_min, s_max;
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < S + 2; k += 256) h[k] = 0;
  if (tid == 0) { s_min = S; s_max = 0; }
  __syncthreads();
  int mn = S, mx = 0;
  for (int j = tid; j < N; j += 256) {
    int k = counts[(long)b * N + j];
    k = k < 0 ? 0 : (k > S ? S : k);
    atomicAdd(&h[k], 1);
    mn = k < mn ? k : mn;
    mx = k > mx ? k : mx;
  }
  atomicMin(&s_min, mn);
  atomicMax(&s_max, mx);
  __syncthreads();
  const int chunk = (S + 2 + 255) / 256;
  const int lo = tid * chunk, hi = lo + chunk < S + 2 ? lo + chunk : S + 2;
  int s = 0;
  for (int k = lo; k < hi; ++k) s += h[k];
  int tot;
  int run = sf_block_exscan<256>(s, part, &tot);
  for (int k = lo; k < hi; ++k) {
    const int c = h[k];
    h[k] = run;
    run += c;
  }
  __syncthreads();
  double first = (double)s_min / (double)S, last = (double)s_max / (double)S;
  if (s_min == s_max) { first -= 0.5; last += 0.5; }
  const double step = (last - first) / (double)nb;
  for (int e = tid; e <= nb; e += 256) {
    double edge = last;
    if (e < nb) {
#pragma clang fp contract(off)  // numpy's linspace: the product is rounded before the sum (no fused multiply-add)
      const double prod = (double)e * step;
      edge = prod + first;
    }
    double val = e == 0 ? 0.0 : 1.0;
    if (e > 0 && e < nb) {
      const double x = floor(edge * (double)S);
      int k = x < 0.0 ? 0 : (x > (double)(S + 1) ? S + 1 : (int)x);
      while (k > 0 && (double)(k - 1) / (double)S >= edge) --k;
      while (k <= S && (double)k / (double)S < edge) ++k;
      val = (double)h[k] / (double)N;
    }
    ecp[(long)b * (nb + 1) + e] = val;
    if (alpha && b == B - 1) alpha[e] = edge;
  }
}

// ---- scratch: sf_scratch.h ------------------------------------------------------------------------------------------
namespace {
SfScratch g_tarp_scratch;

template <int METRIC>
hipError_t launch_count(int D, dim3 grid, size_t lds, hipStream_t st, const float* samples, const float* theta,
                        const float* refs, const float* lowinv, int norm_axis, int N, int S, int TS, const int32_t* offs,
                        const int32_t* occ, uint32_t k0, uint32_t k1, int32_t* counts) {
#define SF_TARP_CASE(d)                                                                                                  \
  case d:                                                                                                                \
    hipLaunchKernelGGL((k_tarp_count<d, METRIC>), grid, dim3(256), lds, st, samples, theta, refs, lowinv, norm_axis, N, \
                       S, TS, offs, occ, k0, k1, counts);                                                                \
    break;
  switch (D) {
    SF_TARP_CASE(1) SF_TARP_CASE(2) SF_TARP_CASE(3) SF_TARP_CASE(4) SF_TARP_CASE(5) SF_TARP_CASE(6) SF_TARP_CASE(7)
    SF_TARP_CASE(8) SF_TARP_CASE(9) SF_TARP_CASE(10) SF_TARP_CASE(11) SF_TARP_CASE(12) SF_TARP_CASE(13)
    SF_TARP_CASE(14) SF_TARP_CASE(15) SF_TARP_CASE(16)
    default: return hipErrorInvalidValue;
  }
#undef SF_TARP_CASE
  return hipGetLastError();
}
}  // namespace

extern "C" int sf_tarp_coverage(const float* samples, const float* theta, int64_t N, int64_t S, int32_t D,
                                const float* references, int32_t metric, int32_t norm_axis, int32_t num_bootstrap,
                                int32_t num_alpha_bins, uint64_t seed, double* ecp, double* alpha, int32_t* counts,
                                int32_t* boot_idx, void* stream) {
  if (!samples || !theta || !ecp) { sf_set_error("sf_tarp_coverage: null argument"); return SF_ERR_INVALID; }
  if (D < 1 || D > SF_TARP_DMAX || S < 1 || S > SF_TARP_SMAX || N < 1 || num_alpha_bins < 1 || num_bootstrap < 0) {
    sf_set_error("sf_tarp_coverage: need 1 <= D <= 16, 1 <= S <= 8192, N >= 1, num_alpha_bins >= 1, num_bootstrap >= 0");
    return SF_ERR_INVALID;
  }
  if (metric < 0 || metric > 1 || norm_axis < -1 || norm_axis > 1) {
    sf_set_error("sf_tarp_coverage: metric is 0 (euclidean) or 1 (manhattan), norm_axis -1 (none), 0 or 1");
    return SF_ERR_INVALID;
  }
  const int64_t B = num_bootstrap > 0 ? num_bootstrap : 1;
  if (N > 0x7fffffffll / B) {  // B * N < 2^31: a cell index is an int32
    sf_set_error("sf_tarp_coverage: num_bootstrap * N must be below 2^31");
    return SF_ERR_INVALID;
  }
  const int boot = num_bootstrap > 0 ? 1 : 0;
  const size_t cells = (size_t)(B * N);
  hipStream_t st = (hipStream_t)stream;
  // scratch: [idx] [counts] rowcnt offs occ lowinv
  const bool own_idx = !(boot && boot_idx), own_counts = !counts;
  SfScratchCall ws(g_tarp_scratch, "sf_tarp_coverage", st);
  const int sub_idx = own_idx ? ws.add(cells * 4) : -1, sub_cnt = own_counts ? ws.add(cells * 4) : -1;
  const int sub_rowcnt = ws.add(((size_t)N + 1) * 4), sub_offs = ws.add(((size_t)N + 1) * 4), sub_occ = ws.add(cells * 4);
  const int sub_norm = norm_axis == 0 ? ws.add((size_t)B * D * 2 * 4) : -1;
  if (int rc = ws.reserve()) return rc;
  int32_t* idx = own_idx ? ws.get<int32_t>(sub_idx) : boot_idx;
  int32_t* cnt = own_counts ? ws.get<int32_t>(sub_cnt) : counts;
  int32_t* rowcnt = ws.get<int32_t>(sub_rowcnt);
  int32_t* offs = ws.get<int32_t>(sub_offs);
  int32_t* occ = ws.get<int32_t>(sub_occ);
  float* lowinv = norm_axis == 0 ? ws.get<float>(sub_norm) : nullptr;
  if (int rc = ws.check()) return rc;
  hipError_t e;

  const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32);
  if ((e = hipMemsetAsync(rowcnt, 0, ((size_t)N + 1) * 4, st)) != hipSuccess) return ws.fail("hipMemsetAsync", e);
  size_t blocks = (cells + 255) / 256;
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(k_tarp_resample, dim3((unsigned)blocks), dim3(256), 0, st, (int)N, (long)cells, boot, s_lo, s_hi ^ 3u, idx,
                     rowcnt);
  if ((e = sf_launch_exclusive_scan_i32(rowcnt, (int)N, offs, offs + N, st)) != hipSuccess) return ws.fail("launch", e);
  hipLaunchKernelGGL(k_tarp_scatter, dim3((unsigned)blocks), dim3(256), 0, st, (long)cells, idx, offs, rowcnt, occ);
  if (norm_axis == 0)
    hipLaunchKernelGGL(k_tarp_minmax, dim3((unsigned)B), dim3(256), 0, st, theta, idx, (int)N, (int)D, lowinv);
  if ((e = hipGetLastError()) != hipSuccess) return ws.fail("launch", e);
  int TS = (SF_TARP_TILE_FLOATS / D) / 64 * 64;                  // draws per tile, whole groups of 64
  const int S64 = (int)((S + 63) / 64 * 64);
  TS = TS > S64 ? S64 : TS;
  const size_t lds = (size_t)D * (TS + 1) * sizeof(float);
  e = metric == 0 ? launch_count<0>(D, dim3((unsigned)N), lds, st, samples, theta, references, lowinv, norm_axis, (int)N, (int)S,
                                    TS, offs, occ, s_lo, s_hi ^ 4u, cnt)
                  : launch_count<1>(D, dim3((unsigned)N), lds, st, samples, theta, references, lowinv, norm_axis, (int)N, (int)S,
                                    TS, offs, occ, s_lo, s_hi ^ 4u, cnt);
  if (e != hipSuccess) return ws.fail("k_tarp_count", e);
  hipLaunchKernelGGL(k_tarp_curve, dim3((unsigned)B), dim3(256), ((size_t)S + 2) * sizeof(int), st, cnt, (int)N, (int)S,
                     (int)num_alpha_bins, (int)B, ecp, alpha);
  if ((e = hipGetLastError()) != hipSuccess) return ws.fail("k_tarp_curve", e);
  return ws.finish();
}
