// sf_latent.hip -- one streaming reduction over the latents z[N, D] of a flow (sf_flow_to_noise): everything the latent
// residual diagnostics need from one pass over HBM.  For a calibrated posterior the latents of the true parameters are
// N(0, I) exactly, so per dimension u = Phi(z_d) is uniform, and so is u_r = F_chi2_D(|z|^2) -- the expected coverage of the
// joint posterior, read in the base space ([UPSTREAM] nflows Flow.transform_to_noise; the reference keeps the name
// plot_latent_residual for it, sbi_runner.py:7200, without a body).
//
//   k_latent_partial  workgroup g takes the tiles g, g + G, ... of 256 rows: a tile is staged in LDS (row stride D | 1 words,
//                     so the row-per-lane reads spread over the banks); lane r owns row r -- finite test (a row with a NaN or
//                     an infinity is counted in n_bad and zeroed in LDS: it then adds nothing to any sum), the D normal CDFs and
//                     the chi-square CDF in fp64, one integer LDS atomic per histogram cell; then thread (i, j) adds the tile's
//                     z_i z_j and thread (power, d) its z_d^power, both in fp64 registers kept over the workgroup's tiles.
//                     At the end every workgroup writes its partials with plain stores.
//   k_latent_reduce   one thread per output cell adds the G partials in the order g = 0 .. G - 1.
// G depends on N alone, integer counts add exactly, and no float atomic is used: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <string>

#include "sf_block.h"
#include "sf_internal.h"
#include "sf_scratch.h"

#define SF_LAT_DMAX 16
#define SF_LAT_NBMAX 1024
#define SF_LAT_ROWS 256   // rows per tile = threads per workgroup
#define SF_LAT_GMAX 256   // workgroups (partials) at the most

// 1 / Gamma(k + 3/2), k = 0 .. 6 (odd D <= 15 needs k < 7)
__constant__ double c_lat_inv_gamma_half[7] = {
    1.1283791670955126,     // 1 / Gamma(3/2)  = 2 / sqrt(pi)
    0.75225277806367508,    // 1 / Gamma(5/2)
    0.30090111122547003,    // 1 / Gamma(7/2)
    0.085971746064420009,   // 1 / Gamma(9/2)
    0.019104832458760002,   // 1 / Gamma(11/2)
    0.0034736059015927277,  // 1 / Gamma(13/2)
    0.00053440090793734272, // 1 / Gamma(15/2)
};

// F_chi2_D(r2), closed forms with y = r2 / 2:
//   D = 2m     : 1 - e^-y sum_{k<m} y^k / k!
//   D = 2m + 1 : erf(sqrt y) - e^-y sum_{k<m} y^(k+1/2) / Gamma(k + 3/2)
// Past y = 700 the subtracted term is below 2^-1074 for every D <= 16 (and y^k would overflow for the largest finite rows).
__device__ __forceinline__ double sf_chi2_cdf(double r2, int D) {
  const double y = 0.5 * r2;
  if (y > 700.0) return 1.0;
  const int m = D >> 1;
  const double ey = exp(-y);
  double s = 0.0, u;
  if ((D & 1) == 0) {
    double term = 1.0;   // y^k / k!
    for (int k = 0; k < m; ++k) {
      s += term;
      term *= y / (double)(k + 1);
    }
    u = 1.0 - ey * s;
  } else {
    const double sq = sqrt(y);
    double yk = sq;      // y^(k + 1/2)
    for (int k = 0; k < m; ++k) {
      s += yk * c_lat_inv_gamma_half[k];
      yk *= y;
    }
    u = erf(sq) - ey * s;
  }
  return fmin(fmax(u, 0.0), 1.0);   // (the difference may leave [0, 1] by a rounding)
}

__device__ __forceinline__ int sf_lat_bin(double u, int nb) {
  const int b = (int)floor(u * (double)nb);
  return b < nb - 1 ? b : nb - 1;
}

// pd[g][D*D + 4*D]: cross, then psum; pn[g][2]: n, n_bad; ph[g][(D + 1) * nb]: pit_counts, then radial_counts
__global__ __launch_bounds__(SF_LAT_ROWS) void k_latent_partial(const float* __restrict__ z, long N, int D, int nb, int want_pit,
                                                                int want_rad, double* __restrict__ pd, long long* __restrict__ pn,
                                                                int* __restrict__ ph) {
  extern __shared__ float s_lat[];
  __shared__ long long s_red[SF_LAT_ROWS];
  const int DP = D | 1;
  float* tile = s_lat;                                             // [256][DP]
  int* hist = reinterpret_cast<int*>(s_lat + SF_LAT_ROWS * DP);    // [(D + 1) * nb]
  const int tid = threadIdx.x;
  const int n_hist = (D + 1) * nb;
  for (int k = tid; k < n_hist; k += SF_LAT_ROWS) hist[k] = 0;
  const int ci = tid / D, cj = tid - ci * D;   // cross: (i, j) for tid < D * D;  psum: (power - 1, d) for tid < 4 * D
  double acc_cross = 0.0, acc_ps = 0.0;
  long long n_ok = 0, n_bad = 0;
  const long n_tiles = (N + SF_LAT_ROWS - 1) / SF_LAT_ROWS;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long r0 = t * SF_LAT_ROWS;
    const int rows = N - r0 < SF_LAT_ROWS ? (int)(N - r0) : SF_LAT_ROWS;
    __syncthreads();   // every thread has finished with the previous tile (and the histogram is cleared)
    const float* src = z + (size_t)r0 * D;
    for (int e = tid; e < SF_LAT_ROWS * D; e += SF_LAT_ROWS) {
      const int r = e / D, d = e - r * D;
      tile[r * DP + d] = r < rows ? src[e] : 0.f;
    }
    __syncthreads();
    if (tid < rows) {
      float v[SF_LAT_DMAX];
      bool ok = true;
#pragma unroll
      for (int d = 0; d < SF_LAT_DMAX; ++d) {
        v[d] = d < D ? tile[tid * DP + d] : 0.f;
        ok = ok && fabsf(v[d]) < __builtin_inff();   // (NaN compares false)
      }
      if (ok) {
        ++n_ok;
        double r2 = 0.0;
#pragma unroll
        for (int d = 0; d < SF_LAT_DMAX; ++d)
          if (d < D) {
            const double zd = (double)v[d];
            r2 += zd * zd;
            if (want_pit) atomicAdd(&hist[d * nb + sf_lat_bin(0.5 * erfc(-zd / 1.4142135623730951), nb)], 1);
          }
        if (want_rad) atomicAdd(&hist[D * nb + sf_lat_bin(sf_chi2_cdf(r2, D), nb)], 1);
      } else {
        ++n_bad;
        for (int d = 0; d < D; ++d) tile[tid * DP + d] = 0.f;
      }
    }
    __syncthreads();
    if (tid < D * D) {
      for (int r = 0; r < SF_LAT_ROWS; ++r) acc_cross += (double)tile[r * DP + ci] * (double)tile[r * DP + cj];
    }
    if (tid < 4 * D) {
      for (int r = 0; r < SF_LAT_ROWS; ++r) {
        const double a = (double)tile[r * DP + cj], a2 = a * a;
        acc_ps += ci == 0 ? a : (ci == 1 ? a2 : (ci == 2 ? a2 * a : a2 * a2));
      }
    }
  }
  const long long tot_ok = sf_block_sum<long long>(n_ok, s_red);
  const long long tot_bad = sf_block_sum<long long>(n_bad, s_red);   // (its first barrier also closes the histogram)
  const size_t g = blockIdx.x;
  double* pdg = pd + g * (size_t)(D * D + 4 * D);
  if (tid < D * D) pdg[tid] = acc_cross;
  if (tid < 4 * D) pdg[D * D + tid] = acc_ps;
  if (tid == 0) { pn[g * 2] = tot_ok; pn[g * 2 + 1] = tot_bad; }
  for (int k = tid; k < n_hist; k += SF_LAT_ROWS) ph[g * (size_t)n_hist + k] = hist[k];
}

// cell c of [cross D*D | psum 4*D | counts (D + 1)*nb | n, n_bad]: the sum of the G partials in order
__global__ __launch_bounds__(256) void k_latent_reduce(int G, int D, int nb, const double* __restrict__ pd, const long long* __restrict__ pn,
                                                       const int* __restrict__ ph, long long* __restrict__ n2, double* __restrict__ psum,
                                                       double* __restrict__ cross, long long* __restrict__ pit, long long* __restrict__ rad) {
  const int nd = D * D + 4 * D, n_hist = (D + 1) * nb;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nd) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += pd[(size_t)g * nd + c];
    if (c < D * D) { if (cross) cross[c] = s; }
    else if (psum) psum[c - D * D] = s;
  } else if (c < nd + n_hist) {
    const int k = c - nd;
    long long s = 0;
    for (int g = 0; g < G; ++g) s += ph[(size_t)g * n_hist + k];
    if (k < D * nb) { if (pit) pit[k] = s; }
    else if (rad) rad[k - D * nb] = s;
  } else if (c < nd + n_hist + 2) {
    const int k = c - nd - n_hist;
    long long s = 0;
    for (int g = 0; g < G; ++g) s += pn[(size_t)g * 2 + k];
    if (n2) n2[k] = s;
  }
}

namespace {
SfScratch g_latent_scratch;
SfAttrCache g_latent_attr;
}  // namespace

extern "C" int sf_latent_summary(const float* z, int64_t N, int32_t D, int32_t nb, int64_t* n2, double* psum, double* cross,
                                 int64_t* pit_counts, int64_t* radial_counts, void* stream) {
  if (D < 1 || D > SF_LAT_DMAX || nb < 1 || nb > SF_LAT_NBMAX || N < 0) {
    sf_set_error("sf_latent_summary: need 1 <= D <= 16, 1 <= nb <= 1024, N >= 0");
    return SF_ERR_INVALID;
  }
  if (N > 0 && !z) { sf_set_error("sf_latent_summary: null argument"); return SF_ERR_INVALID; }
  static_assert(sizeof(long long) == sizeof(int64_t), "int64 outputs are written as long long");
  hipStream_t st = (hipStream_t)stream;
  const long n_tiles = (long)((N + SF_LAT_ROWS - 1) / SF_LAT_ROWS);
  const int G = (int)(n_tiles < SF_LAT_GMAX ? n_tiles : SF_LAT_GMAX);
  const int nd = D * D + 4 * D, n_hist = (D + 1) * nb;
  SfScratchCall ws(g_latent_scratch, "sf_latent_summary", st);
  const int sub_pd = ws.add((size_t)(G ? G : 1) * nd * sizeof(double)), sub_pn = ws.add((size_t)(G ? G : 1) * 2 * sizeof(long long));
  const int sub_ph = ws.add((size_t)(G ? G : 1) * n_hist * sizeof(int));
  if (int rc = ws.reserve()) return rc;
  double* pd = ws.get<double>(sub_pd);
  long long* pn = ws.get<long long>(sub_pn);
  int* ph = ws.get<int>(sub_ph);
  if (int rc = ws.check()) return rc;
  hipError_t e;
  if (G > 0) {
    const size_t lds = ((size_t)SF_LAT_ROWS * (D | 1) + n_hist) * sizeof(float);   // <= 17 KB + 68 KB
    int dev;
    if (lds > 48 * 1024 && g_latent_attr.need(dev)) {
      e = hipFuncSetAttribute((const void*)k_latent_partial, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
      if (e != hipSuccess) return ws.fail("hipFuncSetAttribute", e);
      g_latent_attr.set(dev);
    }
    hipLaunchKernelGGL(k_latent_partial, dim3((unsigned)G), dim3(SF_LAT_ROWS), lds, st, z, (long)N, (int)D, (int)nb,
                       pit_counts ? 1 : 0, radial_counts ? 1 : 0, pd, pn, ph);
    if ((e = hipGetLastError()) != hipSuccess) return ws.fail("k_latent_partial", e);
  }
  const int cells = nd + n_hist + 2;
  hipLaunchKernelGGL(k_latent_reduce, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, G, (int)D, (int)nb, pd, pn, ph,
                     reinterpret_cast<long long*>(n2), psum, cross, reinterpret_cast<long long*>(pit_counts),
                     reinterpret_cast<long long*>(radial_counts));
  if ((e = hipGetLastError()) != hipSuccess) return ws.fail("k_latent_reduce", e);
  return ws.finish();
}
