// sf_post.hip -- posterior summaries on the device: per (galaxy, parameter)
// quantiles of the S draws with numpy's default 'linear' rule, NaN draws ignored (all-NaN -> NaN).
// Replaces the host pass  np.quantile(samples_i, [0.16, 0.5, 0.84], axis=1)
// (ref: src/synference/sbi_runner.py:3250-3282) without materialising (N,S,D) on the host.
#include <hip/hip_runtime.h>

#include <string>

#include "sf_internal.h"
#include "sf_rng.h"

// lower rank of the position (n - 1) q, clamped to [0, n - 1]; defined for every pos (negative, infinite, NaN -> 0 or n - 1)
__device__ __forceinline__ long sf_q_lo(double pos, int n) {
  if (!(pos > 0.0)) return 0;
  if (pos >= (double)(n - 1)) return n - 1;
  return (long)floor(pos);
}

// one 256-thread workgroup per (galaxy, dim); P = S padded to a power of two (<= 8192), bitonic sort in LDS.
// The rule (tests/post_model.py): n = the non-NaN draws, +-inf are ordered values; pos = (n - 1) q in fp64,
// lo = floor(pos), f = pos - lo; v[lo] where f == 0, else v[lo] + f (v[lo + 1] - v[lo]).  For q outside [0, 1] lo is clamped to
// [0, n - 1] and the end segment extrapolated: defined, not meaningful (the Python wrappers refuse such q, as numpy does).
__global__ __launch_bounds__(256) void k_quantiles(const float* __restrict__ samples, long S, int D, int P,
                                                   const float* __restrict__ q, int Q, float* __restrict__ out) {
  extern __shared__ float v[];
  const long g = blockIdx.x / D;
  const int d = blockIdx.x % D;
  const float* src = samples + g * S * D + d;
  const float INF = __builtin_inff();
  __shared__ int n_valid;
  if (threadIdx.x == 0) n_valid = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    float x = i < S ? src[(long)i * D] : INF;
    cnt += (i < S && x == x) ? 1 : 0;  // every non-NaN draw counts, +-inf included (as in k_quantiles_large)
    v[i] = (x == x) ? x : INF;         // NaN -> +inf: sorted to the end, behind (or among) the genuine +inf draws
  }
  atomicAdd(&n_valid, cnt);
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const float a = v[i], b = v[ixj];
          const bool up = (i & k) == 0;
          if ((a > b) == up) { v[i] = b; v[ixj] = a; }
        }
      }
    }
  }
  __syncthreads();
  const int n = n_valid;
  for (int t = threadIdx.x; t < Q; t += blockDim.x) {
    float r = __builtin_nanf("");
    if (n > 0) {
      // position and interpolation in fp64, as in k_quantiles_large: in fp32 the position error times the gap between
      // two modes is thousands of ulp at n = 8192; f == 0 returns the order statistic (no 0 * inf beside an infinite draw)
      const double pos = (double)(n - 1) * (double)q[t];
      const int lo = (int)sf_q_lo(pos, n);
      const int hi = lo + 1 < n ? lo + 1 : n - 1;
      const double vlo = (double)v[lo], vhi = (double)v[hi], f = pos - (double)lo;
      r = (float)(f > 0.0 ? vlo + f * (vhi - vlo) : vlo);
      if (pos != pos) r = __builtin_nanf("");  // a NaN q
    }
    out[(g * D + d) * Q + t] = r;
  }
}

extern "C" int sf_quantiles(const float* samples, int64_t N, int64_t S, int32_t D, const float* q_dev, int32_t Q,
                            float* out, void* stream) {
  if (N == 0) return SF_OK;
  if (!samples || !q_dev || !out) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  if (S < 1 || S > 8192 || D < 1 || Q < 1 || Q > 256) {
    sf_set_error("sf_quantiles: need 1 <= S <= 8192, D >= 1, 1 <= Q <= 256");
    return SF_ERR_INVALID;
  }
  if ((uint64_t)N * (uint64_t)D > 0x7fffffffull) { sf_set_error("N*D too large for one launch"); return SF_ERR_INVALID; }
  int P = 1;
  while (P < S) P <<= 1;
  hipLaunchKernelGGL(k_quantiles, dim3((unsigned)(N * D)), dim3(256), (size_t)P * sizeof(float), (hipStream_t)stream,
                     samples, (long)S, (int)D, P, q_dev, (int)Q, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { sf_set_error(std::string("k_quantiles: ") + hipGetErrorString(e)); return SF_ERR_HIP; }
  return SF_OK;
}

// ---------------------------------------------------------------------------------------------
// The same quantiles for long rows (1 <= S <= 2^24; the pooled nmc x nposterior = 1e5 draws of the missing-band path,
// ref: sbi_runner.py:3292-3297): no sort -- an exact radix select of the order statistics every quantile needs, on the
// order-preserving bit pattern of the draws, 8 bits per pass and up to 8 ranks per batch of passes (ranks that still share
// a prefix share a histogram, so the two ranks around one quantile cost one).  One 256-thread workgroup per (row, dim);
// the first pass reads the row from HBM, the later ones from L2.  The position (n - 1) q is formed in fp64 (in fp32 it
// has no fraction left at n = 1e5) and so is the interpolation.
// ---------------------------------------------------------------------------------------------
#define SF_QL_R 8
__device__ __forceinline__ uint32_t sf_ql_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sf_ql_val(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__global__ __launch_bounds__(256) void k_quantiles_large(const float* __restrict__ samples, long S, int D,
                                                         const float* __restrict__ q, int Q, float* __restrict__ out) {
  __shared__ int s_h0[256];                 // first pass: every finite-or-infinite draw, no prefix
  __shared__ int s_h[SF_QL_R][256];
  __shared__ uint32_t s_pre[SF_QL_R];       // prefix of rank r (the bits above the current digit)
  __shared__ int s_k[SF_QL_R];              // rank r among the draws that share its prefix
  __shared__ int s_slot[SF_QL_R], s_nd;     // histogram slot of rank r; distinct prefixes
  __shared__ uint32_t s_spre[SF_QL_R];
  const long g = blockIdx.x / D;
  const int d = blockIdx.x % D, tid = threadIdx.x;
  const float* src = samples + g * S * D + d;
  float* dst = out + (g * D + d) * Q;
  s_h0[tid] = 0;
  __syncthreads();
  for (long i = tid; i < S; i += 256) {
    const float x = src[i * D];
    if (x == x) atomicAdd(&s_h0[sf_ql_key(x) >> 24], 1);
  }
  __syncthreads();
  int n = 0;
  for (int b = 0; b < 256; ++b) n += s_h0[b];
  if (n == 0) {
    for (int t = tid; t < Q; t += 256) dst[t] = __builtin_nanf("");
    return;
  }
  const int nrank = 2 * Q;                  // rank 2t: floor((n - 1) q_t), rank 2t + 1: the next one
  for (int r0 = 0; r0 < nrank; r0 += SF_QL_R) {
    const int nr = nrank - r0 < SF_QL_R ? nrank - r0 : SF_QL_R;
    __syncthreads();
    if (tid < nr) {
      const int t = (r0 + tid) >> 1;
      const double pos = (double)(n - 1) * (double)q[t];
      const long lo = sf_q_lo(pos, n);
      const long hi = lo + 1 < n ? lo + 1 : n - 1;
      int k = (int)(((r0 + tid) & 1) ? hi : lo), b = 0;
      while (b < 255 && k >= s_h0[b]) { k -= s_h0[b]; ++b; }
      s_k[tid] = k;
      s_pre[tid] = (uint32_t)b;
    }
    for (int p = 1; p < 4; ++p) {
      const int shift = 24 - 8 * p;
      __syncthreads();
      if (tid == 0) {                       // ranks with the same prefix share a histogram
        int nd = 0;
        for (int r = 0; r < nr; ++r) {
          int s = 0;
          while (s < nd && s_spre[s] != s_pre[r]) ++s;
          if (s == nd) s_spre[nd++] = s_pre[r];
          s_slot[r] = s;
        }
        s_nd = nd;
      }
      for (int e = tid; e < SF_QL_R * 256; e += 256) (&s_h[0][0])[e] = 0;
      __syncthreads();
      const int nd = s_nd;
      for (long i = tid; i < S; i += 256) {
        const float x = src[i * D];
        if (x == x) {
          const uint32_t key = sf_ql_key(x), top = key >> (shift + 8);
          for (int s = 0; s < nd; ++s)
            if (top == s_spre[s]) atomicAdd(&s_h[s][(key >> shift) & 255u], 1);
        }
      }
      __syncthreads();
      if (tid < nr) {
        const int* h = s_h[s_slot[tid]];
        int k = s_k[tid], b = 0;
        while (b < 255 && k >= h[b]) { k -= h[b]; ++b; }
        s_k[tid] = k;
        s_pre[tid] = (s_pre[tid] << 8) | (uint32_t)b;
      }
    }
    __syncthreads();
    if (tid < nr && !(tid & 1)) {           // (nr is even: the two ranks of a quantile are in one batch)
      const int t = (r0 + tid) >> 1;
      const double pos = (double)(n - 1) * (double)q[t];
      const long lo = sf_q_lo(pos, n);
      const double vlo = (double)sf_ql_val(s_pre[tid]), vhi = (double)sf_ql_val(s_pre[tid + 1]);
      const double f = pos - (double)lo;
      dst[t] = pos != pos ? __builtin_nanf("") : (float)(f > 0.0 ? vlo + f * (vhi - vlo) : vlo);  // (a NaN q -> NaN)
    }
  }
}

extern "C" int sf_quantiles_large(const float* samples, int64_t N, int64_t S, int32_t D, const float* q_dev, int32_t Q,
                                  float* out, void* stream) {
  if (S < 1 || S > (1ll << 24) || D < 1 || Q < 1 || Q > 256 || N < 0) {
    sf_set_error("sf_quantiles_large: need 1 <= S <= 2^24, D >= 1, 1 <= Q <= 256, N >= 0");
    return SF_ERR_INVALID;
  }
  if (N == 0) return SF_OK;  // (an empty catalogue's buffers may be null, as for sf_quantiles)
  if (!samples || !q_dev || !out) { sf_set_error("sf_quantiles_large: null argument"); return SF_ERR_INVALID; }
  if ((uint64_t)N * (uint64_t)D > 0x7fffffffull) { sf_set_error("sf_quantiles_large: N*D too large for one launch"); return SF_ERR_INVALID; }
  hipLaunchKernelGGL(k_quantiles_large, dim3((unsigned)(N * D)), dim3(256), 0, (hipStream_t)stream, samples, (long)S, (int)D,
                     q_dev, (int)Q, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { sf_set_error(std::string("k_quantiles_large: ") + hipGetErrorString(e)); return SF_ERR_HIP; }
  return SF_OK;
}

// ---------------------------------------------------------------------------------------------
// Feature transform on the device: fluxes in nJy -> AB magnitudes,
//   mag = -2.5 log10(f / 1000) + 23.9 ; f < 0 -> mag_limit ; mag > mag_limit (incl. f == 0 -> +inf) -> mag_limit ;
//   a NaN flux stays NaN (the reference only replaces negative fluxes, sbi_runner.py:1706-1714, so that rows with a
//   missing band are still recognised and masked downstream)
// and, optionally, flux errors -> magnitude errors  2.5 sigma / (ln 10 f).
// Replaces the host numpy pass at ref: src/synference/sbi_runner.py:1698-1716, 1927-1932.  HBM-bound, float4 I/O.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sf_abmag(float f_njy, float lim) {
  if (f_njy != f_njy) return f_njy;  // missing band: NaN propagates
  float m = -2.5f * log10f(f_njy * 1.0e-3f) + 23.9f;
  if (f_njy < 0.f || m > lim) m = lim;  // negative flux and the faint limit (f == 0 gives +inf > lim)
  return m;
}
__global__ void k_flux_to_abmag(const float* __restrict__ flux, const float* __restrict__ err, long n, float lim,
                                float* __restrict__ mag, float* __restrict__ mag_err) {
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float4 f = *reinterpret_cast<const float4*>(flux + i);
      *reinterpret_cast<float4*>(mag + i) = make_float4(sf_abmag(f.x, lim), sf_abmag(f.y, lim), sf_abmag(f.z, lim), sf_abmag(f.w, lim));
      if (err) {
        const float4 e = *reinterpret_cast<const float4*>(err + i);
        const float c = 1.0857362047581294f;  // 2.5 / ln 10
        *reinterpret_cast<float4*>(mag_err + i) = make_float4(c * e.x / f.x, c * e.y / f.y, c * e.z / f.z, c * e.w / f.w);
      }
    } else {
      for (long j = i; j < n; ++j) {
        mag[j] = sf_abmag(flux[j], lim);
        if (err) mag_err[j] = 1.0857362047581294f * err[j] / flux[j];
      }
    }
  }
}

extern "C" int sf_flux_to_abmag(const float* flux_njy, const float* err_njy, int64_t n, float mag_limit, float* mag,
                                float* mag_err, void* stream) {
  if (n == 0) return SF_OK;
  if (!flux_njy || !mag || (err_njy && !mag_err)) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  if ((((uintptr_t)flux_njy | (uintptr_t)mag | (uintptr_t)err_njy | (uintptr_t)mag_err) & 15) != 0) {
    sf_set_error("sf_flux_to_abmag: buffers must be 16-byte aligned");
    return SF_ERR_INVALID;
  }
  long blocks = (n / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(k_flux_to_abmag, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flux_njy, err_njy, (long)n,
                     mag_limit, mag, mag_err);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { sf_set_error(std::string("k_flux_to_abmag: ") + hipGetErrorString(e)); return SF_ERR_HIP; }
  return SF_OK;
}

// ---------------------------------------------------------------------------------------------
// asinh ("luptitude") magnitudes, per-band softening f_b (ref: src/synference/utils.py:647-704, used at
// sbi_runner.py:1718-1731):
//   mag = -2.5 log10(e) * ( asinh(f / (2 f_b)) + ln(f_b / 3631 Jy) ),  err = 2.5 log10(e) * sigma / sqrt(f^2 + (2 f_b)^2)
// flux, err [N,C] row-major in nJy; f_b [C] in nJy (device).  HBM-bound elementwise pass.
// ---------------------------------------------------------------------------------------------
__global__ void k_flux_to_asinh(const float* __restrict__ flux, const float* __restrict__ err, long n, int C,
                                const float* __restrict__ f_b, float* __restrict__ mag, float* __restrict__ mag_err) {
  const float k = 1.0857362047581294f;  // 2.5 log10(e)
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float b = f_b[i % C], f = flux[i];
    const float r = f / (2.f * b);
    mag[i] = -k * (asinhf(r) + logf(b * (1.0e-9f / 3631.f)));
    if (err) mag_err[i] = k * err[i] / sqrtf(f * f + 4.f * b * b);
  }
}

extern "C" int sf_flux_to_asinh(const float* flux_njy, const float* err_njy, int64_t N, int32_t C, const float* f_b_njy,
                                float* mag, float* mag_err, void* stream) {
  if (N == 0) return SF_OK;
  if (!flux_njy || !mag || !f_b_njy || (err_njy && !mag_err)) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  if (N < 0 || C < 1) { sf_set_error("sf_flux_to_asinh: bad shape"); return SF_ERR_INVALID; }
  const long n = (long)N * C;
  long blocks = (n + 255) / 256;
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(k_flux_to_asinh, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flux_njy, err_njy, n, (int)C,
                     f_b_njy, mag, mag_err);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { sf_set_error(std::string("k_flux_to_asinh: ") + hipGetErrorString(e)); return SF_ERR_HIP; }
  return SF_OK;
}

// ---------------------------------------------------------------------------------------------
// Depth-noise scatter (ref: sbi_runner.py:580-691 `_apply_depths`, 1-D depths): every library row is repeated
// n_scatters times and perturbed by N(0, sigma_c), sigma_c = max(depth_c / depth_sigma, |flux| * min_pc / 100);
// the sigma used is returned as the error column.  out row = row * n_scatters + s.  Noise: Philox stream
// (seed, stream 2; counter = (out_row, band block)), so a catalogue is reproducible and independent of launch shape
// (the reference draws from numpy's global generator).
// ---------------------------------------------------------------------------------------------
__global__ void k_scatter_depths(const float* __restrict__ flux, long N, int C, const float* __restrict__ sigma, int n_sig,
                                 int n_scatters, float min_pc, uint32_t k0, uint32_t k1, float* __restrict__ out,
                                 float* __restrict__ err_out) {
  const int CB = (C + 3) / 4;
  const long total = N * n_scatters * CB;
  const long stride = (long)gridDim.x * blockDim.x;
  const double pc = (double)min_pc * 0.01;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long orow = i / CB;
    const int cb = (int)(i % CB);
    const long row = orow / n_scatters;
    const float* sg = sigma + (size_t)((orow % n_scatters) % n_sig) * C;  // one sigma row, or one per scatter copy
    float z[4];
    sf_normal4(k0, k1, (uint64_t)orow, 0u, (uint32_t)cb, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cb * 4 + j;
      if (c < C) {
        const float f = flux[row * C + c];
        // |f| min_pc / 100 in fp64, rounded once (two fp32 products and the rounded 0.01f were up to 1.5 ulp off the formula)
        const float s = fmaxf(sg[c], (float)((double)fabsf(f) * pc));
        out[orow * C + c] = f + s * z[j];
        if (err_out) err_out[orow * C + c] = s;
      }
    }
  }
}

extern "C" int sf_scatter_depths(const float* flux, int64_t N, int32_t C, const float* sigma, int32_t n_sigma_rows,
                                 int32_t n_scatters, float min_flux_pc_error, uint64_t seed, float* out, float* err_out,
                                 void* stream) {
  if (N == 0) return SF_OK;
  if (!flux || !sigma || !out) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  if (N < 0 || C < 1 || n_scatters < 1 || (n_sigma_rows != 1 && n_sigma_rows != n_scatters)) {
    sf_set_error("sf_scatter_depths: bad shape (sigma rows must be 1 or n_scatters)");
    return SF_ERR_INVALID;
  }
  const long total = (long)N * n_scatters * ((C + 3) / 4);
  long blocks = (total + 255) / 256;
  blocks = blocks > 8192 ? 8192 : blocks;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ 2u;
  hipLaunchKernelGGL(k_scatter_depths, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flux, (long)N, (int)C, sigma,
                     (int)n_sigma_rows, (int)n_scatters, min_flux_pc_error, k0, k1, out, err_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { sf_set_error(std::string("k_scatter_depths: ") + hipGetErrorString(e)); return SF_ERR_HIP; }
  return SF_OK;
}

// ---------------------------------------------------------------------------------------------
// PIT ranks (ref: sbi_runner.py:7153-7158): rank[g,d] = #{ s : draw[g,s,d] < truth[g,d] } / #{non-NaN draws}
// one wave per (galaxy, dim); NaN draws ignored (all-NaN -> NaN); +-inf draws are ordered values and count in both the
// numerator and the denominator; a NaN truth is below nothing and gives 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pit_ranks(const float* __restrict__ samples, const float* __restrict__ truth, long N,
                                                   long S, int D, float* __restrict__ out) {
  const long w = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= N * D) return;
  const long g = w / D;
  const int d = (int)(w % D);
  const float t = truth[g * D + d];
  int below = 0, valid = 0;
  for (long s = lane; s < S; s += 64) {
    const float v = samples[(g * S + s) * D + d];
    valid += (v == v) ? 1 : 0;
    below += (v < t) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    below += __shfl_xor(below, o, 64);
    valid += __shfl_xor(valid, o, 64);
  }
  if (lane == 0) out[w] = valid > 0 ? (float)below / (float)valid : __builtin_nanf("");
}

extern "C" int sf_pit_ranks(const float* samples, const float* truth, int64_t N, int64_t S, int32_t D, float* out,
                            void* stream) {
  if (N == 0) return SF_OK;
  if (!samples || !truth || !out) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  if (N < 0 || S < 1 || D < 1) { sf_set_error("sf_pit_ranks: bad shape"); return SF_ERR_INVALID; }
  const long waves = (long)N * D;
  hipLaunchKernelGGL(k_pit_ranks, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, samples, truth, (long)N,
                     (long)S, (int)D, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { sf_set_error(std::string("k_pit_ranks: ") + hipGetErrorString(e)); return SF_ERR_HIP; }
  return SF_OK;
}
