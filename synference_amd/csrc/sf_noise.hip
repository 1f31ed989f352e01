// sf_noise.hip -- empirical noise models on the device: p(sigma | flux) per filter, learned from an observed catalogue on the
// host (synference_amd/noise_models.py), applied to every library row here.
//   sf_scatter_empirical  ref: src/synference/noise_models.py:818-880 (General apply_noise), 507-560 (Asinh apply_noise),
//                         383-390 (sample_uncertainty), 882-957 (SNR mask, flux and error rules), 959-987 (units out)
//   sf_apply_scalings     ref: noise_models.py:1074-1099 (General), 562-592 (Asinh): the deterministic twin
// One thread per (output row, group of 4 bands); the band structs and their tables are staged once per workgroup in LDS; one
// Philox4x32-10 call per output element: key (seed, stream 6), counter (out_row lo, out_row hi, 0, band), the four words
// through sf_u01 are u0..u3 -- a catalogue is reproducible and independent of the launch shape.
// Everything that is constant per band (unit factors, the limit, the replacement error ...) is computed on the host and
// arrives in sf_noise_band (include/synference_hip.h).  Every loop bound is independent of the data.
#include <hip/hip_runtime.h>

#include <string>

#include "sf_internal.h"
#include "sf_rng.h"
#include "sf_scratch.h"

#define SF_NOISE_MAX_BINS 256
#define SF_NOISE_MAX_TABLE_BYTES 65536
#define SF_NOISE_SEARCH_STEPS 8   // 2^8 >= SF_NOISE_MAX_BINS: the bisection ends after this many halvings whatever x is

namespace {

constexpr float kLn10Over2p5 = 0.92103403719761836f;   // ln 10 / 2.5
constexpr float k2p5OverLn10 = 1.0857362047581294f;    // 2.5 / ln 10 = 2.5 log10(e)
constexpr float kInvSqrt2 = 0.70710678118654752f;

__device__ __forceinline__ float sf_nan() { return __builtin_nanf(""); }

// linear interpolation of the median and the std table at x: outside the centres the end values, or -- extrapolate -- the end
// segments continued; NaN in, NaN out (every comparison with NaN is false: the search walks to the first segment and ends)
__device__ __forceinline__ void noise_interp(const sf_noise_band& b, const float* __restrict__ tab, float x, float& mu,
                                             float& ss) {
  const int n = b.n_bins;
  const float* c = tab + b.table_offset;
  const float* md = c + n;
  const float* sd = md + n;
  int lo = 0, hi = n - 1;
#pragma unroll 1
  for (int it = 0; it < SF_NOISE_SEARCH_STEPS; ++it) {
    if (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (c[mid] <= x) lo = mid; else hi = mid;
    }
  }
  const float xc = b.extrapolate ? x : fminf(fmaxf(x, c[0]), c[n - 1]);
  const float t = (xc - c[lo]) / (c[lo + 1] - c[lo]);
  mu = md[lo] + t * (md[lo + 1] - md[lo]);
  const float sv = sd[lo] + t * (sd[lo + 1] - sd[lo]);
  ss = (sv != sv) ? sv : fmaxf(0.f, sv);
  if (x != x) mu = ss = sf_nan();
}

// quantile u of a standard normal truncated to [a, inf): from the tail mass q = Q(a) (1 - u), which keeps its relative
// precision in fp32 where P(a) + u Q(a) rounds to 1
__device__ __forceinline__ float noise_lower_trunc_quantile(float a, float u) {
  const float Qa = 0.5f * erfcf(a * kInvSqrt2);
  const float q = fmaxf(Qa * (1.f - u), 1.17549435e-38f);
  if (q <= 0.5f) return -normcdfinvf(q);
  const float Pa = 0.5f * erfcf(-a * kInvSqrt2);
  return normcdfinvf(Pa + u * Qa);
}

// quantile u of a standard normal truncated to [-c, c], evaluated in the lower half and mirrored
__device__ __forceinline__ float noise_clip_quantile(float c, float u) {
  const float Pl = 0.5f * erfcf(c * kInvSqrt2);
  const bool up = u > 0.5f;
  const float v = up ? 1.f - u : u;
  const float z = normcdfinvf(Pl + v * (1.f - 2.f * Pl));
  return up ? -z : z;
}

// ref 383-390: sigma ~ N(mu(x), ss(x)) truncated to sigma >= 0
__device__ __forceinline__ float noise_sample_sigma(const sf_noise_band& b, const float* __restrict__ tab, float x, float u) {
  float mu, ss;
  noise_interp(b, tab, x, mu, ss);
  const float a = fminf(-mu / (ss > 1e-9f ? ss : 1.f), 12.f);
  return mu + ss * noise_lower_trunc_quantile(a, u);
}

// ref 882-894: below the SNR threshold, or no finite SNR (x, e in the band's interpolation space)
__device__ __forceinline__ bool noise_snr_below(const sf_noise_band& b, float x, float e) {
  float snr;
  if (b.interp_space == SF_NOISE_SPACE_AB) {
    const float fj = exp10f(-0.4f * (x - 8.9f));
    snr = (fj / fj) * (k2p5OverLn10 / e);
  } else {
    snr = x / e;
  }
  return !(fabsf(snr) < __builtin_inff()) || snr < b.snr_threshold;
}

__device__ __forceinline__ float noise_clip_err(const sf_noise_band& b, float s) {
  return (s != s) ? s : fminf(fmaxf(s, b.min_err), b.max_err);
}

__device__ __forceinline__ float noise_asinh_mag(float f_jy, float b_jy) {
  return -k2p5OverLn10 * (asinhf(f_jy / (2.f * b_jy)) + logf(b_jy * (1.f / 3631.f)));
}

__device__ __forceinline__ float noise_input_jy(const sf_noise_band& b, float f) {
  return b.in_space == SF_NOISE_SPACE_AB ? exp10f(-0.4f * (f - 8.9f)) : f * b.in_to_jy;
}

// ref 959-987: (y, s) from the interpolation space of a General model to the output space
__device__ __forceinline__ void noise_general_out(const sf_noise_band& b, float& y, float& s) {
  if (b.interp_space == SF_NOISE_SPACE_AB) {
    if (b.out_space != SF_NOISE_SPACE_AB) {
      const float fo = exp10f(-0.4f * (y - b.zp_out));
      s = fo * s * kLn10Over2p5;
      y = fo;
    }
  } else if (b.out_space == SF_NOISE_SPACE_AB) {
    s = fabsf(k2p5OverLn10 * (s / y));
    y = b.zp_unit - 2.5f * log10f(y);
  } else {
    y *= b.unit_to_out;
    s *= b.unit_to_out;
  }
  s = noise_clip_err(b, s);
}

__device__ __forceinline__ void noise_general_scatter(const sf_noise_band& b, const float* __restrict__ tab, float f,
                                                      const float (&u)[4], float& oy, float& os) {
  float x;
  if (b.interp_space == SF_NOISE_SPACE_AB) x = b.in_space == SF_NOISE_SPACE_AB ? f : b.zp_in - 2.5f * log10f(f);
  else x = b.in_space == SF_NOISE_SPACE_AB ? exp10f(-0.4f * (f - b.zp_unit)) : f * b.in_to_unit;
  const float s1 = noise_sample_sigma(b, tab, x, u[0]);
  const bool lim0 = b.upper_limits && noise_snr_below(b, x, s1);
  float y = x;
  if (!lim0) y += s1 * (b.sigma_clip >= 0.f ? noise_clip_quantile(b.sigma_clip, u[1]) : normcdfinvf(u[1]));
  float s = b.resample ? noise_sample_sigma(b, tab, y, u[2]) : s1;
  if (b.upper_limits && b.has_limit && (lim0 || noise_snr_below(b, y, s))) {
    if (b.flux_rule == SF_NOISE_FLUX_SCATTER) y = b.limit_value + b.std_at_limit * noise_clip_quantile(3.f, u[3]);
    else if (b.flux_rule == SF_NOISE_FLUX_LIMIT) y = b.limit_value;
    else y = b.flux_number;
    if (b.replace_err) s = b.err_value;
  }
  noise_general_out(b, y, s);
  oy = y;
  os = s;
}

// ref 507-560, in the reference's own order
__device__ __forceinline__ void noise_asinh_scatter(const sf_noise_band& b, const float* __restrict__ tab, float f,
                                                    const float (&u)[4], float& oy, float& os) {
  const float fj = noise_input_jy(b, f);
  const float z = normcdfinvf(u[1]);
  float y, s;
  if (b.interp_space == SF_NOISE_SPACE_ASINH) {
    const float m = noise_asinh_mag(fj, b.b_jy);
    const float s1 = noise_sample_sigma(b, tab, m, u[0]);
    y = m + s1 * z;
    s = b.resample ? noise_sample_sigma(b, tab, y, u[2]) : s1;
  } else {
    const float s1 = noise_sample_sigma(b, tab, fj * b.unit_per_jy, u[0]);
    const float yj = fj + (s1 * b.jy_per_unit) * z;
    y = noise_asinh_mag(yj, b.b_jy);
    const float e = b.resample ? noise_sample_sigma(b, tab, yj * b.unit_per_jy, u[2]) : s1;
    s = k2p5OverLn10 * (e * b.jy_per_unit) / sqrtf(yj * yj + 4.f * b.b_jy * b.b_jy);
  }
  oy = y;
  os = noise_clip_err(b, s);
}

// ref 1074-1099 (General) and 562-592 (Asinh): units, SNR cut with the flux rule unscattered, replacement error, units, clip
__device__ __forceinline__ void noise_scalings(const sf_noise_band& b, float f, float e, float& oy, float& os) {
  if (b.kind == SF_NOISE_KIND_ASINH) {
    const float fj = noise_input_jy(b, f);
    const float ej = b.in_space == SF_NOISE_SPACE_AB ? fj * e * kLn10Over2p5 : e * b.in_to_jy;
    oy = noise_asinh_mag(fj, b.b_jy);
    os = noise_clip_err(b, k2p5OverLn10 * ej / sqrtf(fj * fj + 4.f * b.b_jy * b.b_jy));
    return;
  }
  float x, s;
  if (b.interp_space == SF_NOISE_SPACE_AB) {
    if (b.in_space == SF_NOISE_SPACE_AB) { x = f; s = e; }
    else { x = b.zp_in - 2.5f * log10f(f); s = fabsf(k2p5OverLn10 * (e / f)); }
  } else if (b.in_space == SF_NOISE_SPACE_AB) {
    x = exp10f(-0.4f * (f - b.zp_unit));
    s = x * e * kLn10Over2p5;
  } else {
    x = f * b.in_to_unit;
    s = e * b.in_to_unit;
  }
  if (b.upper_limits && b.has_limit && noise_snr_below(b, x, s)) {
    x = b.flux_rule == SF_NOISE_FLUX_NUMBER ? b.flux_number : b.limit_value;
    if (b.replace_err) s = b.err_value;
  }
  noise_general_out(b, x, s);
  oy = x;
  os = s;
}

// blob = [C band structs][n_table floats], words of 4 bytes; SCATTER: err unused, Philox noise; else the deterministic twin
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_noise(const float* __restrict__ flux, const float* __restrict__ err, long N, int C,
                                               const uint32_t* __restrict__ blob, int blob_words, int n_scatters, int vec4,
                                               uint32_t k0, uint32_t k1, float* __restrict__ out,
                                               float* __restrict__ err_out) {
  extern __shared__ uint32_t noise_lds[];
  for (int i = threadIdx.x; i < blob_words; i += blockDim.x) noise_lds[i] = blob[i];
  __syncthreads();
  const sf_noise_band* bands = reinterpret_cast<const sf_noise_band*>(noise_lds);
  const float* tab = reinterpret_cast<const float*>(bands + C);
  const int CB = (C + 3) / 4;
  const long total = N * n_scatters * CB;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long orow = i / CB;
    const int cb = (int)(i % CB);
    const long row = orow / n_scatters;
    float oy[4] = {0.f, 0.f, 0.f, 0.f}, os[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cb * 4 + j;
      if (c < C) {
        const sf_noise_band& b = bands[c];
        const float f = flux[row * C + c];
        if (SCATTER) {
          uint32_t r[4];
          sf_philox4x32_10((uint32_t)orow, (uint32_t)((uint64_t)orow >> 32), 0u, (uint32_t)c, k0, k1, r);
          const float u[4] = {sf_u01(r[0]), sf_u01(r[1]), sf_u01(r[2]), sf_u01(r[3])};
          if (b.kind == SF_NOISE_KIND_ASINH) noise_asinh_scatter(b, tab, f, u, oy[j], os[j]);
          else noise_general_scatter(b, tab, f, u, oy[j], os[j]);
        } else {
          noise_scalings(b, f, err[row * C + c], oy[j], os[j]);
        }
      }
    }
    if (vec4) {   // C % 4 == 0 and 16-byte aligned outputs: the four bands of the group exist
      reinterpret_cast<float4*>(out)[orow * CB + cb] = make_float4(oy[0], oy[1], oy[2], oy[3]);
      if (err_out) reinterpret_cast<float4*>(err_out)[orow * CB + cb] = make_float4(os[0], os[1], os[2], os[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = cb * 4 + j;
        if (c < C) {
          out[orow * C + c] = oy[j];
          if (err_out) err_out[orow * C + c] = os[j];
        }
      }
    }
  }
}

SfScratch g_noise_scratch;

// every check that needs no device; the message names the entry point
int noise_validate(const char* who, int64_t N, int32_t C, const sf_noise_band* bands, const float* table, int64_t n_table,
                   int32_t n_scatters) {
  const std::string w = std::string(who) + ": ";
  if (C < 1 || N < 0 || n_scatters < 1) return sf_fail(SF_ERR_INVALID, w + "need C >= 1, N >= 0, n_scatters >= 1");
  if (!bands || !table || n_table < 0) return sf_fail(SF_ERR_INVALID, w + "null model");
  if (n_table * 4 > SF_NOISE_MAX_TABLE_BYTES)
    return sf_fail(SF_ERR_INVALID, w + "the packed tables exceed 64 KiB (" + std::to_string(n_table * 4) + " bytes): fewer bins or bands per call");
  if ((int64_t)C * (int64_t)sizeof(sf_noise_band) + n_table * 4 > SF_NOISE_MAX_TABLE_BYTES)
    return sf_fail(SF_ERR_INVALID, w + "band structs and tables together exceed the 64 KiB staged per workgroup: fewer bands per call");
  for (int c = 0; c < C; ++c) {
    const sf_noise_band& b = bands[c];
    const std::string bc = w + "band " + std::to_string(c) + ": ";
    if (b.n_bins > SF_NOISE_MAX_BINS) return sf_fail(SF_ERR_INVALID, bc + "more than 256 bins (" + std::to_string(b.n_bins) + ")");
    if (b.n_bins < 2) return sf_fail(SF_ERR_INVALID, bc + "fewer than 2 bins");
    if (b.table_offset < 0 || (int64_t)b.table_offset + 3 * (int64_t)b.n_bins > n_table)
      return sf_fail(SF_ERR_INVALID, bc + "its tables reach past the packed table");
    if (b.kind != SF_NOISE_KIND_GENERAL && b.kind != SF_NOISE_KIND_ASINH) return sf_fail(SF_ERR_INVALID, bc + "unknown kind");
    const bool asinh = b.kind == SF_NOISE_KIND_ASINH;
    const bool spaces_ok = asinh ? ((b.interp_space == SF_NOISE_SPACE_ASINH || b.interp_space == SF_NOISE_SPACE_PHYSICAL) &&
                                    b.out_space == SF_NOISE_SPACE_ASINH)
                                 : ((b.interp_space == SF_NOISE_SPACE_AB || b.interp_space == SF_NOISE_SPACE_PHYSICAL) &&
                                    (b.out_space == SF_NOISE_SPACE_AB || b.out_space == SF_NOISE_SPACE_PHYSICAL));
    if (!spaces_ok || (b.in_space != SF_NOISE_SPACE_AB && b.in_space != SF_NOISE_SPACE_PHYSICAL))
      return sf_fail(SF_ERR_INVALID, bc + "a unit space that this kind of model does not have");
    if (b.flux_rule < SF_NOISE_FLUX_SCATTER || b.flux_rule > SF_NOISE_FLUX_NUMBER) return sf_fail(SF_ERR_INVALID, bc + "unknown flux rule");
    if (asinh && !(b.b_jy > 0.f)) return sf_fail(SF_ERR_INVALID, bc + "an asinh model needs b > 0");
  }
  return SF_OK;
}

template <bool SCATTER>
int noise_run(const char* who, const float* flux, const float* err, int64_t N, int32_t C, const sf_noise_band* bands,
              const float* table, int64_t n_table, int32_t n_scatters, uint64_t seed, float* out, float* err_out,
              void* stream) {
  if (int rc = noise_validate(who, N, C, bands, table, n_table, n_scatters)) return rc;
  if (N == 0) return SF_OK;
  if (!flux || !out || (!SCATTER && (!err || !err_out))) return sf_fail(SF_ERR_INVALID, std::string(who) + ": null argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t band_bytes = (size_t)C * sizeof(sf_noise_band), blob_bytes = band_bytes + (size_t)n_table * 4;
  SfScratchCall ws(g_noise_scratch, who, st);
  const int sub = ws.add(blob_bytes);
  if (int rc = ws.reserve()) return rc;
  uint32_t* blob = ws.get<uint32_t>(sub);
  if (int rc = ws.check()) return rc;
  hipError_t e;
  // pageable host memory: both copies have left the caller's arrays when the calls return
  if ((e = hipMemcpyAsync(blob, bands, band_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return ws.fail("hipMemcpyAsync", e);
  if (n_table > 0 && (e = hipMemcpyAsync((char*)blob + band_bytes, table, (size_t)n_table * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
    return ws.fail("hipMemcpyAsync", e);
  const long total = (long)N * n_scatters * ((C + 3) / 4);
  long blocks = (total + 255) / 256;
  blocks = blocks > 8192 ? 8192 : blocks;
  const int vec4 = (C % 4 == 0) && ((uintptr_t)out % 16 == 0) && (!err_out || (uintptr_t)err_out % 16 == 0);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ 6u;
  hipLaunchKernelGGL((k_noise<SCATTER>), dim3((unsigned)blocks), dim3(256), blob_bytes, st, flux, err, (long)N, (int)C, blob,
                     (int)(blob_bytes / 4), (int)n_scatters, vec4, k0, k1, out, err_out);
  if ((e = hipGetLastError()) != hipSuccess) return ws.fail("k_noise", e);
  return ws.finish();
}

}  // namespace

extern "C" int sf_scatter_empirical(const float* flux, int64_t N, int32_t C, const sf_noise_band* bands, const float* table,
                                    int64_t n_table, int32_t n_scatters, uint64_t seed, float* out, float* err_out,
                                    void* stream) {
  return noise_run<true>("sf_scatter_empirical", flux, nullptr, N, C, bands, table, n_table, n_scatters, seed, out, err_out, stream);
}

extern "C" int sf_apply_scalings(const float* flux, const float* err, int64_t N, int32_t C, const sf_noise_band* bands,
                                 const float* table, int64_t n_table, float* out, float* err_out, void* stream) {
  return noise_run<false>("sf_apply_scalings", flux, err, N, C, bands, table, n_table, 1, 0, out, err_out, stream);
}
