// sf_spectra.hip -- library spectra -> observed-frame spectral features on the device (sf_spectra_transform).
//   ref: src/synference/utils.py:185-254 (transform_spectrum: redshift, kernel width from the resolution curve, rebinning),
//        utils.py:129-182 (convolve_variable_width_gaussian), sbi_runner.py:1096-1178 (_apply_flux_normalization),
//        sbi_runner.py:1339-1381 (units, crop, clip); the rebinning is SpectRes (Carnall 2017, arXiv:1705.05165) with fill 0.
// One workgroup of 256 per spectrum (grid-stride over the rows).  SF_SPECTRA_TRANSFORM: the raw row is staged into LDS once,
// every thread convolves the pixels tid, tid + 256, ... into a second LDS array (consecutive lanes read consecutive words: no
// bank conflicts but for the clamped ends, which broadcast), then every thread rebins the output pixels tid, tid + 256, ...
// from there: a bisection for the first old bin, a walk to the last.  LDS = 2 L floats + 6 KiB: L = 8192 leaves two
// workgroups per CU, L = 16384 (128 KiB) one.
// Wavelengths, bin edges, overlap fractions, sigma and the half-width are fp64 (O(L + M) per spectrum): an fp32 sigma can flip
// ceil(trunc sigma) or the 0.01 test, fp32 edges lose ~1e-7 R of a partial bin.  Flux, weights and the tap sums are fp32.
// Both normalisations are ONE linear functional of the spectrum, so the host folds either into a coefficient table and the
// device takes a dot product: with the raw row (rest frame) or with the finished bins (observed frame).
// Every loop bound is independent of the flux; the tap loop is bounded by h_limit.
#include <hip/hip_runtime.h>

#include <string>

#include "sf_block.h"
#include "sf_internal.h"

namespace {

constexpr double kFwhmPerSigma = 2.3548200450309493;   // 2 sqrt(2 ln 2)

struct SpectraCurve {
  const double* x;
  const double* y;
  int n;
};

// numpy.interp(x, cx, cy): the end values outside, slope * (x - cx[j]) + cy[j] inside
__device__ __forceinline__ double spectra_interp(const SpectraCurve& c, double x) {
  const int n = c.n;
  if (!(x > c.x[0])) return c.y[0];
  if (!(x < c.x[n - 1])) return c.y[n - 1];
  int lo = 0, hi = n - 1;   // c.x[lo] <= x < c.x[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c.x[mid] <= x) lo = mid; else hi = mid;
  }
  const double slope = (c.y[lo + 1] - c.y[lo]) / (c.x[lo + 1] - c.x[lo]);
  return slope * (x - c.x[lo]) + c.y[lo];
}

// edge k of the L + 1 bin edges of the grid w[.] * s (SpectRes: midpoints inside, half a spacing beyond the ends)
__device__ __forceinline__ double spectra_edge(const double* __restrict__ w, double s, int L, int k) {
  if (k == 0) { const double a = w[0] * s, b = w[1] * s; return a - (b - a) / 2; }
  if (k == L) { const double a = w[L - 1] * s, b = w[L - 2] * s; return a + (a - b) / 2; }
  return (w[k] * s + w[k - 1] * s) / 2;
}

__device__ __forceinline__ int spectra_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// normalisation (one scalar per spectrum), units, clip: ref sbi_runner.py:1168-1176, 1361-1367, 1376-1381
__device__ __forceinline__ float spectra_finish(const sf_spectra_desc& d, float v, bool normed, double fac) {
  if (normed) v = fac != 0.0 ? (float)((double)v / fac) : 0.f;
  if (d.unit_code == SF_SPECTRA_UNIT_LINEAR) v = v * d.unit_scale;
  else if (d.unit_code == SF_SPECTRA_UNIT_LOG10) v = log10f(v * d.unit_scale);
  else v = -2.5f * log10f(v * d.unit_scale) + 8.9f;
  return (v != v) ? v : fminf(fmaxf(v, d.clip_lo), d.clip_hi);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_spectra(const sf_spectra_desc d) {
  extern __shared__ __align__(16) float sp_lds[];
  __shared__ double s_red[256];
  __shared__ double s_curve[2 * SF_SPECTRA_MAX_CURVE];
  const int tid = threadIdx.x, L = d.L, M = d.M;
  float* raw = sp_lds;
  float* conv = sp_lds + ((L + 3) & ~3);
  SpectraCurve curve{s_curve, s_curve + SF_SPECTRA_MAX_CURVE, d.n_curve};
  if (MODE == SF_SPECTRA_TRANSFORM) {
    for (int i = tid; i < d.n_curve; i += 256) {
      s_curve[i] = d.curve_wave[i];
      s_curve[SF_SPECTRA_MAX_CURVE + i] = d.curve_r[i];
    }
  }
  const double* __restrict__ w = d.wave;
  for (long row = blockIdx.x; row < d.N; row += gridDim.x) {
    const float* __restrict__ frow = d.flux + row * d.ld_flux;
    float* __restrict__ orow = d.out + row * d.ld_out;
    __syncthreads();   // the previous row's readers of raw / conv are done; the curve is staged
    if (MODE != SF_SPECTRA_UNITS) {
      for (int i = tid; i < L; i += 256) raw[i] = frow[i];
      __syncthreads();
    }
    // the factor on the theory grid: rest frame, and -- as in the reference -- either frame when nothing is redshifted
    const bool norm_raw = d.norm_frame == SF_SPECTRA_NORM_REST || (MODE == SF_SPECTRA_UNITS && d.norm_frame != SF_SPECTRA_NORM_NONE);
    const bool norm_obs = MODE == SF_SPECTRA_TRANSFORM && d.norm_frame == SF_SPECTRA_NORM_OBSERVED;
    double fac = 1.0;
    if (norm_raw) {
      double p = 0.0;
      for (int i = tid; i < L; i += 256) p += (double)(MODE != SF_SPECTRA_UNITS ? raw[i] : frow[i]) * d.norm_table[i];
      fac = sf_block_sum(p, s_red);
    }
    if (MODE == SF_SPECTRA_UNITS) {   // ref 1339-1381: crop (a contiguous range of an ascending grid), units, clip
      for (int j = tid; j < M; j += 256) orow[j] = spectra_finish(d, frow[d.col0 + j], norm_raw, fac);
      continue;
    }
    const double zp1 = MODE == SF_SPECTRA_TRANSFORM ? 1.0 + d.z[row] : 1.0;
    double pix = 1.0;
    if (MODE == SF_SPECTRA_TRANSFORM)   // ref utils.py:234: median(diff(wz)), the middle one / two differences named by the host
      pix = 0.5 * ((w[d.med_lo + 1] * zp1 - w[d.med_lo] * zp1) + (w[d.med_hi + 1] * zp1 - w[d.med_hi] * zp1));
    // ---- variable-width Gaussian: ref utils.py:148-180 ----
    for (int base = 0; base < L; base += 256) {
      const int i = base + tid;
      const bool act = i < L;
      double sg = 0.0;
      if (act) {
        if (MODE == SF_SPECTRA_CONVOLVE) {
          sg = d.sigma_pixels[row * d.sigma_stride + i];
        } else {   // ref utils.py:217-238
          const double wz = w[i] * zp1;
          const double s_inst = wz / spectra_interp(curve, wz) / kFwhmPerSigma;
          const double s_th = wz / (d.theory_r_arr ? d.theory_r_arr[i] : d.theory_r) / kFwhmPerSigma;
          double sq = s_inst * s_inst - s_th * s_th;
          sq = sq < 0.0 ? 0.0 : sq;
          sg = pix != 0.0 ? sqrt(sq) / pix : 0.0;
        }
      }
      const bool copy = sg <= 0.01;
      const double hd = ceil(sg * d.trunc);
      const bool bad = !copy && !(hd <= (double)d.h_limit);   // a kernel wider than h_limit, or a NaN sigma: NaN out
      const int h = (act && !copy && !bad) ? (int)hd : 0;
      const int hmax = spectra_wave_max(h);
      const int ic = act ? i : L - 1;
      const float c = (float)(-0.5 / (sg * sg));
      float acc = raw[ic], wsum = 1.f;
      for (int x = 1; x <= hmax; ++x) {   // to the wave's widest kernel, the taps beyond a lane's own predicated off
        const float fx = (float)x;
        const float t = raw[max(ic - x, 0)] + raw[min(ic + x, L - 1)];
        if (x <= h) {
          const float wt = __expf(c * (fx * fx));
          acc += wt * t;
          wsum += 2.f * wt;
        }
      }
      if (act) {
        const float v = bad ? __builtin_nanf("") : (copy ? raw[i] : acc / wsum);
        if (MODE == SF_SPECTRA_CONVOLVE) orow[i] = v; else conv[i] = v;
      }
    }
    if (MODE == SF_SPECTRA_CONVOLVE) continue;
    __syncthreads();
    // ---- SpectRes onto observed_wave, fill 0 ----
    const double e0 = spectra_edge(w, zp1, L, 0), eL = spectra_edge(w, zp1, L, L);
    double p = 0.0;
    for (int j = tid; j < M; j += 256) {
      const double nl = spectra_edge(d.observed_wave, 1.0, M, j), nr = spectra_edge(d.observed_wave, 1.0, M, j + 1);
      float val = 0.f;
      if (!(nl < e0 || nr > eL)) {
        int lo = 0, hi = L - 1;   // start: the last old bin with edge(start) <= nl
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (spectra_edge(w, zp1, L, mid) <= nl) lo = mid; else hi = mid - 1;
        }
        int k = lo;
        double el = spectra_edge(w, zp1, L, k), er = spectra_edge(w, zp1, L, k + 1);
        if (er >= nr || k == L - 1) {
          val = conv[k];   // the new bin lies inside one old bin
        } else {
          const double wfirst = (er - nl) / (er - el) * (er - el);
          double den = wfirst;
          float num = (float)wfirst * conv[k];
          for (++k; ; ++k) {   // ends at the first old bin with edge(k + 1) >= nr: nr <= eL = edge(L)
            el = er;
            er = spectra_edge(w, zp1, L, k + 1);
            const bool last = er >= nr || k == L - 1;
            const double wk = last ? (nr - el) / (er - el) * (er - el) : er - el;
            num += (float)wk * conv[k];
            den += wk;
            if (last) break;
          }
          val = num / (float)den;
        }
      }
      if (norm_obs) {
        p += (double)val * d.norm_table[j];
        orow[j] = val;
      } else {
        orow[j] = spectra_finish(d, val, norm_raw, fac);
      }
    }
    if (norm_obs) {   // the factor from the finished bins; every thread then rescales the bins it wrote itself
      fac = sf_block_sum(p, s_red);
      for (int j = tid; j < M; j += 256) orow[j] = spectra_finish(d, orow[j], true, fac);
    }
  }
}

template <int MODE>
int spectra_launch(const sf_spectra_desc& d, size_t lds, hipStream_t st) {
  const char* who = "sf_spectra_transform";
  hipError_t e;
  int dev = 0;
  if ((e = hipGetDevice(&dev)) != hipSuccess)
    return sf_fail(SF_ERR_NO_DEVICE, std::string(who) + ": no usable device: " + hipGetErrorString(e));
  if (lds > 32768) {   // 64 KiB and more of dynamic LDS needs the attribute; below, the default covers it with the static 6 KiB
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_spectra<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds)) != hipSuccess)
      return sf_fail(SF_ERR_HIP, std::string(who) + ": hipFuncSetAttribute: " + hipGetErrorString(e));
  }
  const long blocks = d.N > 16384 ? 16384 : d.N;
  hipLaunchKernelGGL((k_spectra<MODE>), dim3((unsigned)blocks), dim3(256), lds, st, d);
  if ((e = hipGetLastError()) != hipSuccess) return sf_fail(SF_ERR_HIP, std::string(who) + ": k_spectra: " + hipGetErrorString(e));
  return SF_OK;
}

}  // namespace

extern "C" int sf_spectra_transform(const sf_spectra_desc* dp, void* stream) {
  const std::string w = "sf_spectra_transform: ";
  if (!dp) return sf_fail(SF_ERR_INVALID, w + "null descriptor");
  const sf_spectra_desc& d = *dp;
  if (d.mode != SF_SPECTRA_UNITS && d.mode != SF_SPECTRA_TRANSFORM && d.mode != SF_SPECTRA_CONVOLVE)
    return sf_fail(SF_ERR_INVALID, w + "unknown mode");
  if (d.N < 0 || d.L < 1 || d.M < 0) return sf_fail(SF_ERR_INVALID, w + "need N >= 0, L >= 1, M >= 0");
  if (d.mode != SF_SPECTRA_UNITS && d.L > SF_SPECTRA_MAX_L)
    return sf_fail(SF_ERR_INVALID, w + "L = " + std::to_string(d.L) + " pixels per spectrum exceeds the cap of " +
                   std::to_string(SF_SPECTRA_MAX_L) + " (two float arrays of L in LDS): crop or rebin the library");
  const int64_t n_out = d.mode == SF_SPECTRA_CONVOLVE ? d.L : d.M;
  if (d.ld_flux < d.L || d.ld_out < n_out) return sf_fail(SF_ERR_INVALID, w + "a row stride shorter than its row");
  if (d.unit_code < SF_SPECTRA_UNIT_LINEAR || d.unit_code > SF_SPECTRA_UNIT_AB) return sf_fail(SF_ERR_INVALID, w + "unknown unit code");
  if (d.norm_frame < SF_SPECTRA_NORM_NONE || d.norm_frame > SF_SPECTRA_NORM_OBSERVED) return sf_fail(SF_ERR_INVALID, w + "unknown normalisation frame");
  if (d.norm_frame != SF_SPECTRA_NORM_NONE && (!d.norm_table || d.mode == SF_SPECTRA_CONVOLVE))
    return sf_fail(SF_ERR_INVALID, w + "a normalisation needs its coefficient table and a mode that has one");
  if (d.mode == SF_SPECTRA_UNITS && (d.col0 < 0 || (int64_t)d.col0 + d.M > d.L))
    return sf_fail(SF_ERR_INVALID, w + "the cropped columns reach past the row");
  if (d.mode == SF_SPECTRA_TRANSFORM) {
    if (d.L < 2 || d.M < 2) return sf_fail(SF_ERR_INVALID, w + "bin edges need at least 2 pixels on either grid");
    if (d.n_curve < 1 || d.n_curve > SF_SPECTRA_MAX_CURVE)
      return sf_fail(SF_ERR_INVALID, w + "a resolution curve of " + std::to_string(d.n_curve) + " nodes does not fit the table of " +
                     std::to_string(SF_SPECTRA_MAX_CURVE) + ": resample the curve");
    if (d.med_lo < 0 || d.med_hi < 0 || d.med_lo > d.L - 2 || d.med_hi > d.L - 2) return sf_fail(SF_ERR_INVALID, w + "median indices outside the grid");
  }
  if (d.mode == SF_SPECTRA_CONVOLVE && d.sigma_stride != 0 && d.sigma_stride < d.L)
    return sf_fail(SF_ERR_INVALID, w + "sigma_pixels: a row stride shorter than L");
  if (d.mode != SF_SPECTRA_UNITS && (!(d.trunc > 0.0) || d.h_limit < 1 || d.h_limit > SF_SPECTRA_MAX_HALF_WIDTH))
    return sf_fail(SF_ERR_INVALID, w + "need trunc > 0 and 1 <= h_limit <= " + std::to_string(SF_SPECTRA_MAX_HALF_WIDTH));
  if (d.N == 0 || n_out == 0) return SF_OK;
  if (!d.flux || !d.out || (d.mode != SF_SPECTRA_CONVOLVE && !d.wave) || (d.mode == SF_SPECTRA_CONVOLVE && !d.sigma_pixels) ||
      (d.mode == SF_SPECTRA_TRANSFORM && (!d.z || !d.observed_wave || !d.curve_wave || !d.curve_r)))
    return sf_fail(SF_ERR_INVALID, w + "null argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = d.mode == SF_SPECTRA_UNITS ? 0 : (size_t)2 * ((d.L + 3) & ~3) * sizeof(float);
  if (d.mode == SF_SPECTRA_UNITS) return spectra_launch<SF_SPECTRA_UNITS>(d, lds, st);
  if (d.mode == SF_SPECTRA_TRANSFORM) return spectra_launch<SF_SPECTRA_TRANSFORM>(d, lds, st);
  return spectra_launch<SF_SPECTRA_CONVOLVE>(d, lds, st);
}
