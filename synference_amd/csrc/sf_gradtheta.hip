// sf_gradtheta.hip -- posterior mode finding.
//   (1) sf_flow_log_prob_grad: log q(theta | x) and d log q / d theta for MAF and the coupling NSF.  The kernels
//       (sf_gradtheta_kernels.h, instantiated per hidden-tile count in sf_gradtheta_inst.hip) are the forward + backward
//       sweep of the training kernels over 32-row tiles with the weight-gradient work left out; the backward products
//       read the transposed operand image.  For training that image is rebuilt from the caller's vector on every call;
//       here it is an INFERENCE image of the handle's own vector: built on the first gradient call after
//       sf_flow_set_params and kept until the next one (buffers of its own, so that training never sees it).
//   (2) sf_map_step: one fused ascent step of the mode search over [B, D] (box transform, chain rule, Adam, best
//       tracking, next theta).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "sf_gradtheta_kernels.h"
#include "sf_internal.h"

#define SF_GDECL(H)                                                                              \
  hipError_t sf_launch_maf_gradtheta_h##H(const SfDev&, const SfGradThetaArgs&, long, hipStream_t); \
  hipError_t sf_launch_nsf_gradtheta_h##H(const SfDev&, const SfGradThetaArgs&, long, hipStream_t);
SF_GDECL(1) SF_GDECL(2) SF_GDECL(3) SF_GDECL(4)

namespace {

// The stash of one launch is bounded; a larger batch runs as several launches over consecutive tiles.  The bound is 256 MiB,
// or one tile per SIMD of the device where that is more: the kernels run one wave per SIMD, so a launch of fewer tiles than
// the device has SIMDs leaves part of it idle (the production NSF, H = 69 / T = 15, stashes 1.4 MB per tile: 189 tiles in
// 256 MiB against 1024 SIMDs, 1.4 GiB for the full width).
constexpr size_t kStashCapFloats = (size_t)64 << 20;  // 256 MiB

long gt_device_simds() {
  int dev = 0;
  hipDeviceProp_t pr;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
    return 4L * pr.multiProcessorCount;
  return 1024;
}
}  // namespace

// ---------------------------------------------------------------------------------------------
// fused ascent step
// ---------------------------------------------------------------------------------------------
struct SfMapStepArgs {
  long B;
  int D;
  float* phi; float* m; float* v;
  float* theta;             // in: the point lp / g were evaluated at; out: the next point
  const float* lp; const float* g;   // g == null: score only (the evaluation after the last step)
  const float* lo; const float* hi;  // null: identity transform
  float* best_theta; float* best_lp;
  float step_size, inv_sqrt_bc2, beta1, beta2, eps;
  int save_best;
};

// one thread per candidate: a candidate's D coordinates share the "finite?" decision and the best-so-far record.  Lanes
// therefore touch [B, D] arrays with stride D (uncoalesced) and the sigmoid is taken twice per coordinate: accepted, the
// launch moves 9 floats per coordinate beside a flow kernel that runs T MADE / coupling networks per row
// (scripts/time_map.py times the two side by side).
__global__ __launch_bounds__(256) void k_map_step(SfMapStepArgs a) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const int D = a.D;
  const float lp = a.lp[b];
  bool ok = isfinite(lp);
  float g[SF_DMAX];
  if (a.g) {
#pragma unroll
    for (int d = 0; d < SF_DMAX; ++d) {
      g[d] = 0.f;
      if (d < D) {
        g[d] = a.g[b * D + d];
        ok = ok && isfinite(g[d]);
      }
    }
  }
  if (!ok) return;  // frozen: phi, theta, the moments and the best stay as they are
  if (a.save_best && lp > a.best_lp[b]) {
    a.best_lp[b] = lp;
#pragma unroll
    for (int d = 0; d < SF_DMAX; ++d)
      if (d < D) a.best_theta[b * D + d] = a.theta[b * D + d];
  }
  if (!a.g) return;
#pragma unroll
  for (int d = 0; d < SF_DMAX; ++d) {
    if (d < D) {
      const long i = b * D + d;
      float phi = a.phi[i];
      float gphi = g[d];
      float lo = 0.f, w = 1.f;
      if (a.lo) {
        lo = a.lo[d];
        w = a.hi[d] - lo;
        const float s = 1.f / (1.f + expf(-phi));
        gphi *= w * s * (1.f - s);
      }
      const float gi = -gphi;  // Adam minimises -log q
      const float mi = a.beta1 * a.m[i] + (1.f - a.beta1) * gi;
      const float vi = a.beta2 * a.v[i] + (1.f - a.beta2) * gi * gi;
      a.m[i] = mi;
      a.v[i] = vi;
      phi -= a.step_size * (mi / (sqrtf(vi) * a.inv_sqrt_bc2 + a.eps));
      a.phi[i] = phi;
      a.theta[i] = a.lo ? lo + w * (1.f / (1.f + expf(-phi))) : phi;
    }
  }
}

extern "C" {

int sf_map_step(int64_t B, int64_t D, float* phi, float* exp_avg, float* exp_avg_sq, float* theta, const float* lp,
                const float* g_theta, const float* lo, const float* hi, float* best_theta, float* best_lp,
                float learning_rate, int64_t step, int save_best, void* stream) {
  if (B == 0) return SF_OK;
  if (B < 0 || D < 1 || D > SF_DMAX) return sf_fail(SF_ERR_INVALID, "sf_map_step: B < 0 or D outside 1..16");
  if (!theta || !lp || !best_theta || !best_lp) return sf_fail(SF_ERR_INVALID, "sf_map_step: null argument");
  if (g_theta && (!phi || !exp_avg || !exp_avg_sq || step < 1))
    return sf_fail(SF_ERR_INVALID, "sf_map_step: a step needs phi, both moments and step >= 1");
  if ((lo == nullptr) != (hi == nullptr)) return sf_fail(SF_ERR_INVALID, "sf_map_step: lo and hi come together");
  SfMapStepArgs a;
  a.B = (long)B; a.D = (int)D; a.phi = phi; a.m = exp_avg; a.v = exp_avg_sq; a.theta = theta; a.lp = lp; a.g = g_theta;
  a.lo = lo; a.hi = hi; a.best_theta = best_theta; a.best_lp = best_lp;
  a.beta1 = 0.9f; a.beta2 = 0.999f; a.eps = 1e-8f;
  const double t = (double)(step < 1 ? 1 : step);
  a.step_size = (float)((double)learning_rate / (1.0 - std::pow(0.9, t)));
  a.inv_sqrt_bc2 = (float)(1.0 / std::sqrt(1.0 - std::pow(0.999, t)));
  a.save_best = save_best;
  hipLaunchKernelGGL(k_map_step, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  SF_TRY_SET(hipGetLastError());
  return SF_OK;
}

int sf_flow_log_prob_grad(sf_flow* f, const float* theta, const float* x, int64_t rows_per_x, int64_t B, float* lp,
                          float* dtheta, void* stream) {
  if (!f) return sf_fail(SF_ERR_INVALID, "null handle");
  if (f->nsf1) return sf_fail(SF_ERR_INVALID, "sf_flow_log_prob_grad: the one-parameter NSF has no theta-gradient path");
  if (f->nsfar)
    return sf_fail(SF_ERR_INVALID, std::string("sf_flow_log_prob_grad: the autoregressive ") +
                                       (f->L.dev.kind == SF_MAF_AR ? "MAF (maf_ar)" : "NSF (nsf_ar)") +
                                       " has no theta-gradient path");
  if (B == 0 || (!lp && !dtheta)) return SF_OK;
  if (B < 0 || rows_per_x < 1) return sf_fail(SF_ERR_INVALID, "sf_flow_log_prob_grad: B < 0 or rows_per_x < 1");
  if (!theta || !x) return sf_fail(SF_ERR_INVALID, "null argument");
  if (!f->params_set || !f->flat_valid)
    return sf_fail(SF_ERR_STATE, "sf_flow_log_prob_grad: no parameters held by the handle (after sf_flow_loss_grad the caller's "
                                 "vector is the master copy: call sf_flow_set_params first)");
  hipStream_t st = (hipStream_t)stream;
  const SfLayout& L = f->L;
  if (dtheta && !f->gt_image_valid) {
    const size_t n = (size_t)L.n_packedT;
    if (!f->d_gtT) {
      // (blocking copies, once per handle: the tables are in place before the gather below is queued on any stream)
      SfFlowGt g;   // all or nothing
      SF_TRY_SET(g.d_gtT.alloc(n));
      SF_TRY_SET(g.d_gt1.alloc(n));
      SF_TRY_SET(g.d_gt2.alloc(n));
      SF_TRY_SET(hipMemcpy(g.d_gt1, L.srcT1.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
      SF_TRY_SET(hipMemcpy(g.d_gt2, L.srcT2.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
      static_cast<SfFlowGt&>(*f) = std::move(g);
    }
    SF_TRY_SET(sf_launch_pack(f->d_flat, f->d_gt1, f->d_gt2, f->d_gtT, (long)n, st));
    f->gt_image_valid = true;
  }
  SfDev m = f->dev();
  m.packedT = f->d_gtT;
  const long tiles = ((long)B + 31) / 32;
  long per_launch = tiles;
  SfGradThetaArgs a;
  a.theta = theta; a.x = x; a.B = (long)B; a.rows_per_x = (long)rows_per_x; a.lp = lp; a.dtheta = dtheta;
  a.act = nullptr; a.act_per_wave = 0;
  if (dtheta) {
    const long tiles_per_wave = (long)m.T * (m.kind == SF_MAF ? ((m.NB + 1) * m.HT + 1) : (2 + (3 * m.NB + 1) * m.HT));
    a.act_per_wave = tiles_per_wave * 4 * 64;  // float4
    const size_t per_tile = (size_t)a.act_per_wave * 4;
    long cap_tiles = (long)(kStashCapFloats / per_tile);
    if (per_launch > cap_tiles) {  // (the device is asked only when the batch does not fit the 256 MiB)
      if (f->gt_simds == 0) f->gt_simds = gt_device_simds();
      if (cap_tiles < f->gt_simds) cap_tiles = f->gt_simds;
      if (per_launch > cap_tiles) per_launch = cap_tiles;
    }
    const size_t need = (size_t)per_launch * per_tile;
    SF_TRY_SET(f->d_act.grow(need));  // (the stash is scratch shared with the training kernels)
    a.act = reinterpret_cast<float4*>(f->d_act.get());
  }
  const bool maf = m.kind == SF_MAF;
  for (long t0 = 0; t0 < tiles; t0 += per_launch) {
    a.tile0 = t0;
    const long n = tiles - t0 < per_launch ? tiles - t0 : per_launch;
    switch (m.HT) {
      case 1: SF_TRY_SET(maf ? sf_launch_maf_gradtheta_h1(m, a, n, st) : sf_launch_nsf_gradtheta_h1(m, a, n, st)); break;
      case 2: SF_TRY_SET(maf ? sf_launch_maf_gradtheta_h2(m, a, n, st) : sf_launch_nsf_gradtheta_h2(m, a, n, st)); break;
      case 3: SF_TRY_SET(maf ? sf_launch_maf_gradtheta_h3(m, a, n, st) : sf_launch_nsf_gradtheta_h3(m, a, n, st)); break;
      case 4: SF_TRY_SET(maf ? sf_launch_maf_gradtheta_h4(m, a, n, st) : sf_launch_nsf_gradtheta_h4(m, a, n, st)); break;
      default: return sf_fail(SF_ERR_INVALID, "bad HT");
    }
  }
  return SF_OK;
}

}  // extern "C"
