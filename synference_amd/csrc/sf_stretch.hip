// sf_stretch.hip -- conditional posteriors: one half-step of the affine-invariant ensemble sampler (Goodman & Weare 2010,
// the "stretch move"; DESIGN.md section 19, tests/stretch_model.py) for N catalogue rows x W walkers.
//
// One launch per half-step, three phases in this order:
//   (1) resolve   the proposals of the previous half-step, given their log-density: walkers, lp, the accept counter
//   (2) collect   the row's walkers and lp into its block of the result, at a collecting point
//   (3) propose   the moves of this half-step's active walkers (w % 2 == half) against partners of the other half
// The proposals of (3) read partners that (1) has just moved, so a row lives in ONE wave: lane = walker (W <= 64), its
// W x D block sits in the wave's slice of LDS between the phases, and the order of the phases is the wave's program order.
// Four rows per workgroup; the waves of a workgroup share nothing.
//
// Memory: `walkers`, `prop` and the result are [., D] arrays with D no multiple of 4.  A row's block is contiguous, so it
// is moved with whole-wave loads and stores of consecutive floats (lane k, k + 64, ...) through LDS; the per-walker work
// reads LDS.  Plain loads and stores only: a row is owned by one wave, nothing is accumulated across waves.
//
// Random words: r = philox4x32_10((p_lo, p_hi, 2 t + h, w), (seed_lo, seed_hi ^ SF_STREAM_STRETCH)), p the row's position
// in the whole catalogue: r0 -> partner, r1 -> stretch factor, r2 -> the accept uniform (regenerated when the half-step is
// resolved, one launch later: nothing is carried between launches but the proposals themselves).
#include <hip/hip_runtime.h>

#include <string>

#include "sf_internal.h"
#include "sf_rng.h"

#define SF_STREAM_STRETCH 0x53545200u
#define SF_STRETCH_ROWS 4   // rows (waves) per workgroup

struct SfStretchArgs {
  long N;
  int D, W;
  float* walkers;           // [N, W, D]
  float* lp;                // [N, W]
  const int32_t* fixed;     // [N] bit d: coordinate d is fixed; negative: the row is dead (NaN row), nothing of it is written
  const float* lo; const float* hi;   // [D], both or neither
  const float* lp_prop;     // [N, W/2] density at the pending proposals (resolve)
  float* prop;              // [N, W/2, D] in: the pending proposals (resolve); out: the new ones (propose)
  int32_t* accepted;        // [N] accepted moves so far
  float* out; float* out_lp;   // [N, S, D], [N, S] (out_lp may be null)
  long S, slot0;            // slot0 = c * W: first slot of this collecting point; < 0: none
  int32_t* trace_partner;   // [N, W/2] partner of every proposal written (may be null)
  int32_t* trace_accept;    // [N, W/2] accept flag of every proposal resolved (may be null)
  unsigned long long row_offset;
  uint32_t k0, k1;
  uint32_t half_step;       // 2 t + h of the half-step that is proposed; the one resolved is half_step - 1
  int resolve, propose;
};

__device__ __forceinline__ void sf_wave_sync() {
  // LDS operations of one wave complete in issue order: only the compiler has to be kept from moving them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the stretch factor of g(z) ~ 1 / sqrt(z) on [1/a, a], a = 2: z = ((a - 1) u + 1)^2 / a
__device__ __forceinline__ float sf_stretch_z(uint32_t r1) {
  const float s = sf_u01(r1) + 1.0f;
  return s * s * 0.5f;
}

__global__ __launch_bounds__(64 * SF_STRETCH_ROWS) void k_stretch_step(SfStretchArgs a) {
  __shared__ float s_w[SF_STRETCH_ROWS][64 * SF_DMAX];
  __shared__ float s_p[SF_STRETCH_ROWS][32 * SF_DMAX];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * SF_STRETCH_ROWS + wave;
  if (i >= a.N) return;   // (whole waves leave: nothing below synchronises across waves)
  const int D = a.D, W = a.W, W2 = a.W >> 1;
  const int32_t fx = a.fixed[i];
  const int n_free = D - __popc((unsigned)fx & ((1u << D) - 1u));
  if (fx < 0 || n_free < 1) return;
  float* sw = s_w[wave];
  float* sp = s_p[wave];
  const size_t wbase = (size_t)i * W * D, pbase = (size_t)i * W2 * D;
  const unsigned long long pos = a.row_offset + (unsigned long long)i;
  const bool mine = lane < W;

  for (int k = lane; k < W * D; k += 64) sw[k] = a.walkers[wbase + k];
  if (a.resolve)
    for (int k = lane; k < W2 * D; k += 64) sp[k] = a.prop[pbase + k];
  float lpw = mine ? a.lp[(size_t)i * W + lane] : 0.f;
  sf_wave_sync();

  // ---- (1) resolve the previous half-step
  if (a.resolve) {
    const uint32_t hs = a.half_step - 1u;
    const int h = (int)(hs & 1u);
    const bool active = mine && (lane & 1) == h;
    const int q = lane >> 1;
    bool acc = false;
    if (active) {
      uint32_t r[4];
      sf_philox4x32_10((uint32_t)pos, (uint32_t)(pos >> 32), hs, (uint32_t)lane, a.k0, a.k1, r);
      const float z = sf_stretch_z(r[1]);
      const float lpy = a.lp_prop[(size_t)i * W2 + q];
      bool inside = true;
      if (a.lo)
        for (int d = 0; d < D; ++d) {
          const float y = sp[q * D + d];
          inside = inside && y >= a.lo[d] && y <= a.hi[d];
        }
      acc = inside && isfinite(lpy) && logf(sf_u01(r[2])) < (float)(n_free - 1) * logf(z) + lpy - lpw;
      if (acc) {
        for (int d = 0; d < D; ++d) sw[lane * D + d] = sp[q * D + d];
        lpw = lpy;
      }
      if (a.trace_accept) a.trace_accept[(size_t)i * W2 + q] = acc ? 1 : 0;
    }
    const int n_acc = __popcll(__ballot(acc));
    if (mine) a.lp[(size_t)i * W + lane] = lpw;
    if (lane == 0) a.accepted[i] += n_acc;
    sf_wave_sync();
    for (int k = lane; k < W * D; k += 64) a.walkers[wbase + k] = sw[k];
  }

  // ---- (2) collect: slots [slot0, slot0 + W) of the row's [S, D] block, those below S
  if (a.slot0 >= 0 && a.slot0 < a.S) {
    const long left = a.S - a.slot0;
    const int nw = left < W ? (int)left : W;
    const size_t obase = ((size_t)i * a.S + a.slot0) * D;
    for (int k = lane; k < nw * D; k += 64) a.out[obase + k] = sw[k];
    if (a.out_lp && lane < nw) a.out_lp[(size_t)i * a.S + a.slot0 + lane] = lpw;
  }

  // ---- (3) propose this half-step
  if (a.propose) {
    sf_wave_sync();   // (the proposals of (1) have been read out of sp)
    const int h = (int)(a.half_step & 1u);
    if (mine && (lane & 1) == h) {
      const int q = lane >> 1;
      uint32_t r[4];
      sf_philox4x32_10((uint32_t)pos, (uint32_t)(pos >> 32), a.half_step, (uint32_t)lane, a.k0, a.k1, r);
      const int j = 2 * (int)(((r[0] >> 9) * (uint32_t)W2) >> 23) + (1 - h);
      const float z = sf_stretch_z(r[1]);
      for (int d = 0; d < D; ++d) {
        const float tw = sw[lane * D + d], tj = sw[j * D + d];
        sp[q * D + d] = ((fx >> d) & 1) ? tw : tj + z * (tw - tj);
      }
      if (a.trace_partner) a.trace_partner[(size_t)i * W2 + q] = j;
    }
    sf_wave_sync();
    for (int k = lane; k < W2 * D; k += 64) a.prop[pbase + k] = sp[k];
  }
}

extern "C" {

int sf_stretch_step(int64_t N, int64_t D, int64_t W, int64_t max_fixed, float* walkers, float* lp, const int32_t* fixed,
                    const float* lo, const float* hi, const float* lp_prop, float* prop, int32_t* accepted, float* out,
                    float* out_lp, int64_t S, int64_t collect, uint64_t seed, int64_t row_offset, int64_t half_step,
                    int resolve, int propose, int32_t* trace_partner, int32_t* trace_accept, void* stream) {
  if (N < 0 || S < 0 || row_offset < 0 || half_step < 0 || half_step > 0xFFFFFFFFll)
    return sf_fail(SF_ERR_INVALID, "sf_stretch_step: a negative size, row_offset or half_step (or half_step >= 2^32)");
  if (D < 1 || D > SF_DMAX) return sf_fail(SF_ERR_INVALID, "sf_stretch_step: D outside 1..16");
  if (W < 4 || W > 64 || (W & 1))
    return sf_fail(SF_ERR_INVALID, "sf_stretch_step: W = " + std::to_string((long long)W) + ": an even number of walkers in 4..64");
  if (max_fixed < 0 || max_fixed >= D)
    return sf_fail(SF_ERR_INVALID, "sf_stretch_step: max_fixed = " + std::to_string((long long)max_fixed) + " of D = " +
                                       std::to_string((long long)D) + ": a row's free set is empty (at least one free coordinate)");
  if (resolve && half_step < 1) return sf_fail(SF_ERR_INVALID, "sf_stretch_step: half-step 0 has no predecessor to resolve");
  if (N == 0) return SF_OK;
  if (!walkers || !lp || !fixed) return sf_fail(SF_ERR_INVALID, "sf_stretch_step: null argument (walkers, lp, fixed)");
  if ((lo == nullptr) != (hi == nullptr)) return sf_fail(SF_ERR_INVALID, "sf_stretch_step: lo and hi come together");
  if (resolve && (!lp_prop || !prop || !accepted))
    return sf_fail(SF_ERR_INVALID, "sf_stretch_step: resolving needs lp_prop, prop and accepted");
  if (propose && !prop) return sf_fail(SF_ERR_INVALID, "sf_stretch_step: proposing needs prop");
  if (collect >= 0 && !out) return sf_fail(SF_ERR_INVALID, "sf_stretch_step: a collecting point needs out");
  if (collect >= 0 && collect * W >= S) return sf_fail(SF_ERR_INVALID, "sf_stretch_step: collecting point beyond the S slots");
  SfStretchArgs a;
  a.N = (long)N; a.D = (int)D; a.W = (int)W; a.walkers = walkers; a.lp = lp; a.fixed = fixed; a.lo = lo; a.hi = hi;
  a.lp_prop = lp_prop; a.prop = prop; a.accepted = accepted; a.out = out; a.out_lp = out_lp; a.S = (long)S;
  a.slot0 = collect >= 0 ? (long)(collect * W) : -1;
  a.trace_partner = trace_partner; a.trace_accept = trace_accept;
  a.row_offset = (unsigned long long)row_offset;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32) ^ SF_STREAM_STRETCH;
  a.half_step = (uint32_t)half_step; a.resolve = resolve ? 1 : 0; a.propose = propose ? 1 : 0;
  const long blocks = ((long)N + SF_STRETCH_ROWS - 1) / SF_STRETCH_ROWS;
  if (blocks > 0x7FFFFFFFl) return sf_fail(SF_ERR_INVALID, "sf_stretch_step: more than 2^33 rows in one launch");
  hipLaunchKernelGGL(k_stretch_step, dim3((unsigned)blocks), dim3(64 * SF_STRETCH_ROWS), 0, (hipStream_t)stream, a);
  SF_TRY_SET(hipGetLastError());
  return SF_OK;
}

}  // extern "C"
