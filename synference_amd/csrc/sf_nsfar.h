// sf_nsfar.h -- the autoregressive NSF of the `backend="lampe"` route (sf_nsfar.hip): state and entry points used by sf_api.hip /
// sf_train.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/synference_hip.h"
#include "sf_buf.h"

// device state built once, all or nothing (ar_ensure): a local one is filled and moved into the handle
struct SfNsfArDev {
  SfBuf<float> d_img;
  SfBuf<int32_t> d_src, d_none, d_perm, d_ptype, d_tend, d_ord, d_dimof, d_dwave;
  SfBuf<float> d_xmean, d_xstd;
  SfBuf<unsigned char> d_live;           // [n_params] 1 = the parameter has a gradient (unmasked weight or bias)
  SfPinned<unsigned long long> h_ctr;    // pinned host copy of d_ctr (read back after the persistent launch and after every round)
  SfBuf<unsigned long long> d_ctr;       // [0] work cursor of the sampler, [1] slots written off, [2] evaluations, [3] first attempts rejected
};
struct SfNsfArSurv { SfBuf<uint32_t> d_surv[2], d_best; };   // survivor lists of the find / resolve rounds, lowest accepted attempt: one capacity
struct SfNsfAr : SfNsfArDev, SfNsfArSurv {
  int D = 0, C = 0, H = 0, Hp = 0, T = 0, K = 0, NP = 0;
  float bound = 5.f, cw = 0.f, cd = 0.f, logdet0 = 0.f;
  float th_scale[16], th_shift[16];
  std::vector<float> h_xmean, h_xstd;
  // hidden rows sorted by type; perm[p] = logical unit of physical row p (-1: padding), ptype[p] its type, tend[r] = rows of type <= r
  std::vector<int32_t> perm, ptype, tend, ord, dimof, dwave, src;
  int64_t n_params = 0;
  long P_t = 0, t_stride = 0;
  int l_W0 = 0, l_b0 = 0, l_W1 = 0, l_b1 = 0, l_W2 = 0, l_b2 = 0;                             // logical offsets in a transform
  int o_L0t = 0, o_b0 = 0, o_L1t = 0, o_L1m = 0, o_b1 = 0, o_L2t = 0, o_b2 = 0, o_L0m = 0, o_L2m = 0;   // image offsets in a transform
  // 16-sample register-tile sampler (sf_nsfar16.hip): s16_nt = hidden tiles (= D x s16_tpt: type r is tile r, or tiles 2 r and 2 r + 1
  // when it has 17..32 units) or 0 when the shape does not take it;
  // fragment-ordered blocks of a transform (lane l of block (ot, kt): W[16 ot + (l & 15)][16 kt + 4 (l >> 4) + 0..3]) in the sampler's
  // own hidden order (s16_ks = ceil(units per type / 4), at least 2: the units of a type sit on the rows with (row & 3) < s16_ks of
  // its tile), biases in that order
  int s16_nt = 0, s16_ni = 0, s16_ks = 4, s16_tpt = 1, o_F0 = 0, o_fb0 = 0, o_F1 = 0, o_fb1 = 0, o_F2 = 0;
  bool dev_ready = false;
  int affine = 0;               // SF_MAF_AR (zuko MAF): MonotonicAffineTransform instead of the spline
  SfBuf<float> d_ustash;
  SfBuf<float> d_gpart;              // per-workgroup gradient partials of the training kernel (small batches)
  SfBuf<int32_t> d_gal;              // [2][M]: attempts / accepted draws per row (progress rule of the uncapped sampler)
  double last_evals = 0.0, last_rej0 = 0.0;   // of the last sampling call that read the counters back
};

int sf_nsfar_create(const sf_flow_desc& d, SfNsfAr** out);
void sf_nsfar_destroy(SfNsfAr* n);
size_t sf_nsfar_lds_bytes(const SfNsfAr& n, int hidden_buffers, int waves = 1);
// re-tiles the logical vector into the masked images (every entry point below reads the images of the LAST pack)
int sf_nsfar_pack(SfNsfAr* n, const float* flat, hipStream_t st);
struct SfLpOut;   // sf_internal.h: lp, z, lad -- each written unless NULL
int sf_nsfar_log_prob(SfNsfAr* n, const float* theta, const float* x, long B, SfLpOut out, hipStream_t st);
int sf_nsfar_inverse(SfNsfAr* n, const float* z, const float* x, long B, float* theta, float* logdet, hipStream_t st);
// count != null: acceptance counting (one attempt per item, item i belongs to row i / S); else the rejection sampler
int sf_nsfar_sample(SfNsfAr* n, const float* x, long M, long S, const uint32_t* slots, long n_slots, const float* lo, const float* hi,
                    uint32_t k0, uint32_t k1, unsigned long long slot_offset, int max_attempts, float* out, int32_t* n_drawn,
                    int32_t* count, int64_t* n_unfilled, hipStream_t st, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// One sampling call as all six sampler kernels take it (sf_ar_sampler.h: the control flow; sf_nsfar.hip / sf_nsfar16.hip: the candidate routines and kernels).
// cursor = d_ctr: [0] work cursor, [2] evaluations, [3] first attempts rejected.
struct SfArLaunch {
  const float* x; long S; const uint32_t* slots; long n_slots; const float* lo; const float* hi; uint32_t k0, k1; unsigned long long slot_offset;
  uint32_t max_attempts; float* out; int32_t* n_drawn; int32_t* count; unsigned long long* cursor; unsigned int* n_unfilled; int32_t* g_try;
  int32_t* g_acc; unsigned long long walk_R, walk_C; uint32_t window_end; uint32_t* surv; unsigned int* n_surv;
};
// One chip-wide round: FIND tries attempts [base, att_end) of the n_surv survivors (64 per workgroup, `chunks` workgroups per
// survivor) and lowers best[]; RESOLVE writes the found draws and appends what stays open to next[] (base == att_end: nothing was
// tried, the last RESOLVE that writes off what the ceiling left open).
struct SfArRound {
  const uint32_t* surv; unsigned int n_surv; uint32_t* best; uint32_t base, chunks, att_end; uint32_t* next; unsigned int* n_next;
};
// sf_nsfar16.hip: the three launches on 16-candidate register tiles, for the shapes that take them
bool sf_nsfar16_eligible(const SfNsfAr& n);
hipError_t sf_nsfar16_launch(const SfNsfAr& n, const SfArLaunch& L, int cus, hipStream_t st);
hipError_t sf_nsfar16_find(const SfNsfAr& n, const SfArLaunch& L, const SfArRound& R, hipStream_t st);
hipError_t sf_nsfar16_resolve(const SfNsfAr& n, const SfArLaunch& L, const SfArRound& R, hipStream_t st);
int sf_nsfar_loss_grad(SfNsfAr* n, const float* flat, const float* theta, const float* x, const long long* idx, long B, float grad_scale,
                       const float* weights, float* loss, double* loss_sum, float* grad, hipStream_t st, hipEvent_t ev0 = nullptr,
                       hipEvent_t ev1 = nullptr);
