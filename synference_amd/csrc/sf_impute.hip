// sf_impute.hip -- SBI++ missing-band imputation on the device: for every observed row with missing bands, the training
// rows nearest in the observed bands, one weighted Gaussian KDE per missing band, and nmc completed photometry vectors
// drawn from them.  Restates MissingPhotometryHandler._get_neighbor_kdes / _chi2dof / generate_imputations (Mode 1)
// (ref: src/synference/sbi_runner.py:7736-7791, 7831-7841) and scipy.stats.gaussian_kde(x, bw_method=bw, weights=w) in 1-D.
//
// Per object m (V = observed bands, X = missing bands):
//   chi2[t]  = (sum_{b in V} ((train[t,b] - obs[m,b]) / sigma[m,b])^2) / dof   fp32, every operation rounded on its own, NaN
//              terms skipped (np.nansum), dof = #{b in V : obs finite}
//   ladder   thr_0 = ini_chi2, thr_{l+1} = thr_l + chi2_step (fp32) while <= max_chi2: the first level that admits at least
//            min_neighbours rows; none -> the rows of the last level; none at all -> the fallback_k smallest chi2 (ties to
//            the lowest row); a final set of fewer than min_neighbours rows is a failure (n_used = -1); no finite observed
//            band: n_used = -2
//   weights  w = 1 / dist, dist = fp64 Euclidean distance over V (0 -> 1e-10); lists are in ascending training row
//   KDE      var_b = bw^2 * sum wn (x - mu)^2 / (1 - sum wn^2), mu = sum wn x, wn = w / sum w, all fp64, fixed order
//   draws    r = philox(counter ((row_offset + m) lo, hi, i, b), key (seed, STREAM 5)) -- streams 0-2 are the sampler's and the
//            depth scatter's, 3-4 TARP's; neighbour j = first with C_j > u * C_last, C = running fp64 sum of w, u = (r0 + 0.5) 2^-32;
//            value = x_j + (float)sqrt(var) * z, z = the first normal of (r2, r3) (sf_rng.h's Box-Muller)
//
// Passes: (1) k_imp_count streams the training set in chunks of 2048 rows against a tile of 32 objects held in LDS and
// writes, per (object, chunk), the int32 number of rows under every ladder level; (2) k_imp_decide picks the level (or
// radix-selects the fallback set on the bit pattern of chi2) and scans the chunk counts into list offsets; (3) k_imp_compact
// recomputes chi2 and writes each object's rows in ascending order (ballot prefix inside a wave, no atomics, no
// unordered append); (4) k_imp_draw, one workgroup per object: weights, CDF, moments, draws.  Objects go through (3)-(4)
// in groups whose neighbour total fits a fixed scratch budget (SF_IMPUTE_SCRATCH_BYTES, default 256 MiB); the group
// boundaries come from pass (2)'s counts, which the host reads back (one small copy and a stream wait per batch).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "sf_block.h"
#include "sf_internal.h"
#include "sf_rng.h"
#include "sf_scratch.h"

#define SF_IMP_BMAX 32
#define SF_IMP_FMAX 64
#define SF_IMP_LMAX 32   // ladder levels
#define SF_IMP_CH 2048   // training rows per chunk (8 sub-tiles of 256)
#define SF_IMP_OT 32     // objects per tile of the counting pass
#define SF_IMP_ENTRY 20  // scratch bytes per list entry: row (4) + weight (8) + running sum (8)

struct SfImpCols { int32_t bc[SF_IMP_BMAX]; int32_t ec[SF_IMP_BMAX]; };
struct SfImpLadder { float thr[SF_IMP_LMAX]; int32_t L; };

// chi2 / dof of one training row; x(b) yields train[t, band_col[b]].  One rounding per operation: the counting pass, the
// fallback selection and the compaction pass must give the same bits for the same row.
template <class XF>
__device__ __forceinline__ float sf_imp_chi2(XF x, const float* y, const float* sg, uint32_t vm, int B, float dof) {
#pragma clang fp contract(off)   // no fused multiply-add of the square into the sum: the same bits wherever this is inlined
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    if ((vm >> b) & 1u) {
      const float q = __fdiv_rn(__fsub_rn(x(b), y[b]), sg[b]);
      const float t = __fmul_rn(q, q);
      if (t == t) acc = __fadd_rn(acc, t);
    }
  }
  return __fdiv_rn(acc, dof);
}

// the object's band values, sigmas, observed-band mask and dof (threads 0..B-1 fill, thread 0 reduces)
__device__ __forceinline__ void sf_imp_load_object(const float* __restrict__ obs, const float* __restrict__ sigma,
                                                   const uint8_t* __restrict__ missing, long m, int F, int B,
                                                   const SfImpCols& cols, float* y, float* sg, uint32_t* vm, float* dof, int t) {
  if (t < B) {
    y[t] = obs[m * F + cols.bc[t]];
    sg[t] = sigma[m * B + t];
  }
  if (t == 0) {
    uint32_t mask = 0;
    int n = 0;
    for (int b = 0; b < B; ++b) {
      if (!missing[m * B + b]) {
        mask |= 1u << b;
        const float v = obs[m * F + cols.bc[b]];
        n += (v == v && fabsf(v) != __builtin_inff()) ? 1 : 0;
      }
    }
    *vm = mask;
    *dof = (float)n;
  }
}

// ---- 1. counts per (object, chunk, level) -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_imp_count(const float* __restrict__ train, long NT, int F, int B, SfImpCols cols,
                                                   const float* __restrict__ obs, const float* __restrict__ sigma,
                                                   const uint8_t* __restrict__ missing, long m0, int Mb, SfImpLadder lad,
                                                   int NCH, int LC, int32_t* __restrict__ cnt) {
  extern __shared__ float s_x[];                       // [B][256] training values of the sub-tile
  __shared__ float s_y[SF_IMP_OT][SF_IMP_BMAX], s_s[SF_IMP_OT][SF_IMP_BMAX], s_dof[SF_IMP_OT];
  __shared__ uint32_t s_vm[SF_IMP_OT];
  __shared__ int s_h[SF_IMP_OT][SF_IMP_LMAX];
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = blockIdx.x, o0 = blockIdx.y * SF_IMP_OT;
  const int no = Mb - o0 < SF_IMP_OT ? Mb - o0 : SF_IMP_OT;
  const int L = lad.L;
  for (int o = 0; o < no; ++o) sf_imp_load_object(obs, sigma, missing, m0 + o0 + o, F, B, cols, s_y[o], s_s[o], &s_vm[o], &s_dof[o], tid);
  for (int e = tid; e < SF_IMP_OT * SF_IMP_LMAX; e += 256) (&s_h[0][0])[e] = 0;
  const long r0 = (long)c * SF_IMP_CH;
  for (int sub = 0; sub < SF_IMP_CH / 256; ++sub) {
    const long rb = r0 + (long)sub * 256;
    if (rb >= NT) break;
    __syncthreads();   // the previous sub-tile has been read; the object table and the histogram are set
    for (int e = tid; e < B * 256; e += 256) {
      const int b = e >> 8;
      const long r = rb + (e & 255);
      s_x[e] = r < NT ? train[r * F + cols.bc[b]] : 0.f;
    }
    __syncthreads();
    const bool live = rb + tid < NT;
    for (int o = 0; o < no; ++o) {
      const float dof = s_dof[o];
      if (dof == 0.f) continue;
      const float chi2 = sf_imp_chi2([&](int b) { return s_x[b * 256 + tid]; }, s_y[o], s_s[o], s_vm[o], B, dof);
      int lvl = L;
      for (int l = L - 1; l >= 0; --l) lvl = chi2 <= lad.thr[l] ? l : lvl;
      if (!live) lvl = L;
      if (__ballot(lvl < L) != 0ull) {
        for (int l = 0; l < L; ++l) {
          const int n = __popcll(__ballot(lvl == l));
          if (lane == 0 && n) atomicAdd(&s_h[o][l], n);
        }
      }
    }
  }
  __syncthreads();
  for (int o = tid; o < no; o += 256) {   // cumulative over the levels: rows with chi2 <= thr_l
    int run = 0;
    int32_t* dst = cnt + ((long)(o0 + o) * NCH + c) * LC;
    for (int l = 0; l < L; ++l) { run += s_h[o][l]; dst[l] = run; }
  }
}

// ---- block helpers (256 threads, fixed order: the same bits on every call); the sums are sf_block.h's ------------------
// ordered rank of the set flags of the workgroup: returns this thread's exclusive rank, *total = flags set
__device__ __forceinline__ int sf_imp_rank(bool flag, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long ball = __ballot(flag);
  __syncthreads();
  if (lane == 0) s_w[wave] = __popcll(ball);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < 4; ++w) { off += w < wave ? s_w[w] : 0; tot += s_w[w]; }
  *total = tot;
  return off + __popcll(ball & ((1ull << lane) - 1ull));
}

// ---- 2. level (or fallback set) of every object, chunk offsets of its list ---------------------------------------------
__global__ __launch_bounds__(256) void k_imp_decide(const float* __restrict__ train, long NT, int F, int B, SfImpCols cols,
                                                    const float* __restrict__ obs, const float* __restrict__ sigma,
                                                    const uint8_t* __restrict__ missing, long m0, SfImpLadder lad, int NCH, int LC,
                                                    int min_nb, int fallback_k, int32_t* __restrict__ cnt,
                                                    int32_t* __restrict__ choff, int32_t* __restrict__ lvlsel,
                                                    int32_t* __restrict__ nsel, uint32_t* __restrict__ pbits,
                                                    int32_t* __restrict__ n_used, float* __restrict__ thr_used) {
  __shared__ float s_y[SF_IMP_BMAX], s_s[SF_IMP_BMAX], s_dof;
  __shared__ uint32_t s_vm;
  __shared__ int s_red[256], s_hist[256], s_tot[SF_IMP_LMAX];
  __shared__ uint32_t s_pre;
  __shared__ int s_kk, s_eq_taken;
  const int o = blockIdx.x, tid = threadIdx.x;
  const long m = m0 + o;
  const int L = lad.L;
  int32_t* co = cnt + (long)o * NCH * LC;
  sf_imp_load_object(obs, sigma, missing, m, F, B, cols, s_y, s_s, &s_vm, &s_dof, tid);
  for (int l = 0; l < L; ++l) {
    int v = 0;
    for (int c = tid; c < NCH; c += 256) v += co[(long)c * LC + l];
    v = sf_block_sum(v, s_red);
    if (tid == 0) s_tot[l] = v;
  }
  __syncthreads();
  const float dof = s_dof;
  int lvl = L - 1;
  for (int l = L - 1; l >= 0; --l) lvl = s_tot[l] >= min_nb ? l : lvl;
  int n = s_tot[lvl];
  bool fb = false;
  if (dof == 0.f) {
    n = 0;
  } else if (n == 0) {
    // the fallback_k smallest chi2: radix select on the bit pattern (chi2 >= 0 or +inf: the pattern orders like the value)
    fb = true;
    const long k = fallback_k < NT ? fallback_k : NT;
    n = (int)k;
    if (tid == 0) { s_pre = 0u; s_kk = (int)k - 1; }
    for (int p = 0; p < 4; ++p) {
      const int shift = 24 - 8 * p;
      s_hist[tid] = 0;
      __syncthreads();
      const uint32_t pre = s_pre;
      for (long r = tid; r < NT; r += 256) {
        const float* row = train + r * F;
        const uint32_t u = __float_as_uint(sf_imp_chi2([&](int b) { return row[cols.bc[b]]; }, s_y, s_s, s_vm, B, dof));
        if (p == 0 || (u >> (shift + 8)) == pre) atomicAdd(&s_hist[(u >> shift) & 255u], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int kk = s_kk, d = 0;
        while (d < 255 && kk >= s_hist[d]) { kk -= s_hist[d]; ++d; }
        s_kk = kk;
        s_pre = (pre << 8) | (uint32_t)d;
      }
      __syncthreads();
    }
    const uint32_t P = s_pre;
    const int need_eq = s_kk + 1;   // rows equal to the k-th value that belong to the set, in row order
    if (tid == 0) s_eq_taken = 0;
    for (int c = 0; c < NCH; ++c) {
      int less = 0, eq = 0;
      for (int j = 0; j < SF_IMP_CH / 256; ++j) {
        const long r = (long)c * SF_IMP_CH + j * 256 + tid;
        if (r < NT) {
          const float* row = train + r * F;
          const uint32_t u = __float_as_uint(sf_imp_chi2([&](int b) { return row[cols.bc[b]]; }, s_y, s_s, s_vm, B, dof));
          less += u < P ? 1 : 0;
          eq += u == P ? 1 : 0;
        }
      }
      less = sf_block_sum(less, s_red);
      eq = sf_block_sum(eq, s_red);
      if (tid == 0) {
        const int left = need_eq - s_eq_taken;
        const int quota = eq < left ? eq : left;
        co[(long)c * LC + 0] = less + quota;
        co[(long)c * LC + 1] = quota;
        s_eq_taken += quota;
      }
    }
    __syncthreads();
    lvl = 0;
  }
  const bool ok = n >= min_nb;
  // exclusive scan of the chosen level's chunk counts
  {
    const int per = (NCH + 255) / 256;
    const int lo = tid * per, hi = lo + per < NCH ? lo + per : NCH;
    int s = 0;
    if (ok)
      for (int c = lo; c < hi; ++c) s += co[(long)c * LC + lvl];
    __syncthreads();
    s_red[tid] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int v = tid >= d ? s_red[tid - d] : 0;
      __syncthreads();
      s_red[tid] += v;
      __syncthreads();
    }
    int run = s_red[tid] - s;
    for (int c = lo; c < hi; ++c) {
      choff[(long)o * NCH + c] = run;
      if (ok) run += co[(long)c * LC + lvl];
    }
  }
  if (tid == 0) {
    lvlsel[o] = ok ? (fb ? -2 : lvl) : -1;   // -1: no list; -2: the fallback set (level slot 0 holds its counts)
    nsel[o] = ok ? n : 0;
    pbits[o] = fb ? s_pre : 0u;
    n_used[m] = ok ? n : (dof == 0.f ? -2 : -1);
    if (thr_used) thr_used[m] = lad.thr[fb ? L - 1 : lvl];
  }
}

// ---- 3. the lists, ascending training row ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_imp_compact(const float* __restrict__ train, long NT, int F, int B, SfImpCols cols,
                                                     const float* __restrict__ obs, const float* __restrict__ sigma,
                                                     const uint8_t* __restrict__ missing, long m0, int g0, SfImpLadder lad,
                                                     int NCH, int LC, const int32_t* __restrict__ cnt,
                                                     const int32_t* __restrict__ choff, const int32_t* __restrict__ lvlsel,
                                                     const uint32_t* __restrict__ pbits, const int32_t* __restrict__ goff,
                                                     int32_t* __restrict__ list) {
  __shared__ float s_y[SF_IMP_BMAX], s_s[SF_IMP_BMAX], s_dof;
  __shared__ uint32_t s_vm;
  __shared__ int s_w[4];
  const int o = g0 + blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int sel = lvlsel[o];
  if (sel == -1) return;
  const bool fb = sel == -2;
  const int lvl = fb ? 0 : sel;
  const int32_t* cc = cnt + ((long)o * NCH + c) * LC;
  const int nc = cc[lvl];
  if (nc == 0) return;
  const int quota = fb ? cc[1] : 0;
  const uint32_t P = pbits[o];
  const float thr = lad.thr[lvl];
  sf_imp_load_object(obs, sigma, missing, m0 + o, F, B, cols, s_y, s_s, &s_vm, &s_dof, tid);
  __syncthreads();
  const float dof = s_dof;
  int32_t* dst = list + goff[o] + choff[(long)o * NCH + c];
  int run = 0, eq_run = 0;
  for (int j = 0; j < SF_IMP_CH / 256; ++j) {
    const long rb = (long)c * SF_IMP_CH + j * 256;
    if (rb >= NT) break;
    const long r = rb + tid;
    bool adm = false, eq = false;
    if (r < NT) {
      const float* row = train + r * F;
      const float chi2 = sf_imp_chi2([&](int b) { return row[cols.bc[b]]; }, s_y, s_s, s_vm, B, dof);
      const uint32_t u = __float_as_uint(chi2);
      adm = fb ? u < P : chi2 <= thr;
      eq = fb && u == P;
    }
    int tot;
    if (fb) {   // (uniform over the workgroup) the first `quota` rows of the chunk that equal the k-th value
      const int er = sf_imp_rank(eq, s_w, &tot);
      if (eq && eq_run + er < quota) adm = true;
      eq_run += tot;
    }
    const int pos = run + sf_imp_rank(adm, s_w, &tot);
    if (adm && pos < nc) dst[pos] = (int32_t)r;
    run += tot;
  }
}

// ---- 4. weights, CDF, moments and draws: one workgroup per object --------------------------------------------------------
__global__ __launch_bounds__(256) void k_imp_draw(const float* __restrict__ train, int F, int B, SfImpCols cols, int has_err,
                                                  const float* __restrict__ obs, const uint8_t* __restrict__ missing, long m0,
                                                  int g0, long row_offset, float bw, int nmc, uint32_t k0, uint32_t k1,
                                                  const int32_t* __restrict__ nsel, const int32_t* __restrict__ goff,
                                                  const int32_t* __restrict__ list, double* __restrict__ wraw,
                                                  double* __restrict__ cdf, float* __restrict__ imputed, float* __restrict__ recon,
                                                  double* __restrict__ kde_var, int32_t* __restrict__ nbr_idx, long nbr_cap,
                                                  int32_t* __restrict__ draw_idx) {
  __shared__ double s_red[256];
  __shared__ float s_y[SF_IMP_BMAX], s_sd[SF_IMP_BMAX];
  __shared__ uint32_t s_mm;
  const int o = g0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long m = m0 + o;
  const int n = nsel[o];
  const float NaN = __builtin_nanf("");
  if (tid < B) s_y[tid] = obs[m * F + cols.bc[tid]];
  if (tid == 0) {
    uint32_t mm = 0;
    for (int b = 0; b < B; ++b) mm |= missing[m * B + b] ? 1u << b : 0u;
    s_mm = mm;
  }
  __syncthreads();
  const uint32_t mm = s_mm;
  float* imp = imputed + m * (long)nmc * F;
  if (n == 0) {   // a failed object: NaN outputs
    for (long e = tid; e < (long)nmc * F; e += 256) imp[e] = NaN;
    for (int b = tid; b < B; b += 256) {
      recon[m * B + b] = NaN;
      if (kde_var) kde_var[m * B + b] = (double)NaN;
    }
    if (draw_idx)
      for (long e = tid; e < (long)nmc * B; e += 256) draw_idx[m * (long)nmc * B + e] = -1;
    return;
  }
  const int32_t* lst = list + goff[o];
  double* w = wraw + goff[o];
  double* C = cdf + goff[o];
  // weights 1 / dist over the observed bands
  for (int j = tid; j < n; j += 256) {
    const float* row = train + (long)lst[j] * F;
    double d2 = 0.0;
    for (int b = 0; b < B; ++b)
      if (!((mm >> b) & 1u)) {
        const double d = (double)s_y[b] - (double)row[cols.bc[b]];
        d2 += d * d;
      }
    double dist = sqrt(d2);
    if (dist == 0.0) dist = 1e-10;
    w[j] = 1.0 / dist;
    if (nbr_idx && j < nbr_cap) nbr_idx[m * nbr_cap + j] = lst[j];
  }
  __syncthreads();
  // running sum: thread t owns a contiguous block
  const int per = (n + 255) / 256;
  const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  {
    double s = 0.0;
    for (int j = lo; j < hi; ++j) s += w[j];
    s_red[tid] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const double v = tid >= d ? s_red[tid - d] : 0.0;
      __syncthreads();
      s_red[tid] += v;
      __syncthreads();
    }
    double run = s_red[tid] - s;
    for (int j = lo; j < hi; ++j) { run += w[j]; C[j] = run; }
  }
  __syncthreads();
  const double W = C[n - 1];
  double v = 0.0;
  for (int j = tid; j < n; j += 256) { const double wn = w[j] / W; v += wn * wn; }
  const double sw2 = sf_block_sum(v, s_red);
  for (int b = 0; b < B; ++b) {
    if (!((mm >> b) & 1u)) continue;
    const int col = cols.bc[b];
    v = 0.0;
    for (int j = tid; j < n; j += 256) v += (w[j] / W) * (double)train[(long)lst[j] * F + col];
    const double mu = sf_block_sum(v, s_red);
    v = 0.0;
    for (int j = tid; j < n; j += 256) { const double d = (double)train[(long)lst[j] * F + col] - mu; v += (w[j] / W) * d * d; }
    const double var = (double)bw * (double)bw * sf_block_sum(v, s_red) / (1.0 - sw2);
    if (tid == 0) {
      s_sd[b] = (float)sqrt(var);
      if (kde_var) kde_var[m * B + b] = var;
    }
  }
  if (kde_var)
    for (int b = tid; b < B; b += 256)
      if (!((mm >> b) & 1u)) kde_var[m * B + b] = (double)NaN;
  __syncthreads();
  // the observed columns, copied; the columns of the missing bands (and their errors) are written by the draws
  unsigned long long repl = 0ull;
  for (int b = 0; b < B; ++b)
    if ((mm >> b) & 1u) {
      repl |= 1ull << cols.bc[b];
      if (has_err) repl |= 1ull << cols.ec[b];
    }
  for (long e = tid; e < (long)nmc * F; e += 256) {
    const int f = (int)(e % F);
    if (!((repl >> f) & 1ull)) imp[e] = obs[m * F + f];
  }
  const uint64_t grow = (uint64_t)(row_offset + m);
  for (long e = tid; e < (long)nmc * B; e += 256) {
    const int i = (int)(e / B), b = (int)(e % B);
    int32_t drawn = -1;
    if ((mm >> b) & 1u) {
      uint32_t r[4];
      sf_philox4x32_10((uint32_t)grow, (uint32_t)(grow >> 32), (uint32_t)i, (uint32_t)b, k0, k1, r);
      const double target = ((double)r[0] + 0.5) * 2.3283064365386963e-10 * W;   // 2^-32
      int a = 0, z = n - 1;   // the first j with C[j] > target (the last entry if none)
      while (a < z) {
        const int mid = (a + z) >> 1;
        if (C[mid] > target) z = mid; else a = mid + 1;
      }
      drawn = lst[a];
      const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(sf_u01(r[2])));
      const float zn = rad * __builtin_amdgcn_cosf(sf_u01(r[3]));
      const float* row = train + (long)drawn * F;
      imp[(long)i * F + cols.bc[b]] = __fadd_rn(row[cols.bc[b]], __fmul_rn(s_sd[b], zn));
      if (has_err) imp[(long)i * F + cols.ec[b]] = row[cols.ec[b]];
    }
    if (draw_idx) draw_idx[m * (long)nmc * B + e] = drawn;
  }
  __syncthreads();   // this workgroup's stores to `imputed` are visible to its own loads below
  for (int b = wave; b < B; b += 4) {
    float res = NaN;
    if ((mm >> b) & 1u) {
      double s = 0.0;
      for (int i = lane; i < nmc; i += 64) s += (double)imp[(long)i * F + cols.bc[b]];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
      res = (float)(s / (double)nmc);
    }
    if (lane == 0) recon[m * B + b] = res;
  }
}

// ---- scratch (sf_scratch.h): region 0 = counts, chunk offsets, per-object words; region 1 = lists, weights, running sums -
namespace {
SfScratch g_imp_scratch;
}  // namespace

extern "C" int sf_impute_missing(const float* train, int64_t NT, int32_t F, const int32_t* band_col, const int32_t* err_col,
                                 int32_t B, const float* obs, const float* sigma, const uint8_t* missing, int64_t M,
                                 int64_t row_offset, float ini_chi2, float chi2_step, float max_chi2, int32_t min_neighbours,
                                 int32_t fallback_k, float bw, int32_t nmc, uint64_t seed, float* imputed, float* recon,
                                 int32_t* n_used, float* thr_used, double* kde_var, int32_t* nbr_idx, int64_t nbr_cap,
                                 int32_t* draw_idx, void* stream) {
  if (!train || !band_col || !obs || !sigma || !missing || !imputed || !recon || !n_used) {
    sf_set_error("sf_impute_missing: null argument");
    return SF_ERR_INVALID;
  }
  if (B < 1 || B > SF_IMP_BMAX || F < B || F > SF_IMP_FMAX || NT < 1 || NT > 0x7fffffffll || M < 0 || nmc < 1 ||
      min_neighbours < 1 || fallback_k < 1 || (nbr_idx && nbr_cap < 1) || row_offset < 0) {
    sf_set_error("sf_impute_missing: need 1 <= B <= 32, B <= F <= 64, 1 <= NT < 2^31, M >= 0, nmc >= 1, min_neighbours >= 1, "
                 "fallback_k >= 1, nbr_cap >= 1 with nbr_idx, row_offset >= 0");
    return SF_ERR_INVALID;
  }
  if (!(chi2_step > 0.f) || !(ini_chi2 <= max_chi2) || !(bw > 0.f)) {
    sf_set_error("sf_impute_missing: need chi2_step > 0, ini_chi2 <= max_chi2, bw > 0");
    return SF_ERR_INVALID;
  }
  SfImpCols cols;
  for (int b = 0; b < SF_IMP_BMAX; ++b) {
    cols.bc[b] = b < B ? band_col[b] : 0;
    cols.ec[b] = (b < B && err_col) ? err_col[b] : 0;
    if (cols.bc[b] < 0 || cols.bc[b] >= F || cols.ec[b] < 0 || cols.ec[b] >= F) {
      sf_set_error("sf_impute_missing: a band or error column lies outside [0, F)");
      return SF_ERR_INVALID;
    }
  }
  SfImpLadder lad;
  lad.L = 0;
  for (float t = ini_chi2; t <= max_chi2; t += chi2_step) {
    if (lad.L == SF_IMP_LMAX) {
      sf_set_error("sf_impute_missing: more than 32 thresholds between ini_chi2 and max_chi2");
      return SF_ERR_INVALID;
    }
    lad.thr[lad.L++] = t;
  }
  for (int l = lad.L; l < SF_IMP_LMAX; ++l) lad.thr[l] = lad.thr[lad.L - 1];
  if ((int64_t)nmc * (F > B ? F : B) > 0x7fffffffll) {
    sf_set_error("sf_impute_missing: nmc * F must be below 2^31");
    return SF_ERR_INVALID;
  }
  if (M == 0) return SF_OK;
  hipStream_t st = (hipStream_t)stream;
  size_t budget = (size_t)256 << 20;
  if (const char* s = std::getenv("SF_IMPUTE_SCRATCH_BYTES")) {
    const long long v = std::atoll(s);
    if (v > 0) budget = (size_t)v;
  }
  const size_t budget_entries = budget / SF_IMP_ENTRY > 0 ? budget / SF_IMP_ENTRY : 1;
  const int NCH = (int)((NT + SF_IMP_CH - 1) / SF_IMP_CH);
  const int LC = lad.L > 2 ? lad.L : 2;
  // objects per batch: the (object, chunk, level) counts stay within 64 MiB
  int64_t MB = ((int64_t)64 << 20) / ((int64_t)NCH * LC * 4);
  MB = MB < 1 ? 1 : (MB > M ? M : MB);
  MB = MB > 65535ll * SF_IMP_OT ? 65535ll * SF_IMP_OT : MB;

  SfScratchCall ws(g_imp_scratch, "sf_impute_missing", st);
  const int sub_cnt = ws.add((size_t)MB * NCH * LC * 4), sub_choff = ws.add((size_t)MB * NCH * 4);
  const int sub_lvlsel = ws.add((size_t)MB * 4), sub_nsel = ws.add((size_t)MB * 4), sub_pbits = ws.add((size_t)MB * 4);
  const int sub_goff = ws.add((size_t)MB * 4);
  if (int rc = ws.reserve()) return rc;
  int32_t* cnt = ws.get<int32_t>(sub_cnt);
  int32_t* choff = ws.get<int32_t>(sub_choff);
  int32_t* lvlsel = ws.get<int32_t>(sub_lvlsel);
  int32_t* nsel = ws.get<int32_t>(sub_nsel);
  uint32_t* pbits = ws.get<uint32_t>(sub_pbits);
  int32_t* goff = ws.get<int32_t>(sub_goff);
  if (int rc = ws.check()) return rc;
  hipError_t e;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ 5u;
  std::vector<int32_t> h_nsel((size_t)MB);

  for (int64_t m0 = 0; m0 < M; m0 += MB) {
    const int Mb = (int)(M - m0 < MB ? M - m0 : MB);
    hipLaunchKernelGGL(k_imp_count, dim3((unsigned)NCH, (unsigned)((Mb + SF_IMP_OT - 1) / SF_IMP_OT)), dim3(256),
                       (size_t)B * 256 * sizeof(float), st, train, (long)NT, (int)F, (int)B, cols, obs, sigma, missing, (long)m0, Mb,
                       lad, NCH, LC, cnt);
    hipLaunchKernelGGL(k_imp_decide, dim3((unsigned)Mb), dim3(256), 0, st, train, (long)NT, (int)F, (int)B, cols, obs, sigma,
                       missing, (long)m0, lad, NCH, LC, (int)min_neighbours, (int)fallback_k, cnt, choff, lvlsel, nsel, pbits,
                       n_used, thr_used);
    if ((e = hipGetLastError()) != hipSuccess) return ws.fail("launch", e);
    if ((e = hipMemcpyAsync(h_nsel.data(), nsel, (size_t)Mb * 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return ws.fail("hipMemcpyAsync", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return ws.fail("hipStreamSynchronize", e);
    int g0 = 0;
    while (g0 < Mb) {
      // a group: consecutive objects whose lists fit the budget (one object on its own may exceed it)
      size_t entries = (size_t)h_nsel[g0];
      int g1 = g0 + 1;
      while (g1 < Mb && g1 - g0 < 65535 && entries + (size_t)h_nsel[g1] <= budget_entries) entries += (size_t)h_nsel[g1++];
      const size_t cap_e = entries > 0 ? entries : 1;
      ws.clear(1);
      const int sub_list = ws.add(cap_e * 4, 1), sub_wraw = ws.add(cap_e * 8, 1), sub_cdf = ws.add(cap_e * 8, 1);
      if (int rc = ws.reserve(1)) return rc;
      int32_t* list = ws.get<int32_t>(sub_list);
      double* wraw = ws.get<double>(sub_wraw);
      double* cdf = ws.get<double>(sub_cdf);
      if (int rc = ws.check()) return rc;
      const int ng = g1 - g0;
      // (no total: goff + g0 has no spare element behind a group)
      if ((e = sf_launch_exclusive_scan_i32(nsel + g0, ng, goff + g0, nullptr, st)) != hipSuccess) return ws.fail("launch", e);
      if (entries > 0)
        hipLaunchKernelGGL(k_imp_compact, dim3((unsigned)NCH, (unsigned)ng), dim3(256), 0, st, train, (long)NT, (int)F, (int)B, cols,
                           obs, sigma, missing, (long)m0, g0, lad, NCH, LC, cnt, choff, lvlsel, pbits, goff, list);
      hipLaunchKernelGGL(k_imp_draw, dim3((unsigned)ng), dim3(256), 0, st, train, (int)F, (int)B, cols, err_col ? 1 : 0, obs, missing,
                         (long)m0, g0, (long)row_offset, bw, (int)nmc, k0, k1, nsel, goff, list, wraw, cdf, imputed, recon, kde_var,
                         nbr_idx, (long)nbr_cap, draw_idx);
      if ((e = hipGetLastError()) != hipSuccess) return ws.fail("launch", e);
      g0 = g1;
    }
  }
  return ws.finish();
}
