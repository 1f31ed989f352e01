// sf_lc2st.hip -- the classifiers of the L-C2ST local calibration test (Linhart et al. 2023): many
// independent copies of sklearn's MLPClassifier (two ReLU layers of W units, logistic output, Adam, L2 term, minibatches of
// 200, early stopping on a held-out validation accuracy) over ONE shared row matrix, each with its own labels and split.
//
// k_c2st_train: one 256-thread workgroup per classifier, its weights in LDS for the whole launch.  A minibatch is walked in
// sub-chunks of 32 rows.  Every matrix product is v_mfma_f32_16x16x4_f32 with the OUTPUT columns split over the four waves
// (wave w owns the 16-wide column tiles w and w + 4), so activations cross waves through two 32-row LDS stages and the
// weight-gradient tiles of a wave stay in its registers for the whole minibatch: nothing is reduced across waves, nothing is
// atomic, and the sum over the rows of a minibatch runs in one fixed order -- the same seed gives the same bits.
// k_c2st_scores: the forward half over the rows of an observation, p = 1 - sigmoid(logit) and mean((p - 0.5)^2).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sf_buf.h"
#include "sf_internal.h"
#include "sf_rng.h"
#include "synference_hip.h"

#define SF_C2ST_RB 32          // rows of a sub-chunk (two 16-row MFMA tiles)
#define SF_C2ST_NSTATE 8       // int32 state words per classifier
#define SF_C2ST_STREAM_ORDER 0x4C433200u

typedef float c2st_f4 __attribute__((ext_vector_type(4)));

struct SfC2stDims {
  int n_in, W, WP, NT, K4, K16, WS, SS;
  int o_b1, o_w2, o_b2, o_w3, o_b3, NP;   // the dense (sklearn) parameter vector: W1[n_in][W] b1 W2[W][W] b2 w3[W] b3
  long R;
  int n_cls, max_iter, n_iter_no_change, early_stopping, batch;
  uint32_t k0, k1;
  float lr, beta1, beta2, eps, alpha;
  double tol;
};

struct SfC2stTrainArgs {
  const float* rows;         // [R][n_in]
  const uint8_t* labels;     // [n_cls][R]
  const int32_t* idx;        // [n_cls][R]: training rows ascending, then validation rows ascending
  float *wcur, *wbest, *am, *av, *gimg;   // [n_cls][NP]
  int32_t* state;            // [n_cls][SF_C2ST_NSTATE]: epoch, adam step, no-improvement count, best_iter, done, n_train, n_val, best count
  int32_t* slog;             // [n_cls][max_iter]: correct validation rows after each epoch
  int first, epochs, finish;
};

struct SfC2stLds {
  float *w1, *w2, *b1, *b2, *w3, *b3, *As, *Bs, *zl, *dl;
  int *ridx, *yv, *misc;
};

__host__ __device__ inline size_t c2st_lds_floats(const SfC2stDims& d) {
  return (size_t)d.K16 * d.WS + (size_t)d.WP * d.WS + 3 * (size_t)d.WP + 4 + 2 * (size_t)SF_C2ST_RB * d.SS + 4 * SF_C2ST_RB + 16;
}

__device__ __forceinline__ SfC2stLds c2st_carve(float* p, const SfC2stDims& d) {
  SfC2stLds l;
  l.w1 = p; p += (size_t)d.K16 * d.WS;
  l.w2 = p; p += (size_t)d.WP * d.WS;
  l.b1 = p; p += d.WP;
  l.b2 = p; p += d.WP;
  l.w3 = p; p += d.WP;
  l.b3 = p; p += 4;
  l.As = p; p += SF_C2ST_RB * d.SS;
  l.Bs = p; p += SF_C2ST_RB * d.SS;
  l.zl = p; p += SF_C2ST_RB;
  l.dl = p; p += SF_C2ST_RB;
  l.ridx = reinterpret_cast<int*>(p); p += SF_C2ST_RB;
  l.yv = reinterpret_cast<int*>(p); p += SF_C2ST_RB;
  l.misc = reinterpret_cast<int*>(p);
  return l;
}

// dense vector -> LDS image (padding zero).  Ends with a barrier.
__device__ void c2st_load(const SfC2stLds& l, const SfC2stDims& d, const float* __restrict__ w) {
  const int tid = threadIdx.x;
  const int nz = d.K16 * d.WS + d.WP * d.WS + 3 * d.WP + 4;
  for (int i = tid; i < nz; i += 256) l.w1[i] = 0.f;
  __syncthreads();
  for (int i = tid; i < d.n_in * d.W; i += 256) l.w1[(i / d.W) * d.WS + i % d.W] = w[i];
  for (int i = tid; i < d.W * d.W; i += 256) l.w2[(i / d.W) * d.WS + i % d.W] = w[d.o_w2 + i];
  for (int i = tid; i < d.W; i += 256) {
    l.b1[i] = w[d.o_b1 + i];
    l.b2[i] = w[d.o_b2 + i];
    l.w3[i] = w[d.o_w3 + i];
  }
  if (tid == 0) l.b3[0] = w[d.o_b3];
  __syncthreads();
}

__device__ void c2st_store(const SfC2stLds& l, const SfC2stDims& d, float* __restrict__ w) {
  const int tid = threadIdx.x;
  for (int i = tid; i < d.n_in * d.W; i += 256) w[i] = l.w1[(i / d.W) * d.WS + i % d.W];
  for (int i = tid; i < d.W * d.W; i += 256) w[d.o_w2 + i] = l.w2[(i / d.W) * d.WS + i % d.W];
  for (int i = tid; i < d.W; i += 256) {
    w[d.o_b1 + i] = l.b1[i];
    w[d.o_b2 + i] = l.b2[i];
    w[d.o_w3 + i] = l.w3[i];
  }
  if (tid == 0) w[d.o_b3] = l.b3[0];
}

// The 32 rows named by l.ridx (-1: no row) through both hidden layers: relu(z1) in As, relu(z2) in Bs, the logit in zl.
// Called by all 256 threads after a barrier that published ridx; ends with a barrier.
template <int OT>
__device__ void c2st_forward(const SfC2stLds& l, const SfC2stDims& d, const float* __restrict__ rows) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    c2st_f4 acc[OT];
#pragma unroll
    for (int oi = 0; oi < OT; ++oi) {
      const int ot = wave + 4 * oi;
      const float b = ot < d.NT ? l.b1[16 * ot + c] : 0.f;
      acc[oi] = {b, b, b, b};
    }
    const int r = l.ridx[mt * 16 + c];
    const float* xr = rows + (long)(r < 0 ? 0 : r) * d.n_in;
#pragma unroll 1
    for (int kb = 0; kb * 4 < d.K4; ++kb) {
      const int k = 4 * kb + g;
      const float a = (r >= 0 && k < d.n_in) ? xr[k] : 0.f;
#pragma unroll
      for (int oi = 0; oi < OT; ++oi) {
        const int ot = wave + 4 * oi;
        if (ot < d.NT) acc[oi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, l.w1[k * d.WS + 16 * ot + c], acc[oi], 0, 0, 0);
      }
    }
#pragma unroll
    for (int oi = 0; oi < OT; ++oi) {
      const int ot = wave + 4 * oi;
      if (ot < d.NT)
#pragma unroll
        for (int i = 0; i < 4; ++i) l.As[(mt * 16 + 4 * g + i) * d.SS + 16 * ot + c] = fmaxf(acc[oi][i], 0.f);
    }
  }
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    c2st_f4 acc[OT];
#pragma unroll
    for (int oi = 0; oi < OT; ++oi) {
      const int ot = wave + 4 * oi;
      const float b = ot < d.NT ? l.b2[16 * ot + c] : 0.f;
      acc[oi] = {b, b, b, b};
    }
#pragma unroll 1
    for (int kb = 0; kb * 4 < d.WP; ++kb) {
      const int k = 4 * kb + g;
      const float a = l.As[(mt * 16 + c) * d.SS + k];
#pragma unroll
      for (int oi = 0; oi < OT; ++oi) {
        const int ot = wave + 4 * oi;
        if (ot < d.NT) acc[oi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, l.w2[k * d.WS + 16 * ot + c], acc[oi], 0, 0, 0);
      }
    }
#pragma unroll
    for (int oi = 0; oi < OT; ++oi) {
      const int ot = wave + 4 * oi;
      if (ot < d.NT)
#pragma unroll
        for (int i = 0; i < 4; ++i) l.Bs[(mt * 16 + 4 * g + i) * d.SS + 16 * ot + c] = fmaxf(acc[oi][i], 0.f);
    }
  }
  __syncthreads();
  {  // the logit: eight threads per row, each over WP / 8 consecutive units, then a fixed tree over the eight
    const int row = tid >> 3, part = tid & 7, n = d.WP >> 3;
    float s = 0.f;
    for (int j = 0; j < n; ++j) s = fmaf(l.Bs[row * d.SS + part * n + j], l.w3[part * n + j], s);
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    if (part == 0) l.zl[row] = s + l.b3[0];
  }
  __syncthreads();
}

__device__ __forceinline__ uint32_t c2st_mix(uint32_t u) {
  u ^= u >> 16; u *= 0x7feb352du;
  u ^= u >> 15; u *= 0x846ca68bu;
  u ^= u >> 16;
  return u;
}
// position j of the epoch -> an index in [0, n): four Feistel rounds over 2 * hb bits, walked until the value is inside
__device__ __forceinline__ uint32_t c2st_order(uint32_t j, uint32_t n, int hb, const uint32_t (&key)[4]) {
  const uint32_t mask = (1u << hb) - 1u;
  uint32_t x = j;
  do {
    uint32_t L = x >> hb, Rr = x & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t F = c2st_mix(Rr ^ key[r]) & mask;
      const uint32_t t = L ^ F;
      L = Rr;
      Rr = t;
    }
    x = (L << hb) | Rr;
  } while (x >= n);
  return x;
}

__device__ __forceinline__ float c2st_adam(float w, float gr, float* __restrict__ m, float* __restrict__ v, int e, float lr_t,
                                           const SfC2stDims& d) {
  const float mn = d.beta1 * m[e] + (1.f - d.beta1) * gr;
  const float vn = d.beta2 * v[e] + (1.f - d.beta2) * gr * gr;
  m[e] = mn;
  v[e] = vn;
  return w + (-lr_t * mn / (sqrtf(vn) + d.eps));
}

// OT: column tiles per wave (1: W <= 64, 2: W <= 128)
template <int OT>
__global__ __launch_bounds__(256) void k_c2st_train(SfC2stDims d, SfC2stTrainArgs a) {
  extern __shared__ float c2st_lds[];
  const SfC2stLds l = c2st_carve(c2st_lds, d);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int clf = a.first + blockIdx.x;
  int32_t* st = a.state + (long)clf * SF_C2ST_NSTATE;
  if (st[4] != 0) return;   // done in an earlier launch (uniform: nothing in this block has written the state yet)
  int epoch = st[0], step = st[1], no_imp = st[2], best_iter = st[3];
  const int n_train = st[5], n_val = st[6];
  int best_cnt = st[7];
  const long cR = (long)clf * d.R;
  const uint8_t* lab = a.labels + cR;
  const int32_t* idx = a.idx + cR;
  float* wcur = a.wcur + (long)clf * d.NP;
  float* wbest = a.wbest + (long)clf * d.NP;
  float* am = a.am + (long)clf * d.NP;
  float* av = a.av + (long)clf * d.NP;
  float* gimg = a.gimg + (long)clf * d.NP;
  c2st_load(l, d, wcur);
  int hb = 1;
  while ((1L << (2 * hb)) < (long)n_train) ++hb;
  int done = (a.finish || epoch >= d.max_iter) ? 1 : 0;

  for (int el = 0; el < a.epochs && !done; ++el) {
    uint32_t key[4];
    sf_philox4x32_10((uint32_t)clf, (uint32_t)epoch, 0u, 0u, d.k0, d.k1 ^ SF_C2ST_STREAM_ORDER, key);
    for (int mb0 = 0; mb0 < n_train; mb0 += d.batch) {
      const int bs = min(d.batch, n_train - mb0);
      const float inv_bs = 1.f / (float)bs;
      c2st_f4 g1[5][OT], g2[4 * OT][OT];
#pragma unroll
      for (int t = 0; t < 4 * OT; ++t)
#pragma unroll
        for (int oi = 0; oi < OT; ++oi) g2[t][oi] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int oi = 0; oi < OT; ++oi) g1[t][oi] = {0.f, 0.f, 0.f, 0.f};
      float gb1 = 0.f, gb2 = 0.f, gw3 = 0.f, gb3 = 0.f;
      for (int sc0 = 0; sc0 < bs; sc0 += SF_C2ST_RB) {
        if (tid < SF_C2ST_RB) {
          const int j = sc0 + tid;
          int r = -1, y = 0;
          if (j < bs) {
            r = idx[c2st_order((uint32_t)(mb0 + j), (uint32_t)n_train, hb, key)];
            y = lab[r];
          }
          l.ridx[tid] = r;
          l.yv[tid] = y;
        }
        __syncthreads();
        c2st_forward<OT>(l, d, a.rows);
        if (tid < SF_C2ST_RB) {
          const float p = 1.f / (1.f + expf(-l.zl[tid]));
          l.dl[tid] = l.ridx[tid] >= 0 ? (p - (float)l.yv[tid]) * inv_bs : 0.f;
        }
        __syncthreads();
        // column pass over the 32 rows: w3 and b2 gradients, and Bs becomes dL/dz2
        if (tid < d.WP) {
          const float w3 = l.w3[tid];
          for (int m = 0; m < SF_C2ST_RB; ++m) {
            const float h = l.Bs[m * d.SS + tid], dm = l.dl[m];
            gw3 = fmaf(h, dm, gw3);
            const float dz = h > 0.f ? w3 * dm : 0.f;
            gb2 += dz;
            l.Bs[m * d.SS + tid] = dz;
          }
        }
        if (tid == 0)
          for (int m = 0; m < SF_C2ST_RB; ++m) gb3 += l.dl[m];
        __syncthreads();
        // dL/dW2[kin][out] += sum_m h1[m][kin] dz2[m][out]
#pragma unroll 1
        for (int ks = 0; ks < SF_C2ST_RB / 4; ++ks) {
          const int m = 4 * ks + g;
          float bv[OT];
#pragma unroll
          for (int oi = 0; oi < OT; ++oi) bv[oi] = (wave + 4 * oi) < d.NT ? l.Bs[m * d.SS + 16 * (wave + 4 * oi) + c] : 0.f;
#pragma unroll
          for (int t = 0; t < 4 * OT; ++t)
            if (t < d.NT) {
              const float av_ = l.As[m * d.SS + 16 * t + c];
#pragma unroll
              for (int oi = 0; oi < OT; ++oi)
                if (wave + 4 * oi < d.NT) g2[t][oi] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_, bv[oi], g2[t][oi], 0, 0, 0);
            }
        }
        // dL/dh1[m][kin] = sum_out dz2[m][out] W2[kin][out], this wave's kin tiles
        c2st_f4 d1[2][OT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int oi = 0; oi < OT; ++oi) {
            d1[mt][oi] = {0.f, 0.f, 0.f, 0.f};
            const int ot = wave + 4 * oi;
            if (ot < d.NT)
#pragma unroll 1
              for (int kb = 0; kb * 4 < d.WP; ++kb) {
                const int k = 4 * kb + g;
                d1[mt][oi] = __builtin_amdgcn_mfma_f32_16x16x4f32(l.Bs[(mt * 16 + c) * d.SS + k], l.w2[(16 * ot + c) * d.WS + k],
                                                                 d1[mt][oi], 0, 0, 0);
              }
          }
        __syncthreads();   // every wave has read h1 for its W2 gradient
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int oi = 0; oi < OT; ++oi) {
            const int ot = wave + 4 * oi;
            if (ot < d.NT)
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                float* p = &l.As[(mt * 16 + 4 * g + i) * d.SS + 16 * ot + c];
                *p = *p > 0.f ? d1[mt][oi][i] : 0.f;
              }
          }
        __syncthreads();
        if (tid < d.WP)
          for (int m = 0; m < SF_C2ST_RB; ++m) gb1 += l.As[m * d.SS + tid];
        // dL/dW1[kin][out] += sum_m x[m][kin] dz1[m][out]
#pragma unroll 1
        for (int ks = 0; ks < SF_C2ST_RB / 4; ++ks) {
          const int m = 4 * ks + g;
          const int r = l.ridx[m];
          const float* xr = a.rows + (long)(r < 0 ? 0 : r) * d.n_in;
          float bv[OT];
#pragma unroll
          for (int oi = 0; oi < OT; ++oi) bv[oi] = (wave + 4 * oi) < d.NT ? l.As[m * d.SS + 16 * (wave + 4 * oi) + c] : 0.f;
#pragma unroll
          for (int t = 0; t < 5; ++t)
            if (16 * t < d.n_in) {
              const int kin = 16 * t + c;
              const float xv = (r >= 0 && kin < d.n_in) ? xr[kin] : 0.f;
#pragma unroll
              for (int oi = 0; oi < OT; ++oi)
                if (wave + 4 * oi < d.NT) g1[t][oi] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv, bv[oi], g1[t][oi], 0, 0, 0);
            }
        }
        __syncthreads();   // the stages and ridx are free again
      }
      // ---- one Adam step (sklearn's AdamOptimizer: the step size carries both bias corrections) ----
      ++step;
      const float lr_t = (float)((double)d.lr * sqrt(1.0 - pow((double)d.beta2, (double)step)) / (1.0 - pow((double)d.beta1, (double)step)));
      const float l2 = d.alpha * inv_bs;
      // the gradient tiles leave the registers for the classifier's gradient image (dense layout; L2), so that the update is
      // one flat loop: 104 tiles of read-modify-write chains unrolled in place cost more registers than the kernel has
#pragma unroll
      for (int oi = 0; oi < OT; ++oi) {
        const int out = 16 * (wave + 4 * oi) + c;
        if (out < d.W) {
#pragma unroll
          for (int t = 0; t < 4 * OT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int kin = 16 * t + 4 * g + i;
              if (kin < d.W) gimg[d.o_w2 + kin * d.W + out] = g2[t][oi][i];
            }
#pragma unroll
          for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int kin = 16 * t + 4 * g + i;
              if (kin < d.n_in) gimg[kin * d.W + out] = g1[t][oi][i];
            }
        }
      }
      __syncthreads();
#pragma unroll 1
      for (int e = tid; e < d.o_b1; e += 256) {
        float* w = &l.w1[(e / d.W) * d.WS + e % d.W];
        *w = c2st_adam(*w, gimg[e] + l2 * *w, am, av, e, lr_t, d);
      }
#pragma unroll 1
      for (int i = tid; i < d.W * d.W; i += 256) {
        float* w = &l.w2[(i / d.W) * d.WS + i % d.W];
        *w = c2st_adam(*w, gimg[d.o_w2 + i] + l2 * *w, am, av, d.o_w2 + i, lr_t, d);
      }
      if (tid < d.W) {
        l.b1[tid] = c2st_adam(l.b1[tid], gb1, am, av, d.o_b1 + tid, lr_t, d);
        l.b2[tid] = c2st_adam(l.b2[tid], gb2, am, av, d.o_b2 + tid, lr_t, d);
        l.w3[tid] = c2st_adam(l.w3[tid], gw3 + l2 * l.w3[tid], am, av, d.o_w3 + tid, lr_t, d);
      }
      if (tid == 0) l.b3[0] = c2st_adam(l.b3[0], gb3, am, av, d.o_b3, lr_t, d);
      __syncthreads();
    }
    ++epoch;
    // ---- validation accuracy ----
    int cnt = 0;
    for (int v0 = 0; v0 < n_val; v0 += SF_C2ST_RB) {
      if (tid < SF_C2ST_RB) {
        const int j = v0 + tid;
        const int r = j < n_val ? idx[n_train + j] : -1;
        l.ridx[tid] = r;
        l.yv[tid] = r >= 0 ? lab[r] : 0;
      }
      __syncthreads();
      c2st_forward<OT>(l, d, a.rows);
      if (tid == 0)
        for (int m = 0; m < SF_C2ST_RB; ++m)
          if (l.ridx[m] >= 0 && (l.zl[m] > 0.f ? 1 : 0) == l.yv[m]) ++cnt;
      __syncthreads();
    }
    // ---- sklearn's _update_no_improvement_count on the validation score, then the stop test ----
    if (tid == 0) {
      int snap = 0;
      a.slog[(long)clf * d.max_iter + (epoch - 1)] = cnt;
      if (d.early_stopping && n_val > 0) {
        const double score = (double)cnt / (double)n_val;
        const double best = best_cnt < 0 ? -INFINITY : (double)best_cnt / (double)n_val;
        if (score < best + d.tol) ++no_imp; else no_imp = 0;
        if (score > best) { best_cnt = cnt; best_iter = epoch; snap = 1; }
        if (no_imp > d.n_iter_no_change) done = 1;
      } else {
        best_iter = epoch;
      }
      if (epoch >= d.max_iter) done = 1;
      l.misc[0] = snap; l.misc[1] = done; l.misc[2] = no_imp; l.misc[3] = best_iter; l.misc[4] = best_cnt;
    }
    __syncthreads();
    const int snap = l.misc[0];
    done = l.misc[1]; no_imp = l.misc[2]; best_iter = l.misc[3]; best_cnt = l.misc[4];
    __syncthreads();
    if (snap) c2st_store(l, d, wbest);
  }
  if (done && d.early_stopping && best_cnt >= 0) {
    __syncthreads();
    c2st_load(l, d, wbest);   // (this block's own global writes, after a barrier)
  }
  c2st_store(l, d, wcur);
  if (tid == 0) {
    st[0] = epoch; st[1] = step; st[2] = no_imp; st[3] = best_iter; st[4] = done; st[7] = best_cnt;
  }
}

// idx[clf]: the rows with vmask 0 ascending, then the rows with vmask 1 ascending; state initialised
__global__ __launch_bounds__(256) void k_c2st_prep(const uint8_t* __restrict__ vmask, int32_t* __restrict__ idx,
                                                   int32_t* __restrict__ state, long R) {
  __shared__ int cnt[256];
  __shared__ int off[257];
  const int tid = threadIdx.x, clf = blockIdx.x;
  const uint8_t* vm = vmask + (long)clf * R;
  int32_t* ix = idx + (long)clf * R;
  const long per = (R + 255) / 256, lo = tid * per < R ? tid * per : R, hi = lo + per < R ? lo + per : R;
  int n = 0;
  for (long r = lo; r < hi; ++r) n += vm[r] == 0;
  cnt[tid] = n;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int i = 0; i < 256; ++i) { off[i] = s; s += cnt[i]; }
    off[256] = s;
  }
  __syncthreads();
  const int n_train = off[256];
  long t = off[tid], v = n_train + (lo - off[tid]);
  for (long r = lo; r < hi; ++r) {
    if (vm[r] == 0) ix[t++] = (int32_t)r;
    else ix[v++] = (int32_t)r;
  }
  if (tid == 0) {
    int32_t* st = state + (long)clf * SF_C2ST_NSTATE;
    st[0] = st[1] = st[2] = st[3] = st[4] = 0;
    st[5] = n_train;
    st[6] = (int32_t)(R - n_train);
    st[7] = -1;
  }
}

struct SfC2stScoreArgs {
  const float* rows;    // [S][n_in]: z-scored (theta_o, x_o)
  const float* wcur;
  long S;
  double* stats;        // [count]
  float* probs;         // [count][S] or null
  int first;
};

template <int OT>
__global__ __launch_bounds__(256) void k_c2st_scores(SfC2stDims d, SfC2stScoreArgs a) {
  extern __shared__ float c2st_lds[];
  const SfC2stLds l = c2st_carve(c2st_lds, d);
  const int tid = threadIdx.x;
  const int clf = a.first + blockIdx.x;
  c2st_load(l, d, a.wcur + (long)clf * d.NP);
  double acc = 0.0;
  for (long s0 = 0; s0 < a.S; s0 += SF_C2ST_RB) {
    if (tid < SF_C2ST_RB) l.ridx[tid] = s0 + tid < a.S ? (int)(s0 + tid) : -1;
    __syncthreads();
    c2st_forward<OT>(l, d, a.rows);
    if (tid < SF_C2ST_RB && l.ridx[tid] >= 0) {
      const float p = 1.f - 1.f / (1.f + expf(-l.zl[tid]));
      if (a.probs) a.probs[(long)blockIdx.x * a.S + s0 + tid] = p;
      l.dl[tid] = p;
    }
    __syncthreads();
    if (tid == 0)
      for (int m = 0; m < SF_C2ST_RB && s0 + m < a.S; ++m) {
        const double q = (double)l.dl[m] - 0.5;
        acc += q * q;
      }
    __syncthreads();
  }
  if (tid == 0) a.stats[blockIdx.x] = a.S > 0 ? acc / (double)a.S : 0.0;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct SfC2stBufs {   // built once, all or nothing (sf_c2st_create)
  SfBuf<int32_t> d_idx, d_state, d_slog;
  SfBuf<float> d_wcur, d_wbest, d_m, d_v, d_g;
};
struct sf_c2st : SfC2stBufs {
  SfC2stDims dims;
  const float* rows = nullptr;
  const uint8_t* labels = nullptr;
  size_t shmem = 0;
};

namespace {
void c2st_fill_dims(SfC2stDims& d, int n_in, int W) {
  d.n_in = n_in; d.W = W;
  d.WP = (W + 15) / 16 * 16; d.NT = d.WP / 16;
  d.K4 = (n_in + 3) / 4 * 4; d.K16 = (n_in + 15) / 16 * 16;
  d.WS = d.WP + 4; d.SS = d.WP + 2;   // strides of the weight images and of the stages (the bank count)
  d.o_b1 = n_in * W; d.o_w2 = d.o_b1 + W; d.o_b2 = d.o_w2 + W * W; d.o_w3 = d.o_b2 + W; d.o_b3 = d.o_w3 + W;
  d.NP = d.o_b3 + 1;
}
// the attribute is set once per device, for the largest classifier the entry points admit (about 142 KiB of the 160)
int c2st_set_lds(const void* fn, SfAttrCache& attr) {
  int dev;
  if (attr.need(dev)) {
    SfC2stDims worst{};
    c2st_fill_dims(worst, SF_C2ST_MAX_IN, SF_C2ST_MAX_W);
    SF_TRY_SET(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(c2st_lds_floats(worst) * sizeof(float))));
    attr.set(dev);
  }
  return SF_OK;
}
}  // namespace

extern "C" {
int sf_c2st_create(const sf_c2st_desc* p, sf_c2st** out, void* stream) {
  if (!p || !out) return sf_fail(SF_ERR_INVALID, "sf_c2st_create: null argument");
  if (p->n_in < 1 || p->n_in > SF_C2ST_MAX_IN)
    return sf_fail(SF_ERR_INVALID, "sf_c2st_create: n_in must be 1 .. " + std::to_string(SF_C2ST_MAX_IN));
  if (p->width < 1 || p->width > SF_C2ST_MAX_W)
    return sf_fail(SF_ERR_INVALID, "sf_c2st_create: hidden width must be 1 .. " + std::to_string(SF_C2ST_MAX_W));
  if (p->R < 1 || p->R >= (1LL << 31) || p->n_cls < 1 || p->max_iter < 1 || p->n_iter_no_change < 0 || p->batch < 1 ||
      (int64_t)p->n_cls * p->max_iter >= (1LL << 31))
    return sf_fail(SF_ERR_INVALID, "sf_c2st_create: need 1 <= R < 2^31, n_cls >= 1, max_iter >= 1, n_iter_no_change >= 0, batch >= 1");
  if (!p->rows || !p->labels || !p->vmask || !p->init_weights) return sf_fail(SF_ERR_INVALID, "sf_c2st_create: null device array");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return sf_fail(SF_ERR_NO_DEVICE, "no HIP device visible: the L-C2ST classifiers have no CPU fallback");
  sf_c2st* h = new sf_c2st();
  SfC2stDims& d = h->dims;
  c2st_fill_dims(d, p->n_in, p->width);
  d.R = p->R; d.n_cls = p->n_cls; d.max_iter = p->max_iter; d.n_iter_no_change = p->n_iter_no_change;
  d.early_stopping = p->early_stopping ? 1 : 0; d.batch = p->batch;
  d.k0 = (uint32_t)p->seed; d.k1 = (uint32_t)(p->seed >> 32);
  d.lr = p->lr; d.beta1 = p->beta1; d.beta2 = p->beta2; d.eps = p->eps; d.alpha = p->alpha; d.tol = p->tol;
  h->rows = p->rows; h->labels = p->labels;
  h->shmem = c2st_lds_floats(d) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  const size_t nw = (size_t)d.n_cls * d.NP;
  SfC2stBufs b;
#define C2ST_TRY(call)                                                                        \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) { delete h; return sf_fail(SF_ERR_HIP, sf_hip_message(#call, e_)); } \
  } while (0)
  C2ST_TRY(b.d_idx.alloc((size_t)d.n_cls * d.R));
  C2ST_TRY(b.d_state.alloc((size_t)d.n_cls * SF_C2ST_NSTATE));
  C2ST_TRY(b.d_slog.alloc((size_t)d.n_cls * d.max_iter));
  C2ST_TRY(b.d_wcur.alloc(nw));
  C2ST_TRY(b.d_wbest.alloc(nw));
  C2ST_TRY(b.d_m.alloc(nw));
  C2ST_TRY(b.d_v.alloc(nw));
  C2ST_TRY(b.d_g.alloc(nw));
  C2ST_TRY(hipMemcpyAsync(b.d_wcur, p->init_weights, nw * sizeof(float), hipMemcpyDeviceToDevice, st));
  C2ST_TRY(hipMemsetAsync(b.d_m, 0, nw * sizeof(float), st));
  C2ST_TRY(hipMemsetAsync(b.d_v, 0, nw * sizeof(float), st));
  C2ST_TRY(hipMemsetAsync(b.d_slog, 0xff, (size_t)d.n_cls * d.max_iter * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_c2st_prep, dim3((unsigned)d.n_cls), dim3(256), 0, st, p->vmask, b.d_idx.get(), b.d_state.get(), d.R);
  C2ST_TRY(hipGetLastError());
  C2ST_TRY(hipStreamSynchronize(st));   // vmask and init_weights may go once the call returns
#undef C2ST_TRY
  static_cast<SfC2stBufs&>(*h) = std::move(b);
  *out = h;
  return SF_OK;
}

void sf_c2st_destroy(sf_c2st* h) { delete h; }

int64_t sf_c2st_num_params(const sf_c2st* h) { return h ? h->dims.NP : 0; }

int sf_c2st_train(sf_c2st* h, int32_t first, int32_t count, int32_t epochs, int32_t finish, int32_t* n_active, void* stream) {
  if (!h) return sf_fail(SF_ERR_INVALID, "sf_c2st_train: null handle");
  const SfC2stDims& d = h->dims;
  if (first < 0 || count < 1 || first + count > d.n_cls || epochs < 0)
    return sf_fail(SF_ERR_INVALID, "sf_c2st_train: classifier range or epoch count out of range");
  hipStream_t st = (hipStream_t)stream;
  static SfAttrCache attr;
  static SfAttrCache attr2;
  const bool wide = d.NT > 4;
  if (int rc = wide ? c2st_set_lds((const void*)k_c2st_train<2>, attr2) : c2st_set_lds((const void*)k_c2st_train<1>, attr)) return rc;
  SfC2stTrainArgs a{};
  a.rows = h->rows; a.labels = h->labels; a.idx = h->d_idx;
  a.wcur = h->d_wcur; a.wbest = h->d_wbest; a.am = h->d_m; a.av = h->d_v; a.gimg = h->d_g;
  a.state = h->d_state; a.slog = h->d_slog;
  a.first = first; a.epochs = epochs; a.finish = finish ? 1 : 0;
  if (wide) hipLaunchKernelGGL(k_c2st_train<2>, dim3((unsigned)count), dim3(256), h->shmem, st, d, a);
  else hipLaunchKernelGGL(k_c2st_train<1>, dim3((unsigned)count), dim3(256), h->shmem, st, d, a);
  SF_TRY_SET(hipGetLastError());
  std::vector<int32_t> s((size_t)count * SF_C2ST_NSTATE);
  SF_TRY_SET(hipMemcpyAsync(s.data(), h->d_state.get() + (size_t)first * SF_C2ST_NSTATE, s.size() * sizeof(int32_t),
                            hipMemcpyDeviceToHost, st));
  SF_TRY_SET(hipStreamSynchronize(st));
  int active = 0;
  for (int i = 0; i < count; ++i) active += s[(size_t)i * SF_C2ST_NSTATE + 4] == 0;
  if (n_active) *n_active = active;
  return SF_OK;
}

int sf_c2st_scores(sf_c2st* h, int32_t first, int32_t count, const float* rows_o, int64_t S, double* stats, float* probs,
                   void* stream) {
  if (!h) return sf_fail(SF_ERR_INVALID, "sf_c2st_scores: null handle");
  const SfC2stDims& d = h->dims;
  if (first < 0 || count < 1 || first + count > d.n_cls || S < 1 || S >= (1LL << 31) || !rows_o || !stats)
    return sf_fail(SF_ERR_INVALID, "sf_c2st_scores: classifier range, 1 <= S < 2^31 and non-null arrays needed");
  hipStream_t st = (hipStream_t)stream;
  static SfAttrCache attr;
  static SfAttrCache attr2;
  const bool wide = d.NT > 4;
  if (int rc = wide ? c2st_set_lds((const void*)k_c2st_scores<2>, attr2) : c2st_set_lds((const void*)k_c2st_scores<1>, attr)) return rc;
  SfC2stScoreArgs a{};
  a.rows = rows_o; a.wcur = h->d_wcur; a.S = S; a.stats = stats; a.probs = probs; a.first = first;
  if (wide) hipLaunchKernelGGL(k_c2st_scores<2>, dim3((unsigned)count), dim3(256), h->shmem, st, d, a);
  else hipLaunchKernelGGL(k_c2st_scores<1>, dim3((unsigned)count), dim3(256), h->shmem, st, d, a);
  SF_TRY_SET(hipGetLastError());
  return SF_OK;
}

int sf_c2st_get(sf_c2st* h, float* weights, int32_t* score_log, int32_t* state, void* stream) {
  if (!h) return sf_fail(SF_ERR_INVALID, "sf_c2st_get: null handle");
  const SfC2stDims& d = h->dims;
  hipStream_t st = (hipStream_t)stream;
  if (weights) SF_TRY_SET(hipMemcpyAsync(weights, h->d_wcur, (size_t)d.n_cls * d.NP * sizeof(float), hipMemcpyDeviceToHost, st));
  if (score_log)
    SF_TRY_SET(hipMemcpyAsync(score_log, h->d_slog, (size_t)d.n_cls * d.max_iter * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (state)
    SF_TRY_SET(hipMemcpyAsync(state, h->d_state, (size_t)d.n_cls * SF_C2ST_NSTATE * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SF_TRY_SET(hipStreamSynchronize(st));
  return SF_OK;
}
}  // extern "C"
