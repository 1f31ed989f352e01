// sf_gradtheta_kernels.h -- log q(theta | x) and d log q / d theta (see the header comment in sf_gradtheta.hip).
//
// The sweep of k_maf_train / k_nsf_train (sf_train_kernels.h) without anything that serves the weight gradients: one
// wave per 32-row tile, no consumer wave, no LDS, no gradient image.  The forward pass stashes only what the DATA
// gradient reads on the way back (MAF: u and the tanh outputs; NSF: u, the residual stream h_0..h_NB and t1 of every
// block); the stash keeps the tile numbering of the training kernels.  What the backward sweep carries from transform
// to transform is G = dL/du with L = -log q; after transform 0 it is dL/du_0, and d log q / d theta = -G * pscale.
#pragma once
#include <hip/hip_runtime.h>

#include "sf_flows.h"
#include "sf_internal.h"
#include "sf_train_kernels.h"

struct SfGradThetaArgs {
  const float* theta;  // [B, D]
  const float* x;      // [ceil(B / rows_per_x), C]
  long B;
  long rows_per_x;     // row b reads context row b / rows_per_x
  long tile0;          // first 32-row tile of this launch (workgroup i works tile tile0 + i, stash slot i)
  float* lp;           // [B] or null
  float* dtheta;       // [B, D] or null (null: forward only, nothing is stashed)
  float4* act;         // activation stash, act_per_wave float4 per workgroup of the launch
  long act_per_wave;
};

template <int HT, int DM>
__global__ __launch_bounds__(64) void k_maf_gradtheta(SfDev m0, SfGradThetaArgs a) {
  const SfDev& m = m0;
  const int lane = threadIdx.x & 63;
  const int c = lane & 31, h = lane >> 5;
  const long base = (a.tile0 + (long)blockIdx.x) * 32;
  if (base >= a.B) return;
  const bool bwd = a.dtheta != nullptr;
  float4* stash = a.act + (long)blockIdx.x * a.act_per_wave;
  const int TPT = (m.NB + 1) * HT + 1;  // stash tiles per transform: u, (h0: not stored), a_1..a_NB

  const long row = base + c;
  const bool valid = row < a.B;
  const long ii = valid ? row : a.B - 1;
  const float* xr[1] = {a.x + (ii / a.rows_per_x) * m.C};
  f32x16 ct0[1][1];
  sf_build_ctx_tile<1>(ct0, xr, m, 0, h);
  float u[1][SF_DMAX];
  float logdet[1] = {m.logdet0};
#pragma unroll
  for (int p = DM; p < SF_DMAX; ++p) u[0][p] = 0.f;
#pragma unroll
  for (int p = 0; p < DM; ++p) {
    u[0][p] = 0.f;
    if (p < m.D) {
      const int td = (int)m.cst[m.c_tdim + p];
      u[0][p] = a.theta[ii * m.D + td] * m.cst[m.c_pscale + p] + m.cst[m.c_pshift + p];
    }
  }
  using Ops = MafOps<HT, 1>;

  // ------------------------------------------------------------------ forward
  for (int t = 0; t < m0.T; ++t) {
    const SfDev m = sf_iter_view(m0);
    const float* tp = m.packed + (size_t)t * m.t_stride;
    if (bwd) {
      f32x16 ut;
#pragma unroll
      for (int p = 0; p < SF_DMAX; ++p) ut[p] = p < DM ? u[0][p] : 0.f;
      sf_stash_store(stash, t * TPT, ut, lane);
    }
    f32x16 act[HT][1];
    sf_init_bias<HT, 1>(act, tp + m.o_b0, h);
    {
      f32x16 ut[1][1];
      sf_build_u_tile<1>(ut, u, h);
      sf_mm_acc<HT, 1, 1, false, false, true>(act, ut, tp + m.o_w0, m.nGu, 0, m.nGu, lane);
    }
    sf_ctx_mm<HT, 1>(act, xr, m, tp + m.o_wc, lane, &ct0);
    if (bwd && m.NB == 0) {  // the head then reads h0 itself
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) sf_stash_store(stash, t * TPT + 1 + mt, act[mt][0], lane);
    }
#pragma unroll
    for (int k = 0; k < SF_NBMAX; ++k) {
      if (k < m.NB) {
        f32x16 b[HT][1];
        sf_init_bias<HT, 1>(b, tp + m.o_bk[k], h);
        sf_mm_acc<HT, 1, HT, false, false, true>(b, act, tp + m.o_wk[k], m.nGh, 0, m.nGh, lane);
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) {
#pragma unroll
          for (int r = 0; r < 16; ++r) act[mt][0][r] = sf_tanh(b[mt][0][r]);
          if (bwd) sf_stash_store(stash, t * TPT + 1 + (k + 1) * HT + mt, act[mt][0], lane);
        }
      }
    }
    f32x16 fin[1][1];
    sf_init_bias<1, 1>(fin, tp + m.o_bf, h);
    sf_mm_acc<1, 1, HT, false, false, true>(fin, act, tp + m.o_wf, m.nGh, 0, m.nGh, lane);
    float ld = 0.f;
#pragma unroll
    for (int p = 0; p < DM; ++p) {
      if (p < m.D) {
        const float s = Ops::scale(m, fin[0][0][2 * (p >> 1)]);
        const float val = s * u[0][p] + fin[0][0][2 * (p >> 1) + 1];
        const bool mine = (h == (p & 1));
        const float oth = sf_xhalf(val);
        u[0][p] = mine ? val : oth;
        ld += mine ? sf_log(s) : 0.f;
      }
    }
    logdet[0] += ld + sf_xhalf(ld);
  }
  float G[SF_DMAX];  // dL/d(output of the current transform), replicated in both halves
  const float w = valid ? 1.f : 0.f;
  {
    float ss = 0.f;
#pragma unroll
    for (int p = 0; p < SF_DMAX; ++p) G[p] = 0.f;
#pragma unroll
    for (int p = 0; p < DM; ++p) {
      if (p < m.D) {
        ss += u[0][p] * u[0][p];
        G[p] = w * u[0][p];
      }
    }
    const float nll = 0.5f * ss + 0.5f * (float)m.D * 1.8378770664093453f - logdet[0];
    if (a.lp && valid && h == 0) a.lp[row] = -nll;
  }
  if (!bwd) return;

  // ------------------------------------------------------------------ backward (data gradients only)
  f32x16 aset[2][HT][1];
  f32x16 utile;
  {
    const int t = m0.T - 1;
#pragma unroll
    for (int mt = 0; mt < HT; ++mt) sf_stash_load(stash, t * TPT + 1 + m.NB * HT + mt, aset[0][mt][0], lane);
    sf_stash_load(stash, t * TPT, utile, lane);
  }
  for (int t = m0.T - 1; t >= 0; --t) {
    const SfDev m = sf_iter_view(m0);
    const float* tp = m.packed + (size_t)t * m.t_stride;
    const float* tpT = m.packedT + (size_t)t * m.tT_stride;
    float uin[SF_DMAX];
#pragma unroll
    for (int p = 0; p < SF_DMAX; ++p) uin[p] = p < DM ? utile[p] : 0.f;
    // output of the block below the top one (needed after the head): in flight behind the head recomputation
    if (m.NB >= 2) {
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) sf_stash_load(stash, t * TPT + 1 + (m.NB - 1) * HT + mt, aset[1][mt][0], lane);
    }
    // recompute the head
    f32x16 fin[1][1];
    sf_init_bias<1, 1>(fin, tp + m.o_bf, h);
    sf_mm_acc<1, 1, HT, false, false, true>(fin, aset[0], tp + m.o_wf, m.nGh, 0, m.nGh, lane);
    f32x16 dfin[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) dfin[0][0][r] = 0.f;
    float Gd[SF_DMAX];
#pragma unroll
    for (int p = 0; p < DM; ++p) {
      Gd[p] = 0.f;
      if (p < m.D) {
        const float av = fin[0][0][2 * (p >> 1)];
        const float s = Ops::scale(m, av);
        const float dsda = (m.scale_fn == 0) ? sf_sigmoid(av)
                                             : sf_sigmoid(av + 2.0f) * (1.0f - sf_sigmoid(av + 2.0f));
        const float ds = G[p] * uin[p] - w / s;
        const bool mine = (h == (p & 1));
        dfin[0][0][2 * (p >> 1)] = mine ? ds * dsda : dfin[0][0][2 * (p >> 1)];
        dfin[0][0][2 * (p >> 1) + 1] = mine ? G[p] : dfin[0][0][2 * (p >> 1) + 1];
        const float gd = G[p] * s;
        const float oth = sf_xhalf(gd);
        Gd[p] = mine ? gd : oth;
      }
    }
    // delta_h = Wf^T dfin
    f32x16 dh[HT][1];
#pragma unroll
    for (int mt = 0; mt < HT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dh[mt][0][r] = 0.f;
    sf_mm_acc<HT, 1, 1, false, false, true>(dh, dfin, tpT + m.oT_wf, m.nGf, 0, m.nGf, lane);
#pragma unroll
    for (int d = 0; d < SF_NBMAX; ++d) {  // d = distance from the top block: block k = NB - 1 - d
      if (d < m.NB) {
        const int k = m.NB - 1 - d;
        int oT_wk = m.oT_wk[0];
#pragma unroll
        for (int q = 1; q < SF_NBMAX; ++q) oT_wk = (k == q) ? m.oT_wk[q] : oT_wk;
        f32x16 (&aout)[HT][1] = aset[d & 1];  // a_{k+1}: output of block k
        f32x16 dpre[HT][1];
#pragma unroll
        for (int mt = 0; mt < HT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) dpre[mt][0][r] = dh[mt][0][r] * (1.0f - aout[mt][0][r] * aout[mt][0][r]);
        // a_{k+1} is dead now: its registers take the output of the block two below (block k - 1's is already loaded)
        if (k >= 2) {
#pragma unroll
          for (int mt = 0; mt < HT; ++mt) sf_stash_load(stash, t * TPT + 1 + (k - 1) * HT + mt, aout[mt][0], lane);
        }
#pragma unroll
        for (int mt = 0; mt < HT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) dh[mt][0][r] = 0.f;
        sf_mm_acc<HT, 1, HT, false, false, true>(dh, dpre, tpT + oT_wk, m.nGh, 0, m.nGh, lane);
      }
    }
    // first loads of the transform above: in flight during the last product of this one
    if (t >= 1) {
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) sf_stash_load(stash, (t - 1) * TPT + 1 + m.NB * HT + mt, aset[0][mt][0], lane);
      sf_stash_load(stash, (t - 1) * TPT, utile, lane);
    }
    // delta_u = W0^T delta_h0
    f32x16 du[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) du[0][0][r] = 0.f;
    sf_mm_acc<1, 1, HT, false, false, true>(du, dh, tpT + m.oT_w0, m.nGh, 0, m.nGh, lane);
#pragma unroll
    for (int p = 0; p < DM; ++p) {
      if (p < m.D) {
        const float v = du[0][0][(p & 3) + 4 * (p >> 3)];
        const float oth = sf_xhalf(v);
        G[p] = Gd[p] + ((h == ((p >> 2) & 1)) ? v : oth);
      }
    }
  }
  if (valid && h == 0) {
#pragma unroll
    for (int p = 0; p < DM; ++p) {
      if (p < m.D) {
        const int td = (int)m.cst[m.c_tdim + p];
        a.dtheta[row * m.D + td] = -G[p] * m.cst[m.c_pscale + p];
      }
    }
  }
}


template <int HT, int PT>
__global__ __launch_bounds__(64) void k_nsf_gradtheta(SfDev m0, SfGradThetaArgs a) {
  const SfDev& m = m0;
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5;
  const int c = lane & 31;
  const long base = (a.tile0 + (long)blockIdx.x) * 32;
  if (base >= a.B) return;
  const bool bwd = a.dtheta != nullptr;
  float4* stash = a.act + (long)blockIdx.x * a.act_per_wave;
  // stash tiles per transform as in k_nsf_train: [0] u_in, [1..HT] h_0, per block k: t1, (t2: not stored), h_{k+1}
  const int TPT = 2 + (3 * m.NB + 1) * HT;
  using Ops = NsfOps<HT, PT, 1>;

  const long row = base + c;
  const bool valid = row < a.B;
  const long ii = valid ? row : a.B - 1;
  const float* xr[1] = {a.x + (ii / a.rows_per_x) * m.C};
  f32x16 ct0[1][1];
  sf_build_ctx_tile<1>(ct0, xr, m, 0, h);
  float u[1][SF_DMAX];
  float logdet[1] = {m.logdet0};
#pragma unroll
  for (int p = 0; p < SF_DMAX; ++p) {
    u[0][p] = 0.f;
    if (p < m.D) u[0][p] = a.theta[ii * m.D + p] * m.cst[m.c_pscale + p] + m.cst[m.c_pshift + p];
  }

  // ------------------------------------------------------------------ forward
  for (int t = 0; t < m0.T; ++t) {
    const SfDev m = sf_iter_view(m0);
    const float* tp = m.packed + (size_t)t * m.t_stride;
    const int sb = t * TPT;
    if (bwd) {
      f32x16 ut;
#pragma unroll
      for (int p = 0; p < SF_DMAX; ++p) ut[p] = u[0][p];
      sf_stash_store(stash, sb, ut, lane);
    }
    f32x16 hid[HT][1];
    sf_init_bias<HT, 1>(hid, tp + m.o_bin, h);
    {
      f32x16 ut[1][1];
      sf_build_u_tile<1>(ut, u, h);
      sf_mm_acc<HT, 1, 1, false, false, true>(hid, ut, tp + m.o_winu, m.nGu, 0, m.nGu, lane);
    }
    sf_ctx_mm<HT, 1>(hid, xr, m, tp + m.o_winc, lane, &ct0);
    if (bwd) {
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) sf_stash_store(stash, sb + 1 + mt, hid[mt][0], lane);
    }
#pragma unroll
    for (int k = 0; k < SF_NBMAX; ++k) {
      if (k < m.NB) {
        const int bb = sb + 1 + HT + k * 3 * HT;
        f32x16 t2[HT][1];
        {
          f32x16 t1[HT][1];
          sf_init_bias<HT, 1>(t1, tp + m.o_b1[k], h);
          sf_mm_acc<HT, 1, HT, true, false, true>(t1, hid, tp + m.o_w1[k], m.nGh, 0, m.nGh, lane);
          if (bwd) {
#pragma unroll
            for (int mt = 0; mt < HT; ++mt) sf_stash_store(stash, bb + mt, t1[mt][0], lane);
          }
          sf_init_bias<HT, 1>(t2, tp + m.o_b2[k], h);
          sf_mm_acc<HT, 1, HT, true, false, true>(t2, t1, tp + m.o_w2[k], m.nGh, 0, m.nGh, lane);
        }
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) {
          f32x16 g[1][1];
          sf_init_bias<1, 1>(g, tp + m.o_bg[k] + mt * 32, h);
          sf_ctx_mm<1, 1>(g, xr, m, tp + m.o_wg[k] + mt * m.nGc * 256, lane, &ct0);
#pragma unroll
          for (int r = 0; r < 16; ++r) hid[mt][0][r] += t2[mt][0][r] * sf_sigmoid(g[0][0][r]);
          if (bwd) sf_stash_store(stash, bb + 2 * HT + mt, hid[mt][0], lane);
        }
      }
    }
    Ops::spline_apply(m, tp, t, hid, u, logdet, false, lane);
    if (m.D > 1) Ops::lu_forward(m, tp + m.o_lu, u, logdet);
  }
  float G[SF_DMAX];
  const float w = valid ? 1.f : 0.f;
  {
    float ss = 0.f;
#pragma unroll
    for (int p = 0; p < SF_DMAX; ++p) {
      G[p] = 0.f;
      if (p < m.D) {
        ss += u[0][p] * u[0][p];
        G[p] = w * u[0][p];
      }
    }
    const float nll = 0.5f * ss + 0.5f * (float)m.D * 1.8378770664093453f - logdet[0];
    if (a.lp && valid && h == 0) a.lp[row] = -nll;
  }
  if (!bwd) return;

  // ------------------------------------------------------------------ backward (data gradients only)
  for (int t = m0.T - 1; t >= 0; --t) {
    const SfDev m = sf_iter_view(m0);
    const float* tp = m.packed + (size_t)t * m.t_stride;
    const float* tpT = m.packedT + (size_t)t * m.tT_stride;
    const int sb = t * TPT;
    const int D = m.D;
    float uin[SF_DMAX];
    {
      f32x16 ut;
      sf_stash_load(stash, sb, ut, lane);
#pragma unroll
      for (int p = 0; p < SF_DMAX; ++p) uin[p] = ut[p];
    }
    // ---- LULinear backward:  y = L t + b, t = U u'  ->  du' = U^T L^T G
    if (D > 1) {
      const float* lp = tp + m.o_lu;
      const float* Lm = lp;
      const float* Um = lp + D * D;
      const float* ud = lp + 2 * D * D;
      float dt[SF_DMAX];
#pragma unroll
      for (int j = 0; j < SF_DMAX; ++j) {
        dt[j] = 0.f;
        if (j < D) {
          dt[j] = G[j];
#pragma unroll
          for (int i = 0; i < SF_DMAX; ++i)
            if (i > j && i < D) dt[j] += Lm[i * D + j] * G[i];
        }
      }
      float Gn[SF_DMAX];
#pragma unroll
      for (int j = 0; j < SF_DMAX; ++j) {
        Gn[j] = 0.f;
        if (j < D) {
          Gn[j] = (sf_softplus(ud[j]) + m.lu_eps) * dt[j];
#pragma unroll
          for (int i = 0; i < SF_DMAX; ++i)
            if (i < j) Gn[j] += Um[i * D + j] * dt[i];
        }
      }
#pragma unroll
      for (int p = 0; p < SF_DMAX; ++p) G[p] = Gn[p];
    }
    // ---- spline head + spline backward
    f32x16 hN[HT][1];
#pragma unroll
    for (int mt = 0; mt < HT; ++mt)
      sf_stash_load(stash, m.NB == 0 ? sb + 1 + mt : sb + 1 + HT + (m.NB - 1) * 3 * HT + 2 * HT + mt, hN[mt][0], lane);
    f32x16 dh[HT][1];
#pragma unroll
    for (int mt = 0; mt < HT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dh[mt][0][r] = 0.f;
    {
      const int start = t & 1;
      const int d_tr = (D - start + 1) / 2;
      for (int jp = 0; jp * 2 < d_tr; ++jp) {
        f32x16 q[PT][1];
        sf_init_bias<PT, 1>(q, tp + m.o_bout + jp * PT * 32, h);
        sf_mm_acc<PT, 1, HT, false, false, true>(q, hN, tp + m.o_wout + jp * PT * m.nGh * 256, m.nGh, 0, m.nGh, lane);
        const int kdim = 2 * jp + h;
        const bool have = kdim < d_tr;
        const int tgt = start + 2 * kdim;
        const int tgt_o = start + 2 * (2 * jp + (1 - h));
        const bool have_o = (2 * jp + (1 - h)) < d_tr;
        float vin = 0.f, Go = 0.f;
#pragma unroll
        for (int p = 0; p < SF_DMAX; ++p) {
          vin = (p == tgt) ? uin[p] : vin;
          Go = (p == tgt) ? G[p] : Go;
        }
        f32x16 dq[PT][1];
        float vout, lad, dv;
        SfSplineBwd<PT>::template eval<1>(m, q, 0, vin, have ? Go : 0.f, have ? -w : 0.f, vout, lad, dv, dq);
        dv = have ? dv : 0.f;
        const float dvo = sf_xhalf(dv);
#pragma unroll
        for (int p = 0; p < SF_DMAX; ++p) {
          G[p] = (have && p == tgt) ? dv : G[p];
          G[p] = (have_o && p == tgt_o) ? dvo : G[p];
        }
        sf_mm_acc<HT, 1, PT, false, false, true>(dh, dq, tpT + m.oT_wout + jp * HT * (PT * 4) * 256, PT * 4, 0, PT * 4, lane);
      }
    }
    // ---- ResidualNet backward
#pragma unroll
    for (int kk = 0; kk < SF_NBMAX; ++kk) {
      const int k = SF_NBMAX - 1 - kk;
      if (k < m.NB) {
        const int bb = sb + 1 + HT + k * 3 * HT;
        f32x16 dt2[HT][1];
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) {
          f32x16 g[1][1];
          sf_init_bias<1, 1>(g, tp + m.o_bg[k] + mt * 32, h);
          sf_ctx_mm<1, 1>(g, xr, m, tp + m.o_wg[k] + mt * m.nGc * 256, lane, &ct0);
#pragma unroll
          for (int r = 0; r < 16; ++r) dt2[mt][0][r] = dh[mt][0][r] * sf_sigmoid(g[0][0][r]);
        }
        f32x16 t1[HT][1];
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) sf_stash_load(stash, bb + mt, t1[mt][0], lane);
        f32x16 dt1[HT][1];
#pragma unroll
        for (int mt = 0; mt < HT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) dt1[mt][0][r] = 0.f;
        sf_mm_acc<HT, 1, HT, false, false, true>(dt1, dt2, tpT + m.oT_w2[k], m.nGh, 0, m.nGh, lane);
#pragma unroll
        for (int mt = 0; mt < HT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) dt1[mt][0][r] = t1[mt][0][r] > 0.f ? dt1[mt][0][r] : 0.f;
        // h_k = input of this block (its sign is the mask of the block's first ReLU)
        f32x16 hk[HT][1];
#pragma unroll
        for (int mt = 0; mt < HT; ++mt)
          sf_stash_load(stash, k == 0 ? sb + 1 + mt : sb + 1 + HT + (k - 1) * 3 * HT + 2 * HT + mt, hk[mt][0], lane);
        f32x16 dr0[HT][1];
#pragma unroll
        for (int mt = 0; mt < HT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) dr0[mt][0][r] = 0.f;
        sf_mm_acc<HT, 1, HT, false, false, true>(dr0, dt1, tpT + m.oT_w1[k], m.nGh, 0, m.nGh, lane);
#pragma unroll
        for (int mt = 0; mt < HT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) dh[mt][0][r] += hk[mt][0][r] > 0.f ? dr0[mt][0][r] : 0.f;
      }
    }
    // ---- initial layer: delta_u = Win_u^T delta_h0
    f32x16 du[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) du[0][0][r] = 0.f;
    sf_mm_acc<1, 1, HT, false, false, true>(du, dh, tpT + m.oT_winu, m.nGh, 0, m.nGh, lane);
#pragma unroll
    for (int p = 0; p < SF_DMAX; ++p) {
      if (p < D) {
        const float v = du[0][0][(p & 3) + 4 * (p >> 3)];
        const float oth = sf_xhalf(v);
        G[p] += (h == ((p >> 2) & 1)) ? v : oth;
      }
    }
  }
  if (valid && h == 0) {
#pragma unroll
    for (int p = 0; p < SF_DMAX; ++p)
      if (p < m.D) a.dtheta[row * m.D + p] = -G[p] * m.cst[m.c_pscale + p];
  }
}
