// sf_train.hip -- training kernels.
//   (1) fused global-norm clip + Adam/AdamW      ref: custom_runner.py:613-618
//   (2) forward + backward of -log_prob          ref: custom_runner.py:604-610
#include "sf_train.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>

#include "sf_internal.h"
#include "sf_train_args.h"
#include "sf_fixacc.h"
#include "sf_nsf1.h"
#include "sf_nsfar.h"
#include "sf_nsfc.h"
#include "sf_pack.h"
#include "sf_trainc.h"

// ---------------------------------------------------------------------------------------------
// clip_grad_norm_ + Adam
// ---------------------------------------------------------------------------------------------
// Two-kernel form (n > 131072, or a gradient that is not 16-byte aligned): every block leaves its share of |grad|^2 in
// shares[blockIdx.x] (SF_ADAM_SHARES at the most), and every block of k_adam sums the shares in the same fixed order.  No atomics:
// the norm -- and with it the clip coefficient and the step -- is the same bits call after call, and its rounding error is that of
// a tree, not of a chain of adds into one growing total (2e-7 relative seen on 129 blocks: more than the rest of the step together).
#define SF_ADAM_SHARES 256
__global__ __launch_bounds__(256) void k_sqnorm(const float* __restrict__ g, long n, float* __restrict__ shares) {
  float s = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    s += g[i] * g[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ float part[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) part[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) shares[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, const float* __restrict__ shares, int n_shares,
                                              float* __restrict__ sq_out, long n, sf_adam_desc d, float bc1, float bc2,
                                              float max_norm, float* __restrict__ norm_out) {
  float s = (int)threadIdx.x < n_shares ? shares[threadIdx.x] : 0.f;   // n_shares <= SF_ADAM_SHARES = blockDim.x
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ float part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  const float sq = (part[0] + part[1]) + (part[2] + part[3]);
  const float total = sqrtf(sq);
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(max_norm / (total + 1e-6f), 1.0f);  // torch clip_grad_norm_
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *sq_out = sq;
    if (norm_out) *norm_out = total;
  }
  const float step_size = d.lr / bc1;
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pi = p[i];
    float gi = g[i] * coef;
    if (d.decoupled) pi *= (1.f - d.lr * d.weight_decay);
    else if (d.weight_decay != 0.f) gi += d.weight_decay * pi;
    const float mi = d.beta1 * m[i] + (1.f - d.beta1) * gi;
    const float vi = d.beta2 * v[i] + (1.f - d.beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + d.eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

// One-launch form for small parameter vectors (n <= 131072): every workgroup first reduces the WHOLE gradient to
// its squared norm (L2-resident re-reads, a fixed summation order -> the clip coefficient is deterministic), then
// updates its own slice.  Replaces memset + k_sqnorm + k_adam.
__global__ __launch_bounds__(1024) void k_adam_fused(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ sq_out, long n,
                                                    sf_adam_desc d, float bc1, float bc2, float max_norm,
                                                    float* __restrict__ norm_out, const float* __restrict__ sq_part, int n_sq) {
  // Everything this thread will need is requested before anything is waited for: its own elements of p / m / v / g (one
  // float4 each for n <= 4096 x blocks: the common case) AND its eight float4 of the gradient for the norm -- the kernel
  // is a chain of L2 round trips (32 k parameters: 12 us when the norm took two trips and the update a third).
  const long n4 = n >> 2;
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  const long own = (long)blockIdx.x * blockDim.x + threadIdx.x;  // first float4 this thread updates (n % 4 == 0 path)
  const bool vec = (n & 3) == 0 && (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  const bool has_own = vec && own < n4;
  float4 po, mo, vo, go;
  if (has_own) {
    po = reinterpret_cast<const float4*>(p)[own]; mo = reinterpret_cast<const float4*>(m)[own];
    vo = reinterpret_cast<const float4*>(v)[own]; go = g4[own];
  }
  float s = 0.f;
  if (sq_part) {   // the gather left the norm in n_sq shares: one short strided read instead of the whole gradient
    for (int i = threadIdx.x; i < n_sq; i += 1024) s += sq_part[i];
  } else {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long i = threadIdx.x; i < n4; i += 8 * 1024) {
      float4 q[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) q[k] = i + k * 1024 < n4 ? g4[i + k * 1024] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += q[k].x * q[k].x + q[k].y * q[k].y + q[k].z * q[k].z + q[k].w * q[k].w;
    }
    s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 1024) s += g[i] * g[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ float part[16];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  float sq = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) sq += part[w];
  const float total = sqrtf(sq);
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(max_norm / (total + 1e-6f), 1.0f);  // torch clip_grad_norm_
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *sq_out = sq;
    if (norm_out) *norm_out = total;
  }
  const float step_size = d.lr / bc1;
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  auto upd = [&](float& pi, float& mi, float& vi, float gi_raw) {
    float gi = gi_raw * coef;
    if (d.decoupled) pi *= (1.f - d.lr * d.weight_decay);
    else if (d.weight_decay != 0.f) gi += d.weight_decay * pi;
    mi = d.beta1 * mi + (1.f - d.beta1) * gi;
    vi = d.beta2 * vi + (1.f - d.beta2) * gi * gi;
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + d.eps;
    pi = pi - step_size * (mi / denom);
  };
  if (vec) {
    if (has_own) {
      upd(po.x, mo.x, vo.x, go.x); upd(po.y, mo.y, vo.y, go.y); upd(po.z, mo.z, vo.z, go.z); upd(po.w, mo.w, vo.w, go.w);
      reinterpret_cast<float4*>(p)[own] = po; reinterpret_cast<float4*>(m)[own] = mo; reinterpret_cast<float4*>(v)[own] = vo;
    }
    // (more float4 than threads: the rest in a strided loop)
    for (long i = own + (long)gridDim.x * blockDim.x; i < n4; i += (long)gridDim.x * blockDim.x) {
      float4 pp = reinterpret_cast<const float4*>(p)[i], mm = reinterpret_cast<const float4*>(m)[i];
      float4 vv = reinterpret_cast<const float4*>(v)[i];
      const float4 gg = g4[i];
      upd(pp.x, mm.x, vv.x, gg.x); upd(pp.y, mm.y, vv.y, gg.y); upd(pp.z, mm.z, vv.z, gg.z); upd(pp.w, mm.w, vv.w, gg.w);
      reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(m)[i] = mm; reinterpret_cast<float4*>(v)[i] = vv;
    }
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
      float pi = p[i], mi = m[i], vi = v[i];
      upd(pi, mi, vi, g[i]);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
  }
}

// the spread loss sums of an epoch call (SfTrcArgs::loss_mask) -> the caller's scalar; the parts are zeroed for the next call
// (values on a 2^-20 grid: the double adds are exact in any order)
__global__ void k_fold_loss(double* __restrict__ part, int n, double* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) { s += part[i]; part[i] = 0.0; }
    *out += s;
  }
}
hipError_t sf_launch_fold_loss(double* part, int n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_fold_loss, dim3(1), dim3(64), 0, st, part, n, out);
  return hipGetLastError();
}

// The shares of the two-kernel form: SF_ADAM_SHARES floats per (device, stream, calling thread), taken on first use and kept for
// the life of the process -- sf_adam_apply has no handle that could own them.  Calls on one stream are ordered, so are the uses of
// its buffer; two threads that name the same stream (hipStreamPerThread is one name for many) never share one.
static float* adam_shares(hipStream_t st) {
  static std::mutex mu;
  static std::map<std::tuple<int, hipStream_t, std::thread::id>, float*> held;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lock(mu);
  float*& p = held[std::make_tuple(dev, st, std::this_thread::get_id())];
  if (!p && hipMalloc(&p, SF_ADAM_SHARES * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
  return p;
}

hipError_t sf_launch_adam(float* params, const float* grad, float* m, float* v, float* norm_scratch, long n,
                          const sf_adam_desc& d, float bc1, float bc2, float max_norm, float* grad_norm_out,
                          hipStream_t st, const float* sq_part, int n_sq) {
  if (n <= 131072 && ((uintptr_t)grad & 15) == 0) {  // (the fused kernel reads the gradient as float4)
    const int nb = (int)((n + 4095) / 4096);
    hipLaunchKernelGGL(k_adam_fused, dim3(nb < 1 ? 1 : nb), dim3(1024), 0, st, params, grad, m, v, norm_scratch, n, d, bc1,
                       bc2, max_norm, grad_norm_out, sq_part, n_sq);
    return hipGetLastError();
  }
  float* shares = adam_shares(st);
  if (!shares) return hipErrorOutOfMemory;
  const int blocks = (int)((n + 1023) / 1024 < SF_ADAM_SHARES ? (n + 1023) / 1024 : SF_ADAM_SHARES);
  hipLaunchKernelGGL(k_sqnorm, dim3(blocks), dim3(256), 0, st, grad, n, shares);
  hipLaunchKernelGGL(k_adam, dim3(blocks), dim3(256), 0, st, params, grad, m, v, shares, blocks, norm_scratch, n, d, bc1, bc2,
                     max_norm, grad_norm_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// forward + backward of  L = w * (-log p(theta | x))
//
// One wave = one 32-sample tile, end to end: forward with the block activations stashed in HBM
// (tile-register layout, float4 per lane, coalesced), then the backward sweep.
//   data gradients   : delta_in = W^T delta_out  -- same MFMA chaining as the forward, on the
//                      transposed operand image (packedT)
//   weight gradients : dW^T tile = in_tile . delta_tile^T over the 32 samples -- both operands
//                      are transposed through a per-wave LDS scratch ([row][33] floats, conflict
//                      free both ways); the accumulator registers ARE the packed float4 groups, so
//                      they are added to the gradient image with 256-byte-contiguous f32 atomics
//   bias gradients   : row sums of the delta tile, taken from the B operands already read
// ---------------------------------------------------------------------------------------------
__global__ void k_grad_gather(const float* __restrict__ gimg, long stride, int copies, const int32_t* __restrict__ gdst,
                              float* __restrict__ grad, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = gdst[i];
  float v = 0.f;
  if (g >= 0) {
    for (int c = 0; c < copies; ++c) v += gimg[(size_t)c * stride + g];  // fixed order over the replicas
  }
  grad[i] = v;
}

// one launch for everything a training step needs before the flow kernel: forward image, transposed image,
// zeroed gradient image (and zeroed context-gradient rows); the pack rules are those of sf_pack.h.  (Of the fp32 tables only the
// 16-row one, u2, carries SF_PACK_TANH_SCALE: for s2, t2 and c2 sf_pack_f32 is the plain two-table sum.)
__global__ void k_train_prep(const float* __restrict__ flat, const int32_t* __restrict__ s1, const int32_t* __restrict__ s2,
                             float* __restrict__ packed, long n1, const int32_t* __restrict__ t1,
                             const int32_t* __restrict__ t2, float* __restrict__ packedT, long n2,
                             float* __restrict__ gimg, int copies, float* __restrict__ dctx, long n4,
                             const int32_t* __restrict__ u1, const int32_t* __restrict__ u2, float* __restrict__ packed16,
                             long n5, const int32_t* __restrict__ sB, unsigned short* __restrict__ packed16B, long n6,
                             const int32_t* __restrict__ c1, const int32_t* __restrict__ c2, float* __restrict__ imgC, long n7) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n1) {
    packed[i] = sf_pack_f32(flat, s1[i], s2[i]);
    for (int c = 0; c < copies; ++c) gimg[(size_t)c * n1 + i] = 0.f;
    return;
  }
  i -= n1;
  if (i < n2) { packedT[i] = sf_pack_f32(flat, t1[i], t2[i]); return; }
  i -= n2;
  if (i < n4) { dctx[i] = 0.f; return; }
  i -= n4;
  if (i < n5) { packed16[i] = sf_pack_f32(flat, u1[i], u2[i]); return; }  // 16-row sampler image (so that sampling right after a training step needs no set_params)
  i -= n5;
  if (i < n6) { packed16B[i] = sf_pack_bf16_split(flat, sB[i]); return; }  // split-bf16 hidden blocks of the persistent sampler
  i -= n6;
  if (i < n7) imgC[i] = sf_pack_f32(flat, c1[i], c2[i]);  // cooperative training image (sf_trainc.hip)
}

#define SF_TDECL(H)                                                                         \
  hipError_t sf_launch_maf_train_h##H(const SfDev&, const SfTrainArgs&, hipStream_t);       \
  hipError_t sf_launch_nsf_train_h##H(const SfDev&, const SfTrainArgs&, hipStream_t);
SF_TDECL(1) SF_TDECL(2) SF_TDECL(3) SF_TDECL(4)


// The epoch loop (sf_flow_train_epoch) asks the gather for the per-block shares of |grad|^2: returns the buffer (grown on demand)
// and notes how many shares the gradient of THIS call comes with; null when nobody asked or the buffer cannot be had.
static float* sq_for(sf_flow* f, const SfLayout& L) {
  f->n_sqpart = 0;
  if (!f->want_sq) return nullptr;
  const long nb = sf_gather_c2_blocks((long)L.n_gradC, f->n_gzeroC);
  if (f->d_sqpart.grow((size_t)nb) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  f->n_sqpart = (int)nb;
  return f->d_sqpart;
}

// ---- lazily built training state: all or nothing -- a failed allocation frees what was already taken (the local group), so
// that the next call starts over instead of launching kernels on half-built state
static int ensure_trainc(sf_flow* f) {   // the cooperative kernels' image and gather tables
  if (f->trainc_ready) return SF_OK;
  const SfLayout& L = f->L;
  SfFlowTrainC c;
  SF_TRY_SET(c.d_imgC.alloc((size_t)L.n_imgC));
  SF_TRY_SET(c.d_sC1.alloc((size_t)L.n_imgC));
  SF_TRY_SET(c.d_sC2.alloc((size_t)L.n_imgC));
  SF_TRY_SET(hipMemcpy(c.d_sC1, L.srcC1.data(), (size_t)L.n_imgC * sizeof(int32_t), hipMemcpyHostToDevice));
  SF_TRY_SET(hipMemcpy(c.d_sC2, L.srcC2.data(), (size_t)L.n_imgC * sizeof(int32_t), hipMemcpyHostToDevice));
  // position -> parameter(s) and the parameters without a position (sf_layout.cpp): the gather walks the partials in THEIR order
  SF_TRY_SET(c.d_gsrcC.upload(L.gsrcC));
  c.n_gzeroC = (long)L.gzeroC.size();
  if (!L.gzeroC.empty()) SF_TRY_SET(c.d_gzeroC.upload(L.gzeroC));
  static_cast<SfFlowTrainC&>(*f) = std::move(c);
  f->trainc_ready = true;
  return SF_OK;
}
static int ensure_train(sf_flow* f) {   // the 32-row kernels' transposed image and gradient image
  if (f->train_ready) return SF_OK;
  const SfLayout& L = f->L;
  SfFlowTrain t;
  SF_TRY_SET(t.d_packedT.alloc((size_t)L.n_packedT));
  SF_TRY_SET(t.d_t1.alloc((size_t)L.n_packedT));
  SF_TRY_SET(t.d_t2.alloc((size_t)L.n_packedT));
  SF_TRY_SET(hipMemcpy(t.d_t1, L.srcT1.data(), (size_t)L.n_packedT * sizeof(int32_t), hipMemcpyHostToDevice));
  SF_TRY_SET(hipMemcpy(t.d_t2, L.srcT2.data(), (size_t)L.n_packedT * sizeof(int32_t), hipMemcpyHostToDevice));
  SF_TRY_SET(t.d_gpacked.alloc((size_t)SF_GCOPIES * L.n_packed));
  SF_TRY_SET(t.d_gdst.upload(L.gdst));
  static_cast<SfFlowTrain&>(*f) = std::move(t);
  f->train_ready = true;
  return SF_OK;
}

// ---- the profiling bracket (sf_flow_set_profiling): the step's flow kernel between the handle's two events
static int train_events(sf_flow* f) {
  if (f->profiling) { SF_TRY_SET(f->ev_train[0].create()); SF_TRY_SET(f->ev_train[1].create()); }
  return SF_OK;
}
template <typename Launch>
static int bracketed(sf_flow* f, hipStream_t st, Launch launch) {
  int rc = train_events(f);
  if (rc) return rc;
  if (f->profiling) SF_TRY_SET(hipEventRecord(f->ev_train[0], st));
  rc = launch();
  if (rc) return rc;
  if (f->profiling) {
    SF_TRY_SET(hipEventRecord(f->ev_train[1], st));
    f->ev_train_valid = true;
  }
  return SF_OK;
}

// ---- cooperative 16-row kernels: MAF (sf_trainc.hip: two blocks, D <= 8, T <= SF_TRC_TS, <= 4 hidden tiles) and
//      NSF (sf_nsfc.hip: two blocks, D <= 8, H <= 64, K <= 11); they share the image / gather machinery
static int coop_loss_grad(sf_flow* f, bool coop_nsf, const float* flat, const float* theta, const float* x, const long long* idx,
                          long B, float grad_scale, const float* weights, float* loss, double* loss_sum, float* grad, float* dctx,
                          hipStream_t st) {
  const SfLayout& L = f->L;
  const SfDev& v = L.dev;
  int rc = ensure_trainc(f);
  if (rc) return rc;
  const int grid = coop_nsf ? sf_nsfc_grid(B, L.nsc.NT) : sf_trainc_grid(B, &L.trc, v.T);
  // Gradient accumulation (sf_fixacc.h): per-workgroup partials + gather while they are few, above that 2^-40 fixed-point
  // contributions added with int64 atomics into one zeroed replica per XCD (L2-resident, order independent).  The gather
  // reads the position -> parameter table (d_gsrcC) either way; SF_GRAD_ACC=partial | fix forces one form.
  const int nsf_mode = coop_nsf ? sf_nsfc_acc_mode(B, grid, (long)L.n_gradC) : 0;
  const bool use_fix = coop_nsf ? nsf_mode != 0 : sf_trainc_fix(grid, (long)L.n_gradC);
  if (use_fix && !f->d_gfixC) SF_TRY_SET(f->d_gfixC.alloc((size_t)SF_FIX_REPLICAS * (size_t)L.n_gradC));
  if (use_fix) SF_TRY_SET(hipMemsetAsync(f->d_gfixC, 0, (size_t)SF_FIX_REPLICAS * (size_t)L.n_gradC * sizeof(long long), st));
  const int n_part = use_fix ? 1 : grid;   // (fix: d_gpartC is only the base the job descriptors count from)
  const size_t need = (size_t)n_part * (size_t)L.n_gradC;
  SF_TRY_SET(f->d_gpartC.grow(need));
  {
    // inside an epoch call (sf_flow_train_epoch, all steps but its last) only the cooperative image is re-tiled: the density
    // and sampler images are not read by the training kernels, and nobody can look at them before the call returns
    const bool lite = f->prep_lite;
    const long n1 = lite ? 0 : (long)L.n_packed;
    const long n4 = dctx ? B * (long)v.C : 0;
    const long n5 = (!lite && f->d_packed16) ? (long)L.n_packed16 : 0;
    const long n6 = (!lite && f->d_packed16B) ? (long)L.n_packed16B : 0;
    const long n7 = (long)L.n_imgC;
    const long tot = n1 + n4 + n5 + n6 + n7;
    hipLaunchKernelGGL(k_train_prep, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, flat, f->d_s1, f->d_s2, f->d_packed,
                       n1, (const int32_t*)nullptr, (const int32_t*)nullptr, (float*)nullptr, 0L, (float*)nullptr, 0,
                       dctx, n4, f->d_s16a, f->d_s16b, f->d_packed16, n5, f->d_s16B, f->d_packed16B, n6, f->d_sC1, f->d_sC2,
                       f->d_imgC, n7);
    SF_TRY_SET(hipGetLastError());
    f->packed16_stale = lite;
    f->packed_stale = lite;
    f->wp_stale = true;
  }
  if (L.n_packedB > 0) SF_TRY_SET(sf_launch_pack_bf16(flat, f->d_bsrc, f->d_packedB, (long)L.n_packedB, st));
  auto common = [&](auto& a) {   // the fields SfNscArgs and SfTrcArgs share
    a.img = f->d_imgC; a.cst = f->d_cst;
    a.D = v.D; a.C = v.C; a.T = v.T; a.logdet0 = v.logdet0;
    a.c_pscale = v.c_pscale; a.c_pshift = v.c_pshift; a.c_xmean = v.c_xmean; a.c_xstd = v.c_xstd;
    a.theta = theta; a.x = x; a.idx = idx; a.wts = weights; a.B = B; a.w = grad_scale;
    a.loss = loss; a.loss_sum = loss_sum; a.loss_mask = 0;
    if (loss_sum && f->d_losspart) { a.loss_sum = f->d_losspart; a.loss_mask = SF_LOSS_PARTS - 1; f->losspart_used = true; }
    a.gpart = f->d_gpartC; a.gpart_stride = (long)L.n_gradC; a.fix = use_fix ? f->d_gfixC : nullptr;
  };
  if (coop_nsf) {
    const long n_chunks = (B + 31) / 32;
    const size_t ust_need = (size_t)n_chunks * 32 * (size_t)v.T * 16;
    SF_TRY_SET(f->d_ustash.grow(ust_need));
    SfNscArgs a;
    common(a);
    a.c = L.nsc;
    a.K = v.K;
    a.tail_bound = v.tail_bound; a.min_w = v.min_w; a.min_h = v.min_h; a.min_d = v.min_d; a.lu_eps = v.lu_eps;
    a.inv_sqrt_h = v.inv_sqrt_h; a.deriv_const = v.deriv_const;
    a.n_chunks = n_chunks; a.fix_mode = nsf_mode;
    a.ustash = f->d_ustash;
#ifdef SF_NSC_TRACE
    a.trace = nullptr;
#endif
    rc = bracketed(f, st, [&]() -> int { SF_TRY_SET(sf_launch_nsf_trainc(a, grid, st)); return SF_OK; });
  } else {
    const long per_chunk = 32L * sf_trainc_groups(B, &L.trc, v.T);
    SfTrcArgs a;
    common(a);
    a.c = L.trc;
    a.scale_fn = v.scale_fn; a.eps = v.eps; a.c_tdim = v.c_tdim;
    a.n_chunks = (B + per_chunk - 1) / per_chunk;
    a.dctx = dctx;
    rc = bracketed(f, st, [&]() -> int { SF_TRY_SET(sf_launch_maf_trainc(a, grid, st)); return SF_OK; });
  }
  if (rc) return rc;
  // the gather: float replicas (NSF only: the partial gather over SF_FIX_REPLICAS images), fixed point, partials by position
  if (use_fix && nsf_mode == 2)
    SF_TRY_SET(sf_launch_gather_c2(reinterpret_cast<const float*>(f->d_gfixC.get()), (long)L.n_gradC, SF_FIX_REPLICAS, f->d_gsrcC, f->d_gzeroC, f->n_gzeroC, grad, st, sq_for(f, L)));
  else if (use_fix) SF_TRY_SET(sf_launch_gather_fix(f->d_gfixC, (long)L.n_gradC, SF_FIX_REPLICAS, f->d_gsrcC, f->d_gzeroC, f->n_gzeroC, grad, st));
  else SF_TRY_SET(sf_launch_gather_c2(f->d_gpartC, (long)L.n_gradC, n_part, f->d_gsrcC, f->d_gzeroC, f->n_gzeroC, grad, st, sq_for(f, L)));
  return SF_OK;
}

int sf_train_loss_grad(sf_flow* f, const float* flat, const float* theta, const float* x, const long long* idx, long B,
                       float grad_scale, const float* weights, float* loss, double* loss_sum, float* grad, float* dctx,
                       hipStream_t st) {
  const SfLayout& L = f->L;
  if (f->nsf1) {  // one-parameter NSF: T context MLPs + a scalar spline chain (sf_nsf1.hip); the handle keeps the vector it was given
    if (dctx) return sf_fail(SF_ERR_INVALID, "the one-parameter NSF has no context-gradient path");
    hipError_t e = hipMemcpyAsync(f->d_flat, flat, (size_t)L.n_params * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return sf_fail(SF_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    return sf_nsf1_loss_grad(f->nsf1, flat, theta, x, idx, B, grad_scale, weights, loss, loss_sum, grad, st);
  }
  if (f->nsfar) {   // (records the two events itself, around its flow kernel)
    if (dctx) return sf_fail(SF_ERR_INVALID, "the autoregressive NSF has no context-gradient path");
    int rc = train_events(f);
    if (rc) return rc;
    const bool p = f->profiling;
    rc = sf_nsfar_loss_grad(f->nsfar, flat, theta, x, idx, B, grad_scale, weights, loss, loss_sum, grad, st,
                            p ? f->ev_train[0].get() : nullptr, p ? f->ev_train[1].get() : nullptr);
    if (!rc && p) f->ev_train_valid = true;
    return rc;
  }
  const bool coop_maf = B > 0 && sf_trainc_eligible(L, dctx != nullptr);
  const bool coop_nsf = B > 0 && !coop_maf && sf_nsfc_eligible(L, dctx != nullptr);
  if (coop_maf || coop_nsf) return coop_loss_grad(f, coop_nsf, flat, theta, x, idx, B, grad_scale, weights, loss, loss_sum, grad, dctx, st);
  int rc = ensure_train(f);
  if (rc) return rc;
  const SfDev& v = L.dev;
  const long waves = (B + 31) / 32;
  const long tiles_per_wave = (long)v.T * (v.kind == SF_MAF ? ((v.NB + 1) * v.HT + 1) : (2 + (3 * v.NB + 1) * v.HT));
  const long act_per_wave = tiles_per_wave * 4 * 64;  // float4
  const size_t need = (size_t)waves * act_per_wave * 4;
  SF_TRY_SET(f->d_act.grow(need));
  // gradient accumulation: one replica per tile + plain stores (bitwise reproducible, and cheaper than atomics) up to
  // 16 tiles (batch 512: the reference's batch sizes), or whenever SF_DETERMINISTIC=1 and the replicas fit 2 GiB
  // (batch 2048: +15 % step time for zeroing and summing 64 replicas); else per-XCD replicas + f32 atomics
  static int force_det = -1;
  if (force_det < 0) { const char* e = std::getenv("SF_DETERMINISTIC"); force_det = e ? std::atoi(e) : 0; }
  const bool det = waves > 0 && (waves <= 16 || (force_det == 1 && (size_t)waves * L.n_packed * sizeof(float) <= ((size_t)2 << 30)));
  const int copies = det ? (int)waves : SF_GCOPIES;
  SF_TRY_SET(f->d_gpacked.grow((size_t)copies * L.n_packed));
  {
    const long n4 = (dctx && B > 0) ? B * (long)L.dev.C : 0;
    const long n5 = f->d_packed16 ? (long)L.n_packed16 : 0;
    const long n6 = f->d_packed16B ? (long)L.n_packed16B : 0;
    const long tot = (long)L.n_packed + (long)L.n_packedT + n4 + n5 + n6;
    hipLaunchKernelGGL(k_train_prep, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, flat, f->d_s1, f->d_s2, f->d_packed,
                       (long)L.n_packed, f->d_t1, f->d_t2, f->d_packedT, (long)L.n_packedT, f->d_gpacked, copies, dctx, n4,
                       f->d_s16a, f->d_s16b, f->d_packed16, n5, f->d_s16B, f->d_packed16B, n6, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, (float*)nullptr, 0L);
    SF_TRY_SET(hipGetLastError());
  }
  f->packed16_stale = false;
  f->wp_stale = true;
  if (L.n_packedB > 0) SF_TRY_SET(sf_launch_pack_bf16(flat, f->d_bsrc, f->d_packedB, (long)L.n_packedB, st));
  if (B > 0) {
    SfTrainArgs a;
    a.theta = theta; a.x = x; a.idx = idx; a.loss_sum = loss_sum; a.B = B; a.w = grad_scale; a.wts = weights; a.loss = loss; a.dctx = dctx; a.gimg = f->d_gpacked; a.gimg_stride = (long)L.n_packed; a.det = det ? 1 : 0;
    a.act = reinterpret_cast<float4*>(f->d_act.get()); a.act_per_wave = act_per_wave;
    const SfDev m = f->dev();
    const bool maf = m.kind == SF_MAF;
    rc = bracketed(f, st, [&]() -> int {
      switch (m.HT) {
        case 1: SF_TRY_SET(maf ? sf_launch_maf_train_h1(m, a, st) : sf_launch_nsf_train_h1(m, a, st)); break;
        case 2: SF_TRY_SET(maf ? sf_launch_maf_train_h2(m, a, st) : sf_launch_nsf_train_h2(m, a, st)); break;
        case 3: SF_TRY_SET(maf ? sf_launch_maf_train_h3(m, a, st) : sf_launch_nsf_train_h3(m, a, st)); break;
        case 4: SF_TRY_SET(maf ? sf_launch_maf_train_h4(m, a, st) : sf_launch_nsf_train_h4(m, a, st)); break;
        default: return sf_fail(SF_ERR_INVALID, "bad HT");
      }
      return SF_OK;
    });
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_grad_gather, dim3((unsigned)((L.n_params + 255) / 256)), dim3(256), 0, st,
                     f->d_gpacked, (long)L.n_packed, copies, f->d_gdst, grad, (long)L.n_params);
  SF_TRY_SET(hipGetLastError());
  return SF_OK;
}
