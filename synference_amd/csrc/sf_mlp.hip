// sf_mlp.hip -- the fully connected embedding net (context path) on the
// register-tile engine: forward, and backward (weight gradients through the same LDS-transposed MFMA
// + f32-atomic gradient image as the flow training kernels).  Standardisation of x is fused in.
#include <hip/hip_runtime.h>

#include <string>

#include "sf_train_kernels.h"

#define SF_MLP_DET_WAVES 16   // 32-row tiles that get a gradient image of their own (sf_mlp_backward)

struct SfMlpArgs {
  const float* x;
  const float* dout;  // backward only
  float* out;         // forward only
  long B;
  float* gimg;
  long gimg_stride;   // backward: floats between the waves' own gradient images; 0 = one image shared by all waves (f32 atomics)
  float4* act;
  long act_per_wave;
};

__device__ __forceinline__ float sf_act_f(int act, float z) {
  if (act == SF_ACT_SILU) return z * sf_sigmoid(z);
  if (act == SF_ACT_RELU) return fmaxf(z, 0.f);
  return sf_tanh(z);
}
__device__ __forceinline__ float sf_act_d(int act, float z) {
  if (act == SF_ACT_SILU) {
    const float s = sf_sigmoid(z);
    return s * (1.f + z * (1.f - s));
  }
  if (act == SF_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  const float t = sf_tanh(z);
  return 1.f - t * t;
}

// input tile kt of the standardised features
__device__ __forceinline__ void sf_mlp_in_tile(f32x16 (&ct)[1][1], const float* __restrict__ xr, const SfMlpDev& m,
                                               int kt, int h) {
  const int pad = ((m.n_in + 3) / 4) * 4;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rho = kt * 32 + sf_row(r, h);
    const bool ok = rho < m.n_in;
    const int rr = ok ? rho : 0;
    const float v = (xr[rr] - m.cst[rr]) / m.cst[pad + rr];
    ct[0][0][r] = ok ? v : 0.f;
  }
}

// z_0 .. z_{L-1} (pre-activations); z[L-1] is the output.  STASH: write z_l (l < L-1) to the stash.
template <int HT, bool STASH>
__device__ __forceinline__ void sf_mlp_forward(const SfMlpDev& m, const float* __restrict__ xr, f32x16 (&z)[HT][1],
                                               float4* stash, int lane) {
  const int h = lane >> 5;
  sf_init_bias<HT, 1>(z, m.packed + m.o_b[0], h);
  for (int kt = 0; kt * 4 < m.nG[0]; ++kt) {
    f32x16 ct[1][1];
    sf_mlp_in_tile(ct, xr, m, kt, h);
    sf_mm_acc<HT, 1, 1, false, false, true>(z, ct, m.packed + m.o_w[0], m.nG[0], kt * 4, min(4, m.nG[0] - kt * 4), lane);
  }
#pragma unroll
  for (int l = 1; l < SF_MLP_LMAX; ++l) {
    if (l < m.L) {
      f32x16 a[HT][1];
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) {
        if (STASH) sf_stash_store(stash, (l - 1) * HT + mt, z[mt][0], lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) a[mt][0][r] = sf_act_f(m.act, z[mt][0][r]);
      }
      sf_init_bias<HT, 1>(z, m.packed + m.o_b[l], h);
      sf_mm_acc<HT, 1, HT, false, false, true>(z, a, m.packed + m.o_w[l], m.nG[l], 0, m.nG[l], lane);
    }
  }
}

template <int HT>
__global__ __launch_bounds__(256) void k_mlp_fwd(SfMlpDev m, SfMlpArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const long base = ((long)blockIdx.x * 4 + wave) * 32;
  if (base >= a.B) return;
  const long row = base + c;
  const bool valid = row < a.B;
  const float* xr = a.x + (valid ? row : a.B - 1) * m.n_in;
  f32x16 z[HT][1];
  sf_mlp_forward<HT, false>(m, xr, z, nullptr, lane);
  if (valid) {
#pragma unroll
    for (int mt = 0; mt < HT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = mt * 32 + sf_row(r, h);
        if (f < m.n_out) a.out[row * m.n_out + f] = z[mt][0][r];
      }
  }
}

template <int HT>
__global__ __launch_bounds__(256) void k_mlp_bwd(SfMlpDev m, SfMlpArgs a) {
  extern __shared__ float lds_all[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const long wid = (long)blockIdx.x * 4 + wave;
  const long base = wid * 32;
  if (base >= a.B) return;
  float* lds = lds_all + wave * (2 * HT) * SF_TL;
  float4* stash = a.act + wid * a.act_per_wave;
  float* const gimg = a.gimg + wid * a.gimg_stride;   // (its own zeroed image: every address is added to once)
  const long row = base + c;
  const bool valid = row < a.B;
  const long ii = valid ? row : a.B - 1;
  const float* xr = a.x + ii * m.n_in;
  {
    f32x16 z[HT][1];
    sf_mlp_forward<HT, true>(m, xr, z, stash, lane);
  }
  f32x16 d[HT][1];  // dL/d z_l, starting from the output gradient
#pragma unroll
  for (int mt = 0; mt < HT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = mt * 32 + sf_row(r, h);
      d[mt][0][r] = (valid && f < m.n_out) ? a.dout[row * m.n_out + f] : 0.f;
    }
#pragma unroll
  for (int ll = 0; ll < SF_MLP_LMAX - 1; ++ll) {
    const int l = SF_MLP_LMAX - 1 - ll;  // 3, 2, 1
    if (l < m.L) {
      f32x16 zin[HT][1], ain[HT][1];
#pragma unroll
      for (int mt = 0; mt < HT; ++mt) {
        sf_stash_load(stash, (l - 1) * HT + mt, zin[mt][0], lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) ain[mt][0][r] = sf_act_f(m.act, zin[mt][0][r]);
      }
      sf_grad_w_local<HT, HT>(lds, d, ain, gimg + m.o_w[l], gimg + m.o_b[l], m.nG[l], 0, m.nG[l], lane);
      f32x16 din[HT][1];
#pragma unroll
      for (int mt = 0; mt < HT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) din[mt][0][r] = 0.f;
      sf_mm_acc<HT, 1, HT, false, false, true>(din, d, m.packedT + m.oT_w[l], m.nGo[l], 0, m.nGo[l], lane);
#pragma unroll
      for (int mt = 0; mt < HT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) d[mt][0][r] = din[mt][0][r] * sf_act_d(m.act, zin[mt][0][r]);
    }
  }
  for (int kt = 0; kt * 4 < m.nG[0]; ++kt) {
    f32x16 ct[1][1];
    sf_mlp_in_tile(ct, xr, m, kt, h);
    sf_grad_w_local<HT, 1>(lds, d, ct, gimg + m.o_w[0], kt == 0 ? gimg + m.o_b[0] : nullptr, m.nG[0], kt * 4,
                     min(4, m.nG[0] - kt * 4), lane);
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct SfMlpBufs {   // built once, all or nothing (mlp_ensure)
  SfBuf<float> d_packed, d_packedT, d_cst;
  SfBuf<int32_t> d_s1, d_s2, d_t1, d_t2, d_gdst;
};
struct sf_mlp : SfMlpBufs {
  SfMlpLayout L;
  bool dev_ready = false;
  SfBuf<float> d_act, d_gimg;   // grown per call
  SfMlpDev dev() const {
    SfMlpDev v = L.dev;
    v.packed = d_packed; v.packedT = d_packedT; v.cst = d_cst;
    return v;
  }
};

__global__ void k_mlp_gather(const float* __restrict__ gimg, long stride, int copies, const int32_t* __restrict__ gdst,
                             float* __restrict__ grad, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = gdst[i];
  float v = 0.f;
  if (g >= 0)
    for (int c = 0; c < copies; ++c) v += gimg[(size_t)c * stride + g];   // fixed order over the waves' images
  grad[i] = v;
}

namespace {

int mlp_ensure(sf_mlp* m) {
  if (m->dev_ready) return SF_OK;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    sf_set_error("no HIP device visible: the embedding kernels have no CPU fallback");
    return SF_ERR_NO_DEVICE;
  }
  const SfMlpLayout& L = m->L;
  SfMlpBufs b;
  SF_TRY_SET(b.d_packed.alloc((size_t)L.n_packed));
  SF_TRY_SET(b.d_packedT.alloc(std::max<size_t>((size_t)L.n_packedT, 64)));
  SF_TRY_SET(b.d_cst.upload(L.cst));
  SF_TRY_SET(b.d_s1.upload(L.src1)); SF_TRY_SET(b.d_s2.upload(L.src2));
  SF_TRY_SET(b.d_t1.upload(L.srcT1)); SF_TRY_SET(b.d_t2.upload(L.srcT2));
  SF_TRY_SET(b.d_gdst.upload(L.gdst));
  static_cast<SfMlpBufs&>(*m) = std::move(b);
  m->dev_ready = true;
  return SF_OK;
}

template <int HT>
hipError_t launch_fwd(const SfMlpDev& d, const SfMlpArgs& a, hipStream_t st) {
  const long grid = ((a.B + 31) / 32 + 3) / 4;
  hipLaunchKernelGGL((k_mlp_fwd<HT>), dim3((unsigned)grid), dim3(256), 0, st, d, a);
  return hipGetLastError();
}
template <int HT>
hipError_t launch_bwd(const SfMlpDev& d, const SfMlpArgs& a, hipStream_t st) {
  const long grid = ((a.B + 31) / 32 + 3) / 4;
  const size_t shmem = (size_t)4 * (2 * HT) * SF_TL * sizeof(float);
  static SfAttrCache attr;
  int attr_dev;
  if (attr.need(attr_dev)) {
    hipError_t e = hipFuncSetAttribute((const void*)k_mlp_bwd<HT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    attr.set(attr_dev);
  }
  hipLaunchKernelGGL((k_mlp_bwd<HT>), dim3((unsigned)grid), dim3(256), shmem, st, d, a);
  return hipGetLastError();
}
}  // namespace

extern "C" {
int sf_mlp_create(const sf_mlp_desc* d, sf_mlp** out) {
  if (!d || !out) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  sf_mlp* m = new sf_mlp();
  if (!sf_build_mlp_layout(*d, m->L)) {
    sf_set_error(m->L.error);
    delete m;
    return SF_ERR_INVALID;
  }
  *out = m;
  return SF_OK;
}
void sf_mlp_destroy(sf_mlp* m) { delete m; }
int64_t sf_mlp_num_params(const sf_mlp* m) { return m ? m->L.n_params : 0; }

int sf_mlp_forward(sf_mlp* m, const float* flat, const float* x, int64_t B, float* out, void* stream) {
  if (!m || !flat) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  if (B == 0) return SF_OK;
  if (!x || !out || B < 0) { sf_set_error("bad argument"); return SF_ERR_INVALID; }
  int rc = mlp_ensure(m);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  SF_TRY_SET(sf_launch_pack(flat, m->d_s1, m->d_s2, m->d_packed, (long)m->L.n_packed, st));
  SfMlpArgs a{};
  a.x = x; a.out = out; a.B = B;
  const SfMlpDev d = m->dev();
  switch (d.HT) {
    case 1: SF_TRY_SET(launch_fwd<1>(d, a, st)); break;
    case 2: SF_TRY_SET(launch_fwd<2>(d, a, st)); break;
    case 3: SF_TRY_SET(launch_fwd<3>(d, a, st)); break;
    default: SF_TRY_SET(launch_fwd<4>(d, a, st)); break;
  }
  return SF_OK;
}

int sf_mlp_backward(sf_mlp* m, const float* flat, const float* x, const float* dout, int64_t B, float* grad,
                    void* stream) {
  if (!m || !flat || !grad) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  if (B > 0 && (!x || !dout)) { sf_set_error("null argument"); return SF_ERR_INVALID; }
  int rc = mlp_ensure(m);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const SfMlpLayout& L = m->L;
  const long waves = (B + 31) / 32;
  const long act_per_wave = (long)std::max(1, (L.dev.L - 1) * L.dev.HT) * 4 * 64;
  const size_t need = (size_t)std::max<long>(waves, 1) * act_per_wave * 4;
  SF_TRY_SET(m->d_act.grow(need));
  SF_TRY_SET(sf_launch_pack(flat, m->d_s1, m->d_s2, m->d_packed, (long)L.n_packed, st));
  if (L.n_packedT > 0) SF_TRY_SET(sf_launch_pack(flat, m->d_t1, m->d_t2, m->d_packedT, (long)L.n_packedT, st));
  // Gradient accumulation as in the 32-row flow kernels (sf_train.hip): up to SF_MLP_DET_WAVES tiles (batch 512) every 32-row wave
  // adds into a zeroed image of its own and the gather sums the images in tile order -- the same inputs give the same bits; above
  // that one shared image and f32 atomics.  (One shared image at every batch repeated to the bit only up to two waves, 64 rows.)
  const int copies = (waves >= 1 && waves <= SF_MLP_DET_WAVES) ? (int)waves : 1;
  SF_TRY_SET(m->d_gimg.grow((size_t)copies * (size_t)L.n_packed));
  SF_TRY_SET(hipMemsetAsync(m->d_gimg, 0, (size_t)copies * (size_t)L.n_packed * sizeof(float), st));
  if (B > 0) {
    SfMlpArgs a{};
    a.x = x; a.dout = dout; a.B = B; a.gimg = m->d_gimg; a.gimg_stride = copies > 1 ? (long)L.n_packed : 0;
    a.act = reinterpret_cast<float4*>(m->d_act.get()); a.act_per_wave = act_per_wave;
    const SfMlpDev d = m->dev();
    switch (d.HT) {
      case 1: SF_TRY_SET(launch_bwd<1>(d, a, st)); break;
      case 2: SF_TRY_SET(launch_bwd<2>(d, a, st)); break;
      case 3: SF_TRY_SET(launch_bwd<3>(d, a, st)); break;
      default: SF_TRY_SET(launch_bwd<4>(d, a, st)); break;
    }
  }
  hipLaunchKernelGGL(k_mlp_gather, dim3((unsigned)((L.n_params + 255) / 256)), dim3(256), 0, st, m->d_gimg, (long)L.n_packed, copies,
                     m->d_gdst, grad, (long)L.n_params);
  SF_TRY_SET(hipGetLastError());
  return SF_OK;
}
}  // extern "C"
