// sf_coop_tile.h -- what the two cooperative 16-row training kernels share: k_maf_trainc (sf_trainc.hip) and k_nsf_trainc
// (sf_nsfc.hip).  Register tiles, the transposed LDS tile, the LDS-only barrier, the laundered argument block and the finish of a
// weight-gradient block.  Everything here is __forceinline__ and ends up inside the kernels' own bodies; what the kernels do NOT
// share (their MFMA step helpers with different k-step skipping, the *_dw_jobs readers of two different delta layouts) stays in
// their files ("Cooperative trainers: what is shared").
// Tile = 16 rows x 16 samples in 4 VGPRs: lane l = sample (l & 15) + 16 * row group (l >> 4), register r = row 4 * (l >> 4) + r --
// the C/D layout of v_mfma_f32_16x16x4_f32 and the B-operand order of the next layer.
#pragma once
#include <hip/hip_runtime.h>

#include "sf_device.h"
#include "sf_fixacc.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define SF_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// a lane's four registers of a tile from / to 16 contiguous bytes (LDS: one ds_read_b128 / ds_write_b128)
__device__ __forceinline__ f32x4 coop_ld4(const float* p) {
  const float4 b = *reinterpret_cast<const float4*>(p);
  f32x4 r;
  r[0] = b.x; r[1] = b.y; r[2] = b.z; r[3] = b.w;
  return r;
}
__device__ __forceinline__ void coop_st4(float* p, const f32x4 v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ f32x4 coop_zero() {
  f32x4 z;
  z[0] = 0.f; z[1] = 0.f; z[2] = 0.f; z[3] = 0.f;
  return z;
}
// weight fragment of block (a, b) of a [.][nb] block array
// (block index first, as a wave-uniform 64-bit base; the lane enters as an unsigned 32-bit offset: the load then takes
//  the SGPR-base + VGPR-offset form and every fragment address shares ONE per-lane register)
__device__ __forceinline__ float4 coop_frag(const float* wp, int nb, int a, int b, int lane) {
  const float4* base = reinterpret_cast<const float4*>(wp) + (a * nb + b) * 64;
  return base[(unsigned)lane];
}

// Transposed LDS tile, the A / B operand of a weight-gradient product (k = sample): element (row, sample) at
// (sample >> 2) * 68 + row * 4 + (sample & 3); lane l = 16 kk + i reads row i, samples 4 kk .. 4 kk + 3 with one ds_read_b128 at
// kk * 68 + i * 4.
//   (round 4: sample groups of 68 floats, not 64 -- COOP_TT = 272 floats per tile: the four ds_write_b32 of a lane then hit
//   4 (s >> 2) + 16 g4 + (s & 3) + 4 r = 64 different banks; with 64 the lanes s, s + 4, s + 8, s + 12 collided and 41 % of
//   k_maf_trainc's LDS cycles were bank conflicts, profiles/r03_pmc_summary.json -- 37 % of k_nsf_trainc's)
constexpr int COOP_TT = 272;
__device__ __forceinline__ int coop_T_rd(int lane) { return (lane >> 4) * 68 + (lane & 15) * 4; }
__device__ __forceinline__ void coop_put_T(float* tile, const f32x4 v, int s, int g4) {
  float* p = tile + (s >> 2) * 68 + (s & 3) + 16 * g4;
  p[0] = v[0]; p[4] = v[1]; p[8] = v[2]; p[12] = v[3];
}

// Workgroup barrier for the LDS hand-overs.  __syncthreads() carries a workgroup-scope fence that also drains the
// wave's outstanding GLOBAL loads (s_waitcnt vmcnt(0)): every weight fragment issued a phase ahead would be waited for
// at the very next barrier.  The exchanged data is LDS only: wait for the wave's own LDS operations, then s_barrier.
__device__ __forceinline__ void coop_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  SF_FUZZ();
}

// The argument block is read through the kernarg segment pointer, laundered where a phase starts: descriptor fields
// are then scalar loads next to their use (scalar-cache hits) instead of ~80 SGPRs held -- and spilled -- for the
// life of the kernel (same device as k_maf_samp16).
template <class Args>
__device__ __forceinline__ const Args& sf_coop_args() {
  auto kp = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return *(const Args*)kp;
}

// One weight-gradient block: acc = sum over the workgroup's samples of delta[ot rows][s] * in[it rows][s], accumulated by the
// kernel's own *_dw_jobs (which knows the layout its delta tiles are in) and finished here.  gb != nullptr: also the bias
// gradient of tile ot (bs = this lane's share of the row sums of delta).
struct CoopJob {
  const float* Xd;  // delta tiles (MAF: transposed, NSF: padded B layout)
  const float* Ti;  // transposed input tiles
  float* gw;        // gradient block (256 floats)
  float* gb;        // bias gradient rows of tile ot (or null)
  int ot, it;
};
// A.mode 0: plain store (first chunk of the workgroup), 1: add to the workgroup's partial (later chunks), 2: f32 atomics into
// the XCD's replica -- compiled in only with F32_ATOMICS (NSF) --, 3: fixed-point (int64) atomics into it (sf_fixacc.h)
template <bool F32_ATOMICS>
__device__ __forceinline__ void coop_dw_finish(const CoopJob& J, f32x4 acc, float bs, const SfAcc& A, int lane) {
  if (F32_ATOMICS && A.mode == 2) {
    float* q = reinterpret_cast<float*>(A.fix) + (J.gw - A.base);
#pragma unroll
    for (int r = 0; r < 4; ++r) sf_l2_add(q + r * 64 + lane, acc[r]);
  } else if (A.mode == 3) {
    long long* q = A.fix + (J.gw - A.base);
#pragma unroll
    for (int r = 0; r < 4; ++r) sf_fix_add(q + r * 64 + lane, acc[r]);
  } else {
    if (A.mode == 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] += J.gw[r * 64 + lane];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) J.gw[r * 64 + lane] = acc[r];
  }
  if (J.gb) {
    bs += __shfl_xor(bs, 16, 64);
    bs += __shfl_xor(bs, 32, 64);
    if (lane < 16) {
      if (F32_ATOMICS && A.mode == 2) sf_l2_add(reinterpret_cast<float*>(A.fix) + (J.gb - A.base) + J.ot * 16 + lane, bs);
      else if (A.mode == 3) sf_fix_add(A.fix + (J.gb - A.base) + J.ot * 16 + lane, bs);
      else J.gb[J.ot * 16 + lane] = A.mode == 1 ? J.gb[J.ot * 16 + lane] + bs : bs;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// compute units of the current device, asked once per process (256 when the runtime does not say): the grids of both kernels
// are capped at one or two workgroups per CU
inline int sf_coop_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t pr;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
              ? pr.multiProcessorCount : 256;
  }
  return cus;
}

#if defined(SF_TRC_TRACE) || defined(SF_NSC_TRACE)
#include <cstdio>
#include <vector>
// Developer builds (-DSF_TRC_TRACE, -DSF_NSC_TRACE): launch(b) runs the kernel on a copy of the arguments whose `trace` points at
// [waves][slots] zeroed cycle stamps, which workgroup 0 fills (SF_TC / SF_NC); every eighth call prints them.
template <class Args, class Launch>
static hipError_t sf_coop_trace_launch(const Args& a, int grid, hipStream_t st, int waves, int slots, const char* tag, Launch launch) {
  static unsigned long long* d_tr = nullptr;
  const size_t n = (size_t)waves * slots;
  if (!d_tr && hipMalloc(&d_tr, n * 8) != hipSuccess) return hipErrorOutOfMemory;
  (void)hipMemsetAsync(d_tr, 0, n * 8, st);
  Args b = a;
  b.trace = d_tr;
  launch(b);
  (void)hipStreamSynchronize(st);
  std::vector<unsigned long long> h(n);
  (void)hipMemcpy(h.data(), d_tr, n * 8, hipMemcpyDeviceToHost);
  static int calls = 0;
  if (++calls % 8 == 0) {
    fprintf(stderr, "[%s trace] B=%ld grid=%d (units of 100 cycles since stamp 0 of wave 0)\n", tag, a.B, grid);
    for (int w = 0; w < waves; ++w) {
      fprintf(stderr, "  wave %d:", w);
      for (int i = 0; i < slots; ++i)
        if (h[(size_t)w * slots + i]) fprintf(stderr, " %d:%.1f", i, (double)(long long)(h[(size_t)w * slots + i] - h[0]) * 0.01);
      fprintf(stderr, "\n");
    }
  }
  return hipGetLastError();
}
#endif
