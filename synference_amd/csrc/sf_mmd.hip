// sf_mmd.hip -- the kernel sums of the MMD misspecification test (synference_amd/misspecification.py):
// Gaussian-kernel sums of one set of rows against another (sf_rbf_rowsum) and over the pairs of many index subsets of one set
// (sf_rbf_subset_sums).  With r_i = sum_{j != i} k(z_i, z_j) over the N training rows, one N x N pass and one m x m pass per
// shuffle give every block sum of the permutation null:  A_s = pair_sum, Cx_s = picked_rowsum - A_s, B_s = R - A_s - 2 Cx_s.
//
// A term is k(a, b) = exp2(d2(a, b) * c2), d2 the squared distance of sf_ood_tile.h (the bits of tests/mmd_model.py), the
// product rounded to fp32, v_exp_f32, a NaN term counted as 0; c2 = -0.5 / scale^2 * log2(e) <= 0 comes from the host.  Terms are
// added in fp64 in an order that the shapes alone fix: no atomics, two calls give the same bits.
//
// sf_rbf_rowsum is k_kde_part without the running minimum: one thread per query, its row in registers, the base cut into S
// contiguous splits (grid.y) and streamed through LDS in chunks of 128 rows; per (query, split) the terms in ascending row
// order, the splits added in ascending order by k_rbf_row_merge.  exclude_self: base row self_offset + q is skipped -- by
// position, never by value.
//
// sf_rbf_subset_sums: a set is m positions of idx; the m x m block is cut into tiles of 256 x 256 positions and only the
// tiles (i, j) with j <= i are visited.  A workgroup holds the 256 gathered rows of tile row i in registers and streams the
// gathered rows of tiles j0 .. j1 (G tiles per workgroup; G = 1 up to m = 16384) through LDS in chunks of 128, each chunk
// gathered ONCE into the interleaved image of sf_ood_tile.h.  Below the diagonal every term stands for the ordered pairs (a, b)
// and (b, a): the thread's sum is doubled (exact); on the diagonal tile both orders are visited and position a == b is skipped.
// The workgroup adds its 256 sums with the fixed tree of sf_block.h and writes ONE partial; k_rbf_subset_merge adds a set's
// partials in ascending (i, j) order and the picked row sums in ascending position order.  Entries of idx outside [0, N) are
// clamped: the device never reads out of bounds (the caller's contract, checked in Python, is that there are none).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "sf_block.h"
#include "sf_internal.h"
#include "sf_ood_tile.h"
#include "sf_scratch.h"

#define SF_MMD_QT 256          // queries (rows of a tile) per workgroup
#define SF_MMD_SMAX 256        // splits of the base in sf_rbf_rowsum
#define SF_MMD_JSMAX 64        // workgroups per tile row in sf_rbf_subset_sums
#define SF_MMD_PART_BYTES (64ull << 20)   // partials of the sets of one launch

// the two terms of a row pair; a NaN (a NaN distance, or inf * 0 of a padding row when c2 == 0) becomes 0
__device__ __forceinline__ sf_f2 sf_mmd_terms(sf_f2 d, float c2) {
  sf_f2 e;
  e.x = __builtin_fmaxf(__builtin_amdgcn_exp2f(d.x * c2), 0.f);
  e.y = __builtin_fmaxf(__builtin_amdgcn_exp2f(d.y * c2), 0.f);
  return e;
}

// ---- rows of one set against another -----------------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(256) void k_rbf_row_part(const float* __restrict__ base, long N, int C, unsigned magic,
                                                      const float* __restrict__ query, long M, float c2, int exclude_self,
                                                      long self_offset, long split_len, int S, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float* s_b = (float*)s_raw;
  const int tid = threadIdx.x, QT = blockDim.x;
  const long m = (long)blockIdx.x * QT + tid;
  const bool live = m < M;
  const int s = blockIdx.y;
  const long sb = (long)s * split_len;
  const long se = sb + split_len < N ? sb + split_len : N;
  const long self = exclude_self ? self_offset + m : -1;
  float q[CP];
  sf_ood_load_query<CP>(query, m, live, C, q);
  double sum = 0.0;
  for (long r0 = sb; r0 < se; r0 += SF_OOD_CH) {
    __syncthreads();
    sf_ood_load_chunk<CP>(base, r0, se, C, magic, s_b);   // rows past the end: +inf, a zero term
    __syncthreads();
    for (int p = 0; p < SF_OOD_CH / 2; ++p) {
      sf_f2 e = sf_mmd_terms(sf_ood_d2pair<CP>(q, s_b, p), c2);
      const long r = r0 + 2 * p;
      e.x = r == self ? 0.f : e.x;
      e.y = r + 1 == self ? 0.f : e.y;
      sum += (double)e.x;
      sum += (double)e.y;
    }
  }
  if (live) part[m * S + s] = sum;
}

__global__ __launch_bounds__(256) void k_rbf_row_merge(const double* __restrict__ part, long M, int S, double* __restrict__ out) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  double tot = 0.0;
  for (int s = 0; s < S; ++s) tot += part[m * S + s];
  out[m] = tot;
}

// ---- the pairs of index subsets ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sf_mmd_clamp(int32_t v, long N) { return v < 0 ? 0 : ((long)v >= N ? (int)(N - 1) : (int)v); }

// grid (nt * JS, sets of this launch); workgroup (i, js) of a set: tile row i against tiles [js G, min(js G + G, i + 1))
template <int CP>
__global__ __launch_bounds__(256) void k_rbf_subset_part(const float* __restrict__ rows, long N, int C, unsigned magic,
                                                         const int32_t* __restrict__ idx, long m, float c2, int JS, int G,
                                                         double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ int s_i[SF_OOD_CH];
  __shared__ double s_red[SF_MMD_QT];
  float* s_b = (float*)s_raw;
  const int tid = threadIdx.x;
  const long i = blockIdx.x / JS, js = blockIdx.x - i * JS;
  const long j0 = js * G;
  if (j0 > i) return;   // (uniform) above the diagonal: no partial, the merge skips it too
  const long j1 = j0 + G < i + 1 ? j0 + G : i + 1;
  const int32_t* id = idx + (long)blockIdx.y * m;
  const long a = i * SF_MMD_QT + tid;
  const bool live = a < m;
  float q[CP];
  sf_ood_load_query<CP>(rows, live ? (long)sf_mmd_clamp(id[a], N) : 0, live, C, q);
  double off = 0.0, diag = 0.0;
  for (long j = j0; j < j1; ++j) {
    for (long b0 = j * SF_MMD_QT; b0 < (j + 1) * SF_MMD_QT && b0 < m; b0 += SF_OOD_CH) {
      __syncthreads();   // the previous chunk has been read
      if (tid < SF_OOD_CH) s_i[tid] = b0 + tid < m ? sf_mmd_clamp(id[b0 + tid], N) : -1;
      if (CP != C)
        for (int e = tid; e < SF_OOD_CH * CP; e += SF_MMD_QT) s_b[e] = 0.f;
      __syncthreads();
      for (int e = tid; e < SF_OOD_CH * C; e += SF_MMD_QT) {   // the chunk's rows, gathered once
        const int r = (int)(((unsigned)e * magic) >> 20);      // e / C
        const int c = e - r * C;
        const int src = s_i[r];
        s_b[((r >> 1) * CP + c) * 2 + (r & 1)] = src >= 0 ? rows[(long)src * C + c] : __builtin_inff();
      }
      __syncthreads();
      if (j == i) {   // (uniform) the diagonal tile: both orders of a pair are visited, the position itself is not
        for (int p = 0; p < SF_OOD_CH / 2; ++p) {
          sf_f2 e = sf_mmd_terms(sf_ood_d2pair<CP>(q, s_b, p), c2);
          const long b = b0 + 2 * p;
          e.x = b == a ? 0.f : e.x;
          e.y = b + 1 == a ? 0.f : e.y;
          diag += (double)e.x;
          diag += (double)e.y;
        }
      } else {
        for (int p = 0; p < SF_OOD_CH / 2; ++p) {
          const sf_f2 e = sf_mmd_terms(sf_ood_d2pair<CP>(q, s_b, p), c2);
          off += (double)e.x;
          off += (double)e.y;
        }
      }
    }
  }
  const double tot = sf_block_sum<double>(live ? 2.0 * off + diag : 0.0, s_red);
  if (tid == 0) part[((long)blockIdx.y * gridDim.x) + blockIdx.x] = tot;
}

// one workgroup per set: its partials in ascending (i, js) order, then the row sums of its positions in ascending order; the
// values come through LDS 256 at a time and thread 0 adds them
__global__ __launch_bounds__(256) void k_rbf_subset_merge(const double* __restrict__ part, long nE, int JS, int G,
                                                          const int32_t* __restrict__ idx, long m, long N,
                                                          const double* __restrict__ rowsum, double* __restrict__ pair_sum,
                                                          double* __restrict__ picked) {
  __shared__ double s_v[256];
  const int tid = threadIdx.x;
  const long s = blockIdx.x;
  double tot = 0.0;
  for (long e0 = 0; e0 < nE; e0 += 256) {
    const long e = e0 + tid;
    const long i = e / JS, js = e - i * JS;
    __syncthreads();
    s_v[tid] = (e < nE && js * G <= i) ? part[s * nE + e] : 0.0;   // (x + 0 = x: skipped slots do not move the sum)
    __syncthreads();
    if (tid == 0)
      for (int t = 0; t < 256; ++t) tot += s_v[t];
  }
  if (tid == 0) pair_sum[s] = tot;
  if (!rowsum) return;
  tot = 0.0;
  for (long a0 = 0; a0 < m; a0 += 256) {
    const long a = a0 + tid;
    __syncthreads();
    s_v[tid] = a < m ? rowsum[sf_mmd_clamp(idx[s * m + a], N)] : 0.0;
    __syncthreads();
    if (tid == 0)
      for (int t = 0; t < 256; ++t) tot += s_v[t];
  }
  if (tid == 0) picked[s] = tot;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {
SfScratch g_mmd_scratch;   // sf_scratch.h: one for both entry points

template <int CP>
struct SfRbfRowLaunch {
  static void go(dim3 grid, size_t lds, hipStream_t st, const float* base, long N, int C, unsigned magic, const float* query,
                 long M, float c2, int ex, long so, long sl, int S, double* part) {
    hipLaunchKernelGGL(k_rbf_row_part<CP>, grid, dim3(SF_MMD_QT), lds, st, base, N, C, magic, query, M, c2, ex, so, sl, S, part);
  }
};
template <int CP>
struct SfRbfSubsetLaunch {
  static void go(dim3 grid, size_t lds, hipStream_t st, const float* rows, long N, int C, unsigned magic, const int32_t* idx,
                 long m, float c2, int JS, int G, double* part) {
    hipLaunchKernelGGL(k_rbf_subset_part<CP>, grid, dim3(SF_MMD_QT), lds, st, rows, N, C, magic, idx, m, c2, JS, G, part);
  }
};

bool sf_mmd_bad_c2(float c2) { return !(c2 <= 0.f) || std::isinf(c2); }
}  // namespace

extern "C" int sf_rbf_rowsum(const float* base, int64_t N, int32_t C, const float* query, int64_t M, float c2,
                             int32_t exclude_self, int64_t self_offset, double* out, void* stream) {
  if (!base || !query || !out) {
    sf_set_error("sf_rbf_rowsum: null argument");
    return SF_ERR_INVALID;
  }
  if (C < 1 || C > SF_OOD_CMAX || N < 1 || N > 0x7fffffffll || M < 0 || (exclude_self != 0 && exclude_self != 1) ||
      self_offset < 0 || (exclude_self && self_offset + M > N) || sf_mmd_bad_c2(c2)) {
    sf_set_error("sf_rbf_rowsum: need 1 <= C <= 64, 1 <= N < 2^31, M >= 0, c2 <= 0 and finite, exclude_self 0 or 1, "
                 "0 <= self_offset and self_offset + M <= N with exclude_self");
    return SF_ERR_INVALID;
  }
  if (M == 0) return SF_OK;
  hipStream_t st = (hipStream_t)stream;
  // splits of the base so that about 2048 workgroups exist, at least 8 chunks each: the shapes alone decide
  const int n_qt = (int)((M + SF_MMD_QT - 1) / SF_MMD_QT);
  long S = (2048 + n_qt - 1) / n_qt;
  const long nch = (long)((N + SF_OOD_CH - 1) / SF_OOD_CH);
  const long smax = nch / 8 > 1 ? nch / 8 : 1;
  S = S > smax ? smax : S;
  S = S > SF_MMD_SMAX ? SF_MMD_SMAX : S;
  const long split_len = (nch + S - 1) / S * SF_OOD_CH;
  S = (long)((N + split_len - 1) / split_len);
  const int CP = (C + 3) & ~3;
  SfScratchCall ws(g_mmd_scratch, "sf_rbf_rowsum", st);
  const int sub_part = ws.add((size_t)M * S * 8);
  if (int rc = ws.reserve()) return rc;
  double* part = ws.get<double>(sub_part);
  if (int rc = ws.check()) return rc;
  sf_ood_dispatch<SfRbfRowLaunch>(CP, dim3((unsigned)n_qt, (unsigned)S), (size_t)SF_OOD_CH * CP * 4, st, base, (long)N, (int)C,
                                  (1u << 20) / (unsigned)C + 1u, query, (long)M, c2, (int)exclude_self, (long)self_offset,
                                  split_len, (int)S, part);
  hipLaunchKernelGGL(k_rbf_row_merge, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const double*)part, (long)M, (int)S,
                     out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ws.fail("launch", e);
  return ws.finish();
}

extern "C" int sf_rbf_subset_sums(const float* rows, int64_t N, int32_t C, const int32_t* idx, int64_t n_sets, int64_t m,
                                  float c2, const double* rowsum, double* pair_sum, double* picked_rowsum, void* stream) {
  if (!rows || !idx || !pair_sum || ((rowsum == nullptr) != (picked_rowsum == nullptr))) {
    sf_set_error("sf_rbf_subset_sums: null argument (rowsum and picked_rowsum are given together or not at all)");
    return SF_ERR_INVALID;
  }
  if (C < 1 || C > SF_OOD_CMAX || N < 1 || N > 0x7fffffffll || n_sets < 0 || m < 2 || m > N || sf_mmd_bad_c2(c2)) {
    sf_set_error("sf_rbf_subset_sums: need 1 <= C <= 64, 1 <= N < 2^31, n_sets >= 0, 2 <= m <= N, c2 <= 0 and finite");
    return SF_ERR_INVALID;
  }
  if (n_sets == 0) return SF_OK;
  hipStream_t st = (hipStream_t)stream;
  const long nt = (long)((m + SF_MMD_QT - 1) / SF_MMD_QT);
  const int G = (int)((nt + SF_MMD_JSMAX - 1) / SF_MMD_JSMAX);
  const int JS = (int)((nt + G - 1) / G);
  const long nE = nt * JS;   // partial slots of one set (those above the diagonal stay unused)
  long per = (long)(SF_MMD_PART_BYTES / ((size_t)nE * 8));
  per = per < 1 ? 1 : (per > 65535 ? 65535 : per);
  per = per > n_sets ? (long)n_sets : per;
  const int CP = (C + 3) & ~3;
  SfScratchCall ws(g_mmd_scratch, "sf_rbf_subset_sums", st);
  const int sub_part = ws.add((size_t)per * nE * 8);
  if (int rc = ws.reserve()) return rc;
  double* part = ws.get<double>(sub_part);
  if (int rc = ws.check()) return rc;
  for (int64_t s0 = 0; s0 < n_sets; s0 += per) {   // (launches on one stream: the partials are reused in order)
    const long ns = n_sets - s0 < per ? (long)(n_sets - s0) : per;
    sf_ood_dispatch<SfRbfSubsetLaunch>(CP, dim3((unsigned)nE, (unsigned)ns), (size_t)SF_OOD_CH * CP * 4, st, rows, (long)N, (int)C,
                                       (1u << 20) / (unsigned)C + 1u, idx + s0 * m, (long)m, c2, JS, G, part);
    hipLaunchKernelGGL(k_rbf_subset_merge, dim3((unsigned)ns), dim3(256), 0, st, (const double*)part, nE, JS, G, idx + s0 * m,
                       (long)m, (long)N, rowsum, pair_sum + s0, picked_rowsum ? picked_rowsum + s0 : nullptr);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ws.fail("launch", e);
  return ws.finish();
}
