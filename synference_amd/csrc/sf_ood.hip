// sf_ood.hip -- the all-pairs work of the out-of-distribution check: exact brute-force k nearest neighbours (sf_knn) and the
// log of a Gaussian kernel sum (sf_kde_logsumexp) of a set of query rows against a base (training) set.  Behind
// synference_amd/ood.py: detect_outliers / detect_outliers_pyod (ref: src/synference/utils.py:991-1340) -- sklearn's
// LocalOutlierFactor / NearestNeighbors, scipy.stats.gaussian_kde and pyod's KNN / LOF / KDE all reduce to these two.
//
// Squared distance, the same bits wherever it is computed (and in tests/ood_model.py):
//   acc = 0; for c ascending: t = q[c] - b[c]; acc = acc + t * t      every operation rounded to nearest in fp32, no fma
// (columns padded to a multiple of four hold zeros on both sides: acc + 0 * 0 = acc).  A NaN distance counts as +inf.
//
// Both kernels: one thread per query, the query row in registers (CP = C rounded up to 4, a template parameter); the base is
// streamed through LDS in chunks of 128 rows, two rows interleaved per column so that one broadcast ds_read_b128 feeds two
// packed fp32 operations (v_pk_add_f32 / v_pk_mul_f32 work on the row pair).  The base is cut into S contiguous splits
// (grid.y) so that few queries still fill the device; a split writes a partial result per query and a second small kernel
// combines them in a fixed order.
//
// sf_knn: every candidate is the 64-bit key (d2 bits << 32 | row); d2 >= +0, so keys order like (d2, row) and the k smallest
// keys are ONE set whatever the chunking, the tiling or the split over calls.  Each thread keeps its k smallest keys sorted in
// LDS (list[j][thread]) and the k-th key's distance in a register; a row is looked at closely only when its distance does
// not exceed that bound (about k ln(N / k) times per query).  Empty list slots hold PAD = (+inf bits, 0xffffffff), above every
// real key.  The combine kernel ranks every real partial entry among all of a query's entries and writes ranks below k: no
// atomics, no unordered append.
// Few queries against a long base mean many short splits, and a list that starts empty takes k (1 + ln(n / k)) insertions per
// split -- with 64 queries per wave nearly every row would leave the fast path.  So with 8 splits or more a first pass
// (k_knn_gmin) takes the minimum distance of every query to G >= 4k contiguous groups of base rows; the k-th smallest of
// those minima (k_knn_bound) belongs to k distinct rows and therefore bounds the k-th neighbour distance from above.  The
// lists then start from that bound: about 1.3 k rows per query pass it over the WHOLE base, whatever the split count.  The
// bound only keeps non-members out: the result is the same set.
//
// sf_kde_logsumexp: per (query, split) the running minimum distance dmin and sum_i exp(-(d2_i - dmin) / 2) in fp64, rows in
// ascending order (v_exp_f32 per term; the sum is rescaled when the minimum drops, about ln N times); the combine kernel
// adds the splits in ascending order in fp64.  The split count depends on the shapes only: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <string>

#include "sf_internal.h"
#include "sf_ood_tile.h"
#include "sf_scratch.h"

#define SF_OOD_KMAX 64
#define SF_OOD_SMAX 256   // splits of the base
#define SF_OOD_PAD 0x7f800000ffffffffull

// ---- kNN: an upper bound of the k-th distance from group minima -----------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(256) void k_knn_gmin(const float* __restrict__ base, long N, int C, unsigned magic,
                                                  const float* __restrict__ query, long M, int exclude_self, long self_offset,
                                                  long split_len, int gs, long gl, float* __restrict__ gmin) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float* s_b = (float*)s_raw;
  const int tid = threadIdx.x, QT = blockDim.x;
  const long m = (long)blockIdx.x * QT + tid;
  const bool live = m < M;
  const int s = blockIdx.y, G = gridDim.y * gs;
  const long sb = (long)s * split_len;
  const long se = sb + split_len < N ? sb + split_len : N;
  const long self = exclude_self ? self_offset + m : -1;
  float q[CP];
  sf_ood_load_query<CP>(query, m, live, C, q);
  float* dst = gmin + m * G + (long)s * gs;
  int j = 0;
  long gend = sb + gl;   // gl is even: a group ends between two row pairs
  float cur = __builtin_inff();
  for (long r0 = sb; r0 < se; r0 += SF_OOD_CH) {
    __syncthreads();
    sf_ood_load_chunk<CP>(base, r0, se, C, magic, s_b);
    __syncthreads();
    for (int p = 0; p < SF_OOD_CH / 2; ++p) {
      const long r = r0 + 2 * p;
      if (r >= gend && j < gs - 1) {   // (uniform; rows past the split's end are +inf and stay with its last group)
        if (live) dst[j] = cur;
        ++j;
        gend += gl;
        cur = __builtin_inff();
      }
      sf_f2 d = sf_ood_d2pair<CP>(q, s_b, p);
      if (exclude_self) {
        d.x = r == self ? __builtin_inff() : d.x;
        d.y = r + 1 == self ? __builtin_inff() : d.y;
      }
      cur = __builtin_fminf(cur, __builtin_fminf(d.x, d.y));   // a NaN distance never becomes the minimum
    }
  }
  if (!live) return;
  for (; j < gs; ++j) {
    dst[j] = cur;
    cur = __builtin_inff();
  }
}

// one workgroup per query: the k-th smallest (with multiplicity) of its G group minima; fewer than k finite ones: +inf
__global__ __launch_bounds__(256) void k_knn_bound(const float* __restrict__ gmin, int G, int k, float* __restrict__ b0) {
  __shared__ unsigned long long s_key[512];
  const long m = blockIdx.x;
  for (int g = threadIdx.x; g < G; g += 256)
    s_key[g] = ((unsigned long long)__float_as_uint(gmin[m * G + g]) << 32) | (unsigned long long)g;
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) {
    const unsigned long long key = s_key[g];
    int rank = 0;
    for (int h = 0; h < G; ++h) rank += s_key[h] < key ? 1 : 0;
    if (rank == k - 1) b0[m] = __uint_as_float((uint32_t)(key >> 32));
  }
}

// ---- kNN: partial lists per (query, split) ----------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(256) void k_knn_part(const float* __restrict__ base, long N, int C, unsigned magic,
                                                  const float* __restrict__ query, long M, int k, int exclude_self,
                                                  long self_offset, long split_len, int S, const float* __restrict__ b0,
                                                  unsigned long long* __restrict__ part, float* __restrict__ d2_out,
                                                  int32_t* __restrict__ idx_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float* s_b = (float*)s_raw;                                                        // [CH/2][CP][2]
  unsigned long long* s_l = (unsigned long long*)(s_raw + SF_OOD_CH * CP * 4);       // [k][blockDim]
  const int tid = threadIdx.x, QT = blockDim.x;
  const long m = (long)blockIdx.x * QT + tid;
  const bool live = m < M;
  const int s = blockIdx.y;
  const long sb = (long)s * split_len;
  const long se = sb + split_len < N ? sb + split_len : N;
  const long self = exclude_self ? self_offset + m : -1;
  float q[CP];
  sf_ood_load_query<CP>(query, m, live, C, q);
  for (int j = 0; j < k; ++j) s_l[j * QT + tid] = SF_OOD_PAD;
  // rows above the bound of the first pass (if there was one) are no candidates: "key < kth0" is "d2 <= bound"
  const unsigned long long kth0 = (b0 && live) ? ((unsigned long long)__float_as_uint(b0[m]) << 32) | 0xffffffffull : SF_OOD_PAD;
  unsigned long long kth = kth0;
  float kth_d = __uint_as_float((uint32_t)(kth >> 32));
  for (long r0 = sb; r0 < se; r0 += SF_OOD_CH) {
    __syncthreads();   // the previous chunk has been read
    sf_ood_load_chunk<CP>(base, r0, se, C, magic, s_b);
    __syncthreads();
    for (int p = 0; p < SF_OOD_CH / 2; ++p) {
      const sf_f2 d = sf_ood_d2pair<CP>(q, s_b, p);
      if (!(d.x > kth_d) || !(d.y > kth_d)) {   // rare once the list has settled; a NaN comes here too
        for (int h = 0; h < 2; ++h) {
          const long r = r0 + 2 * p + h;
          float dd = h ? d.y : d.x;
          if (!(dd == dd)) dd = __builtin_inff();
          const unsigned long long key = ((unsigned long long)__float_as_uint(dd) << 32) | (unsigned long long)(uint32_t)r;
          if (r < se && r != self && key < kth) {
            int j = k - 1;
            while (j > 0) {
              const unsigned long long up = s_l[(j - 1) * QT + tid];
              if (up < key) break;
              s_l[j * QT + tid] = up;
              --j;
            }
            s_l[j * QT + tid] = key;
            kth = s_l[(k - 1) * QT + tid];
            kth = kth < kth0 ? kth : kth0;
            kth_d = __uint_as_float((uint32_t)(kth >> 32));
          }
        }
      }
    }
  }
  if (!live) return;
  if (S == 1) {
    for (int j = 0; j < k; ++j) {
      const unsigned long long key = s_l[j * QT + tid];
      d2_out[m * k + j] = __uint_as_float((uint32_t)(key >> 32));
      idx_out[m * k + j] = (int32_t)(uint32_t)key;
    }
  } else {
    for (int j = 0; j < k; ++j) part[(m * S + s) * k + j] = s_l[j * QT + tid];
  }
}

// one workgroup per query: the rank of every real partial entry among all of them; ranks below k are the result.  Real keys
// are distinct, and there are at least k of them in all (k <= N - exclude_self).  The real entries are first packed into LDS
// in their order (counts, a scan, no atomics) -- with a bound from the first pass most slots hold PAD -- and ranked by plain
// comparison; more than 2048 real entries (no bound, or very many rows at the bound distance): binary searches over the
// sorted partial lists in global memory.
#define SF_OOD_MERGE_LDS 2048
__global__ __launch_bounds__(256) void k_knn_merge(const unsigned long long* __restrict__ part, int S, int k,
                                                   float* __restrict__ d2_out, int32_t* __restrict__ idx_out) {
  __shared__ unsigned long long s_key[SF_OOD_MERGE_LDS];
  __shared__ int s_cnt[256];
  const long m = blockIdx.x;
  const int tid = threadIdx.x;
  const unsigned long long* pm = part + m * S * k;
  const int n = S * k;
  const int per = (n + 255) / 256;
  const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int c = 0;
  for (int e = lo; e < hi; ++e) c += pm[e] != SF_OOD_PAD ? 1 : 0;
  s_cnt[tid] = c;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int v = tid >= d ? s_cnt[tid - d] : 0;
    __syncthreads();
    s_cnt[tid] += v;
    __syncthreads();
  }
  const int R = s_cnt[255];
  if (R <= SF_OOD_MERGE_LDS) {   // (uniform)
    int off = s_cnt[tid] - c;
    for (int e = lo; e < hi; ++e) {
      const unsigned long long key = pm[e];
      if (key != SF_OOD_PAD) s_key[off++] = key;
    }
    __syncthreads();
    for (int i = tid; i < R; i += 256) {
      const unsigned long long key = s_key[i];
      int rank = 0;
      for (int h = 0; h < R; ++h) rank += s_key[h] < key ? 1 : 0;
      if (rank < k) {
        d2_out[m * k + rank] = __uint_as_float((uint32_t)(key >> 32));
        idx_out[m * k + rank] = (int32_t)(uint32_t)key;
      }
    }
    return;
  }
  for (int e = tid; e < n; e += 256) {
    const unsigned long long key = pm[e];
    if (key == SF_OOD_PAD) continue;
    int rank = 0;
    for (int s = 0; s < S && rank < k; ++s) {
      const unsigned long long* l = pm + s * k;
      int a = 0, b = k;   // entries of list s below key
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (l[mid] < key) a = mid + 1; else b = mid;
      }
      rank += a;
    }
    if (rank < k) {
      d2_out[m * k + rank] = __uint_as_float((uint32_t)(key >> 32));
      idx_out[m * k + rank] = (int32_t)(uint32_t)key;
    }
  }
}

// ---- KDE: log sum exp(-d2 / 2) ----------------------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(256) void k_kde_part(const float* __restrict__ base, long N, int C, unsigned magic,
                                                  const float* __restrict__ query, long M, long split_len, int S,
                                                  double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float* s_b = (float*)s_raw;
  const int tid = threadIdx.x, QT = blockDim.x;
  const long m = (long)blockIdx.x * QT + tid;
  const bool live = m < M;
  const int s = blockIdx.y;
  const long sb = (long)s * split_len;
  const long se = sb + split_len < N ? sb + split_len : N;
  float q[CP];
  sf_ood_load_query<CP>(query, m, live, C, q);
  const float hl2e = 0.72134752044448170368f;   // log2(e) / 2
  float dmin = __builtin_inff();
  double sum = 0.0;
  for (long r0 = sb; r0 < se; r0 += SF_OOD_CH) {
    __syncthreads();
    sf_ood_load_chunk<CP>(base, r0, se, C, magic, s_b);
    __syncthreads();
    for (int p = 0; p < SF_OOD_CH / 2; ++p) {
      const sf_f2 d = sf_ood_d2pair<CP>(q, s_b, p);
      const float lo = __builtin_fminf(d.x, d.y);   // the non-NaN one of the two, if any
      if (lo < dmin) {   // a new minimum: the sum so far is rescaled to it
        sum = sum == 0.0 ? 0.0 : sum * exp(-0.5 * ((double)dmin - (double)lo));
        dmin = lo;
      }
      // exp2 of (dmin - d2) log2(e) / 2; inf - inf and a NaN distance (a NaN in the base row) give NaN -> a zero term
      const float ex = __builtin_fmaxf(__builtin_amdgcn_exp2f((dmin - d.x) * hl2e), 0.f);
      const float ey = __builtin_fmaxf(__builtin_amdgcn_exp2f((dmin - d.y) * hl2e), 0.f);
      sum += (double)ex;
      sum += (double)ey;
    }
  }
  if (!live) return;
  part[(m * S + s) * 2 + 0] = (double)dmin;
  part[(m * S + s) * 2 + 1] = sum;
}

__global__ __launch_bounds__(256) void k_kde_merge(const double* __restrict__ part, long M, int S, double* __restrict__ out) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const double* pm = part + m * S * 2;
  double D = pm[0];
  for (int s = 1; s < S; ++s) D = pm[2 * s] < D ? pm[2 * s] : D;
  double tot = 0.0;
  for (int s = 0; s < S; ++s) {
    const double sm = pm[2 * s + 1];
    if (sm > 0.0) tot += sm * exp(-0.5 * (pm[2 * s] - D));
  }
  out[m] = tot > 0.0 ? -0.5 * D + log(tot) : -(double)__builtin_inff();
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {
SfScratch g_ood_scratch;   // sf_scratch.h: one for both entry points

struct SfOodPlan { int QT, S, n_qt, gs; long split_len, gl; unsigned magic; size_t lds; };

// queries per workgroup by list size (the lists stay within 32 KiB of LDS), splits so that about 2048 workgroups exist
SfOodPlan sf_ood_plan(int64_t N, int32_t C, int64_t M, int k) {
  SfOodPlan pl;
  pl.QT = k <= 16 ? 256 : (k <= 32 ? 128 : 64);
  pl.n_qt = (int)((M + pl.QT - 1) / pl.QT);
  long S = (2048 + pl.n_qt - 1) / pl.n_qt;
  const long nch = (long)((N + SF_OOD_CH - 1) / SF_OOD_CH);
  const long smax = nch / 8 > 1 ? nch / 8 : 1;   // at least 8 chunks per split
  S = S > smax ? smax : S;
  S = S > SF_OOD_SMAX ? SF_OOD_SMAX : S;
  const long per = (nch + S - 1) / S;
  pl.split_len = per * SF_OOD_CH;
  pl.S = (int)((N + pl.split_len - 1) / pl.split_len);
  // the bounding pass: with 8 splits or more, gs groups per split so that there are at least 4k groups in all
  pl.gs = pl.S >= 8 ? (4 * k + pl.S - 1) / pl.S : 0;
  pl.gl = pl.gs ? ((pl.split_len + pl.gs - 1) / pl.gs + 1) & ~1l : 0;
  pl.magic = (1u << 20) / (unsigned)C + 1u;
  const int CP = (C + 3) & ~3;
  pl.lds = (size_t)SF_OOD_CH * CP * 4 + (size_t)k * pl.QT * 8;
  return pl;
}

template <int CP>
struct SfKnnLaunch {
  static void go(dim3 grid, int QT, size_t lds, hipStream_t st, const float* base, long N, int C, unsigned magic,
                 const float* query, long M, int k, int ex, long so, long sl, int S, const float* b0, unsigned long long* part,
                 float* d2, int32_t* idx) {
    hipLaunchKernelGGL(k_knn_part<CP>, grid, dim3(QT), lds, st, base, N, C, magic, query, M, k, ex, so, sl, S, b0, part, d2, idx);
  }
};
template <int CP>
struct SfGminLaunch {
  static void go(dim3 grid, int QT, size_t lds, hipStream_t st, const float* base, long N, int C, unsigned magic,
                 const float* query, long M, int ex, long so, long sl, int gs, long gl, float* gmin) {
    hipLaunchKernelGGL(k_knn_gmin<CP>, grid, dim3(QT), lds, st, base, N, C, magic, query, M, ex, so, sl, gs, gl, gmin);
  }
};
template <int CP>
struct SfKdeLaunch {
  static void go(dim3 grid, int QT, size_t lds, hipStream_t st, const float* base, long N, int C, unsigned magic,
                 const float* query, long M, long sl, int S, double* part) {
    hipLaunchKernelGGL(k_kde_part<CP>, grid, dim3(QT), lds, st, base, N, C, magic, query, M, sl, S, part);
  }
};
}  // namespace

extern "C" int sf_knn(const float* base, int64_t N, int32_t C, const float* query, int64_t M, int32_t k, int32_t exclude_self,
                      int64_t self_offset, float* d2, int32_t* idx, void* stream) {
  if (!base || !query || !d2 || !idx) {
    sf_set_error("sf_knn: null argument");
    return SF_ERR_INVALID;
  }
  if (C < 1 || C > SF_OOD_CMAX || k < 1 || k > SF_OOD_KMAX || N < 1 || N > 0x7fffffffll || M < 0 ||
      (exclude_self != 0 && exclude_self != 1) || (int64_t)k > N - exclude_self || self_offset < 0 ||
      (exclude_self && self_offset + M > N)) {
    sf_set_error("sf_knn: need 1 <= C <= 64, 1 <= k <= 64, k <= N - exclude_self, 1 <= N < 2^31, M >= 0, exclude_self 0 or 1, "
                 "0 <= self_offset and self_offset + M <= N with exclude_self");
    return SF_ERR_INVALID;
  }
  if (M == 0) return SF_OK;
  hipStream_t st = (hipStream_t)stream;
  const SfOodPlan pl = sf_ood_plan(N, C, M, k);
  const int G = pl.S * pl.gs;   // <= 256 + 4 * 64 - 1
  SfScratchCall ws(g_ood_scratch, "sf_knn", st);
  const int sub_part = ws.add(pl.S > 1 ? (size_t)M * pl.S * k * 8 : 256);
  const int sub_gmin = G ? ws.add((size_t)M * G * 4) : -1, sub_b0 = G ? ws.add((size_t)M * 4) : -1;
  if (int rc = ws.reserve()) return rc;
  unsigned long long* part = ws.get<unsigned long long>(sub_part);
  float* gmin = G ? ws.get<float>(sub_gmin) : nullptr;
  float* b0 = G ? ws.get<float>(sub_b0) : nullptr;
  if (int rc = ws.check()) return rc;
  const int CP = (C + 3) & ~3;
  const dim3 grid((unsigned)pl.n_qt, (unsigned)pl.S);
  if (G) {
    sf_ood_dispatch<SfGminLaunch>(CP, grid, pl.QT, (size_t)SF_OOD_CH * CP * 4, st, base, (long)N, (int)C, pl.magic, query, (long)M,
                                  (int)exclude_self, (long)self_offset, pl.split_len, pl.gs, pl.gl, gmin);
    hipLaunchKernelGGL(k_knn_bound, dim3((unsigned)M), dim3(256), 0, st, (const float*)gmin, G, (int)k, b0);
  }
  sf_ood_dispatch<SfKnnLaunch>(CP, grid, pl.QT, pl.lds, st, base, (long)N, (int)C, pl.magic, query, (long)M, (int)k,
                               (int)exclude_self, (long)self_offset, pl.split_len, pl.S, (const float*)b0, part, d2, idx);
  if (pl.S > 1)
    hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)M), dim3(256), 0, st, (const unsigned long long*)part, pl.S, (int)k, d2, idx);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ws.fail("launch", e);
  return ws.finish();
}

extern "C" int sf_kde_logsumexp(const float* base_w, int64_t N, int32_t C, const float* query_w, int64_t M, double* out,
                                void* stream) {
  if (!base_w || !query_w || !out) {
    sf_set_error("sf_kde_logsumexp: null argument");
    return SF_ERR_INVALID;
  }
  if (C < 1 || C > SF_OOD_CMAX || N < 1 || N > 0x7fffffffll || M < 0) {
    sf_set_error("sf_kde_logsumexp: need 1 <= C <= 64, 1 <= N < 2^31, M >= 0");
    return SF_ERR_INVALID;
  }
  if (M == 0) return SF_OK;
  hipStream_t st = (hipStream_t)stream;
  SfOodPlan pl = sf_ood_plan(N, C, M, 1);
  pl.lds = (size_t)SF_OOD_CH * ((C + 3) & ~3) * 4;
  SfScratchCall ws(g_ood_scratch, "sf_kde_logsumexp", st);
  const int sub_part = ws.add((size_t)M * pl.S * 16);
  if (int rc = ws.reserve()) return rc;
  double* part = ws.get<double>(sub_part);
  if (int rc = ws.check()) return rc;
  sf_ood_dispatch<SfKdeLaunch>((C + 3) & ~3, dim3((unsigned)pl.n_qt, (unsigned)pl.S), pl.QT, pl.lds, st, base_w, (long)N, (int)C,
                               pl.magic, query_w, (long)M, pl.split_len, pl.S, part);
  hipLaunchKernelGGL(k_kde_merge, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const double*)part, (long)M, pl.S, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ws.fail("launch", e);
  return ws.finish();
}
