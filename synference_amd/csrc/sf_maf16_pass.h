// sf_maf16_pass.h -- device primitives of the 16-row MAF path (sf_maf16.hip): tile arithmetic, the operand forms of the hidden
// blocks and their state, the pass functions, the transforms of the unrolled kernels, staging, and the steps that every kernel
// of that file shares (item decode, context tile, degree-1 pass, tile-pair dispatch, epilogue constants, acceptance mask).
// Each step exists once, here; the kernels, their launchers and the shape plan live in sf_maf16.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sf_device.h"
#include "sf_internal.h"
#include "sf_rng.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define SF_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float sf_sum4groups(float v) {  // sum over the 4 row groups of a sample
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ f32x4 sf_mma16(float4 w, const f32x4& in, f32x4 acc) {
  acc = SF_MFMA16(w.x, in[0], acc);
  acc = SF_MFMA16(w.y, in[1], acc);
  acc = SF_MFMA16(w.z, in[2], acc);
  acc = SF_MFMA16(w.w, in[3], acc);
  return acc;
}
// head rows of one tile for this lane: (a0,m0,a1,m1), (a2,m2,a3,m3); acc = (sum a_r v_r, sum m_r v_r) as packed FMAs
__device__ __forceinline__ f32x2 sf_head_acc(f32x2 acc, const float4& h01, const float4& h23, const f32x4& v) {
  acc += f32x2{h01.x, h01.y} * f32x2{v[0], v[0]};
  acc += f32x2{h01.z, h01.w} * f32x2{v[1], v[1]};
  acc += f32x2{h23.x, h23.y} * f32x2{v[2], v[2]};
  acc += f32x2{h23.z, h23.w} * f32x2{v[3], v[3]};
  return acc;
}
__device__ __forceinline__ f32x4 sf_ld4(const float* p) {
  const float4 b = *reinterpret_cast<const float4*>(p);
  f32x4 r;
  r[0] = b.x; r[1] = b.y; r[2] = b.z; r[3] = b.w;
  return r;
}
// tanh of a tile's four values with the plain arithmetic on packed-f32 instructions (v_pk_add / v_pk_fma: two
// values per instruction at the full rate) -- the kernel is bound by vector ISSUE, and the four exp2 / four rcp cannot be
// packed.
// The argument is PRE-SCALED: the packer multiplies the hidden blocks' weights and biases of the 16-row images by
// 2 log2(e) (SF_PACK_TANH_SCALE, sf_layout.h), so tanh(x) = 1 - 2 / (1 + 2^b) with b = 2 log2(e) x starts at the exp2.
__device__ __forceinline__ float sf_tanh_pre(float b) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(b));
}
__device__ __forceinline__ f32x4 sf_tanh4(const f32x4& b) {
  const f32x2 one = {1.0f, 1.0f}, m2 = {-2.0f, -2.0f};
  const f32x2 e01 = f32x2{__builtin_amdgcn_exp2f(b[0]), __builtin_amdgcn_exp2f(b[1])} + one;
  const f32x2 e23 = f32x2{__builtin_amdgcn_exp2f(b[2]), __builtin_amdgcn_exp2f(b[3])} + one;
  const f32x2 r01 = {__builtin_amdgcn_rcpf(e01[0]), __builtin_amdgcn_rcpf(e01[1])};
  const f32x2 r23 = {__builtin_amdgcn_rcpf(e23[0]), __builtin_amdgcn_rcpf(e23[1])};
  const f32x2 o01 = __builtin_elementwise_fma(r01, m2, one), o23 = __builtin_elementwise_fma(r23, m2, one);
  return f32x4{o01[0], o01[1], o23[0], o23[1]};
}
// weight fragment of (out tile ot, in tile it) of a block with IT input tiles
__device__ __forceinline__ float4 sf_w16(const float* wp, int IT, int ot, int it, int lane) {
  return reinterpret_cast<const float4*>(wp)[(ot * IT + it) * 64 + lane];
}

extern __shared__ float sf_lds16[];

// scale of the affine map from the head's raw value (the only place the flow's scale function is chosen)
__device__ __forceinline__ float sf_scale16(const SfDev& m, float av) {
  return (m.scale_fn == 0 ? sf_softplus(av) : sf_sigmoid(av + 2.0f)) + m.eps;
}
// Finish a dimension: the affine inverse of physical slot sl from its head values (av, mv) and the incoming value u_sl, written
// into the slot's place in the tile-layout quad `ut` (row group sl >> 2, register sl & 3).  Returns the scale (log-determinant).
__device__ __forceinline__ float sf_finish16(const SfDev& m, f32x4& ut, int sl, float u_sl, float av, float mv, int g4) {
  const float sc = sf_scale16(m, av);
  const float wv = sf_div(u_sl - mv, sc);
#pragma unroll
  for (int r = 0; r < 4; ++r) ut[r] = (g4 == (sl >> 2) && r == (sl & 3)) ? wv : ut[r];
  return sc;
}
// The pass of degree 1: that dimension depends on the context only (head bias).  `tp`: the staged image; u_sl: the slot's
// incoming value as the caller holds it (sf_slot16: every row group, sf_slot16_own: the owning one -- no cross-lane move).
__device__ __forceinline__ float sf_pass16_deg1(const SfDev& m, const float* tp, f32x4& ut, int sl, float u_sl, int g4) {
  const float av = tp[m.o16_hvb + 2 * sl], mv = tp[m.o16_hvb + 2 * sl + 1];
  return sf_finish16(m, ut, sl, u_sl, av, mv, g4);
}

struct SfPass16 {
  f32x4 act[3][4];  // act[0] = initial layer, act[k+1] = output of block k; [tile]
  f32x4 c0[4];      // b0 + bc + Wc e(x), per tile
  f32x4 ut;         // finished dimensions of this transform, tile layout: slot 4*g4 + r
  float ldl;
};

// One autoregressive pass with the degree group in (static) tile OT: recompute that tile of every hidden
// layer from the finished dimensions, then the (a, m) head rows of physical slot sl as per-lane dot products.
template <int OT, int NB, bool LD = true>
__device__ __forceinline__ void sf_pass16(const SfDev& m, const float* tp, SfPass16& S, int NT, int sl, float u_sl,
                                          int lane, int g4) {
  // everything that does not depend on this pass's new dimension first: weight fragments, partial sums
  const float* hv = tp + m.o16_hv + sl * 128 + g4 * 32;
  float4 w0 = sf_w16(tp + m.o16_w0, 1, OT, 0, lane);
  float4 wk[2][OT + 1];
  f32x4 bk[2];
  float4 h01[OT + 1], h23[OT + 1];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    bk[k] = sf_ld4(tp + m.o16_bk[k] + (OT * 4 + g4) * 4);
#pragma unroll
    for (int it = 0; it <= OT; ++it) wk[k][it] = sf_w16(tp + m.o16_wk[k], NT, OT, it, lane);
  }
#pragma unroll
  for (int tl = 0; tl <= OT; ++tl) {
    h01[tl] = *reinterpret_cast<const float4*>(hv + tl * 8);
    h23[tl] = *reinterpret_cast<const float4*>(hv + tl * 8 + 4);
  }
  const float ba = tp[m.o16_hvb + 2 * sl], bm = tp[m.o16_hvb + 2 * sl + 1];
  f32x2 pam = {0.f, 0.f};
#pragma unroll
  for (int tl = 0; tl < OT; ++tl) pam = sf_head_acc(pam, h01[tl], h23[tl], S.act[NB][tl]);
#pragma unroll
  for (int k = 0; k < NB; ++k)
#pragma unroll
    for (int it = 0; it < OT; ++it) bk[k] = sf_mma16(wk[k][it], S.act[k][it], bk[k]);
  // the dependent chain
  S.act[0][OT] = sf_mma16(w0, S.ut, S.c0[OT]);
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    const f32x4 b = sf_mma16(wk[k][OT], S.act[k][OT], bk[k]);
#pragma unroll
    for (int r = 0; r < 4; ++r) S.act[k + 1][OT][r] = sf_tanh_pre(b[r]);
  }
  pam = sf_head_acc(pam, h01[OT], h23[OT], S.act[NB][OT]);
  const float av = ba + sf_sum4groups(pam[0]);
  const float mv = bm + sf_sum4groups(pam[1]);
  const float sc = sf_finish16(m, S.ut, sl, u_sl, av, mv, g4);
  if (LD) S.ldl += sf_log(sc);  // (the sampler does not need the log-determinant)
}

// Same pass when the degree group straddles tiles LO..HI (contiguous packing, sf_layout.cpp): every layer is
// recomputed for all of those tiles before the next layer starts (units of one degree feed each other), over the
// input tiles 0..HI; rows of later groups inside these tiles get provisional values that nothing unmasked reads
// and that their own pass overwrites.
template <int LO, int HI, int NB, bool LD = true>
__device__ __forceinline__ void sf_pass16_span(const SfDev& m, const float* tp, SfPass16& S, int NT, int sl, float u_sl,
                                               int lane, int g4) {
  const float* hv = tp + m.o16_hv + sl * 128 + g4 * 32;
#pragma unroll
  for (int ot = LO; ot <= HI; ++ot) S.act[0][ot] = sf_mma16(sf_w16(tp + m.o16_w0, 1, ot, 0, lane), S.ut, S.c0[ot]);
#pragma unroll
  for (int k = 0; k < NB; ++k) {
#pragma unroll
    for (int ot = LO; ot <= HI; ++ot) {
      f32x4 b = sf_ld4(tp + m.o16_bk[k] + (ot * 4 + g4) * 4);
#pragma unroll
      for (int it = 0; it <= HI; ++it) b = sf_mma16(sf_w16(tp + m.o16_wk[k], NT, ot, it, lane), S.act[k][it], b);
#pragma unroll
      for (int r = 0; r < 4; ++r) S.act[k + 1][ot][r] = sf_tanh_pre(b[r]);
    }
  }
  f32x2 pam = {0.f, 0.f};
#pragma unroll
  for (int tl = 0; tl <= HI; ++tl)
    pam = sf_head_acc(pam, *reinterpret_cast<const float4*>(hv + tl * 8), *reinterpret_cast<const float4*>(hv + tl * 8 + 4),
                      S.act[NB][tl]);
  const float av = tp[m.o16_hvb + 2 * sl] + sf_sum4groups(pam[0]);
  const float mv = tp[m.o16_hvb + 2 * sl + 1] + sf_sum4groups(pam[1]);
  const float sc = sf_finish16(m, S.ut, sl, u_sl, av, mv, g4);
  if (LD) S.ldl += sf_log(sc);  // (the sampler does not need the log-determinant)
}

// value of physical slot sl from a tile-layout register quad, broadcast to every row group
__device__ __forceinline__ float sf_slot16(const f32x4& t, int sl, int lane) {
  const int r = sl & 3;
  const float v = r == 0 ? t[0] : (r == 1 ? t[1] : (r == 2 ? t[2] : t[3]));
  return __shfl(v, (lane & 15) + 16 * (sl >> 2), 64);
}

// the same value where it is needed only in the row group that owns the slot (lanes of group sl >> 2): no cross-lane move
__device__ __forceinline__ float sf_slot16_own(const f32x4& t, int sl) {
  const int r = sl & 3;
  return r == 0 ? t[0] : (r == 1 ? t[1] : (r == 2 ? t[2] : t[3]));
}

// ---------------------------------------------------------------------------------------------------------------
// Split-bf16 hidden blocks (k_maf_samp16 only).  The H x H blocks carry ~2/3 of a pass's MACs; on fp32 MFMA
// (v_mfma_f32_16x16x4_f32: 32 cycles for K = 4) they take as long as the same MACs on the vector pipe.  Here every
// operand is split into hi = bf16(v) and lo = bf16(v - hi) and the product is hi.hi + hi.lo + lo.hi on
// v_mfma_f32_16x16x32_bf16 (16 cycles for K = 32, fp32 accumulation): ~2^-17 relative per product -- the draws still
// meet the oracle at the fp32 tolerance of the parity tests -- at a fifth of the matrix-pipe time.
// Operand order: two 16-row activation tiles (4 registers per lane each, lane = sample + 16 * row group) ARE the B
// operand of one K = 32 step: element j of lane l is row 16*(2*pair + (j>>2)) + 4*(l>>4) + (j&3); the weight image
// (sf_layout.cpp, src16B) stores the A operand in the same k order, hi and lo parts as separate 16-byte fragments.
// ---------------------------------------------------------------------------------------------------------------
typedef __bf16 sf_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sf_bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define SF_MFMA16B(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

struct SfSplit2 {  // two activation values' worth of split operands for one 16-row tile: hi/lo packed bf16 pairs
  unsigned int hi[2], lo[2];
};
__device__ __forceinline__ SfSplit2 sf_split16(const f32x4& v) {
  SfSplit2 t;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    // ONE packed conversion per pair (element-wise casts make the compiler convert the pair once packed and its first
    // element once more on its own); round-to-nearest-even, the same values
    const f32x2 pv = {v[2 * q], v[2 * q + 1]};
    const unsigned int hw = __builtin_bit_cast(unsigned int, __builtin_convertvector(pv, sf_bf16x2));
    const f32x2 rv = {v[2 * q] - __builtin_bit_cast(float, hw << 16), v[2 * q + 1] - __builtin_bit_cast(float, hw & 0xffff0000u)};
    t.hi[q] = hw;
    t.lo[q] = __builtin_bit_cast(unsigned int, __builtin_convertvector(rv, sf_bf16x2));
  }
  return t;
}
// acc += W[ot, pair] . (the pair's two tiles)   (three bf16 products; bh / bl ARE the B operands, no moves)
__device__ __forceinline__ f32x4 sf_mma16x3(const u32x4& w_hi, const u32x4& w_lo, const u32x4& bh, const u32x4& bl, f32x4 acc) {
  const sf_bf16x8 Ah = __builtin_bit_cast(sf_bf16x8, w_hi), Al = __builtin_bit_cast(sf_bf16x8, w_lo);
  const sf_bf16x8 Bh = __builtin_bit_cast(sf_bf16x8, bh), Bl = __builtin_bit_cast(sf_bf16x8, bl);
  acc = SF_MFMA16B(Al, Bh, acc);
  acc = SF_MFMA16B(Ah, Bl, acc);
  acc = SF_MFMA16B(Ah, Bh, acc);
  return acc;
}
// fragment of block k: (out tile ot, in-tile pair pr, part 0 = hi / 1 = lo); wB = base of the block in 32-bit words
// CP: aligned placement stores only the pairs a tile can read (sf_layout.cpp): entry ot + (ot == 3) + pr
template <bool CP>
__device__ __forceinline__ u32x4 sf_w16b(const unsigned int* wB, int NP, int ot, int pr, int part, int lane) {
  const int e = CP ? ot + (ot == 3 ? 1 : 0) + pr : ot * NP + pr;
  return reinterpret_cast<const u32x4*>(wB)[(e * 2 + part) * 64 + lane];
}

struct SfPass16B {
  // split inputs of hidden block k ([0] = initial layer, [1] = output of block 0), held per PAIR of tiles exactly as
  // the MFMA wants its B operand: components 0,1 = tile 2p (rows 0,1 | rows 2,3), components 2,3 = tile 2p+1
  u32x4 ph[2][2], pl[2][2];
  f32x4 head[4];       // output of the last block (fp32: the head rows are per-lane dot products); [tile]   (HM = false)
  f32x4 hdone;         // HM: head biases + the head rows' products with every FINISHED hidden tile, as one MFMA output
                       // tile: lane (s, g4), register r = row 4*g4 + r = (a | m) of physical slot (4*g4 + r) >> 1
  f32x4 ut;            // finished dimensions of this transform, tile layout: slot 4*g4 + r
  const float* c0p;    // this draw's context-table row for the transform (b0 + bc + Wc e(x), tile order), or nullptr
  const float* xr;     // the draw's context row (no-table path: c0 is evaluated where it is needed)
  f32x4 c0n;           // table path, aligned placement: c0 of the NEXT pass's tile, requested one pass ahead so that the
                       // L2 round trip is over before the pass that starts its dependent chain with it
  bool tab;            // wave-uniform: the table exists (c0p is per lane, the decision is not)
};
// The same state with the hidden blocks' inputs in fp32 (PREC = 1: v_mfma_f32_16x16x4_f32 everywhere, see sf_pass16f)
struct SfPass16F {
  f32x4 act[2][4];     // inputs of hidden block k ([0] = initial layer, [1] = output of block 0); [tile]: C/D layout of the MFMA
                       // that wrote them = B-operand order of the one that reads them
  f32x4 head[4];       // output of the last block; [tile]   (HM = false)
  f32x4 hdone;         // HM: see SfPass16B
  f32x4 ut;
  const float* c0p;
  const float* xr;
  f32x4 c0n;
  bool tab;
};
// standardised context of the row xr, tile ic: rows 16*ic + 4*g4 + r (zeros past C)
__device__ __forceinline__ f32x4 sf_ctx_tile16(const SfDev& m, const float* xr, int ic, int g4) {
  f32x4 ct;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rho = ic * 16 + 4 * g4 + r;
    const bool ok = rho < m.C;
    const int rr = ok ? rho : 0;
    const float v = sf_div(xr[rr] - m.cst[m.c_xmean + rr], m.cst[m.c_xstd + rr]);
    ct[r] = ok ? v : 0.f;
  }
  return ct;
}
// request c0 of tile `ot` of the current transform (table path only)
template <typename ST>
__device__ __forceinline__ void sf_c0_prefetch(ST& S, int ot, int g4) {
  S.c0n = *reinterpret_cast<const f32x4*>(S.c0p + ot * 16 + 4 * g4);
}
// c0 of tile ot = b0 + bc + Wc e(x): from the per-galaxy table, else evaluated on the spot (rare: tables above the
// size cap); either way it is not kept in registers across the passes
template <typename ST>
__device__ __forceinline__ f32x4 sf_c0_16(const SfDev& m, const float* tp, const ST& S, int ot, int lane, int g4) {
  if (S.c0p) return *reinterpret_cast<const f32x4*>(S.c0p + ot * 16 + 4 * g4);
  f32x4 c = sf_ld4(tp + m.o16_b0 + (ot * 4 + g4) * 4);
  for (int ic = 0; ic < m.nC16; ++ic) {
    c = sf_mma16(sf_w16(tp + m.o16_wc, m.nC16, ot, ic, lane), sf_ctx_tile16(m, S.xr, ic, g4), c);
  }
  return c;
}
template <int TILE>
__device__ __forceinline__ void sf_put16b(SfPass16B& S, int k, const f32x4& v) {  // k is a static loop index at every call
  const SfSplit2 t = sf_split16(v);
  S.ph[k][TILE >> 1][(TILE & 1) * 2] = t.hi[0];
  S.ph[k][TILE >> 1][(TILE & 1) * 2 + 1] = t.hi[1];
  S.pl[k][TILE >> 1][(TILE & 1) * 2] = t.lo[0];
  S.pl[k][TILE >> 1][(TILE & 1) * 2 + 1] = t.lo[1];
}

// One autoregressive pass with the degree group in (static) tile OT (see sf_pass16); hidden blocks on split bf16.
// HM (aligned placement, D <= 8): the head rows of ALL slots are one 16-row MFMA output tile (sf_layout.cpp, o16_wh); a
// pass adds its tile's product to the running tile S.hdone and reads its own (a, m) out of the result -- 4 MFMAs
// instead of 4 (OT + 1) packed FMAs, 2 (OT + 1) LDS reads and a two-step cross-row-group sum, and 4 registers of state
// instead of 16.
template <int OT, int NB, bool CP, bool HM = false>
__device__ __forceinline__ void sf_pass16b(const SfDev& m, const float* tp, const unsigned int* tpB, SfPass16B& S, int NT, int sl,
                                           float u_sl, int lane, int g4, int next_ot = -1) {
  constexpr int PR = OT >> 1;  // the pair that holds tile OT; pairs below it are complete
  const int NP = m.nP16;
  f32x4 c0;
  if (CP && HM && S.tab) {  // (aligned placement: one tile per pass, so the caller knows the next one; HM: the registers for it)
    c0 = S.c0n;
    if (next_ot >= 0) sf_c0_prefetch(S, next_ot, g4);
  } else {
    c0 = sf_c0_16(m, tp, S, OT, lane, g4);
  }
  const float* hv = tp + m.o16_hv + sl * 128 + g4 * 32;
  const float4 w0 = sf_w16(tp + m.o16_w0, 1, OT, 0, lane);
  // head rows of the tiles finished in earlier passes: partial sums first (nothing here depends on this pass)
  f32x2 pam = {0.f, 0.f};
  if (!HM) {
#pragma unroll
    for (int tl = 0; tl < OT; ++tl)
      pam = sf_head_acc(pam, *reinterpret_cast<const float4*>(hv + tl * 8), *reinterpret_cast<const float4*>(hv + tl * 8 + 4), S.head[tl]);
  }
  f32x4 last;
  float4 wh;
  if (HM) {
    // operand fragments are requested one stage ahead of the MFMAs that read them (block 0 under the initial layer's
    // chain, block k + 1 / the head rows under block k's tanh and split), so that an LDS round trip per fragment does
    // not sit in the dependent chain; the scheduling barriers pin that order
    u32x4 fh[PR + 1], fl[PR + 1];
    f32x4 b = sf_ld4(tp + m.o16_bk[0] + (OT * 4 + g4) * 4);
#pragma unroll
    for (int pr = 0; pr <= PR; ++pr) {
      fh[pr] = sf_w16b<CP>(tpB + m.o16B_wk[0], NP, OT, pr, 0, lane);
      fl[pr] = sf_w16b<CP>(tpB + m.o16B_wk[0], NP, OT, pr, 1, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    sf_put16b<OT>(S, 0, sf_mma16(w0, S.ut, c0));
#pragma unroll
    for (int k = 0; k < NB; ++k) {
#pragma unroll
      for (int pr = 0; pr <= PR; ++pr) b = sf_mma16x3(fh[pr], fl[pr], S.ph[k][pr], S.pl[k][pr], b);
      __builtin_amdgcn_sched_barrier(0);
      f32x4 bn;
      if (k + 1 < NB) {
        bn = sf_ld4(tp + m.o16_bk[k + 1 < NB ? k + 1 : k] + (OT * 4 + g4) * 4);
#pragma unroll
        for (int pr = 0; pr <= PR; ++pr) {
          fh[pr] = sf_w16b<CP>(tpB + m.o16B_wk[k + 1 < NB ? k + 1 : k], NP, OT, pr, 0, lane);
          fl[pr] = sf_w16b<CP>(tpB + m.o16B_wk[k + 1 < NB ? k + 1 : k], NP, OT, pr, 1, lane);
        }
      } else {
        wh = sf_w16(tp + m.o16_wh, NT, 0, OT, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
      const f32x4 th = sf_tanh4(b);
      if (k + 1 < NB) { sf_put16b<OT>(S, k + 1, th); b = bn; }
      else last = th;
    }
  } else {
  // initial layer of tile OT (the start of the dependent chain)
  sf_put16b<OT>(S, 0, sf_mma16(w0, S.ut, c0));
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    __builtin_amdgcn_sched_barrier(0);  // keep one block's fragments in flight at a time (registers)
    f32x4 b = sf_ld4(tp + m.o16_bk[k] + (OT * 4 + g4) * 4);
    // complete pairs, then the pair of tile OT: its other tile is either final (OT odd) or one that masked weights
    // never read (OT even)
#pragma unroll
    for (int pr = 0; pr <= PR; ++pr)
      b = sf_mma16x3(sf_w16b<CP>(tpB + m.o16B_wk[k], NP, OT, pr, 0, lane), sf_w16b<CP>(tpB + m.o16B_wk[k], NP, OT, pr, 1, lane),
                     S.ph[k][pr], S.pl[k][pr], b);
    f32x4 th;
#pragma unroll
    for (int r = 0; r < 4; ++r) th[r] = sf_tanh_pre(b[r]);
    if (k + 1 < NB) sf_put16b<OT>(S, k + 1, th);
    else S.head[OT] = th;
  }
  }
  float av, mv;
  if (HM) {
    const f32x4 fresh = sf_mma16(wh, last, S.hdone);
    // the tile is final once the next pass works on another one (several small degree groups may share a tile: each of
    // their passes recomputes it, the running tile takes it once)
    if (next_ot != OT) S.hdone = fresh;
    const bool odd = (sl & 1) != 0;  // rows 2 sl, 2 sl + 1 sit in row group sl >> 1, registers 0,1 or 2,3
    const int src = (lane & 15) + 16 * (sl >> 1);
    av = __shfl(odd ? fresh[2] : fresh[0], src, 64);
    mv = __shfl(odd ? fresh[3] : fresh[1], src, 64);
  } else {
    pam = sf_head_acc(pam, *reinterpret_cast<const float4*>(hv + OT * 8), *reinterpret_cast<const float4*>(hv + OT * 8 + 4), S.head[OT]);
    av = tp[m.o16_hvb + 2 * sl] + sf_sum4groups(pam[0]);
    mv = tp[m.o16_hvb + 2 * sl + 1] + sf_sum4groups(pam[1]);
  }
  sf_finish16(m, S.ut, sl, u_sl, av, mv, g4);
}

// The same pass when the degree group straddles tiles LO..HI (contiguous packing; see sf_pass16_span).
template <int LO, int HI, int NB>
__device__ __forceinline__ void sf_pass16b_span(const SfDev& m, const float* tp, const unsigned int* tpB, SfPass16B& S, int NT,
                                                int sl, float u_sl, int lane, int g4) {
  constexpr int PH = HI >> 1;
  const int NP = m.nP16;
  const float* hv = tp + m.o16_hv + sl * 128 + g4 * 32;
  auto put = [&](int k, int ot, const f32x4& v) {  // (k, ot are unrolled loop indices: static after unrolling)
    const SfSplit2 t = sf_split16(v);
    S.ph[k][ot >> 1][(ot & 1) * 2] = t.hi[0];
    S.ph[k][ot >> 1][(ot & 1) * 2 + 1] = t.hi[1];
    S.pl[k][ot >> 1][(ot & 1) * 2] = t.lo[0];
    S.pl[k][ot >> 1][(ot & 1) * 2 + 1] = t.lo[1];
  };
#pragma unroll
  for (int ot = LO; ot <= HI; ++ot) put(0, ot, sf_mma16(sf_w16(tp + m.o16_w0, 1, ot, 0, lane), S.ut, sf_c0_16(m, tp, S, ot, lane, g4)));
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    f32x4 nb[HI - LO + 1];
#pragma unroll
    for (int ot = LO; ot <= HI; ++ot) {
      f32x4 b = sf_ld4(tp + m.o16_bk[k] + (ot * 4 + g4) * 4);
#pragma unroll
      for (int pr = 0; pr <= PH; ++pr)
        b = sf_mma16x3(sf_w16b<false>(tpB + m.o16B_wk[k], NP, ot, pr, 0, lane), sf_w16b<false>(tpB + m.o16B_wk[k], NP, ot, pr, 1, lane),
                       S.ph[k][pr], S.pl[k][pr], b);
#pragma unroll
      for (int r = 0; r < 4; ++r) nb[ot - LO][r] = sf_tanh_pre(b[r]);
    }
#pragma unroll
    for (int ot = LO; ot <= HI; ++ot) {
      if (k + 1 < NB) put(k + 1, ot, nb[ot - LO]);
      else S.head[ot] = nb[ot - LO];
    }
  }
  f32x2 pam = {0.f, 0.f};
#pragma unroll
  for (int tl = 0; tl <= HI; ++tl)
    pam = sf_head_acc(pam, *reinterpret_cast<const float4*>(hv + tl * 8), *reinterpret_cast<const float4*>(hv + tl * 8 + 4),
                      S.head[tl]);
  const float av = tp[m.o16_hvb + 2 * sl] + sf_sum4groups(pam[0]);
  const float mv = tp[m.o16_hvb + 2 * sl + 1] + sf_sum4groups(pam[1]);
  sf_finish16(m, S.ut, sl, u_sl, av, mv, g4);
}

// ---------------------------------------------------------------------------------------------------------------
// fp32 hidden blocks (PREC = 1): the passes of the persistent sampler with EVERY product on v_mfma_f32_16x16x4_f32 -- the
// arithmetic of BASELINE configs[1] ("fp32"), draw for draw the fmaf chains of the density kernel.  Same incremental
// inverse, same tiles, same queue; what changes is the operand form of the H x H blocks: 16 x 16 fp32 fragments
// (float4[block * 64 + lane], the layout of part A) instead of split-bf16 pairs, and the activation state is the
// accumulator tile itself (no conversion between layers).  The blocks are copied into LDS behind part A from the full
// fp32 image (packed16 + o16_wk): aligned placement (CP) only the blocks on and below the diagonal -- a tile never reads
// tiles above its own -- as entries ot (ot + 1) / 2 + it; contiguous placement all NT x NT.
// Cost: (OT + 1) x 4 MFMAs of 32 cycles per block row instead of (OT / 2 + 1) x 3 of 16: the matrix pipe, not the
// vector issue port, bounds this kernel's dense phase ("fp32 sampler").
// ---------------------------------------------------------------------------------------------------------------
template <bool CP>
__device__ __forceinline__ float4 sf_w16f(const float* wF, int NT, int ot, int it, int lane) {
  const int e = CP ? (ot * (ot + 1)) / 2 + it : ot * NT + it;
  return reinterpret_cast<const float4*>(wF)[e * 64 + lane];
}
template <bool CP>
__device__ __forceinline__ int sf_f16_block_floats(int NT) { return (CP ? NT * (NT + 1) / 2 : NT * NT) * 256; }

template <int OT, int NB, bool CP, bool HM = false>
__device__ __forceinline__ void sf_pass16f(const SfDev& m, const float* tp, const float* tpF, SfPass16F& S, int NT, int sl,
                                           float u_sl, int lane, int g4, int next_ot = -1) {
  const int BF = sf_f16_block_floats<CP>(NT);
  f32x4 c0;
  if (CP && HM && S.tab) {
    c0 = S.c0n;
    if (next_ot >= 0) sf_c0_prefetch(S, next_ot, g4);
  } else {
    c0 = sf_c0_16(m, tp, S, OT, lane, g4);
  }
  const float* hv = tp + m.o16_hv + sl * 128 + g4 * 32;
  const float4 w0 = sf_w16(tp + m.o16_w0, 1, OT, 0, lane);
  f32x2 pam = {0.f, 0.f};
  if (!HM) {
#pragma unroll
    for (int tl = 0; tl < OT; ++tl)
      pam = sf_head_acc(pam, *reinterpret_cast<const float4*>(hv + tl * 8), *reinterpret_cast<const float4*>(hv + tl * 8 + 4), S.head[tl]);
  }
  f32x4 last;
  float4 wh;
  // One block row's fragments are in flight at a time.  The products with the tiles finished in earlier passes (it < OT)
  // do not depend on this pass: they are issued under the initial layer's chain (block 0) and under the tanh of block k
  // (block k + 1), so that the dependent chain of a pass is w0 -> W0[OT, OT] -> tanh -> W1[OT, OT] -> tanh -> head.
  float4 fw[OT + 1];
  f32x4 b = sf_ld4(tp + m.o16_bk[0] + (OT * 4 + g4) * 4);
#pragma unroll
  for (int it = 0; it <= OT; ++it) fw[it] = sf_w16f<CP>(tpF, NT, OT, it, lane);
  __builtin_amdgcn_sched_barrier(0);
  S.act[0][OT] = sf_mma16(w0, S.ut, c0);
#pragma unroll
  for (int it = 0; it < OT; ++it) b = sf_mma16(fw[it], S.act[0][it], b);
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    b = sf_mma16(fw[OT], S.act[k][OT], b);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 bn;
    if (k + 1 < NB) {
      bn = sf_ld4(tp + m.o16_bk[k + 1 < NB ? k + 1 : k] + (OT * 4 + g4) * 4);
#pragma unroll
      for (int it = 0; it <= OT; ++it) fw[it] = sf_w16f<CP>(tpF + (k + 1 < NB ? k + 1 : k) * BF, NT, OT, it, lane);
    } else if (HM) {
      wh = sf_w16(tp + m.o16_wh, NT, 0, OT, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    const f32x4 th = sf_tanh4(b);
    if (k + 1 < NB) {
#pragma unroll
      for (int it = 0; it < OT; ++it) bn = sf_mma16(fw[it], S.act[k + 1][it], bn);
      S.act[k + 1][OT] = th;
      b = bn;
    } else {
      last = th;
    }
  }
  float av, mv;
  if (HM) {
    const f32x4 fresh = sf_mma16(wh, last, S.hdone);
    if (next_ot != OT) S.hdone = fresh;
    const bool odd = (sl & 1) != 0;
    const int src = (lane & 15) + 16 * (sl >> 1);
    av = __shfl(odd ? fresh[2] : fresh[0], src, 64);
    mv = __shfl(odd ? fresh[3] : fresh[1], src, 64);
  } else {
    S.head[OT] = last;
    pam = sf_head_acc(pam, *reinterpret_cast<const float4*>(hv + OT * 8), *reinterpret_cast<const float4*>(hv + OT * 8 + 4), S.head[OT]);
    av = tp[m.o16_hvb + 2 * sl] + sf_sum4groups(pam[0]);
    mv = tp[m.o16_hvb + 2 * sl + 1] + sf_sum4groups(pam[1]);
  }
  sf_finish16(m, S.ut, sl, u_sl, av, mv, g4);
}

// The fp32 pass when the degree group straddles tiles LO..HI (contiguous packing; see sf_pass16_span).
template <int LO, int HI, int NB>
__device__ __forceinline__ void sf_pass16f_span(const SfDev& m, const float* tp, const float* tpF, SfPass16F& S, int NT, int sl,
                                                float u_sl, int lane, int g4) {
  const int BF = sf_f16_block_floats<false>(NT);
  const float* hv = tp + m.o16_hv + sl * 128 + g4 * 32;
#pragma unroll
  for (int ot = LO; ot <= HI; ++ot) S.act[0][ot] = sf_mma16(sf_w16(tp + m.o16_w0, 1, ot, 0, lane), S.ut, sf_c0_16(m, tp, S, ot, lane, g4));
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    f32x4 nb[HI - LO + 1];
#pragma unroll
    for (int ot = LO; ot <= HI; ++ot) {
      f32x4 b = sf_ld4(tp + m.o16_bk[k] + (ot * 4 + g4) * 4);
#pragma unroll
      for (int it = 0; it <= HI; ++it) b = sf_mma16(sf_w16f<false>(tpF + k * BF, NT, ot, it, lane), S.act[k][it], b);
      nb[ot - LO] = sf_tanh4(b);
    }
#pragma unroll
    for (int ot = LO; ot <= HI; ++ot) {
      if (k + 1 < NB) S.act[k + 1][ot] = nb[ot - LO];
      else S.head[ot] = nb[ot - LO];
    }
  }
  f32x2 pam = {0.f, 0.f};
#pragma unroll
  for (int tl = 0; tl <= HI; ++tl)
    pam = sf_head_acc(pam, *reinterpret_cast<const float4*>(hv + tl * 8), *reinterpret_cast<const float4*>(hv + tl * 8 + 4),
                      S.head[tl]);
  const float av = tp[m.o16_hvb + 2 * sl] + sf_sum4groups(pam[0]);
  const float mv = tp[m.o16_hvb + 2 * sl + 1] + sf_sum4groups(pam[1]);
  sf_finish16(m, S.ut, sl, u_sl, av, mv, g4);
}

// ---- what the kernels below see of the two operand forms (PREC: 0 = split bf16 x3, 1 = fp32)
template <int PREC> struct SfHid16;
template <> struct SfHid16<0> {
  using State = SfPass16B;
  template <int OT, int NB, bool CP, bool HM>
  static __device__ __forceinline__ void pass(const SfDev& m, const float* tp, const void* tpH, State& S, int NT, int sl, float u_sl,
                                              int lane, int g4, int next_ot) {
    sf_pass16b<OT, NB, CP, HM>(m, tp, static_cast<const unsigned int*>(tpH), S, NT, sl, u_sl, lane, g4, next_ot);
  }
  template <int LO, int HI, int NB>
  static __device__ __forceinline__ void span(const SfDev& m, const float* tp, const void* tpH, State& S, int NT, int sl, float u_sl,
                                              int lane, int g4) {
    sf_pass16b_span<LO, HI, NB>(m, tp, static_cast<const unsigned int*>(tpH), S, NT, sl, u_sl, lane, g4);
  }
  // cleared per tile and transform: a non-finite value left behind by one draw must not reach another one through a
  // structural zero (a pass only reads tiles that an earlier pass of the SAME tile and transform wrote, or zeros).
  // SEQ (unrolled kernels: passes in tile order 0, 1, 2, 3): the only operands read before this tile and transform wrote
  // them are the odd tiles (the second half of a pair, read with all-zero weights by the pass of the even tile)
  template <bool SEQ, bool HM>
  static __device__ __forceinline__ void clear(State& S) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr)
#pragma unroll
        for (int c = SEQ ? 2 : 0; c < 4; ++c) { S.ph[k][pr][c] = 0u; S.pl[k][pr][c] = 0u; }
    if (!HM) {
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) S.head[ot][r] = 0.f;
    }
  }
  // LDS floats behind part A
  static __host__ __device__ int lds_floats(const SfDev& m, bool /*cp*/) { return m.t16B_stride; }
};
template <> struct SfHid16<1> {
  using State = SfPass16F;
  template <int OT, int NB, bool CP, bool HM>
  static __device__ __forceinline__ void pass(const SfDev& m, const float* tp, const void* tpH, State& S, int NT, int sl, float u_sl,
                                              int lane, int g4, int next_ot) {
    sf_pass16f<OT, NB, CP, HM>(m, tp, static_cast<const float*>(tpH), S, NT, sl, u_sl, lane, g4, next_ot);
  }
  template <int LO, int HI, int NB>
  static __device__ __forceinline__ void span(const SfDev& m, const float* tp, const void* tpH, State& S, int NT, int sl, float u_sl,
                                              int lane, int g4) {
    sf_pass16f_span<LO, HI, NB>(m, tp, static_cast<const float*>(tpH), S, NT, sl, u_sl, lane, g4);
  }
  // SEQ: a pass reads tiles 0 .. OT of its own tile and transform only, all written by then -- nothing to clear
  template <bool SEQ, bool HM>
  static __device__ __forceinline__ void clear(State& S) {
    if (!SEQ) {
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
#pragma unroll
          for (int r = 0; r < 4; ++r) S.act[k][ot][r] = 0.f;
    }
    if (!HM) {
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) S.head[ot][r] = 0.f;
    }
  }
  static __host__ __device__ int lds_floats(const SfDev& m, bool cp) {
    const int nb = m.NB < 2 ? m.NB : 2;
    return nb * (cp ? m.nT16 * (m.nT16 + 1) / 2 : m.nT16 * m.nT16) * 256;
  }
};

// ---------------------------------------------------------------------------------------------------------------
// Fused first layer (PREC = 2; fp32, unrolled kernels with the context table).  nflows' MADE has NO activation between the
// initial layer and the first block's linear (oracle/flows.py::_made: h = W0 u + b0 + Wc e + bc; then h = tanh(W1 h + b1), ...),
// so the two are one affine map of the finished dimensions:
//     W1 (W0 u + c0) + b1  =  W' u + c0',     W' = (W1 o M)(W0 o M0)  [H x D],     c0' = b1 + (W1 o M) c0  [per galaxy and transform]
// W' is computed once per parameter update (k_maf_fuse16, in fp64, rounded to fp32: image block o16_wp), c0' once per galaxy
// behind c0 in the context table (k_maf_ctab16).
// The first layer is not a matrix product here: a hidden unit of degree k sees u_1 .. u_k only, so a 16-input MFMA pass over it
// would be ~90 % structural zeros.  A transform instead starts with the pre-activations of ALL its tiles in registers (c0' from
// the table), and whenever the dimension of degree k is finished every lane adds W'[rows of tile ot, slot of degree k] . w_k
// into each tile ot >= k - 1 (one LDS fragment and two v_pk_fma_f32 per tile; only the update of tile k - 1, the next pass's,
// is on the dependent chain).  k_maf_fuse16 stores exactly those columns, in degree order, as one float4 per row group:
// entry sf_wp16_entry(NT, k, ot).  A pass then cost 4 (OT + 1) + 4 fp32 MFMAs with the head tile (56 per tile and transform for cfg1, against
// 72 with the first layer on the matrix pipe and 112 unfused), and its chain is tanh -> W1[OT, OT] -> tanh -> head -> w.
// The draw state is handed to the passes in the transform's DEGREE order (sf_transform16g): written once per transform to the
// sample's row in LDS in physical slot order and read back by degree, every finished dimension written to its slot there --
// the passes themselves carry no runtime slot select and no write-back into a tile-layout quad.  Same function of the same
// parameters as the two-layer form to fp32 rounding (parity rows: given noise, draw for draw).
// Head rows: per-lane packed FMAs, not the matrix pipe.  The head TILE of the two-layer passes (o16_wh: the rows of all slots as
// one 16-row MFMA output) spends 4 MFMAs = 128 cycles per pass on a tile of which 10 of 16 output rows exist and a row of degree
// d reads only the tiles below d - 1; on gfx950 an fp32 MFMA holds the SIMD like the same FLOPs of v_pk_fma_f32 and nothing
// overlaps it.  Here the state carries one (a, m) accumulator per degree 2 .. D (SfPass16G::ham, zero at the start of a
// transform), and pass OT adds the tile it has just finished into the accumulator of EVERY degree >= OT + 2: its own first (four
// packed FMAs, rows r = 0 .. 3 in order; three where the tile's row 3 is empty), then the sum over the four row groups
// (xor 16, xor 32) and the head bias last -- the order of sf_head_acc + sf_sum4groups in the per-lane passes -- and the later
// degrees' in the shadow of the cross-lane sums.  At D = 5 that is 74 MACs = 37 v_pk_fma_f32 per lane and transform in place of
// 14 MFMAs.  Operands: 32 floats [g4][r][a|m] per (tile, degree) behind the compact image (sf_hr16_entry; SfDev::t16h_stride),
// every offset an immediate.  Registers: the accumulators of the later degrees and the rank-1 updates of the later tiles are
// PINNED in the pass that computes them (an empty asm statement on the value): their first reader is a later pass behind the
// branch of the finish, and the compiler otherwise sinks the FMAs there and keeps the fragments, and a broadcast copy of the
// tile, alive until then (128 VGPRs and 100 - 140 B of scratch instead of 127 / 0 in the flagship).
// ---------------------------------------------------------------------------------------------------------------
struct SfPass16G {
  f32x4 act[4];        // output of block 0 = input of block 1; [tile]
  f32x4 pre[4];        // block 0's pre-activation of tile ot: c0' + the rank-1 updates of the dimensions finished so far
  f32x2 ham[4];        // [q]: head rows (a, m) of degree q + 2: this lane's products with the tiles finished so far (its row group's share)
  const float* c0p;    // this draw's c0' rows of the transform
  bool tab;
};
// Head-row entry of (hidden tile ot, degree k >= ot + 2) in the fused kernels' head-row region: tiles in order, each with its
// degrees ot + 2 .. D; 32 floats [g4][r][a|m] (a lane reads its row group's two float4; the four groups of a sample read 128
// contiguous bytes, and every lane of a group the same address: a broadcast)
__host__ __device__ constexpr int sf_hr16_entry(int D, int ot, int k) { return ot * (D - 1) - ot * (ot - 1) / 2 + (k - ot - 2); }
__host__ __device__ constexpr int sf_hr16_entries(int D) { return D * (D - 1) / 2; }
// acc += (a_r, m_r) v_r, r = 0 .. 3 in order, as packed FMAs (sf_head_acc's order); SKIP: row 3 is a structural zero (sf_mma16k)
template <bool SKIP>
__device__ __forceinline__ f32x2 sf_head_acck(f32x2 acc, const float4& h01, const float4& h23, const f32x4& v) {
  acc = __builtin_elementwise_fma(f32x2{h01.x, h01.y}, f32x2{v[0], v[0]}, acc);
  acc = __builtin_elementwise_fma(f32x2{h01.z, h01.w}, f32x2{v[1], v[1]}, acc);
  acc = __builtin_elementwise_fma(f32x2{h23.x, h23.y}, f32x2{v[2], v[2]}, acc);
  if constexpr (!SKIP) acc = __builtin_elementwise_fma(f32x2{h23.z, h23.w}, f32x2{v[3], v[3]}, acc);
  return acc;
}
// W' fragment entry of (input degree k, hidden tile ot >= k - 1): degrees in order, each with its tiles k - 1 .. NT - 1
__host__ __device__ constexpr int sf_wp16_entry(int NT, int k, int ot) { return (k - 1) * NT - (k - 1) * (k - 2) / 2 + ot - (k - 1); }
// the sample's row of the draw-state scratch (floats; 20, not 16: the per-degree reads of 16 samples hit 16 different banks)
#define SF_G16_ROW 20
#define SF_G16_SCR (16 * SF_G16_ROW)   // per wave
// c0' of every tile of the transform into the pre-activations (table path: requested before the staging barriers)
template <int NT>
__device__ __forceinline__ void sf_pre16g_load(SfPass16G& S, int g4) {
#pragma unroll
  for (int ot = 0; ot < NT; ++ot) S.pre[ot] = *reinterpret_cast<const f32x4*>(S.c0p + ot * 16 + 4 * g4);
}
// acc += w . v, as two packed FMAs
__device__ __forceinline__ f32x4 sf_rank1(const f32x4& acc, const float4& w, float v) {
  const f32x2 vv = {v, v};
  const f32x2 lo = __builtin_elementwise_fma(f32x2{w.x, w.y}, vv, f32x2{acc[0], acc[1]});
  const f32x2 hi = __builtin_elementwise_fma(f32x2{w.z, w.w}, vv, f32x2{acc[2], acc[3]});
  return f32x4{lo[0], lo[1], hi[0], hi[1]};
}
// this lane's fragments of W'[., slot of degree K] for the tiles K - 1 .. NT - 1 (requested before the value they multiply exists)
template <int NT, int K>
struct SfWpCols {
  float4 w[NT - K + 1];
  __device__ __forceinline__ void load(const float* tp, int o_wp, int g4) {
#pragma unroll
    for (int q = 0; q <= NT - K; ++q) w[q] = *reinterpret_cast<const float4*>(tp + o_wp + sf_wp16_entry(NT, K, K - 1 + q) * 16 + 4 * g4);
  }
  // the finished dimension w_K into every tile that sees it: tile K - 1 first (the next pass starts from it)
  __device__ __forceinline__ void apply(SfPass16G& S, float wv) const {
#pragma unroll
    for (int q = 0; q <= NT - K; ++q) {
      S.pre[K - 1 + q] = sf_rank1(S.pre[K - 1 + q], w[q], wv);
      // (pinned here: the compiler otherwise sinks the update of a later tile into the pass that reads it, across the branch of
      //  the finish, and holds the fragment and the value until then)
      if (q > 0) asm volatile("" : "+v"(S.pre[K - 1 + q]));
    }
  }
};
// Tiles whose rows 3, 7, 11, 15 are empty (SfDev::m16_k3: groups of <= 12 units, the trailing K3 tiles): register 3 of the tile
// is a structural zero in every lane, so the k-step that reads it (sf_mma16: register j is the B operand of step j) and its
// tanh are not issued.  SKIP = false is sf_mma16 / sf_tanh4, bit for bit.
template <bool SKIP>
__device__ __forceinline__ f32x4 sf_mma16k(float4 w, const f32x4& in, f32x4 acc) {
  acc = SF_MFMA16(w.x, in[0], acc);
  acc = SF_MFMA16(w.y, in[1], acc);
  acc = SF_MFMA16(w.z, in[2], acc);
  if constexpr (!SKIP) acc = SF_MFMA16(w.w, in[3], acc);
  return acc;
}
template <bool SKIP>
__device__ __forceinline__ f32x4 sf_tanh4k(const f32x4& b) {
  if constexpr (!SKIP) {
    return sf_tanh4(b);
  } else {
    const f32x2 one = {1.0f, 1.0f}, m2 = {-2.0f, -2.0f};
    const f32x2 e01 = f32x2{__builtin_amdgcn_exp2f(b[0]), __builtin_amdgcn_exp2f(b[1])} + one;
    const float e2 = __builtin_amdgcn_exp2f(b[2]) + 1.0f;
    const f32x2 r01 = {__builtin_amdgcn_rcpf(e01[0]), __builtin_amdgcn_rcpf(e01[1])};
    const f32x2 o01 = __builtin_elementwise_fma(r01, m2, one);
    return f32x4{o01[0], o01[1], __builtin_fmaf(__builtin_amdgcn_rcpf(e2), -2.0f, 1.0f), 0.f};
  }
}
// One pass of the fused kernels: degree group in tile OT (degree OT + 1), new dimension = degree OT + 2 in physical slot sl.
// Returns the finished value (every row group of the sample holds it) after adding it into the later tiles.
// K3: the flow's m16_k3 -- tile it >= NT - K3 is read with three k-steps (second block and head rows alike).
template <int OT, int NB, int NT, int K3 = 0>
__device__ __forceinline__ float sf_pass16g(const SfDev& m, const float* tp, const float* tpF, const float* hr, SfPass16G& S, int sl,
                                            const float* scr, int lane, int g4) {
  constexpr bool SK = OT >= NT - K3;   // this pass's own tile
  constexpr int D = NT + 1, NH = D - (OT + 1);   // head-row entries of tile OT: degrees OT + 2 .. D, this pass's own first
  // this row group's head rows of (tile OT, degree OT + 2 + q); a tile with an empty row 3 needs three of the four (a, m) pairs
  float4 h01[NH], h23[NH];
#pragma unroll
  for (int q = 0; q < NH; ++q) {
    const float* p = hr + sf_hr16_entry(D, OT, OT + 2 + q) * 32 + g4 * 8;
    h01[q] = *reinterpret_cast<const float4*>(p);
    if constexpr (SK) { const float2 t = *reinterpret_cast<const float2*>(p + 4); h23[q] = float4{t.x, t.y, 0.f, 0.f}; }
    else h23[q] = *reinterpret_cast<const float4*>(p + 4);
  }
  const float ba = tp[m.o16_hvb + 2 * sl], bm = tp[m.o16_hvb + 2 * sl + 1];
  const float u_in = scr[sl];   // the draw's value of this degree: still in its slot of the sample's row (no pass before this one wrote it)
  float4 fw[OT + 1];
  f32x4 b1;
  if (NB == 2) {
    b1 = sf_ld4(tp + m.o16_bk[1] + (OT * 4 + g4) * 4);
#pragma unroll
    for (int it = 0; it <= OT; ++it) fw[it] = sf_w16f<true>(tpF, NT, OT, it, lane);
  }
  SfWpCols<NT, (OT + 2 <= NT ? OT + 2 : NT)> wu;   // (the last pass's dimension feeds nothing)
  if constexpr (OT + 2 <= NT) wu.load(tp, m.o16_wp, g4);
  __builtin_amdgcn_sched_barrier(0);
  if (NB == 2) {
    // tiles finished in earlier passes: not on the chain   (`it` is static after unrolling: one of the two forms remains)
#pragma unroll
    for (int it = 0; it < OT; ++it) b1 = it >= NT - K3 ? sf_mma16k<true>(fw[it], S.act[it], b1) : sf_mma16k<false>(fw[it], S.act[it], b1);
  }
  f32x4 last = sf_tanh4k<SK>(S.pre[OT]);
  if (NB == 2) {
    S.act[OT] = last;
    b1 = sf_mma16k<SK>(fw[OT], last, b1);
    last = sf_tanh4k<SK>(b1);
  }
  // head rows of this pass's degree: the finished tile into its accumulator, then the four row groups and the bias -- the order
  // of sf_head_acc + sf_sum4groups in the per-lane passes (tile ascending, r ascending, xor-16 then xor-32, bias last)
  const f32x2 pam = sf_head_acck<SK>(S.ham[OT], h01[0], h23[0], last);
  const float sa = sf_sum4groups(pam[0]), sm = sf_sum4groups(pam[1]);
  // off the chain, in the shadow of the cross-lane sums: the same tile into the accumulators of the later degrees
#pragma unroll
  for (int q = 1; q < NH; ++q) {
    S.ham[OT + q] = sf_head_acck<SK>(S.ham[OT + q], h01[q], h23[q], last);
    // (pinned here: left to itself the compiler sinks these FMAs into the pass that first reads the accumulator, across the
    //  branch of the finish, and keeps this tile's fragments and a broadcast copy of `last` in registers until then)
    asm volatile("" : "+v"(S.ham[OT + q]));
  }
  const float av = ba + sa, mv = bm + sm;
  const float wv = sf_div(u_in - mv, sf_scale16(m, av));
  if constexpr (OT + 2 <= NT) wu.apply(S, wv);
  return wv;
}
// One transform of one tile of 16 draws (k_maf_samp16 / k_maf_find16s, PREC 2).  u: the draw in tile layout (lane (s, g4) holds
// physical slots 4 g4 .. 4 g4 + 3), in and out; scr: the sample's row of the wave's scratch; S.pre: c0' of the transform; hr: the
// transform's head-row region.
template <int NB, int DD, int K3 = 0>
__device__ __forceinline__ void sf_transform16g(const SfDev& m, const float* tp, const float* tpF, const float* hr, SfPass16G& S,
                                                int dsl, f32x4& u, float* scr, int lane, int g4) {
  constexpr int NT = DD - 1;
#pragma unroll
  for (int q = 0; q < NT; ++q) S.ham[q] = f32x2{0.f, 0.f};
  // the 4 row groups write the same row: afterwards every lane reads any slot of its sample (one per degree, slots in SGPRs)
  *reinterpret_cast<f32x4*>(scr + 4 * g4) = u;
  int sl[DD];
#pragma unroll
  for (int q = 0; q < DD; ++q) sl[q] = __builtin_amdgcn_readlane(dsl, q);
  {
    // degree 1 depends on the context only (head bias)
    SfWpCols<NT, 1> wu;
    wu.load(tp, m.o16_wp, g4);
    const float av = tp[m.o16_hvb + 2 * sl[0]], mv = tp[m.o16_hvb + 2 * sl[0] + 1];
    const float wv = sf_div(scr[sl[0]] - mv, sf_scale16(m, av));
    wu.apply(S, wv);
    scr[sl[0]] = wv;
  }
  __builtin_amdgcn_sched_barrier(0);   // (the first pass's operands are requested once the degree-1 columns are spent: registers)
  auto pass = [&](auto otc) {
    constexpr int OT = decltype(otc)::value;
    // every degree's incoming value is read from the row in the pass that needs it, not held from the transform's start
    scr[sl[OT + 1]] = sf_pass16g<OT, NB, NT, K3>(m, tp, tpF, hr, S, sl[OT + 1], scr, lane, g4);
  };
  pass(std::integral_constant<int, 0>{});
  if constexpr (DD >= 3) pass(std::integral_constant<int, 1>{});
  if constexpr (DD >= 4) pass(std::integral_constant<int, 2>{});
  if constexpr (DD >= 5) pass(std::integral_constant<int, 3>{});
  u = *reinterpret_cast<const f32x4*>(scr + 4 * g4);
}
template <> struct SfHid16<2> {
  using State = SfPass16G;
  // (no part A, no blocks behind it: these kernels stage the compact fused image, sf_stage16c in sf_maf16.hip)
};

// Direct global -> LDS copy (global_load_lds_dwordx4: no staging registers, no ds_write) of one 4 KiB group by one wave: the LDS
// destination of a wave-instruction is its (wave-uniform) base l + lane * 16 bytes, g is the lane's own source address.  The images
// are padded to whole groups (sf_layout.cpp), so a group takes ONE address and four immediate offsets (the immediate applies to
// the global and to the LDS address alike).  The caller waits for vmcnt(0) before its barrier.
__device__ __forceinline__ void sf_copy_group16(const float4* g, float4* l) {
  __builtin_amdgcn_global_load_lds((const void*)g, (void __attribute__((address_space(3)))*)l, 16, 0, 0);
  __builtin_amdgcn_global_load_lds((const void*)g, (void __attribute__((address_space(3)))*)l, 16, 1024, 0);
  __builtin_amdgcn_global_load_lds((const void*)g, (void __attribute__((address_space(3)))*)l, 16, 2048, 0);
  __builtin_amdgcn_global_load_lds((const void*)g, (void __attribute__((address_space(3)))*)l, 16, 3072, 0);
}

// Staging of one transform's operands (all four waves; the caller brackets it with barriers): part A of the fp32 image
// (`a_floats` floats: input layer, biases, head rows; + the context block without a table) in 4 KiB groups -- ONE address, four
// immediate offsets -- and behind it the hidden blocks: PREC 0 the split-bf16 image (4 KiB groups), PREC 1 the fp32 blocks
// of the full image, 1 KiB (one 16 x 16 block) per wave-instruction.  Direct global -> LDS copies.
template <int PREC, bool CP>
__device__ __forceinline__ void sf_stage16(const SfDev& m, int t, int a_floats, int wave) {
  const int lane_ = threadIdx.x & 63;
  const int ga = a_floats >> 10;
  const float4* __restrict__ sa = reinterpret_cast<const float4*>(m.packed16 + (size_t)t * m.t16_stride);
  float4* __restrict__ d4 = reinterpret_cast<float4*>(sf_lds16);
  if constexpr (PREC == 0) {
    const int gb = m.t16B_stride >> 10;
    const float4* __restrict__ sb = reinterpret_cast<const float4*>(m.packed16B + (size_t)t * m.t16B_stride);
    for (int gi = __builtin_amdgcn_readfirstlane(wave); gi < ga + gb; gi += 4) {
      sf_copy_group16((gi < ga ? sa + gi * 256 : sb + (gi - ga) * 256) + lane_, d4 + gi * 256);
    }
  } else {
    for (int gi = __builtin_amdgcn_readfirstlane(wave); gi < ga; gi += 4) {
      sf_copy_group16(sa + gi * 256 + lane_, d4 + gi * 256);
    }
    const int NT = m.nT16, nb = m.NB < 2 ? m.NB : 2;
    const int per = CP ? NT * (NT + 1) / 2 : NT * NT;
    float4* __restrict__ dF = d4 + (a_floats >> 2);
    for (int e = __builtin_amdgcn_readfirstlane(wave); e < nb * per; e += 4) {
      const int k = e >= per ? 1 : 0, ee = e - k * per;
      int src_blk = ee;
      if (CP) {  // entry ot (ot + 1) / 2 + it  ->  block ot * NT + it   (NT <= 4)
        const int ot = ee >= 6 ? 3 : (ee >= 3 ? 2 : (ee >= 1 ? 1 : 0));
        src_blk = ot * NT + (ee - ot * (ot + 1) / 2);
      }
      const int owk = k ? m.o16_wk[1] : m.o16_wk[0];  // (no dynamic index into the descriptor)
      const float4* g = sa + ((owk >> 2) + src_blk * 64) + lane_;
      __builtin_amdgcn_global_load_lds((const void*)g, (void __attribute__((address_space(3)))*)(dF + e * 64), 16, 0, 0);
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the copies have landed
}

// ---------------------------------------------------------------------------------------------------------------
// Steps that the kernels of sf_maf16.hip share.
// ---------------------------------------------------------------------------------------------------------------
// The pass functions of the non-persistent fp32 kernel (k_maf_inv16: sf_pass16 / sf_pass16_span, state SfPass16 with c0 and the
// log-determinant) behind the interface of SfHid16, so that sf_pass16_tiles dispatches them too.  No operands behind part A, no
// placement variants, head rows as per-lane dot products: tpH, CP, HM and next_ot do not apply.
struct SfHid16Plain {
  using State = SfPass16;
  template <int OT, int NB, bool CP, bool HM>
  static __device__ __forceinline__ void pass(const SfDev& m, const float* tp, const void*, State& S, int NT, int sl, float u_sl,
                                              int lane, int g4, int) {
    sf_pass16<OT, NB>(m, tp, S, NT, sl, u_sl, lane, g4);
  }
  template <int LO, int HI, int NB>
  static __device__ __forceinline__ void span(const SfDev& m, const float* tp, const void*, State& S, int NT, int sl, float u_sl,
                                              int lane, int g4) {
    sf_pass16_span<LO, HI, NB>(m, tp, S, NT, sl, u_sl, lane, g4);
  }
};

// g16_tile / g16_lo (last and first hidden tile of each degree's group) packed 2 bits per degree: static indexing keeps
// them in SGPRs
struct SfTiles16 {
  uint32_t hi = 0, lo = 0;
  __device__ __forceinline__ void pack(const SfDev& m) {
#pragma unroll
    for (int q = 0; q < SF_DMAX; ++q) {
      hi |= (uint32_t)(m.g16_tile[q] & 3) << (2 * q);
      lo |= (uint32_t)(m.g16_lo[q] & 3) << (2 * q);
    }
  }
  __device__ __forceinline__ int tile(int p) const { return (int)((hi >> (2 * (p - 1))) & 3u); }  // last tile of degree p
};
// The pass of degree p >= 2 (new dimension in physical slot sl) of a kernel that learns the tiles at run time: picks the pass
// function from (first tile, last tile) of the degree group.  HID: operand form (SfHid16<PREC>, SfHid16Plain); SPAN: contiguous
// placement (the aligned-placement kernels carry no span code); D: the flow's dimension (the last pass has no next tile).
template <typename HID, int NB, bool SPAN, bool HM>
__device__ __forceinline__ void sf_pass16_tiles(const SfDev& m, const float* tp, const void* tpH, typename HID::State& S, int NT,
                                                const SfTiles16& tb, int p, int D, int sl, float u_sl, int lane, int g4) {
  const uint32_t hi_t = (tb.hi >> (2 * (p - 1))) & 3u;
  const uint32_t lo_t = SPAN ? (tb.lo >> (2 * (p - 1))) & 3u : hi_t;
  const int nx = p < D ? (int)((tb.hi >> (2 * p)) & 3u) : -1;  // tile of the next pass (aligned placement)
  switch (lo_t * 4 + hi_t) {
    case 0: HID::template pass<0, NB, !SPAN, HM>(m, tp, tpH, S, NT, sl, u_sl, lane, g4, nx); break;
    case 5: HID::template pass<1, NB, !SPAN, HM>(m, tp, tpH, S, NT, sl, u_sl, lane, g4, nx); break;
    case 10: HID::template pass<2, NB, !SPAN, HM>(m, tp, tpH, S, NT, sl, u_sl, lane, g4, nx); break;
    case 15: HID::template pass<3, NB, !SPAN, HM>(m, tp, tpH, S, NT, sl, u_sl, lane, g4, nx); break;
    // degree groups that straddle tiles (contiguous packing)
    case 1: if constexpr (SPAN) HID::template span<0, 1, NB>(m, tp, tpH, S, NT, sl, u_sl, lane, g4); break;
    case 2: if constexpr (SPAN) HID::template span<0, 2, NB>(m, tp, tpH, S, NT, sl, u_sl, lane, g4); break;
    case 3: if constexpr (SPAN) HID::template span<0, 3, NB>(m, tp, tpH, S, NT, sl, u_sl, lane, g4); break;
    case 6: if constexpr (SPAN) HID::template span<1, 2, NB>(m, tp, tpH, S, NT, sl, u_sl, lane, g4); break;
    case 7: if constexpr (SPAN) HID::template span<1, 3, NB>(m, tp, tpH, S, NT, sl, u_sl, lane, g4); break;
    default: if constexpr (SPAN) HID::template span<2, 3, NB>(m, tp, tpH, S, NT, sl, u_sl, lane, g4); break;
  }
}

// One transform of one tile of 16 draws with the two-layer pass functions UNROLLED (k_maf_samp16<.., DD> / k_maf_find16s, PREC 0
// and 1; sf_transform16g is the fused form): aligned placement with degree p alone in tile p - 2, head rows on the matrix pipe, so
// pass p is HID::pass<p - 2> with the next tile known.  u: the draw in tile layout, in and out; S.c0n / S.hdone as the caller set
// them for the tile.
template <typename HID, int NB, int DD>
__device__ __forceinline__ void sf_transform16s(const SfDev& m, const float* tp, const void* tpH, typename HID::State& S, int NT,
                                                int dsl, f32x4& u, int lane, int g4) {
  HID::template clear<true, true>(S);
#pragma unroll
  for (int r = 0; r < 4; ++r) S.ut[r] = 0.f;
  {
    const int sl = __builtin_amdgcn_readlane(dsl, 0);
    sf_pass16_deg1(m, tp, S.ut, sl, sf_slot16_own(u, sl), g4);
  }
  auto seq_pass = [&](auto otc) {
    constexpr int OT = decltype(otc)::value;
    const int sl = __builtin_amdgcn_readlane(dsl, OT + 1);
    // (only the owning row group keeps what is computed from the slot's value)
    HID::template pass<OT, NB, true, true>(m, tp, tpH, S, NT, sl, sf_slot16_own(u, sl), lane, g4, OT + 2 < DD ? OT + 1 : -1);
  };
  seq_pass(std::integral_constant<int, 0>{});
  if constexpr (DD >= 3) seq_pass(std::integral_constant<int, 1>{});
  if constexpr (DD >= 4) seq_pass(std::integral_constant<int, 2>{});
  if constexpr (DD >= 5) seq_pass(std::integral_constant<int, 3>{});
  u = S.ut;
}

// Item `it` of a launch without the device queue (k_maf_inv16, k_maf_find16s), row group g4's share of it:
//   given noise (a.z_in): row `it` of z and of x;
//   else attempt att of listed slot ps = it >> log2_attempts (A, a power of two, consecutive items share a slot): att from
//   a.att_list (resolve) or a.attempt + it % A, the draw's noise from Philox block g4 = dimensions 4*g4 .. 4*g4+3.
struct SfItem16 {
  f32x4 u;        // tile layout: physical slots 4*g4 .. 4*g4+3 (zeros past D)
  long gal, ps;   // context row; index into the launch's slot list
  uint32_t slot, att;   // (slot ids fit 32 bits: checked by the API)
};
__device__ __forceinline__ SfItem16 sf_item16(const SfDev& m, const SfSampleArgsHost& a, long it, int g4) {
  SfItem16 I;
  I.ps = it >> a.log2_attempts;
  I.slot = a.z_in ? (uint32_t)it : (a.slots ? a.slots[I.ps] : (uint32_t)(a.slot_base + I.ps));
  I.att = a.att_list ? a.att_list[I.ps] : a.attempt + (uint32_t)(it & ((1L << a.log2_attempts) - 1));
  I.gal = a.z_in ? it : (long)(I.slot / (uint32_t)a.S);
  float z4[4];
  if (a.z_in) {
#pragma unroll
    for (int r = 0; r < 4; ++r) z4[r] = (4 * g4 + r < m.D) ? a.z_in[it * m.D + 4 * g4 + r] : 0.f;
  } else {
    sf_normal4(a.k0, a.k1, (uint64_t)I.slot + a.rng_slot_offset, I.att, (uint32_t)g4, z4);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) I.u[r] = (4 * g4 + r < m.D) ? z4[r] : 0.f;
  return I;
}

// Per-slot constants of the epilogue in LDS, written by the workgroup's first 16 threads (the caller's next barrier publishes
// them): ecb[5 p ..] = {shift, 1 / scale, lo, hi, theta column} of physical slot p.  (Read from global memory where they are used
// they cost every iteration two dependent L2 round trips.)  C2S: also the table theta column -> physical slot behind them, at
// int index 80 + column (the row-linear stores of k_maf_samp16); the block is then 96 words, else 80.
template <bool C2S>
__device__ __forceinline__ void sf_ecb16_build(float* ecb, const SfDev& m, const SfSampleArgsHost& a) {
  if (threadIdx.x < 16) {
    const int p = threadIdx.x;
    const bool on = p < m.D;
    const int td = on ? (int)m.cst[m.c_tdim + p] : 0;
    ecb[p * 5 + 0] = on ? m.cst[m.c_pshift + p] : 0.f;
    ecb[p * 5 + 1] = on ? __builtin_amdgcn_rcpf(m.cst[m.c_pscale + p]) : 0.f;
    ecb[p * 5 + 2] = (on && a.lo) ? a.lo[td] : -3.4e38f;
    ecb[p * 5 + 3] = (on && a.lo) ? a.hi[td] : 3.4e38f;
    reinterpret_cast<int*>(ecb)[p * 5 + 4] = td;
    if (C2S && on) reinterpret_cast<int*>(ecb)[80 + td] = p;
  }
}
// bit s = every row group of sample s says ok, and the sample is a valid item (each lane owns 4 physical slots of its sample; a
// draw is accepted when all 4 row groups agree)
__device__ __forceinline__ uint32_t sf_accept16(bool ok, bool valid) {
  const unsigned long long okb = __ballot(ok);
  return (uint32_t)(okb & (okb >> 16) & (okb >> 32) & (okb >> 48) & 0xffffull) & (uint32_t)(__ballot(valid) & 0xffffull);
}
// Un-standardise this lane's four slots of u with the constants of sf_ecb16_build (th, and their theta columns tdc) and test
// them: finite (NaN compares false) and inside the box; slots >= D: u = 0, shift = 0, 1 / scale = 0 -> 0, always inside.
// The tile's accepted mask is sf_accept16 of the result (a kernel may still veto a lane in between).
__device__ __forceinline__ bool sf_theta_box16(const float* ecb, const f32x4& u, int g4, float (&th)[4], int (&tdc)[4]) {
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float* e = ecb + (4 * g4 + r) * 5;
    th[r] = (u[r] - e[0]) * e[1];
    tdc[r] = reinterpret_cast<const int*>(e)[4];
    ok = ok && (fabsf(th[r]) <= 3.0e38f) && (th[r] >= e[2]) && (th[r] <= e[3]);
  }
  return ok;
}
