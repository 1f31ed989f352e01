// sf_maf16.hip -- incremental MAF inverse / sampler on v_mfma_f32_16x16x4_f32 (16-row granularity).
//
// Same algorithm and the same C-ABI entry points as k_inverse<MafOps> (sf_flows.h, sf_inst_templates.h); only
// the tile geometry differs so that a 12-13 unit MADE degree group costs one 16-row tile instead of a 32-row one:
//   lane l: sample s = l & 15 of a 16-sample tile, row group g4 = l >> 4; a tile is 4 VGPRs, a[r] = row 4*g4 + r
//   C/D layout of the 16x16x4 MFMA == B-operand order of the next layer (k-step r <-> register r), so the
//   activations stay in registers exactly as in the 32-row engine.
//   weights: float4[(ot*IT + it)*64 + l] = W[ot*16 + (l&15)][it*16 + 4*(l>>4) + r], r = 0..3 (sf_layout.cpp)
// One wave = one tile of 16 draws, 4 waves per workgroup; the transform's 16-row image is staged in LDS.  The
// draw itself also lives in tile layout (lane (s, g4) owns physical slots 4*g4..4*g4+3), so Philox, the box test
// and the output writes are split over the four row groups instead of being repeated by them.
// The device primitives (pass functions, operand forms, staging, the steps the kernels share) are in sf_maf16_pass.h; this
// file holds the kernels, their launchers and the shape plan (SfMaf16Plan) that picks among them.
#include "sf_maf16_pass.h"

template <int NB, bool SPAN>
__global__ __launch_bounds__(256, 3) void k_maf_inv16(SfDev m, SfSampleArgsHost a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = lane & 15, g4 = lane >> 4;
  // (no early exit: every wave takes part in the staging barriers)
  const long item = ((long)blockIdx.x * 4 + wave) * 16 + s;
  const bool valid = item < a.n_items;
  const long it = valid ? item : a.n_items - 1;
  // tile layout: this lane holds physical slots 4*g4 .. 4*g4+3 of sample s
  const SfItem16 I = sf_item16(m, a, it, g4);
  f32x4 u = I.u;
  const uint32_t slot = I.slot, att_mine = I.att;
  const long gal = I.gal, ps_idx = I.ps;
  const float* xr = a.x + gal * m.C;
  float logdet = 0.f;

  // standardised context: tile 0 is kept in registers across the transforms
  const float* ctg = (m.ctab && !a.z_in) ? m.ctab + (size_t)gal * m.T * m.ctab_R : nullptr;  // wave-uniform choice
  f32x4 ct0;
  if (!ctg) ct0 = sf_ctx_tile16(m, xr, 0, g4);

  const int NT = m.nT16;
  // activation tiles of the three layers: a pass only reads tiles that an earlier pass of the SAME transform has
  // written (tile index <= its own), so they are cleared once, not per transform
  SfPass16 S;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int ot = 0; ot < 4; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r) S.act[k][ot][r] = 0.f;
  SfTiles16 tiles;
  tiles.pack(m);
  for (int t = m.T - 1; t >= 0; --t) {
    // ---- stage this transform's whole 16-row image, 4 KiB groups dealt to the four waves
    __syncthreads();
    {
      const float4* __restrict__ s4 = reinterpret_cast<const float4*>(m.packed16 + (size_t)t * m.t16_stride);
      float4* __restrict__ d4 = reinterpret_cast<float4*>(sf_lds16);
      const int n4 = m.t16_stride >> 2;
      const int lane_ = threadIdx.x & 63;
      const int ngroups = n4 >> 8;
      for (int gi = __builtin_amdgcn_readfirstlane(wave); gi < ngroups; gi += 4) sf_copy_group16(s4 + gi * 256 + lane_, d4 + gi * 256);
      __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0), other counters untouched: the copies have landed
    }
    __syncthreads();
    const float* tp = sf_lds16;
    // context product hoisted out of the passes: c0 = b0 + bc + Wc e
    if (ctg) {  // per-galaxy table (sf_flow_prepare_context): same values, computed once per galaxy
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
        if (ot < NT) S.c0[ot] = *reinterpret_cast<const f32x4*>(ctg + (size_t)t * m.ctab_R + ot * 16 + 4 * g4);
    } else {
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
        if (ot < NT) {
          S.c0[ot] = sf_ld4(tp + m.o16_b0 + (ot * 4 + g4) * 4);
          S.c0[ot] = sf_mma16(sf_w16(tp + m.o16_wc, m.nC16, ot, 0, lane), ct0, S.c0[ot]);
        }
      for (int ic = 1; ic < m.nC16; ++ic) {
        const f32x4 ct = sf_ctx_tile16(m, xr, ic, g4);
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
          if (ot < NT) S.c0[ot] = sf_mma16(sf_w16(tp + m.o16_wc, m.nC16, ot, ic, lane), ct, S.c0[ot]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) S.ut[r] = 0.f;
    S.ldl = 0.f;
    // physical slot of the dimension with MADE degree p: lane q holds entry q, read back with v_readlane
    const int dsl = (int)m.cst[m.c_dslot + t * SF_DMAX + s];
    {
      const int sl = __builtin_amdgcn_readlane(dsl, 0);
      S.ldl += sf_log(sf_pass16_deg1(m, tp, S.ut, sl, sf_slot16(u, sl, lane), g4));
    }
    for (int p = 2; p <= m.D; ++p) {
      const int sl = __builtin_amdgcn_readlane(dsl, p - 1);
      sf_pass16_tiles<SfHid16Plain, NB, SPAN, false>(m, tp, nullptr, S, NT, tiles, p, m.D, sl, sf_slot16(u, sl, lane), lane, g4);
    }
    logdet -= S.ldl;
    u = S.ut;
  }

  // ---------------------------------------------------------------- un-standardise, box test, outputs
  // each lane owns 4 physical slots of its sample; a draw is accepted when all 4 row groups agree
  float th[4];
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int p = 4 * g4 + r;
    th[r] = 0.f;
    if (p < m.D) {
      const int td = (int)m.cst[m.c_tdim + p];
      th[r] = sf_div(u[r] - m.cst[m.c_pshift + p], m.cst[m.c_pscale + p]);
      ok = ok && (fabsf(th[r]) <= 3.0e38f);  // finite (NaN compares false)
      if (a.lo) ok = ok && (th[r] >= a.lo[td]) && (th[r] <= a.hi[td]);
    }
  }
  if (a.att_list && att_mine == 0xffffffffu) ok = false;  // no attempt to resolve: straight to the rejected list
  const uint32_t acc16 = sf_accept16(ok, valid);
  const bool accepted = (acc16 >> s) & 1u;
  if (a.z_in) {
    if (valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g4 + r < m.D) a.out[item * m.D + (int)m.cst[m.c_tdim + 4 * g4 + r]] = th[r];
      if (a.logdet_out && g4 == 0) a.logdet_out[item] = logdet - m.logdet0;
    }
  } else if (a.best) {
    if (accepted && g4 == 0) atomicMin(&a.best[ps_idx], att_mine);
  } else if (a.count) {
    const long g_first = __shfl(gal, 0, 64);
    const long g_last = __shfl(gal, 15, 64);
    if (g_first == g_last) {
      if (lane == 0 && acc16) atomicAdd(&a.count[g_first], (int)__popc(acc16));
    } else if (accepted && g4 == 0) {
      atomicAdd(&a.count[gal], 1);
    }
  } else {
    // A <= 16 consecutive items hold attempts att..att+A-1 of one slot: the lowest accepted one wins
    const int A = a.attempts_per_slot;
    const int grp0 = (s / A) * A;
    const uint32_t gmask = (acc16 >> grp0) & ((1u << A) - 1u);
    const int first = gmask ? (int)__builtin_ctz(gmask) : -1;
    const int me = s - grp0;
    if (valid) {
      if (g4 == 0 && me == 0 && a.n_drawn && a.attempt > 0) sf_sat_add(&a.n_drawn[gal], first >= 0 ? first + 1 : A);
      if (me == first) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * g4 + r < m.D) sf_out_store(a, (size_t)slot * m.D + (int)m.cst[m.c_tdim + 4 * g4 + r], th[r]);
      } else if (first < 0 && me == 0 && g4 == 0) {
        const uint32_t pos = atomicAdd(a.n_rejected, 1u);
        a.rejected[pos] = (uint32_t)slot;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Persistent sampler: the same tile pipeline as k_maf_inv16, driven by the device work queue of sf_queue.h.  One
// launch resolves every slot of the dense list (first attempts AND retries); sampler only (no parity hook, no
// acceptance mode, no log-determinant).
// Hidden H x H blocks run on split-bf16 MFMA (sf_pass16b); the rest of the arithmetic is fp32 as in k_maf_inv16.
// The two argument blocks are read through the kernarg segment pointer, laundered once per iteration: descriptor
// fields and table entries are then loaded where they are used (scalar-cache hits) instead of being hoisted out of
// the persistent loop and kept in registers for the life of the kernel -- with them live the pass functions spill.
// ---------------------------------------------------------------------------------------------------------------
struct SfSamp16Args {
  SfDev m;
  SfSampleArgsHost a;
};

// Draw tiles per wave and iteration: a workgroup takes 128 items per iteration and every wave walks TWO tiles of 16 draws
// through each staged transform, one after the other -- the queue fetch, the image copy and their barriers are paid once
// per 128 draws instead of once per 64 (together ~20 % of a workgroup's time with one tile per wave); between transforms a
// tile is just its 4 registers of u and its galaxy index.
#define SF_SAMP16_TPW 2
// Offsets of the 16-row sampler image for the shapes of the unrolled kernels (D = DD, DD - 1 hidden tiles of one degree
// group each, NB blocks), as sf_layout.cpp emits them: compile-time constants in those kernels (LDS reads with immediate
// offsets, no descriptor loads inside a pass); the host checks them against the packer's before it picks such a kernel.
template <int NB, int DD>
struct SfFix16 {
  static constexpr int NT = DD - 1;
  static constexpr int o_w0 = 0, o_b0 = NT * 256, o_bk0 = o_b0 + NT * 16, o_bk1 = o_bk0 + NT * 16;
  static constexpr int o_hv = o_b0 + NT * 16 * (1 + NB), o_hvb = o_hv + DD * 128;
  static constexpr int o_wh = (o_hvb + 2 * DD + 3) / 4 * 4, o_bh = o_wh + NT * 256;
  static constexpr int o_wp = (o_bh + 16 + 3) / 4 * 4;
  static constexpr int a_tab = (o_wp + NT * 256 + 1023) / 1024 * 1024;
  static constexpr int entries = NT == 4 ? 6 : (NT == 3 ? 4 : 2);   // (ot, pair) fragments a block keeps: sum of ot / 2 + 1
  static constexpr int oB_wk1 = entries * 512, B_stride = (NB * entries * 512 + 1023) / 1024 * 1024;
  static bool matches(const SfDev& m) {
    return m.nT16 == NT && m.o16_w0 == o_w0 && m.o16_b0 == o_b0 && m.o16_bk[0] == o_bk0 && (NB < 2 || m.o16_bk[1] == o_bk1) &&
           m.o16_hv == o_hv && m.o16_hvb == o_hvb && m.o16_wh == o_wh && m.o16_bh == o_bh && m.o16_wp == o_wp && m.t16_a_tab == a_tab &&
           m.o16B_wk[0] == 0 && (NB < 2 || m.o16B_wk[1] == oB_wk1) && m.t16B_stride == B_stride;
  }
  static __device__ __forceinline__ void apply(SfDev& m) {
    m.nT16 = NT; m.o16_w0 = o_w0; m.o16_b0 = o_b0; m.o16_bk[0] = o_bk0; m.o16_bk[1] = o_bk1; m.o16_hv = o_hv; m.o16_hvb = o_hvb;
    m.o16_wh = o_wh; m.o16_bh = o_bh; m.o16_wp = o_wp; m.t16_a_tab = a_tab; m.o16B_wk[0] = 0; m.o16B_wk[1] = oB_wk1; m.t16B_stride = B_stride;
  }
};

// The same for the compact fused image (sf_layout.h, packed16c): what the PREC 2 kernels stage and read instead of part A and
// the second block.  apply() points the offsets the fused passes use (sf_pass16g / sf_transform16g) into it; the second
// block's fragments start at o_blk.
template <int NB, int DD>
struct SfFixC16 {
  static constexpr int NT = DD - 1, ENT = NT * (NT + 1) / 2;   // W' entries = fragments of a block on and below the diagonal
  static constexpr int o_bk1 = 0, o_hvb = NB == 2 ? NT * 16 : 0, o_bh = o_hvb + (2 * DD + 3) / 4 * 4, o_wh = o_bh + 16;
  static constexpr int o_wp = o_wh + NT * 256, o_blk = o_wp + ENT * 16;
  static constexpr int size = (o_blk + (NB == 2 ? ENT * 256 : 0) + 255) / 256 * 256;
  // behind it, the head rows of the per-lane form (sf_pass16g): sf_hr16_entries(DD) entries of 32 floats, padded to whole groups
  static constexpr int o_hr = size, hr_size = (sf_hr16_entries(DD) * 32 + 255) / 256 * 256, total = size + hr_size;
  // 1 KiB wave-instructions per transform; the groups that hold nothing but the head TILE (o_bh .. o_wp: the matrix-pipe form that
  // these passes no longer read) are not copied
  static constexpr int lds = total + 4 * SF_G16_SCR;   // sf_lds_floats16<2>: then the draw-state scratch of the four waves
  static constexpr int groups = total / 256, dead_lo = (o_bh + 255) / 256, dead_hi = o_wp / 256;
  static bool matches(const SfDev& m) {
    return m.nT16 == NT && m.o16c_bk1 == o_bk1 && m.o16c_hvb == o_hvb && m.o16c_bh == o_bh && m.o16c_wh == o_wh && m.o16c_wp == o_wp &&
           m.o16c_blk == o_blk && m.t16c_stride == size && m.t16h_stride == hr_size;
  }
  static __device__ __forceinline__ void apply(SfDev& m) {
    m.o16_bk[1] = o_bk1; m.o16_hvb = o_hvb; m.o16_wp = o_wp;
  }
};
// LDS floats in front of a sampler kernel's control words / epilogue constants: the staged operands (+ the draw-state scratch)
template <int PREC>
static __host__ __device__ __forceinline__ int sf_lds_floats16(const SfDev& m, bool cp) {
  if constexpr (PREC == 2) return m.t16c_stride + m.t16h_stride + 4 * SF_G16_SCR;   // (then the draw-state scratch of the four waves)
  else return (m.ctab ? m.t16_a_tab : m.t16_a) + SfHid16<PREC>::lds_floats(m, cp);
}
// Staging of one transform's compact image (G KiB; all four waves, the caller brackets it with barriers): direct global -> LDS
// copies, 1 KiB wave-instructions dealt to the four waves.  Groups DEAD_LO .. DEAD_HI - 1 hold only blocks that no PREC 2 kernel
// reads (the head tile and its biases, SfFixC16::dead_lo / dead_hi): they are not copied and their part of the LDS block stays
// UNWRITTEN, while the offsets still span it.  This goes once those blocks leave the image.
template <int G, int DEAD_LO = 0, int DEAD_HI = 0>
__device__ __forceinline__ void sf_stage16c(const float* src, int wave) {
  const float4* __restrict__ g = reinterpret_cast<const float4*>(src) + (threadIdx.x & 63);
  float4* __restrict__ l = reinterpret_cast<float4*>(sf_lds16);
  constexpr int ND = DEAD_HI > DEAD_LO ? DEAD_HI - DEAD_LO : 0;   // groups DEAD_LO .. DEAD_HI - 1 are skipped
  for (int q = __builtin_amdgcn_readfirstlane(wave); q < G - ND; q += 4) {
    const int gi = q < DEAD_LO ? q : q + ND;
    __builtin_amdgcn_global_load_lds((const void*)(g + gi * 64), (void __attribute__((address_space(3)))*)(l + gi * 64), 16, 0, 0);
  }
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the copies have landed
}

// DD > 0 (HM, aligned placement with ONE degree group per tile, D == DD <= 5): the passes of a transform are unrolled
// with the tile of each known at compile time (pass p works on tile p - 2) -- no dispatch, and the per-tile state is
// updated in place instead of being copied into the registers every arm of the switch has to agree on.
// PREC: operand form of the hidden H x H blocks (SfHid16): 0 = split bf16 x3, 1 = fp32.
// Workgroups per CU of the fused-first-layer kernel (PREC 2, D = 5: 30 KB of LDS with the draw-state scratch, 124 VGPRs with the
// pre-activations of every tile in registers).  Round 5, first layer still on the matrix pipe (106 VGPRs): five fit once the
// compiler is held to 96 VGPRs (94 used, no scratch), and measured SLOWER on the headline workload: 2.11-2.15 ms against 2.06 ms
// with four.
#ifndef SF_SAMP16_WG_FUSED
#define SF_SAMP16_WG_FUSED 4
#endif
template <int NB, bool SPAN, bool HM, int DD = 0, int PREC = 0, int K3 = 0>
__global__ __launch_bounds__(256, (SPAN ? 3 : (PREC == 2 ? SF_SAMP16_WG_FUSED : 4))) void k_maf_samp16(SfSamp16Args args_in) {
  static_assert(K3 == 0 || (PREC == 2 && K3 <= DD - 1), "skipped k-steps: the fused passes only, at most every hidden tile");
  static_assert(DD == 0 || (HM && !SPAN && DD >= 2 && DD <= 5), "unrolled passes: head tile, aligned placement, D <= 5");
  static_assert(PREC != 2 || DD >= 3, "fused first layer: unrolled kernels only (m_fix and the compact image's offsets)");
  using HID = SfHid16<PREC>;
  constexpr int TPW = SF_SAMP16_TPW;
  constexpr int IPW = 64 * TPW;
  const int wave = threadIdx.x >> 6;
  using FC = SfFixC16<NB, (PREC == 2 ? DD : 2)>;   // (PREC 2 only: the compact image)
  // with the per-galaxy context table the context block Wc is never read: only the prefix of part A before it is staged
  // (PREC 2: the host launches these kernels only when the packer's sizes are FC's, so the offset is a compile-time one and the
  //  queue's addresses behind it cost no registers)
  unsigned int* ctrl = reinterpret_cast<unsigned int*>(sf_lds16 + (PREC == 2 ? FC::lds : sf_lds_floats16<PREC>(args_in.m, !SPAN)));
  unsigned int pf;
  sf_q_begin<IPW>(args_in.a, ctrl, pf);
  // per-slot constants of the epilogue, once per workgroup, behind the queue's control words
  float* ecb = reinterpret_cast<float*>(ctrl + SF_Q_WORDS(IPW));
  sf_ecb16_build<true>(ecb, args_in.m, args_in.a);
  // (the first sf_q_fetch begins with a barrier: the block is visible to every wave before its first epilogue)
#ifdef SF_Q_STATS
  const unsigned long long qs_k0 = __builtin_amdgcn_s_memtime();
  unsigned long long qs_iters = 0, qs_last_work = 0;
  unsigned long long qs_ph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // [5..9]: the same phases in tail mode
  if (threadIdx.x == 0) atomicMin(&args_in.a.q->stats[10], __builtin_amdgcn_s_memrealtime());  // first start (100 MHz)
#endif
  for (;;) {
    const SfSamp16Args* ap;
    {
      auto kp = __builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(kp));
      ap = (const SfSamp16Args*)kp;
    }
    const SfDev& m_arg = ap->m;
    SfDev m_fix;  // (DD > 0: the descriptor with the image offsets replaced by their compile-time values)
    if constexpr (DD > 0) { m_fix = m_arg; SfFix16<NB, DD>::apply(m_fix); }
    if constexpr (PREC == 2) FC::apply(m_fix);   // (the fused passes read the compact image)
    const SfDev& m = DD > 0 ? m_fix : m_arg;
    const SfSampleArgsHost& a = ap->a;
    const int lane = (threadIdx.x & 63) + sf_opaque_zero();  // lane-derived addresses are recomputed per iteration
    const int s = lane & 15, g4 = lane >> 4;
#ifdef SF_Q_STATS
    const unsigned long long qs_t_top = __builtin_amdgcn_s_memrealtime();
#endif
    if (!sf_q_fetch<IPW, 64>(a, ctrl, pf)) {
#ifdef SF_Q_STATS
      if (threadIdx.x == 0) {
        for (int i = 0; i < 10; ++i) atomicAdd(&a.q->stats[14 + i], qs_ph[i]);  // fetch | prologue | staging | passes | epilogue (10 ns), dense then tail
        atomicAdd(&a.q->stats[9], __builtin_amdgcn_s_memtime() - qs_k0);  // workgroup lifetime
        atomicMax(&a.q->stats[11], qs_iters);                              // most iterations of one workgroup
        atomicMax(&a.q->stats[12], qs_last_work);                          // end of the last flow evaluation (100 MHz)
        atomicMax(&a.q->stats[13], __builtin_amdgcn_s_memrealtime());      // last exit
      }
#endif
      break;
    }
#ifdef SF_Q_STATS
    if (a.qtrace && threadIdx.x == 0 && qs_iters < (2048u * 256u) / gridDim.x) {
      uint32_t* tr = a.qtrace + ((size_t)blockIdx.x * ((2048u * 256u) / gridDim.x) + qs_iters) * 4;
      tr[0] = (uint32_t)__builtin_amdgcn_s_memrealtime(); tr[1] = ctrl[0]; tr[2] = ctrl[1] | (ctrl[9] << 8);
    }
    ++qs_iters;
    const unsigned long long qs_t_fetch = __builtin_amdgcn_s_memrealtime();
    const int qs_o = ctrl[9] ? 5 : 0;
    qs_ph[qs_o + 0] += qs_t_fetch - qs_t_top;
    unsigned long long qs_t_mark = qs_t_fetch;
#endif
    const int NT = m.nT16;
    const unsigned int n_items = ctrl[0] << ctrl[1];  // items of this iteration (entries x attempts per entry)
    // the wave's tiles: tile j covers items (j * 4 + wave) * 16 .. + 15.  Between transforms a tile is its u registers
    // and its galaxy; `cur` is the tile being worked on, `oth` the other one (TPW = 2), swapped after every tile.
    // (the tile being worked on is always entry 0: the entries rotate after every tile, TPW turns restore the order)
    f32x4 u_t[TPW];
    unsigned int g_t[TPW];
    f32x4& u_cur = u_t[0];
    unsigned int& gal_cur = g_t[0];
    if constexpr (PREC == 2 && TPW == 2) {
      // D <= 5: a draw is Philox blocks 0 and 1, so the wave's two tiles are ONE call -- lanes 0..31 (row groups 0, 1) draw blocks
      // 0, 1 of tile 0, lanes 32..63 those of tile 1, and v_permlane32_swap hands the upper half's to row groups 0, 1 (lane L and
      // lane L + 32 hold the same sample).  Row groups 2, 3 are padding.  Same counters (slot, attempt, block) per draw.
      static_assert(DD >= 3 && DD <= 5, "paired Philox call: a draw is blocks 0 and 1, row groups 2 and 3 hold no dimension");
      const int wi = ((g4 >> 1) * 4 + wave) * 16 + s;
      const unsigned int n_ent = ctrl[0];
      const int lgA = (int)ctrl[1];
      const unsigned int e = (unsigned)wi >> lgA;
      const unsigned int ee = e < n_ent ? e : 0u;
      const uint32_t slot = ctrl[SF_Q_HDR + ee];
      const uint32_t att = ctrl[SF_Q_HDR + IPW + ee] + ((unsigned)wi & ((1u << lgA) - 1u));
      float z4[4];
      sf_normal4(a.k0, a.k1, (uint64_t)slot + a.rng_slot_offset, att, (uint32_t)(g4 & 1), z4);
      // (an element of the swap's result goes through a scalar before the bit cast: cast in place, element 1 read element 0)
      const auto gsw = __builtin_amdgcn_permlane32_swap(slot / (uint32_t)a.S, slot / (uint32_t)a.S, false, false);
      const unsigned int gal0 = gsw[0], gal1 = gsw[1];
      g_t[0] = gal0;
      g_t[1] = gal1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned int zb = __builtin_bit_cast(unsigned int, z4[r]);
        const auto zsw = __builtin_amdgcn_permlane32_swap(zb, zb, false, false);
        const unsigned int z0 = zsw[0], z1 = zsw[1];   // every lane: the lower half's value | the upper half's
        const bool on = g4 < 2 && 4 * g4 + r < m.D;
        u_t[0][r] = on ? __builtin_bit_cast(float, z0) : 0.f;
        u_t[1][r] = on ? __builtin_bit_cast(float, z1) : 0.f;
      }
    } else {
#pragma unroll
    for (int j = TPW - 1; j >= 0; --j) {  // (j = 0 last: it is the first `cur`)
      const int wi = (j * 4 + wave) * 16 + s;
      const unsigned int n_ent = ctrl[0];
      const int lgA = (int)ctrl[1];
      const unsigned int e = (unsigned)wi >> lgA;
      const unsigned int ee = e < n_ent ? e : 0u;
      const uint32_t slot = ctrl[SF_Q_HDR + ee];
      const uint32_t att = ctrl[SF_Q_HDR + IPW + ee] + ((unsigned)wi & ((1u << lgA) - 1u));
      float z4[4];
      sf_normal4(a.k0, a.k1, (uint64_t)slot + a.rng_slot_offset, att, (uint32_t)g4, z4);  // Philox block g4 = dimensions 4*g4 .. 4*g4+3
#pragma unroll
      for (int r = 0; r < 4; ++r) u_t[j][r] = (4 * g4 + r < m.D) ? z4[r] : 0.f;
      g_t[j] = slot / (uint32_t)a.S;
    }
    }
    SfTiles16 tiles;
    if constexpr (DD == 0) tiles.pack(m);   // (the unrolled kernels know the tile of every pass: p - 2)
    typename HID::State S;
    S.tab = DD > 0 ? true : m.ctab != nullptr;  // (the unrolled kernels are only launched with the context table)
    for (int t = m.T - 1; t >= 0; --t) {
      // requested before the staging barriers so that their round trips overlap with the image copy: the degree ->
      // slot table of the transform and (table path) c0 of the first tile's first MFMA pass
      const int dsl = (int)m.cst[m.c_dslot + t * SF_DMAX + s];
      S.c0p = S.tab ? m.ctab + ((size_t)gal_cur * m.T + t) * m.ctab_R + (PREC == 2 ? m.nT16 * 16 : 0) : nullptr;
      if constexpr (PREC == 2) sf_pre16g_load<DD - 1>(S, g4);   // (fused: c0' of every tile, the pre-activations' start)
      else if (HM && S.tab) sf_c0_prefetch(S, tiles.tile(2), g4);
#ifdef SF_Q_STATS
      { const unsigned long long n = __builtin_amdgcn_s_memrealtime(); qs_ph[qs_o + (t == m.T - 1 ? 1 : 3)] += n - qs_t_mark; qs_t_mark = n; }
#endif
      __syncthreads();
      // PREC 2: the compact image; else part A of the fp32 image and the hidden blocks, one behind the other in LDS
      if constexpr (PREC == 2) sf_stage16c<FC::groups, FC::dead_lo, FC::dead_hi>(m.packed16c + (size_t)t * FC::total, wave);
      else sf_stage16<PREC, !SPAN>(m, t, S.tab ? m.t16_a_tab : m.t16_a, wave);
      __syncthreads();
#ifdef SF_Q_STATS
      { const unsigned long long n = __builtin_amdgcn_s_memrealtime(); qs_ph[qs_o + 2] += n - qs_t_mark; qs_t_mark = n; }
#endif
      const float* tp = sf_lds16;
      const void* tpB = sf_lds16 + (PREC == 2 ? FC::o_blk : (S.tab ? m.t16_a_tab : m.t16_a));   // the hidden blocks
#pragma unroll 1
      for (int j = 0; j < TPW; ++j) {
        // a wave whose tile holds no item (tail iterations with few entries) skips the flow: its issue slots go to the
        // other workgroups of the CU
        const bool tile_has_work = (unsigned)((j * 4 + wave) * 16) < n_items;
        if (tile_has_work) {
          if (j > 0) {  // (tile 0's requests went out before the staging barriers)
            S.c0p = S.tab ? m.ctab + ((size_t)gal_cur * m.T + t) * m.ctab_R + (PREC == 2 ? m.nT16 * 16 : 0) : nullptr;
            if constexpr (PREC == 2) sf_pre16g_load<DD - 1>(S, g4);
            else if (HM && S.tab) sf_c0_prefetch(S, tiles.tile(2), g4);
          }
          if constexpr (PREC != 2) { if (HM) S.hdone = sf_ld4(tp + m.o16_bh + g4 * 4); }
          if constexpr (PREC == 2) {
            float* scr = sf_lds16 + FC::total + wave * SF_G16_SCR + s * SF_G16_ROW;
            sf_transform16g<NB, DD, K3>(m, tp, static_cast<const float*>(tpB), tp + FC::o_hr, S, dsl, u_cur, scr, lane, g4);
          } else {
            S.xr = a.x + gal_cur * m.C;
            if constexpr (DD > 0) {
              sf_transform16s<HID, NB, DD>(m, tp, tpB, S, NT, dsl, u_cur, lane, g4);
            } else {
              HID::template clear<false, HM>(S);
#pragma unroll
              for (int r = 0; r < 4; ++r) S.ut[r] = 0.f;
              {
                const int sl = __builtin_amdgcn_readlane(dsl, 0);
                sf_pass16_deg1(m, tp, S.ut, sl, sf_slot16_own(u_cur, sl), g4);
              }
              for (int p = 2; p <= m.D; ++p) {
                const int sl = __builtin_amdgcn_readlane(dsl, p - 1);
                // (only the owning row group keeps what is computed from the slot's value)
                sf_pass16_tiles<HID, NB, SPAN, HM>(m, tp, tpB, S, NT, tiles, p, m.D, sl, sf_slot16_own(u_cur, sl), lane, g4);
              }
              u_cur = S.ut;
            }
          }
        }
        if (TPW > 1) {  // the next tile's turn (after TPW turns every tile is entry 0 under its own index again)
          const f32x4 tu = u_t[0];
          const unsigned int tg = g_t[0];
#pragma unroll
          for (int q = 0; q + 1 < TPW; ++q) { u_t[q] = u_t[q + 1]; g_t[q] = g_t[q + 1]; }
          u_t[TPW - 1] = tu;
          g_t[TPW - 1] = tg;
        }
      }
    }
#ifdef SF_Q_STATS
    { const unsigned long long n = __builtin_amdgcn_s_memrealtime(); qs_ph[qs_o + 3] += n - qs_t_mark; qs_t_mark = n; }
#endif
    // ---------------------------------------------------------------- un-standardise, box test, outputs (per tile)
#pragma unroll 1
    for (int j = 0; j < TPW; ++j) {
      const int wi = (j * 4 + wave) * 16 + s;
      // the work words are still in LDS: nothing about the item had to stay in registers through the flow
      const unsigned int n_ent = ctrl[0];
      const int lgA = (int)ctrl[1];
      const unsigned int e = (unsigned)wi >> lgA;
      const bool entry_ok = e < n_ent;
      const unsigned int ee = entry_ok ? e : 0u;
      const uint32_t slot = ctrl[SF_Q_HDR + ee];
      const uint32_t att_base = ctrl[SF_Q_HDR + IPW + ee];
      const uint32_t att = att_base + ((unsigned)wi & ((1u << lgA) - 1u));
      const bool valid = entry_ok && att < a.attempt_limit;
      float th[4];
      int tdc[4];
      const uint32_t acc16 = sf_accept16(sf_theta_box16(ecb, u_cur, g4, th, tdc), valid);
      // A consecutive items hold attempts att_base .. att_base+A-1 of one slot: the lowest accepted one wins.
      // A <= 16: the group sits inside this wave's tile.  A = 32 / 64 (the last few slots of a catalogue, each tried by
      // half of / the whole workgroup at once): the group is tiles j*4 + gw0 .. of the SAME j, one per wave; the waves
      // combine through four LDS words.
      const int A = 1 << lgA;
      int first, me;
      if (lgA <= 4) {
        const int grp0 = (s / A) * A;
        const uint32_t gmask = (acc16 >> grp0) & ((1u << A) - 1u);
        first = gmask ? (int)__builtin_ctz(gmask) : -1;
        me = s - grp0;
      } else {
        if ((threadIdx.x & 63) == 0) ctrl[20 + wave] = acc16 ? (unsigned)__builtin_ctz(acc16) : 16u;
        __syncthreads();  // (lgA is the same for the whole workgroup)
        const int gw0 = (int)(((e << lgA) >> 4) & 3u), gwn = A >> 4;  // first wave of the group, waves per group
        first = -1;
#pragma unroll
        for (int w = 3; w >= 0; --w) {
          const unsigned int cw = ctrl[20 + w];
          if (w >= gw0 && w < gw0 + gwn && cw < 16u) first = (w - gw0) * 16 + (int)cw;
        }
        me = wi - (int)(e << lgA);
        if (TPW > 1) __syncthreads();  // the four words are rewritten for the next tile
      }
      // One attempt per entry (every dense iteration): the tile's 16 x D block of draws is handed to the lanes LINEARLY -- lane L
      // stores element L, L + 64, ... = (draw se = e / D, column c = e % D) at out[slot(se) D + c] -- so that a wave-instruction
      // covers the rows of consecutive draws side by side (the dense order deals RUNS of consecutive draws of a galaxy:
      // dense_run) instead of five 4-byte pieces per draw from two row groups: whole 64-byte segments in HBM, and fewer PCIe
      // packets when `out` is the host's float64 array.  The value sits in lane se + 16 (p >> 2), register p & 3, p = the
      // column's physical slot; the slot id in lane se.
      if (lgA == 0) {
        const int Dn = DD > 0 ? DD : m.D;
        const int* c2s = reinterpret_cast<const int*>(ecb) + 80;
        for (int e0 = 0; e0 < 16 * Dn; e0 += 64) {
          const int e = e0 + (lane & 63);
          const int se = (e / Dn) & 15, c = e - (e / Dn) * Dn;
          const int p = c2s[c];
          const int src = se + 16 * (p >> 2), rr = p & 3;
          const float v0 = __shfl(th[0], src, 64), v1 = __shfl(th[1], src, 64), v2 = __shfl(th[2], src, 64), v3 = __shfl(th[3], src, 64);
          const float v = rr == 0 ? v0 : (rr == 1 ? v1 : (rr == 2 ? v2 : v3));
          const uint32_t sl_e = (uint32_t)__shfl((int)slot, se, 64);
          if (e < 16 * Dn && ((acc16 >> se) & 1u)) sf_out_store(a, (size_t)sl_e * Dn + c, v);
        }
      } else if (valid && me == first) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * g4 + r < m.D) sf_out_store(a, (size_t)slot * m.D + tdc[r], th[r]);
      }
      // accepted -> resolved; rejected -> staged for the retry ring, or for the survivor list once the launch's attempt
      // limit is reached; wave 0 publishes everything the workgroup staged at the top of the next sf_q_fetch
      const bool leader = entry_ok && g4 == 0 && me == 0;
      const uint32_t room = a.attempt_limit > att_base ? a.attempt_limit - att_base : 0u;
      const uint32_t tried = room < (uint32_t)A ? room : (uint32_t)A;  // attempts of this entry evaluated here
      const bool hit = leader && first >= 0;
      const bool retry = leader && first < 0 && att_base + (uint32_t)A < a.attempt_limit;
      const bool surv = leader && first < 0 && !retry;
      if (leader && (a.n_drawn || a.gal_acc)) {
        const long gal = (long)(slot / (uint32_t)a.S);
        // (the caller pre-counts ONE attempt per slot; a first attempt that ran with speculation may have used more)
        const int used = (first >= 0 ? first + 1 : (int)tried) - (att_base == 0u ? 1 : 0);
        if (a.n_drawn && used > 0) sf_sat_add(&a.n_drawn[gal], used);
        if (hit && a.gal_acc && att_base >= 64u) atomicAdd(&a.gal_acc[gal], 1);  // progress past the 64th attempt
      }
      if (retry) {
        const unsigned int pos = atomicAdd(&ctrl[2], 1u);
        ctrl[SF_Q_HDR + 2 * IPW + pos] = slot;
        ctrl[SF_Q_HDR + 3 * IPW + pos] = att_base + (uint32_t)A;
      }
      if (surv) {
        const unsigned int pos = atomicAdd(&ctrl[3], 1u);
        ctrl[SF_Q_HDR + 4 * IPW + pos] = slot;
      }
      const unsigned int n_res = (unsigned)__popcll(__ballot(hit || surv));
      const unsigned int n_ev = (unsigned)__popcll(__ballot(valid && g4 == 0));
      const unsigned int n_r0 = (unsigned)__popcll(__ballot(leader && first < 0 && att_base == 0u));
      if ((threadIdx.x & 63) == 0) {
        if (n_res) atomicAdd(&ctrl[4], n_res);
        if (n_ev) atomicAdd(&ctrl[5], n_ev);
        if (n_r0) atomicAdd(&ctrl[6], n_r0);
      }
      if (TPW > 1) {
        const f32x4 tu = u_t[0];
#pragma unroll
        for (int q = 0; q + 1 < TPW; ++q) u_t[q] = u_t[q + 1];
        u_t[TPW - 1] = tu;
      }
    }
#ifdef SF_Q_STATS
    qs_last_work = __builtin_amdgcn_s_memrealtime();
    qs_ph[qs_o + 4] += qs_last_work - qs_t_mark;
    if (a.qtrace && threadIdx.x == 0 && qs_iters <= (2048u * 256u) / gridDim.x)
      a.qtrace[((size_t)blockIdx.x * ((2048u * 256u) / gridDim.x) + qs_iters - 1) * 4 + 3] = (uint32_t)qs_last_work;
#endif
  }
}

// Find / resolve launches of the deep tail (sf_api.hip: the slots that used up the persistent windows) on the sampler's OWN
// arithmetic and cost per evaluation: the unrolled split-bf16 pass sequence of k_maf_samp16<.., DD> without the queue.
//   find    (a.best):     item i = attempt a.attempt + (i & (A - 1)) of listed slot i >> log2 A; an accepted attempt only lowers
//                         best[slot index] (atomic min)
//   resolve (a.att_list): item i = attempt att_list[i] of listed slot i (0xffffffff: none): writes the draw, or lists the slot
//                         as still open
//   count   (a.count):    item i = first attempt of slot i: += 1 per accepted draw of its galaxy (sf_flow_acceptance)
// A catalogue of 1e5 galaxies spends two thirds of its evaluations here (a few galaxies of acceptance ~1e-4 x 1 000 slots x
// ~1e4 attempts); on the fp32 kernel k_maf_inv16 those ran at 0.6 of the sampler's rate.  Table path, aligned placement with
// one degree group per tile (the shapes of the unrolled sampler); two tiles of 16 items per wave and staged transform.
template <int NB, int DD, int PREC = 0, int K3 = 0>
__global__ __launch_bounds__(256, 4) void k_maf_find16s(SfDev m, SfSampleArgsHost a) {
  static_assert(K3 == 0 || (PREC == 2 && K3 <= DD - 1), "skipped k-steps: the fused passes only");
  using HID = SfHid16<PREC>;
  using FC = SfFixC16<NB, DD>;   // (PREC 2 only: the compact image)
  SfFix16<NB, DD>::apply(m);  // (the launcher only picks this kernel when the packer's offsets are these)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = lane & 15, g4 = lane >> 4;
  float* ecb = sf_lds16 + (PREC == 2 ? FC::lds : sf_lds_floats16<PREC>(m, true));
  sf_ecb16_build<false>(ecb, m, a);  // (80 words: the launcher adds no room for the column -> slot table)
  if constexpr (PREC == 2) FC::apply(m);   // (the fused passes read the compact image)
  const int NT = m.nT16;
  f32x4 u_cur, u_oth;
  long gal_cur = 0, gal_oth = 0;
#pragma unroll
  for (int j = 1; j >= 0; --j) {
    const long item = ((long)blockIdx.x * 8 + j * 4 + wave) * 16 + s;
    const long it = item < a.n_items ? item : a.n_items - 1;
    // (given noise -- the parity hook -- item = row of z / x: the context table was built for those rows)
    const SfItem16 I = sf_item16(m, a, it, g4);
    if (j == 1) { u_oth = I.u; gal_oth = I.gal; }
    else { u_cur = I.u; gal_cur = I.gal; }
  }
  typename HID::State S;
  S.tab = true;
  if constexpr (PREC != 2) S.xr = nullptr;
  for (int t = m.T - 1; t >= 0; --t) {
    const int dsl = (int)m.cst[m.c_dslot + t * SF_DMAX + s];
    S.c0p = m.ctab + ((size_t)gal_cur * m.T + t) * m.ctab_R + (PREC == 2 ? m.nT16 * 16 : 0);
    if constexpr (PREC == 2) sf_pre16g_load<DD - 1>(S, g4);
    else sf_c0_prefetch(S, 0, g4);
    __syncthreads();
    if constexpr (PREC == 2) sf_stage16c<FC::groups, FC::dead_lo, FC::dead_hi>(m.packed16c + (size_t)t * FC::total, wave);
    else sf_stage16<PREC, true>(m, t, m.t16_a_tab, wave);
    __syncthreads();
    const float* tp = sf_lds16;
    const void* tpB = sf_lds16 + (PREC == 2 ? FC::o_blk : m.t16_a_tab);
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
      if (((long)blockIdx.x * 8 + j * 4 + wave) * 16 < a.n_items) {  // (wave-uniform: the tile holds an item)
        if (j > 0) {
          S.c0p = m.ctab + ((size_t)gal_cur * m.T + t) * m.ctab_R + (PREC == 2 ? m.nT16 * 16 : 0);
          if constexpr (PREC == 2) sf_pre16g_load<DD - 1>(S, g4);
          else sf_c0_prefetch(S, 0, g4);
        }
        if constexpr (PREC != 2) S.hdone = sf_ld4(tp + m.o16_bh + g4 * 4);
        if constexpr (PREC == 2) {
          float* scr = sf_lds16 + FC::total + wave * SF_G16_SCR + s * SF_G16_ROW;
          sf_transform16g<NB, DD, K3>(m, tp, static_cast<const float*>(tpB), tp + FC::o_hr, S, dsl, u_cur, scr, lane, g4);
        } else {
          sf_transform16s<HID, NB, DD>(m, tp, tpB, S, NT, dsl, u_cur, lane, g4);
        }
      }
      { const f32x4 tu = u_cur; u_cur = u_oth; u_oth = tu; }
      { const long tg = gal_cur; gal_cur = gal_oth; gal_oth = tg; }
    }
  }
#pragma unroll 1
  for (int j = 0; j < 2; ++j) {
    const long item = ((long)blockIdx.x * 8 + j * 4 + wave) * 16 + s;
    const bool valid = item < a.n_items;
    const long it = valid ? item : a.n_items - 1;
    const long ps = it >> a.log2_attempts;
    const uint32_t att = a.att_list ? a.att_list[ps] : a.attempt + (uint32_t)(it & ((1L << a.log2_attempts) - 1));
    float th[4];
    int tdc[4];
    bool ok = sf_theta_box16(ecb, u_cur, g4, th, tdc);
    if (a.att_list && att == 0xffffffffu) ok = false;  // no attempt to resolve: straight to the open list
    const uint32_t acc16 = sf_accept16(ok, valid);
    const bool accepted = (acc16 >> s) & 1u;
    if (a.z_in) {   // every row is written (no box: lo / hi are null)
      if (valid) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * g4 + r < m.D) a.out[item * m.D + tdc[r]] = th[r];
      }
    } else if (a.best) {
      if (accepted && g4 == 0) atomicMin(&a.best[ps], att);
    } else if (a.count) {  // acceptance counts (leakage correction): item = draw item % S of galaxy item / S
      const long gal = (long)((uint32_t)(a.slots ? a.slots[ps] : (uint32_t)(a.slot_base + ps)) / (uint32_t)a.S);
      const long g_first = __shfl(gal, 0, 64), g_last = __shfl(gal, 15, 64);
      if (g_first == g_last) {
        if (lane == 0 && acc16) atomicAdd(&a.count[g_first], (int)__popc(acc16));
      } else if (accepted && g4 == 0) {
        atomicAdd(&a.count[gal], 1);
      }
    } else if (valid) {  // resolve: one item per listed slot
      const uint32_t slot = a.slots ? a.slots[ps] : (uint32_t)(a.slot_base + ps);
      if (accepted) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * g4 + r < m.D) sf_out_store(a, (size_t)slot * m.D + tdc[r], th[r]);
      } else if (g4 == 0) {
        const uint32_t pos = atomicAdd(a.n_rejected, 1u);
        a.rejected[pos] = slot;
      }
    }
    { const f32x4 tu = u_cur; u_cur = u_oth; u_oth = tu; }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// opt a kernel in to 160 KiB of dynamic LDS, once per device (`attr`: the launcher's static cache for that kernel)
template <typename K>
static hipError_t sf_lds_optin16(K kernel, SfAttrCache& attr) {
  int dev;
  if (!attr.need(dev)) return hipSuccess;
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e == hipSuccess) attr.set(dev);
  return e;
}
// The run-time shape as template arguments: f(NB, SPAN, HM) as integral constants for NB in {1, 2} (anything else takes the
// NB = 2 kernels, as m16_ok never lets it happen) and the placement: contiguous (span code, head rows as dot products), aligned
// with the head rows on the matrix pipe, aligned without.
template <typename F>
static hipError_t sf_visit_shape16(int NB, bool span, bool hm, F&& f) {
  auto nb = [&](auto sp, auto h) {
    return NB == 1 ? f(std::integral_constant<int, 1>{}, sp, h) : f(std::integral_constant<int, 2>{}, sp, h);
  };
  if (span) return nb(std::true_type{}, std::false_type{});
  if (hm) return nb(std::false_type{}, std::true_type{});
  return nb(std::false_type{}, std::false_type{});
}
// The same for the unrolled kernels: f(NB, DD), NB in {1, 2}, DD in 3..5; any other pair is an error
template <typename F>
static hipError_t sf_visit_unrolled16(int NB, int dd, F&& f) {
  auto d = [&](auto nb) {
    switch (dd) {
      case 3: return f(nb, std::integral_constant<int, 3>{});
      case 4: return f(nb, std::integral_constant<int, 4>{});
      case 5: return f(nb, std::integral_constant<int, 5>{});
      default: return (hipError_t)hipErrorInvalidValue;
    }
  };
  if (NB == 1) return d(std::integral_constant<int, 1>{});
  if (NB == 2) return d(std::integral_constant<int, 2>{});
  return hipErrorInvalidValue;
}

// the compact image's offsets against the compile-time ones of the fused kernels: 1 equal, 0 not, -1 no such kernel for the shape
int sf_maf16_compact_fix(const SfDev& m) {
  if (m.t16c_stride <= 0 || m.D < 3 || m.D > 5 || m.nT16 != m.D - 1 || m.NB < 1 || m.NB > 2) return -1;
  if (m.NB == 1) return m.D == 3 ? SfFixC16<1, 3>::matches(m) : (m.D == 4 ? SfFixC16<1, 4>::matches(m) : SfFixC16<1, 5>::matches(m));
  return m.D == 3 ? SfFixC16<2, 3>::matches(m) : (m.D == 4 ? SfFixC16<2, 4>::matches(m) : SfFixC16<2, 5>::matches(m));
}
// the unrolled-pass kernels apply when degree p - 1 sits alone in tile p - 2 (otherwise: the dispatching kernel)
static int sf_maf16_seq_d(const SfDev& m) {
  if (!m.ctab || m.m16_span || m.D < 3 || m.D > 5 || m.nT16 != m.D - 1) return 0;
  for (int p = 2; p <= m.D; ++p)
    if (m.g16_tile[p - 1] != p - 2) return 0;
  bool fits = false;  // the image offsets the unrolled kernels hard-wire
  if (m.NB == 1) fits = m.D == 3 ? SfFix16<1, 3>::matches(m) : (m.D == 4 ? SfFix16<1, 4>::matches(m) : SfFix16<1, 5>::matches(m));
  else if (m.NB == 2) fits = m.D == 3 ? SfFix16<2, 3>::matches(m) : (m.D == 4 ? SfFix16<2, 4>::matches(m) : SfFix16<2, 5>::matches(m));
  return fits ? m.D : 0;
}
// Which kernels of this file a view of a flow runs on, in the process's sampler arithmetic (SfMaf16Plan, sf_internal.h): every
// launcher and the API read the decisions here.
SfMaf16Plan sf_maf16_plan(const SfDev& m) {
  SfMaf16Plan pl;
  pl.fp32 = sf_sampler_fp32_for(SF_MAF) != 0;
  pl.ok16 = m.kind == SF_MAF && m.m16_ok && !m.hidden_bf16 && m.packed16 != nullptr;
  pl.sampler16 = pl.ok16 && (m.packed16B != nullptr || pl.fp32);
  pl.span = m.m16_span != 0;
  pl.head_mfma = !m.m16_span && m.o16_wh >= 0;
  pl.dd = pl.head_mfma ? sf_maf16_seq_d(m) : 0;
  pl.fused = pl.dd > 0 && pl.fp32 && m.o16_wp >= 0 && m.ctab_R == 2 * m.nT16 * 16 && m.packed16c != nullptr && sf_maf16_compact_fix(m) == 1;
  return pl;
}

// The fused kernels' skipped k-steps as a template argument: f(K3) for K3 = m16_k3 in 0 .. DD - 1 (the packer's count of trailing
// hidden tiles with empty rows 3, 7, 11, 15); anything else is an error -- a kernel that skipped a row that holds a unit would be wrong
template <int DD, typename F>
static hipError_t sf_visit_k3(int k3, F&& f) {
  switch (k3) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: if constexpr (DD >= 4) return f(std::integral_constant<int, 3>{}); else return hipErrorInvalidValue;
    case 4: if constexpr (DD >= 5) return f(std::integral_constant<int, 4>{}); else return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}

template <int NB, int DD, int PREC, int K3 = 0>
static hipError_t sf_launch_find16s(const SfDev& m, const SfSampleArgsHost& a, hipStream_t st) {
  static SfAttrCache attr;
  const size_t sh = (size_t)sf_lds_floats16<PREC>(m, true) * sizeof(float) + 80 * sizeof(float);
  if (hipError_t e = sf_lds_optin16(k_maf_find16s<NB, DD, PREC, K3>, attr); e != hipSuccess) return e;
  hipLaunchKernelGGL((k_maf_find16s<NB, DD, PREC, K3>), dim3((unsigned)((a.n_items + 127) / 128)), dim3(256), sh, st, m, a);
  return hipGetLastError();
}

// Parity hook of the persistent sampler's ARITHMETIC: theta = inverse(z | x) from GIVEN noise through exactly the pass
// functions k_maf_samp16 runs (sf_pass16b / sf_pass16b_span: hidden H x H blocks as split-bf16 x3, everything else
// fp32), so that the sampler's precision can be asserted against the fp64 oracle draw for draw, with no Philox and no
// rejection in between (sf_flow_inverse_from_noise_sampler; tests/test_gpu_parity.py).  One wave = 16 rows of z.
template <int NB, bool SPAN, bool HM, int PREC = 0>
__global__ __launch_bounds__(256, 3) void k_maf_inv16b(SfDev m, const float* __restrict__ z, const float* __restrict__ x,
                                                       long n, float* __restrict__ out) {
  using HID = SfHid16<PREC>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = lane & 15, g4 = lane >> 4;
  const long item = ((long)blockIdx.x * 4 + wave) * 16 + s;
  const bool valid = item < n;
  const long it = valid ? item : n - 1;
  f32x4 u;
#pragma unroll
  for (int r = 0; r < 4; ++r) u[r] = (4 * g4 + r < m.D) ? z[it * m.D + 4 * g4 + r] : 0.f;
  const int NT = m.nT16;
  SfTiles16 tiles;
  tiles.pack(m);
  typename HID::State S;
  HID::template clear<false, false>(S);
  for (int t = m.T - 1; t >= 0; --t) {
    __syncthreads();
    sf_stage16<PREC, !SPAN>(m, t, m.t16_a, wave);
    __syncthreads();
    const float* tp = sf_lds16;
    const void* tpB = sf_lds16 + m.t16_a;
    S.c0p = nullptr;
    S.tab = false;
    S.xr = x + it * m.C;
    if (HM) S.hdone = sf_ld4(tp + m.o16_bh + g4 * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) S.ut[r] = 0.f;
    const int dsl = (int)m.cst[m.c_dslot + t * SF_DMAX + s];
    {
      const int sl = __builtin_amdgcn_readlane(dsl, 0);
      sf_pass16_deg1(m, tp, S.ut, sl, sf_slot16(u, sl, lane), g4);
    }
    for (int p = 2; p <= m.D; ++p) {
      const int sl = __builtin_amdgcn_readlane(dsl, p - 1);
      sf_pass16_tiles<HID, NB, SPAN, HM>(m, tp, tpB, S, NT, tiles, p, m.D, sl, sf_slot16(u, sl, lane), lane, g4);
    }
    u = S.ut;
  }
  if (valid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = 4 * g4 + r;
      if (p < m.D) out[item * m.D + (int)m.cst[m.c_tdim + p]] = sf_div(u[r] - m.cst[m.c_pshift + p], m.cst[m.c_pscale + p]);
    }
  }
}

template <int NB, bool SPAN, bool HM, int PREC>
static hipError_t sf_launch16b_hook_p(const SfDev& m, const float* z, const float* x, long n, float* out, hipStream_t st) {
  static SfAttrCache attr;
  const size_t sh = ((size_t)m.t16_a + (size_t)SfHid16<PREC>::lds_floats(m, !SPAN)) * sizeof(float);
  if (hipError_t e = sf_lds_optin16(k_maf_inv16b<NB, SPAN, HM, PREC>, attr); e != hipSuccess) return e;
  hipLaunchKernelGGL((k_maf_inv16b<NB, SPAN, HM, PREC>), dim3((unsigned)((n + 63) / 64)), dim3(256), sh, st, m, z, x, n, out);
  return hipGetLastError();
}
hipError_t sf_launch_maf_inv16b_hook(const SfDev& m, const float* z, const float* x, long n, float* out, hipStream_t st) {
  const SfMaf16Plan pl = sf_maf16_plan(m);
  return sf_visit_shape16(m.NB, pl.span, pl.head_mfma, [&](auto nb, auto sp, auto hm) {
    return pl.fp32 ? sf_launch16b_hook_p<nb(), sp(), hm(), 1>(m, z, x, n, out, st)
                   : sf_launch16b_hook_p<nb(), sp(), hm(), 0>(m, z, x, n, out, st);
  });
}

// Per-galaxy context table of the 16-row path: tab[gal][t][row] = b0 + bc + Wc e(x_gal), rows in tile order.
// One wave = 16 galaxies of ONE transform (blockIdx.y): the T transforms of a galaxy are independent chains of a few MFMAs, and
// the kernel runs in front of every sampling call -- side by side they take one chain's latency instead of T.  Same MFMA
// sequence per (galaxy, transform) as the in-kernel evaluation, so the sampler's draws do not change.
__global__ __launch_bounds__(256) void k_maf_ctab16(SfDev m, const float* __restrict__ x, long M, float* __restrict__ tab) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = lane & 15, g4 = lane >> 4;
  const long gal = ((long)blockIdx.x * 4 + wave) * 16 + s;
  if (((long)blockIdx.x * 4 + wave) * 16 >= M) return;
  const bool valid = gal < M;
  const float* xr = x + (valid ? gal : M - 1) * m.C;
  const int NT = m.nT16;
  {
    const int t = blockIdx.y;
    const float* tp = m.packed16 + (size_t)t * m.t16_stride;
    f32x4 c0[4];
#pragma unroll
    for (int ot = 0; ot < 4; ++ot)
      if (ot < NT) c0[ot] = sf_ld4(tp + m.o16_b0 + (ot * 4 + g4) * 4);
    for (int ic = 0; ic < m.nC16; ++ic) {
      const f32x4 ct = sf_ctx_tile16(m, xr, ic, g4);
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
        if (ot < NT) c0[ot] = sf_mma16(sf_w16(tp + m.o16_wc, m.nC16, ot, ic, lane), ct, c0[ot]);
    }
    if (valid) {
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
        if (ot < NT)
          *reinterpret_cast<f32x4*>(tab + ((size_t)gal * m.T + t) * m.ctab_R + ot * 16 + 4 * g4) = c0[ot];
    }
    if (m.o16_wp >= 0) {   // fused first layer (sf_pass16g): c0' = b1 + (W1 o M) c0, behind c0 in the row
      f32x4 c1[4];
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
        if (ot < NT) {
          c1[ot] = sf_ld4(tp + m.o16_bk[0] + (ot * 4 + g4) * 4);
#pragma unroll
          for (int it = 0; it < 4; ++it)
            if (it < NT) c1[ot] = sf_mma16(sf_w16(tp + m.o16_wk[0], NT, ot, it, lane), c0[it], c1[ot]);
        }
      if (valid) {
#pragma unroll
        for (int ot = 0; ot < 4; ++ot)
          if (ot < NT)
            *reinterpret_cast<f32x4*>(tab + ((size_t)gal * m.T + t) * m.ctab_R + NT * 16 + ot * 16 + 4 * g4) = c1[ot];
      }
    }
  }
}
// W' = (W1 o M)(W0 o M0) of every transform, from the packed fp32 image into its o16_wp block (fp64 sums, one rounding), as the
// fused kernels' rank-1 updates read it (sf_pass16g): for input degree k = 1 .. min(NT, D - 1) and hidden tile ot = k - 1 .. NT - 1,
// entry sf_wp16_entry(NT, k, ot) = 16 floats, float4 g4 = W'[ot*16 + 4 g4 + r][slot of degree k], r = 0..3.  The other columns of
// a tile are structural zeros (a unit of degree d sees u_1 .. u_d).  Masked weights are structural zeros of the image, and the
// packed first block carries the tanh pre-scale (SF_PACK_TANH_SCALE): W' and c0' inherit both.
__global__ __launch_bounds__(256) void k_maf_fuse16(SfDev m) {
  const int t = blockIdx.x;
  const int NT = m.nT16;
  const int KN = NT < m.D - 1 ? NT : m.D - 1;   // (the dimension of degree D feeds nothing)
  const int n_ent = KN * NT - KN * (KN - 1) / 2;
  float* tp = const_cast<float*>(m.packed16) + (size_t)t * m.t16_stride;
  for (int i = threadIdx.x; i < n_ent * 16; i += blockDim.x) {
    const int e = i >> 4, g4 = (i >> 2) & 3, r = i & 3;
    int k = 1;
    while (k < KN && e >= sf_wp16_entry(NT, k + 1, k)) ++k;
    const int ot = k - 1 + (e - sf_wp16_entry(NT, k, k - 1));
    const int row = 4 * g4 + r;
    const int col = (int)m.cst[m.c_dslot + t * SF_DMAX + k - 1];
    double acc = 0.0;
    for (int it = 0; it < NT; ++it)
      for (int kk = 0; kk < 16; ++kk) {
        const float wk = tp[m.o16_wk[0] + ((ot * NT + it) * 64 + row + 16 * (kk >> 2)) * 4 + (kk & 3)];   // W1[ot*16 + row][it*16 + kk]
        const float w0 = tp[m.o16_w0 + (it * 64 + kk + 16 * (col >> 2)) * 4 + (col & 3)];                // W0[it*16 + kk][col]
        acc += (double)wk * (double)w0;
      }
    tp[m.o16_wp + e * 16 + g4 * 4 + r] = (float)acc;
  }
}
hipError_t sf_launch_maf_fuse16(const SfDev& m, hipStream_t st) {
  hipLaunchKernelGGL(k_maf_fuse16, dim3((unsigned)m.T), dim3(256), 0, st, m);
  return hipGetLastError();
}
// The compact fused image (sf_layout.h, packed16c) of every transform and the head rows behind it from the 16-row image, by the
// packer's tables: runs behind k_maf_fuse16 on the same stream, so W' is in it.  tab: [T][t16c_stride + t16h_stride] -- the head
// rows of a degree come from the slot that holds it in THAT transform, so every transform has its own table.
__global__ __launch_bounds__(256) void k_maf_compact16(SfDev m, const int32_t* __restrict__ tab, float* __restrict__ out) {
  const int n = m.t16c_stride + m.t16h_stride;
  const float* tp = m.packed16 + (size_t)blockIdx.x * m.t16_stride;
  const int32_t* tt = tab + (size_t)blockIdx.x * n;
  float* op = out + (size_t)blockIdx.x * n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int s = tt[i];
    op[i] = s >= 0 ? tp[s] : 0.f;
  }
}
hipError_t sf_launch_maf_compact16(const SfDev& m, const int32_t* tab, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_maf_compact16, dim3((unsigned)m.T), dim3(256), 0, st, m, tab, out);
  return hipGetLastError();
}
hipError_t sf_launch_maf_ctab16(const SfDev& m, const float* x, long M, float* tab, hipStream_t st) {
  hipLaunchKernelGGL(k_maf_ctab16, dim3((unsigned)((M + 63) / 64), (unsigned)m.T), dim3(256), 0, st, m, x, M, tab);
  return hipGetLastError();
}

// A = 32 retry rounds stay on the 32-row kernel.
bool sf_maf16_enabled(const SfDev& m, const SfSampleArgsHost& a) {
  return sf_maf16_plan(m).ok16 && (a.attempts_per_slot <= 16 || a.best != nullptr);  // (find mode has no in-tile attempt groups)
}

// workgroups that fit the chip at once (persistent launches): `cap` per CU by registers and LDS (4 with the compact
// image of the aligned placement at 128 VGPRs, 3 for the contiguous one)
static int sf_resident_blocks16(const void* fn, size_t sh, int cap) {
  int dev = 0, cus = 256, per = cap;
  if (hipGetDevice(&dev) == hipSuccess) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) cus = pr.multiProcessorCount;
  }
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 256, sh) == hipSuccess && occ > 0) per = occ < cap ? occ : cap;
  return cus * per;
}

// persistent sampler: no more workgroups than the chip holds (more would only queue behind the spinning ones)
template <int NB, bool SPAN, bool HM, int DD, int PREC, int K3 = 0>
static hipError_t sf_launch16q_p(const SfDev& m, const SfSampleArgsHost& a, hipStream_t st) {
  static SfAttrCache attr;
  static SfResidentCache rcache;
  const size_t sh = (size_t)sf_lds_floats16<PREC>(m, !SPAN) * sizeof(float) + (SF_Q_WORDS(64 * SF_SAMP16_TPW) + 96) * sizeof(unsigned int);
  if (sh > 160 * 1024) return hipErrorInvalidValue;
  if (hipError_t e = sf_lds_optin16(k_maf_samp16<NB, SPAN, HM, DD, PREC, K3>, attr); e != hipSuccess) return e;
  int resident = 0, cur_dev = 0;
  (void)hipGetDevice(&cur_dev);
  if (!rcache.get(cur_dev, sh, resident)) {
    resident = sf_resident_blocks16((const void*)k_maf_samp16<NB, SPAN, HM, DD, PREC, K3>, sh, SPAN ? 3 : (PREC == 2 ? SF_SAMP16_WG_FUSED : 4));
    rcache.put(cur_dev, sh, resident);
  }
  long grid = (a.n_items + 64 * SF_SAMP16_TPW - 1) / (64 * SF_SAMP16_TPW);
  if (grid > resident) grid = resident;
  SfSamp16Args args;
  args.m = m;
  args.a = a;
  hipLaunchKernelGGL((k_maf_samp16<NB, SPAN, HM, DD, PREC, K3>), dim3((unsigned)grid), dim3(256), sh, st, args);
  return hipGetLastError();
}
// ... in the plan's arithmetic: the fused first layer (unrolled kernels only), fp32, or split bf16 where the flow has that image
// (round 5, fp32 kernels: FOUR tiles per wave and staged transform -- fetch, staging and prologue once per 256 draws -- measured
//  2.74 ms per catalogue against 2.62 with two: the coarser iterations cost the tail more than the dense phase saves)
template <int NB, bool SPAN, bool HM, int DD>
static hipError_t sf_launch16q(const SfDev& m, const SfSampleArgsHost& a, const SfMaf16Plan& pl, hipStream_t st) {
  if constexpr (DD > 0) {
    if (pl.fused) return sf_visit_k3<DD>(m.m16_k3, [&](auto k3) { return sf_launch16q_p<NB, SPAN, HM, DD, 2, k3()>(m, a, st); });
  }
  if (pl.fp32) return sf_launch16q_p<NB, SPAN, HM, DD, 1>(m, a, st);
  if (!m.packed16B) return hipErrorInvalidValue;
  return sf_launch16q_p<NB, SPAN, HM, DD, 0>(m, a, st);
}
template <int NB, bool SPAN>
static hipError_t sf_launch16(const SfDev& m, const SfSampleArgsHost& a, hipStream_t st) {
  static SfAttrCache attr;
  const size_t sh = (size_t)m.t16_stride * sizeof(float);
  if (hipError_t e = sf_lds_optin16(k_maf_inv16<NB, SPAN>, attr); e != hipSuccess) return e;
  const long per_block = 4L * 16;
  hipLaunchKernelGGL((k_maf_inv16<NB, SPAN>), dim3((unsigned)((a.n_items + per_block - 1) / per_block)), dim3(256), sh, st, m, a);
  return hipGetLastError();
}
// find / resolve / count launches and the given-noise hook on the unrolled kernels' pass functions, in the plan's arithmetic
static hipError_t sf_launch_find16(const SfDev& m, const SfSampleArgsHost& a, const SfMaf16Plan& pl, hipStream_t st) {
  return sf_visit_unrolled16(m.NB, pl.dd, [&](auto nb, auto dd) {
    constexpr int NB_ = decltype(nb)::value, DD_ = decltype(dd)::value;
    if (pl.fused) return sf_visit_k3<DD_>(m.m16_k3, [&](auto k3) { return sf_launch_find16s<NB_, DD_, 2, k3()>(m, a, st); });
    return (pl.fp32 ? sf_launch_find16s<nb(), dd(), 1>(m, a, st) : sf_launch_find16s<nb(), dd(), 0>(m, a, st));
  });
}
// parity hook of the fused pass functions: theta = inverse(z | x) through k_maf_find16s<.., PREC = 2> in its given-noise mode (the
// context table must have been built for the rows of x: item i reads table row i)
hipError_t sf_launch_maf_find16_zin(const SfDev& m, const SfSampleArgsHost& a, hipStream_t st) {
  const SfMaf16Plan pl = sf_maf16_plan(m);
  return pl.fused ? sf_launch_find16(m, a, pl, st) : hipErrorInvalidValue;
}
hipError_t sf_launch_maf_inv16(const SfDev& m, const SfSampleArgsHost& a, hipStream_t st) {
  const SfMaf16Plan pl = sf_maf16_plan(m);
  if (a.q) {
    if (pl.dd > 0)
      return sf_visit_unrolled16(m.NB, pl.dd, [&](auto nb, auto dd) { return sf_launch16q<nb(), false, true, dd()>(m, a, pl, st); });
    return sf_visit_shape16(m.NB, pl.span, pl.head_mfma,
                            [&](auto nb, auto sp, auto hm) { return sf_launch16q<nb(), sp(), hm(), 0>(m, a, pl, st); });
  }
  // find / resolve launches of the deep tail: the unrolled kernel where the sampler itself runs one
  if ((a.best || a.att_list || a.count) && !a.z_in && pl.dd > 0 && (pl.fp32 || m.packed16B)) return sf_launch_find16(m, a, pl, st);
  return sf_visit_shape16(m.NB, pl.span, false, [&](auto nb, auto sp, auto) { return sf_launch16<nb(), sp()>(m, a, st); });
}
