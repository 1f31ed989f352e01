// sf_ar_sampler.h -- control flow of the rejection sampler of the autoregressive flows (`backend="lampe"`) as function templates
// over an ENGINE, a small struct around a candidate routine:
//   NE                         entries (candidates) per wave
//   DD                         the flow's dimensions when they are a compile-time value (the draw stores unroll), 0: dims() at run time
//   lead()                     does this lane carry the side effects of its entry
//   col()                      the lane's entry column in [0, NE)
//   candidate(g, slot, att, active) -> bool   noise of (slot, attempt) through the inverse flow of row g, finite + box test
//   value(d)                   dimension d of that candidate, valid after candidate()
//   list_seen_dry(), wave_leaves()            developer hooks of the persistent loop (empty unless the engine's file traces)
// The three templates are the bodies of the persistent kernel and of the two chip-wide round kernels.  The 64-candidate LDS
// kernels of sf_nsfar.hip are instantiated from them (ArLdsEngine: NE = 64, every lane leads).  The 16-candidate register-tile
// kernels of sf_nsfar16.hip carry the same control flow WRITTEN OUT (NE = 16, lead = lane < 16, col = lane & 15) and share only
// the fence below: one inlined layer between those kernels and their candidate routine changes the optimiser's output for the
// two-tile shapes (two to three times the spilled registers at D >= 6; profiles/ar_sampler_header_kernel_resources.txt), so a
// change to the control flow is made here and there until that is solved.
// With ArLdsEngine as the only client, parts of the contract do nothing today: lead() is always true, col() is the lane, DD is 0
// (the compile-time branch of ar_each_dim is not taken) and both hooks are empty.  They are kept on purpose: they are exactly what
// differs in the written-out tile kernels (lane < 16, lane & 15, DD unrolled stores, the -DSF_A16_TRACE stamps), i.e. the
// interface those kernels are to be instantiated through, and they cost the LDS kernels nothing (constant-folded).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_device.h"
#include "sf_nsfar.h"

// order the LDS traffic of ONE wave (its LDS operations execute in program order: a read issued after a write of another lane
// of the same wave sees it; this only keeps the compiler from reordering them).  The retry list is wave-private on both
// engines, so this -- not a workgroup barrier -- is the loop's fence; the one-wave workgroups of k_ar_sample had __syncthreads()
// there, so a -DSF_FUZZ_SCHED build no longer delays at those two points (there is no second wave to race with).
__device__ __forceinline__ void ar_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <class E, class F>
__device__ __forceinline__ void ar_each_dim(const E& eng, F f) {
  if constexpr (E::DD > 0) {
#pragma unroll
    for (int d = 0; d < E::DD; ++d) f(d);
  } else {
    for (int d = 0; d < eng.dims(); ++d) f(d);
  }
}
template <class E>
__device__ __forceinline__ void ar_write_nan(const E& eng, float* __restrict__ out, unsigned long long slot) {
  ar_each_dim(eng, [&](int d) { out[slot * eng.dims() + d] = __builtin_nanf(""); });
}
// row of a slot (32-bit division where the call's sizes fit: a 64-bit one is ~200 instructions)
__device__ __forceinline__ long ar_row_of(unsigned long long slot, long S, bool small) {
  return small ? (long)((uint32_t)slot / (uint32_t)S) : (long)(slot / (unsigned long long)S);
}

// PERSISTENT LOOP.  A wave works (slot, attempt) items, NE at a time -- its own rejects first (r_slot / r_att: the wave-private
// retry list) -- until the slot list is exhausted.
//   * The slot list is walked ACROSS its rows: item i is entry (i % R) * C + i / R of the list seen as R x C (whole catalogue:
//     R = rows, C = draws per row, i.e. draw i / M of row i % M; an explicit list, sorted by slot: R = 4096 pieces; positions past
//     n_slots are holes) -- the items of a wave then belong to different rows, so a row that accepts one draw in hundreds leaves
//     ONE stubborn entry in many waves instead of NE in a few.
//   * Once the list has run dry a wave spends its idle columns on its open entries: W = 2^lw <= NE / entries attempts of each side
//     by side, the LOWEST accepted attempt wins (what the one-at-a-time order would have kept).
//   * window_end < max_attempts: an entry that has used up attempts [0, window_end) is appended to surv[] -- the find / resolve
//     rounds spread its further attempts over the whole chip -- instead of being carried on by this wave.
//   * cursor[2]: evaluations (items worked), cursor[3]: first attempts rejected -- statistics for sf_flow_sample_stats; they stay in
//     the wave until it leaves (per round they were two more atomics on the cache line of the queue head that every wave's next
//     fetch waits for).
template <class E>
__device__ __forceinline__ void ar_sample_loop(E& eng, const SfArLaunch& L, int lane, unsigned long long* r_slot, uint32_t* r_att) {
  constexpr int NE = E::NE;
  const int s = eng.col();
  const bool lead = eng.lead();
  const long S = L.S;
  const bool interleave = L.walk_R > 1;
  const unsigned long long n_index = interleave ? L.walk_R * L.walk_C : (unsigned long long)L.n_slots;   // (>= n_slots: holes are skipped)
  const bool small = n_index <= 0xffffffffull && (unsigned long long)L.n_slots <= 0xffffffffull && (unsigned long long)S <= 0xffffffffull;
  int n_retry = 0;
  bool list_done = false;
  unsigned int n_ev = 0, n_rej0 = 0;
  for (;;) {
    if (list_done) eng.list_seen_dry();
    const int take = list_done ? 0 : NE - n_retry;
    unsigned long long base = n_index;
    if (take > 0) {
      if (lane == 0) base = atomicAdd(L.cursor, (unsigned long long)take);
      base = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    }
    int n_fresh = 0;
    if (take > 0) {
      if (base >= n_index) list_done = true;
      else {
        const unsigned long long left = n_index - base;
        n_fresh = left < (unsigned long long)take ? (int)left : take;
        if (n_fresh < take) list_done = true;
      }
    }
    const int n_ent = n_retry + n_fresh;
    if (n_ent == 0) {
      eng.wave_leaves();
      if (lane == 0) {
        if (n_ev) atomicAdd(L.cursor + 2, (unsigned long long)n_ev);
        if (n_rej0) atomicAdd(L.cursor + 3, (unsigned long long)n_rej0);
      }
      break;
    }
    int lw = 0;   // log2 of the speculation width
    if (list_done && !L.count)
      while ((n_ent << (lw + 1)) <= NE) ++lw;
    const int W = 1 << lw;
    const int e = s >> lw, sub = s & (W - 1);
    unsigned long long slot = 0;
    uint32_t att0 = 0;
    bool exists = e < n_ent;   // (an entry of this round: a carried one, or a fresh item that is not a hole of the cover)
    if (exists) {
      if (e < n_retry) { slot = r_slot[e]; att0 = r_att[e]; }
      else {
        const unsigned long long idx = base + (unsigned)(e - n_retry);
        unsigned long long pos = idx;
        if (interleave) {   // (32-bit division where the cover fits)
          if (small) { const uint32_t i32 = (uint32_t)idx, r32 = (uint32_t)L.walk_R; pos = (unsigned long long)(i32 % r32) * L.walk_C + i32 / r32; }
          else pos = (idx % L.walk_R) * L.walk_C + idx / L.walk_R;
        }
        if (pos >= (unsigned long long)L.n_slots) exists = false;   // (a hole of the R x C cover)
        else slot = L.slots ? (unsigned long long)L.slots[pos] : pos;
      }
    }
    const uint32_t att = att0 + (uint32_t)sub;
    const bool active = exists && att < L.window_end;
    ar_wave_sync();   // (the retry list has been read)
    const long g = exists ? ar_row_of(slot, S, small) : 0;
    const bool ok = eng.candidate(g, slot, att, active);
    const unsigned long long m_ok = __ballot(ok && lead);
    n_ev += (unsigned)__popcll(__ballot(active && lead));
    n_rej0 += (unsigned)__popcll(__ballot(active && lead && !ok && att == 0u));
    if (L.count) {   // acceptance counting (leakage correction): one attempt per item, nothing written
      // (items are consecutive slots: those of a wave belong to one row, a few at row boundaries -- one add for the first row's
      //  hits instead of up to NE same-address atomics, the others on their own)
      const long g0 = ((long)__builtin_amdgcn_readfirstlane((int)(g >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)g);
      const unsigned long long same = __ballot(lead && g == g0);
      const int c0 = __popcll(m_ok & same);
      if (lane == 0 && c0) atomicAdd(L.count + g0, c0);
      if (ok && lead && g != g0) atomicAdd(L.count + g, 1);
      n_retry = 0;
      continue;
    }
    // the entry's columns: [e W, e W + W); its lowest accepted attempt (W == 64 takes the whole ballot: no 64-bit shift by 64)
    const unsigned long long grp = (NE == 64 && W == 64) ? m_ok : ((m_ok >> (e * W)) & ((1ull << W) - 1ull));
    const bool resolved = grp != 0ull;
    const int win = resolved ? __builtin_ctzll(grp) : 0;
    const bool leader = exists && sub == 0 && lead;
    const uint32_t tried_now = att0 + (uint32_t)W < L.window_end ? (uint32_t)W : L.window_end - att0;   // attempts of this round that count
    const bool window_out = leader && !resolved && att0 + (uint32_t)W >= L.window_end;
    bool give_up = window_out && L.window_end >= L.max_attempts;
    if (L.g_try && leader) {   // no ceiling asked for: a row whose open slots spent 1e5 attempts without ONE accepted draw is written off
      const int tried = atomicAdd(L.g_try + g, (int)(resolved ? win + 1 : (int)tried_now)) + (int)(resolved ? win + 1 : (int)tried_now);
      if (resolved) atomicAdd(L.g_acc + g, 1);
      else if (tried >= 100000 && __hip_atomic_load(L.g_acc + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) give_up = true;
    }
    if (ok && lead && sub == win) {   // the winner writes the draw
      ar_each_dim(eng, [&](int d) { L.out[slot * eng.dims() + d] = eng.value(d); });
      if (L.n_drawn) sf_sat_add(L.n_drawn + g, (int32_t)(att + 1u));
    }
    if (give_up) {
      ar_write_nan(eng, L.out, slot);
      if (L.n_drawn) sf_sat_add(L.n_drawn + g, (int32_t)(att0 + tried_now));
      atomicAdd(L.n_unfilled, 1u);
    }
    if (window_out && !give_up) L.surv[atomicAdd(L.n_surv, 1u)] = (uint32_t)slot;   // (hand-over; a row written off by the progress rule is not)
    const bool again = leader && !resolved && !give_up && !window_out;
    const unsigned long long m = __ballot(again);
    if (again) {
      const int pos = __popcll(m & ((1ull << lane) - 1ull));
      r_slot[pos] = slot;
      r_att[pos] = att0 + (uint32_t)W;
    }
    n_retry = __popcll(m);
    ar_wave_sync();
  }
}

// FIND: attempts [base, att_end) of every survivor side by side -- workgroup (e, j) tries attempts base + 64 j + NE wv + column of
// survivor e (wv: the wave of the workgroup; 64 attempts per workgroup on both engines); an accepted attempt only lowers best[e].
// RESOLVE (below) re-evaluates exactly attempt best[e] and writes the draw: the slot keeps its LOWEST accepted attempt, whatever
// the round's width and the schedule were.
template <class E>
__device__ __forceinline__ void ar_find_round(E& eng, const SfArLaunch& L, const SfArRound& R, int lane, int wv) {
  const unsigned int e = blockIdx.x / R.chunks, j = blockIdx.x - e * R.chunks;
  if (e >= R.n_surv) return;
  const unsigned long long slot = R.surv[e];
  const uint32_t att = R.base + 64u * j + (uint32_t)(E::NE * wv + eng.col());
  const bool active = att < R.att_end;
  const long g = (long)(slot / (unsigned long long)L.S);
  const bool ok = eng.candidate(g, slot, att, active);
  if (ok && eng.lead()) atomicMin(R.best + e, att);
  const unsigned long long ma = __ballot(active && eng.lead());
  if (lane == 0) atomicAdd(L.cursor + 2, (unsigned long long)__popcll(ma));
}

// RESOLVE: survivor 64 blockIdx + NE wv + column.  Found: its draw is written.  Not found: the ceiling (att_end >= max_attempts) or
// the row-level progress rule write it off, else it goes on to next[].  The round tried attempts [base, att_end).
template <class E>
__device__ __forceinline__ void ar_resolve_round(E& eng, const SfArLaunch& L, const SfArRound& R, int wv) {
  const unsigned int e = blockIdx.x * 64u + (unsigned)(E::NE * wv + eng.col());
  const bool exists = e < R.n_surv;
  const unsigned long long slot = exists ? R.surv[e] : 0ull;
  const uint32_t b = exists ? R.best[e] : 0xffffffffu;
  const bool found = exists && b != 0xffffffffu;
  const long g = exists ? (long)(slot / (unsigned long long)L.S) : 0;
  const bool ok = eng.candidate(g, slot, found ? b : 0u, found);
  if (!eng.lead()) return;
  const uint32_t tried_now = R.att_end - R.base;
  if (found) {   // (ok by construction: the find launch accepted this very attempt)
    ar_each_dim(eng, [&](int d) { L.out[slot * eng.dims() + d] = ok ? eng.value(d) : __builtin_nanf(""); });
    if (L.n_drawn) sf_sat_add(L.n_drawn + g, (int32_t)(b + 1u));
    if (L.g_acc) atomicAdd(L.g_acc + g, 1);
    if (L.g_try) atomicAdd(L.g_try + g, (int)tried_now);
  } else if (exists) {
    bool give_up = R.att_end >= L.max_attempts;
    if (L.g_try) {   // (uncapped: the progress rule, as in the persistent loop)
      const int tried = atomicAdd(L.g_try + g, (int)tried_now) + (int)tried_now;
      if (tried >= 100000 && __hip_atomic_load(L.g_acc + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) give_up = true;
    }
    if (give_up) {
      ar_write_nan(eng, L.out, slot);
      if (L.n_drawn) sf_sat_add(L.n_drawn + g, (int32_t)R.att_end);
      atomicAdd(L.n_unfilled, 1u);
    } else {
      R.next[atomicAdd(R.n_next, 1u)] = (uint32_t)slot;
    }
  }
}
