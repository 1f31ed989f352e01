// sf_pack.h -- the pack rules, one element at a time: logical parameter vector -> one entry of an operand image.  Called by
// k_pack / k_pack_bf16 / k_pack_bf16_split (sf_kernels.hip) and by the segments of k_train_prep (sf_train.hip); the table flags
// are those of sf_layout.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_layout.h"

// fp32: the sum of up to two logical entries (-1: none); second index SF_PACK_TANH_SCALE: the one value x 2 log2(e).
// sf_layout.cpp writes that flag into the 16-row tables (src16b) only: the forward, transposed and cooperative tables hold
// logical indices or -1 as their second index, so for them this is the plain sum.
__device__ __forceinline__ float sf_pack_f32(const float* __restrict__ flat, int a, int b) {
  float v = 0.f;
  if (a >= 0) v = flat[a];
  if (b >= 0) v += flat[b];
  else if (b == SF_PACK_TANH_SCALE) v *= SF_TANH_PRESCALE;
  return v;
}

__device__ __forceinline__ unsigned short sf_pack_bf16(const float* __restrict__ flat, int a) {
  return __builtin_bit_cast(unsigned short, (__bf16)(a >= 0 ? flat[a] : 0.f));  // round to nearest even
}

// split bf16: a = logical index | (part << 30) | SF_PACK_SPLIT_SCALED; part 0 -> hi = bf16(w) (round to nearest even), part 1 ->
// lo = bf16(w - hi)
__device__ __forceinline__ unsigned short sf_pack_bf16_split(const float* __restrict__ flat, int a) {
  if (a < 0) return 0;
  const float w = flat[a & SF_PACK_SPLIT_INDEX] * ((a & SF_PACK_SPLIT_SCALED) ? SF_TANH_PRESCALE : 1.0f);
  const __bf16 hi = (__bf16)w;
  return __builtin_bit_cast(unsigned short, (a >> 30) & 1 ? (__bf16)(w - (float)hi) : hi);
}
