// Device helpers the decode-side cache kernels share: sd_decode.hip (append, split-KV attention, merge as three launches)
// and sd_cache_step.hip (the same work as one launch) -- the partition constants, the 16-byte pack / unpack, the page
// table lookup and the MXFP8 page format.  Moved here unchanged from sd_decode.hip.  Internal: not installed.
#pragma once
#include <math.h>
#include "sd_common.cuh"
#include "../../include/sd_hip.h"

namespace {

constexpr int kPart = 256;  // keys per split-KV partition (fixed: the output bits must not depend on a launch choice)
constexpr int kRec = 132;   // floats of one partial record: max, sum, 2 pad, 128 accumulators (16-byte aligned rows)
constexpr float kNegBig = -1.0e30f;  // "no key yet": finite, so that max - max never forms inf - inf

SD_DEV void unpack8(bf16x8 v, float* f) {
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
}
SD_DEV bf16x8 pack8(const float* f) {
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (bf16)f[e];
  return v;
}
SD_DEV bf16x8 zero8() {
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (bf16)0.f;
  return v;
}
SD_DEV int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

static_assert(SD_KV_PAGE == kPart, "a page is one decode partition");
struct PageArgs {
  const int32_t* table;  // int32 [B][max_pages]
  int max_pages, n_pages;
  uint8_t *k_scale = nullptr, *v_scale = nullptr;  // 8-bit pages only: E8M0 planes [n_pages][256][Hkv*4]
};
// Element offset of slot s (0 <= s < max_pages * 256) of row b in a pool plane.  false: the table entry lies outside the
// pool, and the caller must not store through it.
SD_DEV bool page_slot(const PageArgs& pg, int b, int s, int KD, long* off) {
  const int page = pg.table[(long)b * pg.max_pages + (s >> 8)];
  *off = ((long)page * SD_KV_PAGE + (s & (SD_KV_PAGE - 1))) * KD;
  return page >= 0 && page < pg.n_pages;
}

// ---- 8-bit pages: the number format of mx_quant32 (sd_mx.hip) on the 8 elements a lane owns of a 32-element block.
// The four lanes of a block are a DPP quad (chunks 4i .. 4i + 3 of a head vector sit in four consecutive lanes in every
// kernel below, and those lanes leave together or not at all), so the block maximum is two quad permutes.
SD_DEV float quad_max(float v) {
  v = fmaxf(v, dpp_move<0xB1>(v));  // quad_perm [1,0,3,2]
  return fmaxf(v, dpp_move<0x4E>(v));  // quad_perm [2,3,0,1]
}
// v: the bf16 values the bf16 pool would hold at chunk c (8 elements) of pool row `row`; writes their 8 e4m3 bytes and,
// from the first lane of the block, the block's E8M0 byte.  e = floor(log2(amax)) - 8 clamped below at -127, RNE,
// saturation at +-448: every product is exact in fp32.
SD_DEV void mx_store8(bf16x8 v, uint8_t* data, uint8_t* scale, long row, int Hkv, int c) {
  float f[8];
  unpack8(v, f);
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
  amax = quad_max(amax);
  const int eb = (int)(__builtin_bit_cast(uint32_t, amax) >> 23);  // biased exponent of amax (sign is 0)
  const int sb = eb > 8 ? eb - 8 : 0;                              // e + 127
  const float inv = __builtin_bit_cast(float, (uint32_t)(254 - sb) << 23);  // 2^-e
  float y[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = fminf(fmaxf(f[e] * inv, -448.f), 448.f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  *(u32x2*)(data + (row * Hkv * 16 + c) * 8) = u32x2{(uint32_t)lo, (uint32_t)hi};
  if ((c & 3) == 0) scale[row * Hkv * 4 + (c >> 2)] = (uint8_t)sb;
}
// 8 e4m3 bytes and their block's E8M0 byte -> the values they stand for, float(q) * 2^e.  For scale bytes 3..246 every
// product is a bf16 number, so the fp32 value IS what a bf16 pool holding the dequantised rows would give unpack8.  An
// all-zero block (byte 0) comes out as zeros.
SD_DEV void unpack8_mx(u32x2 q, uint32_t scale_byte, float* f) {
  const float sc = __builtin_bit_cast(float, scale_byte << 23);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[h], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[h], true);
    f[4 * h] = a[0] * sc; f[4 * h + 1] = a[1] * sc; f[4 * h + 2] = b[0] * sc; f[4 * h + 3] = b[1] * sc;
  }
}

}  // namespace
