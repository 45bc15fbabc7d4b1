// What the two weight-streaming GEMVs over MXFP8 weights share (sd_gemv_mx.hip: M <= 16; sd_gemv_mx_wide.hip: M <= 64): the
// arguments, the in-kernel quantiser of a K-step of x (mx_quant32's bytes and scale bytes, sd_mx.hip), the rows' RMSNorm
// statistic, the checks and the two launch rules that fix the summation order (KPW) and the grid.  Both kernels form an
// output element from these statements, which is why a 16-row slice of the wide kernel's result has the bits of the 16-row
// kernel's.  Internal: not installed, not ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sd_hip.h"
#include "sd_common.cuh"

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int kMaxWaves = 8;   // K slices of a workgroup at most
constexpr int kMaxK = 8192;    // = kMaxWaves * 8 K-steps of 128

struct GemvMxArgs {
  const bf16* x;
  const uint8_t *wq, *ws;
  const bf16* r;
  bf16* y;
  float eps;
  int norm;
  int M, N, K;  // N: weight rows of the plain form; columns of act (= I) of the SwiGLU form
  long ldx, ldy, ldr;
  int KS;       // waves of the workgroup = K slices
  int upw;      // 16-row units per workgroup (a multiple of the units per step): tiles, or gate/up tile pairs
};

// One 16-element run of a 32-block whose amax is known: mx_quant32's arithmetic on half a block
SD_DEV u32x4 quant16(const float (&x)[16], float inv) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = fminf(fmaxf(x[4 * i + j] * inv, -448.f), 448.f);
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], p, true);
    w[i] = (uint32_t)p;
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}
// scale byte (e + 127) and 2^-e of a block with this amax: the statements of mx_quant32
SD_DEV int scale_of(float amax, float& inv) {
  const int eb = (int)(__builtin_bit_cast(uint32_t, amax) >> 23);
  const int sb = eb > 8 ? eb - 8 : 0;
  inv = __builtin_bit_cast(float, (uint32_t)(254 - sb) << 23);
  return sb;
}

// The raw bf16 values of one K-step of a row as lane (fr = lane & 15, fg = lane >> 4) holds them -- elements 16 fg .. (lo)
// and 64 + 16 fg .. (hi) -- as floats; not live: zeros
SD_DEV void kstep_floats(const bf16x8 (&raw)[4], bool live, float (&lo)[16], float (&hi)[16]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    lo[e] = live ? (float)raw[0][e] : 0.f; lo[8 + e] = live ? (float)raw[1][e] : 0.f;
    hi[e] = live ? (float)raw[2][e] : 0.f; hi[8 + e] = live ? (float)raw[3][e] : 0.f;
  }
}
// Those floats to the lane's B fragment q and the scale byte sc of block fg (all zeros: a zero fragment).  Every lane of
// the wave takes part: three shuffles.
SD_DEV void quant_kstep(const float (&lo)[16], const float (&hi)[16], int fr, int fg, i32x8& q, int& sc) {
  float alo = 0.f, ahi = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) { alo = fmaxf(alo, fabsf(lo[e])); ahi = fmaxf(ahi, fabsf(hi[e])); }
  // the other half of each 32-block is in the lane with fg ^ 1
  alo = fmaxf(alo, __shfl_xor(alo, 16, 64));
  ahi = fmaxf(ahi, __shfl_xor(ahi, 16, 64));
  float ilo, ihi;
  const int slo = scale_of(alo, ilo), shi = scale_of(ahi, ihi);
  const u32x4 qlo = quant16(lo, ilo), qhi = quant16(hi, ihi);
  q = i32x8{(int)qlo[0], (int)qlo[1], (int)qlo[2], (int)qlo[3], (int)qhi[0], (int)qhi[1], (int)qhi[2], (int)qhi[3]};
  // this lane carries the scale of block fg: blocks 0, 1 are the low runs of the lanes fg = 0, 2; blocks 2, 3 the high
  // runs of the lanes fg = 0, 3
  const int src_g = fg == 1 ? 2 : fg == 2 ? 0 : fg;
  const int both = __shfl(slo | (shi << 8), fr + 16 * src_g, 64);
  sc = (fg < 2 ? both : both >> 8) & 0xff;
}

// The M rows' RMSNorm statistic into rstd_s[0..MAXM): mxfp8_quant_kernel's statements (one wave per row, one 32-block per
// lane and pass); 1 without a norm.  The caller's next __syncthreads() publishes it.
template <int MAXM>
SD_DEV void row_rstd(const bf16* x, long ldx, int M, int K, int norm, float eps, float* rstd_s, int lane, int wv, int nw) {
  if (norm) {
    const int nblk = K >> 5;
    for (int row = wv; row < M; row += nw) {
      const bf16* xr = x + (long)row * ldx;
      float ss = 0.f;
      for (int b = lane; b < nblk; b += 64) {
        float f[32];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bf16x8 v = *(const bf16x8*)(xr + b * 32 + i * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[i * 8 + e] = (float)v[e];
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) ss += f[i] * f[i];
      }
      ss = wave_sum(ss);
      if (lane == 0) rstd_s[row] = rsqrtf(ss / (float)K + eps);
    }
  } else if (threadIdx.x < MAXM) {
    rstd_s[threadIdx.x] = 1.f;
  }
}

// CUs of the current device (kept per device; it only sizes the grid, no output bit depends on it)
int cu_count() {
  static int cached[64];
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev >= 0 && dev < 64 && cached[dev] > 0) return cached[dev];
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (dev >= 0 && dev < 64) cached[dev] = n;
  return n;
}

// the checks of both kernels; max_m: SD_GEMV_MAX_M or SD_GEMV_MX_WIDE_MAX_M
int validate(const void* x, const void* wq, const void* ws, const void* y, const void* r, int M, int N, int K, int64_t ldx,
             int64_t ldy, int64_t ldr, int max_m) {
  if (!x || !wq || !ws || !y || M <= 0 || N <= 0 || K <= 0) return SD_ERR_SHAPE;
  if (M > max_m || (K & 127) || K > kMaxK || N > (1 << 29)) return SD_ERR_UNSUPPORTED;
  if (ldx < K || ldy < N || (r && ldr < N)) return SD_ERR_UNSUPPORTED;
  if ((ldx & 7) || ((uintptr_t)x & 15) || ((uintptr_t)wq & 15) || ((uintptr_t)ws & 3)) return SD_ERR_UNSUPPORTED;
  return 0;
}

// K-steps of 128 per wave, from K alone: it fixes the summation order
inline int kpw_of(int nk) { return nk <= 8 ? 1 : nk <= 16 ? 2 : nk <= 32 ? 4 : 8; }

// grid: from N and the CU count only -- about two workgroups per CU while a workgroup keeps one 16-row unit; the units a
// wave takes per step (1, 2 or 4 tiles; 1 or 2 gate/up pairs) follow from what a workgroup got
inline void grid_of(int units, int cus, bool swiglu, int& upw, int& ups) {
  upw = (units + 2 * cus - 1) / (2 * cus);
  ups = swiglu ? (upw >= 2 ? 2 : 1) : (upw >= 4 ? 4 : upw >= 2 ? 2 : 1);
  upw = (upw + ups - 1) / ups * ups;
}

}  // namespace
