// Weight-streaming GEMV over MXFP8 weights for the decode step on gfx950: y[M,N] = rs[m] * (X^[M,K] . W^[N,K]^T) (+ r) for
// 1 <= M <= 16, W = e4m3fn bytes [N,K] + E8M0 scale bytes [N,K/32] exactly as sd_mxfp8_quant leaves a weight, X^ = the
// MXFP8 quantisation of the bf16 rows of x, made inside the kernel (the bytes and scale bytes of mx_quant32, sd_mx.hip),
// rs[m] = 1 or the row's RMSNorm statistic (sd_mxfp8_quant's rstd).  An optional fused SwiGLU epilogue.  The quantiser of
// a K-step, the row statistic, the checks and the KPW / grid rules are in sd_gemv_mx.cuh, shared with the 64-row kernel of
// sd_gemv_mx_wide.hip.
//
// What they replace in the decode step of an MXFP8 model (one token per sequence, M = batch): per projection the
// sd_mxfp8_quant launch and the 128-row sd_gemm_mxfp8 tile that a batch of <= 16 rows fills to an eighth (HF
// modeling_qwen3.py:239-262, 81-83 through the reference's decode loop, soulxpodcast/engine/llm_engine.py:37-76).
//
// Shape of the kernel: the MFMA form.  The weights are the A operand of v_mfma_scale_f32_16x16x128_f8f6f4 -- one
// instruction takes 16 weight rows x 128 bytes of K with their real E8M0 bytes as the scale operand -- and the <= 16
// quantised rows of x are B, zero-padded to 16 columns.  Column m of the result depends on column m of B only and row n on
// row n of A only.  Lane maps (sd_mx.hip header): lane l = (r = l & 15, g = l >> 4) holds, for A,
// bytes k = 16g .. 16g+15 and k = 64+16g .. of row r of the K-step -- two 16-byte runs, contiguous in the weight row, each
// ONE non-temporal 16-byte load straight into the operand registers -- and the scale byte of (row r, block g); C/D: lane
// holds column (l & 15), rows 4 * (l >> 4) + 0..3.  No weight byte passes through LDS.
//
// K is cut into K-steps of 128; the KS = ceil(nk / KPW) <= 8 waves of a workgroup each own KPW in {1, 2, 4, 8} consecutive
// K-steps (KPW: the smallest that keeps KS <= 8, so it is a function of K alone).  A wave quantises its slices of the M
// rows of x once (the two lanes that share a 32-block exchange their amax by one xor-16 shuffle) and keeps them as B
// fragments in registers for the whole kernel.  A workgroup walks its 16-row tiles TR at a time; a wave's unit of work is
// (step, K-step): TR x 2 loads of 16 bytes and TR scale bytes per lane, the next unit's loads issued ahead of the current
// unit's MFMAs.
//
// Fixed summation order of one output element (a function of K alone, never of M, N, the grid or the CU count):
//   1. inside a K-step: the instruction's own order over its 128 products (every product is exact in fp32);
//   2. a wave's K-steps: ascending, chained through the accumulator operand, from 0;
//   3. the KS waves: through LDS, s = 0 .. KS-1 ascending;
//   4. bf16(sum * rs + float(r)) -- the epilogue expression of gemm_mx_kernel.
// No atomics.  Fused SwiGLU: gate tile and up tile of the same 16 columns sit side by side in a step; both sums are
// rounded to bf16 after the row scale (as gemm_mx_kernel's EPI_SWIGLU does) and swiglu_fwd_kernel's expression follows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sd_hip.h"
#include "sd_common.cuh"
#include "sd_prof.h"
#include "sd_runner.h"
#include "sd_gemv_mx.cuh"

#define ST ((hipStream_t)stream)

namespace {

// TR: 16-row weight tiles a wave takes per step (SwiGLU: TR / 2 gate tiles, each followed by its up tile)
template <int KPW, int TR, bool SWIGLU>
__global__ __launch_bounds__(512) void gemv_mx_kernel(const GemvMxArgs a) {
  __shared__ f32x4 red_s[kMaxWaves][TR][64];
  __shared__ float rstd_s[16];
  const int lane = lane_id(), wv = wave_id_uniform(), nw = a.KS;
  const int fr = lane & 15, fg = lane >> 4;
  const int K = a.K, M = a.M, nk = K >> 7, nblk = K >> 5;
  constexpr int UPS = SWIGLU ? TR / 2 : TR;  // units per step
  const int units = (a.N + 15) >> 4;
  const int u0 = blockIdx.x * a.upw, u1 = min(units, u0 + a.upw);
  const int nsteps = (u1 - u0 + UPS - 1) / UPS;
  if (nsteps <= 0) return;  // block-uniform (the grid leaves no workgroup without rows)

  // weight row behind (step t, tile j, fragment row fr); rows past the edge re-read the last row, never stored
  auto w_row = [&](int t, int j) {
    const int u = min(u0 + t * UPS + (SWIGLU ? j >> 1 : j), u1 - 1);
    const int c = min(u * 16 + fr, a.N - 1);
    return (SWIGLU && (j & 1)) ? a.N + c : c;
  };
  // K-step i of this wave; steps past the end re-read the last one (an address inside the row) and are not multiplied
  const int k0 = wv * KPW;
  auto load = [&](i32x8(&wa)[TR], int (&sa)[TR], int t, int i) {
    const int ks = min(k0 + i, nk - 1);
#pragma unroll
    for (int j = 0; j < TR; ++j) {
      const long row = w_row(t, j);
      const uint8_t* p = a.wq + row * K + ks * 128 + fg * 16;
      const u32x4 lo = __builtin_nontemporal_load((const u32x4*)p);
      const u32x4 hi = __builtin_nontemporal_load((const u32x4*)(p + 64));
      wa[j] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      sa[j] = a.ws[row * nblk + ks * 4 + fg];
    }
  };
  // A queue of D + 1 units: D are in flight while the oldest is multiplied.  Unit u = (step u / KPW, K-step u % KPW); the
  // slots rotate by renaming in the unrolled loop below.  D = 1 is what measured best: most workgroups own one or two
  // steps, and units past a workgroup's last one are loaded all the same (D = 4 / TR cost 1.5-2 us per launch).
  constexpr int D = 1;
  i32x8 wq_[D + 1][TR];
  int sq_[D + 1][TR];
#pragma unroll
  for (int d = 0; d < D; ++d)  // the first weights are on their way before x is touched
    load(wq_[d], sq_[d], min(d / KPW, nsteps - 1), d % KPW);

  // ---- this wave's K-steps of the M rows of x as B fragments: lane (fr, fg) quantises bytes 16fg.. and 64+16fg.. of row fr
  // (a rolled loop whose result is moved into its register set by selects: unrolled, hipcc keeps the 32 floats of every
  // K-step live at once)
  i32x8 xq[KPW];
  int xs[KPW];
#pragma unroll
  for (int j = 0; j < KPW; ++j) { xq[j] = i32x8{0, 0, 0, 0, 0, 0, 0, 0}; xs[j] = 0; }
  // the raw rows of K-step i + 1 are loaded while K-step i is quantised (columns past M and K-steps past the end: a valid
  // address, the values replaced by zeros)
  auto load_x = [&](bf16x8(&raw)[4], int i) {
    const bf16* p = a.x + (long)min(fr, M - 1) * a.ldx + min(k0 + i, nk - 1) * 128 + fg * 16;
    raw[0] = *(const bf16x8*)p; raw[1] = *(const bf16x8*)(p + 8);
    raw[2] = *(const bf16x8*)(p + 64); raw[3] = *(const bf16x8*)(p + 72);
  };
  bf16x8 raw[4], raw_next[4];
  load_x(raw, 0);
#pragma unroll 1
  for (int i = 0; i < KPW; ++i) {
    load_x(raw_next, i + 1);
    float lo[16], hi[16];
    kstep_floats(raw, fr < M && k0 + i < nk, lo, hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) raw[e] = raw_next[e];
    i32x8 q;
    int sc;
    quant_kstep(lo, hi, fr, fg, q, sc);
#pragma unroll
    for (int j = 0; j < KPW; ++j)
      if (j == i) { xq[j] = q; xs[j] = sc; }
  }

  // ---- the rows' RMSNorm statistic (published by the barrier in front of the first combine)
  row_rstd<SD_GEMV_MAX_M>(a.x, a.ldx, M, K, a.norm, a.eps, rstd_s, lane, wv, nw);

  const int tid = threadIdx.x, nthr = nw * 64;
  for (int t = 0; t < nsteps; ++t) {
    f32x4 acc[TR];
#pragma unroll
    for (int j = 0; j < TR; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
      // the loads of the unit D ahead go out first (past the last step: the last step's again, so that the load stays
      // unconditional and the wait in front of the MFMAs counts loads)
      load(wq_[D], sq_[D], min(t + (i + D) / KPW, nsteps - 1), (i + D) % KPW);
      if (k0 + i < nk) {  // wave-uniform
#pragma unroll
        for (int j = 0; j < TR; ++j)
          acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wq_[0][j], xq[i], acc[j], 0, 0, 0, sq_[0][j], 0, xs[i]);
      }
#pragma unroll
      for (int d = 0; d < D; ++d)
#pragma unroll
        for (int j = 0; j < TR; ++j) { wq_[d][j] = wq_[d + 1][j]; sq_[d][j] = sq_[d + 1][j]; }
    }
#pragma unroll
    for (int j = 0; j < TR; ++j) red_s[wv][j][lane] = acc[j];
    __syncthreads();
    // ---- combine: entry (tile or pair q, lane slot l) = column m = l & 15, rows 4 * (l >> 4) + 0..3 of the tile
    for (int e = tid; e < UPS * 64; e += nthr) {
      const int q = e >> 6, l = e & 63;
      const int m = l & 15, u = u0 + t * UPS + q;
      if (m >= M || u >= u1) continue;
      const float rs = rstd_s[m];
      const int n0 = u * 16 + 4 * (l >> 4);
      if constexpr (!SWIGLU) {
        f32x4 sum = red_s[0][q][l];
        for (int s = 1; s < nw; ++s) sum += red_s[s][q][l];  // slice order: fixed
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int n = n0 + c;
          if (n < a.N) {
            const float v = a.r ? sum[c] * rs + (float)a.r[(long)m * a.ldr + n] : sum[c] * rs;
            a.y[(long)m * a.ldy + n] = (bf16)v;
          }
        }
      } else {
        f32x4 sg = red_s[0][2 * q][l], su = red_s[0][2 * q + 1][l];
        for (int s = 1; s < nw; ++s) { sg += red_s[s][2 * q][l]; su += red_s[s][2 * q + 1][l]; }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int n = n0 + c;
          if (n < a.N) {
            // gate and up as the bf16 projection stores them, then swiglu_fwd_kernel's expression
            const float g = (float)(bf16)(sg[c] * rs), up = (float)(bf16)(su[c] * rs);
            a.y[(long)m * a.ldy + n] = (bf16)(g / (1.f + __expf(-g)) * up);
          }
        }
      }
    }
    if (t + 1 < nsteps) __syncthreads();  // red_s is free again before the next step's sums land
  }
}

template <bool SWIGLU>
int launch(GemvMxArgs a, void* stream) {
  const int nk = a.K >> 7;
  const int kpw = kpw_of(nk);
  a.KS = (nk + kpw - 1) / kpw;
  const int cus = cu_count();
  if (cus <= 0) return SD_ERR_WORKSPACE;
  const int units = (a.N + 15) >> 4;
  int upw, ups;
  grid_of(units, cus, SWIGLU, upw, ups);
  a.upw = upw;
  const int tr = SWIGLU ? 2 * ups : ups;
  const unsigned grid = (unsigned)((units + upw - 1) / upw), block = (unsigned)(a.KS * 64);
  SdProfScope prof(SD_K_GEMM_NT, 2.0 * a.M * (SWIGLU ? 2.0 : 1.0) * a.N * a.K, ST);
  SD_PROF_LABEL("gemv_mx_kernel<%d, %d, %s>", kpw, tr, SWIGLU ? "true" : "false");
#define SD_GO(KPW_, TR_) hipLaunchKernelGGL((gemv_mx_kernel<KPW_, TR_, SWIGLU>), dim3(grid), dim3(block), 0, ST, a)
#define SD_TR(KPW_)                                          \
  do {                                                       \
    if (tr == 4) SD_GO(KPW_, 4);                             \
    else if (tr == 2) SD_GO(KPW_, 2);                        \
    else if constexpr (!SWIGLU) SD_GO(KPW_, 1);              \
  } while (0)
  switch (kpw) {
    case 1: SD_TR(1); break;
    case 2: SD_TR(2); break;
    case 4: SD_TR(4); break;
    default: SD_TR(8); break;
  }
#undef SD_TR
#undef SD_GO
  SD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// the checks of the two entries without a launch (the MXFP8 decode step asks before it commits to the GEMV sequence);
// ldy = N and no residual stand for the SwiGLU form with N = I
int sd_gemv_mx_check(const void* x, int64_t ldx, const void* w_q, const void* w_scale, const void* y, int64_t ldy,
                     const void* r, int64_t ldr, int M, int N, int K) {
  return validate(x, w_q, w_scale, y, r, M, N, K, ldx, ldy, ldr, SD_GEMV_MAX_M);
}

extern "C" int sd_gemv_mxfp8(const void* x, int64_t ldx, const void* w_q, const void* w_scale, void* y, int64_t ldy,
                             const void* r, int64_t ldr, int norm, float eps, int M, int N, int K, void* stream) {
  const int rc = validate(x, w_q, w_scale, y, r, M, N, K, ldx, ldy, ldr, SD_GEMV_MAX_M);
  if (rc) return rc;
  GemvMxArgs a = {};
  a.x = (const bf16*)x; a.wq = (const uint8_t*)w_q; a.ws = (const uint8_t*)w_scale; a.r = (const bf16*)r; a.y = (bf16*)y;
  a.eps = eps; a.norm = norm ? 1 : 0; a.M = M; a.N = N; a.K = K;
  a.ldx = ldx; a.ldy = ldy; a.ldr = ldr;
  return launch<false>(a, stream);
}

extern "C" int sd_gemv_mxfp8_swiglu(const void* x, const void* wgu_q, const void* wgu_scale, void* act, int norm, float eps,
                                    int M, int I, int K, void* stream) {
  const int rc = validate(x, wgu_q, wgu_scale, act, nullptr, M, I, K, K, I, 0, SD_GEMV_MAX_M);
  if (rc) return rc;
  GemvMxArgs a = {};
  a.x = (const bf16*)x; a.wq = (const uint8_t*)wgu_q; a.ws = (const uint8_t*)wgu_scale; a.y = (bf16*)act;
  a.eps = eps; a.norm = norm ? 1 : 0; a.M = M; a.N = I; a.K = K;
  a.ldx = K; a.ldy = I; a.ldr = 0;
  return launch<true>(a, stream);
}
