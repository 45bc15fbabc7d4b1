// Wide weight-streaming GEMV over MXFP8 weights for the decode step on gfx950: the semantics of sd_gemv_mx.hip for
// 1 <= M <= 64 -- y[m,n] = bf16(rs[m] * sum_k X^[m,k] W^[n,k] + r[m,n]), X^ the in-kernel MXFP8 quantisation of row m,
// an optional fused SwiGLU epilogue -- in the tiling of sd_gemv_wide.hip.
//
// What they replace in the decode step of an MXFP8 model at 17 .. 64 rows: per projection the sd_mxfp8_quant launch and the
// 128-row sd_gemm_mxfp8 tile that such a batch fills to a half at most (HF modeling_qwen3.py:239-262, 81-83 through the
// reference's decode loop, soulxpodcast/engine/llm_engine.py:37-76).
//
// Shape of the kernel: gemv_mx_kernel with MT = ceil(M / 16) <= 4 B tiles.  The weights are the A operand of
// v_mfma_scale_f32_16x16x128_f8f6f4, two non-temporal 16-byte loads per lane and K-step and the real E8M0 byte as the scale
// operand, no LDS staging; the quantised rows of x are up to four 16-column B tiles multiplied against the same A fragment.
// Column m of a result depends on column m of its B tile only and row n on row n of A only.  Rows >= M of x are never read:
// their lanes form zero fragments and their statistic is never used.  Weight rows past N re-read row N - 1 and are never
// stored.
//
// Where the B fragments live: in registers, 9 per (tile, K-step of the wave) -- GT tiles at a time, GT = min(MT, 16 / KPW).
// For KPW <= 4 (K <= 4096) that is every tile and the kernel is one walk over the workgroup's weights.  For KPW = 8 (K >
// 4096; in the models the 1.7B down projection) four tiles would take 288 registers of the 256 a lane of a 512-thread
// workgroup has, so the tiles go in column groups of two: per group the wave quantises its fragments and walks the
// workgroup's steps again; the second walk's weights (about 16 x K bytes per unit) were read by this workgroup a few
// microseconds earlier.  TR, the weight tiles of a step, is capped by the registers the group leaves (launch()).
//
// Addresses: a wave walks a window of KPW consecutive K-steps that lies inside the row (kb below), so every load is a
// per-lane base plus a constant and no per-step offset or condition is kept in scalar registers (with a clamp per step
// the two-group instantiations spilled SGPRs).
//
// Summation order of one output element: sd_gemv_mx.hip's, statement for statement (the shared sd_gemv_mx.cuh) -- KPW from K
// alone; a wave's K-steps ascending through the accumulator operand, from 0; the KS waves through LDS in wave order; one
// rounding bf16(sum * rs + float(r)).  So any 16-row slice s of x gives sd_gemv_mxfp8_wide(x)[s] == sd_gemv_mxfp8(x[s]) bit
// for bit, both forms.  At most 32 KB of accumulator tiles pass through LDS per combine round, as in sd_gemv_wide.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sd_hip.h"
#include "sd_common.cuh"
#include "sd_prof.h"
#include "sd_runner.h"
#include "sd_gemv_mx.cuh"

#define ST ((hipStream_t)stream)

namespace {

constexpr int kRound = 4;  // accumulator tiles that pass through LDS together

constexpr int group_tiles(int mt, int kpw) { return mt * kpw <= 16 ? mt : 16 / kpw; }
// weight tiles per step that the registers next to a group's B fragments hold (accumulators TR * GT * 4, two weight
// sets 2 * TR * 8)
constexpr int max_tr(int mt, int kpw) { return group_tiles(mt, kpw) * kpw <= 8 ? 4 : 2; }

// MT: 16-row tiles of x; KPW: K-steps per wave; TR: 16-row weight tiles a wave takes per step (SwiGLU: TR / 2 gate tiles,
// each followed by its up tile)
template <int MT, int KPW, int TR, bool SWIGLU>
__global__ __launch_bounds__(512) void gemv_mx_wide_kernel(const GemvMxArgs a) {
  constexpr int GT = group_tiles(MT, KPW);   // B tiles held at once
  constexpr int NG = (MT + GT - 1) / GT;     // column groups
  constexpr int G = SWIGLU ? 2 : 1;          // weight tiles per unit
  constexpr int UPS = TR / G;                // units per step
  constexpr int NA = TR * GT;                // accumulator tiles of a step, in the order (unit, m-tile, gate / up)
  constexpr int RP = NA < kRound ? NA : kRound;
  constexpr int NR = (NA + RP - 1) / RP;
  static_assert(TR % G == 0 && RP % G == 0, "a gate / up pair stays in one round");
  static_assert(TR <= max_tr(MT, KPW), "the registers of a lane");
  __shared__ f32x4 red_s[kMaxWaves][RP][64];
  __shared__ float rstd_s[SD_GEMV_MX_WIDE_MAX_M];
  const int lane = lane_id(), wv = wave_id_uniform(), nw = a.KS;
  const int fr = lane & 15, fg = lane >> 4;
  const int K = a.K, M = a.M, nk = K >> 7, nblk = K >> 5;
  const int units = (a.N + 15) >> 4;
  const int u0 = blockIdx.x * a.upw, u1 = min(units, u0 + a.upw);
  const int nsteps = (u1 - u0 + UPS - 1) / UPS;
  if (nsteps <= 0) return;  // block-uniform (the grid leaves no workgroup without rows)

  // weight row behind (step t, tile j, fragment row fr); rows past the edge re-read the last row, never stored
  auto w_row = [&](int t, int j) {
    const int u = min(u0 + t * UPS + j / G, u1 - 1);
    const int c = min(u * 16 + fr, a.N - 1);
    return (SWIGLU && (j & 1)) ? a.N + c : c;
  };
  // This wave owns the K-steps k0 .. min(k0 + KPW, nk) - 1.  It walks the KPW consecutive K-steps kb + 0 .. KPW - 1 with kb =
  // min(k0, nk - KPW) (nk >= KPW by the KPW rule), so that every address is a base plus a constant and lies inside the row;
  // the steps below k0 -- the last wave's, when nk is no multiple of KPW -- belong to the wave before and are not
  // multiplied.  The multiplied steps are k0, k0 + 1, ... ascending, as in gemv_mx_kernel.
  const int k0 = wv * KPW, kb = min(k0, nk - KPW);
  const int skip = k0 - kb;  // steps i < skip of the window are not this wave's
  auto load = [&](i32x8(&wa)[TR], int (&sa)[TR], int t, int i) {
#pragma unroll
    for (int j = 0; j < TR; ++j) {
      const long row = w_row(t, j);
      const uint8_t* p = a.wq + row * K + kb * 128 + fg * 16 + i * 128;  // i: a constant offset of the load
      const u32x4 lo = __builtin_nontemporal_load((const u32x4*)p);
      const u32x4 hi = __builtin_nontemporal_load((const u32x4*)(p + 64));
      wa[j] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      sa[j] = (a.ws + row * nblk + kb * 4 + fg)[i * 4];
    }
  };
  // the raw values of K-step kb + i of row m (rows past M, K-steps that are not this wave's and the look-ahead past the
  // last one: a valid address, the values replaced by zeros in kstep_floats)
  auto load_x = [&](bf16x8(&raw)[4], int m, int i) {
    const bf16* p = a.x + (long)min(m, M - 1) * a.ldx + min(kb + i, nk - 1) * 128 + fg * 16;
    raw[0] = *(const bf16x8*)p; raw[1] = *(const bf16x8*)(p + 8);
    raw[2] = *(const bf16x8*)(p + 64); raw[3] = *(const bf16x8*)(p + 72);
  };

  // ---- the rows' RMSNorm statistic (published by the barrier in front of the first combine)
  row_rstd<SD_GEMV_MX_WIDE_MAX_M>(a.x, a.ldx, M, K, a.norm, a.eps, rstd_s, lane, wv, nw);

  const int tid = threadIdx.x, nthr = nw * 64;
#pragma unroll 1
  for (int g = 0; g < NG; ++g) {
    // two weight sets: unit u = (step u / KPW, K-step u % KPW) is multiplied while unit u + 1 is in flight; the sets
    // rotate by renaming in the unrolled loop below
    i32x8 w0[TR], w1[TR];
    int s0[TR], s1[TR];
    load(w0, s0, 0, 0);  // the first weights are on their way before x is touched

    // ---- this wave's K-steps of the group's rows as B fragments: lane (fr, fg) quantises bytes 16 fg .. and 64 + 16 fg ..
    // of row 16 q + fr (a rolled loop whose result is moved into its register set by selects, as in gemv_mx_kernel)
    i32x8 xq[GT][KPW];
    int xs[GT][KPW];
#pragma unroll
    for (int q = 0; q < GT; ++q) {
      const int m = (g * GT + q) * 16 + fr;
#pragma unroll
      for (int j = 0; j < KPW; ++j) { xq[q][j] = i32x8{0, 0, 0, 0, 0, 0, 0, 0}; xs[q][j] = 0; }
      bf16x8 raw[4], raw_next[4];
      load_x(raw, m, 0);
#pragma unroll 1
      for (int i = 0; i < KPW; ++i) {
        load_x(raw_next, m, i + 1);
        float lo[16], hi[16];
        kstep_floats(raw, m < M && i >= skip, lo, hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) raw[e] = raw_next[e];
        i32x8 qv;
        int sc;
        quant_kstep(lo, hi, fr, fg, qv, sc);
#pragma unroll
        for (int j = 0; j < KPW; ++j)
          if (j == i) { xq[q][j] = qv; xs[q][j] = sc; }
      }
    }

    for (int t = 0; t < nsteps; ++t) {
      f32x4 acc[TR][GT];
#pragma unroll
      for (int j = 0; j < TR; ++j)
#pragma unroll
        for (int q = 0; q < GT; ++q) acc[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KPW; ++i) {
        // the next unit's loads go out first (past the last step: the last step's again, so that the load stays
        // unconditional and the wait in front of the MFMAs counts loads)
        load(w1, s1, min(t + (i + 1) / KPW, nsteps - 1), (i + 1) % KPW);
        if (i >= skip) {  // wave-uniform
#pragma unroll
          for (int j = 0; j < TR; ++j)
#pragma unroll
            for (int q = 0; q < GT; ++q)
              acc[j][q] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w0[j], xq[q][i], acc[j][q], 0, 0, 0, s0[j], 0,
                                                                           xs[q][i]);
        }
#pragma unroll
        for (int j = 0; j < TR; ++j) { w0[j] = w1[j]; s0[j] = s1[j]; }
      }
      // ---- combine, RP accumulator tiles per round: entry (tile c of the round, lane slot l) = column m = 16 (g GT + q) +
      // (l & 15), rows 4 (l >> 4) + 0..3 of the weight tile
#pragma unroll
      for (int rd = 0; rd < NR; ++rd) {
#pragma unroll
        for (int c = 0; c < RP; ++c) {
          const int idx = rd * RP + c;
          if (idx < NA) red_s[wv][c][lane] = acc[(idx / (G * GT)) * G + idx % G][(idx / G) % GT];
        }
        __syncthreads();
        for (int e = tid; e < (RP / G) * 64; e += nthr) {
          const int c = (e >> 6) * G, l = e & 63;
          const int idx = rd * RP + c;
          if (idx >= NA) continue;
          const int q = (idx / G) % GT, u = u0 + t * UPS + idx / (G * GT);
          const int m = (g * GT + q) * 16 + (l & 15);
          if (m >= M || u >= u1) continue;
          const float rs = rstd_s[m];
          const int n0 = u * 16 + 4 * (l >> 4);
          if constexpr (!SWIGLU) {
            f32x4 sum = red_s[0][c][l];
            for (int s = 1; s < nw; ++s) sum += red_s[s][c][l];  // slice order: fixed
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int n = n0 + k;
              if (n < a.N) {
                const float v = a.r ? sum[k] * rs + (float)a.r[(long)m * a.ldr + n] : sum[k] * rs;
                a.y[(long)m * a.ldy + n] = (bf16)v;
              }
            }
          } else {
            f32x4 sg = red_s[0][c][l], su = red_s[0][c + 1][l];
            for (int s = 1; s < nw; ++s) { sg += red_s[s][c][l]; su += red_s[s][c + 1][l]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int n = n0 + k;
              if (n < a.N) {
                // gate and up as the bf16 projection stores them, then swiglu_fwd_kernel's expression
                const float gt = (float)(bf16)(sg[k] * rs), up = (float)(bf16)(su[k] * rs);
                a.y[(long)m * a.ldy + n] = (bf16)(gt / (1.f + __expf(-gt)) * up);
              }
            }
          }
        }
        // red_s is free again before the next sums land
        if (rd + 1 < NR || t + 1 < nsteps || g + 1 < NG) __syncthreads();
      }
    }
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
  grid_of(units, cus, SWIGLU, upw, ups);  // the grid of sd_gemv_mxfp8: from N and the CU count only
  a.upw = upw;
  // the units of a step, capped by the registers (M, K): 1, 2 and 4 divide one another, so upw stays a multiple
  const int mt = (a.M + 15) >> 4;
  int tr = SWIGLU ? 2 * ups : ups;
  if (tr > max_tr(mt, kpw)) tr = max_tr(mt, kpw);
  const unsigned grid = (unsigned)((units + upw - 1) / upw), block = (unsigned)(a.KS * 64);
  SdProfScope prof(SD_K_GEMM_NT, 2.0 * a.M * (SWIGLU ? 2.0 : 1.0) * a.N * a.K, ST);
  SD_PROF_LABEL("gemv_mx_wide_kernel<%d, %d, %d, %s>", mt, kpw, tr, SWIGLU ? "true" : "false");
#define SD_GO(MT_, KPW_, TR_) \
  hipLaunchKernelGGL((gemv_mx_wide_kernel<MT_, KPW_, TR_, SWIGLU>), dim3(grid), dim3(block), 0, ST, a)
#define SD_TR(MT_, KPW_)                                                   \
  do {                                                                     \
    if constexpr (max_tr(MT_, KPW_) >= 4) {                                \
      if (tr == 4) { SD_GO(MT_, KPW_, 4); break; }                         \
    }                                                                      \
    if (tr >= 2) SD_GO(MT_, KPW_, 2);                                      \
    else if constexpr (!SWIGLU) SD_GO(MT_, KPW_, 1);                       \
  } while (0)
#define SD_KPW(MT_)                          \
  switch (kpw) {                             \
    case 1: SD_TR(MT_, 1); break;            \
    case 2: SD_TR(MT_, 2); break;            \
    case 4: SD_TR(MT_, 4); break;            \
    default: SD_TR(MT_, 8); break;           \
  }
  switch (mt) {
    case 1: SD_KPW(1); break;
    case 2: SD_KPW(2); break;
    case 3: SD_KPW(3); break;
    default: SD_KPW(4); break;
  }
#undef SD_KPW
#undef SD_TR
#undef SD_GO
  SD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// the checks of the two entries without a launch (the wide MXFP8 decode step asks before it commits to the GEMV
// sequence); ldy = N and no residual stand for the SwiGLU form with N = I
int sd_gemv_mx_wide_check(const void* x, int64_t ldx, const void* w_q, const void* w_scale, const void* y, int64_t ldy,
                          const void* r, int64_t ldr, int M, int N, int K) {
  return validate(x, w_q, w_scale, y, r, M, N, K, ldx, ldy, ldr, SD_GEMV_MX_WIDE_MAX_M);
}

extern "C" int sd_gemv_mxfp8_wide(const void* x, int64_t ldx, const void* w_q, const void* w_scale, void* y, int64_t ldy,
                                  const void* r, int64_t ldr, int norm, float eps, int M, int N, int K, void* stream) {
  const int rc = sd_gemv_mx_wide_check(x, ldx, w_q, w_scale, y, ldy, r, ldr, M, N, K);
  if (rc) return rc;
  GemvMxArgs a = {};
  a.x = (const bf16*)x; a.wq = (const uint8_t*)w_q; a.ws = (const uint8_t*)w_scale; a.r = (const bf16*)r; a.y = (bf16*)y;
  a.eps = eps; a.norm = norm ? 1 : 0; a.M = M; a.N = N; a.K = K;
  a.ldx = ldx; a.ldy = ldy; a.ldr = ldr;
  return launch<false>(a, stream);
}

extern "C" int sd_gemv_mxfp8_wide_swiglu(const void* x, const void* wgu_q, const void* wgu_scale, void* act, int norm,
                                         float eps, int M, int I, int K, void* stream) {
  const int rc = sd_gemv_mx_wide_check(x, K, wgu_q, wgu_scale, act, I, nullptr, 0, M, I, K);
  if (rc) return rc;
  GemvMxArgs a = {};
  a.x = (const bf16*)x; a.wq = (const uint8_t*)wgu_q; a.ws = (const uint8_t*)wgu_scale; a.y = (bf16*)act;
  a.eps = eps; a.norm = norm ? 1 : 0; a.M = M; a.N = I; a.K = K;
  a.ldx = K; a.ldy = I; a.ldr = 0;
  return launch<true>(a, stream);
}
