// Wide weight-streaming GEMV for the decode step on gfx950: y[M,N] = xn[M,K] . w[N,K]^T (+ r) for 1 <= M <= 64, bf16
// operands, with an optional fused RMSNorm of x and an optional fused SwiGLU epilogue.  The semantics of sd_gemv.hip; the
// form of sd_gemv_mx.hip, with which it shares the walk over a workgroup's units, the combine with its epilogue and the
// grid rule (sd_gemv_mfma.cuh).
//
// What they replace in the decode step (one token per sequence, M = batch): the projections of HF modeling_qwen3.py:239-262
// (q/k/v, o), :81-83 (the MLP) and the lm_head, with the RMSNorm of :59-64 fused in, reached through the reference's decode
// loop (soulxpodcast/engine/llm_engine.py:37-76) -- for batches the 16-row sd_gemv_bf16 refuses.
//
// Shape of the kernel: the MFMA form.  The weights are the A operand of v_mfma_f32_16x16x32_bf16 -- lane l = (fr = l & 15,
// fg = l >> 4) holds A[row fr][k = 8 fg .. 8 fg + 7] of a K-step of 32: 16 contiguous bytes of one weight row, ONE
// non-temporal 16-byte load straight into the operand registers -- and the rows of x are B (lane l: x[m = 16 q + fr][k = 8 fg
// ..] for the m-tile q), MT = ceil(M / 16) <= 4 tiles against the same A fragment.  C/D: lane holds column (l & 15), rows
// 4 (l >> 4) + 0..3.  Column m of a result depends on column m of B only and row n on row n of A only, so a row's bits do
// not know the batch around it.  No weight byte passes through LDS.
//
// K is cut into K-steps of 32; the KS <= 8 waves of a workgroup each own kpw consecutive K-steps (kpw: even, at least 4, the
// smallest that keeps KS <= 8 -- a function of K alone).  A workgroup walks its 16-row weight tiles TR at a time; a wave's
// unit of work is (step, K-step): TR A loads and MT B loads of 16 bytes per lane and TR x MT MFMAs, the next unit's loads
// issued ahead of the current unit's MFMAs.
//
// Where the rows of x live: nowhere -- the B fragments are re-read for every (step, K-step) from L2 (x is at most 1 MB and
// every workgroup of the launch reads it).  At M = 64, K = 6144 the rows are 786 KB: more than LDS, and a wave's eighth of
// them more than its registers.  Rows >= M are never read: their lanes form a zero fragment in registers.
//
// Fixed summation order of one output element (a function of K alone, never of M, N, the grid or the CU count):
//   1. inside a K-step: the instruction's own order over its 32 products;
//   2. a wave's K-steps: ascending, chained through the accumulator operand, from 0;
//   3. the KS waves: through LDS, s = 0 .. KS-1 ascending;
//   4. one rounding: bf16(sum + float(r)), or bf16(sum) without a residual.
// No atomics, no split of K across workgroups.  The bits are NOT those of sd_gemv_bf16 (another order).
//
// Fused RMSNorm: every workgroup computes the statistic of the M rows itself -- rmsnorm_fwd_kernel restated statement for
// statement (one wave per row, chunks of 512 ascending, wave_sum, rsqrtf(ss / H + eps)); a lane then forms
// bf16(g * (float)(bf16)(x * rstd)) for every B fragment it loads.  Fused SwiGLU: the gate tile and the up tile of the same
// 16 columns sit side by side in a step; both sums are rounded to bf16 and swiglu_fwd_kernel's expression follows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sd_hip.h"
#include "sd_common.cuh"
#include "sd_prof.h"
#include "sd_runner.h"
#include "sd_gemv_mfma.cuh"

#define ST ((hipStream_t)stream)

namespace {

struct WideArgs {
  const bf16 *x, *w, *r, *gain;
  bf16* y;
  float eps;
  int M, N, K;  // N: weight rows of the plain form; columns of act (= I) of the SwiGLU form
  long ldx, ldw, ldy, ldr;
  int KS;       // waves of the workgroup = K slices
  int kpw;      // K-steps per wave (even)
  int upw;      // 16-row units per workgroup (a multiple of the units per step): tiles, or gate/up tile pairs
};

SD_DEV bf16x8 zero8() {
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (bf16)0.f;
  return v;
}

// MT: 16-row tiles of x (B operands); TR: 16-row weight tiles a wave takes per step (SwiGLU: TR / 2 gate tiles, each
// followed by its up tile)
template <int MT, int TR, bool SWIGLU>
__global__ __launch_bounds__(512) void wide_gemv_kernel(const WideArgs a) {
  constexpr int G = SWIGLU ? 2 : 1;          // weight tiles per unit
  __shared__ float rstd_s[SD_GEMV_WIDE_MAX_M];
  const int lane = lane_id(), wv = wave_id_uniform(), nw = a.KS;
  const int fr = lane & 15, fg = lane >> 4;
  const int K = a.K, M = a.M, nk = K >> 5, kpw = a.kpw;
  const UnitWalk<TR / G, G> wk(a.N, a.upw);
  const int nsteps = wk.nsteps;
  if (nsteps <= 0) return;

  // Unit (step t, K-step i of this wave): TR weight fragments, the raw rows of x and -- with a norm -- the gains of the
  // K-step.  K-steps past the end re-read the last one (an address inside the row) and are not multiplied; columns m >= M
  // are not loaded at all.
  const int k0 = wv * kpw;
  const bool norm = a.gain != nullptr;
  auto load = [&](bf16x8(&wa)[TR], bf16x8(&xb)[MT], bf16x8& gv, int t, int i) {
    const int kc = min(k0 + i, nk - 1) * 32 + fg * 8;
#pragma unroll
    for (int j = 0; j < TR; ++j)
      wa[j] = __builtin_nontemporal_load((const bf16x8*)(a.w + (long)wk.w_row(t, j, fr) * a.ldw + kc));
#pragma unroll
    for (int q = 0; q < MT; ++q) {
      const int m = q * 16 + fr;
      xb[q] = zero8();
      if (m < M) xb[q] = *(const bf16x8*)(a.x + (long)m * a.ldx + kc);
    }
    if (norm) gv = *(const bf16x8*)(a.gain + kc);
  };
  bf16x8 wa0[TR], wa1[TR], xb0[MT], xb1[MT], g0 = zero8(), g1 = zero8();
  load(wa0, xb0, g0, 0, 0);  // the first weights are on their way before the statistic is formed

  // ---- fused RMSNorm: rmsnorm_fwd_kernel's statistic, one wave per row over the whole row (H = K <= 4096: 8 chunks)
  float rs[MT];
#pragma unroll
  for (int q = 0; q < MT; ++q) rs[q] = 0.f;
  if (norm) {
    for (int row = wv; row < M; row += nw) {
      const bf16* xr = a.x + (long)row * a.ldx;
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int c = lane * 8 + i * 512;
        if (c < K) {
          const bf16x8 v = *(const bf16x8*)(xr + c);
#pragma unroll
          for (int e = 0; e < 8; ++e) { const float f = (float)v[e]; ss += f * f; }
        }
      }
      ss = wave_sum(ss);
      const float rstd = rsqrtf(ss / (float)K + a.eps);
      if (lane == 0) rstd_s[row] = rstd;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MT; ++q) rs[q] = q * 16 + fr < M ? rstd_s[q * 16 + fr] : 0.f;  // columns >= M stay zero
  }

  AccTiles<TR, MT> acc;
  auto compute = [&](const bf16x8(&wa)[TR], const bf16x8(&xb)[MT], const bf16x8& gv, int i) {
    if (k0 + i >= nk) return;  // wave-uniform
    bf16x8 b[MT];
#pragma unroll
    for (int q = 0; q < MT; ++q) {
      b[q] = xb[q];
      if (norm) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          b[q][e] = (bf16)((float)gv[e] * (float)(bf16)((float)xb[q][e] * rs[q]));  // HF: weight * hidden.to(bf16)
      }
    }
#pragma unroll
    for (int j = 0; j < TR; ++j)
#pragma unroll
      for (int q = 0; q < MT; ++q) acc.t[j][q] = mfma16(wa[j], b[q], acc.t[j][q]);
  };

  for (int t = 0; t < nsteps; ++t) {
#pragma unroll
    for (int j = 0; j < TR; ++j)
#pragma unroll
      for (int q = 0; q < MT; ++q) acc.t[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K-steps in pairs (kpw is even): each unit's loads go out before the unit ahead of it is multiplied.  Past the last
    // step the first unit of the last step is loaded again, so that every load stays unconditional.
    for (int i = 0; i < kpw; i += 2) {
      load(wa1, xb1, g1, t, i + 1);
      compute(wa0, xb0, g0, i);
      const bool more = i + 2 < kpw;
      load(wa0, xb0, g0, more ? t : min(t + 1, nsteps - 1), more ? i + 2 : 0);
      compute(wa1, xb1, g1, i + 1);
    }
    combine_store<TR, MT, SWIGLU, false>(acc, nullptr, a, wk, t, 0, false, wv, lane, nw);
  }
}

// One entry: the checks, the arguments, the launch (N = ldy = I, ldx = ldw = K and no residual: the SwiGLU form)
template <bool SWIGLU>
int run(const void* x, const void* w, void* y, const void* r, const void* norm_gain, float eps, int M, int N, int K,
        int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, void* stream) {
  const int rc = sd_gemv_wide_check(x, w, y, r, norm_gain, M, N, K, ldx, ldw, ldy, ldr);
  if (rc) return rc;
  const int nk = K >> 5;
  int kpw = (nk + kMaxWaves - 1) / kMaxWaves;  // from K alone: it fixes the summation order
  kpw = (kpw + 1) & ~1;
  if (kpw < 4) kpw = 4;
  GemvGrid g;
  if (!grid_for(N, SWIGLU, g)) return SD_ERR_WORKSPACE;  // from N and the CU count only
  const WideArgs a = {(const bf16*)x, (const bf16*)w, (const bf16*)r, (const bf16*)norm_gain, (bf16*)y, eps, M, N, K,
                      ldx, ldw, ldy, ldr, (nk + kpw - 1) / kpw, kpw, g.upw};
  const int tr = g.tr, mt = (M + 15) >> 4;
  const unsigned grid = g.grid, block = (unsigned)(a.KS * 64);
  SdProfScope prof(SD_K_GEMM_NT, 2.0 * M * (SWIGLU ? 2.0 : 1.0) * N * K, ST);
  SD_PROF_LABEL("wide_gemv_kernel<%d, %d, %s>", mt, tr, SWIGLU ? "true" : "false");
#define SD_GO(MT_, TR_) hipLaunchKernelGGL((wide_gemv_kernel<MT_, TR_, SWIGLU>), dim3(grid), dim3(block), 0, ST, a)
#define SD_TR(MT_)                                          \
  do {                                                      \
    if (tr == 4) SD_GO(MT_, 4);                             \
    else if (tr == 2) SD_GO(MT_, 2);                        \
    else if constexpr (!SWIGLU) SD_GO(MT_, 1);              \
  } while (0)
  switch (mt) {
    case 1: SD_TR(1); break;
    case 2: SD_TR(2); break;
    case 3: SD_TR(3); break;
    default: SD_TR(4); break;
  }
#undef SD_TR
#undef SD_GO
  SD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sd_gemv_wide_bf16(const void* x, const void* w, void* y, const void* r, const void* norm_gain, float eps,
                                 int M, int N, int K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, void* stream) {
  return run<false>(x, w, y, r, norm_gain, eps, M, N, K, ldx, ldw, ldy, ldr, stream);
}

extern "C" int sd_gemv_wide_swiglu(const void* x, const void* wgu, void* act, const void* norm_gain, float eps, int M, int I,
                                   int K, void* stream) {
  return run<true>(x, wgu, act, nullptr, norm_gain, eps, M, I, K, K, K, I, 0, stream);
}
