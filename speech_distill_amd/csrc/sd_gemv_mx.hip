// Weight-streaming GEMV over MXFP8 weights for the decode step on gfx950: y[M,N] = rs[m] * (X^[M,K] . W^[N,K]^T) (+ r) for
// 1 <= M <= 64, W = e4m3fn bytes [N,K] + E8M0 scale bytes [N,K/32] exactly as sd_mxfp8_quant leaves a weight, X^ = the
// MXFP8 quantisation of the bf16 rows of x, made inside the kernel (the bytes and scale bytes of mx_quant32, sd_mx.hip),
// rs[m] = 1 or the row's RMSNorm statistic (sd_mxfp8_quant's rstd).  An optional fused SwiGLU epilogue.  Two kernels:
// gemv_mx_kernel behind the 16-row entries (sd_gemv_mxfp8, sd_gemv_mxfp8_swiglu: M <= 16, one B tile) and
// gemv_mx_wide_kernel behind the wide ones (sd_gemv_mxfp8_wide, sd_gemv_mxfp8_wide_swiglu: M <= 64, up to four).  They
// share the arguments, the quantiser of a K-step of x, the rows' statistic, the checks, the KPW rule and the launch below;
// the walk over a workgroup's units, the combine with its epilogue and the grid rule are in sd_gemv_mfma.cuh, shared with
// the bf16 kernel of sd_gemv_wide.hip.  What the two kernels own themselves is how a wave addresses its K-steps (a clamp
// per step; a window base) and how many B tiles it holds: the wide kernel at one B tile is the same arithmetic, but on the
// 0.6B shapes it measured 1-3 % slower than the 16-row kernel, so both stay.
//
// What they replace in the decode step of an MXFP8 model (one token per sequence, M = batch): per projection the
// sd_mxfp8_quant launch and the 128-row sd_gemm_mxfp8 tile that a batch of <= 64 rows fills to a half at most (HF
// modeling_qwen3.py:239-262, 81-83 through the reference's decode loop, soulxpodcast/engine/llm_engine.py:37-76).
//
// Shape of the kernel: the MFMA form.  The weights are the A operand of v_mfma_scale_f32_16x16x128_f8f6f4 -- one
// instruction takes 16 weight rows x 128 bytes of K with their real E8M0 bytes as the scale operand -- and the quantised
// rows of x are MT = ceil(M / 16) <= 4 B tiles of 16 columns, zero-padded, multiplied against the same A fragment.  Column
// m of a result depends on column m of its B tile only and row n on row n of A only.  Lane maps (sd_mx.hip header,
// DESIGN.md section 10): lane l = (r = l & 15, g = l >> 4) holds, for A, bytes k = 16g .. 16g+15 and k = 64+16g .. of row r
// of the K-step -- two 16-byte runs, contiguous in the weight row, each ONE non-temporal 16-byte load straight into the
// operand registers -- and the scale byte of (row r, block g); C/D: lane holds column (l & 15), rows 4 * (l >> 4) + 0..3.
// No weight byte passes through LDS.  Rows >= M of x are never read: their lanes form zero fragments and their statistic
// is never used.  Weight rows past N re-read row N - 1 and are never stored.
//
// K is cut into K-steps of 128; the KS = ceil(nk / KPW) <= 8 waves of a workgroup each own KPW in {1, 2, 4, 8} consecutive
// K-steps (KPW: the smallest that keeps KS <= 8, so it is a function of K alone).  A wave quantises its slices of the rows
// of x once (the two lanes that share a 32-block exchange their amax by one xor-16 shuffle) and keeps them as B fragments
// in registers.  A workgroup walks its 16-row weight tiles TR at a time; a wave's unit of work is (step, K-step): TR x 2
// loads of 16 bytes and TR scale bytes per lane, the next unit's loads issued ahead of the current unit's MFMAs.
//
// Where the B fragments live: in registers, 9 per (tile, K-step of the wave) -- GT tiles at a time, GT = min(MT, 16 / KPW).
// For KPW <= 4 (K <= 4096) that is every tile and the kernel is one walk over the workgroup's weights.  For KPW = 8 (K >
// 4096; in the models the 1.7B down projection) four tiles would take 288 registers of the 256 a lane of a 512-thread
// workgroup has, so the tiles go in column groups of two: per group the wave quantises its fragments and walks the
// workgroup's steps again; the second walk's weights (about 16 x K bytes per unit) were read by this workgroup a few
// microseconds earlier.  TR, the weight tiles of a step, is capped by the registers the group leaves (max_tr).
//
// Addresses of the wide kernel: a wave walks a window of KPW consecutive K-steps that lies inside the row (kb below), so every load is a
// per-lane base plus a constant and no per-step offset or condition is kept in scalar registers (with a clamp per step
// the two-group instantiations spilled SGPRs).
//
// Fixed summation order of one output element (a function of K alone, never of M, N, the grid or the CU count):
//   1. inside a K-step: the instruction's own order over its 128 products (every product is exact in fp32);
//   2. a wave's K-steps: ascending, chained through the accumulator operand, from 0;
//   3. the KS waves: through LDS, s = 0 .. KS-1 ascending;
//   4. bf16(sum * rs + float(r)) -- the epilogue expression of gemm_mx_kernel.
// No atomics.  So any 16-row slice s of x gives sd_gemv_mxfp8_wide(x)[s] == sd_gemv_mxfp8(x[s]) bit for bit, both forms.
// Fused SwiGLU: gate tile and up tile of the same 16 columns sit side by side in a step; both sums are rounded to bf16
// after the row scale (as gemm_mx_kernel's EPI_SWIGLU does) and swiglu_fwd_kernel's expression follows.  At most 32 KB of
// accumulator tiles pass through LDS per combine round.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sd_hip.h"
#include "sd_common.cuh"
#include "sd_prof.h"
#include "sd_runner.h"
#include "sd_gemv_mfma.cuh"

#define ST ((hipStream_t)stream)

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

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

// ------------------------------------------------------------------------------------------ M <= 16: one B tile
// KPW: K-steps per wave; TR: 16-row weight tiles a wave takes per step (SwiGLU: TR / 2 gate tiles, each followed by its
// up tile).  A wave addresses K-step i of its own as min(k0 + i, nk - 1): a clamp per step.
template <int KPW, int TR, bool SWIGLU>
__global__ __launch_bounds__(512) void gemv_mx_kernel(const GemvMxArgs a) {
  constexpr int G = SWIGLU ? 2 : 1;  // weight tiles per unit
  __shared__ float rstd_s[16];
  const int lane = lane_id(), wv = wave_id_uniform(), nw = a.KS;
  const int fr = lane & 15, fg = lane >> 4;
  const int K = a.K, M = a.M, nk = K >> 7, nblk = K >> 5;
  const UnitWalk<TR / G, G> wk(a.N, a.upw);
  const int nsteps = wk.nsteps;
  if (nsteps <= 0) return;

  // K-step i of this wave; steps past the end re-read the last one (an address inside the row) and are not multiplied
  const int k0 = wv * KPW;
  auto load = [&](i32x8(&wa)[TR], int (&sa)[TR], int t, int i) {
    const int ks = min(k0 + i, nk - 1);
#pragma unroll
    for (int j = 0; j < TR; ++j) {
      const long row = wk.w_row(t, j, fr);
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
  row_rstd<16>(a.x, a.ldx, M, K, a.norm, a.eps, rstd_s, lane, wv, nw);

  for (int t = 0; t < nsteps; ++t) {
    AccTiles<TR, 1> acc;
#pragma unroll
    for (int j = 0; j < TR; ++j) acc.t[j][0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
      // the loads of the unit D ahead go out first (past the last step: the last step's again, so that the load stays
      // unconditional and the wait in front of the MFMAs counts loads)
      load(wq_[D], sq_[D], min(t + (i + D) / KPW, nsteps - 1), (i + D) % KPW);
      if (k0 + i < nk) {  // wave-uniform
#pragma unroll
        for (int j = 0; j < TR; ++j)
          acc.t[j][0] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wq_[0][j], xq[i], acc.t[j][0], 0, 0, 0, sq_[0][j], 0,
                                                                       xs[i]);
      }
#pragma unroll
      for (int d = 0; d < D; ++d)
#pragma unroll
        for (int j = 0; j < TR; ++j) { wq_[d][j] = wq_[d + 1][j]; sq_[d][j] = sq_[d + 1][j]; }
    }
    combine_store<TR, 1, SWIGLU, true>(acc, rstd_s, a, wk, t, 0, false, wv, lane, nw);
  }
}

// ------------------------------------------------------------------------------------------ M <= 64: up to four B tiles
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
  static_assert(TR <= max_tr(MT, KPW), "the registers of a lane");
  __shared__ float rstd_s[MT * 16];
  const int lane = lane_id(), wv = wave_id_uniform(), nw = a.KS;
  const int fr = lane & 15, fg = lane >> 4;
  const int K = a.K, M = a.M, nk = K >> 7, nblk = K >> 5;
  const UnitWalk<TR / G, G> wk(a.N, a.upw);
  const int nsteps = wk.nsteps;
  if (nsteps <= 0) return;

  // This wave owns the K-steps k0 .. min(k0 + KPW, nk) - 1.  It walks the KPW consecutive K-steps kb + 0 .. KPW - 1 with kb =
  // min(k0, nk - KPW) (nk >= KPW by the KPW rule), so that every address is a base plus a constant and lies inside the row;
  // the steps below k0 -- the last wave's, when nk is no multiple of KPW -- belong to the wave before and are not
  // multiplied.  The multiplied steps are k0, k0 + 1, ... ascending.
  const int k0 = wv * KPW, kb = min(k0, nk - KPW);
  const int skip = k0 - kb;  // steps i < skip of the window are not this wave's
  auto load = [&](i32x8(&wa)[TR], int (&sa)[TR], int t, int i) {
#pragma unroll
    for (int j = 0; j < TR; ++j) {
      const long row = wk.w_row(t, j, fr);
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
  row_rstd<MT * 16>(a.x, a.ldx, M, K, a.norm, a.eps, rstd_s, lane, wv, nw);

#pragma unroll 1
  for (int g = 0; g < NG; ++g) {
    // two weight sets: unit u = (step u / KPW, K-step u % KPW) is multiplied while unit u + 1 is in flight; the sets
    // rotate by renaming in the unrolled loop below
    i32x8 w0[TR], w1[TR];
    int s0[TR], s1[TR];
    load(w0, s0, 0, 0);  // the first weights are on their way before x is touched

    // ---- this wave's K-steps of the group's rows as B fragments: lane (fr, fg) quantises bytes 16 fg .. and 64 + 16 fg ..
    // of row 16 q + fr (a rolled loop whose result is moved into its register set by selects: unrolled, hipcc keeps the 32
    // floats of every K-step live at once)
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
      AccTiles<TR, GT> acc;
#pragma unroll
      for (int j = 0; j < TR; ++j)
#pragma unroll
        for (int q = 0; q < GT; ++q) acc.t[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
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
              acc.t[j][q] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w0[j], xq[q][i], acc.t[j][q], 0, 0, 0, s0[j], 0,
                                                                           xs[q][i]);
        }
#pragma unroll
        for (int j = 0; j < TR; ++j) { w0[j] = w1[j]; s0[j] = s1[j]; }
      }
      combine_store<TR, GT, SWIGLU, true>(acc, rstd_s, a, wk, t, g * GT, g + 1 < NG, wv, lane, nw);
    }
  }
}

// the checks of the four entries; max_m: SD_GEMV_MAX_M or SD_GEMV_MX_WIDE_MAX_M
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

// One entry: the checks, the arguments, the launch.  WIDE: the wide entries (M <= SD_GEMV_MX_WIDE_MAX_M, gemv_mx_wide_kernel
// at every M); otherwise the 16-row entries (M <= SD_GEMV_MAX_M, gemv_mx_kernel).  The profiler label names the kernel.
template <bool SWIGLU, bool WIDE>
int run(const void* x, int64_t ldx, const void* w_q, const void* w_scale, void* y, int64_t ldy, const void* r, int64_t ldr,
        int norm, float eps, int M, int N, int K, void* stream) {
  const int rc = validate(x, w_q, w_scale, y, r, M, N, K, ldx, ldy, ldr, WIDE ? SD_GEMV_MX_WIDE_MAX_M : SD_GEMV_MAX_M);
  if (rc) return rc;
  const int nk = K >> 7, kpw = kpw_of(nk), mt = (M + 15) >> 4;
  GemvGrid g;
  if (!grid_for(N, SWIGLU, g)) return SD_ERR_WORKSPACE;  // from N and the CU count only
  const GemvMxArgs a = {(const bf16*)x, (const uint8_t*)w_q, (const uint8_t*)w_scale, (const bf16*)r, (bf16*)y, eps,
                        norm ? 1 : 0, M, N, K, ldx, ldy, ldr, (nk + kpw - 1) / kpw, g.upw};
  // the units of a step, capped by the registers (M, K; never at one B tile): 1, 2 and 4 divide one another, so upw stays
  // a multiple
  const int tr = g.tr > max_tr(mt, kpw) ? max_tr(mt, kpw) : g.tr;
  const unsigned grid = g.grid, block = (unsigned)(a.KS * 64);
  SdProfScope prof(SD_K_GEMM_NT, 2.0 * M * (SWIGLU ? 2.0 : 1.0) * N * K, ST);
  if constexpr (WIDE) SD_PROF_LABEL("gemv_mx_wide_kernel<%d, %d, %d, %s>", mt, kpw, tr, SWIGLU ? "true" : "false");
  else SD_PROF_LABEL("gemv_mx_kernel<%d, %d, %s>", kpw, tr, SWIGLU ? "true" : "false");
#define SD_GO(MT_, KPW_, TR_)                                                                                         \
  do {                                                                                                                \
    if constexpr (WIDE)                                                                                               \
      hipLaunchKernelGGL((gemv_mx_wide_kernel<MT_, KPW_, TR_, SWIGLU>), dim3(grid), dim3(block), 0, ST, a);           \
    else                                                                                                              \
      hipLaunchKernelGGL((gemv_mx_kernel<KPW_, TR_, SWIGLU>), dim3(grid), dim3(block), 0, ST, a);                     \
  } while (0)
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
  if constexpr (!WIDE) {
    SD_KPW(1);
  } else {
    switch (mt) {
      case 1: SD_KPW(1); break;
      case 2: SD_KPW(2); break;
      case 3: SD_KPW(3); break;
      default: SD_KPW(4); break;
    }
  }
#undef SD_KPW
#undef SD_TR
#undef SD_GO
  SD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// the checks of the entries without a launch (the MXFP8 decode steps ask before they commit to the GEMV sequence); ldy = N
// and no residual stand for the SwiGLU form with N = I
int sd_gemv_mx_check(const void* x, int64_t ldx, const void* w_q, const void* w_scale, const void* y, int64_t ldy,
                     const void* r, int64_t ldr, int M, int N, int K) {
  return validate(x, w_q, w_scale, y, r, M, N, K, ldx, ldy, ldr, SD_GEMV_MAX_M);
}
int sd_gemv_mx_wide_check(const void* x, int64_t ldx, const void* w_q, const void* w_scale, const void* y, int64_t ldy,
                          const void* r, int64_t ldr, int M, int N, int K) {
  return validate(x, w_q, w_scale, y, r, M, N, K, ldx, ldy, ldr, SD_GEMV_MX_WIDE_MAX_M);
}

extern "C" int sd_gemv_mxfp8(const void* x, int64_t ldx, const void* w_q, const void* w_scale, void* y, int64_t ldy,
                             const void* r, int64_t ldr, int norm, float eps, int M, int N, int K, void* stream) {
  return run<false, false>(x, ldx, w_q, w_scale, y, ldy, r, ldr, norm, eps, M, N, K, stream);
}

extern "C" int sd_gemv_mxfp8_swiglu(const void* x, const void* wgu_q, const void* wgu_scale, void* act, int norm, float eps,
                                    int M, int I, int K, void* stream) {
  return run<true, false>(x, K, wgu_q, wgu_scale, act, I, nullptr, 0, norm, eps, M, I, K, stream);
}

extern "C" int sd_gemv_mxfp8_wide(const void* x, int64_t ldx, const void* w_q, const void* w_scale, void* y, int64_t ldy,
                                  const void* r, int64_t ldr, int norm, float eps, int M, int N, int K, void* stream) {
  return run<false, true>(x, ldx, w_q, w_scale, y, ldy, r, ldr, norm, eps, M, N, K, stream);
}

extern "C" int sd_gemv_mxfp8_wide_swiglu(const void* x, const void* wgu_q, const void* wgu_scale, void* act, int norm,
                                         float eps, int M, int I, int K, void* stream) {
  return run<true, true>(x, K, wgu_q, wgu_scale, act, I, nullptr, 0, norm, eps, M, I, K, stream);
}
