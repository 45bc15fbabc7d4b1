// What the MFMA weight-streaming GEMVs of the decode step share (sd_gemv_mx.hip: MXFP8 weights, M <= 64; sd_gemv_wide.hip:
// bf16 weights, M <= 64): the walk of a workgroup over its 16-row units, the combine of the KS waves' accumulator tiles
// through LDS with its epilogue and write guards -- the block that decides what is written and where -- and the grid rule.
// Each kernel keeps what is its own: the operand format and its loads, the K-steps of a wave, where the rows of x live
// and the rows' RMSNorm.  Internal: not installed, not ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sd_hip.h"
#include "sd_common.cuh"

namespace {

constexpr int kMaxWaves = 8;   // K slices of a workgroup at most
constexpr int kRound = 4;      // accumulator tiles that pass through LDS together

// ---------------------------------------------------------------------------------------------- the work walk
// The 16-row units [u0, u1) of this workgroup, UPS units = UPS * G weight tiles per step (G = 2: a unit is a gate tile and
// the up tile of the same 16 columns).  N: weight rows of the plain form, columns of act of the SwiGLU form; upw: units
// per workgroup.  nsteps <= 0 never happens (the grid leaves no workgroup without rows) and is block-uniform.
template <int UPS, int G>
struct UnitWalk {
  int N, u0, u1, nsteps;
  SD_DEV UnitWalk(int N_, int upw) : N(N_) {
    const int units = (N + 15) >> 4;
    u0 = blockIdx.x * upw;
    u1 = min(units, u0 + upw);
    nsteps = (u1 - u0 + UPS - 1) / UPS;
  }
  // weight row behind (step t, tile j, fragment row fr); rows past the edge re-read the last row, never stored
  SD_DEV int w_row(int t, int j, int fr) const {
    const int u = min(u0 + t * UPS + j / G, u1 - 1);
    const int c = min(u * 16 + fr, N - 1);
    return (G == 2 && (j & 1)) ? N + c : c;
  }
};

// ---------------------------------------------------------------------------------------------- the combine
// accumulator tiles of a round, of the NA a step leaves
constexpr int round_tiles(int na) { return na < kRound ? na : kRound; }

// The accumulator tiles of a step as a wave holds them: TR weight tiles x BT B tiles.  A value type: combine_store takes
// its arguments by value -- handed over by reference, hipcc keeps the tiles of the wide MXFP8 kernel in a second register
// set and copies them in every step (20-30 v_mov per step on 14 instantiations).
template <int TR, int BT>
struct AccTiles {
  f32x4 t[TR][BT];
};

// The tiles acc of step t (taken in the order (unit, B tile, gate / up)) of the nw waves -> y, RP tiles per round: every
// wave stores its tiles to red_s, and after the barrier entry (tile c of the round, lane slot l) = column m = 16 (q0 + q) +
// (l & 15), rows 4 (l >> 4) + 0..3 of the weight tile is summed over the waves s = 0 .. nw - 1 ascending and stored once:
// bf16(sum [* rs] + float(r)), or swiglu_fwd_kernel's expression on the two sums rounded to bf16.  SCALED: the sum is
// multiplied by rstd_s[m] (the bf16 form has no such factor and forms no product).  q0: first B tile of those held;
// more_groups: another column group walks the steps again, so red_s must be free again even after the last step.  Args:
// y, r, ldy, ldr, M, N.  Columns m >= M, units >= u1 and rows n >= N are not stored.
template <int TR, int BT, bool SWIGLU, bool SCALED, class Args, class Walk>
SD_DEV void combine_store(const AccTiles<TR, BT> acc, const float* rstd_s, const Args a, const Walk wk, int t, int q0,
                          bool more_groups, int wv, int lane, int nw) {
  constexpr int G = SWIGLU ? 2 : 1, UPS = TR / G, NA = TR * BT, RP = round_tiles(NA), NR = (NA + RP - 1) / RP;
  static_assert(TR % G == 0 && RP % G == 0, "a gate / up pair stays in one round");
  __shared__ f32x4 red_s[kMaxWaves][RP][64];
  const int tid = threadIdx.x, nthr = nw * 64;
#pragma unroll
  for (int rd = 0; rd < NR; ++rd) {
#pragma unroll
    for (int c = 0; c < RP; ++c) {
      const int idx = rd * RP + c;
      if (idx < NA) red_s[wv][c][lane] = acc.t[(idx / (G * BT)) * G + idx % G][(idx / G) % BT];
    }
    __syncthreads();
    for (int e = tid; e < (RP / G) * 64; e += nthr) {
      const int c = (e >> 6) * G, l = e & 63;
      const int idx = rd * RP + c;
      if (idx >= NA) continue;
      const int q = (idx / G) % BT, u = wk.u0 + t * UPS + idx / (G * BT);
      const int m = (q0 + q) * 16 + (l & 15);
      if (m >= a.M || u >= wk.u1) continue;
      float rs = 0.f;
      if constexpr (SCALED) rs = rstd_s[m];
      const int n0 = u * 16 + 4 * (l >> 4);
      if constexpr (!SWIGLU) {
        f32x4 sum = red_s[0][c][l];
        for (int s = 1; s < nw; ++s) sum += red_s[s][c][l];  // slice order: fixed
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int n = n0 + k;
          if (n < a.N) {
            float v;
            if constexpr (SCALED) v = a.r ? sum[k] * rs + (float)a.r[(long)m * a.ldr + n] : sum[k] * rs;
            else v = a.r ? sum[k] + (float)a.r[(long)m * a.ldr + n] : sum[k];
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
            float g, up;
            if constexpr (SCALED) { g = (float)(bf16)(sg[k] * rs); up = (float)(bf16)(su[k] * rs); }
            else { g = (float)(bf16)sg[k]; up = (float)(bf16)su[k]; }
            a.y[(long)m * a.ldy + n] = (bf16)(g / (1.f + __expf(-g)) * up);
          }
        }
      }
    }
    if (rd + 1 < NR || t + 1 < wk.nsteps || more_groups) __syncthreads();  // red_s is free again before the next sums land
  }
}

// ---------------------------------------------------------------------------------------------- the grid
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

// grid: from N and the CU count only -- about two workgroups per CU while a workgroup keeps one 16-row unit; the units a
// wave takes per step (1, 2 or 4 tiles; 1 or 2 gate/up pairs) follow from what a workgroup got
inline void grid_of(int units, int cus, bool swiglu, int& upw, int& ups) {
  upw = (units + 2 * cus - 1) / (2 * cus);
  ups = swiglu ? (upw >= 2 ? 2 : 1) : (upw >= 4 ? 4 : upw >= 2 ? 2 : 1);
  upw = (upw + ups - 1) / ups * ups;
}

// that rule for a launch over N: units per workgroup, weight tiles per step, workgroups; false without a device
struct GemvGrid {
  int upw, tr;
  unsigned grid;
};
inline bool grid_for(int N, bool swiglu, GemvGrid& g) {
  const int cus = cu_count();
  if (cus <= 0) return false;
  const int units = (N + 15) >> 4;
  int ups;
  grid_of(units, cus, swiglu, g.upw, ups);
  g.tr = swiglu ? 2 * ups : ups;
  g.grid = (unsigned)((units + g.upw - 1) / g.upw);
  return true;
}

}  // namespace
