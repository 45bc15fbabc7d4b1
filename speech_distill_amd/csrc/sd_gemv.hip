// Weight-streaming GEMV kernels for the decode step on gfx950: y[M,N] = xn[M,K] . w[N,K]^T (+ r) for 1 <= M <= 16, with
// an optional fused RMSNorm of x and an optional fused SwiGLU epilogue.
//
// What they replace in the decode step (one token per sequence, M = batch):
//   modeling_qwen3.py:59-64 .... RMSNorm (input_layernorm, post_attention_layernorm, the final norm)
//   modeling_qwen3.py:239-259 .. q/k/v projections, :262 o projection (+ the residual add of :304-323)
//   modeling_qwen3.py:81-83 .... the MLP: down(silu(gate(x)) * up(x))
//   modeling_qwen3.py lm_head .. logits of the last hidden state
// all of which the reference reaches through its decode loop (soulxpodcast/engine/llm_engine.py:37-76).
//
// Shape of the kernel.  K is cut into chunks of 512 columns, one 16-byte piece per lane (c = lane*8 + chunk*512, the lane
// layout of rmsnorm_fwd_kernel).  KS = min(ceil(K/512), 8) waves share one weight row: wave s owns the chunks s, s + KS
// (CH = 1 chunk up to K = 4096, 2 up to 8192); RW = ceil(4 / KS) such groups walk different rows.  A lane keeps its chunks of all M rows of x in registers (packed bf16) for
// the whole kernel and walks the weight rows of its workgroup, RS rows per wave and step (RS = 4; 2 where M > 8 meets
// K > 4096, to stay inside the register file): every weight byte is loaded once, 16 bytes per lane,
// non-temporal, straight into registers, the loads of the next step issued before the current step is consumed.
// No weight passes through LDS.
//
// Fixed reduction order of one output element (it depends on K alone, never on M, N, the grid or the CU count):
//   1. lane partial: fp32 accumulator from 0, chunk by chunk (ascending), four v_dot2c_f32_bf16 per chunk (pairs ascending);
//   2. the 64 lanes: the xor butterfly 32, 16, 8, 4, 2, 1 (the pairing of wave_sum);
//   3. the KS waves: through LDS, s = 0 .. KS-1 ascending;
//   4. one rounding: bf16(sum + float(r)), or bf16(sum) without a residual.
// The M bucket (1, 2, 4, 8, 16) only sets how many rows a lane carries; a row's arithmetic is the same code in each.
//
// Fused RMSNorm: every workgroup normalises the M rows itself -- rmsnorm_fwd_kernel restated statement for statement (one
// wave per row for the statistic, chunks ascending, wave_sum, rsqrtf(ss / H + eps)); each lane then forms
// bf16(g * (float)(bf16)(x * rstd)) for the chunks it keeps.  Fused SwiGLU: the gate row and the up row of a column sit in
// the same wave; both sums are rounded to bf16 (as HF's bf16 projections are) and swiglu_fwd_kernel's expression follows.
#include <stdlib.h>
#include "sd_common.cuh"
#include "../../include/sd_hip.h"
#include "sd_prof.h"
#include "sd_runner.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int kMaxWaves = 8;     // K slices of a workgroup at most (K <= 8 * 2 * 512)
constexpr int kMaxK = 8192;
constexpr int kMaxNormK = 4096;  // the limit of sd_rmsnorm_fwd

struct GemvArgs {
  const bf16 *x, *w, *r, *gain;
  bf16* y;
  float eps;
  int M, N, K;  // N: weight rows walked (2I in the SwiGLU form, gate and up rows interleaved: 2 col, 2 col + 1)
  int I;        // SwiGLU: columns of act; gate rows [0,I), up rows [I,2I) of w
  long ldx, ldw, ldy, ldr;
  int KS, RW;   // K slices x row groups = waves of the workgroup
  int rpw;      // weight rows per workgroup (even)
};

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
// 8 products into one fp32 accumulator: v_dot2c_f32_bf16 on the pairs (0,1) (2,3) (4,5) (6,7), in that order
SD_DEV float dot8(bf16x8 x, bf16x8 w, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(x, x, 0, 1), __builtin_shufflevector(w, w, 0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(x, x, 2, 3), __builtin_shufflevector(w, w, 2, 3), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(x, x, 4, 5), __builtin_shufflevector(w, w, 4, 5), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(x, x, 6, 7), __builtin_shufflevector(w, w, 6, 7), acc, false);
  return acc;
}

// Sums NV values per lane over the 64 lanes with the pairing of wave_sum (xor 32, 16, .. 1).  While more than one value
// is left, a step also halves the set: the lane whose bit is clear keeps the lower half, its partner the upper half, and
// each adds what the other sends -- a + b either way, so every total is the butterfly's, bit for bit.  Value idx ends in
// the lanes with lane >> (6 - log2 NV) == idx, in v[0].
template <int NV, int N, int O>
SD_DEV void wave_sum_step(float (&v)[NV], int lane) {
  if constexpr (O > 0) {
    if constexpr (N > 1) {
      const bool up = lane & O;
#pragma unroll
      for (int i = 0; i < N / 2; ++i) {
        const float keep = up ? v[i + N / 2] : v[i];
        const float send = up ? v[i] : v[i + N / 2];
        v[i] = keep + __shfl_xor(send, O, 64);
      }
      wave_sum_step<NV, N / 2, O / 2>(v, lane);
    } else {
      v[0] += __shfl_xor(v[0], O, 64);
      wave_sum_step<NV, 1, O / 2>(v, lane);
    }
  }
}
template <int NV>
SD_DEV void wave_sum_many(float (&v)[NV]) {
  wave_sum_step<NV, NV, 32>(v, lane_id());
}
constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x >> 1); }

template <int MB, int CH, bool SWIGLU>
__global__ __launch_bounds__(512) void gemv_kernel(const GemvArgs a) {
  constexpr int RS = (MB * CH >= 32) ? 2 : 4;  // weight rows a wave takes per step
  constexpr int NV = RS * MB;
  static_assert(NV <= 64, "one value per lane at most");
  __shared__ float red_s[2][kMaxWaves][NV];
  __shared__ float rstd_s[16];
  const int lane = lane_id(), wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int KS = a.KS, RW = a.RW, K = a.K, M = a.M;
  const int s = wv % KS, rw = wv / KS;

  // ---- the weight rows [n0, n1) of this workgroup, RW * RS per step
  const int n0 = blockIdx.x * a.rpw;
  const int n1 = min(a.N, n0 + a.rpw);
  const int step_rows = RW * RS;
  const int nsteps = (n1 - n0 + step_rows - 1) / step_rows;
  if (nsteps <= 0) return;  // block-uniform (the grid leaves no workgroup without rows)

  // This lane's columns.  A chunk past K is read at the row's last 8 columns instead (an address inside the row) and
  // meets zeros in x, so that every load below is unconditional: the waits then count loads, they do not drain them.
  int col[CH], lcol[CH];
  bool cok[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    col[i] = lane * 8 + (s + i * KS) * 512;
    cok[i] = col[i] < K;
    lcol[i] = cok[i] ? col[i] : K - 8;
  }
  // rows past n1 re-read row n1 - 1; their sums are never stored
  auto load = [&](bf16x8(&wq)[RS][CH], int t) {
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
      for (int j = 0; j < RS; ++j) {
        const int v = min(n0 + (t * RW + rw) * RS + j, n1 - 1);
        const int row = SWIGLU ? ((v & 1) ? a.I + (v >> 1) : (v >> 1)) : v;
        wq[j][i] = __builtin_nontemporal_load((const bf16x8*)(a.w + (long)row * a.ldw + lcol[i]));
      }
  };
  bf16x8 wa[RS][CH], wb[RS][CH];
  load(wa, 0);  // the first weights are on their way before x is touched

  // ---- this lane's chunks of the M rows of x, packed bf16, for the whole kernel
  bf16x8 xq[MB][CH];
#pragma unroll
  for (int i = 0; i < CH; ++i)
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      xq[m][i] = zero8();
      if (m < M) xq[m][i] = *(const bf16x8*)(a.x + (long)m * a.ldx + lcol[i]);
    }

  // ---- fused RMSNorm.  The statistic is rmsnorm_fwd_kernel's, one wave per row over the whole row (H = K, up to 8
  // chunks): wave wv takes the rows wv, wv + nw, ..  All their loads are issued first; the sums then run chunk by chunk.
  // (CH = 2 means K > 4096, where the entries refuse a norm: no code for it there.)
  if (CH == 1 && a.gain) {
    constexpr int JMAX = (MB + 3) / 4;  // nw >= 4
    bf16x8 sv[JMAX][8];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      const int row = wv + j * nw;
      if (row < M) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i * 512 < K) {
            const int c = lane * 8 + i * 512;
            sv[j][i] = *(const bf16x8*)(a.x + (long)row * a.ldx + (c < K ? c : K - 8));
          }
      }
    }
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      const int row = wv + j * nw;
      if (row < M) {
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int c = lane * 8 + i * 512;
          if (c < K) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float f = (float)sv[j][i][e]; ss += f * f; }
          }
        }
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss / (float)K + a.eps);
        if (lane == 0) rstd_s[row] = rstd;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      float g[8];
      unpack8(*(const bf16x8*)(a.gain + lcol[i]), g);
#pragma unroll
      for (int m = 0; m < MB; ++m)
        if (m < M) {
          const float rstd = rstd_s[m];
          float f[8];
          unpack8(xq[m][i], f);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = g[e] * (float)(bf16)(f[e] * rstd);  // HF: weight * hidden.to(bf16)
          xq[m][i] = pack8(f);
        }
    }
  }
#pragma unroll
  for (int i = 0; i < CH; ++i)
    if (!cok[i]) {
#pragma unroll
      for (int m = 0; m < MB; ++m) xq[m][i] = zero8();
    }

  // the residual element this thread adds in step t's combine, loaded AHEAD of the next step's weights: the counter of
  // outstanding loads retires in order, so a residual load issued behind them would wait for all of them
  auto load_r = [&](int t) {
    float rv = 0.f;
    if constexpr (!SWIGLU) {
      const int tid = threadIdx.x;
      const int m = tid / step_rows, n = n0 + t * step_rows + tid % step_rows;
      if (a.r && tid < step_rows * MB && m < M && n < n1) rv = (float)a.r[(long)m * a.ldr + n];
    }
    return rv;
  };

  auto body = [&](const bf16x8(&wq)[RS][CH], int t, float rv) {
    float acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
      for (int j = 0; j < RS; ++j)
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[j * MB + m] = dot8(xq[m][i], wq[j][i], acc[j * MB + m]);
    wave_sum_many<NV>(acc);
    constexpr int SH = 6 - ilog2(NV);
    float(&red)[kMaxWaves][NV] = red_s[t & 1];
    if ((lane & ((1 << SH) - 1)) == 0) red[wv][lane >> SH] = acc[0];
    __syncthreads();  // one barrier per step: the two halves of red_s alternate
    const int base = n0 + t * step_rows;
    const int tid = threadIdx.x;
    if constexpr (!SWIGLU) {
      if (tid < step_rows * MB) {
        const int m = tid / step_rows, q = tid % step_rows;
        const int g = q / RS, j = q % RS;
        float sum = red[g * KS][j * MB + m];
        for (int k = 1; k < KS; ++k) sum += red[g * KS + k][j * MB + m];  // slice order: fixed
        const int n = base + q;
        if (m < M && n < n1) {
          if (a.r) sum += rv;
          a.y[(long)m * a.ldy + n] = (bf16)sum;
        }
      }
    } else {
      constexpr int RC = RS / 2;  // columns a wave takes per step
      const int step_cols = RW * RC;
      if (tid < step_cols * MB) {
        const int m = tid / step_cols, q = tid % step_cols;
        const int g = q / RC, jc = q % RC;
        float sg = red[g * KS][(2 * jc) * MB + m], su = red[g * KS][(2 * jc + 1) * MB + m];
        for (int k = 1; k < KS; ++k) {
          sg += red[g * KS + k][(2 * jc) * MB + m];
          su += red[g * KS + k][(2 * jc + 1) * MB + m];
        }
        const int c = (base >> 1) + q;
        if (m < M && 2 * c < n1) {
          // gate and up as the bf16 GEMV stores them, then swiglu_fwd_kernel's expression
          const float gt = (float)(bf16)sg, up = (float)(bf16)su;
          a.y[(long)m * a.ldy + c] = (bf16)(gt / (1.f + __expf(-gt)) * up);
        }
      }
    }
  };

  // Steps in pairs while a step follows the pair: both prefetches are real and sit in straight-line code, so the wait
  // in front of a step's sums counts the loads behind it.  The last one or two steps prefetch only what exists.
  int t = 0;
  for (; t + 2 < nsteps; t += 2) {
    const float r0 = load_r(t);
    load(wb, t + 1);
    body(wa, t, r0);
    const float r1 = load_r(t + 1);
    load(wa, t + 2);
    body(wb, t + 1, r1);
  }
  const bool two = t + 1 < nsteps;  // block-uniform
  const float r0 = load_r(t);
  if (two) load(wb, t + 1);
  body(wa, t, r0);
  if (two) body(wb, t + 1, load_r(t + 1));
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

int validate(const void* x, const void* w, const void* y, const void* r, const void* gain, int M, int N, int K, int64_t ldx,
             int64_t ldw, int64_t ldy, int64_t ldr) {
  if (!x || !w || !y || M <= 0 || N <= 0 || K <= 0) return SD_ERR_SHAPE;
  if (M > SD_GEMV_MAX_M || (K & 7) || K > kMaxK || (gain && K > kMaxNormK)) return SD_ERR_UNSUPPORTED;
  if (ldx < K || ldw < K || ldy < N || (r && ldr < N)) return SD_ERR_UNSUPPORTED;
  if ((ldx & 7) || (ldw & 7) || ((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)gain & 15)) return SD_ERR_UNSUPPORTED;
  return 0;
}

template <bool SWIGLU>
int launch(GemvArgs a, void* stream) {
  const int nch = (a.K + 511) / 512;
  a.KS = nch < kMaxWaves ? nch : kMaxWaves;
  a.RW = (4 + a.KS - 1) / a.KS;  // at least 4 waves: 4, 2, 2, 1, 1, ..
  const int ch = (nch + a.KS - 1) / a.KS;  // 1 or 2
  // grid: from N, K (through RW) and the CU count only -- eight workgroups per CU (resident together at small M: the
  // chip's loads in flight come from many workgroups, not from a deep pipeline in each) while a workgroup keeps at least
  // one full step of RW * 4 rows
  const int cus = cu_count();
  if (cus <= 0) return SD_ERR_WORKSPACE;
  int rpw = (a.N + 8 * cus - 1) / (8 * cus);
  rpw = (rpw + 3) & ~3;
  if (rpw < a.RW * 4) rpw = a.RW * 4;
  a.rpw = rpw;
  const unsigned grid = (unsigned)((a.N + rpw - 1) / rpw);
  const unsigned block = (unsigned)(a.KS * a.RW * 64);
  const int mb = a.M <= 1 ? 1 : a.M <= 2 ? 2 : a.M <= 4 ? 4 : a.M <= 8 ? 8 : 16;
  SdProfScope prof(SD_K_GEMM_NT, 2.0 * a.M * a.N * a.K, ST);
  SD_PROF_LABEL("gemv_kernel<%d, %d, %s>", mb, ch, SWIGLU ? "true" : "false");
#define SD_GEMV_GO(MB_, CH_) hipLaunchKernelGGL((gemv_kernel<MB_, CH_, SWIGLU>), dim3(grid), dim3(block), 0, ST, a)
#define SD_GEMV_CH(MB_) do { if (ch == 1) SD_GEMV_GO(MB_, 1); else SD_GEMV_GO(MB_, 2); } while (0)
  switch (mb) {
    case 1: SD_GEMV_CH(1); break;
    case 2: SD_GEMV_CH(2); break;
    case 4: SD_GEMV_CH(4); break;
    case 8: SD_GEMV_CH(8); break;
    default: SD_GEMV_CH(16); break;
  }
#undef SD_GEMV_CH
#undef SD_GEMV_GO
  SD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// the checks of the two entries without a launch (the decode step asks before it commits to the GEMV sequence)
int sd_gemv_check(const void* x, const void* w, const void* y, const void* r, const void* norm_gain, int M, int N, int K,
                  int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr) {
  return validate(x, w, y, r, norm_gain, M, N, K, ldx, ldw, ldy, ldr);
}

extern "C" int sd_gemv_bf16(const void* x, const void* w, void* y, const void* r, const void* norm_gain, float eps, int M,
                            int N, int K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, void* stream) {
  const int rc = validate(x, w, y, r, norm_gain, M, N, K, ldx, ldw, ldy, ldr);
  if (rc) return rc;
  GemvArgs a = {};
  a.x = (const bf16*)x; a.w = (const bf16*)w; a.r = (const bf16*)r; a.gain = (const bf16*)norm_gain; a.y = (bf16*)y;
  a.eps = eps; a.M = M; a.N = N; a.K = K; a.I = 0;
  a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldr = ldr;
  return launch<false>(a, stream);
}

extern "C" int sd_gemv_swiglu(const void* x, const void* wgu, void* act, const void* norm_gain, float eps, int M, int I, int K,
                              void* stream) {
  if (I > (1 << 29)) return SD_ERR_UNSUPPORTED;
  const int rc = validate(x, wgu, act, nullptr, norm_gain, M, I, K, K, K, I, 0);
  if (rc) return rc;
  GemvArgs a = {};
  a.x = (const bf16*)x; a.w = (const bf16*)wgu; a.gain = (const bf16*)norm_gain; a.y = (bf16*)act;
  a.eps = eps; a.M = M; a.N = 2 * I; a.K = K; a.I = I;
  a.ldx = K; a.ldw = K; a.ldy = I; a.ldr = 0;
  return launch<true>(a, stream);
}
