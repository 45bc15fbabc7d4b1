// MXFP8 (OCP Microscaling FP8: e4m3fn elements, one E8M0 power-of-two scale per 32 elements along K) for the FROZEN
// teacher's decoder projections (train.py:60-69, 155-169; HF modeling_qwen3.py:252-254, 279, 81-83):
//   mxfp8_quant_kernel   bf16 rows -> e4m3 bytes + E8M0 scale bytes (+ the row's rstd), used once per weight at load and
//                        for every activation that no producer epilogue emits;
//   gemm_mx_kernel       C = rowscale * (A . B^T) (+ R), both operands MXFP8, on v_mfma_scale_f32_16x16x128_f8f6f4 with
//                        the real E8M0 bytes as scale operands; epilogues: plain / residual, and gate|up with SwiGLU whose
//                        bf16 result leaves only as MXFP8;
//   sd_qwen3_forward_mx  the decoder runner of that precision (attention, final norm and lm_head are the bf16 entries).
// The operand and scale lane maps of the instruction (measured with exact integer data):
//   lane l = (r = l & 15, g = l >> 4) holds A[row r][k = 64 * (j >> 4) + 16 * g + (j & 15)] in byte j = 0..31 of its
//   8-VGPR fragment (two 16-byte runs: k = 16g.. and k = 64 + 16g..), B[col r] likewise; the scale VGPR of lane l
//   carries, in the byte op_sel names, the E8M0 scale of (row r, 32-element block g).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sd_hip.h"
#include "sd_debug.h"
#include "sd_common.cuh"
#include "sd_prof.h"
#include "sd_runner.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

// ------------------------------------------------------------------------------------------ the number format
// 32 bf16-exact values -> 32 e4m3fn bytes + the block's E8M0 byte.  e = floor(log2(amax)) - 8 clamped to [-127, 127]
// (amax == 0: -127), q = RNE_e4m3fn(clamp(x * 2^-e, -448, 448)).  Every product below is exact in fp32.
SD_DEV void mx_quant32(const float (&x)[32], u32x4& q_lo, u32x4& q_hi, uint8_t& scale_byte) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(x[i]));
  const int eb = (int)(__builtin_bit_cast(uint32_t, amax) >> 23);  // biased exponent of amax (sign is 0)
  const int sb = eb > 8 ? eb - 8 : 0;                              // e + 127
  const float inv = __builtin_bit_cast(float, (uint32_t)(254 - sb) << 23);  // 2^-e
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = fminf(fmaxf(x[4 * i + j] * inv, -448.f), 448.f);
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], p, true);
    w[i] = (uint32_t)p;
  }
  q_lo = u32x4{w[0], w[1], w[2], w[3]};
  q_hi = u32x4{w[4], w[5], w[6], w[7]};
  scale_byte = (uint8_t)sb;
}

// One wave per row, one 32-element block per lane and pass.  rstd (nullable) = rsqrt(mean(x^2) + eps) of the row.
__global__ __launch_bounds__(256) void mxfp8_quant_kernel(const bf16* __restrict__ x, long ldx, uint8_t* __restrict__ q,
                                                          uint8_t* __restrict__ scale, float* __restrict__ rstd, float eps,
                                                          int M, int K) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const int nblk = K >> 5;
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
    u32x4 lo, hi;
    uint8_t sb;
    mx_quant32(f, lo, hi, sb);
    uint8_t* qr = q + (long)row * K + b * 32;
    *(u32x4*)qr = lo;
    *(u32x4*)(qr + 16) = hi;
    scale[(long)row * nblk + b] = sb;
  }
  if (rstd) {
    ss = wave_sum(ss);
    if (lane == 0) rstd[row] = rsqrtf(ss / (float)K + eps);
  }
}

// ------------------------------------------------------------------------------------------ the GEMM
// BM x 128 output tile (BM = 128: 4 waves, BM = 256: 8 waves), every wave 64 x 64 = 4 x 4 MFMA tiles; one K-step = 128
// bytes of K = one MFMA per tile.  Operands AND their scale bytes go global -> LDS by DMA into an NST-deep ring: the wait
// for K-step t is a COUNTED s_waitcnt vmcnt that leaves the NST - 2 younger steps in flight across a raw s_barrier (a
// two-deep ring left the whole global latency exposed at every step: 0.8 PF/s).  The next step's DMA pieces are issued
// BETWEEN the MFMA rows.  LDS is read by asm ds_read (sd_common.cuh: hipcc would drain the DMA in front of a C++ LDS read).
// LDS image of an operand tile: [rows][8 chunks of 16 bytes], chunk c of row r stored in slot c ^ ((r >> 1) & 7): the
// 16 rows x 2 chunks that one ds_read_b128 lane group touches then fall into 16 different 16-byte bank groups.
// A lane's fragment is chunk g and chunk 4 + g of its row (the lane map in the file header); the scale image is one
// dword per tile row (the 4 block scales of this K-step), lane (r, g) reads byte g of its row's dword.
// EPI_PLAIN : C[m][n] = bf16(rowscale[m] * acc + R[m][n])
// EPI_SWIGLU: B tile rows 0..63 = gate rows n0.., 64..127 = up rows I + n0..; g, u = bf16(rowscale * acc);
//             act = bf16(silu(g) * u) as sd_swiglu_fwd computes it, stored ONLY as MXFP8 (act_q, act_scale).
// The epilogue passes the fp32 tile through LDS (over the operand ring), so that one thread owns a whole 32-column
// block of a row: full-width stores, and the same mx_quant32 as the standalone kernel (bit-identical by construction).
constexpr int EPI_PLAIN = 0, EPI_SWIGLU = 1;
constexpr int kCStride = 132;  // fp32 words per row of the epilogue image

SD_DEV void lds_rd128(i32x4& d, unsigned addr) { asm volatile("ds_read_b128 %0, %1" : "=v"(d) : "v"(addr)); }
SD_DEV void lds_rd8(int& d, unsigned addr) { asm volatile("ds_read_u8 %0, %1" : "=v"(d) : "v"(addr)); }
SD_DEV void lds_wait8(i32x4 (&a)[8]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]));
}
SD_DEV void lds_wait8i(int (&a)[8]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]));
}
SD_DEV void glds4(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const SD_GLB void*)gsrc, (SD_LDS void*)lds_wave_base, 4, 0, 0);
}

template <int BM, int NST>
struct MxCfg {
  static constexpr int NT = BM * 2;                             // threads: one wave per 64 x 64 of the tile
  static constexpr int PA = BM * 8 / NT, PB = 128 * 8 / NT;     // 16-byte DMA pieces per thread and K-step
  static constexpr int LOADS = PA + PB + 1;                     // + the scale dword
  static constexpr int kStage = (BM + 128) * 128 + NT * 4;      // A tile | B tile | one scale dword per thread
  static constexpr int kEpi = BM * kCStride * 4;
  static constexpr int kLds = NST * kStage > kEpi ? NST * kStage : kEpi;
};

template <int EPI, int BM, int NST>
__global__ __launch_bounds__(BM * 2, 1) void gemm_mx_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ As,
                                                            const uint8_t* __restrict__ B, const uint8_t* __restrict__ Bs,
                                                            bf16* __restrict__ C, const bf16* R,
                                                            const float* __restrict__ rowscale, uint8_t* __restrict__ Cq,
                                                            uint8_t* __restrict__ Cs, int M, int N, int K, long ldc,
                                                            long ldr, int tiles_m, int n_tiles) {
  using Cfg = MxCfg<BM, NST>;
  constexpr int NT = Cfg::NT, PA = Cfg::PA, PB = Cfg::PB;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_uniform();
  const int tile = xcd_remap(blockIdx.x, n_tiles);
  const int tm = tile % tiles_m, tn = tile / tiles_m;
  const int m0 = tm * BM;
  // N = rows of B the tile's columns come from.  SWIGLU: N is I, the tile owns 64 act columns
  const int n0 = EPI == EPI_SWIGLU ? tn * 64 : tn * 128;
  const int nblk = K >> 5, nk = K >> 7;
  auto b_row = [&](int r) {  // global row of B behind row r of the B tile
    if (EPI == EPI_SWIGLU) return r < 64 ? n0 + r : N + n0 + (r - 64);
    const int br = n0 + r;
    return br < N ? br : N - 1;  // rows past the edge re-read the last row; their results are never stored
  };
  auto a_row = [&](int r) { const int ar = m0 + r; return ar < M ? ar : M - 1; };

  // staging: thread tid moves slots i * NT + tid of each operand: row s >> 3, chunk slot s & 7; and one scale dword
  const uint8_t* ga[PA];
  const uint8_t* gb[PB];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    const int s = i * NT + tid, r = s >> 3, c = (s & 7) ^ ((r >> 1) & 7);
    ga[i] = A + (long)a_row(r) * K + c * 16;
  }
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int s = i * NT + tid, r = s >> 3, c = (s & 7) ^ ((r >> 1) & 7);
    gb[i] = B + (long)b_row(r) * K + c * 16;
  }
  // scale dword of tile row tid: A rows, then B rows, then (BM = 256) spare threads repeating the last B row
  const uint8_t* gs = tid < BM ? As + (long)a_row(tid) * nblk : Bs + (long)b_row(tid - BM < 128 ? tid - BM : 127) * nblk;

  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const unsigned lds0 = lds_addr(smem);
  const unsigned swx = (unsigned)((fr >> 1) & 7);
  // byte offsets inside a stage of this lane's fragment chunks (MFMA tile t adds 16 rows = 2048 bytes) and scale bytes
  const unsigned oa_lo = (wm * 64 + fr) * 128 + ((fg ^ swx) << 4), oa_hi = (wm * 64 + fr) * 128 + (((4 + fg) ^ swx) << 4);
  const unsigned ob_lo = BM * 128 + (wn * 64 + fr) * 128 + ((fg ^ swx) << 4);
  const unsigned ob_hi = BM * 128 + (wn * 64 + fr) * 128 + (((4 + fg) ^ swx) << 4);
  const unsigned osa = (BM + 128) * 128 + (wm * 64 + fr) * 4 + fg, osb = (BM + 128) * 128 + (BM + wn * 64 + fr) * 4 + fg;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // piece i (0..3) of K-step kt into ring slot buf
  auto stage_piece = [&](int kt, int buf, int i) {
    uint8_t* st = smem + buf * Cfg::kStage;
    if (i < PA) glds16(ga[i] + kt * 128, st + (i * NT + wave * 64) * 16);
    if (i < PB) glds16(gb[i] + kt * 128, st + BM * 128 + (i * NT + wave * 64) * 16);
    if (i == 3) glds4(gs + kt * 4, st + (BM + 128) * 128 + wave * 64 * 4);
  };
  // Steps past the end re-stage the last one (into a slot nobody reads any more): no branch, uniform vmcnt accounting.
#pragma unroll
  for (int s = 0; s < NST - 1; ++s)
#pragma unroll
    for (int i = 0; i < 4; ++i) stage_piece(s < nk ? s : nk - 1, s, i);

  int buf = 0, buf_in = NST - 1;
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * Cfg::LOADS) : "memory");  // my pieces of step kt have landed
    __builtin_amdgcn_s_barrier();  // ... and everybody's; every wave is done reading step kt - 1 (slot buf_in)
    const unsigned st = lds0 + buf * Cfg::kStage;
    i32x4 fa[8], fb[8];
    int xs[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      lds_rd128(fa[2 * t], st + oa_lo + t * 2048);
      lds_rd128(fa[2 * t + 1], st + oa_hi + t * 2048);
      lds_rd128(fb[2 * t], st + ob_lo + t * 2048);
      lds_rd128(fb[2 * t + 1], st + ob_hi + t * 2048);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      lds_rd8(xs[t], st + osa + t * 64);
      lds_rd8(xs[4 + t], st + osb + t * 64);
    }
    lds_wait8(fa);
    lds_wait8(fb);
    lds_wait8i(xs);
    const int kn = kt + NST - 1 < nk ? kt + NST - 1 : nk - 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const i32x8 av = {fa[2 * i][0], fa[2 * i][1], fa[2 * i][2], fa[2 * i][3],
                        fa[2 * i + 1][0], fa[2 * i + 1][1], fa[2 * i + 1][2], fa[2 * i + 1][3]};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const i32x8 bv = {fb[2 * j][0], fb[2 * j][1], fb[2 * j][2], fb[2 * j][3],
                          fb[2 * j + 1][0], fb[2 * j + 1][1], fb[2 * j + 1][2], fb[2 * j + 1][3]};
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc[i][j], 0, 0, 0, xs[i], 0, xs[4 + j]);
      }
      __builtin_amdgcn_sched_barrier(0);
      stage_piece(kn, buf_in, i);
      __builtin_amdgcn_sched_barrier(0);
    }
    buf_in = buf;
    buf = buf + 1 == NST ? 0 : buf + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail stages have landed before LDS is reused

  // ---- epilogue: fp32 tile -> LDS (C/D map: col = lane & 15, row = 4 * (lane >> 4) + reg), then one 32-column block
  // of one row per thread and pass
  __syncthreads();  // every wave is done reading the last operand tile
  float* ct = (float*)smem;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ct[(wm * 64 + i * 16 + fg * 4 + r) * kCStride + wn * 64 + j * 16 + fr] = acc[i][j][r];
  __syncthreads();

  if (EPI == EPI_PLAIN) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int u = it * NT + tid, lr = u >> 2, blk = u & 3;
      const int row = m0 + lr, col = n0 + blk * 32;
      if (row >= M || col >= N) continue;  // N % 32 == 0: a block is inside or outside as a whole
      const float rs = rowscale ? rowscale[row] : 1.f;
      const float* src = ct + lr * kCStride + blk * 32;
#pragma unroll
      for (int c8 = 0; c8 < 4; ++c8) {
        const f32x4 v0 = *(const f32x4*)(src + c8 * 8), v1 = *(const f32x4*)(src + c8 * 8 + 4);
        float f[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        if (R) {
          const bf16x8 rv = *(const bf16x8*)(R + (long)row * ldr + col + c8 * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = f[e] * rs + (float)rv[e];
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = f[e] * rs;
        }
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)f[e];
        *(bf16x8*)(C + (long)row * ldc + col + c8 * 8) = o;
      }
    }
  } else {
    const int lr = tid >> 1, blk = tid & 1;
    const int row = m0 + lr, col = n0 + blk * 32;  // act column; N (= I) % 64 == 0: always inside
    if (row < M) {
      const float rs = rowscale ? rowscale[row] : 1.f;
      const float* gs = ct + lr * kCStride + blk * 32;
      const float* us = gs + 64;
      float f[32];
#pragma unroll
      for (int c4 = 0; c4 < 8; ++c4) {
        const f32x4 gv = *(const f32x4*)(gs + c4 * 4), uv = *(const f32x4*)(us + c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = (float)(bf16)(gv[e] * rs), up = (float)(bf16)(uv[e] * rs);
          f[c4 * 4 + e] = (float)(bf16)(g / (1.f + __expf(-g)) * up);
        }
      }
      u32x4 lo, hi;
      uint8_t sbyte;
      mx_quant32(f, lo, hi, sbyte);
      uint8_t* qr = Cq + (long)row * N + col;
      *(u32x4*)qr = lo;
      *(u32x4*)(qr + 16) = hi;
      Cs[(long)row * (N >> 5) + (col >> 5)] = sbyte;
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// BM = 256 (8 waves, 3-deep ring) when that still gives every CU a tile, else BM = 128 (4 waves, 4-deep ring).
// `tiles_n`: column tiles (128 output columns, or 64 act columns of the SwiGLU form).
template <int EPI, int BM, int NST>
int launch_mx(const void* a_q, const void* a_scale, const void* b_q, const void* b_scale, void* C, const void* R,
              const float* rowscale, void* c_q, void* c_scale, int M, int N, int K, long ldc, long ldr, int tiles_n,
              hipStream_t st) {
  using Cfg = MxCfg<BM, NST>;
  auto kern = gemm_mx_kernel<EPI, BM, NST>;
  // more than 64 KiB of dynamic LDS has to be allowed per function (and device); the call is a host-side table update
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLds) != hipSuccess)
    return SD_ERR_UNSUPPORTED;
  const int tiles_m = (M + BM - 1) / BM;
  SD_PROF_LABEL("gemm_mx_kernel<%d, %d, %d>", EPI, BM, NST);
  hipLaunchKernelGGL(kern, dim3(tiles_m * tiles_n), dim3(Cfg::NT), Cfg::kLds, st, (const uint8_t*)a_q,
                     (const uint8_t*)a_scale, (const uint8_t*)b_q, (const uint8_t*)b_scale, (bf16*)C, (const bf16*)R,
                     rowscale, (uint8_t*)c_q, (uint8_t*)c_scale, M, N, K, ldc, ldr, tiles_m, tiles_m * tiles_n);
  SD_CHECK_LAUNCH();
  return 0;
}
inline bool use_bm256(int M, int tiles_n) { return (long)((M + 255) / 256) * tiles_n >= 256; }

}  // namespace

extern "C" int sd_mxfp8_quant(const void* x, int64_t ldx, void* q, void* scale, float* rstd, float eps, int M, int K,
                              void* stream) {
  if (M <= 0 || K <= 0 || (K & 127) || ldx < K || (ldx & 7)) return SD_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(q) || ((uintptr_t)scale & 3)) return SD_ERR_ALIGN;
  SdProfScope prof(SD_K_MISC, 3.0 * M * K, (hipStream_t)stream);
  SD_PROF_LABEL("mxfp8_quant_kernel");
  hipLaunchKernelGGL(mxfp8_quant_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (long)ldx,
                     (uint8_t*)q, (uint8_t*)scale, rstd, eps, M, K);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_gemm_mxfp8(const void* a_q, const void* a_scale, const void* b_q, const void* b_scale, void* C,
                             const void* R, const float* rowscale, int M, int N, int K, int64_t ldc, int64_t ldr,
                             void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (K & 127) || (N & 31) || ldc < N || (ldc & 7) || (R && (ldr < N || (ldr & 7))))
    return SD_ERR_SHAPE;
  if (!aligned16(a_q) || !aligned16(b_q) || !aligned16(C) || !aligned16(R) || ((uintptr_t)a_scale & 3) ||
      ((uintptr_t)b_scale & 3))
    return SD_ERR_ALIGN;
  const int tiles_n = (N + 127) / 128;
  SdProfScope prof(SD_K_GEMM_NT, 2.0 * M * N * K, (hipStream_t)stream);
  if (use_bm256(M, tiles_n))
    return launch_mx<EPI_PLAIN, 256, 3>(a_q, a_scale, b_q, b_scale, C, R, rowscale, nullptr, nullptr, M, N, K, (long)ldc,
                                        (long)ldr, tiles_n, (hipStream_t)stream);
  return launch_mx<EPI_PLAIN, 128, 4>(a_q, a_scale, b_q, b_scale, C, R, rowscale, nullptr, nullptr, M, N, K, (long)ldc,
                                      (long)ldr, tiles_n, (hipStream_t)stream);
}

extern "C" int sd_gemm_mxfp8_swiglu(const void* a_q, const void* a_scale, const void* wgu_q, const void* wgu_scale,
                                    const float* rowscale, void* act_q, void* act_scale, int M, int I, int K,
                                    void* stream) {
  if (M <= 0 || I <= 0 || K <= 0 || (K & 127) || (I & 127)) return SD_ERR_SHAPE;
  if (!aligned16(a_q) || !aligned16(wgu_q) || !aligned16(act_q) || ((uintptr_t)a_scale & 3) || ((uintptr_t)wgu_scale & 3))
    return SD_ERR_ALIGN;
  const int tiles_n = I / 64;
  SdProfScope prof(SD_K_GEMM_NT, 4.0 * M * I * K, (hipStream_t)stream);
  if (use_bm256(M, tiles_n))
    return launch_mx<EPI_SWIGLU, 256, 3>(a_q, a_scale, wgu_q, wgu_scale, nullptr, nullptr, rowscale, act_q, act_scale, M, I,
                                         K, 0L, 0L, tiles_n, (hipStream_t)stream);
  return launch_mx<EPI_SWIGLU, 128, 4>(a_q, a_scale, wgu_q, wgu_scale, nullptr, nullptr, rowscale, act_q, act_scale, M, I, K,
                                       0L, 0L, tiles_n, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ the decoder runner
namespace {

struct MxActs : SdShape {
  char *x_a, *x_b, *x_mid, *xq, *xs, *rstd, *qkv, *qk, *ao, *lse, *aoq, *aos, *actq, *acts, *rstd_f, *xn_f, *xn_rows;
  int64_t total;
  MxActs(const sd_qwen3_dims* d, int B, int T, char* p) : SdShape(d, B, T) {
    char* p0 = p;
    auto take = [&](int64_t n) { char* r = p; p += al(n); return r; };
    const int64_t x = (int64_t)M * h * 2;
    x_a = take(x); x_b = take(x); x_mid = take(x);
    xq = take((int64_t)M * h); xs = take((int64_t)M * h / 32);
    rstd = take((int64_t)M * 4);
    qkv = take((int64_t)M * QKV * 2); qk = take((int64_t)M * QK * 2); ao = take((int64_t)M * QD * 2);
    lse = take((int64_t)M * Hq * 4);
    aoq = take((int64_t)M * QD); aos = take((int64_t)M * QD / 32);
    actq = take((int64_t)M * I); acts = take((int64_t)M * I / 32);
    rstd_f = take((int64_t)M * 4); xn_f = take(x); xn_rows = take(x);
    total = p - p0;
  }
};

bool mx_supported(const sd_qwen3_dims* d) {
  return d->head_dim == 128 && d->hidden > 0 && (d->hidden % 128) == 0 && d->inter > 0 && (d->inter % 128) == 0 &&
         d->n_q > 0 && d->n_kv > 0;
}

}  // namespace

extern "C" int sd_qwen3_mx_supported(const sd_qwen3_dims* d) { return d && mx_supported(d) ? 1 : 0; }

extern "C" int64_t sd_qwen3_mx_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  if (!d || !mx_supported(d)) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || T <= 0) return SD_ERR_SHAPE;
  return MxActs(d, B, T, nullptr).total;
}

// The forward of sd_qwen3_forward_mx and of the two block entries over a KV cache below.  sink (sd_qwen3_mx_prefill): each
// layer's K / V rows below kv_len also go to planes l of the cache, right behind the layer's q|k|v step.  sink->past
// (sd_qwen3_mx_extend): bt's cos/sin tables hold one row per TOKEN (sd_rope_rows_at) and sink->extend stands where the
// attention does, as in layer_forward of the bf16 runner.
static int forward_mx_impl(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const sd_qwen3_batch* bt, void* acts,
                           int64_t acts_bytes, void* logits, int flags, void* stream, const KvSink* sink) {
  if (!d || !p || !mx_supported(d)) return SD_ERR_UNSUPPORTED;
  RUN(sd_batch_check(bt));
  if (flags & ~SD_FWD_CONCURRENT) return SD_ERR_SHAPE;
  const int B = bt->B, T = bt->T;
  MxActs a(d, B, T, (char*)acts);
  if (acts_bytes < a.total) return SD_ERR_WORKSPACE;
  SdSharedGpuScope shared((flags & SD_FWD_CONCURRENT) ? 1 : 0);  // read by the bf16 GEMM dispatch (lm_head)
  const int M = a.M, h = a.h;
  const bool extend = sink && sink->past;
  const int Trope = extend ? M : T;  // per-token tables: row m of them belongs to token m
  char* x_cur = a.x_a;
  RUN(sd_embedding_fwd(bt->ids, p->embed, x_cur, M, h, a.V, stream));
  for (int l = 0; l < a.L; ++l) {
    const sd_qwen3_layer_mx& w = p->layers_host[l];
    char* x_out = x_cur == a.x_a ? a.x_b : a.x_a;
    // input RMSNorm folded: its gain is in wqkv, its row statistic is the q|k|v GEMM's row scale (HF:59-64, 252-254)
    RUN(sd_mxfp8_quant(x_cur, h, a.xq, a.xs, (float*)a.rstd, d->eps, M, h, stream));
    RUN(sd_gemm_mxfp8(a.xq, a.xs, w.wqkv_q, w.wqkv_scale, a.qkv, nullptr, (const float*)a.rstd, M, a.QKV, h, a.QKV, 0,
                      stream));
    RUN(sd_qknorm_rope_fwd(a.qkv, w.q_gain, w.k_gain, bt->cos_tab, bt->sin_tab, a.qk, M, Trope, a.Hq, a.Hkv, d->eps, stream));
    if (extend) {
      RUN(sink->extend(a, l, a.qk, a.qkv, a.ao, B, T, stream));
    } else {
      if (sink) RUN(sink->store(a, l, a.qk, a.qkv, bt->kv_len, B, T, stream));
      RUN(sd_layer_attn_fwd(a, *bt, a.qk, a.qkv, a.ao, a.lse, stream));
    }
    RUN(sd_mxfp8_quant(a.ao, a.QD, a.aoq, a.aos, nullptr, 0.f, M, a.QD, stream));
    RUN(sd_gemm_mxfp8(a.aoq, a.aos, w.wo_q, w.wo_scale, a.x_mid, x_cur, nullptr, M, h, a.QD, h, h, stream));
    // post-attention RMSNorm folded into wgu the same way (HF:59-64, 81-83)
    RUN(sd_mxfp8_quant(a.x_mid, h, a.xq, a.xs, (float*)a.rstd, d->eps, M, h, stream));
    RUN(sd_gemm_mxfp8_swiglu(a.xq, a.xs, w.wgu_q, w.wgu_scale, (const float*)a.rstd, a.actq, a.acts, M, a.I, h, stream));
    RUN(sd_gemm_mxfp8(a.actq, a.acts, w.wdown_q, w.wdown_scale, x_out, a.x_mid, nullptr, M, h, a.I, h, h, stream));
    x_cur = x_out;
  }
  return sd_head_fwd(d, a, *bt, x_cur, p->final_norm, p->lm_head, a.rstd_f, a.xn_f, a.xn_rows, logits, stream);
}

extern "C" int sd_qwen3_forward_mx(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const sd_qwen3_batch* bt, void* acts,
                                   int64_t acts_bytes, void* logits, int flags, void* stream) {
  return forward_mx_impl(d, p, bt, acts, acts_bytes, logits, flags, stream, nullptr);
}

// ------------------------------------------------------------------------------------------ generation on MXFP8 weights
// (llm_engine.py:37-76: prefill the prompt once, then one token per step over the cache) -- the three runner entries of
// sd_model.hip over sd_qwen3_params_mx; one descriptor (sd_kv_ref) names the cache of any of the three kinds.
namespace {

// head rows behind the forward's activation set -- for an extend also the gathered cos / sin rows -- then the forward
int block_forward_mx(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids, const int32_t* kv_len,
                     const void* cos_tab, const void* sin_tab, void* acts, void* logits, int B, int T, void* stream,
                     const KvSink& sink) {
  const int64_t base = al(sd_qwen3_mx_acts_bytes(d, B, T));
  int64_t* rows = (int64_t*)((char*)acts + base);
  RUN(sd_last_rows(sink.past ? sink.new_len : kv_len, rows, B, T, stream));
  sd_qwen3_batch bt = {ids, kv_len, nullptr, cos_tab, sin_tab, rows, B, B, T, 0};
  if (sink.past) {  // (an extend has no kv_len)
    char* cos_rows = (char*)acts + al(sd_qwen3_mx_prefill_acts_bytes(d, B, T));
    char* sin_rows = cos_rows + al((int64_t)B * T * 128 * 2);
    RUN(sd_rope_rows_at(cos_tab, sin_tab, sink.past, cos_rows, sin_rows, B, T, sink.cap, stream));
    bt.cos_tab = cos_rows; bt.sin_tab = sin_rows;
  }
  return forward_mx_impl(d, p, &bt, acts, base, logits, 0, stream, &sink);
}

// The buffers of a decode step: the bf16 rows of both kinds of step, the MXFP8 operands of the tile kind, the attention's
// workspace
struct MxDecodeActs : SdShape {
  char *x, *x_mid, *xn, *qkv, *q, *ao, *act, *xq, *xs, *rstd, *aoq, *aos, *actq, *acts, *ws;
  int32_t* tickets = nullptr;  // fused: the tickets of the one-launch cache step, int32 [L][B][Hkv], at the tail
  int64_t ws_bytes, total;
  MxDecodeActs(const sd_qwen3_dims* d, int B, int cap, char* p, bool fused = false) : SdShape(d, B, 1) {
    int64_t off = 0;  // (p == nullptr: a size query, no address is formed)
    auto take = [&](int64_t n) { char* q = p ? p + off : nullptr; off += al(n); return q; };
    const int64_t xb = (int64_t)M * h * 2;
    x = take(xb); x_mid = take(xb); xn = take(xb);
    qkv = take((int64_t)M * QKV * 2); q = take((int64_t)M * QD * 2); ao = take((int64_t)M * QD * 2);
    act = take((int64_t)M * I * 2);
    xq = take((int64_t)M * h); xs = take((int64_t)M * h / 32); rstd = take((int64_t)M * 4);
    aoq = take((int64_t)M * QD); aos = take((int64_t)M * QD / 32);
    actq = take((int64_t)M * I); acts = take((int64_t)M * I / 32);
    ws_bytes = sd_attn_decode_workspace_bytes(B, Hq, cap);
    ws = take(ws_bytes);
    if (fused) tickets = (int32_t*)take(KvSink::ticket_bytes(*this, B));
    total = off;
  }
};

// true when every GEMV of a skinny step accepts its shape: decided for the whole step before the first launch.  wide: the
// step of sd_qwen3_mx_decode_step_wide (the 64-row kernels, the head on sd_gemv_wide_bf16)
bool skinny_mx_ok(const sd_qwen3_params_mx* p, const MxDecodeActs& a, const void* logits, int B, bool wide) {
  const auto check = wide ? sd_gemv_mx_wide_check : sd_gemv_mx_check;
  bool ok = (wide ? sd_gemv_wide_check(a.x, p->lm_head, logits, nullptr, p->final_norm, B, a.V, a.h, a.h, a.h, a.V, 0)
                  : sd_gemv_check(a.x, p->lm_head, logits, nullptr, p->final_norm, B, a.V, a.h, a.h, a.h, a.V, 0)) == 0;
  for (int l = 0; ok && l < a.L; ++l) {
    const sd_qwen3_layer_mx& w = p->layers_host[l];
    ok = check(a.x, a.h, w.wqkv_q, w.wqkv_scale, a.qkv, a.QKV, nullptr, 0, B, a.QKV, a.h) == 0 &&
         check(a.ao, a.QD, w.wo_q, w.wo_scale, a.x_mid, a.h, a.x, a.h, B, a.h, a.QD) == 0 &&
         check(a.x_mid, a.h, w.wgu_q, w.wgu_scale, a.act, a.I, nullptr, 0, B, a.I, a.h) == 0 &&
         check(a.act, a.I, w.wdown_q, w.wdown_scale, a.x, a.h, a.x_mid, a.h, B, a.h, a.I) == 0;
  }
  return ok;
}

}  // namespace

extern "C" int64_t sd_qwen3_mx_prefill_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  const int64_t base = sd_qwen3_mx_acts_bytes(d, B, T);
  return base < 0 ? base : al(base) + al((int64_t)B * 8);  // + the head rows (int64 [B])
}

extern "C" int sd_qwen3_mx_prefill(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids,
                                   const int32_t* kv_len, const void* cos_tab, const void* sin_tab, void* acts,
                                   int64_t acts_bytes, const sd_kv_ref* kv, void* logits, int B, int T, void* stream) {
  if (!d || !p || !kv) return SD_ERR_SHAPE;
  if (!mx_supported(d)) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || T <= 0 || !logits || !ids || !acts) return SD_ERR_SHAPE;
  KvSink sink = {};
  RUN(ref_sink(d, kv, B, &sink));
  if (sink.cap < T) return SD_ERR_SHAPE;
  if (acts_bytes < sd_qwen3_mx_prefill_acts_bytes(d, B, T)) return SD_ERR_WORKSPACE;
  return block_forward_mx(d, p, ids, kv_len, cos_tab, sin_tab, acts, logits, B, T, stream, sink);
}

extern "C" int64_t sd_qwen3_mx_extend_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  if (!d) return SD_ERR_SHAPE;
  const int64_t base = sd_qwen3_mx_prefill_acts_bytes(d, B, T);
  return base < 0 ? base : al(base) + 2 * al((int64_t)B * T * 128 * 2);
}

extern "C" int sd_qwen3_mx_extend(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids,
                                  const int32_t* past, const int32_t* new_len, const void* cos_tab, const void* sin_tab,
                                  void* acts, int64_t acts_bytes, const sd_kv_ref* kv, void* logits, int B, int T,
                                  void* stream) {
  if (!d || !p || !kv) return SD_ERR_SHAPE;
  if (!mx_supported(d)) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || T <= 0 || !ids || !past || !new_len || !cos_tab || !sin_tab || !acts || !logits) return SD_ERR_SHAPE;
  KvSink sink = {};
  RUN(ref_sink(d, kv, B, &sink));
  if (sink.cap < T) return SD_ERR_SHAPE;
  RUN(gqa_check(d));
  if (acts_bytes < sd_qwen3_mx_extend_acts_bytes(d, B, T)) return SD_ERR_WORKSPACE;
  sink.past = past; sink.new_len = new_len;
  return block_forward_mx(d, p, ids, nullptr, cos_tab, sin_tab, acts, logits, B, T, stream, sink);
}

extern "C" int64_t sd_qwen3_mx_decode_step_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  if (!d || !mx_supported(d)) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || cap <= 0) return SD_ERR_SHAPE;
  return MxDecodeActs(d, B, cap, nullptr).total;
}

// the checks and launches of sd_qwen3_mx_decode_step; fused: on the one-launch cache step (sd_qwen3_mx_decode_step_fused);
// shared: on the shared-page decode attention over a paged cache (sd_qwen3_mx_decode_step_shared); wide: the skinny
// sequence on the 64-row kernels (sd_qwen3_mx_decode_step_wide)
static int mx_decode_step(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids, const int32_t* pos,
                          int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_ref* kvr, void* acts,
                          int64_t acts_bytes, void* logits, int B, int flags, void* stream, bool fused,
                          bool shared = false, bool wide = false) {
  if (flags & ~SD_DECODE_SKINNY) return SD_ERR_SHAPE;
  if (!d || !p || !kvr) return SD_ERR_SHAPE;
  if (!mx_supported(d)) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || max_len <= 0 || !ids || !pos || !logits || !acts) return SD_ERR_SHAPE;
  if ((fused || shared) && (!cos_tab || !sin_tab)) return SD_ERR_SHAPE;
  if (shared && kvr->kind == 0) return SD_ERR_SHAPE;  // rows of a contiguous cache share nothing
  RUN(gqa_check(d));
  KvSink kv = {};
  RUN(ref_sink(d, kvr, B, &kv));
  const MxDecodeActs a(d, B, kv.cap, (char*)acts, fused);
  if (acts_bytes < a.total) return SD_ERR_WORKSPACE;
  if (fused) RUN(fused_align_check(acts, kv));
  kv.tickets = a.tickets;
  kv.shared = shared;
  const int h = a.h;
  const float eps = d->eps;
  const bool skinny = (flags & SD_DECODE_SKINNY) && skinny_mx_ok(p, a, logits, B, wide);
  RUN(kv.begin_step(a, B, stream));
  RUN(sd_embedding_fwd(ids, p->embed, a.x, B, h, a.V, stream));
  if (skinny) {
    const auto gemv = wide ? sd_gemv_mxfp8_wide : sd_gemv_mxfp8;
    const auto gemv_swiglu = wide ? sd_gemv_mxfp8_wide_swiglu : sd_gemv_mxfp8_swiglu;
    for (int l = 0; l < a.L; ++l) {
      const sd_qwen3_layer_mx& w = p->layers_host[l];
      RUN(gemv(a.x, h, w.wqkv_q, w.wqkv_scale, a.qkv, a.QKV, nullptr, 0, 1, eps, B, a.QKV, h, stream));
      RUN(kv.step(a, l, w.q_gain, w.k_gain, a.qkv, a.q, a.ao, cos_tab, sin_tab, pos, a.ws, a.ws_bytes, B, max_len, eps,
                  stream));
      RUN(gemv(a.ao, a.QD, w.wo_q, w.wo_scale, a.x_mid, h, a.x, h, 0, 0.f, B, h, a.QD, stream));
      RUN(gemv_swiglu(a.x_mid, w.wgu_q, w.wgu_scale, a.act, 1, eps, B, a.I, h, stream));
      RUN(gemv(a.act, a.I, w.wdown_q, w.wdown_scale, a.x, h, a.x_mid, h, 0, 0.f, B, h, a.I, stream));
    }
    return (wide ? sd_gemv_wide_bf16 : sd_gemv_bf16)(a.x, p->lm_head, logits, nullptr, p->final_norm, eps, B, a.V, h, h, h,
                                                     a.V, 0, stream);
  }
  for (int l = 0; l < a.L; ++l) {
    const sd_qwen3_layer_mx& w = p->layers_host[l];
    RUN(sd_mxfp8_quant(a.x, h, a.xq, a.xs, (float*)a.rstd, eps, B, h, stream));
    RUN(sd_gemm_mxfp8(a.xq, a.xs, w.wqkv_q, w.wqkv_scale, a.qkv, nullptr, (const float*)a.rstd, B, a.QKV, h, a.QKV, 0,
                      stream));
    RUN(kv.step(a, l, w.q_gain, w.k_gain, a.qkv, a.q, a.ao, cos_tab, sin_tab, pos, a.ws, a.ws_bytes, B, max_len, eps, stream));
    RUN(sd_mxfp8_quant(a.ao, a.QD, a.aoq, a.aos, nullptr, 0.f, B, a.QD, stream));
    RUN(sd_gemm_mxfp8(a.aoq, a.aos, w.wo_q, w.wo_scale, a.x_mid, a.x, nullptr, B, h, a.QD, h, h, stream));
    RUN(sd_mxfp8_quant(a.x_mid, h, a.xq, a.xs, (float*)a.rstd, eps, B, h, stream));
    RUN(sd_gemm_mxfp8_swiglu(a.xq, a.xs, w.wgu_q, w.wgu_scale, (const float*)a.rstd, a.actq, a.acts, B, a.I, h, stream));
    RUN(sd_gemm_mxfp8(a.actq, a.acts, w.wdown_q, w.wdown_scale, a.x, a.x_mid, nullptr, B, h, a.I, h, h, stream));
  }
  RUN(sd_rmsnorm_fwd(a.x, p->final_norm, a.xn, nullptr, B, h, eps, stream));
  return sd_gemm_bf16(a.xn, p->lm_head, logits, nullptr, B, a.V, h, h, h, a.V, 0, 0, 0, stream);
}

extern "C" int sd_qwen3_mx_decode_step(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids,
                                       const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                       const sd_kv_ref* kvr, void* acts, int64_t acts_bytes, void* logits, int B, int flags,
                                       void* stream) {
  return mx_decode_step(d, p, ids, pos, max_len, cos_tab, sin_tab, kvr, acts, acts_bytes, logits, B, flags, stream, false);
}

extern "C" int64_t sd_qwen3_mx_decode_step_fused_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  if (!d || !mx_supported(d)) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || cap <= 0) return SD_ERR_SHAPE;
  return MxDecodeActs(d, B, cap, nullptr, true).total;
}

extern "C" int sd_qwen3_mx_decode_step_fused(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids,
                                             const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                             const sd_kv_ref* kvr, void* acts, int64_t acts_bytes, void* logits, int B,
                                             int flags, void* stream) {
  return mx_decode_step(d, p, ids, pos, max_len, cos_tab, sin_tab, kvr, acts, acts_bytes, logits, B, flags, stream, true);
}

extern "C" int64_t sd_qwen3_mx_decode_step_shared_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  return sd_qwen3_mx_decode_step_acts_bytes(d, B, cap);
}

extern "C" int sd_qwen3_mx_decode_step_shared(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids,
                                              const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                              const sd_kv_ref* kvr, void* acts, int64_t acts_bytes, void* logits, int B,
                                              int flags, void* stream) {
  return mx_decode_step(d, p, ids, pos, max_len, cos_tab, sin_tab, kvr, acts, acts_bytes, logits, B, flags, stream, false,
                        true);
}

// sd_qwen3_mx_decode_step_wide: the skinny sequence on the 64-row kernels over a cache of any kind
extern "C" int64_t sd_qwen3_mx_decode_step_wide_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  return sd_qwen3_mx_decode_step_acts_bytes(d, B, cap);
}

extern "C" int sd_qwen3_mx_decode_step_wide(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids,
                                            const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                            const sd_kv_ref* kvr, void* acts, int64_t acts_bytes, void* logits, int B,
                                            void* stream) {
  return mx_decode_step(d, p, ids, pos, max_len, cos_tab, sin_tab, kvr, acts, acts_bytes, logits, B, SD_DECODE_SKINNY,
                        stream, false, false, true);
}
