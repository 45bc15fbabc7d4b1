// Device functions shared by the kernels that stream whole vocabulary rows (sd_loss.hip, sd_topk.hip): the 8-element
// load / convert / store, the prefetched row sweep, the online max / sum-exp step and its cross-thread merge, and the
// zero fill of a masked row's gradient.  Each is stated once; DESIGN.md sections 12a and 12e list who calls what.
#pragma once
#include "sd_common.cuh"

// 8 consecutive elements of a bf16 or fp32 row (16-byte aligned) <-> 8 floats
template <typename T> struct Ld8;
template <> struct Ld8<bf16> {
  typedef bf16x8 Raw;  // 8 elements as loaded (prefetched chunks wait in registers in this form)
  static SD_DEV Raw raw(const bf16* p) { return *(const bf16x8*)p; }
  static SD_DEV void cvt(const Raw& v, float* f) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
  }
  static SD_DEV void load(const bf16* p, float* f) { cvt(raw(p), f); }
  static SD_DEV void store(bf16* p, const float* f) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16)f[e];
    *(bf16x8*)p = v;
  }
};
template <> struct Ld8<float> {
  struct Raw { f32x4 a, b; };
  static SD_DEV Raw raw(const float* p) { return Raw{*(const f32x4*)p, *(const f32x4*)(p + 4)}; }
  static SD_DEV void cvt(const Raw& v, float* f) {
    f[0] = v.a[0]; f[1] = v.a[1]; f[2] = v.a[2]; f[3] = v.a[3]; f[4] = v.b[0]; f[5] = v.b[1]; f[6] = v.b[2]; f[7] = v.b[3];
  }
  static SD_DEV void load(const float* p, float* f) { cvt(raw(p), f); }
  static SD_DEV void store(float* p, const float* f) {
    *(f32x4*)p = f32x4{f[0], f[1], f[2], f[3]};
    *(f32x4*)(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
  }
};

constexpr int ROW_PF = 4;  // 8-element chunks in flight per thread and row

// Streams a row (PAIR: a row pair) through `body(c, f, g)` with NF threads: c is the first element of an 8-element
// chunk, f its values in s and, if PAIR, g its values in tl (else g is not to be read, and no teacher register or load
// exists).  Thread t takes the chunks t, t + NF, t + 2 NF, ... in increasing order, so sums are bit for bit those of a
// plain loop.
// ROW_PF chunks per thread are in flight: with one (load, wait, compute) per trip the 32 waves of a CU keep 32 KB
// outstanding, which at ~2 us of loaded HBM latency is 4 TB/s whatever the kernel does (measured 3.9-4.1).  Each slot is
// refilled before the arithmetic on it.
// Every load is UNCONDITIONAL: a chunk past the end re-reads the row's last one (the clamp) and is never used.  With
// loads behind branches hipcc's wait insertion falls back to vmcnt(0) at every use and drains the chunks in flight.
// `body` may store to chunk c of a buffer that aliases `s`: a thread only ever reads ahead in its OWN chunks, which it
// has not written yet, and the clamped re-read of the last chunk is never used.
template <typename T, int NF, bool PAIR, typename F>
SD_DEV void row_sweep(const T* s, const T* tl, int V, F&& body) {
  typedef typename Ld8<T>::Raw Raw;
  constexpr int stride = NF * 8;
  Raw sbuf[ROW_PF], tbuf[PAIR ? ROW_PF : 1];
  const int clast = ((V - 1) >> 3) << 3;  // start of the row's last chunk
#pragma unroll
  for (int j = 0; j < ROW_PF; ++j) {
    const int cj = min((int)threadIdx.x * 8 + j * stride, clast);
    sbuf[j] = Ld8<T>::raw(s + cj);
    if constexpr (PAIR) tbuf[j] = Ld8<T>::raw(tl + cj);
  }
  for (int c0 = threadIdx.x * 8; c0 < V; c0 += ROW_PF * stride) {
#pragma unroll
    for (int j = 0; j < ROW_PF; ++j) {
      const int c = c0 + j * stride;
      float f[8], g[8];
      Ld8<T>::cvt(sbuf[j], f);
      if constexpr (PAIR) Ld8<T>::cvt(tbuf[j], g);
      const int cn = min(c + ROW_PF * stride, clast);
      sbuf[j] = Ld8<T>::raw(s + cn);
      if constexpr (PAIR) tbuf[j] = Ld8<T>::raw(tl + cn);
      if (c >= V) continue;
      body(c, f, g);
    }
  }
}

SD_DEV float chunk_max8(const float* f) {
  float cm = f[0];
#pragma unroll
  for (int e = 1; e < 8; ++e) cm = fmaxf(cm, f[e]);
  return cm;
}

// One online max / sum-exp step: a chunk maximum cm above the running maximum m rescales the sum at T = 1 (s1), the
// sum at T (sT) and every further accumulator of terms weighted by exp((x - m) / T) (`atT`: the dense teacher's cross
// term), then raises m.  T2 (temperature == 2): exp(d) = exp(d / 2)^2, one exponential instead of two.
template <bool T2, typename... Acc>
SD_DEV void online_raise(float cm, float invT, float& m, float& s1, float& sT, Acc&... atT) {
  if (cm > m) {
    const float rT = __expf((m - cm) * invT), r1 = T2 ? rT * rT : __expf(m - cm);
    s1 *= r1;
    sT *= rT;
    ((atT *= rT), ...);
    m = cm;
  }
}

// merge the (m, s1, sT[, atT...]) partials of online_raise across the block; every thread gets the block totals
template <int NF, typename... Acc>
SD_DEV void block_merge(float& m, float& s1, float& sT, float invT, float* sc, Acc&... atT) {
  const float M = block_max<NF>(m, sc);
  const float f1 = (m == -INFINITY) ? 0.f : __expf(m - M);
  const float fT = (m == -INFINITY) ? 0.f : __expf((m - M) * invT);
  s1 = block_sum<NF>(s1 * f1, sc);
  sT = block_sum<NF>(sT * fT, sc);
  ((atT = block_sum<NF>(atT * fT, sc)), ...);
  m = M;
}

// A row's membership bitmap in LDS (the top-K tail kernels): bit j of `bits` says that vocabulary index j is one of the
// row's top-K indices.  V bits, rounded up to whole 16-byte stores: row_bits_bytes(V) of (dynamic) LDS, 19 936 bytes at
// V = 159 488.  Cleared per row by the whole block, set with LDS atomicOr (indices share words), read one BYTE per
// 8-element chunk: V % 8 == 0 and chunks start at multiples of 8, so bit e of that byte is element c + e.
inline __host__ __device__ int row_bits_bytes(int V) { return ((V + 127) >> 7) << 4; }
template <int NF>
SD_DEV void row_bits_clear(uint32_t* bits, int V) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  for (int i = threadIdx.x; i < row_bits_bytes(V) >> 4; i += NF) ((u32x4*)bits)[i] = u32x4{0u, 0u, 0u, 0u};
}
SD_DEV void row_bits_set(uint32_t* bits, int j) { atomicOr(&bits[j >> 5], 1u << (j & 31)); }
SD_DEV unsigned row_bits_chunk(const uint32_t* bits, int c) { return ((const uint8_t*)bits)[c >> 3]; }

// the gradient of a masked row: V zeros, NF threads
template <typename T, int NF>
SD_DEV void zero_row(T* g, int V) {
  const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = threadIdx.x * 8; c < V; c += NF * 8) Ld8<T>::store(g + c, z);
}
