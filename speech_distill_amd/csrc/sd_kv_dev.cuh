// Device functions the decode-side cache kernels share: sd_decode.hip (append, split-KV attention, merge as three
// launches), sd_cache_step.hip (the same work as one launch) and sd_attn_shared.hip (the attention for rows that share
// pages).  The partition constants, the 16-byte pack / unpack, the page table lookup and the MXFP8 page format; and, in the
// second half, the ONE statement of the arithmetic those kernels must agree on bit for bit: the q/k-norm + RoPE of a head
// chunk, a trip of the key loop, the group merge and the partition merge.  Internal: not installed.
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

// =====================================================================================================================
// The arithmetic of the decode cache step, stated once.  Every expression in which a multiply feeds an add is written
// operation by operation under `#pragma clang fp contract(off)`, with __builtin_fmaf where a fused operation is meant, so
// the bits do not depend on what a compiler would contract in the code around a call.  The operation sequences are the
// ones the kernels compiled to while each of them held these statements itself and left the choice to the compiler
// (attn_decode_part_kernel, attn_decode_merge_kernel and qknorm_rope_append_kernel of sd_decode.hip before they called
// these functions); tests/test_gpu_kv_step_golden.py holds the outputs of that build.  Where a sequence looks arbitrary
// (which products of a chain are fused), that is why: it is kept for bit compatibility, not chosen.

// ---- q/k-norm + RoPE of the 8 elements lane j (of the 16 lanes that own a head vector) holds of one head at position
// t: HF's q_norm / k_norm (the normed value rounded to bf16 twice, as HF holds it) and apply_rotary_pos_emb.  Every lane
// of the 16 runs this (the DPP row operations want whole rows active).
//   ss = p0 + p1 + ... + p7 with rounded products (exact anyway: the square of a bf16 fits fp32);
//   rs = rsqrt(fma(ss, 1/128, eps));  o = fma(n, cos, round(rot * sin)).
SD_DEV void kv_qknorm_rope8(bf16x8 raw, const bf16* __restrict__ gain, const bf16* __restrict__ cosb,
                            const bf16* __restrict__ sinb, int t, int j, float eps, float* o) {
#pragma clang fp contract(off)
  float f[8], g[8], cs[8], sn[8];
  unpack8(raw, f);
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) ss = ss + f[e] * f[e];
  ss = row16_sum(ss);
  const float rs = rsqrtf(__builtin_fmaf(ss, 1.f / 128.f, eps));
  unpack8(*(const bf16x8*)(gain + j * 8), g);
  unpack8(*(const bf16x8*)(cosb + (long)t * 128 + j * 8), cs);
  unpack8(*(const bf16x8*)(sinb + (long)t * 128 + j * 8), sn);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float n = (float)(bf16)(g[e] * (float)(bf16)(f[e] * rs));  // normed value as HF holds it (bf16)
    const float pr = row16_xor8(n);
    const float rot = (j < 8) ? -pr : pr;
    o[e] = __builtin_fmaf(n, cs[e], rot * sn[e]);
  }
}

// ---- where a lane finds its 8 elements of the keys of one partition: key k of the walk is row row0 + k of the planes
// (contiguous: row0 = b * cap; pages: row0 = (page - p) * 256, so that key = p * 256 + r lands on row r of the page).
// 8-bit pages: a row is 8 bytes per lane plus the dword of the head's four block scales, the same address for the 16
// lanes of the group; lane j's block is j >> 2.
SD_DEV int kv_page(const PageArgs& pg, int b, int p) {  // a read entry outside the pool is clamped
  return clampi(pg.table[(long)b * pg.max_pages + p], 0, pg.n_pages - 1);
}
struct KvPart {
  long off;                // element offset of the lane's chunk in row row0 (bf16 planes: elements; 8-bit: bytes)
  const uint8_t *ks, *vs;  // 8-bit pages: the scale dword of the head in row row0
};
template <bool MX>
SD_DEV KvPart kv_part(const PageArgs& pg, long row0, int Hkv, int hk, int j) {
  KvPart pt{row0 * (Hkv * 128) + hk * 128 + j * 8, nullptr, nullptr};
  if constexpr (MX) {
    const long so = row0 * Hkv * 4 + hk * 4;
    pt.ks = pg.k_scale + so;
    pt.vs = pg.v_scale + so;
  }
  return pt;
}

// ---- the 4 key rows and 4 value rows of a trip (keys key0 + 16 u) as loaded, the 8 loads issued together.  A key at or
// past nvis is not loaded and stands for zeros.  key / val: row u as fp32.  KvTripF: the rows unpacked once, for a kernel
// that scores many heads against them.
template <bool MX>
struct KvTrip {
  bf16x8 k[4], v[4];
  SD_DEV void key(int u, int, float* f) const { unpack8(k[u], f); }
  SD_DEV void val(int u, int, float* f) const { unpack8(v[u], f); }
};
template <>
struct KvTrip<true> {
  u32x2 k[4], v[4];
  uint32_t ks[4], vs[4];
  SD_DEV void key(int u, int j, float* f) const { unpack8_mx(k[u], (ks[u] >> (8 * (j >> 2))) & 255u, f); }
  SD_DEV void val(int u, int j, float* f) const { unpack8_mx(v[u], (vs[u] >> (8 * (j >> 2))) & 255u, f); }
};
struct KvTripF {
  float k[4][8], v[4][8];
  template <class T>
  SD_DEV void unpack(const T& t, int j) {
#pragma unroll
    for (int u = 0; u < 4; ++u) { t.key(u, j, k[u]); t.val(u, j, v[u]); }
  }
  SD_DEV void key(int u, int, float* f) const {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = k[u][e];
  }
  SD_DEV void val(int u, int, float* f) const {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = v[u][e];
  }
};
template <bool MX>
SD_DEV void kv_load_trip(const bf16* kp, const bf16* vp, const KvPart& pt, int Hkv, int key0, int nvis, KvTrip<MX>& t) {
  const int KD = Hkv * 128;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int key = key0 + u * 16;
    if constexpr (MX) {
      t.k[u] = t.v[u] = u32x2{0u, 0u};
      t.ks[u] = t.vs[u] = 0u;
      if (key < nvis) {
        t.k[u] = *(const u32x2*)((const uint8_t*)kp + pt.off + (long)key * KD);  // one byte per element
        t.v[u] = *(const u32x2*)((const uint8_t*)vp + pt.off + (long)key * KD);
        t.ks[u] = *(const uint32_t*)(pt.ks + (long)key * Hkv * 4);
        t.vs[u] = *(const uint32_t*)(pt.vs + (long)key * Hkv * 4);
      }
    } else {
      t.k[u] = zero8();
      t.v[u] = zero8();
      if (key < nvis) {
        t.k[u] = *(const bf16x8*)(kp + pt.off + (long)key * KD);
        t.v[u] = *(const bf16x8*)(vp + pt.off + (long)key * KD);
      }
    }
  }
}

// ---- one query head, one trip: the scores of keys key0 + 16 u against the lane's 8 elements, summed over the 16 lanes; a
// key at or past n scores -inf and gets probability exactly 0; the online softmax (log2 domain) on (m, l, acc).
//   score: fma over elements 0..3, then four rounded products added in order;
//   l = fma(l, c, p0) + p1 + p2 + p3;
//   acc, G = 2 and 4: round(a * c), then four fma;
//   acc, G = 1: fma(c, a, round(p0 * v0)), then fma for elements 0..5 and a + round(p * v) for elements 6 and 7 -- what the
//   vectoriser made of the one-head loop; kept for bit compatibility only.
template <int G, class T>
SD_DEV void kv_head_trip(const float (&qf)[8], const T& t, int j, int key0, int n, float scale_log2, float& m, float& l,
                         float (&acc)[8]) {
#pragma clang fp contract(off)
  float s[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float kf[8];
    t.key(u, j, kf);
    float d = __builtin_fmaf(qf[0], kf[0], 0.f);
#pragma unroll
    for (int e = 1; e < 4; ++e) d = __builtin_fmaf(qf[e], kf[e], d);
#pragma unroll
    for (int e = 4; e < 8; ++e) d = d + qf[e] * kf[e];
    d = row16_sum(d);
    s[u] = key0 + u * 16 < n ? d * scale_log2 : -INFINITY;
  }
  const float mn = fmaxf(fmaxf(m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
  const float c = exp2f(m - mn);
  float pu[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) pu[u] = exp2f(s[u] - mn);  // masked key: exp2(-inf) = 0
  l = ((__builtin_fmaf(l, c, pu[0]) + pu[1]) + pu[2]) + pu[3];
  float vf[4][8];
#pragma unroll
  for (int u = 0; u < 4; ++u) t.val(u, j, vf[u]);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float a = acc[e];
    if constexpr (G == 1) {
      a = __builtin_fmaf(c, a, pu[0] * vf[0][e]);
#pragma unroll
      for (int u = 1; u < 4; ++u) a = e < 6 ? __builtin_fmaf(pu[u], vf[u][e], a) : a + pu[u] * vf[u][e];
    } else {
      a = a * c;
#pragma unroll
      for (int u = 0; u < 4; ++u) a = __builtin_fmaf(pu[u], vf[u][e], a);
    }
    acc[e] = a;
  }
  m = mn;
}

// ---- the 16 group states of a head -> one partial record, through sh[16][NH][kRec]: group sg parks head hh's state,
// and after a barrier the thread of column c merges the 16 in group order (fixed) and stores the record.
//   L = fma(l_x, w_x, L) for all 16 groups;  A = fma(a_x, w_x, A) for groups 0..3, then A + round(a_x * w_x).
template <int NH>
SD_DEV void kv_group_put(float (&sh)[16][NH][kRec], int sg, int hh, int j, float m, float l, const float (&acc)[8]) {
  if (j == 0) { sh[sg][hh][0] = m; sh[sg][hh][1] = l; }
#pragma unroll
  for (int e = 0; e < 8; ++e) sh[sg][hh][4 + j * 8 + e] = acc[e];
}
template <int NH>
SD_DEV void kv_group_merge(const float (&sh)[16][NH][kRec], int hh, int c, float* rec) {
#pragma clang fp contract(off)
  float M = sh[0][hh][0];
#pragma unroll
  for (int x = 1; x < 16; ++x) M = fmaxf(M, sh[x][hh][0]);
  float L = 0.f, A = 0.f;
#pragma unroll
  for (int x = 0; x < 16; ++x) {
    const float w = exp2f(sh[x][hh][0] - M);
    L = __builtin_fmaf(sh[x][hh][1], w, L);
    A = x < 4 ? __builtin_fmaf(sh[x][hh][4 + c], w, A) : A + sh[x][hh][4 + c] * w;
  }
  rec[4 + c] = A;
  if (c == 0) { rec[0] = M; rec[1] = L; }
}

// ---- the np partial records of a head (rec: the first), merged in increasing partition order -> column c of the output
// row and, from column 0, the head's LSE (lse_h may be null).  np == 0: a zero, LSE = -inf.
//   L = fma(L, c0, round(lp * c1));  A = fma(A, c0, round(ap * c1)).
SD_DEV void kv_part_merge(const float* rec, int np, int c, bf16* o_row, float* lse_h) {
#pragma clang fp contract(off)
  float M = kNegBig, L = 0.f, A = 0.f;
  for (int p = 0; p < np; ++p, rec += kRec) {
    const float mp = rec[0], lp = rec[1], ap = rec[4 + c];
    const float mn = fmaxf(M, mp);
    const float c0 = exp2f(M - mn), c1 = exp2f(mp - mn);
    L = __builtin_fmaf(L, c0, lp * c1);
    A = __builtin_fmaf(A, c0, ap * c1);
    M = mn;
  }
  o_row[c] = (bf16)(np > 0 ? A / L : 0.f);
  if (lse_h && c == 0) *lse_h = np > 0 ? (M + log2f(L)) * 0.6931471805599453f : -INFINITY;
}

}  // namespace
