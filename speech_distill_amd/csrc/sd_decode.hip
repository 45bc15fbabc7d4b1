// KV-cache generation for gfx950: cache store / append, single-token (decode) attention, and the on-GPU sampler.
//
// What the reference runs for this (its inference engine, not the training path):
//   soulxpodcast/engine/llm_engine.py:37-76 ... the decode loop over a KV cache (vLLM / HF generate underneath)
//   soulxpodcast/config.py:107-118 ............. SamplingParams (temperature 0.6, top-k 100, top-p 0.9, repetition penalty
//                                                1.25, min/max tokens, RAS window 25 / threshold 0.2)
//   soulxpodcast/models/modules/sampler.py:136-189 the HF sampling loop with repetition-aware sampling (VALL-E 2)
// and, inside HF, transformers/generation/logits_process.py (RepetitionPenalty, MinNewTokensLength, Temperature, TopK,
// TopP) whose arithmetic the sampler restates.
//
// Cache layout: one caller-owned bf16 buffer [L][2][B][cap][Hkv*128] (K plane, V plane per layer); a row is
// [kv head][128], the layout the attention kernels read.  Every kernel below clamps the device-side lengths it is handed
// into [0, cap] before it forms an address: no access leaves [0, cap) of a cache row whatever those arrays hold.
// All stores are ordinary vector stores from plain C++.
//
// Paged form (llm_engine.py:91, vLLM's paged cache with enable_prefix_caching): the planes become pool planes
// [n_pages][256][Hkv*128] and slot s of row b lives at page table[b][s >> 8], row s & 255 (include/sd_hip.h).  The four
// cache kernels below take the page table as a TRAILING PARAMETER PACK, empty for the contiguous instantiation: its
// kernel arguments, and with them its code, stay exactly what they were before the paged instantiation existed.
//
// 8-bit paged form (MXFP8 pages, include/sd_hip.h): the pool planes hold e4m3 bytes, [n_pages][256][Hkv*128], beside
// scale planes [n_pages][256][Hkv*4] with one E8M0 byte per 32 elements of a head vector.  The pack then also carries the
// two scale planes (five arguments): the stores quantise the bf16 value the paged instantiation would have stored, the
// decode attention turns the bytes back into the bf16 numbers they stand for, in registers.
#include <math.h>
#include <stdlib.h>
#include "sd_common.cuh"
#include "../../include/sd_hip.h"
#include "sd_kv_dev.cuh"  // the partition constants, the page and 8-bit helpers, the cache step's arithmetic
#include "sd_prof.h"
#include "sd_runner.h"

#define ST ((hipStream_t)stream)

namespace {

// ------------------------------------------------------------------------------------------- cache store (prefill)
// One thread per 16 bytes of a K or V row of the layer: rows t < kv_len[b] go to cache slot t, nothing else is written.
template <class... PG>
__global__ __launch_bounds__(256) void kvcache_store_kernel(const bf16* __restrict__ qk, const bf16* __restrict__ qkv,
                                                            bf16* __restrict__ kp, bf16* __restrict__ vp,
                                                            const int32_t* __restrict__ kv_len, int B, int T, int cap,
                                                            int Hq, int Hkv, PG... pga) {
  const int cpr = Hkv * 16;  // 16-byte chunks per row
  const long total = 2l * B * T * cpr;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % cpr);
  const long r = idx / cpr;
  const int which = (int)(r / ((long)B * T));  // 0 = K, 1 = V
  const int m = (int)(r % ((long)B * T));
  const int b = m / T, t = m % T;
  const int lim = T < cap ? T : cap;
  const int n = kv_len ? clampi(kv_len[b], 0, lim) : lim;
  if (t >= n) return;
  long dst = ((long)b * cap + t) * (Hkv * 128) + c * 8;
  if constexpr (sizeof...(PG) == 5) {  // 8-bit pages: the same source row, quantised
    const PageArgs pg{pga...};
    long row;
    if (!page_slot(pg, b, t, 1, &row)) return;
    const bf16x8 v = which == 0 ? *(const bf16x8*)(qk + (long)m * (Hq + Hkv) * 128 + Hq * 128 + c * 8)
                                : *(const bf16x8*)(qkv + (long)m * (Hq + 2 * Hkv) * 128 + (Hq + Hkv) * 128 + c * 8);
    mx_store8(v, (uint8_t*)(which == 0 ? kp : vp), which == 0 ? pg.k_scale : pg.v_scale, row, Hkv, c);
    return;
  } else if constexpr (sizeof...(PG) > 0) {
    if (!page_slot(PageArgs{pga...}, b, t, Hkv * 128, &dst)) return;
    dst += c * 8;
  }
  if (which == 0) *(bf16x8*)(kp + dst) = *(const bf16x8*)(qk + (long)m * (Hq + Hkv) * 128 + Hq * 128 + c * 8);
  else *(bf16x8*)(vp + dst) = *(const bf16x8*)(qkv + (long)m * (Hq + 2 * Hkv) * 128 + (Hq + Hkv) * 128 + c * 8);
}

// The same sink at an offset (a block of T new tokens behind past[b] cached ones): row t < new_len[b] goes to slot
// past[b] + t, nothing else is written.  past is clamped to [0, cap], new_len to [0, min(T, cap - past)] first.
template <class... PG>
__global__ __launch_bounds__(256) void kvcache_store_at_kernel(const bf16* __restrict__ qk, const bf16* __restrict__ qkv,
                                                               bf16* __restrict__ kp, bf16* __restrict__ vp,
                                                               const int32_t* __restrict__ past,
                                                               const int32_t* __restrict__ new_len, int B, int T, int cap,
                                                               int Hq, int Hkv, PG... pga) {
  const int cpr = Hkv * 16;  // 16-byte chunks per row
  const long total = 2l * B * T * cpr;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % cpr);
  const long r = idx / cpr;
  const int which = (int)(r / ((long)B * T));  // 0 = K, 1 = V
  const int m = (int)(r % ((long)B * T));
  const int b = m / T, t = m % T;
  const int p0 = clampi(past[b], 0, cap);
  const int room = cap - p0;
  const int n = clampi(new_len[b], 0, T < room ? T : room);
  if (t >= n) return;
  long dst = ((long)b * cap + p0 + t) * (Hkv * 128) + c * 8;
  if constexpr (sizeof...(PG) == 5) {  // 8-bit pages: the same source row, quantised
    const PageArgs pg{pga...};
    long row;
    if (!page_slot(pg, b, p0 + t, 1, &row)) return;
    const bf16x8 v = which == 0 ? *(const bf16x8*)(qk + (long)m * (Hq + Hkv) * 128 + Hq * 128 + c * 8)
                                : *(const bf16x8*)(qkv + (long)m * (Hq + 2 * Hkv) * 128 + (Hq + Hkv) * 128 + c * 8);
    mx_store8(v, (uint8_t*)(which == 0 ? kp : vp), which == 0 ? pg.k_scale : pg.v_scale, row, Hkv, c);
    return;
  } else if constexpr (sizeof...(PG) > 0) {
    if (!page_slot(PageArgs{pga...}, b, p0 + t, Hkv * 128, &dst)) return;
    dst += c * 8;
  }
  if (which == 0) *(bf16x8*)(kp + dst) = *(const bf16x8*)(qk + (long)m * (Hq + Hkv) * 128 + Hq * 128 + c * 8);
  else *(bf16x8*)(vp + dst) = *(const bf16x8*)(qkv + (long)m * (Hq + 2 * Hkv) * 128 + (Hq + Hkv) * 128 + c * 8);
}

// cos / sin rows of the positions past[b] + t (clamped to [0, cap - 1]) of a block of T tokens per sequence, gathered
// into [B*T, 128] tables: the q/k-norm + RoPE step then takes row m of them for token m.  One thread per 16 bytes.
__global__ __launch_bounds__(256) void rope_rows_at_kernel(const bf16* __restrict__ cosb, const bf16* __restrict__ sinb,
                                                           const int32_t* __restrict__ past, bf16* __restrict__ cos_out,
                                                           bf16* __restrict__ sin_out, int B, int T, int cap) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2l * B * T * 16) return;
  const int c = (int)(idx & 15);
  const long r = idx >> 4;
  const int which = (int)(r / ((long)B * T));
  const int m = (int)(r % ((long)B * T));
  const int b = m / T, t = m % T;
  const long p = (long)clampi(past[b], 0, cap) + t;
  const long pos = p < cap - 1 ? p : cap - 1;
  if (which == 0) *(bf16x8*)(cos_out + (long)m * 128 + c * 8) = *(const bf16x8*)(cosb + pos * 128 + c * 8);
  else *(bf16x8*)(sin_out + (long)m * 128 + c * 8) = *(const bf16x8*)(sinb + pos * 128 + c * 8);
}

// last valid row of every sequence: rows[b] = b*T + clamp(kv_len[b], 1, T) - 1 (the clamp of sd_attn_fwd)
__global__ void last_rows_kernel(const int32_t* __restrict__ kv_len, int64_t* __restrict__ rows, int B, int T) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = kv_len ? clampi(kv_len[b], 1, T) : T;
  rows[b] = (int64_t)b * T + n - 1;
}

// ------------------------------------------------------------------------------- q/k norm + RoPE + append (decode)
// The arithmetic of qknorm_rope_fwd_kernel (sd_elementwise.hip) for ONE token per sequence whose position is pos[b]
// (kv_qknorm_rope8 in sd_kv_dev.cuh, shared with cache_step_kernel): q goes to q_out, k and the raw v into cache slot
// pos[b].  A head vector of 128 bf16 is owned by 16 lanes; every lane runs the norm / rotation (the DPP row operations
// want whole rows active), the head kind only picks the store.
template <class... PG>
__global__ __launch_bounds__(256) void qknorm_rope_append_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ qw,
                                                                 const bf16* __restrict__ kw, const bf16* __restrict__ cosb,
                                                                 const bf16* __restrict__ sinb,
                                                                 const int32_t* __restrict__ pos, bf16* __restrict__ q_out,
                                                                 bf16* __restrict__ kp, bf16* __restrict__ vp, int B,
                                                                 int cap, int Hq, int Hkv, float eps, PG... pga) {
  const int lane = lane_id();
  const int sub = lane >> 4, j = lane & 15;
  const int nh = Hq + 2 * Hkv;
  const long total = (long)B * nh;
  const long idx = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + sub;
  const bool ok = idx < total;
  const long id = ok ? idx : total - 1;
  const int b = (int)(id / nh), hh = (int)(id % nh);
  const int p = pos[b];
  bool inb = p >= 0 && p < cap;
  const int t = clampi(p, 0, cap - 1);
  const bf16x8 raw = *(const bf16x8*)(qkv + (long)b * nh * 128 + hh * 128 + j * 8);
  float o[8];
  kv_qknorm_rope8(raw, hh < Hq ? qw : kw, cosb, sinb, t, j, eps, o);
  if (!ok) return;
  long slot = ((long)b * cap + t) * (Hkv * 128);
  if constexpr (sizeof...(PG) == 5) {  // 8-bit pages: q as ever; the bf16 K and V the paged twin stores, quantised
    const PageArgs pg{pga...};
    if (hh < Hq) {
      *(bf16x8*)(q_out + (long)b * Hq * 128 + hh * 128 + j * 8) = pack8(o);
      return;
    }
    long row;
    if (!inb || !page_slot(pg, b, t, 1, &row)) return;
    if (hh < Hq + Hkv) mx_store8(pack8(o), (uint8_t*)kp, pg.k_scale, row, Hkv, (hh - Hq) * 16 + j);
    else mx_store8(raw, (uint8_t*)vp, pg.v_scale, row, Hkv, (hh - Hq - Hkv) * 16 + j);
    return;
  } else if constexpr (sizeof...(PG) > 0) {
    if (hh >= Hq && inb) inb = page_slot(PageArgs{pga...}, b, t, Hkv * 128, &slot);
  }
  if (hh < Hq) *(bf16x8*)(q_out + (long)b * Hq * 128 + hh * 128 + j * 8) = pack8(o);
  else if (hh < Hq + Hkv) { if (inb) *(bf16x8*)(kp + slot + (hh - Hq) * 128 + j * 8) = pack8(o); }
  else if (inb) *(bf16x8*)(vp + slot + (hh - Hq - Hkv) * 128 + j * 8) = raw;
}

// ------------------------------------------------------------------------------------------------ decode attention
// Phase 1.  One workgroup = (partition of 256 keys, kv head, sequence), serving the G query heads of the group.  A key
// row (128 bf16 = 256 bytes) is read by a 16-lane group with one 16-byte load per lane, straight into registers; the 16
// groups of the workgroup take keys base + 16 i + group, 4 keys per trip with the 8 loads of the trip issued together.
// Scores: fp32 FMAs on the vector ALU, summed over the 16 lanes by DPP; the online softmax (log2 domain) and the 8 V
// columns a lane owns stay in registers per group, and the 16 group states are merged in group order through LDS.
// Keys >= n are never loaded and get probability exactly 0.
// Paged: the partition IS a page; the workgroup reads table[b][p] once (uniform: a scalar load), after the early exit.
// The loads, the per-head arithmetic and the group merge are the device functions of sd_kv_dev.cuh, shared with
// cache_step_kernel and attn_shared_part_kernel.
template <int G, class... PG>
__global__ __launch_bounds__(256) void attn_decode_part_kernel(const bf16* __restrict__ q, const bf16* __restrict__ kp,
                                                               const bf16* __restrict__ vp, float* __restrict__ ws,
                                                               const int32_t* __restrict__ len, int len_add, int cap,
                                                               int max_len, int Hq, int Hkv, int pstride,
                                                               float scale_log2, PG... pga) {
  __shared__ __attribute__((aligned(16))) float sh[16][G][kRec];
  const int p = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int n = clampi(len[b] + len_add, 0, cap < max_len ? cap : max_len);
  if (p * kPart >= n) return;  // block-uniform: this partition holds no visible key
  const int lane = lane_id(), j = lane & 15;
  const int sg = (threadIdx.x >> 6) * 4 + (lane >> 4);
  float qf[G][8], m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    unpack8(*(const bf16x8*)(q + (long)b * Hq * 128 + (hk * G + g) * 128 + j * 8), qf[g]);
    m[g] = kNegBig;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  }
  constexpr bool MX = sizeof...(PG) == 5;  // 8-bit pages: five pack arguments
  const PageArgs pg{pga...};
  long row0 = (long)b * cap;
  if constexpr (sizeof...(PG) > 0) row0 = ((long)kv_page(pg, b, p) - p) * kPart;  // p < max_pages: p * 256 < n <= cap
  const KvPart pt = kv_part<MX>(pg, row0, Hkv, hk, j);
  for (int it = 0; it < 16; it += 4) {
    const int base = p * kPart + it * 16;
    if (base >= n) break;  // block-uniform
    KvTrip<MX> tr;
    kv_load_trip(kp, vp, pt, Hkv, base + sg, n, tr);
#pragma unroll
    for (int g = 0; g < G; ++g) kv_head_trip<G>(qf[g], tr, j, base + sg, n, scale_log2, m[g], l[g], acc[g]);
  }
#pragma unroll
  for (int g = 0; g < G; ++g) kv_group_put(sh, sg, g, j, m[g], l[g], acc[g]);
  __syncthreads();
  for (int i = threadIdx.x; i < G * 128; i += 256) {
    const int g = i >> 7, c = i & 127;
    kv_group_merge(sh, g, c, ws + (((long)b * Hq + hk * G + g) * pstride + p) * kRec);
  }
}

// Phase 2.  One workgroup per (query head, sequence), one thread per output column: the partitions [0, ceil(n/256)) are
// merged in increasing index order (kv_part_merge, shared with cache_step_kernel).  n == 0: a zero row, LSE = -inf.
__global__ __launch_bounds__(128) void attn_decode_merge_kernel(const float* __restrict__ ws, bf16* __restrict__ o,
                                                                float* __restrict__ lse, const int32_t* __restrict__ len,
                                                                int len_add, int cap, int max_len, int Hq, int pstride) {
  const int h = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
  const int n = clampi(len[b] + len_add, 0, cap < max_len ? cap : max_len);
  const int np = (n + kPart - 1) / kPart;
  kv_part_merge(ws + ((long)b * Hq + h) * pstride * kRec, np, c, o + ((long)b * Hq + h) * 128,
                lse ? lse + (long)b * Hq + h : nullptr);
}

// --------------------------------------------------------------------------------------------------------- sampler
struct SampleArgs {
  const bf16* logits;   // raw [B, ld]
  long ld;
  float* proc;          // processed scores fp32 [B, V] (penalty + EOS suppression; temperature is applied by readers)
  const int32_t* top_i; // [B, K] indices of the K largest processed scores, descending, ties to the lowest index
  float* bpart;         // [B, nblk, 2] block max / block sum of the full-vocabulary draw
  int32_t* flag;        // [B] 1 = the row's token comes from the full-vocabulary draw
  const float* u;       // [B, 2]
  int64_t* seq;         // [B, cap]
  const int32_t* prompt_len;
  int32_t* len;
  uint8_t* finished;
  int64_t* next_out;
  int32_t* pos_out;
  int B, V, cap, K, nblk;
  sd_sample_params sp;
};

SD_DEV void row_bounds(const SampleArgs& a, int b, int* n, int* np) {
  *n = clampi(a.len[b], 0, a.cap);
  *np = clampi(a.prompt_len[b], 0, *n);
}

// The per-row form (sd_sample_step_rows): every row's parameters, budget and uniform stream live in device memory.  K is
// the launch's top-k (>= 1), the stride of top_i; `sp` is unused.  flag: 1 = full draw from the processed row, 2 = from
// the raw logits (one step may need both).
struct SampleRowsArgs : SampleArgs {
  const sd_sample_params* spv;  // [B] device
  const int32_t* max_new;       // [B] device
  int u_stride, any_full, any_ras;
};

// Where a row's parameters come from: the kernels below are written once over these accessors (as the paged stores are
// over their page arguments).  SampleArgs: the one host set in the kernel arguments, exactly the code sd_sample_step had.
SD_DEV const sd_sample_params& row_params(const SampleArgs& a, int) { return a.sp; }
SD_DEV const float* row_uniforms(const SampleArgs& a, int b) { return a.u + 2 * b; }
SD_DEV int row_topk(const SampleArgs& a, const sd_sample_params&) { return a.K; }
SD_DEV int full_flag(const SampleArgs&, bool) { return 1; }
template <typename T> SD_DEV bool full_mine(const SampleArgs&, int flag) { return flag != 0; }
template <typename T> SD_DEV float full_temp(const SampleArgs&, int, float temp) { return temp; }
SD_DEV bool budget_spent(const SampleArgs&, int, int) { return false; }

// SampleRowsArgs: row b's set is loaded from device memory and every field is brought into its legal range before it is
// used (include/sd_hip.h): top_k to [0, K] (greedy: 1; 0 without a full-vocabulary launch: K), RAS off without its
// launch or its candidates, win_size to [0, cap], an EOS id >= V means none, pad to [0, V), a non-positive or NaN
// temperature / top_p / penalty to 1.
SD_DEV sd_sample_params row_params(const SampleRowsArgs& a, int b) {
  sd_sample_params s = a.spv[b];
  s.do_sample = s.do_sample != 0;
  s.top_k = s.do_sample ? clampi(s.top_k, 0, a.K) : 1;
  if (s.top_k == 0 && !a.any_full) s.top_k = a.K;
  s.use_ras = s.do_sample && s.use_ras != 0 && s.top_k > 0 && a.any_ras;
  s.win_size = clampi(s.win_size, 0, a.cap);
  if (s.eos_token_id >= a.V) s.eos_token_id = -1;
  s.pad_token_id = clampi(s.pad_token_id, 0, a.V - 1);
  if (!(s.temperature > 0.f)) s.temperature = 1.f;
  if (!(s.top_p > 0.f)) s.top_p = 1.f;
  if (!(s.repetition_penalty > 0.f)) s.repetition_penalty = 1.f;
  return s;
}
// pair g = tokens generated so far, clamped to [0, u_stride)
SD_DEV const float* row_uniforms(const SampleRowsArgs& a, int b) {
  int n, np;
  row_bounds(a, b, &n, &np);
  return a.u + ((long)b * a.u_stride + clampi(n - np, 0, a.u_stride - 1)) * 2;
}
SD_DEV int row_topk(const SampleRowsArgs&, const sd_sample_params& sp) { return sp.top_k; }
SD_DEV int full_flag(const SampleRowsArgs&, bool raw) { return raw ? 2 : 1; }
template <typename T> SD_DEV bool full_mine(const SampleRowsArgs&, int flag) { return flag == (sizeof(T) == 2 ? 2 : 1); }
template <typename T> SD_DEV float full_temp(const SampleRowsArgs& a, int b, float temp) {
  return sizeof(T) == 2 ? temp : row_params(a, b).temperature;
}
// after a commit at slot L: the row has spent its budget (np from the length before the commit)
SD_DEV bool budget_spent(const SampleRowsArgs& a, int b, int L) {
  return L + 1 - clampi(a.prompt_len[b], 0, L) >= a.max_new[b];
}

// The token of an unfinished row: appended at seq[b, len], len advanced, EOS sets finished.  A full row finishes.
template <class A>
SD_DEV void commit(const A& a, const sd_sample_params& sp, int b, long tok) {
  const int L = clampi(a.len[b], 0, a.cap);
  if (L >= a.cap) {
    a.next_out[b] = sp.pad_token_id;
    a.pos_out[b] = a.cap - 1;
    a.finished[b] = 1;
    return;
  }
  a.seq[(long)b * a.cap + L] = tok;
  a.len[b] = L + 1;
  a.next_out[b] = tok;
  a.pos_out[b] = L;
  if (sp.eos_token_id >= 0 && tok == sp.eos_token_id) a.finished[b] = 1;
  if (budget_spent(a, b, L)) a.finished[b] = 1;
}

// Step 1 + 2 of the chain (HF RepetitionPenaltyLogitsProcessor fed the generated ids, MinNewTokensLength): the raw row is
// copied to fp32, then every GENERATED token's column gets raw < 0 ? raw * p : raw / p.  The penalty reads the raw row
// and writes the copy, so a token that occurs twice is written twice with the same value: "each distinct token once".
// grid (slices, B): a workgroup owns a contiguous slice of columns and applies the tokens that fall into it.
template <class A>
__global__ __launch_bounds__(1024) void sample_scores_kernel(A a, int per) {
  const int b = blockIdx.y;
  if (a.finished[b]) return;
  const auto& sp = row_params(a, b);
  const int c0 = blockIdx.x * per, c1 = min(a.V, c0 + per);
  const bf16* raw = a.logits + (long)b * a.ld;
  float* out = a.proc + (long)b * a.V;
  for (int c = c0 + threadIdx.x * 8; c < c1; c += 1024 * 8) {
    float f[8];
    unpack8(*(const bf16x8*)(raw + c), f);
    *(f32x4*)(out + c) = f32x4{f[0], f[1], f[2], f[3]};
    *(f32x4*)(out + c + 4) = f32x4{f[4], f[5], f[6], f[7]};
  }
  __syncthreads();
  int n, np;
  row_bounds(a, b, &n, &np);
  const float pen = sp.repetition_penalty;
  if (pen != 1.0f)
    for (int i = np + threadIdx.x; i < n; i += 1024) {
      const long tok = a.seq[(long)b * a.cap + i];
      if (tok >= c0 && tok < c1) {
        const float r = (float)raw[tok];
        out[tok] = r < 0.f ? r * pen : r / pen;
      }
    }
  __syncthreads();
  const int eos = sp.eos_token_id;
  if (threadIdx.x == 0 && eos >= c0 && eos < c1 && n - np < sp.min_new_tokens) out[eos] = -INFINITY;
}

// Steps 3-6 on the top-K candidates, one workgroup per row; thread 0 walks the <= 128 candidates in descending order.
// Temperature: score / T.  Top-p (HF TopPLogitsWarper on the top-k survivors): walking up from the smallest
// probability, a candidate is dropped while the cumulative mass is <= 1 - top_p; the largest always stays.
// Draw: the first candidate whose cumulative mass (descending order, renormalised over the survivors) exceeds u.
template <class A>
__global__ __launch_bounds__(128) void sample_pick_kernel(A a) {
  __shared__ float e_s[128];
  __shared__ int id_s[128];
  const int b = blockIdx.x;
  const auto& sp = row_params(a, b);
  const int K = row_topk(a, sp);   // the row's candidates: a prefix of the launch's a.K
  int n, np;
  row_bounds(a, b, &n, &np);
  if (a.finished[b]) {
    if (threadIdx.x == 0) {
      a.next_out[b] = sp.pad_token_id;
      a.pos_out[b] = n > 0 ? n - 1 : 0;
      a.flag[b] = 0;
    }
    return;
  }
  if (K == 0) {  // no top-k: the whole processed row is the distribution (sample_full_*)
    if (threadIdx.x == 0) a.flag[b] = full_flag(a, false);
    return;
  }
  if (threadIdx.x < K) {
    const int id = clampi(a.top_i[(long)b * a.K + threadIdx.x], 0, a.V - 1);
    id_s[threadIdx.x] = id;
    e_s[threadIdx.x] = a.proc[(long)b * a.V + id] / sp.temperature;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!sp.do_sample) {
    a.flag[b] = 0;
    commit(a, sp, b, id_s[0]);
    return;
  }
  const float mx = e_s[0];
  float Z = 0.f;
  for (int k = 0; k < K; ++k) {
    e_s[k] = expf(e_s[k] - mx);
    Z += e_s[k];
  }
  int keep = K;
  if (sp.top_p < 1.0f) {
    const float drop = 1.0f - sp.top_p;
    float cum = 0.f;
    while (keep > 1) {
      cum += e_s[keep - 1] / Z;
      if (!(cum <= drop)) break;
      --keep;
    }
  }
  float Zk = 0.f;
  for (int k = 0; k < keep; ++k) Zk += e_s[k];
  auto draw = [&](float u) {
    const float target = u * Zk;
    float c = 0.f;
    for (int k = 0; k < keep; ++k) {
      c += e_s[k];
      if (target < c) return k;
    }
    return keep - 1;
  };
  if (sp.use_ras) {
    const int cand = id_s[draw(row_uniforms(a, b)[0])];
    int cnt = 0;
    const int w0 = n - sp.win_size > 0 ? n - sp.win_size : 0;
    for (int i = w0; i < n; ++i) cnt += a.seq[(long)b * a.cap + i] == cand;
    if (cnt + 1 >= sp.ras_min_count) {  // the final draw is from softmax(raw logits): sample_full_*
      a.flag[b] = full_flag(a, true);
      return;
    }
  }
  a.flag[b] = 0;
  commit(a, sp, b, id_s[draw(row_uniforms(a, b)[1])]);
}

// Full-vocabulary draw, pass 1: per block of 1024 columns the maximum and the sum of exp(x - block max), fp32, for the
// rows whose flag is set.  x = value / temp (the raw bf16 row with temp 1, or the processed fp32 row).
template <typename T, class A>
__global__ __launch_bounds__(256) void sample_full_partial_kernel(A a, const T* __restrict__ src, long ld, float temp) {
  __shared__ float red[32];
  const int b = blockIdx.y;
  if (!full_mine<T>(a, a.flag[b])) return;
  temp = full_temp<T>(a, b, temp);
  const int c0 = blockIdx.x * 1024 + threadIdx.x * 4;
  float x[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = c0 + e < a.V ? (float)src[(long)b * ld + c0 + e] / temp : -INFINITY;
  const float bm = block_max<256>(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), red);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) s += x[e] == -INFINITY ? 0.f : expf(x[e] - bm);
  s = block_sum<256>(s, red);
  if (threadIdx.x == 0) {
    a.bpart[((long)b * a.nblk + blockIdx.x) * 2] = bm;
    a.bpart[((long)b * a.nblk + blockIdx.x) * 2 + 1] = s;
  }
}

// Pass 2: scan the block sums (thread 0, block order) to the block that holds u * Z, then scan that block's 1024 columns
// in column order and take the first whose cumulative mass exceeds the target.
template <typename T, class A>
__global__ __launch_bounds__(1024) void sample_full_pick_kernel(A a, const T* __restrict__ src, long ld, float temp) {
  __shared__ float red[32];
  __shared__ float wsum[16];
  __shared__ float sel_base, sel_target, sel_M;
  __shared__ int sel_blk, first_hit;
  const int b = blockIdx.x, t = threadIdx.x;
  if (!full_mine<T>(a, a.flag[b])) return;
  temp = full_temp<T>(a, b, temp);
  const float* bp = a.bpart + (long)b * a.nblk * 2;
  float mx = -INFINITY;
  for (int i = t; i < a.nblk; i += 1024) mx = fmaxf(mx, bp[2 * i]);
  mx = block_max<1024>(mx, red);
  if (t == 0) {
    float Z = 0.f;
    for (int i = 0; i < a.nblk; ++i) Z += bp[2 * i] == -INFINITY ? 0.f : bp[2 * i + 1] * expf(bp[2 * i] - mx);
    const float target = row_uniforms(a, b)[1] * Z;
    float c = 0.f, base = 0.f;
    int blk = a.nblk - 1;  // rounding may leave the target at or past Z: the last block then
    for (int i = 0; i < a.nblk; ++i) {
      const float s = bp[2 * i] == -INFINITY ? 0.f : bp[2 * i + 1] * expf(bp[2 * i] - mx);
      base = c;
      if (target < c + s) { blk = i; break; }
      c += s;
    }
    sel_blk = blk; sel_base = base; sel_target = target; sel_M = mx;
    first_hit = 1024;
  }
  __syncthreads();
  const int col = sel_blk * 1024 + t;
  float x = col < a.V ? (float)src[(long)b * ld + col] / temp : -INFINITY;
  const float e = x == -INFINITY ? 0.f : expf(x - sel_M);
  float incl = e;  // inclusive scan over the 1024 threads: wave scan, then the wave totals in wave order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(incl, o, 64);
    if ((t & 63) >= o) incl += v;
  }
  if ((t & 63) == 63) wsum[t >> 6] = incl;
  __syncthreads();
  float before = sel_base;
  for (int w = 0; w < (t >> 6); ++w) before += wsum[w];
  const bool hit = e > 0.f && sel_target < before + incl;
  if (hit) atomicMin(&first_hit, t);
  __syncthreads();
  if (t == 0) {
    int pick = first_hit;
    if (pick >= 1024) {  // rounding left the target past the block's last column: its last column inside the vocabulary
      pick = a.V - 1 - sel_blk * 1024;
      pick = pick > 1023 ? 1023 : pick;
    }
    commit(a, row_params(a, b), b, (long)sel_blk * 1024 + pick);
  }
}

int64_t sample_ws_layout(int B, int V, int64_t* o_topi, int64_t* o_topv, int64_t* o_bpart, int64_t* o_flag) {
  auto al = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
  int64_t p = al((int64_t)B * V * 4);
  *o_topi = p; p += al((int64_t)B * 128 * 4);
  *o_topv = p; p += al((int64_t)B * 128 * 2);
  *o_bpart = p; p += al((int64_t)B * ((V + 1023) / 1024) * 8);
  *o_flag = p; p += al((int64_t)B * 4);
  return p;
}

}  // namespace

extern "C" int64_t sd_kvcache_bytes(const sd_qwen3_dims* d, int B, int cap) {
  if (!d || d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || cap <= 0) return SD_ERR_SHAPE;
  return (int64_t)d->layers * 2 * B * cap * d->n_kv * 128 * 2;
}

extern "C" int sd_kvcache_store(const void* qk, const void* qkv, void* k_plane, void* v_plane, const int32_t* kv_len, int B,
                                int T, int cap, int Hq, int Hkv, void* stream) {
  if (B <= 0 || T <= 0 || cap <= 0 || T > cap || Hq <= 0 || Hkv <= 0) return SD_ERR_SHAPE;
  const long total = 2l * B * T * Hkv * 16;
  SdProfScope prof(SD_K_MISC, 2.0 * total * 16, ST);
  SD_PROF_LABEL("kvcache_store_kernel");
  hipLaunchKernelGGL(kvcache_store_kernel<>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST, (const bf16*)qk,
                     (const bf16*)qkv, (bf16*)k_plane, (bf16*)v_plane, kv_len, B, T, cap, Hq, Hkv);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_kvcache_store_at(const void* qk, const void* qkv, void* k_plane, void* v_plane, const int32_t* past,
                                   const int32_t* new_len, int B, int T, int cap, int Hq, int Hkv, void* stream) {
  if (B <= 0 || T <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || !qk || !qkv || !k_plane || !v_plane || !past || !new_len)
    return SD_ERR_SHAPE;
  const long total = 2l * B * T * Hkv * 16;
  SdProfScope prof(SD_K_MISC, 2.0 * total * 16, ST);
  SD_PROF_LABEL("kvcache_store_at_kernel");
  hipLaunchKernelGGL(kvcache_store_at_kernel<>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST, (const bf16*)qk,
                     (const bf16*)qkv, (bf16*)k_plane, (bf16*)v_plane, past, new_len, B, T, cap, Hq, Hkv);
  SD_CHECK_LAUNCH();
  return 0;
}

// ---- paged twins of the two stores (llm_engine.py:91): same checks, same grid, the table in the trailing pack
extern "C" int64_t sd_kvpool_bytes(const sd_qwen3_dims* d, int n_pages) {
  if (!d || d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (n_pages <= 0) return SD_ERR_SHAPE;
  return (int64_t)d->layers * 2 * n_pages * SD_KV_PAGE * d->n_kv * 128 * 2;
}

extern "C" int sd_kvcache_store_paged(const void* qk, const void* qkv, void* k_pool, void* v_pool, const int32_t* table,
                                      int max_pages, int n_pages, const int32_t* kv_len, int B, int T, int Hq, int Hkv,
                                      void* stream) {
  if (!table || max_pages <= 0 || n_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  const int cap = max_pages * SD_KV_PAGE;
  if (B <= 0 || T <= 0 || T > cap || Hq <= 0 || Hkv <= 0 || !qk || !qkv || !k_pool || !v_pool) return SD_ERR_SHAPE;
  const long total = 2l * B * T * Hkv * 16;
  SdProfScope prof(SD_K_MISC, 2.0 * total * 16, ST);
  SD_PROF_LABEL("kvcache_store_kernel<paged>");
  hipLaunchKernelGGL((kvcache_store_kernel<const int32_t*, int, int>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     ST, (const bf16*)qk, (const bf16*)qkv, (bf16*)k_pool, (bf16*)v_pool, kv_len, B, T, cap, Hq, Hkv, table,
                     max_pages, n_pages);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_kvcache_store_at_paged(const void* qk, const void* qkv, void* k_pool, void* v_pool, const int32_t* table,
                                         int max_pages, int n_pages, const int32_t* past, const int32_t* new_len, int B,
                                         int T, int Hq, int Hkv, void* stream) {
  if (!table || max_pages <= 0 || n_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  if (B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || !qk || !qkv || !k_pool || !v_pool || !past || !new_len) return SD_ERR_SHAPE;
  const long total = 2l * B * T * Hkv * 16;
  SdProfScope prof(SD_K_MISC, 2.0 * total * 16, ST);
  SD_PROF_LABEL("kvcache_store_at_kernel<paged>");
  hipLaunchKernelGGL((kvcache_store_at_kernel<const int32_t*, int, int>), dim3((unsigned)((total + 255) / 256)), dim3(256),
                     0, ST, (const bf16*)qk, (const bf16*)qkv, (bf16*)k_pool, (bf16*)v_pool, past, new_len, B, T,
                     max_pages * SD_KV_PAGE, Hq, Hkv, table, max_pages, n_pages);
  SD_CHECK_LAUNCH();
  return 0;
}

// ---- 8-bit pages: the paged twins' checks and grids, the four planes of a layer and the scale planes in the pack
extern "C" int64_t sd_kvpool_mx_bytes(const sd_qwen3_dims* d, int n_pages) {
  if (!d || d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (n_pages <= 0) return SD_ERR_SHAPE;
  return (int64_t)d->layers * 2 * n_pages * SD_KV_PAGE * d->n_kv * (128 + 4);
}

#define SD_MX_PACK const int32_t*, int, int, uint8_t*, uint8_t*

extern "C" int sd_kvcache_store_paged_mx(const void* qk, const void* qkv, void* k_data, void* k_scale, void* v_data,
                                         void* v_scale, const int32_t* table, int max_pages, int n_pages,
                                         const int32_t* kv_len, int B, int T, int Hq, int Hkv, void* stream) {
  if (!table || max_pages <= 0 || n_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  const int cap = max_pages * SD_KV_PAGE;
  if (B <= 0 || T <= 0 || T > cap || Hq <= 0 || Hkv <= 0 || !qk || !qkv || !k_data || !k_scale || !v_data || !v_scale)
    return SD_ERR_SHAPE;
  const long total = 2l * B * T * Hkv * 16;
  SdProfScope prof(SD_K_MISC, 1.52 * total * 16, ST);
  SD_PROF_LABEL("kvcache_store_kernel<paged, mx>");
  hipLaunchKernelGGL((kvcache_store_kernel<SD_MX_PACK>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST,
                     (const bf16*)qk, (const bf16*)qkv, (bf16*)k_data, (bf16*)v_data, kv_len, B, T, cap, Hq, Hkv, table,
                     max_pages, n_pages, (uint8_t*)k_scale, (uint8_t*)v_scale);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_kvcache_store_at_paged_mx(const void* qk, const void* qkv, void* k_data, void* k_scale, void* v_data,
                                            void* v_scale, const int32_t* table, int max_pages, int n_pages,
                                            const int32_t* past, const int32_t* new_len, int B, int T, int Hq, int Hkv,
                                            void* stream) {
  if (!table || max_pages <= 0 || n_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  if (B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || !qk || !qkv || !k_data || !k_scale || !v_data || !v_scale || !past ||
      !new_len)
    return SD_ERR_SHAPE;
  const long total = 2l * B * T * Hkv * 16;
  SdProfScope prof(SD_K_MISC, 1.52 * total * 16, ST);
  SD_PROF_LABEL("kvcache_store_at_kernel<paged, mx>");
  hipLaunchKernelGGL((kvcache_store_at_kernel<SD_MX_PACK>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST,
                     (const bf16*)qk, (const bf16*)qkv, (bf16*)k_data, (bf16*)v_data, past, new_len, B, T,
                     max_pages * SD_KV_PAGE, Hq, Hkv, table, max_pages, n_pages, (uint8_t*)k_scale, (uint8_t*)v_scale);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_qknorm_rope_append_paged_mx(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                                              const void* sin_tab, const int32_t* pos, void* q_out, void* k_data,
                                              void* k_scale, void* v_data, void* v_scale, const int32_t* table,
                                              int max_pages, int n_pages, int B, int Hq, int Hkv, float eps, void* stream) {
  if (!table || max_pages <= 0 || n_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || !pos || !qkv || !q_out || !k_data || !k_scale || !v_data || !v_scale)
    return SD_ERR_SHAPE;
  const long items = (long)B * (Hq + 2 * Hkv);
  SdProfScope prof(SD_K_MISC, 4.0 * items * 128, ST);
  SD_PROF_LABEL("qknorm_rope_append_kernel<paged, mx>");
  hipLaunchKernelGGL((qknorm_rope_append_kernel<SD_MX_PACK>), dim3((unsigned)((items + 15) / 16)), dim3(256), 0, ST,
                     (const bf16*)qkv, (const bf16*)q_gain, (const bf16*)k_gain, (const bf16*)cos_tab,
                     (const bf16*)sin_tab, pos, (bf16*)q_out, (bf16*)k_data, (bf16*)v_data, B, max_pages * SD_KV_PAGE, Hq,
                     Hkv, eps, table, max_pages, n_pages, (uint8_t*)k_scale, (uint8_t*)v_scale);
  SD_CHECK_LAUNCH();
  return 0;
}

// internal (sd_runner.h): the gathered RoPE tables of sd_qwen3_extend
int sd_rope_rows_at(const void* cos_tab, const void* sin_tab, const int32_t* past, void* cos_out, void* sin_out, int B,
                    int T, int cap, void* stream) {
  if (B <= 0 || T <= 0 || cap <= 0 || !cos_tab || !sin_tab || !past || !cos_out || !sin_out) return SD_ERR_SHAPE;
  const long total = 2l * B * T * 16;
  SdProfScope prof(SD_K_MISC, 2.0 * total * 16, ST);
  SD_PROF_LABEL("rope_rows_at_kernel");
  hipLaunchKernelGGL(rope_rows_at_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST, (const bf16*)cos_tab,
                     (const bf16*)sin_tab, past, (bf16*)cos_out, (bf16*)sin_out, B, T, cap);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_last_rows(const int32_t* kv_len, int64_t* rows, int B, int T, void* stream) {
  if (B <= 0 || T <= 0 || !rows) return SD_ERR_SHAPE;
  hipLaunchKernelGGL(last_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, ST, kv_len, rows, B, T);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_qknorm_rope_append(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                                     const void* sin_tab, const int32_t* pos, void* q_out, void* k_plane, void* v_plane,
                                     int B, int cap, int Hq, int Hkv, float eps, void* stream) {
  if (B <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || !pos) return SD_ERR_SHAPE;
  const long items = (long)B * (Hq + 2 * Hkv);
  SdProfScope prof(SD_K_MISC, 4.0 * items * 128, ST);
  SD_PROF_LABEL("qknorm_rope_append_kernel");
  hipLaunchKernelGGL(qknorm_rope_append_kernel<>, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, ST, (const bf16*)qkv,
                     (const bf16*)q_gain, (const bf16*)k_gain, (const bf16*)cos_tab, (const bf16*)sin_tab, pos,
                     (bf16*)q_out, (bf16*)k_plane, (bf16*)v_plane, B, cap, Hq, Hkv, eps);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_qknorm_rope_append_paged(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                                           const void* sin_tab, const int32_t* pos, void* q_out, void* k_pool, void* v_pool,
                                           const int32_t* table, int max_pages, int n_pages, int B, int Hq, int Hkv,
                                           float eps, void* stream) {
  if (!table || max_pages <= 0 || n_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || !pos || !qkv || !q_out || !k_pool || !v_pool) return SD_ERR_SHAPE;
  const long items = (long)B * (Hq + 2 * Hkv);
  SdProfScope prof(SD_K_MISC, 4.0 * items * 128, ST);
  SD_PROF_LABEL("qknorm_rope_append_kernel<paged>");
  hipLaunchKernelGGL((qknorm_rope_append_kernel<const int32_t*, int, int>), dim3((unsigned)((items + 15) / 16)), dim3(256),
                     0, ST, (const bf16*)qkv, (const bf16*)q_gain, (const bf16*)k_gain, (const bf16*)cos_tab,
                     (const bf16*)sin_tab, pos, (bf16*)q_out, (bf16*)k_pool, (bf16*)v_pool, B, max_pages * SD_KV_PAGE, Hq,
                     Hkv, eps, table, max_pages, n_pages);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t sd_attn_decode_workspace_bytes(int B, int Hq, int cap) {
  if (B <= 0 || Hq <= 0 || cap <= 0) return SD_ERR_SHAPE;
  return (int64_t)B * Hq * ((cap + kPart - 1) / kPart) * kRec * 4;
}

extern "C" int sd_attn_decode(const void* q, const void* k_plane, const void* v_plane, void* o, float* lse,
                              const int32_t* len, int len_add, void* workspace, int64_t workspace_bytes, int B, int cap,
                              int max_len, int Hq, int Hkv, int head_dim, float scale, void* stream) {
  if (head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || cap <= 0 || max_len <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || !len) return SD_ERR_SHAPE;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (B > 65535 || Hkv > 65535) return SD_ERR_SHAPE;
  if (workspace_bytes < sd_attn_decode_workspace_bytes(B, Hq, cap) || !workspace) return SD_ERR_WORKSPACE;
  if (max_len > cap) max_len = cap;
  const int pstride = (cap + kPart - 1) / kPart, np = (max_len + kPart - 1) / kPart;
  const float sl2 = scale * 1.4426950408889634f;
  {
    // K and V rows of max_len keys per (sequence, kv head), read once
    SdProfScope prof(SD_K_MISC, 2.0 * B * Hkv * 256.0 * max_len, ST);
    SD_PROF_LABEL("attn_decode_part_kernel<%d>", G);
#define SD_DEC_GO(G_)                                                                                                 \
  hipLaunchKernelGGL((attn_decode_part_kernel<G_>), dim3(np, Hkv, B), dim3(256), 0, ST, (const bf16*)q,               \
                     (const bf16*)k_plane, (const bf16*)v_plane, (float*)workspace, len, len_add, cap, max_len, Hq, Hkv, \
                     pstride, sl2)
    if (G == 1) SD_DEC_GO(1); else if (G == 2) SD_DEC_GO(2); else SD_DEC_GO(4);
#undef SD_DEC_GO
    SD_CHECK_LAUNCH();
  }
  SdProfScope prof(SD_K_MISC, (double)B * Hq * np * kRec * 4, ST);
  SD_PROF_LABEL("attn_decode_merge_kernel");
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(Hq, B), dim3(128), 0, ST, (const float*)workspace, (bf16*)o, lse, len,
                     len_add, cap, max_len, Hq, pstride);
  SD_CHECK_LAUNCH();
  return 0;
}

// internal (sd_runner.h): phase 2 alone, the second launch of the three entries around it, for sd_attn_shared.hip --
// the grouped phase 1 there is finished by this very kernel
int sd_attn_decode_merge_launch(const void* workspace, void* o, float* lse, const int32_t* len, int len_add, int cap,
                                int max_len, int B, int Hq, int pstride, int np, void* stream) {
  SdProfScope prof(SD_K_MISC, (double)B * Hq * np * kRec * 4, ST);
  SD_PROF_LABEL("attn_decode_merge_kernel");
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(Hq, B), dim3(128), 0, ST, (const float*)workspace, (bf16*)o, lse, len,
                     len_add, cap, max_len, Hq, pstride);
  SD_CHECK_LAUNCH();
  return 0;
}

// The paged twin (llm_engine.py:91): phase 1 reads its page from the table, phase 2 and the workspace are the twin's.
extern "C" int sd_attn_decode_paged(const void* q, const void* k_pool, const void* v_pool, const int32_t* table,
                                    int max_pages, int n_pages, void* o, float* lse, const int32_t* len, int len_add,
                                    void* workspace, int64_t workspace_bytes, int B, int max_len, int Hq, int Hkv,
                                    int head_dim, float scale, void* stream) {
  if (head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (!table || max_pages <= 0 || n_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  if (B <= 0 || max_len <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || !len || !q || !k_pool || !v_pool || !o) return SD_ERR_SHAPE;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (B > 65535 || Hkv > 65535) return SD_ERR_SHAPE;
  const int cap = max_pages * SD_KV_PAGE;
  if (workspace_bytes < sd_attn_decode_workspace_bytes(B, Hq, cap) || !workspace) return SD_ERR_WORKSPACE;
  if (max_len > cap) max_len = cap;
  const int pstride = max_pages, np = (max_len + kPart - 1) / kPart;
  const float sl2 = scale * 1.4426950408889634f;
  {
    SdProfScope prof(SD_K_MISC, 2.0 * B * Hkv * 256.0 * max_len, ST);
    SD_PROF_LABEL("attn_decode_part_kernel<%d, paged>", G);
#define SD_DEC_GO(G_)                                                                                                  \
  hipLaunchKernelGGL((attn_decode_part_kernel<G_, const int32_t*, int, int>), dim3(np, Hkv, B), dim3(256), 0, ST,      \
                     (const bf16*)q, (const bf16*)k_pool, (const bf16*)v_pool, (float*)workspace, len, len_add, cap,   \
                     max_len, Hq, Hkv, pstride, sl2, table, max_pages, n_pages)
    if (G == 1) SD_DEC_GO(1); else if (G == 2) SD_DEC_GO(2); else SD_DEC_GO(4);
#undef SD_DEC_GO
    SD_CHECK_LAUNCH();
  }
  SdProfScope prof(SD_K_MISC, (double)B * Hq * np * kRec * 4, ST);
  SD_PROF_LABEL("attn_decode_merge_kernel");
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(Hq, B), dim3(128), 0, ST, (const float*)workspace, (bf16*)o, lse, len,
                     len_add, cap, max_len, Hq, pstride);
  SD_CHECK_LAUNCH();
  return 0;
}

// The 8-bit twin: sd_attn_decode_paged's checks, grid, workspace and merge; phase 1 reads e4m3 rows and their scales.
extern "C" int sd_attn_decode_paged_mx(const void* q, const void* k_data, const void* k_scale, const void* v_data,
                                       const void* v_scale, const int32_t* table, int max_pages, int n_pages, void* o,
                                       float* lse, const int32_t* len, int len_add, void* workspace,
                                       int64_t workspace_bytes, int B, int max_len, int Hq, int Hkv, int head_dim,
                                       float scale, void* stream) {
  if (head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (!table || max_pages <= 0 || n_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  if (B <= 0 || max_len <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || !len || !q || !k_data || !k_scale || !v_data ||
      !v_scale || !o)
    return SD_ERR_SHAPE;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (B > 65535 || Hkv > 65535) return SD_ERR_SHAPE;
  const int cap = max_pages * SD_KV_PAGE;
  if (workspace_bytes < sd_attn_decode_workspace_bytes(B, Hq, cap) || !workspace) return SD_ERR_WORKSPACE;
  if (max_len > cap) max_len = cap;
  const int pstride = max_pages, np = (max_len + kPart - 1) / kPart;
  const float sl2 = scale * 1.4426950408889634f;
  {
    SdProfScope prof(SD_K_MISC, 2.0 * B * Hkv * 132.0 * max_len, ST);
    SD_PROF_LABEL("attn_decode_part_kernel<%d, paged, mx>", G);
#define SD_DEC_GO(G_)                                                                                                  \
  hipLaunchKernelGGL((attn_decode_part_kernel<G_, SD_MX_PACK>), dim3(np, Hkv, B), dim3(256), 0, ST, (const bf16*)q,    \
                     (const bf16*)k_data, (const bf16*)v_data, (float*)workspace, len, len_add, cap, max_len, Hq, Hkv, \
                     pstride, sl2, table, max_pages, n_pages, (uint8_t*)k_scale, (uint8_t*)v_scale)
    if (G == 1) SD_DEC_GO(1); else if (G == 2) SD_DEC_GO(2); else SD_DEC_GO(4);
#undef SD_DEC_GO
    SD_CHECK_LAUNCH();
  }
  SdProfScope prof(SD_K_MISC, (double)B * Hq * np * kRec * 4, ST);
  SD_PROF_LABEL("attn_decode_merge_kernel");
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(Hq, B), dim3(128), 0, ST, (const float*)workspace, (bf16*)o, lse, len,
                     len_add, cap, max_len, Hq, pstride);
  SD_CHECK_LAUNCH();
  return 0;
}
#undef SD_MX_PACK

extern "C" int64_t sd_sample_workspace_bytes(int B, int V) {
  if (B <= 0 || V <= 0) return SD_ERR_SHAPE;
  int64_t a, b, c, d;
  return sample_ws_layout(B, V, &a, &b, &c, &d);
}

extern "C" int sd_sample_step(const void* logits, int64_t row_stride, const float* uniforms, int64_t* seq,
                              const int32_t* prompt_len, int32_t* len, uint8_t* finished, int64_t* next_out,
                              int32_t* pos_out, void* workspace, int64_t workspace_bytes, const sd_sample_params* sp, int B,
                              int V, int cap, void* stream) {
  if (!sp || !logits || !uniforms || !seq || !prompt_len || !len || !finished || !next_out || !pos_out) return SD_ERR_SHAPE;
  if (B <= 0 || B > 65535 || V <= 0 || cap <= 0 || row_stride < V) return SD_ERR_SHAPE;
  if ((V & 7) || (row_stride & 7) || ((uintptr_t)logits & 15) || ((uintptr_t)workspace & 15)) return SD_ERR_ALIGN;
  if (sp->top_k < 0 || sp->top_k > 128 || sp->top_k > V) return SD_ERR_SHAPE;
  if (sp->pad_token_id < 0 || sp->pad_token_id >= V || sp->eos_token_id >= V) return SD_ERR_SHAPE;
  if (sp->do_sample && (!(sp->temperature > 0.f) || !(sp->top_p > 0.f) || !(sp->repetition_penalty > 0.f))) return SD_ERR_SHAPE;
  // the top-p rule and RAS need the sorted top-k candidates
  if (sp->do_sample && sp->top_k == 0 && (sp->top_p < 1.0f || sp->use_ras)) return SD_ERR_UNSUPPORTED;
  if (sp->use_ras && (sp->win_size <= 0 || sp->ras_min_count <= 0)) return SD_ERR_SHAPE;
  int64_t o_topi, o_topv, o_bpart, o_flag;
  if (workspace_bytes < sample_ws_layout(B, V, &o_topi, &o_topv, &o_bpart, &o_flag) || !workspace) return SD_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  SampleArgs a;
  a.logits = (const bf16*)logits; a.ld = row_stride; a.proc = (float*)ws; a.top_i = (const int32_t*)(ws + o_topi);
  a.bpart = (float*)(ws + o_bpart); a.flag = (int32_t*)(ws + o_flag); a.u = uniforms; a.seq = seq;
  a.prompt_len = prompt_len; a.len = len; a.finished = finished; a.next_out = next_out; a.pos_out = pos_out;
  a.B = B; a.V = V; a.cap = cap; a.K = sp->do_sample ? sp->top_k : 1; a.nblk = (V + 1023) / 1024; a.sp = *sp;
  {
    SdProfScope prof(SD_K_MISC, 6.0 * B * V, ST);
    SD_PROF_LABEL("sample_scores_kernel");
    const int slices = 8, per = ((V + slices - 1) / slices + 7) & ~7;
    hipLaunchKernelGGL(sample_scores_kernel<SampleArgs>, dim3(slices, B), dim3(1024), 0, ST, a, per);
    SD_CHECK_LAUNCH();
  }
  if (a.K > 0) {
    const int rc = sd_logsoftmax_topk(a.proc, ws + o_topv, ws + o_topi, nullptr, B, V, V, a.K, SD_DTYPE_F32, stream);
    if (rc) return rc;
  }
  {
    SdProfScope prof(SD_K_MISC, 8.0 * B * 128, ST);
    SD_PROF_LABEL("sample_pick_kernel");
    hipLaunchKernelGGL(sample_pick_kernel<SampleArgs>, dim3(B), dim3(128), 0, ST, a);
    SD_CHECK_LAUNCH();
  }
  if (!sp->do_sample || (a.K > 0 && !sp->use_ras)) return 0;
  SdProfScope prof(SD_K_MISC, 2.0 * B * V, ST);
  SD_PROF_LABEL("sample_full_kernels");
  if (a.K == 0) {  // the processed row at the caller's temperature
    hipLaunchKernelGGL((sample_full_partial_kernel<float, SampleArgs>), dim3(a.nblk, B), dim3(256), 0, ST, a, (const float*)a.proc,
                       (long)V, sp->temperature);
    SD_CHECK_LAUNCH();
    hipLaunchKernelGGL((sample_full_pick_kernel<float, SampleArgs>), dim3(B), dim3(1024), 0, ST, a, (const float*)a.proc, (long)V,
                       sp->temperature);
  } else {  // RAS fallback: softmax of the raw logits
    hipLaunchKernelGGL((sample_full_partial_kernel<bf16, SampleArgs>), dim3(a.nblk, B), dim3(256), 0, ST, a, a.logits, a.ld, 1.0f);
    SD_CHECK_LAUNCH();
    hipLaunchKernelGGL((sample_full_pick_kernel<bf16, SampleArgs>), dim3(B), dim3(1024), 0, ST, a, a.logits, a.ld, 1.0f);
  }
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_sample_step_rows(const void* logits, int64_t row_stride, const float* uniforms, int u_stride, int64_t* seq,
                                   const int32_t* prompt_len, int32_t* len, uint8_t* finished, int64_t* next_out,
                                   int32_t* pos_out, void* workspace, int64_t workspace_bytes,
                                   const sd_sample_params* params, const int32_t* max_new, const sd_sample_env* env, int B,
                                   int V, int cap, void* stream) {
  if (!env || !params || !max_new || !logits || !uniforms || !seq || !prompt_len || !len || !finished || !next_out || !pos_out)
    return SD_ERR_SHAPE;
  if (B <= 0 || B > 65535 || V <= 0 || cap <= 0 || row_stride < V || u_stride <= 0) return SD_ERR_SHAPE;
  if ((V & 7) || (row_stride & 7) || ((uintptr_t)logits & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)params & 3))
    return SD_ERR_ALIGN;
  if (env->max_top_k < 0 || env->max_top_k > 128 || env->max_top_k > V) return SD_ERR_SHAPE;
  int64_t o_topi, o_topv, o_bpart, o_flag;
  if (workspace_bytes < sample_ws_layout(B, V, &o_topi, &o_topv, &o_bpart, &o_flag) || !workspace) return SD_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  const bool sampling = env->any_sample != 0;
  SampleRowsArgs a;
  a.logits = (const bf16*)logits; a.ld = row_stride; a.proc = (float*)ws; a.top_i = (const int32_t*)(ws + o_topi);
  a.bpart = (float*)(ws + o_bpart); a.flag = (int32_t*)(ws + o_flag); a.u = uniforms; a.seq = seq;
  a.prompt_len = prompt_len; a.len = len; a.finished = finished; a.next_out = next_out; a.pos_out = pos_out;
  a.B = B; a.V = V; a.cap = cap; a.nblk = (V + 1023) / 1024; a.sp = sd_sample_params{};
  // one top-K launch with the envelope's K; a greedy row takes its first candidate, so K >= 1
  a.K = sampling && env->max_top_k > 1 ? env->max_top_k : 1;
  a.spv = params; a.max_new = max_new; a.u_stride = u_stride;
  a.any_full = sampling && env->any_full; a.any_ras = sampling && env->any_ras;
  {
    SdProfScope prof(SD_K_MISC, 6.0 * B * V, ST);
    SD_PROF_LABEL("sample_scores_kernel<rows>");
    const int slices = 8, per = ((V + slices - 1) / slices + 7) & ~7;
    hipLaunchKernelGGL(sample_scores_kernel<SampleRowsArgs>, dim3(slices, B), dim3(1024), 0, ST, a, per);
    SD_CHECK_LAUNCH();
  }
  const int rc = sd_logsoftmax_topk(a.proc, ws + o_topv, ws + o_topi, nullptr, B, V, V, a.K, SD_DTYPE_F32, stream);
  if (rc) return rc;
  {
    SdProfScope prof(SD_K_MISC, 8.0 * B * 128, ST);
    SD_PROF_LABEL("sample_pick_kernel<rows>");
    hipLaunchKernelGGL(sample_pick_kernel<SampleRowsArgs>, dim3(B), dim3(128), 0, ST, a);
    SD_CHECK_LAUNCH();
  }
  if (!a.any_full && !a.any_ras) return 0;
  SdProfScope prof(SD_K_MISC, 2.0 * B * V, ST);
  SD_PROF_LABEL("sample_full_kernels<rows>");
  if (a.any_full) {  // rows flagged 1: the processed row at the row's temperature
    hipLaunchKernelGGL((sample_full_partial_kernel<float, SampleRowsArgs>), dim3(a.nblk, B), dim3(256), 0, ST, a,
                       (const float*)a.proc, (long)V, 1.0f);
    SD_CHECK_LAUNCH();
    hipLaunchKernelGGL((sample_full_pick_kernel<float, SampleRowsArgs>), dim3(B), dim3(1024), 0, ST, a,
                       (const float*)a.proc, (long)V, 1.0f);
    SD_CHECK_LAUNCH();
  }
  if (a.any_ras) {  // rows flagged 2: the RAS fallback, softmax of the raw logits
    hipLaunchKernelGGL((sample_full_partial_kernel<bf16, SampleRowsArgs>), dim3(a.nblk, B), dim3(256), 0, ST, a, a.logits,
                       a.ld, 1.0f);
    SD_CHECK_LAUNCH();
    hipLaunchKernelGGL((sample_full_pick_kernel<bf16, SampleRowsArgs>), dim3(B), dim3(1024), 0, ST, a, a.logits, a.ld,
                       1.0f);
    SD_CHECK_LAUNCH();
  }
  return 0;
}
