// What the decoder runners of sd_model.hip (bf16) and sd_mx.hip (MXFP8 teacher) share.  Internal: not installed, not ABI.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/sd_hip.h"

#define RUN(call) do { int e__ = (call); if (e__) return e__; } while (0)

static inline int64_t al(int64_t x) { return (x + 255) & ~(int64_t)255; }

constexpr float kSdAttnScale = 0.08838834764831845f;  // 128^-1/2

// sd_gemv.hip: the checks of sd_gemv_bf16 / sd_gemv_swiglu without a launch (0, or the code the entry would return).  The
// skinny decode step asks them for every projection before its first launch.  Internal: not exported from the library.
__attribute__((visibility("hidden"))) int sd_gemv_check(const void* x, const void* w, const void* y, const void* r,
                                                        const void* norm_gain, int M, int N, int K, int64_t ldx,
                                                        int64_t ldw, int64_t ldy, int64_t ldr);

// The checks of sd_gemv_wide_bf16 (and, with N = ldy = I and no residual, of sd_gemv_wide_swiglu) without a launch: 0, or
// the code the entry returns.  sd_gemv_wide.hip runs them in front of every launch; the wide decode step asks them for
// every projection before its first launch.  K <= 8192 = 8 waves x 32 K-steps of 32; a norm stops at sd_rmsnorm_fwd's 4096.
static inline int sd_gemv_wide_check(const void* x, const void* w, const void* y, const void* r, const void* norm_gain, int M,
                                     int N, int K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr) {
  if (!x || !w || !y || M <= 0 || N <= 0 || K <= 0) return SD_ERR_SHAPE;
  if (M > SD_GEMV_WIDE_MAX_M || (K & 31) || K > 8192 || (norm_gain && K > 4096) || N > (1 << 29)) return SD_ERR_UNSUPPORTED;
  if (ldx < K || ldw < K || ldy < N || (r && ldr < N)) return SD_ERR_UNSUPPORTED;
  if ((ldx & 7) || (ldw & 7) || ((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)norm_gain & 15))
    return SD_ERR_UNSUPPORTED;
  return 0;
}

// sd_decode.hip: cos / sin rows of the positions past[b] + t (clamped to [0, cap - 1]) gathered into [B*T,128] tables, on
// the device.  sd_qwen3_extend runs its q/k-norm + RoPE step on them with one "sequence" of B*T rows, the way the packed
// forward feeds per-token positions.  Internal: not exported from the library.
__attribute__((visibility("hidden"))) int sd_rope_rows_at(const void* cos_tab, const void* sin_tab, const int32_t* past,
                                                          void* cos_out, void* sin_out, int B, int T, int cap,
                                                          void* stream);

// sd_decode.hip: attn_decode_merge_kernel on the records of a phase 1 (B, Hq checked by the caller; np: partitions of the
// launch, for the profiler's byte count).  sd_attn_shared.hip ends its entries with it.  Internal: not exported.
__attribute__((visibility("hidden"))) int sd_attn_decode_merge_launch(const void* workspace, void* o, float* lse,
                                                                      const int32_t* len, int len_add, int cap,
                                                                      int max_len, int B, int Hq, int pstride, int np,
                                                                      void* stream);

// the shape ints every runner derives from the dims and the batch
struct SdShape {
  int M, h, I, QD, KD, QKV, QK, V, L, Hq, Hkv;
  SdShape(const sd_qwen3_dims* d, int B, int T) {
    M = B * T; h = d->hidden; I = d->inter; Hq = d->n_q; Hkv = d->n_kv;
    QD = Hq * d->head_dim; KD = Hkv * d->head_dim; QKV = QD + 2 * KD; QK = QD + KD; V = d->vocab; L = d->layers;
  }
};

// Head bases inside a token row of the two buffers a layer keeps: q and k in the normalised + rotated q|k buffer
// [M,QK], v in the raw q|k|v buffer [M,QKV] (the gradients d(q|k), d(q|k|v) have the same layout)
struct SdQkv {
  char *q, *k, *v;
  SdQkv(const SdShape& s, char* qk, char* qkv) : q(qk), k(qk + (int64_t)s.QD * 2), v(qkv + (int64_t)(s.QD + s.KD) * 2) {}
};

// sd_gemv_mx.hip: the checks of sd_gemv_mxfp8 (and, with ldy = N = I and no residual, of sd_gemv_mxfp8_swiglu) without a
// launch.  The skinny MXFP8 decode step asks them for every projection before its first launch.  Internal.
__attribute__((visibility("hidden"))) int sd_gemv_mx_check(const void* x, int64_t ldx, const void* w_q, const void* w_scale,
                                                           const void* y, int64_t ldy, const void* r, int64_t ldr, int M,
                                                           int N, int K);
// sd_gemv_mx.hip: the same for sd_gemv_mxfp8_wide / _wide_swiglu (M <= SD_GEMV_MX_WIDE_MAX_M).  The entries run them in
// front of every launch; the wide MXFP8 decode step asks them for every projection before its first launch.  Internal.
__attribute__((visibility("hidden"))) int sd_gemv_mx_wide_check(const void* x, int64_t ldx, const void* w_q,
                                                                const void* w_scale, const void* y, int64_t ldy,
                                                                const void* r, int64_t ldr, int M, int N, int K);

// Where a prefill leaves the keys and values of its layers: the cache [L][2][B][cap][Hkv*128] of sd_kvcache_bytes
// -- or, in the paged form (table != nullptr; llm_engine.py:91), the pool [L][2][n_pages][256][Hkv*128] of
// sd_kvpool_bytes: cache is then the pool's base, cap = max_pages * 256, and plane() gives the layer's pool planes.  The
// five cache kernels are reached through the members below, which pick the contiguous entry or its paged twin.
// Third form (mx; 8-bit MXFP8 pages): the pool of sd_kvpool_mx_bytes, per layer K data | K scale | V data | V scale, and
// the _paged_mx entries.  Shared by the bf16 runner entries (sd_model.hip) and the MXFP8-weight ones (sd_mx.hip).
struct KvSink {
  char* cache;
  int cap;
  // sd_qwen3_extend: the block's rows go behind past[b] cached ones and attend over the cache (nullptr: a prefill)
  const int32_t *past = nullptr, *new_len = nullptr;
  const int32_t* table = nullptr;
  int n_pages = 0, max_pages = 0;
  bool mx = false;
  // The decode step on the one-launch cache step (sd_cache_step): int32 [L][B][Hkv] at the tail of the step's acts,
  // zeroed by begin_step ahead of layer 0; layer l draws from its own [B][Hkv] slice.  nullptr: the two-entry step.
  int32_t* tickets = nullptr;
  // Paged kinds only (sd_qwen3_decode_step_shared): the decode attention of step() is sd_attn_decode_shared_paged{,_mx},
  // which reads a physical page once for all the rows of a group that map it.  Same bits; the append is unchanged.
  bool shared = false;
  // 8-bit pages: the data (u8 [n_pages][256][Hkv*128]) or scale (u8 [n_pages][256][Hkv*4]) plane of K (0) or V (1)
  char* mx_plane(const SdShape& s, int l, int which, bool scale) const {
    const int64_t data = (int64_t)n_pages * SD_KV_PAGE * s.KD;
    return cache + ((int64_t)l * 2 + which) * (data + data / 32) + (scale ? data : 0);
  }
  char* plane(const SdShape& s, int B, int l, int which) const {
    if (table) return cache + ((int64_t)l * 2 + which) * n_pages * SD_KV_PAGE * s.KD * 2;
    return cache + ((int64_t)l * 2 + which) * B * cap * s.KD * 2;
  }
  int store(const SdShape& s, int l, const void* qk, const void* qkv, const int32_t* kv_len, int B, int T, void* stream) const {
    if (mx)
      return sd_kvcache_store_paged_mx(qk, qkv, mx_plane(s, l, 0, false), mx_plane(s, l, 0, true), mx_plane(s, l, 1, false),
                                       mx_plane(s, l, 1, true), table, max_pages, n_pages, kv_len, B, T, s.Hq, s.Hkv, stream);
    char *kp = plane(s, B, l, 0), *vp = plane(s, B, l, 1);
    if (table) return sd_kvcache_store_paged(qk, qkv, kp, vp, table, max_pages, n_pages, kv_len, B, T, s.Hq, s.Hkv, stream);
    return sd_kvcache_store(qk, qkv, kp, vp, kv_len, B, T, cap, s.Hq, s.Hkv, stream);
  }
  // store_at + attention of an extend block
  int extend(const SdShape& s, int l, const void* qk, const void* qkv, void* ao, int B, int T, void* stream) const {
    if (mx) {
      char *kd = mx_plane(s, l, 0, false), *ks = mx_plane(s, l, 0, true), *vd = mx_plane(s, l, 1, false),
           *vs = mx_plane(s, l, 1, true);
      RUN(sd_kvcache_store_at_paged_mx(qk, qkv, kd, ks, vd, vs, table, max_pages, n_pages, past, new_len, B, T, s.Hq, s.Hkv,
                                       stream));
      return sd_attn_extend_paged_mx(qk, kd, ks, vd, vs, table, max_pages, n_pages, ao, nullptr, past, new_len, s.QK, s.QD, B,
                                     T, s.Hq, s.Hkv, 128, kSdAttnScale, stream);
    }
    char *kp = plane(s, B, l, 0), *vp = plane(s, B, l, 1);
    if (table) {
      RUN(sd_kvcache_store_at_paged(qk, qkv, kp, vp, table, max_pages, n_pages, past, new_len, B, T, s.Hq, s.Hkv, stream));
      return sd_attn_extend_paged(qk, kp, vp, table, max_pages, n_pages, ao, nullptr, past, new_len, s.QK, s.QD, B, T, s.Hq,
                                  s.Hkv, 128, kSdAttnScale, stream);
    }
    RUN(sd_kvcache_store_at(qk, qkv, kp, vp, past, new_len, B, T, cap, s.Hq, s.Hkv, stream));
    return sd_attn_extend(qk, kp, vp, ao, nullptr, past, new_len, s.QK, s.QD, B, T, cap, s.Hq, s.Hkv, 128, kSdAttnScale,
                          stream);
  }
  // append + attention of a decode step (q_gain, k_gain: the layer's q/k-norm gains)
  int step(const SdShape& s, int l, const void* q_gain, const void* k_gain, const void* qkv, void* q, void* ao,
           const void* cos_tab, const void* sin_tab, const int32_t* pos, void* ws, int64_t ws_bytes, int B, int max_len,
           float eps, void* stream) const {
    if (tickets) {
      sd_kv_planes pl = {};
      pl.kind = mx ? 2 : table ? 1 : 0;
      pl.k = mx ? mx_plane(s, l, 0, false) : plane(s, B, l, 0);
      pl.v = mx ? mx_plane(s, l, 1, false) : plane(s, B, l, 1);
      if (mx) { pl.k_scale = mx_plane(s, l, 0, true); pl.v_scale = mx_plane(s, l, 1, true); }
      pl.cap = cap; pl.table = table; pl.max_pages = max_pages; pl.n_pages = n_pages;
      return sd_cache_step(qkv, q_gain, k_gain, cos_tab, sin_tab, pos, &pl, ao, nullptr, ws, ws_bytes,
                           tickets + (int64_t)l * B * s.Hkv, B, max_len, s.Hq, s.Hkv, 128, eps, kSdAttnScale, stream);
    }
    if (mx) {
      char *kd = mx_plane(s, l, 0, false), *ks = mx_plane(s, l, 0, true), *vd = mx_plane(s, l, 1, false),
           *vs = mx_plane(s, l, 1, true);
      RUN(sd_qknorm_rope_append_paged_mx(qkv, q_gain, k_gain, cos_tab, sin_tab, pos, q, kd, ks, vd, vs, table, max_pages,
                                         n_pages, B, s.Hq, s.Hkv, eps, stream));
      return (shared ? sd_attn_decode_shared_paged_mx : sd_attn_decode_paged_mx)(
          q, kd, ks, vd, vs, table, max_pages, n_pages, ao, nullptr, pos, 1, ws, ws_bytes, B, max_len, s.Hq, s.Hkv, 128,
          kSdAttnScale, stream);
    }
    char *kp = plane(s, B, l, 0), *vp = plane(s, B, l, 1);
    if (table) {
      RUN(sd_qknorm_rope_append_paged(qkv, q_gain, k_gain, cos_tab, sin_tab, pos, q, kp, vp, table, max_pages, n_pages, B,
                                      s.Hq, s.Hkv, eps, stream));
      return (shared ? sd_attn_decode_shared_paged : sd_attn_decode_paged)(
          q, kp, vp, table, max_pages, n_pages, ao, nullptr, pos, 1, ws, ws_bytes, B, max_len, s.Hq, s.Hkv, 128,
          kSdAttnScale, stream);
    }
    RUN(sd_qknorm_rope_append(qkv, q_gain, k_gain, cos_tab, sin_tab, pos, q, kp, vp, B, cap, s.Hq, s.Hkv, eps, stream));
    return sd_attn_decode(q, kp, vp, ao, nullptr, pos, 1, ws, ws_bytes, B, cap, max_len, s.Hq, s.Hkv, 128, kSdAttnScale,
                          stream);
  }
  // bytes of the tickets of a decode step on sd_cache_step
  static int64_t ticket_bytes(const SdShape& s, int B) { return al((int64_t)s.L * B * s.Hkv * 4); }
  // ahead of layer 0 of a decode step: the ONE memset of the step's tickets, on the launch stream.  A launch that found
  // them poisoned (an aborted step, fresh memory) must not survive into this step, so the reducers' own reset is not
  // relied on.  Nothing without tickets.
  int begin_step(const SdShape& s, int B, void* stream) const {
    if (!tickets) return 0;
    if (hipMemsetAsync(tickets, 0, (size_t)s.L * B * s.Hkv * 4, (hipStream_t)stream) != hipSuccess) return SD_ERR_WORKSPACE;
    return 0;
  }
};

// the query heads per kv head the cache attention kernels serve (0, or the code to return)
static inline int gqa_check(const sd_qwen3_dims* d) {
  if (d->n_kv <= 0 || d->n_q % d->n_kv) return SD_ERR_SHAPE;
  const int G = d->n_q / d->n_kv;
  return G != 1 && G != 2 && G != 4 ? SD_ERR_UNSUPPORTED : 0;
}

// the checked arguments of the paged runner entries -> a KvSink over the pool (0, or the code to return)
// mx: the pool holds 8-bit pages (sd_kvpool_mx_bytes)
static inline int paged_sink(const sd_qwen3_dims* d, const sd_kv_pages* kv, KvSink* sink, bool mx = false) {
  if (!kv || !kv->pool || !kv->table || kv->n_pages <= 0 || kv->max_pages <= 0 || kv->max_pages > (1 << 22))
    return SD_ERR_SHAPE;
  // sd_kvpool_mx_bytes = sd_kvpool_bytes x 132 / 256: 128 + 4 bytes where bf16 takes 256 per (position, kv head)
  const int64_t bf16_bytes = sd_kvpool_bytes(d, kv->n_pages);
  if (kv->pool_bytes < (mx ? bf16_bytes / 256 * 132 : bf16_bytes)) return SD_ERR_WORKSPACE;
  *sink = KvSink{(char*)kv->pool, kv->max_pages * SD_KV_PAGE, nullptr, nullptr, kv->table, kv->n_pages, kv->max_pages, mx};
  return 0;
}

// the cache descriptor of any kind -> a KvSink (0, or the code to return); B is positive
static inline int ref_sink(const sd_qwen3_dims* d, const sd_kv_ref* kv, int B, KvSink* sink) {
  if (kv->kind == 1 || kv->kind == 2) return paged_sink(d, kv->pages, sink, kv->kind == 2);
  if (kv->kind != 0 || !kv->cache || kv->cap <= 0) return SD_ERR_SHAPE;
  if (kv->cache_bytes < sd_kvcache_bytes(d, B, kv->cap)) return SD_ERR_WORKSPACE;
  *sink = KvSink{(char*)kv->cache, kv->cap};
  return 0;
}

// sd_cache_step's alignment rule held against a step's buffers before the first launch: every buffer of the acts lies a
// multiple of 256 bytes behind `acts`, every plane of a layer a multiple of 16 bytes (8-bit pages: 4) behind the cache
static inline int fused_align_check(const void* acts, const KvSink& kv) {
  return (((uintptr_t)acts | (uintptr_t)kv.cache) & 15) ? SD_ERR_ALIGN : 0;
}

// every check a batch descriptor must pass before anything is launched
static inline int sd_batch_check(const sd_qwen3_batch* b) {
  if (!b || b->B <= 0 || b->T <= 0) return SD_ERR_SHAPE;
  if (b->vl && (b->kv_len || b->B != 1)) return SD_ERR_SHAPE;
  if (b->head_rows && (b->n_head_rows <= 0 || b->n_head_rows > b->B * b->T)) return SD_ERR_SHAPE;
  return SD_OK;
}

// The layer's attention: per batch row (kv_len: right padding), or per packed document when b.vl is given (B = 1, T = M)
static inline int sd_layer_attn_fwd(const SdShape& s, const sd_qwen3_batch& b, char* qk, char* qkv, char* ao, char* lse,
                                    void* stream) {
  const SdQkv f(s, qk, qkv);
  if (b.vl)
    return sd_attn_fwd_varlen(f.q, f.k, f.v, ao, (float*)lse, b.vl, s.QK, s.QK, s.QKV, s.QD, s.M, s.Hq, s.Hkv, 128,
                              kSdAttnScale, stream);
  return sd_attn_fwd(f.q, f.k, f.v, ao, (float*)lse, b.kv_len, s.QK, s.QK, s.QKV, s.QD, b.B, b.T, s.Hq, s.Hkv, 128,
                     kSdAttnScale, stream);
}

// The tail of every forward: final RMSNorm of x_last -> xn_f (rstd_f kept for the backward), then the lm_head (HF:441) on
// every row or on the gathered b.head_rows (xn_rows); logits nullable = stop after the norm.
static inline int sd_head_fwd(const sd_qwen3_dims* d, const SdShape& s, const sd_qwen3_batch& b, const void* x_last,
                              const void* final_norm, const void* lm_head, char* rstd_f, char* xn_f, char* xn_rows,
                              void* logits, void* stream) {
  RUN(sd_rmsnorm_fwd(x_last, final_norm, xn_f, (float*)rstd_f, s.M, s.h, d->eps, stream));
  if (logits && b.head_rows) {
    // lm_head only for the rows the loss will read (HF computes all B*T rows, train.py:54-55; the rows whose shifted
    // label is -100 never reach the loss, distillation_loss.py:37-45)
    RUN(sd_embedding_fwd(b.head_rows, xn_f, xn_rows, b.n_head_rows, s.h, s.M, stream));
    RUN(sd_gemm_bf16(xn_rows, lm_head, logits, nullptr, b.n_head_rows, s.V, s.h, s.h, s.h, s.V, 0, 0, 0, stream));
  } else if (logits) {
    RUN(sd_gemm_bf16(xn_f, lm_head, logits, nullptr, s.M, s.V, s.h, s.h, s.h, s.V, 0, 0, 0, stream));
  }
  return 0;
}
