// What the decoder runners of sd_model.hip (bf16) and sd_mx.hip (MXFP8 teacher) share.  Internal: not installed, not ABI.
#pragma once
#include <stdint.h>
#include "../../include/sd_hip.h"

#define RUN(call) do { int e__ = (call); if (e__) return e__; } while (0)

static inline int64_t al(int64_t x) { return (x + 255) & ~(int64_t)255; }

constexpr float kSdAttnScale = 0.08838834764831845f;  // 128^-1/2

// sd_gemv.hip: the checks of sd_gemv_bf16 / sd_gemv_swiglu without a launch (0, or the code the entry would return).  The
// skinny decode step asks them for every projection before its first launch.  Internal: not exported from the library.
__attribute__((visibility("hidden"))) int sd_gemv_check(const void* x, const void* w, const void* y, const void* r,
                                                        const void* norm_gain, int M, int N, int K, int64_t ldx,
                                                        int64_t ldw, int64_t ldy, int64_t ldr);

// sd_decode.hip: cos / sin rows of the positions past[b] + t (clamped to [0, cap - 1]) gathered into [B*T,128] tables, on
// the device.  sd_qwen3_extend runs its q/k-norm + RoPE step on them with one "sequence" of B*T rows, the way the packed
// forward feeds per-token positions.  Internal: not exported from the library.
__attribute__((visibility("hidden"))) int sd_rope_rows_at(const void* cos_tab, const void* sin_tab, const int32_t* past,
                                                          void* cos_out, void* sin_out, int B, int T, int cap,
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
