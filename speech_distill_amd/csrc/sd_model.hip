// Host-side runner: one C call launches the whole Qwen3 decoder forward (student or frozen teacher)
// or the whole student backward on a HIP stream, kernel after kernel, with every activation laid
// out in one caller-provided HBM buffer (288 GB per MI355X: nothing is recomputed, nothing is
// re-allocated).  Mirrors HF Qwen3ForCausalLM.forward (modeling_qwen3.py:381-441, layer 304-323)
// as the reference calls it at train.py:54 (student, with grad) and train.py:60-69 (teacher, no grad).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/sd_hip.h"
#include "sd_events.h"
#include "sd_debug.h"
#include "sd_common.cuh"
#include "sd_prof.h"
#include "sd_runner.h"

namespace {

struct Sizes : SdShape {
  int64_t x, rstd, qkv, qk, ao, lse, gu, act;
  Sizes(const sd_qwen3_dims* d, int B, int T) : SdShape(d, B, T) {
    x = al((int64_t)M * h * 2); rstd = al((int64_t)M * 4); qkv = al((int64_t)M * QKV * 2); qk = al((int64_t)M * QK * 2);
    ao = al((int64_t)M * QD * 2); lse = al((int64_t)B * Hq * T * 4); gu = al((int64_t)M * 2 * I * 2);
    act = al((int64_t)M * I * 2);
  }
  int64_t per_layer() const { return 4 * x + 2 * rstd + qkv + qk + ao + lse + gu + act; }
  int64_t tail() const { return 3 * x + rstd; }  // x_last, rstd_f, xn_f, xn_rows (head rows gathered)
  int64_t ssq() const { return al((int64_t)M * 16 * 4); }  // one set of per-tile sums of squares (folded norms)
  // activation storage by mode (sd_hip.h SD_SAVE_*): every layer's buffers | L layer inputs + two layer work sets
  // (recompute; two, because the grouped dW of layer l still reads its set while layer l-1 is recomputed) | one set
  // + a ping-pong x (inference)
  int64_t body(int save) const {
    return save == SD_SAVE_ALL ? (int64_t)L * per_layer() : save == SD_SAVE_LAYER_INPUTS ? (int64_t)L * x + 2 * per_layer()
                                                                                          : per_layer() + x;  // both inference modes
  }
};

struct LayerActs {
  char *x_in, *rstd1, *xn1, *qkv, *qk, *ao, *lse, *x_mid, *rstd2, *xn2, *gu, *act;
};

LayerActs carve(const Sizes& s, char* p) {
  LayerActs a;
  a.x_in = p; p += s.x;
  a.rstd1 = p; p += s.rstd;
  a.xn1 = p; p += s.x;
  a.qkv = p; p += s.qkv;
  a.qk = p; p += s.qk;
  a.ao = p; p += s.ao;
  a.lse = p; p += s.lse;
  a.x_mid = p; p += s.x;
  a.rstd2 = p; p += s.rstd;
  a.xn2 = p; p += s.x;
  a.gu = p; p += s.gu;
  a.act = p; p += s.act;
  return a;
}

// The buffers a layer's weight-gradient GEMMs read (dxa = gradient entering the layer, dgu, dxb, dqkv) and the gain
// partials reduced on the side stream exist twice, used by layer parity: the grouped dW launch of layer l runs on
// the side stream under the dX chain of layer l-1, which writes the other set.
struct BwdScratch {
  char *dxa[2], *dxb[2], *dqkv[2], *dgu[2], *ws_norm2[2], *ws_qk[2], *ws_norm1[2];
  char *dxn, *dqk, *dao, *delta, *dact, *ws_norm, *ws_splitk;
  int64_t total, splitk_bytes;
  BwdScratch(const Sizes& s, char* p) {
    char* p0 = p;
    for (int i = 0; i < 2; ++i) {
      dxa[i] = p; p += s.x;
      dxb[i] = p; p += s.x;
      dqkv[i] = p; p += s.qkv;
      dgu[i] = p; p += s.gu;
      ws_norm2[i] = p; p += al(sd_rmsnorm_bwd_workspace_bytes(s.M, s.h));
      ws_qk[i] = p; p += al(sd_qknorm_rope_bwd_workspace_bytes(s.M, s.Hq, s.Hkv));
      ws_norm1[i] = p; p += al(sd_rmsnorm_bwd_workspace_bytes(s.M, s.h));
    }
    dxn = p; p += s.x;
    dqk = p; p += s.qk;
    dao = p; p += s.ao;
    delta = p; p += s.lse;
    dact = p; p += s.act;
    ws_norm = p; p += al(sd_rmsnorm_bwd_workspace_bytes(s.M, s.h));
    splitk_bytes = sd_gemm_splitk_workspace_bytes(s.M, s.h, s.V);
    for (int k : {s.QKV, 2 * s.I, s.QD, s.I}) {
      const int64_t b1 = sd_gemm_splitk_workspace_bytes(s.M, s.h, k);
      splitk_bytes = b1 > splitk_bytes ? b1 : splitk_bytes;
    }
    ws_splitk = p; p += al(splitk_bytes);
    total = p - p0;
  }
};

// where layer l's buffers live in `acts` for a training forward (SD_SAVE_ALL / SD_SAVE_LAYER_INPUTS)
LayerActs layer_acts(const Sizes& s, char* base, int l, int save) {
  if (save == SD_SAVE_ALL) return carve(s, base + (int64_t)l * s.per_layer());
  LayerActs a = carve(s, base + (int64_t)s.L * s.x + (int64_t)(l & 1) * s.per_layer());
  a.x_in = base + (int64_t)l * s.x;
  return a;
}

// Where a prefill leaves the keys and values of its layers: the cache [L][2][B][cap][Hkv*128] of sd_kvcache_bytes
// -- or, in the paged form (table != nullptr; llm_engine.py:91), the pool [L][2][n_pages][256][Hkv*128] of
// sd_kvpool_bytes: cache is then the pool's base, cap = max_pages * 256, and plane() gives the layer's pool planes.  The
// five cache kernels are reached through the members below, which pick the contiguous entry or its paged twin.
struct KvSink {
  char* cache;
  int cap;
  // sd_qwen3_extend: the block's rows go behind past[b] cached ones and attend over the cache (nullptr: a prefill)
  const int32_t *past = nullptr, *new_len = nullptr;
  const int32_t* table = nullptr;
  int n_pages = 0, max_pages = 0;
  char* plane(const Sizes& s, int B, int l, int which) const {
    if (table) return cache + ((int64_t)l * 2 + which) * n_pages * SD_KV_PAGE * s.KD * 2;
    return cache + ((int64_t)l * 2 + which) * B * cap * s.KD * 2;
  }
  int store(const Sizes& s, int l, const void* qk, const void* qkv, const int32_t* kv_len, int B, int T, void* stream) const {
    char *kp = plane(s, B, l, 0), *vp = plane(s, B, l, 1);
    if (table) return sd_kvcache_store_paged(qk, qkv, kp, vp, table, max_pages, n_pages, kv_len, B, T, s.Hq, s.Hkv, stream);
    return sd_kvcache_store(qk, qkv, kp, vp, kv_len, B, T, cap, s.Hq, s.Hkv, stream);
  }
  // store_at + attention of an extend block
  int extend(const Sizes& s, int l, const void* qk, const void* qkv, void* ao, int B, int T, void* stream) const {
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
  // append + attention of a decode step
  int step(const Sizes& s, int l, const sd_qwen3_layer& w, const void* qkv, void* q, void* ao, const void* cos_tab,
           const void* sin_tab, const int32_t* pos, void* ws, int64_t ws_bytes, int B, int max_len, float eps,
           void* stream) const {
    char *kp = plane(s, B, l, 0), *vp = plane(s, B, l, 1);
    if (table) {
      RUN(sd_qknorm_rope_append_paged(qkv, w.q_gain, w.k_gain, cos_tab, sin_tab, pos, q, kp, vp, table, max_pages, n_pages,
                                      B, s.Hq, s.Hkv, eps, stream));
      return sd_attn_decode_paged(q, kp, vp, table, max_pages, n_pages, ao, nullptr, pos, 1, ws, ws_bytes, B, max_len, s.Hq,
                                  s.Hkv, 128, kSdAttnScale, stream);
    }
    RUN(sd_qknorm_rope_append(qkv, w.q_gain, w.k_gain, cos_tab, sin_tab, pos, q, kp, vp, B, cap, s.Hq, s.Hkv, eps, stream));
    return sd_attn_decode(q, kp, vp, ao, nullptr, pos, 1, ws, ws_bytes, B, cap, max_len, s.Hq, s.Hkv, 128, kSdAttnScale,
                          stream);
  }
};

// the checked arguments of the paged runner entries -> a KvSink over the pool (0, or the code to return)
int paged_sink(const sd_qwen3_dims* d, const sd_kv_pages* kv, KvSink* sink) {
  if (!kv || !kv->pool || !kv->table || kv->n_pages <= 0 || kv->max_pages <= 0 || kv->max_pages > (1 << 22))
    return SD_ERR_SHAPE;
  if (kv->pool_bytes < sd_kvpool_bytes(d, kv->n_pages)) return SD_ERR_WORKSPACE;
  *sink = KvSink{(char*)kv->pool, kv->max_pages * SD_KV_PAGE};
  sink->table = kv->table;
  sink->n_pages = kv->n_pages;
  sink->max_pages = kv->max_pages;
  return 0;
}

// One decoder layer (HF modeling_qwen3.py:227-250): a.x_in -> x_out, every intermediate into `a`.  x_out == nullptr
// stops after the SwiGLU (the backward's recompute does not need the layer output again); keep_gu: gate|up is kept
// for the backward.  sink (sd_qwen3_prefill): the layer's K / V rows below kv_len also go to planes l of the cache.
// sink->past (sd_qwen3_extend): bt's cos/sin tables hold one row per TOKEN (sd_rope_rows_at), the K / V rows t <
// new_len[b] go to slots past[b] + t and the attention is sd_attn_extend over the planes.
int layer_forward(const sd_qwen3_dims* d, const Sizes& s, const LayerActs& a, const sd_qwen3_layer& w, char* x_out,
                  bool keep_gu, const sd_qwen3_batch& bt, void* stream, const KvSink* sink = nullptr, int l = 0) {
  const int B = bt.B, T = bt.T;
  const void *cos_tab = bt.cos_tab, *sin_tab = bt.sin_tab;
  const bool extend = sink && sink->past;
  const int Trope = extend ? s.M : T;  // per-token tables: row m of them belongs to token m
  RUN(sd_rmsnorm_fwd(a.x_in, w.ln1, a.xn1, (float*)a.rstd1, s.M, s.h, d->eps, stream));
  // q|k|v projection with q/k-norm + RoPE in the GEMM epilogue (one head = one 128-column tile)
  int rc = sd_gemm_qkv_rope(a.xn1, w.wqkv, a.qkv, a.qk, w.q_gain, w.k_gain, cos_tab, sin_tab, s.M, Trope, s.Hq, s.Hkv,
                            s.h, d->eps, stream);
  if (rc == SD_ERR_UNSUPPORTED) {
    RUN(sd_gemm_bf16(a.xn1, w.wqkv, a.qkv, nullptr, s.M, s.QKV, s.h, s.h, s.h, s.QKV, 0, 0, 0, stream));
    RUN(sd_qknorm_rope_fwd(a.qkv, w.q_gain, w.k_gain, cos_tab, sin_tab, a.qk, s.M, Trope, s.Hq, s.Hkv, d->eps, stream));
  } else if (rc) {
    return rc;
  }
  if (extend) {
    RUN(sink->extend(s, l, a.qk, a.qkv, a.ao, B, T, stream));
  } else {
    if (sink) RUN(sink->store(s, l, a.qk, a.qkv, bt.kv_len, B, T, stream));
    RUN(sd_layer_attn_fwd(s, bt, a.qk, a.qkv, a.ao, a.lse, stream));
  }
  RUN(sd_gemm_bf16(a.ao, w.wo, a.x_mid, a.x_in, s.M, s.h, s.QD, s.QD, s.QD, s.h, s.h, 0, 0, stream));
  RUN(sd_rmsnorm_fwd(a.x_mid, w.ln2, a.xn2, (float*)a.rstd2, s.M, s.h, d->eps, stream));
  // gate|up projection: SwiGLU runs in the GEMM epilogue when gate|up need not be kept (no backward follows:
  // the frozen teacher).  With the 2*I-wide store as well the fused epilogue is no faster than the separate
  // elementwise pass (tests/bench_fused.py), so the student keeps the two-kernel form.
  rc = (keep_gu && !g_sd_debug.model_fuse_student_swiglu)
           ? SD_ERR_UNSUPPORTED
           : sd_gemm_swiglu(a.xn2, w.wgu, keep_gu ? a.gu : nullptr, a.act, s.M, s.I, s.h, stream);
  if (rc == SD_ERR_UNSUPPORTED) {
    RUN(sd_gemm_bf16(a.xn2, w.wgu, a.gu, nullptr, s.M, 2 * s.I, s.h, s.h, s.h, 2 * s.I, 0, 0, 0, stream));
    RUN(sd_swiglu_fwd(a.gu, a.act, s.M, s.I, stream));
  } else if (rc) {
    return rc;
  }
  if (!x_out) return 0;
  RUN(sd_gemm_bf16(a.act, w.wdown, x_out, a.x_mid, s.M, s.h, s.I, s.I, s.I, s.h, s.h, 0, 0, stream));
  return 0;
}

// The same layer for the frozen teacher with the two RMSNorm gains folded into w.wqkv / w.wgu (SD_SAVE_NONE_FOLDED,
// HF:59-64 + 252-254 / 81-83): no norm launch, no normalised copy of the row.  ssq_in: partial sums of squares of a.x_in
// (from the embedding or the previous layer's down projection); ssq_mid: scratch for those of a.x_mid; ssq_next
// (nullable): where the down projection leaves those of x_out for the next layer.  w.ln1 / w.ln2 are not read.
int layer_forward_folded(const sd_qwen3_dims* d, const Sizes& s, const LayerActs& a, const sd_qwen3_layer& w, char* x_out,
                         const sd_qwen3_batch& bt, const float* ssq_in, float* ssq_mid, float* ssq_next, void* stream) {
  RUN(sd_gemm_qkv_rope_rs(a.x_in, w.wqkv, a.qkv, a.qk, w.q_gain, w.k_gain, bt.cos_tab, bt.sin_tab, ssq_in, s.M, bt.T, s.Hq,
                          s.Hkv, s.h, d->eps, stream));
  RUN(sd_layer_attn_fwd(s, bt, a.qk, a.qkv, a.ao, a.lse, stream));
  RUN(sd_gemm_bf16_ssq(a.ao, w.wo, a.x_mid, a.x_in, ssq_mid, s.M, s.h, s.QD, s.QD, s.QD, s.h, s.h, stream));
  RUN(sd_gemm_swiglu_rs(a.x_mid, w.wgu, nullptr, a.act, ssq_mid, d->eps, s.M, s.I, s.h, stream));
  if (ssq_next) RUN(sd_gemm_bf16_ssq(a.act, w.wdown, x_out, a.x_mid, ssq_next, s.M, s.h, s.I, s.I, s.I, s.h, s.h, stream));
  else RUN(sd_gemm_bf16(a.act, w.wdown, x_out, a.x_mid, s.M, s.h, s.I, s.I, s.I, s.h, s.h, 0, 0, stream));
  return 0;
}

bool fold_supported(const sd_qwen3_dims* d) {
  const int h = d->hidden;
  return d->head_dim == 128 && (h % 512) == 0 && h / 128 <= 16 && (d->inter % 64) == 0;
}


// Stage-1 lm_head dW rows [lo, hi) with hi - lo < 8, hi = lo rounded up to 8: the rows at which the aligned GEMM of
// the SD_BWD_EMBED_ONLY backward cannot start (its operands must be 16-byte aligned).  dW[r,:] (+)= sum_k dY[k,r] X[k,:]
// for k < K in increasing k per wave, the 16 waves' partials summed in wave order: deterministic.  One 16-byte load of dY
// covers every row of the strip (they share one aligned group of 8 columns).
constexpr int kStripWaves = 16;
__global__ __launch_bounds__(1024) void head_dw_strip_kernel(const bf16* __restrict__ dY, const bf16* __restrict__ X,
                                                             bf16* dW, int lo, int hi, int ldy, int H, int K, int acc) {
  __shared__ float part[kStripWaves][512];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 512 + lane * 8;
  const int g0 = lo & ~7;
  float a[8][8];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int e = 0; e < 8; ++e) a[r][e] = 0.f;
  if (c < H) {
    for (int k = w; k < K; k += kStripWaves) {
      const bf16x8 y = *(const bf16x8*)(dY + (long)k * ldy + g0);
      const bf16x8 x = *(const bf16x8*)(X + (long)k * H + c);
#pragma unroll
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) a[r][e] += (float)y[r] * (float)x[e];
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {  // (unrolled: a[][] stays in registers)
    if (r < lo - g0 || r >= hi - g0) continue;  // block-uniform
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) part[w][lane * 8 + e] = a[r][e];
    __syncthreads();
    for (int j = threadIdx.x; j < 512; j += 1024) {
      const int cc = blockIdx.x * 512 + j;
      if (cc >= H) continue;
      float t = 0.f;
      for (int q = 0; q < kStripWaves; ++q) t += part[q][j];
      bf16* o = dW + (long)(g0 + r) * H + cc;
      *o = (bf16)(acc ? (float)*o + t : t);
    }
  }
}

int head_dw_strip(const void* dY, const void* X, void* dW, int lo, int hi, int ldy, int H, int K, int acc, void* stream) {
  if (hi <= lo) return 0;
  SdProfScope prof(SD_K_GEMM_TN, 2.0 * (hi - lo) * H * K, (hipStream_t)stream);
  SD_PROF_LABEL("head_dw_strip_kernel");
  hipLaunchKernelGGL(head_dw_strip_kernel, dim3((H + 511) / 512), dim3(1024), 0, (hipStream_t)stream, (const bf16*)dY,
                     (const bf16*)X, (bf16*)dW, lo, hi, ldy, H, K, acc);
  SD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

namespace {
std::mutex g_ev_mu;
std::vector<SdEventSet*> g_ev_free;
}  // namespace

SdEventSet* sd_lease_events() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  {
    std::lock_guard<std::mutex> lk(g_ev_mu);
    for (size_t i = 0; i < g_ev_free.size(); ++i)
      if (g_ev_free[i]->device == dev) {
        SdEventSet* s = g_ev_free[i];
        g_ev_free.erase(g_ev_free.begin() + i);
        return s;
      }
  }
  SdEventSet* s = new SdEventSet;
  s->device = dev;
  for (int i = 0; i < kSdEventsPerSet; ++i)
    if (hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming) != hipSuccess) {
      for (int j = 0; j < i; ++j) (void)hipEventDestroy(s->ev[j]);
      delete s;
      return nullptr;
    }
  return s;
}
void sd_return_events(SdEventSet* s) {
  std::lock_guard<std::mutex> lk(g_ev_mu);
  g_ev_free.push_back(s);
}

extern "C" int sd_abi_version(void) { return 2; }

extern "C" int sd_qwen3_fold_supported(const sd_qwen3_dims* d) { return d && fold_supported(d) ? 1 : 0; }

extern "C" int64_t sd_qwen3_acts_bytes(const sd_qwen3_dims* d, int B, int T, int save) {
  Sizes s(d, B, T);
  save &= ~SD_FWD_CONCURRENT;
  if (save < SD_SAVE_NONE || save > SD_SAVE_NONE_FOLDED) return SD_ERR_SHAPE;
  if (save == SD_SAVE_NONE_FOLDED) return fold_supported(d) ? s.body(SD_SAVE_NONE) + s.tail() + 2 * s.ssq() : SD_ERR_UNSUPPORTED;
  return s.body(save) + s.tail();
}

extern "C" int64_t sd_qwen3_bwd_scratch_bytes(const sd_qwen3_dims* d, int B, int T) {
  Sizes s(d, B, T);
  BwdScratch b(s, nullptr);
  return b.total;
}

// The forward of both entries: per batch row (kv_len), or per packed document when bt->vl is given (B = 1, T = M)
static int forward_impl(const sd_qwen3_dims* d, const sd_qwen3_params* p, const sd_qwen3_batch* bt, void* acts,
                        int64_t acts_bytes, void* logits, int save, void* stream, const KvSink* sink) {
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  RUN(sd_batch_check(bt));
  const int B = bt->B, T = bt->T;
  if (sink && (bt->vl || (save & ~SD_FWD_CONCURRENT) != SD_SAVE_NONE)) return SD_ERR_SHAPE;
  Sizes s(d, B, T);
  const bool concurrent = (save & SD_FWD_CONCURRENT) != 0;
  save &= ~SD_FWD_CONCURRENT;
  if (save < SD_SAVE_NONE || save > SD_SAVE_NONE_FOLDED) return SD_ERR_SHAPE;
  const bool folded = save == SD_SAVE_NONE_FOLDED;
  if (folded) {
    if (!fold_supported(d)) return SD_ERR_UNSUPPORTED;
    if (acts_bytes < sd_qwen3_acts_bytes(d, B, T, save)) return SD_ERR_WORKSPACE;
    save = SD_SAVE_NONE;  // same buffers as the plain inference forward, plus the two ssq sets behind the tail
  }
  if (acts_bytes < sd_qwen3_acts_bytes(d, B, T, save)) return SD_ERR_WORKSPACE;
  char* base = (char*)acts;
  char* tail = base + s.body(save);
  char* x_last = tail;
  char* rstd_f = tail + s.x;
  char* xn_f = rstd_f + s.rstd;
  char* xn_rows = xn_f + s.x;
  char* pong = base + s.per_layer();  // inference only
  float* ssq_a = (float*)(tail + s.tail());  // folded inference only
  float* ssq_b = (float*)(tail + s.tail() + s.ssq());

  char* x_cur = save ? layer_acts(s, base, 0, save).x_in : base;
  if (folded) RUN(sd_embedding_fwd_ssq(bt->ids, p->embed, x_cur, ssq_a, s.M, s.h, s.V, stream));
  else RUN(sd_embedding_fwd(bt->ids, p->embed, x_cur, s.M, s.h, s.V, stream));
  for (int l = 0; l < s.L; ++l) {
    LayerActs a = save ? layer_acts(s, base, l, save) : carve(s, base);
    a.x_in = x_cur;
    // read by the GEMM dispatch for every launch of this layer ("model.shared_layers": measurement, sd_hip_debug.h)
    const int lim = save ? g_sd_debug.model_shared_layers_train : g_sd_debug.model_shared_layers;
    SdSharedGpuScope shared(concurrent && (lim < 0 || l < lim) ? 1 : 0);
    char* x_out;
    if (save) x_out = (l + 1 < s.L) ? layer_acts(s, base, l + 1, save).x_in : x_last;
    else x_out = (l + 1 < s.L) ? ((x_cur == pong) ? base : pong) : x_last;
    if (folded)
      RUN(layer_forward_folded(d, s, a, p->layers_host[l], x_out, *bt, ssq_a, ssq_b, l + 1 < s.L ? ssq_a : nullptr,
                               stream));
    else
      RUN(layer_forward(d, s, a, p->layers_host[l], x_out, save != SD_SAVE_NONE, *bt, stream, sink, l));
    x_cur = x_out;
  }
  return sd_head_fwd(d, s, *bt, x_last, p->final_norm, p->lm_head, rstd_f, xn_f, xn_rows, logits, stream);
}

extern "C" int sd_qwen3_forward(const sd_qwen3_dims* d, const sd_qwen3_params* p, const sd_qwen3_batch* batch, void* acts,
                                int64_t acts_bytes, void* logits, int mode, void* stream) {
  return forward_impl(d, p, batch, acts, acts_bytes, logits, mode, stream, nullptr);
}

// The student backward.  Without SD_BWD_EMBED_ONLY: every gradient.  With it (Stage-1): the same dX chain, no per-layer
// weight / gain gradient, the lm_head dW over rows [grad_row_lo, V) only and the embedding scatter restricted to
// ids >= grad_row_lo.
extern "C" int sd_qwen3_backward(const sd_qwen3_dims* d, const sd_qwen3_params* p, const sd_qwen3_params* g,
                                 const sd_qwen3_batch* bt, void* acts, int64_t acts_bytes, void* dlogits, void* scratch,
                                 int64_t scratch_bytes, const sd_qwen3_bwd_opts* opts, void* stream) {
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  RUN(sd_batch_check(bt));
  if (!opts) return SD_ERR_SHAPE;
  const sd_qwen3_bwd_opts& o = *opts;
  const int accumulate = o.flags & ~SD_BWD_EMBED_ONLY, grad_row_lo = o.grad_row_lo;
  const bool dw = !(o.flags & SD_BWD_EMBED_ONLY);  // per-layer weight and gain gradients wanted
  void *const dx0_out = o.dx0_out, *const cb_user = o.cb_user, *const side_stream = o.side_stream;
  const sd_stage_cb on_grads_ready = o.on_grads_ready;
  const int64_t *const ids = bt->ids, *const head_rows = bt->head_rows;
  const int32_t* const kv_len = bt->kv_len;
  const sd_varlen* const vl = bt->vl;
  const void *const cos_tab = bt->cos_tab, *const sin_tab = bt->sin_tab;
  const int n_head_rows = bt->n_head_rows, B = bt->B, T = bt->T;
  if (!dw && (grad_row_lo < 0 || grad_row_lo > d->vocab || dx0_out || on_grads_ready)) return SD_ERR_SHAPE;
  if (accumulate & ~(SD_BWD_ACCUMULATE | SD_BWD_RECOMPUTE)) return SD_ERR_SHAPE;
  Sizes s(d, B, T);
  // SD_BWD_RECOMPUTE: `acts` came from a forward with SD_SAVE_LAYER_INPUTS; each layer's forward is run again from its
  // saved input right before its backward (the last layer's buffers are still those of the forward itself)
  const int save = (accumulate & SD_BWD_RECOMPUTE) ? SD_SAVE_LAYER_INPUTS : SD_SAVE_ALL;
  if (acts_bytes < sd_qwen3_acts_bytes(d, B, T, save)) return SD_ERR_WORKSPACE;
  BwdScratch b(s, (char*)scratch);
  if (scratch_bytes < b.total) return SD_ERR_WORKSPACE;
  char* base = (char*)acts;
  char* tail = base + s.body(save);
  char* x_last = tail;
  char* rstd_f = tail + s.x;
  char* xn_f = rstd_f + s.rstd;
  char* xn_rows = xn_f + s.x;
  const int acc = (accumulate & SD_BWD_ACCUMULATE) ? 1 : 0;
#define ACC(ptr) (acc ? (const void*)(ptr) : (const void*)nullptr)
  // A/B switch for measurements ("model.overlap_mask", sd_hip_debug.h): bit0 lm_head dW, bit1 gain reduces, bit2 attention
  // dQ, bit3 grouped per-layer dW, bit4 batched per-layer gain reduce (default all on)
  const int ovl = g_sd_debug.model_overlap_mask;
  hipStream_t s1 = (hipStream_t)stream, s2 = (hipStream_t)side_stream;
  SdEventLease lease;
  if (s2 && !(lease.set = sd_lease_events())) return SD_ERR_WORKSPACE;
  hipEvent_t* g_ev = lease.set ? lease.set->ev : nullptr;  // this call's events
  void* wstream = s2 ? side_stream : stream;  // where weight-gradient GEMMs go
  SdSharedGpuScope shared(s2 ? 1 : 0);  // two streams share the GPU: the persistent dW launches leave CUs to the dX chain
  // main -> side: "this buffer is final"; side -> main: "this layer's dW GEMMs have read their inputs"
#define SIGNAL(i) do { if (s2) { if (hipEventRecord(g_ev[i], s1) != hipSuccess || hipStreamWaitEvent(s2, g_ev[i], 0) != hipSuccess) return SD_ERR_WORKSPACE; } } while (0)
#define JOIN() do { if (s2) { if (hipEventRecord(g_ev[7], s2) != hipSuccess || hipStreamWaitEvent(s1, g_ev[7], 0) != hipSuccess) return SD_ERR_WORKSPACE; } } while (0)

  // lm_head: dxn = dlogits . W ; dW (+)= dlogits^T . xn_f
  const int top = (s.L - 1) & 1;  // buffer set of the last layer (the first one the backward visits)
  SIGNAL(0);  // dlogits (produced on `stream` by the caller) is final: lm_head dW runs beside lm_head dX
  int nsp = 1;
  if (!dw) {
    // Stage-1: dW of the new rows only.  The GEMM starts at the first multiple of 8 at or above grad_row_lo (16-byte
    // aligned operands); the < 8 rows before it take the strip kernel.
    const int lo = grad_row_lo, lo8 = ((lo + 7) & ~7) < s.V ? ((lo + 7) & ~7) : s.V;
    const void* xs = head_rows ? (const void*)xn_rows : (const void*)xn_f;
    const int K = head_rows ? n_head_rows : s.M;
    void* hs = (ovl & 1) ? wstream : stream;
    char* gh = (char*)g->lm_head;
    if (lo8 < s.V)
      RUN(sd_gemm_bf16((const char*)dlogits + (int64_t)lo8 * 2, xs, gh + (int64_t)lo8 * s.h * 2,
                       ACC(gh + (int64_t)lo8 * s.h * 2), s.V - lo8, s.h, K, s.V, s.h, s.h, s.h, 1, 1, hs));
    RUN(head_dw_strip(dlogits, xs, g->lm_head, lo, lo8, s.V, s.h, K, acc, hs));
  }
  if (head_rows) {
    // dlogits holds only the n_head_rows rows the forward produced; every other row of d(xn_f) is zero
    if (dw)
      RUN(sd_gemm_bf16(dlogits, xn_rows, g->lm_head, ACC(g->lm_head), s.V, s.h, n_head_rows, s.V, s.h, s.h, s.h, 1, 1,
                       (ovl & 1) ? wstream : stream));
    RUN(sd_gemm_bf16_splitk(dlogits, p->lm_head, b.dxb[top], nullptr, n_head_rows, s.h, s.V, s.V, s.h, s.h, 0, 0, 1,
                            b.ws_splitk, b.splitk_bytes, stream));
    RUN(sd_rows_scatter(b.dxb[top], head_rows, b.dxn, n_head_rows, s.M, s.h, stream));
  } else {
    if (dw)
      RUN(sd_gemm_bf16(dlogits, xn_f, g->lm_head, ACC(g->lm_head), s.V, s.h, s.M, s.V, s.h, s.h, s.h, 1, 1,
                       (ovl & 1) ? wstream : stream));
    RUN(sd_gemm_bf16_splitk_partial(dlogits, p->lm_head, b.dxn, s.M, s.h, s.V, s.V, s.h, s.h, 0, 1, b.ws_splitk,
                                    b.splitk_bytes, &nsp, stream));
  }
  if (g->embed != g->lm_head && !acc) {
    const int64_t r0 = dw ? 0 : grad_row_lo;
    if (hipMemsetAsync((char*)g->embed + r0 * s.h * 2, 0, (size_t)(s.V - r0) * s.h * 2, (hipStream_t)stream) != hipSuccess)
      return SD_ERR_WORKSPACE;
  }
  // the norm backward sums the split-K slabs itself (no separate reduce pass)
#define NORM_BWD(X, W, RSTD, DRES, DX, DW, WS, RS, EV)                                                                   \
  do {                                                                                                                   \
    if (nsp > 1) RUN(sd_rmsnorm_bwd_slabs((const float*)b.ws_splitk, nsp, X, W, RSTD, DRES, DX, DW, acc, WS, s.M, s.h, RS, \
                                          EV, stream));                                                                  \
    else RUN(sd_rmsnorm_bwd2(b.dxn, X, W, RSTD, DRES, DX, DW, acc, WS, s.M, s.h, RS, EV, stream));                         \
  } while (0)
  NORM_BWD(x_last, p->final_norm, (const float*)rstd_f, nullptr, b.dxa[top], dw ? g->final_norm : nullptr, b.ws_norm, nullptr,
           nullptr);
  JOIN();
  if (on_grads_ready) on_grads_ready(SD_STAGE_HEAD, cb_user);
  // The four weight gradients of a layer run as ONE persistent grouped launch (sd_gemm_grouped_tn: 926 vs 587 TFLOP/s
  // for four separate launches) on the side stream once the layer's dX chain has produced their inputs, i.e. under
  // the chain of the NEXT layer; that layer joins it (event) before it overwrites the gradient buffer they share,
  // and only then is the finished layer reported to the caller.  SD_OVERLAP_MASK bit 3 = 0 keeps four separate GEMMs
  // launched as their inputs appear.
  const bool grouped = dw && (ovl & 8) != 0;
  const bool batch_gains = grouped && (ovl & 16) != 0;  // bit 4: one batched gain-gradient reduce per layer
  int pending = -1;  // layer whose grouped dW is in flight on the side stream
  for (int l = s.L - 1; l >= 0; --l) {
    const int P = l & 1;
    char *dx_in = b.dxa[P], *dx_out = (l == 0 && dx0_out) ? (char*)dx0_out : b.dxa[P ^ 1];
    char *dxb = b.dxb[P], *dqkv = b.dqkv[P], *dgu = b.dgu[P];
    const LayerActs a = layer_acts(s, base, l, save);
    const sd_qwen3_layer& w = p->layers_host[l];
    static const sd_qwen3_layer kNoGrads = {};
    const sd_qwen3_layer& gw = dw ? g->layers_host[l] : kNoGrads;  // Stage-1: g->layers_host may be NULL
    // recompute: this layer's work set was last read by the weight-gradient GEMMs of layer l+2, which `stream` has
    // already waited for (the `pending` join of layer l+1 below)
    if (save == SD_SAVE_LAYER_INPUTS && l != s.L - 1)
      RUN(layer_forward(d, s, a, w, nullptr, true, *bt, stream));
    // MLP
    if (!grouped && dw) {
      SIGNAL(0);  // dx_in final
      RUN(sd_gemm_bf16(dx_in, a.act, gw.wdown, ACC(gw.wdown), s.h, s.I, s.M, s.h, s.I, s.I, s.I, 1, 1, wstream));
    }
    // d(act) = dx_in . W_down with the SwiGLU backward in the epilogue: d(act) itself never reaches HBM
    {
      const int rc = sd_gemm_swiglu_bwd(dx_in, w.wdown, a.gu, dgu, s.M, s.I, s.h, stream);
      if (rc == SD_ERR_UNSUPPORTED) {
        RUN(sd_gemm_bf16(dx_in, w.wdown, b.dact, nullptr, s.M, s.I, s.h, s.h, s.I, s.I, 0, 0, 1, stream));
        RUN(sd_swiglu_bwd(b.dact, a.gu, dgu, s.M, s.I, stream));
      } else if (rc) {
        return rc;
      }
    }
    if (!grouped && dw) SIGNAL(1);  // dgu final
    RUN(sd_gemm_bf16_splitk_partial(dgu, w.wgu, b.dxn, s.M, s.h, 2 * s.I, 2 * s.I, s.h, s.h, 0, 1, b.ws_splitk,
                                    b.splitk_bytes, &nsp, stream));
    if (!grouped && dw) RUN(sd_gemm_bf16(dgu, a.xn2, gw.wgu, ACC(gw.wgu), 2 * s.I, s.h, s.M, 2 * s.I, s.h, s.h, s.h, 1, 1, wstream));
    // gain gradients of the layer: the kernels leave per-workgroup partial sums, ONE batched reduce finishes all four
    // (input norm, post-attention norm, q gain, k gain) on the side stream once the layer's last kernel is enqueued
    NORM_BWD(a.x_mid, w.ln2, (const float*)a.rstd2, dx_in, dxb, batch_gains ? nullptr : gw.ln2, b.ws_norm2[P],
             ((ovl & 2) && dw) ? side_stream : nullptr, (s2 && dw) ? (void*)g_ev[8] : nullptr);
    if (!grouped && dw) SIGNAL(2);  // dxb final
    // attention
    // d(attention output) = dxb . Wo with delta = rowsum(dO * O) in the epilogue (one 128-column tile = one head)
    const void* o_for_delta = a.ao;
    {
      const int rc = sd_gemm_odx_delta(dxb, w.wo, b.dao, a.ao, s.QD, (float*)b.delta, s.M, T, s.Hq, s.h, stream);
      if (rc == SD_ERR_UNSUPPORTED) RUN(sd_gemm_bf16(dxb, w.wo, b.dao, nullptr, s.M, s.QD, s.h, s.h, s.QD, s.QD, 0, 0, 1, stream));
      else if (rc) return rc;
      else o_for_delta = nullptr;
    }
    if (!grouped && dw) RUN(sd_gemm_bf16(dxb, a.ao, gw.wo, ACC(gw.wo), s.h, s.QD, s.M, s.h, s.QD, s.QD, s.QD, 1, 1, wstream));
    const SdQkv f(s, a.qk, a.qkv), df(s, b.dqk, dqkv);
    if (vl)
      RUN(sd_attn_bwd_varlen(f.q, f.k, f.v, o_for_delta, b.dao, (const float*)a.lse, (float*)b.delta, df.q, df.k, df.v, vl,
                             s.QK, s.QK, s.QKV, s.QD, s.QK, s.QK, s.QKV, s.M, s.Hq, s.Hkv, 128, kSdAttnScale,
                             (ovl & 4) ? side_stream : nullptr, stream));
    else
      RUN(sd_attn_bwd2(f.q, f.k, f.v, o_for_delta, b.dao, (const float*)a.lse, (float*)b.delta, df.q, df.k, df.v, kv_len,
                       s.QK, s.QK, s.QKV, s.QD, s.QK, s.QK, s.QKV, B, T, s.Hq, s.Hkv, 128, kSdAttnScale,
                       (ovl & 4) ? side_stream : nullptr, stream));
    RUN(sd_qknorm_rope_bwd2(b.dqk, a.qkv, w.q_gain, w.k_gain, cos_tab, sin_tab, dqkv, batch_gains ? nullptr : gw.q_gain,
                            batch_gains ? nullptr : gw.k_gain, acc, b.ws_qk[P], s.M, T, s.Hq, s.Hkv, d->eps,
                            ((ovl & 2) && dw) ? side_stream : nullptr, (s2 && dw) ? (void*)g_ev[9] : nullptr, stream));
    if (dw) SIGNAL(3);  // dqkv final (and with it dx_in, dgu, dxb of this layer)
    if (grouped) {
      sd_gemm_problem pr[4] = {
          {dqkv, a.xn1, gw.wqkv, s.QKV, s.h, s.h, s.QKV, s.h},    // dW_qkv  [QKV,h]  = dqkv^T . xn1
          {dgu, a.xn2, gw.wgu, 2 * s.I, s.h, s.h, 2 * s.I, s.h},  // dW_gu   [2I,h]   = dgu^T  . xn2
          {dx_in, a.act, gw.wdown, s.h, s.I, s.I, s.h, s.I},      // dW_down [h,I]    = dx_in^T . act
          {dxb, a.ao, gw.wo, s.h, s.QD, s.QD, s.h, s.QD}};        // dW_o    [h,QD]   = dxb^T  . ao
      const int rc = sd_gemm_grouped_tn(pr, 4, s.M, acc, wstream);
      if (rc == SD_ERR_UNSUPPORTED) {
        for (const sd_gemm_problem& q : pr)
          RUN(sd_gemm_bf16(q.A, q.B, q.C, acc ? q.C : nullptr, q.M, q.N, s.M, q.lda, q.ldb, q.ldc, q.ldc, 1, 1, wstream));
      } else if (rc) {
        return rc;
      }
      if (!batch_gains && s2 && hipEventRecord(g_ev[10 + P], s2) != hipSuccess) return SD_ERR_WORKSPACE;
    } else if (dw) {
      RUN(sd_gemm_bf16(dqkv, a.xn1, gw.wqkv, ACC(gw.wqkv), s.QKV, s.h, s.M, s.QKV, s.h, s.h, s.h, 1, 1, wstream));
    }
    RUN(sd_gemm_bf16_splitk_partial(dqkv, w.wqkv, b.dxn, s.M, s.h, s.QKV, s.QKV, s.h, s.h, 0, 1, b.ws_splitk,
                                    b.splitk_bytes, &nsp, stream));
    if (grouped) {
      // the previous layer's grouped dW reads the buffer this layer is about to overwrite with its output gradient
      if (pending >= 0 && s2 && hipStreamWaitEvent(s1, g_ev[10 + (pending & 1)], 0) != hipSuccess) return SD_ERR_WORKSPACE;
    } else if (dw) {
      JOIN();  // the layer's dW GEMMs are done before their inputs are overwritten and before the callback
    }
    NORM_BWD(a.x_in, w.ln1, (const float*)a.rstd1, dxb, dx_out, batch_gains ? nullptr : gw.ln1,
             batch_gains ? b.ws_norm1[P] : b.ws_norm, nullptr, nullptr);
    if (batch_gains) {
      // the side stream (after this layer's grouped dW) waits for the partials, reduces, and only then marks the
      // layer finished: the event below now covers the weight AND the gain gradients of layer l
      if (s2 && (hipEventRecord(g_ev[6], s1) != hipSuccess || hipStreamWaitEvent(s2, g_ev[6], 0) != hipSuccess))
        return SD_ERR_WORKSPACE;
      const int nb_n = sd_rmsnorm_bwd_partial_rows(s.M, s.h), nb_q = sd_qknorm_rope_bwd_partial_rows(s.M, s.Hq, s.Hkv);
      const sd_colsum_problem cp[4] = {{(const float*)b.ws_norm2[P], gw.ln2, nb_n, s.h, s.h, acc},
                                       {(const float*)b.ws_norm1[P], gw.ln1, nb_n, s.h, s.h, acc},
                                       {(const float*)b.ws_qk[P], gw.q_gain, nb_q, 128, 256, acc},
                                       {(const float*)b.ws_qk[P] + 128, gw.k_gain, nb_q, 128, 256, acc}};
      RUN(sd_colsum_reduce_batch(cp, 4, wstream));
      if (s2 && hipEventRecord(g_ev[10 + P], s2) != hipSuccess) return SD_ERR_WORKSPACE;
    }
    if (grouped) {
      if (pending >= 0 && on_grads_ready) on_grads_ready(pending, cb_user);
      pending = l;
    } else if (on_grads_ready && dw) {
      on_grads_ready(l, cb_user);
    }
  }
  if (grouped && pending >= 0) {
    if (s2 && hipStreamWaitEvent(s1, g_ev[10 + (pending & 1)], 0) != hipSuccess) return SD_ERR_WORKSPACE;
    if (on_grads_ready) on_grads_ready(pending, cb_user);
  }
  JOIN();  // everything the side stream was given (gain reduces, dQ) before the call returns
  if (!dw) RUN(sd_embedding_bwd_range(ids, b.dxa[1], g->embed, s.M, s.h, s.V, grad_row_lo, 1.0f, stream));
  else if (!dx0_out) RUN(sd_embedding_bwd(ids, b.dxa[1], g->embed, s.M, s.h, s.V, 1.0f, stream));
  if (on_grads_ready) on_grads_ready(SD_STAGE_EMBED, cb_user);
#undef ACC
#undef NORM_BWD
#undef SIGNAL
#undef JOIN
  return 0;
}

// ------------------------------------------------------------------------------------------ KV-cache generation
// (engine/llm_engine.py:37-76: prefill the prompt once, then one token per step over the cache)
extern "C" int64_t sd_qwen3_prefill_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  const int64_t base = sd_qwen3_acts_bytes(d, B, T, SD_SAVE_NONE);
  return base < 0 ? base : al(base) + al((int64_t)B * 8);  // + the head rows (int64 [B])
}

extern "C" int sd_qwen3_prefill(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* kv_len,
                                const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes, void* cache,
                                int64_t cache_bytes, int cap, void* logits, int B, int T, void* stream) {
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || T <= 0 || cap < T || !logits || !cache) return SD_ERR_SHAPE;
  if (acts_bytes < sd_qwen3_prefill_acts_bytes(d, B, T) || cache_bytes < sd_kvcache_bytes(d, B, cap)) return SD_ERR_WORKSPACE;
  const int64_t base = al(sd_qwen3_acts_bytes(d, B, T, SD_SAVE_NONE));
  int64_t* rows = (int64_t*)((char*)acts + base);
  RUN(sd_last_rows(kv_len, rows, B, T, stream));
  const KvSink sink = {(char*)cache, cap};
  const sd_qwen3_batch bt = {ids, kv_len, nullptr, cos_tab, sin_tab, rows, B, B, T, 0};
  return forward_impl(d, p, &bt, acts, base, logits, SD_SAVE_NONE, stream, &sink);
}

// Carrying on from a live cache (soulxpodcast.py:342,378-380: one DynamicCache handed to llm.generate turn after turn, each
// turn feeding only the tokens the cache has not seen).  acts: the prefill's set, then the head rows and the gathered
// cos / sin rows of the block.
extern "C" int64_t sd_qwen3_extend_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  if (!d) return SD_ERR_SHAPE;
  const int64_t base = sd_qwen3_prefill_acts_bytes(d, B, T);
  return base < 0 ? base : al(base) + 2 * al((int64_t)B * T * 128 * 2);
}

extern "C" int sd_qwen3_extend(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* past,
                               const int32_t* new_len, const void* cos_tab, const void* sin_tab, void* acts,
                               int64_t acts_bytes, void* cache, int64_t cache_bytes, int cap, void* logits, int B, int T,
                               void* stream) {
  if (!d || !p) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || T <= 0 || cap < T || !ids || !past || !new_len || !cos_tab || !sin_tab || !acts || !logits || !cache)
    return SD_ERR_SHAPE;
  if (d->n_kv <= 0 || d->n_q % d->n_kv) return SD_ERR_SHAPE;
  const int G = d->n_q / d->n_kv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (acts_bytes < sd_qwen3_extend_acts_bytes(d, B, T) || cache_bytes < sd_kvcache_bytes(d, B, cap)) return SD_ERR_WORKSPACE;
  const int64_t base = al(sd_qwen3_acts_bytes(d, B, T, SD_SAVE_NONE));
  int64_t* rows = (int64_t*)((char*)acts + base);
  char* cos_rows = (char*)acts + al(sd_qwen3_prefill_acts_bytes(d, B, T));
  char* sin_rows = cos_rows + al((int64_t)B * T * 128 * 2);
  RUN(sd_last_rows(new_len, rows, B, T, stream));
  RUN(sd_rope_rows_at(cos_tab, sin_tab, past, cos_rows, sin_rows, B, T, cap, stream));
  KvSink sink = {(char*)cache, cap};
  sink.past = past;
  sink.new_len = new_len;
  const sd_qwen3_batch bt = {ids, nullptr, nullptr, cos_rows, sin_rows, rows, B, B, T, 0};
  return forward_impl(d, p, &bt, acts, base, logits, SD_SAVE_NONE, stream, &sink);
}

// The two block entries over a page pool (llm_engine.py:91): the twins' launches with the paged sinks.
extern "C" int64_t sd_qwen3_prefill_paged_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  return sd_qwen3_prefill_acts_bytes(d, B, T);
}

extern "C" int sd_qwen3_prefill_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                      const int32_t* kv_len, const void* cos_tab, const void* sin_tab, void* acts,
                                      int64_t acts_bytes, const sd_kv_pages* kv, void* logits, int B, int T, void* stream) {
  if (!d || !p) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  KvSink sink = {};
  RUN(paged_sink(d, kv, &sink));
  if (B <= 0 || T <= 0 || sink.cap < T || !logits || !ids || !acts) return SD_ERR_SHAPE;
  if (acts_bytes < sd_qwen3_prefill_acts_bytes(d, B, T)) return SD_ERR_WORKSPACE;
  const int64_t base = al(sd_qwen3_acts_bytes(d, B, T, SD_SAVE_NONE));
  int64_t* rows = (int64_t*)((char*)acts + base);
  RUN(sd_last_rows(kv_len, rows, B, T, stream));
  const sd_qwen3_batch bt = {ids, kv_len, nullptr, cos_tab, sin_tab, rows, B, B, T, 0};
  return forward_impl(d, p, &bt, acts, base, logits, SD_SAVE_NONE, stream, &sink);
}

extern "C" int64_t sd_qwen3_extend_paged_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  return sd_qwen3_extend_acts_bytes(d, B, T);
}

extern "C" int sd_qwen3_extend_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                     const int32_t* past, const int32_t* new_len, const void* cos_tab, const void* sin_tab,
                                     void* acts, int64_t acts_bytes, const sd_kv_pages* kv, void* logits, int B, int T,
                                     void* stream) {
  if (!d || !p) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  KvSink sink = {};
  RUN(paged_sink(d, kv, &sink));
  if (B <= 0 || T <= 0 || sink.cap < T || !ids || !past || !new_len || !cos_tab || !sin_tab || !acts || !logits)
    return SD_ERR_SHAPE;
  if (d->n_kv <= 0 || d->n_q % d->n_kv) return SD_ERR_SHAPE;
  const int G = d->n_q / d->n_kv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (acts_bytes < sd_qwen3_extend_acts_bytes(d, B, T)) return SD_ERR_WORKSPACE;
  const int64_t base = al(sd_qwen3_acts_bytes(d, B, T, SD_SAVE_NONE));
  int64_t* rows = (int64_t*)((char*)acts + base);
  char* cos_rows = (char*)acts + al(sd_qwen3_prefill_acts_bytes(d, B, T));
  char* sin_rows = cos_rows + al((int64_t)B * T * 128 * 2);
  RUN(sd_last_rows(new_len, rows, B, T, stream));
  RUN(sd_rope_rows_at(cos_tab, sin_tab, past, cos_rows, sin_rows, B, T, sink.cap, stream));
  sink.past = past;
  sink.new_len = new_len;
  const sd_qwen3_batch bt = {ids, nullptr, nullptr, cos_rows, sin_rows, rows, B, B, T, 0};
  return forward_impl(d, p, &bt, acts, base, logits, SD_SAVE_NONE, stream, &sink);
}

namespace {
struct DecodeActs {
  char *x, *x_mid, *xn, *qkv, *q, *ao, *gu, *act, *ws;
  int64_t ws_bytes, total;
  DecodeActs(const sd_qwen3_dims* d, int B, int cap, char* p) {
    const Sizes s(d, B, 1);
    char* p0 = p;
    x = p; p += s.x;
    x_mid = p; p += s.x;
    xn = p; p += s.x;
    qkv = p; p += s.qkv;
    q = p; p += s.ao;
    ao = p; p += s.ao;
    gu = p; p += s.gu;
    act = p; p += s.act;
    ws_bytes = sd_attn_decode_workspace_bytes(B, s.Hq, cap);
    ws = p; p += al(ws_bytes);
    total = p - p0;
  }
};
}  // namespace

extern "C" int64_t sd_qwen3_decode_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  if (!d || d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || cap <= 0) return SD_ERR_SHAPE;
  return DecodeActs(d, B, cap, nullptr).total;
}

namespace {
// true when every GEMV of a skinny step accepts its shape: decided for the whole step before the first launch
bool skinny_step_ok(const sd_qwen3_params* p, const Sizes& s, const DecodeActs& a, const void* logits, int B) {
  bool ok = sd_gemv_check(a.x, p->lm_head, logits, nullptr, p->final_norm, B, s.V, s.h, s.h, s.h, s.V, 0) == 0;
  for (int l = 0; ok && l < s.L; ++l) {
    const sd_qwen3_layer& w = p->layers_host[l];
    ok = sd_gemv_check(a.x, w.wqkv, a.qkv, nullptr, w.ln1, B, s.QKV, s.h, s.h, s.h, s.QKV, 0) == 0 &&
         sd_gemv_check(a.ao, w.wo, a.x_mid, a.x, nullptr, B, s.h, s.QD, s.QD, s.QD, s.h, s.h) == 0 &&
         sd_gemv_check(a.x_mid, w.wgu, a.act, nullptr, w.ln2, B, s.I, s.h, s.h, s.h, s.I, 0) == 0 &&
         sd_gemv_check(a.act, w.wdown, a.x, a.x_mid, nullptr, B, s.h, s.I, s.I, s.I, s.h, s.h) == 0;
  }
  return ok;
}
}  // namespace

namespace {
// the launches of a decode step over either kind of cache; every argument was checked by the entry
int decode_step_impl(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos, int max_len,
                     const void* cos_tab, const void* sin_tab, const KvSink& kv, const Sizes& s, const DecodeActs& a,
                     void* logits, int B, int flags, void* stream);
}  // namespace

extern "C" int sd_qwen3_decode_step_flags(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                          const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                          void* cache, int64_t cache_bytes, int cap, void* acts, int64_t acts_bytes,
                                          void* logits, int B, int flags, void* stream) {
  if (flags & ~SD_DECODE_SKINNY) return SD_ERR_SHAPE;
  if (!d || !p) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || cap <= 0 || max_len <= 0 || !ids || !pos || !logits || !cache) return SD_ERR_SHAPE;
  const Sizes s(d, B, 1);
  const DecodeActs a(d, B, cap, (char*)acts);
  if (acts_bytes < a.total || cache_bytes < sd_kvcache_bytes(d, B, cap)) return SD_ERR_WORKSPACE;
  const KvSink kv = {(char*)cache, cap};
  return decode_step_impl(d, p, ids, pos, max_len, cos_tab, sin_tab, kv, s, a, logits, B, flags, stream);
}

// sd_qwen3_decode_step_paged (llm_engine.py:91): the same launches over a page pool
extern "C" int64_t sd_qwen3_decode_step_paged_acts_bytes(const sd_qwen3_dims* d, int B, int max_pages) {
  if (max_pages <= 0 || max_pages > (1 << 22)) return SD_ERR_SHAPE;
  return sd_qwen3_decode_acts_bytes(d, B, max_pages * SD_KV_PAGE);
}

extern "C" int sd_qwen3_decode_step_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                          const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                          const sd_kv_pages* kvp, void* acts, int64_t acts_bytes, void* logits, int B,
                                          int flags, void* stream) {
  if (flags & ~SD_DECODE_SKINNY) return SD_ERR_SHAPE;
  if (!d || !p) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || max_len <= 0 || !ids || !pos || !logits || !acts) return SD_ERR_SHAPE;
  if (d->n_kv <= 0 || d->n_q % d->n_kv) return SD_ERR_SHAPE;
  const int G = d->n_q / d->n_kv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  KvSink kv = {};
  RUN(paged_sink(d, kvp, &kv));
  const Sizes s(d, B, 1);
  const DecodeActs a(d, B, kv.cap, (char*)acts);
  if (acts_bytes < a.total) return SD_ERR_WORKSPACE;
  return decode_step_impl(d, p, ids, pos, max_len, cos_tab, sin_tab, kv, s, a, logits, B, flags, stream);
}

namespace {
int decode_step_impl(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos, int max_len,
                     const void* cos_tab, const void* sin_tab, const KvSink& kv, const Sizes& s, const DecodeActs& a,
                     void* logits, int B, int flags, void* stream) {
  const bool skinny = (flags & SD_DECODE_SKINNY) && skinny_step_ok(p, s, a, logits, B);
  RUN(sd_embedding_fwd(ids, p->embed, a.x, B, s.h, s.V, stream));
  if (skinny) {
    for (int l = 0; l < s.L; ++l) {
      const sd_qwen3_layer& w = p->layers_host[l];
      RUN(sd_gemv_bf16(a.x, w.wqkv, a.qkv, nullptr, w.ln1, d->eps, B, s.QKV, s.h, s.h, s.h, s.QKV, 0, stream));
      RUN(kv.step(s, l, w, a.qkv, a.q, a.ao, cos_tab, sin_tab, pos, a.ws, a.ws_bytes, B, max_len, d->eps, stream));
      RUN(sd_gemv_bf16(a.ao, w.wo, a.x_mid, a.x, nullptr, 0.f, B, s.h, s.QD, s.QD, s.QD, s.h, s.h, stream));
      RUN(sd_gemv_swiglu(a.x_mid, w.wgu, a.act, w.ln2, d->eps, B, s.I, s.h, stream));
      RUN(sd_gemv_bf16(a.act, w.wdown, a.x, a.x_mid, nullptr, 0.f, B, s.h, s.I, s.I, s.I, s.h, s.h, stream));
    }
    RUN(sd_gemv_bf16(a.x, p->lm_head, logits, nullptr, p->final_norm, d->eps, B, s.V, s.h, s.h, s.h, s.V, 0, stream));
    return 0;
  }
  for (int l = 0; l < s.L; ++l) {
    const sd_qwen3_layer& w = p->layers_host[l];
    RUN(sd_rmsnorm_fwd(a.x, w.ln1, a.xn, nullptr, B, s.h, d->eps, stream));
    RUN(sd_gemm_bf16(a.xn, w.wqkv, a.qkv, nullptr, B, s.QKV, s.h, s.h, s.h, s.QKV, 0, 0, 0, stream));
    RUN(kv.step(s, l, w, a.qkv, a.q, a.ao, cos_tab, sin_tab, pos, a.ws, a.ws_bytes, B, max_len, d->eps, stream));
    RUN(sd_gemm_bf16(a.ao, w.wo, a.x_mid, a.x, B, s.h, s.QD, s.QD, s.QD, s.h, s.h, 0, 0, stream));
    RUN(sd_rmsnorm_fwd(a.x_mid, w.ln2, a.xn, nullptr, B, s.h, d->eps, stream));
    const int rc = sd_gemm_swiglu(a.xn, w.wgu, nullptr, a.act, B, s.I, s.h, stream);
    if (rc == SD_ERR_UNSUPPORTED) {
      RUN(sd_gemm_bf16(a.xn, w.wgu, a.gu, nullptr, B, 2 * s.I, s.h, s.h, s.h, 2 * s.I, 0, 0, 0, stream));
      RUN(sd_swiglu_fwd(a.gu, a.act, B, s.I, stream));
    } else if (rc) {
      return rc;
    }
    RUN(sd_gemm_bf16(a.act, w.wdown, a.x, a.x_mid, B, s.h, s.I, s.I, s.I, s.h, s.h, 0, 0, stream));
  }
  RUN(sd_rmsnorm_fwd(a.x, p->final_norm, a.xn, nullptr, B, s.h, d->eps, stream));
  RUN(sd_gemm_bf16(a.xn, p->lm_head, logits, nullptr, B, s.V, s.h, s.h, s.h, s.V, 0, 0, 0, stream));
  return 0;
}
}  // namespace

extern "C" int sd_qwen3_decode_step(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                    const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab, void* cache,
                                    int64_t cache_bytes, int cap, void* acts, int64_t acts_bytes, void* logits, int B,
                                    void* stream) {
  return sd_qwen3_decode_step_flags(d, p, ids, pos, max_len, cos_tab, sin_tab, cache, cache_bytes, cap, acts, acts_bytes,
                                    logits, B, 0, stream);
}
