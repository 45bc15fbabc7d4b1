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
  auto take = [&](int64_t n) { char* q = p; p += n; return q; };  // the next n bytes of the caller's buffer
  LayerActs a;
  a.x_in = take(s.x); a.rstd1 = take(s.rstd); a.xn1 = take(s.x); a.qkv = take(s.qkv); a.qk = take(s.qk);
  a.ao = take(s.ao); a.lse = take(s.lse); a.x_mid = take(s.x); a.rstd2 = take(s.rstd); a.xn2 = take(s.x);
  a.gu = take(s.gu); a.act = take(s.act);
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
    int64_t off = 0;  // (p == nullptr: a size query, no address is formed)
    auto take = [&](int64_t n) { char* q = p ? p + off : nullptr; off += n; return q; };
    const int64_t norm_ws = al(sd_rmsnorm_bwd_workspace_bytes(s.M, s.h));
    for (int i = 0; i < 2; ++i) {
      dxa[i] = take(s.x); dxb[i] = take(s.x); dqkv[i] = take(s.qkv); dgu[i] = take(s.gu);
      ws_norm2[i] = take(norm_ws);
      ws_qk[i] = take(al(sd_qknorm_rope_bwd_workspace_bytes(s.M, s.Hq, s.Hkv)));
      ws_norm1[i] = take(norm_ws);
    }
    dxn = take(s.x); dqk = take(s.qk); dao = take(s.ao); delta = take(s.lse); dact = take(s.act);
    ws_norm = take(norm_ws);
    splitk_bytes = sd_gemm_splitk_workspace_bytes(s.M, s.h, s.V);
    for (int k : {s.QKV, 2 * s.I, s.QD, s.I}) {
      const int64_t b1 = sd_gemm_splitk_workspace_bytes(s.M, s.h, k);
      splitk_bytes = b1 > splitk_bytes ? b1 : splitk_bytes;
    }
    ws_splitk = take(al(splitk_bytes));
    total = off;
  }
};

// where layer l's buffers live in `acts` for a training forward (SD_SAVE_ALL / SD_SAVE_LAYER_INPUTS)
LayerActs layer_acts(const Sizes& s, char* base, int l, int save) {
  if (save == SD_SAVE_ALL) return carve(s, base + (int64_t)l * s.per_layer());
  LayerActs a = carve(s, base + (int64_t)s.L * s.x + (int64_t)(l & 1) * s.per_layer());
  a.x_in = base + (int64_t)l * s.x;
  return a;
}

// "The fused entry, or the two-kernel form when it answers SD_ERR_UNSUPPORTED": rc is what the fused entry returned
template <class F>
int fused_or(int rc, F two_kernel_form) { return rc == SD_ERR_UNSUPPORTED ? two_kernel_form() : rc; }

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
  RUN(fused_or(sd_gemm_qkv_rope(a.xn1, w.wqkv, a.qkv, a.qk, w.q_gain, w.k_gain, cos_tab, sin_tab, s.M, Trope, s.Hq, s.Hkv, s.h,
                                d->eps, stream), [&] {
    RUN(sd_gemm_bf16(a.xn1, w.wqkv, a.qkv, nullptr, s.M, s.QKV, s.h, s.h, s.h, s.QKV, 0, 0, 0, stream));
    return sd_qknorm_rope_fwd(a.qkv, w.q_gain, w.k_gain, cos_tab, sin_tab, a.qk, s.M, Trope, s.Hq, s.Hkv, d->eps, stream);
  }));
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
  const int rc = (keep_gu && !g_sd_debug.model_fuse_student_swiglu)
                     ? SD_ERR_UNSUPPORTED
                     : sd_gemm_swiglu(a.xn2, w.wgu, keep_gu ? a.gu : nullptr, a.act, s.M, s.I, s.h, stream);
  RUN(fused_or(rc, [&] {
    RUN(sd_gemm_bf16(a.xn2, w.wgu, a.gu, nullptr, s.M, 2 * s.I, s.h, s.h, s.h, 2 * s.I, 0, 0, 0, stream));
    return sd_swiglu_fwd(a.gu, a.act, s.M, s.I, stream);
  }));
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

// what lies behind the layers' buffers in `acts`: written by the head of every forward, read again by the backward
struct Tail {
  char *x_last, *rstd_f, *xn_f, *xn_rows;  // (xn_rows: the head rows gathered)
  Tail(const Sizes& s, char* p) : x_last(p), rstd_f(p + s.x), xn_f(rstd_f + s.rstd), xn_rows(xn_f + s.x) {}
};

// ------------------------------------------------------------------------------------------------ the student backward
// The context of one sd_qwen3_backward call and the steps over it.  `stream` ("main") carries the dX chain; weight-gradient
// GEMMs and gain reduces go to the side stream when the caller gives one, ordered by the events of sd_events.h (SdBwdEvent).
struct Bwd {
  const sd_qwen3_dims* d;
  const sd_qwen3_params *p, *g;
  const sd_qwen3_batch& bt;
  const sd_qwen3_bwd_opts& o;
  const Sizes& s;
  const BwdScratch& b;
  char* acts; int save;  // the forward's activations, kept in mode `save`
  void *dlogits, *stream;
  Tail tail{s, acts + s.body(save)};
  void* wstream = o.side_stream ? o.side_stream : stream;  // where weight-gradient GEMMs go
  int acc = (o.flags & SD_BWD_ACCUMULATE) ? 1 : 0;         // add to the gradient buffers
  bool dw = !(o.flags & SD_BWD_EMBED_ONLY);                // per-layer weight and gain gradients wanted (false: Stage-1)
  // A/B switch for measurements ("model.overlap_mask", sd_hip_debug.h; default all on): bit0 lm_head dW, bit1 gain
  // reduces, bit2 attention dQ beside the main stream; bit3 the layer's four dW as one grouped launch (else `separate`:
  // four GEMMs launched as their inputs appear); bit4 one batched gain-gradient reduce per layer
  int ovl = g_sd_debug.model_overlap_mask;
  bool head_dw_beside = ovl & 1, gains_beside = (ovl & 2) && dw, dq_beside = ovl & 4, grouped = dw && (ovl & 8),
       separate = dw && !grouped, batch_gains = grouped && (ovl & 16);
  SdStreamOrder ord;
  int nsp = 1;       // live split-K slab count: what the last sd_gemm_bf16_splitk_partial left for the next norm backward
  int pending = -1;  // layer whose grouped dW is in flight on the side stream (hand_over, layer_dx_out, bwd_drain)
  const void* accp(const void* ptr) const { return acc ? ptr : nullptr; }  // the residual operand of an accumulating GEMM
  void ready(int stage) const { if (o.on_grads_ready) o.on_grads_ready(stage, o.cb_user); }
};

// One layer's view of the context.  The buffers the weight-gradient GEMMs read exist twice (BwdScratch), used by parity P.
static const sd_qwen3_layer kNoGrads = {};
enum { kDwQkv, kDwGu, kDwDown, kDwO };
struct BwdLayer {
  const Bwd& c;
  int l, P = l & 1;
  char *dx_in = c.b.dxa[P], *dx_out = (l == 0 && c.o.dx0_out) ? (char*)c.o.dx0_out : c.b.dxa[P ^ 1];
  char *dxb = c.b.dxb[P], *dqkv = c.b.dqkv[P], *dgu = c.b.dgu[P];
  LayerActs a = layer_acts(c.s, c.acts, l, c.save);
  const sd_qwen3_layer &w = c.p->layers_host[l], &gw = c.dw ? c.g->layers_host[l] : kNoGrads;  // Stage-1: g->layers_host may be NULL
  // the layer's weight gradients dW [M,N] (+)= dY^T . X over the s.M tokens, in grouped-launch order
  sd_gemm_problem pr[4] = {
      {dqkv, a.xn1, gw.wqkv, c.s.QKV, c.s.h, c.s.h, c.s.QKV, c.s.h},    // dW_qkv  [QKV,h]  = dqkv^T . xn1
      {dgu, a.xn2, gw.wgu, 2 * c.s.I, c.s.h, c.s.h, 2 * c.s.I, c.s.h},  // dW_gu   [2I,h]   = dgu^T  . xn2
      {dx_in, a.act, gw.wdown, c.s.h, c.s.I, c.s.I, c.s.h, c.s.I},      // dW_down [h,I]    = dx_in^T . act
      {dxb, a.ao, gw.wo, c.s.h, c.s.QD, c.s.QD, c.s.h, c.s.QD}};        // dW_o    [h,QD]   = dxb^T  . ao
};

// RMSNorm backward of the gradient in b.dxn, or of the split-K slabs its producer left (c.nsp > 1: summed in the kernel)
int norm_bwd(const Bwd& c, const void* x, const void* w, const char* rstd, const void* dres, void* dx, void* dwp, void* ws,
             void* rs, void* ev) {
  if (c.nsp > 1)
    return sd_rmsnorm_bwd_slabs((const float*)c.b.ws_splitk, c.nsp, x, w, (const float*)rstd, dres, dx, dwp, c.acc, ws, c.s.M,
                                c.s.h, rs, ev, c.stream);
  return sd_rmsnorm_bwd2(c.b.dxn, x, w, (const float*)rstd, dres, dx, dwp, c.acc, ws, c.s.M, c.s.h, rs, ev, c.stream);
}

// one weight gradient as a plain TN GEMM over K rows
int dw_gemm(const Bwd& c, const sd_gemm_problem& q, int K, void* stream) {
  return sd_gemm_bf16(q.A, q.B, q.C, c.accp(q.C), q.M, q.N, K, q.lda, q.ldb, q.ldc, q.ldc, 1, 1, stream);
}
// The separate-GEMM schedule launches each weight gradient as soon as its input is final: main says so (`ev`, see
// SdBwdEvent), the side stream waits, the GEMM follows there.  In the other schedules both are no-ops.
int input_final(const Bwd& c, int ev) { return c.separate ? c.ord.side_waits_for_main(ev) : 0; }
int dw_separate(const Bwd& c, const sd_gemm_problem& q) { return c.separate ? dw_gemm(c, q, c.s.M, c.wstream) : 0; }

// lm_head: dxn = dlogits . W ; dW (+)= dlogits^T . xn_f ; then the final norm's backward -> the last layer's dx_in
int bwd_head(Bwd& c) {
  const Sizes& s = c.s; const BwdScratch& b = c.b;
  const int top = (s.L - 1) & 1;  // buffer set of the last layer (the first one the backward visits)
  // dlogits (produced on main by the caller) is final: lm_head dW runs beside lm_head dX
  RUN(c.ord.side_waits_for_main(kEvGradIn));
  // with head rows, dlogits holds only the n_head_rows rows the forward produced; every other row of d(xn_f) is zero
  const void* xs = c.bt.head_rows ? c.tail.xn_rows : c.tail.xn_f;
  const int K = c.bt.head_rows ? c.bt.n_head_rows : s.M;
  void* hs = c.head_dw_beside ? c.wstream : c.stream;
  auto head_dw = [&](int r0) {  // dW rows [r0, V) (+)= dlogits[:, r0:]^T . xs
    char* gh = (char*)c.g->lm_head + (int64_t)r0 * s.h * 2;
    return dw_gemm(c, {(const char*)c.dlogits + (int64_t)r0 * 2, xs, gh, s.V, s.h, s.h, s.V - r0, s.h}, K, hs);
  };
  if (c.dw) {
    RUN(head_dw(0));
  } else {
    // Stage-1: dW of the new rows only.  The GEMM starts at the first multiple of 8 at or above grad_row_lo (16-byte
    // aligned operands); the < 8 rows before it take the strip kernel.
    const int lo = c.o.grad_row_lo, lo8 = ((lo + 7) & ~7) < s.V ? ((lo + 7) & ~7) : s.V;
    if (lo8 < s.V) RUN(head_dw(lo8));
    RUN(head_dw_strip(c.dlogits, xs, c.g->lm_head, lo, lo8, s.V, s.h, K, c.acc, hs));
  }
  if (c.bt.head_rows) {
    RUN(sd_gemm_bf16_splitk(c.dlogits, c.p->lm_head, b.dxb[top], nullptr, K, s.h, s.V, s.V, s.h, s.h, 0, 0, 1, b.ws_splitk,
                            b.splitk_bytes, c.stream));
    RUN(sd_rows_scatter(b.dxb[top], c.bt.head_rows, b.dxn, K, s.M, s.h, c.stream));
  } else {
    RUN(sd_gemm_bf16_splitk_partial(c.dlogits, c.p->lm_head, b.dxn, s.M, s.h, s.V, s.V, s.h, s.h, 0, 1, b.ws_splitk,
                                    b.splitk_bytes, &c.nsp, c.stream));
  }
  if (c.g->embed != c.g->lm_head && !c.acc) {
    const int64_t r0 = c.dw ? 0 : c.o.grad_row_lo;
    if (hipMemsetAsync((char*)c.g->embed + r0 * s.h * 2, 0, (size_t)(s.V - r0) * s.h * 2, (hipStream_t)c.stream) != hipSuccess)
      return SD_ERR_WORKSPACE;
  }
  RUN(norm_bwd(c, c.tail.x_last, c.p->final_norm, c.tail.rstd_f, nullptr, b.dxa[top], c.dw ? c.g->final_norm : nullptr,
               b.ws_norm, nullptr, nullptr));
  RUN(c.ord.main_waits_for_side(kEvSideDrained));  // the lm_head dW is enqueued and joined before it is reported
  c.ready(SD_STAGE_HEAD);
  return 0;
}

// The layer's dX chain from dx_in down to d(q|k|v): MLP, post-attention norm, o projection, attention, q/k-norm + RoPE
int layer_dx(Bwd& c, const BwdLayer& y) {
  const Sizes& s = c.s; const BwdScratch& b = c.b; const LayerActs& a = y.a;
  // recompute: this work set was last read by the dW GEMMs of layer l+2, which main has waited for (layer l+1's join)
  if (c.save == SD_SAVE_LAYER_INPUTS && y.l != s.L - 1) RUN(layer_forward(c.d, s, a, y.w, nullptr, true, c.bt, c.stream));
  RUN(input_final(c, kEvGradIn));
  RUN(dw_separate(c, y.pr[kDwDown]));
  // d(act) = dx_in . W_down with the SwiGLU backward in the epilogue: d(act) itself never reaches HBM
  RUN(fused_or(sd_gemm_swiglu_bwd(y.dx_in, y.w.wdown, a.gu, y.dgu, s.M, s.I, s.h, c.stream), [&] {
    RUN(sd_gemm_bf16(y.dx_in, y.w.wdown, b.dact, nullptr, s.M, s.I, s.h, s.h, s.I, s.I, 0, 0, 1, c.stream));
    return sd_swiglu_bwd(b.dact, a.gu, y.dgu, s.M, s.I, c.stream);
  }));
  RUN(input_final(c, kEvDgu));
  RUN(sd_gemm_bf16_splitk_partial(y.dgu, y.w.wgu, b.dxn, s.M, s.h, 2 * s.I, 2 * s.I, s.h, s.h, 0, 1, b.ws_splitk,
                                  b.splitk_bytes, &c.nsp, c.stream));
  RUN(dw_separate(c, y.pr[kDwGu]));
  // gain gradient: reduced from the kernel's partial sums beside the main stream (lent event), or left to gain_reduce
  RUN(norm_bwd(c, a.x_mid, y.w.ln2, a.rstd2, y.dx_in, y.dxb, c.batch_gains ? nullptr : y.gw.ln2, b.ws_norm2[y.P],
               c.gains_beside ? c.o.side_stream : nullptr, c.dw ? c.ord.event(kEvLentNorm) : nullptr));
  RUN(input_final(c, kEvDxb));
  // d(attention output) = dxb . Wo with delta = rowsum(dO * O) in the epilogue (one 128-column tile = one head)
  const void* o_for_delta = nullptr;
  RUN(fused_or(sd_gemm_odx_delta(y.dxb, y.w.wo, b.dao, a.ao, s.QD, (float*)b.delta, s.M, c.bt.T, s.Hq, s.h, c.stream), [&] {
    o_for_delta = a.ao;
    return sd_gemm_bf16(y.dxb, y.w.wo, b.dao, nullptr, s.M, s.QD, s.h, s.h, s.QD, s.QD, 0, 0, 1, c.stream);
  }));
  RUN(dw_separate(c, y.pr[kDwO]));
  const SdQkv f(s, a.qk, a.qkv), df(s, b.dqk, y.dqkv);
  void* dq_stream = c.dq_beside ? c.o.side_stream : nullptr;
  if (c.bt.vl)
    RUN(sd_attn_bwd_varlen(f.q, f.k, f.v, o_for_delta, b.dao, (const float*)a.lse, (float*)b.delta, df.q, df.k, df.v, c.bt.vl,
                           s.QK, s.QK, s.QKV, s.QD, s.QK, s.QK, s.QKV, s.M, s.Hq, s.Hkv, 128, kSdAttnScale, dq_stream,
                           c.stream));
  else
    RUN(sd_attn_bwd2(f.q, f.k, f.v, o_for_delta, b.dao, (const float*)a.lse, (float*)b.delta, df.q, df.k, df.v, c.bt.kv_len,
                     s.QK, s.QK, s.QKV, s.QD, s.QK, s.QK, s.QKV, c.bt.B, c.bt.T, s.Hq, s.Hkv, 128, kSdAttnScale, dq_stream,
                     c.stream));
  void *dq_gain = c.batch_gains ? nullptr : y.gw.q_gain, *dk_gain = c.batch_gains ? nullptr : y.gw.k_gain;
  return sd_qknorm_rope_bwd2(b.dqk, a.qkv, y.w.q_gain, y.w.k_gain, c.bt.cos_tab, c.bt.sin_tab, y.dqkv, dq_gain, dk_gain, c.acc,
                             b.ws_qk[y.P], s.M, c.bt.T, s.Hq, s.Hkv, c.d->eps, c.gains_beside ? c.o.side_stream : nullptr,
                             c.dw ? c.ord.event(kEvLentQkNorm) : nullptr, c.stream);
}

// The layer's weight gradients, now that d(q|k|v) -- and with it dx_in, dgu, dxb of this layer -- is final.  Grouped: all
// four as ONE persistent launch (sd_gemm_grouped_tn: 926 vs 587 TFLOP/s for four separate launches) on the side stream,
// i.e. under the dX chain of the NEXT layer.  Separate: the last of the four GEMMs, the others are already enqueued.
int layer_dw(const Bwd& c, const BwdLayer& y) {
  if (!c.dw) return 0;
  RUN(c.ord.side_waits_for_main(kEvDqkv));
  if (!c.grouped) return dw_gemm(c, y.pr[kDwQkv], c.s.M, c.wstream);
  RUN(fused_or(sd_gemm_grouped_tn(y.pr, 4, c.s.M, c.acc, c.wstream), [&] {
    for (const sd_gemm_problem& q : y.pr) RUN(dw_gemm(c, q, c.s.M, c.wstream));
    return 0;
  }));
  // the layer is finished on the side stream here, unless its batched gain reduce is still to come (gain_reduce)
  return c.batch_gains ? 0 : c.ord.record_on_side(kEvLayerDone + y.P);
}

// d(q|k|v) -> dx_out: q|k|v projection dX, then the input norm's backward.  dx_out of layer l is dx_in of layer l+1, so
// main first waits for the dW GEMMs that still read it: grouped, the launch of layer l+1 (`pending`, by the event it
// recorded); separate, this layer's own four (dx_in, dgu, dxb, dqkv are reused too), done before the callback as well.
int layer_dx_out(Bwd& c, const BwdLayer& y) {
  const Sizes& s = c.s;
  RUN(sd_gemm_bf16_splitk_partial(y.dqkv, y.w.wqkv, c.b.dxn, s.M, s.h, s.QKV, s.QKV, s.h, s.h, 0, 1, c.b.ws_splitk,
                                  c.b.splitk_bytes, &c.nsp, c.stream));
  if (c.grouped && c.pending >= 0) RUN(c.ord.main_waits_for_record(kEvLayerDone + (c.pending & 1)));
  if (c.separate) RUN(c.ord.main_waits_for_side(kEvSideDrained));
  return norm_bwd(c, y.a.x_in, y.w.ln1, y.a.rstd1, y.dxb, y.dx_out, c.batch_gains ? nullptr : y.gw.ln1,
                  c.batch_gains ? c.b.ws_norm1[y.P] : c.b.ws_norm, nullptr, nullptr);
}

// batch_gains: ONE reduce finishes the layer's four gain gradients on the side stream, behind the layer's grouped dW
int gain_reduce(const Bwd& c, const BwdLayer& y) {
  if (!c.batch_gains) return 0;
  const Sizes& s = c.s;
  RUN(c.ord.side_waits_for_main(kEvGainPartials));  // the last partials (input norm) are enqueued on main
  const int nb_n = sd_rmsnorm_bwd_partial_rows(s.M, s.h), nb_q = sd_qknorm_rope_bwd_partial_rows(s.M, s.Hq, s.Hkv);
  const sd_colsum_problem cp[4] = {{(const float*)c.b.ws_norm2[y.P], y.gw.ln2, nb_n, s.h, s.h, c.acc},
                                   {(const float*)c.b.ws_norm1[y.P], y.gw.ln1, nb_n, s.h, s.h, c.acc},
                                   {(const float*)c.b.ws_qk[y.P], y.gw.q_gain, nb_q, 128, 256, c.acc},
                                   {(const float*)c.b.ws_qk[y.P] + 128, y.gw.k_gain, nb_q, 128, 256, c.acc}};
  RUN(sd_colsum_reduce_batch(cp, 4, c.wstream));
  return c.ord.record_on_side(kEvLayerDone + y.P);  // now covers the weight AND the gain gradients of the layer
}

// Reports finished layers to the caller.  A grouped layer is still in flight when its chain ends: it becomes `pending` and
// is reported by the next layer, which has made main wait for it (layer_dx_out) (layer 0: by bwd_drain).
void hand_over(Bwd& c, int l) {
  if (!c.grouped) { if (c.dw) c.ready(l); return; }
  if (c.pending >= 0) c.ready(c.pending);
  c.pending = l;
}

int bwd_drain(Bwd& c) {
  if (c.grouped && c.pending >= 0) {
    RUN(c.ord.main_waits_for_record(kEvLayerDone + (c.pending & 1)));  // layer 0's grouped dW, before it is reported
    c.ready(c.pending);
  }
  return c.ord.main_waits_for_side(kEvSideDrained);  // all the side stream was given (gain reduces, dQ), before the call returns
}

struct DecodeActs {
  char *x, *x_mid, *xn, *qkv, *q, *ao, *gu, *act, *ws;
  int32_t* tickets = nullptr;  // fused: the tickets of the one-launch cache step, int32 [L][B][Hkv], at the tail
  int64_t ws_bytes, total;
  DecodeActs(const sd_qwen3_dims* d, int B, int cap, char* p, bool fused = false) {
    const Sizes s(d, B, 1);
    int64_t off = 0;  // (p == nullptr: a size query, no address is formed)
    auto take = [&](int64_t n) { char* q = p ? p + off : nullptr; off += n; return q; };
    x = take(s.x); x_mid = take(s.x); xn = take(s.x); qkv = take(s.qkv); q = take(s.ao); ao = take(s.ao);
    gu = take(s.gu); act = take(s.act);
    ws_bytes = sd_attn_decode_workspace_bytes(B, s.Hq, cap);
    ws = take(al(ws_bytes));
    if (fused) tickets = (int32_t*)take(KvSink::ticket_bytes(s, B));
    total = off;
  }
};

// true when every GEMV of a skinny (sd_gemv_check) or wide (sd_gemv_wide_check) step accepts its shape: decided for the
// whole step before the first launch
using GemvCheck = int (*)(const void*, const void*, const void*, const void*, const void*, int, int, int, int64_t, int64_t,
                          int64_t, int64_t);
bool gemv_step_ok(GemvCheck chk, const sd_qwen3_params* p, const Sizes& s, const DecodeActs& a, const void* logits, int B) {
  bool ok = chk(a.x, p->lm_head, logits, nullptr, p->final_norm, B, s.V, s.h, s.h, s.h, s.V, 0) == 0;
  for (int l = 0; ok && l < s.L; ++l) {
    const sd_qwen3_layer& w = p->layers_host[l];
    ok = chk(a.x, w.wqkv, a.qkv, nullptr, w.ln1, B, s.QKV, s.h, s.h, s.h, s.QKV, 0) == 0 &&
         chk(a.ao, w.wo, a.x_mid, a.x, nullptr, B, s.h, s.QD, s.QD, s.QD, s.h, s.h) == 0 &&
         chk(a.x_mid, w.wgu, a.act, nullptr, w.ln2, B, s.I, s.h, s.h, s.h, s.I, 0) == 0 &&
         chk(a.act, w.wdown, a.x, a.x_mid, nullptr, B, s.h, s.I, s.I, s.I, s.h, s.h) == 0;
  }
  return ok;
}

// internal step kind of decode_step_impl (no entry accepts it as a flag bit): the GEMV sequence on the wide kernels
constexpr int kStepWide = 0x100;

// the launches of a decode step over either kind of cache; every argument was checked by the entry
int decode_step_impl(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos, int max_len,
                     const void* cos_tab, const void* sin_tab, const KvSink& kv, const Sizes& s, const DecodeActs& a,
                     void* logits, int B, int flags, void* stream) {
  const bool wide = (flags & kStepWide) && gemv_step_ok(sd_gemv_wide_check, p, s, a, logits, B);
  const bool skinny = (flags & SD_DECODE_SKINNY) && gemv_step_ok(sd_gemv_check, p, s, a, logits, B);
  RUN(kv.begin_step(s, B, stream));
  RUN(sd_embedding_fwd(ids, p->embed, a.x, B, s.h, s.V, stream));
  if (skinny || wide) {
    const auto gemv = wide ? sd_gemv_wide_bf16 : sd_gemv_bf16;
    const auto gemv_swiglu = wide ? sd_gemv_wide_swiglu : sd_gemv_swiglu;
    for (int l = 0; l < s.L; ++l) {
      const sd_qwen3_layer& w = p->layers_host[l];
      RUN(gemv(a.x, w.wqkv, a.qkv, nullptr, w.ln1, d->eps, B, s.QKV, s.h, s.h, s.h, s.QKV, 0, stream));
      RUN(kv.step(s, l, w.q_gain, w.k_gain, a.qkv, a.q, a.ao, cos_tab, sin_tab, pos, a.ws, a.ws_bytes, B, max_len, d->eps,
                  stream));
      RUN(gemv(a.ao, w.wo, a.x_mid, a.x, nullptr, 0.f, B, s.h, s.QD, s.QD, s.QD, s.h, s.h, stream));
      RUN(gemv_swiglu(a.x_mid, w.wgu, a.act, w.ln2, d->eps, B, s.I, s.h, stream));
      RUN(gemv(a.act, w.wdown, a.x, a.x_mid, nullptr, 0.f, B, s.h, s.I, s.I, s.I, s.h, s.h, stream));
    }
    return gemv(a.x, p->lm_head, logits, nullptr, p->final_norm, d->eps, B, s.V, s.h, s.h, s.h, s.V, 0, stream);
  }
  for (int l = 0; l < s.L; ++l) {
    const sd_qwen3_layer& w = p->layers_host[l];
    RUN(sd_rmsnorm_fwd(a.x, w.ln1, a.xn, nullptr, B, s.h, d->eps, stream));
    RUN(sd_gemm_bf16(a.xn, w.wqkv, a.qkv, nullptr, B, s.QKV, s.h, s.h, s.h, s.QKV, 0, 0, 0, stream));
    RUN(kv.step(s, l, w.q_gain, w.k_gain, a.qkv, a.q, a.ao, cos_tab, sin_tab, pos, a.ws, a.ws_bytes, B, max_len, d->eps,
                stream));
    RUN(sd_gemm_bf16(a.ao, w.wo, a.x_mid, a.x, B, s.h, s.QD, s.QD, s.QD, s.h, s.h, 0, 0, stream));
    RUN(sd_rmsnorm_fwd(a.x_mid, w.ln2, a.xn, nullptr, B, s.h, d->eps, stream));
    RUN(fused_or(sd_gemm_swiglu(a.xn, w.wgu, nullptr, a.act, B, s.I, s.h, stream), [&] {
      RUN(sd_gemm_bf16(a.xn, w.wgu, a.gu, nullptr, B, 2 * s.I, s.h, s.h, s.h, 2 * s.I, 0, 0, 0, stream));
      return sd_swiglu_fwd(a.gu, a.act, B, s.I, stream);
    }));
    RUN(sd_gemm_bf16(a.act, w.wdown, a.x, a.x_mid, B, s.h, s.I, s.I, s.I, s.h, s.h, 0, 0, stream));
  }
  RUN(sd_rmsnorm_fwd(a.x, p->final_norm, a.xn, nullptr, B, s.h, d->eps, stream));
  return sd_gemm_bf16(a.xn, p->lm_head, logits, nullptr, B, s.V, s.h, s.h, s.h, s.V, 0, 0, 0, stream);
}

// the event pool of sd_events.h
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
  const Tail t(s, base + s.body(save));
  char* pong = base + s.per_layer();  // inference only
  float* ssq_a = (float*)(t.x_last + s.tail());  // folded inference only
  float* ssq_b = (float*)(t.x_last + s.tail() + s.ssq());

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
    if (save) x_out = (l + 1 < s.L) ? layer_acts(s, base, l + 1, save).x_in : t.x_last;
    else x_out = (l + 1 < s.L) ? ((x_cur == pong) ? base : pong) : t.x_last;
    if (folded)
      RUN(layer_forward_folded(d, s, a, p->layers_host[l], x_out, *bt, ssq_a, ssq_b, l + 1 < s.L ? ssq_a : nullptr,
                               stream));
    else
      RUN(layer_forward(d, s, a, p->layers_host[l], x_out, save != SD_SAVE_NONE, *bt, stream, sink, l));
    x_cur = x_out;
  }
  return sd_head_fwd(d, s, *bt, t.x_last, p->final_norm, p->lm_head, t.rstd_f, t.xn_f, t.xn_rows, logits, stream);
}

extern "C" int sd_qwen3_forward(const sd_qwen3_dims* d, const sd_qwen3_params* p, const sd_qwen3_batch* batch, void* acts,
                                int64_t acts_bytes, void* logits, int mode, void* stream) {
  return forward_impl(d, p, batch, acts, acts_bytes, logits, mode, stream, nullptr);
}

// The student backward: checks, context, head, layers, drain, embedding.  With SD_BWD_EMBED_ONLY (Stage-1): the same dX
// chain, no per-layer gradient, the lm_head dW over rows [grad_row_lo, V) and the embedding scatter of ids >= grad_row_lo.
extern "C" int sd_qwen3_backward(const sd_qwen3_dims* d, const sd_qwen3_params* p, const sd_qwen3_params* g,
                                 const sd_qwen3_batch* bt, void* acts, int64_t acts_bytes, void* dlogits, void* scratch,
                                 int64_t scratch_bytes, const sd_qwen3_bwd_opts* opts, void* stream) {
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  RUN(sd_batch_check(bt));
  if (!opts) return SD_ERR_SHAPE;
  const sd_qwen3_bwd_opts& o = *opts;
  if ((o.flags & SD_BWD_EMBED_ONLY) && (o.grad_row_lo < 0 || o.grad_row_lo > d->vocab || o.dx0_out || o.on_grads_ready))
    return SD_ERR_SHAPE;
  if (o.flags & ~(SD_BWD_EMBED_ONLY | SD_BWD_ACCUMULATE | SD_BWD_RECOMPUTE)) return SD_ERR_SHAPE;
  const Sizes s(d, bt->B, bt->T);
  // SD_BWD_RECOMPUTE: `acts` came from a forward with SD_SAVE_LAYER_INPUTS; each layer's forward is run again from its
  // saved input right before its backward (the last layer's buffers are still those of the forward itself)
  const int save = (o.flags & SD_BWD_RECOMPUTE) ? SD_SAVE_LAYER_INPUTS : SD_SAVE_ALL;
  if (acts_bytes < sd_qwen3_acts_bytes(d, bt->B, bt->T, save)) return SD_ERR_WORKSPACE;
  const BwdScratch b(s, (char*)scratch);
  if (scratch_bytes < b.total) return SD_ERR_WORKSPACE;
  Bwd c{d, p, g, *bt, o, s, b, (char*)acts, save, dlogits, stream};
  RUN(c.ord.init(stream, o.side_stream));  // leases this call's events when there is a side stream
  SdSharedGpuScope shared(c.ord.side ? 1 : 0);  // two streams share the GPU: the persistent dW launches leave CUs to the dX chain
  RUN(bwd_head(c));
  for (int l = s.L - 1; l >= 0; --l) {
    const BwdLayer y{c, l};
    RUN(layer_dx(c, y));
    RUN(layer_dw(c, y));
    RUN(layer_dx_out(c, y));
    RUN(gain_reduce(c, y));
    hand_over(c, l);
  }
  RUN(bwd_drain(c));
  if (!c.dw) RUN(sd_embedding_bwd_range(bt->ids, b.dxa[1], g->embed, s.M, s.h, s.V, o.grad_row_lo, 1.0f, stream));
  else if (!o.dx0_out) RUN(sd_embedding_bwd(bt->ids, b.dxa[1], g->embed, s.M, s.h, s.V, 1.0f, stream));
  c.ready(SD_STAGE_EMBED);
  return 0;
}

// ------------------------------------------------------------------------------------------ KV-cache generation
// What the four block entries (prefill, extend, and their paged twins) do after their own checks: the head rows behind the
// prefill's activation set -- for an extend (sink.past) also the gathered cos / sin rows of the block -- then the forward.
static int block_forward(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* kv_len,
                         const void* cos_tab, const void* sin_tab, void* acts, void* logits, int B, int T, void* stream,
                         const KvSink& sink) {
  const int64_t base = al(sd_qwen3_acts_bytes(d, B, T, SD_SAVE_NONE));
  int64_t* rows = (int64_t*)((char*)acts + base);
  RUN(sd_last_rows(sink.past ? sink.new_len : kv_len, rows, B, T, stream));
  sd_qwen3_batch bt = {ids, kv_len, nullptr, cos_tab, sin_tab, rows, B, B, T, 0};
  if (sink.past) {  // (an extend has no kv_len)
    char* cos_rows = (char*)acts + al(sd_qwen3_prefill_acts_bytes(d, B, T));
    char* sin_rows = cos_rows + al((int64_t)B * T * 128 * 2);
    RUN(sd_rope_rows_at(cos_tab, sin_tab, sink.past, cos_rows, sin_rows, B, T, sink.cap, stream));
    bt.cos_tab = cos_rows; bt.sin_tab = sin_rows;
  }
  return forward_impl(d, p, &bt, acts, base, logits, SD_SAVE_NONE, stream, &sink);
}

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
  return block_forward(d, p, ids, kv_len, cos_tab, sin_tab, acts, logits, B, T, stream, KvSink{(char*)cache, cap});
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
  RUN(gqa_check(d));
  if (acts_bytes < sd_qwen3_extend_acts_bytes(d, B, T) || cache_bytes < sd_kvcache_bytes(d, B, cap)) return SD_ERR_WORKSPACE;
  return block_forward(d, p, ids, nullptr, cos_tab, sin_tab, acts, logits, B, T, stream, KvSink{(char*)cache, cap, past, new_len});
}

// The two block entries over a page pool (llm_engine.py:91): the twins' launches with the paged sinks.
extern "C" int64_t sd_qwen3_prefill_paged_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  return sd_qwen3_prefill_acts_bytes(d, B, T);
}

static int prefill_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* kv_len,
                         const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes, const sd_kv_pages* kv,
                         void* logits, int B, int T, void* stream, bool mx) {
  if (!d || !p) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  KvSink sink = {};
  RUN(paged_sink(d, kv, &sink, mx));
  if (B <= 0 || T <= 0 || sink.cap < T || !logits || !ids || !acts) return SD_ERR_SHAPE;
  if (acts_bytes < sd_qwen3_prefill_acts_bytes(d, B, T)) return SD_ERR_WORKSPACE;
  return block_forward(d, p, ids, kv_len, cos_tab, sin_tab, acts, logits, B, T, stream, sink);
}

extern "C" int sd_qwen3_prefill_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                      const int32_t* kv_len, const void* cos_tab, const void* sin_tab, void* acts,
                                      int64_t acts_bytes, const sd_kv_pages* kv, void* logits, int B, int T, void* stream) {
  return prefill_paged(d, p, ids, kv_len, cos_tab, sin_tab, acts, acts_bytes, kv, logits, B, T, stream, false);
}

// 8-bit pages: the prompt still attends over its in-flight bf16 K / V (sd_attn_fwd); only the sink quantises
extern "C" int sd_qwen3_prefill_paged_mx(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                         const int32_t* kv_len, const void* cos_tab, const void* sin_tab, void* acts,
                                         int64_t acts_bytes, const sd_kv_pages* kv, void* logits, int B, int T,
                                         void* stream) {
  return prefill_paged(d, p, ids, kv_len, cos_tab, sin_tab, acts, acts_bytes, kv, logits, B, T, stream, true);
}

extern "C" int64_t sd_qwen3_extend_paged_acts_bytes(const sd_qwen3_dims* d, int B, int T) {
  return sd_qwen3_extend_acts_bytes(d, B, T);
}

static int extend_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* past,
                        const int32_t* new_len, const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes,
                        const sd_kv_pages* kv, void* logits, int B, int T, void* stream, bool mx) {
  if (!d || !p) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  KvSink sink = {};
  RUN(paged_sink(d, kv, &sink, mx));
  if (B <= 0 || T <= 0 || sink.cap < T || !ids || !past || !new_len || !cos_tab || !sin_tab || !acts || !logits)
    return SD_ERR_SHAPE;
  RUN(gqa_check(d));
  if (acts_bytes < sd_qwen3_extend_acts_bytes(d, B, T)) return SD_ERR_WORKSPACE;
  sink.past = past; sink.new_len = new_len;
  return block_forward(d, p, ids, nullptr, cos_tab, sin_tab, acts, logits, B, T, stream, sink);
}

extern "C" int sd_qwen3_extend_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                     const int32_t* past, const int32_t* new_len, const void* cos_tab, const void* sin_tab,
                                     void* acts, int64_t acts_bytes, const sd_kv_pages* kv, void* logits, int B, int T,
                                     void* stream) {
  return extend_paged(d, p, ids, past, new_len, cos_tab, sin_tab, acts, acts_bytes, kv, logits, B, T, stream, false);
}

extern "C" int sd_qwen3_extend_paged_mx(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                        const int32_t* past, const int32_t* new_len, const void* cos_tab,
                                        const void* sin_tab, void* acts, int64_t acts_bytes, const sd_kv_pages* kv,
                                        void* logits, int B, int T, void* stream) {
  return extend_paged(d, p, ids, past, new_len, cos_tab, sin_tab, acts, acts_bytes, kv, logits, B, T, stream, true);
}

extern "C" int64_t sd_qwen3_decode_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  if (!d || d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || cap <= 0) return SD_ERR_SHAPE;
  return DecodeActs(d, B, cap, nullptr).total;
}

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

static int decode_step_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos,
                             int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_pages* kvp, void* acts,
                             int64_t acts_bytes, void* logits, int B, int flags, void* stream, bool mx) {
  if (flags & ~SD_DECODE_SKINNY) return SD_ERR_SHAPE;
  if (!d || !p) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || max_len <= 0 || !ids || !pos || !logits || !acts) return SD_ERR_SHAPE;
  RUN(gqa_check(d));
  KvSink kv = {};
  RUN(paged_sink(d, kvp, &kv, mx));
  const Sizes s(d, B, 1);
  const DecodeActs a(d, B, kv.cap, (char*)acts);
  if (acts_bytes < a.total) return SD_ERR_WORKSPACE;
  return decode_step_impl(d, p, ids, pos, max_len, cos_tab, sin_tab, kv, s, a, logits, B, flags, stream);
}

extern "C" int sd_qwen3_decode_step_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                          const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                          const sd_kv_pages* kvp, void* acts, int64_t acts_bytes, void* logits, int B,
                                          int flags, void* stream) {
  return decode_step_paged(d, p, ids, pos, max_len, cos_tab, sin_tab, kvp, acts, acts_bytes, logits, B, flags, stream,
                           false);
}

extern "C" int sd_qwen3_decode_step_paged_mx(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                             const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                             const sd_kv_pages* kvp, void* acts, int64_t acts_bytes, void* logits, int B,
                                             int flags, void* stream) {
  return decode_step_paged(d, p, ids, pos, max_len, cos_tab, sin_tab, kvp, acts, acts_bytes, logits, B, flags, stream, true);
}

// sd_qwen3_decode_step_wide: the GEMV sequence on the wide kernels over a cache of any kind
extern "C" int64_t sd_qwen3_decode_step_wide_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  return sd_qwen3_decode_acts_bytes(d, B, cap);
}

extern "C" int sd_qwen3_decode_step_wide(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                         const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                         const sd_kv_ref* kvr, void* acts, int64_t acts_bytes, void* logits, int B,
                                         void* stream) {
  if (!d || !p || !kvr) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || max_len <= 0 || !ids || !pos || !logits || !acts) return SD_ERR_SHAPE;
  RUN(gqa_check(d));
  KvSink kv = {};
  RUN(ref_sink(d, kvr, B, &kv));
  const Sizes s(d, B, 1);
  const DecodeActs a(d, B, kv.cap, (char*)acts);
  if (acts_bytes < a.total) return SD_ERR_WORKSPACE;
  return decode_step_impl(d, p, ids, pos, max_len, cos_tab, sin_tab, kv, s, a, logits, B, kStepWide, stream);
}

// sd_qwen3_decode_step_fused: any of the three sequences over a cache of any kind, on the one-launch cache step
extern "C" int64_t sd_qwen3_decode_step_fused_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  if (!d || d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || cap <= 0) return SD_ERR_SHAPE;
  return DecodeActs(d, B, cap, nullptr, true).total;
}

extern "C" int sd_qwen3_decode_step_fused(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                          const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                          const sd_kv_ref* kvr, void* acts, int64_t acts_bytes, void* logits, int B,
                                          int kernels, void* stream) {
  if (kernels < 0 || kernels > 2) return SD_ERR_SHAPE;
  if (!d || !p || !kvr) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || max_len <= 0 || !ids || !pos || !logits || !acts || !cos_tab || !sin_tab) return SD_ERR_SHAPE;
  RUN(gqa_check(d));
  KvSink kv = {};
  RUN(ref_sink(d, kvr, B, &kv));
  const Sizes s(d, B, 1);
  const DecodeActs a(d, B, kv.cap, (char*)acts, true);
  if (acts_bytes < a.total) return SD_ERR_WORKSPACE;
  RUN(fused_align_check(acts, kv));
  kv.tickets = a.tickets;
  const int flags = kernels == 2 ? kStepWide : kernels == 1 ? SD_DECODE_SKINNY : 0;
  return decode_step_impl(d, p, ids, pos, max_len, cos_tab, sin_tab, kv, s, a, logits, B, flags, stream);
}

// sd_qwen3_decode_step_shared: any of the three sequences over a PAGED cache, on the shared-page decode attention
extern "C" int64_t sd_qwen3_decode_step_shared_acts_bytes(const sd_qwen3_dims* d, int B, int cap) {
  return sd_qwen3_decode_acts_bytes(d, B, cap);
}

extern "C" int sd_qwen3_decode_step_shared(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                           const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                           const sd_kv_ref* kvr, void* acts, int64_t acts_bytes, void* logits, int B,
                                           int kernels, void* stream) {
  if (kernels < 0 || kernels > 2) return SD_ERR_SHAPE;
  if (!d || !p || !kvr) return SD_ERR_SHAPE;
  if (d->head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (B <= 0 || max_len <= 0 || !ids || !pos || !logits || !acts || !cos_tab || !sin_tab) return SD_ERR_SHAPE;
  if (kvr->kind == 0) return SD_ERR_SHAPE;  // rows of a contiguous cache share nothing
  RUN(gqa_check(d));
  KvSink kv = {};
  RUN(ref_sink(d, kvr, B, &kv));
  const Sizes s(d, B, 1);
  const DecodeActs a(d, B, kv.cap, (char*)acts);
  if (acts_bytes < a.total) return SD_ERR_WORKSPACE;
  kv.shared = true;
  const int flags = kernels == 2 ? kStepWide : kernels == 1 ? SD_DECODE_SKINNY : 0;
  return decode_step_impl(d, p, ids, pos, max_len, cos_tab, sin_tab, kv, s, a, logits, B, flags, stream);
}

extern "C" int sd_qwen3_decode_step(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids,
                                    const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab, void* cache,
                                    int64_t cache_bytes, int cap, void* acts, int64_t acts_bytes, void* logits, int B,
                                    void* stream) {
  return sd_qwen3_decode_step_flags(d, p, ids, pos, max_len, cos_tab, sin_tab, cache, cache_bytes, cap, acts, acts_bytes,
                                    logits, B, 0, stream);
}
