// Fused temperature-scaled KL + CE distillation loss over the expanded speech-token vocabulary,
// forward and backward, for gfx950.  HBM-bound: one 1024-thread workgroup streams one logits row.
//
// Replaces DistillationLoss.forward and its autograd backward:
//   /root/reference/distillation_loss.py:31-45   causal shift + valid-row predicate (no compaction
//                                                copy here: the predicate is evaluated per row)
//   /root/reference/distillation_loss.py:47-53   N == 0 -> zeros
//   /root/reference/distillation_loss.py:56-71   dense KL (batchmean) * T^2, teacher CE monitor
//   /root/reference/distillation_loss.py:73-118  sparse top-K KL, approximate teacher monitor
//   /root/reference/distillation_loss.py:123-128 CE task loss, alpha mix
// Gradient:
//   d total / d s = a (softmax(s) - e_y)/N + (1-a) T (softmax(s/T) - q)/N   on valid rows, else 0.
//
// Forward keeps per-row normalisers (lse at T=1, lse at T, teacher lse at T) so that backward is one
// read of the logits and one write of the gradient.  All reductions are deterministic (per-row
// partials + a fixed-order final reduce); no float atomics.
#include <type_traits>
#include "sd_rows.cuh"
#include "../../include/sd_hip.h"
#include "sd_prof.h"

namespace {

constexpr int NT = 1024;
constexpr int KMAX = 1024;

// Host dispatch of a run-time value to a template argument: fn gets a tag whose ::type is the element type / an
// integral_constant whose ::value is the flag.  Every entry's check has refused all dtypes but bf16 and fp32 before.
template <typename T> struct TypeTag { typedef T type; };
template <typename F> int by_dtype(int dtype, F&& fn) {
  return dtype == SD_DTYPE_BF16 ? fn(TypeTag<bf16>{}) : fn(TypeTag<float>{});
}
template <typename F> void by_flag(bool b, F&& fn) {
  if (b) fn(std::true_type{}); else fn(std::false_type{});
}
#define SD_TAG_TYPE(tag) typename decltype(tag)::type
#define SD_FLAG(tag) decltype(tag)::value
inline const char* type_name(size_t size) { return size == 2 ? "__bf16" : "float"; }
inline const char* flag_name(bool b) { return b ? "true" : "false"; }
// fn(NF): the threads per row of a forward with a top-K teacher, one thread per entry in its epilogue -- 512, and 1024
// only where the K entries do not fit one thread each at 512
typedef std::integral_constant<int, 512> Threads512;
template <typename F> void by_threads(int K, F&& fn) {
  if (K > 512) fn(std::integral_constant<int, 1024>{}); else fn(Threads512{});
}

// What every rows entry asks of its rows, in this order: V a multiple of 8, S (and the dense teacher S2, if there is
// one) 16-byte aligned, bf16 or fp32.  Each family's check puts its own conditions before and after.
int rows_check(int V, int dtype, const void* S, const void* S2 = nullptr) {
  if (V & 7) return SD_ERR_ALIGN;
  if (((uintptr_t)S & 15) || ((uintptr_t)S2 & 15)) return SD_ERR_ALIGN;
  if (dtype != SD_DTYPE_BF16 && dtype != SD_DTYPE_F32) return SD_ERR_UNSUPPORTED;
  return 0;
}

// The launch path of every rows entry: the dtype becomes the element type T, `launch(tag of T)` runs inside a profiler
// record of `kind` over elems x sizeof(T) bytes and is checked; then `fin()`, a forward's finalize launch, is run and
// checked -- after the record has ended, or (fin_in_scope: sd_kdloss_fwd*, whose record has always covered both) inside.
template <typename L, typename F>
int rows_launch(int dtype, int kind, double elems, hipStream_t st, bool fin_in_scope, L&& launch, F&& fin) {
  return by_dtype(dtype, [&](auto tt) -> int {
    SdProfScope prof(kind, elems * sizeof(SD_TAG_TYPE(tt)), st);
    launch(tt);
    SD_CHECK_LAUNCH();
    if (!fin_in_scope) prof.close();
    fin();
    SD_CHECK_LAUNCH();
    return 0;
  });
}
template <typename L> int rows_launch(int dtype, int kind, double elems, hipStream_t st, L&& launch) {  // a backward
  return rows_launch(dtype, kind, elems, st, true, launch, [] {});
}

// the exit of a forward kernel on a masked row: its stats are all zeros (valid = 0)
template <typename Stats> SD_DEV void masked_row(Stats* stats, int row) {
  if (threadIdx.x == 0) stats[row] = Stats{};
}

// row -> (b, t); label / mask are taken at t+1 (the causal shift).  T == 0: the caller already selected and
// shifted the rows (sd_kdloss_fwd_rows): label / mask are taken at `row` itself.
SD_DEV bool row_valid(const int64_t* labels, const uint8_t* mask, int row, int T, long* y) {
  int at = row;
  if (T) {
    const int t = row % T;
    if (t == T - 1) return false;
    at = row + 1;
  }
  const long lab = labels[at];
  *y = lab;
  if (lab == -100) return false;
  if (mask && !mask[at]) return false;
  return true;
}

struct RowStats {  // 8 floats per row
  float lse1, lseT, t_lseT, valid, task, distill, teacher, hits;
};

// T2: temperature == 2 (the reference's default, train.py:488-491).  Then exp(z) = exp(z / 2)^2, so the sum-exp at T = 1
// comes from the T = 2 exponential by one multiplication: half the transcendentals of a kernel that is bound by them
// (129 us = 3.8 TB/s before, with two v_exp_f32 per logit at a quarter of the vector rate).
// NF threads per row: 512 (four workgroups per CU, 128 chunks of a CU in flight) whenever the K teacher entries fit one
// thread each, else 1024.  DENSE: teacher logits instead of top-K (its prefetch registers only exist in that variant).
// The bf16 1024-thread variant is held to 8 waves per SIMD (64 VGPRs, two workgroups per CU): left alone the compiler
// lands on 64 or 66 registers with the shape of the surrounding code, and 66 leaves one workgroup per CU.
template <typename T, bool T2, int NF, bool DENSE>
__global__ __launch_bounds__(NF, (NF == 1024 && sizeof(T) == 2) ? 8 : 1) void kd_fwd_kernel(const T* __restrict__ S, const T* __restrict__ Tl,
                                                    const _Float16* __restrict__ topv, const int32_t* __restrict__ topi,
                                                    const int64_t* __restrict__ labels, const uint8_t* __restrict__ mask,
                                                    RowStats* __restrict__ stats, int rows, int Tlen, int V, int K,
                                                    float temperature) {
  __shared__ float sc[32];
  const int row = blockIdx.x;
  long y = 0;
  const bool valid = row_valid(labels, mask, row, Tlen, &y);
  if (!valid || y < 0 || y >= V) return masked_row(stats, row);
  const float invT = 1.f / temperature;
  const float k1 = 1.4426950408889634f, kT = invT * k1;  // log2(e), log2(e) / T
  const T* s = S + (long)row * V;
  // ---- student normalisers (online max / sum-exp at T=1 and at T)
  float m = -INFINITY, s1 = 0.f, sT = 0.f;
  // ---- dense teacher: max, sum-exp at 1 and T, cross = sum exp((t-mt)/T) (t - s)
  float mt = -INFINITY, t1 = 0.f, tT = 0.f, cross = 0.f;
  const T* tl = DENSE ? Tl + (long)row * V : nullptr;
  row_sweep<T, NF, DENSE>(s, tl, V, [&](int, const float* f, const float* g) {
    online_raise<T2>(chunk_max8(f), invT, m, s1, sT);
    // exp((f - m) / T) = exp2(f * kT - m * kT): one fused multiply-add per exponential argument.  The fold leaves the
    // rounding error of m * kT in every exponent, which a forward KL forgives (gjsd_fwd_kernel says why it cannot)
    const float mkT = -m * kT, mk1 = -m * k1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float q = __builtin_amdgcn_exp2f(__builtin_fmaf(f[e], kT, mkT));
      sT += q;
      s1 += T2 ? q * q : __builtin_amdgcn_exp2f(__builtin_fmaf(f[e], k1, mk1));
    }
    if constexpr (DENSE) {
      online_raise<T2>(chunk_max8(g), invT, mt, t1, tT, cross);
      const float tkT = -mt * kT, tk1 = -mt * k1;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float w = __builtin_amdgcn_exp2f(__builtin_fmaf(g[e], kT, tkT));
        t1 += T2 ? w * w : __builtin_amdgcn_exp2f(__builtin_fmaf(g[e], k1, tk1));
        tT += w;
        cross += w * (g[e] - f[e]);
      }
    }
  });
  block_merge<NF>(m, s1, sT, invT, sc);
  const float lse1 = m + __logf(s1);
  const float lseT = m * invT + __logf(sT);
  const float sy = (float)s[y];
  const float task = lse1 - sy;
  float distill = 0.f, teacher = 0.f, hits = 0.f, t_lseT = 0.f;
  if constexpr (DENSE) {
    block_merge<NF>(mt, t1, tT, invT, sc, cross);
    t_lseT = mt * invT + __logf(tT);
    // sum_v q (log q - log p) = (1/T) sum_v q (t - s) - t_lseT + lseT      (sum_v q = 1)
    distill = cross / tT * invT - t_lseT + lseT;
    teacher = mt + __logf(t1) - (float)tl[y];
    hits = 1.f;
  } else {
    // sparse: q = softmax(v/T) over the K stored teacher log-probs (renormalised over top-K)
    const long kb = (long)row * K;
    const bool act = threadIdx.x < K;
    const float v = act ? (float)topv[kb + threadIdx.x] : -INFINITY;
    const int idx = act ? topi[kb + threadIdx.x] : 0;
    const float mv = block_max<NF>(v, sc);
    const float ev = act ? __expf((v - mv) * invT) : 0.f;
    const float sv = block_sum<NF>(ev, sc);
    const float logq = (v - mv) * invT - __logf(sv);
    float term = 0.f, hv = 0.f, hc = 0.f;
    if (act) {
      const int ii = idx < 0 ? 0 : (idx >= V ? V - 1 : idx);
      const float logp = (float)s[ii] * invT - lseT;
      term = (ev / sv) * (logq - logp);
      if ((long)idx == y) { hv = v; hc = 1.f; }
    }
    distill = block_sum<NF>(term, sc);
    teacher = block_sum<NF>(hv, sc);   // sum of teacher log-probs at the label, over hits
    hits = block_sum<NF>(hc, sc);
  }
  if (threadIdx.x == 0) stats[row] = RowStats{lse1, lseT, t_lseT, 1.f, task, distill, teacher, hits};
}

// The batch scalars from the per-row stats of kd_fwd_kernel (RowStats, HITS), gjsd_fwd_kernel (GjsdStats) or
// gjsd_topk_fwd_kernel (GjsdTopkStats, HITS): single block, fixed order.
//   RowStats:      out[0..5] = total, task, distill, teacher, N, n_hits
//   GjsdStats:     out[0..7] = total, task, distill, teacher, N, N, 0, 0
//   GjsdTopkStats: out[0..7] = total, task, distill, teacher, N, n_hits, 0, 0
template <typename Stats, bool HITS>
__global__ __launch_bounds__(NT) void kd_finalize_kernel(const Stats* __restrict__ stats, float* __restrict__ out, int rows,
                                                         float temperature, float alpha, int dense) {
  __shared__ float sc[32];
  float n = 0, task = 0, dist = 0, teach = 0, hits = 0;
  for (int r = threadIdx.x; r < rows; r += NT) {
    const Stats st = stats[r];
    n += st.valid; task += st.task; dist += st.distill; teach += st.teacher;
    if constexpr (HITS) hits += st.hits;
  }
  n = block_sum<NT>(n, sc); task = block_sum<NT>(task, sc); dist = block_sum<NT>(dist, sc); teach = block_sum<NT>(teach, sc);
  if constexpr (HITS) hits = block_sum<NT>(hits, sc);
  if (threadIdx.x != 0) return;
  if constexpr (HITS) {
    if constexpr (!std::is_same<Stats, RowStats>::value) out[6] = out[7] = 0.f;  // GjsdTopkStats: fp32[8], as GjsdStats
    if (n == 0.f) {
      out[0] = out[1] = out[2] = out[3] = 0.f; out[4] = 0.f; out[5] = 0.f;
    } else {
      const float tk = task / n;
      const float ds = dist / n * temperature * temperature;
      const float tc = dense ? teach / n : (hits > 0.f ? -teach / hits : 0.f);
      out[0] = alpha * tk + (1.f - alpha) * ds; out[1] = tk; out[2] = ds; out[3] = tc; out[4] = n; out[5] = hits;
    }
  } else {
    float tk = 0.f, ds = 0.f, tc = 0.f;
    if (n != 0.f) {
      tk = task / n;
      ds = dist / n * temperature * temperature;
      tc = teach / n;
    }
    out[0] = n != 0.f ? alpha * tk + (1.f - alpha) * ds : 0.f;
    out[1] = tk; out[2] = ds; out[3] = tc; out[4] = n; out[5] = n; out[6] = 0.f; out[7] = 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void kd_bwd_kernel(const T* S, const T* __restrict__ Tl,
                                                    const _Float16* __restrict__ topv, const int32_t* __restrict__ topi,
                                                    const int64_t* __restrict__ labels, const RowStats* __restrict__ stats,
                                                    const float* __restrict__ loss_out, const float* __restrict__ grad_out,
                                                    T* G, int rows, int Tlen, int V, int K, float temperature,
                                                    float alpha) {
  __shared__ float sc[32];
  __shared__ float k_q[KMAX];
  __shared__ float k_s[KMAX];
  __shared__ int k_i[KMAX];
  const int row = blockIdx.x;
  const RowStats st = stats[row];
  T* g = G + (long)row * V;
  if (st.valid == 0.f) return zero_row<T, NT>(g, V);
  const float invT = 1.f / temperature;
  const float N = loss_out[4];
  const float go = grad_out ? grad_out[0] : 1.f;
  const float a1 = go * alpha / N;                       // * softmax(s)
  const float aT = go * (1.f - alpha) * temperature / N;  // * softmax(s/T)  and  * q
  const long y = labels[row + (Tlen ? 1 : 0)];
  const T* s = S + (long)row * V;
  const T* tl = Tl ? Tl + (long)row * V : nullptr;
  const bool sparse = (tl == nullptr);
  if (sparse) {
    // gather everything the fix-up needs BEFORE the dense pass (G may alias S)
    const long kb = (long)row * K;
    const bool act = threadIdx.x < K;
    const float v = act ? (float)topv[kb + threadIdx.x] : -INFINITY;
    const int idx = act ? topi[kb + threadIdx.x] : -1;
    const float mv = block_max<NT>(v, sc);
    const float ev = act ? __expf((v - mv) * invT) : 0.f;
    const float sv = block_sum<NT>(ev, sc);
    if (act) {
      k_q[threadIdx.x] = ev / sv;
      k_i[threadIdx.x] = idx;
      k_s[threadIdx.x] = (idx >= 0 && idx < V) ? (float)s[idx] : 0.f;
    }
    __syncthreads();
  }
  for (int c = threadIdx.x * 8; c < V; c += NT * 8) {
    float f[8], o[8];
    Ld8<T>::load(s + c, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = a1 * __expf(f[e] - st.lse1) + aT * __expf(f[e] * invT - st.lseT);
    if (tl) {
      float q[8];
      Ld8<T>::load(tl + c, q);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] -= aT * __expf(q[e] * invT - st.t_lseT);
    }
    if (y >= c && y < c + 8) o[y - c] -= a1;
    Ld8<T>::store(g + c, o);
  }
  if (sparse) {
    __syncthreads();  // every dense store of this row is complete (vmcnt(0) + barrier) before the fix-up
    if (threadIdx.x < K) {
      const int idx = k_i[threadIdx.x];
      bool first = idx >= 0 && idx < V;
      float qs = 0.f;
      for (int k2 = 0; k2 < K; ++k2) {
        if (k_i[k2] == idx) {
          if (k2 < (int)threadIdx.x) first = false;
          qs += k_q[k2];  // duplicates of an index sum their q (gather semantics of the reference)
        }
      }
      if (first) {
        const float sv = k_s[threadIdx.x];
        float o = a1 * __expf(sv - st.lse1) + aT * __expf(sv * invT - st.lseT) - aT * qs;
        if ((long)idx == y) o -= a1;
        g[idx] = (T)o;
      }
    }
  }
}

int check(const void* S, const void* Tl, const void* topv, const void* topi, int B, int Tlen, int V, int K, int dtype) {
  if (B <= 0 || Tlen < 0 || V <= 0) return SD_ERR_SHAPE;
  if (int e = rows_check(V, dtype, S)) return e;
  if (!Tl && !(topv && topi)) return SD_ERR_NO_TEACHER;
  if (!Tl && (K <= 0 || K > KMAX)) return SD_ERR_SHAPE;
  return 0;
}

// a forward's finalize launch over the family's stats (rows_launch's `fin`)
template <typename Stats, bool HITS>
auto finalize(const void* stats, float* out, int rows, float temperature, float alpha, int dense, hipStream_t st) {
  return [=] {
    hipLaunchKernelGGL((kd_finalize_kernel<Stats, HITS>), dim3(1), dim3(NT), 0, st, (const Stats*)stats, out, rows,
                       temperature, alpha, dense);
  };
}

// Both forward entries: B sequences of Tlen positions, shifted and masked by the kernel (sd_kdloss_fwd), or Tlen == 0 and
// no mask: B rows the caller already shifted and selected (sd_kdloss_fwd_rows).
int kd_fwd(const void* S, const void* Tl, const void* topv, const void* topi, const int64_t* labels, const uint8_t* mask,
           void* stats, float* out, int B, int Tlen, int V, int K, float temperature, float alpha, int dtype, void* stream) {
  if (int e = check(S, Tl, topv, topi, B, Tlen, V, K, dtype)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int rows = Tlen ? B * Tlen : B;
  return rows_launch(dtype, SD_K_LOSS_FWD, (double)rows * V * (Tl ? 2 : 1), st, true, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    auto launch = [&](auto t2, auto nf, auto dense) {
      constexpr int NF = SD_FLAG(nf);
      // the symbol as rocprofv3 --kernel-trace prints it
      SD_PROF_LABEL("kd_fwd_kernel<%s, %s, %d, %s>", type_name(sizeof(T)), flag_name(SD_FLAG(t2)), NF, flag_name(SD_FLAG(dense)));
      hipLaunchKernelGGL((kd_fwd_kernel<T, SD_FLAG(t2), NF, SD_FLAG(dense)>), dim3(rows), dim3(NF), 0, st, (const T*)S,
                         (const T*)Tl, (const _Float16*)topv, (const int32_t*)topi, labels, mask, (RowStats*)stats, rows, Tlen,
                         V, K, temperature);
    };
    by_flag(temperature == 2.0f, [&](auto t2) {
      if (Tl) launch(t2, Threads512{}, std::true_type{});
      else by_threads(K, [&](auto nf) { launch(t2, nf, std::false_type{}); });
    });
  }, finalize<RowStats, true>(stats, out, rows, temperature, alpha, Tl ? 1 : 0, st));
}

int kd_bwd(const void* S, const void* Tl, const void* topv, const void* topi, const int64_t* labels, const void* stats,
           const float* out, const float* go, void* G, int B, int Tlen, int V, int K, float temperature, float alpha,
           int dtype, void* stream) {
  if (int e = check(S, Tl, topv, topi, B, Tlen, V, K, dtype)) return e;
  if ((uintptr_t)G & 15) return SD_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int rows = Tlen ? B * Tlen : B;
  return rows_launch(dtype, SD_K_LOSS_BWD, (double)rows * V * (Tl ? 3 : 2), st, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    SD_PROF_LABEL("kd_bwd_kernel<%s>", type_name(sizeof(T)));
    hipLaunchKernelGGL((kd_bwd_kernel<T>), dim3(rows), dim3(NT), 0, st, (const T*)S, (const T*)Tl, (const _Float16*)topv,
                       (const int32_t*)topi, labels, (const RowStats*)stats, out, go, (T*)G, rows, Tlen, V, K, temperature,
                       alpha);
  });
}

}  // namespace

extern "C" int64_t sd_kdloss_stats_bytes(int B, int T) { return (int64_t)B * T * sizeof(RowStats); }

extern "C" int sd_kdloss_fwd_rows(const void* student_logits, const void* teacher_logits, const void* top_k_v,
                                  const void* top_k_i, const int64_t* row_labels, void* row_stats, float* loss_out, int R,
                                  int V, int K, float temperature, float alpha, int dtype, void* stream) {
  return kd_fwd(student_logits, teacher_logits, top_k_v, top_k_i, row_labels, nullptr, row_stats, loss_out, R, 0, V, K,
                temperature, alpha, dtype, stream);
}

extern "C" int sd_kdloss_bwd_rows(const void* student_logits, const void* teacher_logits, const void* top_k_v,
                                  const void* top_k_i, const int64_t* row_labels, const void* row_stats,
                                  const float* loss_out, const float* grad_total, void* grad_logits, int R, int V, int K,
                                  float temperature, float alpha, int dtype, void* stream) {
  return kd_bwd(student_logits, teacher_logits, top_k_v, top_k_i, row_labels, row_stats, loss_out, grad_total, grad_logits,
                R, 0, V, K, temperature, alpha, dtype, stream);
}

extern "C" int sd_kdloss_fwd(const void* student_logits, const void* teacher_logits, const void* top_k_v,
                             const void* top_k_i, const int64_t* labels, const uint8_t* speech_mask, void* row_stats,
                             float* loss_out, int B, int T, int V, int K, float temperature, float alpha, int dtype,
                             void* stream) {
  return kd_fwd(student_logits, teacher_logits, top_k_v, top_k_i, labels, speech_mask, row_stats, loss_out, B, T, V, K,
                temperature, alpha, dtype, stream);
}

extern "C" int sd_kdloss_bwd(const void* student_logits, const void* teacher_logits, const void* top_k_v,
                             const void* top_k_i, const int64_t* labels, const void* row_stats, const float* loss_out,
                             const float* grad_total, void* grad_logits, int B, int T, int V, int K, float temperature,
                             float alpha, int dtype, void* stream) {
  return kd_bwd(student_logits, teacher_logits, top_k_v, top_k_i, labels, row_stats, loss_out, grad_total, grad_logits, B, T,
                V, K, temperature, alpha, dtype, stream);
}

// ---------------------------------------------------------------------------------------- causal-LM cross-entropy
// Stage-1 alignment loss (stage1.py: TRL SFTTrainer over HF Qwen3ForCausalLM(labels=...), i.e. HF's ForCausalLMLoss:
// logits.float(), shift by one, cross_entropy(ignore_index=-100, reduction = "sum" / num_items_in_batch when the Trainer
// passes num_items_in_batch, else "mean")) on rows the caller already shifted and selected -- the teacher-free
// counterpart of sd_kdloss_*_rows.  Same row streaming as kd_fwd_kernel (row_sweep), one exponential per logit; per-row stats + a fixed-order single-block finalize: deterministic, no atomics.
namespace {

struct CeStats {  // 4 floats per row
  float lse, loss, valid, pad;
};

template <typename T, int NF>
__global__ __launch_bounds__(NF) void ce_fwd_kernel(const T* __restrict__ S, const int64_t* __restrict__ labels,
                                                    CeStats* __restrict__ stats, int V) {
  __shared__ float sc[32];
  const int row = blockIdx.x;
  const long y = labels[row];
  if (y < 0 || y >= V) return masked_row(stats, row);  // -100 (and anything outside the vocabulary) masks the row
  const float k1 = 1.4426950408889634f;  // log2(e)
  const T* s = S + (long)row * V;
  float m = -INFINITY, s1 = 0.f;
  row_sweep<T, NF, false>(s, (const T*)nullptr, V, [&](int, const float* f, const float*) {
    const float cm = chunk_max8(f);
    if (cm > m) {  // one sum, rescaled with exp2 (online_raise, for kd_fwd_kernel's two sums, rescales with __expf)
      s1 *= __builtin_amdgcn_exp2f((m - cm) * k1);
      m = cm;
    }
    const float mk1 = -m * k1;
#pragma unroll
    for (int e = 0; e < 8; ++e) s1 += __builtin_amdgcn_exp2f(__builtin_fmaf(f[e], k1, mk1));
  });
  const float M = block_max<NF>(m, sc);
  s1 = block_sum<NF>(m == -INFINITY ? 0.f : s1 * __expf(m - M), sc);
  const float lse = M + __logf(s1);
  if (threadIdx.x == 0) stats[row] = CeStats{lse, lse - (float)s[y], 1.f, 0.f};
}

// out[0..3] = loss, sum of row losses, N valid rows, divisor used (single block, fixed order)
__global__ __launch_bounds__(NT) void ce_finalize_kernel(const CeStats* __restrict__ stats, const float* __restrict__ divisor,
                                                         float* __restrict__ out, int rows) {
  __shared__ float sc[32];
  float n = 0.f, sum = 0.f;
  for (int r = threadIdx.x; r < rows; r += NT) {
    const CeStats st = stats[r];
    n += st.valid;
    sum += st.loss;
  }
  n = block_sum<NT>(n, sc);
  sum = block_sum<NT>(sum, sc);
  if (threadIdx.x == 0) {
    const float d = divisor ? divisor[0] : n;
    out[0] = d != 0.f ? sum / d : 0.f;  // no valid row (or a zero divisor): loss 0, gradient 0
    out[1] = sum;
    out[2] = n;
    out[3] = d;
  }
}

// d loss / d s = go (softmax(s) - e_y) / divisor on valid rows, 0 elsewhere.  G may alias S.
template <typename T>
__global__ __launch_bounds__(NT) void ce_bwd_kernel(const T* S, const int64_t* __restrict__ labels,
                                                    const CeStats* __restrict__ stats, const float* __restrict__ loss_out,
                                                    const float* __restrict__ grad_out, T* G, int V) {
  const int row = blockIdx.x;
  const CeStats st = stats[row];
  T* g = G + (long)row * V;
  const float d = loss_out[3];
  if (st.valid == 0.f || d == 0.f) return zero_row<T, NT>(g, V);
  const float a = (grad_out ? grad_out[0] : 1.f) / d;
  const long y = labels[row];
  const T* s = S + (long)row * V;
  for (int c = threadIdx.x * 8; c < V; c += NT * 8) {
    float f[8], o[8];
    Ld8<T>::load(s + c, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = a * __expf(f[e] - st.lse);
    if (y >= c && y < c + 8) o[y - c] -= a;
    Ld8<T>::store(g + c, o);
  }
}

int ce_check(const void* S, const int64_t* labels, int R, int V, int dtype) {
  if (R <= 0 || V <= 0 || !labels) return SD_ERR_SHAPE;
  return rows_check(V, dtype, S);
}

}  // namespace

extern "C" int64_t sd_celoss_stats_bytes(int R) { return (int64_t)R * sizeof(CeStats); }

extern "C" int sd_celoss_fwd_rows(const void* logits, const int64_t* row_labels, const float* divisor, void* row_stats,
                                  float* loss_out, int R, int V, int dtype, void* stream) {
  if (int e = ce_check(logits, row_labels, R, V, dtype)) return e;
  hipStream_t st = (hipStream_t)stream;
  return rows_launch(dtype, SD_K_LOSS_FWD, (double)R * V, st, false, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    SD_PROF_LABEL("ce_fwd_kernel<%s, 512>", type_name(sizeof(T)));
    hipLaunchKernelGGL((ce_fwd_kernel<T, 512>), dim3(R), dim3(512), 0, st, (const T*)logits, row_labels,
                       (CeStats*)row_stats, V);
  }, [&] {
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(NT), 0, st, (const CeStats*)row_stats, divisor, loss_out, R);
  });
}

extern "C" int sd_celoss_bwd_rows(const void* logits, const int64_t* row_labels, const void* row_stats,
                                  const float* loss_out, const float* grad_total, void* grad_logits, int R, int V, int dtype,
                                  void* stream) {
  if (int e = ce_check(logits, row_labels, R, V, dtype)) return e;
  if ((uintptr_t)grad_logits & 15) return SD_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  return rows_launch(dtype, SD_K_LOSS_BWD, (double)R * V * 2, st, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    SD_PROF_LABEL("ce_bwd_kernel<%s>", type_name(sizeof(T)));
    hipLaunchKernelGGL((ce_bwd_kernel<T>), dim3(R), dim3(NT), 0, st, (const T*)logits, row_labels, (const CeStats*)row_stats,
                       loss_out, grad_total, (T*)grad_logits, V);
  });
}

// ---------------------------------------------------------------------------------------- loss rows
// distillation_loss.py:31-45: the loss reads position t of sequence b iff t < T-1, labels[b][t+1] != -100 and (with a
// speech mask) speech_mask[b][t+1] != 0.  One workgroup compacts the flat indices b*T+t of those rows IN ORDER (ballot
// prefix inside a wave, wave totals through LDS), writes the label each one predicts, and checks that the attention
// masks are valid-prefix (right-padded) masks -- everything the host needs before it can size the lm_head GEMMs, in one
// launch and one 8-byte read instead of ~15 tiny torch kernels.
namespace {

// One chunk of 1024 candidates of a 1024-thread workgroup, compacted IN ORDER: thread tid's candidate e (with its label)
// is appended to rows / row_labels iff `valid`, behind the *base_s rows of the chunks before -- ballot prefix inside a
// wave, the 16 wave totals through LDS -- and *base_s moves on.  Its three barriers included: every thread calls it.
SD_DEV void compact_chunk(bool valid, long long e, long long lab, long long* __restrict__ rows,
                          long long* __restrict__ row_labels, int* wave_tot, int* base_s) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned long long bal = __ballot(valid);
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wv] = __popcll(bal);
  __syncthreads();
  int off = *base_s;
  for (int w = 0; w < wv; ++w) off += wave_tot[w];
  if (valid) {
    rows[off + before] = e;
    row_labels[off + before] = lab;
  }
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < 16; ++w) tot += wave_tot[w];
    *base_s += tot;
  }
  __syncthreads();
}

__global__ __launch_bounds__(1024) void loss_rows_kernel(const long long* __restrict__ labels,
                                                         const long long* __restrict__ speech_mask,
                                                         const long long* __restrict__ mask_a,
                                                         const long long* __restrict__ mask_b, long long* __restrict__ rows,
                                                         long long* __restrict__ row_labels, int* __restrict__ meta, int B,
                                                         int T) {
  __shared__ int wave_tot[16];
  __shared__ int base_s, bad_s;
  const int tid = threadIdx.x;
  if (tid == 0) { base_s = 0; bad_s = 0; }
  __syncthreads();
  const long n = (long)B * T;
  int bad = 0;
  for (long c0 = 0; c0 < n; c0 += 1024) {
    const long e = c0 + tid;
    bool valid = false;
    long long lab = -100;
    if (e < n) {
      const int t = (int)(e % T);
      if (t + 1 < T) {
        lab = labels[e + 1];
        valid = lab != -100 && (!speech_mask || speech_mask[e + 1] != 0);
      }
      if (t > 0) {
        if (mask_a && mask_a[e] != 0 && mask_a[e - 1] == 0) bad = 1;
        if (mask_b && mask_b[e] != 0 && mask_b[e - 1] == 0) bad = 1;
      }
    }
    compact_chunk(valid, e, lab, rows, row_labels, wave_tot, &base_s);
  }
  if (bad) atomicOr(&bad_s, 1);
  __syncthreads();
  if (tid == 0) {
    meta[0] = base_s;
    meta[1] = bad_s;
  }
}

}  // namespace

extern "C" int sd_loss_rows(const int64_t* labels, const int64_t* speech_mask, const int64_t* mask_a, const int64_t* mask_b,
                            int64_t* rows, int64_t* row_labels, int32_t* meta, int B, int T, void* stream) {
  if (B <= 0 || T <= 0 || (long)B * T > (1l << 30)) return SD_ERR_SHAPE;
  if (!labels || !rows || !row_labels || !meta) return SD_ERR_SHAPE;
  SD_PROF_LABEL("loss_rows B=%d T=%d", B, T);
  SdProfScope prof(SD_K_MISC, 8.0 * B * T, (hipStream_t)stream);
  hipLaunchKernelGGL(loss_rows_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const long long*)labels,
                     (const long long*)speech_mask, (const long long*)mask_a, (const long long*)mask_b, (long long*)rows,
                     (long long*)row_labels, meta, B, T);
  SD_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------- loss rows of packed documents
// The same selection over ONE flat row of n_seqs documents laid end to end (padding-free packing): token m is a loss row
// iff m+1 < M, m+1 is not the first token of a document (the last token of a document predicts nothing, whatever label
// the next document starts with), labels[m+1] != -100 and (with a mask) speech_mask[m+1] != 0.  The launch also checks
// the segment array and reduces what the host needs to build the varlen descriptor and the RoPE gather without reading
// anything else: the longest document and the largest position.  A chunk of 1024 tokens marks its document starts in LDS
// from cu_seqlens (every offset is range-checked against the chunk before it indexes anything, so a malformed array gives
// wrong rows and meta[1] bit 0, never an access outside [0, M)); the compaction is compact_chunk, as in loss_rows_kernel.
namespace {

__global__ __launch_bounds__(1024) void packed_rows_kernel(const long long* __restrict__ labels,
                                                           const long long* __restrict__ speech_mask,
                                                           const int* __restrict__ cu, int n_seqs,
                                                           const long long* __restrict__ pos, long long* __restrict__ rows,
                                                           long long* __restrict__ row_labels, int* __restrict__ meta,
                                                           int M) {
  __shared__ int wave_tot[16];
  __shared__ int base_s, bad_s, longest_s, maxpos_s;
  __shared__ unsigned char next_starts[1024];  // next_starts[i]: token c0 + i + 1 opens a document
  const int tid = threadIdx.x;
  if (tid == 0) { base_s = 0; bad_s = 0; longest_s = 0; maxpos_s = 0; }
  __syncthreads();
  int bad = 0, longest = 0, maxpos = 0;
  for (int s = tid; s < n_seqs; s += 1024) {
    const int a = cu[s], b = cu[s + 1];
    if (b < a || (s == 0 && a != 0) || (s == n_seqs - 1 && b != M)) bad |= 1;
    longest = max(longest, b - a);
  }
  for (int c0 = 0; c0 < M; c0 += 1024) {
    next_starts[tid] = 0;
    __syncthreads();
    for (int s = tid; s <= n_seqs; s += 1024) {
      const long d = (long)cu[s] - c0 - 1;
      if (d >= 0 && d < 1024) next_starts[d] = 1;
    }
    __syncthreads();
    const int e = c0 + tid;
    bool valid = false;
    long long lab = -100;
    if (e < M) {
      if (e + 1 < M && !next_starts[tid]) {
        lab = labels[e + 1];
        valid = lab != -100 && (!speech_mask || speech_mask[e + 1] != 0);
      }
      if (pos) {
        const long long p = pos[e];
        if (p < 0) bad |= 2;
        maxpos = max(maxpos, (int)min(p, 0x7fffffffll));
      }
    }
    compact_chunk(valid, e, lab, rows, row_labels, wave_tot, &base_s);
  }
  if (bad) atomicOr(&bad_s, bad);
  atomicMax(&longest_s, longest);
  atomicMax(&maxpos_s, maxpos);
  __syncthreads();
  if (tid == 0) {
    meta[0] = base_s;
    meta[1] = bad_s;
    meta[2] = longest_s;
    meta[3] = maxpos_s;
  }
}

}  // namespace

extern "C" int sd_packed_rows(const int64_t* labels, const int64_t* speech_mask, const int32_t* cu_seqlens, int n_seqs,
                              const int64_t* position_ids, int64_t* rows, int64_t* row_labels, int32_t* meta, int M,
                              void* stream) {
  if (M <= 0 || n_seqs <= 0 || M > (1 << 30)) return SD_ERR_SHAPE;
  if (!labels || !cu_seqlens || !rows || !row_labels || !meta) return SD_ERR_SHAPE;
  SD_PROF_LABEL("packed_rows M=%d n=%d", M, n_seqs);
  SdProfScope prof(SD_K_MISC, 8.0 * M, (hipStream_t)stream);
  hipLaunchKernelGGL(packed_rows_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const long long*)labels,
                     (const long long*)speech_mask, cu_seqlens, n_seqs, (const long long*)position_ids, (long long*)rows,
                     (long long*)row_labels, meta, M);
  SD_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------- reverse KL / skewed JSD
// On-policy (generalised) distillation: divergences that do not force the student to cover every teacher mode.  With
// q = softmax(s/T), p = softmax(t/T) per selected row:
//   SD_DIV_REVERSE_KL  D = KL(q || p) = sum q (log q - log p)
//   SD_DIV_JSD         m = (1-b) q + b p,  D = b KL(p || m) + (1-b) KL(q || m),  0 < b < 1
//   d total / d s_j = [ a (softmax(s)_j - e_y) + (1-a) T q_j (g_j - c) ] / N,   c = sum_v q_v g_v
//     reverse KL: g_j = log q_j - log p_j (c = D);   JSD: g_j = (1-b)(log q_j - log m_j) (c = (1-b) KL(q || m))
// Unlike the forward KL of kd_fwd_kernel, no term can be formed before BOTH normalisers are known (log q and log p sit
// inside the sum), so the forward is one kernel that sweeps the row pair twice: sweep 1 is kd_fwd_kernel's dense sweep
// (online max / sum-exp of s at 1 and T, of t at 1 and T), sweep 2 forms the divergence terms.  One workgroup owns the pair,
// so the 2 x V x sizeof(T) bytes of sweep 2 (638 KB at V = 159 488 bf16) were read by this same workgroup microseconds
// before, where a second launch would re-read 0.98 GB behind a full grid.  With 512 row pairs in flight (327 MB, more than
// the Infinity Cache) only part of sweep 2 is served on-die: measured, it costs 0.7 x of an HBM sweep.
// Same streaming as kd_fwd_kernel (512 threads, row_sweep, exp2, the T == 2 squaring).  Transcendentals per logit pair:
// sweep 1: 2 at T == 2, else 4; sweep 2: reverse KL 1 (exp), JSD 3 (exp, exp, log); backward: one more exp for
// softmax(s) unless T == 2, where softmax(s)_j = q_j^2 exp(2 lseT - lse1).
// 0 log 0 = 0: an element whose q (or p) underflows contributes 0 -- guarded by a select, not by a log-domain logaddexp;
// m is clamped at FLT_MIN before its log (v_log_f32 takes no denormal), which moves a term of weight < 1e-37 by < 1e-36.
namespace {

// Every log-normaliser is kept as (row maximum, log of the max-subtracted sum) and applied as (x - max) / T - log sum:
// the difference is exact where it matters (0 at the maximum itself) and the log is small, where x / T - lse rounds at
// the magnitude of lse -- on a peaked row (one logit 60 above the rest) that alone is 2e-6 on every log q.
// The logs and c stay in the log2 units they were computed in, so that the backward forms bit for bit the forward's terms.
struct GjsdStats {  // 12 floats per row; m .. c are what the backward reads: lse(s) = m + ln 2 ls1, lse(s/T) = m / T + ln 2 lsT,
  float m, ls1, lsT, mt, ltT, c, valid, task, distill, teacher, pad0, pad1;  // lse(t/T) = mt / T + ln 2 ltT; c: see the forward
};

constexpr int GJ_NF = 512;  // threads per row, as kd_fwd_kernel's dense variant (here 2 to 4 workgroups per CU by VGPRs)
constexpr float GJ_LN2 = 0.6931471805599453f, GJ_LOG2E = 1.4426950408889634f, GJ_FLT_MIN = 1.17549435e-38f;

// One element x of a normaliser sweep after online_raise: sT += exp((x - m) / T), s1 += exp(x - m), UNFOLDED --
// exp2((x - m) kT), NOT kd_fwd_kernel's folded exp2(x kT - m kT): the fold leaves the rounding error of m kT in every
// exponent (the maximum itself gives 1 + 1e-6 instead of 1).  A forward KL forgives that, it shifts lse(s) and the
// cross term alike; here log q and log p each take their own shift, which on a peaked row near its teacher is
// ten thousand times D.  One subtraction more per logit, next to exponentials at a quarter of the vector rate.
template <bool T2>
SD_DEV void unfolded_step(float x, float m, float kT, float k1, float& s1, float& sT) {
  const float d = x - m;
  const float q = __builtin_amdgcn_exp2f(d * kT);
  sT += q;
  s1 += T2 ? q * q : __builtin_amdgcn_exp2f(d * k1);
}

// one element of sweep 2 / of the backward: q and (in log2 units) log q - log p, or log q - log m.
// m, mt: the row maxima; A0, B0: -log2 of the max-subtracted sums at T
template <bool JSD>
SD_DEV void gj_term(float f, float g, float m, float mt, float kT, float A0, float B0, float beta, float& q, float& dq,
                    float& p, float& dp) {
  const float a2 = __builtin_fmaf(f - m, kT, A0), b2 = __builtin_fmaf(g - mt, kT, B0);  // log2 q, log2 p
  q = __builtin_amdgcn_exp2f(a2);
  if constexpr (JSD) {
    p = __builtin_amdgcn_exp2f(b2);
    const float lm = __builtin_amdgcn_logf(fmaxf(__builtin_fmaf(1.f - beta, q, beta * p), GJ_FLT_MIN));  // v_log_f32 = log2
    dq = a2 - lm;
    dp = b2 - lm;
  } else {
    p = 0.f;
    dq = a2 - b2;
    dp = 0.f;
  }
}

template <typename T, bool T2, bool JSD>
__global__ __launch_bounds__(GJ_NF) void gjsd_fwd_kernel(const T* __restrict__ S, const T* __restrict__ Tl,
                                                         const int64_t* __restrict__ labels, GjsdStats* __restrict__ stats,
                                                         int V, float temperature, float beta) {
  __shared__ float sc[32];
  const int row = blockIdx.x;
  const long y = labels[row];
  if (y < 0 || y >= V) return masked_row(stats, row);  // -100 (and anything outside the vocabulary) masks the row
  const float invT = 1.f / temperature;
  const float k1 = GJ_LOG2E, kT = invT * k1;
  const T* s = S + (long)row * V;
  const T* tl = Tl + (long)row * V;
  // ---- sweep 1: the four normalisers (kd_fwd_kernel's dense sweep without its cross term)
  float m = -INFINITY, s1 = 0.f, sT = 0.f, mt = -INFINITY, t1 = 0.f, tT = 0.f;
  row_sweep<T, GJ_NF, true>(s, tl, V, [&](int, const float* f, const float* g) {
    online_raise<T2>(chunk_max8(f), invT, m, s1, sT);
    online_raise<T2>(chunk_max8(g), invT, mt, t1, tT);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      unfolded_step<T2>(f[e], m, kT, k1, s1, sT);
      unfolded_step<T2>(g[e], mt, kT, k1, t1, tT);
    }
  });
  block_merge<GJ_NF>(m, s1, sT, invT, sc);
  block_merge<GJ_NF>(mt, t1, tT, invT, sc);
  const float ls1 = __builtin_amdgcn_logf(s1), lt1 = __builtin_amdgcn_logf(t1);  // v_log_f32: log2
  const float lsT = __builtin_amdgcn_logf(sT), ltT = __builtin_amdgcn_logf(tT);
  // ---- sweep 2: the divergence terms, in log2 units (one multiplication by ln 2 per row)
  const float A0 = -lsT, B0 = -ltT;
  float accq = 0.f, accp = 0.f;
  row_sweep<T, GJ_NF, true>(s, tl, V, [&](int, const float* f, const float* g) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float q, dq, p, dp;
      gj_term<JSD>(f[e], g[e], m, mt, kT, A0, B0, beta, q, dq, p, dp);
      accq += q > 0.f ? q * dq : 0.f;
      if constexpr (JSD) accp += p > 0.f ? p * dp : 0.f;
    }
  });
  // c is kept as it was summed (log2 units, without the 1 - beta of g): the backward forms (log q_j - log . _j) - c in
  // those units first, so that on a one-hot q, where c IS the peak's own term, the difference is exactly 0
  const float c = block_sum<GJ_NF>(accq, sc);  // KL(q || p) / ln 2, or KL(q || m) / ln 2
  float D = c * GJ_LN2;
  if constexpr (JSD) D = beta * (block_sum<GJ_NF>(accp, sc) * GJ_LN2) + (1.f - beta) * D;
  if (threadIdx.x == 0)
    stats[row] = GjsdStats{m, ls1, lsT, mt, ltT, c, 1.f, (m - (float)s[y]) + ls1 * GJ_LN2, D,
                           (mt - (float)tl[y]) + lt1 * GJ_LN2, 0.f, 0.f};
}

// One read of both rows, one write of the gradient; G may alias S (see row_sweep).
template <typename T, bool T2, bool JSD>
__global__ __launch_bounds__(GJ_NF) void gjsd_bwd_kernel(const T* S, const T* __restrict__ Tl,
                                                         const int64_t* __restrict__ labels,
                                                         const GjsdStats* __restrict__ stats,
                                                         const float* __restrict__ loss_out,
                                                         const float* __restrict__ grad_out, T* G, int V, float temperature,
                                                         float alpha, float beta) {
  const int row = blockIdx.x;
  const GjsdStats st = stats[row];
  T* gr = G + (long)row * V;
  if (st.valid == 0.f) return zero_row<T, GJ_NF>(gr, V);
  const float invT = 1.f / temperature;
  const float k1 = GJ_LOG2E, kT = invT * k1;
  const float N = loss_out[4];
  const float go = grad_out ? grad_out[0] : 1.f;
  const float a1 = go * alpha / N;                        // * (softmax(s) - e_y)
  const float gs = JSD ? (1.f - beta) * GJ_LN2 : GJ_LN2;        // log2 units -> g
  const float aT = go * (1.f - alpha) * temperature / N * gs;  // * q (g - c), g - c still in log2 units
  const long y = labels[row];
  const float A0 = -st.lsT, B0 = -st.ltT, L1 = -st.ls1;
  const float r1 = T2 ? __builtin_amdgcn_exp2f(2.f * st.lsT - st.ls1) : 0.f;  // softmax(s) = q^2 r1 at T == 2
  row_sweep<T, GJ_NF, true>(S + (long)row * V, Tl + (long)row * V, V, [&](int c, const float* f, const float* g) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float q, dq, p, dp;
      gj_term<JSD>(f[e], g[e], st.m, st.mt, kT, A0, B0, beta, q, dq, p, dp);
      const float sm = T2 ? q * q * r1 : __builtin_amdgcn_exp2f(__builtin_fmaf(f[e] - st.m, k1, L1));
      const float w = q > 0.f ? q * (dq - st.c) : 0.f;
      o[e] = __builtin_fmaf(a1, sm, aT * w);
    }
    if (y >= c && y < c + 8) o[y - c] -= a1;
    Ld8<T>::store(gr + c, o);
  });
}

// The check of the three sd_gjsd*_rows families, in its one order: the row arrays, the family's teacher form (`teacher`: the
// code its own conditions gave, or 0), rows_check, the family's modes (`modes`, likewise), temperature, and the beta of a JSD.
// S2: a dense teacher, else null.  The backward's (G: true) gradient pointer comes last.
int gjsd_check(const void* S, const void* S2, const int64_t* labels, const void* stats, const float* out, int R, int V,
               float temperature, float beta, bool jsd, int dtype, int teacher, int modes, bool G, const void* grad) {
  if (R <= 0 || V <= 0 || !S || !labels || !stats || !out) return SD_ERR_SHAPE;
  if (teacher) return teacher;
  if (int e = rows_check(V, dtype, S, S2)) return e;
  if (modes) return modes;
  if (!(temperature > 0.f) || !(temperature < INFINITY)) return SD_ERR_SHAPE;  // NaN fails both comparisons
  if (jsd && !(beta > 0.f && beta < 1.f)) return SD_ERR_SHAPE;                  // likewise
  if (G && !grad) return SD_ERR_SHAPE;
  if (G && ((uintptr_t)grad & 15)) return SD_ERR_ALIGN;
  return 0;
}

// fn(T2, JSD): the two flags every gjsd kernel is instantiated over
template <typename F> void gjsd_flags(float temperature, int mode, F&& fn) {
  by_flag(temperature == 2.0f, [&](auto t2) { by_flag(mode == SD_DIV_JSD, [&](auto jsd) { fn(t2, jsd); }); });
}

int gjsd_dense_check(const void* S, const void* Tl, const int64_t* labels, const void* stats, const float* out, int R, int V,
                     float temperature, float beta, int mode, int dtype, bool G = false, const void* grad = nullptr) {
  return gjsd_check(S, Tl, labels, stats, out, R, V, temperature, beta, mode == SD_DIV_JSD, dtype,
                    !Tl ? SD_ERR_NO_TEACHER : 0, mode != SD_DIV_REVERSE_KL && mode != SD_DIV_JSD ? SD_ERR_UNSUPPORTED : 0, G, grad);
}

}  // namespace

extern "C" int64_t sd_gjsd_stats_bytes(int R) { return (int64_t)R * sizeof(GjsdStats); }

extern "C" int sd_gjsd_fwd_rows(const void* student_logits, const void* teacher_logits, const int64_t* row_labels,
                                void* row_stats, float* loss_out, int R, int V, float temperature, float alpha, float beta,
                                int mode, int dtype, void* stream) {
  if (int e = gjsd_dense_check(student_logits, teacher_logits, row_labels, row_stats, loss_out, R, V, temperature, beta, mode, dtype))
    return e;
  hipStream_t st = (hipStream_t)stream;
  return rows_launch(dtype, SD_K_LOSS_FWD, (double)R * V * 2, st, false, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    gjsd_flags(temperature, mode, [&](auto t2, auto jsd) {
      SD_PROF_LABEL("gjsd_fwd_kernel<%s, %s, %s>", type_name(sizeof(T)), flag_name(SD_FLAG(t2)), flag_name(SD_FLAG(jsd)));
      hipLaunchKernelGGL((gjsd_fwd_kernel<T, SD_FLAG(t2), SD_FLAG(jsd)>), dim3(R), dim3(GJ_NF), 0, st,
                         (const T*)student_logits, (const T*)teacher_logits, row_labels, (GjsdStats*)row_stats, V,
                         temperature, beta);
    });
  }, finalize<GjsdStats, false>(row_stats, loss_out, R, temperature, alpha, 1, st));
}

extern "C" int sd_gjsd_bwd_rows(const void* student_logits, const void* teacher_logits, const int64_t* row_labels,
                                const void* row_stats, const float* loss_out, const float* grad_total, void* grad_logits,
                                int R, int V, float temperature, float alpha, float beta, int mode, int dtype, void* stream) {
  if (int e = gjsd_dense_check(student_logits, teacher_logits, row_labels, row_stats, loss_out, R, V, temperature, beta, mode,
                               dtype, true, grad_logits))
    return e;
  hipStream_t st = (hipStream_t)stream;
  return rows_launch(dtype, SD_K_LOSS_BWD, (double)R * V * 3, st, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    gjsd_flags(temperature, mode, [&](auto t2, auto jsd) {
      SD_PROF_LABEL("gjsd_bwd_kernel<%s, %s, %s>", type_name(sizeof(T)), flag_name(SD_FLAG(t2)), flag_name(SD_FLAG(jsd)));
      hipLaunchKernelGGL((gjsd_bwd_kernel<T, SD_FLAG(t2), SD_FLAG(jsd)>), dim3(R), dim3(GJ_NF), 0, st,
                         (const T*)student_logits, (const T*)teacher_logits, row_labels, (const GjsdStats*)row_stats, loss_out,
                         grad_total, (T*)grad_logits, V, temperature, alpha, beta);
    });
  });
}

// ---------------------------------------------------------------------------------------- skewed JSD, top-K teacher
// SD_DIV_JSD against the reference's sparse teacher (distillation_loss.py:73-118: K stored log-probs v_k and indices i_k
// per row).  p_k = softmax(v / T)_k over the K entries, P_j = sum_{k: i_k = j} p_k, S = {j : P_j > 0}; then exactly
// gjsd_fwd_kernel's JSD with P as the teacher distribution.  Off S the mixture is m_j = (1-b) q_j, so every off-support
// element has the same g_j = g0 = -(1-b) log(1-b) and the V - |S| terms collapse into (1 - Q_S) g0, Q_S = sum_S q_j:
//   D = b sum_S P_j (log P_j - log m_j) + (1-b) sum_S q_j (log q_j - log m_j) + (1 - Q_S) g0
//   c = sum_v q_v g_v = (1-b) sum_S q_j (log q_j - log m_j) + (1 - Q_S) g0
// Nothing but the student's normalisers needs the whole row: ONE sweep (kd_fwd_kernel's sparse sweep with gjsd_fwd_kernel's
// unfolded exponent) and an epilogue over the K entries.  The backward is one read and one write of the row with one
// exponential per element at T == 2 (every off-support element is a1 softmax(s)_j + aT q_j (g0 - c)), then a fix-up of
// the at most K on-support elements after a barrier, as kd_bwd_kernel has it.
// An entry whose index is outside [0, V) or whose value is not finite carries no mass: it is dropped before the
// renormalisation and its index is never used as an address.  A merged mass below FLT_MIN counts as 0 (v_log_f32 takes no
// denormal): such an element is treated as off-support, which moves D by less than 1e-36.
namespace {

struct GjsdTopkStats {  // 12 floats per row; m .. c are what the backward reads (GjsdStats' conventions: log2 units)
  float m, ls1, lsT, c, valid, task, distill, teacher, hits, mv, sv, pad0;  // mv, sv: the teacher's renormalisation, so that
};                                                                            // the backward forms the forward's p_k bit for bit

typedef int i32x4 __attribute__((ext_vector_type(4)));

// The row's K entries -> LDS: k_i[k] the index (-1: dropped), k_p[k] = softmax(v / T)_k over the kept entries; both
// padded to a multiple of 4 with (-1, 0).  Thread t takes the entries t + u NF, u < E.  hv / hc: this thread's sum of v_k
// and count over its kept entries with i_k == y (the sparse forward KL's teacher monitor).  false: no entry is kept.
// mv, sv: the maximum of the kept v_k and the sum of exp((v_k - mv) / T).  GIVEN (the backward): they are the forward's,
// read from the row's stats -- no reduction here, and p_k does not depend on how many threads the caller runs.
template <int NF, int E, bool GIVEN>
SD_DEV bool tk_renorm(const _Float16* __restrict__ topv, const int32_t* __restrict__ topi, long kb, int K, int V, float kT,
                      long y, float* sc, int* k_i, float* k_p, float& hv, float& hc, float& mv, float& sv) {
  float v[E], mx = -INFINITY;
  int idx[E];
  hv = hc = 0.f;
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int k = threadIdx.x + u * NF;
    idx[u] = k < K ? topi[kb + k] : -1;
    v[u] = k < K ? (float)topv[kb + k] : -INFINITY;
    if (idx[u] < 0 || idx[u] >= V || !(fabsf(v[u]) < INFINITY)) {  // NaN fails the comparison
      idx[u] = -1;
      v[u] = -INFINITY;
    } else if ((long)idx[u] == y) {
      hv += v[u];
      hc += 1.f;
    }
    mx = fmaxf(mx, v[u]);
  }
  if constexpr (!GIVEN) {
    mv = block_max<NF>(mx, sc);
    if (mv == -INFINITY) return false;
  }
  float ev[E], se = 0.f;
#pragma unroll
  for (int u = 0; u < E; ++u) {
    ev[u] = idx[u] >= 0 ? __builtin_amdgcn_exp2f((v[u] - mv) * kT) : 0.f;
    se += ev[u];
  }
  if constexpr (!GIVEN) sv = block_sum<NF>(se, sc);
  const int K4 = (K + 3) & ~3;
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int k = threadIdx.x + u * NF;
    if (k < K4) {
      k_i[k] = idx[u];
      k_p[k] = ev[u] / sv;
    }
  }
  __syncthreads();
  return true;
}

// P of index idx over the K entries, summed in entry order whoever asks (so the forward and the backward get the same
// bits), and whether entry k is the first one that holds it.  Four entries per LDS read, every lane the same address.
// A thread without a kept entry (idx < 0) does not walk: a wave that holds none skips the loop altogether.
SD_DEV float tk_mass(const int* k_i, const float* k_p, int K, int k, int idx, bool& first) {
  first = idx >= 0;
  float P = 0.f;
  if (idx < 0) return P;
  for (int k2 = 0; k2 < K; k2 += 4) {
    const i32x4 ii = *(const i32x4*)(k_i + k2);
    const f32x4 pp = *(const f32x4*)(k_p + k2);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (ii[e] == idx) {
        P += pp[e];
        if (k2 + e < k) first = false;
      }
    }
  }
  return P;
}

// one on-support element: q_j, a2 = log2 q_j and lm = log2 m_j.  m: the row maximum, A0 = -log2 of the max-subtracted sum at T
SD_DEV void tk_term(float sj, float P, float m, float kT, float A0, float beta, float& q, float& a2, float& lm) {
  a2 = __builtin_fmaf(sj - m, kT, A0);
  q = __builtin_amdgcn_exp2f(a2);
  lm = __builtin_amdgcn_logf(fmaxf(__builtin_fmaf(1.f - beta, q, beta * P), GJ_FLT_MIN));  // v_log_f32 = log2
}

// Entry k of a row: its index (-1: none, or dropped) and the mass of that index, P = scale x tk_mass (scale: 1, or
// 1 - tau where the teacher has a tail bucket).  true: this entry owns the element -- it is the first one that holds
// the index, and P is a normal number (the support S of both families).
SD_DEV bool tk_entry(const int* k_i, const float* k_p, int K, int k, float scale, int& idx, float& P) {
  bool first = false;
  idx = k < K ? k_i[k] : -1;
  P = scale * tk_mass(k_i, k_p, K, k, idx, first);
  return first && P >= GJ_FLT_MIN;
}

// No register cap (kd_fwd_kernel's 8 waves per SIMD): held to 64 VGPRs every bf16 instantiation spills (20 / 108 bytes of
// scratch per lane); left alone they take 68 (NF = 512: three workgroups per CU) and 93-95 (NF = 1024: one).
template <typename T, bool T2, int NF>
__global__ __launch_bounds__(NF) void gjsd_topk_fwd_kernel(const T* __restrict__ S, const _Float16* __restrict__ topv,
                                                           const int32_t* __restrict__ topi,
                                                           const int64_t* __restrict__ labels,
                                                           GjsdTopkStats* __restrict__ stats, int V, int K,
                                                           float temperature, float beta) {
  __shared__ float sc[32];
  __shared__ __attribute__((aligned(16))) float k_p[NF];
  __shared__ __attribute__((aligned(16))) int k_i[NF];
  const int row = blockIdx.x;
  const long y = labels[row];
  const float invT = 1.f / temperature;
  const float k1 = GJ_LOG2E, kT = invT * k1;
  float hv = 0.f, hc = 0.f, mv = 0.f, sv = 0.f;
  // -100 (and anything outside the vocabulary) masks the row, and so does a teacher without a single kept entry
  if (y < 0 || y >= V || !tk_renorm<NF, 1, false>(topv, topi, (long)row * K, K, V, kT, y, sc, k_i, k_p, hv, hc, mv, sv))
    return masked_row(stats, row);
  const T* s = S + (long)row * V;
  // ---- the one sweep: the student's normalisers at 1 and at T, exponent unfolded
  float m = -INFINITY, s1 = 0.f, sT = 0.f;
  row_sweep<T, NF, false>(s, (const T*)nullptr, V, [&](int, const float* f, const float*) {
    online_raise<T2>(chunk_max8(f), invT, m, s1, sT);
#pragma unroll
    for (int e = 0; e < 8; ++e) unfolded_step<T2>(f[e], m, kT, k1, s1, sT);
  });
  block_merge<NF>(m, s1, sT, invT, sc);
  const float ls1 = __builtin_amdgcn_logf(s1), lsT = __builtin_amdgcn_logf(sT);  // v_log_f32: log2
  // ---- epilogue: one thread per entry; the first entry of an index owns its element of S
  int idx;
  float P, tp = 0.f, tq = 0.f, qs = 0.f;
  if (tk_entry(k_i, k_p, K, threadIdx.x, 1.f, idx, P)) {
    float q, a2, lm;
    tk_term((float)s[idx], P, m, kT, -lsT, beta, q, a2, lm);
    tp = P * (__builtin_amdgcn_logf(P) - lm);
    tq = q > 0.f ? q * (a2 - lm) : 0.f;
    qs = q;
  }
  const float Sp = block_sum<NF>(tp, sc), Sq = block_sum<NF>(tq, sc), Qs = block_sum<NF>(qs, sc);
  hv = block_sum<NF>(hv, sc);
  hc = block_sum<NF>(hc, sc);
  // c in log2 units and without the 1 - beta of g, as gjsd_fwd_kernel keeps it: sum_S q_j d_j + (1 - Q_S) d0
  const float c = __builtin_fmaf(fmaxf(1.f - Qs, 0.f), -__builtin_amdgcn_logf(1.f - beta), Sq);
  const float D = (beta * Sp + (1.f - beta) * c) * GJ_LN2;
  if (threadIdx.x == 0)
    stats[row] = GjsdTopkStats{m, ls1, lsT, c, 1.f, (m - (float)s[y]) + ls1 * GJ_LN2, D, hv, hc, mv, sv, 0.f};
}

// The backward of a row against a top-K teacher (both families; Stats: GjsdTopkStats or GjsdTailStats, `st` the row's):
// one read of the student row, one write of the gradient.  Every element is a1 (softmax(s)_j - e_y) plus
//   on S:  aT on_w(q_j, log2 q_j, log2 m_j, P_j),   off S:  aT d0c off(s_j, q_j, log2 q_j),
// aT = go (1 - alpha) T / N x gs.  The family gives gs (the units of on_w and d0c), the scale of P (tk_entry), d0c (what
// every off-support element of the row shares) and the two callables.
// G may alias S.  The on-support values fo[] are formed from gathers of s BEFORE the dense pass, and the first barrier
// stands between the two: every gather has returned (fo[] is computed from it) in EVERY wave before any wave stores,
// because with G == S the dense pass overwrites logits that another wave's entries point at (kd_bwd_kernel's barrier,
// same place).  The dense pass itself is row_sweep's case of a body that stores to its own chunk.  The second barrier
// (with its vmcnt(0)) completes every dense store of the row before the fix-up stores the at most K on-support elements.
template <typename T, bool T2, typename Stats, typename OnW, typename Off>
SD_DEV void tk_bwd_row(const T* S, const _Float16* __restrict__ topv, const int32_t* __restrict__ topi,
                       const int64_t* __restrict__ labels, const Stats& st, const float* __restrict__ loss_out,
                       const float* __restrict__ grad_out, T* G, int V, int K, float temperature, float alpha, float beta,
                       float gs, float scale, float d0c, OnW&& on_w, Off&& off) {
  constexpr int E = KMAX / GJ_NF;  // entries per thread
  __shared__ float sc[32];
  __shared__ __attribute__((aligned(16))) float k_p[KMAX];
  __shared__ __attribute__((aligned(16))) int k_i[KMAX];
  const int row = blockIdx.x;
  T* gr = G + (long)row * V;
  if (st.valid == 0.f) return zero_row<T, GJ_NF>(gr, V);
  const float invT = 1.f / temperature;
  const float k1 = GJ_LOG2E, kT = invT * k1;
  const float N = loss_out[4];
  const float go = grad_out ? grad_out[0] : 1.f;
  const float a1 = go * alpha / N;  // * (softmax(s) - e_y)
  const float aT = go * (1.f - alpha) * temperature / N * gs;
  const long y = labels[row];
  const T* s = S + (long)row * V;
  const float A0 = -st.lsT, L1 = -st.ls1;
  const float r1 = T2 ? __builtin_amdgcn_exp2f(2.f * st.lsT - st.ls1) : 0.f;  // softmax(s) = q^2 r1 at T == 2
  auto soft1 = [&](float f, float q) { return T2 ? q * q * r1 : __builtin_amdgcn_exp2f(__builtin_fmaf(f - st.m, k1, L1)); };
  float hv, hc, mv = st.mv, sv = st.sv;  // the forward's renormalisation (a valid row keeps an entry)
  tk_renorm<GJ_NF, E, true>(topv, topi, (long)row * K, K, V, kT, y, sc, k_i, k_p, hv, hc, mv, sv);
  int fi[E];
  float fo[E];
#pragma unroll
  for (int u = 0; u < E; ++u) {
    int idx;
    float P;
    fi[u] = -1;
    fo[u] = 0.f;
    if (tk_entry(k_i, k_p, K, threadIdx.x + u * GJ_NF, scale, idx, P)) {
      const float sj = (float)s[idx];
      float q, a2, lm;
      tk_term(sj, P, st.m, kT, A0, beta, q, a2, lm);
      fi[u] = idx;
      fo[u] = __builtin_fmaf(a1, soft1(sj, q), aT * on_w(q, a2, lm, P)) - ((long)idx == y ? a1 : 0.f);
    }
  }
  __syncthreads();
  const float w0 = aT * d0c;
  row_sweep<T, GJ_NF, false>(s, (const T*)nullptr, V, [&](int c, const float* f, const float*) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float a2 = __builtin_fmaf(f[e] - st.m, kT, A0);
      const float q = __builtin_amdgcn_exp2f(a2);
      o[e] = __builtin_fmaf(a1, soft1(f[e], q), w0 * off(f[e], q, a2));
    }
    if (y >= c && y < c + 8) o[y - c] -= a1;
    Ld8<T>::store(gr + c, o);
  });
  __syncthreads();
#pragma unroll
  for (int u = 0; u < E; ++u)
    if (fi[u] >= 0) gr[fi[u]] = (T)fo[u];
}

// tk_bwd_row with the JSD's weights, in log2 units: on S q (d - c), d = log2 q - log2 m; off S every element has
// d_0 = -log2(1 - beta)
template <typename T, bool T2>
__global__ __launch_bounds__(GJ_NF) void gjsd_topk_bwd_kernel(const T* S, const _Float16* __restrict__ topv,
                                                              const int32_t* __restrict__ topi,
                                                              const int64_t* __restrict__ labels,
                                                              const GjsdTopkStats* __restrict__ stats,
                                                              const float* __restrict__ loss_out,
                                                              const float* __restrict__ grad_out, T* G, int V, int K,
                                                              float temperature, float alpha, float beta) {
  const GjsdTopkStats st = stats[blockIdx.x];
  tk_bwd_row<T, T2>(S, topv, topi, labels, st, loss_out, grad_out, G, V, K, temperature, alpha, beta, (1.f - beta) * GJ_LN2,
                    1.f, -__builtin_amdgcn_logf(1.f - beta) - st.c,
                    [&](float q, float a2, float lm, float) { return q > 0.f ? q * ((a2 - lm) - st.c) : 0.f; },
                    [](float, float q, float) { return q; });
}

int gjsd_topk_check(const void* S, const void* topv, const void* topi, const int64_t* labels, const void* stats,
                    const float* out, int R, int V, int K, float temperature, float beta, int dtype, bool G = false,
                    const void* grad = nullptr) {
  return gjsd_check(S, nullptr, labels, stats, out, R, V, temperature, beta, true, dtype,
                    (!topv || !topi) ? SD_ERR_NO_TEACHER : (K <= 0 || K > KMAX) ? SD_ERR_SHAPE : 0, 0, G, grad);
}

}  // namespace

extern "C" int64_t sd_gjsd_topk_stats_bytes(int R) { return (int64_t)R * sizeof(GjsdTopkStats); }

extern "C" int sd_gjsd_topk_fwd_rows(const void* student_logits, const void* top_k_v, const void* top_k_i,
                                     const int64_t* row_labels, void* row_stats, float* loss_out, int R, int V, int K,
                                     float temperature, float alpha, float beta, int dtype, void* stream) {
  if (int e = gjsd_topk_check(student_logits, top_k_v, top_k_i, row_labels, row_stats, loss_out, R, V, K, temperature, beta, dtype))
    return e;
  hipStream_t st = (hipStream_t)stream;
  return rows_launch(dtype, SD_K_LOSS_FWD, (double)R * V, st, false, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    by_flag(temperature == 2.0f, [&](auto t2) {
      by_threads(K, [&](auto nf) {
        constexpr int NF = SD_FLAG(nf);
        SD_PROF_LABEL("gjsd_topk_fwd_kernel<%s, %s, %d>", type_name(sizeof(T)), flag_name(SD_FLAG(t2)), NF);
        hipLaunchKernelGGL((gjsd_topk_fwd_kernel<T, SD_FLAG(t2), NF>), dim3(R), dim3(NF), 0, st, (const T*)student_logits,
                           (const _Float16*)top_k_v, (const int32_t*)top_k_i, row_labels, (GjsdTopkStats*)row_stats, V, K,
                           temperature, beta);
      });
    });
  }, finalize<GjsdTopkStats, true>(row_stats, loss_out, R, temperature, alpha, 0, st));
}

extern "C" int sd_gjsd_topk_bwd_rows(const void* student_logits, const void* top_k_v, const void* top_k_i,
                                     const int64_t* row_labels, const void* row_stats, const float* loss_out,
                                     const float* grad_total, void* grad_logits, int R, int V, int K, float temperature,
                                     float alpha, float beta, int dtype, void* stream) {
  if (int e = gjsd_topk_check(student_logits, top_k_v, top_k_i, row_labels, row_stats, loss_out, R, V, K, temperature, beta, dtype,
                              true, grad_logits))
    return e;
  hipStream_t st = (hipStream_t)stream;
  return rows_launch(dtype, SD_K_LOSS_BWD, (double)R * V * 2, st, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    by_flag(temperature == 2.0f, [&](auto t2) {
      SD_PROF_LABEL("gjsd_topk_bwd_kernel<%s, %s>", type_name(sizeof(T)), flag_name(SD_FLAG(t2)));
      hipLaunchKernelGGL((gjsd_topk_bwd_kernel<T, SD_FLAG(t2)>), dim3(R), dim3(GJ_NF), 0, st, (const T*)student_logits,
                         (const _Float16*)top_k_v, (const int32_t*)top_k_i, row_labels, (const GjsdTopkStats*)row_stats,
                         loss_out, grad_total, (T*)grad_logits, V, K, temperature, alpha, beta);
    });
  });
}

// ---------------------------------------------------------------------- top-K teacher with a tail bucket: KL, reverse KL, JSD
// The top-K teacher of above plus ONE number per row: tau, the teacher's mass outside its top-K at T (sd_topk_tail).
// Teacher and student are compared as distributions over K + 1 outcomes -- the indices of S and bucket 0, "anything else":
//   P_j = (1 - tau) sum_{k: i_k = j} p_k on S,  P_0 = tau;   q_j = softmax(s / T)_j on S,  q_0 = sum_{j not in S} q_j
//   SD_DIV_FORWARD_KL  D = sum_b P_b (log P_b - log q_b)         d D / d s_j = (q_j - P_j) / T on S, q_j (1 - tau / q_0) / T off
//   SD_DIV_REVERSE_KL  D = sum_b q_b (log q_b - log P_b)         g_b = log q_b - log P_b  (+ 1)
//   SD_DIV_JSD         D = b sum_b P_b (log P_b - log m_b) + (1-b) sum_b q_b (log q_b - log m_b),  g_b = (1-b)(log q_b - log m_b)
//   d D / d s_j = q_j (g_b(j) - c) / T,  c = sum_b q_b g_b;  every off-support element shares g_0.
// p, the kept entries and the duplicate merge are tk_renorm / tk_mass; S = {j : P_j >= FLT_MIN}.
// Forward: the members of S are marked in an LDS bitmap (sd_rows.cuh) BEFORE the sweep, and the sweep takes the online
// (max, sum-exp at 1, sum-exp at T) over the OFF-support elements only, with their own maximum m0: log q_0 =
// (m0 - m) / T + log sum0 - log sumT never passes through q_0 (a student spike of 200 on a support index leaves q_0 =
// 1e-80, and 1 - Q_S = 0).  The at most K on-support logits are gathered in the epilogue and added to the normalisers.
// Backward: gjsd_topk_bwd_kernel's shape; no bitmap (the fix-up overwrites the on-support elements).  The forward KL's
// off-support element is q_j - tau q_j / q_0 = q_j - exp2(log2 q_j + log2 tau - log2 q_0): the second exponential is the
// price of never forming tau / q_0, which overflows where q_0 underflows.
namespace {

struct GjsdTailStats {  // 12 floats per row, GjsdTopkStats' layout with log2 q_0 in its last slot
  float m, ls1, lsT, c, valid, task, distill, teacher, hits, mv, sv, lq0;
};

constexpr float GJ_TAIL_MIN = 0x1p-100f;  // a tail in [0, 2^-100) counts as 2^-100

// tau of a row that is not masked by it: in [0, 1), NaN fails
SD_DEV bool tail_ok(float tau) { return tau >= 0.f && tau < 1.f; }

// log2 m_0 of the JSD's bucket 0, m_0 = (1 - beta) q_0 + beta tau, from log2 q_0 and log2 tau: in log space
SD_DEV float tail_lm0(float lq0, float lt, float beta) {
  const float a = __builtin_amdgcn_logf(1.f - beta) + lq0, b = __builtin_amdgcn_logf(beta) + lt;
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  return hi + __builtin_amdgcn_logf(1.f + __builtin_amdgcn_exp2f(lo - hi));
}

// No register cap, as gjsd_topk_fwd_kernel (see the note in front of it).
template <typename T, bool T2, int NF>
__global__ __launch_bounds__(NF) void gjsd_tail_fwd_kernel(const T* __restrict__ S, const _Float16* __restrict__ topv,
                                                           const int32_t* __restrict__ topi,
                                                           const float* __restrict__ tail,
                                                           const int64_t* __restrict__ labels,
                                                           GjsdTailStats* __restrict__ stats, int V, int K,
                                                           float temperature, float beta, int mode) {
  extern __shared__ __attribute__((aligned(16))) uint32_t row_bits[];
  __shared__ float sc[32];
  __shared__ __attribute__((aligned(16))) float k_p[NF];
  __shared__ __attribute__((aligned(16))) int k_i[NF];
  const int row = blockIdx.x;
  const long y = labels[row];
  const float invT = 1.f / temperature;
  const float k1 = GJ_LOG2E, kT = invT * k1;
  const float tau_in = tail[row];
  float hv = 0.f, hc = 0.f, mv = 0.f, sv = 0.f;
  if (y < 0 || y >= V || !tail_ok(tau_in) ||
      !tk_renorm<NF, 1, false>(topv, topi, (long)row * K, K, V, kT, y, sc, k_i, k_p, hv, hc, mv, sv))
    return masked_row(stats, row);
  const float tau = fmaxf(tau_in, GJ_TAIL_MIN);
  const T* s = S + (long)row * V;
  // ---- the support: one thread per entry; the first entry of an index owns its element of S and marks it
  row_bits_clear<NF>(row_bits, V);
  int idx;
  float P;
  const bool on = tk_entry(k_i, k_p, K, threadIdx.x, 1.f - tau, idx, P);
  __syncthreads();
  if (on) row_bits_set(row_bits, idx);
  __syncthreads();
  // ---- the one sweep: the OFF-support normalisers at 1 and at T with their own maximum, exponent unfolded
  float m0 = -INFINITY, s1 = 0.f, sT = 0.f;
  row_sweep<T, NF, false>(s, (const T*)nullptr, V, [&](int c, const float* f, const float*) {
    const unsigned b = row_bits_chunk(row_bits, c);
    float g[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = ((b >> e) & 1u) ? -INFINITY : f[e];
    const float cm = chunk_max8(g);
    if (cm == -INFINITY) return;  // a chunk of members only
    online_raise<T2>(cm, invT, m0, s1, sT);
#pragma unroll
    for (int e = 0; e < 8; ++e) unfolded_step<T2>(g[e], m0, kT, k1, s1, sT);
  });
  block_merge<NF>(m0, s1, sT, invT, sc);
  const float ls0 = __builtin_amdgcn_logf(sT);  // v_log_f32: log2
  // ---- epilogue: the on-support logits join the normalisers, then the K + 1 terms
  const float sj = on ? (float)s[idx] : -INFINITY;
  const float m = block_max<NF>(fmaxf(m0, sj), sc);
  const float eT = on ? __builtin_amdgcn_exp2f((sj - m) * kT) : 0.f;
  const float e1 = on ? (T2 ? eT * eT : __builtin_amdgcn_exp2f((sj - m) * k1)) : 0.f;
  const float d0 = m0 - m;
  sT = __builtin_fmaf(sT, __builtin_amdgcn_exp2f(d0 * kT), block_sum<NF>(eT, sc));
  s1 = __builtin_fmaf(s1, __builtin_amdgcn_exp2f(d0 * k1), block_sum<NF>(e1, sc));
  const float ls1 = __builtin_amdgcn_logf(s1), lsT = __builtin_amdgcn_logf(sT);
  const float lq0 = __builtin_fmaf(d0, kT, ls0) - lsT;
  float tp = 0.f, tq = 0.f;
  if (on) {
    float q, a2, lm;
    tk_term(sj, P, m, kT, -lsT, beta, q, a2, lm);
    const float lP = __builtin_amdgcn_logf(P);
    if (mode == SD_DIV_FORWARD_KL) {
      tp = P * (lP - a2);
    } else {
      const float ref = mode == SD_DIV_JSD ? lm : lP;
      tq = q > 0.f ? q * (a2 - ref) : 0.f;
      if (mode == SD_DIV_JSD) tp = P * (lP - lm);
    }
  }
  float Sp = block_sum<NF>(tp, sc), Sq = block_sum<NF>(tq, sc);
  hv = block_sum<NF>(hv, sc);
  hc = block_sum<NF>(hc, sc);
  // bucket 0, and c in log2 units without the 1 - beta of the JSD's g (gjsd_fwd_kernel's convention)
  const float lt = __builtin_amdgcn_logf(tau), q0 = __builtin_amdgcn_exp2f(lq0);
  float D;
  if (mode == SD_DIV_FORWARD_KL) {
    Sp = __builtin_fmaf(tau, lt - lq0, Sp);
    D = Sp * GJ_LN2;
  } else if (mode == SD_DIV_REVERSE_KL) {
    Sq = __builtin_fmaf(q0, lq0 - lt, Sq);
    D = Sq * GJ_LN2;
  } else {
    const float lm0 = tail_lm0(lq0, lt, beta);
    Sp = __builtin_fmaf(tau, lt - lm0, Sp);
    Sq = __builtin_fmaf(q0, lq0 - lm0, Sq);
    D = (beta * Sp + (1.f - beta) * Sq) * GJ_LN2;
  }
  if (threadIdx.x == 0)
    stats[row] = GjsdTailStats{m, ls1, lsT, Sq, 1.f, (m - (float)s[y]) + ls1 * GJ_LN2, D, hv, hc, mv, sv, lq0};
}

// tk_bwd_row with P scaled by 1 - tau and the weights of the K + 1 outcomes.  Forward KL: q - P on S, and off S
// q_j - tau q_j / q_0 = q_j - exp2(log2 q_j + dl), in natural units.  The others, in log2 units: q (d - c) on S with
// d = log2 q - log2 P (reverse KL) or log2 q - log2 m (JSD), and the row's d_0 - c times q_j off S.
template <typename T, bool T2, int MODE>
__global__ __launch_bounds__(GJ_NF) void gjsd_tail_bwd_kernel(const T* S, const _Float16* __restrict__ topv,
                                                              const int32_t* __restrict__ topi,
                                                              const float* __restrict__ tail,
                                                              const int64_t* __restrict__ labels,
                                                              const GjsdTailStats* __restrict__ stats,
                                                              const float* __restrict__ loss_out,
                                                              const float* __restrict__ grad_out, T* G, int V, int K,
                                                              float temperature, float alpha, float beta) {
  constexpr bool FKL = MODE == SD_DIV_FORWARD_KL, JSD = MODE == SD_DIV_JSD;
  const GjsdTailStats st = stats[blockIdx.x];
  const float tau = fmaxf(tail[blockIdx.x], GJ_TAIL_MIN);  // (a valid row's tau passed tail_ok in the forward)
  const float lt = __builtin_amdgcn_logf(tau);
  const float dl = lt - st.lq0;
  tk_bwd_row<T, T2>(S, topv, topi, labels, st, loss_out, grad_out, G, V, K, temperature, alpha, beta,
                    FKL ? 1.f : (JSD ? (1.f - beta) * GJ_LN2 : GJ_LN2), 1.f - tau,
                    FKL ? 1.f : (st.lq0 - (JSD ? tail_lm0(st.lq0, lt, beta) : lt)) - st.c,
                    [&](float q, float a2, float lm, float P) {
                      if constexpr (FKL) {
                        return q - P;
                      } else {
                        const float ref = JSD ? lm : __builtin_amdgcn_logf(P);
                        return q > 0.f ? q * ((a2 - ref) - st.c) : 0.f;
                      }
                    },
                    [&](float, float q, float a2) { return FKL ? q - __builtin_amdgcn_exp2f(a2 + dl) : q; });
}

constexpr int GJ_TAIL_VMAX = 458752;  // the forward's V-bit bitmap beside its other LDS: 56 KB of the 64 KB

int gjsd_tail_check(const void* S, const void* topv, const void* topi, const float* tail, const int64_t* labels,
                    const void* stats, const float* out, int R, int V, int K, float temperature, float beta, int mode,
                    int dtype, bool G = false, const void* grad = nullptr) {
  const bool known = mode == SD_DIV_FORWARD_KL || mode == SD_DIV_REVERSE_KL || mode == SD_DIV_JSD;
  return gjsd_check(S, nullptr, labels, stats, out, R, V, temperature, beta, mode == SD_DIV_JSD, dtype,
                    (!topv || !topi || !tail) ? SD_ERR_NO_TEACHER
                    : (K <= 0 || K > KMAX || K >= V) ? SD_ERR_SHAPE : 0,  // K < V: an off-support element always exists
                    (!known || V > GJ_TAIL_VMAX) ? SD_ERR_UNSUPPORTED : 0, G, grad);
}

}  // namespace

extern "C" int64_t sd_gjsd_tail_stats_bytes(int R) { return (int64_t)R * sizeof(GjsdTailStats); }

extern "C" int sd_gjsd_tail_fwd_rows(const void* student_logits, const void* top_k_v, const void* top_k_i,
                                     const float* top_k_tail, const int64_t* row_labels, void* row_stats, float* loss_out,
                                     int R, int V, int K, float temperature, float alpha, float beta, int mode, int dtype,
                                     void* stream) {
  if (int e = gjsd_tail_check(student_logits, top_k_v, top_k_i, top_k_tail, row_labels, row_stats, loss_out, R, V, K,
                              temperature, beta, mode, dtype))
    return e;
  hipStream_t st = (hipStream_t)stream;
  return rows_launch(dtype, SD_K_LOSS_FWD, (double)R * V, st, false, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    by_flag(temperature == 2.0f, [&](auto t2) {
      by_threads(K, [&](auto nf) {
        constexpr int NF = SD_FLAG(nf);
        SD_PROF_LABEL("gjsd_tail_fwd_kernel<%s, %s, %d>", type_name(sizeof(T)), flag_name(SD_FLAG(t2)), NF);
        hipLaunchKernelGGL((gjsd_tail_fwd_kernel<T, SD_FLAG(t2), NF>), dim3(R), dim3(NF), row_bits_bytes(V), st,
                           (const T*)student_logits, (const _Float16*)top_k_v, (const int32_t*)top_k_i, top_k_tail,
                           row_labels, (GjsdTailStats*)row_stats, V, K, temperature, beta, mode);
      });
    });
  }, finalize<GjsdTailStats, true>(row_stats, loss_out, R, temperature, alpha, 0, st));
}

extern "C" int sd_gjsd_tail_bwd_rows(const void* student_logits, const void* top_k_v, const void* top_k_i,
                                     const float* top_k_tail, const int64_t* row_labels, const void* row_stats,
                                     const float* loss_out, const float* grad_total, void* grad_logits, int R, int V, int K,
                                     float temperature, float alpha, float beta, int mode, int dtype, void* stream) {
  if (int e = gjsd_tail_check(student_logits, top_k_v, top_k_i, top_k_tail, row_labels, row_stats, loss_out, R, V, K,
                              temperature, beta, mode, dtype, true, grad_logits))
    return e;
  hipStream_t st = (hipStream_t)stream;
  return rows_launch(dtype, SD_K_LOSS_BWD, (double)R * V * 2, st, [&](auto tt) {
    typedef SD_TAG_TYPE(tt) T;
    by_flag(temperature == 2.0f, [&](auto t2) {
      auto go = [&](auto md) {
        constexpr int MODE = decltype(md)::value;
        SD_PROF_LABEL("gjsd_tail_bwd_kernel<%s, %s, %d>", type_name(sizeof(T)), flag_name(SD_FLAG(t2)), MODE);
        hipLaunchKernelGGL((gjsd_tail_bwd_kernel<T, SD_FLAG(t2), MODE>), dim3(R), dim3(GJ_NF), 0, st,
                           (const T*)student_logits, (const _Float16*)top_k_v, (const int32_t*)top_k_i, top_k_tail,
                           row_labels, (const GjsdTailStats*)row_stats, loss_out, grad_total, (T*)grad_logits, V, K,
                           temperature, alpha, beta);
      };
      if (mode == SD_DIV_FORWARD_KL) go(std::integral_constant<int, SD_DIV_FORWARD_KL>{});
      else if (mode == SD_DIV_REVERSE_KL) go(std::integral_constant<int, SD_DIV_REVERSE_KL>{});
      else go(std::integral_constant<int, SD_DIV_JSD>{});
    });
  });
}

