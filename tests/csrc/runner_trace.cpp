// Launch trace of the decoder runner (speech_distill_amd/csrc/sd_model.hip) without a GPU.  The runner never reads
// device memory: it computes addresses and calls other entries.  This program defines every symbol the runner's object
// leaves undefined -- the sd_* entries, the few HIP runtime calls, the debug / profiler state -- as a stub that appends
// one line to a trace, and drives the runner with fabricated, well-separated base addresses, so that every line is
// deterministic.  It is linked against the runner's object only (no HIP runtime library): it cannot open a GPU.
//
//   runner_trace OUTDIR     writes OUTDIR/<case>.txt for every case; tests/test_runner_trace_cpu.py compares them byte
//                           for byte with tests/golden/runner_trace/, recorded before the runner was split into steps.
//
// Pointers print as <region>[.<sub-buffer>][+<hex offset>] (A acts, S scratch, C cache / pool, LG logits, DL dlogits, P / G
// top-level params / grads, P<l> / G<l> layer l, IN batch inputs, X dx0_out, U callback user), streams as S1 (main) / S2
// (side), events as E<index in the leased set>.  Host arrays (GEMM / column-sum problems, the varlen descriptor) print their
// contents.  GEMM-family lines end with |<value of t_sd_shared_gpu>.  Stubs that only log are not written out here: the
// test writes runner_trace_stubs.inc from the prototypes of sd_hip.h.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/sd_hip.h"
#include "../../speech_distill_amd/csrc/sd_debug.h"

struct ihipStream_t;
struct ihipEvent_t;
typedef ihipStream_t* hipStream_t;
typedef ihipEvent_t* hipEvent_t;
struct dim3 { unsigned x, y, z; };

SdDebug g_sd_debug;
thread_local int t_sd_shared_gpu = 0;
bool sd_prof_enabled = false;
void sd_prof_open(int, double, hipStream_t, int*) {}
void sd_prof_close(int, hipStream_t) {}
void sd_prof_label(const char*, ...) {}

namespace {

// ------------------------------------------------------------------------------------------------ fabricated addresses
enum Region { R_ACTS = 1, R_SCRATCH, R_CACHE, R_LOGITS, R_DLOGITS, R_P, R_G, R_IN, R_DX0, R_USER, R_STREAM, R_EVENT,
              R_PL = 0x20, R_GL = 0x40 };
char* addr(int region, int sub = 0) { return (char*)(((uintptr_t)region << 40) | ((uintptr_t)sub << 32)); }
void* const kMain = addr(R_STREAM, 1);
void* const kSide = addr(R_STREAM, 2);

std::string ptr_name(const void* p) {  // <region>[.<sub-buffer>][+<hex offset>]
  if (!p) return "0";
  const uintptr_t v = (uintptr_t)p;
  const int r = (int)(v >> 40), sub = (int)(v >> 32) & 255;
  const unsigned long long off = v & 0xffffffffull;
  static const char* names[] = {"?", "A", "S", "C", "LG", "DL", "P", "G", "IN", "X", "U", "S", "E"};
  char b[64];
  if (r == R_STREAM || r == R_EVENT) { snprintf(b, sizeof b, "%s%d", names[r], sub); return b; }
  int n;
  if (r >= R_GL && r < R_GL + 16) n = snprintf(b, sizeof b, "G%d", r - R_GL);
  else if (r >= R_PL && r < R_PL + 16) n = snprintf(b, sizeof b, "P%d", r - R_PL);
  else if (r >= R_ACTS && r <= R_USER) n = snprintf(b, sizeof b, "%s", names[r]);
  else n = snprintf(b, sizeof b, "?%d", r);
  if (sub) n += snprintf(b + n, sizeof b - n, ".%d", sub);
  if (off || !sub) snprintf(b + n, sizeof b - n, "+%llx", off);
  return b;
}

// ------------------------------------------------------------------------------------------------ the trace
enum Knob { K_ZERO, K_UNSUP, K_SLAB1, K_SLAB3, K_SLABMIX };
std::vector<std::string> g_trace;
bool g_on = false;
int g_knob = K_ZERO;
int g_partial_calls = 0;

void put(std::string& s, int v) { s += std::to_string(v); }
void put(std::string& s, unsigned v) { s += std::to_string(v); }
void put(std::string& s, long v) { s += std::to_string(v); }
void put(std::string& s, unsigned long v) { s += std::to_string(v); }
void put(std::string& s, float v) { char b[32]; snprintf(b, sizeof b, "%.9g", v); s += b; }
void put(std::string& s, const std::string& v) { s += v; }
template <class T> void put(std::string& s, T* p) { s += ptr_name((const void*)p); }

// the entries that may answer SD_ERR_UNSUPPORTED (K_UNSUP): the runner then takes its two-kernel form
bool refuses(const char* name) {
  for (const char* f : {"sd_gemm_qkv_rope", "sd_gemm_swiglu", "sd_gemm_swiglu_bwd", "sd_gemm_odx_delta", "sd_gemm_grouped_tn",
                        "sd_gemv_check"})
    if (!strcmp(name, f)) return g_knob == K_UNSUP;
  return false;
}
template <class... A> int rec(const char* name, A... a) {
  const int rc = refuses(name) ? SD_ERR_UNSUPPORTED : 0;
  if (!g_on) return rc;
  std::string s = name;
  s += '(';
  int i = 0;
  ((s += (i++ ? " " : ""), put(s, a)), ...);
  s += ')';
  if (!strncmp(name, "sd_gemm", 7) || !strncmp(name, "sd_gemv", 7)) s += " |" + std::to_string(t_sd_shared_gpu);
  g_trace.push_back(s);
  return rc;
}
#define REC(...) rec(__func__, __VA_ARGS__)

}  // namespace

// ------------------------------------------------------------------------------------------------ HIP runtime stubs
extern "C" {
static hipEvent_t g_next_event = (hipEvent_t)addr(R_EVENT, 0);
static int g_get_device_rc = 0;
int hipGetDevice(int* dev) { *dev = 0; return g_get_device_rc; }
int hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  *e = g_next_event;
  g_next_event = (hipEvent_t)((char*)g_next_event + ((uintptr_t)1 << 32));
  return REC(*e, flags);
}
int hipEventDestroy(hipEvent_t e) { return REC(e); }
int hipEventRecord(hipEvent_t e, hipStream_t st) { return REC(e, st); }
int hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned flags) { return REC(st, e, flags); }
int hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t st) { return REC(dst, value, bytes, st); }
int hipGetLastError(void) { return 0; }
static dim3 g_grid, g_block;
static size_t g_shmem;
static hipStream_t g_cfg_stream;
int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t st) {
  g_grid = grid; g_block = block; g_shmem = shmem; g_cfg_stream = st;
  return 0;
}
int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* st) {
  *grid = g_grid; *block = g_block; *shmem = g_shmem; *st = g_cfg_stream;
  return 0;
}
// the runner's only kernel: head_dw_strip_kernel(dY, X, dW, lo, hi, ldy, H, K, acc)
int hipLaunchKernel(const void*, dim3 grid, dim3 block, void** a, size_t shmem, hipStream_t st) {
  return rec("head_dw_strip_kernel", grid.x, block.x, shmem, st, *(void**)a[0], *(void**)a[1], *(void**)a[2], *(int*)a[3],
             *(int*)a[4], *(int*)a[5], *(int*)a[6], *(int*)a[7], *(int*)a[8]);
}
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
}

// ------------------------------------------------------------------------------------------------ hidden library entries
int sd_gemv_check(const void* x, const void* w, const void* y, const void* r, const void* norm_gain, int M, int N, int K,
                  int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr) {
  return REC(x, w, y, r, norm_gain, M, N, K, ldx, ldw, ldy, ldr);
}
int sd_rope_rows_at(const void* cos_tab, const void* sin_tab, const int32_t* past, void* cos_out, void* sin_out, int B, int T,
                    int cap, void* stream) {
  return REC(cos_tab, sin_tab, past, cos_out, sin_out, B, T, cap, stream);
}

// ------------------------------------------------------------------------------------------------ sd_* entry stubs
extern "C" {
int64_t sd_gemm_splitk_workspace_bytes(int M, int N, int K) { return (int64_t)M * N * 4 * 3 + K; }
int64_t sd_rmsnorm_bwd_workspace_bytes(int M, int H) { return (int64_t)64 * H * 4 + M; }
int64_t sd_qknorm_rope_bwd_workspace_bytes(int M, int Hq, int Hkv) { return (int64_t)32 * 256 * 4 + M + Hq + Hkv; }
int sd_rmsnorm_bwd_partial_rows(int M, int H) { return 64; }
int sd_qknorm_rope_bwd_partial_rows(int M, int Hq, int Hkv) { return 32; }
int64_t sd_kvcache_bytes(const sd_qwen3_dims* d, int B, int cap) {
  return (int64_t)d->layers * 2 * B * cap * d->n_kv * d->head_dim * 2;
}
int64_t sd_kvpool_bytes(const sd_qwen3_dims* d, int n_pages) {
  return (int64_t)d->layers * 2 * n_pages * SD_KV_PAGE * d->n_kv * d->head_dim * 2;
}
int64_t sd_attn_decode_workspace_bytes(int B, int Hq, int cap) { return (int64_t)B * Hq * ((cap + 255) / 256) * 130 * 4; }

int sd_gemm_bf16_splitk_partial(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb,
                                int64_t ldc, int trans_a, int trans_b, void* workspace, int64_t workspace_bytes,
                                int* nsplit_out, void* stream) {
  const int n = g_partial_calls++;
  if (g_knob == K_SLAB1) *nsplit_out = 1;
  if (g_knob == K_SLAB3) *nsplit_out = 3;
  if (g_knob == K_SLABMIX) *nsplit_out = (n & 1) ? 1 : 3;
  return REC(A, B, C, M, N, K, lda, ldb, ldc, trans_a, trans_b, workspace, workspace_bytes, std::string("nsplit=") +
             std::to_string(*nsplit_out), stream);
}
int sd_gemm_grouped_tn(const sd_gemm_problem* pr, int n, int K, int accumulate, void* stream) {
  std::string s;
  for (int i = 0; i < n; ++i) {
    s += i ? " {" : "{";
    s += ptr_name(pr[i].A) + " " + ptr_name(pr[i].B) + " " + ptr_name(pr[i].C) + " " + std::to_string(pr[i].lda) + " " +
         std::to_string(pr[i].ldb) + " " + std::to_string(pr[i].ldc) + " " + std::to_string(pr[i].M) + " " +
         std::to_string(pr[i].N) + "}";
  }
  return REC(s, n, K, accumulate, stream);
}
int sd_colsum_reduce_batch(const sd_colsum_problem* cp, int n, void* stream) {
  std::string s;
  for (int i = 0; i < n; ++i) {
    s += i ? " {" : "{";
    s += ptr_name(cp[i].partials) + " " + ptr_name(cp[i].out) + " " + std::to_string(cp[i].nb) + " " +
         std::to_string(cp[i].H) + " " + std::to_string(cp[i].stride) + " " + std::to_string(cp[i].accumulate) + "}";
  }
  return REC(s, n, stream);
}
static std::string varlen(const sd_varlen* vl) {
  return "{" + ptr_name(vl->cu_seqlens) + " " + std::to_string(vl->n_seqs) + " " + std::to_string(vl->max_seqlen) + " " +
         ptr_name(vl->work) + "}";
}
int sd_attn_fwd_varlen(const void* q, const void* k, const void* v, void* o, float* lse, const sd_varlen* vl, int64_t ldq,
                       int64_t ldk, int64_t ldv, int64_t ldo, int M, int Hq, int Hkv, int head_dim, float scale, void* stream) {
  return REC(q, k, v, o, lse, varlen(vl), ldq, ldk, ldv, ldo, M, Hq, Hkv, head_dim, scale, stream);
}
int sd_attn_bwd_varlen(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                       float* delta, void* dq, void* dk, void* dv, const sd_varlen* vl, int64_t ldq, int64_t ldk, int64_t ldv,
                       int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, int M, int Hq, int Hkv, int head_dim, float scale,
                       void* side_stream, void* stream) {
  return REC(q, k, v, o, d_o, lse, delta, dq, dk, dv, varlen(vl), ldq, ldk, ldv, ldo, lddq, lddk, lddv, M, Hq, Hkv, head_dim,
             scale, side_stream, stream);
}
// every other int-returning entry of sd_hip.h: "return REC(<its parameters>);", written by tests/test_runner_trace_cpu.py
#include "runner_trace_stubs.inc"
}  // extern "C"

// ------------------------------------------------------------------------------------------------ driving the runner
namespace {

const char* g_outdir;
int g_failures = 0;

struct Model {
  sd_qwen3_dims d;
  sd_qwen3_layer pl[16], gl[16];
  sd_qwen3_params p, g;
  Model(int L, int hidden = 128, bool tied = false) {
    d = {520, hidden, 192, L, 4, 2, 128, tied ? 1 : 0, 1e-6f, 0};
    for (int l = 0; l < L; ++l) {
      void** pw = (void**)&pl[l];
      void** gw = (void**)&gl[l];
      for (int f = 0; f < 8; ++f) { pw[f] = addr(R_PL + l, f); gw[f] = addr(R_GL + l, f); }
    }
    p = {addr(R_P, 0), tied ? addr(R_P, 0) : addr(R_P, 1), addr(R_P, 2), pl};
    g = {addr(R_G, 0), tied ? addr(R_G, 0) : addr(R_G, 1), addr(R_G, 2), gl};
  }
};

void begin(int knob) {
  g_trace.clear();
  g_knob = knob;
  g_partial_calls = 0;
  g_sd_debug = SdDebug();
  g_on = true;
}
void finish(const std::string& name, int rc) {
  g_on = false;
  g_trace.push_back("-> " + std::to_string(rc));
  const std::string path = std::string(g_outdir) + "/" + name + ".txt";
  FILE* f = fopen(path.c_str(), "w");
  if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); ++g_failures; return; }
  for (const std::string& s : g_trace) fprintf(f, "%s\n", s.c_str());
  fclose(f);
}

void on_grads(int stage, void* user) { rec("on_grads_ready", stage, user); }

const sd_varlen kVl = {(const int32_t*)addr(R_IN, 5), 3, 20, nullptr};
sd_qwen3_batch batch(bool head_rows, bool vl, int B = 2, int T = 24) {
  sd_qwen3_batch bt = {};
  bt.ids = (const int64_t*)addr(R_IN, 0);
  bt.kv_len = vl ? nullptr : (const int32_t*)addr(R_IN, 1);
  bt.vl = vl ? &kVl : nullptr;
  bt.cos_tab = addr(R_IN, 2);
  bt.sin_tab = addr(R_IN, 3);
  bt.head_rows = head_rows ? (const int64_t*)addr(R_IN, 4) : nullptr;
  bt.n_head_rows = head_rows ? 17 : 0;
  bt.B = vl ? 1 : B;
  bt.T = vl ? B * T : T;
  return bt;
}

struct Bwd {
  const char* name;
  bool side;
  int mask, flags, row_lo;
  bool head_rows, vl, dx0, cb;
  int knob;
  bool tied;
};

int run_bwd(const Model& m, const sd_qwen3_batch* bt, const sd_qwen3_bwd_opts* o, int64_t acts_slack = 0,
            int64_t scratch_slack = 0) {
  const int save = (o && (o->flags & SD_BWD_RECOMPUTE)) ? SD_SAVE_LAYER_INPUTS : SD_SAVE_ALL;
  const int B = bt ? bt->B : 2, T = bt ? bt->T : 24;
  return sd_qwen3_backward(&m.d, &m.p, &m.g, bt, addr(R_ACTS), sd_qwen3_acts_bytes(&m.d, B, T, save) + acts_slack,
                           addr(R_DLOGITS), addr(R_SCRATCH), sd_qwen3_bwd_scratch_bytes(&m.d, B, T) + scratch_slack, o, kMain);
}

void bwd_case(const Bwd& c) {
  Model m(3, 128, c.tied);
  if (c.flags & SD_BWD_EMBED_ONLY) { m.g.layers_host = nullptr; m.g.final_norm = nullptr; }  // Stage-1 may pass neither
  const sd_qwen3_batch bt = batch(c.head_rows, c.vl);
  sd_qwen3_bwd_opts o = {};
  o.flags = c.flags;
  o.grad_row_lo = c.row_lo;
  o.dx0_out = c.dx0 ? addr(R_DX0) : nullptr;
  o.on_grads_ready = c.cb ? on_grads : nullptr;
  o.cb_user = c.cb ? addr(R_USER) : nullptr;
  o.side_stream = c.side ? kSide : nullptr;
  begin(c.knob);
  g_sd_debug.model_overlap_mask = c.mask;
  finish(std::string("bwd_") + c.name, run_bwd(m, &bt, &o));
}

const int ACC = SD_BWD_ACCUMULATE, REC_ = SD_BWD_RECOMPUTE, EMB = SD_BWD_EMBED_ONLY;
//                      name             side  mask flags      lo  rows   vl     dx0    cb     knob     tied
const Bwd kBwd[] = {
    {"s_m31_slab1",         true,  31, 0,          0,   false, false, false, false, K_SLAB1, false},
    {"s_m23_unsup_acc",     true,  23, ACC,        0,   false, false, true,  true,  K_UNSUP, false},
    {"s_m31_unsup_rows",    true,  31, 0,          0,   true,  false, false, true,  K_UNSUP, false},
    {"s_m23_slab3_rec_vl",  true,  23, REC_,       0,   false, true,  false, false, K_SLAB3, false},
    {"s_m31_slab3_ddp",     true,  31, ACC,        0,   true,  false, true,  true,  K_SLAB3, false},
    {"s_m23_slab1_dx0",     true,  23, 0,          0,   false, false, true,  false, K_SLAB1, false},
    {"s_m15_slabmix_cb",    true,  15, 0,          0,   false, false, false, true,  K_SLABMIX, false},
    {"s_m27_vl_rows_tied",  true,  27, 0,          0,   true,  true,  false, true,  K_ZERO,  true},
    {"s_m0_acc_cb",         true,  0,  ACC,        0,   false, false, false, true,  K_ZERO,  false},
    {"s_m31_emb507_rows",   true,  31, EMB,        507, true,  false, false, false, K_ZERO,  false},
    {"s_m23_emb512_rec",    true,  23, EMB | REC_, 512, false, false, false, false, K_ZERO,  true},
    {"s_m0_emb515_acc_vl",  true,  0,  EMB | ACC,  515, false, true,  false, false, K_ZERO,  false},
    {"n_m31_slab3_cb",      false, 31, 0,          0,   false, false, false, true,  K_SLAB3, false},
};

// ---- forward: the four save modes, with and without SD_FWD_CONCURRENT (the folded mode needs hidden % 512 == 0)
void fwd_cases() {
  const char* names[] = {"none", "all_vl_fused_nologits", "inputs", "folded"};
  for (int save = 0; save < 4; ++save)
    for (int conc = 0; conc < 2; ++conc) {
      const Model m(2, save == SD_SAVE_NONE_FOLDED ? 512 : 128);
      // SD_SAVE_ALL also carries the forward's other branches.  Alone: packed documents, SwiGLU fused although gate|up is
      // kept, no logits.  Concurrent: fused entries refuse, head rows, shared tiles on the first layer only.
      const bool all = save == SD_SAVE_ALL;
      const sd_qwen3_batch bt = batch(all && conc, all && !conc);
      begin(all && conc ? K_UNSUP : K_ZERO);
      g_sd_debug.model_fuse_student_swiglu = all && !conc;
      if (all && conc) g_sd_debug.model_shared_layers_train = 1;
      const int rc = sd_qwen3_forward(&m.d, &m.p, &bt, addr(R_ACTS), sd_qwen3_acts_bytes(&m.d, bt.B, bt.T, save),
                                      all && !conc ? nullptr : addr(R_LOGITS), save | (conc ? SD_FWD_CONCURRENT : 0), kMain);
      finish(std::string("fwd_") + (all && conc ? "all_conc_rows_unsup" : conc ? std::string(names[save]) + "_conc" : names[save]), rc);
    }
}

// ---- block and decode entries over a contiguous cache and over a page pool
struct Gen {
  Model m{2};
  int B = 2, T = 24, cap = 300;
  const int64_t* ids = (const int64_t*)addr(R_IN, 0);
  const int32_t *kv_len = (const int32_t*)addr(R_IN, 1), *past = (const int32_t*)addr(R_IN, 6),
                *new_len = (const int32_t*)addr(R_IN, 7), *pos = (const int32_t*)addr(R_IN, 8);
  const void *cos_tab = addr(R_IN, 2), *sin_tab = addr(R_IN, 3);
  sd_kv_pages kv = {addr(R_CACHE), 0, (const int32_t*)addr(R_IN, 9), 5, 2};
  Gen() { kv.pool_bytes = sd_kvpool_bytes(&m.d, kv.n_pages); }
  int64_t cache_bytes() const { return sd_kvcache_bytes(&m.d, B, cap); }
  int prefill(int64_t slack = 0) {
    return sd_qwen3_prefill(&m.d, &m.p, ids, kv_len, cos_tab, sin_tab, addr(R_ACTS), sd_qwen3_prefill_acts_bytes(&m.d, B, T) + slack,
                            addr(R_CACHE), cache_bytes(), cap, addr(R_LOGITS), B, T, kMain);
  }
  int extend(int64_t slack = 0) {
    return sd_qwen3_extend(&m.d, &m.p, ids, past, new_len, cos_tab, sin_tab, addr(R_ACTS),
                           sd_qwen3_extend_acts_bytes(&m.d, B, T) + slack, addr(R_CACHE), cache_bytes(), cap, addr(R_LOGITS), B, T,
                           kMain);
  }
  int prefill_paged(int64_t slack = 0) {
    return sd_qwen3_prefill_paged(&m.d, &m.p, ids, kv_len, cos_tab, sin_tab, addr(R_ACTS),
                                  sd_qwen3_prefill_paged_acts_bytes(&m.d, B, T) + slack, &kv, addr(R_LOGITS), B, T, kMain);
  }
  int extend_paged(int64_t slack = 0) {
    return sd_qwen3_extend_paged(&m.d, &m.p, ids, past, new_len, cos_tab, sin_tab, addr(R_ACTS),
                                 sd_qwen3_extend_paged_acts_bytes(&m.d, B, T) + slack, &kv, addr(R_LOGITS), B, T, kMain);
  }
  int decode(int flags, int64_t slack = 0) {
    return sd_qwen3_decode_step_flags(&m.d, &m.p, ids, pos, 40, cos_tab, sin_tab, addr(R_CACHE), cache_bytes(), cap, addr(R_ACTS),
                                      sd_qwen3_decode_acts_bytes(&m.d, B, cap) + slack, addr(R_LOGITS), B, flags, kMain);
  }
  int decode_paged(int flags, int64_t slack = 0) {
    return sd_qwen3_decode_step_paged(&m.d, &m.p, ids, pos, 40, cos_tab, sin_tab, &kv, addr(R_ACTS),
                                      sd_qwen3_decode_step_paged_acts_bytes(&m.d, B, kv.max_pages) + slack, addr(R_LOGITS), B,
                                      flags, kMain);
  }
};

void gen_cases() {
  Gen g;
  begin(K_ZERO); finish("gen_prefill", g.prefill());
  begin(K_ZERO); finish("gen_extend", g.extend());
  begin(K_ZERO); finish("gen_prefill_paged", g.prefill_paged());
  begin(K_ZERO); finish("gen_extend_paged", g.extend_paged());
  begin(K_ZERO); finish("gen_decode", g.decode(0));
  begin(K_ZERO); finish("gen_decode_skinny", g.decode(SD_DECODE_SKINNY));
  begin(K_ZERO); finish("gen_decode_paged", g.decode_paged(0));
  begin(K_ZERO); finish("gen_decode_paged_skinny", g.decode_paged(SD_DECODE_SKINNY));
  begin(K_UNSUP); finish("gen_decode_skinny_unsup", g.decode(SD_DECODE_SKINNY));  // a GEMV refuses: the unflagged sequence
}

// ---- refusals: one line per refused call -- its code and how many trace lines it left behind (0: nothing was launched)
std::vector<std::string> g_refusals;
void refusal_begin() { begin(K_ZERO); }
void refused(const char* what, int rc) {
  g_on = false;
  g_refusals.push_back(std::string(what) + " -> " + std::to_string(rc) + " lines=" + std::to_string(g_trace.size()));
}

void refusal_cases() {
  const Model m(3);
  const sd_qwen3_batch ok = batch(false, false);
  const sd_qwen3_bwd_opts none = {};
  auto bwd = [&](const char* what, const Model& mm, const sd_qwen3_batch* bt, const sd_qwen3_bwd_opts* o, int64_t as = 0,
                 int64_t ss = 0) {
    refusal_begin();
    refused(what, run_bwd(mm, bt, o, as, ss));
  };
  { Model x(3); x.d.head_dim = 64; bwd("bwd head_dim 64", x, &ok, &none); }
  bwd("bwd batch NULL", m, nullptr, &none);
  { sd_qwen3_batch b = ok; b.B = 0; bwd("bwd B 0", m, &b, &none); }
  { sd_qwen3_batch b = ok; b.T = -1; bwd("bwd T -1", m, &b, &none); }
  { sd_qwen3_batch b = ok; b.vl = &kVl; bwd("bwd vl with kv_len", m, &b, &none); }
  { sd_qwen3_batch b = batch(false, true); b.B = 2; b.T = 24; bwd("bwd vl with B 2", m, &b, &none); }
  { sd_qwen3_batch b = batch(true, false); b.n_head_rows = 0; bwd("bwd n_head_rows 0", m, &b, &none); }
  { sd_qwen3_batch b = batch(true, false); b.n_head_rows = 49; bwd("bwd n_head_rows 49", m, &b, &none); }
  bwd("bwd opts NULL", m, &ok, nullptr);
  { sd_qwen3_bwd_opts o = {}; o.flags = 8; bwd("bwd flags 8", m, &ok, &o); }
  { sd_qwen3_bwd_opts o = {}; o.flags = EMB; o.grad_row_lo = -1; bwd("bwd embed_only row_lo -1", m, &ok, &o); }
  { sd_qwen3_bwd_opts o = {}; o.flags = EMB; o.grad_row_lo = 521; bwd("bwd embed_only row_lo 521", m, &ok, &o); }
  { sd_qwen3_bwd_opts o = {}; o.flags = EMB; o.dx0_out = addr(R_DX0); bwd("bwd embed_only dx0_out", m, &ok, &o); }
  { sd_qwen3_bwd_opts o = {}; o.flags = EMB; o.on_grads_ready = on_grads; bwd("bwd embed_only callback", m, &ok, &o); }
  { sd_qwen3_bwd_opts o = {}; o.flags = EMB | 8; o.grad_row_lo = 521; bwd("bwd embed_only row_lo 521 and flags 8", m, &ok, &o); }
  bwd("bwd acts one byte short", m, &ok, &none, -1);
  { sd_qwen3_bwd_opts o = {}; o.flags = REC_; bwd("bwd recompute acts one byte short", m, &ok, &o, -1); }
  bwd("bwd scratch one byte short", m, &ok, &none, 0, -1);
  bwd("bwd acts and scratch short", m, &ok, &none, -1, -1);

#define GEN(what, setup, call) do { Gen g; setup; refusal_begin(); refused(what, g.call); } while (0)
  GEN("prefill head_dim 64", g.m.d.head_dim = 64, prefill());
  GEN("prefill B 0", g.B = 0, prefill());
  GEN("prefill cap < T", g.cap = 23, prefill());
  GEN("prefill acts one byte short", (void)0, prefill(-1));
  GEN("extend head_dim 64", g.m.d.head_dim = 64, extend());
  GEN("extend T 0", g.T = 0, extend());
  GEN("extend past NULL", g.past = nullptr, extend());
  GEN("extend n_kv 0", g.m.d.n_kv = 0, extend());
  GEN("extend n_q 3 n_kv 2", g.m.d.n_q = 3, extend());
  GEN("extend n_q 6 n_kv 2", g.m.d.n_q = 6, extend());
  GEN("extend acts one byte short", (void)0, extend(-1));
  GEN("prefill_paged head_dim 64", g.m.d.head_dim = 64, prefill_paged());
  GEN("prefill_paged pool NULL", g.kv.pool = nullptr, prefill_paged());
  GEN("prefill_paged n_pages 0", g.kv.n_pages = 0, prefill_paged());
  GEN("prefill_paged max_pages too large", g.kv.max_pages = (1 << 22) + 1, prefill_paged());
  GEN("prefill_paged pool one byte short", g.kv.pool_bytes -= 1, prefill_paged());
  GEN("prefill_paged pool short and B 0", (g.kv.pool_bytes -= 1, g.B = 0), prefill_paged());
  GEN("prefill_paged capacity < T", g.T = 600, prefill_paged());
  GEN("prefill_paged ids NULL", g.ids = nullptr, prefill_paged());
  GEN("prefill_paged acts one byte short", (void)0, prefill_paged(-1));
  GEN("extend_paged table NULL", g.kv.table = nullptr, extend_paged());
  GEN("extend_paged new_len NULL", g.new_len = nullptr, extend_paged());
  GEN("extend_paged n_q 6 n_kv 2", g.m.d.n_q = 6, extend_paged());
  GEN("extend_paged n_q 3 n_kv 2", g.m.d.n_q = 3, extend_paged());
  GEN("extend_paged acts one byte short", (void)0, extend_paged(-1));
  GEN("decode flags 2", (void)0, decode(2));
  GEN("decode head_dim 64", g.m.d.head_dim = 64, decode(0));
  GEN("decode pos NULL", g.pos = nullptr, decode(0));
  GEN("decode acts one byte short", (void)0, decode(0, -1));
  GEN("decode_paged flags 2", (void)0, decode_paged(2));
  GEN("decode_paged ids NULL", g.ids = nullptr, decode_paged(0));
  GEN("decode_paged n_q 6 n_kv 2", g.m.d.n_q = 6, decode_paged(0));
  GEN("decode_paged n_pages 0", g.kv.n_pages = 0, decode_paged(0));
  GEN("decode_paged acts one byte short", (void)0, decode_paged(0, -1));
#undef GEN
  {  // no event set can be leased: refused before anything is enqueued (the pool is emptied of nothing: a failing hipGetDevice)
    sd_qwen3_bwd_opts o = {};
    o.side_stream = kSide;
    g_get_device_rc = 1;
    bwd("bwd side stream, no event set", m, &ok, &o);
    g_get_device_rc = 0;
  }
  const std::string path = std::string(g_outdir) + "/refusals.txt";
  FILE* f = fopen(path.c_str(), "w");
  if (!f) { ++g_failures; return; }
  for (const std::string& s : g_refusals) fprintf(f, "%s\n", s.c_str());
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: runner_trace OUTDIR\n"); return 2; }
  g_outdir = argv[1];
  {  // the first lease of an event set creates its events: traced once, on its own, so that no case depends on the order
    const Model m(3);
    const sd_qwen3_batch bt = batch(false, false);
    sd_qwen3_bwd_opts o = {};
    o.side_stream = kSide;
    begin(K_ZERO);
    const int rc = run_bwd(m, &bt, &o);
    while (g_trace.size() > 12) g_trace.pop_back();
    finish("first_lease", rc);
  }
  for (const Bwd& c : kBwd) bwd_case(c);
  fwd_cases();
  gen_cases();
  refusal_cases();
  return g_failures ? 1 : 0;
}
