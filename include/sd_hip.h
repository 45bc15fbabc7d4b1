/* sd_hip.h -- C ABI of libsd_hip.so: the gfx950 (MI355X / CDNA4) kernels and step runner of the
 * Stage-2 distillation hot path of indiejoseph/speech-distill.
 *
 * The reference is pure Python and binds nothing native for this path; what it CALLS there are
 * third-party CUDA kernels (flash_attn, cuBLAS, ATen).  Each entry point below cites the reference
 * (or third-party HF) code whose arithmetic it replaces.  "HF:" = transformers/models/qwen3/
 * modeling_qwen3.py, the decoder the reference instantiates at train.py:155-178.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; bf16 tensors are row-major,
 *     16-byte aligned, leading dimensions are in ELEMENTS and multiples of 8;
 *   - `stream` is a hipStream_t (torch's current stream); launchers never allocate device memory and never
 *     synchronise; scratch comes from the caller (see *_workspace_bytes).  Process state reachable from THIS header is
 *     limited to: (1) a pool of timing-disabled hipEvent_t sets, leased per sd_qwen3_backward / sd_attn_bwd2 call and per
 *     device (two concurrent backward calls never share an event); (2) the sd_prof_* accumulators (only between
 *     sd_prof_begin/end).  The library never reads the environment.  Measurement and test switches (forced kernel variants,
 *     A/B thresholds, the CU budget of a multi-GPU run) are a separate interface, include/sd_hip_debug.h;
 *   - return value: SD_OK (0), a negative SD_ERR_* code, or a positive hipError_t from the launch.
 */
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SD_OK 0
#define SD_ERR_SHAPE (-1)
#define SD_ERR_ALIGN (-2)
#define SD_ERR_UNSUPPORTED (-3)
#define SD_ERR_NO_TEACHER (-4) /* distillation_loss.py:120 ValueError("Either teacher_logits or top_k must be provided") */
#define SD_ERR_WORKSPACE (-5)

#define SD_DTYPE_BF16 0
#define SD_DTYPE_F32 1

int sd_abi_version(void);

/* ---- GEMM: every nn.Linear of the decoder and its backward (HF:81-83, 252-254, 279, 441).
 * C[M,N] = op(A) op(B) (+ R).  trans_a=0: A is [M][K]; 1: A is stored [K][M].  trans_b=0: B is [N][K]
 * (torch weight layout); 1: B is stored [K][N].  R (nullable, may alias C) is added in fp32.
 * Operands may be strided views (ld* >= the row length, ld* % 8 == 0, 16-byte aligned pointers).  C[m][n] depends only
 * on the K elements of op(A)'s row m and of op(B)'s column n (and R[m][n]): the bytes between the rows of a view are never
 * interpreted (a NaN or Inf there, or in another row, does not reach it), and nothing outside the M x N elements of C is
 * written. */
int sd_gemm_bf16(const void* A, const void* B, void* C, const void* R, int M, int N, int K, int64_t lda,
                 int64_t ldb, int64_t ldc, int64_t ldr, int trans_a, int trans_b, void* stream);

/* Split-K form for GEMMs with few output tiles and a very long K (lm_head dX: K = vocab): K slices
 * write fp32 slabs into `workspace`, summed in a fixed order by a second kernel (deterministic).
 * sd_gemm_splitk_plan returns the number of slices the library would use (1 = no split). */
int sd_gemm_splitk_plan(int M, int N, int K);
int64_t sd_gemm_splitk_workspace_bytes(int M, int N, int K);
int sd_gemm_bf16_splitk(const void* A, const void* B, void* C, const void* R, int M, int N, int K, int64_t lda,
                        int64_t ldb, int64_t ldc, int64_t ldr, int trans_a, int trans_b, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* same, but the slabs are left un-reduced for a consumer that sums them (sd_rmsnorm_bwd_slabs); *nsplit_out = number
 * of slabs written to workspace ([nsplit][M][N] fp32), or 1 when no split was planned and bf16 C was written. */
int sd_gemm_bf16_splitk_partial(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb,
                                int64_t ldc, int trans_a, int trans_b, void* workspace, int64_t workspace_bytes,
                                int* nsplit_out, void* stream);

/* o-projection dX (autograd of HF:279) with delta = rowsum(dO * O) per (token, head) -- the row constant of the
 * flash-attention backward (flash_attn, train.py:160,177) -- computed in its epilogue: d_ao [M,Hq*128] = dy [M,H] . Wo,
 * delta [B,Hq,T] fp32.  Pass the result to sd_attn_bwd2 with o = NULL ("delta is already filled").
 * SD_ERR_UNSUPPORTED: use sd_gemm_bf16 + sd_attn_bwd2 with o. */
int sd_gemm_odx_delta(const void* dy, const void* wo, void* d_ao, const void* o, int64_t ldo, float* delta, int M, int T,
                      int Hq, int H, void* stream);

/* Fused forward GEMMs (fall back to the separate launchers when they return SD_ERR_UNSUPPORTED):
 * sd_gemm_swiglu: act [M,I] = silu(x Wg^T) * (x Wu^T), wgu = [gate rows | up rows] [2I,K]; gu_out [M,2I] nullable (HF:81-83).
 * sd_gemm_qkv_rope: raw q|k|v [M,(Hq+2Hkv)*128] plus RMS-normalised + RoPE-rotated q|k [M,(Hq+Hkv)*128] (HF:252-257). */
int sd_gemm_swiglu(const void* x, const void* wgu, void* gu_out, void* act_out, int M, int I, int K, void* stream);
/* The four weight-gradient GEMMs of a decoder layer (autograd of HF:252-254, 279, 81-83) as ONE persistent launch:
 * C_p [M_p,N_p] = A_p^T . B_p, p < n <= 4, A_p = dY_p [K,M_p] (row stride lda), B_p = X_p [K,N_p], common K = tokens.
 * accumulate: 0 overwrite C_p, 1 C_p += (gradient accumulation).  Same results as n calls of
 * sd_gemm_bf16(trans_a=1, trans_b=1[, R = C]). */
typedef struct {
  const void* A;
  const void* B;
  void* C;
  int64_t lda, ldb, ldc;
  int32_t M, N;
} sd_gemm_problem;
int sd_gemm_grouped_tn(const sd_gemm_problem* probs, int n, int K, int accumulate, void* stream);
/* backward twin: d(gate|up) [M,2I] = SwiGLU'(gate_up) applied to d(act) = dy [M,H] . W_down [H,I], in the epilogue of
 * that GEMM (d(act) is never stored); equals sd_gemm_bf16 (NN) + sd_swiglu_bwd bit for bit. */
int sd_gemm_swiglu_bwd(const void* dy, const void* wdown, const void* gate_up, void* dgate_up, int M, int I, int H,
                       void* stream);
int sd_gemm_qkv_rope(const void* x, const void* wqkv, void* qkv_out, void* qk_out, const void* q_gain, const void* k_gain,
                     const void* cos_tab, const void* sin_tab, int M, int T, int Hq, int Hkv, int K, float eps,
                     void* stream);

/* ---- RMSNorm folded into the projection behind it (the FROZEN teacher, train.py:60-69 / 165-169: its weights never
 * change, so HF:59-64's  y = g * (x * rstd)  followed by  y W^T  (HF:252-254, 81-83) is  rstd * (x (W diag g)^T):
 * the gain is multiplied into the weight rows once at load and the row statistic is applied as a row scale in the
 * consuming GEMM's epilogue.  The statistic travels as per-128-column-tile partial sums of squares, fp32 [M, H/128]
 * (H % 512 == 0, H/128 <= 16), written by whoever produced the row and summed in a fixed order by the consumer:
 *   sd_embedding_fwd_ssq  the lookup of sd_embedding_fwd + the partials of its rows (input of layer 0);
 *   sd_gemm_bf16_ssq      C = A . B^T + R (the o / down projection with its residual, HF:304-323) + the partials of C;
 *   sd_gemm_qkv_rope_rs   sd_gemm_qkv_rope on the UN-normalised x with wqkv = Wqkv diag(input_layernorm gain);
 *   sd_gemm_swiglu_rs     sd_gemm_swiglu on the UN-normalised x with wgu = Wgu diag(post_attention_layernorm gain).
 * Arithmetic differs from the unfolded path only in rounding: the gain meets the weight instead of the activation, and
 * the normalised row is never rounded to bf16 (tolerance test: test_folded_teacher_forward_matches_unfolded). */
int sd_embedding_fwd_ssq(const int64_t* ids, const void* E, void* x, float* ssq_out, int M, int H, int V, void* stream);
int sd_gemm_bf16_ssq(const void* A, const void* B, void* C, const void* R, float* ssq_out, int M, int N, int K, int64_t lda,
                     int64_t ldb, int64_t ldc, int64_t ldr, void* stream);
int sd_gemm_qkv_rope_rs(const void* x, const void* wqkv, void* qkv_out, void* qk_out, const void* q_gain, const void* k_gain,
                        const void* cos_tab, const void* sin_tab, const float* ssq, int M, int T, int Hq, int Hkv, int K,
                        float eps, void* stream);
int sd_gemm_swiglu_rs(const void* x, const void* wgu, void* gu_out, void* act_out, const float* ssq, float eps, int M, int I,
                      int K, void* stream);

/* ---- RMSNorm (HF:59-64).  rstd (fp32 [M], nullable in fwd) is saved for backward. */
int sd_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int M, int H, float eps, void* stream);
int64_t sd_rmsnorm_bwd_workspace_bytes(int M, int H);
/* dx = d(norm)/dx . dy (+ dres, nullable: the residual-stream gradient); dw (+)= sum_rows dy * xhat */
int sd_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                   void* dw, int accumulate_dw, void* workspace, int M, int H, void* stream);

/* *_bwd2: same, with the (tiny) gain-gradient reduce launched on `reduce_stream` after `event` (a hipEvent_t the
 * caller owns); both nullable = everything on `stream`.  The caller joins the streams before reusing `workspace`. */
int sd_rmsnorm_bwd2(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                    void* dw, int accumulate_dw, void* workspace, int M, int H, void* reduce_stream, void* event,
                    void* stream);
/* dy given as nsplit fp32 slabs [nsplit][M][H] (un-reduced split-K output), summed in slab order inside the kernel */
int sd_rmsnorm_bwd_slabs(const float* dy_slabs, int nsplit, const void* x, const void* w, const float* rstd,
                         const void* dres, void* dx, void* dw, int accumulate_dw, void* workspace, int M, int H,
                         void* reduce_stream, void* event, void* stream);
int sd_qknorm_rope_bwd2(const void* dqk, const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                        const void* sin_tab, void* dqkv, void* dq_gain, void* dk_gain, int accumulate_dw, void* workspace,
                        int M, int T, int Hq, int Hkv, float eps, void* reduce_stream, void* event, void* stream);

/* Deferred gain-gradient reduce: with dw == NULL (sd_rmsnorm_bwd2 / _slabs) or dq_gain == NULL (sd_qknorm_rope_bwd2)
 * the per-workgroup partial sums stay in `workspace` -- [sd_rmsnorm_bwd_partial_rows(M,H)][H] fp32, or
 * [sd_qknorm_rope_bwd_partial_rows(M,Hq,Hkv)][256] fp32 with the q gain in columns 0..127 and the k gain in
 * 128..255 -- and up to 8 such column sums are finished by ONE sd_colsum_reduce_batch launch (a layer's four gain
 * gradients: HF:59-64 weight of input_layernorm / post_attention_layernorm, HF:237-238 q_norm / k_norm).
 * out[c] (bf16) = (accumulate ? out[c] : 0) + sum_r partials[r*stride + c], fixed summation order. */
typedef struct {
  const float* partials;
  void* out;
  int nb, H, stride, accumulate;
} sd_colsum_problem;
int sd_rmsnorm_bwd_partial_rows(int M, int H);
int sd_qknorm_rope_bwd_partial_rows(int M, int Hq, int Hkv);
int sd_colsum_reduce_batch(const sd_colsum_problem* problems_host, int n, void* stream);

/* ---- per-head q/k RMSNorm (head_dim 128) then rotate-half RoPE (HF:252-257, 121-170).
 * qkv [M,(Hq+2Hkv)*128] -> qk_out [M,(Hq+Hkv)*128]; cos/sin tables bf16 [T,128]; token m has position m % T. */
int sd_qknorm_rope_fwd(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                       const void* sin_tab, void* qk_out, int M, int T, int Hq, int Hkv, float eps, void* stream);
int64_t sd_qknorm_rope_bwd_workspace_bytes(int M, int Hq, int Hkv);
int sd_qknorm_rope_bwd(const void* dqk, const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                       const void* sin_tab, void* dqkv, void* dq_gain, void* dk_gain, int accumulate_dw, void* workspace,
                       int M, int T, int Hq, int Hkv, float eps, void* stream);

/* ---- SwiGLU (HF:81-83): gate_up [M,2I] (gate | up) -> act [M,I] = silu(gate)*up */
int sd_swiglu_fwd(const void* gate_up, void* act, int M, int I, void* stream);
int sd_swiglu_bwd(const void* dact, const void* gate_up, void* dgate_up, int M, int I, void* stream);

/* ---- Contracts of the row kernels on ids and on untouched columns (pinned by tests/test_gpu_row_kernels.py):
 *   sd_embedding_fwd, sd_embedding_fwd_ssq   an id outside [0, V) is CLAMPED: id < 0 reads row 0, id >= V reads row V - 1
 *                                            (no error is raised; E is never read outside its V rows);
 *   sd_embedding_bwd                         a token whose id is outside [0, V) is SKIPPED: it adds to no row of dE, and
 *                                            the rows of the other ids get exactly the sums they get without it;
 *   sd_embedding_bwd_range                   likewise for ids outside [row_lo, V): rows of dE below row_lo are never read
 *                                            or written (row_lo == V: dE is left as it was);
 *   sd_rows_scatter                          a row index outside [0, M) is SKIPPED: dst is the zero-filled scatter of
 *                                            the remaining rows (n == 0: dst is all zero);
 *   sd_qknorm_rope_bwd, sd_qknorm_rope_bwd2  write the q and k columns [0, (Hq+Hkv)*128) of every row of dqkv and leave
 *                                            the v columns [(Hq+Hkv)*128, (Hq+2Hkv)*128) UNTOUCHED (in the decoder runner
 *                                            the attention backward has already stored dV there). */

/* ---- embedding (HF:381) and its deterministic scatter-add backward (dE += scale * rows of dx) */
int sd_embedding_fwd(const int64_t* ids, const void* E, void* x, int M, int H, int V, void* stream);
int sd_embedding_bwd(const int64_t* ids, const void* dx, void* dE, int M, int H, int V, float scale, void* stream);
/* the same scatter-add restricted to ids >= row_lo (0 <= row_lo <= V): rows of dE below row_lo are never read or written,
 * the others get the sums of sd_embedding_bwd (same increasing-token order, no float atomics).  Stage-1 alignment
 * (stage1.py:29-73): the embedding gradient is masked to the new speech-token rows [V - num_new_tokens, V). */
int sd_embedding_bwd_range(const int64_t* ids, const void* dx, void* dE, int M, int H, int V, int row_lo, float scale,
                           void* stream);
/* dst [M,H] = 0, then dst[rows[i]] = src[i] (rows unique): un-compacts the gradient of the rows the head kept
 * (inverse of the row gather sd_embedding_fwd(rows, table=x) ; distillation_loss.py:45 `x[valid]` run backwards) */
int sd_rows_scatter(const void* src, const int64_t* rows, void* dst, int n, int M, int H, void* stream);

/* ---- causal GQA flash attention, head_dim 128 (flash_attn via train.py:160,177; maths HF:185-207).
 * q [B*T, ldq] head hq at column hq*128; k, v likewise per kv head; o [B*T, ldo]; lse fp32 [B,Hq,T].
 * kv_len (int32 [B], nullable): keys >= kv_len[b] are masked (right padding).  Pinned by tests/test_gpu_attn_edges.py:
 *   - kv_len[b] is clamped to [1, T] (0 or a negative value behaves as 1: key 0 stays visible; NULL is T);
 *   - masked key rows of k and v may hold any FINITE values: they change no output bit.  Not NaN / inf: masked
 *     probabilities are exact zeros that still go through the P.V product, and 0 * inf is NaN;
 *   - query rows >= kv_len[b] are computed like any other row (they attend to the keys < kv_len[b]): o, lse and dq are
 *     written for all B*T rows;
 *   - dk and dv rows >= kv_len[b] are written, as zeros;
 *   - every output element of the head columns of rows [0, B*T) is stored (outputs need no zero fill), nothing else is;
 *   - the backward reads o and d_o with ONE row stride, ldo. */
int sd_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* kv_len, int64_t ldq,
                int64_t ldk, int64_t ldv, int64_t ldo, int B, int T, int Hq, int Hkv, int head_dim, float scale,
                void* stream);
/* delta: fp32 [B,Hq,T] scratch (rowsum(dO*O)).  sd_attn_bwd2: the same call; dQ, dK and dV come from ONE launch on
 * `stream`, and `side_stream` (nullable) is not used (it carried the dQ kernel while that was a launch of its own). */
int sd_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                float* delta, void* dq, void* dk, void* dv, const int32_t* kv_len, int64_t ldq, int64_t ldk, int64_t ldv,
                int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, int B, int T, int Hq, int Hkv, int head_dim,
                float scale, void* stream);

int sd_attn_bwd2(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                 float* delta, void* dq, void* dk, void* dv, const int32_t* kv_len, int64_t ldq, int64_t ldk, int64_t ldv,
                 int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, int B, int T, int Hq, int Hkv, int head_dim,
                 float scale, void* side_stream, void* stream);

/* ---- packed sequences without padding (HF padding-free packing: position_ids restart per document, flash-attn varlen).
 * The M tokens of a call hold n_seqs documents end to end: document s is the flat tokens [cu_seqlens[s], cu_seqlens[s+1]),
 * and a token attends to the tokens of its own document from the document start up to itself, to nothing else.
 * cu_seqlens: int32 [n_seqs + 1] in device memory, non-decreasing, cu_seqlens[0] = 0, cu_seqlens[n_seqs] = M.  Empty
 * documents are allowed.  Starts and ends are clamped into [0, M]: a malformed array gives wrong numbers, never an access
 * outside rows [0, M).  max_seqlen: the largest document length (a host-side hint, only used for the profiler's work
 * estimate).  work: device scratch of sd_varlen_work_bytes(M) bytes (nullable while that is 0, as it is now: the
 * kernels locate their document by a search in cu_seqlens). */
typedef struct {
  const int32_t* cu_seqlens;
  int n_seqs;
  int max_seqlen;
  void* work;
} sd_varlen;
int64_t sd_varlen_work_bytes(int M);
/* sd_attn_fwd / sd_attn_bwd2 over packed documents: the descriptor and M in place of kv_len, B, T; q, k, v, o, dq, dk, dv
 * [M, ld]; lse and delta fp32 [Hq, M] (one row per head, token-major).  Per document the results are bit-identical to the
 * padded entries run on that document alone with B = 1, T = its length, and the classic (not software-pipelined) forward. */
int sd_attn_fwd_varlen(const void* q, const void* k, const void* v, void* o, float* lse, const sd_varlen* vl,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int M, int Hq, int Hkv, int head_dim,
                       float scale, void* stream);
int sd_attn_bwd_varlen(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                       float* delta, void* dq, void* dk, void* dv, const sd_varlen* vl, int64_t ldq, int64_t ldk,
                       int64_t ldv, int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, int M, int Hq, int Hkv,
                       int head_dim, float scale, void* side_stream, void* stream);

/* ---- teacher log-softmax + top-K (train.py:80-91; extract_teacher_logits.py:114-129).
 * logits [rows, row_stride], first V columns used -> top_v fp16 [rows,K], top_i int32 [rows,K] sorted
 * descending, ties to the lowest index; lse_out fp32 [rows] nullable. */
int sd_logsoftmax_topk(const void* logits, void* top_v, void* top_i, float* lse_out, int rows, int64_t row_stride,
                       int V, int K, int dtype, void* stream);
/* the teacher's TAIL mass at a temperature, from the same logits and the top-K indices of above (top_i int32 [rows,K]):
 *   tail_out[r] = sum_{j not in {top_i[r,k]}} exp(x_j / T) / sum_{j < V} exp(x_j / T)       fp32 [rows]
 * summed directly over the non-members (not 1 - the members' share: that loses a tail below ~1e-6), membership by index
 * (ties cross the K-th value).  An index outside [0, V) is ignored and never used as an address, a duplicate counts
 * once; columns V..row_stride are never read.  One sweep of the row; fixed reduction order.
 * rows, V or K <= 0, K > 1024, K > V, row_stride < V, a NULL pointer, temperature not in (0, inf) SD_ERR_SHAPE; V or
 * row_stride % 8 != 0 or logits off 16 bytes SD_ERR_ALIGN; V > 524 288 (the row's bitmap is 64 KB of LDS) or an unknown
 * dtype SD_ERR_UNSUPPORTED. */
int sd_topk_tail(const void* logits, const void* top_i, float* tail_out, int rows, int64_t row_stride, int V, int K,
                 float temperature, int dtype, void* stream);

/* ---- which rows the loss reads (distillation_loss.py:31-45: shift by one, labels != -100, optional speech mask).
 * labels int64 [B,T]; speech_mask int64 [B,T] nullable; mask_a / mask_b: attention masks int64 [B,T] (nullable) to
 * validate as valid-prefix (right-padded) masks in the same launch.  rows / row_labels: int64 [B*T] out, the first
 * meta[0] entries are the flat indices b*T+t in increasing order and the label each row predicts; meta[1] != 0 when a
 * mask has a 1 after a 0.  meta int32 [2] in device memory (the host reads it once: the row count sizes the lm_heads). */
int sd_loss_rows(const int64_t* labels, const int64_t* speech_mask, const int64_t* mask_a, const int64_t* mask_b,
                 int64_t* rows, int64_t* row_labels, int32_t* meta, int B, int T, void* stream);

/* ---- the same selection over packed documents (sd_varlen's layout: labels int64 [M], document s = the flat tokens
 * [cu_seqlens[s], cu_seqlens[s+1]), int32 [n_seqs + 1] in device memory).  Flat token m is a loss row iff m + 1 < M, m + 1
 * lies in the same document as m (the last token of a document predicts nothing, whatever the label of the next document's
 * first token), labels[m+1] != -100 and (with a mask) speech_mask[m+1] != 0.  rows / row_labels: int64 [M] out, as above.
 * meta int32 [4] in device memory, ONE 16-byte host read for everything a packed step needs on the host:
 *   meta[0] row count;
 *   meta[1] error bits: bit 0 when cu_seqlens[0] != 0, cu_seqlens[n_seqs] != M or the array decreases anywhere; bit 1 when
 *           position_ids is given and holds a negative value;
 *   meta[2] the longest document;  meta[3] the largest position (0 without position_ids; int64 [M], nullable).
 * Empty documents are allowed.  With a malformed cu_seqlens the kernel still reads and writes only inside [0, M) (the
 * contract of sd_varlen).  SD_ERR_SHAPE: a NULL required pointer, M <= 0, n_seqs <= 0 or M > 2^30. */
int sd_packed_rows(const int64_t* labels, const int64_t* speech_mask, const int32_t* cu_seqlens, int n_seqs,
                   const int64_t* position_ids, int64_t* rows, int64_t* row_labels, int32_t* meta, int M, void* stream);

/* ---- DistillationLoss.forward / backward (distillation_loss.py:14-128).
 * student_logits [B,T,V] (bf16 or fp32 per `dtype`); exactly one of teacher_logits [B,T,V] (dense) or
 * (top_k_v fp16, top_k_i int32) [B,T,K] (sparse); labels int64 [B,T]; speech_mask uint8 [B,T] nullable.
 * loss_out fp32[8] = {total, task, distill, teacher, N_valid, n_hits, 0, 0}; row_stats: scratch of
 * sd_kdloss_stats_bytes(B,T) kept from fwd to bwd.  grad_total: fp32[1] upstream gradient (nullable = 1).
 * grad_logits may alias student_logits. */
int64_t sd_kdloss_stats_bytes(int B, int T);
int sd_kdloss_fwd(const void* student_logits, const void* teacher_logits, const void* top_k_v, const void* top_k_i,
                  const int64_t* labels, const uint8_t* speech_mask, void* row_stats, float* loss_out, int B, int T, int V,
                  int K, float temperature, float alpha, int dtype, void* stream);
int sd_kdloss_bwd(const void* student_logits, const void* teacher_logits, const void* top_k_v, const void* top_k_i,
                  const int64_t* labels, const void* row_stats, const float* loss_out, const float* grad_total,
                  void* grad_logits, int B, int T, int V, int K, float temperature, float alpha, int dtype, void* stream);

/* Same loss on rows the caller already shifted and selected (distillation_loss.py:31-45 done by the caller):
 * student_logits [R,V], teacher_logits [R,V] or (top_k_v, top_k_i) [R,K], row_labels int64 [R] = the label each row
 * predicts (-100 still masks a row); row_stats of sd_kdloss_stats_bytes(R,1). */
int sd_kdloss_fwd_rows(const void* student_logits, const void* teacher_logits, const void* top_k_v, const void* top_k_i,
                       const int64_t* row_labels, void* row_stats, float* loss_out, int R, int V, int K,
                       float temperature, float alpha, int dtype, void* stream);
int sd_kdloss_bwd_rows(const void* student_logits, const void* teacher_logits, const void* top_k_v, const void* top_k_i,
                       const int64_t* row_labels, const void* row_stats, const float* loss_out, const float* grad_total,
                       void* grad_logits, int R, int V, int K, float temperature, float alpha, int dtype, void* stream);

/* ---- on-policy (generalised) distillation: reverse KL and the beta-skewed Jensen-Shannon divergence on selected rows.
 * With q = softmax(s/T), p = softmax(t/T) per row, the row's divergence D is
 *   SD_DIV_REVERSE_KL: KL(q || p);      SD_DIV_JSD: beta KL(p || m) + (1 - beta) KL(q || m),  m = (1 - beta) q + beta p
 * (TRL's generalized_jsd_loss for 0 < beta < 1; its beta = 0 / 1 are the forward KL of sd_kdloss_* / SD_DIV_REVERSE_KL).
 * student_logits, teacher_logits [R,V] (bf16 or fp32 per `dtype`, the teacher dense) whose rows the caller already
 * shifted and selected; row_labels int64 [R], -100 or a value outside [0, V) masks a row (stats zero, gradient exactly
 * zero).  loss_out fp32[8] = {total, task, distill, teacher, N, N, 0, 0}: distill = T^2 mean D, task = mean CE of the
 * student, total = alpha task + (1 - alpha) distill, teacher = mean CE of the teacher; all zero when no row is valid.
 * row_stats: scratch of sd_gjsd_stats_bytes(R) kept from fwd to bwd; a row's stats do not depend on the other rows.
 * grad_total fp32 [1] nullable (= 1); grad_logits may alias student_logits; beta is ignored by SD_DIV_REVERSE_KL.
 * fp32 arithmetic, fixed reduction order.  Before any launch: R or V <= 0 or a NULL student / labels / stats / loss_out /
 * grad_logits, temperature not in (0, inf), SD_DIV_JSD with beta outside (0, 1) (NaN included) SD_ERR_SHAPE; a NULL
 * teacher SD_ERR_NO_TEACHER; V % 8 != 0 or a logits / gradient pointer off 16 bytes SD_ERR_ALIGN; an unknown mode or
 * dtype SD_ERR_UNSUPPORTED. */
#define SD_DIV_REVERSE_KL 1
#define SD_DIV_JSD 2
int64_t sd_gjsd_stats_bytes(int R);
int sd_gjsd_fwd_rows(const void* student_logits, const void* teacher_logits, const int64_t* row_labels, void* row_stats,
                     float* loss_out, int R, int V, float temperature, float alpha, float beta, int mode, int dtype,
                     void* stream);
int sd_gjsd_bwd_rows(const void* student_logits, const void* teacher_logits, const int64_t* row_labels,
                     const void* row_stats, const float* loss_out, const float* grad_total, void* grad_logits, int R, int V,
                     float temperature, float alpha, float beta, int mode, int dtype, void* stream);

/* ---- the same skewed Jensen-Shannon divergence against a TOP-K teacher (the reference's sparse teacher,
 * distillation_loss.py:73-118: top_k_v fp16 [R,K] stored log-probs, top_k_i int32 [R,K] their indices).  Per row:
 *   p_k = softmax(v / T)_k over the K entries,  P_j = sum_{k: i_k = j} p_k (duplicated indices sum their mass),
 *   S = {j : P_j > 0},  q = softmax(s / T) over the vocabulary,  m = (1 - beta) q + beta P,
 *   D = beta sum_S P_j (log P_j - log m_j) + (1 - beta) sum_S q_j (log q_j - log m_j) + (1 - Q_S) g0,
 *   Q_S = sum_S q_j,  g0 = -(1 - beta) log(1 - beta)
 * i.e. SD_DIV_JSD against the dense distribution P; D reaches 0 only when the student puts all its mass on S.  An entry
 * whose index is outside [0, V) or whose value is not finite carries no mass and behaves as absent (never read or
 * written through); a row whose entries are all absent is a masked row, as is a row whose label is -100 or outside
 * [0, V): stats zero, gradient exactly zero, not counted in N.
 * loss_out fp32[8] = {total, task, distill, teacher, N, n_hits, 0, 0}; teacher / n_hits as sd_kdloss_*'s sparse form
 * (minus the mean of v_k over the entries with i_k = the label; 0 without a hit).  row_stats: scratch of
 * sd_gjsd_topk_stats_bytes(R) kept from fwd to bwd; a row's stats do not depend on the other rows.  grad_total fp32 [1]
 * nullable (= 1); grad_logits may alias student_logits.  fp32 arithmetic, fixed reduction order, no float atomics.
 * Before any launch: R or V <= 0, K <= 0 or K > 1024, a NULL student / labels / stats / loss_out / grad_logits,
 * temperature not in (0, inf), beta outside (0, 1) (NaN included) SD_ERR_SHAPE; a NULL top_k_v / top_k_i
 * SD_ERR_NO_TEACHER; V % 8 != 0 or a logits / gradient pointer off 16 bytes SD_ERR_ALIGN; an unknown dtype
 * SD_ERR_UNSUPPORTED.  (Reverse KL has no such form: KL(q || P) is infinite wherever P_j = 0 < q_j.) */
int64_t sd_gjsd_topk_stats_bytes(int R);
int sd_gjsd_topk_fwd_rows(const void* student_logits, const void* top_k_v, const void* top_k_i, const int64_t* row_labels,
                          void* row_stats, float* loss_out, int R, int V, int K, float temperature, float alpha, float beta,
                          int dtype, void* stream);
int sd_gjsd_topk_bwd_rows(const void* student_logits, const void* top_k_v, const void* top_k_i, const int64_t* row_labels,
                          const void* row_stats, const float* loss_out, const float* grad_total, void* grad_logits, int R,
                          int V, int K, float temperature, float alpha, float beta, int dtype, void* stream);

/* ---- a top-K teacher WITH A TAIL BUCKET: forward KL, reverse KL and the skewed JSD over K + 1 outcomes.  top_k_tail fp32
 * [R] is the teacher's mass outside its top-K at the loss temperature (sd_topk_tail).  Per row, with p, the kept
 * entries and the duplicate merge as sd_gjsd_topk_*:
 *   P_j = (1 - tau) sum_{k: i_k = j} p_k on S = {j : P_j > 0},  P_0 = tau;   q = softmax(s / T),  q_j on S,
 *   q_0 = sum_{j not in S} q_j                       (b ranges over S and bucket 0, 0 log 0 = 0)
 *   SD_DIV_FORWARD_KL  D = sum_b P_b (log P_b - log q_b)
 *   SD_DIV_REVERSE_KL  D = sum_b q_b (log q_b - log P_b)
 *   SD_DIV_JSD         D = beta sum_b P_b (log P_b - log m_b) + (1 - beta) sum_b q_b (log q_b - log m_b),  m = (1 - beta) q + beta P
 * Every D is finite, exact on the top-K part, and a lower bound of the divergence against the dense teacher (merging
 * outcomes cannot increase it).  log q_0 is formed in log space from the off-support elements' own maximum.
 * A row is masked (stats zero, gradient exactly zero, not in N) when its label is -100 or outside [0, V), when no entry
 * is kept, or when its tau is NaN, < 0 or >= 1; a tau in [0, 2^-100) counts as 2^-100.
 * loss_out, row_stats (sd_gjsd_tail_stats_bytes(R)), grad_total, aliasing, arithmetic and order: as sd_gjsd_topk_*.
 * Before any launch: what sd_gjsd_topk_* refuses, with beta checked for SD_DIV_JSD only; K >= V SD_ERR_SHAPE (an
 * off-support element always exists); a NULL top_k_tail SD_ERR_NO_TEACHER; an unknown mode, or V > 458 752 (the
 * forward keeps a V-bit bitmap in LDS), SD_ERR_UNSUPPORTED. */
#define SD_DIV_FORWARD_KL 0
int64_t sd_gjsd_tail_stats_bytes(int R);
int sd_gjsd_tail_fwd_rows(const void* student_logits, const void* top_k_v, const void* top_k_i, const float* top_k_tail,
                          const int64_t* row_labels, void* row_stats, float* loss_out, int R, int V, int K,
                          float temperature, float alpha, float beta, int mode, int dtype, void* stream);
int sd_gjsd_tail_bwd_rows(const void* student_logits, const void* top_k_v, const void* top_k_i, const float* top_k_tail,
                          const int64_t* row_labels, const void* row_stats, const float* loss_out,
                          const float* grad_total, void* grad_logits, int R, int V, int K, float temperature, float alpha,
                          float beta, int mode, int dtype, void* stream);

/* ---- causal-LM cross-entropy on selected rows: the Stage-1 loss (stage1.py: TRL SFTTrainer over HF
 * Qwen3ForCausalLM(labels=...), i.e. HF ForCausalLMLoss -- shift by one, ignore_index -100, reduction "sum" divided by
 * num_items_in_batch when the Trainer passes it, else the mean over valid rows).  Teacher-free counterpart of
 * sd_kdloss_*_rows: logits [R,V] (bf16 or fp32 per `dtype`) whose rows the caller already shifted and selected,
 * row_labels int64 [R] (-100 masks a row).  divisor: fp32 [1] in device memory (nullable = number of valid rows).
 * loss_out fp32 [4] = {loss, sum of row losses, N valid, divisor used}; a zero divisor gives loss 0 and gradient 0.
 * row_stats: scratch of sd_celoss_stats_bytes(R) kept from fwd to bwd.  grad_total fp32 [1] nullable (= 1);
 * grad_logits may alias logits.  fp32 accumulation, fixed reduction order. */
int64_t sd_celoss_stats_bytes(int R);
int sd_celoss_fwd_rows(const void* logits, const int64_t* row_labels, const float* divisor, void* row_stats,
                       float* loss_out, int R, int V, int dtype, void* stream);
int sd_celoss_bwd_rows(const void* logits, const int64_t* row_labels, const void* row_stats, const float* loss_out,
                       const float* grad_total, void* grad_logits, int R, int V, int dtype, void* stream);

/* ---- fused AdamW on bf16 params with bf16 state (HF Trainer default optimizer on the bf16 student,
 * train.py:174,331-354; quirk Q5) and the global grad-norm / clip (HF trainer max_grad_norm). */
/* out_accum[0] += sum x^2; `partials`: SD_SUMSQ_PARTIALS floats of caller-owned device scratch holding the per-workgroup
 * sums between the two launches (fixed-order reduction: the norm is bit-identical on every data-parallel rank; calls
 * that may overlap on different streams pass different scratch). */
#define SD_SUMSQ_PARTIALS 2048
int sd_sumsq_bf16(const void* x, int64_t n, float* out_accum, float* partials, void* stream);
int sd_adamw_bf16(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* grad_sumsq, float max_grad_norm,
                  void* stream);

/* ---- LoRA student (train.py:180-202: peft LoRA, r = 32, on q/k/v/o/gate/up/down_proj of every decoder layer;
 * parity unpinned -- peft is an unvendored dependency, oracle/lora.py restates its published layer).
 * The adapter is applied to the MERGED weight: W_eff = W_res + (s B) A once per optimizer step (sd_lora_merge), the
 * decoder backward writes the full weight gradient dW, and dA = (s B)^T dW, dB = dW (s A)^T (sd_lora_project).  All
 * targets go in ONE launch each, driven by a plan the host builds once.
 *   A [r_pad, in] and B [out, r_pad] are fp32 masters (rows / columns r..r_pad are zero and stay zero; r_pad = r
 *   rounded up to 32, 64 or 128); the kernels read their bf16 shadows, written by sd_adamw_f32_shadow:
 *   a_shadow = bf16(A), a_scaled = bf16(s A), b_scaled = bf16(s B).  d_a / d_b: bf16, same shapes as A / B.
 * Shapes: in_features % 128 == 0, out_features % 32 == 0, else SD_ERR_UNSUPPORTED; every pointer 16-byte aligned. */
typedef struct {
  const void* w_res;   /* [out, in] bf16: frozen (residual) base weight */
  void* w_out;         /* [out, in] bf16: merged weight the decoder reads */
  const void* w_grad;  /* [out, in] bf16: gradient w.r.t. the merged weight */
  const void* a_shadow;
  const void* a_scaled;
  const void* b_scaled;
  void* d_a;
  void* d_b;
  int32_t out_features, in_features;
} SdLoraTarget;
int64_t sd_lora_plan_bytes(int n_targets);
/* Fills `plan_host` (host memory, sd_lora_plan_bytes(n) bytes); the caller copies it to the device once.  Every target is
 * judged before the first byte is written: a refused build (a null member or n <= 0: SD_ERR_SHAPE; a member off 16 bytes:
 * SD_ERR_ALIGN) leaves `plan_host` as it was. */
int sd_lora_plan_build(const SdLoraTarget* targets, int n_targets, int r_pad, void* plan_host, int64_t plan_bytes);
int sd_lora_merge(const void* plan_dev, const void* plan_host, void* stream);
int sd_lora_project(const void* plan_dev, const void* plan_host, void* stream);
/* AdamW on fp32 parameters with fp32 moments and a bf16 gradient (same update rule and clip as sd_adamw_bf16), also
 * writing shadow = bf16(p) and shadow_scaled = bf16(scale * p).  n % 4 == 0. */
int sd_adamw_f32_shadow(float* param, const void* grad, float* exp_avg, float* exp_avg_sq, void* shadow,
                        void* shadow_scaled, float scale, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, const float* grad_sumsq, float max_grad_norm, void* stream);

/* ---- whole-decoder runner: Qwen3ForCausalLM forward (HF:381-441) / backward, one C call each.
 * Weight layout: q|k|v projections fused row-wise into wqkv [(Hq+2Hkv)*128, h]; gate|up into wgu [2I, h]. */
typedef struct {
  int32_t vocab, hidden, inter, layers, n_q, n_kv, head_dim, tied;
  float eps;
  int32_t pad_;
} sd_qwen3_dims;

typedef struct {
  void *wqkv, *wo, *wgu, *wdown, *q_gain, *k_gain, *ln1, *ln2;
} sd_qwen3_layer;

typedef struct {
  void* embed;      /* [V,h] */
  void* lm_head;    /* [V,h]; == embed when tied */
  void* final_norm; /* [h] */
  const sd_qwen3_layer* layers_host; /* HOST array of `layers` entries holding DEVICE pointers */
} sd_qwen3_params;

/* What a forward keeps in `acts` (the low bits of the `mode` argument below):
 *   SD_SAVE_NONE          inference (the frozen teacher): one layer's buffers + a ping-pong residual stream;
 *   SD_SAVE_ALL           every activation the backward reads, for all layers (default training mode);
 *   SD_SAVE_LAYER_INPUTS  layer-granular recompute = what `gradient_checkpointing_enable()` means in HF
 *                         (train.py:204-208, modeling_qwen3.py decoder-layer checkpointing): only the residual stream
 *                         entering each layer + two layer work sets; the backward (SD_BWD_RECOMPUTE) runs a layer's
 *                         forward again right before its backward.  Same kernels on the same inputs, so the
 *                         gradients are bit-identical to SD_SAVE_ALL.
 *   SD_SAVE_NONE_FOLDED   inference with every decoder layer's two RMSNorm gains folded into the weights the caller passes:
 *                         layers_host[l].wqkv = Wqkv diag(ln1), .wgu = Wgu diag(ln2) (bf16(W[n][k] * g[k]), done once at
 *                         load); ln1 / ln2 are not read and no RMSNorm kernel runs except the final one (its consumer is
 *                         the tied embedding table): 1 instead of 2 L + 1 norm launches per pass.  Only for dims with
 *                         sd_qwen3_fold_supported(d) != 0; logits agree with SD_SAVE_NONE to bf16 rounding. */
#define SD_SAVE_NONE 0
#define SD_SAVE_ALL 1
#define SD_SAVE_LAYER_INPUTS 2
#define SD_SAVE_NONE_FOLDED 3
/* OR-ed into `mode` of sd_qwen3_forward: the caller runs ANOTHER pass beside this one on a second stream (the frozen
 * teacher beside the student's forward, train.py:60-69 vs :54).  Launches are then sized for CU-time per FLOP instead of
 * for covering every CU on their own (larger tiles on fewer workgroups for the N = hidden projections); results agree with
 * the unflagged pass to bf16 rounding.  Without a second stream the flag costs time: leave it off for a pass that runs alone. */
#define SD_FWD_CONCURRENT 0x100
int sd_qwen3_fold_supported(const sd_qwen3_dims* d);
/* bytes of activation storage for `sd_qwen3_forward` in that mode (negative: SD_ERR_* for an unknown mode) */
int64_t sd_qwen3_acts_bytes(const sd_qwen3_dims* d, int B, int T, int save_for_backward);
int64_t sd_qwen3_bwd_scratch_bytes(const sd_qwen3_dims* d, int B, int T);

/* One call's tokens, the same descriptor for a forward and for the backward of that forward.
 *   padded: ids int64 [B,T]; kv_len int32 [B] nullable (right padding); cos/sin bf16 [T,128];
 *   packed: vl given (sd_varlen above), then kv_len = NULL, B = 1, T = M: ids int64 [M], attention per document, and
 *     cos/sin are PER-TOKEN tables bf16 [M,128] (row m holds the rotary angles of token m's position in its document),
 *     read unchanged by the rope consumers.  acts / scratch are sized for B = 1, T = M.  Only the attention calls differ.
 *   head_rows (int64 [n_head_rows], flat b*T+t indices, unique, device memory; NULL = every row): the lm_head runs on
 *     those rows only, logits and dlogits are then bf16 [n_head_rows, V].  The training step needs only the rows whose
 *     shifted label is not -100 (distillation_loss.py:37-45); HF computes all of them (train.py:54-55).
 * SD_ERR_SHAPE: a NULL batch, B or T <= 0, vl together with kv_len or with B != 1, n_head_rows outside [1, B*T]. */
typedef struct {
  const int64_t* ids;
  const int32_t* kv_len;
  const sd_varlen* vl;
  const void *cos_tab, *sin_tab;
  const int64_t* head_rows;
  int32_t n_head_rows, B, T, pad_;
} sd_qwen3_batch;
/* acts: caller buffer of sd_qwen3_acts_bytes(d, B, T, mode); logits bf16 [B*T, V] or [n_head_rows, V] out (nullable:
 * stop after the final norm); mode = SD_SAVE_* | SD_FWD_CONCURRENT, anything else is SD_ERR_SHAPE. */
int sd_qwen3_forward(const sd_qwen3_dims* d, const sd_qwen3_params* p, const sd_qwen3_batch* batch, void* acts,
                     int64_t acts_bytes, void* logits, int mode, void* stream);
/* Backward of a forward made with the same batch.  g: same structure as p but holding gradient buffers (bf16, same
 * shapes); dlogits bf16, shaped like the forward's logits; scratch of sd_qwen3_bwd_scratch_bytes(d, B, T).  Options
 * (all-zero = the plain full backward on one stream):
 * flags: SD_BWD_ACCUMULATE (add to the gradient buffers: gradient accumulation; otherwise overwrite), SD_BWD_RECOMPUTE
 *   (`acts` was written by a forward with SD_SAVE_LAYER_INPUTS), SD_BWD_EMBED_ONLY; any other bit is SD_ERR_SHAPE.
 * on_grads_ready (nullable) is called ON THE HOST, from inside this call, each time the kernels that
 *   finish one group of gradients have been enqueued on `stream`: stage = SD_STAGE_HEAD (lm_head dW
 *   + final norm, before any layer), layer index L-1..0 (that layer's 8 tensors), SD_STAGE_EMBED (the
 *   embedding scatter-add, last).  A data-parallel caller records an event there and starts that
 *   bucket's RCCL all-reduce on a second stream, overlapping it with the rest of backward.
 * side_stream (nullable hipStream_t): when given, the weight-gradient GEMMs of a layer (dW = dY^T X, which
 *   nothing else in the layer depends on) are launched there and overlap the dX chain on `stream`; ordering
 *   is by HIP events, `stream` has waited for all of them when the call returns (and before each callback).
 * dx0_out (nullable, bf16 [B*T,h]): when given, the gradient w.r.t. the embedding OUTPUT is written there and
 *   the local embedding scatter-add is skipped -- the data-parallel caller then reduces the dense (lm_head)
 *   part of the tied gradient early and exchanges only the B*T touched rows (ddp.py).
 * SD_BWD_EMBED_ONLY: the Stage-1 alignment backward (stage1.py:29-73 freeze_model_weights: every decoder weight frozen,
 *   the embedding / lm_head gradients masked to rows >= old_vocab = V - num_new_tokens).  grad_row_lo (read only with
 *   this flag; 0 <= grad_row_lo <= V, any value: the < 8 rows before the first multiple of 8 are handled apart from the
 *   aligned GEMM); dx0_out or on_grads_ready with it is SD_ERR_SHAPE.  Writes ONLY rows [grad_row_lo, V) of g->embed, and
 *   of g->lm_head when untied; never reads or writes the rows below grad_row_lo or any other gradient buffer
 *   (g->layers_host and g->final_norm may be NULL).  Launches the dX chain of the full backward (SD_BWD_RECOMPUTE
 *   honoured), no per-layer weight or gain gradient, the lm_head dW of the new rows beside the lm_head dX on side_stream,
 *   then sd_embedding_bwd_range. */
#define SD_STAGE_HEAD (-1)
#define SD_STAGE_EMBED (-2)
#define SD_BWD_ACCUMULATE 1
#define SD_BWD_RECOMPUTE 2
#define SD_BWD_EMBED_ONLY 4
typedef void (*sd_stage_cb)(int stage, void* user);
typedef struct {
  int32_t flags;
  int32_t grad_row_lo;
  void* dx0_out;
  sd_stage_cb on_grads_ready;
  void* cb_user;
  void* side_stream;
} sd_qwen3_bwd_opts;
int sd_qwen3_backward(const sd_qwen3_dims* d, const sd_qwen3_params* p, const sd_qwen3_params* g,
                      const sd_qwen3_batch* batch, void* acts, int64_t acts_bytes, void* dlogits, void* scratch,
                      int64_t scratch_bytes, const sd_qwen3_bwd_opts* opts, void* stream);
/* ABI 2 folded the _rows, _varlen, _embed_rows and _embed_varlen twins of these entries into the batch and the options. */

/* ---- MXFP8 frozen teacher (train.py:60-69, 155-169: the teacher is loaded once, frozen, and only ever run forward; the
 * reference offers it in 8 bit through bitsandbytes, train.py:155-162 -- this is the format gfx950 has hardware for, not
 * bitsandbytes').  OCP Microscaling FP8: e4m3fn elements, one E8M0 scale byte per 32 consecutive elements along K.
 * For a block of bf16 values x: amax = max |x|; e = floor(log2(amax)) - 8 clamped to [-127, 127] (amax == 0: e = -127);
 * scale byte = e + 127; q = RNE_e4m3fn(clamp(x * 2^-e, -448, 448)); value = float(q) * 2^e.  NaN / Inf inputs are outside
 * the contract.  Every quantisation takes bf16-rounded values, also inside a GEMM epilogue.
 *   sd_mxfp8_quant: x bf16 [M,K] (row stride ldx elements) -> q e4m3 [M,K] + scale E8M0 [M,K/32]; rstd (nullable) fp32 [M]
 *     = rsqrt(mean(x^2) + eps) of the same row (HF:59-64: the RMSNorm statistic, applied as the consuming GEMM's row scale).
 *     K % 128 == 0.
 *   sd_gemm_mxfp8 (HF:252-254, 279, 83): C bf16 [M,N] = bf16(rowscale[m] * (A . B^T) + R), A [M,K] and B [N,K] (torch
 *     weight layout) both MXFP8, fp32 accumulation on v_mfma_scale_f32_16x16x128_f8f6f4; rowscale fp32 [M] and R bf16
 *     [M,N] (may alias C) nullable.  K % 128 == 0, N % 32 == 0.
 *   sd_gemm_mxfp8_swiglu (HF:81-83): wgu = [gate rows | up rows] [2I,K]; g, u = bf16(rowscale * (A . W^T)),
 *     act = bf16(silu(g) * u) exactly as sd_swiglu_fwd computes it, written ONLY as MXFP8: act_q [M,I], act_scale [M,I/32]
 *     (equals sd_gemm_mxfp8 + sd_swiglu_fwd + sd_mxfp8_quant bit for bit; the bf16 act is never stored).  I % 128 == 0. */
int sd_mxfp8_quant(const void* x, int64_t ldx, void* q, void* scale, float* rstd, float eps, int M, int K, void* stream);
int sd_gemm_mxfp8(const void* a_q, const void* a_scale, const void* b_q, const void* b_scale, void* C, const void* R,
                  const float* rowscale, int M, int N, int K, int64_t ldc, int64_t ldr, void* stream);
int sd_gemm_mxfp8_swiglu(const void* a_q, const void* a_scale, const void* wgu_q, const void* wgu_scale,
                         const float* rowscale, void* act_q, void* act_scale, int M, int I, int K, void* stream);

/* The decoder runner at that precision: inference only.  Per layer the four projections carry the RMSNorm gain in front
 * of them folded in (bf16(W[n][k] * g[k]), as SD_SAVE_NONE_FOLDED does) and are then quantised by sd_mxfp8_quant; the
 * residual stream, attention, q/k-norm + RoPE, the final RMSNorm, embedding and lm_head stay bf16.
 * Launches per layer: quant(x)+rstd, q|k|v GEMM, sd_qknorm_rope_fwd, attention, quant(ao), o GEMM + residual,
 * quant(x_mid)+rstd, gate|up GEMM + SwiGLU -> MXFP8, down GEMM + residual.
 * sd_qwen3_mx_supported: head_dim 128, hidden and inter multiples of 128.  `flags`: 0 or SD_FWD_CONCURRENT.  The other
 * arguments are those of sd_qwen3_forward; acts of sd_qwen3_mx_acts_bytes(d, B, T). */
typedef struct {
  void *wqkv_q, *wqkv_scale, *wo_q, *wo_scale, *wgu_q, *wgu_scale, *wdown_q, *wdown_scale; /* e4m3 [N,K] + E8M0 [N,K/32] */
  void *q_gain, *k_gain;                                                                    /* bf16 [128] */
} sd_qwen3_layer_mx;
typedef struct {
  void* embed;      /* bf16 [V,h] */
  void* lm_head;    /* bf16 [V,h]; == embed when tied */
  void* final_norm; /* bf16 [h] */
  const sd_qwen3_layer_mx* layers_host; /* HOST array of `layers` entries holding DEVICE pointers */
} sd_qwen3_params_mx;
int sd_qwen3_mx_supported(const sd_qwen3_dims* d);
int64_t sd_qwen3_mx_acts_bytes(const sd_qwen3_dims* d, int B, int T);
int sd_qwen3_forward_mx(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const sd_qwen3_batch* batch, void* acts,
                        int64_t acts_bytes, void* logits, int flags, void* stream);

/* ---- KV-cache generation (the reference's inference engine: soulxpodcast/engine/llm_engine.py:37-76 decodes one token per
 * step over a KV cache with the sampling recipe of soulxpodcast/config.py:107-118 and the repetition-aware rule of
 * soulxpodcast/models/modules/sampler.py:136-189; the attention maths is HF:185-207 for a single query row).
 * Cache: ONE caller-owned bf16 buffer [L][2][B][cap][Hkv*128] of sd_kvcache_bytes(d, B, cap) bytes -- per layer a K plane
 * then a V plane, each [B][cap][Hkv*128] with rows in the [token][kv head * 128] layout sd_attn_fwd reads.  head_dim 128
 * only (SD_ERR_UNSUPPORTED otherwise).  The entries below take the two planes of one layer.  Device-side lengths and
 * positions are clamped before any address is formed: nothing is read or written outside [0, cap) of a cache row. */
int64_t sd_kvcache_bytes(const sd_qwen3_dims* d, int B, int cap);
/* prefill sink (HF:252-257 outputs kept as past_key_values): for t < kv_len[b] (clamped to [0, T]; NULL = T) copies the
 * normalised + rotated K of qk [B*T,(Hq+Hkv)*128] and the raw V of qkv [B*T,(Hq+2Hkv)*128] into slot t; writes nothing
 * else.  T <= cap. */
int sd_kvcache_store(const void* qk, const void* qkv, void* k_plane, void* v_plane, const int32_t* kv_len, int B, int T,
                     int cap, int Hq, int Hkv, void* stream);
/* rows[b] = b*T + clamp(kv_len[b], 1, T) - 1 (int64 [B]; kv_len NULL = T): the last valid row of every right-padded
 * sequence, i.e. the row whose logits predict the first new token (HF generate reads logits[:, -1] of a left-padded
 * batch, sampler.py:136). */
int sd_last_rows(const int32_t* kv_len, int64_t* rows, int B, int T, void* stream);
/* decode twin of sd_qknorm_rope_fwd (HF:252-257) for ONE new token per sequence: qkv [B,(Hq+2Hkv)*128] raw; cos/sin bf16
 * [cap,128]; pos int32 [B] (device) = tokens already cached = the new token's position.  q_out [B,Hq*128] gets the
 * normalised + rotated q, cache slot pos[b] the normalised + rotated K and the raw V; q and K are bit-identical to
 * sd_qknorm_rope_fwd at that position.  A row with pos[b] outside [0, cap) writes nothing to the cache (its q_out row is
 * rotated by the clamped position). */
int sd_qknorm_rope_append(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab, const void* sin_tab,
                          const int32_t* pos, void* q_out, void* k_plane, void* v_plane, int B, int cap, int Hq, int Hkv,
                          float eps, void* stream);
/* single-token attention over the cache (HF:185-207 with one query row; flash-decoding split-KV): q [B,Hq*128], o
 * [B,Hq*128] bf16, lse fp32 [B,Hq] nullable (natural log).  Sequence b attends to keys [0, n), n = len[b] + len_add
 * clamped to [0, min(cap, max_len)]; len int32 [B] in device memory.  n == 0: a zero row (lse -inf).
 * Two launches: every (partition of 256 keys, kv head, sequence) with a visible key writes fp32 partials (max, sum, 128
 * accumulators per query head of the group) to `workspace` (sd_attn_decode_workspace_bytes(B, Hq, cap)); the second merges
 * the partitions of a row in increasing index order.  max_len: a HOST upper bound of every n (longest prompt + steps
 * taken) that sizes the grid.  Partition size and merge order are fixed, so the output bits depend on n and the data
 * only -- not on cap, max_len or the number of partitions launched.  Cache slots >= n may hold any finite values: they
 * are never read.  Hq / Hkv in {1, 2, 4}. */
int64_t sd_attn_decode_workspace_bytes(int B, int Hq, int cap);
int sd_attn_decode(const void* q, const void* k_plane, const void* v_plane, void* o, float* lse, const int32_t* len,
                   int len_add, void* workspace, int64_t workspace_bytes, int B, int cap, int max_len, int Hq, int Hkv,
                   int head_dim, float scale, void* stream);
/* sd_kvcache_store at an offset (the sink of a block of T new tokens behind a live cache, soulxpodcast.py:378-380): row
 * (b, t) with t < new_len[b] goes to slot past[b] + t; writes nothing else.  past, new_len int32 [B] (device), clamped
 * before any address is formed: past to [0, cap], new_len to [0, min(T, cap - past)]. */
int sd_kvcache_store_at(const void* qk, const void* qkv, void* k_plane, void* v_plane, const int32_t* past,
                        const int32_t* new_len, int B, int T, int cap, int Hq, int Hkv, void* stream);
/* causal attention of a block of T new query rows per sequence, at positions past[b] + t, over the keys already in the
 * cache plus the block itself (HF:185-207 with past_key_values; what a turn of soulxpodcast.py:378-380, a chunk of a
 * chunked prefill or a speculative verify step runs).  q, o [B*T, ld] bf16, head hq at column hq*128; k_plane, v_plane
 * one layer's planes [B][cap][Hkv*128], which already hold the block's own K / V at slots past[b] .. past[b] +
 * new_len[b] - 1 (sd_kvcache_store_at runs first); lse fp32 [B,Hq,T], natural log, nullable; past, new_len int32 [B]
 * (device), clamped as in sd_kvcache_store_at.  Row (b,t) sees keys [0, min(past[b] + t + 1, past[b] + new_len[b])); rows
 * t >= new_len[b] are padding, computed over that capped key set and stored like any other (as sd_attn_fwd does for rows
 * >= kv_len); a row with no visible key is zeros with lse = -inf.  Every head column of all B*T rows of o is stored,
 * nothing else is written; slots >= past[b] + new_len[b] are never read and may hold anything finite.
 * The bits of o[b,t,h,:] and lse[b,h,t] depend on that row's query, its position past[b] + t and the visible K / V rows
 * only: not on how the sequence was split into past and block, nor on T, B, cap, the other rows or the grid (key tiles
 * are anchored at cache slot 0, every row's online softmax is private to it, a masked key has probability exactly 0 and
 * stays out of the row maximum; no atomics, no split over keys).  head_dim 128 and Hq / Hkv in {1, 2, 4}; anything else
 * that is sane is SD_ERR_UNSUPPORTED, a NULL pointer (lse apart), T <= 0 or cap <= 0 SD_ERR_SHAPE, both before any launch. */
int sd_attn_extend(const void* q, const void* k_plane, const void* v_plane, void* o, float* lse, const int32_t* past,
                   const int32_t* new_len, int64_t ldq, int64_t ldo, int B, int T, int cap, int Hq, int Hkv, int head_dim,
                   float scale, void* stream);
/* one sampling step for B rows (sampler.py:136-189; HF logits_process.py in generate's order):
 *   1 repetition penalty over the row's GENERATED tokens seq[b, prompt_len[b] .. len[b]) only, each distinct token once:
 *     score < 0 ? score * p : score / p;   2 EOS = -inf while fewer than min_new_tokens were generated;   3 / temperature;
 *   4 top-k (1..128; the indices come from sd_logsoftmax_topk over the processed fp32 row, the scores are gathered from
 *     that row);   5 top-p on the renormalised top-k distribution: walking up from the smallest probability a candidate
 *     is dropped while the cumulative mass is <= 1 - top_p, the largest always stays;   6 inverse-CDF draw over the
 *     survivors in descending order (ties: lowest index first) with the caller's uniform.
 *   do_sample = 0: arg-max of the processed scores, ties to the lowest index.
 *   use_ras (sampler.py:142-148): a candidate is drawn with u[b,0]; if it occurs at least ras_min_count - 1 times in the
 *     last win_size tokens of seq[b, 0 .. len[b]) (prompt included; ras_min_count = ceil(win_size * tau_r), so that
 *     count + 1 >= win_size * tau_r) the token is drawn with u[b,1] from softmax(RAW logits) over the whole vocabulary,
 *     else with u[b,1] from the processed distribution.  Without use_ras the draw uses u[b,1].
 *   top_k = 0 (only with top_p = 1 and no RAS): the whole processed row is the distribution.  Full-vocabulary draws walk
 *     the vocabulary in index order: fp32 sums in blocks of 1024 columns, a scan of the block sums, a scan in the block.
 * logits bf16 [B, row_stride] (V columns used, never written); uniforms fp32 [B,2] in [0,1); seq int64 [B,cap];
 * prompt_len, len int32 [B]; finished uint8 [B].  An unfinished row gets its token at seq[b, len[b]], len[b] += 1,
 * next_out[b] = token, pos_out[b] = its index, finished[b] = 1 on EOS (or when the row is full).  A finished row gets
 * next_out[b] = pad_token_id and nothing else changes.  eos_token_id < 0: none. */
typedef struct {
  int32_t do_sample, top_k, use_ras, win_size, ras_min_count, min_new_tokens, eos_token_id, pad_token_id;
  float temperature, top_p, repetition_penalty, pad_;
} sd_sample_params;
int64_t sd_sample_workspace_bytes(int B, int V);
int sd_sample_step(const void* logits, int64_t row_stride, const float* uniforms, int64_t* seq, const int32_t* prompt_len,
                   int32_t* len, uint8_t* finished, int64_t* next_out, int32_t* pos_out, void* workspace,
                   int64_t workspace_bytes, const sd_sample_params* sp, int B, int V, int cap, void* stream);
/* sd_sample_step with everything per row (llm_engine.py:97-109: one SamplingParams per request of a continuously batched
 * step).  Row b is sampled exactly as sd_sample_step samples it alone with params[b] and its own uniform pair: the same
 * kernels, instantiated over where the parameters come from, and bit-identical results.
 *   params   sd_sample_params [B] in DEVICE memory (4-byte aligned), eos_token_id and pad_token_id included.
 *   max_new  int32 [B], device: after a commit a row with len[b] - prompt_len[b] >= max_new[b] gets finished[b] = 1, on top
 *            of the EOS rule and the row-full rule.
 *   uniforms fp32 [B, u_stride, 2]: row b reads pair g = len[b] - prompt_len[b] (the tokens it has generated), clamped to
 *            [0, u_stride); the host indexes nothing per step and a row's stream depends on that row only.
 *   env      HOST, launch decisions only: max_top_k = the largest top_k of any sampling row (0..128, <= V), any_sample =
 *            some row has do_sample, any_ras = some row may take the RAS fallback, any_full = some row has top_k == 0.
 * Launches: the scores, ONE sd_logsoftmax_topk with K = max(max_top_k, 1) (candidates come sorted descending, ties to the
 * lowest index, so a row's own top_k is a prefix of them; a greedy row takes the first), the pick, then the full-vocabulary
 * pair over the processed rows when any_full and again over the raw logits when any_ras -- each flagged row is served by
 * its own source.  Without any_sample every row is treated as greedy.
 * Every field read from device memory is brought into its legal range before it is used or an address is formed: top_k
 * to [0, K] (0 without any_full: K), use_ras off without any_ras or with top_k == 0, win_size to [0, cap], eos >= V = none,
 * pad to [0, V), temperature / top_p / repetition_penalty not > 0 (NaN included) = 1, g as above, len and prompt_len as in
 * sd_sample_step.  Nothing is written outside seq[b, 0 .. cap), and next_out is always a token id in [0, V).
 * Host checks, all before the first launch, with sd_sample_step's codes: a NULL pointer (env included), B, V, cap,
 * row_stride, u_stride or env.max_top_k out of range SD_ERR_SHAPE; V or row_stride not a multiple of 8, a misaligned
 * logits / workspace / params pointer SD_ERR_ALIGN; a short or NULL workspace (sd_sample_workspace_bytes) SD_ERR_WORKSPACE. */
typedef struct {
  int32_t max_top_k, any_sample, any_ras, any_full;
} sd_sample_env;
int sd_sample_step_rows(const void* logits, int64_t row_stride, const float* uniforms, int u_stride, int64_t* seq,
                        const int32_t* prompt_len, int32_t* len, uint8_t* finished, int64_t* next_out, int32_t* pos_out,
                        void* workspace, int64_t workspace_bytes, const sd_sample_params* params, const int32_t* max_new,
                        const sd_sample_env* env, int B, int V, int cap, void* stream);
/* The runner over the cache (unfolded bf16 weights only).
 * sd_qwen3_prefill: the SD_SAVE_NONE forward of sd_qwen3_forward with sd_kvcache_store after each layer's q|k|v step
 *   and the lm_head on the last valid row of each sequence (sd_last_rows, on the device): logits bf16 [B,V], bit-identical
 *   to sd_qwen3_forward with those head_rows.  cos/sin [T,128]; acts of sd_qwen3_prefill_acts_bytes(d, B, T); T <= cap.
 * sd_qwen3_decode_step: ids int64 [B] (device: the sampler's next_out), pos int32 [B] (device: the sampler's pos_out, the
 *   tokens already cached per row), max_len = host upper bound of every pos[b] + 1; cos/sin [cap,128].  Per layer: RMSNorm,
 *   q|k|v GEMM, sd_qknorm_rope_append, sd_attn_decode (len = pos + 1), o GEMM + residual, RMSNorm, gate|up + SwiGLU
 *   (sd_gemm_swiglu, else GEMM + sd_swiglu_fwd), down GEMM + residual; then the final norm and the lm_head:
 *   logits bf16 [B,V].  acts of sd_qwen3_decode_acts_bytes(d, B, cap).
 * sd_qwen3_decode_step_flags: the same step with flags = 0.  SD_DECODE_SKINNY (B <= SD_GEMV_MAX_M): every projection is a
 *   weight-streaming GEMV and the norms and the SwiGLU ride in them -- per layer sd_gemv_bf16(norm_gain = ln1) for q|k|v,
 *   sd_qknorm_rope_append, sd_attn_decode, sd_gemv_bf16(r = x) for o, sd_gemv_swiglu(norm_gain = ln2), sd_gemv_bf16(r =
 *   x_mid) for down (7 launches instead of 9), then ONE launch for the final norm + lm_head.  In that mode row b of the
 *   logits depends on row b's token, position and cache only (not on B or the other rows).  When any GEMV of the step
 *   would refuse its shape (B > 16, hidden > 4096, ...) the WHOLE step runs the unflagged sequence, so a step's arithmetic
 *   is one of two kinds, never a mixture.  An unknown flag bit is SD_ERR_SHAPE before any launch.
 * sd_qwen3_extend (soulxpodcast.py:342,378-380: ONE DynamicCache handed to llm.generate for every turn, each turn feeding
 *   only the tokens the cache has not seen; llm_engine.py:91 enable_prefix_caching): the SD_SAVE_NONE forward over a block
 *   of T right-padded NEW tokens per row, ids int64 [B*T], behind past[b] cached positions.  Token (b,t) takes position
 *   past[b] + t (cos/sin [cap,128]; the rows are gathered on the device, positions clamped to cap - 1; q and K are
 *   bit-identical to sd_qknorm_rope_fwd at that position), sd_kvcache_store_at follows each layer's q|k|v step and
 *   sd_attn_extend stands where sd_attn_fwd does.  The lm_head runs on row b*T + clamp(new_len[b], 1, T) - 1: logits bf16
 *   [B,V].  past, new_len int32 [B] (device), clamped as in sd_attn_extend; acts of sd_qwen3_extend_acts_bytes(d, B, T);
 *   T <= cap.  Argument checks as sd_qwen3_prefill (SD_ERR_SHAPE, SD_ERR_WORKSPACE, SD_ERR_UNSUPPORTED; Hq / Hkv outside
 *   {1, 2, 4} is SD_ERR_UNSUPPORTED), all before the first launch.
 * The three step / extend entries return SD_ERR_SHAPE for a NULL d or p. */
#define SD_DECODE_SKINNY 1
int64_t sd_qwen3_prefill_acts_bytes(const sd_qwen3_dims* d, int B, int T);
int sd_qwen3_prefill(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* kv_len,
                     const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes, void* cache,
                     int64_t cache_bytes, int cap, void* logits, int B, int T, void* stream);
int64_t sd_qwen3_extend_acts_bytes(const sd_qwen3_dims* d, int B, int T);
int sd_qwen3_extend(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* past,
                    const int32_t* new_len, const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes,
                    void* cache, int64_t cache_bytes, int cap, void* logits, int B, int T, void* stream);
int64_t sd_qwen3_decode_acts_bytes(const sd_qwen3_dims* d, int B, int cap);
int sd_qwen3_decode_step(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos,
                         int max_len, const void* cos_tab, const void* sin_tab, void* cache, int64_t cache_bytes, int cap,
                         void* acts, int64_t acts_bytes, void* logits, int B, void* stream);
int sd_qwen3_decode_step_flags(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos,
                               int max_len, const void* cos_tab, const void* sin_tab, void* cache, int64_t cache_bytes,
                               int cap, void* acts, int64_t acts_bytes, void* logits, int B, int flags, void* stream);

/* ---- paged KV cache (the reference's engine runs vLLM with enable_prefix_caching=True, soulxpodcast/engine/
 * llm_engine.py:91: a block-paged cache whose blocks requests with a common prefix share).  Opt-in twins of the cache
 * entries above; the contiguous entries and their bits are unchanged.
 * Page: SD_KV_PAGE = 256 positions, fixed -- one sd_attn_decode partition and four 64-key sd_attn_extend tiles, so a
 *   partition or a tile never straddles a page and the paged kernels walk the same keys in the same order as their twins.
 * Pool: ONE caller-owned bf16 buffer [L][2][n_pages][256][Hkv*128] of sd_kvpool_bytes(d, n_pages) bytes -- per layer a K
 *   pool plane then a V pool plane, each [n_pages][256][Hkv*128], rows as in the contiguous planes (K normalised + rotated,
 *   V raw).  The kernel entries take the two pool planes of one layer.
 * Page table: int32 [B][max_pages] in device memory, one for all layers: entry i of row b is the physical page holding
 *   positions 256 i .. 256 i + 255 of that row; the row's logical capacity is cap = max_pages * 256.
 * Rules: entries of logical pages a row does not reach are never read ("slots >= n are never read"); an entry that IS read
 *   and lies outside [0, n_pages) is a caller error -- no access leaves the pool: a store through it is skipped, a load
 *   through it arrives from page 0 (decode) or as zeros (extend), and that row's result is unspecified.  Device-side
 *   lengths and positions are clamped into [0, cap] first, as in the twins.
 * Bit contract: for ANY assignment of physical pages, o / lse / q_out and the rows gathered back through the table are
 *   bit-identical to the twin run on a contiguous cache holding the same rows.
 * Each entry mirrors its twin with (k_pool, v_pool, table, max_pages, n_pages) where the twin takes (k_plane, v_plane,
 *   cap); argument checks return the twin's codes before any launch, and a NULL table, max_pages <= 0 or n_pages <= 0 is
 *   SD_ERR_SHAPE.  sd_attn_decode_paged: workspace of sd_attn_decode_workspace_bytes(B, Hq, max_pages * 256); the
 *   workgroup of partition p reads table[b][p] once, after the "no visible key" exit. */
#define SD_KV_PAGE 256
int64_t sd_kvpool_bytes(const sd_qwen3_dims* d, int n_pages);
int sd_kvcache_store_paged(const void* qk, const void* qkv, void* k_pool, void* v_pool, const int32_t* table, int max_pages,
                           int n_pages, const int32_t* kv_len, int B, int T, int Hq, int Hkv, void* stream);
int sd_kvcache_store_at_paged(const void* qk, const void* qkv, void* k_pool, void* v_pool, const int32_t* table,
                              int max_pages, int n_pages, const int32_t* past, const int32_t* new_len, int B, int T, int Hq,
                              int Hkv, void* stream);
int sd_qknorm_rope_append_paged(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                                const void* sin_tab, const int32_t* pos, void* q_out, void* k_pool, void* v_pool,
                                const int32_t* table, int max_pages, int n_pages, int B, int Hq, int Hkv, float eps,
                                void* stream);
int sd_attn_decode_paged(const void* q, const void* k_pool, const void* v_pool, const int32_t* table, int max_pages,
                         int n_pages, void* o, float* lse, const int32_t* len, int len_add, void* workspace,
                         int64_t workspace_bytes, int B, int max_len, int Hq, int Hkv, int head_dim, float scale,
                         void* stream);
int sd_attn_extend_paged(const void* q, const void* k_pool, const void* v_pool, const int32_t* table, int max_pages,
                         int n_pages, void* o, float* lse, const int32_t* past, const int32_t* new_len, int64_t ldq,
                         int64_t ldo, int B, int T, int Hq, int Hkv, int head_dim, float scale, void* stream);
/* The runner over a paged cache (llm_engine.py:91): the launches of sd_qwen3_prefill / sd_qwen3_extend /
 * sd_qwen3_decode_step_flags in the same order with only the five cache kernels swapped for their paged twins, so the
 * logits are bit-identical.  kv: the pool, its size in bytes, the table [B][max_pages] and the two counts; cap =
 * max_pages * 256 wherever the twin takes cap (cos/sin [cap,128], T <= cap, the *_acts_bytes).  A NULL kv, pool or table,
 * n_pages <= 0 or max_pages <= 0 is SD_ERR_SHAPE, pool_bytes < sd_kvpool_bytes(d, n_pages) SD_ERR_WORKSPACE, an unknown
 * flag bit SD_ERR_SHAPE; everything else as the twin; every check runs before the first launch. */
typedef struct {
  void* pool;
  int64_t pool_bytes;
  const int32_t* table;
  int32_t n_pages, max_pages;
} sd_kv_pages;
int64_t sd_qwen3_prefill_paged_acts_bytes(const sd_qwen3_dims* d, int B, int T);
int sd_qwen3_prefill_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* kv_len,
                           const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes, const sd_kv_pages* kv,
                           void* logits, int B, int T, void* stream);
int64_t sd_qwen3_extend_paged_acts_bytes(const sd_qwen3_dims* d, int B, int T);
int sd_qwen3_extend_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* past,
                          const int32_t* new_len, const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes,
                          const sd_kv_pages* kv, void* logits, int B, int T, void* stream);
int64_t sd_qwen3_decode_step_paged_acts_bytes(const sd_qwen3_dims* d, int B, int max_pages);
int sd_qwen3_decode_step_paged(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos,
                               int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_pages* kv, void* acts,
                               int64_t acts_bytes, void* logits, int B, int flags, void* stream);

/* ---- 8-bit (MXFP8) pages of the paged KV cache.  Opt-in; the contiguous cache, the bf16 paged cache, their entries and
 * their bits are unchanged.  Every decode step reads every byte of every live row's cache: these pages hold 132 bytes per
 * (position, kv head) where the bf16 pages hold 256.
 * Format: exactly that of the "MXFP8 frozen teacher" section above -- e4m3fn elements, one E8M0 scale byte per 32
 *   consecutive elements along the head dimension (4 scale bytes per position and kv head), e = floor(log2(amax)) - 8
 *   with the same clamp, RNE, saturation at +-448 -- taken from the bf16 value the bf16 twin would have stored.
 * Pool: ONE caller-owned byte buffer of sd_kvpool_mx_bytes(d, n_pages) = L * 2 * n_pages * 256 * Hkv * 132 bytes; per
 *   layer, in this order: a K data plane [n_pages][256][Hkv*128] u8, a K scale plane [n_pages][256][Hkv*4] u8, a V data
 *   plane and a V scale plane laid out like the K ones.  The kernel entries take the four planes of one layer where the
 *   bf16 twin takes (k_pool, v_pool); data planes 16-byte, scale planes 4-byte aligned.
 * SD_KV_PAGE, the page table and every rule of the paged section carry over: entries a row does not reach are never
 *   read; an out-of-range entry that is read skips the store, or clamps (decode) or zeroes (extend) the load; lengths and
 *   positions are clamped first.
 * The value of a cached element is bf16(float(q) * 2^e).  For scale bytes 3..246 that product is a bf16 number for every
 *   finite e4m3 code, so nothing is rounded on the way back; it fails only for bytes 0-2 and 247-254, i.e. for a block
 *   whose amax lies below about 2^-116 or above about 2^118.  Such blocks are outside the contract, as NaN / Inf are; an
 *   all-zero block (byte 0, all codes 0) is inside it.
 * Stores (sd_kvcache_store_paged_mx, sd_kvcache_store_at_paged_mx, sd_qknorm_rope_append_paged_mx): the twin's arithmetic,
 *   statement for statement, up to the bf16 head vector it would store; that vector is then quantised (a 16-lane group
 *   owns its 128 elements, the 4 lanes of a block share one maximum; 8 data bytes per lane, one scale byte per block).
 *   q_out of the append is the twin's bf16.  The three kernels write identical bytes for identical input rows.
 * Attention (sd_attn_decode_paged_mx, sd_attn_extend_paged_mx): the twins' kernels with only the K / V read replaced --
 *   8 bytes per lane and row plus the row's scales, turned back into the bf16 numbers in registers (decode) or on the way
 *   into the LDS tile (extend: no LDS-DMA; one tile of loads is kept in flight in registers).  Work split, key order,
 *   masks, online softmax, merge, workspace and the max_len rule are the twins'; keys >= n are never loaded.
 * Bit contracts (by construction; tests/test_gpu_paged_mx.py):
 *   - for ANY page layout, o and lse of the two attention entries equal those of sd_attn_decode_paged /
 *     sd_attn_extend_paged run on a bf16 pool holding the dequantised values;
 *   - the stored data and scale bytes equal the quantisation above (tests/mx_ref.py mx_quant) of what the bf16 twin stores.
 * Argument checks: the twins' codes, all before any launch; a NULL plane, a NULL table, max_pages <= 0 or n_pages <= 0 is
 *   SD_ERR_SHAPE. */
int64_t sd_kvpool_mx_bytes(const sd_qwen3_dims* d, int n_pages);
int sd_kvcache_store_paged_mx(const void* qk, const void* qkv, void* k_data, void* k_scale, void* v_data, void* v_scale,
                              const int32_t* table, int max_pages, int n_pages, const int32_t* kv_len, int B, int T, int Hq,
                              int Hkv, void* stream);
int sd_kvcache_store_at_paged_mx(const void* qk, const void* qkv, void* k_data, void* k_scale, void* v_data, void* v_scale,
                                 const int32_t* table, int max_pages, int n_pages, const int32_t* past,
                                 const int32_t* new_len, int B, int T, int Hq, int Hkv, void* stream);
int sd_qknorm_rope_append_paged_mx(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                                   const void* sin_tab, const int32_t* pos, void* q_out, void* k_data, void* k_scale,
                                   void* v_data, void* v_scale, const int32_t* table, int max_pages, int n_pages, int B,
                                   int Hq, int Hkv, float eps, void* stream);
int sd_attn_decode_paged_mx(const void* q, const void* k_data, const void* k_scale, const void* v_data, const void* v_scale,
                            const int32_t* table, int max_pages, int n_pages, void* o, float* lse, const int32_t* len,
                            int len_add, void* workspace, int64_t workspace_bytes, int B, int max_len, int Hq, int Hkv,
                            int head_dim, float scale, void* stream);
int sd_attn_extend_paged_mx(const void* q, const void* k_data, const void* k_scale, const void* v_data, const void* v_scale,
                            const int32_t* table, int max_pages, int n_pages, void* o, float* lse, const int32_t* past,
                            const int32_t* new_len, int64_t ldq, int64_t ldo, int B, int T, int Hq, int Hkv, int head_dim,
                            float scale, void* stream);
/* The runner over 8-bit pages: sd_qwen3_prefill_paged / sd_qwen3_extend_paged / sd_qwen3_decode_step_paged with the five
 * cache kernels swapped for the entries above -- the same launches in the same order through the same code.  kv is the
 * same descriptor; pool_bytes is held against sd_kvpool_mx_bytes(d, n_pages) (a shortfall is SD_ERR_WORKSPACE); acts of
 * the paged twins' *_acts_bytes; every other check and code as the paged twin.  The decode step honours SD_DECODE_SKINNY.
 * sd_qwen3_prefill_paged_mx still attends over the in-flight bf16 K / V of the prompt (sd_attn_fwd): only its sink
 * quantises, so a prompt's own logits are those of the bf16 prefill, and they differ from what sd_qwen3_extend_paged_mx
 * with past = 0 computes, which attends over the quantised rows; the bytes the two leave in layer 0 are the same. */
int sd_qwen3_prefill_paged_mx(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* kv_len,
                              const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes,
                              const sd_kv_pages* kv, void* logits, int B, int T, void* stream);
int sd_qwen3_extend_paged_mx(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* past,
                             const int32_t* new_len, const void* cos_tab, const void* sin_tab, void* acts,
                             int64_t acts_bytes, const sd_kv_pages* kv, void* logits, int B, int T, void* stream);
int sd_qwen3_decode_step_paged_mx(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos,
                                  int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_pages* kv, void* acts,
                                  int64_t acts_bytes, void* logits, int B, int flags, void* stream);

/* ---- weight-streaming GEMV for decode (M = batch <= 16): the projections of HF:239-262 (q/k/v, o), HF:81-83 (MLP) and the
 * lm_head for one token per sequence, with the RMSNorm of HF:59-64 and the SwiGLU of HF:81-83 fused in.  bf16 operands,
 * fp32 accumulation, nothing transposed: w is [N,K] with K contiguous.
 * sd_gemv_bf16: y[M,N] = xn[M,K] . w[N,K]^T (+ r[M,N]), one rounding: bf16(acc + float(r)).  xn = x, or
 *   RMSNorm(x; norm_gain, eps) when norm_gain != NULL -- bit-identical to sd_rmsnorm_fwd into a bf16 buffer followed by
 *   sd_gemv_bf16 without a norm.
 * sd_gemv_swiglu: act[M,I] = silu(xn Wg^T) * (xn Wu^T), wgu = [gate rows | up rows] [2I,K] -- bit-identical to
 *   sd_gemv_bf16 with N = 2I into a bf16 gate|up buffer followed by sd_swiglu_fwd.
 * The bits of y[m,n] depend on x[m,:], w[n,:], r[m,n], norm_gain, eps and K only: not on M, the other rows, N or the grid
 * (every element is reduced over K in one fixed order, no atomics).  Weights are read once, 16 bytes per lane,
 * non-temporal, with no LDS staging.  y may be r (an element's residual is read by the thread that stores it, before the
 * store); y must not overlap x or w: every workgroup reads all of x while others already store.
 * Supported: 1 <= M <= SD_GEMV_MAX_M, N >= 1, K % 8 == 0, K <= 8192 (<= 4096 with a norm, the limit of sd_rmsnorm_fwd),
 * ld* >= the row length, x / w / norm_gain rows 16-byte aligned; anything else that is sane is SD_ERR_UNSUPPORTED, M <= 0
 * or a NULL x / w / y is SD_ERR_SHAPE.  Both are decided before any launch. */
#define SD_GEMV_MAX_M 16
int sd_gemv_bf16(const void* x, const void* w, void* y, const void* r, const void* norm_gain, float eps, int M, int N, int K,
                 int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, void* stream);
int sd_gemv_swiglu(const void* x, const void* wgu, void* act, const void* norm_gain, float eps, int M, int I, int K,
                   void* stream);

/* ---- the same GEMV over MXFP8 weights (the decode step of a model whose projections are quantised, sd_qwen3_params_mx).
 * sd_gemv_mxfp8: y[m,n] = bf16(rs[m] * sum_k X^[m,k] * W^[n,k] + r[m,n]).  x bf16 [M,K] (row stride ldx); w_q e4m3fn [N,K]
 *   and w_scale E8M0 [N,K/32], exactly what sd_mxfp8_quant produces for a weight; X^ is the dequantised sd_mxfp8_quant of
 *   row m, quantised inside the kernel (the same bytes and scale bytes); rs[m] = that call's rstd, rsqrtf(ss / K + eps),
 *   when norm != 0, else 1; r (nullable, row stride ldr) may alias y under the rule of sd_gemv_bf16.
 * sd_gemv_mxfp8_swiglu: wgu = [gate rows | up rows] [2I,K]; g, u = bf16(rs * sum), act bf16 [M,I] = bf16(silu(g) * u) as
 *   sd_swiglu_fwd computes it -- sd_gemv_mxfp8 with N = 2I followed by sd_swiglu_fwd, bit for bit; sd_mxfp8_quant of act
 *   gives the bytes sd_gemm_mxfp8_swiglu emits whenever g and u agree.
 * Every product X^ * W^ is exact in fp32.  The bits of y[m,n] depend on x[m,:], w[n,:] with its scales, r[m,n], eps and K
 * only: not on M, N, the other rows, the grid or the CU count (one fixed summation order per element, no atomics).  The
 * weights run as the A operand of v_mfma_scale_f32_16x16x128_f8f6f4 with their E8M0 bytes as its scale operand, read once,
 * 16 bytes per lane, non-temporal, with no LDS staging.
 * Supported: 1 <= M <= SD_GEMV_MAX_M, N >= 1, K % 128 == 0, K <= 8192, ldx >= K, ldy >= N, ldr >= N, x rows and w_q 16-byte
 * aligned, w_scale 4-byte aligned; anything else that is sane is SD_ERR_UNSUPPORTED; M, N or K <= 0 or a NULL x / w_q /
 * w_scale / y is SD_ERR_SHAPE.  Both are decided before any launch. */
int sd_gemv_mxfp8(const void* x, int64_t ldx, const void* w_q, const void* w_scale, void* y, int64_t ldy, const void* r,
                  int64_t ldr, int norm, float eps, int M, int N, int K, void* stream);
int sd_gemv_mxfp8_swiglu(const void* x, const void* wgu_q, const void* wgu_scale, void* act, int norm, float eps, int M, int I,
                         int K, void* stream);

/* ---- generation on MXFP8 weights: sd_qwen3_prefill / _extend / _decode_step over sd_qwen3_params_mx.  One descriptor
 * names the cache of any kind, so there are three entries.  kind 0: the contiguous bf16 cache (cache, cache_bytes >=
 * sd_kvcache_bytes(d, B, cap), cap); kind 1: bf16 pages and kind 2: MXFP8 pages (pages, held against sd_kvpool_bytes /
 * sd_kvpool_mx_bytes).  Another kind is SD_ERR_SHAPE.
 * sd_qwen3_mx_prefill: the launches of sd_qwen3_forward_mx with the cache store behind each layer's q|k|v step and the
 *   lm_head on each row's last valid token: logits bf16 [B,V], bit-identical to sd_qwen3_forward_mx with those head rows.
 * sd_qwen3_mx_extend: the same forward on per-token cos / sin rows, the cache's store-at + extend attention standing where
 *   the attention does (as sd_qwen3_extend).
 * sd_qwen3_mx_decode_step: flags = 0 runs, per layer, sd_mxfp8_quant(x) + rstd, sd_gemm_mxfp8 (q|k|v), the cache's append
 *   + decode attention, sd_mxfp8_quant(ao), sd_gemm_mxfp8 + residual (o), sd_mxfp8_quant(x_mid) + rstd,
 *   sd_gemm_mxfp8_swiglu, sd_gemm_mxfp8 + residual (down); then sd_rmsnorm_fwd and the bf16 lm_head GEMM.
 *   SD_DECODE_SKINNY (B <= SD_GEMV_MAX_M): sd_gemv_mxfp8(norm) (q|k|v), the cache step, sd_gemv_mxfp8(r = x) (o),
 *   sd_gemv_mxfp8_swiglu(norm), sd_gemv_mxfp8(r = x_mid) (down); then sd_gemv_bf16(norm_gain = final_norm) for the lm_head.
 *   When any GEMV of the step would refuse its shape the whole step runs the tile sequence: never a mixture.
 * Embedding, q/k-norm + RoPE, attention, the final norm and the lm_head are the bf16 entries.  acts of the *_acts_bytes
 * queries (the step's takes cap = the cache's capacity: cap, or max_pages * 256).  Checks and codes as the bf16 twins
 * (SD_ERR_SHAPE, SD_ERR_WORKSPACE, SD_ERR_UNSUPPORTED for dims outside sd_qwen3_mx_supported or Hq / Hkv outside
 * {1, 2, 4}); an unknown flag bit is SD_ERR_SHAPE; all before the first launch. */
typedef struct {
  int kind;              /* 0: contiguous bf16, 1: bf16 pages, 2: MXFP8 pages */
  void* cache;           /* kind 0 */
  int64_t cache_bytes;   /* kind 0 */
  int cap;               /* kind 0: positions per row */
  const sd_kv_pages* pages; /* kinds 1, 2 */
} sd_kv_ref;
int64_t sd_qwen3_mx_prefill_acts_bytes(const sd_qwen3_dims* d, int B, int T);
int sd_qwen3_mx_prefill(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids, const int32_t* kv_len,
                        const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes, const sd_kv_ref* kv,
                        void* logits, int B, int T, void* stream);
int64_t sd_qwen3_mx_extend_acts_bytes(const sd_qwen3_dims* d, int B, int T);
int sd_qwen3_mx_extend(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids, const int32_t* past,
                       const int32_t* new_len, const void* cos_tab, const void* sin_tab, void* acts, int64_t acts_bytes,
                       const sd_kv_ref* kv, void* logits, int B, int T, void* stream);
int64_t sd_qwen3_mx_decode_step_acts_bytes(const sd_qwen3_dims* d, int B, int cap);
int sd_qwen3_mx_decode_step(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids, const int32_t* pos,
                            int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_ref* kv, void* acts,
                            int64_t acts_bytes, void* logits, int B, int flags, void* stream);

/* ---- wide weight-streaming GEMV for decode (M = batch <= 64): the semantics of sd_gemv_bf16 / sd_gemv_swiglu in the form of
 * sd_gemv_mxfp8 -- the weights run as the A operand of v_mfma_f32_16x16x32_bf16, the rows of x as up to four 16-column B
 * tiles against the same A fragment.
 * sd_gemv_wide_bf16: y[m,n] = bf16(sum_k xn[m,k] w[n,k] + r[m,n]); xn = x, or RMSNorm(x; norm_gain, eps) when norm_gain !=
 *   NULL -- bit-identical to sd_rmsnorm_fwd into a bf16 buffer followed by sd_gemv_wide_bf16 without a norm.
 * sd_gemv_wide_swiglu: act[M,I] = silu(xn Wg^T) * (xn Wu^T), wgu = [gate rows | up rows] [2I,K]; gate and up are rounded to
 *   bf16 -- bit-identical to sd_gemv_wide_bf16 with N = 2I into a bf16 gate|up buffer followed by sd_swiglu_fwd.
 * Row independence: the bits of y[m,n] depend on x[m,:], w[n,:], r[m,n], norm_gain, eps and K only -- not on M, the other
 *   rows, the slot of a 16-column B tile that row m occupies, N, the grid or the CU count.
 * Reduction order of one element, fixed by K alone (no atomics, no split of K across workgroups): inside a K-step of 32 the
 *   instruction's own order; a wave's K-steps ascending through the accumulator operand; the waves of a workgroup through
 *   LDS in wave order; one rounding, bf16(sum + float(r)).  The bits are NOT those of sd_gemv_bf16: the order differs.
 * Loads: the weights are read once per launch, 16 bytes per lane, non-temporal, with no LDS staging; rows >= M of x are
 *   never read (zero fragments are formed in registers); nothing outside y[0..M, 0..N) is written.  y may be r under the
 *   rule of sd_gemv_bf16; y must not overlap x or w.
 * Supported: 1 <= M <= SD_GEMV_WIDE_MAX_M, N >= 1 (any), K % 32 == 0, K <= 8192 (<= 4096 with a norm), ld* >= the row
 * length, x / w / norm_gain rows 16-byte aligned; anything else that is sane is SD_ERR_UNSUPPORTED, M <= 0 or a NULL x / w /
 * y is SD_ERR_SHAPE.  Both are decided before any launch, y untouched. */
#define SD_GEMV_WIDE_MAX_M 64
int sd_gemv_wide_bf16(const void* x, const void* w, void* y, const void* r, const void* norm_gain, float eps, int M, int N,
                      int K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, void* stream);
int sd_gemv_wide_swiglu(const void* x, const void* wgu, void* act, const void* norm_gain, float eps, int M, int I, int K,
                        void* stream);
/* sd_qwen3_decode_step_wide: the decode step of sd_qwen3_decode_step_flags (bf16 weights) on the wide GEMV, over a cache of
 * any kind (sd_kv_ref).  The embedding; per layer sd_gemv_wide_bf16(norm_gain = ln1) for q|k|v, the cache's append and
 * decode attention, sd_gemv_wide_bf16(r = x) for o, sd_gemv_wide_swiglu(norm_gain = ln2), sd_gemv_wide_bf16(r = x_mid) for
 * down; ONE launch for the final norm + lm_head: 7 L + 2 launches.  Row b of the logits then depends on row b's token,
 * position and cache only.  When any projection would refuse its shape (B > 64, hidden > 4096, ...) the WHOLE step runs
 * the unflagged tile sequence of sd_qwen3_decode_step: never a mixture.  acts of sd_qwen3_decode_step_wide_acts_bytes(d,
 * B, cap) with cap = the cache's capacity (cap, or max_pages * 256).  A NULL d / p / kv or a bad kind is SD_ERR_SHAPE, short
 * acts SD_ERR_WORKSPACE, head_dim != 128 or Hq / Hkv outside {1, 2, 4} SD_ERR_UNSUPPORTED; every other check as
 * sd_qwen3_mx_decode_step; all before the first launch. */
int64_t sd_qwen3_decode_step_wide_acts_bytes(const sd_qwen3_dims* d, int B, int cap);
int sd_qwen3_decode_step_wide(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos,
                              int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_ref* kv, void* acts,
                              int64_t acts_bytes, void* logits, int B, void* stream);

/* ---- wide weight-streaming GEMV over MXFP8 weights (M = batch <= 64): sd_gemv_mxfp8 / sd_gemv_mxfp8_swiglu, argument for
 * argument and statement for statement, with up to four 16-column B tiles of quantised rows against the same weight
 * fragment (the tiling of sd_gemv_wide_bf16).
 * Order contract: one element's summation order is sd_gemv_mxfp8's -- K-steps of 128 per wave from K alone (nk <= 8: 1,
 *   <= 16: 2, <= 32: 4, else 8), a wave's K-steps ascending through the accumulator from 0, the waves through LDS in wave
 *   order, one rounding bf16(sum * rs + float(r)).  So for any 16-row slice s of x, sd_gemv_mxfp8_wide(x)[s] ==
 *   sd_gemv_mxfp8(x[s]) bit for bit, both forms, any M, N, K; a row's bits do not know the batch around it or the slot
 *   of the tile it occupies.
 * Loads and stores: the weights are read 16 bytes per lane, non-temporal, with no LDS staging -- once per launch for K <=
 *   4096, once per group of two B tiles (M > 32: twice) above it; rows >= M of x are never read; weight rows past N
 *   re-read row N - 1; nothing outside y[0..M, 0..N) is written.  y may be r under the rule of sd_gemv_bf16.
 * Supported: 1 <= M <= SD_GEMV_MX_WIDE_MAX_M; every other limit and the SD_ERR_SHAPE / SD_ERR_UNSUPPORTED split are those
 * of sd_gemv_mxfp8.  Decided before any launch, y untouched. */
#define SD_GEMV_MX_WIDE_MAX_M 64
int sd_gemv_mxfp8_wide(const void* x, int64_t ldx, const void* w_q, const void* w_scale, void* y, int64_t ldy, const void* r,
                       int64_t ldr, int norm, float eps, int M, int N, int K, void* stream);
int sd_gemv_mxfp8_wide_swiglu(const void* x, const void* wgu_q, const void* wgu_scale, void* act, int norm, float eps, int M,
                              int I, int K, void* stream);
/* sd_qwen3_mx_decode_step_wide: the SD_DECODE_SKINNY sequence of sd_qwen3_mx_decode_step on the wide kernels, over a cache
 * of any kind.  The embedding; per layer sd_gemv_mxfp8_wide(norm) for q|k|v, the cache's append and decode attention,
 * sd_gemv_mxfp8_wide(r = x) for o, sd_gemv_mxfp8_wide_swiglu(norm), sd_gemv_mxfp8_wide(r = x_mid) for down; then
 * sd_gemv_wide_bf16(norm_gain = final_norm) for the lm_head at every B: 7 L + 2 launches.  Row b of the logits depends on
 * row b's token, position and cache only; the hidden state entering the head has the bits of the skinny step's at B <= 16
 * (the logits do not: another head kernel).  When any projection or the head would refuse its shape (B > 64, ...) the
 * WHOLE step runs the tile sequence of sd_qwen3_mx_decode_step(flags = 0): never a mixture.  acts of
 * sd_qwen3_mx_decode_step_wide_acts_bytes (= sd_qwen3_mx_decode_step_acts_bytes).  Checks and codes as
 * sd_qwen3_mx_decode_step; all before the first launch. */
int64_t sd_qwen3_mx_decode_step_wide_acts_bytes(const sd_qwen3_dims* d, int B, int cap);
int sd_qwen3_mx_decode_step_wide(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids, const int32_t* pos,
                                 int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_ref* kv, void* acts,
                                 int64_t acts_bytes, void* logits, int B, void* stream);

/* ---- the cache step of a decode layer as ONE launch (llm_engine.py:37-76, the decode loop over a KV cache, :91 for the
 * paged form; per layer HF:252-257 q/k-norm + RoPE, the cache update, HF:185-207 with one query row).
 * sd_cache_step does what sd_qknorm_rope_append{,_paged,_paged_mx} followed by sd_attn_decode{,_paged,_paged_mx} with len =
 * pos and len_add = 1 do, BIT FOR BIT: o [B,Hq*128] bf16, lse fp32 [B,Hq] (nullable) and every byte of the planes are what
 * that pair leaves, for every pos (values outside [0, cap) store nothing), every max_len (a bound below pos + 1 still
 * stores the row) and every page layout.  q is formed in registers and never written.
 * sd_kv_planes: ONE layer's planes of any kind.  kind 0: k, v = the contiguous planes [B][cap][Hkv*128] bf16; kind 1: the
 *   pool planes [n_pages][256][Hkv*128] bf16 and the table int32 [B][max_pages] (device); kind 2: the e4m3 data planes and
 *   the E8M0 scale planes of MXFP8 pages.  Fields another kind uses are ignored.
 * Grid (ceil(min(cap, max_len) / 256), Hkv, B): a workgroup owns a partition of 256 keys of one kv head of one sequence.
 *   The workgroup whose partition holds slot pos[b] appends the row and is the only one that reads it, after its own
 *   stores have landed.  The partitions that hold a visible key publish their records and draw a ticket; the workgroup
 *   that draws the last one merges them in increasing partition order (one partition: no ticket, no fence).  No workgroup
 *   ever waits for another.  One rule the pair does not need: a slot that one row appends in a step must not be a visible
 *   key of ANOTHER row in the same step (rows that share a page share only positions below both their pos).
 * workspace: sd_cache_step_workspace_bytes(B, Hq, Hkv, cap) bytes (cap, or max_pages * 256), the partition records; it may
 *   hold anything.  tickets: int32 [B][Hkv], which MUST be zero at the launch (the caller zeroes them on the stream, once
 *   for all the layers of a step, each layer taking its own [B][Hkv] slice) and are zero again when it ends.
 * Checks, all before the launch: head_dim != 128 or Hq / Hkv outside {1, 2, 4} SD_ERR_UNSUPPORTED; a NULL pointer (lse
 *   apart), an unknown kind, B / cap / max_len / a page count <= 0, Hq % Hkv != 0 SD_ERR_SHAPE; a short or NULL workspace
 *   SD_ERR_WORKSPACE; qkv / gains / cos / sin / planes not 16-byte aligned (8-bit data planes 8, scale planes 4), workspace
 *   or tickets not 4-byte aligned SD_ERR_ALIGN. */
typedef struct {
  int kind;               /* 0: contiguous bf16, 1: bf16 pages, 2: MXFP8 pages */
  void *k, *v;            /* the layer's K and V planes (kind 2: the data planes) */
  void *k_scale, *v_scale; /* kind 2: the scale planes */
  int cap;                /* kind 0: positions per row */
  const int32_t* table;   /* kinds 1, 2 */
  int max_pages, n_pages; /* kinds 1, 2 */
} sd_kv_planes;
int64_t sd_cache_step_workspace_bytes(int B, int Hq, int Hkv, int cap);
int sd_cache_step(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab, const void* sin_tab,
                  const int32_t* pos, const sd_kv_planes* kv, void* o, float* lse, void* workspace, int64_t workspace_bytes,
                  int32_t* tickets, int B, int max_len, int Hq, int Hkv, int head_dim, float eps, float scale,
                  void* stream);
/* The decode steps on the one-launch cache step, over a cache of any kind (sd_kv_ref).  The launches of
 * sd_qwen3_decode_step_flags (kernels = 0: the tile sequence, 1: SD_DECODE_SKINNY) or sd_qwen3_decode_step_wide (kernels =
 * 2), and of sd_qwen3_mx_decode_step (flags = 0 or SD_DECODE_SKINNY), with sd_cache_step standing where the append and the
 * decode attention do: two launches fewer per layer (5 L + 2 kernels on the GEMV sequences, 7 L + 2 on the bf16 tile
 * sequence, 9 L + 2 on the MXFP8 tile one), plus ONE memset of the step's tickets ahead of layer 0.  Logits and cache are
 * bit-identical to those entries.  A step whose GEMVs would refuse their shape runs the tile sequence, still on
 * sd_cache_step.  acts of the *_fused_acts_bytes queries (the twins' set + the tickets int32 [L][B][Hkv]).  Another
 * `kernels` / flag value is SD_ERR_SHAPE; every other check and code as sd_qwen3_decode_step_wide / sd_qwen3_mx_decode_step;
 * all before the first launch. */
int64_t sd_qwen3_decode_step_fused_acts_bytes(const sd_qwen3_dims* d, int B, int cap);
int sd_qwen3_decode_step_fused(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos,
                               int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_ref* kv, void* acts,
                               int64_t acts_bytes, void* logits, int B, int kernels, void* stream);
int64_t sd_qwen3_mx_decode_step_fused_acts_bytes(const sd_qwen3_dims* d, int B, int cap);
int sd_qwen3_mx_decode_step_fused(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids,
                                  const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                  const sd_kv_ref* kv, void* acts, int64_t acts_bytes, void* logits, int B, int flags,
                                  void* stream);

/* ---- decode attention for rows that SHARE pages (llm_engine.py:91: prefix caching; a forked session maps the history's
 * full pages into every row's table).  sd_attn_decode_paged{,_mx} runs one workgroup per (page, kv head, row) and so reads
 * a page once per row that maps it.  The shared entries take exactly the twins' arguments and leave o and lse BIT-IDENTICAL
 * to them, for any table, lengths, len_add, max_len and page layout, through the same workspace
 * (sd_attn_decode_workspace_bytes), the same records and the same merge launch; checks and codes are the twins', in the
 * twins' order, all before the first launch.
 * Rows are taken in GROUPS of R consecutive rows, R = sd_attn_shared_group_rows(Hq, Hkv); the last group may be short.  Grid
 *   (R * ceil(min(cap, max_len) / 256), Hkv, ceil(B / R)): one workgroup per (logical page p, row w of the group, kv head).
 *   The rows of the group that are live for p (p * 256 < n_b) are partitioned by table[b][p]; the workgroup of the FIRST row
 *   of a set walks the set's physical page once, loading and unpacking each key / value row once for all the rows mapped to
 *   it, and the workgroups of the set's other rows leave at once.  So every DISTINCT physical page of a group is walked
 *   once; a group that shares nothing does the twin's work in the twin's number of workgroups.  Sharing is found on the device from the table, per logical index p (one
 *   physical page at different logical indices of two rows is two walks); the host passes nothing.  The entry of a row that
 *   is not live for p is never read; an entry outside [0, n_pages) is clamped as in the twin (no access leaves the pool,
 *   that row alone is unspecified).
 * One rule the twin does not need: where rows of DIFFERENT lengths share a page, the shorter row meets the value rows up
 *   to the longest length as 0 * value, so those slots must hold finite numbers (8-bit pages: no NaN code, no scale byte
 *   255).  A fork shares only full pages, and a pool that was zero-filled or written satisfies it.
 * R = 4 for Hq == Hkv and 2 for Hq / Hkv in {2, 4}: 4 query heads per workgroup (8 for Hq / Hkv = 4).  Registers would
 *   admit 16 heads (R = 8, 8, 4: 256 VGPRs, no scratch), but a workgroup's time grows with its heads -- one wave per SIMD
 *   scoring 16 heads took twice the time of 4 -- so the measured rule is the small one.
 * sd_attn_shared_group_rows: R, or SD_ERR_SHAPE (Hq, Hkv <= 0, Hq % Hkv != 0) / SD_ERR_UNSUPPORTED (Hq / Hkv not 1, 2, 4). */
int sd_attn_shared_group_rows(int Hq, int Hkv);
int sd_attn_decode_shared_paged(const void* q, const void* k_pool, const void* v_pool, const int32_t* table, int max_pages,
                                int n_pages, void* o, float* lse, const int32_t* len, int len_add, void* workspace,
                                int64_t workspace_bytes, int B, int max_len, int Hq, int Hkv, int head_dim, float scale,
                                void* stream);
int sd_attn_decode_shared_paged_mx(const void* q, const void* k_data, const void* k_scale, const void* v_data,
                                   const void* v_scale, const int32_t* table, int max_pages, int n_pages, void* o, float* lse,
                                   const int32_t* len, int len_add, void* workspace, int64_t workspace_bytes, int B,
                                   int max_len, int Hq, int Hkv, int head_dim, float scale, void* stream);
/* The decode steps with the shared attention standing where sd_attn_decode_paged{,_mx} does, over a PAGED cache
 * (sd_kv_ref kind 1 or 2; kind 0 is SD_ERR_SHAPE).  kernels: 0 the tile sequence, 1 SD_DECODE_SKINNY, 2 wide (bf16 weights);
 * flags: 0 or SD_DECODE_SKINNY (MXFP8 weights).  The launches, the acts (the *_shared_acts_bytes queries: the twins' sizes)
 * and every other check and code are those of sd_qwen3_decode_step_paged{,_mx} / _wide / sd_qwen3_mx_decode_step; logits and
 * every byte of the pool are bit-identical to them.  All checks before the first launch. */
int64_t sd_qwen3_decode_step_shared_acts_bytes(const sd_qwen3_dims* d, int B, int cap);
int sd_qwen3_decode_step_shared(const sd_qwen3_dims* d, const sd_qwen3_params* p, const int64_t* ids, const int32_t* pos,
                                int max_len, const void* cos_tab, const void* sin_tab, const sd_kv_ref* kv, void* acts,
                                int64_t acts_bytes, void* logits, int B, int kernels, void* stream);
int64_t sd_qwen3_mx_decode_step_shared_acts_bytes(const sd_qwen3_dims* d, int B, int cap);
int sd_qwen3_mx_decode_step_shared(const sd_qwen3_dims* d, const sd_qwen3_params_mx* p, const int64_t* ids,
                                   const int32_t* pos, int max_len, const void* cos_tab, const void* sin_tab,
                                   const sd_kv_ref* kv, void* acts, int64_t acts_bytes, void* logits, int B, int flags,
                                   void* stream);

/* ---- stream placement.  HIP multiplexes streams onto a few hardware queues (4 by default); streams that share a
 * queue never overlap.  Measures, with a `spin_us`-long busy-wait kernel on stream_a and an empty one on stream_b,
 * whether work on b runs while a is busy: *overlap = 1/0.  Synchronises both streams (a calibration call, made once
 * when the host picks its side streams: teacher beside student (train.py:60-69 vs :54), dW beside dX, RCCL beside
 * backward). */
int sd_streams_overlap(void* stream_a, void* stream_b, float spin_us, int* overlap);

/* ---- optional live timing (bench.py): HIP events around every launch, on the launch stream.
 * kinds index the arrays of sd_prof_end; work = algorithmic FLOPs (GEMM, attention) or bytes (others). */
enum {
  SD_K_GEMM_NT = 0, SD_K_GEMM_NN, SD_K_GEMM_TN, SD_K_ATTN_FWD, SD_K_ATTN_BWD_DKV, SD_K_ATTN_BWD_DQ, SD_K_LOSS_FWD,
  SD_K_LOSS_BWD, SD_K_TOPK, SD_K_RMSNORM, SD_K_QKROPE, SD_K_SWIGLU, SD_K_EMBED, SD_K_OPTIM, SD_K_MISC, SD_K_GEMM_NT_STAG,
  SD_K_COUNT
};
int sd_prof_begin(void);
int sd_prof_end(double* ms, double* work, int64_t* count, int n_kinds);
/* The same measurement per KERNEL SYMBOL (as rocprofv3 --kernel-trace names it, without namespace and arguments), as
 * text lines "symbol<TAB>kind<TAB>ms<TAB>work<TAB>launches"; returns the bytes needed (cap = 0 sizes the buffer). */
int64_t sd_prof_symbols(char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
