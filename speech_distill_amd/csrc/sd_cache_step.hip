// The cache step of a decode layer as ONE launch for gfx950: q/k-norm + RoPE, append of the new K / V row, split-KV
// attention of the one query row, and the merge of the partitions.
//
// What the reference runs for this: soulxpodcast/engine/llm_engine.py:37-76, the decode loop over a KV cache (vLLM / HF
// generate underneath; llm_engine.py:91 for the paged form) -- per layer HF's q_norm / k_norm + apply_rotary_pos_emb
// (HF:252-257), the cache update, and the attention of a single query row (HF:185-207).
//
// What it replaces here: sd_qknorm_rope_append{,_paged,_paged_mx} followed by sd_attn_decode{,_paged,_paged_mx} with len =
// pos and len_add = 1 (sd_decode.hip) -- three launches between which q and the partition records make two dependent
// round trips through memory.  The contract is bit equality with that pair: o, lse and every byte of the cache.  It
// holds because the arithmetic is stated once, with contraction off, in the device functions of sd_kv_dev.cuh that the
// three kernels and this one call; the number formats, the page lookup and the constants are that file's too.
//
// One workgroup = (partition of 256 keys, kv head, sequence), as in attn_decode_part_kernel; written once over the cache
// kind with that file's trailing pack (empty: contiguous, three arguments: bf16 pages, five: MXFP8 pages).
//   q       every workgroup forms the q vectors of its G heads itself from the raw q|k|v row, in the 16-lane layout the
//           key loop uses (each of the 16 groups redundantly: 16 lanes x 16 bytes per head, from L2).  q never reaches memory:
//           the pair rounds it to bf16 on the way, so it is rounded to bf16 here.
//   append  for each (b, hk) the workgroup of the partition that slot pos[b] falls into stores K (normed, rotated) and the
//           raw V -- under the pair's condition, 0 <= pos < cap and (pages) a table entry inside the pool -- BEFORE it
//           looks whether it has a visible key.  It is also the only workgroup that reads slot pos[b] in this launch, and
//           it reads it back from memory: store -> s_waitcnt vmcnt(0) -> barrier -> loads (workgroup-scope visibility of
//           a CU's own stores), so an 8-bit page hands back exactly the bytes another launch would see.
//   merge   np = ceil(n / 256) partitions hold a visible key.  np == 0: workgroup 0 writes the zero row.  np == 1: the one
//           workgroup finishes its heads from its own record (vmcnt(0) + barrier: no fence, no ticket).  np > 1: every workgroup publishes its records (plain stores,
//           vmcnt(0), barrier, one agent-scope release fence by thread 0) and draws a ticket; the one that draws np - 1
//           acquires (agent scope) and merges the np records of each head in increasing partition order.  Nobody waits for
//           anybody: a workgroup either leaves or finds every record already published.
// All stores are ordinary vector stores from plain C++.
#include <math.h>
#include "sd_common.cuh"
#include "../../include/sd_hip.h"
#include "sd_kv_dev.cuh"
#include "sd_prof.h"

#define ST ((hipStream_t)stream)

namespace {

// The work of qknorm_rope_append_kernel, attn_decode_part_kernel and attn_decode_merge_kernel (sd_decode.hip) in their
// order; this kernel holds the control flow, the stores and the ordering, the arithmetic is sd_kv_dev.cuh's.
// ws: records [B][Hq][pstride][kRec] as attn_decode_part_kernel lays them out; ticket: int32 [B][Hkv], zero on entry,
// zero again on exit.  kp / vp are read and written by this launch: no __restrict__ on them.
template <int G, class... PG>
__global__ __launch_bounds__(256) void cache_step_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ qw,
                                                         const bf16* __restrict__ kw, const bf16* __restrict__ cosb,
                                                         const bf16* __restrict__ sinb, const int32_t* __restrict__ pos,
                                                         bf16* kp, bf16* vp, float* ws, bf16* __restrict__ o,
                                                         float* __restrict__ lse, int32_t* ticket, int cap, int max_len,
                                                         int Hq, int Hkv, int pstride, float eps, float scale_log2,
                                                         PG... pga) {
  // the ONE LDS object: the 16 group states, and afterwards (word 0) the "I am the reducer" flag
  __shared__ __attribute__((aligned(16))) float sh[16][G][kRec];
  constexpr bool MX = sizeof...(PG) == 5;
  const int p = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int pz = pos[b];
  const bool inb = pz >= 0 && pz < cap;
  const int t = clampi(pz, 0, cap - 1);
  const int n = clampi(pz + 1, 0, cap < max_len ? cap : max_len);
  const int np = (n + kPart - 1) / kPart;
  const int last_part = (int)gridDim.x - 1;
  const bool appender = p == ((t >> 8) < last_part ? (t >> 8) : last_part);
  const bool zero_row = np == 0 && p == 0;
  if (!appender && p >= np && !zero_row) return;  // block-uniform: nothing to store, no visible key

  const int lane = lane_id(), j = lane & 15;
  const int sg = (threadIdx.x >> 6) * 4 + (lane >> 4);
  const int nh = Hq + 2 * Hkv, KD = Hkv * 128;

  if (appender) {  // block-uniform: K (normed, rotated) and the raw V of head hk -> slot pos[b]
    const bf16x8 vraw = *(const bf16x8*)(qkv + (long)b * nh * 128 + (Hq + Hkv + hk) * 128 + j * 8);
    const bf16x8 raw = *(const bf16x8*)(qkv + (long)b * nh * 128 + (Hq + hk) * 128 + j * 8);
    float ko[8];
    kv_qknorm_rope8(raw, kw, cosb, sinb, t, j, eps, ko);
    bool st = inb && sg == 0;  // one 16-lane group stores the row
    if constexpr (MX) {
      const PageArgs pg{pga...};
      long prow = 0;
      if (st) st = page_slot(pg, b, t, 1, &prow);
      if (st) {
        mx_store8(pack8(ko), (uint8_t*)kp, pg.k_scale, prow, Hkv, hk * 16 + j);
        mx_store8(vraw, (uint8_t*)vp, pg.v_scale, prow, Hkv, hk * 16 + j);
      }
    } else {
      long slot = ((long)b * cap + t) * KD;
      if constexpr (sizeof...(PG) > 0) {
        if (st) st = page_slot(PageArgs{pga...}, b, t, KD, &slot);
      }
      if (st) {
        *(bf16x8*)(kp + slot + hk * 128 + j * 8) = pack8(ko);
        *(bf16x8*)(vp + slot + hk * 128 + j * 8) = vraw;
      }
    }
    // the key loop below reads slot pos[b] (this workgroup alone does): the row has to have landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  if (p >= np) {  // block-uniform
    if (zero_row)
      for (int i = threadIdx.x; i < G * 128; i += 256) {
        const int h = hk * G + (i >> 7), c = i & 127;
        o[((long)b * Hq + h) * 128 + c] = (bf16)0.f;
        if (lse && c == 0) lse[(long)b * Hq + h] = -INFINITY;
      }
    return;
  }

  // ---- q of the G heads, rounded to the bf16 that qknorm_rope_append_kernel hands sd_attn_decode
  float qf[G][8], m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float qo[8];
    kv_qknorm_rope8(*(const bf16x8*)(qkv + (long)b * nh * 128 + (hk * G + g) * 128 + j * 8), qw, cosb, sinb, t, j, eps, qo);
    unpack8(pack8(qo), qf[g]);
    m[g] = kNegBig;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  }

  // ---- the walk of attn_decode_part_kernel, to its record stores
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
  // every wave: its record stores have left; then every thread is done with sh, and a record of this workgroup that
  // another of its threads wrote is visible to it (np == 1 reads its own record back below)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  if (np > 1) {  // block-uniform: publish, draw a ticket; the last arrival merges
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int drawn = __hip_atomic_fetch_add(ticket + (long)b * Hkv + hk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool reducer = drawn == np - 1;
      if (reducer) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      sh[0][0][0] = reducer ? 1.f : 0.f;
    }
    __syncthreads();
    if (sh[0][0][0] == 0.f) return;  // block-uniform: a later arrival merges
  }

  // ---- the partition merge of attn_decode_merge_kernel, for the G heads (np == 1: over this workgroup's own record)
  for (int i = threadIdx.x; i < G * 128; i += 256) {
    const int h = hk * G + (i >> 7), c = i & 127;
    kv_part_merge(ws + ((long)b * Hq + h) * pstride * kRec, np, c, o + ((long)b * Hq + h) * 128,
                  lse ? lse + (long)b * Hq + h : nullptr);
  }
  // every ticket of this (b, hk) has been drawn: back to zero for the next launch on these tickets
  if (np > 1 && threadIdx.x == 0)
    __hip_atomic_store(ticket + (long)b * Hkv + hk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" int64_t sd_cache_step_workspace_bytes(int B, int Hq, int Hkv, int cap) {
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || cap <= 0) return SD_ERR_SHAPE;
  return (int64_t)B * Hq * ((cap + kPart - 1) / kPart) * kRec * 4;
}

extern "C" int sd_cache_step(const void* qkv, const void* q_gain, const void* k_gain, const void* cos_tab,
                             const void* sin_tab, const int32_t* pos, const sd_kv_planes* kv, void* o, float* lse,
                             void* workspace, int64_t workspace_bytes, int32_t* tickets, int B, int max_len, int Hq, int Hkv,
                             int head_dim, float eps, float scale, void* stream) {
  if (head_dim != 128) return SD_ERR_UNSUPPORTED;
  if (!kv || kv->kind < 0 || kv->kind > 2) return SD_ERR_SHAPE;
  const bool paged = kv->kind != 0, mx = kv->kind == 2;
  if (paged && (!kv->table || kv->max_pages <= 0 || kv->n_pages <= 0 || kv->max_pages > (1 << 22))) return SD_ERR_SHAPE;
  const int cap = paged ? kv->max_pages * SD_KV_PAGE : kv->cap;
  if (B <= 0 || cap <= 0 || max_len <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv)) return SD_ERR_SHAPE;
  if (!qkv || !q_gain || !k_gain || !cos_tab || !sin_tab || !pos || !o || !tickets || !kv->k || !kv->v) return SD_ERR_SHAPE;
  if (mx && (!kv->k_scale || !kv->v_scale)) return SD_ERR_SHAPE;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (B > 65535 || Hkv > 65535) return SD_ERR_SHAPE;
  if (workspace_bytes < sd_cache_step_workspace_bytes(B, Hq, Hkv, cap) || !workspace) return SD_ERR_WORKSPACE;
  if (((uintptr_t)qkv & 15) || ((uintptr_t)q_gain & 15) || ((uintptr_t)k_gain & 15) || ((uintptr_t)cos_tab & 15) ||
      ((uintptr_t)sin_tab & 15) || ((uintptr_t)o & 1) || ((uintptr_t)workspace & 3) || ((uintptr_t)tickets & 3) ||
      ((uintptr_t)kv->k & (mx ? 7 : 15)) || ((uintptr_t)kv->v & (mx ? 7 : 15)) || (mx && ((uintptr_t)kv->k_scale & 3)) ||
      (mx && ((uintptr_t)kv->v_scale & 3)))
    return SD_ERR_ALIGN;
  if (max_len > cap) max_len = cap;
  const int pstride = (cap + kPart - 1) / kPart, np = (max_len + kPart - 1) / kPart;
  const float sl2 = scale * 1.4426950408889634f;
  // the raw q|k|v row, K and V rows of max_len keys per (sequence, kv head), the new row, o
  SdProfScope prof(SD_K_MISC, (mx ? 132.0 : 256.0) * 2.0 * B * Hkv * max_len + 512.0 * B * (Hq + Hkv), ST);
  static const char* const kKind[3] = {"", ", paged", ", paged, mx"};
  SD_PROF_LABEL("cache_step_kernel<%d%s>", G, kKind[kv->kind]);
#define SD_CS_ARGS                                                                                                      \
  dim3(np, Hkv, B), dim3(256), 0, ST, (const bf16*)qkv, (const bf16*)q_gain, (const bf16*)k_gain, (const bf16*)cos_tab, \
      (const bf16*)sin_tab, pos, (bf16*)kv->k, (bf16*)kv->v, (float*)workspace, (bf16*)o, lse, tickets, cap, max_len, Hq, \
      Hkv, pstride, eps, sl2
#define SD_CS_GO(G_)                                                                                                   \
  do {                                                                                                                 \
    if (mx)                                                                                                            \
      hipLaunchKernelGGL((cache_step_kernel<G_, const int32_t*, int, int, uint8_t*, uint8_t*>), SD_CS_ARGS, kv->table, \
                         kv->max_pages, kv->n_pages, (uint8_t*)kv->k_scale, (uint8_t*)kv->v_scale);                    \
    else if (paged)                                                                                                    \
      hipLaunchKernelGGL((cache_step_kernel<G_, const int32_t*, int, int>), SD_CS_ARGS, kv->table, kv->max_pages,      \
                         kv->n_pages);                                                                                 \
    else                                                                                                               \
      hipLaunchKernelGGL((cache_step_kernel<G_>), SD_CS_ARGS);                                                         \
  } while (0)
  if (G == 1) SD_CS_GO(1); else if (G == 2) SD_CS_GO(2); else SD_CS_GO(4);
#undef SD_CS_GO
#undef SD_CS_ARGS
  SD_CHECK_LAUNCH();
  return 0;
}
