// The cache step of a decode layer as ONE launch for gfx950: q/k-norm + RoPE, append of the new K / V row, split-KV
// attention of the one query row, and the merge of the partitions.
//
// What the reference runs for this: soulxpodcast/engine/llm_engine.py:37-76, the decode loop over a KV cache (vLLM / HF
// generate underneath; llm_engine.py:91 for the paged form) -- per layer HF's q_norm / k_norm + apply_rotary_pos_emb
// (HF:252-257), the cache update, and the attention of a single query row (HF:185-207).
//
// What it replaces here: sd_qknorm_rope_append{,_paged,_paged_mx} followed by sd_attn_decode{,_paged,_paged_mx} with len =
// pos and len_add = 1 (sd_decode.hip) -- three launches between which q and the partition records make two dependent
// round trips through memory.  The contract is bit equality with that pair: o, lse and every byte of the cache.  The
// kernel below therefore holds the three kernels' statements unchanged and in place (they stay as they are: moving their
// loops into shared functions changed their code, and with it which products become FMAs); the number formats, the page
// lookup and the constants are the shared ones of sd_kv_dev.cuh.
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

// The body below holds the statements of qknorm_rope_append_kernel, attn_decode_part_kernel and attn_decode_merge_kernel
// (sd_decode.hip) UNCHANGED and in their order, written out in place the way those kernels write them: which products the
// compiler contracts into FMAs depends on the shape of the code around them, and the contract is bit equality.
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
    float f[8], g[8], cs[8], sn[8];
    unpack8(raw, f);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += f[e] * f[e];
    ss = row16_sum(ss);
    const float rs = rsqrtf(ss * (1.f / 128.f) + eps);
    unpack8(*(const bf16x8*)(kw + j * 8), g);
    unpack8(*(const bf16x8*)(cosb + (long)t * 128 + j * 8), cs);
    unpack8(*(const bf16x8*)(sinb + (long)t * 128 + j * 8), sn);
    float ko[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float n = (float)(bf16)(g[e] * (float)(bf16)(f[e] * rs));  // normed value as HF holds it (bf16)
      const float pr = row16_xor8(n);
      const float rot = (j < 8) ? -pr : pr;
      ko[e] = n * cs[e] + rot * sn[e];
    }
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

  // ---- q of the G heads: qknorm_rope_append_kernel's statements, rounded to the bf16 it hands sd_attn_decode
  float qf[G][8], m[G], l[G], acc[G][8];
#pragma unroll
  for (int gq = 0; gq < G; ++gq) {
    const bf16x8 raw = *(const bf16x8*)(qkv + (long)b * nh * 128 + (hk * G + gq) * 128 + j * 8);
    float f[8], g[8], cs[8], sn[8];
    unpack8(raw, f);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += f[e] * f[e];
    ss = row16_sum(ss);
    const float rs = rsqrtf(ss * (1.f / 128.f) + eps);
    unpack8(*(const bf16x8*)(qw + j * 8), g);
    unpack8(*(const bf16x8*)(cosb + (long)t * 128 + j * 8), cs);
    unpack8(*(const bf16x8*)(sinb + (long)t * 128 + j * 8), sn);
    float qo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float n = (float)(bf16)(g[e] * (float)(bf16)(f[e] * rs));  // normed value as HF holds it (bf16)
      const float pr = row16_xor8(n);
      const float rot = (j < 8) ? -pr : pr;
      qo[e] = n * cs[e] + rot * sn[e];
    }
    unpack8(pack8(qo), qf[gq]);
    m[gq] = kNegBig;
    l[gq] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[gq][e] = 0.f;
  }

  // ---- attn_decode_part_kernel from here to its record stores
  long off = (long)b * cap * KD + hk * 128 + j * 8;
  const uint8_t *ksb = nullptr, *vsb = nullptr;
  if constexpr (sizeof...(PG) > 0) {
    const PageArgs pg{pga...};
    const int page = clampi(pg.table[(long)b * pg.max_pages + p], 0, pg.n_pages - 1);  // p < max_pages: p * 256 < n <= cap
    off = ((long)page - p) * kPart * KD + hk * 128 + j * 8;  // key = p * 256 + r below lands on row r of the page
    if constexpr (MX) {
      const long so = ((long)page - p) * kPart * Hkv * 4 + hk * 4;
      ksb = pg.k_scale + so;
      vsb = pg.v_scale + so;
    }
  }
  const bf16* kb = kp + off;
  const bf16* vb = vp + off;
  const uint8_t *kb8 = (const uint8_t*)kp + off, *vb8 = (const uint8_t*)vp + off;  // 8-bit pages: one byte per element
  for (int it = 0; it < 16; it += 4) {
    if (p * kPart + it * 16 >= n) break;  // block-uniform
    bf16x8 kv[4], vv[4];
    u32x2 kq[4], vq[4];
    uint32_t ksd[4], vsd[4];
    bool okk[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int key = p * kPart + (it + u) * 16 + sg;
      okk[u] = key < n;
      if constexpr (MX) {
        kq[u] = vq[u] = u32x2{0u, 0u};
        ksd[u] = vsd[u] = 0u;
        if (okk[u]) {
          kq[u] = *(const u32x2*)(kb8 + (long)key * KD);
          vq[u] = *(const u32x2*)(vb8 + (long)key * KD);
          ksd[u] = *(const uint32_t*)(ksb + (long)key * Hkv * 4);
          vsd[u] = *(const uint32_t*)(vsb + (long)key * Hkv * 4);
        }
      } else {
        kv[u] = zero8();
        vv[u] = zero8();
        if (okk[u]) {
          kv[u] = *(const bf16x8*)(kb + (long)key * KD);
          vv[u] = *(const bf16x8*)(vb + (long)key * KD);
        }
      }
    }
    float s[G][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float kf[8];
      if constexpr (MX) unpack8_mx(kq[u], (ksd[u] >> (8 * (j >> 2))) & 255u, kf);
      else unpack8(kv[u], kf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d += qf[g][e] * kf[e];
        d = row16_sum(d);
        s[g][u] = okk[u] ? d * scale_log2 : -INFINITY;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float mn = fmaxf(fmaxf(m[g], fmaxf(s[g][0], s[g][1])), fmaxf(s[g][2], s[g][3]));
      const float c = exp2f(m[g] - mn);
      l[g] *= c;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] *= c;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float pu = exp2f(s[g][u] - mn);  // masked key: exp2(-inf) = 0
        float vf[8];
        if constexpr (MX) unpack8_mx(vq[u], (vsd[u] >> (8 * (j >> 2))) & 255u, vf);
        else unpack8(vv[u], vf);
        l[g] += pu;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] += pu * vf[e];
      }
      m[g] = mn;
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (j == 0) { sh[sg][g][0] = m[g]; sh[sg][g][1] = l[g]; }
#pragma unroll
    for (int e = 0; e < 8; ++e) sh[sg][g][4 + j * 8 + e] = acc[g][e];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < G * 128; i += 256) {
    const int g = i >> 7, c = i & 127;
    float M = sh[0][g][0];
    for (int x = 1; x < 16; ++x) M = fmaxf(M, sh[x][g][0]);
    float L = 0.f, A = 0.f;
    for (int x = 0; x < 16; ++x) {  // group order: fixed
      const float w = exp2f(sh[x][g][0] - M);
      L += sh[x][g][1] * w;
      A += sh[x][g][4 + c] * w;
    }
    float* rec = ws + (((long)b * Hq + hk * G + g) * pstride + p) * kRec;
    rec[4 + c] = A;
    if (c == 0) { rec[0] = M; rec[1] = L; }
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

  // ---- attn_decode_merge_kernel's statements, for the G heads of the group (np == 1: over this workgroup's own record)
  for (int i = threadIdx.x; i < G * 128; i += 256) {
    const int h = hk * G + (i >> 7), c = i & 127;
    float M = kNegBig, L = 0.f, A = 0.f;
    const float* rec = ws + ((long)b * Hq + h) * pstride * kRec;
    for (int pp = 0; pp < np; ++pp, rec += kRec) {
      const float mp = rec[0], lp = rec[1], ap = rec[4 + c];
      const float mn = fmaxf(M, mp);
      const float c0 = exp2f(M - mn), c1 = exp2f(mp - mn);
      L = L * c0 + lp * c1;
      A = A * c0 + ap * c1;
      M = mn;
    }
    o[((long)b * Hq + h) * 128 + c] = (bf16)(np > 0 ? A / L : 0.f);
    if (lse && c == 0) lse[(long)b * Hq + h] = np > 0 ? (M + log2f(L)) * 0.6931471805599453f : -INFINITY;
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
