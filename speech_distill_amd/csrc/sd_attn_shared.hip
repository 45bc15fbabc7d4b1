// Decode attention over a page pool for rows that SHARE pages (a forked session: n answers to one prompt, the history's
// full pages mapped into every row's table; llm_engine.py:91, vLLM's prefix caching under best-of-n).
//
// sd_attn_decode_paged{,_mx} (sd_decode.hip) runs one workgroup per (page, kv head, ROW): R forked rows read one physical
// page R times.  Here the grid holds one workgroup per (logical page p, row w of a GROUP of R consecutive rows, kv head).
// It reads the R table entries of its page index; if row w is the FIRST live row of the group on its physical page, the
// workgroup walks that page once for all the rows of the group mapped to it -- the key and value rows of a trip are loaded
// and unpacked once and every member row's query heads are scored against them -- and every other workgroup leaves at
// once.  So every DISTINCT physical page of a group is walked once, and distinct pages are walked side by side.
//
// The bits are the twin's.  Every query head keeps its own (m, l, acc) and sees, in the twin's order, the keys
// base + 16 i + group in trips of 4; a key at or past the row's own length scores -inf and gets probability exactly 0, a
// trip that starts at or past the row's length is not applied to the row at all (the twin's `break`), and the 16 key groups
// are merged in the twin's fixed order into the twin's record.  The one thing a row can see that the twin never loads is
// the VALUE row of a key between its own length and the longest length among the rows that share the page: it enters as
// 0 * value, which leaves the accumulator's value alone as long as the slot is finite (at most the sign of an accumulator
// that is zero can differ, and the group merge starts from +0 and erases it).  See include/sd_hip.h.
//
// Sharing is found on the device from the table alone, per logical index p: rows whose entries at p are equal share the
// walk.  A table entry of a row that is not live for p (p * 256 >= n_b) is never read.  Plain C++ loads and stores; no
// atomics; no workgroup waits for another.
#include <math.h>
#include <stdlib.h>
#include "sd_common.cuh"
#include "../../include/sd_hip.h"
#include "sd_kv_dev.cuh"
#include "sd_prof.h"
#include "sd_runner.h"  // sd_attn_decode_merge_launch

#define ST ((hipStream_t)stream)

namespace {

// R rows x G query heads per kv head = the heads one workgroup serves from one K/V read.  Their softmax states live in
// registers (18 floats per head and lane); the queries live in LDS (a lane re-reads its 8 floats per head and trip), which
// is what lets 16 heads fit the register file (R = 8, 8, 4 compile to 256 VGPRs without scratch; the entries instantiate
// R = 4, 2, 2, which measured twice as fast: shared_part_launch).  Every array below is indexed by unrolled loop counters only; who
// belongs to the walk is carried in block-uniform scalars (ne[r]: the row's length, 0 = not a member of this set).
template <int R, int G, class... PG>
__global__ __launch_bounds__(256) void attn_shared_part_kernel(const bf16* __restrict__ q, const bf16* __restrict__ kp,
                                                               const bf16* __restrict__ vp, float* __restrict__ ws,
                                                               const int32_t* __restrict__ len, int len_add, int cap,
                                                               int max_len, int B, int Hq, int Hkv, int pstride,
                                                               float scale_log2, PG... pga) {
  constexpr int H = R * G;
  constexpr bool MX = sizeof...(PG) == 5;
  __shared__ __attribute__((aligned(16))) float qs[H][128];
  constexpr int CH = 4 / G;  // rows whose group states go through LDS together (4 heads: the buffer of the twin at G = 4)
  __shared__ __attribute__((aligned(16))) float sh[16][CH * G][kRec];
  const PageArgs pg{pga...};
  // x = w * np + p: the workgroups of one w are neighbours.  (p fastest and w slowest on purpose: with w fastest the
  // workgroups that do the walking are every R-th one, and the round-robin over the eight XCDs puts them all on one.)
  const int np = gridDim.x / R;
  const int p = blockIdx.x % np, w = blockIdx.x / np, hk = blockIdx.y, b0 = blockIdx.z * R;
  const int lim = cap < max_len ? cap : max_len;
  // block-uniform: the rows of the group that are live for page p and their physical page
  int n[R], page[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    n[r] = 0;
    page[r] = 0;
    if (b0 + r < B) {
      const int nn = clampi(len[b0 + r] + len_add, 0, lim);
      if (p * kPart < nn) {  // p < max_pages: p * 256 < n <= cap; a row that is not live forms no table address
        n[r] = nn;
        page[r] = kv_page(pg, b0 + r, p);
      }
    }
  }
  // This workgroup's set: the live rows on row w's physical page -- if row w is the first of them.  ne[r]: the length of
  // member r, 0 for everybody else.  Every other workgroup of the group leaves here.
  int nw = 0, pw = 0;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r == w) { nw = n[r]; pw = page[r]; }
  if (nw == 0) return;  // block-uniform: row w has no visible key on this page (or lies past the batch)
  int ne[R], nmax = 0;
  bool first = true;
  unsigned members = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool same = n[r] > 0 && page[r] == pw;
    if (same && r < w) first = false;
    ne[r] = same && r >= w ? n[r] : 0;
    nmax = ne[r] > nmax ? ne[r] : nmax;
    members |= (ne[r] > 0 ? 1u : 0u) << r;
  }
  if (!first) return;  // block-uniform: an earlier row's workgroup walks this page for row w
  const int lane = lane_id(), j = lane & 15;
  const int sg = (threadIdx.x >> 6) * 4 + (lane >> 4);
  // the group's queries -> LDS as fp32 (exact), one 16-byte chunk per thread and pass
  for (int c = threadIdx.x; c < H * 16; c += 256) {
    const int h = c >> 4, r = h / G, g = h - r * G;
    if (b0 + r < B) {
      float f[8];
      unpack8(*(const bf16x8*)(q + (long)(b0 + r) * Hq * 128 + (hk * G + g) * 128 + (c & 15) * 8), f);
      *(f32x4*)&qs[h][(c & 15) * 8] = f32x4{f[0], f[1], f[2], f[3]};
      *(f32x4*)&qs[h][(c & 15) * 8 + 4] = f32x4{f[4], f[5], f[6], f[7]};
    }
  }
  float m[R][G], l[R][G], acc[R][G][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      m[r][g] = kNegBig;
      l[r][g] = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[r][g][e] = 0.f;
    }
  __syncthreads();
  // the one walk of the page
  {
    const KvPart pt = kv_part<MX>(pg, ((long)pw - p) * kPart, Hkv, hk, j);  // key = p * 256 + r lands on row r of the page
    for (int it = 0; it < 16; it += 4) {
      const int base = p * kPart + it * 16;
      if (base >= nmax) break;  // block-uniform
      // the trip's 4 key and value rows, loaded (up to the longest member's length) and unpacked ONCE for every member
      KvTrip<MX> tr;
      kv_load_trip(kp, vp, pt, Hkv, base + sg, nmax, tr);
      KvTripF tf;
      tf.unpack(tr, j);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (base >= ne[r]) continue;  // block-uniform: the twin's `break` (and every trip of a row outside the set)
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const f32x4 q0 = *(const f32x4*)&qs[r * G + g][j * 8], q1 = *(const f32x4*)&qs[r * G + g][j * 8 + 4];
          const float qf[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
          kv_head_trip<G>(qf, tf, j, base + sg, ne[r], scale_log2, m[r][g], l[r][g], acc[r][g]);  // masks by the row's OWN length
        }
      }
    }
  }
  // the twin's group merge, CH rows at a time through the one buffer; rows outside the set are not written
#pragma unroll
  for (int r0 = 0; r0 < R; r0 += CH) {
    if (((members >> r0) & ((1u << CH) - 1u)) == 0) continue;  // block-uniform
#pragma unroll
    for (int rr = 0; rr < CH; ++rr)
#pragma unroll
      for (int g = 0; g < G; ++g) kv_group_put(sh, sg, rr * G + g, j, m[r0 + rr][g], l[r0 + rr][g], acc[r0 + rr][g]);
    __syncthreads();
    for (int i = threadIdx.x; i < CH * G * 128; i += 256) {
      const int hh = i >> 7, c = i & 127, rr = hh / G, g = hh - rr * G;
      if (!((members >> (r0 + rr)) & 1u)) continue;
      kv_group_merge(sh, hh, c, ws + (((long)(b0 + r0 + rr) * Hq + hk * G + g) * pstride + p) * kRec);
    }
    __syncthreads();
  }
}

// the launch of the instantiation that serves G query heads per kv head; pga: the twin's trailing pack
template <class... PG>
void shared_part_launch(int G, const void* q, const void* kd, const void* vd, void* ws, const int32_t* len, int len_add,
                        int cap, int max_len, int B, int Hq, int Hkv, int pstride, int np, float sl2, void* stream,
                        PG... pga) {
#define SD_SHARED_GO(R_, G_)                                                                                             \
  hipLaunchKernelGGL((attn_shared_part_kernel<R_, G_, PG...>), dim3(np * R_, Hkv, (B + R_ - 1) / R_), dim3(256), 0, ST,        \
                     (const bf16*)q, (const bf16*)kd, (const bf16*)vd, (float*)ws, len, len_add, cap, max_len, B, Hq, Hkv, \
                     pstride, sl2, pga...)
  if (G == 1) SD_SHARED_GO(4, 1); else if (G == 2) SD_SHARED_GO(2, 2); else SD_SHARED_GO(2, 4);
#undef SD_SHARED_GO
}

}  // namespace

extern "C" int sd_attn_shared_group_rows(int Hq, int Hkv) {
  if (Hq <= 0 || Hkv <= 0 || (Hq % Hkv)) return SD_ERR_SHAPE;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  return G == 1 ? 4 : 2;  // 4 query heads per workgroup (8 for G = 4): what shared_part_launch instantiates
}

// The twin's checks in the twin's order (sd_attn_decode_paged), then the grouped phase 1 and the twin's phase 2.
extern "C" int sd_attn_decode_shared_paged(const void* q, const void* k_pool, const void* v_pool, const int32_t* table,
                                           int max_pages, int n_pages, void* o, float* lse, const int32_t* len,
                                           int len_add, void* workspace, int64_t workspace_bytes, int B, int max_len,
                                           int Hq, int Hkv, int head_dim, float scale, void* stream) {
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
  {
    // work: the twin's figure, the bound; what is read is that over the sharing the table holds
    SdProfScope prof(SD_K_MISC, 2.0 * B * Hkv * 256.0 * max_len, ST);
    SD_PROF_LABEL("attn_shared_part_kernel<%d, %d, paged>", sd_attn_shared_group_rows(Hq, Hkv), G);
    shared_part_launch(G, q, k_pool, v_pool, workspace, len, len_add, cap, max_len, B, Hq, Hkv, pstride, np,
                       scale * 1.4426950408889634f, stream, table, max_pages, n_pages);
    SD_CHECK_LAUNCH();
  }
  return sd_attn_decode_merge_launch(workspace, o, lse, len, len_add, cap, max_len, B, Hq, pstride, np, stream);
}

extern "C" int sd_attn_decode_shared_paged_mx(const void* q, const void* k_data, const void* k_scale, const void* v_data,
                                              const void* v_scale, const int32_t* table, int max_pages, int n_pages,
                                              void* o, float* lse, const int32_t* len, int len_add, void* workspace,
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
  {
    SdProfScope prof(SD_K_MISC, 2.0 * B * Hkv * 132.0 * max_len, ST);
    SD_PROF_LABEL("attn_shared_part_kernel<%d, %d, paged, mx>", sd_attn_shared_group_rows(Hq, Hkv), G);
    shared_part_launch(G, q, k_data, v_data, workspace, len, len_add, cap, max_len, B, Hq, Hkv, pstride, np,
                       scale * 1.4426950408889634f, stream, table, max_pages, n_pages, (uint8_t*)k_scale,
                       (uint8_t*)v_scale);
    SD_CHECK_LAUNCH();
  }
  return sd_attn_decode_merge_launch(workspace, o, lse, len, len_add, cap, max_len, B, Hq, pstride, np, stream);
}
