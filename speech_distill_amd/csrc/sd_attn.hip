// Causal GQA flash attention (head_dim 128) forward + backward for gfx950, bf16 in/out, fp32 softmax.
//
// Replaces the flash_attn kernels the reference selects with attn_implementation="flash_attention_2"
// (train.py:160,177); the maths is HF eager_attention_forward (modeling_qwen3.py:185-207):
//     softmax(Q K^T d^-1/2 + causal/key-padding mask, fp32) V,  kv head j serves q heads jG..jG+G-1.
//
// All three kernels use v_mfma_f32_32x32x16_bf16 and ONE LDS image for every [rows][128] bf16 tile:
//     off(row, chunk16B) = 256*row + 16*(chunk ^ (((row&3)<<2) | ((row>>2)&3)))
// which is bank-conflict-free both for row reads (ds_read_b128, operand whose k index is d) and for
// transposed reads (ds_read_b64_tr_b16, operand whose k index is the row).  Tiles arrive by 16-byte
// LDS-DMA with the swizzle applied on the per-lane source address, double buffered.
//
// forward / dQ kernels: S^T = K Q^T, so a lane owns ONE query row (column l&31 of the 32x32 tile) and
//   the online softmax, the LSE / delta terms and the rescale are lane-local; P^T (dS^T) accumulator
//   registers feed the next MFMA as its B operand with no lane movement: O^T = V^T P^T, dQ^T = K^T dS^T.
// dK/dV kernel: S = Q K^T with the key on the lane; a wave owns 32 keys and keeps dK^T, dV^T in
//   registers over all query tiles and all G query heads of its kv head (no atomics, deterministic):
//   dV^T = dO^T P, dK^T = Q^T dS.
#include <type_traits>
#include "sd_common.cuh"
#include "../../include/sd_hip.h"
#include "sd_prof.h"
#include "sd_debug.h"
#include "sd_events.h"

namespace {

constexpr int D = 128;
constexpr int TILE = 64 * D * 2;  // one 64-row tile: 16 KiB
constexpr float NEG = -1.0e30f;
constexpr float LOG2E = 1.4426950408889634f;

SD_DEV int f_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// Stage 64 rows of a [*, 128]-column slice (row stride ld) into a 16 KiB LDS tile through a buffer descriptor
// (buffer_load_dwordx4 ... lds): per-lane offsets are computed once, a tile advance is one scalar offset, rows
// past the end of the (batch, head) slice read as zeros (they are masked later).
template <int NP = 4>  // 1 KiB pieces per wave: 4 when four waves stage a tile, 2 when all eight do
struct TileDma {
  int voff[NP];
  long row_bytes;
#if defined(__HIP_DEVICE_COMPILE__)
  __amdgpu_buffer_rsrc_t rsrc;
#endif
  // g: first element of the slice (row 0 of this batch, this head); rows: rows in the slice
  SD_DEV void init(const bf16* g, long ld, int rows, int w, int lane) {
    row_bytes = ld * 2;
#if defined(__HIP_DEVICE_COMPILE__)
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g, 0, (int)(((long)(rows - 1) * ld + D) * 2), 0x00020000);
#endif
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = (w * NP + i) * 64 + lane;
      const int row = p >> 4, s = p & 15;
      voff[i] = (int)(((long)row * ld + ((s ^ f_swz(row)) * 8)) * 2);
    }
  }
  // the same per-lane offsets over another slice (a page of a paged cache): scalar work only.  rows <= 0: every load
  // arrives as zeros
  SD_DEV void rebase(const bf16* g, int rows) {
#if defined(__HIP_DEVICE_COMPILE__)
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g, 0, rows > 0 ? (int)(((rows - 1) * row_bytes) + D * 2) : 0, 0x00020000);
#endif
  }
  SD_DEV void issue(int row0, char* lds, int w) const {
#if defined(__HIP_DEVICE_COMPILE__)
    const int soff = (int)(row0 * row_bytes);
#pragma unroll
    for (int i = 0; i < NP; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (SD_LDS void*)(lds + (w * NP + i) * 1024), 16, voff[i], soff, 0, 0);
#endif
  }
};

// operand whose k index is d: lane (r = l&31, h = l>>5) holds tile[row0 + r][16*st + 8h .. +7]
SD_DEV bf16x8 row_frag(const char* lds, int row0, int st, int lane) {
  const int row = row0 + (lane & 31);
  const int ch = 2 * st + (lane >> 5);
  return *(const bf16x8*)(lds + row * 256 + ((ch ^ f_swz(row)) << 4));
}

// Operand whose k index is the tile ROW (transposed read): lane (r = l&31 -> column db*32 + r, h = l>>5) holds
// tile[rb + 8(j>>2) + 4h + (j&3)][db*32 + r], j = 0..7  (rb = first row of this 16-row k-step) -- exactly the k
// order of accumulator registers 8s..8s+7 used as the other operand.  Two ds_read_b64_tr_b16 per fragment.
// The fragments for db = 0..3 at once, as asm reads (see lds_tr16_pair_asm: the builtin makes hipcc drain the K/V
// prefetch before every transposed read) followed by one lgkmcnt(0).
SD_DEV void tr_frag4(const char* lds, int rb, int lane, bf16x8 (&out)[4]) {
  const int gi = lane >> 4, i = lane & 15, q4 = i >> 2, pp = i & 3;
  const int rA = rb + 4 * (gi >> 1) + q4, rB = rA + 8;
  const int sA = f_swz(rA), sB = f_swz(rB);
  const unsigned base = lds_addr(lds) + 8 * (pp & 1);
  const unsigned aA = base + rA * 256, aB = base + rB * 256;
  const int chl = (gi & 1) * 2 + (pp >> 1);
  sd_u64 raw[8];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const int ch = db * 4 + chl;
    lds_tr16_pair_asm(raw[2 * db], raw[2 * db + 1], aA + ((ch ^ sA) << 4), aB + ((ch ^ sB) << 4));
  }
  lds_tr_wait8(raw);
#pragma unroll
  for (int db = 0; db < 4; ++db) out[db] = cat8_u64(raw[2 * db], raw[2 * db + 1]);
}

// the same reads without the wait: issue now, tr_finish4 later (the latency hides under whatever runs in between)
SD_DEV void tr_issue4(const char* lds, int rb, int lane, sd_u64 (&raw)[8]) {
  const int gi = lane >> 4, i = lane & 15, q4 = i >> 2, pp = i & 3;
  const int rA = rb + 4 * (gi >> 1) + q4, rB = rA + 8;
  const int sA = f_swz(rA), sB = f_swz(rB);
  const unsigned base = lds_addr(lds) + 8 * (pp & 1);
  const unsigned aA = base + rA * 256, aB = base + rB * 256;
  const int chl = (gi & 1) * 2 + (pp >> 1);
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const int ch = db * 4 + chl;
    lds_tr16_pair_asm(raw[2 * db], raw[2 * db + 1], aA + ((ch ^ sA) << 4), aB + ((ch ^ sB) << 4));
  }
}
SD_DEV void tr_finish4(sd_u64 (&raw)[8], bf16x8 (&out)[4]) {
  lds_tr_wait8(raw);
#pragma unroll
  for (int db = 0; db < 4; ++db) out[db] = cat8_u64(raw[2 * db], raw[2 * db + 1]);
}

// max of a value and the one the lane 32 away holds (v_permlane32_swap: one instruction, no LDS round trip).  As asm:
// hipcc folds fmaxf(pr[0], pr[1]) of __builtin_amdgcn_permlane32_swap(u, u, ..) to pr[0] (it takes the two results of a
// swap of equal operands for equal), which silently leaves every row with the maximum of its first lane half only.
SD_DEV float halves_max(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b));  // a = lo|lo, b = hi|hi
  return fmaxf(a, b);
}

SD_DEV bf16x8 acc_frag(const f32x16& p, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16)p[8 * s + j];
  return r;
}

// row index (within a 32x32 accumulator tile) of register `reg` for lane half h
SD_DEV int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// Epilogue store of a wave's 32 x 128 output tile held as four TRANSPOSED 32x32 accumulators (lane r = l&31 owns output
// ROW r; register e of block db is column db*32 + acc_row(e, h)).  Stored straight from the registers this is 16
// 8-byte stores per lane at a row stride -- every wave-instruction touches 32 different 256-byte rows, and the store
// ISSUE, not bandwidth, sets the time (~9k cycles per workgroup, MI355X_MICROARCH "attention epilogue store tail").
// Instead the tile goes through a wave-private 8 KiB LDS image in the [row][128] swizzled layout of every other tile
// and leaves as whole rows: 16 B per lane, four complete 256-byte rows per wave-instruction, 8 instructions.
SD_DEV void store_tile_rows(char* img, const f32x16 (&acc)[4], float mul, bf16* g_row0, long ld, int rows_valid, int lane) {
  const int r = lane & 31, h = lane >> 5;
  const int swr = f_swz(r);
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (bf16)(acc[db][4 * g4 + e] * mul);
      *(bf16x4*)(img + r * 256 + (((db * 4 + g4) ^ swr) << 4) + 8 * h) = v;
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave's LDS operations complete in order; keep the compiler's too
  const int ch = lane & 15;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = 4 * i + (lane >> 4);
    const bf16x8 v = *(const bf16x8*)(img + row * 256 + ((ch ^ f_swz(row)) << 4));
    if (row < rows_valid) *(bf16x8*)(g_row0 + (long)row * ld + ch * 8) = v;
  }
}

// Workgroup -> (pair, head, batch), XCD-aware.  The hardware deals workgroups to the 8 XCDs round-robin by linear id,
// and every XCD has its own 4 MiB L2.  The `gs` workgroups that stream the same tensors (forward / dQ: the tile pairs of
// the G query heads of one kv head; dK/dV: the key-block pairs of one kv head) would sit on `gs` different XCDs under the
// natural numbering, every L2 would pull every K/V stream (8.4 MB at B=4,T=512), and the first tile of a launch took
// 14 k cycles to arrive.  Here a group is dealt to ONE XCD: id -> (xcd = id % 8, slot = id / 8), group = xcd + 8 *
// (slot / gs), member = slot % gs (when the number of groups is a multiple of 8; the natural order otherwise).
struct AttnWg { int pair, member_head, hkv, b; };
SD_DEV AttnWg attn_wg(int id, int npairs, int heads_per_group, int Hkv, int B) {
  const int gs = npairs * heads_per_group, ng = Hkv * B;
  int g, mem;
  if ((ng & 7) == 0) {
    const int xcd = id & 7, slot = id >> 3;
    g = xcd + 8 * (slot / gs);
    mem = slot % gs;
  } else {
    g = id / gs;
    mem = id % gs;
  }
  AttnWg o;
  o.b = g / Hkv;
  o.hkv = g % Hkv;
  o.member_head = mem / npairs;
  o.pair = mem % npairs;
  return o;
}

// Packed (varlen) calls: the M tokens of the call hold n documents end to end, document s = flat tokens [cu[s], cu[s+1]),
// and every kernel below runs per document exactly as it runs per batch row (tok0 = document start, T = klen = its
// length) when instantiated with VARLEN.  LSE and delta are then [Hq, M].  The tile pairs of document s are numbered
// from base(s) = cu[s] / 128 + s: a document of L tokens has ceil(L / 128) pairs and base(s+1) - base(s) >= that, so
// the numbering never overlaps and stays below the host-known bound ceil(M / 128) + n.  A workgroup finds its document
// by a 64-way search of that (non-decreasing) numbering, one wave-wide load per round, with no scratch and no host
// synchronisation; a slot past a document's last pair exits at once.  Starts and ends are clamped into [0, M] (end >=
// start), so a malformed cu_seqlens can give wrong numbers but never an access outside rows [0, M).
struct VarlenArgs {
  const int* cu;
  int n, M;
};
struct VarlenDoc { int tok0, len, pair; };  // len == 0: nothing to do for this workgroup

SD_DEV int varlen_start(const VarlenArgs& vl, int s) { return min(max(vl.cu[s], 0), vl.M); }

SD_DEV VarlenDoc varlen_doc(const VarlenArgs& vl, int slot, int lane) {
  VarlenDoc d = {0, 0, 0};
  int lo = 0, cnt = vl.n;  // the answer (last s with base(s) <= slot) lies in [lo, lo + cnt)
  bool found = false;
  while (cnt > 0) {
    const int step = (cnt + 63) >> 6;
    const int s = lo + lane * step;
    const bool ok = lane * step < cnt && varlen_start(vl, s) / 128 + s <= slot;
    const unsigned long long bal = __ballot(ok);
    if (!bal) break;  // round 0 only: slot lies before document 0's first pair
    const int k = 63 - __clzll(bal);
    lo += k * step;
    found = true;
    if (step == 1) break;
    cnt = min(step, cnt - k * step);
  }
  if (!found) return d;
  const int start = varlen_start(vl, lo);
  const int end = max(varlen_start(vl, lo + 1), start);
  const int pair = slot - (start / 128 + lo);
  if (pair >= (end - start + 127) / 128) return d;
  d.tok0 = start;
  d.len = end - start;
  d.pair = pair;
  return d;
}

#ifdef SD_STAMPS
// DIAGNOSTIC BUILD ONLY (make stamps): s_memtime at the phase boundaries of workgroup (0,0,0) of attn_fwd_kernel,
// [wave 0..7][point 0..255] (tests/bench_attn_stamps.py)
#define SD_ATT_STAMP_PARAM , unsigned long long* stamps
#define ATT_STAMP()                                                                                   \
  do {                                                                                                \
    if (stamping && lane == 0 && sidx < 256) stamps[w8 * 256 + sidx] = __builtin_amdgcn_s_memtime();   \
    ++sidx;                                                                                           \
  } while (0)
#define ATT_STAMP_AT(COND, SLOT)                                                                            \
  do {                                                                                                      \
    if (stamping && (COND) && lane == 0) stamps[w8 * 256 + (SLOT)] = __builtin_amdgcn_s_memtime();           \
  } while (0)
#else
#define SD_ATT_STAMP_PARAM
#define ATT_STAMP() do { } while (0)
#define ATT_STAMP_AT(COND, SLOT) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------ forward
// grid ceil(ceil(T/64)/2) * Hq * B (decoded by attn_wg), 512 threads.  Under the causal mask a 64-row query tile t sees t+1 K/V tiles, so
// equal row ranges are unequal work (at T = 512: 2, 4, 6, 8 tiles for the four 128-row tiles, and the chip waits for the
// heaviest).  A workgroup therefore takes a PAIR of 64-row query tiles, the j-th lightest and the j-th heaviest (every
// pair sees ceil(T/64)+1 tiles in total): waves 0-3 own the heavy tile, waves 4-7 the light one, and since waves w and
// w+4 share a SIMD every SIMD carries one wave of each.  Both tiles belong to the same (batch, head), so they read the
// same K/V stream: ONE ring streams the heavy tile's K/V tiles, the light tile's waves use the first of them and then
// only keep staging.  Inside a group of four: rb = w&1 is the 32-row block, half = (w>>1)&1 takes keys 32*half..+31 of
// EVERY K/V tile, so all eight waves walk one stream in lockstep through a FOUR-stage ring (4 x (K,V) = 128 KiB): three
// tiles are in flight while one is used.  (Until round 2 the halves took alternate tiles through a double buffer each:
// one tile ahead is less than the L2 latency with all 256 CUs pulling at once, and an iteration cost 3.2 us at T = 512
// against 0.85 us of MFMA time.)  With two waves per SIMD the DMA issue, LDS reads, MFMAs and softmax VALU of one wave
// overlap the other's.  The two partial (m, l, O) states of a row block are merged through LDS at the end (fixed order).
// VARLEN: grid (ceil(M/128) + n) * Hq, one document per workgroup (VarlenArgs above); T is then the call's M on entry.
// The VarlenArgs travel as a trailing parameter pack, empty for the padded instantiation: its kernel arguments, and with
// them its code, stay exactly what they were before the varlen instantiation existed.
template <bool VARLEN, class... VA>
__global__ __launch_bounds__(512) void attn_fwd_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ Kp,
                                                       const bf16* __restrict__ Vp, bf16* __restrict__ O,
                                                       float* __restrict__ LSE, const int* __restrict__ kv_len, long ldq,
                                                       long ldk, long ldv, long ldo, int T, int Hq, int Hkv,
                                                       float scale SD_ATT_STAMP_PARAM, VA... vla) {
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE];  // ring of 4 stages x (K,V)
  const int lane = lane_id(), w8 = wave_id_uniform();
  const VarlenArgs vl{vla...};
  AttnWg vwg = {};
  long vtok0 = 0;
  if constexpr (VARLEN) {
    vwg = attn_wg((int)blockIdx.x, (int)gridDim.x / Hq, Hq / Hkv, Hkv, 1);
    const VarlenDoc dc = varlen_doc(vl, vwg.pair, lane);
    if (dc.len == 0) return;
    T = dc.len;
    vwg.pair = dc.pair;
    vtok0 = dc.tok0;
  }
  const int n64 = (T + 63) / 64;
  const AttnWg wg = VARLEN ? vwg : attn_wg((int)blockIdx.x, (n64 + 1) / 2, Hq / Hkv, Hkv, (int)gridDim.x / (((n64 + 1) / 2) * Hq));
#ifdef SD_STAMPS
  const bool stamping = stamps && wg.pair == 0 && wg.member_head == 0 && wg.hkv == 0 && wg.b == 0;
  int sidx = 0;
#endif
  ATT_STAMP();  // 0: kernel entry
  const int grp = w8 >> 2, rb = w8 & 1, half = (w8 >> 1) & 1;
  const int w = grp * 2 + rb;  // 0..3 inside my half: staging share and merge slot
  // heavy / light 64-row query tile of this workgroup.  (Pairing ADJACENT tiles instead, which keeps both tiles' waves
  // busy for the whole stream, was measured for launches of several rounds of workgroups: slower at every shape, e.g.
  // B=16,T=512 62.5 vs 55.6 us, B=4,T=2048 134.5 vs 131.5 us -- two working waves per SIMD share one vector ALU.)
  const int tA = n64 - 1 - wg.pair, tB = wg.pair;
  const bool active = grp == 0 || tB != tA;      // odd tile count: the middle tile has no partner
  const int hkv = wg.hkv, b = wg.b;
  const int hq = hkv * (Hq / Hkv) + wg.member_head;
  const int q0w = (grp == 0 ? tA : tB) * 64 + 32 * rb;
  const int r = lane & 31, h = lane >> 5;
  const long tok0 = VARLEN ? vtok0 : (long)b * T;
  const bf16* qb = Q + tok0 * ldq + hq * D;
  const bf16* kb = Kp + tok0 * ldk + hkv * D;
  const bf16* vb = Vp + tok0 * ldv + hkv * D;

  // The K/V stream starts before anything else: the first tiles take ~2 us to arrive (cold TLB / L2), and the Q loads,
  // the kv_len read and the rest of the set-up fit under that.
  const int kv_hi = min(tA * 64 + 64, T);  // the heavy tile's diagonal bounds the stream
  const int nkv = (kv_hi + 63) / 64;
  TileDma<2> kd, vd;  // all eight waves stage: two 1 KiB pieces of K and of V per wave and tile
  kd.init(kb, ldk, T, w8, lane);
  vd.init(vb, ldv, T, w8, lane);
  // ring of four (K,V) stages; tile i lives in stage i & 3.  Only tile 0 and the Q fragments go out now: the compiler
  // waits for ALL outstanding loads before the loop (Q lives in registers across it), so anything else issued here
  // would only delay the first tile.  Tiles 1..3 follow right after the first barrier, tile i+3 when tile i-1 retires.
  kd.issue(0, smem, w8);
  vd.issue(0, smem + TILE, w8);
  const int q = q0w + r;  // this lane's query row
  const int qc = q < T ? q : T - 1;
  bf16x8 qf[8];
#pragma unroll
  for (int st = 0; st < 8; ++st) qf[st] = *(const bf16x8*)(qb + (long)qc * ldq + 16 * st + 8 * h);
  ATT_STAMP();  // 1: prologue issued
  const int klen = kv_len ? max(1, min(kv_len[b], T)) : T;
  const int lim = min(q, klen - 1);  // keys > lim are masked for this row

  f32x16 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  float m = NEG, l = 0.f;
  const float c = scale * LOG2E;

  auto visible = [&](int i) { const int kv0 = i * 64 + 32 * half; return active && kv0 < kv_hi && kv0 <= q0w + 31; };
  // One tile = S^T (8 MFMAs, K fragments from LDS) -> online softmax (VALU) -> O^T += V^T P^T (8 MFMAs, transposed V
  // reads, requested before the softmax so that they are there when it ends).  The loop is VALU-bound, not latency- or
  // MFMA-bound (ISA count in round 2: 350 vector-ALU instructions per tile = ~1 600 issue cycles beside 512 cycles of
  // MFMA; two working waves per SIMD take twice as long), so everything that does not depend on the tile is computed
  // once: the per-lane LDS offsets of the K fragments and of the transposed V reads (a tile is then one add per read),
  // and the causal / padding mask sits behind a scalar branch that only the diagonal tiles take.
  unsigned kfo[8], vfo[2][8];
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    const int row = 32 * half + (lane & 31), ch = 2 * st + (lane >> 5);
    kfo[st] = (unsigned)(row * 256 + ((ch ^ f_swz(row)) << 4));
  }
  {
    const int gi = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, pp = i16 & 3;
    const int chl = (gi & 1) * 2 + (pp >> 1);
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const int rA = 32 * half + 16 * ss + 4 * (gi >> 1) + q4, rB = rA + 8;
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const int ch = db * 4 + chl;
        vfo[ss][2 * db] = (unsigned)(8 * (pp & 1) + rA * 256 + ((ch ^ f_swz(rA)) << 4));
        vfo[ss][2 * db + 1] = (unsigned)(8 * (pp & 1) + rB * 256 + ((ch ^ f_swz(rB)) << 4));
      }
    }
  }
  const unsigned smem_a = lds_addr(smem);
  auto tile = [&](int i, int stage) {
    const char* ks = smem + stage * 2 * TILE;
    const unsigned vsa = smem_a + stage * 2 * TILE + TILE;
    f32x16 s1;
#pragma unroll
    for (int e = 0; e < 16; ++e) s1[e] = 0.f;
#pragma unroll
    for (int st = 0; st < 8; ++st) s1 = mfma32(*(const bf16x8*)(ks + kfo[st]), qf[st], s1);
    ATT_STAMP_AT(i == 3, 201);  // S^T MFMAs issued
    sd_u64 rv0[8], rv1[8];
#pragma unroll
    for (int db = 0; db < 4; ++db) lds_tr16_pair_asm(rv0[2 * db], rv0[2 * db + 1], vsa + vfo[0][2 * db], vsa + vfo[0][2 * db + 1]);
#pragma unroll
    for (int db = 0; db < 4; ++db) lds_tr16_pair_asm(rv1[2 * db], rv1[2 * db + 1], vsa + vfo[1][2 * db], vsa + vfo[1][2 * db + 1]);
    const int kv0 = i * 64 + 32 * half;
    // wave-uniform: my keys touch the diagonal / the padding (readfirstlane: a scalar branch, not 16 selects per tile)
    const bool need_mask = __builtin_amdgcn_readfirstlane((int)((kv0 + 31 > q0w) || (kv0 + 31 >= klen))) != 0;
    if (need_mask) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s1[e] = (kv0 + acc_row(e, h)) > lim ? NEG : s1[e];
    }
    float mx = fmaxf(fmaxf(s1[0], s1[1]), s1[2]);
#pragma unroll
    for (int e = 3; e < 15; e += 2) mx = fmaxf(fmaxf(mx, s1[e]), s1[e + 1]);
    mx = fmaxf(mx, s1[15]);
    ATT_STAMP_AT(i == 3, 202);  // lane maxima (S^T complete)
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    ATT_STAMP_AT(i == 3, 203);  // row maxima
    const float mn = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * c);
    m = mn;
    const float mnc = -mn * c;
    float rs = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[e], c, mnc));
      s1[e] = p;
      rs += p;
    }
    l = l * alpha + rs;
    ATT_STAMP_AT(i == 3, 204);  // exponentials
    if (__any(alpha != 1.f)) {  // the running maximum moved for some row of this wave
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
    }
    ATT_STAMP_AT(i == 3, 205);  // rescaled
    bf16x8 vt[4];
    tr_finish4(rv0, vt);  // waits for rv1 too (LDS returns in order)
    ATT_STAMP_AT(i == 3, 206);  // V^T fragments here
    const bf16x8 p0 = acc_frag(s1, 0), p1 = acc_frag(s1, 1);
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = mfma32(vt[db], p0, o[db]);
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = mfma32(cat8_u64(rv1[2 * db], rv1[2 * db + 1]), p1, o[db]);
    ATT_STAMP_AT(i == 3, 207);  // P.V MFMAs issued
  };
  for (int i = 0; i < nkv; ++i) {
    // my share of tile i has landed; younger tiles (4 loads each) may still be in flight
    if (i == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (i + 2 < nkv) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (i + 1 < nkv) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ATT_STAMP();  // 2+4i: my loads of tile i landed
    __builtin_amdgcn_s_barrier();  // everybody's share of tile i has landed; everybody is done reading tile i-1
    asm volatile("" ::: "memory");
    ATT_STAMP();  // 3+4i: barrier passed
    for (int t = (i == 0 ? 1 : i + 3); t <= i + 3; ++t)  // wave-uniform; 1, 2, 3 after the first barrier
      if (t < nkv) {
        char* nx = smem + (t & 3) * 2 * TILE;
        kd.issue(t * 64, nx, w8);
        vd.issue(t * 64, nx + TILE, w8);
      }
    ATT_STAMP();  // 4+4i: next tile issued
    if (visible(i)) {
      ATT_STAMP_AT(i == 3, 200);
      tile(i, i & 3);
    }
    ATT_STAMP();  // 5+4i: tile computed (issue side)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the tail tiles before the ring is reused
  __syncthreads();
  ATT_STAMP();  // 2+4nkv: loop left, ring free
  // merge the two halves: half 1 parks (m, l, O) in LDS, half 0 combines.  Layout [w][slot][lane] floats.
  float* xo = (float*)smem + (long)w * 66 * 64;
  if (half == 1) {
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) xo[(db * 16 + e) * 64 + lane] = o[db][e];
    xo[64 * 64 + lane] = m;
    xo[65 * 64 + lane] = l;
  }
  __syncthreads();
  if (half == 1) return;
  {
    const float m1 = xo[64 * 64 + lane], l1 = xo[65 * 64 + lane];
    const float mn = fmaxf(m, m1);
    const float a0 = __builtin_amdgcn_exp2f((m - mn) * c), a1 = __builtin_amdgcn_exp2f((m1 - mn) * c);
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[db][e] = o[db][e] * a0 + xo[(db * 16 + e) * 64 + lane] * a1;
    l = l * a0 + l1 * a1;
    m = mn;
  }
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.f / l;
  // every lane of a row has the same `inv` only after the two column halves are combined: lanes r and r+32 hold the
  // same row, and `l` was just summed over them, so scaling per lane before the transposing store is exact
  ATT_STAMP();  // 2+4nkv+1: merged
  if (!active) return;
  store_tile_rows((char*)xo, o, inv, O + (tok0 + q0w) * ldo + hq * D, ldo, T - q0w, lane);
  if (q < T && h == 0) LSE[VARLEN ? (long)hq * vl.M + tok0 + q : ((long)b * Hq + hq) * T + q] = m * scale + __logf(l);
  ATT_STAMP();  // stores issued
}

// The same decomposition, ring, merge and arithmetic (bit-identical outputs) with the K/V-tile loop SOFTWARE-PIPELINED
// inside the wave.  In attn_fwd_kernel a tile is one dependent chain -- K fragments -> 8 MFMAs -> maxima -> 16 v_exp ->
// bf16 P -> 8 MFMAs -- of ~2.1 k cycles for 512 cycles of matrix work, and on the heavy tile's SIMDs nothing else runs
// beside it (round-2 stamps, profiles/r02_attn_fwd_stamps.txt: 2.9 k cycles per tile with the DMA issue and the barrier).
// Here iteration i issues S^T(i+1) = K(i+1) Q^T FIRST and runs tile i's exponentials, row sums and bf16 conversion while the
// matrix pipe works on it, then issues O^T += V(i)^T P(i)^T and computes tile i+1's mask and row maxima beside those:
// both matrix products of an iteration have vector work of ANOTHER tile next to them.  The running-maximum update and
// the (rare) rescale of O^T sit at the top of the iteration, before anything is issued.  Tile i+1 has to be in LDS one
// iteration earlier than before, so the four-stage ring keeps two tiles in flight instead of three.
__global__ __launch_bounds__(512) void attn_fwd_pipe_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ Kp,
                                                            const bf16* __restrict__ Vp, bf16* __restrict__ O,
                                                            float* __restrict__ LSE, const int* __restrict__ kv_len,
                                                            long ldq, long ldk, long ldv, long ldo, int T, int Hq, int Hkv,
                                                            float scale SD_ATT_STAMP_PARAM) {
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE];  // ring of 4 stages x (K,V)
  const int lane = lane_id(), w8 = wave_id_uniform();
  const int n64 = (T + 63) / 64;
  const AttnWg wg = attn_wg((int)blockIdx.x, (n64 + 1) / 2, Hq / Hkv, Hkv, (int)gridDim.x / (((n64 + 1) / 2) * Hq));
#ifdef SD_STAMPS
  const bool stamping = stamps && wg.pair == 0 && wg.member_head == 0 && wg.hkv == 0 && wg.b == 0;
  int sidx = 0;
#endif
  ATT_STAMP();  // 0: kernel entry
  const int grp = w8 >> 2, rb = w8 & 1, half = (w8 >> 1) & 1;
  const int w = grp * 2 + rb;
  const int tA = n64 - 1 - wg.pair, tB = wg.pair;
  const bool active = grp == 0 || tB != tA;
  const int hkv = wg.hkv, b = wg.b;
  const int hq = hkv * (Hq / Hkv) + wg.member_head;
  const int q0w = (grp == 0 ? tA : tB) * 64 + 32 * rb;
  const int r = lane & 31, h = lane >> 5;
  const long tok0 = (long)b * T;
  const bf16* qb = Q + tok0 * ldq + hq * D;
  const bf16* kb = Kp + tok0 * ldk + hkv * D;
  const bf16* vb = Vp + tok0 * ldv + hkv * D;
  const int kv_hi = min(tA * 64 + 64, T);
  const int nkv = (kv_hi + 63) / 64;
  TileDma<2> kd, vd;
  kd.init(kb, ldk, T, w8, lane);
  vd.init(vb, ldv, T, w8, lane);
  kd.issue(0, smem, w8);
  vd.issue(0, smem + TILE, w8);
  const int q = q0w + r;
  const int qc = q < T ? q : T - 1;
  bf16x8 qf[8];
#pragma unroll
  for (int st = 0; st < 8; ++st) qf[st] = *(const bf16x8*)(qb + (long)qc * ldq + 16 * st + 8 * h);
  const int klen = kv_len ? max(1, min(kv_len[b], T)) : T;
  const int lim = min(q, klen - 1);

  f32x16 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  float m = NEG, l = 0.f;
  const float c = scale * LOG2E;
  // tiles a wave computes: 0 .. nvis-1 (its keys of tile i start at 64 i + 32 half; at or below its rows' diagonal)
  int nvis = 0;
  if (active) {
    const int last = (q0w + 31 - 32 * half) >> 6;  // floor; negative when even tile 0 is above the diagonal
    nvis = (q0w + 31 - 32 * half) < 0 ? 0 : min(last + 1, (kv_hi - 32 * half + 63) >> 6);
  }
  // LDS offsets inside a tile.  The swizzle is an XOR on the 16-byte chunk index, so the eight K fragments of a lane are
  // ONE offset XOR (st << 5), and the transposed V reads of a 16-key step are two offsets XOR (db << 6): 5 registers
  // live across the loop instead of 24.
  unsigned kf0, vf0[2][2];
  {
    const int row = 32 * half + (lane & 31);
    kf0 = (unsigned)(row * 256 + (((lane >> 5) ^ f_swz(row)) << 4));
    const int gi = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, pp = i16 & 3;
    const int chl = (gi & 1) * 2 + (pp >> 1);
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const int rA = 32 * half + 16 * ss + 4 * (gi >> 1) + q4, rB = rA + 8;
      vf0[ss][0] = (unsigned)(8 * (pp & 1) + rA * 256 + ((chl ^ f_swz(rA)) << 4));
      vf0[ss][1] = (unsigned)(8 * (pp & 1) + rB * 256 + ((chl ^ f_swz(rB)) << 4));
    }
  }
  const unsigned smem_a = lds_addr(smem);
  // S^T of one tile (this wave's 32 keys x its 32 rows): eight chained MFMAs on K fragments read from `stage`
  auto s_tile = [&](int stage, f32x16& s) __attribute__((always_inline)) {
    const char* ks = smem + stage * 2 * TILE;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
    for (int st = 0; st < 8; ++st) s = mfma32(*(const bf16x8*)(ks + (kf0 ^ (unsigned)(st << 5))), qf[st], s);
  };
  // causal / padding mask (diagonal tiles only, behind a scalar branch) and the row maxima of a fresh S^T tile
  auto mask_max = [&](int t, f32x16& s) __attribute__((always_inline)) -> float {
    const int kv0 = t * 64 + 32 * half;
    const bool need_mask = __builtin_amdgcn_readfirstlane((int)((kv0 + 31 > q0w) || (kv0 + 31 >= klen))) != 0;
    if (need_mask) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = (kv0 + acc_row(e, h)) > lim ? NEG : s[e];
    }
    float mx = fmaxf(fmaxf(s[0], s[1]), s[2]);
#pragma unroll
    for (int e = 3; e < 15; e += 2) mx = fmaxf(fmaxf(mx, s[e]), s[e + 1]);
    mx = fmaxf(mx, s[15]);
    return halves_max(mx);
  };

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // Q fragments and my share of tile 0
  // hipcc does not see that wait: without a use of the Q registers HERE it would wait for their loads at their first
  // use inside the loop, with vmcnt(7..0) -- which by then drains the K/V tiles in flight
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    u32x4 t4 = __builtin_bit_cast(u32x4, qf[st]);
    asm volatile("" : "+v"(t4));
    qf[st] = __builtin_bit_cast(bf16x8, t4);
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  for (int t = 1; t <= 2; ++t)
    if (t < nkv) {
      char* nx = smem + (t & 3) * 2 * TILE;
      kd.issue(t * 64, nx, w8);
      vd.issue(t * 64, nx + TILE, w8);
    }
  f32x16 sc, sn;
  float mx = NEG;
  if (nvis > 0) {
    s_tile(0, sc);
    mx = mask_max(0, sc);
  }
  ATT_STAMP();  // 1: prologue done (tile 0 landed, S^T(0) issued)
  for (int i = 0; i < nkv; ++i) {
    // tile i+1 (whose K fragments this iteration reads) has landed; tile i+2 (4 loads of mine) may still be in flight
    if (i + 2 < nkv) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ATT_STAMP();  // 2+4i: my loads of tile i+1 landed
    __builtin_amdgcn_s_barrier();  // everybody's share of tile i+1 is there; everybody is done with tile i-1
    asm volatile("" ::: "memory");
    ATT_STAMP();  // 3+4i: barrier passed
    const bool comp = i < nvis;  // wave-uniform
    // All LDS reads of the iteration go out first, as asm (hipcc keeps only two K fragments in flight and then paces
    // the S^T chain by the LDS latency: ~100 cycles per MFMA instead of 32): the 8 K fragments of tile i+1, then the
    // transposed V reads of tile i's keys 0-15 of this wave; keys 16-31 follow once the K fragments are back (the
    // LDS counter holds 15).  ONE code path: S^T(i+1) is also issued after the wave's last tile (on whatever the next
    // stage holds; the result is dropped) -- a second path without it made hipcc copy the 64 O^T registers around the
    // join every iteration.
    const unsigned ksa = smem_a + ((i + 1) & 3) * 2 * TILE + kf0;
    const unsigned vsa = smem_a + (i & 3) * 2 * TILE + TILE;
    const unsigned va[2][2] = {{vsa + vf0[0][0], vsa + vf0[0][1]}, {vsa + vf0[1][0], vsa + vf0[1][1]}};
    u32x4 kf[8];
    sd_u64 rv0[8], rv1[8];
    if (comp) {
#pragma unroll
      for (int st = 0; st < 8; ++st) asm volatile("ds_read_b128 %0, %1" : "=&v"(kf[st]) : "v"(ksa ^ (unsigned)(st << 5)));
#pragma unroll
      for (int db = 0; db < 4; ++db) lds_tr16_pair_asm(rv0[2 * db], rv0[2 * db + 1], va[0][0] ^ (unsigned)(db << 6), va[0][1] ^ (unsigned)(db << 6));
    }
    // the next tile's DMA goes out while those reads are in flight (~80 cycles of issue per piece)
    if (i + 3 < nkv) {
      char* nx = smem + ((i + 3) & 3) * 2 * TILE;
      kd.issue((i + 3) * 64, nx, w8);
      vd.issue((i + 3) * 64, nx + TILE, w8);
    }
    ATT_STAMP();  // 4+4i: reads and tile i+3 issued
    if (!comp) {
      ATT_STAMP();
      continue;
    }
    const float mn = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * c);
    m = mn;
    const float mnc = -mn * c;
    if (__any(alpha != 1.f)) {  // the running maximum moved for some row of this wave
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
    }
    asm volatile("s_waitcnt lgkmcnt(8)"
                 : "+v"(kf[0]), "+v"(kf[1]), "+v"(kf[2]), "+v"(kf[3]), "+v"(kf[4]), "+v"(kf[5]), "+v"(kf[6]), "+v"(kf[7]));
#pragma unroll
    for (int db = 0; db < 4; ++db) lds_tr16_pair_asm(rv1[2 * db], rv1[2 * db + 1], va[1][0] ^ (unsigned)(db << 6), va[1][1] ^ (unsigned)(db << 6));
#pragma unroll
    for (int e = 0; e < 16; ++e) sn[e] = 0.f;
    // every MFMA of the S^T(i+1) chain with its share of tile i's vector work behind it, fenced: two exponentials
    // (16 of the gap's 32 cycles), their two multiply-adds and two row-sum adds
    float rs = 0.f;
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      sn = mfma32(__builtin_bit_cast(bf16x8, kf[st]), qf[st], sn);
#pragma unroll
      for (int e = 2 * st; e < 2 * st + 2; ++e) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[e], c, mnc));
        sc[e] = p;
        rs += p;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    l = l * alpha + rs;
    const bf16x8 p0 = acc_frag(sc, 0), p1 = acc_frag(sc, 1);
    asm volatile("s_waitcnt lgkmcnt(8)"
                 : "+v"(rv0[0]), "+v"(rv0[1]), "+v"(rv0[2]), "+v"(rv0[3]), "+v"(rv0[4]), "+v"(rv0[5]), "+v"(rv0[6]), "+v"(rv0[7]));
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = mfma32(cat8_u64(rv0[2 * db], rv0[2 * db + 1]), p0, o[db]);
    lds_tr_wait8(rv1);
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = mfma32(cat8_u64(rv1[2 * db], rv1[2 * db + 1]), p1, o[db]);
    mx = mask_max(i + 1, sn);
    sc = sn;
    ATT_STAMP();  // 5+4i: tile i computed (issue side)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  ATT_STAMP();  // 2+4nkv: loop left, ring free
  float* xo = (float*)smem + (long)w * 66 * 64;
  if (half == 1) {
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) xo[(db * 16 + e) * 64 + lane] = o[db][e];
    xo[64 * 64 + lane] = m;
    xo[65 * 64 + lane] = l;
  }
  __syncthreads();
  if (half == 1) return;
  {
    const float m1 = xo[64 * 64 + lane], l1 = xo[65 * 64 + lane];
    const float mn = fmaxf(m, m1);
    const float a0 = __builtin_amdgcn_exp2f((m - mn) * c), a1 = __builtin_amdgcn_exp2f((m1 - mn) * c);
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[db][e] = o[db][e] * a0 + xo[(db * 16 + e) * 64 + lane] * a1;
    l = l * a0 + l1 * a1;
    m = mn;
  }
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.f / l;
  ATT_STAMP();  // merged
  if (!active) return;
  store_tile_rows((char*)xo, o, inv, O + (tok0 + q0w) * ldo + hq * D, ldo, T - q0w, lane);
  if (q < T && h == 0) LSE[((long)b * Hq + hq) * T + q] = m * scale + __logf(l);
  ATT_STAMP();  // stores issued
}

// -------------------------------------------------------------------------- delta = rowsum(dO * O)
__global__ __launch_bounds__(256) void attn_delta_kernel(const bf16* __restrict__ dO, const bf16* __restrict__ O,
                                                         float* __restrict__ delta, long ldo, int T, int Hq, long total) {
  const int lane = lane_id();
  const long idx = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);  // (token, head)
  const int j = lane & 15;
  const bool ok = idx < total;
  const long id = ok ? idx : total - 1;
  const long tok = id / Hq;
  const int hh = (int)(id % Hq);
  bf16x8 a = *(const bf16x8*)(dO + tok * ldo + hh * D + j * 8);
  bf16x8 bb = *(const bf16x8*)(O + tok * ldo + hh * D + j * 8);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += (float)a[e] * (float)bb[e];
  s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 8, 64);
  if (ok && j == 0) {
    const long bidx = tok / T;
    const int t = (int)(tok % T);
    delta[(bidx * Hq + hh) * T + t] = s;
  }
}

// ----------------------------------------------------------------------------------------------- dQ
// Same decomposition as forward: a workgroup takes the j-th heaviest and the j-th lightest 64-row query tile of one
// (batch, head) -- waves 0-3 the heavy one, waves 4-7 the light one, one of each per SIMD -- over ONE K/V stream; inside
// a group rb = w&1 is the 32-row block and half = (w>>1)&1 splits the K/V tiles (t = 2i + half) through its own double
// buffer; the two partial dQ^T of a row block are added through LDS at the end in a fixed order.
// dQ^T[d][q] = scale * sum_key K^T[d][key] dS^T[key][q].
// The body of workgroup `wg_id` of `n_wg` (the numbering attn_wg decodes), written once for the kernel of its own and
// for attn_bwd_kernel; smem: the caller's ONE __shared__ object, 8 tiles = 2 halves x 2 stages x (K,V).
template <bool VARLEN, class... VA>  // as attn_fwd_kernel
SD_DEV void attn_bwd_dq_body(char* smem, int wg_id, int n_wg, const bf16* __restrict__ Q, const bf16* __restrict__ Kp,
                             const bf16* __restrict__ Vp, const bf16* __restrict__ dO, const float* __restrict__ LSE,
                             const float* __restrict__ delta, bf16* __restrict__ dQ, const int* __restrict__ kv_len,
                             long ldq, long ldk, long ldv, long ldo, long lddq, int T, int Hq, int Hkv, float scale,
                             VA... vla) {
  const int lane = lane_id(), w8 = wave_id_uniform();
  const VarlenArgs vl{vla...};
  AttnWg vwg = {};
  long vtok0 = 0;
  if constexpr (VARLEN) {
    vwg = attn_wg(wg_id, n_wg / Hq, Hq / Hkv, Hkv, 1);
    const VarlenDoc dc = varlen_doc(vl, vwg.pair, lane);
    if (dc.len == 0) return;
    T = dc.len;
    vwg.pair = dc.pair;
    vtok0 = dc.tok0;
  }
  const int grp = w8 >> 2, rb = w8 & 1, half = (w8 >> 1) & 1;
  const int w = grp * 2 + rb;  // 0..3 inside my half: staging share and merge slot
  const int n64 = (T + 63) / 64;
  const AttnWg wg = VARLEN ? vwg : attn_wg(wg_id, (n64 + 1) / 2, Hq / Hkv, Hkv, n_wg / (((n64 + 1) / 2) * Hq));
  const int tA = n64 - 1 - wg.pair, tB = wg.pair;
  const bool active = grp == 0 || tB != tA;
  const int hkv = wg.hkv, b = wg.b;
  const int hq = hkv * (Hq / Hkv) + wg.member_head;
  const int q0w = (grp == 0 ? tA : tB) * 64 + 32 * rb;
  const int r = lane & 31, h = lane >> 5;
  const int klen = kv_len ? max(1, min(kv_len[b], T)) : T;
  const long tok0 = VARLEN ? vtok0 : (long)b * T;
  const bf16* qb = Q + tok0 * ldq + hq * D;
  const bf16* kb = Kp + tok0 * ldk + hkv * D;
  const bf16* vb = Vp + tok0 * ldv + hkv * D;
  const bf16* dob = dO + tok0 * ldo + hq * D;
  const int q = q0w + r;
  const int qc = q < T ? q : T - 1;
  bf16x8 qf[8], dof[8];
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    qf[st] = *(const bf16x8*)(qb + (long)qc * ldq + 16 * st + 8 * h);
    dof[st] = *(const bf16x8*)(dob + (long)qc * ldo + 16 * st + 8 * h);
  }
  const int lim = min(q, klen - 1);
  const long sidx = VARLEN ? (long)hq * vl.M + tok0 + qc : ((long)b * Hq + hq) * T + qc;
  const float lse2 = LSE[sidx] * LOG2E;
  const float dl = delta[sidx];
  const float c = scale * LOG2E;
  f32x16 acc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[db][e] = 0.f;

  const int kv_hi = min(tA * 64 + 64, T);
  const int nkv = (kv_hi + 63) / 64;
  const int nit = (nkv + 1) >> 1;  // trips of both halves; half 1 idles through the last one when nkv is odd
  TileDma<> kd, vd;
  kd.init(kb, ldk, T, w, lane);
  vd.init(vb, ldv, T, w, lane);
  char* ring = smem + half * 4 * TILE;
  kd.issue(half * 64, ring, w);
  vd.issue(half * 64, ring + TILE, w);
  int cur_i = 0;
  for (int i = 0; i < nit; ++i) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // my half's tile i has landed; everybody is done reading the other stage
    asm volatile("" ::: "memory");
    if ((2 * (i + 1) + half) * 64 < kv_hi) {  // wave-uniform; a tile nobody will read is not fetched (and not waited for)
      char* nx = ring + (cur_i ^ 1) * 2 * TILE;
      kd.issue((2 * (i + 1) + half) * 64, nx, w);
      vd.issue((2 * (i + 1) + half) * 64, nx + TILE, w);
    }
    const char* ks = ring + cur_i * 2 * TILE;
    const char* vs = ks + TILE;
    cur_i ^= 1;
    const int kv0 = (2 * i + half) * 64;
    if (active && kv0 < kv_hi && kv0 <= q0w + 31) {
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
        for (int st = 0; st < 8; ++st) {
          s = mfma32(row_frag(ks, kb2 * 32, st, lane), qf[st], s);     // S^T  = K Q^T
          dp = mfma32(row_frag(vs, kb2 * 32, st, lane), dof[st], dp);  // dP^T = V dO^T
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = kv0 + kb2 * 32 + acc_row(e, h);
          const float p = key > lim ? 0.f : __builtin_amdgcn_exp2f(s[e] * c - lse2);
          s[e] = p * (dp[e] - dl);  // dS^T (without the d^-1/2 factor)
        }
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
          const bf16x8 df = acc_frag(s, ss);
          bf16x8 kt4[4];
          tr_frag4(ks, kb2 * 32 + 16 * ss, lane, kt4);
#pragma unroll
          for (int db = 0; db < 4; ++db) acc[db] = mfma32(kt4[db], df, acc[db]);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the tail tiles before the ring is reused
  __syncthreads();
  float* xo = (float*)smem + (long)w * 64 * 64;  // [w][slot][lane] floats
  if (half == 1) {
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) xo[(db * 16 + e) * 64 + lane] = acc[db][e];
  }
  __syncthreads();
  if (half == 1 || !active) return;
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[db][e] += xo[(db * 16 + e) * 64 + lane];
  store_tile_rows((char*)xo, acc, scale, dQ + (tok0 + q0w) * lddq + hq * D, lddq, T - q0w, lane);
}

// -------------------------------------------------------------------------------------------- dK, dV
// grid ceil(ceil(T/64)/2) * Hkv * B (decoded by attn_wg), 512 threads = 8 waves, two per SIMD.  Key block kb (64 keys) is seen by the query
// tiles kb .. ceil(T/64)-1, so the first blocks carry most of the work; a workgroup takes the j-th heaviest and the
// j-th lightest block (every pair: ceil(T/64)+1 block-tile visits per query head): waves 0-3 the heavy one, waves 4-7
// the light one, one of each per SIMD.  Inside a group sub = w&1 is the 32-key sub-block a wave owns (the lane owns one
// key: S = Q K^T with the key on the lane) and rh = (w>>1)&1 the 32-row half of every 64-row (Q, dO) tile it takes.
// The block loops over the G query heads of the group and over the query tiles at or below the heavy block's
// diagonal (the light block's waves skip the tiles above theirs); a wave keeps dK^T, dV^T of its keys in registers
// (dV^T = dO^T P, dK^T = Q^T dS), and the two row halves are added through LDS at the end in a fixed order (no atomics,
// deterministic).  With ONE wave per SIMD a wave ran its DMA issue, LDS reads, 64 MFMAs and the exp/mask VALU of a
// tile strictly one after the other; two independent waves per SIMD overlap those phases.  To fit two waves into the
// SIMD's 512 registers the two blocks' K and V (128 keys) live in LDS instead of registers (64 KiB), beside a 2-stage
// (Q, dO) ring (64 KiB): waves 0-3 stage K and the Q tiles, waves 4-7 stage V and the dO tiles.
// The body of workgroup `wg_id` of `n_wg`, as attn_bwd_dq_body.  smem, 8 tiles + 1 KiB:
// [K: heavy block 64 rows | light block 64 rows][V: same][stage 0: Q, dO | stage 1: Q, dO | stat[2 stages][lse2|delta][64 q rows]]
template <bool VARLEN, class... VA>  // as attn_fwd_kernel, (ceil(M/128) + n) * Hkv workgroups
SD_DEV void attn_bwd_dkv_body(char* smem, int wg_id, int n_wg, const bf16* __restrict__ Q, const bf16* __restrict__ Kp,
                              const bf16* __restrict__ Vp, const bf16* __restrict__ dO, const float* __restrict__ LSE,
                              const float* __restrict__ delta, bf16* __restrict__ dK, bf16* __restrict__ dV,
                              const int* __restrict__ kv_len, long ldq, long ldk, long ldv, long ldo, long lddk,
                              long lddv, int T, int Hq, int Hkv, float scale, VA... vla) {
  const int lane = lane_id(), w8 = wave_id_uniform();
  const VarlenArgs vl{vla...};
  AttnWg vwg = {};
  long vtok0 = 0;
  if constexpr (VARLEN) {
    vwg = attn_wg(wg_id, n_wg / Hkv, 1, Hkv, 1);
    const VarlenDoc dc = varlen_doc(vl, vwg.pair, lane);
    if (dc.len == 0) return;
    T = dc.len;
    vwg.pair = dc.pair;
    vtok0 = dc.tok0;
  }
  const int grp = w8 >> 2, sub = w8 & 1, rh = (w8 >> 1) & 1;  // compute role
  const int sw = w8 & 3;                                       // staging share inside my group of four
  const int G = Hq / Hkv;
  const int n64 = (T + 63) / 64;
  const AttnWg wg = VARLEN ? vwg : attn_wg(wg_id, (n64 + 1) / 2, 1, Hkv, n_wg / (((n64 + 1) / 2) * Hkv));
  const int hkv = wg.hkv, b = wg.b;
  const int kbA = wg.pair, kbB = n64 - 1 - wg.pair;  // heavy / light key block
  const bool active = grp == 0 || kbB != kbA;                       // odd block count: the middle block has no partner
  const int k0w = (grp == 0 ? kbA : kbB) * 64 + 32 * sub;
  const int r = lane & 31, h = lane >> 5;
  const int klen = kv_len ? max(1, min(kv_len[b], T)) : T;
  const long tok0 = VARLEN ? vtok0 : (long)b * T;
  const int key = k0w + r;  // this lane's key (column of S)
  const bool key_ok = key < klen;  // padded / out-of-range keys receive no probability
  const float c = scale * LOG2E;
  char* const ksm = smem;
  char* const vsm = smem + 2 * TILE;
  char* const ring = smem + 4 * TILE;
  float* const stat = (float*)(smem + 8 * TILE);  // [stage][which][64]
  {
    TileDma<> kvd;
    kvd.init((grp ? Vp + tok0 * ldv : Kp + tok0 * ldk) + hkv * D, grp ? ldv : ldk, T, sw, lane);
    char* dst = grp ? vsm : ksm;
    kvd.issue(kbA * 64, dst, sw);
    kvd.issue(kbB * 64, dst + TILE, sw);
  }
  f32x16 dk[4], dv[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) { dk[db][e] = 0.f; dv[db][e] = 0.f; }

  const int qt0 = kbA;                 // first 64-row query tile that can see a key of the heavy block
  const int per_head = n64 - qt0;
  const int nit = G * per_head;
  const int st_i = threadIdx.x & 63, st_which = (threadIdx.x >> 6) & 1;
  // LSE / delta of the 64 query rows of tile `it` (threads 0..127), loaded an iteration before they are written to LDS
  auto load_stat = [&](int it) -> float {
    if (threadIdx.x >= 128) return 0.f;
    const int itc = it < nit ? it : nit - 1;
    const int hq = hkv * G + itc / per_head;
    int qq = (qt0 + itc % per_head) * 64 + st_i;
    qq = qq < T ? qq : T - 1;
    const long o = VARLEN ? (long)hq * vl.M + tok0 + qq : ((long)b * Hq + hq) * T + qq;
    return st_which ? delta[o] : LSE[o] * LOG2E;
  };
  // one tile = Q rows (waves 0-3) + dO rows (waves 4-7) of query head g, rows qt*64 .. +63
  auto stage_it = [&](int it, int buf) {
    const int g = it / per_head, qt = qt0 + it % per_head;
    const int hq = hkv * G + g;
    TileDma<> d;  // the query head changes with `it`: the descriptor is rebuilt (scalar work only)
    d.init((grp ? dO + tok0 * ldo : Q + tok0 * ldq) + hq * D, grp ? ldo : ldq, T, sw, lane);
    d.issue(qt * 64, ring + buf * 2 * TILE + grp * TILE, sw);
  };
  {
    const float sv0 = load_stat(0);
    stage_it(0, 0);
    if (threadIdx.x < 128) stat[st_which * 64 + st_i] = sv0;
  }
  float pend_sv = load_stat(1);
  for (int it = 0; it < nit; ++it) {
    const int buf = it & 1;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // tile `it` (and K, V) landed; everybody has finished reading the other stage
    asm volatile("" ::: "memory");
    if (threadIdx.x < 128) stat[(buf ^ 1) * 128 + st_which * 64 + st_i] = pend_sv;
    pend_sv = load_stat(it + 2);
    if (it + 1 < nit) stage_it(it + 1, buf ^ 1);
    const char* qs = ring + buf * 2 * TILE;
    const char* dos = qs + TILE;
    const int qb0 = (qt0 + it % per_head) * 64 + 32 * rh;
    if (!active || qb0 + 31 < k0w) continue;  // wave-uniform: this wave's 32 query rows are all above its keys
    f32x16 s, dp;
#pragma unroll
    for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      s = mfma32(row_frag(qs, 32 * rh, st, lane), row_frag(ksm, 64 * grp + 32 * sub, st, lane), s);     // S  = Q K^T
      dp = mfma32(row_frag(dos, 32 * rh, st, lane), row_frag(vsm, 64 * grp + 32 * sub, st, lane), dp);  // dP = dO V^T
    }
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const f32x4 l2 = *(const f32x4*)&stat[buf * 128 + 32 * rh + 8 * g4 + 4 * h];
      const f32x4 dl = *(const f32x4*)&stat[buf * 128 + 64 + 32 * rh + 8 * g4 + 4 * h];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int qq = qb0 + 8 * g4 + 4 * h + e;
        const bool vis = key_ok && key <= qq && qq < T;
        const float p = vis ? __builtin_amdgcn_exp2f(s[4 * g4 + e] * c - l2[e]) : 0.f;
        s[4 * g4 + e] = p;
        dp[4 * g4 + e] = p * (dp[4 * g4 + e] - dl[e]);  // dS (without the d^-1/2 factor)
      }
    }
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      bf16x8 t4[4];
      const bf16x8 pf = acc_frag(s, ss);
      tr_frag4(dos, 32 * rh + 16 * ss, lane, t4);
#pragma unroll
      for (int db = 0; db < 4; ++db) dv[db] = mfma32(t4[db], pf, dv[db]);  // dV^T += dO^T P
      const bf16x8 df = acc_frag(dp, ss);
      tr_frag4(qs, 32 * rh + 16 * ss, lane, t4);
#pragma unroll
      for (int db = 0; db < 4; ++db) dk[db] = mfma32(t4[db], df, dk[db]);  // dK^T += Q^T dS
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // drain before LDS is reused
  __syncthreads();
  // merge: row half 1 parks dK^T then dV^T of its keys in LDS ([slot][reg][lane] floats, 16 KiB per wave and round)
  float* xo = (float*)smem + (long)(grp * 2 + sub) * 64 * 64;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    f32x16* acc = round ? dv : dk;
    if (rh == 1) {
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) xo[(db * 16 + e) * 64 + lane] = acc[db][e];
    }
    __syncthreads();
    if (rh == 0) {
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[db][e] += xo[(db * 16 + e) * 64 + lane];
    }
    __syncthreads();
  }
  if (rh == 0 && active) {
    store_tile_rows((char*)xo, dk, scale, dK + (tok0 + k0w) * lddk + hkv * D, lddk, T - k0w, lane);
    store_tile_rows((char*)xo + 8192, dv, 1.f, dV + (tok0 + k0w) * lddv + hkv * D, lddv, T - k0w, lane);
  }
}

// The whole backward as ONE launch: the role of a workgroup follows from blockIdx.x.  Ids [0, n_dkv) run the dK/dV body,
// ids n_dkv8 + [0, n_dq) the dQ body, n_dkv8 = n_dkv rounded up to a multiple of 8 (the ids between return at once): a dQ
// workgroup's own id then has the low three bits of blockIdx.x, which attn_wg takes for the XCD.  The two bodies share
// read-only inputs only, and a workgroup is one or the other, so every barrier stays workgroup-uniform.  Workgroups are
// dispatched in id order: the long dK/dV workgroups go out first and the dQ workgroups fill what is left (longest first).
// Against two launches on two streams joined by events: 43 us instead of 38 + 23 us per layer on one stream, -0.44 /
// -0.50 ms per config-2 step (tests/bench_knob_ab.py attn.bwd_split 0 1).
// (ONE __shared__ object for both roles: a second one beside an LDS-DMA target makes hipcc drain vmcnt before LDS reads)
template <bool VARLEN, class... VA>
__global__ __launch_bounds__(512) void attn_bwd_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ Kp,
                                                       const bf16* __restrict__ Vp, const bf16* __restrict__ dO,
                                                       const float* __restrict__ LSE, const float* __restrict__ delta,
                                                       bf16* __restrict__ dQ, bf16* __restrict__ dK, bf16* __restrict__ dV,
                                                       const int* __restrict__ kv_len, long ldq, long ldk, long ldv,
                                                       long ldo, long lddq, long lddk, long lddv, int T, int Hq, int Hkv,
                                                       float scale, int n_dkv, int n_dq, VA... vla) {
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE + 1024];
  const int id = (int)blockIdx.x, n_dkv8 = (n_dkv + 7) & ~7;
  if (id < n_dkv)
    attn_bwd_dkv_body<VARLEN>(smem, id, n_dkv, Q, Kp, Vp, dO, LSE, delta, dK, dV, kv_len, ldq, ldk, ldv, ldo, lddk, lddv, T,
                              Hq, Hkv, scale, vla...);
  else if (id >= n_dkv8)
    attn_bwd_dq_body<VARLEN>(smem, id - n_dkv8, n_dq, Q, Kp, Vp, dO, LSE, delta, dQ, kv_len, ldq, ldk, ldv, ldo, lddq, T, Hq,
                             Hkv, scale, vla...);
}

// The two bodies as kernels of their own (attn.bwd_split: the two-launch schedule, for A/B measurements and parity tests)
template <bool VARLEN, class... VA>
__global__ __launch_bounds__(512) void attn_bwd_dq_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ Kp,
                                                          const bf16* __restrict__ Vp, const bf16* __restrict__ dO,
                                                          const float* __restrict__ LSE, const float* __restrict__ delta,
                                                          bf16* __restrict__ dQ, const int* __restrict__ kv_len, long ldq,
                                                          long ldk, long ldv, long ldo, long lddq, int T, int Hq, int Hkv,
                                                          float scale, VA... vla) {
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE];
  attn_bwd_dq_body<VARLEN>(smem, (int)blockIdx.x, (int)gridDim.x, Q, Kp, Vp, dO, LSE, delta, dQ, kv_len, ldq, ldk, ldv, ldo,
                           lddq, T, Hq, Hkv, scale, vla...);
}
template <bool VARLEN, class... VA>
__global__ __launch_bounds__(512) void attn_bwd_dkv_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ Kp,
                                                           const bf16* __restrict__ Vp, const bf16* __restrict__ dO,
                                                           const float* __restrict__ LSE, const float* __restrict__ delta,
                                                           bf16* __restrict__ dK, bf16* __restrict__ dV,
                                                           const int* __restrict__ kv_len, long ldq, long ldk, long ldv,
                                                           long ldo, long lddk, long lddv, int T, int Hq, int Hkv,
                                                           float scale, VA... vla) {
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE + 1024];
  attn_bwd_dkv_body<VARLEN>(smem, (int)blockIdx.x, (int)gridDim.x, Q, Kp, Vp, dO, LSE, delta, dK, dV, kv_len, ldq, ldk, ldv,
                            ldo, lddk, lddv, T, Hq, Hkv, scale, vla...);
}

int check_common(int B, int T, int Hq, int Hkv, long ldq, long ldk, long ldv, long ldo) {
  if (B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv)) return SD_ERR_SHAPE;
  if ((ldq | ldk | ldv | ldo) & 7) return SD_ERR_ALIGN;
  return 0;
}

}  // namespace

#ifdef SD_STAMPS
static unsigned long long* g_attn_stamps = nullptr;
extern "C" void sd_debug_attn_stamp_buffer(void* p) { g_attn_stamps = (unsigned long long*)p; }
#define SD_ATT_STAMP_ARG , g_attn_stamps
#else
#define SD_ATT_STAMP_ARG
#endif

// bit 0: forward without the in-wave software pipeline (attn_fwd_kernel) at any T; bit 1: with it at any T (default:
// from T = 1024); tests and A/B measurements
// (g_sd_debug.attn_variant, include/sd_hip_debug.h key "attn.variant")

extern "C" int sd_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* kv_len,
                           int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int B, int T, int Hq, int Hkv,
                           int head_dim, float scale, void* stream) {
  if (head_dim != D) return SD_ERR_UNSUPPORTED;
  if (int e = check_common(B, T, Hq, Hkv, ldq, ldk, ldv, ldo)) return e;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) return SD_ERR_ALIGN;
  SdProfScope prof(SD_K_ATTN_FWD, 2.0 * B * Hq * (double)T * T * D, (hipStream_t)stream);  // 2 products, causal half
  const dim3 grid((((T + 63) / 64 + 1) / 2) * Hq * B);
  // Measured (tests/bench_attn_pipe.py, MI355X, 16/8 heads): the pipelined kernel is 3-5 % faster from T = 1024 (21.8 vs
  // 22.2 us at B=2, 32.9 vs 34.6 us at B=1 T=2048, 119 vs 123 us at B=4 T=2048) and ties or loses 0.1-0.5 us below
  // (its prologue computes S^T(0) before the loop and needs tile 1 for the first iteration), so short streams keep the
  // classic kernel.  bit 1 of the variant forces the pipelined one at any T (tests).
  const bool pipe = (g_sd_debug.attn_variant & 2) || (!(g_sd_debug.attn_variant & 1) && T >= 1024);
  if (pipe) {
    hipLaunchKernelGGL(attn_fwd_pipe_kernel, grid, dim3(512), 0, (hipStream_t)stream, (const bf16*)q, (const bf16*)k,
                       (const bf16*)v, (bf16*)o, lse, kv_len, ldq, ldk, ldv, ldo, T, Hq, Hkv, scale SD_ATT_STAMP_ARG);
    SD_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(attn_fwd_kernel<false>, grid, dim3(512), 0, (hipStream_t)stream, (const bf16*)q,
                     (const bf16*)k, (const bf16*)v, (bf16*)o, lse, kv_len, ldq, ldk, ldv, ldo, T, Hq, Hkv, scale SD_ATT_STAMP_ARG);
  SD_CHECK_LAUNCH();
  return 0;
}

namespace {

struct BwdTensors {
  const bf16 *q, *k, *v, *d_o; const float *lse, *delta; bf16 *dq, *dk, *dv; const int* kv_len;
  long ldq, ldk, ldv, ldo, lddq, lddk, lddv; int T, Hq, Hkv; float scale;
};

// dQ, dK and dV of one call once delta is final on `stream`.  groups: tile pairs times batch rows, i.e. workgroups per
// head; work: FLOPs of ONE of the seven half-masked products.  One launch on `stream` (attn_bwd_kernel); `side_stream`
// is not used.  attn.bwd_split (sd_hip_debug.h): the dQ kernel on the side stream (when given) beside the dK/dV kernel,
// ordered by this call's events.
template <bool VARLEN, class... VA>
int launch_bwd(const BwdTensors& t, long groups, double work, void* side_stream, void* stream, VA... va) {
  const long n_dq = groups * t.Hq, n_dkv = groups * t.Hkv, n_dkv8 = (n_dkv + 7) & ~7L;
  if (n_dkv8 + n_dq > 0x7fffffffL) return SD_ERR_SHAPE;
  if (!g_sd_debug.attn_bwd_split) {
    hipStream_t st = (hipStream_t)stream;
    SdProfScope prof(SD_K_ATTN_BWD_DKV, 7.0 * work, st);  // S, dP, dV, dK + S, dP (recomputed), dQ
    hipLaunchKernelGGL((attn_bwd_kernel<VARLEN, VA...>), dim3((unsigned)(n_dkv8 + n_dq)), dim3(512), 0, st, t.q, t.k, t.v,
                       t.d_o, t.lse, t.delta, t.dq, t.dk, t.dv, t.kv_len, t.ldq, t.ldk, t.ldv, t.ldo, t.lddq, t.lddk, t.lddv,
                       t.T, t.Hq, t.Hkv, t.scale, (int)n_dkv, (int)n_dq, va...);
    SD_CHECK_LAUNCH();
    return 0;
  }
  SdStreamOrder ord;  // this call's events (per call, per device)
  if (int e = ord.init(stream, side_stream)) return e;
  hipStream_t st = ord.main, sq = ord.side ? ord.side : ord.main;  // sq: stream of the dQ kernel
  if (int e = ord.side_waits_for_main(kEvAttnInputs)) return e;
  {
    SdProfScope prof2(SD_K_ATTN_BWD_DQ, 3.0 * work, sq);  // S, dP (recomputed), dQ
    hipLaunchKernelGGL((attn_bwd_dq_kernel<VARLEN, VA...>), dim3((unsigned)n_dq), dim3(512), 0, sq, t.q, t.k, t.v, t.d_o,
                       t.lse, t.delta, t.dq, t.kv_len, t.ldq, t.ldk, t.ldv, t.ldo, t.lddq, t.T, t.Hq, t.Hkv, t.scale, va...);
  }
  SD_CHECK_LAUNCH();
  {
    SdProfScope prof(SD_K_ATTN_BWD_DKV, 4.0 * work, st);  // S, dP, dV, dK
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<VARLEN, VA...>), dim3((unsigned)n_dkv), dim3(512), 0, st, t.q, t.k, t.v, t.d_o,
                       t.lse, t.delta, t.dk, t.dv, t.kv_len, t.ldq, t.ldk, t.ldv, t.ldo, t.lddk, t.lddv, t.T, t.Hq, t.Hkv,
                       t.scale, va...);
  }
  SD_CHECK_LAUNCH();
  return ord.main_waits_for_side(kEvAttnDq);
}

}  // namespace

extern "C" int sd_attn_bwd2(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                            float* delta, void* dq, void* dk, void* dv, const int32_t* kv_len, int64_t ldq, int64_t ldk,
                            int64_t ldv, int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, int B, int T, int Hq,
                            int Hkv, int head_dim, float scale, void* side_stream, void* stream) {
  if (head_dim != D) return SD_ERR_UNSUPPORTED;
  if (int e = check_common(B, T, Hq, Hkv, ldq, ldk, ldv, ldo)) return e;
  if ((lddq | lddk | lddv) & 7) return SD_ERR_ALIGN;
  const long total = (long)B * T * Hq;
  if (o) {  // o == NULL: `delta` already holds rowsum(dO * O) (sd_gemm_odx_delta)
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16*)d_o, (const bf16*)o, delta, ldo, T, Hq, total);
    SD_CHECK_LAUNCH();
  }
  const BwdTensors t{(const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)d_o, lse, delta, (bf16*)dq, (bf16*)dk,
                     (bf16*)dv, kv_len, ldq, ldk, ldv, ldo, lddq, lddk, lddv, T, Hq, Hkv, scale};
  return launch_bwd<false>(t, (long)(((T + 63) / 64 + 1) / 2) * B, (double)B * Hq * (double)T * T * D, side_stream, stream);
}

extern "C" int sd_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                           float* delta, void* dq, void* dk, void* dv, const int32_t* kv_len, int64_t ldq, int64_t ldk,
                           int64_t ldv, int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, int B, int T, int Hq,
                           int Hkv, int head_dim, float scale, void* stream) {
  return sd_attn_bwd2(q, k, v, o, d_o, lse, delta, dq, dk, dv, kv_len, ldq, ldk, ldv, ldo, lddq, lddk, lddv, B, T, Hq,
                      Hkv, head_dim, scale, nullptr, stream);
}

// ------------------------------------------------------------------------------------ packed (varlen) entries
extern "C" int64_t sd_varlen_work_bytes(int M) { return M < 0 ? SD_ERR_SHAPE : 0; }

namespace {

// validates a descriptor; grid pairs per head = ceil(M/128) + n (VarlenArgs)
int varlen_check(const sd_varlen* vl, int M, int Hq, int Hkv, long ldq, long ldk, long ldv, long ldo, VarlenArgs* va,
                 unsigned* pairs) {
  if (!vl || !vl->cu_seqlens || vl->n_seqs <= 0) return SD_ERR_SHAPE;
  if (int e = check_common(1, M, Hq, Hkv, ldq, ldk, ldv, ldo)) return e;
  const long p = (M + 127L) / 128 + vl->n_seqs;
  if (p * Hq > 0x7fffffffL) return SD_ERR_SHAPE;
  va->cu = vl->cu_seqlens;
  va->n = vl->n_seqs;
  va->M = M;
  *pairs = (unsigned)p;
  return 0;
}

}  // namespace

extern "C" int sd_attn_fwd_varlen(const void* q, const void* k, const void* v, void* o, float* lse, const sd_varlen* vl,
                                  int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int M, int Hq, int Hkv,
                                  int head_dim, float scale, void* stream) {
  if (head_dim != D) return SD_ERR_UNSUPPORTED;
  VarlenArgs va;
  unsigned pairs;
  if (int e = varlen_check(vl, M, Hq, Hkv, ldq, ldk, ldv, ldo, &va, &pairs)) return e;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) return SD_ERR_ALIGN;
  // work: sum over documents of L^2 <= M * max_seqlen (the bound; the host does not know the lengths)
  const double ml = vl->max_seqlen > 0 ? (double)(vl->max_seqlen < M ? vl->max_seqlen : M) : (double)M;
  SdProfScope prof(SD_K_ATTN_FWD, 2.0 * Hq * (double)M * ml * D, (hipStream_t)stream);
  attn_fwd_kernel<true, VarlenArgs><<<dim3(pairs * Hq), dim3(512), 0, (hipStream_t)stream>>>(
      (const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, lse, nullptr, ldq, ldk, ldv, ldo, M, Hq, Hkv,
      scale SD_ATT_STAMP_ARG, va);
  SD_CHECK_LAUNCH();
  return 0;
}

extern "C" int sd_attn_bwd_varlen(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                                  const float* lse, float* delta, void* dq, void* dk, void* dv, const sd_varlen* vl,
                                  int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddq, int64_t lddk,
                                  int64_t lddv, int M, int Hq, int Hkv, int head_dim, float scale, void* side_stream,
                                  void* stream) {
  if (head_dim != D) return SD_ERR_UNSUPPORTED;
  VarlenArgs va;
  unsigned pairs;
  if (int e = varlen_check(vl, M, Hq, Hkv, ldq, ldk, ldv, ldo, &va, &pairs)) return e;
  if ((lddq | lddk | lddv) & 7) return SD_ERR_ALIGN;
  const long total = (long)M * Hq;
  if (o) {  // per token: one row of M tokens is exactly the [Hq, M] layout of the packed LSE / delta
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16*)d_o, (const bf16*)o, delta, ldo, M, Hq, total);
    SD_CHECK_LAUNCH();
  }
  const double ml = vl->max_seqlen > 0 ? (double)(vl->max_seqlen < M ? vl->max_seqlen : M) : (double)M;
  const BwdTensors t{(const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)d_o, lse, delta, (bf16*)dq, (bf16*)dk,
                     (bf16*)dv, nullptr, ldq, ldk, ldv, ldo, lddq, lddk, lddv, M, Hq, Hkv, scale};
  return launch_bwd<true>(t, (long)pairs, Hq * (double)M * ml * D, side_stream, stream, va);
}

// ------------------------------------------------------------------------------------------ extend
// Causal attention of a block of T new query rows per sequence, at positions past[b] + t, over a live KV cache: the keys
// already cached plus the block's own (stored into the planes before this call).  The decomposition of attn_fwd_kernel
// (S^T = K Q^T, a lane owns one query row, O^T = V^T P^T, one swizzled LDS image, LDS-DMA), arranged for the cache:
//   grid (ceil(T/64), Hkv, B), 128 G threads (G = Hq / Hkv).  A workgroup owns one 64-row query tile of one sequence and
//   ALL G query heads of one kv head: wave w serves head hkv*G + (w >> 1), rows 32 (w & 1) .. + 31 of the tile, and every
//   wave takes all 64 keys of a K/V tile, so a tile is staged once for the whole group (two stages of (K,V), 64 KiB).
//   K/V tiles come from the cache plane (row stride Hkv*128) and are ANCHORED AT CACHE SLOT 0: tile i is slots 64 i ..
//   64 i + 63 whatever past is, and the loop stops at the tile of the workgroup's last visible key.
// Bit contract (tests/test_gpu_attn_extend.py): o and lse of a row depend on its query, its position and the visible
// K / V rows only.  A row's running (m, l, O) live in its own lane pair; the online softmax steps over the same absolute
// tiles however the sequence was split into past and block; a masked key gets the score -1e30 BEFORE the row maximum and
// therefore probability exactly 0 (exp2 underflows; key 0 is visible to every row that sees anything, so the maximum is
// a real score from the first tile on); a tile that lies wholly above a row's diagonal changes nothing for that row
// (alpha = 1, p = 0), which is why a wave may skip it or compute it.  No atomics, no split over keys.
// Slots >= past + new_len are outside the buffer descriptor of the stream: they read as zeros and are masked.
// Paged (llm_engine.py:91; the page table travels as a trailing parameter pack, empty for the contiguous instantiation,
// whose arguments and code stay what they were): a page is four tiles, so a tile never straddles one.  The buffer
// descriptor is rebuilt per page -- base = the page's first row for this kv head, min(256, kv_end - 256 page_index)
// records, so the slots >= kv_end still arrive as zeros -- from a page number held in scalar registers, which is
// fetched one page (four tiles) ahead of the DMA that needs it.  Tile order, masks, online softmax and stores are untouched.
// 8-bit pages (MXFP8, include/sd_hip.h; the pack then also carries the two E8M0 scale planes): only the staging differs.
// A tile cannot go global -> LDS by DMA, so every lane loads the 8 e4m3 bytes of each 16-byte piece TileDma would have
// handed it (same row, same swizzled source chunk) and the piece's block scale byte, turns them into the bf16x8 they stand
// for and writes it to the LDS address the DMA would have written; rows at or past min(256, kv_end - 256 page_index), and
// every row of an out-of-range page, are written as zeros, as the descriptor delivers them.  The loads of tile i + 1 are
// issued before tile i is computed and held in registers (2 NP x 8 bytes + 2 NP scale bytes per lane) until the ring
// slot is free.  The LDS image, and everything that reads it, is the same.
namespace {
static_assert(SD_KV_PAGE % 64 == 0, "a 64-key tile must not straddle a page");
struct ExtPageArgs {
  const int* table;  // int32 [B][max_pages]
  int max_pages, n_pages;
  const uint8_t *k_scale = nullptr, *v_scale = nullptr;  // 8-bit pages only: E8M0 planes [n_pages][256][Hkv*4]
};
// 8 e4m3 bytes and their block's E8M0 byte -> the bf16 values they stand for (exact for scale bytes 3..246)
SD_DEV bf16x8 mx_to_bf16x8(u32x2 q, uint32_t scale_byte) {
  const float sc = __builtin_bit_cast(float, scale_byte << 23);
  bf16x8 r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[h], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[h], true);
    r[4 * h] = (bf16)(a[0] * sc); r[4 * h + 1] = (bf16)(a[1] * sc);
    r[4 * h + 2] = (bf16)(b[0] * sc); r[4 * h + 3] = (bf16)(b[1] * sc);
  }
  return r;
}
template <int G, class... PG>
__global__ __launch_bounds__(128 * G) void attn_extend_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ Kp,
                                                              const bf16* __restrict__ Vp, bf16* __restrict__ O,
                                                              float* __restrict__ LSE, const int* __restrict__ past_p,
                                                              const int* __restrict__ new_p, long ldq, long ldo, int T,
                                                              int cap, int Hq, int Hkv, float scale, PG... pga) {
  constexpr bool PAGED = sizeof...(PG) > 0;
  constexpr bool MX = sizeof...(PG) == 5;
  constexpr int TPP = SD_KV_PAGE / 64;  // tiles per page
  const ExtPageArgs pg{pga...};
  constexpr int NW = 2 * G;    // waves
  constexpr int NP = 16 / NW;  // 1 KiB pieces of a tile each wave stages
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];  // 2 stages x (K,V); then a store image per wave
  const int lane = lane_id(), w = wave_id_uniform();
  const int qt = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  // clamped before any address is formed
  const int past = min(max(past_p[b], 0), cap);
  const int nnew = min(max(new_p[b], 0), min(T, cap - past));
  const int kv_end = past + nnew;  // <= cap: keys [0, kv_end) exist
  const int hq = hkv * G + (w >> 1);
  const int t0w = qt * 64 + 32 * (w & 1);  // first block row of this wave
  const int r = lane & 31, h = lane >> 5;
  const int t = t0w + r;  // this lane's row of the block
  const int tc = t < T ? t : T - 1;
  bf16* orow = O + ((long)b * T + t0w) * ldo + hq * D;
  float* lrow = LSE ? LSE + ((long)b * Hq + hq) * T : nullptr;
  char* img = smem + w * 8192;

  f32x16 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  if (kv_end == 0) {  // workgroup-uniform: no row of this sequence sees a key
    store_tile_rows(img, o, 0.f, orow, ldo, T - t0w, lane);
    if (lrow && t < T && h == 0) lrow[t] = -INFINITY;
    return;
  }
  const int kv_hi = min(past + qt * 64 + 64, kv_end);  // one past the last key any row of the tile sees
  const int nkv = (kv_hi + 63) >> 6;
  const int wave_hi = min(past + t0w + 32, kv_end);    // the same for this wave's 32 rows
  const int lim = min(past + t, kv_end - 1);           // keys > lim are masked for this row (lim >= 0)
  const int KD = Hkv * D;
  TileDma<NP> kd, vd;
  // paged: logical page pi of this row -> its descriptors; pages visited hold a visible key, so pi < max_pages
  // The table entry comes by a VECTOR buffer load (every lane the same address; the descriptor covers this row of the
  // table): its arrival is then counted by vmcnt, which the loop waits on for the tile DMA anyway, so a look-ahead
  // fetch needs no wait of its own (a scalar load shares its counter with the LDS reads of the tile in flight).  The
  // value is made uniform by readfirstlane where a descriptor is built from it.
  auto page_no = [&](int pi) -> int {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (PAGED) {
      const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(pg.table + (long)b * pg.max_pages), 0, pg.max_pages * 4, 0x00020000);
      return (int)__builtin_amdgcn_raw_buffer_load_b32(trs, pi * 4, 0, 0);
    }
#endif
    return 0;
  };
  auto set_page = [&](int pi, int page_v) {
    const int page = __builtin_amdgcn_readfirstlane(page_v);
    const bool ok = page >= 0 && page < pg.n_pages;
    const long first = ((long)(ok ? page : 0) * SD_KV_PAGE) * KD + hkv * D;
    const int rows = ok ? min(SD_KV_PAGE, kv_end - SD_KV_PAGE * pi) : 0;
    kd.rebase(Kp + first, rows);
    vd.rebase(Vp + first, rows);
  };
  // ---- 8-bit pages: the tile in flight lives in registers between mx_load and mx_put
  u32x2 kq[MX ? NP : 1], vq[MX ? NP : 1];
  uint32_t ksc[MX ? NP : 1], vsc[MX ? NP : 1];
  long mx_first = 0;  // pool row of the open page's row 0
  int mx_rows = 0;    // rows of the open page that exist: the others are staged as zeros
  auto mx_set_page = [&](int pi, int page_v) {
    const int page = __builtin_amdgcn_readfirstlane(page_v);
    const bool ok = page >= 0 && page < pg.n_pages;
    mx_first = (long)(ok ? page : 0) * SD_KV_PAGE;
    mx_rows = ok ? min(SD_KV_PAGE, kv_end - SD_KV_PAGE * pi) : 0;
  };
  auto mx_load = [&](int row0) {  // rows row0 .. row0 + 63 of the open page
    if constexpr (MX) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int pc = (w * NP + i) * 64 + lane;
        const int row = pc >> 4, ch = (pc & 15) ^ f_swz(row);
        kq[i] = vq[i] = u32x2{0u, 0u};
        ksc[i] = vsc[i] = 0u;
        if (row0 + row < mx_rows) {
          const long pr = mx_first + row0 + row;
          const long od = pr * KD + hkv * D + ch * 8, os = (pr * Hkv + hkv) * 4 + (ch >> 2);
          kq[i] = *(const u32x2*)((const uint8_t*)Kp + od);
          vq[i] = *(const u32x2*)((const uint8_t*)Vp + od);
          ksc[i] = pg.k_scale[os];
          vsc[i] = pg.v_scale[os];
        }
      }
    }
  };
  auto mx_put = [&](char* dst) {  // (K tile, V tile) at dst: the addresses TileDma::issue writes
    if constexpr (MX) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int o16 = ((w * NP + i) * 64 + lane) * 16;
        *(bf16x8*)(dst + o16) = mx_to_bf16x8(kq[i], ksc[i]);
        *(bf16x8*)(dst + TILE + o16) = mx_to_bf16x8(vq[i], vsc[i]);
      }
    }
  };
  int page_nx = 0;  // the page of the NEXT page boundary the stream crosses
  if constexpr (MX) {
    mx_set_page(0, page_no(0));
    if (nkv > TPP) page_nx = page_no(1);
    mx_load(0);
  } else if constexpr (PAGED) {
    kd.init(Kp + hkv * D, KD, 1, w, lane);
    vd.init(Vp + hkv * D, KD, 1, w, lane);
    set_page(0, page_no(0));
    if (nkv > TPP) page_nx = page_no(1);
  } else {
    kd.init(Kp + (long)b * cap * KD + hkv * D, KD, kv_end, w, lane);
    vd.init(Vp + (long)b * cap * KD + hkv * D, KD, kv_end, w, lane);
  }
  if constexpr (!MX) {
    kd.issue(0, smem, w);
    vd.issue(0, smem + TILE, w);
  }
  bf16x8 qf[8];
  {
    const bf16* qp = Q + ((long)b * T + tc) * ldq + hq * D + 8 * h;
#pragma unroll
    for (int st = 0; st < 8; ++st) qf[st] = *(const bf16x8*)(qp + 16 * st);
  }
  float m = NEG, l = 0.f;
  const float c = scale * LOG2E;

  auto tile = [&](int i, int stage) {
    const char* ks = smem + stage * 2 * TILE;
    const char* vs = ks + TILE;
    f32x16 s[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[kh][e] = 0.f;
#pragma unroll
      for (int st = 0; st < 8; ++st) s[kh] = mfma32(row_frag(ks, 32 * kh, st, lane), qf[st], s[kh]);
    }
    const int k0 = i * 64;
    // wave-uniform: the tile touches a diagonal of mine or the end of the keys (computed from ABSOLUTE positions: the
    // diagonal falls mid-tile whenever past % 64 != 0)
    const bool need_mask = __builtin_amdgcn_readfirstlane((int)((k0 + 63 > past + t0w) || (k0 + 63 >= kv_end))) != 0;
    if (need_mask) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int e = 0; e < 16; ++e) s[kh][e] = (k0 + 32 * kh + acc_row(e, h)) > lim ? NEG : s[kh][e];
    }
    float mx = fmaxf(s[0][0], s[1][0]);
#pragma unroll
    for (int e = 1; e < 16; ++e) mx = fmaxf(fmaxf(mx, s[0][e]), s[1][e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * c);
    m = mn;
    const float mnc = -mn * c;
    float rs = 0.f;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kh][e], c, mnc));
        s[kh][e] = p;
        rs += p;
      }
    l = l * alpha + rs;
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
    }
#pragma unroll
    for (int ss = 0; ss < 4; ++ss) {  // 16 keys per step
      bf16x8 vt[4];
      tr_frag4(vs, 16 * ss, lane, vt);
      const bf16x8 pf = acc_frag(s[ss >> 1], ss & 1);
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] = mfma32(vt[db], pf, o[db]);
    }
  };
  if constexpr (MX) {
    for (int i = 0; i < nkv; ++i) {
      // tile i: registers -> ring slot i & 1, last read as tile i - 2, which everybody left before the barrier of i - 1
      mx_put(smem + (i & 1) * 2 * TILE);
      if (i + 1 < nkv) {  // tile i + 1 travels while tile i is computed
        const int pi = (i + 1) / TPP;
        if ((i + 1) % TPP == 0) {  // tile i + 1 opens page pi: its number was fetched when page pi - 1 was opened
          mx_set_page(pi, page_nx);
          if ((pi + 1) * TPP < nkv) page_nx = page_no(pi + 1);
        }
        mx_load(((i + 1) % TPP) * 64);
      }
      __syncthreads();  // everybody's share of tile i is in LDS
      if (i * 64 < wave_hi) tile(i, i & 1);  // wave-uniform
    }
  } else
  for (int i = 0; i < nkv; ++i) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // my share of tile i (and, the first time, my Q rows)
    __builtin_amdgcn_s_barrier();  // everybody's share of tile i has landed; everybody is done reading tile i-1
    asm volatile("" ::: "memory");
    if (i + 1 < nkv) {
      char* nx = smem + ((i + 1) & 1) * 2 * TILE;
      if constexpr (PAGED) {
        const int pi = (i + 1) / TPP;
        if ((i + 1) % TPP == 0) {  // tile i + 1 opens page pi: its number was fetched when page pi - 1 was opened
          set_page(pi, page_nx);
          if ((pi + 1) * TPP < nkv) page_nx = page_no(pi + 1);
        }
        kd.issue(((i + 1) % TPP) * 64, nx, w);
        vd.issue(((i + 1) % TPP) * 64, nx + TILE, w);
      } else {
        kd.issue((i + 1) * 64, nx, w);
        vd.issue((i + 1) * 64, nx + TILE, w);
      }
    }
    if (i * 64 < wave_hi) tile(i, i & 1);  // wave-uniform
  }
  __syncthreads();  // nothing is in flight (the last iteration issued nothing); the ring becomes the store images
  l += __shfl_xor(l, 32, 64);
  store_tile_rows(img, o, 1.f / l, orow, ldo, T - t0w, lane);
  if (lrow && t < T && h == 0) lrow[t] = m * scale + __logf(l);
}
}  // namespace

extern "C" int sd_attn_extend(const void* q, const void* k_plane, const void* v_plane, void* o, float* lse,
                              const int32_t* past, const int32_t* new_len, int64_t ldq, int64_t ldo, int B, int T, int cap,
                              int Hq, int Hkv, int head_dim, float scale, void* stream) {
  if (!q || !k_plane || !v_plane || !o || !past || !new_len) return SD_ERR_SHAPE;
  if (B <= 0 || T <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || head_dim <= 0) return SD_ERR_SHAPE;
  if (head_dim != D) return SD_ERR_UNSUPPORTED;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (ldq < (int64_t)Hq * D || ldo < (int64_t)Hq * D) return SD_ERR_SHAPE;
  if ((ldq | ldo) & 7) return SD_ERR_ALIGN;
  if (((uintptr_t)q | (uintptr_t)k_plane | (uintptr_t)v_plane | (uintptr_t)o) & 15) return SD_ERR_ALIGN;
  // a cache row of one sequence is addressed with 32-bit byte offsets; the grid's y and z are 16-bit
  if ((int64_t)cap * Hkv * D * 2 >= ((int64_t)1 << 31) || T > (1 << 30) || B > 65535 || Hkv > 65535) return SD_ERR_UNSUPPORTED;
  SdProfScope prof(SD_K_ATTN_FWD, 4.0 * B * Hq * (double)T * cap * D, (hipStream_t)stream);  // upper bound: every key
  SD_PROF_LABEL("attn_extend_kernel<%d>", G);
  const dim3 grid((T + 63) / 64, Hkv, B);
#define SD_EXT_GO(G_)                                                                                                \
  hipLaunchKernelGGL((attn_extend_kernel<G_>), grid, dim3(128 * G_), 0, (hipStream_t)stream, (const bf16*)q,         \
                     (const bf16*)k_plane, (const bf16*)v_plane, (bf16*)o, lse, past, new_len, (long)ldq, (long)ldo, T, \
                     cap, Hq, Hkv, scale)
  if (G == 1) SD_EXT_GO(1); else if (G == 2) SD_EXT_GO(2); else SD_EXT_GO(4);
#undef SD_EXT_GO
  SD_CHECK_LAUNCH();
  return 0;
}

// The paged twin (llm_engine.py:91): the twin's checks with cap = max_pages * 256, the same grid.
extern "C" int sd_attn_extend_paged(const void* q, const void* k_pool, const void* v_pool, const int32_t* table,
                                    int max_pages, int n_pages, void* o, float* lse, const int32_t* past,
                                    const int32_t* new_len, int64_t ldq, int64_t ldo, int B, int T, int Hq, int Hkv,
                                    int head_dim, float scale, void* stream) {
  if (!q || !k_pool || !v_pool || !o || !past || !new_len || !table) return SD_ERR_SHAPE;
  if (B <= 0 || T <= 0 || max_pages <= 0 || n_pages <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || head_dim <= 0)
    return SD_ERR_SHAPE;
  if (head_dim != D) return SD_ERR_UNSUPPORTED;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (ldq < (int64_t)Hq * D || ldo < (int64_t)Hq * D) return SD_ERR_SHAPE;
  if ((ldq | ldo) & 7) return SD_ERR_ALIGN;
  if (((uintptr_t)q | (uintptr_t)k_pool | (uintptr_t)v_pool | (uintptr_t)o) & 15) return SD_ERR_ALIGN;
  // a PAGE is addressed with 32-bit byte offsets; cap = max_pages * 256 must fit an int; the grid's y and z are 16-bit
  if ((int64_t)SD_KV_PAGE * Hkv * D * 2 >= ((int64_t)1 << 31) || max_pages > (1 << 22) || T > (1 << 30) || B > 65535 ||
      Hkv > 65535)
    return SD_ERR_UNSUPPORTED;
  const int cap = max_pages * SD_KV_PAGE;
  SdProfScope prof(SD_K_ATTN_FWD, 4.0 * B * Hq * (double)T * cap * D, (hipStream_t)stream);  // upper bound: every key
  SD_PROF_LABEL("attn_extend_kernel<%d, paged>", G);
  const dim3 grid((T + 63) / 64, Hkv, B);
#define SD_EXT_GO(G_)                                                                                                  \
  hipLaunchKernelGGL((attn_extend_kernel<G_, const int*, int, int>), grid, dim3(128 * G_), 0, (hipStream_t)stream,     \
                     (const bf16*)q, (const bf16*)k_pool, (const bf16*)v_pool, (bf16*)o, lse, past, new_len, (long)ldq, \
                     (long)ldo, T, cap, Hq, Hkv, scale, (const int*)table, max_pages, n_pages)
  if (G == 1) SD_EXT_GO(1); else if (G == 2) SD_EXT_GO(2); else SD_EXT_GO(4);
#undef SD_EXT_GO
  SD_CHECK_LAUNCH();
  return 0;
}

// The 8-bit twin: sd_attn_extend_paged's checks and grid; K / V arrive as e4m3 planes with their E8M0 scale planes.
extern "C" int sd_attn_extend_paged_mx(const void* q, const void* k_data, const void* k_scale, const void* v_data,
                                       const void* v_scale, const int32_t* table, int max_pages, int n_pages, void* o,
                                       float* lse, const int32_t* past, const int32_t* new_len, int64_t ldq, int64_t ldo,
                                       int B, int T, int Hq, int Hkv, int head_dim, float scale, void* stream) {
  if (!q || !k_data || !k_scale || !v_data || !v_scale || !o || !past || !new_len || !table) return SD_ERR_SHAPE;
  if (B <= 0 || T <= 0 || max_pages <= 0 || n_pages <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || head_dim <= 0)
    return SD_ERR_SHAPE;
  if (head_dim != D) return SD_ERR_UNSUPPORTED;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4) return SD_ERR_UNSUPPORTED;
  if (ldq < (int64_t)Hq * D || ldo < (int64_t)Hq * D) return SD_ERR_SHAPE;
  if ((ldq | ldo) & 7) return SD_ERR_ALIGN;
  if (((uintptr_t)q | (uintptr_t)k_data | (uintptr_t)v_data | (uintptr_t)o) & 15) return SD_ERR_ALIGN;
  if (((uintptr_t)k_scale | (uintptr_t)v_scale) & 3) return SD_ERR_ALIGN;
  if ((int64_t)SD_KV_PAGE * Hkv * D * 2 >= ((int64_t)1 << 31) || max_pages > (1 << 22) || T > (1 << 30) || B > 65535 ||
      Hkv > 65535)
    return SD_ERR_UNSUPPORTED;
  const int cap = max_pages * SD_KV_PAGE;
  SdProfScope prof(SD_K_ATTN_FWD, 4.0 * B * Hq * (double)T * cap * D, (hipStream_t)stream);  // upper bound: every key
  SD_PROF_LABEL("attn_extend_kernel<%d, paged, mx>", G);
  const dim3 grid((T + 63) / 64, Hkv, B);
#define SD_EXT_GO(G_)                                                                                                   \
  hipLaunchKernelGGL((attn_extend_kernel<G_, const int*, int, int, const uint8_t*, const uint8_t*>), grid,              \
                     dim3(128 * G_), 0, (hipStream_t)stream, (const bf16*)q, (const bf16*)k_data, (const bf16*)v_data,  \
                     (bf16*)o, lse, past, new_len, (long)ldq, (long)ldo, T, cap, Hq, Hkv, scale, (const int*)table,     \
                     max_pages, n_pages, (const uint8_t*)k_scale, (const uint8_t*)v_scale)
  if (G == 1) SD_EXT_GO(1); else if (G == 2) SD_EXT_GO(2); else SD_EXT_GO(4);
#undef SD_EXT_GO
  SD_CHECK_LAUNCH();
  return 0;
}
