"""Windows, guards, references and the case list of tests/test_gpu_gemm_views.py (the ADDRESSING of csrc/sd_gemm.hip:
leading dimensions, write bounds, K tails, non-finite neighbours).

TEST INFRASTRUCTURE ONLY, CPU only (never imported by the product, no GPU in it).  tests/test_gemm_ref_cpu.py shows on the
CPU that every probe accepts a correct GEMM, that each named addressing fault is caught by the probe meant for it, and --
through `_lib.gemm_plan`, which needs no GPU -- that every entry of FAMILIES reaches the kernel it is named for, with
contiguous operands and with windows alike.

A window is a rows x cols view of a larger, filled parent (guard rows above and below, a gap of ld - cols elements between
rows); ld % 8 == 0 and col0 % 8 == 0 keep every row 16-byte aligned, which is all the C ABI asks of a view.
  inputs:  LOUD  finite, |x| = 3e4 with alternating sign: a gap element that meets a non-zero partner is unmistakable
           NAN   bf16 bits 0x7FC0;  INF  +infinity: a gap element that meets a ZERO partner still shows (0 * x is NaN)
  outputs: SENTINEL, a NaN payload no kernel produces (bf16 bits 0x7FA5, fp32 bits 0x7FA5A5A5), compared as bits
"""
from __future__ import annotations

import torch

from parity_ref import half_ulp

BF = torch.bfloat16
LOUD, NAN, INF, SENTINEL = "loud", "nan", "inf", "sentinel"
SENTINEL_BITS = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5}
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
PAD, COL0, GUARD = 24, 8, 2  # the windows of the GPU tests: ld = natural + 24, first column 8, two guard rows


def filled(shape, fill, dtype=BF):
    n = 1
    for s in shape:
        n *= s
    if fill == LOUD:
        sign = 1.0 - 2.0 * (torch.arange(n) % 2).float()
        return (3e4 * sign).to(dtype).reshape(shape)
    if fill == INF:
        return torch.full(shape, float("inf"), dtype=dtype)
    bits = {NAN: 0x7FC0 if dtype == BF else 0x7FC00000, SENTINEL: SENTINEL_BITS[dtype]}[fill]
    return torch.full(shape, bits, dtype=_INT[dtype]).view(dtype)


def view_of(parent, rows, cols, col0, guard_rows):
    return parent[guard_rows:guard_rows + rows, col0:col0 + cols]


def window(rows, cols, ld, col0, guard_rows, fill, dtype=BF):
    """-> (parent [rows + 2 * guard_rows, ld] holding `fill`, view = parent[guard_rows:guard_rows + rows, col0:col0 + cols])"""
    assert ld % 8 == 0 and col0 % 8 == 0 and col0 + cols <= ld, (cols, ld, col0)
    parent = filled((rows + 2 * guard_rows, ld), fill, dtype)
    return parent, view_of(parent, rows, cols, col0, guard_rows)


def bits(t):
    return t.contiguous().view(_INT[t.dtype])


def outside_untouched(parent_before, parent_after, guard_rows, rows, col0, cols):
    """None when every element of the parent OUTSIDE the window holds the bits it held before, else the first changed
    (row, column) of the parent."""
    changed = bits(parent_before.cpu()) != bits(parent_after.cpu())
    changed[guard_rows:guard_rows + rows, col0:col0 + cols] = False
    if not bool(changed.any()):
        return None
    return tuple(int(v) for v in changed.nonzero()[0])


def first_diff(got, want):
    """None when two tensors hold the same bits, else the first differing coordinate"""
    d = bits(got.cpu()) != bits(want.cpu())
    return tuple(int(v) for v in d.nonzero()[0]) if bool(d.any()) else None


def ref64(a, b, ta, tb, r=None):
    """C = op(a) op(b) (+ r) in fp64; ta: a is stored [K][M]; tb False: b is stored [N][K] (sd_gemm_bf16's layouts)"""
    A = a.double().T if ta else a.double()
    B = b.double() if tb else b.double().T
    c = A @ B
    return c if r is None else c + r.double()


def int_expect(a, b, ta, tb, r=None):
    """the one right answer for integer data in [-4, 4]: |sum| <= 16 K + 4 is exact in fp32, then one rounding to bf16.
    A sum that is zero is +0: the accumulator starts at +0 and (+0) + (-0) = +0, while a bare product 0 * -3 (all there is
    at K = 1) is -0."""
    return (ref64(a, b, ta, tb, r) + 0.0).float().bfloat16()


def elem_bound(a, b, ta, tb, r, K):
    """Per-element bound for random data: d = 2 K 2^-24 (|A| |B| + |R|) is the worst fp32 accumulation error of ANY
    summation order (the factor 2: slab sums and the residual add), half_ulp(|ref| + d) one correct rounding of whatever
    fp32 value lies within d of the reference.  Sharp while d is well under half an ulp: K <= 200."""
    d = 2.0 * K * 2.0 ** -24 * ref64(a.abs(), b.abs(), ta, tb, None if r is None else r.abs())
    ref = ref64(a, b, ta, tb, r)
    return half_ulp(ref.abs() + d, BF) + d


def worst_ratio(got, a, b, ta, tb, r, K):
    """max over elements of |got - ref| / elem_bound (<= 1 passes)"""
    err = (got.double().cpu() - ref64(a, b, ta, tb, r)).abs()
    return float((err / elem_bound(a, b, ta, tb, r, K)).max())


def int_operands(M, N, K, ta, tb, res, seed):
    """integers in [-3, 3] (bf16-exact), row 0 of each stored operand raised by one (asymmetric: a transposition or a
    swapped operand shows)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (K, M) if ta else (M, K), generator=g).float()
    b = torch.randint(-3, 4, (K, N) if tb else (N, K), generator=g).float()
    a[0, :] += 1.0
    b[0, :] += 1.0
    r = torch.randint(-3, 4, (M, N), generator=g).float().to(BF) if res else None
    return a.to(BF), b.to(BF), r


# ------------------------------------------------------------------------------------------------ the case list
LAYOUTS = {"nt": (False, False), "nn": (False, True), "tn": (True, True), "ta": (True, False)}
VARIANTS = [(64, 2), (64, 3), (64, 4), (128, 2), (128, 3), (128, 4), (256, 2), (256, 3)]  # gemm_bf16_kernel's tiles
STAG = {"gemm.force_bm": 256, "gemm.force_nst": 9}


def _b(x):
    return "true" if x else "false"


def desc_staging_sound(ta, tb, K):
    """The contract (include/sd_hip.h, sd_gemm_bf16), not the dispatch code: buffer-descriptor staging zero-fills k >= K
    only for a transposed operand; a K-contiguous one reads on into the gap or the next row, so it needs K % 64 == 0."""
    return (ta and tb) or K % 64 == 0


def tail_k(lay, k_tail, k_whole):
    """the K at which a layout still takes descriptor staging: with a tail for TN, a whole number of K tiles otherwise"""
    return k_tail if lay == "tn" else k_whole


def bf16_symbol(bm, nst, ta, tb, epi, fast):
    return f"gemm_bf16_kernel<{bm}, {nst}, {_b(ta)}, {_b(tb)}, {epi}, {_b(fast)}>"


def force(bm, nst, checked=False):
    return {"gemm.force_bm": bm, "gemm.force_nst": nst, "gemm.checked_staging": int(checked)}


def _families():
    fam = []

    def add(name, entry, shape, lay, symbol, switches, res=False, **kw):
        ta, tb = LAYOUTS[lay]
        fam.append(dict(name=name, entry=entry, shape=shape, layout=lay, ta=ta, tb=tb, res=res, switches=dict(switches),
                        symbol=symbol, **kw))

    for lay, (ta, tb) in LAYOUTS.items():
        for bm, nst in VARIANTS:
            # descriptor staging: K = 200 (a K tail) where both operands are transposed, else 192; pointer staging at K = 200
            add(f"bf16_{bm}x{nst}_{lay}_desc", "gemm", (520, 264, tail_k(lay, 200, 192)), lay,
                bf16_symbol(bm, nst, ta, tb, 0, True), force(bm, nst))
            add(f"bf16_{bm}x{nst}_{lay}_checked", "gemm", (520, 264, 200), lay, bf16_symbol(bm, nst, ta, tb, 0, False),
                force(bm, nst, True))
        for res in (False, True):
            add(f"stag_{lay}_r{int(res)}", "gemm", (520, 264, tail_k(lay, 200, 192)), lay,
                f"gemm_stag_kernel<{_b(ta)}, {_b(tb)}, {int(res)}>", STAG, res=res)
        # more 256 x 128 tiles than CUs (4 x 84): the persistent kernel
        add(f"pstag_{lay}", "gemm", (1000, 128 * 83 + 40, tail_k(lay, 72, 64)), lay,
            f"gemm_pstag_kernel<4, {_b(ta)}, {_b(tb)}, 0>", {**STAG, "gemm.no_p256": 1})
    p256 = (1000, 256 * 60 + 40, 64)  # 4 x 61 tiles of 256 x 256
    add("p256_paired", "gemm", p256, "nt", "gemm_p256_kernel<0, true>", {"gemm.p256_min_tiles": 150})
    add("p256_unpaired", "gemm", p256, "nt", "gemm_p256_kernel<0, false>", {"gemm.p256_min_tiles": 150, "gemm.p256_unpaired": 1})
    add("splitk", "splitk", (256, 1024, 6144), "nn", "gemm_stag_kernel<false, true, 2>", {})
    add("splitk_partial", "splitk_partial", (256, 1024, 6144), "nn", "gemm_stag_kernel<false, true, 2>", {})
    for acc in (False, True):
        add(f"grouped_tn_acc{int(acc)}", "grouped", None, "tn", f"gemm_pgroup_tn_kernel<{_b(acc)}>", {}, accumulate=acc,
            problems=GROUPED_PROBLEMS)
    # the fused epilogues (their leading dimensions are fixed by the entry point): dims -> the plan query of the entry
    sw = dict(M=150, K=256, I=192)
    for tag, switches, sym in (("h", {}, bf16_symbol(64, 4, False, False, 3, True)),
                               ("64x4", force(64, 4), bf16_symbol(64, 4, False, False, 3, True)),
                               ("128x3", force(128, 3), bf16_symbol(128, 3, False, False, 3, True)),
                               ("stag", STAG, "gemm_stag_kernel<false, false, 3>")):
        add(f"swiglu_{tag}", "swiglu", (150, 384, 256), "nt", sym, switches, dims=sw, plan=dict(epi_kind=3, epi_I=192))
    big = dict(M=1100, K=192, I=5760)  # 5 x 45 tiles of 256 x 256; 5 x 90 of 256 x 128
    add("swiglu_p256", "swiglu", (1100, 11520, 192), "nt", "gemm_p256_kernel<3, true>", {"gemm.p256_min_tiles": 150}, dims=big,
        plan=dict(epi_kind=3, epi_I=5760))
    add("swiglu_pstag", "swiglu", (1100, 11520, 192), "nt", "gemm_pstag_kernel<4, false, false, 3>", {"gemm.no_p256": 1},
        dims=big, plan=dict(epi_kind=3, epi_I=5760))
    qk = dict(M=150, T=50, K=256, Hq=4, Hkv=2)
    for tag, switches, sym in (("h", {}, bf16_symbol(64, 4, False, False, 4, True)),
                               ("128x3", force(128, 3), bf16_symbol(128, 3, False, False, 4, True)),
                               ("stag", STAG, "gemm_stag_kernel<false, false, 4>")):
        add(f"qkv_rope_{tag}", "qkv_rope", (150, 1024, 256), "nt", sym, switches, dims=qk, plan=dict(epi_kind=4))
    sb = dict(M=300, H=256, I=520)
    for tag, switches, sym in (("h", {}, bf16_symbol(64, 3, False, True, 5, True)),
                               ("128x2", force(128, 2), bf16_symbol(128, 2, False, True, 5, True)),
                               ("128x3", force(128, 3), bf16_symbol(128, 3, False, True, 5, True)),
                               ("stag", STAG, "gemm_stag_kernel<false, true, 5>")):
        add(f"swiglu_bwd_{tag}", "swiglu_bwd", (300, 520, 256), "nn", sym, switches, dims=sb, plan=dict(epi_kind=5))
    od = dict(M=300, T=100, Hq=2, H=256)
    for tag, switches, sym in (("h", {}, bf16_symbol(64, 3, False, True, 6, True)),
                               ("128x2", force(128, 2), bf16_symbol(128, 2, False, True, 6, True)),
                               ("stag", STAG, "gemm_stag_kernel<false, true, 6>")):
        add(f"odx_delta_{tag}", "odx_delta", (300, 256, 256), "nn", sym, switches, dims=od, plan=dict(epi_kind=6))
    sq = dict(M=150, N=512, K=256)
    for tag, switches, sym in (("h", {}, bf16_symbol(64, 4, False, False, 1, True)),
                               ("128x3", force(128, 3), bf16_symbol(128, 3, False, False, 1, True)),
                               ("stag", STAG, "gemm_stag_kernel<false, false, 1>")):
        add(f"ssq_{tag}", "ssq", (150, 512, 256), "nt", sym, switches, res=True, dims=sq, plan={})
    return fam


GROUPED_PROBLEMS = [(520, 1000), (264, 2048), (1032, 264), (8, 136)]  # (M, N) of C = A^T B, common K
FAMILIES = _families()
BY_NAME = {f["name"]: f for f in FAMILIES}
assert len(BY_NAME) == len(FAMILIES)


def plan_query(f, windowed):
    """keyword arguments of `_lib.gemm_plan` for a FAMILIES entry that goes through gemm_plan (every one but the grouped
    kernel); windowed: the leading dimensions of the GPU tests' windows instead of contiguous operands"""
    M, N, K = f["shape"]
    q = dict(M=M, N=N, K=K, trans_a=f["ta"], trans_b=f["tb"], residual=f["res"],
             split_k=f["entry"] in ("splitk", "splitk_partial"), **f.get("plan", {}))
    if windowed and f["entry"] in ("gemm", "splitk", "splitk_partial"):
        q.update(lda=(M if f["ta"] else K) + PAD, ldb=(N if f["tb"] else K) + PAD, ldc=N + PAD)
    return q
