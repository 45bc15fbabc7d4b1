"""CPU only: the probes of tests/gemm_ref.py (used by tests/test_gpu_gemm_views.py) accept a correct GEMM that writes
into a window, each seeded addressing fault fails the probe meant for it, `elem_bound` accepts the fp32 reference and
rejects one element moved by 1.5 half-ulps, and every FAMILIES entry reaches the kernel it names (through `_lib.gemm_plan`,
which launches nothing) with windowed leading dimensions as with contiguous ones."""
import random

import pytest
import torch

import gemm_ref as G
from gemm_ref import BF, GUARD, COL0, PAD, LOUD, NAN, INF, SENTINEL
from speech_distill_amd import _lib

M, N, K = 40, 24, 72  # one K tile and a tail of 8


def place(x, fill):
    rows, cols = x.shape
    parent, view = G.window(rows, cols, cols + PAD, COL0, GUARD, fill)
    view.copy_(x)
    return parent, view


def emulate(ta, tb, fill=LOUD, fault=None, res=False):
    """A torch GEMM over windows, as the GPU tests run the kernels: -> (C parent before, C parent after, expected window).
    fault: one of the addressing mistakes the probes exist for."""
    a, b, r = G.int_operands(M, N, K, ta, tb, res, seed=3)
    (pa, va), (pb, vb) = place(a, fill), place(b, fill)
    pc, vc = G.window(M, N, N + PAD, COL0, GUARD, SENTINEL)
    if res:
        vc.copy_(r)
    before = pc.clone()
    want = G.int_expect(a, b, ta, tb, r)
    rr = vc.clone() if res else None
    if fault == "natural_ld":  # the natural row length instead of the given leading dimension, for A
        va = torch.as_strided(pa, va.shape, (va.shape[1], 1), va.storage_offset())
    if fault == "drop_k_tail":
        k = K - K % 64
        va, vb = (va[:k] if ta else va[:, :k]), (vb[:k] if tb else vb[:, :k])
    if fault == "zero_partner":  # descriptor staging of a K-contiguous operand: k in [K, 64 ceil(K / 64)) read from the parent
        k64 = -(-K // 64) * 64
        assert not ta or not tb
        if not ta:
            va = torch.as_strided(pa, (M, k64), (pa.shape[1], 1), va.storage_offset())
        else:
            va = torch.cat([va, torch.zeros(k64 - K, M, dtype=BF)])
        if not tb:
            vb = torch.as_strided(pb, (N, k64), (pb.shape[1], 1), vb.storage_offset())
        else:
            vb = torch.cat([vb, torch.zeros(k64 - K, N, dtype=BF)])
        if not ta and not tb:  # two K-contiguous operands: the partner of A's tail is zero, as the partner of B's
            vb = vb.clone()
            vb[:, K:] = 0
    A = va.float().T if ta else va.float()
    B = vb.float() if tb else vb.float().T
    c = A @ B  # fp32: 0 * NaN is NaN, as in the MFMA
    c = (c if rr is None else c + rr.float()).bfloat16()
    if fault == "past_n":
        pc[GUARD:GUARD + M, COL0:COL0 + N + 8] = torch.cat([c, torch.zeros(M, 8, dtype=BF)], 1)
    else:
        vc.copy_(c)
    if fault == "guard_row":
        pc[GUARD + M, COL0:COL0 + N] = 0
    if fault == "unwritten":
        vc[M - 1, N - 1] = before[GUARD + M - 1, COL0 + N - 1]
    return before, pc, want


def probes(before, after, want):
    """what the GPU tests assert: (first wrong element of the window, first changed element outside it)"""
    return G.first_diff(G.view_of(after, M, N, COL0, GUARD), want), G.outside_untouched(before, after, GUARD, M, COL0, N)


@pytest.mark.parametrize("lay", list(G.LAYOUTS))
@pytest.mark.parametrize("fill", [LOUD, NAN, INF])
@pytest.mark.parametrize("res", [False, True])
def test_fault_free_emulator_passes_every_probe(lay, fill, res):
    assert probes(*emulate(*G.LAYOUTS[lay], fill=fill, res=res)) == (None, None)


def test_each_seeded_fault_fails_its_probe():
    for lay, (ta, tb) in G.LAYOUTS.items():
        wrong, outside = probes(*emulate(ta, tb, fault="past_n"))
        assert wrong is None and outside == (GUARD, COL0 + N), lay
        wrong, outside = probes(*emulate(ta, tb, fault="guard_row"))
        assert wrong is None and outside == (GUARD + M, COL0), lay
        wrong, outside = probes(*emulate(ta, tb, fault="natural_ld"))
        assert wrong is not None and outside is None, lay
        wrong, outside = probes(*emulate(ta, tb, fault="drop_k_tail"))
        assert wrong is not None and outside is None, lay
        wrong, outside = probes(*emulate(ta, tb, fault="unwritten"))
        assert wrong == (M - 1, N - 1) and outside is None, lay
        wrong, outside = probes(*emulate(ta, tb, fault="unwritten", res=True))  # accumulate form: the old value stays
        assert wrong == (M - 1, N - 1) and outside is None, lay


@pytest.mark.parametrize("lay", ["nt", "nn", "ta"])
def test_zero_partner_fault_needs_the_non_finite_fills(lay):
    """The hazard of descriptor staging with a K-contiguous operand and a K tail: finite garbage times zero passes every
    probe (which is why LOUD windows alone do not find it), a NaN or Inf gap does not."""
    ta, tb = G.LAYOUTS[lay]
    assert probes(*emulate(ta, tb, fill=LOUD, fault="zero_partner")) == (None, None)
    for fill in (NAN, INF):
        wrong, outside = probes(*emulate(ta, tb, fill=fill, fault="zero_partner"))
        assert wrong is not None and outside is None, (lay, fill)


def test_window_geometry_and_fills():
    parent, view = G.window(5, 16, 40, 8, 2, LOUD)
    assert parent.shape == (9, 40) and view.shape == (5, 16) and view.stride() == (40, 1)
    assert view.data_ptr() % 16 == 0 and view.data_ptr() - parent.data_ptr() == (2 * 40 + 8) * 2
    assert float(parent.float().abs().min()) > 2.9e4 and float(parent.float().sum()) == 0.0
    assert bool(G.filled((3, 8), NAN).isnan().all()) and bool(G.filled((3, 8), INF).isinf().all())
    for dt, width in ((torch.bfloat16, 0xFFFF), (torch.float32, 0xFFFFFFFF)):
        s = G.filled((2, 8), SENTINEL, dt)
        assert bool(s.isnan().all()) and int(G.bits(s)[0, 0]) & width == G.SENTINEL_BITS[dt]
    # a result, finite or not, never carries the sentinel's payload: the canonical NaN and Inf differ from it
    assert G.first_diff(G.filled((2, 8), SENTINEL), G.filled((2, 8), NAN)) == (0, 0)
    with pytest.raises(AssertionError):
        G.window(5, 16, 36, 8, 2, LOUD)
    # outside_untouched sees a single changed bit, in a guard row and in the gap, and ignores the window
    after = parent.clone()
    after[2:7, 8:24] = 1.0
    assert G.outside_untouched(parent, after, 2, 5, 8, 16) is None
    after[3, 24] = -after[3, 24]
    assert G.outside_untouched(parent, after, 2, 5, 8, 16) == (3, 24)
    after[0, 39] = 0
    assert G.outside_untouched(parent, after, 2, 5, 8, 16) == (0, 39)


def test_int_expect_is_exact_and_rounds_once():
    a, b, r = G.int_operands(200, 136, 515, True, True, True, seed=1)
    assert float(a.float().abs().max()) <= 4 and float(a[0].float().sum()) != float(a[1].float().sum())
    c64 = G.ref64(a, b, True, True, r)
    assert torch.equal(c64, c64.round()) and float(c64.abs().max()) > 256  # integers, some above bf16's exact range
    assert torch.equal(G.int_expect(a, b, True, True, r).double(), c64.float().bfloat16().double())
    assert torch.equal((a.float().T @ b.float() + r.float()).double(), c64)  # and exact in fp32, whatever the order
    # K = 1: a bare product 0 * -3 is -0, an accumulator that starts at +0 gives +0: the expectation holds no -0
    a1, b1, _ = G.int_operands(64, 64, 1, True, True, False, seed=1)
    assert bool(torch.signbit(G.ref64(a1, b1, True, True)[G.ref64(a1, b1, True, True) == 0]).any())
    e1 = G.int_expect(a1, b1, True, True)
    assert not bool(torch.signbit(e1[e1 == 0]).any())


@pytest.mark.parametrize("shape,res", [((200, 136, 72), False), ((520, 264, 200), True), ((64, 128, 8), False)])
def test_elem_bound_accepts_fp32_and_rejects_one_and_a_half_half_ulps(shape, res):
    Mm, Nn, Kk = shape
    g = torch.Generator().manual_seed(Kk)
    a, b = torch.randn(Mm, Kk, generator=g).to(BF), torch.randn(Kk, Nn, generator=g).to(BF)
    r = (torch.randn(Mm, Nn, generator=g) * 8).to(BF) if res else None
    c32 = a.float() @ b.float()
    got = (c32 if r is None else c32 + r.float()).bfloat16()
    assert G.worst_ratio(got, a, b, False, True, r, Kk) <= 1.0
    ref = G.ref64(a, b, False, True, r)
    i = tuple(int(v) for v in (ref.abs() == ref.abs().max()).nonzero()[0])
    bad = ref.clone()
    bad[i] += 1.5 * float(G.half_ulp(ref, BF)[i])
    assert G.worst_ratio(ref, a, b, False, True, r, Kk) == 0.0 and G.worst_ratio(bad, a, b, False, True, r, Kk) > 1.0


# ------------------------------------------------------------------------------------------------- the dispatch
@pytest.fixture()
def default_switches():
    _lib.debug_set("reset", 0)
    yield
    _lib.debug_set("reset", 0)


def test_every_family_names_its_kernel_windowed_as_contiguous(default_switches):
    planned = [f for f in G.FAMILIES if f["entry"] != "grouped"]
    for f in planned:
        _lib.debug_set("reset", 0)
        for k, v in f["switches"].items():
            _lib.debug_set(k, v)
        for windowed in (False, True):
            assert _lib.gemm_plan(**G.plan_query(f, windowed))["symbol"] == f["symbol"], (f["name"], windowed)
    # every kernel family of the table, in every layout it supports
    syms = {f["symbol"] for f in G.FAMILIES}
    for ta in ("false", "true"):
        for tb in ("false", "true"):
            for bm, nst in G.VARIANTS:
                assert {f"gemm_bf16_kernel<{bm}, {nst}, {ta}, {tb}, 0, {fast}>" for fast in ("true", "false")} <= syms
            assert {f"gemm_stag_kernel<{ta}, {tb}, {e}>" for e in (0, 1)} | {f"gemm_pstag_kernel<4, {ta}, {tb}, 0>"} <= syms
    assert {"gemm_p256_kernel<0, true>", "gemm_p256_kernel<0, false>", "gemm_p256_kernel<3, true>",
            "gemm_pstag_kernel<4, false, false, 3>", "gemm_stag_kernel<false, true, 2>", "gemm_pgroup_tn_kernel<false>",
            "gemm_pgroup_tn_kernel<true>"} <= syms
    assert {f"gemm_stag_kernel<false, {'true' if e >= 5 else 'false'}, {e}>" for e in (3, 4, 5, 6)} <= syms


def test_descriptor_staging_only_where_it_zero_fills(default_switches):
    """include/sd_hip.h: bytes between rows are never interpreted.  Buffer-descriptor staging reads a K-contiguous operand
    on past K up to the end of the K tile, so the plan may take it only when both operands are transposed or K % 64 == 0;
    a fused epilogue, which has no pointer form, is refused instead (the callers run the two-kernel form)."""
    rnd = random.Random(11)
    n_desc = n_ptr = n_refused = 0
    for _ in range(4000):
        Mm, Nn, Kk = (8 * rnd.randint(1, 600) for _ in range(3))
        lay = rnd.choice(list(G.LAYOUTS))
        ta, tb = G.LAYOUTS[lay]
        epi = 0 if ta else rnd.choice([0, 0, 5, 6] if tb else [0, 0, 3, 4])
        _lib.debug_set("reset", 0)
        if rnd.random() < 0.5:
            bm, nst = rnd.choice(G.VARIANTS + [(256, 9)])
            _lib.debug_set("gemm.force_bm", bm)
            _lib.debug_set("gemm.force_nst", nst)
        q = dict(trans_a=ta, trans_b=tb, epi_kind=epi, epi_I=Nn // 2 if epi == 3 else 0, residual=epi == 0 and rnd.random() < 0.3,
                 split_k=epi == 0 and rnd.random() < 0.2)
        sound = G.desc_staging_sound(ta, tb, Kk)
        try:
            sym = _lib.gemm_plan(Mm, Nn, Kk, **q)["symbol"]
        except _lib.SdHipError:
            assert epi >= 3 and not sound, (Mm, Nn, Kk, q)
            n_refused += 1
            continue
        desc = not sym.endswith("false>") if sym.startswith("gemm_bf16_kernel") else True  # every other kernel: descriptors only
        assert desc == sound, (Mm, Nn, Kk, q, sym)
        n_desc, n_ptr = n_desc + desc, n_ptr + (not desc)
    assert min(n_desc, n_ptr, n_refused) > 100
