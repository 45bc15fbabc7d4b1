"""-m gpu tests of the three MXFP8 teacher kernels of csrc/sd_mx.hip -- sd_mxfp8_quant, sd_gemm_mxfp8 and
sd_gemm_mxfp8_swiglu (include/sd_hip.h "MXFP8 frozen teacher") -- at the edges of the number format and of the tile.

Every assertion is exact: torch.equal on bytes, == on dequantised values (so that -0 equals +0), and the 1e-6 relative bound
of tests/test_gpu_mx.py for rstd.  Every reference is CPU torch (fp32 where the sum is exact in fp32, else fp64) or
tests/mx_ref.py, never a kernel.  The data come from mx_ref and are checked on the CPU by tests/test_mx_cpu.py:
  A  the quantiser on deterministic edge blocks (ratio sweep, every finite bf16 pattern, fixed blocks), views, write bounds;
  B  the GEMM on one-hot probes: the whole e4m3 code table, scale bytes 0..254, every k position -- on either operand;
  C  the GEMM on exact integers at nk = K / 128 around both ring depths (NST = 4 at BM = 128, 3 at BM = 256), tile asserted;
  D  out= / residual views, write bounds, R aliasing C, a row scale that is no power of two;
  E  the SwiGLU epilogue against arithmetic: data whose act is exact whatever the exp;
  F  the refusal codes of the three entries."""
import pytest
import torch

import mx_ref
from gpu_util import dev, to_dev

pytestmark = pytest.mark.gpu

PLAIN128, PLAIN256 = "gemm_mx_kernel<0, 128, 4>", "gemm_mx_kernel<0, 256, 3>"
SWIGLU128, SWIGLU256 = "gemm_mx_kernel<1, 128, 4>", "gemm_mx_kernel<1, 256, 3>"
NAN16 = 0x7FC1       # a bf16 NaN pattern: gaps and guards, never read
GUARD8 = 0xA5


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


@pytest.fixture(scope="module")
def lib(ops):
    return ops.load_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _profiled(ops, fn):
    """fn() under the launch profile -> (its result, {gemm_mx_kernel symbol: launches})."""
    ops.prof_begin()
    try:
        out = fn()
    finally:
        ops.prof_end()
    return out, {k: v[2] for k, v in ops.prof_symbols().items() if k.startswith("gemm_mx_kernel")}


def _same(got, want):
    """== on every element (NaN equals nothing, -0 equals +0)."""
    bad = ~(got.cpu().double() == want.cpu().double())
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


def _nan_arena(rows, cols):
    return torch.full((rows, cols), NAN16, dtype=torch.int16, device=dev())


# ------------------------------------------------------------------------------------------------ A: the quantiser
@pytest.fixture(scope="module")
def edge():
    """The edge matrix [217, 512] and its reference image (computed once, left unchanged)."""
    x = mx_ref.edge_matrix(4)
    q, s = mx_ref.mx_quant(x.float())
    return x, s, mx_ref.mx_deq(q, s)


def test_quant_edge_blocks_equal_the_reference_rule(ops, edge):
    """Ratio sweep (every bf16 mantissa at every exponent below 23 block maxima from the smallest subnormal to the top
    exponent: all ties, the saturating band, e4m3 subnormals, flush to zero, scale byte 0), all 65,280 finite bf16 patterns
    and the fixed blocks: scale bytes and every dequantised element equal mx_ref; the same bytes without rstd and from a
    strided view whose gap columns hold NaN patterns.  rstd against fp64 to 1e-6 on the rows whose sum of squares lies in
    [2^-100, 2^100]."""
    x, ref_s, ref_d = edge
    M, K = x.shape
    xd = to_dev(x)
    q, s, rstd = ops.mxfp8_quant(xd, want_rstd=True, eps=1e-6)
    assert torch.equal(s.cpu(), ref_s), f"{int((s.cpu() != ref_s).sum())} scale bytes differ"
    _same(mx_ref.mx_deq(q.cpu(), s.cpu()), ref_d)
    q2, s2 = ops.mxfp8_quant(xd)
    assert torch.equal(q2, q) and torch.equal(s2, s)
    big = _nan_arena(M, K + 264).view(torch.bfloat16)
    big[:, 128:128 + K] = xd
    for want_rstd in (False, True):
        got = ops.mxfp8_quant(big[:, 128:128 + K], want_rstd=want_rstd, eps=1e-6)
        assert torch.equal(got[0], q) and torch.equal(got[1], s)
        if want_rstd:
            assert torch.equal(got[2].view(torch.int32), rstd.view(torch.int32))
    ss = x.double().pow(2).sum(-1)
    ok = (ss >= 2.0 ** -100) & (ss <= 2.0 ** 100)
    assert bool(ok[1]) and bool(ok[2]) and int(ok.sum()) >= M // 4  # the fixed rows and the middle of both block lists
    ref_rstd = torch.rsqrt(ss / K + 1e-6)
    rel = ((rstd.cpu().double() - ref_rstd).abs() / ref_rstd)[ok]
    print(f"rstd: {int(ok.sum())} of {M} rows in range, worst relative error {float(rel.max()):.3e}")
    assert float(rel.max()) <= 1e-6


@pytest.mark.parametrize("M", [1, 5, 7])
def test_quant_writes_nothing_outside_its_outputs(ops, lib, edge, M):
    """q, scale and rstd are windows inside guard-filled arenas, M % 4 != 0 (the last workgroup has idle waves): the windows
    hold the reference image, every byte around them is unchanged.  The rows include all-zero rows, the +-448 * 2^k blocks
    and sweep rows whose sum of squares leaves the fp32 range (their rstd is not compared, their neighbours' is)."""
    x, ref_s, ref_d = edge
    K = x.shape[1]
    r0 = 2
    xd = to_dev(x[r0:r0 + M])
    for with_rstd in (True, False):
        qa = torch.full(((M + 4) * K,), GUARD8, dtype=torch.uint8, device=dev())
        sa = torch.full((M * K // 32 + 128,), GUARD8, dtype=torch.uint8, device=dev())
        ra = torch.full((M + 8,), 0x7FC00001, dtype=torch.int32, device=dev())
        qo, so, ro = 2 * K, 64, 3
        rc = lib.sd_mxfp8_quant(xd.data_ptr(), K, qa.data_ptr() + qo, sa.data_ptr() + so,
                                ra.data_ptr() + 4 * ro if with_rstd else None, 1e-6, M, K, _stream())
        assert rc == 0
        q, s = qa[qo:qo + M * K].view(M, K).cpu(), sa[so:so + M * K // 32].view(M, K // 32).cpu()
        assert torch.equal(s, ref_s[r0:r0 + M])
        _same(mx_ref.mx_deq(q, s), ref_d[r0:r0 + M])
        assert bool((qa[:qo] == GUARD8).all()) and bool((qa[qo + M * K:] == GUARD8).all())
        assert bool((sa[:so] == GUARD8).all()) and bool((sa[so + M * K // 32:] == GUARD8).all())
        assert bool((ra[:ro] == 0x7FC00001).all()) and bool((ra[ro + M:] == 0x7FC00001).all())
        if with_rstd:
            ss = x[r0:r0 + M].double().pow(2).sum(-1)
            ok = (ss >= 2.0 ** -100) & (ss <= 2.0 ** 100)
            ref = torch.rsqrt(ss / K + 1e-6)
            got = ra[ro:ro + M].view(torch.float32).cpu().double()
            assert bool(ok.any()) and float(((got - ref).abs() / ref)[ok].max()) <= 1e-6
        else:
            assert bool((ra == 0x7FC00001).all())


# ------------------------------------------------------------------------------------------------ B: one-hot probes
def _gemm_side(ops, side, aq, as_, bq, bs):
    """The probe rows as the A operand, or -- transposed -- as the B operand."""
    if side == "a":
        return ops.gemm_mxfp8(to_dev(aq), to_dev(as_), to_dev(bq), to_dev(bs))
    return ops.gemm_mxfp8(to_dev(bq), to_dev(bs), to_dev(aq), to_dev(as_)).T


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("run", range(mx_ref.CODE_TABLE_RUNS))
def test_gemm_reads_every_e4m3_code_and_every_scale_byte(ops, run, side):
    """mx_ref.code_table_probe: each of the 254 finite codes (-0 included, in a zero block of scale byte 0) times 1.0,
    under scale bytes 0..254 on the probed side with exponent sums over [-100, 100]; every output is one product, a
    normal bf16 number or 0, so C must EQUAL it."""
    aq, as_, bq, bs, want, _, _ = mx_ref.code_table_probe(run)
    _same(_gemm_side(ops, side, aq, as_, bq, bs), want)


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("K", [128, 384])
def test_gemm_maps_every_k_position_to_its_own_scale_block(ops, K, side):
    """mx_ref.position_probe: the one-hot element runs through every k; the probed operand's scale differs from block to
    block of a row and the other operand differs along k, so a wrong byte-to-k map or a scale of another block changes C."""
    aq, as_, bq, bs, want = mx_ref.position_probe(K)
    _same(_gemm_side(ops, side, aq, as_, bq, bs), want)


# ------------------------------------------------------------------------------------------------ C: ring depths, exact
KMAX = 7 * 128
_OPERANDS = {}


def _int_rows(rows, K):
    """`rows` rows of the integer operand (|v| <= 8, scales 2^-2..2^2), first K columns; generated once per row count."""
    if rows not in _OPERANDS:
        _OPERANDS[rows] = mx_ref.int_operand(rows, KMAX, 8, 2, torch.Generator().manual_seed(rows))
    q, s = _OPERANDS[rows]
    return q[:, :K].contiguous(), s[:, :K // 32].contiguous()


def _int_case(M, N, K):
    """Operands, an integer residual and the exact results.  |a|, |b| <= 8 * 4 in units of 2^-2: every partial sum of every
    order is a multiple of 2^-4 below K * 2^10 <= 2^20 (asserted), an fp32 number -- the CPU's fp32 matmul is exact."""
    aq, as_ = _int_rows(M, K)
    bq, bs = _int_rows(N, K)
    a, b = mx_ref.mx_deq(aq, as_), mx_ref.mx_deq(bq, bs)
    assert K * float(a.abs().max()) * float(b.abs().max()) * 16 < 2 ** 24
    ref = a @ b.T
    assert float(ref.abs().max()) < 2 ** 20 and torch.equal(ref * 16, (ref * 16).round())
    r = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(M + N + K)).float()
    return aq, as_, bq, bs, r.bfloat16(), ref.bfloat16(), (ref + r).bfloat16()  # ref + r: exact too, one rounding


@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 7])
def test_gemm_exact_at_every_ring_depth_on_the_128_row_tile(ops, nk):
    """nk = 1..3 (steps past the end re-staged), NST = 4, NST + 1 and 7 (the ring wraps) for M in {1, 77, 129} (one row, a
    ragged tile, one row into the second tile) x N in {32, 96, 160} (N % 128 of 32, 96, 32 behind a full tile)."""
    K = nk * 128
    cases = [(M, N) + _int_case(M, N, K) for M in (1, 77, 129) for N in (32, 96, 160)]

    def run():
        out = []
        for M, N, aq, as_, bq, bs, r, want, want_r in cases:
            ops_in = [to_dev(t) for t in (aq, as_, bq, bs)]
            out.append((ops.gemm_mxfp8(*ops_in), ops.gemm_mxfp8(*ops_in, residual=to_dev(r))))
        return out
    got, syms = _profiled(ops, run)
    assert syms == {PLAIN128: 2 * len(cases)}, syms
    for (M, N, *_, want, want_r), (c, c_r) in zip(cases, got):
        assert torch.equal(c.cpu(), want), (M, N, int((c.cpu() != want).sum()))
        assert torch.equal(c_r.cpu(), want_r), (M, N, int((c_r.cpu() != want_r).sum()))


@pytest.mark.parametrize("M,N", [(300, 16384), (1, 32768)])
@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 7])
def test_gemm_exact_at_every_ring_depth_on_the_256_row_tile(ops, nk, M, N):
    """The 3-deep ring of the 8-wave tile at nk = NST - 2 .. NST + 2 and 7: M = 300 (a ragged second tile row) and M = 1 (a
    whole tile of clamped rows, spare scale threads).  (nk = 5, 7 at N = 32768 make B 20 and 28 MiB.)"""
    aq, as_, bq, bs, r, want, want_r = _int_case(M, N, nk * 128)
    ops_in = [to_dev(t) for t in (aq, as_, bq, bs)]
    (c, c_r), syms = _profiled(ops, lambda: (ops.gemm_mxfp8(*ops_in), ops.gemm_mxfp8(*ops_in, residual=to_dev(r))))
    assert syms == {PLAIN256: 2}, syms
    assert torch.equal(c.cpu(), want), int((c.cpu() != want).sum())
    assert torch.equal(c_r.cpu(), want_r), int((c_r.cpu() != want_r).sum())


# ------------------------------------------------------------------------------------------------ D: views, bounds, aliasing
def _gemm_raw(lib, dev_ops, c_ptr, ldc, M, N, K, r_ptr=None, ldr=0, rs=None):
    rc = lib.sd_gemm_mxfp8(*[t.data_ptr() for t in dev_ops], c_ptr, r_ptr, None if rs is None else rs.data_ptr(), M, N, K,
                           ldc, ldr, _stream())
    assert rc == 0, rc


@pytest.mark.parametrize("M,N,K,sym", [(77, 96, 256, PLAIN128), (129, 160, 384, PLAIN128), (300, 16384, 256, PLAIN256)])
def test_gemm_views_write_bounds_aliasing_and_row_scale(ops, lib, M, N, K, sym):
    """C is a window (ldc = N + 24) of a NaN-pattern arena with guard columns directly right of N and guard rows below M; R a
    view (ldr = N + 40) whose gaps hold NaN patterns; then R and C the same window.  The window equals the contiguous
    result bit for bit, the arena around it is unchanged.  With a row scale that is no power of two, on exact integers: one
    fp32 rounding before the bf16 store, so every element is the correctly rounded bf16 of fp64 rs * acc + r or one of
    its two neighbours."""
    aq, as_, bq, bs, r, want, want_r = _int_case(M, N, K)
    dev_ops = [to_dev(t) for t in (aq, as_, bq, bs)]
    ldc, ldr, r0, c0 = N + 24, N + 40, 1, 8

    def arena():
        a = _nan_arena(M + 3, ldc)
        return a, a.view(torch.bfloat16)[r0:r0 + M, c0:c0 + N]

    def untouched(a):
        g = a.clone()
        g[r0:r0 + M, c0:c0 + N] = NAN16
        return bool((g == NAN16).all())
    rbig = _nan_arena(M, ldr).view(torch.bfloat16)
    rview = rbig[:, 16:16 + N]
    rview.copy_(to_dev(r))

    def run():
        base = ops.gemm_mxfp8(*dev_ops)
        a1, w1 = arena()
        ops.gemm_mxfp8(*dev_ops, out=w1)
        a2, w2 = arena()
        _gemm_raw(lib, dev_ops, w2.data_ptr(), ldc, M, N, K, rview.data_ptr(), ldr)
        a3, w3 = arena()
        w3.copy_(to_dev(r))
        _gemm_raw(lib, dev_ops, w3.data_ptr(), ldc, M, N, K, w3.data_ptr(), ldc)
        return base, (a1, w1), (a2, w2), (a3, w3)
    (base, (a1, w1), (a2, w2), (a3, w3)), syms = _profiled(ops, run)
    assert syms == {sym: 4}, syms
    assert torch.equal(base.cpu(), want)
    assert torch.equal(w1, base) and untouched(a1)
    assert torch.equal(w2.cpu(), want_r) and untouched(a2)
    assert torch.equal(w3.cpu(), want_r) and untouched(a3)
    assert torch.equal(rview.cpu(), r)  # and the residual view itself is as it was
    # a row scale that is no power of two
    rs = (0.3 + 0.013 * torch.arange(M)).float()
    acc = mx_ref.mx_deq(aq, as_).double() @ mx_ref.mx_deq(bq, bs).double().T
    for res in (None, rview):
        a4, w4 = arena()
        _gemm_raw(lib, dev_ops, w4.data_ptr(), ldc, M, N, K, None if res is None else res.data_ptr(), ldr, to_dev(rs))
        ref = rs.double()[:, None] * acc + (0 if res is None else r.double())
        got = w4.cpu().double()
        c, up, down = mx_ref.bf16_neighbours(ref)
        ok = (got == c) | (got == up) | (got == down)
        assert bool(ok.all()), f"{int((~ok).sum())} of {ok.numel()} elements are further than one bf16 ulp away"
        assert untouched(a4)


# ------------------------------------------------------------------------------------------------ E: the SwiGLU epilogue
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("M,I,K,sym", [(1, 128, 384, SWIGLU128), (130, 128, 384, SWIGLU128), (1, 384, 128, SWIGLU128),
                                       (130, 384, 128, SWIGLU128), (1, 16384, 128, SWIGLU256), (300, 16384, 128, SWIGLU256)])
def test_swiglu_epilogue_against_arithmetic(ops, lib, M, I, K, sym, scaled):
    """mx_ref.swiglu_probe: gates of 32, 64 (silu(g) = g for any exp) and -104 (silu = -0), integer up values of both signs:
    act = g * u or 0 exactly, so the emitted image must be mx_ref.mx_quant(act) -- scale bytes equal (the zero block of
    every row: byte 0), dequantised values equal.  A gate/up swap, a wrong N + n0 or a wrong 64-column ownership changes
    values here.  Then the same call with act_q / act_scale as windows of guard-filled arenas: same bytes, and the rows
    >= M of the last tile leave everything behind the windows untouched."""
    aq, as_, wq, ws, rs, act = mx_ref.swiglu_probe(M, I, K, scaled)
    ref_q, ref_s = mx_ref.mx_quant(act.float())
    dev_ops = [to_dev(t) for t in (aq, as_, wq, ws)]
    rs_d = None if rs is None else to_dev(rs)
    qa = torch.full((M * I + 4096,), GUARD8, dtype=torch.uint8, device=dev())
    sa = torch.full((M * I // 32 + 256,), GUARD8, dtype=torch.uint8, device=dev())
    qo, so = 1024, 64

    def run():
        out = ops.gemm_mxfp8_swiglu(*dev_ops, rowscale=rs_d)
        rc = lib.sd_gemm_mxfp8_swiglu(*[t.data_ptr() for t in dev_ops], None if rs_d is None else rs_d.data_ptr(),
                                      qa.data_ptr() + qo, sa.data_ptr() + so, M, I, K, _stream())
        assert rc == 0, rc
        return out
    (q, s), syms = _profiled(ops, run)
    assert syms == {sym: 2}, syms
    assert torch.equal(s.cpu(), ref_s), f"{int((s.cpu() != ref_s).sum())} scale bytes differ"
    _same(mx_ref.mx_deq(q.cpu(), s.cpu()), mx_ref.mx_deq(ref_q, ref_s))
    assert torch.equal(qa[qo:qo + M * I].view(M, I), q) and torch.equal(sa[so:so + M * I // 32].view(M, I // 32), s)
    assert bool((qa[:qo] == GUARD8).all()) and bool((qa[qo + M * I:] == GUARD8).all())
    assert bool((sa[:so] == GUARD8).all()) and bool((sa[so + M * I // 32:] == GUARD8).all())


# ------------------------------------------------------------------------------------------------ F: refusals
def test_refusals_return_their_codes_without_a_launch(lib):
    """K % 128, N % 32, I % 128, ldc < N, ldc % 8, ldr < N, ldr % 8, ldx < K, ldx % 8, M <= 0: SD_ERR_SHAPE (-1); an operand,
    C or R pointer off a 16-byte boundary, a scale pointer off a 4-byte one: SD_ERR_ALIGN (-2).  The pointers are not
    device memory: a launch would fault, the codes come back before one."""
    P, SHAPE, ALIGN = 0x10000, -1, -2

    def quant(x=P, ldx=None, q=P, s=P, M=4, K=128):
        return lib.sd_mxfp8_quant(x, K if ldx is None else ldx, q, s, None, 1e-6, M, K, None)

    def gemm(a=P, as_=P, b=P, bs=P, c=P, r=None, M=4, N=32, K=128, ldc=None, ldr=None):
        return lib.sd_gemm_mxfp8(a, as_, b, bs, c, r, None, M, N, K, N if ldc is None else ldc,
                                 (N if r else 0) if ldr is None else ldr, None)

    def swiglu(a=P, as_=P, w=P, ws=P, q=P, s=P, M=4, I=128, K=128):
        return lib.sd_gemm_mxfp8_swiglu(a, as_, w, ws, None, q, s, M, I, K, None)

    for call in (quant, gemm, swiglu):
        assert call(K=96) == SHAPE and call(K=0) == SHAPE and call(K=192) == SHAPE
        assert call(M=0) == SHAPE and call(M=-1) == SHAPE
    assert quant(ldx=120) == SHAPE and quant(ldx=132) == SHAPE
    assert quant(x=P + 8) == ALIGN and quant(q=P + 8) == ALIGN and quant(s=P + 2) == ALIGN
    assert gemm(N=48) == SHAPE and gemm(N=0) == SHAPE and gemm(N=16) == SHAPE
    assert gemm(N=64, ldc=56) == SHAPE and gemm(N=64, ldc=68) == SHAPE
    assert gemm(N=64, r=P, ldr=56) == SHAPE and gemm(N=64, r=P, ldr=68) == SHAPE
    assert gemm(a=P + 8) == ALIGN and gemm(b=P + 8) == ALIGN and gemm(c=P + 8) == ALIGN and gemm(r=P + 8) == ALIGN
    assert gemm(as_=P + 2) == ALIGN and gemm(bs=P + 2) == ALIGN
    assert swiglu(I=64) == SHAPE and swiglu(I=192) == SHAPE and swiglu(I=0) == SHAPE
    assert swiglu(a=P + 8) == ALIGN and swiglu(w=P + 8) == ALIGN and swiglu(q=P + 8) == ALIGN
    assert swiglu(as_=P + 2) == ALIGN and swiglu(ws=P + 2) == ALIGN
    torch.cuda.synchronize()
