"""-m gpu tests of the weight-streaming GEMV over MXFP8 weights (include/sd_hip.h "the same GEMV over MXFP8 weights";
csrc/sd_gemv_mx.hip): sd_gemv_mxfp8 and sd_gemv_mxfp8_swiglu for 1 <= M <= 16.

References are tests/mx_ref.py and fp64 torch on the CPU, never the code under test; the two yardsticks that are kernels
(``ops.gemm_mxfp8``, ``ops.mxfp8_quant``, ``ops.swiglu_fwd``) are the existing entries the new ones are specified against.
Exact where the format allows it: integer data whose every partial sum is an fp32 number pins the operand, scale and
result lane maps of the block-scaled MFMA, the in-kernel quantiser is read back through an identity weight, and the
remaining tests state their bound.  Shapes: M in {1, 2, 3, 5, 8, 9, 16}; K in {128, 384, 512, 2048, 4224, 6144, 8192} (one
K-step, no multiple of 512, more than 4096, the maximum -- and every K-steps-per-wave variant: 1, 2, 4, 8); N in {1, 15,
16, 17, 37, 160, 600} (less than one MFMA tile, one past a tile, a ragged last workgroup)."""
import ctypes as C

import pytest
import torch

import mx_ref
from gpu_util import dev, record, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


def _int_weight(rows, K, vmax, smax, g):
    """A weight built directly as bytes: integer elements |v| <= vmax and power-of-two scales 2^-smax..2^smax, different per
    row and per block (the rule of tests/test_gpu_mx.py::_int_operand)."""
    v = torch.randint(-vmax, vmax + 1, (rows, K), generator=g).float()
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    s = (127 + torch.randint(-smax, smax + 1, (rows, K // 32), generator=g)).to(torch.uint8)
    return q, s


def _int_x(M, K, g):
    """bf16 integers |v| <= 8: every one has at most three significant bits, so each 32-block quantises without loss
    whatever its scale; asserted on the CPU reference."""
    x = torch.randint(-8, 9, (M, K), generator=g).float()
    assert torch.equal(mx_ref.mx_round(x), x)
    return x.bfloat16()


EXACT = [(1, 1, 128, 8, 2), (2, 15, 384, 8, 2), (3, 16, 512, 8, 2), (5, 17, 2048, 4, 1), (8, 37, 4224, 4, 1),
         (9, 160, 6144, 4, 1), (16, 600, 8192, 4, 1), (16, 600, 128, 8, 2), (1, 160, 1024, 8, 2)]


# ------------------------------------------------------------------------------------------------ 1: exact integers
@pytest.mark.parametrize("M,N,K,vmax,smax", EXACT)
def test_gemv_exact_integers_pin_the_operand_and_scale_maps(ops, M, N, K, vmax, smax):
    """|w| <= 4 with scales 2^-1..2 against |x| <= 8 at K = 8192: |sum| <= 8192 * 4 * 2 * 8 = 2^19 in units of 2^-1, so every
    partial sum is exact in fp32 in any order (wider ranges at small K; asserted below on the CPU) and the result must EQUAL
    bf16(fp32 matmul of the dequantised operands + r).  W is unrelated to x (asymmetric), scales differ per row and block."""
    g = torch.Generator().manual_seed(K + 31 * M + N)
    wq, ws = _int_weight(N, K, vmax, smax, g)
    x = _int_x(M, K, g)
    r = torch.randint(-64, 65, (M, N), generator=g).float().bfloat16()
    ref = x.double() @ mx_ref.mx_deq(wq, ws).double().T
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref.float().double(), ref)
    assert torch.equal((ref + r.double()).float().double(), ref + r.double())
    got = ops.gemv_mxfp8(to_dev(x), to_dev(wq), to_dev(ws))
    want = ref.float().bfloat16()
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).sum())} of {want.numel()} elements differ"
    got_r = ops.gemv_mxfp8(to_dev(x), to_dev(wq), to_dev(ws), residual=to_dev(r))
    want_r = (ref + r.double()).float().bfloat16()
    assert torch.equal(got_r.cpu(), want_r), f"{int((got_r.cpu() != want_r).sum())} of {want_r.numel()} elements differ"
    # r may alias y
    y = to_dev(r.clone())
    ops.gemv_mxfp8(to_dev(x), to_dev(wq), to_dev(ws), residual=y, out=y)
    assert torch.equal(y.cpu(), want_r)


# ------------------------------------------------------------------------------------------------ 2: the quantiser
@pytest.mark.parametrize("K", [128, 512])
@pytest.mark.parametrize("M", [1, 5, 16])
def test_in_kernel_quantiser_equals_the_reference_rule(ops, M, K):
    """W = identity (bytes of 1.0, scale byte 127), N = K: y[m, k] = X^[m, k], and every MX value is a bf16 number, so y
    must EQUAL mx_deq(mx_quant(x)).  x: random, with a zero block and a block holding +-448 * 2^k (saturating values)."""
    g = torch.Generator().manual_seed(M + K)
    x = (torch.randn(M, K, generator=g) * torch.randn(M, K, generator=g).exp()).bfloat16()
    x[:, 32:64] = 0
    x[0, 64:96] = 0
    x[:, 96] = 448.0 * 4
    x[:, 97] = -448.0 * 4
    x[M - 1, 100] = 480.0 * 4      # in (448, 512) * 2^2: saturates to 448 * 4
    wq = torch.eye(K).to(torch.float8_e4m3fn).view(torch.uint8)
    ws = torch.full((K, K // 32), 127, dtype=torch.uint8)
    want = mx_ref.mx_deq(*mx_ref.mx_quant(x.float()))
    assert torch.equal(want.bfloat16().float(), want)
    got = ops.gemv_mxfp8(to_dev(x), to_dev(wq), to_dev(ws))
    assert torch.equal(got.float().cpu(), want), f"{int((got.float().cpu() != want).sum())} elements differ"


@pytest.mark.parametrize("M,wide", [(5, False), (16, False), (33, True)])
def test_in_kernel_quantiser_on_the_ratio_sweep(ops, M, wide):
    """The same identity-weight probe on the deterministic edge rows of mx_ref (fixed blocks, then the ratio sweep: every
    bf16 mantissa at every exponent below block maxima from the smallest bf16 subnormal to the top exponent -- every tie,
    the saturating band, e4m3 subnormals, scale byte 0), M rows per call, on the 16-row kernel and (M = 33) the wide one."""
    x = mx_ref.edge_matrix(4, mx_ref.sweep_blocks())
    K = x.shape[1]
    wq = to_dev(torch.eye(K).to(torch.float8_e4m3fn).view(torch.uint8))
    ws = to_dev(torch.full((K, K // 32), 127, dtype=torch.uint8))
    want = mx_ref.mx_deq(*mx_ref.mx_quant(x.float()))
    assert torch.equal(want.bfloat16().float(), want)
    got = torch.cat([ops.gemv_mxfp8(to_dev(x[r:r + M]), wq, ws, wide=wide) for r in range(0, x.shape[0], M)]).float().cpu()
    bad = ~(got == want)
    assert not bool(bad.any()), f"{int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}"


# ------------------------------------------------------------------------------------------------ 3: norm and residual
@pytest.mark.parametrize("M,N,K", [(3, 37, 384), (9, 160, 2048), (16, 17, 6144)])
def test_norm_and_residual_within_one_bf16_ulp(ops, M, N, K):
    """Exact-integer weights, so acc is exact; x is integers too, rstd comes from the existing ops.mxfp8_quant.  Reference
    rstd * acc + r in fp64.  One fp32 rounding before the bf16 store can move a result to the adjacent bf16 number and no
    further: every element is the correctly rounded bf16 or one of its two neighbours.  No measured tolerance."""
    g = torch.Generator().manual_seed(M * N + K)
    wq, ws = _int_weight(N, K, 4, 1, g)
    x = _int_x(M, K, g)
    r = torch.randn(M, N, generator=g).bfloat16()
    _, _, rstd = ops.mxfp8_quant(to_dev(x), want_rstd=True, eps=1e-6)
    acc = x.double() @ mx_ref.mx_deq(wq, ws).double().T
    assert float(acc.abs().max()) < 2 ** 24
    for res in (None, r):
        ref = rstd.cpu().double()[:, None] * acc + (0 if res is None else res.double())
        got = ops.gemv_mxfp8(to_dev(x), to_dev(wq), to_dev(ws), residual=None if res is None else to_dev(res), norm=True,
                             eps=1e-6).cpu().double()
        c, up, down = mx_ref.bf16_neighbours(ref)
        ok = (got == c) | (got == up) | (got == down)
        assert bool(ok.all()), f"{int((~ok).sum())} of {ok.numel()} elements are further than one bf16 ulp away"


# ------------------------------------------------------------------------------------------------ 4: random data
TEACHER = [(4096, 2048), (2048, 2048), (12288, 2048), (2048, 6144)]   # q|k|v, o, gate|up, down of the 1.7B teacher (N, K)


@pytest.mark.parametrize("N,K", TEACHER)
@pytest.mark.parametrize("M", [1, 16])
def test_gemv_random_within_the_tile_gemm_error(ops, M, N, K):
    """Against fp64 of the dequantised operands with rstd and a residual.  Yardstick: the existing ops.gemm_mxfp8 on
    ops.mxfp8_quant(x) and the same weights, rowscale = rstd, the same residual: rms error <= 1.5 x its rms error and worst
    error <= 2 x its worst (the project's factors, tests/test_gpu_mx.py)."""
    g = torch.Generator().manual_seed(M + N + K)
    x = to_dev(torch.randn(M, K, generator=g).bfloat16())
    w = to_dev((0.02 * torch.randn(N, K, generator=g)).bfloat16())
    r = to_dev(torch.randn(M, N, generator=g).bfloat16())
    wq, ws = ops.mxfp8_quant(w)
    xq, xs, rstd = ops.mxfp8_quant(x, want_rstd=True, eps=1e-6)
    got = ops.gemv_mxfp8(x, wq, ws, residual=r, norm=True, eps=1e-6)
    yard = ops.gemm_mxfp8(xq, xs, wq, ws, rowscale=rstd, residual=r)
    ref = rstd.double()[:, None] * (mx_ref.mx_deq(xq, xs).double() @ mx_ref.mx_deq(wq, ws).double().T) + r.double()
    e_got, e_yard = got.double() - ref, yard.double() - ref
    rms_ratio = float(e_got.pow(2).mean().sqrt() / e_yard.pow(2).mean().sqrt())
    max_ratio = float(e_got.abs().max() / e_yard.abs().max())
    print(f"gemv_mxfp8 {M}x{N}x{K}: rms ratio {rms_ratio:.4f} max ratio {max_ratio:.4f}")
    record("gemv_mxfp8_vs_gemm_mxfp8", M=M, N=N, K=K, rms_ratio=rms_ratio, max_ratio=max_ratio)
    assert rms_ratio <= 1.5 and max_ratio <= 2.0


# ------------------------------------------------------------------------------------------------ 5: independence
@pytest.mark.parametrize("N,K", [(600, 2048), (37, 4224), (160, 8192), (17, 128)])
def test_rows_and_columns_are_independent(ops, N, K):
    """Row m of an M = 16 call equals the M = 1 call on that row; a call on w[n0:n1] equals columns n0:n1 of the full call;
    strided x, y and r views give the bits of contiguous ones."""
    g = torch.Generator().manual_seed(N + K)
    x = to_dev(torch.randn(16, K, generator=g).bfloat16())
    w = to_dev((0.05 * torch.randn(N, K, generator=g)).bfloat16())
    r = to_dev(torch.randn(16, N, generator=g).bfloat16())
    wq, ws = ops.mxfp8_quant(w)
    full = ops.gemv_mxfp8(x, wq, ws, residual=r, norm=True)
    for m in (0, 7, 15):
        one = ops.gemv_mxfp8(x[m:m + 1], wq, ws, residual=r[m:m + 1], norm=True)
        assert torch.equal(one[0], full[m]), m
    for M in (2, 3, 5, 8, 9):
        assert torch.equal(ops.gemv_mxfp8(x[:M], wq, ws, residual=r[:M], norm=True), full[:M]), M
    for n0, n1 in ((0, 1), (N // 3, N // 3 + 16), (N - 15, N), (1, N)):
        n0 = max(n0, 0)
        part = ops.gemv_mxfp8(x, wq[n0:n1].contiguous(), ws[n0:n1].contiguous(), residual=r[:, n0:n1], norm=True)
        assert torch.equal(part, full[:, n0:n1]), (n0, n1)
    # strided views: x inside a wider buffer, out and r inside wider ones
    xb = to_dev(torch.randn(16, K + 256, generator=g).bfloat16())
    xb[:, 128:128 + K] = x
    rb = to_dev(torch.randn(16, N + 24, generator=g).bfloat16())
    rb[:, 8:8 + N] = r
    ob = torch.zeros(16, N + 40, dtype=torch.bfloat16, device=dev())
    ops.gemv_mxfp8(xb[:, 128:128 + K], wq, ws, residual=rb[:, 8:8 + N], norm=True, out=ob[:, 3:3 + N])
    assert torch.equal(ob[:, 3:3 + N], full)
    assert bool((ob[:, :3] == 0).all()) and bool((ob[:, 3 + N:] == 0).all())


# ------------------------------------------------------------------------------------------------ 6: SwiGLU
@pytest.mark.parametrize("M,I,K", [(1, 128, 128), (5, 40, 512), (16, 600, 2048), (9, 160, 4224), (3, 1024, 1024)])
def test_swiglu_equals_the_unfused_sequence_bit_for_bit(ops, M, I, K):
    """(sd_swiglu_fwd takes I % 8 == 0; an odd I is held against a wider call below.)"""
    g = torch.Generator().manual_seed(M + I + K)
    x = to_dev((3 * torch.randn(M, K, generator=g)).bfloat16())
    w = to_dev((0.05 * torch.randn(2 * I, K, generator=g)).bfloat16())
    wq, ws = ops.mxfp8_quant(w)
    for norm in (True, False):
        gu = ops.gemv_mxfp8(x, wq, ws, norm=norm)
        want = ops.swiglu_fwd(gu)
        got = ops.gemv_mxfp8_swiglu(x, wq, ws, norm=norm)
        assert torch.equal(got, want), f"norm={norm}: {int((got != want).sum())} of {want.numel()} elements differ"


def test_swiglu_columns_are_independent_at_an_odd_width(ops):
    """I = 37 (no multiple of the tile, of 8 or of 2): act equals columns 0:37 of the I = 40 call whose gate and up rows
    0:37 are the same rows."""
    g = torch.Generator().manual_seed(37)
    M, I, K = 5, 40, 512
    x = to_dev((3 * torch.randn(M, K, generator=g)).bfloat16())
    wq, ws = ops.mxfp8_quant(to_dev((0.05 * torch.randn(2 * I, K, generator=g)).bfloat16()))
    wide = ops.gemv_mxfp8_swiglu(x, wq, ws, norm=True)
    rows = torch.cat([torch.arange(37), I + torch.arange(37)]).to(dev())
    odd = ops.gemv_mxfp8_swiglu(x, wq[rows].contiguous(), ws[rows].contiguous(), norm=True)
    assert odd.shape == (M, 37) and torch.equal(odd, wide[:, :37])


@pytest.mark.parametrize("M,I,K", [(16, 128, 512), (7, 256, 2048)])
def test_swiglu_quantised_equals_the_tile_epilogue_on_exact_integers(ops, M, I, K):
    """On exact-integer data the gate|up bf16 values of the GEMV and of the tile GEMM agree (both are the exact sum, rounded
    once), so mx_quant of the GEMV's act must be the bytes sd_gemm_mxfp8_swiglu emits."""
    g = torch.Generator().manual_seed(I + K)
    wq, ws = _int_weight(2 * I, K, 4, 1, g)
    x = _int_x(M, K, g)
    xq, xs = ops.mxfp8_quant(to_dev(x))
    assert torch.equal(mx_ref.mx_deq(xq.cpu(), xs.cpu()), x.float())
    act = ops.gemv_mxfp8_swiglu(to_dev(x), to_dev(wq), to_dev(ws))
    aq, as_ = ops.mxfp8_quant(act)
    fq, fs = ops.gemm_mxfp8_swiglu(xq, xs, to_dev(wq), to_dev(ws))
    assert torch.equal(as_, fs) and torch.equal(aq, fq)
    rq, rs = mx_ref.mx_quant(act.float().cpu())
    assert torch.equal(as_.cpu(), rs) and torch.equal(mx_ref.mx_deq(aq.cpu(), as_.cpu()), mx_ref.mx_deq(rq, rs))


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_return_their_codes_without_a_launch(ops):
    """M = 17, K = 96, K = 8320, a misaligned pointer: SD_ERR_UNSUPPORTED (-3); a NULL argument, M = 0: SD_ERR_SHAPE (-1).
    The pointers are not device memory: a launch would fault, the codes come back before one."""
    from speech_distill_amd import _lib
    lib = _lib.load_lib()
    P = 0x10000

    def gemv(x=P, ldx=None, wq=P, ws=P, y=P, M=1, N=16, K=128, r=None):
        return lib.sd_gemv_mxfp8(x, K if ldx is None else ldx, wq, ws, y, N, r, N if r else 0, 0, C.c_float(0.0), M, N, K, None)

    def swiglu(x=P, wq=P, ws=P, act=P, M=1, I=16, K=128):
        return lib.sd_gemv_mxfp8_swiglu(x, wq, ws, act, 1, C.c_float(1e-6), M, I, K, None)

    for call in (gemv, swiglu):
        assert call(M=17) == -3 and call(K=96) == -3 and call(K=8320) == -3
        assert call(x=P + 8) == -3 and call(wq=P + 4) == -3 and call(ws=P + 2) == -3
        assert call(x=None) == -1 and call(wq=None) == -1 and call(ws=None) == -1 and call(M=0) == -1 and call(K=0) == -1
    assert gemv(y=None) == -1 and swiglu(act=None) == -1 and gemv(N=0) == -1 and swiglu(I=0) == -1
    assert gemv(ldx=120) == -3 and gemv(ldx=132) == -3
    torch.cuda.synchronize()
