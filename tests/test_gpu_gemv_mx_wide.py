"""-m gpu tests of the wide weight-streaming GEMV over MXFP8 weights (include/sd_hip.h "wide weight-streaming GEMV over MXFP8
weights"; gemv_mx_wide_kernel in csrc/sd_gemv_mx.hip): sd_gemv_mxfp8_wide and sd_gemv_mxfp8_wide_swiglu for 1 <= M <= 64.

The order contract is the first oracle: any 16-row slice of a wide call must EQUAL the existing 16-row kernel (sd_gemv_mxfp8)
on that slice -- the oracle is the old kernel, not the code under test.  Independent of it: exact integers against an fp64
product, the in-kernel quantiser read back through an identity weight against tests/mx_ref.py, row / column independence,
the SwiGLU form against ops.swiglu_fwd, the write footprint, and the refusals.  Shapes: M in {1, 16, 17, 33, 48, 64} (every
tile count MT = 1..4, a ragged last tile); K in {128, 1152, 2048, 4224, 6144, 8192} (K-steps per wave 1, 2, 4, 8: K = 1152 is
nine K-steps -- KPW 2, five waves, a one-step tail; 4224 is 33 -- KPW 8, a tail wave; 6144 is KPW 8 with six waves, where M
> 32 walks two column groups); N in {1, 17, 37, 600} (less than a tile, one past a tile, a ragged last workgroup).  On a
256-CU device those N give every workgroup one 16-row unit (TR = 1, SwiGLU TR = 2, one step); the large-N cases below reach
the kernels with 2 and 4 weight tiles per step, the register cap on them, and a second step."""
import ctypes as C

import pytest
import torch

import mx_ref
from gpu_util import dev, to_dev

pytestmark = pytest.mark.gpu

MS = (1, 16, 17, 33, 48, 64)


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


def _int_weight(rows, K, vmax, smax, g):
    """A weight built directly as bytes: integer elements |v| <= vmax and power-of-two scales 2^-smax..2^smax, different per
    row and per block (the construction of tests/test_gpu_gemv_mx.py)."""
    v = torch.randint(-vmax, vmax + 1, (rows, K), generator=g).float()
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    s = (127 + torch.randint(-smax, smax + 1, (rows, K // 32), generator=g)).to(torch.uint8)
    return q, s


def _int_x(M, K, g):
    """bf16 integers |v| <= 8: at most three significant bits, so each 32-block quantises without loss whatever its scale."""
    x = torch.randint(-8, 9, (M, K), generator=g).float()
    assert torch.equal(mx_ref.mx_round(x), x)
    return x.bfloat16()


def _slices(M):
    return [(s, min(s + 16, M)) for s in range(0, M, 16)]


_CASES = {}


def _case(ops, N, K):
    """Random x [64, K] (rows of very different magnitude), weight [N, K] in MXFP8 and a residual, made once per (N, K)."""
    if (N, K) not in _CASES:
        g = torch.Generator().manual_seed(7 * N + K)
        x = (torch.randn(64, K, generator=g) * torch.randn(64, 1, generator=g).exp()).bfloat16()
        w = (0.05 * torch.randn(N, K, generator=g)).bfloat16()
        r = torch.randn(64, N, generator=g).bfloat16()
        wq, ws = ops.mxfp8_quant(to_dev(w))
        _CASES[(N, K)] = (to_dev(x), wq, ws, to_dev(r))
    return _CASES[(N, K)]


# every M meets K = 1152 and K = 6144; every K and every N is met
SLICE_CASES = [(M, K, N) for M in MS for K, N in ((1152, 37), (6144, 17))] + \
              [(17, 128, 1), (64, 128, 600), (33, 2048, 600), (48, 2048, 1), (64, 4224, 37), (17, 4224, 600), (48, 8192, 17),
               (64, 8192, 1), (33, 6144, 600), (64, 1152, 600)]


# ------------------------------------------------------------------------------------------------ 1: the order contract
@pytest.mark.parametrize("M,K,N", SLICE_CASES)
def test_every_16_row_slice_equals_the_16_row_kernel(ops, M, K, N):
    """Plain, norm, norm + residual, and the residual aliasing the output: sd_gemv_mxfp8_wide(x)[s] == sd_gemv_mxfp8(x[s])."""
    x, wq, ws, r = _case(ops, N, K)
    x, r = x[:M], r[:M]
    for norm, res in ((False, None), (True, None), (True, r), (False, r)):
        got = ops.gemv_mxfp8(x, wq, ws, residual=res, norm=norm, wide=True)
        for a, b in _slices(M):
            want = ops.gemv_mxfp8(x[a:b], wq, ws, residual=None if res is None else res[a:b], norm=norm)
            assert torch.equal(got[a:b], want), (norm, res is not None, a, int((got[a:b] != want).sum()))
    y = r.clone()
    ops.gemv_mxfp8(x, wq, ws, residual=y, norm=True, out=y, wide=True)   # r may alias y
    assert torch.equal(y, ops.gemv_mxfp8(x, wq, ws, residual=r, norm=True, wide=True))


@pytest.mark.parametrize("M,K,N", [(33, 1152, 37), (64, 6144, 17), (48, 2048, 600)])
def test_strided_rows_give_the_bits_of_contiguous_ones(ops, M, K, N):
    x, wq, ws, r = _case(ops, N, K)
    x, r = x[:M], r[:M]
    full = ops.gemv_mxfp8(x, wq, ws, residual=r, norm=True, wide=True)
    g = torch.Generator().manual_seed(M)
    xb = to_dev(torch.randn(M, K + 256, generator=g).bfloat16())
    xb[:, 128:128 + K] = x
    rb = to_dev(torch.randn(M, N + 24, generator=g).bfloat16())
    rb[:, 8:8 + N] = r
    ob = torch.zeros(M, N + 40, dtype=torch.bfloat16, device=dev())
    ops.gemv_mxfp8(xb[:, 128:128 + K], wq, ws, residual=rb[:, 8:8 + N], norm=True, out=ob[:, 3:3 + N], wide=True)
    assert torch.equal(ob[:, 3:3 + N], full)
    assert bool((ob[:, :3] == 0).all()) and bool((ob[:, 3 + N:] == 0).all())


@pytest.mark.parametrize("M,I,K", [(M, 40, K) for M in MS for K in (1152, 6144)] +
                         [(17, 600, 2048), (64, 600, 4224), (33, 600, 128), (48, 40, 8192)])
def test_swiglu_slices_equal_the_16_row_kernel(ops, M, I, K):
    g = torch.Generator().manual_seed(M + I + K)
    x = to_dev((3 * torch.randn(M, K, generator=g)).bfloat16())
    wq, ws = ops.mxfp8_quant(to_dev((0.05 * torch.randn(2 * I, K, generator=g)).bfloat16()))
    for norm in (True, False):
        got = ops.gemv_mxfp8_swiglu(x, wq, ws, norm=norm, wide=True)
        for a, b in _slices(M):
            want = ops.gemv_mxfp8_swiglu(x[a:b], wq, ws, norm=norm)
            assert torch.equal(got[a:b], want), (norm, a, int((got[a:b] != want).sum()))


# More than 512 / 1024 / 1536 units of 16 weight rows: with about two workgroups per CU (256 CUs) a workgroup then owns 2 or
# 4 units.  (M, K, N): (64, 1152, 8208) two tiles per step; (64, 6144, 8208) the same in two column groups; (64, 1152, 24592)
# four tiles per step; (33, 6144, 24592) four units per workgroup capped to two tiles per step by the registers: two steps,
# the barrier and the look-ahead load between them.  Made on the device: the weights are up to 151 MB.
LARGE_N = [(64, 1152, 8208), (64, 6144, 8208), (64, 1152, 24592), (33, 6144, 24592)]


@pytest.mark.parametrize("M,K,N", LARGE_N)
def test_slices_at_widths_where_a_workgroup_owns_several_units(ops, M, K, N):
    """Both forms against the 16-row kernel on every 16-row slice, and columns 0:600 of the plain form against the wide
    call on the first 600 weight rows (one unit per workgroup: another instantiation, another grid)."""
    g = torch.Generator(device=dev()).manual_seed(N + K + M)
    x = (torch.randn(M, K, generator=g, device=dev()) * torch.randn(M, 1, generator=g, device=dev()).exp()).bfloat16()
    r = torch.randn(M, N, generator=g, device=dev()).bfloat16()
    wq, ws = ops.mxfp8_quant((0.05 * torch.randn(N, K, generator=g, device=dev())).bfloat16())
    got = ops.gemv_mxfp8(x, wq, ws, residual=r, norm=True, wide=True)
    for a, b in _slices(M):
        want = ops.gemv_mxfp8(x[a:b], wq, ws, residual=r[a:b], norm=True)
        assert torch.equal(got[a:b], want), (a, int((got[a:b] != want).sum()))
    part = ops.gemv_mxfp8(x, wq[:600], ws[:600], residual=r[:, :600], norm=True, wide=True)
    assert torch.equal(part, got[:, :600])
    act = ops.gemv_mxfp8_swiglu(x, wq, ws, norm=True, wide=True)      # I = N / 2: half the units, SwiGLU pairs
    for a, b in _slices(M):
        want = ops.gemv_mxfp8_swiglu(x[a:b], wq, ws, norm=True)
        assert torch.equal(act[a:b], want), (a, int((act[a:b] != want).sum()))
    assert torch.equal(act, ops.swiglu_fwd(ops.gemv_mxfp8(x, wq, ws, norm=True, wide=True)))


# ------------------------------------------------------------------------------------------------ 2: exact integers
@pytest.mark.parametrize("M,N,K,vmax,smax", [(33, 17, 2048, 4, 1), (64, 37, 4224, 4, 1), (17, 1, 128, 8, 2)])
def test_exact_integers_equal_the_integer_product(ops, M, N, K, vmax, smax):
    """|w| <= 4 with scales 2^-1..2 against |x| <= 8 at K = 4224: |sum| < 2^19 in units of 2^-1, so every partial sum is an
    fp32 number in any order (asserted on the CPU) and the result must EQUAL bf16(product + r).  Independent of the 16-row
    kernel: it pins the operand, scale and result lane maps of every B tile."""
    g = torch.Generator().manual_seed(K + 31 * M + N)
    wq, ws = _int_weight(N, K, vmax, smax, g)
    x = _int_x(M, K, g)
    r = torch.randint(-64, 65, (M, N), generator=g).float().bfloat16()
    ref = x.double() @ mx_ref.mx_deq(wq, ws).double().T
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref.float().double(), ref)
    assert torch.equal((ref + r.double()).float().double(), ref + r.double())
    got = ops.gemv_mxfp8(to_dev(x), to_dev(wq), to_dev(ws), wide=True)
    want = ref.float().bfloat16()
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).sum())} of {want.numel()} elements differ"
    got_r = ops.gemv_mxfp8(to_dev(x), to_dev(wq), to_dev(ws), residual=to_dev(r), wide=True)
    want_r = (ref + r.double()).float().bfloat16()
    assert torch.equal(got_r.cpu(), want_r), f"{int((got_r.cpu() != want_r).sum())} of {want_r.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ 3: the quantiser
def test_in_kernel_quantiser_equals_the_reference_rule(ops):
    """W = identity (bytes of 1.0, scale byte 127), N = K = 512, M = 64: y[m, k] = X^[m, k] and every MX value is a bf16
    number, so y must EQUAL mx_deq(mx_quant(x)).  x: random, with zero blocks and blocks holding saturating values."""
    M, K = 64, 512
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
    got = ops.gemv_mxfp8(to_dev(x), to_dev(wq), to_dev(ws), wide=True)
    assert torch.equal(got.float().cpu(), want), f"{int((got.float().cpu() != want).sum())} elements differ"


# ------------------------------------------------------------------------------------------------ 4: independence
@pytest.mark.parametrize("K", [1152, 6144])
def test_rows_and_columns_are_independent(ops, K):
    """Row m of a 64-row call equals the same row alone at M = 1 (slot 0 of tile 0) and in another slot of another tile of
    a 40-row call; a call on w[n0:n1] equals columns n0:n1 of the full call (N = 37)."""
    N = 37
    x, wq, ws, r = _case(ops, N, K)
    full = ops.gemv_mxfp8(x, wq, ws, residual=r, norm=True, wide=True)
    perm = torch.tensor([(m * 23 + 5) % 64 for m in range(40)], device=dev())   # row perm[i] sits in slot i of the 40-row call
    moved = ops.gemv_mxfp8(x[perm].contiguous(), wq, ws, residual=r[perm].contiguous(), norm=True, wide=True)
    assert torch.equal(moved, full[perm])
    for m in (0, 15, 16, 37, 63):
        one = ops.gemv_mxfp8(x[m:m + 1], wq, ws, residual=r[m:m + 1], norm=True, wide=True)
        assert torch.equal(one[0], full[m]), m
    for n0, n1 in ((0, 1), (12, 28), (N - 15, N), (1, N)):
        part = ops.gemv_mxfp8(x, wq[n0:n1].contiguous(), ws[n0:n1].contiguous(), residual=r[:, n0:n1], norm=True, wide=True)
        assert torch.equal(part, full[:, n0:n1]), (n0, n1)


# ------------------------------------------------------------------------------------------------ 5: SwiGLU
@pytest.mark.parametrize("M,I,K", [(33, 40, 512), (64, 600, 2048)])
def test_swiglu_equals_swiglu_fwd_of_the_2i_call(ops, M, I, K):
    g = torch.Generator().manual_seed(M + I + K)
    x = to_dev((3 * torch.randn(M, K, generator=g)).bfloat16())
    wq, ws = ops.mxfp8_quant(to_dev((0.05 * torch.randn(2 * I, K, generator=g)).bfloat16()))
    for norm in (True, False):
        want = ops.swiglu_fwd(ops.gemv_mxfp8(x, wq, ws, norm=norm, wide=True))
        got = ops.gemv_mxfp8_swiglu(x, wq, ws, norm=norm, wide=True)
        assert torch.equal(got, want), f"norm={norm}: {int((got != want).sum())} of {want.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ 6: the write footprint
@pytest.mark.parametrize("M,N,K", [(17, 37, 1152), (33, 17, 6144), (48, 600, 2048), (1, 1, 128)])
def test_nothing_outside_the_result_is_written_and_rows_past_m_are_not_read(ops, M, N, K):
    """y lies inside a buffer of sentinels (rows above and below, columns left and right); x lies inside a buffer whose
    other rows are NaN.  The sentinels must survive and the result must equal the call on a clean copy: a lane that read a
    row >= M into its fragment would turn NaN * 0 into NaN for every column of its tile."""
    x, wq, ws, r = _case(ops, N, K)
    clean = ops.gemv_mxfp8(x[:M].contiguous(), wq, ws, norm=True, wide=True)
    xb = torch.full((M + 66, K), float("nan"), dtype=torch.bfloat16, device=dev())
    xb[1:1 + M] = x[:M]
    SENT = -12345.0
    ob = torch.full((M + 66, N + 16), SENT, dtype=torch.bfloat16, device=dev())
    ops.gemv_mxfp8(xb[1:1 + M], wq, ws, norm=True, out=ob[1:1 + M, 8:8 + N], wide=True)
    assert torch.equal(ob[1:1 + M, 8:8 + N], clean)
    ob[1:1 + M, 8:8 + N] = SENT
    assert bool((ob == SENT).all()), f"{int((ob != SENT).sum())} elements outside y[0..M, 0..N) were written"
    if N >= 2:   # the SwiGLU form on the first 2 I weight rows, act between sentinel rows
        I = N // 2
        act = torch.full((M + 66, I), SENT, dtype=torch.bfloat16, device=dev())
        lib = ops.load_lib()
        from speech_distill_amd.ops import _stream
        rc = lib.sd_gemv_mxfp8_wide_swiglu(xb[1:1 + M].data_ptr(), wq[:2 * I].data_ptr(), ws[:2 * I].data_ptr(),
                                           act[1:1 + M].data_ptr(), 1, C.c_float(1e-6), M, I, K, _stream())
        assert rc == 0
        want = ops.gemv_mxfp8_swiglu(x[:M].contiguous(), wq[:2 * I].contiguous(), ws[:2 * I].contiguous(), norm=True, wide=True)
        assert torch.equal(act[1:1 + M], want)
        assert bool((act[:1] == SENT).all()) and bool((act[1 + M:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_return_their_codes_and_leave_y_alone(ops):
    """M = 65, K % 128 != 0, K > 8192, misaligned pointers or strides: SD_ERR_UNSUPPORTED (-3); a NULL argument or a
    non-positive size: SD_ERR_SHAPE (-1).  y is real memory full of sentinels and must keep them; the other pointers are not
    device memory -- a launch would fault, the codes come back before one."""
    lib = ops.load_lib()
    P = 0x10000
    ybuf = torch.full((65 * 16,), 7.0, dtype=torch.bfloat16, device=dev())
    Y = ybuf.data_ptr()

    def gemv(x=P, ldx=None, wq=P, ws=P, y=Y, M=1, N=16, K=128, r=None, ldy=None, ldr=None):
        return lib.sd_gemv_mxfp8_wide(x, K if ldx is None else ldx, wq, ws, y, N if ldy is None else ldy, r,
                                      (N if r else 0) if ldr is None else ldr, 0, C.c_float(0.0), M, N, K, None)

    def swiglu(x=P, wq=P, ws=P, act=Y, M=1, I=16, K=128):
        return lib.sd_gemv_mxfp8_wide_swiglu(x, wq, ws, act, 1, C.c_float(1e-6), M, I, K, None)

    for call in (gemv, swiglu):
        assert call(M=65) == -3 and call(K=96) == -3 and call(K=8320) == -3
        assert call(x=P + 8) == -3 and call(wq=P + 4) == -3 and call(ws=P + 2) == -3
        assert call(x=None) == -1 and call(wq=None) == -1 and call(ws=None) == -1 and call(M=0) == -1 and call(K=0) == -1
    assert gemv(y=None) == -1 and swiglu(act=None) == -1 and gemv(N=0) == -1 and swiglu(I=0) == -1
    assert gemv(ldx=120) == -3 and gemv(ldx=132) == -3 and gemv(ldy=8) == -3 and gemv(r=P, ldr=8) == -3
    torch.cuda.synchronize()
    assert bool((ybuf == 7.0).all())
