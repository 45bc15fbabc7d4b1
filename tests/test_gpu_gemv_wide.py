"""-m gpu: the wide weight-streaming GEMV kernels (speech_distill_amd/csrc/sd_gemv_wide.hip): sd_gemv_wide_bf16 with its
optional residual and fused RMSNorm, sd_gemv_wide_swiglu, for 1 <= M <= 64.

Yardsticks, taken over from test_gpu_gemv.py: plain fp64 torch under that file's derived bound, exact integer data for the
lane map and the K-steps, the existing kernels sd_rmsnorm_fwd and sd_swiglu_fwd for what the fused forms must equal bit for
bit, and the kernel itself at other M, N and row slots for the row independence the generation loop relies on."""
import pytest
import torch

from gpu_util import dev
from test_gpu_gemv import SENT, ops, same_bits  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

MS = (1, 5, 16, 17, 33, 64)
# one K-step slice (128: one wave), four waves, eight waves of 8 K-steps, eight waves of 32; N: two and a half tiles, whole
# tiles, a ragged last tile, three tiles
NK = [(40, 128), (256, 512), (100, 2048), (48, 8192)]

_DATA = {}


def data(N, K):
    """x [64,K], w [N,K], r [64,N] ~ N(0,1) rounded to bf16, and the fp64 product and magnitude sums of all 64 rows: made
    once per shape and never changed."""
    if (N, K) not in _DATA:
        g = torch.Generator().manual_seed(7000 * N + K)
        x, w, r = (torch.randn(*s, generator=g).to(torch.bfloat16) for s in ((64, K), (N, K), (64, N)))
        y0, mag = x.double() @ w.double().T, x.double().abs() @ w.double().abs().T
        _DATA[(N, K)] = (x, w, r, y0, mag, x.to(dev()), w.to(dev()), r.to(dev()))
    return _DATA[(N, K)]


def wide(ops, x, w, **kw):
    return ops.gemv_bf16(x, w, wide=True, **kw)


# ------------------------------------------------------------------------------------------------------ 1. fp64 parity
@pytest.mark.parametrize("N,K", NK)
def test_wide_gemv_against_fp64(ops, N, K):
    """Per element |y - y64| <= 2^-8 |y64| + K 2^-22 (sum_k |x_k w_k| + |r|): the bound of test_gemv_against_fp64 -- one
    bf16 rounding plus the fp32 accumulation bound with 4x slack, so it holds for any summation order."""
    x, w, r, y0_all, mag_all, xd, wd, rd = data(N, K)
    for M in MS:
        for with_r in (False, True):
            y64 = y0_all[:M] + (r[:M].double() if with_r else 0)
            allow = 2.0 ** -8 * y64.abs() + K * 2.0 ** -22 * (mag_all[:M] + (r[:M].double().abs() if with_r else 0))
            got = wide(ops, xd[:M].contiguous(), wd, residual=rd[:M].contiguous() if with_r else None).double().cpu()
            e = ((got - y64).abs() / allow).max()
            print(f"wide gemv N={N} K={K} M={M} r={with_r}: worst err / bound {float(e):.3f}")
            assert bool(torch.isfinite(got).all())
            assert float(e) <= 1.0, (M, with_r, float(e))


# ------------------------------------------------------------------------------------------------ 2. exact integer data
@pytest.mark.parametrize("N,K", NK)
def test_wide_gemv_is_exact_on_small_integers(ops, N, K):
    """x in [-3, 3], w in [-4, 4], r in [-8, 8], all integers: every product and every partial sum is an integer below 2^24,
    exact in fp32 in any order, so y must be the bf16 rounding of the integer result -- any lane map or K-step that is off
    changes an integer."""
    g = torch.Generator().manual_seed(N + K)
    x = torch.randint(-3, 4, (64, K), generator=g)
    w = torch.randint(-4, 5, (N, K), generator=g)
    r = torch.randint(-8, 9, (64, N), generator=g)
    xd, wd, rd = (t.to(torch.bfloat16).to(dev()) for t in (x, w, r))
    y = x @ w.T
    for M in MS:
        for with_r in (False, True):
            want = (y[:M] + (r[:M] if with_r else 0)).to(torch.float32).to(torch.bfloat16)
            got = wide(ops, xd[:M].contiguous(), wd, residual=rd[:M].contiguous() if with_r else None).cpu()
            assert same_bits(got, want), (M, with_r, int((got.float() != want.float()).sum()))


# ------------------------------------------------------------------------------------------------ 3. row independence
@pytest.mark.parametrize("N,K", [(100, 2048), (40, 128)])
def test_wide_gemv_rows_do_not_depend_on_the_call(ops, N, K):
    x, w, r, _, _, xd, wd, rd = data(N, K)
    full = wide(ops, xd, wd, residual=rd)
    assert same_bits(wide(ops, xd, wd, residual=rd), full)          # the same bits twice
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5)).to(dev())
    assert same_bits(wide(ops, xd[perm].contiguous(), wd, residual=rd[perm].contiguous()), full[perm])    # rows permuted
    for m in range(64):                                              # each row alone at M = 1
        one = wide(ops, xd[m:m + 1].contiguous(), wd, residual=rd[m:m + 1].contiguous())
        assert same_bits(one, full[m:m + 1]), m
    assert same_bits(wide(ops, xd[:17].contiguous(), wd, residual=rd[:17].contiguous()), full[:17])       # M = 17
    # rows at other slots of other tiles: rows 40..44 at the slots 13..17 of a 21-row batch (they straddle two B tiles)
    idx = torch.tensor(list(range(13)) + [40, 41, 42, 43, 44] + [60, 61, 62], device=dev())
    moved = wide(ops, xd[idx].contiguous(), wd, residual=rd[idx].contiguous())
    assert same_bits(moved[13:18], full[40:45]) and same_bits(moved, full[idx])
    plain = wide(ops, xd, wd)
    for n1 in (1, 16, 17, N - 1):                                    # N cut to a prefix (a view: ldw unchanged)
        assert same_bits(wide(ops, xd, wd[:n1]), plain[:, :n1]), n1
    assert same_bits(wide(ops, xd, wd[3:N]), plain[:, 3:N])         # and other rows into the tiles' slots


# --------------------------------------------------------------------------------------- 4. fused norm = composition
@pytest.mark.parametrize("K", [128, 1024, 4096])
def test_wide_gemv_fused_norm_equals_rmsnorm_then_gemv(ops, K):
    g = torch.Generator().manual_seed(K)
    N = 100
    x = torch.randn(64, K, generator=g)
    x *= torch.tensor([1e-3, 1.0, 1e3, 1.0] * 16)[:, None]    # rstd over six decades
    x = x.to(torch.bfloat16).to(dev())
    w = torch.randn(N, K, generator=g).to(torch.bfloat16).to(dev())
    gain = (1 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev())
    for M in (3, 64):
        xm = x[:M].contiguous()
        xn, _ = ops.rmsnorm_fwd(xm, gain, 1e-6)
        want = wide(ops, xn, w)
        got = wide(ops, xm, w, norm_gain=gain, eps=1e-6)
        assert same_bits(got, want), (K, M)
        assert bool(torch.isfinite(got.float()).all())


# ------------------------------------------------------------------------------------- 5. fused SwiGLU = composition
@pytest.mark.parametrize("I,K", [(24, 128), (24, 2048), (256, 128), (256, 2048)])
def test_wide_gemv_swiglu_equals_gemv_then_swiglu(ops, I, K):
    g = torch.Generator().manual_seed(I + K)
    x = torch.randn(64, K, generator=g).to(torch.bfloat16).to(dev())
    wgu = torch.randn(2 * I, K, generator=g).to(torch.bfloat16).to(dev())
    gain = (1 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev())
    for M in (1, 17, 64):
        xm = x[:M].contiguous()
        for ng in (None, gain):
            want = ops.swiglu_fwd(wide(ops, xm, wgu, norm_gain=ng))
            got = ops.gemv_swiglu(xm, wgu, norm_gain=ng, wide=True)
            assert same_bits(got, want), (I, K, M, ng is not None)
            assert bool(torch.isfinite(got.float()).all())


# ------------------------------------------------------------------------------------------------- 6. write footprint
@pytest.mark.parametrize("M,N,K", [(3, 40, 128), (17, 100, 2048), (64, 100, 2048)])
def test_wide_gemv_writes_only_its_block_and_reads_no_gap(ops, M, N, K):
    """Sentinels in the ldy gap, in two guard rows before row 0 and after row M - 1; NaNs in the gaps of x, w and r (a read
    of one would show in y)."""
    x, w, r, _, _, xd, wd, rd = data(N, K)
    ldx, ldw, ldy, ldr = K + 8, K + 16, N + 5, N + 3
    nan = float("nan")
    xs = torch.full((M, ldx), nan, dtype=torch.bfloat16)
    ws = torch.full((N, ldw), nan, dtype=torch.bfloat16)
    rs = torch.full((M, ldr), nan, dtype=torch.bfloat16)
    xs[:, :K], ws[:, :K], rs[:, :N] = x[:M], w, r[:M]
    xs, ws, rs = xs.to(dev()), ws.to(dev()), rs.to(dev())
    want = wide(ops, xd[:M].contiguous(), wd, residual=rd[:M].contiguous())
    buf = torch.full((M + 4, ldy), SENT, dtype=torch.int16, device=dev())
    out = buf.view(torch.bfloat16)[2:2 + M, :N]
    wide(ops, xs[:, :K], ws[:, :K], residual=rs[:, :N], out=out)
    got = buf.clone()
    assert same_bits(got.view(torch.bfloat16)[2:2 + M, :N], want)
    got[2:2 + M, :N] = SENT
    assert bool((got == SENT).all())


@pytest.mark.parametrize("M,N,K", [(5, 40, 128), (64, 100, 2048)])
def test_wide_gemv_y_may_alias_r(ops, M, N, K):
    _, _, _, _, _, xd, wd, rd = data(N, K)
    want = wide(ops, xd[:M].contiguous(), wd, residual=rd[:M].contiguous())
    y = rd[:M].clone()
    wide(ops, xd[:M].contiguous(), wd, residual=y, out=y)
    assert same_bits(y, want)


# ------------------------------------------------------------------------------------------------------- 7. refusals
def test_wide_gemv_refuses_unsupported_shapes_and_leaves_y_alone(ops):
    lib = ops.load_lib()
    UNSUPPORTED = -3
    x = torch.zeros(65, 8224, dtype=torch.bfloat16, device=dev())
    w = torch.zeros(16, 8224, dtype=torch.bfloat16, device=dev())
    gain = torch.ones(8224, dtype=torch.bfloat16, device=dev())
    y = torch.full((65, 16), SENT, dtype=torch.int16, device=dev())

    def call(M, K, norm):
        return lib.sd_gemv_wide_bf16(x.data_ptr(), w.data_ptr(), y.data_ptr(), None, gain.data_ptr() if norm else None,
                                     1e-6, M, 16, K, 8224, 8224, 16, 0, None)
    assert call(65, 1024, False) == UNSUPPORTED
    assert call(4, 1040, False) == UNSUPPORTED          # K % 32 != 0
    assert call(4, 8224, False) == UNSUPPORTED
    assert call(4, 8192, True) == UNSUPPORTED
    assert lib.sd_gemv_wide_swiglu(x.data_ptr(), w.data_ptr(), y.data_ptr(), None, 1e-6, 65, 8, 1024, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == SENT).all())
