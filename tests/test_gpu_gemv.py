"""-m gpu: the weight-streaming GEMV kernels of the decode step (speech_distill_amd/csrc/sd_gemv.hip): sd_gemv_bf16 with
its optional residual and fused RMSNorm, sd_gemv_swiglu.

Yardsticks: plain fp64 torch for the values (with the tile GEMM sd_gemm_bf16 pushed through the same bound), the existing
kernels sd_rmsnorm_fwd and sd_swiglu_fwd for what the fused forms must equal bit for bit, and the kernel itself at other
M, N and row offsets for the invariance the generation loop relies on."""
import pytest
import torch

from gpu_util import dev

pytestmark = pytest.mark.gpu

SENT = 0x7FC1
NK = [(8, 128), (136, 512), (1000, 1024), (257, 3072)]
# Beyond one step per workgroup and beyond K = 4096.  Rows per workgroup are max(4 RW, ceil(N / (8 CUs)) rounded up to 4), 4 RW
# rows per step: on 256 CUs the shapes above are ONE step everywhere.  (40000, 1024): 20 rows = steps of 8, 8, 4 (the last
# partial); (30001, 2048): 16 rows = 4 steps, a last workgroup of 1 row; K = 6144 and 8192: two chunks per wave.
NK_DEEP = [(40000, 1024), (30001, 2048), (264, 6144), (264, 8192)]


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


_DATA = {}


def data(N, K):
    """x [16,K], w [N,K], r [16,N] ~ N(0,1) rounded to bf16, made once per shape and never changed."""
    if (N, K) not in _DATA:
        g = torch.Generator().manual_seed(1000 * N + K)
        _DATA[(N, K)] = tuple(torch.randn(*s, generator=g).to(torch.bfloat16) for s in ((16, K), (N, K), (16, N)))
    return _DATA[(N, K)]


# ------------------------------------------------------------------------------------------------------ 1. fp64 parity
@pytest.mark.parametrize("N,K", NK + NK_DEEP)
def test_gemv_against_fp64(ops, N, K):
    """Per element |y - y64| <= 2^-8 |y64| + K 2^-22 (sum_k |x_k w_k| + |r|): one bf16 rounding (8 significand bits) plus
    the fp32 accumulation bound K 2^-24 sum|xw| with 4x slack.  The bound is derived, not measured, so the tile GEMM
    (sd_gemm_bf16) is held to it on the same inputs."""
    x, w, r = data(N, K)
    xd, wd, rd = x.to(dev()), w.to(dev()), r.to(dev())
    Np = (N + 7) // 8 * 8           # sd_gemm_bf16 wants N % 8 == 0: it gets zero rows of w (and zeros of r) behind the N real ones
    wp = torch.zeros(Np, K, dtype=torch.bfloat16, device=dev())
    rp = torch.zeros(16, Np, dtype=torch.bfloat16, device=dev())
    wp[:N], rp[:, :N] = wd, rd
    w64 = w.double()
    y0_all, mag_all = x.double() @ w64.T, x.double().abs() @ w64.abs().T      # the reference, once for all 16 rows
    del w64
    for M in (1, 2, 3, 8, 16):
        y0, mag = y0_all[:M], mag_all[:M]
        for with_r in (False, True):
            y64 = y0 + (r[:M].double() if with_r else 0)
            allow = 2.0 ** -8 * y64.abs() + K * 2.0 ** -22 * (mag + (r[:M].double().abs() if with_r else 0))
            res = rd[:M].contiguous() if with_r else None
            got = ops.gemv_bf16(xd[:M].contiguous(), wd, residual=res).double().cpu()
            tile = ops.gemm(xd[:M].contiguous(), wp, residual=rp[:M].contiguous() if with_r else None)[:, :N].double().cpu()
            e_v, e_t = ((got - y64).abs() / allow).max(), ((tile - y64).abs() / allow).max()
            print(f"gemv N={N} K={K} M={M} r={with_r}: worst err / bound gemv {float(e_v):.3f} tile {float(e_t):.3f}")
            assert bool(torch.isfinite(got).all())
            assert float(e_t) <= 1.0, "the tile GEMM breaks the bound: the bound's derivation is wrong"
            assert float(e_v) <= 1.0, (M, with_r, float(e_v))


# ------------------------------------------------------------------------------------------- 2. nothing else is written
@pytest.mark.parametrize("M,N,K", [(3, 136, 512), (16, 257, 3072), (1, 8, 128)])
def test_gemv_writes_only_its_block_and_reads_no_gap(ops, M, N, K):
    x, w, r = data(N, K)
    ldx, ldw, ldy, ldr = K + 8, K + 16, N + 5, N + 3
    nan = float("nan")
    xs = torch.full((M, ldx), nan, dtype=torch.bfloat16)
    ws = torch.full((N, ldw), nan, dtype=torch.bfloat16)
    rs = torch.full((M, ldr), nan, dtype=torch.bfloat16)
    xs[:, :K], ws[:, :K], rs[:, :N] = x[:M], w, r[:M]
    xs, ws, rs = xs.to(dev()), ws.to(dev()), rs.to(dev())
    want = ops.gemv_bf16(x[:M].to(dev()), w.to(dev()), residual=r[:M].contiguous().to(dev()))
    buf = torch.full((M + 4, ldy), SENT, dtype=torch.int16, device=dev())   # two guard rows before and after
    out = buf.view(torch.bfloat16)[2:2 + M, :N]
    ops.gemv_bf16(xs[:, :K], ws[:, :K], residual=rs[:, :N], out=out)
    got = buf.clone()
    assert same_bits(got.view(torch.bfloat16)[2:2 + M, :N], want)
    assert not bool(torch.isnan(got.view(torch.bfloat16)[2:2 + M, :N].float()).any())
    got[2:2 + M, :N] = SENT
    assert bool((got == SENT).all())


# ------------------------------------------------------------------------------- 3. row, column and batch invariance
@pytest.mark.parametrize("N,K", [(1000, 1024), (257, 3072)] + NK_DEEP)
def test_gemv_rows_and_columns_do_not_depend_on_the_call(ops, N, K):
    x, w, r = data(N, K)
    xd, wd, rd = x.to(dev()), w.to(dev()), r.to(dev())
    full = ops.gemv_bf16(xd, wd, residual=rd)
    assert same_bits(ops.gemv_bf16(xd, wd, residual=rd), full)        # and the same bits twice
    five = ops.gemv_bf16(xd[3:8].contiguous(), wd, residual=rd[3:8].contiguous())
    assert same_bits(five, full[3:8])
    two = ops.gemv_bf16(xd[9:11].contiguous(), wd, residual=rd[9:11].contiguous())
    assert same_bits(two, full[9:11])
    for m in range(16):
        one = ops.gemv_bf16(xd[m:m + 1].contiguous(), wd, residual=rd[m:m + 1].contiguous())
        assert same_bits(one, full[m:m + 1]), m
    plain = ops.gemv_bf16(xd, wd)
    for n0, n1 in ((3, 260), (999, 1000), (5, N)):       # the last keeps a deep N deep: other workgroup ranges, same bits
        n0, n1 = min(n0, N - 1), min(n1, N)           # N = 257: (3, 257) and the last column
        part = ops.gemv_bf16(xd, wd[n0:n1])           # a view: ldw unchanged
        assert same_bits(part, plain[:, n0:n1]), (n0, n1)


# --------------------------------------------------------------------------------------- 4. fused norm = composition
@pytest.mark.parametrize("K", [128, 1024, 2048, 4096])
def test_gemv_fused_norm_equals_rmsnorm_then_gemv(ops, K):
    g = torch.Generator().manual_seed(K)
    N = 264
    x = torch.randn(16, K, generator=g)
    x *= torch.tensor([1e-3, 1.0, 1e3, 1.0] * 4)[:, None]    # rstd over six decades
    x = x.to(torch.bfloat16).to(dev())
    w = torch.randn(N, K, generator=g).to(torch.bfloat16).to(dev())
    gain = (1 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev())
    for M in (1, 16):
        for row0 in ((0, 2) if M == 1 else (0,)):
            xm = x[row0:row0 + M].contiguous()
            xn, _ = ops.rmsnorm_fwd(xm, gain, 1e-6)
            want = ops.gemv_bf16(xn, w)
            got = ops.gemv_bf16(xm, w, norm_gain=gain, eps=1e-6)
            assert same_bits(got, want), (K, M, row0)


# ------------------------------------------------------------------------------------- 5. fused SwiGLU = composition
# (10000, 1024): 12 weight rows per workgroup = steps of 8 and 4; (20000, 2048): 20 rows = 5 steps; (264, 6144): two chunks
@pytest.mark.parametrize("I,K", [(256, 128), (3072, 1024), (10000, 1024), (20000, 2048), (264, 6144)])
def test_gemv_swiglu_equals_gemv_then_swiglu(ops, I, K):
    g = torch.Generator().manual_seed(I + K)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16).to(dev())
    wgu = torch.randn(2 * I, K, generator=g).to(torch.bfloat16).to(dev())
    gain = (1 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev())
    for M in (1, 2, 16):
        xm = x[:M].contiguous()
        for ng in ((None, gain) if K <= 4096 else (None,)):     # a fused norm stops at K = 4096
            want = ops.swiglu_fwd(ops.gemv_bf16(xm, wgu, norm_gain=ng))
            got = ops.gemv_swiglu(xm, wgu, norm_gain=ng)
            assert same_bits(got, want), (I, K, M, ng is not None)
            assert bool(torch.isfinite(got.float()).all())


# ------------------------------------------------------------------------------------------------------- 6. refusals
def test_gemv_refuses_unsupported_shapes_and_leaves_y_alone(ops):
    lib = ops.load_lib()
    UNSUPPORTED = -3
    x = torch.zeros(17, 8192, dtype=torch.bfloat16, device=dev())
    w = torch.zeros(16, 8192, dtype=torch.bfloat16, device=dev())
    gain = torch.ones(8192, dtype=torch.bfloat16, device=dev())
    y = torch.full((17, 16), SENT, dtype=torch.int16, device=dev())

    def call(M, K, norm):
        return lib.sd_gemv_bf16(x.data_ptr(), w.data_ptr(), y.data_ptr(), None, gain.data_ptr() if norm else None, 1e-6,
                                M, 16, K, 8192, 8192, 16, 0, None)
    assert call(17, 1024, False) == UNSUPPORTED
    assert call(4, 1028, False) == UNSUPPORTED
    assert call(4, 8192, True) == UNSUPPORTED
    assert lib.sd_gemv_swiglu(x.data_ptr(), w.data_ptr(), y.data_ptr(), None, 1e-6, 17, 8, 1024, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == SENT).all())
