"""-m gpu: the ADDRESSING of csrc/sd_gemm.hip -- strided views, write bounds, odd K, non-finite neighbours, refusals.

tests/test_gpu_kernels.py pins the arithmetic of the GEMMs on contiguous tensors through speech_distill_amd.ops; here every
call goes through the C ABI (ops.load_lib(), data_ptr(), stride(0)), so that operands and outputs can be WINDOWS of larger,
filled parents (tests/gemm_ref.py: LOUD / NAN / INF gaps around the inputs, a SENTINEL bit pattern around and under the
outputs).  Data are integers in [-3, 3] (row 0 raised by one): the one right answer is gemm_ref.int_expect, compared bit
for bit; the parent of every output is compared bit for bit outside the window.  Every launch is profiled and the gemm_*
symbol it ran must be the one `_lib.gemm_plan` names for that very call (and, on 256 CUs, the one gemm_ref.FAMILIES
names), so no probe passes on another kernel than it claims.  tests/test_gemm_ref_cpu.py proves the probes on the CPU.

Contract under test (include/sd_hip.h, sd_gemm_bf16): C[m][n] depends only on its own operand rows; the bytes between the
rows of a view are never interpreted; nothing outside C's M x N elements is written; bad arguments are refused before any
launch."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as G
from gemm_ref import BF, COL0, GUARD, INF, LOUD, NAN, PAD, SENTINEL
from gpu_util import dev, record
from speech_distill_amd import _lib

pytestmark = pytest.mark.gpu

WIN = (PAD, COL0, GUARD)   # ld = natural + 24, first column 8, two guard rows
FLAT = (0, 0, 0)           # a contiguous operand
ROWS = (0, 0, GUARD)       # natural leading dimension (fixed by the entry point), guard rows in front and behind
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def ops():
    import speech_distill_amd.ops as ops_
    ops_.load_lib()
    _lib.debug_set("reset", 0)
    yield ops_
    _lib.debug_set("reset", 0)


@pytest.fixture(autouse=True)
def default_switches():
    _lib.debug_set("reset", 0)
    yield
    _lib.debug_set("reset", 0)


@contextlib.contextmanager
def switched(switches):
    try:
        for k, v in switches.items():
            _lib.debug_set(k, v)
        yield
    finally:
        _lib.debug_set("reset", 0)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def place(x, fill, geom=WIN):
    """a CPU matrix -> its copy on the GPU as a window of a parent filled with `fill`"""
    pad, col0, guard = geom
    rows, cols = x.shape
    parent, view = G.window(rows, cols, cols + pad, col0, guard, fill, x.dtype)
    view.copy_(x)
    return G.view_of(parent.to(dev()), rows, cols, col0, guard)


class Out:
    """an output window over a SENTINEL parent (`init`: what the window holds before the call)"""

    def __init__(self, rows, cols, geom=WIN, dtype=BF, init=None):
        pad, col0, guard = geom
        self.rows, self.cols, self.col0, self.guard = rows, cols, col0, guard
        self.before, view = G.window(rows, cols, cols + pad, col0, guard, SENTINEL, dtype)
        if init is not None:
            view.copy_(init)
        self.parent = self.before.to(dev())
        self.view = G.view_of(self.parent, rows, cols, col0, guard)

    def got(self):
        """the window after the call; asserts first that nothing outside it changed"""
        torch.cuda.synchronize()
        after = self.parent.cpu()
        bad = G.outside_untouched(self.before, after, self.guard, self.rows, self.col0, self.cols)
        assert bad is None, f"parent element {bad} outside the {self.rows} x {self.cols} window was written"
        return G.view_of(after, self.rows, self.cols, self.col0, self.guard)

    def assert_untouched(self):
        torch.cuda.synchronize()
        assert G.first_diff(self.parent, self.before) is None


def profiled(ops, call):
    """-> (status, the gemm_* symbols the call launched)"""
    ops.prof_begin()
    try:
        rc = call()
    finally:
        ops.prof_end()
    torch.cuda.synchronize()
    return rc, [s for s in ops.prof_symbols() if s.startswith("gemm_")]


def same_bits(got, want, what):
    bad = G.first_diff(got, want)
    assert bad is None, f"{what}: first wrong element {bad}: got {float(got[bad])}, want {float(want[bad])}"


SEEN = {}


def note(test, symbol):
    SEEN.setdefault(test, set()).add(symbol)


@pytest.fixture(scope="module", autouse=True)
def log_symbols():
    yield
    for test, syms in sorted(SEEN.items()):
        record("gemm_views_symbols", probe=test, symbols=sorted(syms))


def run_gemm(ops, M, N, K, ta, tb, a, b, r=None, alias=False, fill=LOUD, entry="gemm", geom=WIN, a_geom=None, out_geom=WIN,
             symbol=None, test="", expect=None):
    """One sd_gemm_bf16 / _splitk call on windows; asserts status, plan == launch (== symbol on 256 CUs), the guards of
    C (and of the split-K workspace), and, given `expect`, the bits of the window.  -> the window (CPU)."""
    lib = ops.load_lib()
    va, vb = place(a, fill, a_geom or geom), place(b, fill, geom)
    c = Out(M, N, out_geom, init=r if alias else None)
    vr = c.view if alias else (None if r is None else place(r, fill, geom))
    ldr = 0 if vr is None else vr.stride(0)
    split = entry != "gemm"
    plan = _lib.gemm_plan(M, N, K, ta, tb, lda=va.stride(0), ldb=vb.stride(0), ldc=c.view.stride(0), residual=r is not None,
                          split_k=split, cus=cus())["symbol"]
    ws = None
    if split:
        nsplit = lib.sd_gemm_splitk_plan(M, N, K)
        ws = Out(nsplit * M if nsplit > 1 else 8, N, ROWS, torch.float32)
        nb = nsplit * M * N * 4 if nsplit > 1 else 0
        assert lib.sd_gemm_splitk_workspace_bytes(M, N, K) == nb
        call = lambda: lib.sd_gemm_bf16_splitk(ptr(va), ptr(vb), ptr(c.view), ptr(vr), M, N, K, va.stride(0), vb.stride(0),  # noqa: E731
                                               c.view.stride(0), ldr, int(ta), int(tb), ptr(ws.view), nb, stream())
    else:
        call = lambda: lib.sd_gemm_bf16(ptr(va), ptr(vb), ptr(c.view), ptr(vr), M, N, K, va.stride(0), vb.stride(0),  # noqa: E731
                                        c.view.stride(0), ldr, int(ta), int(tb), stream())
    rc, syms = profiled(ops, call)
    assert rc == OK, rc
    assert syms == [plan], (syms, plan)
    if symbol is not None and cus() == 256:
        assert plan == symbol, (plan, symbol)
    note(test, plan)
    got = c.got()
    if ws is not None:
        ws.got()
    if expect is not None:
        same_bits(got, expect, f"{test} {plan} ({M}, {N}, {K}) ta={ta} tb={tb}")
    return got


def random_operands(M, N, K, ta, tb, res, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((K, M) if ta else (M, K), generator=g).to(BF)
    b = torch.randn((K, N) if tb else (N, K), generator=g).to(BF)
    return a, b, ((torch.randn(M, N, generator=g) * 8).to(BF) if res else None)


# ---------------------------------------------------------------------------------------------------- 1. views
PLAIN = [f["name"] for f in G.FAMILIES if f["entry"] in ("gemm", "splitk")]


@pytest.mark.parametrize("name", PLAIN)
def test_views(ops, name):
    """A, B, R and C as windows (LOUD gaps, SENTINEL around C): the exact result inside C's window, nothing written outside
    it; with a residual window, with C aliasing R (accumulate), and one random-data pass under gemm_ref.elem_bound."""
    f = G.BY_NAME[name]
    (M, N, K), ta, tb, entry = f["shape"], f["ta"], f["tb"], f["entry"]
    a, b, r = G.int_operands(M, N, K, ta, tb, True, seed=len(name) + K)
    base = r if f["res"] else None
    with switched(f["switches"]):
        run_gemm(ops, M, N, K, ta, tb, a, b, base, entry=entry, symbol=f["symbol"], test=name, expect=G.int_expect(a, b, ta, tb, base))
        want = G.int_expect(a, b, ta, tb, r)
        run_gemm(ops, M, N, K, ta, tb, a, b, r, entry=entry, test=name, expect=want)
        run_gemm(ops, M, N, K, ta, tb, a, b, r, alias=True, entry=entry, test=name, expect=want)
        ra, rb, rr = random_operands(M, N, K, ta, tb, f["res"], seed=K)
        got = run_gemm(ops, M, N, K, ta, tb, ra, rb, rr, entry=entry, symbol=f["symbol"], test=name)
    ratio = G.worst_ratio(got, ra, rb, ta, tb, rr, K)
    record(f"gemm_views_random_{name}", worst_err_over_bound=ratio, K=K)
    assert ratio <= 1.0, ratio


def run_grouped(ops, problems, K, accumulate, seed, fill=LOUD, integers=True, a_geom=None, test=""):
    lib = ops.load_lib()
    probs = (_lib.GemmProblem * len(problems))()
    keep, outs = [], []
    for i, (M, N) in enumerate(problems):
        a, b, r = (G.int_operands if integers else random_operands)(M, N, K, True, True, accumulate, seed + i)
        va, vb = place(a, fill, a_geom or WIN), place(b, fill)
        c = Out(M, N, init=r)
        keep.append((va, vb))
        outs.append((c, a, b, r))
        probs[i] = _lib.GemmProblem(ptr(va), ptr(vb), ptr(c.view), va.stride(0), vb.stride(0), c.view.stride(0), M, N)
    rc, syms = profiled(ops, lambda: lib.sd_gemm_grouped_tn(ctypes.cast(probs, ctypes.c_void_p), len(problems), K,
                                                            int(accumulate), stream()))
    want = f"gemm_pgroup_tn_kernel<{'true' if accumulate else 'false'}>"
    assert rc == OK and syms == [want], (rc, syms)
    note(test, want)
    return [(c.got(), a, b, r) for c, a, b, r in outs]


@pytest.mark.parametrize("accumulate", [False, True])
def test_views_grouped_tn(ops, accumulate):
    f = G.BY_NAME[f"grouped_tn_acc{int(accumulate)}"]
    for n in (4, 1):
        for got, a, b, r in run_grouped(ops, f["problems"][:n], 200, accumulate, seed=n, test=f["name"]):
            same_bits(got, G.int_expect(a, b, True, True, r), f"{f['name']} n={n} {tuple(got.shape)}")
    worst = max(G.worst_ratio(got, a, b, True, True, r, 200)
                for got, a, b, r in run_grouped(ops, f["problems"], 200, accumulate, seed=9, integers=False, test=f["name"]))
    record(f"gemm_views_random_{f['name']}", worst_err_over_bound=worst, K=200)
    assert worst <= 1.0, worst


def test_views_splitk_partial(ops):
    """sd_gemm_bf16_splitk_partial writes exactly nsplit * M * N floats (their sum is the product) and leaves C alone; with
    nsplit == 1 it writes none of them and the bf16 C instead."""
    lib = ops.load_lib()
    f = G.BY_NAME["splitk_partial"]
    for (M, N, K), sym in ((f["shape"], f["symbol"]), ((200, 136, 72), None)):
        a, b, _ = G.int_operands(M, N, K, False, True, False, seed=K)
        va, vb, c = place(a, LOUD), place(b, LOUD), Out(M, N)
        nsplit = lib.sd_gemm_splitk_plan(M, N, K)
        assert (nsplit > 1) == (sym is not None)
        ws = Out((nsplit + 1) * M, N, ROWS, torch.float32)  # room for one slab more than planned: it must stay
        nsp = ctypes.c_int(0)
        plan = _lib.gemm_plan(M, N, K, False, True, lda=va.stride(0), ldb=vb.stride(0), ldc=c.view.stride(0), split_k=True,
                              cus=cus())["symbol"]
        rc, syms = profiled(ops, lambda: lib.sd_gemm_bf16_splitk_partial(
            ptr(va), ptr(vb), ptr(c.view), M, N, K, va.stride(0), vb.stride(0), c.view.stride(0), 0, 1, ptr(ws.view),
            (nsplit + 1) * M * N * 4, ctypes.cast(ctypes.byref(nsp), ctypes.c_void_p), stream()))
        assert rc == OK and syms == [plan] and nsp.value == nsplit, (rc, syms, nsp.value)
        if sym is not None and cus() == 256:
            assert plan == sym
        note(f["name"], plan)
        slabs, want = ws.got(), G.ref64(a, b, False, True)
        if nsplit > 1:
            c.assert_untouched()
            written = G.bits(slabs) != G.SENTINEL_BITS[torch.float32]
            assert bool(written[:nsplit * M].all()) and not bool(written[nsplit * M:].any())
            assert torch.equal(slabs[:nsplit * M].double().view(nsplit, M, N).sum(0), want)
        else:
            ws.assert_untouched()
            same_bits(c.got(), want.float().bfloat16(), "splitk_partial, one slice")


# ------------------------------------------------------------------------------ 2. write bounds of the fused outputs
def int_mat(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (rows, cols), generator=g).float()
    x[0, :] += 1.0
    return x.to(BF)


def fused_call(ops, f, call):
    plan = _lib.gemm_plan(**G.plan_query(f, False), cus=cus())["symbol"]
    rc, syms = profiled(ops, call)
    assert rc == OK and syms == [plan], (rc, syms, plan)
    if cus() == 256:
        assert plan == f["symbol"], (plan, f["symbol"])
    note(f["name"], plan)


@pytest.mark.parametrize("name", [f["name"] for f in G.FAMILIES if f["entry"] == "swiglu"])
def test_fused_swiglu_write_bounds(ops, name):
    f = G.BY_NAME[name]
    lib, (M, K, I) = ops.load_lib(), (f["dims"][k] for k in "MKI")
    x, w = int_mat(M, K, 1), int_mat(2 * I, K, 2)
    xd, wd = x.to(dev()), w.to(dev())
    gu, act, act2 = Out(M, 2 * I, ROWS), Out(M, I, ROWS), Out(M, I, ROWS)
    with switched(f["switches"]):
        fused_call(ops, f, lambda: lib.sd_gemm_swiglu(ptr(xd), ptr(wd), ptr(gu.view), ptr(act.view), M, I, K, stream()))
        got_gu, got_act = gu.got(), act.got()
        spare = Out(M, 2 * I, ROWS)  # save_gu = False (C = NULL): no gate|up is written anywhere
        fused_call(ops, f, lambda: lib.sd_gemm_swiglu(ptr(xd), ptr(wd), 0, ptr(act2.view), M, I, K, stream()))
        spare.assert_untouched()
    same_bits(got_gu, G.int_expect(x, w, False, False), name + " gate|up")
    want = ops.swiglu_fwd(got_gu.to(dev())).cpu()
    same_bits(got_act, want, name + " act")
    same_bits(act2.got(), want, name + " act, save_gu=False")
    assert G.first_diff(gu.parent, gu.before) is not None


@pytest.mark.parametrize("name", [f["name"] for f in G.FAMILIES if f["entry"] == "qkv_rope"])
def test_fused_qkv_rope_write_bounds(ops, name):
    f = G.BY_NAME[name]
    lib, d = ops.load_lib(), f["dims"]
    M, T, K, Hq, Hkv = d["M"], d["T"], d["K"], d["Hq"], d["Hkv"]
    NQ, NK = (Hq + 2 * Hkv) * 128, (Hq + Hkv) * 128
    g = torch.Generator().manual_seed(4)
    x, w = int_mat(M, K, 3), int_mat(NQ, K, 4)
    qg, kg = ((1 + 0.2 * torch.randn(128, generator=g)).to(BF).to(dev()) for _ in range(2))
    cos, sin = ops.rope_tables(T, dev())
    xd, wd = x.to(dev()), w.to(dev())
    qkv, qk = Out(M, NQ, ROWS), Out(M, NK, ROWS)
    with switched(f["switches"]):
        fused_call(ops, f, lambda: lib.sd_gemm_qkv_rope(ptr(xd), ptr(wd), ptr(qkv.view), ptr(qk.view), ptr(qg), ptr(kg), ptr(cos),
                                                        ptr(sin), M, T, Hq, Hkv, K, 1e-6, stream()))
    got = qkv.got()
    same_bits(got, G.int_expect(x, w, False, False), name + " q|k|v")
    same_bits(qk.got(), ops.qknorm_rope_fwd(got.to(dev()), qg, kg, cos, sin, T, Hq, Hkv).cpu(), name + " rotated q|k")


@pytest.mark.parametrize("name", [f["name"] for f in G.FAMILIES if f["entry"] == "swiglu_bwd"])
def test_fused_swiglu_bwd_write_bounds(ops, name):
    f = G.BY_NAME[name]
    lib, (M, H, I) = ops.load_lib(), (f["dims"][k] for k in "MHI")
    dy, w = int_mat(M, H, 5), int_mat(H, I, 6)
    gate_up = torch.randn(M, 2 * I, generator=torch.Generator().manual_seed(7)).to(BF).to(dev())
    dyd, wd = dy.to(dev()), w.to(dev())
    dgu = Out(M, 2 * I, ROWS)
    with switched(f["switches"]):
        fused_call(ops, f, lambda: lib.sd_gemm_swiglu_bwd(ptr(dyd), ptr(wd), ptr(gate_up), ptr(dgu.view), M, I, H, stream()))
    dact = G.int_expect(dy, w, False, True).to(dev())
    same_bits(dgu.got(), ops.swiglu_bwd(dact, gate_up).cpu(), name)


@pytest.mark.parametrize("name", [f["name"] for f in G.FAMILIES if f["entry"] == "odx_delta"])
def test_fused_odx_delta_write_bounds(ops, name):
    f = G.BY_NAME[name]
    lib, d = ops.load_lib(), f["dims"]
    M, T, Hq, H = d["M"], d["T"], d["Hq"], d["H"]
    QD = Hq * 128
    dy, w, o = int_mat(M, H, 8), int_mat(H, QD, 9), int_mat(M, QD, 10)
    dyd, wd, ov = dy.to(dev()), w.to(dev()), place(o, LOUD)  # o has a leading dimension of its own: a window
    dao, delta = Out(M, QD, ROWS), Out(1, M * Hq, ROWS, torch.float32)
    with switched(f["switches"]):
        fused_call(ops, f, lambda: lib.sd_gemm_odx_delta(ptr(dyd), ptr(wd), ptr(dao.view), ptr(ov), ov.stride(0), ptr(delta.view),
                                                         M, T, Hq, H, stream()))
    want = G.int_expect(dy, w, False, True)
    same_bits(dao.got(), want, name + " d_ao")
    # integer products: the fp32 row sums are exact in any order (|d_ao * o| <= 4 * 4112, 128 terms)
    dsum = (want.double() * o.double()).view(M // T, T, Hq, 128).sum(-1).permute(0, 2, 1).reshape(1, -1)
    same_bits(delta.got(), dsum.float(), name + " delta")


@pytest.mark.parametrize("name", [f["name"] for f in G.FAMILIES if f["entry"] == "ssq"])
def test_fused_ssq_write_bounds(ops, name):
    f = G.BY_NAME[name]
    lib, (M, N, K) = ops.load_lib(), (f["dims"][k] for k in "MNK")
    a, b, r = G.int_operands(M, N, K, False, False, True, seed=11)
    va, vb, vr = place(a, LOUD), place(b, LOUD), place(r, LOUD)
    c, ssq = Out(M, N), Out(1, (N // 128) * M, ROWS, torch.float32)
    with switched(f["switches"]):
        fused_call(ops, f, lambda: lib.sd_gemm_bf16_ssq(ptr(va), ptr(vb), ptr(c.view), ptr(vr), ptr(ssq.view), M, N, K, va.stride(0),
                                                        vb.stride(0), c.view.stride(0), vr.stride(0), stream()))
    got = c.got()
    same_bits(got, G.int_expect(a, b, False, False, r), name + " C")
    want = got.double().view(M, N // 128, 128).pow(2).sum(-1).t().reshape(1, -1)  # tile-major [N / 128][M]
    np.testing.assert_allclose(ssq.got().double().numpy(), want.numpy(), rtol=1e-5)


# ------------------------------------------------------------------------------------------- 3. odd and tiny K
ODD_K = [1, 7, 63, 64, 65, 129, 515]
TN_KERNELS = [(64, 3), (128, 2), (256, 3), (256, 9)]
STAGE1 = (40, 40, GUARD)  # A = wide[:, r0:]: a column window that ends with its parent's row (the lm_head dW of Stage 1)


@pytest.mark.parametrize("K", ODD_K)
def test_tn_odd_k(ops, K):
    """The contraction length of a weight gradient is a token count: any number.  Both operands transposed, so the staging
    relies on the hardware range check ending exactly at row K - 1 of each operand's window."""
    M, N = 520, 264
    a, b, r = G.int_operands(M, N, K, True, True, True, seed=K)
    want, want_r = G.int_expect(a, b, True, True), G.int_expect(a, b, True, True, r)
    for bm, nst in TN_KERNELS:
        stag = nst == 9
        sym = "gemm_stag_kernel<true, true, %d>" if stag else f"gemm_bf16_kernel<{bm}, {nst}, true, true, %d, true>"
        with switched(G.force(bm, nst)):
            run_gemm(ops, M, N, K, True, True, a, b, symbol=sym % 0, test="tn_odd_k", expect=want)
            run_gemm(ops, M, N, K, True, True, a, b, r, alias=True, symbol=sym % 1, test="tn_odd_k", expect=want_r)
            run_gemm(ops, M, N, K, True, True, a, b, a_geom=STAGE1, symbol=sym % 0, test="tn_odd_k", expect=want)
            run_gemm(ops, M, N, K, True, True, a, b, fill=NAN, symbol=sym % 0, test="tn_odd_k", expect=want)


@pytest.mark.parametrize("K", ODD_K)
def test_tn_odd_k_persistent(ops, K):
    M, N = 1000, 128 * 83 + 40
    a, b, _ = G.int_operands(M, N, K, True, True, False, seed=K)
    with switched(G.STAG):
        run_gemm(ops, M, N, K, True, True, a, b, a_geom=STAGE1, symbol="gemm_pstag_kernel<4, true, true, 0>",
                 test="tn_odd_k_persistent", expect=G.int_expect(a, b, True, True))


@pytest.mark.parametrize("K", ODD_K)
def test_tn_odd_k_grouped(ops, K):
    for accumulate in (False, True):
        for got, a, b, r in run_grouped(ops, G.GROUPED_PROBLEMS, K, accumulate, seed=K, a_geom=STAGE1, test="tn_odd_k_grouped"):
            same_bits(got, G.int_expect(a, b, True, True, r), f"grouped K={K} acc={accumulate} {tuple(got.shape)}")


@pytest.mark.parametrize("K", [8, 56, 72, 136])
@pytest.mark.parametrize("lay", ["nt", "nn", "ta"])
def test_small_k_every_tile_and_ring_depth(ops, lay, K):
    """fewer K tiles than ring stages, a K tail of 8 and of 56, on every tile and ring depth (and the staggered tile)"""
    ta, tb = G.LAYOUTS[lay]
    M, N = 520, 264
    a, b, _ = G.int_operands(M, N, K, ta, tb, False, seed=K)
    want = G.int_expect(a, b, ta, tb)
    for bm, nst in G.VARIANTS + [(256, 9)]:
        with switched(G.force(bm, nst)):
            run_gemm(ops, M, N, K, ta, tb, a, b, test="small_k", expect=want)


# --------------------------------------------------------------------------------------------- 4. M and N edges
@pytest.mark.parametrize("lay,Ms", [("nt", (1, 7, 8, 257)), ("nn", (1, 7, 8, 257)), ("ta", (8, 264)), ("tn", (8, 264))])
def test_m_and_n_edges(ops, lay, Ms):
    ta, tb = G.LAYOUTS[lay]
    for M in Ms:
        for N in (8, 136):
            for K in (64, 72):
                a, b, r = G.int_operands(M, N, K, ta, tb, True, seed=M + N)
                want = G.int_expect(a, b, ta, tb, r)
                for bm, nst in ((64, 4), (128, 3), (256, 3)):
                    with switched(G.force(bm, nst)):
                        run_gemm(ops, M, N, K, ta, tb, a, b, r, test="edges", expect=want)
                        run_gemm(ops, M, N, K, ta, tb, a, b, r, alias=True, test="edges", expect=want)


# --------------------------------------------------------------------------------------- 5. non-finite neighbours
NEIGHBOUR_KERNELS = [{}, G.force(64, 3), G.force(128, 3), G.force(256, 3), G.STAG]


@pytest.mark.parametrize("lay,K", [(lay, K) for lay in ("nn", "ta", "nt") for K in (8, 72, 200)] + [("nn", 192), ("tn", 200)])
def test_non_finite_neighbours(ops, lay, K):
    """C[m][n] depends on its own operand rows only.  (a) windows whose gaps and guards hold NaN, then Inf; (b) contiguous
    operands whose rows behind row m of op(A) and row n of op(B) hold Inf: C[:m + 1, :n + 1] keeps the finite result's bits.
    A kernel that stages a K-contiguous row on past K, up to the end of its K tile, multiplies what lies there by the other
    operand's zeros: NaN.  That is what buffer-descriptor staging did for NN and ta=1,tb=0 at K = 8, 72 and 200 (NaN from
    element (0, 0) on, in (a) and (b), on every kernel) while gemm_plan took it whenever ONE operand was transposed; NT (pointer
    staging), NN at K = 192 and TN at K = 200 were right then as now."""
    ta, tb = G.LAYOUTS[lay]
    M, N, m, n = 200, 136, 76, 49
    a, b, _ = G.int_operands(M, N, K, ta, tb, False, seed=K)
    want = G.int_expect(a, b, ta, tb)
    ai, bi = a.clone(), b.clone()
    if ta:
        ai[:, m + 1:] = float("inf")
    else:
        ai[m + 1:] = float("inf")
    if tb:
        bi[:, n + 1:] = float("inf")
    else:
        bi[n + 1:] = float("inf")
    for switches in NEIGHBOUR_KERNELS:
        with switched(switches):
            for fill in (NAN, INF):
                run_gemm(ops, M, N, K, ta, tb, a, b, fill=fill, test="neighbours", expect=want)
            got = run_gemm(ops, M, N, K, ta, tb, ai, bi, geom=FLAT, test="neighbours")
        same_bits(got[:m + 1, :n + 1], want[:m + 1, :n + 1], f"rows behind ({m}, {n}) are Inf, {lay} K={K} {switches}")


# -------------------------------------------------------------------------------------------------- 6. refusals
def refused(ops, code, call, outs):
    rc, _ = profiled(ops, call)
    assert rc == code, (rc, code)
    assert ops.prof_symbols() == {}, ops.prof_symbols()
    for o in outs:
        o.assert_untouched()


BAD_ARGS = [  # what to break, the code check_args gives
    (dict(A=2), ERR_ALIGN), (dict(B=2), ERR_ALIGN), (dict(C=2), ERR_ALIGN), (dict(R=2), ERR_ALIGN),
    (dict(lda=4), ERR_ALIGN), (dict(ldb=4), ERR_ALIGN), (dict(ldc=4), ERR_ALIGN), (dict(ldr=4), ERR_ALIGN),
    (dict(N=60), ERR_ALIGN), (dict(K=60), ERR_ALIGN), (dict(K=60, tb=1), ERR_ALIGN), (dict(K=60, ta=1), ERR_ALIGN),
    (dict(M=60, ta=1, tb=1), ERR_ALIGN), (dict(M=60, ta=1), ERR_ALIGN),
    (dict(M=0), ERR_SHAPE), (dict(N=0), ERR_SHAPE), (dict(K=0), ERR_SHAPE), (dict(M=-8), ERR_SHAPE), (dict(N=-8), ERR_SHAPE),
    (dict(K=-64), ERR_SHAPE),
]


@pytest.mark.parametrize("entry", ["sd_gemm_bf16", "sd_gemm_bf16_splitk", "sd_gemm_bf16_splitk_partial", "sd_gemm_bf16_ssq"])
def test_refusals_leave_c_alone(ops, entry):
    lib = ops.load_lib()
    S = 512 if entry.endswith("ssq") else 64
    x = int_mat(S, S, 1)
    va, vb, vr = place(x, LOUD), place(x, LOUD), place(x, LOUD)
    c, ws, nsp = Out(S, S), Out(4 * S, S, ROWS, torch.float32), ctypes.c_int(0)

    def call(A=0, B=0, C=0, R=0, M=S, N=S, K=S, lda=0, ldb=0, ldc=0, ldr=0, ta=0, tb=0, no_r=False):
        pa, pb, pc, pr = ptr(va) + A, ptr(vb) + B, ptr(c.view) + C, 0 if no_r else ptr(vr) + R
        la, lb, lc, lr = va.stride(0) + lda, vb.stride(0) + ldb, c.view.stride(0) + ldc, vr.stride(0) + ldr
        if entry == "sd_gemm_bf16":
            return lib.sd_gemm_bf16(pa, pb, pc, pr, M, N, K, la, lb, lc, lr, ta, tb, stream())
        if entry == "sd_gemm_bf16_splitk":
            return lib.sd_gemm_bf16_splitk(pa, pb, pc, pr, M, N, K, la, lb, lc, lr, ta, tb, ptr(ws.view), 4 * S * S * 4, stream())
        if entry == "sd_gemm_bf16_splitk_partial":
            return lib.sd_gemm_bf16_splitk_partial(pa, pb, pc, M, N, K, la, lb, lc, ta, tb, ptr(ws.view), 4 * S * S * 4,
                                                   ctypes.cast(ctypes.byref(nsp), ctypes.c_void_p), stream())
        return lib.sd_gemm_bf16_ssq(pa, pb, pc, pr, ptr(ws.view), M, N, K, la, lb, lc, lr, stream())

    n = 0
    for bad, code in BAD_ARGS:
        if entry.endswith("partial") and ("R" in bad or "ldr" in bad):
            continue  # no residual in this entry
        if entry.endswith("ssq") and ("ta" in bad or "tb" in bad):
            continue  # NT only
        refused(ops, code, lambda: call(**bad), [c, ws])
        n += 1
    if entry.endswith("ssq"):
        refused(ops, ERR_UNSUPPORTED, lambda: call(no_r=True), [c, ws])
        refused(ops, ERR_UNSUPPORTED, lambda: call(N=384), [c, ws])  # N / 128 is no multiple of 4
        n += 2
    assert n >= 14
    assert call() == OK  # and the unbroken call is accepted
    torch.cuda.synchronize()


def test_refusals_grouped_tn(ops):
    lib = ops.load_lib()
    K, shapes = 64, [(64, 128), (128, 64)]
    va = [place(int_mat(K, M, i), LOUD) for i, (M, _) in enumerate(shapes)]
    vb = [place(int_mat(K, N, 5 + i), LOUD) for i, (_, N) in enumerate(shapes)]
    cs = [Out(M, N) for M, N in shapes]

    def call(n=2, K=K, accumulate=0, null=False, **bad):
        probs = (_lib.GemmProblem * 5)()
        for i in range(5):
            j = i % 2
            q = dict(A=ptr(va[j]), B=ptr(vb[j]), C=ptr(cs[j].view), lda=va[j].stride(0), ldb=vb[j].stride(0),
                     ldc=cs[j].view.stride(0), M=shapes[j][0], N=shapes[j][1])
            if i == 1:
                for k, v in bad.items():
                    q[k] += v
            probs[i] = _lib.GemmProblem(*(q[k] for k in ("A", "B", "C", "lda", "ldb", "ldc", "M", "N")))
        return lib.sd_gemm_grouped_tn(0 if null else ctypes.cast(probs, ctypes.c_void_p), n, K, accumulate, stream())

    for kw, code in [(dict(n=0), ERR_SHAPE), (dict(n=5), ERR_SHAPE), (dict(n=-1), ERR_SHAPE), (dict(K=0), ERR_SHAPE),
                     (dict(K=-8), ERR_SHAPE), (dict(null=True), ERR_SHAPE),
                     (dict(A=2), ERR_ALIGN), (dict(B=2), ERR_ALIGN), (dict(C=2), ERR_ALIGN), (dict(lda=4), ERR_ALIGN),
                     (dict(ldb=4), ERR_ALIGN), (dict(ldc=4), ERR_ALIGN), (dict(M=-4), ERR_ALIGN), (dict(N=-4), ERR_ALIGN),
                     (dict(M=-128), ERR_ALIGN), (dict(N=-64), ERR_ALIGN)]:
        for accumulate in (0, 1):
            refused(ops, code, lambda: call(accumulate=accumulate, **kw), cs)
    assert call() == OK
    torch.cuda.synchronize()


def test_refusals_fused_entries(ops):
    """the fused entry points: a misaligned pointer is SD_ERR_ALIGN, a shape the epilogue cannot run SD_ERR_UNSUPPORTED (the
    callers then run the two-kernel form), both before any launch.  A K tail with a K-contiguous operand is such a shape:
    the fused epilogues have no pointer-staging form."""
    lib = ops.load_lib()
    M, K, I, T, Hq, Hkv = 64, 128, 128, 32, 2, 1
    NQ, NK = (Hq + 2 * Hkv) * 128, (Hq + Hkv) * 128
    big = place(int_mat(264, 520, 1), LOUD)  # every input pointer: large enough for each call below, were it launched
    outs = [Out(M, 520, ROWS), Out(M, 520, ROWS), Out(1, 1024, ROWS, torch.float32)]
    o1, o2, o3 = (ptr(o.view) for o in outs)
    p, st = ptr(big), stream()
    cases = [
        (lambda: lib.sd_gemm_swiglu(p + 2, p, o1, o2, M, I, K, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_swiglu(p, p, o1 + 2, o2, M, I, K, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_swiglu(p, p, o1, o2 + 2, M, I, K, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_swiglu(p, p, o1, o2, M, 100, K, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_swiglu(p, p, o1, o2, M, I, 72, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_swiglu(p, p, o1, o2, 0, I, K, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_swiglu(p, p, o1, o2, M, -64, K, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_qkv_rope(p + 2, p, o1, o2, p, p, p, p, M, T, Hq, Hkv, K, 1e-6, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_qkv_rope(p, p, o1, o2 + 2, p, p, p, p, M, T, Hq, Hkv, K, 1e-6, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_qkv_rope(p, p, o1, o2, p, p, p, p, M, T, Hq, Hkv, 72, 1e-6, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_qkv_rope(p, p, o1, o2, p, p, p, p, M, 48, Hq, Hkv, K, 1e-6, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_qkv_rope(p, p, o1, o2, p, p, p, p, 0, T, Hq, Hkv, K, 1e-6, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_qkv_rope(p, p, o1, 0, p, p, p, p, M, T, Hq, Hkv, K, 1e-6, st), ERR_UNSUPPORTED),
        # the folded-RMSNorm forms without their row statistic
        (lambda: lib.sd_gemm_swiglu_rs(p, p, o1, o2, 0, 1e-6, M, I, K, st), ERR_SHAPE),
        (lambda: lib.sd_gemm_qkv_rope_rs(p, p, o1, o2, p, p, p, p, 0, M, T, Hq, Hkv, K, 1e-6, st), ERR_SHAPE),
        (lambda: lib.sd_gemm_swiglu_rs(p, p, o1, o2, p, 1e-6, M, I, 192, st), ERR_UNSUPPORTED),  # K / 128 must be 4, 8, 12 or 16
        (lambda: lib.sd_gemm_swiglu_bwd(p + 2, p, p, o1, M, I, K, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_swiglu_bwd(p, p, p, o1 + 2, M, I, K, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_swiglu_bwd(p, p, p, o1, M, 100, K, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_swiglu_bwd(p, p, p, o1, M, I, 60, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_swiglu_bwd(p, p, p, o1, M, I, 72, st), ERR_UNSUPPORTED),   # a K tail: no descriptor staging
        (lambda: lib.sd_gemm_swiglu_bwd(p, p, p, o1, -8, I, K, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_odx_delta(p + 2, p, o1, p, 520, o3, M, T, Hq, K, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_odx_delta(p, p, o1, p, 520, o3 + 4, M, T, Hq, K, st), ERR_ALIGN),
        (lambda: lib.sd_gemm_odx_delta(p, p, o1, p, 524, o3, M, T, Hq, K, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_odx_delta(p, p, o1, p, 520, o3, M, 48, Hq, K, st), ERR_UNSUPPORTED),
        (lambda: lib.sd_gemm_odx_delta(p, p, o1, p, 520, o3, M, T, Hq, 72, st), ERR_UNSUPPORTED),  # a K tail again
        (lambda: lib.sd_gemm_odx_delta(p, p, o1, p, 520, o3, M, T, 0, K, st), ERR_UNSUPPORTED),
    ]
    for call, code in cases:
        refused(ops, code, call, outs)
    assert NQ <= 520 and NK <= 520 and 2 * I <= 520
