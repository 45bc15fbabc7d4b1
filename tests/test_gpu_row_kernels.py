"""-m gpu: the row kernels of sd_elementwise.hip (RMSNorm, q/k-norm + RoPE, SwiGLU, embedding gather / scatter-add,
rows_scatter, the column-sum reducers) against fp64 references, per element, on every launcher path.

tests/rowk_ref.py holds the references, the bounds, the case tables and the restated launcher decisions;
tests/test_rowk_ref_cpu.py shows on the CPU that the rules reject wrong formulas and that each case reaches the path it
is named for.  The launchers are called through the C ABI (ops.load_lib()) because every output here is a view into a
larger buffer: two sentinel rows before and after it must come back intact, and every input sits between NaN rows, so
that a read of a neighbouring row poisons the result.  All accesses stay inside allocations the test owns.
"""
import time

import numpy as np
import pytest
import torch

import rowk_ref as R
from gpu_util import dev, record, to_dev
from parity_ref import rowwise_close
from rowk_ref import BF
from speech_distill_amd import _lib

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENTINEL = -776.0   # exact in bf16
POISON = 555.0      # what an output holds before the launch: an element the kernel skips shows


@pytest.fixture(scope="module")
def ops():
    import speech_distill_amd.ops as ops_
    ops_.load_lib()
    yield ops_
    _lib.debug_set("reset", 0)


@pytest.fixture(scope="module")
def lib(ops):
    return ops.load_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guards:
    """Buffers of one kernel call.  out(): a [rows, cols] view with two sentinel rows on either side; inp(): a copy of a
    CPU tensor between two NaN rows on either side.  intact(): every sentinel row is as it was."""

    def __init__(self):
        self.outs = []

    def out(self, rows, cols, dtype=BF, init=None):
        full = torch.full((rows + 4, cols), SENTINEL, dtype=dtype, device=dev())
        v = full[2:rows + 2]
        v.fill_(POISON) if init is None else v.copy_(init.reshape(rows, cols))
        self.outs.append(full)
        return v

    def inp(self, t):
        t2 = t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t.reshape(1, -1)
        full = torch.full((t2.shape[0] + 4, t2.shape[1]), float("nan"), dtype=t.dtype, device=dev())
        v = full[2:t2.shape[0] + 2]
        v.copy_(t2)
        return v

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((torch.cat([f[:2], f[-2:]]) == SENTINEL).all()) for f in self.outs)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _untouched(v):
    return bool((v == POISON).all())


def _log(name, **verdicts):
    rec = {}
    for k, v in verdicts.items():
        rec[k] = v.err / max(v.bound, 1e-300) if hasattr(v, "worst_rel") else (v.ratio if hasattr(v, "ratio") else v)
    print(name, rec)
    record("parity_rowk_" + name, **rec)


# ------------------------------------------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("M,H", R.RMS_CASES)
def test_rmsnorm_forward(ops, lib, M, H):
    inp = R.rms_inputs(M, H)
    ref = R.rmsnorm_ref(inp["x"], inp["w"])
    g = Guards()
    x, w = g.inp(inp["x"]), g.inp(inp["w"])
    y, rstd = g.out(M, H), g.out(M, 1, F32)
    ops.prof_begin()
    rc = lib.sd_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), M, H, R.EPS, _stream())
    ops.prof_end()
    assert rc == 0 and g.intact()
    assert f"rmsnorm_fwd_kernel<{R.rms_nch(H)}>" in ops.prof_symbols()
    v = R.elem_close(y, ref["y"], R.rmsnorm_fwd_bound(inp["x"], inp["w"], ref))
    rel = float(((rstd.cpu().double()[:, 0] - ref["rstd"]).abs() / ref["rstd"]).max())
    want, _ = R.rmsnorm_fwd_f32(inp["x"], inp["w"], rstd32=ref["rstd"].float())
    share = R.differing_share(y, want)
    _log(f"rmsnorm_fwd_M{M}_H{H}", y=v, rstd_rel_over_bound=rel / R.RSTD_RTOL, rounding_share=share)
    assert v.ok, v
    assert rel <= R.RSTD_RTOL, rel
    assert share <= R.ROUNDING_SHARE, share
    # rstd is nullable
    y2 = g.out(M, H)
    assert lib.sd_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y2.data_ptr(), 0, M, H, R.EPS, _stream()) == 0
    assert torch.equal(y2, y) and g.intact()


def _rms_bwd(ops, lib, name, inp, dres_on, acc):
    M, H = inp["x"].shape
    dres, dw0 = (inp["dres"] if dres_on else None), (inp["dw0"] if acc else None)
    ref = R.rmsnorm_ref(inp["x"], inp["w"], R.rms_grad_of(inp), dres, dw0)
    grid = R.rms_bwd_grid(M, H)
    g = Guards()
    x, w, rstd = g.inp(inp["x"]), g.inp(inp["w"]), g.inp(ref["rstd"].float()[:, None])
    dr = None if dres is None else g.inp(dres)
    dx, dw = g.out(M, H), g.out(1, H, init=dw0)
    ws_rows = lib.sd_rmsnorm_bwd_workspace_bytes(M, H) // (4 * H)
    assert ws_rows >= grid.nb == lib.sd_rmsnorm_bwd_partial_rows(M, H)
    ws = g.out(ws_rows, H, F32)
    ops.prof_begin()
    if inp["slabs"] is None:
        dy = g.inp(inp["dy"])
        rc = lib.sd_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), _p(dr), dx.data_ptr(),
                                dw.data_ptr(), int(acc), ws.data_ptr(), M, H, _stream())
    else:
        ns = inp["slabs"].shape[0]
        sl = g.inp(inp["slabs"].reshape(ns * M, H))
        rc = lib.sd_rmsnorm_bwd_slabs(sl.data_ptr(), ns, x.data_ptr(), w.data_ptr(), rstd.data_ptr(), _p(dr), dx.data_ptr(),
                                      dw.data_ptr(), int(acc), ws.data_ptr(), M, H, 0, 0, _stream())
    ops.prof_end()
    assert rc == 0, f"{name}: sd_rmsnorm_bwd returned {rc} (dynamic LDS {grid.lds_bytes} bytes)"
    assert g.intact()
    label = f"rmsnorm_bwd_kernel<{R.rms_nch(H)}, {'false' if inp['slabs'] is None else 'true'}>"
    assert label in ops.prof_symbols(), (label, list(ops.prof_symbols()))
    vx = rowwise_close(dx, ref["dx"], BF, R.RMS_BWD_FLOOR)
    vw = R.elem_close(dw, ref["dw"][None], R.gain_bound(ref["dw"], ref["dw_n"], ref["dw_abs"])[None])
    _log("rmsnorm_bwd_" + name, dx=vx, dw=vw)
    assert vx.ok, vx
    assert vw.ok, vw
    return g, (x, w, rstd, dx, dw, ws)


_SMALL = [r for r in R.rms_bwd_runs() if r[1]["x"].shape[0] <= 5]
_BIG = [r for r in R.rms_bwd_runs() if r[1]["x"].shape[0] > 5]


@pytest.mark.parametrize("run", _SMALL, ids=[r[0] for r in _SMALL])
def test_rmsnorm_backward_small(ops, lib, run):
    """Every NCH with a full and a partial last chunk, idle waves (M < 4), one wave with a second workgroup (M = 5);
    H = 4096 asks for exactly 64 KB of dynamic LDS."""
    _rms_bwd(ops, lib, *run)


@pytest.mark.parametrize("run", _BIG, ids=[r[0] for r in _BIG])
def test_rmsnorm_backward_row_loop(ops, lib, run):
    """More than one row per wave, a short last workgroup, dres on / off, accumulate_dw 0 / 1; the slab form."""
    _rms_bwd(ops, lib, *run)


def test_rmsnorm_refusals_leave_the_output_alone(ops, lib):
    for H, want in R.RMS_REFUSED.items():
        g = Guards()
        M = 3
        x, w, dy = (g.inp(torch.ones(M, H, dtype=BF)) for _ in range(3))
        rstd = g.inp(torch.ones(M, 1))
        y, dx, dw, r_out = g.out(M, H), g.out(M, H), g.out(1, H), g.out(M, 1, F32)
        ws = g.out(4, H, F32)
        assert lib.sd_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), r_out.data_ptr(), M, H, R.EPS, _stream()) == want
        assert lib.sd_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), 0, dx.data_ptr(), dw.data_ptr(),
                                  0, ws.data_ptr(), M, H, _stream()) == want
        assert g.intact() and all(_untouched(t) for t in (y, dx, dw, r_out, ws))
    # a slab pointer that is not 16-byte aligned
    inp = R.rms_inputs(5, 136, 1)
    g = Guards()
    x, w, rstd = g.inp(inp["x"]), g.inp(inp["w"]), g.inp(torch.ones(5, 1))
    sl = g.inp(torch.zeros(6, 136))
    dx, dw, ws = g.out(5, 136), g.out(1, 136), g.out(2, 136, F32)
    rc = lib.sd_rmsnorm_bwd_slabs(sl.data_ptr() + 4, 1, x.data_ptr(), w.data_ptr(), rstd.data_ptr(), 0, dx.data_ptr(),
                                  dw.data_ptr(), 0, ws.data_ptr(), 5, 136, 0, 0, _stream())
    assert rc == -1 and g.intact() and all(_untouched(t) for t in (dx, dw, ws))


# ------------------------------------------------------------------------------------------------- q/k norm + RoPE
def _qk_dev(g, inp):
    return {k: g.inp(inp[k]) for k in ("qkv", "qg", "kg", "cos", "sin", "dout")}


@pytest.mark.parametrize("case", R.QK_CASES, ids=str)
def test_qknorm_rope_forward(ops, lib, case):
    B, T, Hq, Hkv = case
    M, nh = B * T, Hq + Hkv
    inp = R.qk_inputs(*case)
    ref = R.qk_ref(inp, T, Hq, Hkv)
    g = Guards()
    d = _qk_dev(g, inp)
    out = g.out(M, nh * 128)
    rc = lib.sd_qknorm_rope_fwd(d["qkv"].data_ptr(), d["qg"].data_ptr(), d["kg"].data_ptr(), d["cos"].data_ptr(),
                                d["sin"].data_ptr(), out.data_ptr(), M, T, Hq, Hkv, R.EPS, _stream())
    assert rc == 0 and g.intact()
    v = R.elem_close(out, ref["out"], R.qk_fwd_bound(inp, T, Hq, Hkv))
    share = R.differing_share(out, R.qk_fwd_f32(inp, T, Hq, Hkv, rstd32=R.qk_rstd64(inp, Hq, Hkv).float()))
    _log(f"qk_fwd_{B}_{T}_{Hq}_{Hkv}", out=v, rounding_share=share)
    assert v.ok, v
    assert share <= R.ROUNDING_SHARE, share


@pytest.mark.parametrize("case", list(R.QK_BWD_CASES), ids=str)
@pytest.mark.parametrize("acc", [False, True])
def test_qknorm_rope_backward(ops, lib, case, acc):
    B, T, Hq, Hkv, blocks = case
    M, nh, nqkv = B * T, Hq + Hkv, Hq + 2 * Hkv
    inp = R.qk_inputs(B, T, Hq, Hkv)
    ref = R.qk_ref(inp, T, Hq, Hkv, backward=True, accumulate=acc)
    grid = R.qk_bwd_grid(M * nh, blocks)
    g = Guards()
    d = _qk_dev(g, inp)
    pattern = ((torch.arange(M * Hkv * 128) % 251) - 125).float().view(M, Hkv * 128).to(BF)
    init = torch.full((M, nqkv * 128), POISON, dtype=BF)
    init[:, nh * 128:] = pattern
    dqkv = g.out(M, nqkv * 128, init=init)
    dqg, dkg = g.out(1, 128, init=inp["dqg0"] if acc else None), g.out(1, 128, init=inp["dkg0"] if acc else None)
    try:
        if blocks:
            _lib.debug_set("qk_bwd.blocks", blocks)
        assert lib.sd_qknorm_rope_bwd_partial_rows(M, Hq, Hkv) == grid.nb
        assert lib.sd_qknorm_rope_bwd_workspace_bytes(M, Hq, Hkv) == grid.nb * 256 * 4
        ws = g.out(grid.nb, 256, F32)
        rc = lib.sd_qknorm_rope_bwd(d["dout"].data_ptr(), d["qkv"].data_ptr(), d["qg"].data_ptr(), d["kg"].data_ptr(),
                                    d["cos"].data_ptr(), d["sin"].data_ptr(), dqkv.data_ptr(), dqg.data_ptr(), dkg.data_ptr(),
                                    int(acc), ws.data_ptr(), M, T, Hq, Hkv, R.EPS, _stream())
        torch.cuda.synchronize()
    finally:
        if blocks:
            _lib.debug_set("qk_bwd.blocks", 0)
    assert rc == 0 and g.intact()
    assert torch.equal(dqkv[:, nh * 128:].cpu(), pattern), "the v columns of dqkv were touched"
    vx = rowwise_close(dqkv[:, :nh * 128].reshape(-1, 128), ref["dqk"].reshape(-1, 128), BF, R.QK_BWD_FLOOR)
    vq = R.elem_close(dqg, ref["dqg"][None], R.gain_bound(ref["dqg"], ref["dqg_n"], ref["dqg_abs"])[None])
    vk = R.elem_close(dkg, ref["dkg"][None], R.gain_bound(ref["dkg"], ref["dkg_n"], ref["dkg_abs"])[None])
    _log(f"qk_bwd_{B}_{T}_{Hq}_{Hkv}_blocks{blocks}_acc{int(acc)}", dqkv=vx, dq_gain=vq, dk_gain=vk)
    assert vx.ok, vx
    assert vq.ok, vq
    assert vk.ok, vk


# ------------------------------------------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("M,I", R.SWIGLU_CASES)
def test_swiglu(ops, lib, M, I):
    gu_c, d_c, exempt = R.swiglu_inputs(M, I)
    ref = R.swiglu_ref(gu_c, d_c)
    g = Guards()
    gu, dact = g.inp(gu_c), g.inp(d_c)
    act, dgu = g.out(M, I), g.out(M, 2 * I)
    assert lib.sd_swiglu_fwd(gu.data_ptr(), act.data_ptr(), M, I, _stream()) == 0
    assert lib.sd_swiglu_bwd(dact.data_ptr(), gu.data_ptr(), dgu.data_ptr(), M, I, _stream()) == 0
    assert g.intact()
    dgu_c = dgu.cpu()
    va = R.elem_close(act, ref["act"], R.swiglu_bound(ref["act"], ref["act_mag"], exempt))
    vg = R.elem_close(dgu_c[:, :I], ref["dg"], R.swiglu_bound(ref["dg"], ref["dg_mag"], exempt))
    vu = R.elem_close(dgu_c[:, I:], ref["du"], R.swiglu_bound(ref["du"], ref["du_mag"], exempt))
    _log(f"swiglu_M{M}_I{I}", act=va, dgate=vg, dup=vu)
    assert va.ok, va
    assert vg.ok, vg
    assert vu.ok, vu


# ------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("H", R.COLSUM_H)
def test_colsum_reduce_batch_loop_boundaries(ops, lib, H):
    """Integer data: the result is the fp64 sum rounded once, whatever the order.  Stride H + 24 with NaN in the padding."""
    for nb in R.COLSUM_NB:
        for acc in (False, True):
            p, o0 = R.colsum_inputs(nb, H)
            g = Guards()
            out = g.out(1, H, init=o0)
            ops.colsum_reduce_batch([(g.inp(p), out[0], H, acc)])
            assert g.intact()
            assert torch.equal(out[0].cpu(), R.colsum_ref(p, o0, H, acc)), (nb, H, acc)
    # a batch of 8 problems in one launch
    g = Guards()
    probs, wants = [], []
    for i, nb in enumerate(R.COLSUM_NB):
        Hi = (H, 8, 40, 72)[i % 4]
        p, o0 = R.colsum_inputs(nb, Hi, seed=i + 1)
        out = g.out(1, Hi, init=o0)
        probs.append((g.inp(p), out[0], Hi, bool(i & 1)))
        wants.append(R.colsum_ref(p, o0, Hi, bool(i & 1)))
    ops.colsum_reduce_batch(probs)
    assert g.intact()
    for (_, out, _, _), want in zip(probs, wants):
        assert torch.equal(out.cpu(), want)
    record(f"parity_rowk_colsum_batch_H{H}", exact=True)


@pytest.mark.parametrize("H", R.COLSUM_H)
def test_colsum_single_problem_kernel_behind_rmsnorm_bwd(ops, lib, H):
    """M = 4 nb rows give nb workgroups; with integer x and dy, w = 1 and rstd = 1 every partial is an exact integer and
    dw = bf16(dw0 + sum_m dy x)."""
    for nb in R.COLSUM_NB:
        M = 4 * nb
        assert R.rms_bwd_grid(M, H).nb == nb
        gen = torch.Generator().manual_seed(nb * 100 + H)
        xc = torch.randint(-4, 5, (M, H), generator=gen).float().to(BF)
        dyc = torch.randint(-4, 5, (M, H), generator=gen).float().to(BF)
        dw0 = torch.randint(-64, 65, (H,), generator=gen).float().to(BF)
        for acc in (False, True):
            g = Guards()
            x, dy, w, rstd = g.inp(xc), g.inp(dyc), g.inp(torch.ones(H, dtype=BF)), g.inp(torch.ones(M, 1))
            dx, dw, ws = g.out(M, H), g.out(1, H, init=dw0), g.out(nb, H, F32)
            rc = lib.sd_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), 0, dx.data_ptr(),
                                    dw.data_ptr(), int(acc), ws.data_ptr(), M, H, _stream())
            assert rc == 0 and g.intact()
            want = ((dyc.double() * xc.double()).sum(0) + (dw0.double() if acc else 0)).to(BF)
            assert torch.equal(dw[0].cpu(), want), (nb, H, acc)
    record(f"parity_rowk_colsum_single_H{H}", exact=True)


# ------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("M,H", R.EMB_FWD_CASES)
def test_embedding_forward_clamps_ids(ops, lib, M, H):
    V = R.EMB_V
    Ec = torch.randn(V, H, generator=torch.Generator().manual_seed(H + M)).to(BF)
    ids = R.emb_fwd_ids(M, V)
    g = Guards()
    E, x = g.inp(Ec), g.out(M, H)
    ids_d = to_dev(ids)
    assert lib.sd_embedding_fwd(ids_d.data_ptr(), E.data_ptr(), x.data_ptr(), M, H, V, _stream()) == 0
    assert g.intact()
    got = x.cpu()
    assert torch.equal(got, R.emb_fwd_ref(ids, Ec))
    assert torch.equal(got[0], Ec[0]) and (M == 1 or torch.equal(got[M - 1], Ec[V - 1]))  # -3 -> row 0, V + 2 -> row V - 1
    record(f"parity_rowk_embedding_fwd_M{M}_H{H}", exact=True)


@pytest.mark.parametrize("M,H", R.EMB_SSQ_CASES)
def test_embedding_fwd_ssq(ops, lib, M, H):
    V = R.EMB_V
    Ec = torch.randn(V, H, generator=torch.Generator().manual_seed(H + M)).to(BF)
    ids = R.emb_fwd_ids(M, V)
    g = Guards()
    E, x, ssq = g.inp(Ec), g.out(M, H), g.out(H // 128, M, F32)
    ids_d = to_dev(ids)
    assert lib.sd_embedding_fwd_ssq(ids_d.data_ptr(), E.data_ptr(), x.data_ptr(), ssq.data_ptr(), M, H, V, _stream()) == 0
    assert g.intact()
    want = R.emb_fwd_ref(ids, Ec)
    assert torch.equal(x.cpu(), want)
    want_ssq = want.double().view(M, H // 128, 128).pow(2).sum(-1).t()
    np.testing.assert_allclose(ssq.cpu().double().numpy(), want_ssq.numpy(), rtol=1e-5)
    record(f"parity_rowk_embedding_ssq_M{M}_H{H}", ssq_rel=float(((ssq.cpu().double() - want_ssq).abs() / want_ssq).max()))


def test_embedding_fwd_ssq_refusals(ops, lib):
    for H, want in R.EMB_SSQ_REFUSED.items():
        g = Guards()
        E, x, ssq = g.inp(torch.ones(R.EMB_V, H, dtype=BF)), g.out(3, H), g.out(H // 128, 3, F32)
        ids = to_dev(torch.tensor([0, 1, 2]))
        assert lib.sd_embedding_fwd_ssq(ids.data_ptr(), E.data_ptr(), x.data_ptr(), ssq.data_ptr(), 3, H, R.EMB_V, _stream()) == want
        assert g.intact() and _untouched(x) and _untouched(ssq)


@pytest.mark.parametrize("M", R.EMB_BWD_M)
def test_embedding_backward_exact(ops, lib, M):
    """Integer data: dE[id] = bf16(dE0[id] + scale * sum); ids -1 and V are skipped, every other row is unaffected; the
    _range form leaves the rows below row_lo bit-identical."""
    V, H = R.EMB_BWD_V, R.EMB_BWD_H
    ids, dxc, dE0 = R.emb_bwd_inputs(M, H, V)
    ids_d = to_dev(ids)
    for scale in (1.0, 0.5):
        for row_lo in (None, 0, 3, V):
            g = Guards()
            dx, dE = g.inp(dxc), g.out(V, H, init=dE0)
            if row_lo is None:
                rc = lib.sd_embedding_bwd(ids_d.data_ptr(), dx.data_ptr(), dE.data_ptr(), M, H, V, scale, _stream())
            else:
                rc = lib.sd_embedding_bwd_range(ids_d.data_ptr(), dx.data_ptr(), dE.data_ptr(), M, H, V, row_lo, scale, _stream())
            assert rc == 0 and g.intact()
            got = dE.cpu()
            assert torch.equal(got, R.emb_bwd_ref(ids, dxc, dE0, scale, row_lo or 0)), (M, scale, row_lo)
            assert torch.equal(got[:row_lo or 0], dE0[:row_lo or 0])
    record(f"parity_rowk_embedding_bwd_M{M}", exact=True)


def test_embedding_backward_serial_scan(ops, lib):
    """M = 65 537 tokens: one more than the LDS bitmap holds, so every id's row is summed by the serial scan."""
    M, H, V = (R.EMB_SERIAL[k] for k in ("M", "H", "V"))
    assert R.emb_bwd_path(M) == "serial"
    ids, dxc, dE0 = R.emb_bwd_inputs(M, H, V)
    assert int(dxc.float().abs().sum(0).max()) + 16 < 2 ** 24
    g = Guards()
    dx, dE, ids_d = g.inp(dxc), g.out(V, H, init=dE0), to_dev(ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = lib.sd_embedding_bwd(ids_d.data_ptr(), dx.data_ptr(), dE.data_ptr(), M, H, V, 0.5, _stream())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print("embedding_bwd serial scan", ms, "ms")
    record("parity_rowk_embedding_bwd_serial", exact=True, ms=ms)
    assert rc == 0 and g.intact()
    assert torch.equal(dE.cpu(), R.emb_bwd_ref(ids, dxc, dE0, 0.5))


@pytest.mark.parametrize("n,H", R.SCATTER_CASES)
def test_rows_scatter(ops, lib, n, H):
    M = R.SCATTER_M
    src_c = (torch.randn(max(n, 1), H, generator=torch.Generator().manual_seed(n + H)) + 3).to(BF)
    rows = R.scatter_rows(n, M)
    g = Guards()
    src, dst = g.inp(src_c), g.out(M, H)
    rows_d = to_dev(rows) if n else to_dev(torch.zeros(1, dtype=torch.int64))
    assert lib.sd_rows_scatter(src.data_ptr(), rows_d.data_ptr(), dst.data_ptr(), n, M, H, _stream()) == 0
    assert g.intact()
    want = R.scatter_ref(src_c[:n], rows, M)
    assert torch.equal(dst.cpu(), want)
    if n:
        keep = (rows >= 0) & (rows < M)
        assert torch.equal(ops.rows_scatter(to_dev(src_c[:n][keep]), to_dev(rows[keep]), M).cpu(), want)
    record(f"parity_rowk_rows_scatter_n{n}_H{H}", exact=True)
