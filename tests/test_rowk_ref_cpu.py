"""CPU only: the acceptance rules of tests/rowk_ref.py (the references of tests/test_gpu_row_kernels.py) accept an fp32
restatement of every row kernel and the exactly rounded reference, reject each named wrong formula on a named case,
and every case of the tables reaches the launcher path it is named for.  No GPU, no compiled library."""
import pytest
import torch

import rowk_ref as R
from parity_ref import rowwise_close
from rowk_ref import BF


# ------------------------------------------------------------------------------------------------- paths
def test_every_case_reaches_the_path_it_is_named_for():
    for H, (nch, partial) in R.RMS_PATHS.items():
        assert R.rms_nch(H) == nch and (H % 512 != 0) == partial and R.rms_status(H) == 0, H
    assert sorted(R.RMS_PATHS) == sorted(R.RMS_H)
    assert {(R.rms_nch(H), H % 512 != 0) for H in R.RMS_H} == {(n, p) for n in (1, 2, 4, 8) for p in (True, False)}
    for M in R.RMS_M:  # idle waves: fewer than four rows in the last (only) workgroup
        g = R.rms_bwd_grid(M, 136)
        assert g.wave_trips == 1 and g.nb == -(-M // 4)
    for (M, H), want in R.RMS_BWD_BIG.items():
        g = R.rms_bwd_grid(M, H)
        assert {k: getattr(g, k) for k in want} == want, (M, H, g)
    assert R.rms_bwd_grid(5, 4096).lds_bytes == 64 * 1024
    for H, rc in R.RMS_REFUSED.items():
        assert R.rms_status(H) == rc
    for M, H, ns in R.RMS_SLAB_CASES:
        assert R.rms_status(H) == 0 and ns in (1, 3)
    assert R.rms_bwd_grid(2049, 520).wave_trips == 2

    for c in R.QK_CASES:
        assert c[0] * c[1] * (c[2] + c[3]) == R.QK_ITEMS[c]
    assert sorted(R.QK_ITEMS.values()) == [2, 45, 48, 330, 8200]
    for (B, T, Hq, Hkv, blocks), want in R.QK_BWD_CASES.items():
        g = R.qk_bwd_grid(B * T * (Hq + Hkv), blocks)
        assert {k: getattr(g, k) for k in want} == want, ((B, T, Hq, Hkv, blocks), g)
    assert max(T for _, T, _, _ in R.QK_CASES) > 4096

    wraps = {c: R.swiglu_grid(*c) for c in R.SWIGLU_CASES}
    assert wraps[(1025, 8192)] == (4096, 1049600, 1024)
    assert all(wraps[c][2] == 0 for c in R.SWIGLU_CASES[:3])
    assert (24 // 8) & (24 // 8 - 1)  # an I / 8 that is no power of two

    for nb in R.COLSUM_NB:
        assert R.colsum_trips(nb) == R.COLSUM_TRIPS[nb], nb
    assert {t[0] for t in R.COLSUM_TRIPS.values()} == {0, 1, 2}

    assert all(R.emb_bwd_path(M) == "bitmap" for M in R.EMB_BWD_M + (65536,))
    assert R.emb_bwd_path(R.EMB_SERIAL["M"]) == "serial"
    assert all(R.ssq_status(H) == 0 for _, H in R.EMB_SSQ_CASES)
    assert all(R.ssq_status(H) == rc for H, rc in R.EMB_SSQ_REFUSED.items())


def test_every_family_holds_every_row_kind():
    def kinds(x):
        x = x.float()
        amax, nz = x.abs().amax(-1), (x != 0).sum(-1)
        return {"zero": bool((nz == 0).any()), "onehot": bool((nz == 1).any()), "tiny": bool(((amax < 2e-2) & (nz > 1)).any()),
                "big": bool((amax > 150).any())}
    rms = torch.cat([R.rms_inputs(M, 136)["x"] for M in R.RMS_M])
    assert all(kinds(rms).values())
    for M, H in R.RMS_CASES:
        w = R.rms_inputs(M, H)["w"]
        assert (w == 0).any() and (w < 0).any()
    for c in R.QK_CASES[1:]:
        inp = R.qk_inputs(*c)
        nh = c[2] + c[3]
        assert all(kinds(inp["qkv"][:, :nh * 128].reshape(-1, 128)).values()), c
        assert (inp["qg"] == 0).any() and (inp["kg"] < 0).any()
    gu, d, exempt = R.swiglu_inputs(7, 24)
    assert all(kinds(gu[:, 24:]).values())
    g = gu[:, :24].float()
    assert set(R.SWIGLU_FIXED_GATES) <= set(g[0].tolist()) and int(exempt.sum()) == 2
    assert float(g[:, :24 - 5].abs().max()) <= R.SWIGLU_GATE_MAX


def test_floors_are_what_measure_floors_gives():
    m = R.measure_floors()
    for got, measured, chosen in ((m["rms_bwd"], R.RMS_BWD_MEASURED, R.RMS_BWD_FLOOR),
                                  (m["qk_bwd"], R.QK_BWD_MEASURED, R.QK_BWD_FLOOR), (m["rstd"], R.RSTD_MEASURED, R.RSTD_RTOL)):
        assert 0.8 * measured <= got <= measured * 1.005, (got, measured)
        assert 4 * measured <= chosen <= 4.2 * measured, (measured, chosen)
    assert R.RSTD_RTOL + R.ULP32 <= R.FWD_FLOOR


# ------------------------------------------------------------------------------------------------- RMSNorm
def _rms_fwd_check(got_y, got_rstd, inp, ref):
    v = R.elem_close(got_y, ref["y"], R.rmsnorm_fwd_bound(inp["x"], inp["w"], ref))
    rel = float(((got_rstd.double() - ref["rstd"]).abs() / ref["rstd"]).max())
    return v, rel


@pytest.mark.parametrize("M,H", R.RMS_CASES)
def test_rmsnorm_forward_rules(M, H):
    inp = R.rms_inputs(M, H)
    ref = R.rmsnorm_ref(inp["x"], inp["w"])
    y, rstd = R.rmsnorm_fwd_f32(inp["x"], inp["w"])
    v, rel = _rms_fwd_check(y, rstd, inp, ref)
    assert v.ok and rel <= R.RSTD_RTOL, (v, rel)
    assert _rms_fwd_check(ref["y"].to(BF), ref["rstd"].float(), inp, ref)[0].ok  # the exactly rounded reference
    # rule 3: against itself, under an rstd two ulps off either way, and with the kernel's own statistic (w * n is a
    # product of two bf16 values, exact in fp32, and x * rstd is rounded to bf16 at once: nothing here for an FMA to contract)
    want, _ = R.rmsnorm_fwd_f32(inp["x"], inp["w"], rstd32=ref["rstd"].float())
    assert R.differing_share(want, want) == 0.0
    for k in (-2, 2):
        y2, _ = R.rmsnorm_fwd_f32(inp["x"], inp["w"], rstd32=R.nudge_ulps(ref["rstd"].float(), k))
        assert R.differing_share(y2, want) <= R.ROUNDING_SHARE
    assert R.differing_share(y, want) <= R.ROUNDING_SHARE


def _fails(v):
    return not v.ok


def test_rmsnorm_forward_wrong_formulas_are_rejected():
    # mean over 512 NCH columns instead of H: case (3, 520), a partial last chunk (at H = 512 the two agree)
    inp = R.rms_inputs(3, 520)
    ref = R.rmsnorm_ref(inp["x"], inp["w"])
    y, rstd = R.rmsnorm_fwd_f32(inp["x"], inp["w"], mean_n=512 * R.rms_nch(520))
    v, rel = _rms_fwd_check(y, rstd, inp, ref)
    assert _fails(v) and rel > R.RSTD_RTOL
    # eps = 1e-5: case (5, 136), and there the row scaled by 1e-3 (a randn row does not notice)
    inp = R.rms_inputs(5, 136)
    ref = R.rmsnorm_ref(inp["x"], inp["w"])
    y, rstd = R.rmsnorm_fwd_f32(inp["x"], inp["w"], eps=1e-5)
    bound = R.rmsnorm_fwd_bound(inp["x"], inp["w"], ref)
    v = R.elem_close(y, ref["y"], bound)
    tiny = [r for r in range(5) if float(inp["x"][r].float().abs().max()) < 2e-2 and int((inp["x"][r] != 0).sum()) > 1]
    assert _fails(v) and v.row in tiny
    bad = ~((y.double() - ref["y"]).abs() <= bound)
    assert float(bad[tiny[0]].double().mean()) > 0.9
    randn = [r for r in range(5) if 1 < float(inp["x"][r].float().abs().max()) < 50]
    assert not bool(bad[randn].any())
    # the gain applied before the inner rounding (one rounding of w x rstd): inside the interval bound, caught by rule 3
    inp = R.rms_inputs(5, 1032)
    ref = R.rmsnorm_ref(inp["x"], inp["w"])
    want, _ = R.rmsnorm_fwd_f32(inp["x"], inp["w"], rstd32=ref["rstd"].float())
    y, _ = R.rmsnorm_fwd_f32(inp["x"], inp["w"], rstd32=ref["rstd"].float(), round_inner=False)
    assert R.elem_close(y, ref["y"], R.rmsnorm_fwd_bound(inp["x"], inp["w"], ref)).ok
    assert R.differing_share(y, want) > 0.1
    y, _ = R.rmsnorm_fwd_f32(inp["x"], inp["w"], rstd32=ref["rstd"].float(), gain_first=True)
    assert R.differing_share(y, want) > 0.1


def _rms_bwd_verdicts(dx, dw, ref):
    return (rowwise_close(dx, ref["dx"], BF, R.RMS_BWD_FLOOR),
            R.elem_close(dw, ref["dw"][None], R.gain_bound(ref["dw"], ref["dw_n"], ref["dw_abs"])[None]))


_RMS_BWD_RUNS = R.rms_bwd_runs()


@pytest.mark.parametrize("run", _RMS_BWD_RUNS, ids=[r[0] for r in _RMS_BWD_RUNS])
def test_rmsnorm_backward_rules(run):
    name, inp, dres_on, acc = run
    dres, dw0 = (inp["dres"] if dres_on else None), (inp["dw0"] if acc else None)
    ref = R.rmsnorm_ref(inp["x"], inp["w"], R.rms_grad_of(inp), dres, dw0)
    dx32, dw32 = R.rmsnorm_bwd_f32(inp["x"], inp["w"], ref["rstd"].float(), inp["dy"], inp["slabs"], dres)
    if acc:
        dw32 = dw32 + dw0.float()
    vx, vw = _rms_bwd_verdicts(dx32.to(BF), dw32.to(BF)[None], ref)
    assert vx.ok and vw.ok, (vx, vw)
    vx, vw = _rms_bwd_verdicts(ref["dx"].to(BF), ref["dw"].to(BF)[None], ref)
    assert vx.ok and vw.ok, (vx, vw)


def test_rmsnorm_backward_wrong_formulas_are_rejected():
    # without the / H: case (3, 136)
    inp = R.rms_inputs(3, 136)
    x, w, d = inp["x"].double(), inp["w"].double(), inp["dy"].double()
    ref = R.rmsnorm_ref(inp["x"], inp["w"], inp["dy"], inp["dres"], None)
    rs = ref["rstd"][:, None]
    good = rs * (d * w - x * rs * ((d * w * x * rs).sum(-1, keepdim=True) / 136)) + inp["dres"].double()
    assert rowwise_close(good.to(BF), ref["dx"], BF, R.RMS_BWD_FLOOR).ok
    wrong = rs * (d * w - x * rs * (d * w * x * rs).sum(-1, keepdim=True)) + inp["dres"].double()
    assert _fails(rowwise_close(wrong.to(BF), ref["dx"], BF, R.RMS_BWD_FLOOR))
    # dres dropped: the same case
    assert _fails(rowwise_close((good - inp["dres"].double()).to(BF), ref["dx"], BF, R.RMS_BWD_FLOOR))
    # accumulate ignored: case (3, 136) with accumulate_dw = 1
    ref1 = R.rmsnorm_ref(inp["x"], inp["w"], inp["dy"], inp["dres"], inp["dw0"])
    assert _rms_bwd_verdicts(good.to(BF), ref1["dw"].to(BF)[None], ref1)[1].ok
    assert _fails(_rms_bwd_verdicts(good.to(BF), ref["dw"].to(BF)[None], ref1)[1])


# ------------------------------------------------------------------------------------------------- q/k norm + RoPE
@pytest.mark.parametrize("case", R.QK_CASES, ids=str)
def test_qk_forward_rules(case):
    B, T, Hq, Hkv = case
    inp = R.qk_inputs(*case)
    ref = R.qk_ref(inp, T, Hq, Hkv)
    bound = R.qk_fwd_bound(inp, T, Hq, Hkv)
    out = R.qk_fwd_f32(inp, T, Hq, Hkv)
    assert R.elem_close(out, ref["out"], bound).ok
    assert R.elem_close(ref["out"].to(BF), ref["out"], bound).ok
    r32 = R.qk_rstd64(inp, Hq, Hkv).float()
    want = R.qk_fwd_f32(inp, T, Hq, Hkv, rstd32=r32)
    assert R.differing_share(want, want) == 0.0
    for k in (-2, 2):
        assert R.differing_share(R.qk_fwd_f32(inp, T, Hq, Hkv, rstd32=R.nudge_ulps(r32, k)), want) <= R.ROUNDING_SHARE
    assert R.differing_share(out, want) <= R.ROUNDING_SHARE
    # n cos + rot(n) sin with the products left unrounded, as an FMA contraction would: one rounding of the exact sum
    M, nh = inp["qkv"].shape[0], Hq + Hkv
    x = inp["qkv"][:, :nh * 128].float().view(M, nh, 128)
    gain = torch.cat([inp["qg"].float()[None].expand(Hq, 128), inp["kg"].float()[None].expand(Hkv, 128)], 0)[None]
    n = (gain * (x * r32[..., None]).to(BF).float()).to(BF).double()
    pos = torch.arange(M) % T
    fma = (n * inp["cos"].double()[pos][:, None] + R._rot(n) * inp["sin"].double()[pos][:, None]).float().to(BF)
    assert R.differing_share(fma.reshape(M, -1), want) <= R.ROUNDING_SHARE


def test_qk_forward_wrong_formulas_are_rejected():
    case = (3, 5, 2, 1)  # every one of these is rejected by case (3, 5, 2, 1): T > 1, B > 1, both kinds of head
    B, T, Hq, Hkv = case
    inp = R.qk_inputs(*case)
    ref = R.qk_ref(inp, T, Hq, Hkv)
    bound = R.qk_fwd_bound(inp, T, Hq, Hkv)
    for kw in (dict(rot_sign=-1.0), dict(pos_div=True), dict(k_uses_q_gain=True), dict(eps=1e-5)):
        assert _fails(R.elem_close(R.qk_fwd_f32(inp, T, Hq, Hkv, **kw), ref["out"], bound)), kw
    # a dropped inner rounding stays inside the interval bound and is caught by rule 3 (case (2, 33, 3, 2))
    case = (2, 33, 3, 2)
    B, T, Hq, Hkv = case
    inp = R.qk_inputs(*case)
    r32 = R.qk_rstd64(inp, Hq, Hkv).float()
    want = R.qk_fwd_f32(inp, T, Hq, Hkv, rstd32=r32)
    for kw in (dict(round_x=False), dict(round_n=False)):
        assert R.differing_share(R.qk_fwd_f32(inp, T, Hq, Hkv, rstd32=r32, **kw), want) > 0.1, kw


def _qk_bwd_verdicts(dqk, dqg, dkg, ref):
    return (rowwise_close(dqk.reshape(-1, 128), ref["dqk"].reshape(-1, 128), BF, R.QK_BWD_FLOOR),
            R.elem_close(dqg[None], ref["dqg"][None], R.gain_bound(ref["dqg"], ref["dqg_n"], ref["dqg_abs"])[None]),
            R.elem_close(dkg[None], ref["dkg"][None], R.gain_bound(ref["dkg"], ref["dkg_n"], ref["dkg_abs"])[None]))


@pytest.mark.parametrize("case", list(R.QK_BWD_CASES), ids=str)
@pytest.mark.parametrize("acc", [False, True])
def test_qk_backward_rules(case, acc):
    B, T, Hq, Hkv, _ = case
    inp = R.qk_inputs(B, T, Hq, Hkv)
    ref = R.qk_ref(inp, T, Hq, Hkv, backward=True, accumulate=acc)
    o32, gq, gk = R.qk_bwd_f32(inp, T, Hq, Hkv)
    if acc:
        gq, gk = gq + inp["dqg0"].float(), gk + inp["dkg0"].float()
    vs = _qk_bwd_verdicts(o32.to(BF), gq.to(BF), gk.to(BF), ref)
    assert all(v.ok for v in vs), vs
    vs = _qk_bwd_verdicts(ref["dqk"].to(BF), ref["dqg"].to(BF), ref["dkg"].to(BF), ref)
    assert all(v.ok for v in vs), vs
    if acc and case == (3, 5, 2, 1, 0):  # accumulate ignored: rejected by case (3, 5, 2, 1) (a sum over 24 600 items hides it)
        ref0 = R.qk_ref(inp, T, Hq, Hkv, backward=True, accumulate=False)
        vs = _qk_bwd_verdicts(ref["dqk"].to(BF), ref0["dqg"].to(BF), ref0["dkg"].to(BF), ref)
        assert _fails(vs[1]) and _fails(vs[2])


# ------------------------------------------------------------------------------------------------- SwiGLU
def _swiglu_verdicts(act, dg, du, ref, exempt):
    return (R.elem_close(act, ref["act"], R.swiglu_bound(ref["act"], ref["act_mag"], exempt)),
            R.elem_close(dg, ref["dg"], R.swiglu_bound(ref["dg"], ref["dg_mag"], exempt)),
            R.elem_close(du, ref["du"], R.swiglu_bound(ref["du"], ref["du_mag"], exempt)))


@pytest.mark.parametrize("M,I", R.SWIGLU_CASES)
def test_swiglu_rules(M, I):
    gu, d, exempt = R.swiglu_inputs(M, I)
    ref = R.swiglu_ref(gu, d)
    act, dg, du = R.swiglu_f32(gu, d)
    vs = _swiglu_verdicts(act.to(BF), dg.to(BF), du.to(BF), ref, exempt)
    assert all(v.ok for v in vs), vs
    vs = _swiglu_verdicts(ref["act"].to(BF), ref["dg"].to(BF), ref["du"].to(BF), ref, exempt)
    assert all(v.ok for v in vs), vs
    # the overflow columns: the reference rounds to zero, and zero is accepted
    col = int(torch.nonzero(exempt)[-1])
    live = gu[:, col] == -100
    if bool(live.any()):
        assert float(ref["act"][live, col].abs().max()) < 2.0 ** -134 and float(ref["dg"][live, col].abs().max()) < 2.0 ** -134
        assert bool((act.to(BF)[live, col] == 0).all())


def test_swiglu_backward_with_s_in_place_of_one_minus_s_is_rejected():
    gu, d, exempt = R.swiglu_inputs(7, 24)  # case (7, 24)
    ref = R.swiglu_ref(gu, d)
    wrong = R.swiglu_ref(gu, d, wrong_s=True)
    vs = _swiglu_verdicts(ref["act"].to(BF), wrong["dg"].to(BF), ref["du"].to(BF), ref, exempt)
    assert vs[0].ok and _fails(vs[1]) and vs[2].ok


# ------------------------------------------------------------------------------------------------- exact kernels
def test_exact_references():
    for nb in R.COLSUM_NB:
        p, o0 = R.colsum_inputs(nb, 40)
        assert float(p[:, :40].abs().sum(0).max()) + 64 < 2 ** 24
        for acc in (False, True):  # the fp32 sum in any order is the fp64 sum
            got = (p[:, :40].flip(0).sum(0) + (o0.float() if acc else 0)).to(BF)
            assert torch.equal(got, R.colsum_ref(p, o0, 40, acc))
    for M in R.EMB_BWD_M + (R.EMB_SERIAL["M"],):  # a duplicate across every 32-token word boundary, whatever M
        ids = R.emb_bwd_inputs(M, R.EMB_BWD_H, R.EMB_BWD_V)[0]
        assert all(0 <= int(ids[b]) == int(ids[b - 1]) < R.EMB_BWD_V for b in range(32, M, 32)), M
        assert M <= 2 or (-1 in ids[:3] and R.EMB_BWD_V in ids[:3])
    ids, dx, dE0 = R.emb_bwd_inputs(70, R.EMB_BWD_H, R.EMB_BWD_V)
    assert -1 in ids and R.EMB_BWD_V in ids and ids[31] == ids[32] and ids[63] == ids[64]
    for scale in (1.0, 0.5):
        for lo in (0, 3, R.EMB_BWD_V):
            ref = R.emb_bwd_ref(ids, dx, dE0, scale, lo)
            assert torch.equal(ref[:lo], dE0[:lo])
            acc = torch.zeros(dE0.shape)
            for i in range(70):  # token by token in fp32
                if lo <= int(ids[i]) < R.EMB_BWD_V:
                    acc[ids[i]] += dx[i].float()
            assert torch.equal((dE0.float() + scale * acc).to(BF), ref)
    assert torch.equal(R.emb_bwd_ref(ids, dx, dE0, 1.0, R.EMB_BWD_V), dE0)
    E = torch.arange(R.EMB_V * 8).view(R.EMB_V, 8).to(BF)
    ids = R.emb_fwd_ids(5, R.EMB_V)
    assert ids[0] == -3 and ids[4] == R.EMB_V + 2
    ref = R.emb_fwd_ref(ids, E)
    assert torch.equal(ref[0], E[0]) and torch.equal(ref[4], E[R.EMB_V - 1])
    rows = R.scatter_rows(5, R.SCATTER_M)
    assert -1 in rows and R.SCATTER_M in rows
    keep = rows[(rows >= 0) & (rows < R.SCATTER_M)]
    assert len(set(keep.tolist())) == len(keep) == 3
    src = torch.arange(5 * 8).view(5, 8).to(BF) + 1
    dst = R.scatter_ref(src, rows, R.SCATTER_M)
    assert int((dst != 0).any(-1).sum()) == 3
