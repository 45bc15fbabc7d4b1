"""The instruments of tests/test_gpu_attn_edges.py, tested before the kernels are (CPU only).

1. attn_ref equals torch autograd of a naive fp64 softmax attention.
2. The acceptance rule (attn_ref.judge: per-row error against the bf16-storage emulation's worst row of the same 64-row
   tile, the global max / rms limits, LSE against fp64) accepts, over five seeds, the clean emulation and a second clean
   run that rounds differently (an independent draw of the noise, as a kernel's is), and rejects the emulation run with
   a deliberately wrong mask, on the input family meant to catch that mistake.  One global norm over randn inputs lets
   "row 447 also sees key 448" through; that case is kept here as the reason for the per-row rule.
3. Why dQ / dK / dV rows are measured on the o each side was handed, where the rms limit is widened, and that the kv_len
   launches of the GPU module cover their set.
"""
import math

import pytest
import torch

import attn_ref as A

T, SCALE = 512, 128 ** -0.5


# ------------------------------------------------------------------------------------ attn_ref against autograd
@pytest.mark.parametrize("B,T_,Hq,Hkv,kv_len", [(2, 37, 4, 2, (37, 5)), (3, 70, 6, 2, (1, 64, 200)), (1, 16, 2, 2, None)])
def test_attn_ref_equals_autograd(B, T_, Hq, Hkv, kv_len):
    q, k, v, do = (t.double() for t in A.randn_inputs(B, T_, Hq, Hkv, seed=T_))
    scale = 0.21
    got = A.attn_ref(q, k, v, do, B, T_, Hq, Hkv, kv_len, scale)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    G = Hq // Hkv
    qh = qr.view(B, T_, Hq, 128).transpose(1, 2)
    kh = kr.view(B, T_, Hkv, 128).transpose(1, 2).repeat_interleave(G, 1)
    vh = vr.view(B, T_, Hkv, 128).transpose(1, 2).repeat_interleave(G, 1)
    s = scale * qh @ kh.transpose(-1, -2)
    s = s.masked_fill(~A.visible_mask(B, T_, kv_len)[:, None], -math.inf)
    o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B * T_, Hq * 128)
    (o * do).sum().backward()
    want = {"o": o.detach(), "lse": torch.logsumexp(s, -1).detach(), "dq": qr.grad, "dk": kr.grad, "dv": vr.grad}
    for n in A.NAMES:
        torch.testing.assert_close(got[n], want[n], rtol=1e-10, atol=1e-12, msg=lambda m, n=n: f"{n}: {m}")
    # the backward as an operator on a given o: delta from that o, i.e. the gradient with delta held as a constant
    og = (o.detach() + 0.01 * torch.randn(o.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1)))
    got2 = A.attn_ref(q, k, v, do, B, T_, Hq, Hkv, kv_len, scale, o_given=og)
    for t in (qr, kr, vr):
        t.grad = None
    p = torch.softmax(s, -1)
    dp = do.view(B, T_, Hq, 128).transpose(1, 2) @ vh.transpose(-1, -2)
    ds = (p * (dp - (do * og).view(B, T_, Hq, 128).transpose(1, 2).sum(-1, keepdim=True))).detach()
    (scale * (ds * (qh @ kh.transpose(-1, -2))).sum() + (p.detach() * dp).sum()).backward()
    for n, t in (("dq", qr), ("dk", kr), ("dv", vr)):
        torch.testing.assert_close(got2[n], t.grad, rtol=1e-10, atol=1e-12, msg=lambda m, n=n: f"o_given {n}: {m}")


def test_kv_len_is_clamped_and_padding_rows_get_no_gradient():
    q, k, v, do = A.randn_inputs(2, 20, 2, 1, seed=3)
    a = A.attn_ref(q, k, v, do, 2, 20, 2, 1, (0, 99))
    b = A.attn_ref(q, k, v, do, 2, 20, 2, 1, (1, 20))
    for n in A.NAMES:
        assert torch.equal(a[n], b[n])
    assert (a["dk"][1:20] == 0).all() and (a["dv"][1:20] == 0).all()
    assert torch.isfinite(a["o"]).all() and a["o"][5].abs().sum() > 0   # query rows >= kv_len are ordinary rows


def test_row_err_and_builders():
    ref = torch.ones(4, 256, dtype=torch.float64)
    ref[0, :128] = 0
    got = ref.clone()
    got[1, 128:] *= 1.5
    e = A.row_err(got, ref)
    assert e.shape == (8,) and e[3] == pytest.approx(0.5) and e.sum() == pytest.approx(0.5)
    got[0, :128] = 1e-3   # zero reference row: measured against the floor, 0.05 x the median row norm
    assert A.row_err(got, ref)[0] == pytest.approx(1e-3 / 0.05)
    z = torch.zeros(4, 128, dtype=torch.float64)
    z2 = z.clone()
    z2[2, 0] = 1e-30
    assert A.row_err(z2, z).tolist() == [0, 0, math.inf, 0]
    # the ramp: exact in bf16, score(i, j) = sign * step * j + O(0.1)
    for sign, step in ((1, 0.25), (-1, 1.0)):
        q, k, v, do = A.ramp_inputs(1, 200, 2, 1, 0, sign, step)
        s = SCALE * q.double()[:, :128] @ k.double().T
        want = sign * step * torch.arange(200.)[None, :]
        assert (s - want).abs().max() < 0.6 + 0.01 * step * 200   # g is step * sqrt(128) rounded to bf16: 2^-9 relative
    kp, vp = A.poison(k, v, 1, 200, (150,))
    assert torch.equal(kp[:150], k[:150]) and torch.equal(vp[:150], v[:150])
    assert torch.isfinite(kp.float()).all() and vp[150:].float().abs().mean() > 100


# --------------------------------------------------------------------------------------- the rule against wrong masks
def _leak(m):          # row 447 also sees key 448
    m[447, 448] = True


def _diag_drop(m):     # the first row of every 64-row tile loses its diagonal key
    for i in range(64, T, 64):
        m[i, i] = False


def _key0_drop(m):     # rows >= 64 lose key 0
    m[64:, 0] = False


def _tile_drop(m):     # one interior 64 x 64 tile is skipped
    m[256:320, 128:192] = False


MUTATIONS = {"leak": _leak, "diag_drop": _diag_drop, "key0_drop": _key0_drop, "tile_drop": _tile_drop}
FAMILIES = {
    "randn": (lambda seed: A.randn_inputs(1, T, 1, 1, seed), ("o", "dq", "dk", "dv"), ()),
    # P is almost one-hot on the ramps, dQ / dK rows nearly cancel (emulated worst row 0.1 - 0.2): per-row on O, dV only,
    # and the rms limit of dQ follows the emulation where the emulation itself exceeds the global one (attn_ref.judge)
    "rising": (lambda seed: A.ramp_inputs(1, T, 1, 1, seed, +1, 0.25), ("o", "dv"), ("dq",)),
    "falling": (lambda seed: A.ramp_inputs(1, T, 1, 1, seed, -1, 0.25), ("o", "dv"), ("dq",)),
}


def _run(family, seed, mutate=None, got_mode="unnorm", o_given=True):
    """The rule applied to a stand-in for the kernel: a clean run of the OTHER emulation (unnormalised P rounded in the
    forward -- different roundings, hence an independent draw of the noise, as a kernel's is), or with ``mutate`` the
    emulation under a wrong mask."""
    make, per_row, rms_budget = FAMILIES[family]
    q, k, v, do = make(seed)
    args = (q, k, v, do, 1, T, 1, 1, None, SCALE)
    ref = A.attn_ref(*args)
    emu = A.attn_ref(*args, emulate=True)
    if mutate is None:
        got = A.attn_ref(*args, emulate=got_mode)
    else:
        m = A.visible_mask(1, T)[0].clone()
        mutate(m)
        got = A.attn_ref(*args, emulate=True, mask=m)
    tol = A.lse_tolerance(q, k, ref["lse"], 1, T, 1, 1, SCALE)
    ref_e = A.attn_ref(*args, o_given=emu["o"]) if o_given else ref
    ref_g = A.attn_ref(*args, o_given=got["o"]) if o_given else ref
    return A.judge(got, ref, emu, ref_g, ref_e, 1, T, tol, per_row, rms_budget)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("seed", range(5))
def test_rule_accepts_a_clean_run(family, seed):
    """No false alarm of the tile-local rule on an independently rounded clean run; the worst ratios are printed."""
    res = _run(family, seed)
    print(family, seed, {n: round(r["ratio"], 3) for n, r in res.items()})
    assert not A.rejected(res), res
    same = _run(family, seed, got_mode=True)   # the emulation against itself: the global limits alone
    assert not A.rejected(same), same


def test_rms_limit_is_widened_only_where_the_emulation_exceeds_it():
    for family, want in (("randn", False), ("falling", False), ("rising", True)):
        res = _run(family, 0)
        assert res["dq"]["rms_widened"] is want, (family, res["dq"])
        assert res["dq"]["rms_lim"] == (A.F_RMS * res["dq"]["rms_emu"] if want else A.GLOBAL_LIMITS["dq"][1])
        assert not res["dk"]["rms_widened"] and res["dk"]["rms_lim"] == A.GLOBAL_LIMITS["dk"][1]


def test_first_rows_of_dq_need_the_o_given_reference():
    """Against the plain reference the two clean emulations, which differ only in how the forward rounds P, disagree in
    the first rows of dQ by more than F_ROW on some seed (delta carries the rounding of O into rows whose dS nearly
    cancels); with each side measured on its own o they agree on every seed."""
    plain = [_run("randn", seed, o_given=False)["dq"] for seed in range(5)]
    given = [_run("randn", seed)["dq"] for seed in range(5)]
    print([round(r["ratio"], 2) for r in plain], [round(r["ratio"], 2) for r in given])
    assert max(r["ratio"] for r in plain) > A.F_ROW
    assert all(r["worst_row"] < 64 for r in plain if r["ratio"] > A.F_ROW)
    assert max(r["ratio"] for r in given) <= A.F_ROW


def test_kv_launches_cover_the_set():
    for T_ in (64, 65, 200, 512):
        launches = A.kv_launches(T_)
        assert all(len(kl) == 8 for kl in launches)
        assert {x for kl in launches for x in kl} == {x for x in A.KV_SET + (T_ - 1, T_) if 1 <= x <= T_}
    assert A.kv_values(64) == [1, 2, 31, 32, 33, 63, 64] and len(A.kv_launches(512)) == 2


@pytest.mark.parametrize("family,mutation", [("randn", "leak"), ("randn", "tile_drop"), ("randn", "diag_drop"),
                                             ("rising", "leak"), ("rising", "diag_drop"), ("falling", "key0_drop")])
@pytest.mark.parametrize("seed", range(5))
def test_rule_rejects_a_wrong_mask(family, mutation, seed):
    res = _run(family, seed, MUTATIONS[mutation])
    bad = A.rejected(res)
    print(family, mutation, seed, {n: (r.get("ratio"), r["ok"]) for n, r in res.items()})
    assert bad, f"{mutation} on {family} inputs passed the rule: {res}"


def test_one_global_norm_lets_a_single_leak_through():
    """Why the per-row rule exists: on randn inputs "row 447 also sees key 448" stays inside every global max / rms
    limit of test_attention_fwd_bwd, while its own row is off by tens of noise floors."""
    res = _run("randn", 0, _leak)
    for n in ("o", "dq", "dk", "dv"):
        assert res[n]["max_rel"] <= A.GLOBAL_LIMITS[n][0] and res[n]["rms_rel"] <= A.GLOBAL_LIMITS[n][1], (n, res[n])
    assert max(res[n]["ratio"] for n in ("o", "dq", "dk", "dv")) > 5 * A.F_ROW, res   # ratio: row error / (allowance / F)


def test_noise_floor_of_the_emulation():
    """Worst emulated row on randn inputs: a few bf16 roundings for every output, dQ included once the backward is
    measured on the o it was handed (against the plain reference its first rows show 1.5e-2 and more)."""
    res = _run("randn", 0)
    print({n: r.get("row_emu") for n, r in res.items()})
    assert res["o"]["row_emu"] < 8e-3 and res["dv"]["row_emu"] < 8e-3 and res["dk"]["row_emu"] < 1.2e-2
    assert res["dq"]["row_emu"] < 8e-3
