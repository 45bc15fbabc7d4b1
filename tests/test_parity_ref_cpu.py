"""The tests of tests/test_gpu_loss_topk_optim.py's own tools (tests/parity_ref.py), on the CPU.

They show that the acceptance rule has teeth at the inputs the GPU tests use: it rejects each named wrong formula
(rounded to the stored type, as a wrong kernel would deliver it) and accepts the rounded exact reference; that the
recorded floors are what the fp32 evaluation measures; and that every top-K and loss case reaches the kernel path it is
named for, by a restatement of the launchers' decisions.
"""
import numpy as np
import pytest
import torch

import parity_ref as P
from parity_ref import BF, F32


# ------------------------------------------------------------------------------------------------- the rule
def test_rowwise_close_names_the_worst_element_and_judges_rows_separately():
    ref = torch.tensor([[1.0, 2.0, 1000.0], [1e-3, 2e-3, 4e-3]], dtype=torch.float64)
    ok = P.rowwise_close(ref.bfloat16(), ref, BF, 0.0)
    assert ok.ok
    got = ref.clone()
    got[1, 0] = 1.1e-3  # 10 % wrong, 1e-7 of the TENSOR maximum: invisible to a whole-tensor bound, not to this one
    v = P.rowwise_close(got, ref, BF, 1e-6)
    assert not v.ok and (v.row, v.col) == (1, 0) and v.got == pytest.approx(1.1e-3) and v.ref == pytest.approx(1e-3)
    got = ref.clone()
    got[0, 1] = float("nan")
    v = P.rowwise_close(got, ref, F32, 1e-3)
    assert not v.ok and (v.row, v.col) == (0, 1)
    # a row that is exactly zero in the reference admits nothing else
    z = torch.zeros(1, 8, dtype=torch.float64)
    assert P.rowwise_close(z, z, BF, 1e-3).ok
    assert not P.rowwise_close(z + 1e-30, z, BF, 1e-3).ok
    # half an ulp is reached, never passed, by one correct rounding: bottom and top of a binade, both types
    x = torch.tensor([[1.0 + 2.0 ** -8 + 2.0 ** -20, 2.0 - 2.0 ** -8 - 2.0 ** -20, 3.0]], dtype=torch.float64)
    assert P.rowwise_close(x.bfloat16(), x, BF, 0.0).ok
    assert float(P.half_ulp(x, BF)[0, 0]) == 2.0 ** -8 and float(P.half_ulp(x, torch.float16)[0, 1]) == 2.0 ** -11
    assert not P.rowwise_close(x.bfloat16() + torch.tensor([[2.0 ** -7, 0, 0]]), x, BF, 0.0).ok  # one ulp off
    assert float(((x.bfloat16().double() - x).abs() / x.abs()).max()) > 2.0 ** -9  # why a flat 2^-9 |ref| cannot be the rule
    # fp32 results get no relative term at all
    assert not P.rowwise_close(ref * (1 + 1e-5), ref, F32, 1e-6).ok
    assert P.rowwise_close(ref.half(), ref, torch.float16, 0.0).ok


def test_recorded_floors_are_what_the_fp32_evaluation_measures():
    """Each floor is 4 x its recorded measurement, and the measurement reproduces (25 % slack for another libm)."""
    m = P.measure_floors()
    rec = {"loss_grad": (P.LOSS_GRAD_MEASURED, P.LOSS_GRAD_FLOOR), "ce_grad": (P.CE_GRAD_MEASURED, P.CE_GRAD_FLOOR),
           "ce_scalar": (P.CE_SCALAR_MEASURED, P.CE_SCALAR_RTOL), "topk_val": (P.TOPK_VAL_MEASURED, P.TOPK_VAL_FLOOR),
           "adamw": (P.ADAMW_MEASURED, P.ADAMW_FLOOR),
           "loss_scalar_dense": (P.LOSS_SCALAR_MEASURED["dense"], P.LOSS_SCALAR_RTOL["dense"]),
           "loss_scalar_sparse": (P.LOSS_SCALAR_MEASURED["sparse"], P.LOSS_SCALAR_RTOL["sparse"])}
    for k, (measured, floor) in rec.items():
        assert 0 < m[k] <= 1.25 * measured, (k, m[k], measured)
        assert 4 * measured <= floor * (1 + 1e-9) and floor <= 4.1 * measured, (k, measured, floor)
        assert floor <= 2e-5


# ------------------------------------------------------------------------------------------------- AdamW
def adamw_variant(mut, p, g, m, v, lr, b1, b2, eps, wd, step, sumsq=None, max_norm=0.0):
    """fp64 AdamW with one named mistake (None: no mistake, must equal adamw_ref64)."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    clip = 1.0
    if sumsq is not None and max_norm > 0:
        clip = min(1.0, max_norm / (sumsq ** 0.5 + 1e-6))
    gm = gv = g * clip
    if mut == "clip_ignored":
        gm = gv = g
    if mut == "clip_m_only":
        gv = g
    if mut == "l2_wd":  # the decay folded into the gradient instead of applied to the parameter
        gm, gv = gm + wd * p, gv + wd * p
    p1 = p if mut in ("no_wd", "l2_wd") else p * (1 - lr * wd)
    m1 = m if mut == "m_frozen" else b1 * m + (1 - b1) * gm
    v1 = v if mut == "v_frozen" else b2 * v + (1 - b2) * gv * gv
    bc1 = 1.0 if mut == "no_bc1" else 1 - b1 ** step
    bc2 = 1.0 if mut == "no_bc2" else 1 - b2 ** step
    denom = (v1 / bc2 + eps).sqrt() if mut == "eps_in_sqrt" else (v1 / bc2).sqrt() + eps
    return p1 - lr / bc1 * m1 / denom, m1, v1


ADAMW_MUTANTS = ("no_wd", "l2_wd", "no_bc1", "no_bc2", "eps_in_sqrt", "clip_ignored", "clip_m_only", "v_frozen", "m_frozen")


def test_every_adamw_mutant_is_killed_by_some_set():
    for mut in ADAMW_MUTANTS:
        assert any(mut in hp["kills"] for hp in P.ADAMW_SETS.values()), mut
    assert {s for s in P.ADAMW_BIG_SETS} <= set(P.ADAMW_SETS)
    assert {hp["step"] for hp in P.ADAMW_SETS.values()} >= {1, 3, 1000}
    assert {hp["clip"] for hp in P.ADAMW_SETS.values()} == {"none", "zero", "below", "above"}


@pytest.mark.parametrize("set_name", list(P.ADAMW_SETS))
def test_adamw_comparator_accepts_the_reference_and_rejects_the_mutants(set_name):
    (p, g, m, v), (ss, mx) = P.adamw_inputs(4096, set_name)
    hp = P.adamw_hp(set_name)
    ref = P.adamw_ref64(p, g, m, v, *hp, sumsq=ss, max_norm=mx)
    same = adamw_variant(None, p, g, m, v, *hp, sumsq=ss, max_norm=mx)
    for a, b in zip(same, ref):
        assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())
    verdicts = P.adamw_close([t.bfloat16() for t in ref], ref)
    assert all(x.ok for x in verdicts.values()), verdicts
    # the fp32 evaluation of the same formula, rounded: what a correct kernel delivers
    r32 = P.adamw_ref64(p, g, m, v, *hp, sumsq=ss, max_norm=mx, acc=torch.float32)
    verdicts = P.adamw_close([t.bfloat16() for t in r32], ref)
    assert all(x.ok for x in verdicts.values()), verdicts
    for mut in P.ADAMW_SETS[set_name]["kills"]:
        wrong = adamw_variant(mut, p, g, m, v, *hp, sumsq=ss, max_norm=mx)
        verdicts = P.adamw_close([t.bfloat16() for t in wrong], ref)
        assert not all(x.ok for x in verdicts.values()), (set_name, mut)
    clip = P.ADAMW_SETS[set_name]["clip"]
    if clip in ("none", "zero", "below"):  # the clip is exactly 1 in these: the reference is the no-clip one bit for bit
        plain = P.adamw_ref64(p, g, m, v, *hp)
        assert all(torch.equal(a, b) for a, b in zip(plain, ref))
    else:
        assert not torch.equal(P.adamw_ref64(p, g, m, v, *hp)[0], ref[0])


def test_the_old_adamw_bound_misses_what_the_new_one_catches():
    """check_close(..., 8e-3, 3e-3) relative to the tensor maximum, at the hyper-parameters of test_adamw_and_clip, accepts
    AdamW without weight decay; the per-element rule at the same inputs does not."""
    gen = torch.Generator().manual_seed(11)
    n = 100003
    p, g = torch.randn(n, generator=gen).bfloat16(), torch.randn(n, generator=gen).bfloat16()
    m, v = (torch.randn(n, generator=gen) * 0.1).bfloat16(), (torch.rand(n, generator=gen) * 0.1).bfloat16()
    hp = (1e-2, 0.9, 0.999, 1e-8, 0.01, 3)
    ss = float(g.double().pow(2).sum())
    ref = P.adamw_ref64(p, g, m, v, *hp, sumsq=ss, max_norm=1.0)
    wrong = [t.bfloat16() for t in adamw_variant("no_wd", p, g, m, v, *hp, sumsq=ss, max_norm=1.0)]
    old_max = float((wrong[0].double() - ref[0]).abs().max() / ref[0].abs().max())
    assert old_max <= 8e-3
    assert not P.adamw_close(wrong, ref)["p"].ok


# ------------------------------------------------------------------------------------------------- loss
def loss_variant(mut, s, labels, top_v, top_i, T, a):
    """fp64 sparse distillation loss on selected rows with one named mistake (None: must equal the oracle).
    -> ((total, task, distill, teacher), grad [R, V])."""
    s = s.double()
    R, V = s.shape
    valid = labels != -100
    N = R if mut == "mean_all_rows" else int(valid.sum())
    y = labels.clamp_min(0)
    lse = (lambda x: torch.logsumexp(x, -1))
    lse1, lseT = lse(s), lse(s / T)
    v, idx = top_v.float().double(), top_i.long()
    logq = v / T - lse(v / T)[:, None]
    q = logq.exp()
    task_r = lse1 - s.gather(-1, y[:, None]).squeeze(-1)
    dist_r = (q * (logq - (s.gather(-1, idx) / T - lseT[:, None]))).sum(-1)
    t_fac = T if mut == "T_not_T2" else T * T
    task = float(task_r[valid].sum() / N)
    dist = float(dist_r[valid].sum() / N * t_fac)
    hit = (idx == labels[:, None]) & valid[:, None]
    teach = float(-(v[hit]).mean()) if bool(hit.any()) else 0.0
    p1 = (s - lse1[:, None]).exp()
    pT = p1 if mut == "kl_softmax_T1" else (s / T - lseT[:, None]).exp()
    e_y = torch.zeros_like(s)
    if mut != "no_label_term":
        e_y[torch.arange(R), y] = 1.0
    Q = torch.zeros_like(s)
    Q = Q.scatter(-1, idx, q) if mut == "dup_not_summed" else Q.scatter_add(-1, idx, q)
    grad = (a * (p1 - e_y) + (1 - a) * (t_fac / T) * (pT - Q)) / N
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return (a * task + (1 - a) * dist, task, dist, teach), grad


LOSS_MUTANTS = ("no_label_term", "dup_not_summed", "T_not_T2", "mean_all_rows", "kl_softmax_T1")


@pytest.mark.parametrize("dtype,T", [(BF, 2.0), (F32, 3.0)])
def test_loss_comparator_accepts_the_reference_and_rejects_the_mutants(dtype, T):
    s, _ = P.loss_inputs(P.LOSS_V, dtype)
    tv, ti, labels = P.sparse_extras(P.LOSS_V, dtype)["duplicates"]
    ref_l, n, hits, ref_g = P.oracle_rows(s, labels, top_v=tv, top_i=ti, temperature=T, alpha=P.LOSS_ALPHA)
    assert n == 7 and hits == 3 + 1 + 2  # row 0: its label three times; row 1 as placed by loss_labels; row 3: twice
    same_l, same_g = loss_variant(None, s, labels, tv, ti, T, P.LOSS_ALPHA)
    np.testing.assert_allclose(same_l, ref_l, rtol=1e-12)
    assert float((same_g - ref_g).abs().max()) <= 1e-14
    rounded = (lambda l, g: (np.float32(l), g.to(dtype)))
    ok, why = P.loss_close(*rounded(ref_l, ref_g), ref_l, ref_g, dtype, "sparse")
    assert ok, why
    # the oracle evaluated in fp32, rounded: what a correct kernel delivers
    l32, _, _, g32 = P.oracle_rows(s, labels, top_v=tv, top_i=ti, temperature=T, alpha=P.LOSS_ALPHA, acc=torch.float32)
    ok, why = P.loss_close(*rounded(l32, g32), ref_l, ref_g, dtype, "sparse")
    assert ok, why
    for mut in LOSS_MUTANTS:
        l, g = loss_variant(mut, s, labels, tv, ti, T, P.LOSS_ALPHA)
        ok, why = P.loss_close(*rounded(l, g), ref_l, ref_g, dtype, "sparse")
        assert not ok, mut
        if mut in ("no_label_term", "dup_not_summed", "kl_softmax_T1"):  # gradient-only mistakes: the gradient rule alone
            assert not P.rowwise_close(g.to(dtype), ref_g, dtype, P.LOSS_GRAD_FLOOR).ok, mut
        if mut == "T_not_T2":
            assert not P.scalar_close(np.float32(l), ref_l, P.LOSS_SCALAR_RTOL["sparse"])[0]


def test_sparse_extras_are_what_they_say():
    for dtype in (BF, F32):
        ex = P.sparse_extras(P.LOSS_V, dtype)
        tv, ti, lab = ex["duplicates"]
        assert int((ti[0] == ti[0, 5]).sum()) == 2 and int((ti[0] == lab[0]).sum()) == 3 and int((ti[3] == lab[3]).sum()) == 2
        tv, ti, lab = ex["ends"]
        assert int(ti[0, 0]) == int(lab[0]) and int(ti[1, -1]) == int(lab[1])
        assert int((ti[:7] == lab[:7, None]).sum()) == 2
        tv, ti, lab = ex["no_hit"]
        assert int((ti[:7] == lab[:7, None]).sum()) == 0 and int(lab[7]) == -100


# ------------------------------------------------------------------------------------------------- paths
@pytest.mark.parametrize("name,dtype,nt", P.topk_case_list((512, 256, 1024)),
                         ids=lambda x: x if isinstance(x, (str, int)) else str(x).split(".")[-1])
def test_topk_case_reaches_its_path(name, dtype, nt):
    c = P.TOPK_CASES[name]
    x = c["make"](dtype)
    assert x.dtype == dtype
    xv = x if c["vocab"] is None else x[:, :c["vocab"]]
    paths = [P.topk_path(row, c["K"], nt, dtype) for row in xv]
    assert [p.path for p in paths] == c["nt"][nt], paths
    V = xv.shape[1]
    if name == "a_all_equal":
        assert all(p.trips == V // (nt * 8) and p.nc == V for p in paths) and (nt == 1024 or paths[0].trips >= 2)
    if name == "b_ties_across_trips":
        # 50 distinct winners, then 78 ties whose lowest indices lie on both sides of a trip boundary of the radix select
        _, idx = P.topk_ref(xv, c["K"])
        ties = sorted(int(i) for i in idx[0, 50:])
        assert ties == list(range(8150, 8228)) and 8192 % (nt * 8) == 0 and paths[0].trips >= 2
        assert len(set(float(v) for v in xv[0, idx[0, :50]].float())) == 50
        assert float(xv[0, idx[0, 49]]) > float(xv[0, 8150])
    if name == "c_plain_loops":
        assert all(p.plain_loops for p in paths) and V > 40 * 512 * 8
    elif nt == 512:
        assert not any(p.plain_loops for p in paths)
    if name in ("d_k513", "d_k1024") and nt == 512:
        assert all(p.trips == 2 for p in paths)
    if name == "e_v8_k8":
        assert all(p.trips == 1 for p in paths)
    if name == "f_vocab_tail":
        assert x.shape[1] == 4104 and float(x[:, 4096:].min()) == 100.0 and float(xv.max()) < 100.0


def test_topk_path_on_rows_whose_path_is_known_by_construction():
    # distinct values: the K-th largest thread maximum admits at most K + (elements above it) candidates: fast
    x = torch.arange(8192, dtype=torch.float32)
    # thread t holds chunks t and 512 + t: its maximum is (512 + t) * 8 + 7; the 16th largest is thread 496's, 8071
    assert P.topk_path(x, 16, 512, F32) == P.TopkPath("fast", 0, False, 8192 - 8071)
    # bf16 truncation: t0 keeps 16 key bits, so values sharing them with the K-th thread maximum all count
    assert P.topk_path(torch.zeros(1024), 16, 512, BF).path == "fast"       # 1024 candidates <= 2048
    assert P.topk_path(torch.zeros(4096), 16, 512, BF).path == "overflow"   # 4096 candidates
    assert P.topk_path(torch.zeros(64), 64, 512, BF) == P.TopkPath("general", 1, False, None)
    np.testing.assert_array_equal(np.argsort(P.f2key(np.array([-2.0, -0.5, 0.0, 0.5, 3.0], dtype=np.float32))), np.arange(5))


def test_topk_ref_orders_by_value_then_index():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, 2.0, 1.0, 1.0]])
    v, i = P.topk_ref(x, 6)
    assert i.tolist() == [[1, 2, 4, 5, 0, 6]]
    lse = float(torch.logsumexp(x.double(), -1))
    np.testing.assert_allclose(v[0].numpy(), np.array([3, 3, 3, 2, 1, 1]) - lse, rtol=1e-15)
    # the project's oracle agrees wherever it is exact
    from oracle.distill_loss import extract_topk
    xr = torch.randn(3, 512, generator=torch.Generator().manual_seed(3)).bfloat16()
    assert torch.equal(extract_topk(xr.float(), 40)[1].long(), P.topk_ref(xr, 40)[1])


def test_loss_cases_reach_all_twelve_instantiations_at_several_chunks_per_thread():
    reached = {}
    for name, V, dt, T, te in P.LOSS_CASES:
        lp = P.loss_path(V, 0 if te == "dense" else te, te == "dense", T, dt)
        assert lp.chunks_per_thread > 4, (name, lp)  # more than one prefetch trip, ragged last one
        assert (V // 8) % lp.nf != 0
        reached.setdefault((lp.dtype, lp.t2, lp.nf, lp.dense), []).append(name)
    assert len(P.LOSS_INSTANTIATIONS) == 12
    for inst, case in P.LOSS_INSTANTIATIONS.items():
        assert case in reached.get(inst, []), (inst, case, reached.get(inst))
    # temperature 1 runs the generic (T2 = false) code with invT = 1
    assert [n for n, *_ in P.LOSS_CASES if "_T1_" in n] == ["bf16_T1_dense", "fp32_T1_100"]
    edges = {}
    for name, V, dt, T, te in P.LOSS_EDGE_CASES:
        lp = P.loss_path(V, 0 if te == "dense" else te, te == "dense", T, dt)
        edges.setdefault(V, set()).add((lp.dtype, lp.dense))
        assert lp.nf == 512
        assert te == "dense" or te <= V
    assert set(edges) == {8, 4096, 16384, 16392}
    assert all(e == {("bf16", True), ("bf16", False), ("fp32", True), ("fp32", False)} for e in edges.values())
    assert P.loss_path(16384, 100, False, 2.0, BF).chunks_per_thread == 4.0  # exactly one full prefetch trip


def test_loss_rows_are_the_kinds_they_are_named_for():
    for dt in (BF, F32):
        s, t = P.loss_inputs(P.LOSS_V, dt)
        lab = P.loss_labels(P.LOSS_V, dt)
        assert s.dtype == dt and t.dtype == dt and len(P.ROW_KINDS) == 8
        f = s.float()
        assert bool((f[3, 1:] >= f[3, :-1]).all()) and bool((f[4, 1:] <= f[4, :-1]).all())
        assert float(f[5].max()) == 60.0 and float(f[5].abs().kthvalue(P.LOSS_V - 1).values) < 1.0
        assert int(f[5].argmax()) != int(lab[5])
        assert float(f[6].min()) == float(f[6].max())
        assert int(lab[7]) == -100 and int((lab[:7] >= 0).sum()) == 7 and int(lab.max()) == P.LOSS_V - 1
        # every thread of the streaming loop meets a new running maximum after its first chunk on the rising row
        assert float(f[3, -1]) > float(f[3, 8 * 1024])
