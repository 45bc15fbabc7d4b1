"""CPU: the reference of the top-K Jensen-Shannon loss (tests/gjsd_topk_ref.py) is the definition, its tolerances are what
the fp32 evaluation measures, and the Python layers accept and refuse "jsd_topk" where they should -- no GPU needed."""
import importlib.util
import math
import os
import tempfile

import pytest
import torch

import gjsd_ref as G
import gjsd_topk_ref as R
import parity_ref as P
from parity_ref import BF, F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    out = [("V8", R.table_inputs(8, F32)), ("V4096", R.table_inputs(4096, BF)), ("V16392_K513", R.table_inputs(16392, F32, 513)),
           ("duplicates", R.extras_inputs(R.TABLE_V, F32, "duplicates")), ("dropped", R.dropped_inputs(R.DROP_V, BF)[0]),
           ("peaked", R.peaked_inputs(R.TABLE_V, F32)), ("underflow", R.underflow_inputs(R.UNDERFLOW_V, F32))]
    return out


@pytest.mark.parametrize("mode", R.MODES, ids=R.mode_id)
def test_reference_gradient_is_the_autograd_gradient_of_the_definition(mode):
    beta, T = mode
    for name, (s, tv, ti, labels) in _cases():
        losses, n, hits, D, g = R.topk_rows(s, tv, ti, labels, beta, T, R.ALPHA)
        x = s.double().requires_grad_(True)
        total = R.topk_total_autograd(x, tv, ti, labels, beta, T, R.ALPHA)
        total.backward()
        assert abs(losses[0] - float(total.detach())) <= 1e-13 * abs(losses[0]), (name, losses[0], float(total.detach()))
        rel = ((x.grad - g).abs().amax(-1) / g.abs().amax(-1).clamp_min(1e-300)).max()
        assert float(rel) <= 1e-12, (name, float(rel))
        assert float(g[labels < 0].abs().max()) == 0.0


@pytest.mark.parametrize("mode", R.MODES, ids=R.mode_id)
def test_divergence_is_gjsd_refs_jsd_on_the_dense_teacher_built_from_P(mode):
    """logits T log P_j on S and -inf off it (duplicates merged) have softmax(t / T) = P: gjsd_ref's dense "jsd" on them is
    the same number, term by term without the collapsed off-support sum."""
    beta, T = mode
    for name, (s, tv, ti, labels) in _cases():
        V = s.shape[1]
        Pd, some = R.scatter_P(tv, ti, V, T)
        assert torch.allclose(Pd.sum(-1)[some], torch.ones(int(some.sum()), dtype=torch.float64), atol=1e-14)
        t = R.dense_teacher_logits(tv, ti, V, T)
        ours = R.divergence_terms(s, Pd, beta, T)[0][some]
        theirs = G.divergence_terms(s[some], t[some], "jsd", beta, T)[0]
        assert bool(torch.isfinite(theirs).all()), name
        assert float((ours - theirs).abs().max()) <= 1e-12 * max(1.0, float(theirs.abs().max())), (name, ours, theirs)


def test_task_teacher_and_hits_are_the_sparse_forward_kls():
    for name, (s, tv, ti, labels) in _cases():
        if name == "dropped":
            continue   # (the oracle has no notion of an absent entry)
        ours = R.topk_rows(s, tv, ti, labels, 0.5, 2.0, R.ALPHA)
        o_l, o_n, o_hits, _ = P.oracle_rows(s, labels, top_v=tv, top_i=ti, temperature=2.0, alpha=R.ALPHA)
        assert ours[1] == o_n and ours[2] == o_hits, name
        assert abs(ours[0][1] - o_l[1]) <= 1e-12 * abs(o_l[1]) and abs(ours[0][3] - o_l[3]) <= 1e-12 * max(abs(o_l[3]), 1.0), name


def test_dropped_entries_behave_as_absent_and_an_empty_teacher_masks_the_row():
    for dt in (BF, F32):
        with_, without = R.dropped_inputs(R.DROP_V, dt)
        assert int((~R.kept(with_[1], with_[2], R.DROP_V)).sum(-1).min()) == R.DROP
        assert not bool(R.kept(with_[1], with_[2], R.DROP_V)[6].any())
        for beta, T in R.MODES:
            a = R.topk_rows(*with_, beta, T, R.ALPHA)
            b = R.topk_rows(*without, beta, T, R.ALPHA)
            assert a[1] == b[1] == 6 and a[2] == b[2]
            assert all(abs(x - y) <= 1e-13 * max(abs(y), 1.0) for x, y in zip(a[0], b[0])), (a[0], b[0])
            assert float((a[4] - b[4]).abs().max()) <= 1e-15 and float(a[4][6].abs().max()) == 0.0
    s, tv, ti, labels = R.table_inputs(8, F32)
    none = R.topk_rows(s, tv, torch.full_like(ti, -1), labels, 0.5, 2.0, R.ALPHA)
    assert none[0] == (0.0, 0.0, 0.0, 0.0) and none[1] == 0 and float(none[4].abs().max()) == 0.0


def test_divergence_is_zero_only_with_all_student_mass_on_the_support():
    """q = P exactly (logits T log P on S, -inf off it): D = 0.  The same student with mass off the support: D > 0, at least
    the off-support share times g0."""
    s, tv, ti, labels = R.table_inputs(4096, F32)
    for beta, T in R.MODES:
        Pd, _ = R.scatter_P(tv, ti, 4096, T)
        t = R.dense_teacher_logits(tv, ti, 4096, T)
        D = R.divergence_terms(t, Pd, beta, T)[0]
        assert float(D.abs().max()) <= 1e-14
        leaky = torch.where(torch.isfinite(t), t, torch.full_like(t, float(t[torch.isfinite(t)].min()) - 3.0))
        D2, q, _, _ = R.divergence_terms(leaky, Pd, beta, T)
        off = torch.where(Pd > 0, torch.zeros_like(q), q).sum(-1)
        assert bool((D2 >= off * (-(1 - beta) * math.log(1 - beta)) - 1e-15).all()) and bool((D2 > 0).all())


def test_recorded_tolerances_are_what_the_fp32_evaluation_measures():
    """Each bound is 4 x its recorded measurement (two digits, rounded up), and the measurement reproduces (25 % slack for
    another libm)."""
    m = R.measure_floors()
    ce = max(v["ce"] for v in m.values())
    assert 0 < ce <= 1.25 * R.CE_MEASURED and 4 * R.CE_MEASURED <= R.CE_RTOL * (1 + 1e-9) <= 4.4 * R.CE_MEASURED
    assert max(v["teacher"] for v in m.values()) == R.TEACHER_MEASURED == R.TEACHER_RTOL == 0.0
    for fam in ("table", "peaked", "underflow"):
        pairs = list(zip(m[fam]["grad"], R.GRAD_MEASURED[fam], R.GRAD_FLOOR[fam]))
        pairs.append((m[fam]["distill_rel"], R.DISTILL_MEASURED[fam], R.DISTILL_RTOL[fam]))
        for now, measured, floor in pairs:
            assert 0 < now <= 1.25 * measured, (fam, now, measured)
            assert 4 * measured <= floor * (1 + 1e-9) and floor <= 4.4 * measured, (fam, measured, floor)
        small, atol = R.SMALL_ABS_MEASURED[fam], R.SCALAR_ATOL[fam]
        assert m[fam]["small_abs"] <= 1.25 * small or small == 0.0 == m[fam]["small_abs"], (fam, m[fam]["small_abs"])
        assert atol >= P.LOSS_SCALAR_ATOL and 4 * small <= atol * (1 + 1e-9) and atol <= max(4.4 * small, P.LOSS_SCALAR_ATOL)


def test_underflow_and_peaked_rows_are_finite_in_fp32():
    for fam in ("peaked", "underflow"):
        for inputs, (beta, T) in R.family_cases(fam):
            l32, _, _, D, g32 = R.topk_rows(*inputs, beta, T, R.ALPHA, acc=torch.float32)
            assert all(math.isfinite(x) for x in l32) and bool(torch.isfinite(g32).all()) and bool(torch.isfinite(D).all())
            ok, why = R.topk_close(l32, g32, *[R.topk_rows(*inputs, beta, T, R.ALPHA)[i] for i in (0, 4)], F32, fam)
            assert ok, why
    # the two regimes the peaked family is built for
    s, tv, ti, labels = R.peaked_inputs(R.TABLE_V, F32)
    D = R.topk_rows(s, tv, ti, labels, 0.5, 2.0, R.ALPHA)[3]
    Pd, _ = R.scatter_P(tv, ti, R.TABLE_V, 2.0)
    q = R.divergence_terms(s, Pd, 0.5, 2.0)[1]
    Qs = torch.where(Pd > 0, q, torch.zeros_like(q)).sum(-1)
    assert float(D[0]) < 1e-3 and float(Qs[0]) > 0.999 and float(Qs[1]) < 1e-6 and float(D[1]) > 0.5


# ------------------------------------------------------------------------------------------------- Python layers, no GPU
def test_loss_accepts_and_refuses_jsd_topk_before_any_launch():
    import speech_distill_amd as sda
    for beta in (0.0, 1.0, float("nan"), -0.1):
        with pytest.raises(ValueError, match="0 < beta < 1"):
            sda.DistillationLoss(divergence="jsd_topk", beta=beta)
    with pytest.raises(ValueError, match="jsd_topk"):      # the list of known names carries the new one
        sda.DistillationLoss(divergence="tv")
    fn = sda.DistillationLoss(divergence="jsd_topk", beta=0.3)
    assert fn.divergence == "jsd_topk" and fn.beta == 0.3
    s, lab = torch.randn(1, 4, 64), torch.tensor([[1, 2, 3, 4]])
    topk = dict(teacher_top_k_v=torch.zeros(1, 4, 2), teacher_top_k_i=torch.zeros(1, 4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="divergence='jsd'"):     # dense logits: pointed to "jsd"
        fn(s, lab, teacher_logits=torch.randn(1, 4, 64))
    with pytest.raises(ValueError, match="divergence='jsd'"):
        fn.forward_rows(s[0], lab[0], teacher_logits=torch.randn(4, 64))
    with pytest.raises(ValueError, match="divergence='jsd'"):     # both forms at once: still not a top-K-only call
        fn.forward_rows(s[0], lab[0], teacher_logits=torch.randn(4, 64), teacher_top_k_v=topk["teacher_top_k_v"][0],
                        teacher_top_k_i=topk["teacher_top_k_i"][0])
    with pytest.raises(ValueError, match="Either teacher_logits or top_k"):
        fn(s, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # accepted up to the kernel, which has no CPU form
        fn.forward_rows(s[0], lab[0], teacher_top_k_v=topk["teacher_top_k_v"][0], teacher_top_k_i=topk["teacher_top_k_i"][0])
    # the dense divergences still refuse a top-K teacher, with their message
    for div in ("jsd", "reverse_kl"):
        with pytest.raises(ValueError, match="dense teacher"):
            sda.DistillationLoss(divergence=div).forward_rows(s[0], lab[0], teacher_top_k_v=topk["teacher_top_k_v"][0],
                                                              teacher_top_k_i=topk["teacher_top_k_i"][0])


def _trainer(**kw):
    import speech_distill_amd as sda
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    dims = sda.Qwen3Dims(640, 128, 256, 2, 2, 1)
    student = sda.HipQwen3ForCausalLM(dims, device="cpu", seed=0)
    args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False, label_names=["labels"],
                             save_strategy="no", use_cpu=True)
    teacher = kw.pop("teacher_model", "build")
    if teacher == "build":
        teacher = sda.HipQwen3ForCausalLM(dims, device="cpu", seed=1)
    return DistillationTrainer(model=student, args=args, teacher_model=teacher, **kw)


def test_trainer_accepts_and_refuses_jsd_topk():
    for kw in (dict(top_k=0), dict(top_k=-1), dict(top_k=16, is_quantized_teacher=True)):
        with pytest.raises(ValueError, match="divergence='jsd'"):
            _trainer(divergence="jsd_topk", **kw)
    with pytest.raises(ValueError, match="0 < beta < 1"):
        _trainer(divergence="jsd_topk", beta=1.0, top_k=16)
    with pytest.raises(ValueError, match="top_k=0"):          # unchanged: the dense jsd on a top-K teacher
        _trainer(divergence="jsd", top_k=100)
    tr = _trainer(divergence="jsd_topk", beta=0.3, top_k=16)
    assert tr.distill_loss_fn.divergence == "jsd_topk" and tr.distill_loss_fn.beta == 0.3 and tr.top_k == 16
    tr = _trainer(divergence="jsd_topk", top_k=16, teacher_model=None)    # a pre-extracted dataset needs no teacher
    assert tr.teacher_model is None
    # a batch with pre-extracted top-K passes the trainer's own checks (the dense divergences refuse it there) and
    # reaches the kernels, which have no CPU form
    batch = {"input_ids": torch.zeros(1, 4, dtype=torch.int64), "labels": torch.zeros(1, 4, dtype=torch.int64),
             "teacher_top_k_v": torch.zeros(1, 4, 2), "teacher_top_k_i": torch.zeros(1, 4, 2, dtype=torch.int64)}
    with pytest.raises(Exception) as e:
        tr.compute_loss(tr.model, batch)
    assert "pre-extracted" not in str(e.value) and not isinstance(e.value, ValueError), e.value
    with pytest.raises(ValueError, match="teacher model"):
        _trainer(divergence="jsd_topk", top_k=16, lmbda=0.5, on_policy_generate={"max_new_tokens": 8}, teacher_model=None)


def _train_script():
    spec = importlib.util.spec_from_file_location("sd_train_script_topk", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_accepts_jsd_topk_with_a_topk_teacher_only():
    tr = _train_script()
    assert tr.distill_kwargs(tr.parse_args(["--divergence", "jsd_topk", "--beta", "0.3"])) == dict(divergence="jsd_topk", beta=0.3)
    assert tr.distill_kwargs(tr.parse_args(["--divergence", "jsd_topk", "--top_k", "16"])) == dict(divergence="jsd_topk", beta=0.5)
    for extra in (["--top_k", "0"], ["--load_teacher_in_8bit"], ["--load_teacher_in_4bit"]):
        with pytest.raises(SystemExit, match="--divergence jsd"):
            tr.distill_kwargs(tr.parse_args(["--divergence", "jsd_topk"] + extra))
    with pytest.raises(SystemExit, match="--top_k 0"):       # unchanged
        tr.distill_kwargs(tr.parse_args(["--divergence", "jsd"]))
