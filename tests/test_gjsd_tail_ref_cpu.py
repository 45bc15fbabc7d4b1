"""CPU: the reference of the tail-bucket divergences (tests/gjsd_tail_ref.py) is the definition, its tolerances are what
the fp32 evaluation measures, and the Python layers -- loss, trainer, collator, extraction script, command line -- accept,
carry and refuse "forward_kl_tail" / "reverse_kl_tail" / "jsd_tail" where they should.  No GPU needed."""
import importlib.util
import math
import os
import tempfile
import types

import pytest
import torch

import gjsd_ref as G
import gjsd_tail_ref as R
import gjsd_topk_ref as K
import parity_ref as P
from oracle import distill_loss as L
from parity_ref import BF, F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIV = pytest.mark.parametrize("div", R.DIVERGENCES)


def _cases(T):
    return [("V8", R.table_inputs(8, F32, T)), ("V4096", R.table_inputs(4096, BF, T)),
            ("V16392_K513", R.table_inputs(16392, F32, T, 513)), ("duplicates", R.extras_inputs(R.TABLE_V, F32, T, "duplicates")),
            ("dropped", R.dropped_inputs(R.DROP_V, BF, T)[0]), ("bad_tails", R.bad_tail_inputs(R.DROP_V, F32, T)),
            ("peaked", R.peaked_inputs(R.TABLE_V, F32))]


@_DIV
@pytest.mark.parametrize("T", [1.0, 2.0, 3.0])
def test_closed_form_gradient_is_the_autograd_gradient_of_the_definition(div, T):
    for name, (s, tv, ti, tau, labels) in _cases(T):
        losses, n, hits, D, g = R.tail_rows(s, tv, ti, tau, labels, div, 0.3, T, R.ALPHA)
        x = s.double().requires_grad_(True)
        total = R.tail_total_autograd(x, tv, ti, tau, labels, div, 0.3, T, R.ALPHA)
        total.backward()
        assert abs(losses[0] - float(total.detach())) <= 1e-12 * abs(losses[0]), (name, losses[0], float(total.detach()))
        rel = ((x.grad - g).abs().amax(-1) / g.abs().amax(-1).clamp_min(1e-300)).max()
        assert float(rel) <= 1e-11, (name, float(rel))
        assert float(g[labels < 0].abs().max()) == 0.0
        # every gradient row sums to 0 (a softmax's logits move the loss only against each other)
        assert float(g.sum(-1).abs().max()) <= 1e-15 * max(1.0, float(g.abs().max()) * s.shape[1]), name


def test_bucket_teacher_is_the_true_teacher_restricted_to_its_top_k():
    """(1 - tau) softmax(v / T) over the stored top-K is the tempered teacher itself on those indices, and tau its mass
    elsewhere: not an approximation (up to the fp16 rounding of the stored log-probs)."""
    V, Kk = 4096, 64
    t = torch.randn(4, V, generator=torch.Generator().manual_seed(3)).double() * 3
    for T in (1.0, 2.0, 3.0):
        lp = torch.log_softmax(t, -1)
        v, i = lp.topk(Kk, -1)
        tau = R.tail_direct(t, i, T)
        true = torch.softmax(t / T, -1)
        ours = (1.0 - tau)[:, None] * torch.softmax(v / T, -1)
        assert float((ours - true.gather(-1, i)).abs().max()) <= 1e-12
        assert float((tau - (1.0 - true.gather(-1, i).sum(-1))).abs().max()) <= 1e-12


@pytest.mark.parametrize("T", [1.0, 2.0, 3.0])
def test_with_one_element_in_bucket_0_each_divergence_is_the_dense_one(T):
    """V = 8, K = 7: bucket 0 is a single element, nothing is merged, and the tail divergences are gjsd_ref's dense
    reverse_kl / jsd and the oracle's dense forward KL against the true teacher (the stored log-probs kept in fp64)."""
    V, Kk = 8, 7
    gen = torch.Generator().manual_seed(11)
    s, t = torch.randn(6, V, generator=gen) * 2, torch.randn(6, V, generator=gen) * 2
    lp = torch.log_softmax(t.double(), -1)
    order = lp.argsort(-1, descending=True)[:, :Kk]
    tv64, ti = lp.gather(-1, order), order.int()
    tau = R.tail_direct(t, ti, T)
    labels = torch.tensor([0, 1, 2, 3, 4, 5])
    Pd, on, tt, usable = R.bucket_P(tv64, ti, tau, V, T)
    assert bool(usable.all()) and int(on.sum(-1).min()) == Kk
    for div, dense in (("reverse_kl_tail", "reverse_kl"), ("jsd_tail", "jsd")):
        ours = R.divergence_terms(s, Pd, on, tt, div, 0.3, T)[0]
        theirs = G.divergence_terms(s, t, dense, 0.3, T)[0]
        assert float((ours - theirs).abs().max()) <= 1e-12, (div, ours, theirs)
    ours = R.divergence_terms(s, Pd, on, tt, "forward_kl_tail", 0.5, T)[0].mean() * T * T
    theirs = P.oracle_rows(s, labels, teacher=t, temperature=T, alpha=0.5)[0][2]
    assert abs(float(ours) - theirs) <= 1e-12 * max(1.0, abs(theirs))


@_DIV
def test_tail_divergence_is_a_lower_bound_of_the_dense_one(div):
    """Merging outcomes cannot increase a divergence: D_tail <= D_dense against the true teacher on random rows."""
    V, Kk = 512, 16
    gen = torch.Generator().manual_seed(17)
    s, t = torch.randn(32, V, generator=gen) * 2, torch.randn(32, V, generator=gen) * 2
    lp = torch.log_softmax(t.double(), -1)
    tv64, ti = lp.topk(Kk, -1)
    for T in (1.0, 2.0):
        tau = R.tail_direct(t, ti, T)
        Pd, on, tt, _ = R.bucket_P(tv64, ti.int(), tau, V, T)
        ours = R.divergence_terms(s, Pd, on, tt, div, 0.3, T)[0]
        if div == "forward_kl_tail":
            a, b = torch.log_softmax(s.double() / T, -1), torch.log_softmax(t.double() / T, -1)
            dense = (b.exp() * (b - a)).sum(-1)
        else:
            dense = G.divergence_terms(s, t, div[:-len("_tail")], 0.3, T)[0]
        assert bool((ours <= dense + 1e-13).all()) and bool((ours > 0).all()) and bool((ours < dense).any())


def test_jsd_tail_with_a_vanishing_tail_is_jsd_topk():
    """tau = 2^-100 (what a tail of 0 counts as): P is the renormalised top-K and jsd_tail is gjsd_topk_ref's jsd_topk."""
    for beta, T in R.MODES:
        s, tv, ti, _, labels = R.table_inputs(4096, F32, T)
        tau = torch.zeros(len(labels))
        ours = R.tail_rows(s, tv, ti, tau, labels, "jsd_tail", beta, T, R.ALPHA)
        theirs = K.topk_rows(s, tv, ti, labels, beta, T, R.ALPHA)
        assert ours[1:3] == theirs[1:3]
        assert all(abs(a - b) <= 1e-12 * max(1.0, abs(b)) for a, b in zip(ours[0], theirs[0])), (ours[0], theirs[0])
        assert float((ours[4] - theirs[4]).abs().max()) <= 1e-12 * float(theirs[4].abs().max())


def test_bad_tails_mask_their_rows_and_zero_counts_as_two_to_the_minus_100():
    s, tv, ti, tau, labels = R.bad_tail_inputs(R.DROP_V, F32, 2.0)
    assert math.isnan(float(tau[0])) and [float(x) for x in tau[1:4]] == [float(torch.tensor(x, dtype=torch.float32)) for x in R.BAD_TAILS[1:]]
    for div in R.DIVERGENCES:
        losses, n, hits, D, g = R.tail_rows(s, tv, ti, tau, labels, div, 0.5, 2.0, R.ALPHA)
        assert n == 4 and float(g[:3].abs().max()) == 0.0 and float(D[:3].abs().max()) == 0.0 and float(g[3].abs().max()) > 0
        tiny = tau.clone()
        tiny[3] = R.TAIL_MIN
        again = R.tail_rows(s, tv, ti, tiny, labels, div, 0.5, 2.0, R.ALPHA)
        assert again[0] == losses and torch.equal(again[4], g)


def test_dropped_entries_behave_as_absent():
    for dt in (BF, F32):
        with_, without = R.dropped_inputs(R.DROP_V, dt, 2.0)
        for div in R.DIVERGENCES:
            a = R.tail_rows(*with_, div, 0.5, 2.0, R.ALPHA)
            b = R.tail_rows(*without, div, 0.5, 2.0, R.ALPHA)
            assert a[1] == b[1] == 6 and a[2] == b[2]
            assert all(abs(x - y) <= 1e-13 * max(abs(y), 1.0) for x, y in zip(a[0], b[0])), (a[0], b[0])
            assert float((a[4] - b[4]).abs().max()) <= 1e-15 and float(a[4][6].abs().max()) == 0.0


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
    now = R.measure_tail_floor()
    assert 0 < now <= 1.25 * R.TAIL_MEASURED and 4 * R.TAIL_MEASURED <= R.TAIL_RTOL * (1 + 1e-9) <= 4.4 * R.TAIL_MEASURED


def test_underflow_rows_are_finite_in_fp32_and_only_log_q0_exists():
    for inputs, (beta, T) in R.family_cases("underflow"):
        for div in R.DIVERGENCES:
            l32, _, _, D, g32 = R.tail_rows(*inputs, div, beta, T, R.ALPHA, acc=torch.float32)
            assert all(math.isfinite(x) for x in l32) and bool(torch.isfinite(g32).all()) and bool(torch.isfinite(D).all())
            ok, why = R.tail_close(l32, g32, *[R.tail_rows(*inputs, div, beta, T, R.ALPHA)[i] for i in (0, 4)], F32, "underflow")
            assert ok, (div, why)
    s, tv, ti, tau, labels = R.underflow_inputs(R.UNDERFLOW_V, F32)
    Pd, on, _, _ = R.bucket_P(tv, ti, tau, R.UNDERFLOW_V, 1.0)
    q = torch.softmax(s.double(), -1)
    q0 = torch.where(on, torch.zeros_like(q), q).sum(-1)
    assert 0 < float(q0[0]) < 1e-60 and float(q0[0].float()) == 0.0       # q_0 is there, and not in fp32
    assert float(1.0 - torch.where(on, q, torch.zeros_like(q)).sum(-1)[0]) == 0.0   # and 1 - Q_S is 0 even in fp64


def test_direct_tail_keeps_the_digits_one_minus_the_members_loses():
    t, ti, V = R.tail_case("spike", F32)
    want = R.tail_direct(t, ti, 1.0, V)
    assert 1e-13 < float(want.max()) < 1e-10
    x = t.float()
    p = torch.softmax(x, -1)
    lossy = 1.0 - p.gather(-1, ti.long()).sum(-1)
    assert float(((lossy.double() - want).abs() / want).min()) > 0.5        # fp32 "1 - sum": no digit left
    direct32 = R.tail_direct(t, ti, 1.0, V, acc=torch.float32).double()
    assert float(((direct32 - want).abs() / want).max()) <= R.TAIL_RTOL
    # membership is by index: of 300 tied logits only the ones the top-K holds are members
    t, ti, V = R.tail_case("ties", F32)
    tied = (ti.long() >= 1000) & (ti.long() < 1300)
    assert 0 < int(tied.sum(-1).min()) and int(tied.sum(-1).max()) < 300
    by_value = torch.where(t.double() >= 9.0, torch.zeros(()).double(), (t.double() - t.double().amax(-1, keepdim=True)).exp())
    assert float((R.tail_direct(t, ti, 1.0, V) - by_value.sum(-1) / (t.double() - t.double().amax(-1, keepdim=True)).exp().sum(-1)).min()) > 1e-3


# ------------------------------------------------------------------------------------------------- Python layers, no GPU
def test_check_divergence_knows_the_tail_names():
    from speech_distill_amd import ops
    for div in R.DIVERGENCES:
        ops.check_divergence(div, 0.5)
        assert ops.TAIL_DIVERGENCES[div] == R.DIVERGENCES.index(div)
    for beta in (0.0, 1.0, float("nan")):
        ops.check_divergence("forward_kl_tail", beta)        # beta is the JSD's alone
        ops.check_divergence("reverse_kl_tail", beta)
        with pytest.raises(ValueError, match="0 < beta < 1"):
            ops.check_divergence("jsd_tail", beta)
    with pytest.raises(ValueError) as e:
        ops.check_divergence("tail", 0.5)
    for name in ("forward_kl", "reverse_kl", "jsd", "jsd_topk") + R.DIVERGENCES:
        assert repr(name) in str(e.value)


def test_tail_from_logprobs_is_the_t1_fallback():
    from speech_distill_amd import ops
    t = torch.randn(3, 5, 4096, generator=torch.Generator().manual_seed(2)) * 3
    tv, ti = L.extract_topk(t, 64)
    got = ops.tail_from_logprobs(tv)
    assert got.dtype == torch.float32 and got.shape == (3, 5)
    want = R.tail_direct(t.reshape(-1, 4096), ti.reshape(-1, 64), 1.0).reshape(3, 5)
    assert float((got.double() - want).abs().max()) <= 1e-3 and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert float(ops.tail_from_logprobs(torch.zeros(2, 4, dtype=torch.float16)).max()) == 0.0    # clamped, never negative


def test_loss_accepts_and_refuses_the_tail_divergences_before_any_launch():
    import speech_distill_amd as sda
    s, lab = torch.randn(1, 4, 64), torch.tensor([[1, 2, 3, 4]])
    topk = dict(teacher_top_k_v=torch.zeros(1, 4, 2), teacher_top_k_i=torch.zeros(1, 4, 2, dtype=torch.int64))
    rows = dict(teacher_top_k_v=topk["teacher_top_k_v"][0], teacher_top_k_i=topk["teacher_top_k_i"][0])
    for div in R.DIVERGENCES:
        dense = div[:-len("_tail")]
        fn = sda.DistillationLoss(divergence=div, beta=0.3)
        with pytest.raises(ValueError, match=f"divergence='{dense}'"):       # dense logits: pointed to the dense name
            fn(s, lab, teacher_logits=torch.randn(1, 4, 64))
        with pytest.raises(ValueError, match=f"divergence='{dense}'"):
            fn.forward_rows(s[0], lab[0], teacher_logits=torch.randn(4, 64))
        with pytest.raises(ValueError, match="teacher_top_k_tail"):          # T = 2 and no tail: the missing key is named
            fn.forward_rows(s[0], lab[0], **rows)
        with pytest.raises(ValueError, match="teacher_top_k_tail"):
            fn(s, lab, **topk)
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # with the tail: accepted up to the kernel
            fn.forward_rows(s[0], lab[0], teacher_top_k_tail=torch.full((4,), 0.1), **rows)
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # T = 1: the tail is derived
            sda.DistillationLoss(temperature=1.0, divergence=div).forward_rows(s[0], lab[0], **rows)
    for beta in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="0 < beta < 1"):
            sda.DistillationLoss(divergence="jsd_tail", beta=beta)
        sda.DistillationLoss(divergence="reverse_kl_tail", beta=beta)
    # the drop-in signature holds: the new keyword is the last one
    import inspect
    assert list(inspect.signature(sda.DistillationLoss.forward).parameters)[-2:] == ["speech_token_mask", "teacher_top_k_tail"]
    # the dense divergences still refuse a top-K teacher, tail or not
    for div in ("jsd", "reverse_kl"):
        with pytest.raises(ValueError, match="dense teacher"):
            sda.DistillationLoss(divergence=div).forward_rows(s[0], lab[0], **rows)


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


@_DIV
def test_trainer_refusal_matrix(div):
    dense = div[:-len("_tail")]
    for kw in (dict(top_k=0), dict(top_k=-1), dict(top_k=16, is_quantized_teacher=True)):
        with pytest.raises(ValueError, match=f"divergence='{dense}'"):
            _trainer(divergence=div, **kw)
    if div == "jsd_tail":
        with pytest.raises(ValueError, match="0 < beta < 1"):
            _trainer(divergence=div, beta=1.0, top_k=16)
    tr = _trainer(divergence=div, beta=0.3, top_k=16)
    assert tr.distill_loss_fn.divergence == div and tr.top_k == 16
    assert _trainer(divergence=div, top_k=16, teacher_model=None).teacher_model is None    # a pre-extracted dataset
    # a batch with pre-extracted top-K and its tail passes the trainer's own checks and reaches the kernels (no CPU form)
    batch = {"input_ids": torch.zeros(1, 4, dtype=torch.int64), "labels": torch.zeros(1, 4, dtype=torch.int64),
             "teacher_top_k_v": torch.zeros(1, 4, 2), "teacher_top_k_i": torch.zeros(1, 4, 2, dtype=torch.int64)}
    with pytest.raises(Exception) as e:
        tr.compute_loss(tr.model, dict(batch, teacher_top_k_tail=torch.full((1, 4), 0.1)))
    assert "pre-extracted" not in str(e.value) and not isinstance(e.value, ValueError), e.value
    with pytest.raises(ValueError, match="teacher model"):
        _trainer(divergence=div, top_k=16, lmbda=0.5, on_policy_generate={"max_new_tokens": 8}, teacher_model=None)
    # unchanged refusals: the dense names on a top-K teacher, and on a batch with pre-extracted keys
    with pytest.raises(ValueError, match="top_k=0"):
        _trainer(divergence=dense if dense != "forward_kl" else "jsd", top_k=100)
    old = _trainer(divergence="reverse_kl", top_k=0)
    with pytest.raises(ValueError, match="pre-extracted"):
        old.compute_loss(old.model, dict(batch, teacher_top_k_tail=torch.full((1, 4), 0.1)))


def _script(name):
    spec = importlib.util.spec_from_file_location("sd_tail_script_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@_DIV
def test_cli_accepts_the_tail_divergences_with_a_topk_teacher_only(div):
    tr = _script("train")
    dense = div[:-len("_tail")]
    assert tr.distill_kwargs(tr.parse_args(["--divergence", div, "--beta", "0.3"])) == dict(divergence=div, beta=0.3)
    assert tr.distill_kwargs(tr.parse_args(["--divergence", div, "--top_k", "16"])) == dict(divergence=div, beta=0.5)
    for extra in (["--top_k", "0"], ["--load_teacher_in_8bit"], ["--load_teacher_in_4bit"]):
        with pytest.raises(SystemExit, match=f"--divergence {dense}$"):
            tr.distill_kwargs(tr.parse_args(["--divergence", div] + extra))
    # on-policy with the default top-K teacher: the point of the feature
    kw = tr.distill_kwargs(tr.parse_args(["--divergence", div, "--lmbda", "0.5"]))
    assert kw["divergence"] == div and kw["lmbda"] == 0.5
    with pytest.raises(SystemExit, match="--padding_free"):      # unchanged
        tr.distill_kwargs(tr.parse_args(["--divergence", div, "--lmbda", "0.5", "--padding_free"]))
    with pytest.raises(SystemExit, match="--top_k 0"):           # unchanged: reverse_kl / jsd on the default top-K
        tr.distill_kwargs(tr.parse_args(["--divergence", "reverse_kl", "--lmbda", "0.5"]))


def test_train_script_exits_on_a_tail_of_another_temperature():
    tr = _script("train")

    class DS(list):
        column_names = ["student_input_ids", "teacher_top_k_tail", "teacher_top_k_tail_T"]
    ds = DS([{"teacher_top_k_tail_T": 3.0}])
    cfg = tr.parse_args(["--divergence", "reverse_kl_tail", "--temperature", "3.0"])
    tr.check_tail_temperature(ds, cfg)
    with pytest.raises(SystemExit, match="extracted at temperature 3.0"):
        tr.check_tail_temperature(ds, tr.parse_args(["--divergence", "reverse_kl_tail", "--temperature", "2.0"]))
    tr.check_tail_temperature(ds, tr.parse_args(["--divergence", "jsd_topk", "--temperature", "2.0"]))   # not a tail divergence
    plain = DS([{}])
    plain.column_names = ["student_input_ids"]
    tr.check_tail_temperature(plain, tr.parse_args(["--divergence", "reverse_kl_tail"]))                  # no such column


def test_extraction_flag_and_columns():
    ex = _script("extract_teacher_logits")
    base = ["--teacher_model_path", "m", "--dataset_path", "d", "--output_path", "o"]
    assert ex.parse_args(base).tail_temperature is None                      # default: off
    assert ex.parse_args(base + ["--tail_temperature", "2"]).tail_temperature == 2.0
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            ex.parse_args(base + ["--tail_temperature", bad])
    assert ex.tail_columns(None, None) == {}
    import numpy as np
    import pyarrow as pa
    cols = ex.tail_columns([np.array([0.25, 0.5], dtype=np.float32), np.array([0.125], dtype=np.float32)], 2.0)
    assert list(cols) == ["teacher_top_k_tail", "teacher_top_k_tail_T"]
    assert cols["teacher_top_k_tail"].type == pa.list_(pa.float32()) and cols["teacher_top_k_tail"].to_pylist() == [[0.25, 0.5], [0.125]]
    assert cols["teacher_top_k_tail_T"].type == pa.float32() and cols["teacher_top_k_tail_T"].to_pylist() == [2.0, 2.0]


def _features(with_tail):
    g = torch.Generator().manual_seed(4)
    out = []
    for n, nt in ((5, 5), (3, 4), (6, 2)):          # the top-K blocks are as long as, longer and shorter than the student row
        f = {"student_input_ids": torch.randint(1, 50, (n,), generator=g).tolist(), "student_attention_mask": [1] * n,
             "teacher_input_ids": torch.randint(1, 50, (n,), generator=g).tolist(), "teacher_attention_mask": [1] * n,
             "teacher_top_k_v": torch.randn(nt, 4, generator=g).half().numpy(), "teacher_top_k_i": torch.randint(0, 50, (nt, 4), generator=g).int().numpy()}
        if with_tail:
            f["teacher_top_k_tail"] = (torch.rand(nt, generator=g) * 0.5).tolist()
            f["teacher_top_k_tail_T"] = 2.0
        out.append(f)
    return out


@pytest.mark.parametrize("padding_free", [False, True])
def test_collator_passes_the_tail_through_with_pad_one(padding_free):
    from speech_distill_amd.collator import ProcessedDataCollator
    tok = types.SimpleNamespace(encode=lambda *a, **k: [])
    coll = ProcessedDataCollator(tok, pad_token_id=0, **({"padding_free": True} if padding_free else {}))
    feats = _features(True)
    batch = coll(feats)
    tail = batch["teacher_top_k_tail"]
    assert tail.dtype == torch.float32 and tuple(tail.shape) == tuple(batch["teacher_top_k_v"].shape[:2])
    assert "teacher_top_k_tail_T" not in batch
    lens = [len(f["student_input_ids"]) for f in feats]
    at = 0
    for b, (f, n) in enumerate(zip(feats, lens)):
        row = tail[0, at:at + n] if padding_free else tail[b]
        have = min(n if padding_free else tail.shape[1], len(f["teacher_top_k_tail"]))   # cut at the sample's / the batch's width
        assert torch.equal(row[:have], torch.tensor(f["teacher_top_k_tail"][:have], dtype=torch.float32))
        assert bool((row[have:] == 1.0).all())                     # cut or padded like the top-K blocks, pad value 1.0
        v = batch["teacher_top_k_v"][0, at:at + n] if padding_free else batch["teacher_top_k_v"][b]
        assert bool((v[have:] == 0).all())
        at += n if padding_free else 0
    # without the column: the same batch less that key (nothing else reads it)
    plain = coll([{k: v for k, v in f.items() if not k.startswith("teacher_top_k_tail")} for f in feats])
    assert list(plain) == [k for k in batch if k != "teacher_top_k_tail"]
    for k in plain:
        assert torch.equal(plain[k], batch[k]) if torch.is_tensor(plain[k]) else plain[k] == batch[k]
