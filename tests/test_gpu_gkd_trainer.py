"""-m gpu: DistillationTrainer with the new divergences and on-policy micro-batches, on the tiny configuration of
tests/test_gpu_trainer.py (student 640/128/256/2 layers, teacher 640/256/512/2 layers), B = 2, T = 64, prompts of 12 and
20 tokens: (a) a jsd step against tests/gjsd_ref.py, (b) lmbda = 1 with a rollout that returns the dataset's own
completion changes nothing, (c) a real greedy rollout, (d) the defaults are bit for bit today's trainer."""
import tempfile

import pytest
import torch

import gjsd_ref as G
from gpu_util import dev, record, to_dev

pytestmark = pytest.mark.gpu

B, T, V, PAD = 2, 64, 640, 639
PROMPTS = (12, 20)
GREEDY = {"max_new_tokens": 64, "top_k": 1, "temperature": 1.0}


@pytest.fixture(scope="module")
def sda():
    import speech_distill_amd as m
    m.load_lib()
    return m


def _rows(n=2, seed=11):
    """n micro-batches of B rows: random tokens below the pad id, labels -100 on the prompt."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n * B):
        b = len(out) % B
        ids = torch.randint(0, PAD, (T,), generator=g)
        labels = ids.clone()
        labels[:PROMPTS[b]] = -100
        out.append({"input_ids": ids, "attention_mask": torch.ones(T, dtype=torch.int64), "labels": labels,
                    "teacher_input_ids": ids.clone(), "teacher_attention_mask": torch.ones(T, dtype=torch.int64)})
    return out


def _collate(feats):
    return {k: torch.stack([f[k] for f in feats]) for k in feats[0]}


def _batch(mb=0):
    return {k: to_dev(v) for k, v in _collate(_rows()[mb * B:(mb + 1) * B]).items()}


def _trainer(sda, rows=None, max_steps=-1, **kw):
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 128, 256, 2, 2, 1), device=dev(), seed=0)
    teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 256, 512, 2, 4, 2), device=dev(), seed=1)
    teacher.eval().requires_grad_(False)
    args = TrainingArguments(
        output_dir=tempfile.mkdtemp(), per_device_train_batch_size=B, gradient_accumulation_steps=1, max_steps=max_steps,
        learning_rate=1e-3, logging_steps=1, save_strategy="no", report_to=[], remove_unused_columns=False,
        label_names=["labels"], seed=42, data_seed=42, lr_scheduler_type="constant", warmup_steps=0, weight_decay=0.0,
        max_grad_norm=1.0, dataloader_num_workers=0, bf16=True)
    kw.setdefault("top_k", 0)
    tr = DistillationTrainer(model=student, args=args, train_dataset=rows, data_collator=_collate, teacher_model=teacher,
                             temperature=2.0, alpha=0.5, **kw)
    tr.logged = []
    tr.log = lambda d, *a, **k: tr.logged.append(dict(d))
    tr.current_gradient_accumulation_steps = 1   # HF's loop sets it; training_step is called directly below
    return tr, student, teacher


def _step(tr, student, batch):
    student.zero_grad()
    loss = tr.training_step(student, dict(batch))
    torch.cuda.synchronize()
    return float(loss), student.flat_grad.clone()


def test_a_jsd_step_matches_the_reference_on_recomputed_logits(sda):
    tr, student, teacher = _trainer(sda, divergence="jsd", beta=0.5)
    batch = _batch()
    loss, grad = _step(tr, student, batch)
    with torch.no_grad():
        s = student(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"]).logits
        t = teacher(input_ids=batch["teacher_input_ids"], attention_mask=batch["teacher_attention_mask"]).logits
    lab = batch["labels"].cpu()
    nxt = torch.full_like(lab, -100)
    nxt[:, :-1] = lab[:, 1:]
    keep = (nxt != -100).reshape(-1)
    ref, n, _, _ = G.gjsd_rows(s.reshape(-1, V).cpu()[keep], t.reshape(-1, V).cpu()[keep], nxt.reshape(-1)[keep], "jsd", 0.5, 2.0,
                               0.5)
    assert n == (T - 12) + (T - 20)
    record("gkd_trainer_jsd_step", loss=loss, ref=ref[0], logged=tr.logged[-1])
    assert abs(loss - ref[0]) <= 2e-2 * abs(ref[0])     # the bound of test_c1_compute_loss_matches_reference
    got3 = [tr.logged[-1]["student_loss"], tr.logged[-1]["distill_loss"], tr.logged[-1]["teacher_loss"]]
    for got, want in zip(got3, ref[1:]):
        assert abs(got - want) <= 3e-2 * abs(want), (got3, ref)
    assert "on_policy_fraction" not in tr.logged[-1]
    assert bool(torch.isfinite(grad.float()).all()) and float(grad.float().abs().max()) > 0
    with pytest.raises(ValueError, match="pre-extracted teacher_top_k_v"):
        tr.compute_loss(student, dict(batch, teacher_top_k_v=torch.zeros(B, T, 4), teacher_top_k_i=torch.zeros(B, T, 4)))


def test_b_a_rollout_that_returns_the_datasets_completion_changes_nothing(sda):
    batch = _batch()
    tr0, student0, _ = _trainer(sda, divergence="reverse_kl")
    loss0, grad0 = _step(tr0, student0, batch)
    tr1, student1, _ = _trainer(sda, divergence="reverse_kl", lmbda=1.0, on_policy_generate=dict(GREEDY))
    calls = []

    def stub(input_ids, attention_mask=None, max_new_tokens=20, seed=None, **kw):
        plen = attention_mask.sum(1)
        assert plen.tolist() == list(PROMPTS) and max_new_tokens == T - min(PROMPTS)
        cols = (plen[:, None] + torch.arange(max_new_tokens, device=input_ids.device)[None, :]).clamp_max(T - 1)
        calls.append(seed)
        return torch.cat([input_ids, input_ids.gather(1, cols)], 1)
    student1.generate = stub
    seen = []
    inner = tr1.compute_loss
    tr1.compute_loss = lambda model, inputs, *a, **k: (seen.append({x: y.clone() for x, y in inputs.items()}),
                                                       inner(model, inputs, *a, **k))[1]
    loss1, grad1 = _step(tr1, student1, batch)
    assert len(calls) == 1 and isinstance(calls[0], int)
    assert set(seen[0]) == set(batch) and all(torch.equal(seen[0][k], batch[k]) for k in batch)
    assert loss1 == loss0 and torch.equal(grad1, grad0)
    assert tr1.logged[-1]["on_policy_fraction"] == 1.0


def test_b_a_rollout_that_ends_at_once_in_every_row_is_a_zero_step(sda):
    """EOS == pad (what scripts/train.py passes) as the first token of every row: the completion is one attended EOS whose
    label is -100 by the collator's rule, so the batch has no loss row.  The step returns a zero loss and a zero gradient
    instead of failing."""
    batch = _batch()
    tr, student, _ = _trainer(sda, divergence="jsd", beta=0.5, lmbda=1.0,
                              on_policy_generate=dict(GREEDY, eos_token_id=PAD, pad_token_id=PAD))
    student.generate = lambda input_ids, max_new_tokens=20, **kw: torch.cat(
        [input_ids, torch.full((B, max_new_tokens), PAD, device=input_ids.device)], 1)
    seen = []
    inner = tr.compute_loss
    tr.compute_loss = lambda model, inputs, *a, **k: (seen.append({x: y.clone() for x, y in inputs.items()}),
                                                      inner(model, inputs, *a, **k))[1]
    loss, grad = _step(tr, student, batch)
    assert bool((seen[0]["labels"] == -100).all())
    assert seen[0]["attention_mask"].sum(1).tolist() == [p + 1 for p in PROMPTS]
    assert loss == 0.0 and float(grad.float().abs().max()) == 0.0
    assert [tr.logged[-1][k] for k in ("student_loss", "teacher_loss", "distill_loss")] == [0.0, 0.0, 0.0]
    # evaluation on the same kind of batch (the [B,T,V] form) neither fails nor touches the on-policy counters
    tr._on_policy_seen = [3, 4]
    student.eval()
    with torch.no_grad():
        ev = tr.compute_loss(student, dict(seen[0]), return_outputs=True)[0]
    student.train()
    assert float(ev) == 0.0 and tr._on_policy_seen == [3, 4] and "on_policy_fraction" not in tr.logged[-1]


def test_c_greedy_rollout_feeds_the_students_own_tokens(sda):
    batch = _batch()
    tr, student, _ = _trainer(sda, divergence="jsd", beta=0.5, lmbda=1.0, on_policy_generate=dict(GREEDY))
    real, calls, seen = student.generate, [], []

    def spy(input_ids, **kw):
        calls.append((input_ids.clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}))
        return real(input_ids, **kw)
    student.generate = spy
    inner = tr.compute_loss
    tr.compute_loss = lambda model, inputs, *a, **k: (seen.append({x: y.clone() for x, y in inputs.items()}),
                                                      inner(model, inputs, *a, **k))[1]
    student.train()
    flat = student.flat.clone()
    loss, grad = _step(tr, student, batch)
    assert torch.equal(student.flat, flat)                      # the rollout (and the step: no optimizer) left the weights
    assert student.training and len(calls) == 1
    assert loss == loss and abs(loss) < float("inf") and float(grad.float().abs().max()) > 0
    # the same call, made by the test: same prompts, keywords and seed -> the completion handed to compute_loss
    ids, kw = calls[0]
    assert kw["max_new_tokens"] == T - min(PROMPTS) and kw["top_k"] == 1 and isinstance(kw["seed"], int)
    again = real(ids, **kw)[:, T:]
    got = seen[0]
    for b, p in enumerate(PROMPTS):
        assert torch.equal(got["input_ids"][b, :p], batch["input_ids"][b, :p])
        assert torch.equal(got["input_ids"][b, p:], again[b, :T - p])
        assert torch.equal(got["teacher_input_ids"][b, p:], again[b, :T - p])
        assert torch.equal(got["labels"][b, :p], torch.full((p,), -100, device=dev()))
        want = again[b, :T - p]
        assert torch.equal(got["labels"][b, p:], want)          # no pad / eos id was given: every token is a target
    assert not torch.equal(got["input_ids"], batch["input_ids"])
    assert bool(got["attention_mask"].all()) and got["input_ids"].shape == (B, T)
    assert tr.logged[-1]["on_policy_fraction"] == 1.0


def test_c_two_runs_with_one_seed_end_at_the_same_weights(sda):
    def run():
        tr, student, _ = _trainer(sda, rows=_rows(n=3), max_steps=3, divergence="jsd", beta=0.5, lmbda=1.0,
                                  on_policy_generate=dict(GREEDY, top_k=8, max_new_tokens=24))
        tr._get_train_sampler = lambda *a, **k: torch.utils.data.SequentialSampler(tr.train_dataset)
        start = student.flat.clone()
        tr.train()
        assert tr.state.global_step == 3 and not torch.equal(student.flat, start)
        fr = [h["on_policy_fraction"] for h in tr.logged if "on_policy_fraction" in h]
        assert fr and all(f == 1.0 for f in fr)
        return student.flat.clone()
    assert torch.equal(run(), run())


def test_d_defaults_are_todays_trainer_bit_for_bit(sda):
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    batch = _batch()
    res = []
    for new_keywords in (False, True):
        student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 128, 256, 2, 2, 1), device=dev(), seed=0)
        teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 256, 512, 2, 4, 2), device=dev(), seed=1)
        teacher.eval().requires_grad_(False)
        args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False,
                                 label_names=["labels"], save_strategy="no", logging_steps=1, bf16=True)
        kw = dict(divergence="forward_kl", beta=0.5, lmbda=0.0, on_policy_generate=None) if new_keywords else {}
        for top_k in (16, 0):
            tr = DistillationTrainer(model=student, args=args, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=top_k,
                                     **kw)
            tr.log = lambda d, *a, **k: None
            tr.current_gradient_accumulation_steps = 1
            res.append(_step(tr, student, batch))
    for (la, ga), (lb, gb) in zip(res[:2], res[2:]):
        assert la == lb and torch.equal(ga, gb)
