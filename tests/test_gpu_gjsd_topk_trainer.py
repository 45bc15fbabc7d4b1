"""-m gpu: DistillationTrainer with divergence="jsd_topk" on one-layer models (V = 2048): a live teacher at top_k = 16, a
batch with pre-extracted top-K and no teacher model, a packed batch, one optimizer step, an on-policy micro-step, and
the default trainer untouched by all of it.

``compute_loss`` is compared with ``DistillationLoss.forward_rows`` on rows and top-K taken by hand: a spy on the loss
records what the trainer hands it; the rows' labels and the top-K must be exactly the hand-made ones, the student logits
the model's logits of those rows, and the loss bit for bit the loss of a second call on them."""
import tempfile

import pytest
import torch

from gpu_util import dev, record, to_dev

pytestmark = pytest.mark.gpu

V, PAD, BOS, K = 2048, 2047, 2046, 16
ST, TE = (V, 128, 256, 1, 2, 1), (V, 256, 512, 1, 4, 2)
LENS, PROMPTS = (48, 33, 64, 21), (12, 20, 5, 9)


class _Tok:
    pad_token = "<|semantic_token_end|>"
    pad_token_id = PAD

    def encode(self, text, add_special_tokens=False):
        return [BOS]


@pytest.fixture(scope="module")
def sda():
    import speech_distill_amd as m
    m.load_lib()
    return m


def _feats(seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n, p in zip(LENS, PROMPTS):
        ids = torch.randint(0, BOS, (n,), generator=g)
        ids[p] = BOS
        ids = ids.tolist()
        out.append({"student_input_ids": ids, "student_attention_mask": [1] * n, "teacher_input_ids": list(ids),
                    "teacher_attention_mask": [1] * n})
    return out


def _collator(padding_free=False):
    from speech_distill_amd.collator import ProcessedDataCollator
    return ProcessedDataCollator(_Tok(), pad_token_id=PAD, **({"padding_free": True} if padding_free else {}))


def _on_dev(batch):
    return {k: (to_dev(v) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _trainer(sda, teacher="build", rows=None, collator=None, max_steps=-1, **kw):
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*ST), device=dev(), seed=0)
    if teacher == "build":
        teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*TE), device=dev(), seed=1)
        teacher.eval().requires_grad_(False)
    args = TrainingArguments(
        output_dir=tempfile.mkdtemp(), per_device_train_batch_size=4, gradient_accumulation_steps=1, max_steps=max_steps,
        learning_rate=1e-3, logging_steps=1, save_strategy="no", report_to=[], remove_unused_columns=False,
        label_names=["labels"], seed=42, data_seed=42, lr_scheduler_type="constant", warmup_steps=0, weight_decay=0.0,
        max_grad_norm=1.0, dataloader_num_workers=0, bf16=True)
    kw.setdefault("divergence", "jsd_topk")
    kw.setdefault("beta", 0.3)
    kw.setdefault("top_k", K)
    tr = DistillationTrainer(model=student, args=args, train_dataset=rows, data_collator=collator or _collator(),
                             teacher_model=teacher, temperature=2.0, alpha=0.5, **kw)
    tr.logged = []
    tr.log = lambda d, *a, **k: tr.logged.append(dict(d))
    tr.current_gradient_accumulation_steps = 1   # HF's loop sets it; training_step is called directly below
    tr.overlap_teacher = False   # (beside a teacher the student's GEMMs take another tile: SD_FWD_CONCURRENT)
    return tr, student, teacher


def _spy(tr):
    """Record what compute_loss hands the loss (the logits are cloned: the training step overwrites them in place)."""
    seen = []
    inner = tr.distill_loss_fn.forward_rows

    def forward_rows(student_logits, row_labels, teacher_logits=None, teacher_top_k_v=None, teacher_top_k_i=None):
        seen.append(dict(s=student_logits.detach().clone(), labels=row_labels.clone(), t=teacher_logits,
                         v=teacher_top_k_v.clone(), i=teacher_top_k_i.clone()))
        return inner(student_logits, row_labels, teacher_logits=teacher_logits, teacher_top_k_v=teacher_top_k_v,
                     teacher_top_k_i=teacher_top_k_i)
    tr.distill_loss_fn.forward_rows = forward_rows
    return seen


def _step(tr, student, batch):
    student.zero_grad()
    loss = tr.training_step(student, dict(batch))
    torch.cuda.synchronize()
    return float(loss), student.flat_grad.clone()


def _by_hand(sda, got, loss, rows, row_labels, tv, ti, logits):
    """The spy's record against the hand-made rows / top-K / logits, and the step's loss against a second loss call."""
    assert got["t"] is None and torch.equal(got["labels"], row_labels)
    assert got["v"].shape == (rows.numel(), K) and torch.equal(got["v"], tv) and torch.equal(got["i"].int(), ti.int())
    assert got["s"].shape == logits.shape and torch.equal(got["s"], logits)
    fn = sda.DistillationLoss(2.0, 0.5, divergence="jsd_topk", beta=0.3)
    again = fn.forward_rows(got["s"], row_labels, teacher_top_k_v=tv, teacher_top_k_i=ti)
    assert float(again[0]) == loss and loss > 0
    return [float(x) for x in again]


def test_live_teacher_step_equals_forward_rows_on_rows_and_topk_taken_by_hand(sda):
    from speech_distill_amd import ops
    tr, student, teacher = _trainer(sda)
    seen = _spy(tr)
    batch = _on_dev(_collator()(_feats()))
    loss, grad = _step(tr, student, batch)
    rows, row_labels = ops.loss_rows(batch["labels"])
    assert rows.numel() == sum(n - p for n, p in zip(LENS, PROMPTS))   # the BOS at p is the first label
    with torch.no_grad():
        t = teacher(input_ids=batch["teacher_input_ids"], attention_mask=batch["teacher_attention_mask"], logit_rows=rows).logits
        tv, ti = ops.logsoftmax_topk(t, K, V)
        s = student(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], logit_rows=rows).logits
    again = _by_hand(sda, seen[0], loss, rows, row_labels, tv, ti, s)
    record("gjsd_topk_trainer_live", loss=loss, again=again, logged=tr.logged[-1])
    assert [tr.logged[-1][k] for k in ("student_loss", "distill_loss", "teacher_loss")] == again[1:]
    assert "on_policy_fraction" not in tr.logged[-1]
    assert bool(torch.isfinite(grad.float()).all()) and float(grad.float().abs().max()) > 0


def _pre_extracted(sda, teacher, feats):
    """Per-sample [len, K] top-K of the teacher's full logits, as the offline extraction stores them."""
    from speech_distill_amd import ops
    out = []
    with torch.no_grad():
        for f in feats:
            ids = to_dev(torch.tensor([f["teacher_input_ids"]]))
            v, i = ops.logsoftmax_topk(teacher(input_ids=ids, attention_mask=torch.ones_like(ids)).logits, K, V)
            out.append(dict(f, teacher_top_k_v=v[0].cpu(), teacher_top_k_i=i[0].cpu()))
    return out


def test_pre_extracted_batch_without_a_teacher_model(sda):
    from speech_distill_amd import ops
    _, _, teacher = _trainer(sda)
    feats = _pre_extracted(sda, teacher, _feats())
    tr, student, none = _trainer(sda, teacher=None)
    assert none is None and tr.teacher_model is None
    seen = _spy(tr)
    batch = _on_dev(_collator()(feats))
    assert batch["teacher_top_k_v"].shape == (4, max(LENS), K)
    loss, grad = _step(tr, student, batch)
    rows, row_labels = ops.loss_rows(batch["labels"])
    with torch.no_grad():
        s = student(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], logit_rows=rows).logits
    tv, ti = batch["teacher_top_k_v"].reshape(-1, K)[rows], batch["teacher_top_k_i"].reshape(-1, K)[rows]
    _by_hand(sda, seen[0], loss, rows, row_labels, tv.half(), ti, s)
    assert float(grad.float().abs().max()) > 0
    # the [B,T,V] path of evaluation gives the same loss from the same logits
    student.eval()
    with torch.no_grad():
        ev, outputs = tr.compute_loss(student, dict(batch), return_outputs=True)
    student.train()
    assert outputs.logits.shape == (4, max(LENS), V)
    assert abs(float(ev) - loss) <= 2e-3 * loss, (float(ev), loss)   # (the lm_head of all rows takes another GEMM shape)


def test_packed_batch_against_the_padded_one(sda):
    from speech_distill_amd import ops
    tr0, student0, _ = _trainer(sda)
    padded_loss, _ = _step(tr0, student0, _on_dev(_collator()(_feats())))
    tr, student, teacher = _trainer(sda, collator=_collator(True))
    seen = _spy(tr)
    batch = _on_dev(_collator(True)(_feats()))
    assert "attention_mask" not in batch and batch["input_ids"].shape == (1, sum(LENS))
    loss, grad = _step(tr, student, batch)
    rows, row_labels, _, _ = ops.packed_rows(batch["labels"], batch["cu_seq_lens_q"], None, batch["position_ids"])
    assert rows.numel() == sum(n - p for n, p in zip(LENS, PROMPTS))   # the BOS at p is the first label
    packed = {k: batch[k] for k in tr.PACKED_KEYS}
    with torch.no_grad():
        t = teacher(input_ids=batch["teacher_input_ids"], logit_rows=rows, **packed).logits
        tv, ti = ops.logsoftmax_topk(t, K, V)
        s = student(input_ids=batch["input_ids"], logit_rows=rows, **packed).logits
    again = _by_hand(sda, seen[0], loss, rows, row_labels, tv, ti, s)
    record("gjsd_topk_trainer_packed", loss=loss, padded=padded_loss, logged=tr.logged[-1])
    # the same samples, padded: the bounds test_gpu_distill_packed.py applies to the forward KL
    assert abs(loss - padded_loss) <= 2e-2 * abs(padded_loss), (loss, padded_loss)
    for k in ("student_loss", "distill_loss", "teacher_loss"):
        assert abs(tr.logged[-1][k] - tr0.logged[-1][k]) <= 3e-2 * abs(tr0.logged[-1][k]), k
    assert float(grad.float().abs().max()) > 0
    with pytest.raises(ValueError, match="lmbda > 0 with a packed batch"):
        tr.lmbda = 0.5
        tr.training_step(student, dict(batch))


class _DS(torch.utils.data.Dataset):
    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return dict(self.rows[i])


def test_one_optimizer_step_moves_the_weights(sda):
    tr, student, _ = _trainer(sda, rows=_DS(_feats() * 2), max_steps=1)
    start = student.flat.clone()
    tr.train()
    assert tr.state.global_step == 1 and not torch.equal(student.flat, start)
    assert bool(torch.isfinite(student.flat.float()).all())
    assert any("distill_loss" in h and h["distill_loss"] > 0 for h in tr.logged)


def test_on_policy_micro_step_runs_and_logs_its_fraction(sda):
    tr, student, _ = _trainer(sda, lmbda=1.0, on_policy_generate={"max_new_tokens": 8, "top_k": 1, "temperature": 1.0})
    seen = _spy(tr)
    batch = _on_dev(_collator()(_feats()))
    loss, grad = _step(tr, student, batch)
    assert loss == loss and 0 < loss < float("inf") and float(grad.float().abs().max()) > 0
    assert tr.logged[-1]["on_policy_fraction"] == 1.0
    assert seen[0]["v"].shape[1] == K and seen[0]["t"] is None
    # pre-extracted batches cannot be rolled out: there is no teacher distribution for the student's own tokens
    with pytest.raises(ValueError, match="teacher model"):
        tr.training_step(student, dict(batch, teacher_top_k_v=torch.zeros(4, max(LENS), K, device=dev()),
                                       teacher_top_k_i=torch.zeros(4, max(LENS), K, dtype=torch.int32, device=dev())))


def test_the_default_trainer_is_untouched(sda):
    """The forward-KL trainer's loss and gradient on one batch, before and after a jsd_topk step in the same process."""
    batch = _on_dev(_collator()(_feats()))

    def default():
        tr, student, _ = _trainer(sda, divergence="forward_kl", beta=0.5)
        return _step(tr, student, batch)
    l0, g0 = default()
    tr, student, _ = _trainer(sda)
    _step(tr, student, batch)
    l1, g1 = default()
    assert l0 == l1 and torch.equal(g0, g1)
