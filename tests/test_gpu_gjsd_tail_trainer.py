"""-m gpu: DistillationTrainer with the tail-bucket divergences on one-layer models (V = 2048): a live teacher at
top_k = 16 (its pass also returns the tail), a batch with pre-extracted top-K and tail and no teacher model, a packed
batch, an on-policy training step at the default kind of teacher, and the temperature-1 fallback.

``compute_loss`` is compared with the same launches composed by hand: a spy on the loss records what the trainer hands it;
the rows' labels, the top-K and the tail must be exactly the hand-made ones (``ops.logsoftmax_topk`` + ``ops.topk_tail``
on the teacher's logits of the hand-selected rows), the student logits the model's logits of those rows, and the losses
and the student's flat gradient ``torch.equal`` to those of a second student taken through the same calls by hand."""
import tempfile

import pytest
import torch

from gpu_util import dev, record, to_dev

pytestmark = pytest.mark.gpu

V, PAD, BOS, K = 2048, 2047, 2046, 16
ST, TE = (V, 128, 256, 1, 2, 1), (V, 256, 512, 1, 4, 2)
LENS, PROMPTS = (48, 33, 64, 21), (12, 20, 5, 9)
TEMP = 2.0


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


def _trainer(sda, teacher="build", collator=None, temperature=TEMP, **kw):
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*ST), device=dev(), seed=0)
    if teacher == "build":
        teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*TE), device=dev(), seed=1)
        teacher.eval().requires_grad_(False)
    args = TrainingArguments(
        output_dir=tempfile.mkdtemp(), per_device_train_batch_size=4, gradient_accumulation_steps=1, max_steps=-1,
        learning_rate=1e-3, logging_steps=1, save_strategy="no", report_to=[], remove_unused_columns=False,
        label_names=["labels"], seed=42, data_seed=42, lr_scheduler_type="constant", warmup_steps=0, weight_decay=0.0,
        max_grad_norm=1.0, dataloader_num_workers=0, bf16=True)
    kw.setdefault("divergence", "reverse_kl_tail")
    kw.setdefault("beta", 0.3)
    kw.setdefault("top_k", K)
    tr = DistillationTrainer(model=student, args=args, train_dataset=None, data_collator=collator or _collator(),
                             teacher_model=teacher, temperature=temperature, alpha=0.5, **kw)
    tr.logged = []
    tr.log = lambda d, *a, **k: tr.logged.append(dict(d))
    tr.current_gradient_accumulation_steps = 1   # HF's loop sets it; training_step is called directly below
    tr.overlap_teacher = False   # (beside a teacher the student's GEMMs take another tile: SD_FWD_CONCURRENT)
    return tr, student, teacher


def _spy(tr):
    """Record what compute_loss hands the loss (the logits are cloned: the training step overwrites them in place)."""
    seen = []
    inner = tr.distill_loss_fn.forward_rows

    def forward_rows(student_logits, row_labels, teacher_logits=None, teacher_top_k_v=None, teacher_top_k_i=None,
                     teacher_top_k_tail=None):
        seen.append(dict(s=student_logits.detach().clone(), labels=row_labels.clone(), t=teacher_logits,
                         v=teacher_top_k_v.clone(), i=teacher_top_k_i.clone(),
                         tail=None if teacher_top_k_tail is None else teacher_top_k_tail.clone()))
        return inner(student_logits, row_labels, teacher_logits=teacher_logits, teacher_top_k_v=teacher_top_k_v,
                     teacher_top_k_i=teacher_top_k_i, teacher_top_k_tail=teacher_top_k_tail)
    tr.distill_loss_fn.forward_rows = forward_rows
    return seen


def _step(tr, student, batch):
    student.zero_grad()
    loss = tr.training_step(student, dict(batch))
    torch.cuda.synchronize()
    return float(loss), student.flat_grad.clone()


def _by_hand(sda, div, got, loss, grad, rows, row_labels, tv, ti, tail, model_kw, temperature=TEMP):
    """The spy's record against the hand-made rows / top-K / tail, then the same launches composed by hand on a second
    student with the same weights: its losses and flat gradient are the step's, bit for bit."""
    assert got["t"] is None and torch.equal(got["labels"], row_labels)
    assert got["v"].shape == (rows.numel(), K) and torch.equal(got["v"], tv) and torch.equal(got["i"].int(), ti.int())
    assert got["tail"].dtype == torch.float32 and got["tail"].shape == (rows.numel(),) and torch.equal(got["tail"], tail)
    twin = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*ST), device=dev(), seed=0)
    twin.zero_grad()
    s = twin(logit_rows=rows, **model_kw).logits
    assert torch.equal(s.detach(), got["s"])
    fn = sda.DistillationLoss(temperature, 0.5, divergence=div, beta=0.3, inplace_grad=True)
    again = fn.forward_rows(s, row_labels, teacher_top_k_v=tv, teacher_top_k_i=ti, teacher_top_k_tail=tail)
    again[0].backward()
    torch.cuda.synchronize()
    assert float(again[0]) == loss and loss > 0 and float(again[2]) > 0
    assert torch.equal(twin.flat_grad, grad) and float(grad.float().abs().max()) > 0
    return [float(x) for x in again]


@pytest.mark.parametrize("div", ["reverse_kl_tail", "jsd_tail", "forward_kl_tail"])
def test_live_teacher_step_equals_the_same_launches_composed_by_hand(sda, div):
    from speech_distill_amd import ops
    tr, student, teacher = _trainer(sda, divergence=div)
    seen = _spy(tr)
    batch = _on_dev(_collator()(_feats()))
    loss, grad = _step(tr, student, batch)
    rows, row_labels = ops.loss_rows(batch["labels"])
    assert rows.numel() == sum(n - p for n, p in zip(LENS, PROMPTS))   # the BOS at p is the first label
    with torch.no_grad():
        t = teacher(input_ids=batch["teacher_input_ids"], attention_mask=batch["teacher_attention_mask"], logit_rows=rows).logits
        tv, ti = ops.logsoftmax_topk(t, K, V)
        tail = ops.topk_tail(t, ti, TEMP, V)
    assert 0.0 < float(tail.min()) and float(tail.max()) < 1.0
    again = _by_hand(sda, div, seen[0], loss, grad, rows, row_labels, tv, ti, tail,
                     dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"]))
    record("gjsd_tail_trainer_live_" + div, loss=loss, again=again, logged=tr.logged[-1])
    assert [tr.logged[-1][k] for k in ("student_loss", "distill_loss", "teacher_loss")] == again[1:]


def _pre_extracted(sda, teacher, feats, tail_temperature=TEMP):
    """Per-sample [len, K] top-K and [len] tails of the teacher's full logits, as the offline extraction stores them."""
    from speech_distill_amd import ops
    out = []
    with torch.no_grad():
        for f in feats:
            ids = to_dev(torch.tensor([f["teacher_input_ids"]]))
            logits = teacher(input_ids=ids, attention_mask=torch.ones_like(ids)).logits
            v, i = ops.logsoftmax_topk(logits, K, V)
            g = dict(f, teacher_top_k_v=v[0].cpu(), teacher_top_k_i=i[0].cpu())
            if tail_temperature is not None:
                g.update(teacher_top_k_tail=ops.topk_tail(logits, i, tail_temperature, V)[0].cpu(), teacher_top_k_tail_T=tail_temperature)
            out.append(g)
    return out


def test_pre_extracted_batch_with_its_tail_and_no_teacher_model(sda):
    from speech_distill_amd import ops
    _, _, teacher = _trainer(sda)
    feats = _pre_extracted(sda, teacher, _feats())
    tr, student, none = _trainer(sda, teacher=None)
    assert none is None and tr.teacher_model is None
    seen = _spy(tr)
    batch = _on_dev(_collator()(feats))
    assert batch["teacher_top_k_tail"].shape == (4, max(LENS)) and batch["teacher_top_k_tail"].dtype == torch.float32
    assert float(batch["teacher_top_k_tail"][3, LENS[3]:].min()) == 1.0      # padded positions: tail 1
    loss, grad = _step(tr, student, batch)
    rows, row_labels = ops.loss_rows(batch["labels"])
    tv, ti = batch["teacher_top_k_v"].reshape(-1, K)[rows], batch["teacher_top_k_i"].reshape(-1, K)[rows]
    tail = batch["teacher_top_k_tail"].reshape(-1)[rows]
    _by_hand(sda, "reverse_kl_tail", seen[0], loss, grad, rows, row_labels, tv.half(), ti, tail,
             dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"]))
    # the [B,T,V] path of evaluation gives the same loss from the same logits
    student.eval()
    with torch.no_grad():
        ev, outputs = tr.compute_loss(student, dict(batch), return_outputs=True)
    student.train()
    assert outputs.logits.shape == (4, max(LENS), V)
    assert abs(float(ev) - loss) <= 2e-3 * loss, (float(ev), loss)   # (the lm_head of all rows takes another GEMM shape)
    # without the tail column at T = 2 the step names the missing key
    with pytest.raises(ValueError, match="teacher_top_k_tail"):
        tr.training_step(student, {k: v for k, v in batch.items() if k != "teacher_top_k_tail"})


def test_temperature_one_fallback_for_a_dataset_without_tails(sda):
    from speech_distill_amd import ops
    _, _, teacher = _trainer(sda)
    feats = _pre_extracted(sda, teacher, _feats(), tail_temperature=None)
    tr, student, _ = _trainer(sda, teacher=None, temperature=1.0)
    seen = _spy(tr)
    batch = _on_dev(_collator()(feats))
    assert "teacher_top_k_tail" not in batch
    loss, grad = _step(tr, student, batch)
    assert seen[0]["tail"] is None                               # the loss derives it from the stored log-probs
    rows, row_labels = ops.loss_rows(batch["labels"])
    tv, ti = batch["teacher_top_k_v"].reshape(-1, K)[rows].half(), batch["teacher_top_k_i"].reshape(-1, K)[rows]
    tail = ops.tail_from_logprobs(tv)
    fn = sda.DistillationLoss(1.0, 0.5, divergence="reverse_kl_tail")
    again = fn.forward_rows(seen[0]["s"], row_labels, teacher_top_k_v=tv, teacher_top_k_i=ti, teacher_top_k_tail=tail)
    assert float(again[0]) == loss and 0 < loss < float("inf") and float(grad.float().abs().max()) > 0
    # the implied tail is the true one to the fp16 precision of the stored log-probs
    with torch.no_grad():
        t = teacher(input_ids=batch["teacher_input_ids"], attention_mask=batch["teacher_attention_mask"], logit_rows=rows).logits
    assert float((ops.topk_tail(t, ti, 1.0, V) - tail).abs().max()) <= 1e-3


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
    assert rows.numel() == sum(n - p for n, p in zip(LENS, PROMPTS))
    packed = {k: batch[k] for k in tr.PACKED_KEYS}
    with torch.no_grad():
        t = teacher(input_ids=batch["teacher_input_ids"], logit_rows=rows, **packed).logits
        tv, ti = ops.logsoftmax_topk(t, K, V)
        tail = ops.topk_tail(t, ti, TEMP, V)
    _by_hand(sda, "reverse_kl_tail", seen[0], loss, grad, rows, row_labels, tv, ti, tail, dict(input_ids=batch["input_ids"], **packed))
    record("gjsd_tail_trainer_packed", loss=loss, padded=padded_loss, logged=tr.logged[-1])
    # the same samples, padded: the bounds test_gpu_distill_packed.py applies to the forward KL
    assert abs(loss - padded_loss) <= 2e-2 * abs(padded_loss), (loss, padded_loss)
    with pytest.raises(ValueError, match="lmbda > 0 with a packed batch"):
        tr.lmbda = 0.5
        tr.training_step(student, dict(batch))


def test_on_policy_training_step_with_a_topk_teacher(sda):
    """lmbda = 1 with reverse_kl_tail and top_k > 0 -- what reverse_kl refuses: the step finishes with a finite loss and a
    non-zero gradient, and the teacher's tail of the student's own tokens reached the loss."""
    from speech_distill_amd.trainer import DistillationTrainer
    with pytest.raises(ValueError, match="top_k=0"):
        _trainer(sda, divergence="reverse_kl", lmbda=1.0, on_policy_generate={"max_new_tokens": 8})
    tr, student, _ = _trainer(sda, lmbda=1.0, on_policy_generate={"max_new_tokens": 8, "top_k": 1, "temperature": 1.0})
    seen = _spy(tr)
    batch = _on_dev(_collator()(_feats()))
    loss, grad = _step(tr, student, batch)
    assert loss == loss and 0 < loss < float("inf") and float(grad.float().abs().max()) > 0
    assert bool(torch.isfinite(grad.float()).all())
    assert tr.logged[-1]["on_policy_fraction"] == 1.0 and tr.logged[-1]["distill_loss"] > 0
    assert seen[0]["v"].shape[1] == K and seen[0]["t"] is None and seen[0]["tail"].shape == (seen[0]["v"].shape[0],)
    assert 0.0 < float(seen[0]["tail"].min()) and float(seen[0]["tail"].max()) < 1.0
    # pre-extracted batches cannot be rolled out: there is no teacher distribution for the student's own tokens
    with pytest.raises(ValueError, match="teacher model"):
        tr.training_step(student, dict(batch, teacher_top_k_v=torch.zeros(4, max(LENS), K, device=dev()),
                                       teacher_top_k_i=torch.zeros(4, max(LENS), K, dtype=torch.int32, device=dev()),
                                       teacher_top_k_tail=torch.full((4, max(LENS)), 0.5, device=dev())))
    assert isinstance(tr, DistillationTrainer)


def test_the_default_trainer_is_untouched(sda):
    """The forward-KL trainer's loss and gradient on one batch, before and after a tail step in the same process."""
    batch = _on_dev(_collator()(_feats()))

    def default():
        tr, student, _ = _trainer(sda, divergence="forward_kl", beta=0.5)
        return _step(tr, student, batch)
    l0, g0 = default()
    tr, student, _ = _trainer(sda)
    _step(tr, student, batch)
    l1, g1 = default()
    assert l0 == l1 and torch.equal(g0, g1)
