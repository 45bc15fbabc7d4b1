"""-m gpu: the reference's Stage-2 loop settings through the real HF Trainer on the HIP path -- epoch checkpoints,
epoch evaluation (``prediction_step`` -> ``compute_loss(..., return_outputs=True)``, train.py:116),
``load_best_model_at_end`` (train.py:331-354) -- and BASELINE config 4 (T=2048, batch 4) through
``DistillationTrainer.compute_loss`` as stated."""
import os
import tempfile

import numpy as np
import pytest
import torch

from gpu_util import dev, record, to_dev
from test_gpu_model import _Tok, _build, _c1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sda():
    import speech_distill_amd as m
    m.load_lib()
    return m


def test_c1_trainer_epoch_checkpoints_eval_and_best_model(sda):
    """BASELINE config 1 with the reference's TrainingArguments (train.py:331-354): eval_strategy="epoch",
    save_strategy="epoch", load_best_model_at_end=True, save_total_limit=3, gradient_checkpointing=True, bf16.
    VERDICT r1: Trainer.save_model raised on the HIP student; evaluation on the GPU was untested."""
    from safetensors.torch import load_file
    from transformers import Qwen3ForCausalLM, TrainingArguments
    from oracle import qwen3 as Q
    from oracle import step as S
    from speech_distill_amd.collator import ProcessedDataCollator
    from speech_distill_amd.trainer import DistillationTrainer
    z, st, te, sw, tw, feats, pad, bos = _c1(sda)
    student, teacher = _build(sda, st, sw), _build(sda, te, tw)
    teacher.eval().requires_grad_(False)
    out = tempfile.mkdtemp()
    args = TrainingArguments(
        output_dir=out, per_device_train_batch_size=4, per_device_eval_batch_size=4, gradient_accumulation_steps=2,
        num_train_epochs=4, learning_rate=1e-3, logging_steps=1, eval_strategy="epoch", save_strategy="epoch",
        load_best_model_at_end=True, save_total_limit=3, gradient_checkpointing=True, report_to=[],
        remove_unused_columns=False, label_names=["labels"], seed=42, data_seed=42, lr_scheduler_type="constant",
        warmup_steps=0, weight_decay=0.0, max_grad_norm=1.0, dataloader_num_workers=0, bf16=True)

    class DS(torch.utils.data.Dataset):
        def __init__(self, rows):
            self.rows = rows

        def __len__(self):
            return len(self.rows)

        def __getitem__(self, i):
            return dict(self.rows[i])
    coll = ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad)
    eval_rows = feats[:4]
    tr = DistillationTrainer(model=student, args=args, train_dataset=DS(feats), eval_dataset=DS(eval_rows),
                             data_collator=coll, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=16)
    tr._get_train_sampler = lambda *a, **k: torch.utils.data.SequentialSampler(tr.train_dataset)
    tr.train()

    # training itself is unchanged by checkpointing / evaluation: the reference's loss trajectory (3 epochs pinned)
    hist = [h["loss"] for h in tr.state.log_history if "loss" in h]
    np.testing.assert_allclose(hist[:3], z["train_loss_per_step"], rtol=2e-2)
    # one evaluation per epoch through prediction_step -> compute_loss(return_outputs=True)
    evals = [h["eval_loss"] for h in tr.state.log_history if "eval_loss" in h]
    assert len(evals) == 4 and all(np.isfinite(evals)) and evals[-1] < evals[0]
    # save_total_limit=3 of 4 epoch checkpoints, each an HF directory
    ckpts = sorted(d for d in os.listdir(out) if d.startswith("checkpoint-"))
    assert len(ckpts) == 3, ckpts
    for c in ckpts:
        assert {"config.json", "model.safetensors", "optimizer.pt", "trainer_state.json"} <= set(os.listdir(os.path.join(out, c)))
    # load_best_model_at_end: the student now holds the best checkpoint's weights (lowest eval_loss), bit for bit
    best = tr.state.best_model_checkpoint
    assert best is not None and os.path.basename(best) in ckpts
    sd = load_file(os.path.join(best, "model.safetensors"))
    assert "lm_head.weight" not in sd
    for k, v in student.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    hf = Qwen3ForCausalLM.from_pretrained(best, dtype=torch.bfloat16)  # what a user of the reference would do next
    assert torch.equal(hf.lm_head.weight, sd["model.embed_tokens.weight"])
    # the evaluation loss of the loaded model == the oracle's loss on the same batch with the same weights
    ev = tr.evaluate()
    batch = coll([dict(f) for f in eval_rows])
    ref = S.distill_step({k: v.float() for k, v in hf.state_dict().items() if k != "lm_head.weight"}, Q.Qwen3Shape(*st),
                         {k: v.bfloat16().float() for k, v in tw.items()}, Q.Qwen3Shape(*te), batch, 2.0, 0.5, top_k=16,
                         with_grad=False, acc=torch.float32)
    record("c1_eval_vs_oracle", eval_loss=ev["eval_loss"], oracle=float(ref["total"]), evals=evals)
    assert abs(ev["eval_loss"] - float(ref["total"])) <= 2e-2 * abs(float(ref["total"]))
    assert abs(ev["eval_loss"] - min(evals)) <= 1e-6 + 1e-3 * abs(min(evals))


def test_model_moves_as_one_flat_buffer_and_rejects_left_padding(sda):
    """HF Trainer calls model.to(args.device): the HF-named parameters must stay views of the flat buffer; a left-padded
    attention mask must raise instead of silently attending over the wrong keys."""
    cpu = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device="cpu", seed=3)
    ref = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device=dev(), seed=3)
    m = cpu.to(dev())
    assert m is cpu and m.flat.is_cuda and m._params["model.norm.weight"].is_cuda
    assert m._params["model.embed_tokens.weight"].data_ptr() == m.flat.data_ptr()
    ids = torch.randint(0, 640, (2, 40), device=dev())
    am = torch.ones_like(ids)
    am[1, 30:] = 0
    a = m(input_ids=ids, attention_mask=am).logits
    b = ref(input_ids=ids, attention_mask=am).logits
    assert torch.equal(a, b)
    a.float().sum().backward()
    assert m.flat_grad is not None and m.flat_grad.is_cuda and bool(torch.isfinite(m.flat_grad.float()).all())
    left = torch.ones_like(ids)
    left[1, :10] = 0
    with pytest.raises(ValueError, match="right-padded"):
        m(input_ids=ids, attention_mask=left)
    from speech_distill_amd import ops
    with pytest.raises(ValueError, match="right-padded"):
        ops.loss_rows(ids.clone(), None, right_padded=(left,))
    rows, lab = ops.loss_rows(ids.clone(), None, right_padded=(am, None))
    assert rows.numel() == 2 * 39


def test_config4_as_stated_through_the_trainer(sda):
    """BASELINE config 4 on one GPU as stated: T=2048, batch 4, gradient checkpointing "on" (train.py:512-517),
    Qwen3-0.6B-shape student + SoulX-1.7B-shape teacher, through DistillationTrainer.compute_loss: student forward,
    teacher forward, on-the-fly top-128, loss, backward.  No CPU oracle finishes at this size; size-independent
    properties: CE ~ ln V at random init, the teacher monitor loss is finite, every gradient finite, bitwise
    determinism of two identical steps, the compact-head path == the full [B,T,V] path on the loss, and the peak
    HBM footprint is recorded (DESIGN.md states it)."""
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims.student_06b(), device=dev(), seed=0)
    teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims.teacher_17b(), device=dev(), seed=1)
    teacher.eval().requires_grad_(False)
    student.gradient_checkpointing_enable()
    args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False,
                             label_names=["labels"], save_strategy="no", bf16=True, logging_steps=1)
    tr = DistillationTrainer(model=student, args=args, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=128)
    logged = []
    tr.log = lambda d, *a, **k: logged.append(dict(d))
    g = torch.Generator().manual_seed(4)
    B, T, V = 4, 2048, 159488
    ids = torch.randint(0, V, (B, T), generator=g)
    ids[:, T // 4:] = torch.randint(152927, V, (B, T - T // 4), generator=g)
    am = torch.ones(B, T, dtype=torch.long)
    am[3, T - 200:] = 0  # one right-padded row
    labels = ids.clone()
    labels[:, :T // 4 + 1] = -100
    labels[am == 0] = -100
    batch = {k: to_dev(v) for k, v in dict(input_ids=ids, attention_mask=am, labels=labels, teacher_input_ids=ids,
                                           teacher_attention_mask=am).items()}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = []
    for rep in range(2):
        student.zero_grad()
        loss = tr.compute_loss(student, dict(batch))
        loss.backward()
        torch.cuda.synchronize()
        res.append((float(loss), dict(logged[-1]), student.flat_grad.clone()))
    peak = torch.cuda.max_memory_allocated()
    n_rows = int((labels[:, 1:] != -100).sum())
    record("config4_trainer_step", loss=res[0][0], logged=res[0][1], lnV=float(np.log(V)), rows=n_rows,
           peak_gib=peak / 2**30, resident_before_gib=base / 2**30)
    assert abs(res[0][1]["student_loss"] - np.log(V)) < 0.5
    assert np.isfinite(res[0][1]["teacher_loss"]) and np.isfinite(res[0][1]["distill_loss"]) and res[0][1]["distill_loss"] > 0
    assert bool(torch.isfinite(res[0][2].float()).all()) and float(res[0][2].float().abs().max()) > 0
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2]), "C4 step is not deterministic"
    # full-head path (what evaluation uses) gives the same loss on the same batch
    tr.compact_head = False
    student.zero_grad()
    full = tr.compute_loss(student, dict(batch))
    assert abs(float(full) - res[0][0]) <= 1e-4 * abs(res[0][0]), (float(full), res[0][0])
    assert peak < 200 * 2**30
    # "grad-checkpointing on" taken literally: layer-granular recompute (policy "always") -- the same loss and the
    # same gradient bit for bit, from a smaller activation footprint, for one more student forward
    tr.compact_head = True
    del full
    student.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"recompute": "always"})
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    student.zero_grad()
    loss = tr.compute_loss(student, dict(batch))
    loss.backward()
    torch.cuda.synchronize()
    peak_ck = torch.cuda.max_memory_allocated()
    record("config4_trainer_step_recompute", peak_gib=peak_ck / 2**30, peak_saved_all_gib=peak / 2**30)
    assert float(loss) == res[0][0] and torch.equal(student.flat_grad, res[0][2])
    assert peak_ck < peak - 7 * 2**30  # 28 layers x 0.37 GB of activations -> 28 x 17 MB + two work sets


def test_config4_real_width_long_context_vs_oracle(sda):
    """BASELINE config 4's sequence length against the CPU oracle: real widths (student h=1024/I=3072, teacher
    h=2048/I=6144, 16/8 heads, V=159 488) at depth 2, B=1, T=2048 with a right-padded tail, through
    DistillationTrainer.compute_loss (student + teacher forward, top-128, loss on the loss rows, backward): loss and the
    three logged sub-losses within 2e-2 of the fp32 oracle on bf16-rounded weights, gradient norms within 8e-2."""
    from transformers import TrainingArguments
    from oracle import qwen3 as Q
    from oracle import step as S
    from speech_distill_amd.trainer import DistillationTrainer
    st, te = Q.Qwen3Shape(159488, 1024, 3072, 2, 16, 8), Q.Qwen3Shape(159488, 2048, 6144, 2, 16, 8)
    sw = {k: v.bfloat16().float() for k, v in Q.init_weights(st, seed=21).items()}
    tw = {k: v.bfloat16().float() for k, v in Q.init_weights(te, seed=22).items()}
    student = _build(sda, (159488, 1024, 3072, 2, 16, 8), sw)
    teacher = _build(sda, (159488, 2048, 6144, 2, 16, 8), tw)
    teacher.eval().requires_grad_(False)
    g = torch.Generator().manual_seed(8)
    B, T, V = 1, 2048, 159488
    ids = torch.randint(0, V, (B, T), generator=g)
    ids[:, T // 4:] = torch.randint(152927, V, (B, T - T // 4), generator=g)
    am = torch.ones(B, T, dtype=torch.long)
    am[0, T - 300:] = 0
    labels = ids.clone()
    labels[:, :T // 4 + 1] = -100
    labels[am == 0] = -100
    batch = {"input_ids": ids, "attention_mask": am, "labels": labels, "teacher_input_ids": ids.clone(),
             "teacher_attention_mask": am.clone()}
    ref = S.distill_step(sw, st, tw, te, batch, 2.0, 0.5, top_k=128, acc=torch.float32)
    args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False,
                             label_names=["labels"], save_strategy="no", bf16=True, logging_steps=1)
    tr = DistillationTrainer(model=student, args=args, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=128)
    logged = []
    tr.log = lambda d, *a, **k: logged.append(dict(d))
    loss = tr.compute_loss(student, {k: to_dev(v) for k, v in batch.items()})
    loss.backward()
    got = [float(loss), logged[-1]["student_loss"], logged[-1]["distill_loss"]]
    want = [float(ref["total"]), float(ref["task"]), float(ref["distill"])]
    record("config4_real_width_vs_oracle", got=got, ref=want)
    np.testing.assert_allclose(got, want, rtol=2e-2)
    for k in ("model.layers.1.mlp.down_proj.weight", "model.layers.0.self_attn.q_proj.weight",
              "model.layers.0.self_attn.k_norm.weight", "model.norm.weight"):
        gn, rn = float(student._params[k].grad.double().norm()), float(ref["grads"][k].double().norm())
        record("config4_real_width_gnorm", param=k, got=gn, ref=rn)
        assert abs(gn - rn) <= 8e-2 * rn, (k, gn, rn)


def test_extract_then_train_from_precomputed_topk_on_disk(sda, tmp_path, monkeypatch):
    """The reference's two-script workflow end to end, as a user runs it: scripts/extract_teacher_logits.py writes
    teacher top-K columns next to a pre-processed dataset (extract_teacher_logits.py:120-145), scripts/train.py then
    trains from them (train.py:234-256 load_from_disk, data.py:329-372 collation, train.py:95-103 pre-computed branch of
    compute_loss).  The same run with the teacher's top-K taken on the fly (train.py:60-94) must log the same losses:
    both paths feed the loss the same fp16 top-K values of the same teacher."""
    import importlib.util
    import json
    import sys
    from datasets import Dataset
    from conftest import ROOT

    def load(name):
        spec = importlib.util.spec_from_file_location("sd_" + name, os.path.join(ROOT, "scripts", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    V, bos, pad = 640, 320, 639
    student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 128, 256, 2, 2, 1), device=dev(), seed=0)
    teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 256, 512, 2, 4, 2), device=dev(), seed=1)
    sdir, tdir, ddir, xdir = (str(tmp_path / n) for n in ("student", "teacher", "data", "data_topk"))
    student.save_pretrained(sdir)
    teacher.save_pretrained(tdir)
    del student, teacher
    g = torch.Generator().manual_seed(77)
    rows = []
    for _ in range(12):
        n = int(torch.randint(24, 49, (1,), generator=g))
        nt = n // 4
        ids = torch.cat([torch.randint(0, bos, (nt,), generator=g), torch.tensor([bos]),
                         torch.randint(bos + 1, pad, (n - nt - 2,), generator=g), torch.tensor([pad])]).tolist()
        rows.append({"student_input_ids": ids, "student_attention_mask": [1] * n,
                     "teacher_input_ids": ids, "teacher_attention_mask": [1] * n})
    Dataset.from_list(rows).save_to_disk(ddir)
    monkeypatch.setattr(sys, "argv", ["extract_teacher_logits.py", "--teacher_model_path", tdir, "--dataset_path", ddir,
                                      "--output_path", xdir, "--top_k", "16", "--batch_size", "5", "--pad_token_id", str(pad)])
    load("extract_teacher_logits").main()

    def train(data, tag):
        log = str(tmp_path / (tag + ".json"))
        monkeypatch.setattr(sys, "argv", [
            "train.py", "--teacher_model", tdir, "--student_model", sdir, "--dataset_path", data, "--output_dir",
            str(tmp_path / tag), "--max_length", "64", "--top_k", "16", "--per_device_train_batch_size", "2",
            "--gradient_accumulation_steps", "1", "--num_train_epochs", "1", "--max_steps", "4", "--logging_steps", "1",
            "--save_strategy", "no", "--learning_rate", "1e-3", "--warmup_steps", "0", "--pad_token_id", str(pad),
            "--speech_bos_id", str(bos), "--log_json", log])
        load("train").main()
        hist = json.load(open(log))["log_history"]
        return [e for e in hist if "loss" in e], [e for e in hist if "distill_loss" in e]

    fly, fly_sub = train(ddir, "on_the_fly")
    pre, pre_sub = train(xdir, "precomputed")
    record("extract_then_train", on_the_fly=[e["loss"] for e in fly], precomputed=[e["loss"] for e in pre])
    assert len(fly) == len(pre) == 4 and len(fly_sub) == len(pre_sub) > 0
    for a, b in zip(fly, pre):
        assert abs(a["loss"] - b["loss"]) <= 2e-3 * abs(a["loss"]), (a, b)
    for a, b in zip(fly_sub, pre_sub):  # the sub-losses are logged on their own cadence (quirk Q3, train.py:105-114)
        assert abs(a["distill_loss"] - b["distill_loss"]) <= 2e-3 * abs(a["distill_loss"]), (a, b)
        assert abs(a["student_loss"] - b["student_loss"]) <= 2e-3 * abs(a["student_loss"]), (a, b)
        assert abs(a["teacher_loss"] - b["teacher_loss"]) <= 2e-3 * max(1.0, abs(a["teacher_loss"])), (a, b)


def test_hf_default_optimizer_still_works_and_agrees_with_the_fused_one(sda):
    """DistillationTrainer builds FlatAdamW and folds HF's clipping into it by default; with ``fused_optimizer = False`` it
    keeps HF's own AdamW (torch, ~310 parameter views) and clips the flat gradient buffer in place.  Same data, same
    init: the logged gradient norms agree (same reduction) and the loss trajectories stay together."""
    from transformers import TrainingArguments
    from speech_distill_amd.collator import ProcessedDataCollator
    from speech_distill_amd.optim import FlatAdamW
    from speech_distill_amd.trainer import DistillationTrainer
    z, st, te, sw, tw, feats, pad, bos = _c1(sda)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(feats)

        def __getitem__(self, i):
            return dict(feats[i])

    def run(fused):
        student, teacher = _build(sda, st, sw), _build(sda, te, tw)
        teacher.eval().requires_grad_(False)
        args = TrainingArguments(
            output_dir=tempfile.mkdtemp(), per_device_train_batch_size=4, gradient_accumulation_steps=2, max_steps=3,
            learning_rate=1e-3, logging_steps=1, save_strategy="no", report_to=[], remove_unused_columns=False,
            label_names=["labels"], seed=42, data_seed=42, lr_scheduler_type="constant", warmup_steps=0, weight_decay=0.0,
            max_grad_norm=0.5, dataloader_num_workers=0, bf16=True)
        tr = DistillationTrainer(model=student, args=args, train_dataset=DS(), teacher_model=teacher, temperature=2.0,
                                 alpha=0.5, top_k=16, data_collator=ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad))
        tr.fused_optimizer = fused
        tr._get_train_sampler = lambda *a, **k: torch.utils.data.SequentialSampler(tr.train_dataset)
        tr.train()
        opt = getattr(tr.optimizer, "optimizer", tr.optimizer)
        logs = [h for h in tr.state.log_history if "loss" in h]
        return opt, [h["loss"] for h in logs], [h["grad_norm"] for h in logs]

    opt_f, loss_f, gn_f = run(True)
    opt_h, loss_h, gn_h = run(False)
    assert isinstance(opt_f, FlatAdamW) and not isinstance(opt_h, FlatAdamW) and isinstance(opt_h, torch.optim.AdamW)
    record("fused_vs_hf_optimizer", loss_fused=loss_f, loss_hf=loss_h, gn_fused=gn_f, gn_hf=gn_h)
    assert len(loss_f) == len(loss_h) == 3
    assert abs(gn_f[0] - gn_h[0]) <= 1e-3 * gn_h[0]           # step 1: identical gradients, two routes to the same norm
    np.testing.assert_allclose(loss_f, loss_h, rtol=2e-2)     # bf16 moments either way; the updates differ by rounding
    np.testing.assert_allclose(gn_f, gn_h, rtol=5e-2)


def test_teacher_batch_of_another_length_is_refused_on_the_gpu_path(sda):
    """the collator pads teacher and student separately, so T_teacher can differ from T; the fused
    row-selection kernel indexes every mask as [B, T] with the LABELS' T.  The trainer must refuse such a batch (the
    reference dies in its loss with an IndexError, distillation_loss.py:31-45) before any kernel reads the short mask;
    and HF's real training log carries tokens_per_second."""
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    z, st, te, sw, tw, feats, pad, bos = _c1(sda)
    student, teacher = _build(sda, st, sw), _build(sda, te, tw)
    teacher.eval().requires_grad_(False)
    args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False, label_names=["labels"],
                             save_strategy="no", logging_steps=1, bf16=True)
    tr = DistillationTrainer(model=student, args=args, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=16)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 640, (2, 40), generator=g)
    labels = ids.clone()
    labels[:, :9] = -100
    for dt in (-7, +5):
        tids = torch.randint(0, 640, (2, 40 + dt), generator=g)
        batch = {"input_ids": to_dev(ids), "attention_mask": to_dev(torch.ones_like(ids)), "labels": to_dev(labels),
                 "teacher_input_ids": to_dev(tids), "teacher_attention_mask": to_dev(torch.ones_like(tids))}
        with pytest.raises(ValueError, match="position-aligned"):
            tr.compute_loss(student, batch)
    # int32 labels (an arrow column read without a cast): same loss as int64 labels
    base = {"input_ids": to_dev(ids), "attention_mask": to_dev(torch.ones_like(ids)),
            "teacher_input_ids": to_dev(ids), "teacher_attention_mask": to_dev(torch.ones_like(ids))}
    a = tr.compute_loss(student, dict(base, labels=to_dev(labels)))
    b = tr.compute_loss(student, dict(base, labels=to_dev(labels.to(torch.int32))))
    assert float(a) == float(b) and float(a) > 0


def test_zero_row_batch_planned_ahead_takes_the_full_path(sda, monkeypatch):
    """``compute_loss``'s own zero-row fall-back with a HIP student on the GPU: a padded batch without a loss row gives the
    reference's zeros (distillation_loss.py:47-53) when it is planned in place, and the same when its plan was made ahead --
    the stored plan is taken (no second selection) although no row of it is used, and it keeps its event, which the
    teacher's stream then waits for."""
    from transformers import TrainingArguments
    from speech_distill_amd import ops
    from speech_distill_amd.trainer import DistillationTrainer, _Ahead
    z, st, te, sw, tw, feats, pad, bos = _c1(sda)
    student, teacher = _build(sda, st, sw), _build(sda, te, tw)
    teacher.eval().requires_grad_(False)
    args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False, label_names=["labels"],
                             save_strategy="no", logging_steps=1, bf16=True)
    tr = DistillationTrainer(model=student, args=args, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=16)
    logged, reads = [], []
    tr.log = lambda d, *a, **k: logged.append(dict(d))
    monkeypatch.setattr(ops, "loss_rows", lambda *a, _f=ops.loss_rows, **k: reads.append(1) or _f(*a, **k))
    ids = torch.randint(0, 640, (2, 40), generator=torch.Generator().manual_seed(0))
    batch = {"input_ids": to_dev(ids), "attention_mask": to_dev(torch.ones_like(ids)), "labels": to_dev(torch.full_like(ids, -100)),
             "teacher_input_ids": to_dev(ids), "teacher_attention_mask": to_dev(torch.ones_like(ids))}
    zeros = {"student_loss": 0.0, "teacher_loss": 0.0, "distill_loss": 0.0}
    in_place = tr.compute_loss(student, dict(batch))
    n_in_place = len(reads)
    assert float(in_place) == 0.0 and logged[-1] == zeros and n_in_place >= 1
    ready = torch.cuda.Event()
    ready.record()
    plan = tr._plan_step(student, batch, batch["labels"], None, batch["teacher_attention_mask"], True, event=ready)
    assert plan.rows.numel() == 0 and plan.event is ready and plan.student_kw == plan.teacher_kw == {"padding_checked": True}
    tr._ahead[id(batch["labels"])] = _Ahead(plan)
    del reads[:]
    ahead = tr.compute_loss(student, dict(batch))
    assert float(ahead) == 0.0 and logged[-1] == zeros and not tr._ahead
    assert len(reads) == n_in_place - 1      # the selection was not made again


def test_window_lookahead_serves_the_same_batches_in_the_same_order(sda, monkeypatch):
    """DistillationTrainer.get_batch_samples fetches one accumulation window ahead and training_step enqueues the next
    micro-batch's teacher pass early (both only re-order host work).  Over two epochs whose last window is a remainder
    (13 samples, batch 2, accumulation 2: 7 micro-batches = 4 optimizer steps per epoch, the last with one micro-batch
    of one sample), the loop must see the same micro-batches in the same order, log the same losses and end at the
    same parameters as with the plain HF order (SD_ROWS_AHEAD=0)."""
    import tempfile
    from transformers import TrainingArguments
    from speech_distill_amd import ops
    from speech_distill_amd.collator import ProcessedDataCollator
    from speech_distill_amd.trainer import DistillationTrainer
    z, st, te, sw, tw, feats, pad, bos = _c1(sda)
    rows = (feats * 2)[:13]

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(rows)

        def __getitem__(self, i):
            return dict(rows[i])

    def run(ahead):
        monkeypatch.setenv("SD_ROWS_AHEAD", "1" if ahead else "0")
        student, teacher = _build(sda, st, sw), _build(sda, te, tw)
        teacher.eval().requires_grad_(False)
        args = TrainingArguments(
            output_dir=tempfile.mkdtemp(), per_device_train_batch_size=2, gradient_accumulation_steps=2, num_train_epochs=2,
            learning_rate=1e-3, logging_steps=1, save_strategy="no", eval_strategy="no", report_to=[],
            remove_unused_columns=False, label_names=["labels"], seed=7, data_seed=7, lr_scheduler_type="constant",
            warmup_steps=0, max_grad_norm=1.0, dataloader_num_workers=0, bf16=True)
        tr = DistillationTrainer(model=student, args=args, train_dataset=DS(), teacher_model=teacher, temperature=2.0,
                                 alpha=0.5, top_k=16, data_collator=ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad))
        seen, early, reads = [], [], []
        inner = tr.compute_loss

        def spy(model, inputs, *a, **k):
            seen.append(inputs["input_ids"].cpu().clone())
            early.append(getattr(tr._ahead.get(id(inputs["labels"])), "teacher", None) is not None)
            return inner(model, inputs, *a, **k)
        tr.compute_loss = spy
        with monkeypatch.context() as mp:
            for name in ("loss_rows", "packed_rows"):   # the selections, each with the micro-batch's one host read
                mp.setattr(ops, name, lambda *a, _f=getattr(ops, name), **k: reads.append(1) or _f(*a, **k))
            tr.train()
        return seen, early, [h["loss"] for h in tr.state.log_history if "loss" in h], student.flat.clone(), len(reads)
    seen_a, early_a, loss_a, flat_a, reads_a = run(True)
    seen_b, early_b, loss_b, flat_b, reads_b = run(False)
    assert len(seen_a) == len(seen_b) == 14 and len(loss_a) == 8
    assert reads_a == reads_b == 14      # one selection per micro-batch, made ahead or in compute_loss, never both
    for a, b in zip(seen_a, seen_b):
        assert a.shape == b.shape and torch.equal(a, b)
    assert loss_a == loss_b and torch.equal(flat_a, flat_b)
    # with the lookahead every micro-batch but the first of an epoch found its teacher pass already enqueued
    assert not any(early_b) and early_a == [False] + [True] * 6 + [False] + [True] * 6, early_a
