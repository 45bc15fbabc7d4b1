"""CPU: the on-policy batch builder (speech_distill_amd/on_policy.py) on hand-made "generated" tokens -- every output
key compared exactly --, the ValueErrors of the loss and the trainer that need no GPU, and the new command-line flags."""
import importlib.util
import os
import tempfile

import pytest
import torch

from conftest import ROOT
from speech_distill_amd import on_policy as OP

PAD, EOS = 9, 7
I = -100


def _batch(with_teacher=True, with_speech=True):
    """B = 4, T = 8.  Row 0: prompt of 3; row 1: prompt of 5; row 2: no labelled position (left alone); row 3: prompt of 2
    whose old completion was padded."""
    ids = torch.tensor([[11, 12, 13, 21, 22, 23, 24, 25],
                        [31, 32, 33, 34, 35, 41, 42, 43],
                        [51, 52, 53, 54, PAD, PAD, PAD, PAD],
                        [61, 62, 71, 72, PAD, PAD, PAD, PAD]])
    labels = torch.tensor([[I, I, I, 21, 22, 23, 24, 25],
                           [I, I, I, I, I, 41, 42, 43],
                           [I, I, I, I, I, I, I, I],
                           [I, I, 71, 72, I, I, I, I]])
    am = torch.tensor([[1] * 8, [1] * 8, [1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0]])
    b = {"input_ids": ids, "labels": labels, "attention_mask": am}
    if with_teacher:   # position-aligned prefixes: other prompt tokens, the same completion
        tids = ids.clone()
        tids[:, :2] += 100
        b["teacher_input_ids"] = tids
        b["teacher_attention_mask"] = am.clone()
    if with_speech:
        b["speech_token_mask"] = (labels != I).to(torch.int64)
    return b


def test_prompt_lengths_and_generate_keywords():
    b = _batch()
    assert OP.prompt_lengths(b["labels"]).tolist() == [3, 5, 8, 2]
    OP.check_generate_kwargs({"max_new_tokens": 4, "top_k": 1})
    for bad in (None, {}, {"top_k": 1}, {"max_new_tokens": 0}, {"max_new_tokens": 4, "num_beams": 2}):
        with pytest.raises(ValueError):
            OP.check_generate_kwargs(bad)
    assert OP.fill_token(EOS, None) == EOS and OP.fill_token(None, None) == 0 and OP.fill_token(EOS, PAD) == PAD


def test_replace_completion_ragged_prompts_eos_in_the_middle_and_cut_at_T():
    b = _batch()
    before = {k: v.clone() for k, v in b.items()}
    # M = 6 new tokens per row (T - the shortest prompt); generate pads with PAD after a row's EOS
    new = torch.tensor([[81, 82, EOS, PAD, PAD, PAD],      # row 0: EOS in the middle
                        [91, 92, 93, 94, 95, 96],          # row 1: no EOS, cut at T (3 slots)
                        [1, 2, 3, 4, 5, 6],                # row 2: dropped
                        [77, 78, 79, 80, 83, 84]])         # row 3: fills its 6 slots
    out = OP.replace_completion(b, new, OP.prompt_lengths(b["labels"]), eos_token_id=EOS, pad_token_id=PAD)
    assert all(torch.equal(b[k], before[k]) for k in b), "the input batch must not be modified"
    assert set(out) == set(b) and all(out[k].dtype == b[k].dtype and out[k].shape == b[k].shape for k in b)
    assert out["input_ids"].tolist() == [[11, 12, 13, 81, 82, EOS, PAD, PAD],
                                         [31, 32, 33, 34, 35, 91, 92, 93],
                                         [51, 52, 53, 54, PAD, PAD, PAD, PAD],
                                         [61, 62, 77, 78, 79, 80, 83, 84]]
    assert out["teacher_input_ids"].tolist() == [[111, 112, 13, 81, 82, EOS, PAD, PAD],
                                                 [131, 132, 33, 34, 35, 91, 92, 93],
                                                 [151, 152, 53, 54, PAD, PAD, PAD, PAD],
                                                 [161, 162, 77, 78, 79, 80, 83, 84]]
    mask = [[1, 1, 1, 1, 1, 1, 0, 0], [1] * 8, [1, 1, 1, 1, 0, 0, 0, 0], [1] * 8]
    assert out["attention_mask"].tolist() == mask and out["teacher_attention_mask"].tolist() == mask
    assert out["labels"].tolist() == [[I, I, I, 81, 82, EOS, I, I],
                                      [I, I, I, I, I, 91, 92, 93],
                                      [I] * 8,
                                      [I, I, 77, 78, 79, 80, 83, 84]]
    assert out["speech_token_mask"].tolist() == [[0, 0, 0, 1, 1, 1, 0, 0], [0, 0, 0, 0, 0, 1, 1, 1], [0] * 8,
                                                 [0, 0, 1, 1, 1, 1, 1, 1]]


def test_replace_completion_eos_equal_to_pad_and_optional_keys():
    """EOS == pad (the project's <|semantic_token_end|>): the EOS is attended to, and its label is -100 by the collator's
    own rule.  A batch without teacher ids / speech mask gets none."""
    b = _batch(with_teacher=False, with_speech=False)
    new = torch.tensor([[81, PAD, PAD, PAD, PAD, PAD], [PAD, PAD, PAD, PAD, PAD, PAD], [0] * 6, [77, 78, 79, 80, 83, PAD]])
    out = OP.replace_completion(b, new, OP.prompt_lengths(b["labels"]), eos_token_id=PAD, pad_token_id=PAD)
    assert set(out) == {"input_ids", "labels", "attention_mask"}
    assert out["input_ids"].tolist() == [[11, 12, 13, 81, PAD, PAD, PAD, PAD], [31, 32, 33, 34, 35, PAD, PAD, PAD],
                                         [51, 52, 53, 54, PAD, PAD, PAD, PAD], [61, 62, 77, 78, 79, 80, 83, PAD]]
    assert out["attention_mask"].tolist() == [[1, 1, 1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0], [1] * 8]
    assert out["labels"].tolist() == [[I, I, I, 81, I, I, I, I], [I] * 8, [I] * 8, [I, I, 77, 78, 79, 80, 83, I]]
    # no EOS given: every generated token counts, nothing is -100 but the pad token itself
    out = OP.replace_completion(b, new, OP.prompt_lengths(b["labels"]))
    assert out["attention_mask"].tolist() == [[1] * 8, [1] * 8, [1, 1, 1, 1, 0, 0, 0, 0], [1] * 8]
    assert out["labels"].tolist()[0] == [I, I, I, 81, PAD, PAD, PAD, PAD]


def test_rollout_calls_generate_once_with_the_prompt_mask_and_a_capped_length():
    b = _batch()
    calls = []

    def generate(input_ids, attention_mask=None, seed=None, **kw):
        calls.append(dict(kw, seed=seed, mask=attention_mask.clone(), ids=input_ids.clone(), grad=torch.is_grad_enabled()))
        new = torch.arange(4 * kw["max_new_tokens"]).reshape(4, -1) + 200
        return torch.cat([input_ids, new], 1)
    out = OP.rollout(generate, b, {"max_new_tokens": 50, "top_k": 1, "eos_token_id": EOS, "pad_token_id": PAD}, seed=123)
    assert len(calls) == 1
    c = calls[0]
    assert c["max_new_tokens"] == 6 and c["seed"] == 123 and c["top_k"] == 1 and c["grad"] is False
    assert torch.equal(c["ids"], b["input_ids"])
    assert c["mask"].tolist() == [[1, 1, 1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0],
                                  [1, 1, 0, 0, 0, 0, 0, 0]]
    assert out["input_ids"][0].tolist() == [11, 12, 13, 200, 201, 202, 203, 204]
    assert out["input_ids"][1].tolist() == [31, 32, 33, 34, 35, 206, 207, 208]
    assert torch.equal(out["input_ids"][2], b["input_ids"][2]) and torch.equal(out["labels"][2], b["labels"][2])
    # a smaller request is kept; a batch with no labelled position is returned as it is, without a call
    OP.rollout(generate, b, {"max_new_tokens": 2}, seed=1)
    assert calls[-1]["max_new_tokens"] == 2
    none = dict(b, labels=torch.full_like(b["labels"], I))
    assert OP.rollout(generate, none, {"max_new_tokens": 2}, seed=1) is none and len(calls) == 2
    with pytest.raises(ValueError, match="teacher model"):
        OP.rollout(generate, dict(b, teacher_top_k_v=torch.zeros(4, 8, 2)), {"max_new_tokens": 2}, seed=1)
    with pytest.raises(ValueError, match="position-aligned"):
        OP.rollout(generate, dict(b, teacher_input_ids=torch.zeros(4, 9, dtype=torch.int64)), {"max_new_tokens": 2}, seed=1)


# ------------------------------------------------------------------------------------------------- errors, no GPU
def test_loss_refuses_before_any_launch():
    import speech_distill_amd as sda
    with pytest.raises(ValueError, match="unknown divergence"):
        sda.DistillationLoss(divergence="tv")
    for beta in (0.0, 1.0, float("nan"), -0.1):
        with pytest.raises(ValueError, match="0 < beta < 1"):
            sda.DistillationLoss(divergence="jsd", beta=beta)
    sda.DistillationLoss(divergence="reverse_kl", beta=0.0)   # beta belongs to jsd only
    fn = sda.DistillationLoss(divergence="reverse_kl")
    s, lab = torch.randn(1, 4, 64), torch.tensor([[1, 2, 3, 4]])
    topk = dict(teacher_top_k_v=torch.zeros(1, 4, 2), teacher_top_k_i=torch.zeros(1, 4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="dense teacher"):     # before the CPU tensors could be refused
        fn(s, lab, **topk)
    with pytest.raises(ValueError, match="dense teacher"):
        fn.forward_rows(s[0], lab[0], teacher_top_k_v=topk["teacher_top_k_v"][0], teacher_top_k_i=topk["teacher_top_k_i"][0])
    with pytest.raises(ValueError, match="Either teacher_logits or top_k"):
        fn(s, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn.forward_rows(s[0], lab[0], teacher_logits=torch.randn(4, 64))


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


def test_trainer_refuses_what_it_cannot_run():
    with pytest.raises(ValueError, match="top_k=0"):
        _trainer(divergence="jsd", top_k=100)
    with pytest.raises(ValueError, match="unknown divergence"):
        _trainer(divergence="hellinger", top_k=0)
    with pytest.raises(ValueError, match="0 < beta < 1"):
        _trainer(divergence="jsd", beta=1.0, top_k=0)
    for lm in (-0.1, 1.5):
        with pytest.raises(ValueError, match="lmbda"):
            _trainer(lmbda=lm)
    with pytest.raises(ValueError, match="max_new_tokens"):
        _trainer(lmbda=0.5)
    with pytest.raises(ValueError, match="teacher model"):
        _trainer(lmbda=0.5, on_policy_generate={"max_new_tokens": 8}, teacher_model=None)
    with pytest.raises(ValueError, match="on the GPU without LoRA"):   # this student sits on the CPU
        _trainer(lmbda=0.5, on_policy_generate={"max_new_tokens": 8})
    tr = _trainer(divergence="reverse_kl", top_k=0)
    assert tr.distill_loss_fn.divergence == "reverse_kl" and tr.lmbda == 0.0
    tr = _trainer(divergence="jsd", beta=0.3, top_k=100, is_quantized_teacher=True)   # a quantised teacher is dense
    assert tr.distill_loss_fn.beta == 0.3
    batch = {"input_ids": torch.zeros(1, 4, dtype=torch.int64), "labels": torch.zeros(1, 4, dtype=torch.int64),
             "teacher_top_k_v": torch.zeros(1, 4, 2), "teacher_top_k_i": torch.zeros(1, 4, 2, dtype=torch.int64)}
    with pytest.raises(ValueError, match="pre-extracted teacher_top_k_v"):
        tr.compute_loss(tr.model, batch)
    plain = _trainer()
    assert plain.distill_loss_fn.divergence == "forward_kl" and plain.lmbda == 0.0 and plain._on_policy_rng is None


# ------------------------------------------------------------------------------------------------- command line
def _train_script():
    spec = importlib.util.spec_from_file_location("sd_train_script", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_parse_and_the_defaults_construct_todays_trainer():
    tr = _train_script()
    cfg = tr.parse_args([])
    assert (cfg.divergence, cfg.beta, cfg.lmbda) == ("forward_kl", 0.5, 0.0) and cfg.top_k == 128
    assert tr.distill_kwargs(cfg, pad=5) == {}          # no new keyword reaches DistillationTrainer
    cfg = tr.parse_args(["--divergence", "jsd", "--beta", "0.3", "--top_k", "0", "--lmbda", "0.25", "--on_policy_max_new_tokens",
                         "64", "--on_policy_temperature", "0.8", "--on_policy_top_k", "20", "--on_policy_decode_kernels", "skinny"])
    assert tr.distill_kwargs(cfg, pad=5) == dict(
        divergence="jsd", beta=0.3, lmbda=0.25,
        on_policy_generate=dict(max_new_tokens=64, temperature=0.8, top_k=20, decode_kernels="skinny", eos_token_id=5,
                                pad_token_id=5))
    OP.check_generate_kwargs(tr.distill_kwargs(cfg, pad=5)["on_policy_generate"])
    with pytest.raises(SystemExit, match="--top_k 0"):
        tr.distill_kwargs(tr.parse_args(["--divergence", "reverse_kl"]))
    assert tr.distill_kwargs(tr.parse_args(["--divergence", "reverse_kl", "--load_teacher_in_8bit"])) == \
        dict(divergence="reverse_kl", beta=0.5)
    with pytest.raises(SystemExit):
        tr.parse_args(["--divergence", "tv"])
