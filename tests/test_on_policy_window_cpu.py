"""CPU: the window rollout's bookkeeping (speech_distill_amd/on_policy.py rollout_window) against the micro-batch path
(on_policy.rollout) with a stand-in engine and a stand-in ``generate`` built from ONE token function, the draw stream, and
the new keywords of DistillationTrainer and scripts/train.py.  No GPU: every comparison is torch.equal on CPU tensors."""
import importlib.util
import os
import tempfile
import types

import pytest
import torch

from conftest import ROOT
from speech_distill_amd import on_policy as OP

PAD = 7            # the EOS id too, as scripts/train.py passes it
I = -100
KW = {"max_new_tokens": 4, "temperature": 1.0, "top_k": 50, "eos_token_id": PAD, "pad_token_id": PAD,
      "decode_kernels": "wide"}


def f(prompt, request_seed, step):
    """The one token function of both stand-ins: in 1..11, so PAD (= EOS) comes up now and then."""
    return (sum(prompt) + 3 * request_seed + 5 * step) % 11 + 1


def _tokens(prompt, rseed, budget):
    """What a request yields: f step by step, through the first EOS."""
    out = []
    for s in range(budget):
        out.append(f(prompt, rseed, s))
        if out[-1] == PAD:
            break
    return out


class Engine:
    """The stand-in engine: submit / run / result / forget, every call recorded."""

    def __init__(self):
        self.submitted, self.results, self.forgotten, self.runs = [], {}, [], 0

    def submit(self, input_ids, max_new_tokens=20, seed=None, **kw):
        assert input_ids.dim() == 1 and not torch.is_grad_enabled()
        self.submitted.append(dict(kw, prompt=input_ids.tolist(), max_new_tokens=max_new_tokens, seed=seed))
        return len(self.submitted) - 1

    def run(self):
        self.runs += 1
        for rid, s in enumerate(self.submitted):
            self.results.setdefault(rid, torch.tensor(_tokens(s["prompt"], s["seed"], s["max_new_tokens"]), dtype=torch.int64))

    def result(self, rid):
        return self.results[rid]

    def forget(self, rids):
        self.forgotten += list(rids)


def generate(input_ids, attention_mask=None, seed=None, max_new_tokens=20, eos_token_id=None, pad_token_id=None, **kw):
    """The stand-in ``generate``: row b continues its prompt with f under ``request_seed(seed, b)``, its budget cut at its
    own width (max_new_tokens per row), ``pad_token_id`` behind its end.  -> [B, T + max_new_tokens]."""
    B, T = input_ids.shape
    new = torch.full((B, max_new_tokens), pad_token_id, dtype=torch.int64)
    for b in range(B):
        p = int(attention_mask[b].sum())
        tok = _tokens(input_ids[b, :p].tolist(), OP.request_seed(seed, b), min(max_new_tokens, T - p))
        new[b, :len(tok)] = torch.tensor(tok, dtype=torch.int64)
    return torch.cat([input_ids, new], 1)


def _batch(prompts, T=10, base=20, teacher=True, speech=True):
    """Rows with the given prompt lengths (T: a row with no labelled position), a dataset completion behind each prompt
    and padding behind that."""
    B = len(prompts)
    g = torch.Generator().manual_seed(base)
    ids = torch.randint(12, 40, (B, T), generator=g)
    labels = ids.clone()
    am = torch.ones(B, T, dtype=torch.int64)
    for b, p in enumerate(prompts):
        labels[b, :p] = I
        end = min(T, p + 3)          # the dataset's completion: three tokens, padding behind
        ids[b, end:], labels[b, end:], am[b, end:] = PAD, I, 0
    out = {"input_ids": ids, "labels": labels, "attention_mask": am}
    if teacher:
        tids = ids.clone()
        tids[:, 0] += 100
        out["teacher_input_ids"], out["teacher_attention_mask"] = tids, am.clone()
    if speech:
        out["speech_token_mask"] = (labels != I).to(torch.int64)
    return out


def _window():
    """Three micro-batches: ragged prompts with an unlabelled row (row 2) and a row whose width leaves it 2 of the 4
    tokens (row 3); an off-policy batch; a batch without the optional keys whose last row has 1 slot."""
    return [_batch([3, 5, 10, 8], base=20), _batch([4, 4], base=21), _batch([2, 6, 9], base=22, teacher=False, speech=False)]


SEEDS = [1234567, None, 2 ** 31 - 3]


def test_window_bookkeeping_equals_the_micro_batch_path():
    window = _window()
    before = [{k: v.clone() for k, v in b.items()} for b in window]
    eng = Engine()
    out = OP.rollout_window(eng, window, KW, SEEDS)
    assert len(out) == 3 and out[1] is window[1]                    # the off-policy batch: the same object
    assert all(torch.equal(b[k], a[k]) for b, a in zip(window, before) for k in a), "the inputs must not be modified"
    assert eng.runs == 1 and sorted(eng.forgotten) == list(range(len(eng.submitted)))
    ends = []
    for i in (0, 2):
        want = OP.rollout(generate, window[i], KW, SEEDS[i])
        assert set(out[i]) == set(window[i]) == set(want)
        for k in want:
            assert out[i][k].dtype == want[k].dtype and torch.equal(out[i][k], want[k]), (i, k, out[i][k], want[k])
        assert not torch.equal(out[i]["input_ids"], window[i]["input_ids"])
        ends += out[i]["attention_mask"].sum(1).tolist()
    # the unlabelled row kept every key
    assert all(torch.equal(out[0][k][2], window[0][k][2]) for k in window[0])
    # the cases the window is there for: an early EOS (= pad: attended to, label -100) and rows that ran to their budget
    plens = [3, 5, 10, 8, 2, 6, 9]
    new = [e - p for e, p in zip(ends, plens)]
    assert any(0 < n < min(4, 10 - p) for n, p in zip(new, plens)) and any(n == 4 for n in new), new
    where = [(0, b) for b in range(4)] + [(2, b) for b in range(3)]
    (i, b), t = next((w, int(e) - 1) for w, e, p, n in zip(where, ends, plens, new) if 0 < n < min(4, 10 - p))
    assert int(out[i]["input_ids"][b, t]) == PAD and int(out[i]["labels"][b, t]) == I and int(out[i]["attention_mask"][b, t]) == 1


def test_budgets_seeds_and_keywords_of_the_requests():
    window = _window()
    eng = Engine()
    OP.rollout_window(eng, window, KW, SEEDS)
    got = [(s["prompt"], s["max_new_tokens"], s["seed"]) for s in eng.submitted]
    want = []
    for i, plens in ((0, [3, 5, 10, 8]), (2, [2, 6, 9])):
        for b, p in enumerate(plens):
            if p < 10:                                              # the unlabelled row is not submitted
                want.append((window[i]["input_ids"][b, :p].tolist(), min(4, 10 - p), OP.request_seed(SEEDS[i], b)))
    assert got == want and [w[1] for w in want] == [4, 4, 2, 4, 4, 1]
    for s in eng.submitted:   # the sampling keywords, and only those
        assert {k: v for k, v in s.items() if k not in ("prompt", "max_new_tokens", "seed")} == \
            {"temperature": 1.0, "top_k": 50, "eos_token_id": PAD, "pad_token_id": PAD}
    # nothing on-policy: the list comes back with the same objects and the engine is not touched
    eng = Engine()
    out = OP.rollout_window(eng, window, KW, [None, None, None])
    assert all(a is b for a, b in zip(out, window)) and not eng.submitted and eng.runs == 0
    # on-policy batches without a labelled position: nothing to submit, nothing to run
    none = dict(window[1], labels=torch.full_like(window[1]["labels"], I))
    out = OP.rollout_window(eng, [none], KW, [5])
    assert out[0] is none and not eng.submitted and eng.runs == 0


def test_request_seed_is_distinct_per_row_and_in_range():
    for seed in (0, 1, 12345, 2 ** 31 - 2):
        got = [OP.request_seed(seed, b) for b in range(64)]
        assert len(set(got)) == 64 and all(0 <= s < 2 ** 31 - 1 for s in got) and got[0] == seed


def test_every_refusal_fires_before_the_first_submit():
    good = _window()[0]
    bad_shape = dict(good, labels=good["labels"][:, :9])
    bad_teacher = dict(good, teacher_input_ids=torch.zeros(4, 11, dtype=torch.int64))
    topk = dict(good, teacher_top_k_v=torch.zeros(4, 10, 2))
    at0 = dict(good, labels=good["input_ids"].clone())              # every row labelled from position 0
    for bad, match in ((bad_shape, "labels"), (bad_teacher, "position-aligned"), (topk, "teacher model"), (at0, "position 0")):
        eng = Engine()
        with pytest.raises(ValueError, match=match):
            OP.rollout_window(eng, [good, bad], KW, [1, 2])         # the good batch comes first: still nothing submitted
        assert not eng.submitted and eng.runs == 0
    eng = Engine()
    OP.rollout_window(eng, [good, topk], KW, [1, None])             # an off-policy batch is not looked at
    assert len(eng.submitted) == 3
    with pytest.raises(ValueError, match="seeds"):
        OP.rollout_window(Engine(), [good], KW, [1, 2])
    with pytest.raises(ValueError, match="max_new_tokens"):
        OP.rollout_window(Engine(), [good], {"top_k": 1}, [1])


# ------------------------------------------------------------------------------------------------- the draw stream
@pytest.mark.parametrize("lmbda", [0.3, 1.0])
def test_draw_reproduces_the_stream_of_maybe_on_policy(lmbda, monkeypatch):
    from speech_distill_amd import trainer as TR
    n = 40
    tr = TR.DistillationTrainer.__new__(TR.DistillationTrainer)     # the draw needs no model: only these attributes
    tr.lmbda, tr.on_policy_generate, tr._on_policy_seen = lmbda, dict(KW), [0, 0]
    tr._on_policy_rng = torch.Generator().manual_seed(42)
    tr._prepare_inputs = lambda x: x
    seen = []
    monkeypatch.setattr(TR.on_policy, "rollout", lambda generate, batch, kw, seed: seen.append(seed) or "rolled")
    model = types.SimpleNamespace(generate=None)
    trainer_stream = []
    for _ in range(n):
        k = len(seen)
        r = tr._maybe_on_policy(model, "batch")
        trainer_stream.append((True, seen[-1]) if len(seen) > k else (False, None))
        assert r == ("rolled" if len(seen) > k else "batch")
    rng = torch.Generator().manual_seed(42)
    ours = [OP.draw(rng, lmbda) for _ in range(n)]
    assert ours == trainer_stream and tr._on_policy_seen == [len(seen), n]
    assert all(isinstance(s, int) and 0 <= s < 2 ** 31 - 1 for on, s in ours if on)
    if lmbda == 1.0:
        assert all(on for on, _ in ours)
    else:
        assert 0 < sum(on for on, _ in ours) < n
    # both generators are where n micro-batch draws leave them
    assert torch.equal(rng.get_state(), tr._on_policy_rng.get_state())


# ------------------------------------------------------------------------------------------------- keywords, no GPU
def _trainer(accum=1, bs=8, student=None, collator=None, **kw):
    import speech_distill_amd as sda
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    dims = sda.Qwen3Dims(640, 128, 256, 2, 2, 1)
    student = student if student is not None else sda.HipQwen3ForCausalLM(dims, device="cpu", seed=0)
    args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False, label_names=["labels"],
                             save_strategy="no", use_cpu=True, per_device_train_batch_size=bs,
                             gradient_accumulation_steps=accum)
    teacher = kw.pop("teacher_model", "build")
    if teacher == "build":
        teacher = sda.HipQwen3ForCausalLM(dims, device="cpu", seed=1)
    return DistillationTrainer(model=student, args=args, teacher_model=teacher, data_collator=collator, **kw)


def test_constructor_defaults_and_refusals(monkeypatch):
    import speech_distill_amd as sda
    from speech_distill_amd.trainer import DistillationTrainer
    plain = _trainer()
    assert plain.on_policy_rollout == "micro_batch" and plain.on_policy_engine == {} and plain._engine is None
    with pytest.raises(ValueError, match="on_policy_rollout"):
        _trainer(on_policy_rollout="epoch")
    for bad in ({"rows": 4}, {"admission": "all"}, {"max_batch": 0}, {"n_pages": 2.5}, [4]):
        with pytest.raises(ValueError, match="on_policy_engine"):
            _trainer(on_policy_engine=bad)
    # window with lmbda = 0 is inert: nothing is checked, drawn or built (not even what window mode refuses)
    monkeypatch.setenv("WORLD_SIZE", "1")
    tr = _trainer(on_policy_rollout="window", on_policy_engine={"max_batch": 32})
    assert tr.lmbda == 0.0 and tr._on_policy_rng is None and tr._engine is None and tr.engines_built == 0
    assert tr.on_policy_engine == {"max_batch": 32}
    # ---- the refusals of window mode, each before HF's constructor (the CPU student would be refused after it)
    gen = {"max_new_tokens": 8, "decode_kernels": "skinny"}
    win = dict(lmbda=0.5, on_policy_rollout="window")
    with pytest.raises(ValueError, match="teacher model"):
        _trainer(on_policy_generate=gen, teacher_model=None, **win)
    lora_student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device="cpu", seed=0)
    lora_student._lora = object()        # what lora.get_lora_model attaches (on the GPU only)
    with pytest.raises(ValueError, match="LoRA student"):
        _trainer(on_policy_generate=gen, student=lora_student, **win)
    with pytest.raises(ValueError, match="packed"):
        _trainer(on_policy_generate=gen, collator=types.SimpleNamespace(padding_free=True), **win)
    with pytest.raises(ValueError, match='"wide"'):       # 8 x 4 = 32 rows on the 16-row kernels
        _trainer(accum=4, on_policy_generate=gen, **win)
    with pytest.raises(ValueError, match='"wide"'):
        _trainer(on_policy_generate=gen, on_policy_engine={"max_batch": 17}, **win)
    with pytest.raises(ValueError, match="up to 64 rows"):
        _trainer(on_policy_generate=dict(gen, decode_kernels="wide"), on_policy_engine={"max_batch": 65}, **win)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one rank"):
        DistillationTrainer._window_plan(None, None, None, gen, {})
    monkeypatch.setenv("WORLD_SIZE", "1")
    # what passes them reaches the check every lmbda > 0 trainer makes: this student sits on the CPU
    with pytest.raises(ValueError, match="on the GPU without LoRA"):
        _trainer(accum=2, on_policy_generate=gen, **win)
    # the engine's shape: batch x accumulation rows, at most 64; explicit values are kept
    targs = types.SimpleNamespace(per_device_train_batch_size=4, gradient_accumulation_steps=3, world_size=1)
    plan = DistillationTrainer._window_plan(None, targs, None, gen, {})
    assert plan == {"max_batch": 12, "sync_every": 16, "admission": "single", "n_pages": None}
    targs.gradient_accumulation_steps = 32
    assert DistillationTrainer._window_plan(None, targs, None, {"max_new_tokens": 8, "decode_kernels": "wide"},
                                            {"admission": "batch", "n_pages": 9, "sync_every": 4}) == \
        {"max_batch": 64, "sync_every": 4, "admission": "batch", "n_pages": 9}
    with pytest.raises(ValueError, match="packed batch"):      # a packed batch that arrives anyway is refused at the window
        tr = DistillationTrainer.__new__(DistillationTrainer)
        tr.lmbda, tr.model = 0.5, None
        tr._roll_out_window([{"input_ids": torch.zeros(1, 4, dtype=torch.int64), "position_ids": torch.zeros(1, 4)}])


def _train_script():
    spec = importlib.util.spec_from_file_location("sd_train_script", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags():
    tr = _train_script()
    cfg = tr.parse_args([])
    assert (cfg.on_policy_rollout, cfg.on_policy_max_batch, cfg.on_policy_admission) == ("micro_batch", None, "single")
    assert tr.distill_kwargs(cfg, pad=5) == {}
    # window at --lmbda 0 is accepted and inert: no keyword reaches the trainer
    cfg = tr.parse_args(["--on_policy_rollout", "window", "--on_policy_max_batch", "32", "--on_policy_admission", "batch"])
    assert tr.distill_kwargs(cfg, pad=5) == {}
    base = ["--lmbda", "0.5", "--divergence", "reverse_kl_tail", "--on_policy_decode_kernels", "wide"]
    kw = tr.distill_kwargs(tr.parse_args(base), pad=5)
    assert "on_policy_rollout" not in kw and "on_policy_engine" not in kw      # the defaults pass nothing new
    kw = tr.distill_kwargs(tr.parse_args(base + ["--on_policy_rollout", "window"]), pad=5)
    assert kw["on_policy_rollout"] == "window" and "on_policy_engine" not in kw and kw["lmbda"] == 0.5
    kw = tr.distill_kwargs(tr.parse_args(base + ["--on_policy_rollout", "window", "--on_policy_max_batch", "32",
                                                 "--on_policy_admission", "batch"]), pad=5)
    assert kw["on_policy_engine"] == {"max_batch": 32, "admission": "batch"}
    for bad in (["--on_policy_rollout", "epoch"], ["--on_policy_admission", "all"], ["--on_policy_max_batch", "0"]):
        with pytest.raises(SystemExit):
            tr.parse_args(bad)
