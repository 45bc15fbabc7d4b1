"""-m gpu: the on-policy window rollout (on_policy.rollout_window through a GenerationEngine) on the
tiny model of tests/test_gpu_engine.py.  The window: three micro-batches of two rows, T = 24, max_new_tokens = 8, prompts
of 3, 7, 11, 16 and 20 tokens (the last one's width leaves it 4 tokens) and one row without a label.  With "skinny" and
"wide" kernels and admission="single" everything is torch.equal against ``model.generate`` on each prompt alone."""
import tempfile

import pytest
import torch

from gpu_util import dev, record
from speech_distill_amd import on_policy as OP
from test_gpu_generate import _model

pytestmark = pytest.mark.gpu

T, NEW, V, PAD = 24, 8, 640, 2
PLENS = [[3, 7], [11, T], [16, 20]]          # T: no labelled position
SEEDS = [101, 202, 303]


@pytest.fixture(scope="module")
def model():
    m, _, _ = _model("student")
    return m


def _window(device=None):
    """The three micro-batches (CPU unless ``device``): random tokens, labels on everything behind the prompt."""
    g = torch.Generator().manual_seed(7)
    out = []
    for plens in PLENS:
        ids = torch.randint(3, V, (2, T), generator=g)
        labels = ids.clone()
        for b, p in enumerate(plens):
            labels[b, :p] = -100
        tids = ids.clone()
        tids[:, 0] = 1
        b = {"input_ids": ids, "attention_mask": torch.ones(2, T, dtype=torch.int64), "labels": labels,
             "teacher_input_ids": tids, "teacher_attention_mask": torch.ones(2, T, dtype=torch.int64)}
        out.append({k: v.to(device) for k, v in b.items()} if device is not None else b)
    return out


def _live():
    """(micro-batch, row, prompt length, budget) of every row that is submitted, in submission order."""
    return [(i, b, p, min(NEW, T - p)) for i, plens in enumerate(PLENS) for b, p in enumerate(plens) if p < T]


def _alone(model, window, kw, eos):
    """The yardstick: ``model.generate`` on each prompt alone with the row's budget, request_seed and keywords; -> the
    completions cut behind their first EOS, in submission order."""
    sampling = {k: v for k, v in kw.items() if k not in ("max_new_tokens", "eos_token_id", "pad_token_id")}
    out = []
    for i, b, p, n in _live():
        full = model.generate(window[i]["input_ids"][b:b + 1, :p], max_new_tokens=n, seed=OP.request_seed(SEEDS[i], b),
                              eos_token_id=eos, pad_token_id=PAD if eos is not None else None, **sampling)
        new = full[0, p:]
        hit = (new == eos).nonzero().flatten() if eos is not None else new[:0]
        out.append(new[:int(hit[0]) + 1] if hit.numel() else new)
    return out


def _rebuilt_by_hand(window, tokens, eos):
    """``replace_completion`` on the yardstick's tokens, PAD behind each completion's end."""
    out = []
    for i, batch in enumerate(window):
        new = torch.full((2, NEW), PAD, dtype=torch.int64, device=dev())
        for (j, b, _, _), tok in zip(_live(), tokens):
            if j == i:
                new[b, :tok.numel()] = tok
        out.append(OP.replace_completion(batch, new, OP.prompt_lengths(batch["labels"]), eos, PAD))
    return out


def _engine(model, kernels, max_batch=4, admission="single", sync_every=4):
    pool = model.kv_page_pool(max_batch + 1)
    return pool, model.generation_engine(pool, max_batch=max_batch, decode_kernels=kernels, sync_every=sync_every,
                                         admission=admission)


def _roll(eng, window, kw):
    """rollout_window with the engine's results recorded: -> (rebuilt batches, the requests' tokens in submission order)."""
    got, inner = [], eng.result
    eng.result = lambda rid: (got.append(inner(rid)), got[-1])[1]
    try:
        return OP.rollout_window(eng, window, kw, SEEDS), got
    finally:
        del eng.result


@pytest.mark.parametrize("top_k", [0, 50])
@pytest.mark.parametrize("kernels", ["skinny", "wide"])
def test_window_rollout_equals_one_row_generate(model, kernels, top_k):
    """The EOS id is read from a first run of the one-row yardstick with the case's own sampling keywords and no EOS (the
    third token of the first request): the same seed draws the same tokens up to it, so that request is sure to stop
    early -- a token of a greedy run need not come up in a sampled one."""
    window = _window(dev())
    base = {"max_new_tokens": NEW, "temperature": 1.0, "top_k": top_k, "decode_kernels": kernels}
    eos = int(_alone(model, window, base, None)[0][2])
    kw = dict(base, eos_token_id=eos, pad_token_id=PAD)
    want = _alone(model, window, kw, eos)
    lens, budgets = [w.numel() for w in want], [n for _, _, _, n in _live()]
    assert budgets == [8, 8, 8, 8, 4] and lens[0] <= 3 and any(n < b for n, b in zip(lens, budgets)), (lens, budgets)
    pool, eng = _engine(model, kernels)         # 5 requests in 4 rows: one row is refilled
    free = pool.free_pages
    out, got = _roll(eng, window, kw)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.dtype == torch.int64 and torch.equal(a, b), (a.tolist(), b.tolist())
    by_hand = _rebuilt_by_hand(window, want, eos)
    for o, h, src in zip(out, by_hand, window):
        assert set(o) == set(src) and all(torch.equal(o[k], h[k]) for k in src)
    assert torch.equal(out[1]["input_ids"][1], window[1]["input_ids"][1])       # the unlabelled row
    assert eng.stats["prefills"] == 5 and not eng.requests                       # finished requests were dropped
    assert pool.free_pages == free                                               # every page but the parking page is back
    eng.close()


def test_one_engine_follows_the_live_weights():
    """ONE engine, two rollouts of the same window with the flat weights changed in place between them (N(0, 0.05) added:
    more than twice the init's std, so the yardstick itself changes)."""
    m, _, _ = _model("student")
    window = _window(dev())
    kw = {"max_new_tokens": NEW, "temperature": 1.0, "top_k": 50, "decode_kernels": "skinny"}
    pool, eng = _engine(m, "skinny")
    first = _roll(eng, window, kw)[1]
    want_first = _alone(m, window, kw, None)
    assert all(torch.equal(a, b) for a, b in zip(first, want_first))
    with torch.no_grad():
        m.flat.add_((0.05 * torch.randn(m.flat.numel(), generator=torch.Generator().manual_seed(3))).to(m.flat))
    eng.reset_stats()
    second = _roll(eng, window, kw)[1]
    want_second = _alone(m, window, kw, None)
    assert any(not torch.equal(a, b) for a, b in zip(want_first, want_second)), "the perturbation must move the yardstick"
    assert all(torch.equal(a, b) for a, b in zip(second, want_second))
    assert any(not torch.equal(a, b) for a, b in zip(first, second))
    assert eng.stats["prefills"] == 5 and not eng.requests and pool.free_pages == pool.n_pages - 1
    eng.close()


def _first_logits(model, window, admission):
    """Serve the window's five requests with the rows' first-step logits (the prefill's) recorded.
    -> ({request id: logits fp32 CPU}, the rows of each prefill pass, the engine, its pool, the request ids)."""
    pool, eng = _engine(model, "wide", admission=admission)
    seen, passes = {}, []
    seat, pre = eng._seat, eng.decoder.prefill_rows
    eng._seat = lambda req, logits: (seen.__setitem__(req.id, logits.float().cpu()), seat(req, logits))[1]
    eng.decoder.prefill_rows = lambda rows, *a, **k: (passes.append(list(rows)), pre(rows, *a, **k))[1]
    rids = [eng.submit(window[i]["input_ids"][b, :p], max_new_tokens=n, seed=OP.request_seed(SEEDS[i], b), temperature=1.0,
                       top_k=50, eos_token_id=5, pad_token_id=5) for i, b, p, n in _live()]
    eng.run()
    return seen, passes, eng, pool, rids


def test_batch_admission_properties_and_logits_budget():
    """admission="batch" gives up the one-row bit contract, so: properties of the tokens, and the admitted rows' first-step
    logits against the fp32 CPU oracle within 1.5 x the error of the "single" admission's logits against the same oracle
    (rms over the rows that shared a prefill pass)."""
    from oracle import qwen3 as Q
    m, shape, w = _model("student")
    window = _window(dev())
    seen_b, passes_b, eng, pool, rids = _first_logits(m, window, "batch")
    assert passes_b[0] == [0, 1, 2, 3] and sum(len(p) for p in passes_b) == 5    # four rows in ONE pass, then the refill
    for rid, (_, _, _, n) in zip(rids, _live()):
        tok = eng.result(rid)
        assert 1 <= tok.numel() <= n and bool(((tok >= 0) & (tok < V)).all())    # within budget, in the vocabulary
        assert not bool((tok[:-1] == 5).any()) and (int(tok[-1]) == 5 or tok.numel() == n)   # nothing follows an EOS
    assert pool.free_pages == pool.n_pages - 1                                   # the pages are returned
    eng.forget()
    assert not eng.requests
    eng.close()
    seen_s, passes_s, eng_s, _, _ = _first_logits(m, window, "single")
    assert all(len(p) == 1 for p in passes_s) and len(passes_s) == 5
    eng_s.close()
    shared = rids[:4]
    with torch.no_grad():
        ora = {rid: Q.forward(w, shape, window[i]["input_ids"][b:b + 1, :p].cpu())[0, -1].float()
               for rid, (i, b, p, _) in zip(rids, _live())}

    def rms(seen):
        return float(torch.stack([seen[r] - ora[r] for r in shared]).double().pow(2).mean().sqrt())
    err_batch, err_single = rms(seen_b), rms(seen_s)
    record("on_policy_window_batch_admission_logits", err_batch=err_batch, err_single=err_single, factor=1.5)
    print(f"first-step logits vs the fp32 oracle: batch {err_batch:.3e}, single {err_single:.3e}")
    assert err_single > 0 and err_batch <= 1.5 * err_single


# ------------------------------------------------------------------------------------------------------- the trainer
def _rows(n_batches):
    out = []
    for k in range(n_batches):
        for batch in _window():
            for b in range(2):
                out.append({key: v[b].clone() for key, v in batch.items()})
    return out


def _collate(feats):
    return {k: torch.stack([f[k] for f in feats]) for k in feats[0]}


def _trainer(lmbda, max_steps=2, **kw):
    import speech_distill_amd as sda
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 128, 256, 2, 2, 1), device=dev(), seed=0)
    teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 256, 512, 2, 4, 2), device=dev(), seed=1)
    teacher.eval().requires_grad_(False)
    args = TrainingArguments(
        output_dir=tempfile.mkdtemp(), per_device_train_batch_size=2, gradient_accumulation_steps=3, max_steps=max_steps,
        learning_rate=1e-3, logging_steps=1, save_strategy="no", report_to=[], remove_unused_columns=False,
        label_names=["labels"], seed=42, data_seed=42, lr_scheduler_type="constant", warmup_steps=0, weight_decay=0.0,
        max_grad_norm=1.0, dataloader_num_workers=0, bf16=True)
    tr = DistillationTrainer(model=student, args=args, train_dataset=_rows(max_steps), data_collator=_collate,
                             teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=16, divergence="reverse_kl_tail",
                             lmbda=lmbda, on_policy_rollout="window",
                             on_policy_generate={"max_new_tokens": NEW, "temperature": 1.0, "top_k": 50,
                                                 "decode_kernels": "skinny", "eos_token_id": PAD, "pad_token_id": PAD}, **kw)
    tr._get_train_sampler = lambda *a, **k: torch.utils.data.SequentialSampler(tr.train_dataset)
    tr.logged = []
    tr.log = lambda d, *a, **k: tr.logged.append(dict(d))
    return tr, student


def test_trainer_rolls_out_window_by_window_through_one_engine():
    tr, student = _trainer(1.0)
    assert tr.on_policy_engine == {"max_batch": 6, "sync_every": 16, "admission": "single", "n_pages": None}
    windows, counted = [], []
    inner = tr._roll_out_window

    def spy(batch_samples):
        grad = student.flat_grad.clone() if student.flat_grad is not None else None
        training = student.training
        out = inner(batch_samples)
        torch.cuda.synchronize()
        same_grad = grad is None or torch.equal(student.flat_grad.view(torch.int16), grad.view(torch.int16))
        windows.append(dict(given=list(batch_samples), out=list(out), same_grad=same_grad,
                            training=(training, student.training),
                            pages=(tr._engine_pool.free_pages, tr._engine_pool.n_pages), requests=len(tr._engine.requests)))
        return out
    tr._roll_out_window = spy
    step = tr.compute_loss
    tr.compute_loss = lambda *a, **k: (counted.append(tuple(tr._on_policy_seen)), step(*a, **k))[1]
    start = student.flat.clone()
    tr.train()
    assert tr.state.global_step == 2 and not torch.equal(student.flat, start) and student.training
    assert len(windows) >= 2 and tr.engines_built == 1                      # one engine for every window
    for w in windows[:2]:
        assert len(w["given"]) == 3 and w["same_grad"] and w["training"] == (True, True)
        assert w["pages"] == (6 * 1, 6 * 1 + 1) and w["requests"] == 0     # all but the parking page are back in the pool
        for given, out in zip(w["given"], w["out"]):
            assert out is not given and out["input_ids"].shape == (2, T)
            assert not torch.equal(out["input_ids"], given["input_ids"].to(dev()))
    # the counters: each of the 6 micro-batches is seen, and on-policy, when its step comes
    assert counted == [(1, 1)] * 6
    fr = [h["on_policy_fraction"] for h in tr.logged if "on_policy_fraction" in h]
    assert fr == [1.0] * 6
    losses = [h[k] for h in tr.logged for k in ("student_loss", "teacher_loss", "distill_loss") if k in h]
    assert len(losses) == 18 and all(x == x and abs(x) < float("inf") for x in losses)
    pool = tr._engine_pool
    tr.close_engine()
    assert tr._engine is None and pool.free_pages == pool.n_pages


def test_trainer_passes_undrawn_micro_batches_through():
    tr, student = _trainer(0.5, max_steps=2)
    windows = []
    inner = tr._roll_out_window
    tr._roll_out_window = lambda bs: (windows.append((list(bs), inner(bs))), windows[-1][1])[1]
    tr.train()
    rng = torch.Generator().manual_seed(42)                                 # args.seed + process index 0
    got, want = [], []
    for given, out in windows:
        assert len(out) == len(given)
        want += [OP.draw(rng, 0.5)[0] for _ in given]
        got += [o is not g for g, o in zip(given, out)]                      # undrawn: the same object comes back
    assert got == want and want[:6] == [False, False, True, False, True, True], (got, want)   # (seed 42's stream)
    fr = [h["on_policy_fraction"] for h in tr.logged if "on_policy_fraction" in h]
    assert fr == [float(x) for x in got[:6]]
    assert tr.engines_built == 1
    tr.close_engine()
