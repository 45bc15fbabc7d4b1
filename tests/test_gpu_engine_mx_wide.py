"""-m gpu: the request engine (speech_distill_amd/engine.py) on MXFP8 weights with ``gemv_rows=64``, above the 16 rows of
the skinny MXFP8 step.  The scenario of tests/test_gpu_engine_wide.py, restated: a request served by a 20-row engine with
("skinny", "mxfp8", gemv_rows=64) yields, bit for bit, the tokens a one-row session with the same three keywords over another
pool yields for it alone, cut at its EOS, over bf16 and over MXFP8 pages; and the engine's statistics are the scheduler's,
replayed on the host from the realised lengths.  All comparisons are torch.equal."""
import pytest
import torch

from gpu_util import dev
from speech_distill_amd.engine import Replay

pytestmark = pytest.mark.gpu

STUDENT = (640, 128, 256, 2, 2, 1)   # the "student" shape, prompts and lengths of tests/test_gpu_generate.py, restated
PROMPT_LENS = [24, 17, 9, 1]


def _prompts():
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 640, (4, 24), generator=g)
    cont = torch.randint(0, 640, (4, 64), generator=g)
    return ids, cont

PAD, MAX_BATCH, N_PAGES = 2, 20, 14
MODE = dict(decode_kernels="skinny", weight_dtype="mxfp8", gemv_rows=64)
GREEDY = dict(do_sample=False, repetition_penalty=1.3)
REQUESTS = [   # (prompt row, prompt length, seed, budget, sampling keywords): 12 requests, budgets <= 24
    (0, PROMPT_LENS[0], 21, 24, dict(do_sample=True, temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.25,
                                     use_ras=True, win_size=25, tau_r=0.2, min_new_tokens=8)),
    (1, PROMPT_LENS[1], 22, 20, dict(do_sample=True, temperature=1.3, top_k=20, top_p=0.8, min_new_tokens=3)),
    (2, PROMPT_LENS[2], 23, 12, GREEDY),
    (3, PROMPT_LENS[3], 24, 24, dict(do_sample=True, temperature=0.8, top_k=0, repetition_penalty=1.2)),
    (0, PROMPT_LENS[1], 25, 18, dict(do_sample=True, temperature=1.5, top_k=2, min_new_tokens=1)),
    (1, PROMPT_LENS[2], 26, 24, dict(do_sample=True, temperature=0.9, top_k=128, use_ras=True, win_size=10, tau_r=0.3)),
    (2, PROMPT_LENS[0], 27, 5, GREEDY),
    (3, PROMPT_LENS[0], 28, 16, dict(do_sample=True, temperature=1.0, top_k=50)),
    (0, PROMPT_LENS[2], 29, 1, dict(do_sample=True, temperature=0.7, top_k=10, top_p=0.95)),
    (1, PROMPT_LENS[3], 30, 22, dict(do_sample=False)),
    (2, PROMPT_LENS[1], 31, 9, dict(do_sample=True, temperature=2.0, top_k=0)),
    (3, PROMPT_LENS[2], 32, 24, dict(do_sample=True, temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.25)),
]


@pytest.fixture(scope="module")
def model():
    import speech_distill_amd as sda
    from oracle import qwen3 as Q
    w = {k: v.bfloat16().float() for k, v in Q.init_weights(Q.Qwen3Shape(*STUDENT), seed=1).items()}
    m = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*STUDENT), device=dev(), init_std=0)
    m.load_hf_state_dict(w)
    return m.eval().requires_grad_(False)   # MXFP8 weights are for a frozen model


def _prompt(i):
    row, T = REQUESTS[i][0], REQUESTS[i][1]
    return _prompts()[0][row, :T].to(dev())


def _alone(model, i, eos, kv_dtype):
    """The yardstick: a one-row session with the same three keywords over a pool of its own, cut at the first EOS."""
    _, T, seed, budget, kw = REQUESTS[i]
    pool = model.kv_page_pool(2, kv_dtype=kv_dtype)
    sess = model.start_session(1, 256, pool=pool, **MODE)
    new = sess.generate(_prompt(i)[None], max_new_tokens=budget, eos_token_id=eos, pad_token_id=PAD, seed=seed, **kw)[0]
    sess.close()
    hit = (new == eos).nonzero().flatten() if eos is not None else new[:0]
    return new[:int(hit[0]) + 1] if hit.numel() else new


@pytest.fixture(scope="module")
def eos(model):
    """A token that makes request 0 (budget 24, at least 8 new tokens) stop early.  Suppressing the EOS during the first 8
    steps shifts the draws of a model whose logits are this flat, so a candidate -- a token request 0 draws at step 10 or
    later without an EOS -- is kept only once the run WITH it as the EOS has stopped before the budget."""
    seq = _alone(model, 0, None, "bf16").tolist()
    for _ in range(3):
        for cand in dict.fromkeys(seq[10:]):
            seq = _alone(model, 0, cand, "bf16").tolist()
            if len(seq) < REQUESTS[0][3]:
                return cand
    raise AssertionError("no EOS candidate stops request 0 early")


@pytest.mark.parametrize("kv_dtype", ["bf16", "mxfp8"])
def test_every_request_of_a_20_row_engine_equals_the_one_row_session(model, eos, kv_dtype):
    want = [_alone(model, i, eos, kv_dtype) for i in range(len(REQUESTS))]
    lens, budgets = [w.numel() for w in want], [r[3] for r in REQUESTS]
    if kv_dtype == "bf16":
        assert any(n < b for n, b in zip(lens, budgets)) and any(n == b for n, b in zip(lens, budgets))
    pool = model.kv_page_pool(N_PAGES, kv_dtype=kv_dtype)
    free = pool.free_pages
    eng = model.generation_engine(pool, max_batch=MAX_BATCH, sync_every=16, **MODE)
    assert eng.decoder.mx_wide and eng.gemv_rows == 64 and eng.decoder.B == MAX_BATCH
    rids = [eng.submit(_prompt(i), max_new_tokens=r[3], seed=r[2], eos_token_id=eos, pad_token_id=PAD, **r[4])
            for i, r in enumerate(REQUESTS)]
    done = eng.run()
    assert sorted(done) == sorted(rids)
    for i, rid in enumerate(rids):
        got = eng.result(rid)
        assert got.dtype == torch.int64 and got.dim() == 1 and torch.equal(got, want[i]), (i, got.tolist(), want[i].tolist())
    stats = dict(eng.stats)
    rep = Replay(max_batch=MAX_BATCH, n_pages=N_PAGES, max_pages=eng.decoder.max_pages, capacity=eng.sched.capacity,
                 sync_every=16)
    for (_, T, _, budget, _), n in zip(REQUESTS, lens):
        rep.submit(T, budget, n)
    rep.run()
    print("realised lengths", lens, "of budgets", budgets, "stats", stats)
    assert stats == rep.stats and stats["prefills"] == len(REQUESTS)
    assert pool.free_pages == free - 1
    eng.close()
    assert pool.free_pages == free
