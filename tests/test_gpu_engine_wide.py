"""-m gpu: the request engine (speech_distill_amd/engine.py) with decode_kernels="wide" above the 16 rows of the skinny step.
The contract of tests/test_gpu_engine.py carries over as written: a request served by a 20-row engine yields, bit for bit,
the tokens a one-row "wide" session over another pool yields for it alone, cut at its EOS, over bf16 and over MXFP8 pages;
and the engine's statistics are the scheduler's, replayed on the host from the realised lengths.  All comparisons are
torch.equal."""
import pytest
import torch

from gpu_util import dev
from speech_distill_amd.engine import Replay
from test_gpu_generate import PROMPT_LENS, _model, _prompts

pytestmark = pytest.mark.gpu

PAD, MAX_BATCH, N_PAGES = 2, 20, 14
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
    m, _, _ = _model("student")
    return m


def _prompt(i):
    row, T = REQUESTS[i][0], REQUESTS[i][1]
    return _prompts()[0][row, :T].to(dev())


def _alone(model, i, eos, kv_dtype):
    """The yardstick: a one-row "wide" session over a pool of its own, cut at the first EOS."""
    _, T, seed, budget, kw = REQUESTS[i]
    pool = model.kv_page_pool(2, kv_dtype=kv_dtype)
    sess = model.start_session(1, 256, pool=pool, decode_kernels="wide")
    new = sess.generate(_prompt(i)[None], max_new_tokens=budget, eos_token_id=eos, pad_token_id=PAD, seed=seed, **kw)[0]
    sess.close()
    hit = (new == eos).nonzero().flatten() if eos is not None else new[:0]
    return new[:int(hit[0]) + 1] if hit.numel() else new


@pytest.fixture(scope="module")
def eos(model):
    """A token request 0 (budget 24, at least 8 new tokens) draws for the first time at its step 10 or later: that
    request stops early."""
    seq = _alone(model, 0, None, "bf16").tolist()
    return next(t for j, t in enumerate(seq) if j >= 10 and t not in seq[:j])


@pytest.mark.parametrize("kv_dtype", ["bf16", "mxfp8"])
def test_every_request_of_a_20_row_wide_engine_equals_the_one_row_wide_session(model, eos, kv_dtype):
    want = [_alone(model, i, eos, kv_dtype) for i in range(len(REQUESTS))]
    lens, budgets = [w.numel() for w in want], [r[3] for r in REQUESTS]
    if kv_dtype == "bf16":
        assert any(n < b for n, b in zip(lens, budgets)) and any(n == b for n, b in zip(lens, budgets))
    pool = model.kv_page_pool(N_PAGES, kv_dtype=kv_dtype)
    free = pool.free_pages
    eng = model.generation_engine(pool, max_batch=MAX_BATCH, decode_kernels="wide", sync_every=16)
    assert eng.decoder.wide and eng.decoder.B == MAX_BATCH
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
