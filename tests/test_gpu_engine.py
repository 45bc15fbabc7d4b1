"""-m gpu: the request engine (speech_distill_amd/engine.py) in skinny mode.  The contract is exact: a request served by the
engine yields, bit for bit, the tokens a one-row session over another pool yields for it alone, cut at its EOS -- whatever
``sync_every``, the submission timing, the pool's page order or ``max_batch``.  Six requests over the four prompt lengths
of tests/test_gpu_generate.py, two rows, four pages (one parked): two requests need two pages each, so rows are refilled
and the head of the queue waits for pages.  All comparisons are torch.equal."""
import pytest
import torch

from gpu_util import dev
from speech_distill_amd.engine import Replay
from test_gpu_generate import PROMPT_LENS, _model, _prompts

pytestmark = pytest.mark.gpu

PAD = 2
GREEDY = dict(do_sample=False, repetition_penalty=1.3)
REQUESTS = [   # (prompt row, prompt length, seed, budget, sampling keywords)
    (0, PROMPT_LENS[0], 11, 40, dict(do_sample=True, temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.25,
                                     use_ras=True, win_size=25, tau_r=0.2, min_new_tokens=8)),
    (1, PROMPT_LENS[1], 12, 250, dict(do_sample=True, temperature=1.3, top_k=20, top_p=0.8, min_new_tokens=3)),
    (2, PROMPT_LENS[2], 13, 12, GREEDY),
    (3, PROMPT_LENS[3], 14, 30, dict(do_sample=True, temperature=0.8, top_k=0, repetition_penalty=1.2)),
    (0, PROMPT_LENS[1], 15, 260, dict(do_sample=True, temperature=1.5, top_k=2, min_new_tokens=1)),
    (1, PROMPT_LENS[2], 16, 25, dict(do_sample=True, temperature=0.9, top_k=128, use_ras=True, win_size=10, tau_r=0.3)),
]


@pytest.fixture(scope="module")
def model():
    m, _, _ = _model("student")
    return m


def _prompt(i):
    row, T = REQUESTS[i][0], REQUESTS[i][1]
    return _prompts()[0][row, :T].to(dev())


def _alone(model, i, eos, kv_dtype="bf16", weight_dtype="bf16"):
    """The yardstick: a one-row session over a pool of its own, cut at the first EOS."""
    _, T, seed, budget, kw = REQUESTS[i]
    pool = model.kv_page_pool(3, kv_dtype=kv_dtype)
    sess = model.start_session(1, 512, pool=pool, decode_kernels="skinny", weight_dtype=weight_dtype)
    new = sess.generate(_prompt(i)[None], max_new_tokens=budget, eos_token_id=eos, pad_token_id=PAD, seed=seed, **kw)[0]
    sess.close()
    hit = (new == eos).nonzero().flatten() if eos is not None else new[:0]
    return new[:int(hit[0]) + 1] if hit.numel() else new


@pytest.fixture(scope="module")
def eos(model):
    """The first token that request 1 (budget 250, two pages) draws for the first time after its 100th step: that request
    stops early, but only after the short ones before request 4 are done -- so request 4, which needs two pages too,
    finds a free row and has to wait for pages."""
    seq = _alone(model, 1, None).tolist()
    return next(t for j, t in enumerate(seq) if 100 <= j < 240 and t not in seq[:j])


@pytest.fixture(scope="module")
def want(model, eos):
    return [_alone(model, i, eos) for i in range(len(REQUESTS))]


def _submit(eng, i, eos, pad=PAD):
    _, _, seed, budget, kw = REQUESTS[i]
    return eng.submit(_prompt(i), max_new_tokens=budget, seed=seed, eos_token_id=eos, pad_token_id=pad, **kw)


def _serve(model, eos, max_batch=2, sync_every=16, n_pages=4, order=None, late=False, decode_kernels="skinny",
           kv_dtype="bf16", weight_dtype="bf16", pad=PAD):
    """-> (results in submission order, the engine's stats, (its table's pages per row, its capacity))."""
    pool = model.kv_page_pool(n_pages, order=order, kv_dtype=kv_dtype)
    free = pool.free_pages
    eng = model.generation_engine(pool, max_batch=max_batch, decode_kernels=decode_kernels, sync_every=sync_every,
                                  weight_dtype=weight_dtype)
    shape = (eng.decoder.max_pages, eng.sched.capacity)
    n = len(REQUESTS)
    if late:      # two up front, one more after every third step
        rids, done = [_submit(eng, 0, eos, pad), _submit(eng, 1, eos, pad)], []
        it = 0
        while len(rids) < n or eng.sched.live or eng.sched.waiting:
            done += eng.step()
            it += 1
            if it % 3 == 0 and len(rids) < n:
                rids.append(_submit(eng, len(rids), eos, pad))
    else:
        rids = [_submit(eng, i, eos, pad) for i in range(n)]
        done = eng.run()
    assert sorted(done) == sorted(rids)
    out = [eng.result(r) for r in rids]
    stats = dict(eng.stats)
    assert pool.free_pages == free - 1          # everything but the parking page is back ...
    eng.close()
    assert pool.free_pages == free              # ... and close() returns that one too
    return out, stats, shape


def _equal(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == torch.int64 and a.dim() == 1 and torch.equal(a, b), (i, a.tolist(), b.tolist())


def test_every_request_equals_the_one_row_session(model, eos, want):
    lens = [w.numel() for w in want]
    budgets = [r[3] for r in REQUESTS]
    assert any(n < b for n, b in zip(lens, budgets)) and any(n == b for n, b in zip(lens, budgets))   # early stops and full runs
    got, stats, (max_pages, capacity) = _serve(model, eos)
    _equal(got, want)
    assert stats["prefills"] == len(REQUESTS) and stats["peak_pages"] == 4
    # the step count is the scheduler's, replayed on the host from the realised lengths
    rep = Replay(max_batch=2, n_pages=4, max_pages=max_pages, capacity=capacity, sync_every=16)
    for (_, T, _, budget, _), n in zip(REQUESTS, lens):
        rep.submit(T, budget, n)
    rep.run()
    print("realised lengths", lens, "of budgets", budgets, "stats", stats)
    assert stats == rep.stats
    roomy = Replay(max_batch=2, n_pages=16, max_pages=max_pages, capacity=capacity, sync_every=16)
    for (_, T, _, budget, _), n in zip(REQUESTS, lens):
        roomy.submit(T, budget, n)
    roomy.run()
    assert roomy.stats["iterations"] < stats["iterations"]      # the head of the queue really waited for pages
    assert stats["decode_steps"] < sum(max(budgets[i:i + 2]) for i in range(0, 6, 2))   # fewer than the static schedule's


def test_results_do_not_depend_on_sync_every(model, eos, want):
    _equal(_serve(model, eos, sync_every=1)[0], want)


def test_results_do_not_depend_on_submission_timing(model, eos, want):
    _equal(_serve(model, eos, late=True)[0], want)


def test_results_do_not_depend_on_the_page_order(model, eos, want):
    _equal(_serve(model, eos, n_pages=6, order=[4, 1, 5, 0, 3, 2])[0], want)


def test_results_do_not_depend_on_max_batch(model, eos, want):
    _equal(_serve(model, eos, max_batch=4, n_pages=7)[0], want)


def test_mxfp8_pages_equal_the_one_row_session_over_such_pages(model, eos):
    got = _serve(model, eos, kv_dtype="mxfp8")[0]
    _equal(got, [_alone(model, i, eos, kv_dtype="mxfp8") for i in range(len(REQUESTS))])


def test_mxfp8_weights_equal_the_one_row_session_with_such_weights(eos):
    m, _, _ = _model("student")
    m.eval().requires_grad_(False)
    got = _serve(m, eos, weight_dtype="mxfp8")[0]
    _equal(got, [_alone(m, i, eos, weight_dtype="mxfp8") for i in range(len(REQUESTS))])


def test_tile_mode_is_served_with_property_checks_only(model, eos):
    """The tile step is not batch-invariant, so no equality is claimed: tokens lie in range, lengths are within budget,
    and pad (here the EOS id itself, the default, so that no sampled token can be mistaken for padding) never appears
    before the EOS -- only a result's last token may be it, and a result without it has spent its budget."""
    got, stats, _ = _serve(model, eos, decode_kernels="tile", pad=eos)
    for (_, _, _, budget, _), t in zip(REQUESTS, got):
        assert 1 <= t.numel() <= budget and bool(((t >= 0) & (t < 640)).all())
        assert not bool((t[:-1] == eos).any())
        assert int(t[-1]) == eos or t.numel() == budget
    assert stats["prefills"] == len(REQUESTS)


def test_submit_refuses_what_can_never_run_and_changes_nothing(model):
    pool = model.kv_page_pool(3)
    eng = model.generation_engine(pool, max_batch=2)
    ids = _prompt(0)
    before = (pool.free_pages, len(eng.sched.waiting), len(eng.requests))
    for kw in (dict(max_new_tokens=0), dict(max_new_tokens=600), dict(top_k=129), dict(top_k=0, top_p=0.5),
               dict(temperature=0.0), dict(use_ras=True, top_k=5, win_size=0), dict(eos_token_id=640),
               dict(pad_token_id=-1), dict(min_new_tokens=-1)):
        with pytest.raises(ValueError):
            eng.submit(ids, **kw)
        assert (pool.free_pages, len(eng.sched.waiting), len(eng.requests)) == before
    with pytest.raises(ValueError):
        eng.submit(ids[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.submit(ids.cpu())
    rid = eng.submit(ids, max_new_tokens=3, do_sample=False)
    with pytest.raises(ValueError, match="not finished"):
        eng.result(rid)
    assert eng.run() == [rid] and eng.result(rid).numel() == 3
    eng.close()
    assert pool.free_pages == 3
