"""The scheduler of the request engine (speech_distill_amd/engine.py) on the host alone: ``Replay`` is the engine's loop
with a stub decoder (lengths given in advance), so admission order, page accounting and the step count are checked
without a device.  Plus the command line of scripts/generate.py --continuous."""
import importlib.util
import os

import pytest

from conftest import ROOT
from speech_distill_amd.engine import Replay, Scheduler, static_steps
from speech_distill_amd.paged import PAGE, PageAllocator, PageTable


def _sched(n_pages=8, B=2, max_pages=4, capacity=1024, sync_every=16):
    alloc = PageAllocator(n_pages)
    return Scheduler(PageTable(alloc, B, max_pages), capacity, sync_every), alloc


def _snapshot(s):
    return ([list(r) for r in s.table.rows], set(s.table.dirty), list(s.alloc._free), list(s.alloc.refs), list(s.free_rows),
            [r.id for r in s.waiting], sorted(s.live), s._next_id)


def test_admission_is_strict_fifo():
    s, _ = _sched(n_pages=9, B=2)
    reqs = [s.submit(10, 20), s.submit(300, 300), s.submit(5, 5), s.submit(7, 7)]
    assert [r.id for r in reqs] == [0, 1, 2, 3]
    first = s.admit()
    assert [r.id for r in first] == [0, 1] and [r.row for r in first] == [0, 1]
    assert s.admit() == []                                  # no free row
    s.finish(1)
    assert [(r.id, r.row) for r in s.admit()] == [(2, 1)]   # the freed row goes to the next in line
    s.finish(0)
    assert [(r.id, r.row) for r in s.admit()] == [(3, 0)]
    assert not s.waiting


def test_the_head_waits_for_pages_and_is_never_overtaken():
    s, alloc = _sched(n_pages=4, B=2)           # 3 usable pages
    s.submit(200, 300)                          # 2 pages
    s.submit(400, 200)                          # 3 pages: must wait for the first to finish
    s.submit(1, 1)                              # 1 page: would fit now, but is behind the head
    assert [r.id for r in s.admit()] == [0]
    before = _snapshot(s)
    assert s.admit() == [] and _snapshot(s) == before       # a refused admission leaves everything untouched
    assert alloc.free_pages == 1 and s.free_rows == [1]
    s.finish(0)
    assert [r.id for r in s.admit()] == [1]                 # admitted after the release ...
    assert s.admit() == [] and [r.id for r in s.waiting] == [2]   # ... and the small one still waits (no page left)
    s.finish(0)
    assert [r.id for r in s.admit()] == [2]


def test_a_request_that_can_never_fit_raises_at_submit_and_changes_nothing():
    s, _ = _sched(n_pages=4, B=2, max_pages=4, capacity=900)
    s.submit(10, 10)
    before = _snapshot(s)
    for T, n in ((0, 5), (5, 0), (500, 401), (3 * PAGE, 1), (700, 200)):
        with pytest.raises(ValueError):
            s.submit(T, n)
        assert _snapshot(s) == before
    s2, _ = _sched(n_pages=8, B=1, max_pages=2, capacity=4096)
    with pytest.raises(ValueError, match="table"):
        s2.submit(2 * PAGE, 1)
    with pytest.raises(ValueError, match="capacity"):
        _sched(capacity=100)[0].submit(60, 41)
    with pytest.raises(ValueError, match="parking"):
        _sched(n_pages=3, max_pages=8)[0].submit(2 * PAGE, 1)
    with pytest.raises(ValueError):
        Scheduler(PageTable(PageAllocator(1), 1, 1), 10).alloc.take(1)   # the parking page took the only one


def test_pages_return_to_the_pool_after_run_except_the_parking_page():
    eng = Replay(max_batch=3, n_pages=6, max_pages=3, capacity=768, sync_every=4)
    alloc = eng.sched.alloc
    assert alloc.pages_in_use == 1 and alloc.refs[eng.sched.park] == 1
    reqs = [(24, 40, 40), (300, 300, 17), (9, 500, 500), (1, 3, 1), (256, 1, 1), (17, 250, 250), (100, 600, 30)]
    ids = [eng.submit(*r) for r in reqs]
    done = eng.run()
    assert sorted(done) == ids == sorted(eng.finished_order)
    assert alloc.pages_in_use == 1 and alloc.free_pages == 5 and all(not r for r in eng.sched.table.rows)
    assert sorted(eng.sched.free_rows) == [0, 1, 2] and not eng.sched.live and not eng.sched.waiting
    assert eng.stats["prefills"] == len(reqs) and 1 < eng.stats["peak_pages"] <= 6
    eng.sched.close()
    assert alloc.pages_in_use == 0


def _by_hand(reqs, B, sync_every):
    """The loop written out again, without pages: (decode steps, iterations)."""
    waiting, live, it, steps = list(range(len(reqs))), {}, 0, 0
    while waiting or live:
        for row in range(B):
            if row not in live and waiting:
                live[row] = [waiting.pop(0), 0]
        it += 1
        gone = []
        for row, st in live.items():
            st[1] += 1
            T, budget, realised = reqs[st[0]]
            if st[1] >= budget or (it % sync_every == 0 and st[1] >= realised):
                gone.append(row)
        for row in gone:
            del live[row]
        steps += bool(live)
    return steps, it


@pytest.mark.parametrize("sync_every", [1, 3, 16])
def test_replay_counts_the_steps_of_the_schedule(sync_every):
    reqs = [(5, 40, 40), (5, 12, 3), (5, 64, 20), (5, 9, 9), (5, 33, 33), (5, 33, 1), (5, 2, 2)]
    eng = Replay(max_batch=2, n_pages=16, max_pages=2, capacity=512, sync_every=sync_every)
    for r in reqs:
        eng.submit(*r)
    eng.run()
    assert (eng.stats["decode_steps"], eng.stats["iterations"]) == _by_hand(reqs, 2, sync_every)
    # with every length at its budget and sync_every = 1 a row is never stepped past its end
    full = Replay(max_batch=2, n_pages=16, max_pages=2, capacity=512, sync_every=1)
    budgets = [40, 12, 64, 9]
    for n in budgets:
        full.submit(5, n, n)
    full.run()
    assert full.stats["iterations"] <= static_steps(budgets, 2) and full.stats["iterations"] >= -(-sum(budgets) // 2)


def test_static_steps_of_the_bench_workload():
    budgets = [(32, 64, 128, 512)[i % 4] for i in range(64)]
    assert static_steps(budgets, 8) == 8 * 512 and sum(budgets) == 11776


def _generate_script():
    spec = importlib.util.spec_from_file_location("generate_script", os.path.join(ROOT, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_continuous_needs_a_page_pool(capsys):
    g = _generate_script()
    with pytest.raises(SystemExit) as e:
        g.parse_args(["ckpt", "prompts.jsonl", "--continuous"])
    assert e.value.code == 2 and "--kv_pool_pages" in capsys.readouterr().err
    a = g.parse_args(["ckpt", "prompts.jsonl", "--continuous", "--kv_pool_pages", "64", "--batch_size", "4"])
    assert a.continuous and a.batch_size == 4


def test_generate_script_defaults_are_unchanged():
    a = _generate_script().parse_args(["ckpt", "prompts.jsonl"])
    assert not a.continuous
    assert (a.batch_size, a.temperature, a.repetition_penalty, a.top_k, a.top_p, a.min_tokens, a.max_tokens) == \
        (8, 0.6, 1.25, 100, 0.9, 8, 3000)
    assert (a.stop_token_id, a.pad_token_id, a.no_ras, a.win_size, a.tau_r, a.greedy, a.seed, a.sync_every) == \
        (151675, None, False, 25, 0.2, False, None, 16)
    assert (a.decode_kernels, a.kv_pool_pages, a.kv_cache_dtype, a.weight_dtype, a.output) == \
        ("tile", 0, "bf16", "bf16", "generated.jsonl")
