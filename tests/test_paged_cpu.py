"""No GPU: the host bookkeeping of the paged KV cache (speech_distill_amd/paged.py: PageAllocator, PageTable) and the
refusal codes of every paged C entry, which are decided before any launch (the pattern of tests/test_gemv_cpu.py)."""
import ctypes

import pytest

from speech_distill_amd.paged import PAGE, PageAllocator, PageTable, fork_split, pages_for

SHAPE, ALIGN, UNSUPPORTED, WORKSPACE = -1, -2, -3, -5
P = 0x1000   # a 16-byte aligned address that is never dereferenced: every call below returns before a launch


# ------------------------------------------------------------------------------------------------- host bookkeeping
def test_order_is_honoured_and_default_is_ascending():
    a = PageAllocator(5, order=[3, 0, 4, 1, 2])
    assert a.take(2) == [3, 0] and a.take(3) == [4, 1, 2]
    assert PageAllocator(3).take(3) == [0, 1, 2]
    for bad in ([0, 1], [0, 1, 1], [0, 1, 3]):
        with pytest.raises(ValueError):
            PageAllocator(3, order=bad)
    with pytest.raises(ValueError):
        PageAllocator(0)


def test_exhaustion_raises_and_leaves_the_counts_unchanged():
    a = PageAllocator(4)
    got = a.take(3)
    before = (a.free_pages, a.pages_in_use, list(a.refs))
    with pytest.raises(ValueError):
        a.take(2)
    assert (a.free_pages, a.pages_in_use, list(a.refs)) == before == (1, 3, [1, 1, 1, 0])
    a.release(got[:2])
    assert a.free_pages == 3 and a.pages_in_use == 1
    assert sorted(a.take(3)) == [0, 1, 3]


def test_a_shared_page_is_freed_only_at_count_zero():
    a = PageAllocator(2)
    (p,) = a.take(1)
    a.share([p]), a.share([p])
    assert a.refs[p] == 3
    a.release([p]), a.release([p])
    assert a.pages_in_use == 1 and a.refs[p] == 1
    a.release([p])
    assert a.pages_in_use == 0 and a.refs[p] == 0
    with pytest.raises(ValueError):
        a.release([p])
    with pytest.raises(ValueError):
        a.share([p])


def test_admission_trims_then_takes_and_is_all_or_nothing():
    a = PageAllocator(8, order=[7, 6, 5, 4, 3, 2, 1, 0])
    t = PageTable(a, 2, max_pages=4)
    t.admit([0, 0], [300, 1])                       # ceil(300/256) + ceil(1/256)
    assert t.rows == [[7, 6], [5]] and a.pages_in_use == 3 and t.dirty == {0, 1}
    t.dirty.clear()
    # the turn ended at lengths 200 and 1: row 0's second page is a leftover; the next turn wants 700 and 257 positions
    t.admit([200, 1], [700, 257])
    assert [len(r) for r in t.rows] == [3, 2] and a.pages_in_use == 5 and t.rows[0][0] == 7 and t.rows[1][0] == 5
    assert t.dirty == {0, 1}
    assert t.entries(1) == t.rows[1] + [-1, -1]
    # beyond the table's reach: refused before anything changes
    rows, used = [list(r) for r in t.rows], a.pages_in_use
    with pytest.raises(ValueError):
        t.admit([200, 1], [1025, 1])
    assert [list(r) for r in t.rows] == rows and a.pages_in_use == used


def test_admission_one_page_short_changes_nothing():
    a = PageAllocator(4)
    t = PageTable(a, 2, max_pages=4)
    t.admit([0, 0], [512, 256])                      # 3 pages, 1 free
    rows, used, refs = [list(r) for r in t.rows], a.pages_in_use, list(a.refs)
    t.dirty.clear()
    with pytest.raises(ValueError):
        t.admit([100, 256], [100 + 512, 256 + 256])  # keeps 1 + 1, wants 3 + 2 = 3 more; 1 free + 1 given back
    assert [list(r) for r in t.rows] == rows and a.pages_in_use == used and list(a.refs) == refs and not t.dirty
    t.admit([100, 256], [100 + 256, 256 + 256])      # 2 more: exactly what is free after the give-back
    assert a.free_pages == 0 and [len(r) for r in t.rows] == [2, 2]


def test_trim_reserve_and_release():
    a = PageAllocator(6)
    t = PageTable(a, 2, max_pages=3)
    t.reserve([600, 10])
    assert [len(r) for r in t.rows] == [3, 1]
    t.reserve([1, 300])                               # never gives back
    assert [len(r) for r in t.rows] == [3, 2] and a.pages_in_use == 5
    with pytest.raises(ValueError):
        t.reserve([1, 769])
    t.trim([257, 0])
    assert [len(r) for r in t.rows] == [2, 0] and a.pages_in_use == 2
    t.release([0])
    assert a.pages_in_use == 0 and t.rows == [[], []]


@pytest.mark.parametrize("cached,shared,copied", [(0, 0, 0), (255, 0, 1), (256, 1, 0), (257, 1, 1), (512, 2, 0)])
def test_the_partial_page_rule(cached, shared, copied):
    assert fork_split(cached) == (shared, copied)
    a = PageAllocator(16)
    t = PageTable(a, 1, max_pages=4)
    t.reserve([max(cached, 1) + 40])
    owned, used = list(t.rows[0]), a.pages_in_use
    f, copies = t.fork([0, 0, 0], [cached])
    assert a.pages_in_use == used + 3 * copied and len(copies) == 3 * copied
    for i in range(3):
        assert f.rows[i][:shared] == owned[:shared] and len(f.rows[i]) == shared + copied
    for src, dst in copies:
        assert src == owned[shared] and dst not in owned
    assert len({d for _, d in copies}) == len(copies)
    assert [a.refs[p] for p in owned[:shared]] == [4] * shared and all(a.refs[p] == 1 for p in owned[shared:])
    # the forks go one by one, then the source: a shared page is free only after its last holder
    for i in range(3):
        f.release([i])
        assert all(a.refs[p] == 3 - i for p in owned[:shared])
    assert a.pages_in_use == used
    t.release()
    assert a.pages_in_use == 0


def test_fork_without_room_for_the_copies_changes_nothing():
    a = PageAllocator(3)
    t = PageTable(a, 1, max_pages=2)
    t.reserve([300])
    refs = list(a.refs)
    with pytest.raises(ValueError):
        t.fork([0, 0], [300])                         # two copies of the partial page, one page free
    assert list(a.refs) == refs and a.pages_in_use == 2
    assert pages_for(0) == 0 and pages_for(1) == 1 and pages_for(PAGE) == 1 and pages_for(PAGE + 1) == 2


# ------------------------------------------------------------------------------------- refusal codes, before any launch
@pytest.fixture(scope="module")
def lib():
    import speech_distill_amd as sda
    return sda.load_lib()


def test_paged_kernel_entries_refuse_before_any_launch(lib):
    def store(table=P, max_pages=2, n_pages=4, B=2, T=8, pool=P):
        return lib.sd_kvcache_store_paged(P, P, pool, P, table, max_pages, n_pages, None, B, T, 4, 2, None)

    def store_at(table=P, max_pages=2, n_pages=4, B=2, T=8, pool=P):
        return lib.sd_kvcache_store_at_paged(P, P, pool, P, table, max_pages, n_pages, P, P, B, T, 4, 2, None)

    def append(table=P, max_pages=2, n_pages=4, B=2, pool=P):
        return lib.sd_qknorm_rope_append_paged(P, P, P, P, P, P, P, pool, P, table, max_pages, n_pages, B, 4, 2, 1e-6, None)

    def decode(table=P, max_pages=2, n_pages=4, B=2, pool=P, Hq=4, Hkv=2, hd=128, ws=1 << 40):
        return lib.sd_attn_decode_paged(P, pool, P, table, max_pages, n_pages, P, None, P, 0, P, ws, B, 8, Hq, Hkv, hd,
                                        0.1, None)

    def extend(table=P, max_pages=2, n_pages=4, B=2, T=8, pool=P, Hq=4, Hkv=2, hd=128):
        return lib.sd_attn_extend_paged(P, pool, P, table, max_pages, n_pages, P, None, P, P, Hq * 128, Hq * 128, B, T, Hq,
                                        Hkv, hd, 0.1, None)

    for f in (store, store_at, append, decode, extend):
        assert f(table=None) == SHAPE, f.__name__
        assert f(pool=None) == SHAPE, f.__name__
        assert f(max_pages=0) == SHAPE and f(max_pages=-1) == SHAPE, f.__name__
        assert f(n_pages=0) == SHAPE and f(n_pages=-3) == SHAPE, f.__name__
        assert f(B=0) == SHAPE, f.__name__
    for f in (store, store_at, extend):
        assert f(T=0) == SHAPE and f(T=-1) == SHAPE, f.__name__
    assert store(T=513) == SHAPE                      # T > cap = 2 pages, as the twin's T > cap
    for f in (decode, extend):
        assert f(hd=64) == UNSUPPORTED, f.__name__
        assert f(Hq=6, Hkv=2) == UNSUPPORTED and f(Hq=16, Hkv=2) == UNSUPPORTED, f.__name__
        assert f(Hq=5, Hkv=2) == SHAPE, f.__name__
    assert decode(ws=0) == WORKSPACE
    assert lib.sd_kvpool_bytes(None, 4) == UNSUPPORTED


def test_paged_runner_entries_refuse_before_any_launch(lib):
    from speech_distill_amd import _lib
    dims = _lib.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)
    d, p = ctypes.byref(dims), ctypes.byref(_lib.Params())
    per_page = 2 * 2 * 256 * 2 * 128 * 2              # L * 2 * 256 * Hkv * 128 * 2 bytes
    assert lib.sd_kvpool_bytes(d, 3) == 3 * per_page
    assert lib.sd_kvpool_bytes(d, 0) == SHAPE

    def kv(pool=P, pool_bytes=1 << 40, table=P, n_pages=4, max_pages=2):
        return ctypes.byref(_lib.KvPages(pool, pool_bytes, table, n_pages, max_pages))

    def prefill(kvp, dd=d, B=2, T=8, acts_bytes=1 << 40):
        return lib.sd_qwen3_prefill_paged(dd, p, P, P, P, P, P, acts_bytes, kvp, P, B, T, None)

    def extend(kvp, dd=d, B=2, T=8, acts_bytes=1 << 40):
        return lib.sd_qwen3_extend_paged(dd, p, P, P, P, P, P, P, acts_bytes, kvp, P, B, T, None)

    def step(kvp, dd=d, B=2, T=8, acts_bytes=1 << 40, flags=0):
        return lib.sd_qwen3_decode_step_paged(dd, p, P, P, 8, P, P, kvp, P, acts_bytes, P, B, flags, None)

    hd64 = ctypes.byref(_lib.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    g3 = ctypes.byref(_lib.Dims(640, 256, 512, 2, 6, 2, 128, 1, 1e-6, 0))
    for f in (prefill, extend, step):
        assert f(None) == SHAPE, f.__name__
        assert f(kv(pool=None)) == SHAPE and f(kv(table=None)) == SHAPE, f.__name__
        assert f(kv(n_pages=0)) == SHAPE and f(kv(max_pages=0)) == SHAPE and f(kv(max_pages=-2)) == SHAPE, f.__name__
        assert f(kv(pool_bytes=4 * per_page - 1)) == WORKSPACE, f.__name__
        assert f(kv(), B=0) == SHAPE, f.__name__
        assert f(kv(), dd=hd64) == UNSUPPORTED, f.__name__
        assert f(kv(pool_bytes=4 * per_page), acts_bytes=0) == WORKSPACE, f.__name__   # as far as the workspace check
    for f in (prefill, extend):
        assert f(kv(), T=0) == SHAPE and f(kv(), T=513) == SHAPE, f.__name__     # T <= cap = max_pages * 256
    for f in (extend, step):
        assert f(kv(), dd=g3) == UNSUPPORTED, f.__name__
    assert step(kv(), flags=2) == SHAPE and step(kv(), flags=0x100) == SHAPE and step(kv(), flags=3) == SHAPE
    assert step(kv(), flags=1, acts_bytes=0) == WORKSPACE
    assert lib.sd_qwen3_decode_step_paged_acts_bytes(d, 2, 0) == SHAPE
    assert lib.sd_qwen3_decode_step_paged_acts_bytes(d, 2, 2) == lib.sd_qwen3_decode_acts_bytes(d, 2, 512)
    assert lib.sd_qwen3_prefill_paged_acts_bytes(d, 2, 8) == lib.sd_qwen3_prefill_acts_bytes(d, 2, 8)
    assert lib.sd_qwen3_extend_paged_acts_bytes(d, 2, 8) == lib.sd_qwen3_extend_acts_bytes(d, 2, 8)
