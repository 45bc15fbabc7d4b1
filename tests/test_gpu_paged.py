"""-m gpu: the paged KV cache -- the five paged cache kernels, the three paged runner entries, and paged sessions with a
shared pool, trim and fork (sd_decode.hip, sd_attn.hip, sd_model.hip, paged.py, generation.py).

The yardstick is always the contiguous twin fed the same rows, and every comparison is ``torch.equal``: a page is one
decode partition and four extend tiles, so the paged kernels walk the same keys in the same order.  Each
paged kernel case is built from the contiguous one: a pool with more pages than needed, a random permutation table that
interleaves the rows' pages, table entries beyond each row's reach set to -1 and to n_pages, every unowned page filled
with the 0x7FC1 sentinel of tests/test_gpu_session.py, the owned pages filled from the contiguous planes."""
import pytest
import torch

from gpu_util import dev
from test_gpu_generate import SHAPES, _mask, _model

pytestmark = pytest.mark.gpu

D, PAGE, SENT = 128, 256, 0x7FC1
N_POOL = 16
PROMPT_LENS = [250, 256, 3, 130]
TURN2_LENS = [12, 7, 1, 3]


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


def i16(t):
    return t.contiguous().view(torch.int16)


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=dev())


def rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16().to(dev())


def pages_for(n):
    return (n + PAGE - 1) // PAGE


class Paged:
    """Pool planes + table built from contiguous planes kc, vc [B, max_pages * 256, KD]; row b owns ``owned[b]`` pages."""

    def __init__(self, kc, vc, owned, seed=0):
        B, cap, KD = kc.shape
        self.B, self.max_pages, self.owned = B, cap // PAGE, list(owned)
        perm = torch.randperm(N_POOL, generator=torch.Generator().manual_seed(seed)).tolist()
        self.pages = [[] for _ in range(B)]
        for i in range(self.max_pages):        # page i of every row before page i + 1 of any: the rows interleave
            for b in range(B):
                if i < owned[b]:
                    self.pages[b].append(perm.pop())
        table = [[(-1, N_POOL)[(b + i) % 2] for i in range(self.max_pages)] for b in range(B)]
        for b in range(B):
            table[b][:owned[b]] = self.pages[b]
        self.table = i32(table)
        self.k = torch.full((N_POOL, PAGE, KD), 0, dtype=torch.int16, device=dev()).fill_(SENT).view(torch.bfloat16)
        self.v = self.k.clone()
        self.fill(kc, vc)
        self.unowned = torch.tensor(sorted(perm), dtype=torch.int64, device=dev())
        assert len(perm) > 0

    def fill(self, kc, vc):
        for b in range(self.B):
            for i, p in enumerate(self.pages[b]):
                self.k[p] = kc[b, i * PAGE:(i + 1) * PAGE]
                self.v[p] = vc[b, i * PAGE:(i + 1) * PAGE]

    def gather(self, b):
        idx = torch.tensor(self.pages[b], dtype=torch.int64, device=dev())
        return self.k[idx].flatten(0, 1), self.v[idx].flatten(0, 1)

    def check_sentinel(self):
        for pool in (self.k, self.v):
            assert bool((i16(pool[self.unowned]) == SENT).all())

    def check_rows_equal(self, kc, vc):
        """every owned page, whole, holds the bits of the contiguous planes"""
        for b in range(self.B):
            k, v = self.gather(b)
            n = self.owned[b] * PAGE
            assert torch.equal(i16(k), i16(kc[b, :n])) and torch.equal(i16(v), i16(vc[b, :n])), b


# ------------------------------------------------------------------------------------------------------ 1. decode
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("lens", [[1, 255, 256], [257, 512, 513], [700, 0, 300]])
def test_decode_attention_bits(ops, lens, G):
    Hkv, B, cap = 2, 3, 4 * PAGE
    Hq = Hkv * G
    q = rnd(B, Hq * D, seed=1)
    kc, vc = rnd(B, cap, Hkv * D, seed=2), rnd(B, cap, Hkv * D, seed=3)
    lens_d = i32(lens)
    pg = Paged(kc, vc, [pages_for(n) for n in lens], seed=sum(lens) + G)
    want_o, want_lse = ops.attn_decode(q, kc, vc, lens_d, Hq, Hkv, max_len=max(lens), want_lse=True)
    for hint in (max(lens), max(lens) + 200, cap, cap + 999):
        o, lse = ops.attn_decode_paged(q, pg.k, pg.v, pg.table, lens_d, Hq, Hkv, max_len=hint, want_lse=True)
        assert torch.equal(i16(o), i16(want_o)), hint
        assert torch.equal(lse, want_lse), hint
    pg.check_sentinel()
    pg.check_rows_equal(kc, vc)


# ------------------------------------------------------------------------------------------------------ 2. append
def test_append_bits_and_out_of_range_rows(ops):
    Hq, Hkv, cap = 4, 2, 2 * PAGE
    pos = [0, 255, 256, 511, -1, cap]
    owned = [1, 1, 2, 2, 2, 1]
    B = len(pos)
    qkv = rnd(B, (Hq + 2 * Hkv) * D, seed=4)
    qg, kg = rnd(D, seed=5), rnd(D, seed=6)
    cos, sin = ops.rope_tables(cap, dev())
    kc, vc = rnd(B, cap, Hkv * D, seed=7), rnd(B, cap, Hkv * D, seed=8)
    pg = Paged(kc, vc, owned, seed=11)
    before_k, before_v = pg.k.clone(), pg.v.clone()
    pos_d = i32(pos)
    want_q = ops.qknorm_rope_append(qkv, qg, kg, cos, sin, pos_d, kc, vc, Hq, Hkv)
    got_q = ops.qknorm_rope_append_paged(qkv, qg, kg, cos, sin, pos_d, pg.k, pg.v, pg.table, Hq, Hkv)
    assert torch.equal(i16(got_q), i16(want_q))
    pg.check_rows_equal(kc, vc)
    pg.check_sentinel()
    # exactly the rows' slots changed: rows 4 (pos -1) and 5 (pos cap) changed no byte of the pool
    changed_k, changed_v = (i16(pg.k) != i16(before_k)).any(-1), (i16(pg.v) != i16(before_v)).any(-1)   # [pages, 256]
    expect = torch.zeros(N_POOL, PAGE, dtype=torch.bool, device=dev())
    for b in range(4):
        expect[pg.pages[b][pos[b] // PAGE], pos[b] % PAGE] = True
    assert torch.equal(changed_k, expect) and torch.equal(changed_v, expect)


# ------------------------------------------------------------------------------------------- 3. store and store_at
def _blank(B, cap, KD):
    return torch.empty(B, cap, KD, dtype=torch.int16, device=dev()).fill_(SENT).view(torch.bfloat16)


def test_store_bits_and_nothing_else_is_written(ops):
    Hq, Hkv, T, cap = 4, 2, 300, 2 * PAGE
    kv_len = [300, 256, 1, 0]
    B = len(kv_len)
    qk, qkv = rnd(B * T, (Hq + Hkv) * D, seed=12), rnd(B * T, (Hq + 2 * Hkv) * D, seed=13)
    kc, vc = _blank(B, cap, Hkv * D), _blank(B, cap, Hkv * D)
    pg = Paged(kc, vc, [pages_for(n) for n in kv_len], seed=14)
    ops.kvcache_store(qk, qkv, kc, vc, i32(kv_len), B, T, Hq, Hkv)
    ops.kvcache_store_paged(qk, qkv, pg.k, pg.v, pg.table, i32(kv_len), B, T, Hq, Hkv)
    assert not bool((i16(kc[0, :300]) == SENT).any())
    pg.check_rows_equal(kc, vc)      # whole owned pages: the slots >= kv_len still hold the sentinel on both sides
    pg.check_sentinel()


def test_store_at_bits_and_nothing_else_is_written(ops):
    Hq, Hkv, T, cap = 4, 2, 32, 2 * PAGE
    past, new = [250, 256, 0, 500], [20, 1, 32, 0]
    B = len(past)
    qk, qkv = rnd(B * T, (Hq + Hkv) * D, seed=15), rnd(B * T, (Hq + 2 * Hkv) * D, seed=16)
    kc, vc = _blank(B, cap, Hkv * D), _blank(B, cap, Hkv * D)
    pg = Paged(kc, vc, [pages_for(p + n) for p, n in zip(past, new)], seed=17)
    ops.kvcache_store_at(qk, qkv, kc, vc, i32(past), i32(new), B, T, Hq, Hkv)
    ops.kvcache_store_at_paged(qk, qkv, pg.k, pg.v, pg.table, i32(past), i32(new), B, T, Hq, Hkv)
    assert not bool((i16(kc[0, 250:270]) == SENT).any())
    pg.check_rows_equal(kc, vc)
    pg.check_sentinel()


# ------------------------------------------------------------------------------------------------------ 4. extend
EXTEND_ROWS = [[(0, 130), (37, 130), (200, 130)], [(256, 66), (300, 1), (511, 2)], [(0, 0), (37, 130), (511, 2)]]


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("rows", EXTEND_ROWS)
def test_extend_attention_bits_and_no_leak(ops, rows, G):
    Hkv, B, T, cap = 2, 3, 130, 4 * PAGE
    Hq = Hkv * G
    past, new = [p for p, _ in rows], [n for _, n in rows]
    ends = [p + n for p, n in rows]
    q = rnd(B * T, Hq * D, seed=18)
    kc, vc = rnd(B, cap, Hkv * D, seed=19), rnd(B, cap, Hkv * D, seed=20)
    pg = Paged(kc, vc, [pages_for(e) for e in ends], seed=sum(ends) + G)
    want_o, want_lse = ops.attn_extend(q, kc, vc, i32(past), i32(new), T, Hq, Hkv)
    o, lse = ops.attn_extend_paged(q, pg.k, pg.v, pg.table, i32(past), i32(new), T, Hq, Hkv)
    assert torch.equal(i16(o), i16(want_o))
    assert torch.equal(lse, want_lse)
    pg.check_sentinel()
    pg.check_rows_equal(kc, vc)
    # +-1e4 in the owned slots >= past + new_len and in the query rows t >= new_len: no bit of a valid row moves
    junk = torch.where(torch.arange(Hkv * D) % 2 == 0, 1e4, -1e4).to(torch.bfloat16).to(dev())
    kj, vj, qj = kc.clone(), vc.clone(), q.clone().view(B, T, Hq * D)
    for b, e in enumerate(ends):
        kj[b, e:], vj[b, e:] = junk, -junk
        qj[b, new[b]:] = junk.repeat(G)
    pg.fill(kj, vj)
    o2, lse2 = ops.attn_extend_paged(qj.view(B * T, Hq * D), pg.k, pg.v, pg.table, i32(past), i32(new), T, Hq, Hkv)
    o, o2 = o.view(B, T, Hq * D), o2.view(B, T, Hq * D)
    for b, n in enumerate(new):
        assert torch.equal(i16(o2[b, :n]), i16(o[b, :n])), b
        assert torch.equal(lse2[b, :, :n], lse[b, :, :n]), b
    pg.check_sentinel()


# ------------------------------------------------------------------------------------------- 5. the runner: logits
def _pool(m, n_pages, seed=0):
    order = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    pool = m.kv_page_pool(n_pages, order=order)
    pool.buffer.view(torch.int16).fill_(SENT)
    return pool


def _prompt_ids(B=4, T=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 640, (B, T), generator=g), torch.randint(0, 640, (B, 64), generator=g)


@pytest.mark.parametrize("kernels", ["tile", "skinny"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_runner_logits_are_bit_identical(name, kernels):
    """prefill, 24 teacher-forced steps (row 0 crosses 256, row 1's first new token opens a fresh page), an extend of
    [12, 7, 1, 3] new tokens, 8 more steps: every logits tensor equals the contiguous Decoder's."""
    from speech_distill_amd.generation import Decoder
    m, _, _ = _model(name)
    ids, cont = _prompt_ids()
    ids_d, cont_d = ids.to(dev()), cont.to(dev())
    B, cap = 4, 512
    lens = list(PROMPT_LENS)
    pool = _pool(m, 8)
    flat = Decoder(m, B, cap, kernels)
    paged = Decoder(m, B, cap, kernels, pool=pool)
    paged.reserve([n + 24 + t + 8 for n, t in zip(lens, TURN2_LENS)])
    assert [len(r) for r in paged.pages.rows] == [2, 2, 1, 1] and pool.pages_in_use == 6
    assert flat.planes(0)[0].shape[1] == cap

    def both(call):
        a, b = call(flat).clone(), call(paged)
        assert torch.equal(i16(a), i16(b))

    both(lambda d: d.prefill(ids_d, i32(lens)))
    for t in range(24):
        both(lambda d: d.step(cont_d[:, t].contiguous(), i32([n + t for n in lens]), max(lens) + t + 1))
    lens = [n + 24 for n in lens]
    blk = cont_d[:, 24:36].contiguous()
    both(lambda d: d.extend(blk, i32(lens), i32(TURN2_LENS)))
    lens = [n + t for n, t in zip(lens, TURN2_LENS)]
    for t in range(8):
        both(lambda d: d.step(cont_d[:, 40 + t].contiguous(), i32([n + t for n in lens]), max(lens) + t + 1))
    lens = [n + 8 for n in lens]
    for l in range(m.dims.num_hidden_layers):
        kf, vf = flat.planes(l)
        for b, n in enumerate(lens):
            k, v = paged.gather(l, b, n)
            assert torch.equal(i16(k), i16(kf[b, :n])) and torch.equal(i16(v), i16(vf[b, :n])), (l, b)
    # the two pages nobody owns were never written
    free = torch.tensor(sorted(set(range(8)) - {p for r in paged.pages.rows for p in r}), device=dev())
    for l in range(m.dims.num_hidden_layers):
        for plane in pool.planes(l):
            assert bool((i16(plane[free]) == SENT).all())
    paged.close()
    assert pool.pages_in_use == 0


# ------------------------------------------------------------------------------------------------------ 6. sessions
def _turn_args(i, eos=None):
    from speech_distill_amd.generation import REFERENCE_SAMPLING
    if i == 1:
        return dict(do_sample=False)
    return dict(REFERENCE_SAMPLING, seed=100 + i, eos_token_id=eos if i == 2 else None)


def _three_turns(sess, ids, cont, new_tokens, eos=None, hook=None):
    """turn 0: the ragged prompts, sampled; turn 1: [12, 7, 1, 3] given tokens, greedy; turn 2: one given token, sampled,
    with an EOS.  -> the three token tensors and the lengths after each turn."""
    given = [(ids, _mask(PROMPT_LENS, ids.shape[1])), (cont[:, :12], _mask(TURN2_LENS, 12)), (cont[:, 12:13], None)]
    out = []
    for i, (x, am) in enumerate(given):
        before = sess.lengths().tolist()
        new = sess.generate(x.to(dev()), None if am is None else am.to(dev()), max_new_tokens=new_tokens,
                            **_turn_args(i, eos))
        if hook:
            hook(i, before, [int(v) for v in (am.sum(-1) if am is not None else [x.shape[1]] * x.shape[0])])
        out.append((new.cpu(), sess.lengths().tolist()))
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_paged_session_equals_the_contiguous_session(name):
    m, _, _ = _model(name)
    ids, cont = _prompt_ids()
    NEW, cap = 16, 512
    probe = _three_turns(m.start_session(4, capacity=cap), ids, cont, NEW)
    eos = int(probe[2][0][0, 5])                      # occurs in row 0 of the third turn, at step 5 at the latest
    want = _three_turns(m.start_session(4, capacity=cap), ids, cont, NEW, eos)
    assert want[2][1][0] < probe[2][1][0]             # row 0 did stop early
    pool = _pool(m, 12)
    sess = m.start_session(4, capacity=cap, pool=pool)

    def admitted(i, before, n_in):
        assert pool.pages_in_use == sum(pages_for(a + b + NEW) for a, b in zip(before, n_in)), i

    got = _three_turns(sess, ids, cont, NEW, eos, hook=admitted)
    for i in range(3):
        assert torch.equal(got[i][0], want[i][0]) and got[i][1] == want[i][1], i
    sess.trim()
    assert pool.pages_in_use == sum(pages_for(n) for n in got[2][1])
    assert [len(r) for r in sess.decoder.pages.rows] == [pages_for(n) for n in got[2][1]]
    sess.reset()
    assert pool.pages_in_use == 0 and pool.free_pages == 12


def test_two_sessions_share_one_pool():
    m, _, _ = _model("student")
    ids, cont = _prompt_ids(B=3)
    NEW, cap = 12, 512
    lens = {2: [250, 3], 3: [256, 130, 255]}

    def turns(sess, B, other=None):
        out = []
        x = ids[:B]
        out.append(sess.generate(x.to(dev()), _mask(lens[B], 256).to(dev()), max_new_tokens=NEW, do_sample=False).cpu())
        if other:
            other(0)
        out.append(sess.generate(cont[:B, :5].to(dev()), max_new_tokens=NEW, do_sample=True, top_k=20, seed=7).cpu())
        if other:
            other(1)
        out.append(sess.generate(cont[:B, 5:6].to(dev()), max_new_tokens=NEW, do_sample=False).cpu())
        return out

    alone2 = turns(m.start_session(2, capacity=cap), 2)
    alone3 = turns(m.start_session(3, capacity=cap), 3)
    pool = _pool(m, 16, seed=3)
    s2, s3 = m.start_session(2, capacity=cap, pool=pool), m.start_session(3, capacity=cap, pool=pool)
    got3 = []

    def other(i):     # the B = 3 session's turns run between the B = 2 session's
        x, am = (ids[:3], _mask(lens[3], 256).to(dev())) if i == 0 else (cont[:3, :5], None)
        kw = dict(do_sample=False) if i == 0 else dict(do_sample=True, top_k=20, seed=7)
        got3.append(s3.generate(x.to(dev()), am, max_new_tokens=NEW, **kw).cpu())

    got2 = turns(s2, 2, other)
    owned2, owned3 = {p for r in s2.decoder.pages.rows for p in r}, {p for r in s3.decoder.pages.rows for p in r}
    assert owned2 and owned3 and not (owned2 & owned3)
    s2.reset()                                          # must leave the other session's next turn unchanged
    assert pool.pages_in_use == len(owned3)
    got3.append(s3.generate(cont[:3, 5:6].to(dev()), max_new_tokens=NEW, do_sample=False).cpu())
    for a, b in zip(got2 + got3, alone2 + alone3):
        assert torch.equal(a, b)
    del s2, s3
    assert pool.pages_in_use == 0                       # dropping a session releases its pages


def test_a_pool_one_page_short_raises_and_changes_nothing():
    m, _, _ = _model("student")
    ids, cont = _prompt_ids()
    NEW, cap = 16, 1024
    mask = _mask(PROMPT_LENS, 256).to(dev())
    control = m.start_session(4, capacity=cap)
    control.generate(ids.to(dev()), mask, max_new_tokens=NEW, do_sample=False)
    want = control.generate(cont[:, :4].to(dev()), max_new_tokens=NEW, do_sample=False).cpu()
    need = sum(pages_for(n + NEW) for n in PROMPT_LENS)             # 2 + 2 + 1 + 1
    pool = _pool(m, need)
    sess = m.start_session(4, capacity=cap, pool=pool)
    sess.generate(ids.to(dev()), mask, max_new_tokens=NEW, do_sample=False)
    lens, used = sess.lengths().tolist(), pool.pages_in_use
    assert used == need and pool.free_pages == 0
    rows = [list(r) for r in sess.decoder.pages.rows]
    # 4 given + 120 new tokens take the row of 146 tokens into a second page: one page more than the pool holds
    big = 120
    assert sum(pages_for(n + 4 + big) for n in lens) == need + 1
    assert sum(pages_for(n + 4 + NEW) for n in lens) == need
    with pytest.raises(ValueError):
        sess.generate(cont[:, :4].to(dev()), max_new_tokens=big, do_sample=False)
    assert pool.pages_in_use == used and sess.lengths().tolist() == lens
    assert [list(r) for r in sess.decoder.pages.rows] == rows
    got = sess.generate(cont[:, :4].to(dev()), max_new_tokens=NEW, do_sample=False).cpu()
    assert torch.equal(got, want)


def test_fork_shares_full_pages_and_copies_the_partial_one():
    m, _, _ = _model("student")
    ids, cont = _prompt_ids(B=1, T=320)
    L = m.dims.num_hidden_layers
    with pytest.raises(ValueError):
        m.start_session(1, capacity=512).fork([0])
    pool = _pool(m, 12, seed=5)
    src = m.start_session(1, capacity=512, decode_kernels="skinny", pool=pool)
    src.extend(ids[:, :300].to(dev()))
    snap = [src.decoder.gather(l, 0, 300) for l in range(L)]
    assert pool.pages_in_use == 2
    f = src.fork([0, 0, 0])
    assert f.B == 3 and f.lengths().tolist() == [300] * 3 and pool.pages_in_use == 5
    shared = src.decoder.pages.rows[0][0]
    ft, st = f.decoder.table.cpu(), src.decoder.table.cpu()
    assert ft[:, 0].tolist() == [shared] * 3 and int(st[0, 0]) == shared
    assert len({int(st[0, 1])} | set(ft[:, 1].tolist())) == 4      # the partial page: one private copy each
    assert pool.alloc.refs[shared] == 4
    tok = ids[:, 300:301].to(dev())
    g = f.generate(tok.expand(3, 1).contiguous(), max_new_tokens=8, do_sample=False).cpu()
    assert torch.equal(g[0], g[1]) and torch.equal(g[0], g[2])
    own = src.generate(tok, max_new_tokens=8, do_sample=False).cpu()
    assert torch.equal(own[0], g[0])
    s = f.generate(cont[:1, :1].expand(3, 1).contiguous().to(dev()), max_new_tokens=8, do_sample=True, seed=3).cpu()
    assert not (torch.equal(s[0], s[1]) and torch.equal(s[0], s[2]))     # the rows draw different uniforms
    for l in range(L):
        for sess, rows in ((f, 3), (src, 1)):
            for b in range(rows):
                k, v = sess.decoder.gather(l, b, 300)
                assert torch.equal(i16(k), i16(snap[l][0])) and torch.equal(i16(v), i16(snap[l][1])), (l, b)
    for i in range(3):           # the forks go one by one: the shared page stays while anybody holds it
        f.reset([i])
        assert pool.alloc.refs[shared] == 3 - i
    assert pool.pages_in_use == len(src.decoder.pages.rows[0])
    src.reset()
    assert pool.alloc.refs[shared] == 0 and pool.pages_in_use == 0
