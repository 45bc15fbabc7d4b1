"""-m gpu: 8-bit (MXFP8) pages of the paged KV cache -- the three quantising stores, the two attention kernels, the three
runner entries and sessions over an mxfp8 pool (sd_decode.hip, sd_attn.hip, sd_model.hip, paged.py, generation.py).

Yardsticks.  Stores: ``mx_ref.mx_quant`` of the rows the bf16 paged twin writes with the same inputs, byte for byte.
Attention: the bf16 paged twin run on a pool that holds ``mx_deq(...).bfloat16()`` of the same bytes, ``torch.equal`` --
every finite e4m3 code times 2^e is a bf16 number (tests/test_paged_mx_cpu.py), so the two kernels see the same values
and do the same arithmetic.  Runner: exact where a layer depends on the embeddings only (layer 0), loose and said so
against tests/kvq_ref.py for the logits.  Pools are pre-filled with the 0x7FC1 pattern, tables are shuffled, and the
entries a row does not reach are -1 / n_pages, as in tests/test_gpu_paged.py, whose helpers this file reuses."""
import pytest
import torch

import attn_ref as A
import gen_ref as R
import kvq_ref
import mx_ref
from gpu_util import dev, record, rel_err
from test_gpu_generate import SHAPES, _mask, _model
from test_gpu_paged import D, EXTEND_ROWS, N_POOL, PAGE, SENT, Paged, _blank, i16, i32, pages_for, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


def u8(t):
    return t.contiguous().view(torch.uint8)


def quant(x):
    """bf16 rows [..., Hkv*128] (any device) -> (e4m3 bytes uint8 [..., Hkv*128], E8M0 bytes uint8 [..., Hkv*4]), CPU."""
    q, s = mx_ref.mx_quant(x.cpu())
    return u8(q), s


def deq(q, s):
    """-> the bf16 rows a bf16 pool must hold for the twin to see the same values"""
    return mx_ref.mx_deq(q, s).bfloat16()


def pattern(*shape):
    """uint8 [*shape] on the device holding the 0x7FC1 pattern (last dimension even)"""
    return torch.empty(*shape, dtype=torch.uint8, device=dev()).view(torch.int16).fill_(SENT).view(torch.uint8)


class PagedMx:
    """The 8-bit planes over the SAME table and page assignment as a ``Paged`` (tests/test_gpu_paged.py)."""

    def __init__(self, pg, KD):
        self.pg = pg
        self.kd, self.vd = pattern(N_POOL, PAGE, KD), pattern(N_POOL, PAGE, KD)
        self.ks, self.vs = pattern(N_POOL, PAGE, KD // 32), pattern(N_POOL, PAGE, KD // 32)

    @property
    def planes(self):
        return self.kd, self.ks, self.vd, self.vs

    def fill(self, kc, vc):
        """owned pages <- the quantised rows of contiguous planes kc, vc [B, max_pages * 256, KD]; -> what the bf16 pool
        must hold beside them (the dequantised rows, [B, cap, KD] bf16 on the device)"""
        (kq, ks), (vq, vs) = quant(kc), quant(vc)
        for b in range(self.pg.B):
            for i, p in enumerate(self.pg.pages[b]):
                sl = slice(i * PAGE, (i + 1) * PAGE)
                self.kd[p], self.ks[p], self.vd[p], self.vs[p] = (t[b, sl].to(dev()) for t in (kq, ks, vq, vs))
        return deq(kq, ks).to(dev()), deq(vq, vs).to(dev())

    def check_sentinel(self):
        for plane in self.planes:
            assert bool((plane[self.pg.unowned].view(torch.int16) == SENT).all())


def both_pools(kc, vc, owned, seed):
    """-> (bf16 ``Paged`` holding the dequantised rows, ``PagedMx`` holding the bytes), one table"""
    pg = Paged(kc, vc, owned, seed=seed)
    mx = PagedMx(pg, kc.shape[-1])
    pg.fill(*mx.fill(kc, vc))
    return pg, mx


JUNK = torch.where(torch.arange(2 * D) % 2 == 0, 1e4, -1e4).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------ 1. decode
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("lens", [[1, 255, 256], [257, 512, 513], [700, 0, 300]])
def test_decode_attention_bits(ops, lens, G):
    Hkv, B, cap = 2, 3, 4 * PAGE
    Hq = Hkv * G
    q = rnd(B, Hq * D, seed=1)
    kc, vc = rnd(B, cap, Hkv * D, seed=2), rnd(B, cap, Hkv * D, seed=3)
    lens_d = i32(lens)
    pg, mx = both_pools(kc, vc, [pages_for(n) for n in lens], seed=sum(lens) + G)
    want_o, want_lse = ops.attn_decode_paged(q, pg.k, pg.v, pg.table, lens_d, Hq, Hkv, max_len=max(lens), want_lse=True)
    for hint in (max(lens), max(lens) + 200, cap, cap + 999):
        o, lse = ops.attn_decode_paged_mx(q, mx.planes, pg.table, lens_d, Hq, Hkv, max_len=hint, want_lse=True)
        assert torch.equal(i16(o), i16(want_o)), hint
        assert torch.equal(lse, want_lse), hint
    mx.check_sentinel()
    # +-1e4 in every owned slot >= n: no bit moves
    kj, vj = kc.clone(), vc.clone()
    for b, n in enumerate(lens):
        kj[b, n:], vj[b, n:] = JUNK.to(dev()), -JUNK.to(dev())
    mx.fill(kj, vj)
    o, lse = ops.attn_decode_paged_mx(q, mx.planes, pg.table, lens_d, Hq, Hkv, max_len=cap, want_lse=True)
    assert torch.equal(i16(o), i16(want_o)) and torch.equal(lse, want_lse)


# ------------------------------------------------------------------------------------------------------ 2. extend
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("rows", EXTEND_ROWS + [[(250, 20), (0, 130), (506, 6)]])   # + a block across a page boundary
def test_extend_attention_bits_and_no_leak(ops, rows, G):
    Hkv, B, T, cap = 2, 3, 130, 4 * PAGE
    Hq = Hkv * G
    past, new = [p for p, _ in rows], [n for _, n in rows]
    ends = [p + n for p, n in rows]
    q = rnd(B * T, Hq * D, seed=18)
    kc, vc = rnd(B, cap, Hkv * D, seed=19), rnd(B, cap, Hkv * D, seed=20)
    pg, mx = both_pools(kc, vc, [pages_for(e) for e in ends], seed=sum(ends) + G)
    want_o, want_lse = ops.attn_extend_paged(q, pg.k, pg.v, pg.table, i32(past), i32(new), T, Hq, Hkv)
    o, lse = ops.attn_extend_paged_mx(q, mx.planes, pg.table, i32(past), i32(new), T, Hq, Hkv)
    assert torch.equal(i16(o), i16(want_o))
    assert torch.equal(lse, want_lse)
    mx.check_sentinel()
    # +-1e4 in the owned slots >= past + new_len and in the query rows t >= new_len: no bit of a valid row moves
    kj, vj, qj = kc.clone(), vc.clone(), q.clone().view(B, T, Hq * D)
    for b, e in enumerate(ends):
        kj[b, e:], vj[b, e:] = JUNK.to(dev()), -JUNK.to(dev())
        qj[b, new[b]:] = JUNK.to(dev()).repeat(G)
    mx.fill(kj, vj)
    o2, lse2 = ops.attn_extend_paged_mx(qj.view(B * T, Hq * D), mx.planes, pg.table, i32(past), i32(new), T, Hq, Hkv)
    o, o2 = o.view(B, T, Hq * D), o2.view(B, T, Hq * D)
    for b, n in enumerate(new):
        assert torch.equal(i16(o2[b, :n]), i16(o[b, :n])), b
        assert torch.equal(lse2[b, :, :n], lse[b, :, :n]), b
    mx.check_sentinel()


# ------------------------------------------------------------------------------------------------------ 3. stores
def with_special_blocks(x, col0):
    """Rows of x get, from column col0 on: an all-zero block, a block whose amax is an exact power of two, and a block with
    values in (448, 512) * 2^e, which must saturate to +-448 * 2^e (amax 496: e = 0)."""
    x = x.clone()
    x[:, col0:col0 + 32] = 0
    x[:, col0 + 32:col0 + 64] = (x[:, col0 + 32:col0 + 64].float().clamp(-1, 1)).bfloat16()
    x[:, col0 + 37] = 2.0
    x[:, col0 + 64] = 480.0
    x[:, col0 + 65] = -496.0
    return x


def check_planes_are_the_quantised_twin(pg, mx):
    """Every row the bf16 twin wrote holds mx_quant of it; every other byte of all four planes keeps its pattern."""
    for bf, data, scale in ((pg.k, mx.kd, mx.ks), (pg.v, mx.vd, mx.vs)):
        rows = bf.cpu()
        written = (i16(rows) != SENT).any(-1)                      # [pages, 256]
        q, s = quant(torch.where(written[..., None], rows, torch.zeros_like(rows)))
        pat_d, pat_s = pattern(*data.shape).cpu(), pattern(*scale.shape).cpu()
        assert torch.equal(data.cpu(), torch.where(written[..., None], q, pat_d))
        assert torch.equal(scale.cpu(), torch.where(written[..., None], s, pat_s))
    pg.check_sentinel()
    mx.check_sentinel()
    return int(written.sum())


def test_special_blocks_quantise_as_the_format_says():
    """the reference itself on the three named cases (CPU arithmetic; guards the yardstick of the store tests)"""
    x = with_special_blocks(torch.randn(2, 128, generator=torch.Generator().manual_seed(0)).bfloat16(), 0)
    q, s = mx_ref.mx_quant(x)
    v = mx_ref.mx_deq(q, s)
    assert bool((u8(q)[:, :32] == 0).all()) and bool((s[:, 0] == 0).all())           # zero block: byte 0, codes 0
    assert bool((s[:, 1] == 1 - 8 + 127).all()) and bool((v[:, 37] == 2.0).all())    # amax 2 = 2^1: e = -7, exact
    assert bool((s[:, 2] == 127).all()) and bool((v[:, 64] == 448.0).all()) and bool((v[:, 65] == -448.0).all())


def test_store_bits_and_nothing_else_is_written(ops):
    Hq, Hkv, T, cap = 4, 2, 300, 2 * PAGE
    kv_len = [300, 256, 1, 0, 40]
    B = len(kv_len)
    qk = with_special_blocks(rnd(B * T, (Hq + Hkv) * D, seed=12), Hq * D + 128)
    qkv = with_special_blocks(rnd(B * T, (Hq + 2 * Hkv) * D, seed=13), (Hq + Hkv) * D)
    kc, vc = _blank(B, cap, Hkv * D), _blank(B, cap, Hkv * D)
    owned = [pages_for(n) for n in kv_len]
    owned[4] = 0            # row 4 reaches entry 0, which lies outside the pool (-1 / n_pages): nothing is written
    pg = Paged(kc, vc, owned, seed=14)
    mx = PagedMx(pg, Hkv * D)
    ops.kvcache_store_paged(qk, qkv, pg.k, pg.v, pg.table, i32(kv_len), B, T, Hq, Hkv)
    ops.kvcache_store_paged_mx(qk, qkv, mx.planes, pg.table, i32(kv_len), B, T, Hq, Hkv)
    assert check_planes_are_the_quantised_twin(pg, mx) == 300 + 256 + 1


def test_store_at_bits_and_nothing_else_is_written(ops):
    Hq, Hkv, T, cap = 4, 2, 32, 2 * PAGE
    past, new = [250, 256, 0, 500, 10], [20, 1, 32, 0, 5]
    B = len(past)
    qk = with_special_blocks(rnd(B * T, (Hq + Hkv) * D, seed=15), Hq * D)
    qkv = with_special_blocks(rnd(B * T, (Hq + 2 * Hkv) * D, seed=16), (Hq + Hkv) * D + 128)
    kc, vc = _blank(B, cap, Hkv * D), _blank(B, cap, Hkv * D)
    owned = [pages_for(p + n) for p, n in zip(past, new)]
    owned[4] = 0            # an out-of-range entry that is read
    pg = Paged(kc, vc, owned, seed=17)
    mx = PagedMx(pg, Hkv * D)
    ops.kvcache_store_at_paged(qk, qkv, pg.k, pg.v, pg.table, i32(past), i32(new), B, T, Hq, Hkv)
    ops.kvcache_store_at_paged_mx(qk, qkv, mx.planes, pg.table, i32(past), i32(new), B, T, Hq, Hkv)
    assert check_planes_are_the_quantised_twin(pg, mx) == 20 + 1 + 32


def test_append_bits_and_the_three_stores_agree(ops):
    Hq, Hkv, cap = 4, 2, 2 * PAGE
    pos = [0, 255, 256, 511, -1, cap, 7]
    owned = [1, 1, 2, 2, 2, 1, 0]      # rows 4, 5: positions outside [0, cap); row 6: an out-of-range entry that is read
    B = len(pos)
    qkv = with_special_blocks(rnd(B, (Hq + 2 * Hkv) * D, seed=4), (Hq + Hkv) * D)
    qg, kg = rnd(D, seed=5), rnd(D, seed=6)
    cos, sin = ops.rope_tables(cap, dev())
    kc, vc = _blank(B, cap, Hkv * D), _blank(B, cap, Hkv * D)
    pg = Paged(kc, vc, owned, seed=11)
    mx = PagedMx(pg, Hkv * D)
    pos_d = i32(pos)
    want_q = ops.qknorm_rope_append_paged(qkv, qg, kg, cos, sin, pos_d, pg.k, pg.v, pg.table, Hq, Hkv)
    got_q = ops.qknorm_rope_append_paged_mx(qkv, qg, kg, cos, sin, pos_d, mx.planes, pg.table, Hq, Hkv)
    assert torch.equal(i16(got_q), i16(want_q))           # q_out is the twin's bf16
    assert check_planes_are_the_quantised_twin(pg, mx) == 4
    # identical input rows through the other two stores give identical bytes: the rows the append wrote (K normalised and
    # rotated by the twin, V raw), fed to store (slot = t) and to store_at (past 3), B = 1
    rows = [0, 1, 2, 3]
    k_rows = torch.stack([pg.k[pg.pages[b][pos[b] // PAGE], pos[b] % PAGE] for b in rows])
    n = len(rows)
    qk = torch.zeros(n, (Hq + Hkv) * D, dtype=torch.bfloat16, device=dev())
    qk[:, Hq * D:] = k_rows
    qkv4 = qkv[rows].contiguous()
    want = [mx.kd, mx.ks, mx.vd, mx.vs]
    for off, call in ((0, lambda m2, t: ops.kvcache_store_paged_mx(qk, qkv4, m2.planes, t, i32([n]), 1, n, Hq, Hkv)),
                      (3, lambda m2, t: ops.kvcache_store_at_paged_mx(qk, qkv4, m2.planes, t, i32([3]), i32([n]), 1, n, Hq,
                                                                      Hkv))):
        pg2 = Paged(_blank(1, PAGE, Hkv * D), _blank(1, PAGE, Hkv * D), [1], seed=3)
        m2 = PagedMx(pg2, Hkv * D)
        call(m2, pg2.table)
        page = pg2.pages[0][0]
        for plane2, plane in zip(m2.planes, want):
            for j, b in enumerate(rows):
                assert torch.equal(plane2[page, off + j], plane[pg.pages[b][pos[b] // PAGE], pos[b] % PAGE]), (off, b)


# ------------------------------------------------------------------------------------------- 4. the runner: wiring
CHUNK1 = [250, 256, 3, 130]
CHUNK2 = [12, 7, 1, 3]


def _pool(m, n_pages, seed=0, kv_dtype="mxfp8", shuffle=True):
    order = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist() if shuffle else None
    pool = m.kv_page_pool(n_pages, order=order, kv_dtype=kv_dtype)
    pool.buffer.view(torch.int16).fill_(SENT)
    return pool


def _prompt_ids(B=4, T=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 640, (B, T), generator=g), torch.randint(0, 640, (B, 64), generator=g)


def _by_hand(dec, ids, cont, lens1, lens2, steps):
    """Extend-only: the ragged block ``ids`` behind past = 0 (every position goes through the extend kernel), the ragged
    block cont[:, :12] behind it, then ``steps`` teacher-forced decode steps.  -> the logits of every call [2 + steps, B, V]
    and the final lengths."""
    dec.reserve([a + b + steps for a, b in zip(lens1, lens2)])
    out = [dec.extend(ids.to(dev()), i32([0] * len(lens1)), i32(lens1)).clone()]
    out.append(dec.extend(cont[:, :12].contiguous().to(dev()), i32(lens1), i32(lens2)).clone())
    lens = [a + b for a, b in zip(lens1, lens2)]
    cont_d = cont.to(dev())
    for t in range(steps):
        out.append(dec.step(cont_d[:, 12 + t].contiguous(), i32([n + t for n in lens]), max(lens) + t + 1).clone())
    return torch.stack(out), [n + steps for n in lens]


@pytest.mark.parametrize("kernels", ["tile", "skinny"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_runner_wiring_layer0_bytes_are_the_quantised_bf16_rows(name, kernels):
    """Layer 0's K / V depend on the embeddings only, so they are the same rows whatever the cache precision did to the
    layers above: after two ragged extends and 8 steps the bytes of the mxfp8 decoder equal mx_quant of the bf16 paged
    decoder's rows, and ``gather`` returns their dequantised values."""
    from speech_distill_amd.generation import Decoder
    m, _, _ = _model(name)
    ids, cont = _prompt_ids()
    B, cap = 4, 512
    bf = Decoder(m, B, cap, kernels, pool=_pool(m, 8, kv_dtype="bf16"))
    mx = Decoder(m, B, cap, kernels, pool=_pool(m, 8, seed=1))
    _, lens = _by_hand(bf, ids, cont, CHUNK1, CHUNK2, 8)
    logits, lens_mx = _by_hand(mx, ids, cont, CHUNK1, CHUNK2, 8)
    assert lens == lens_mx and bool(torch.isfinite(logits.float()).all())
    for b, n in enumerate(lens):
        k, v = bf.gather(0, b, n)
        kd, ks, vd, vs = mx.gather_raw(0, b, n)
        (kq, ksq), (vq, vsq) = quant(k), quant(v)
        assert torch.equal(kd.cpu(), kq) and torch.equal(ks.cpu(), ksq), b
        assert torch.equal(vd.cpu(), vq) and torch.equal(vs.cpu(), vsq), b
        kg, vg = mx.gather(0, b, n)
        assert kg.dtype == torch.bfloat16 and torch.equal(i16(kg.cpu()), i16(deq(kq, ksq))), b
        assert torch.equal(i16(vg.cpu()), i16(deq(vq, vsq))), b
    # the pages nobody owns were never written, in any plane of any layer
    free = torch.tensor(sorted(set(range(8)) - {p for r in mx.pages.rows for p in r}), device=dev())
    assert len(free) > 0
    for l in range(m.dims.num_hidden_layers):
        for plane in mx.pool.planes(l):
            assert bool((plane[free].view(torch.int16) == SENT).all())
    mx.close(), bf.close()
    assert mx.pool.pages_in_use == 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_runner_arithmetic_against_the_torch_restatement(name):
    """LOOSE and said so (the rule of test_gpu_mx.py::test_model_arithmetic_against_the_torch_restatement): quantisation is
    discontinuous, so a one-ulp bf16 difference upstream moves some cached elements by a whole e4m3 step.  Reference:
    tests/kvq_ref.py, the fp32 forward whose cached K / V rows pass through bf16 and the MXFP8 round trip for all keys.
    Budget: A.F_RMS (1.5) x the rms error of that restatement with storage="bf16" against itself in fp32, computed on the
    CPU (no code under test in it).  Also: the HIP logits are closer to the quantised restatement than to the
    unquantised oracle.  Measured on an MI355X: err / base 1.016 (student), 1.013 (twin); rms error against the
    unquantised oracle 0.035 / 0.040 where the quantised restatement is met within 0.014 / 0.018."""
    from speech_distill_amd.generation import Decoder
    m, shape, w = _model(name)
    ids, cont = _prompt_ids(T=70, seed=5)
    lens1, steps = [70, 64, 3, 33], 16
    dec = Decoder(m, 4, 256, "tile", pool=_pool(m, 6, seed=2))
    got, _ = _by_hand(dec, ids, cont, lens1, CHUNK2, steps)        # [2 + steps, B, V]
    got = got.float().cpu()
    refs = {"q": [], "q_bf16": [], "noq": []}
    with torch.no_grad():
        for b in range(4):
            seq = torch.cat([ids[b, :lens1[b]], cont[b, :CHUNK2[b]], cont[b, 12:12 + steps]])[None]
            n1, n2 = lens1[b], lens1[b] + CHUNK2[b]
            at = torch.tensor([n1 - 1, n2 - 1] + [n2 + t for t in range(steps)])
            refs["q"].append(kvq_ref.forward_kvq(w, shape, seq)[0, at])
            refs["q_bf16"].append(kvq_ref.forward_kvq(w, shape, seq, storage="bf16")[0, at])
            refs["noq"].append(kvq_ref.forward_kvq(w, shape, seq, quant=False)[0, at])
    ref, ref_bf16, noq = (torch.stack(refs[k], 1) for k in ("q", "q_bf16", "noq"))      # [2 + steps, B, V]
    base = rel_err(ref_bf16, ref)[1]
    err = rel_err(got, ref)[1]
    err_noq = rel_err(got, noq)[1]
    print(f"kv mxfp8 {name}: rms err vs quantised restatement {err:.4f}, budget base {base:.4f}, ratio {err / base:.3f}; "
          f"vs unquantised {err_noq:.4f}")
    record("paged_mx_model_vs_restatement", shape=name, rms_err=err, base=base, ratio=err / base,
           rms_vs_unquantised=err_noq)
    assert err <= A.F_RMS * base
    assert err < err_noq


# ------------------------------------------------------------------------------------------------------ 5. sessions
def _two_turns(m, pool, sync_every=16, seed=123):
    ids, cont = _prompt_ids()
    sess = m.start_session(4, capacity=512, pool=pool)
    kw = dict(max_new_tokens=24, eos_token_id=5, pad_token_id=2, sync_every=sync_every, **R.REFERENCE)
    a = sess.generate(ids.to(dev()), _mask(CHUNK1, 256).to(dev()), seed=seed, **kw)
    b = sess.generate(cont[:, :12].to(dev()), _mask(CHUNK2, 12).to(dev()), seed=seed + 1, **kw)
    out = torch.cat([a, b], 1).cpu(), sess.lengths().tolist()
    sess.close()
    return out


def test_session_tokens_do_not_depend_on_the_page_order_or_on_sync_every():
    m, _, _ = _model("student")
    base, lens = _two_turns(m, _pool(m, 10, shuffle=False))
    assert base.shape == (4, 48)
    got, l2 = _two_turns(m, _pool(m, 10, seed=7))
    assert torch.equal(got, base) and l2 == lens
    for se in (1, 3):
        got, l2 = _two_turns(m, _pool(m, 10, seed=se), sync_every=se)
        assert torch.equal(got, base) and l2 == lens, se
    other, _ = _two_turns(m, _pool(m, 10, seed=7), seed=124)
    assert not torch.equal(other, base)


def test_bytes_per_page_and_pool_members():
    m, _, _ = _model("student")
    bf, mx = m.kv_page_pool(3), m.kv_page_pool(3, kv_dtype="mxfp8")
    assert bf.kv_dtype == "bf16" and mx.kv_dtype == "mxfp8"
    assert mx.bytes_per_page * 256 == bf.bytes_per_page * 132
    L, Hkv = m.dims.num_hidden_layers, m.dims.num_key_value_heads
    assert mx.bytes_per_page == L * 2 * 256 * Hkv * 132 and mx.buffer.numel() == 3 * mx.bytes_per_page
    kd, ks, vd, vs = mx.planes(L - 1)
    assert kd.shape == vd.shape == (3, 256, Hkv * 128) and ks.shape == vs.shape == (3, 256, Hkv * 4)
    assert all(t.dtype == torch.uint8 for t in (kd, ks, vd, vs))
    end = vs.data_ptr() + vs.numel()
    assert end == mx.buffer.data_ptr() + mx.buffer.numel()            # the last plane of the last layer ends the buffer
    assert ks.data_ptr() == kd.data_ptr() + kd.numel() and vd.data_ptr() == ks.data_ptr() + ks.numel()
    with pytest.raises(ValueError):
        m.kv_page_pool(3, kv_dtype="fp8")
    other, _, _ = _model("twin")
    from speech_distill_amd.generation import Decoder
    with pytest.raises(ValueError):
        Decoder(other, 1, 256, pool=mx)                                # a pool of another model


def test_fork_shares_full_pages_and_copies_data_and_scales():
    from speech_distill_amd.paged import fork_split
    m, _, _ = _model("student")
    ids, cont = _prompt_ids(B=1, T=320)
    L = m.dims.num_hidden_layers
    pool = _pool(m, 12, seed=5)
    src = m.start_session(1, capacity=512, decode_kernels="skinny", pool=pool)
    src.extend(ids[:, :300].to(dev()))
    snap = [src.decoder.gather_raw(l, 0, 300) for l in range(L)]
    assert pool.pages_in_use == 2
    f = src.fork([0, 0, 0])
    shared, copied = fork_split(300)                                   # the rule of DESIGN.md 11b: (1, 1)
    assert (shared, copied) == (1, 1) and pool.pages_in_use == 2 + 3 * copied
    page0 = src.decoder.pages.rows[0][0]
    assert pool.alloc.refs[page0] == 1 + 3 * shared
    ft, st = f.decoder.table.cpu(), src.decoder.table.cpu()
    assert ft[:, 0].tolist() == [page0] * 3 and len({int(st[0, 1])} | set(ft[:, 1].tolist())) == 4
    for l in range(L):                                                 # data AND scale bytes came along, in every layer
        for b in range(3):
            for got, want in zip(f.decoder.gather_raw(l, b, 300), snap[l]):
                assert torch.equal(got, want), (l, b)
    tok = ids[:, 300:301].to(dev())
    g = f.generate(tok.expand(3, 1).contiguous(), max_new_tokens=8, do_sample=False).cpu()
    assert torch.equal(g[0], g[1]) and torch.equal(g[0], g[2])
    # every fork of row 0 continues as an independent session does that cached the same 300 tokens itself, seed by seed
    for i in range(3):
        fi = src.fork([0])
        ind = m.start_session(1, capacity=512, decode_kernels="skinny", pool=pool)
        ind.extend(ids[:, :300].to(dev()))
        kw = dict(max_new_tokens=8, seed=40 + i, **R.REFERENCE)
        assert torch.equal(fi.generate(tok, **kw), ind.generate(tok, **kw)), i
        fi.close(), ind.close()
    f.close(), src.close()
    assert pool.pages_in_use == 0


def test_a_pool_one_page_short_raises_and_changes_nothing():
    m, _, _ = _model("student")
    ids, cont = _prompt_ids()
    NEW, cap = 16, 1024
    mask = _mask(CHUNK1, 256).to(dev())
    need = sum(pages_for(n + NEW) for n in CHUNK1)                   # 2 + 2 + 1 + 1
    control = m.start_session(4, capacity=cap, pool=_pool(m, need + 1, seed=1))
    control.generate(ids.to(dev()), mask, max_new_tokens=NEW, do_sample=False)
    want = control.generate(cont[:, :4].to(dev()), max_new_tokens=NEW, do_sample=False).cpu()
    pool = _pool(m, need)
    sess = m.start_session(4, capacity=cap, pool=pool)
    sess.generate(ids.to(dev()), mask, max_new_tokens=NEW, do_sample=False)
    lens, used = sess.lengths().tolist(), pool.pages_in_use
    assert used == need and pool.free_pages == 0
    rows = [list(r) for r in sess.decoder.pages.rows]
    big = 120
    assert sum(pages_for(n + 4 + big) for n in lens) == need + 1
    with pytest.raises(ValueError):
        sess.generate(cont[:, :4].to(dev()), max_new_tokens=big, do_sample=False)
    assert pool.pages_in_use == used and sess.lengths().tolist() == lens
    assert [list(r) for r in sess.decoder.pages.rows] == rows
    got = sess.generate(cont[:, :4].to(dev()), max_new_tokens=NEW, do_sample=False).cpu()
    assert torch.equal(got, want)


def test_prefill_sink_quantises_what_the_extend_path_quantises():
    """A one-turn greedy session starts with sd_qwen3_prefill_paged_mx, whose prompt attends over its own bf16 K / V: only
    the sink quantises (include/sd_hip.h).  Layer 0 depends on the embeddings only, so its bytes equal those the
    extend-only path leaves, and they are mx_quant of the bf16 session's rows."""
    from speech_distill_amd.generation import Decoder
    m, _, _ = _model("student")
    ids, _ = _prompt_ids()
    mask = _mask(CHUNK1, 256).to(dev())
    sess = m.start_session(4, capacity=512, pool=_pool(m, 8, seed=3))
    sess.generate(ids.to(dev()), mask, max_new_tokens=4, do_sample=False)
    hand = Decoder(m, 4, 512, "tile", pool=_pool(m, 8, seed=4))
    hand.reserve(CHUNK1)
    hand.extend(ids.to(dev()), i32([0] * 4), i32(CHUNK1))
    bf = m.start_session(4, capacity=512, pool=_pool(m, 8, seed=5, kv_dtype="bf16"))
    bf.generate(ids.to(dev()), mask, max_new_tokens=4, do_sample=False)
    for b, n in enumerate(CHUNK1):
        a, c = sess.decoder.gather_raw(0, b, n), hand.gather_raw(0, b, n)
        k, v = bf.decoder.gather(0, b, n)
        for x, y, z in zip(a, c, quant(k) + quant(v)):
            assert torch.equal(x, y) and torch.equal(x.cpu(), z), b
