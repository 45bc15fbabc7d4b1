"""-m gpu: generation on MXFP8 weights with ``gemv_rows=64`` -- the decode step on the 64-row block-scaled GEMV
(sd_qwen3_mx_decode_step_wide; csrc/sd_gemv_mx.hip, sd_mx.hip, generation.py).

Yardsticks: the step's launches composed by hand from the ``ops`` bindings over a cache of the hand's own (logits and
every cache byte, each cache kind), the same step on one row for the batch invariance, sd_qwen3_mx_decode_step(flags = 0)
for the whole fallback, the skinny MXFP8 step for the hidden state at B <= 16, and the default keyword for everything that
must not change.  The model is the tiny shape of tests/test_gpu_mx.py (``SHP``, restated here); the pool shapes are those of
tests/test_gpu_generate_mx.py with one page per row for 33 rows.  All comparisons are torch.equal."""
import pytest
import torch

from gpu_util import dev, to_dev

pytestmark = pytest.mark.gpu

SHP = (1200, 512, 1024, 3, 4, 2)   # the tiny model of tests/test_gpu_mx.py, restated


def _weights(seed):
    from oracle import qwen3 as Q
    shp = Q.Qwen3Shape(*SHP)
    return shp, {k: v.bfloat16().float() for k, v in Q.init_weights(shp, seed=seed, norm_jitter=0.25).items()}


def _model(sda, w, device=None):
    model = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*SHP), device=device or dev(), init_std=0)
    model.load_hf_state_dict(w)
    model.eval().requires_grad_(False)
    return model


SENT = 0x7FC1
KINDS = ("contig", "paged", "paged_mx")
CAP = 256
B33 = 33
LENS4 = [24, 17, 9, 1]
MODE = dict(decode_kernels="skinny", weight_dtype="mxfp8", gemv_rows=64)


@pytest.fixture(scope="module")
def sda():
    import speech_distill_amd as m
    m.load_lib()
    return m


@pytest.fixture(scope="module")
def model(sda):
    _, w = _weights(9)
    return _model(sda, w)


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=dev())


def _pool(m, kind, seed=0, n_pages=B33 + 3):
    if kind == "contig":
        return None
    order = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    pool = m.kv_page_pool(n_pages, order=order, kv_dtype="mxfp8" if kind == "paged_mx" else "bf16")
    pool.buffer.view(torch.int16).fill_(SENT)
    return pool


def _lens(B):
    return [LENS4[b % 4] for b in range(B)]


def _ids(B, T=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, SHP[0], (B, T), generator=g), torch.randint(0, SHP[0], (B, 16), generator=g)


def _mask(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)


def _decoder(model, B, kind="contig", seed=0, **kw):
    from speech_distill_amd.generation import Decoder
    dec = Decoder(model, B, CAP, pool=_pool(model, kind, seed), **(kw or MODE))
    if kind != "contig":
        dec.reserve([n + 8 for n in _lens(B)])
    return dec


def _storage(dec):
    return dec.cache if dec.pool is None else dec.pool.buffer


class Hand:
    """The launches of sd_qwen3_mx_decode_step_wide composed from the ops bindings on the model's own quantised weights
    (``model._mx[2]``), over storage of the hand's own (a paged hand reads the table of the decoder it shadows)."""

    def __init__(self, model, kind, shadow):
        from speech_distill_amd import ops
        self.ops, self.m, self.kind = ops, model, kind
        d = model.dims
        self.Hq, self.Hkv, self.eps, self.L = d.num_attention_heads, d.num_key_value_heads, d.rms_norm_eps, d.num_hidden_layers
        model._mx_params()
        self.keep = model._mx[2]
        self.cos, self.sin = model._tables(CAP, dev())
        self.table = None if kind == "contig" else shadow.table
        if kind == "contig":
            from speech_distill_amd.generation import Decoder
            self.own = Decoder(model, shadow.B, CAP, "tile", weight_dtype="mxfp8")
            self.own.cache.copy_(shadow.cache)
            self.planes = [self.own.planes(l) for l in range(self.L)]
            self.storage = self.own.cache
        else:
            self.pool = _pool(model, kind)
            self.pool.buffer.copy_(shadow.pool.buffer)          # the same cached rows on the same pages
            self.planes = [self.pool.planes(l) for l in range(self.L)]
            self.storage = self.pool.buffer

    def hidden(self, ids, pos, max_len):
        ops, m = self.ops, self.m
        x = ops.embedding_fwd(ids, m._params["model.embed_tokens.weight"].data)
        for l in range(self.L):
            p = f"model.layers.{l}.self_attn."
            qg, kg = m._params[p + "q_norm.weight"].data, m._params[p + "k_norm.weight"].data
            wqkv_q, wqkv_s, wgu_q, wgu_s, wo_q, wo_s, wd_q, wd_s = self.keep[8 * l:8 * l + 8]
            qkv = ops.gemv_mxfp8(x, wqkv_q, wqkv_s, norm=True, eps=self.eps, wide=True)
            pl = self.planes[l]
            if self.kind == "contig":
                q = ops.qknorm_rope_append(qkv, qg, kg, self.cos, self.sin, pos, *pl, self.Hq, self.Hkv, self.eps)
                ao = ops.attn_decode(q, *pl, pos, self.Hq, self.Hkv, max_len=max_len, len_add=1)
            elif self.kind == "paged":
                q = ops.qknorm_rope_append_paged(qkv, qg, kg, self.cos, self.sin, pos, *pl, self.table, self.Hq, self.Hkv,
                                                 self.eps)
                ao = ops.attn_decode_paged(q, *pl, self.table, pos, self.Hq, self.Hkv, max_len=max_len, len_add=1)
            else:
                q = ops.qknorm_rope_append_paged_mx(qkv, qg, kg, self.cos, self.sin, pos, pl, self.table, self.Hq, self.Hkv,
                                                    self.eps)
                ao = ops.attn_decode_paged_mx(q, pl, self.table, pos, self.Hq, self.Hkv, max_len=max_len, len_add=1)
            x_mid = ops.gemv_mxfp8(ao, wo_q, wo_s, residual=x, wide=True)
            act = ops.gemv_mxfp8_swiglu(x_mid, wgu_q, wgu_s, norm=True, eps=self.eps, wide=True)
            x = ops.gemv_mxfp8(act, wd_q, wd_s, residual=x_mid, wide=True)
        return x

    def head(self, x):
        return self.ops.gemv_bf16(x, self.m.lm_head.weight.data, norm_gain=self.m._params["model.norm.weight"].data,
                                  eps=self.eps, wide=True)

    def step(self, ids, pos, max_len):
        return self.head(self.hidden(ids, pos, max_len))


# ------------------------------------------------------------------------------------------------ 1: wiring
@pytest.mark.parametrize("kind", KINDS)
def test_a_33_row_step_equals_the_hand_composed_launches(model, kind):
    """A ragged prefill of 33 rows, then two steps: the logits and EVERY byte of the cache / pool equal the same launches
    composed by hand over a copy of the storage; pages nobody owns keep their pattern."""
    ids, cont = _ids(B33)
    lens = _lens(B33)
    dec = _decoder(model, B33, kind, seed=1)
    assert dec.mx_wide and dec.flags == 1 and not dec.wide
    dec.prefill(to_dev(ids), i32(lens))
    hand = Hand(model, kind, dec)
    cont_d = cont.to(dev())
    for t in range(2):
        pos = i32([n + t for n in lens])
        got = dec.step(cont_d[:, t].contiguous(), pos, max(lens) + t + 1).clone()
        want = hand.step(cont_d[:, t].contiguous(), pos, max(lens) + t + 1)
        assert bool(torch.isfinite(got.float()).all())
        assert torch.equal(got, want), f"step {t}: {int((got != want).sum())} logits differ"
        assert torch.equal(_storage(dec), hand.storage), f"step {t}: the cache bytes differ"
    if kind != "contig":
        free = torch.tensor(sorted(set(range(dec.pool.n_pages)) - {p for r in dec.pages.rows for p in r}), device=dev())
        assert len(free) > 0
        for l in range(model.dims.num_hidden_layers):
            for plane in dec.pool.planes(l):
                assert bool((plane[free].view(torch.int16) == SENT).all())
        dec.close()


def test_row_b_of_a_33_row_step_equals_the_one_row_step(model):
    """Over the same cached rows (copied across: the prefill runs tile GEMMs at another M)."""
    ids, cont = _ids(B33, seed=2)
    lens = _lens(B33)
    dec = _decoder(model, B33)
    dec.prefill(to_dev(ids), i32(lens))
    cont_d = cont.to(dev())
    before = [tuple(p.clone() for p in dec.planes(l)) for l in range(model.dims.num_hidden_layers)]
    full = [dec.step(cont_d[:, t].contiguous(), i32([n + t for n in lens]), max(lens) + t + 1).clone() for t in range(2)]
    for b in (0, 15, 16, 32):
        one = _decoder(model, 1)
        for l, planes in enumerate(before):
            for dst, src in zip(one.planes(l), planes):
                dst[0] = src[b]
        for t in range(2):
            row = one.step(cont_d[b:b + 1, t].contiguous(), i32([lens[b] + t]), lens[b] + t + 1)
            assert torch.equal(row[0], full[t][b]), (b, t)


# ------------------------------------------------------------------------------------- 2: fallback and launch labels
def _one_step(model, B, **kw):
    """(logits, {kernel symbol: launches}) of one decode step after an 8-token prefill of B rows."""
    from speech_distill_amd import ops
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, SHP[0], (B, 8), generator=g).to(dev())
    nxt = torch.randint(0, SHP[0], (B,), generator=g).to(dev())
    dec = _decoder(model, B, **kw)
    kv_len = torch.full((B,), 8, dtype=torch.int32, device=dev())
    dec.prefill(ids, kv_len)
    ops.prof_begin()
    logits = dec.step(nxt, kv_len, 9).clone()
    ops.prof_end()
    return logits, {sym: int(v[2]) for sym, v in ops.prof_symbols().items()}


def _count(launches, prefix):
    return sum(n for sym, n in launches.items() if sym.startswith(prefix))


def test_the_step_falls_back_whole_at_65_rows_and_takes_the_new_kernels_at_33(model):
    """B = 65: the step IS sd_qwen3_mx_decode_step(flags = 0) -- same bits, no GEMV launch of either family.  B = 33: 4
    gemv_mx_wide_kernel launches per layer, the head on wide_gemv_kernel, no 16-row GEMV, quantiser, RMSNorm, SwiGLU or
    tile GEMM: 7 L + 2 launches in all.  With the keyword at its default the 16-row kernels run as before."""
    L = model.dims.num_hidden_layers
    new65, sym65 = _one_step(model, 65, **MODE)
    tile65, _ = _one_step(model, 65, decode_kernels="tile", weight_dtype="mxfp8")
    assert torch.equal(new65, tile65)
    assert _count(sym65, "gemv_mx_wide_kernel") == 0 and _count(sym65, "wide_gemv_kernel") == 0
    _, sym33 = _one_step(model, 33, **MODE)
    assert _count(sym33, "gemv_mx_wide_kernel<3, ") == 4 * L, sym33
    assert _count(sym33, "wide_gemv_kernel") == 1 and _count(sym33, "gemv_mx_kernel") == 0, sym33
    assert _count(sym33, "gemv_kernel") == 0 and _count(sym33, "rmsnorm") == 0 and _count(sym33, "swiglu") == 0, sym33
    assert _count(sym33, "gemm") == 0 and _count(sym33, "mxfp8_quant") == 0, sym33
    assert sum(sym33.values()) == 7 * L + 2, sym33
    _, sym4 = _one_step(model, 4, decode_kernels="skinny", weight_dtype="mxfp8")
    assert _count(sym4, "gemv_mx_wide_kernel") == 0 and _count(sym4, "gemv_mx_kernel") == 4 * L, sym4


def test_the_hidden_state_before_the_head_is_the_skinny_steps_at_4_rows(model):
    """B = 4: the hidden state that enters the head (the first buffer of the step's acts, where the last down projection
    leaves it) has the bits of the skinny MXFP8 step's; the logits are the wide head on it (hand-composed), which also
    pins the buffer that was read."""
    ids, cont = _ids(4, seed=3)
    new, old = _decoder(model, 4), _decoder(model, 4, decode_kernels="skinny", weight_dtype="mxfp8")
    h = model.dims.hidden_size
    for dec in (new, old):
        dec.prefill(to_dev(ids), i32(LENS4))
    hand = Hand(model, "contig", new)
    tok, pos = cont[:, 0].contiguous().to(dev()), i32(LENS4)
    logits_new = new.step(tok, pos, max(LENS4) + 1).clone()
    logits_old = old.step(tok, pos, max(LENS4) + 1).clone()
    x_new = new.step_acts[:4 * h * 2].view(torch.bfloat16).view(4, h)
    x_old = old.step_acts[:4 * h * 2].view(torch.bfloat16).view(4, h)
    assert torch.equal(x_new, x_old)
    assert torch.equal(hand.head(x_old), logits_new)
    from speech_distill_amd import ops
    assert torch.equal(ops.gemv_bf16(x_old, model.lm_head.weight.data, norm_gain=model._params["model.norm.weight"].data,
                                     eps=model.dims.rms_norm_eps), logits_old)


# ------------------------------------------------------------------------------------------------ 3: batch invariance
def test_generate_of_33_ragged_rows_equals_each_prompt_alone(model):
    """Greedy: every row's new tokens are those of the prompt generated alone with the same keywords; sampled with a seed:
    the tokens do not depend on sync_every (row-wise sampled equality is the next test)."""
    ids, _ = _ids(B33, seed=4)
    lens = _lens(B33)
    am = _mask(lens, 24)
    junk = torch.where(am.bool(), ids, torch.full_like(ids, SHP[0] - 1))   # the pad slots hold a token the rows never see
    greedy = dict(max_new_tokens=8, do_sample=False, **MODE)
    out = model.generate(junk.to(dev()), attention_mask=am.to(dev()), **greedy).cpu()
    for b, n in enumerate(lens):
        alone = model.generate(ids[b:b + 1, :n].to(dev()), **greedy).cpu()
        assert torch.equal(alone[0, n:], out[b, 24:]), b
    sampled = dict(attention_mask=am.to(dev()), max_new_tokens=8, do_sample=True, top_k=20, temperature=0.9, seed=3,
                   eos_token_id=int(out[0, 26]), pad_token_id=2, **MODE)
    assert torch.equal(model.generate(junk.to(dev()), sync_every=1, **sampled),
                       model.generate(junk.to(dev()), sync_every=16, **sampled))


def test_sampled_rows_equal_each_prompt_alone(model):
    """33 rows through one decoder and the sampler against a one-row decoder per prompt fed the same uniforms u[:, b]."""
    from speech_distill_amd.ops import sample_params, sample_step
    B, steps = B33, 6
    ids, _ = _ids(B, seed=5)
    lens = _lens(B)
    u = torch.rand(steps, B, 2, generator=torch.Generator().manual_seed(6)).to(dev())
    sp = sample_params(True, 0.9, 20, 1.0, 1.0, 0, None, 0, False, 25, 0.2)

    def run(rows):
        n = len(rows)
        dec = _decoder(model, n)
        kv = i32([lens[b] for b in rows])
        logits = dec.prefill(ids[rows].to(dev()), kv)
        seq = torch.zeros(n, CAP, dtype=torch.int64, device=dev())
        seq[:, :24] = ids[rows].to(dev())
        start, ln = kv.clone(), kv.clone()
        fin = torch.zeros(n, dtype=torch.uint8, device=dev())
        nxt = torch.empty(n, dtype=torch.int64, device=dev())
        pos = torch.empty(n, dtype=torch.int32, device=dev())
        toks = []
        for t in range(steps):
            sample_step(logits, u[t, rows].contiguous(), seq, start, ln, fin, sp, next_out=nxt, pos_out=pos)
            toks.append(nxt.clone())
            logits = dec.step(nxt, pos, 24 + t + 1)
        return torch.stack(toks, 1).cpu()

    batch = run(list(range(B)))
    for b in (0, 1, 2, 3, 15, 16, 31, 32):
        assert torch.equal(run([b])[0], batch[b]), b


# ------------------------------------------------------------------------------------------------ 4: sessions
def _two_turns(m, kind, sync_every=16, seed=0):
    ids, cont = _ids(4, seed=7)
    sess = m.start_session(4, capacity=CAP, pool=_pool(m, kind, seed, n_pages=8), **MODE)
    assert sess.gemv_rows == 64 and sess.decoder.mx_wide
    kw = dict(max_new_tokens=8, do_sample=False, sync_every=sync_every)
    a = sess.generate(to_dev(ids), to_dev(_mask(LENS4, 24)), **kw)
    b = sess.generate(to_dev(cont[:, :12].contiguous()), to_dev(_mask([12, 7, 1, 3], 12)), **kw)
    out = torch.cat([a, b], 1).cpu()
    sess.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_session_tokens_do_not_depend_on_sync_every_or_the_page_order(model, kind):
    base = _two_turns(model, kind)
    assert base.shape == (4, 16)
    assert torch.equal(_two_turns(model, kind, sync_every=1, seed=3), base)


def test_fork_inherits_the_keyword_and_continues_a_row_as_an_independent_session_does(model):
    ids, _ = _ids(1, T=200, seed=8)
    pool = _pool(model, "paged_mx", seed=5, n_pages=40)
    src = model.start_session(1, capacity=CAP, pool=pool, **MODE)
    src.extend(to_dev(ids[:, :180]))
    f = src.fork([0] * 20)
    assert f.gemv_rows == 64 and f.decoder.mx_wide and f.weight_dtype == "mxfp8" and f.decoder.B == 20
    with pytest.raises(ValueError, match="not built"):
        src.fork([0, 0], shared_kv_reads=True)
    tok = to_dev(ids[:, 180:181])
    g = f.generate(tok.expand(20, 1).contiguous(), max_new_tokens=6, do_sample=False).cpu()
    assert all(torch.equal(g[0], g[b]) for b in range(1, 20))
    ind = model.start_session(1, capacity=CAP, pool=pool, **MODE)
    ind.extend(to_dev(ids[:, :180]))
    assert torch.equal(ind.generate(tok, max_new_tokens=6, do_sample=False).cpu()[0], g[0])
    f.close(), ind.close(), src.close()
    assert pool.pages_in_use == 0


def test_reloaded_weights_are_the_ones_decoded_with(sda):
    """The decoder fetches the quantised weights on every call: after load_hf_state_dict a LIVE decoder's step computes
    what a decoder made after the reload computes."""
    _, w = _weights(9)
    _, w2 = _weights(10)
    m = _model(sda, w)
    ids, _ = _ids(B33, seed=9)
    lens = _lens(B33)
    live = _decoder(m, B33)
    live.prefill(to_dev(ids), i32(lens))
    tok = to_dev(ids[:, 0].contiguous())
    before = live.step(tok, i32(lens), max(lens) + 1).clone()
    m.load_hf_state_dict(w2)
    live.prefill(to_dev(ids), i32(lens))
    after = live.step(tok, i32(lens), max(lens) + 1).clone()
    fresh = _decoder(m, B33)
    fresh.prefill(to_dev(ids), i32(lens))
    assert torch.equal(after, fresh.step(tok, i32(lens), max(lens) + 1))
    assert not torch.equal(after, before)


# ---------------------------------------------------------------------------------------------------- 5: defaults
def test_the_default_keyword_leaves_every_existing_path_alone(model):
    from speech_distill_amd.generation import Decoder
    ids, _ = _ids(4, seed=10)
    am = to_dev(_mask(LENS4, 24))
    for kernels, weights in (("skinny", "mxfp8"), ("tile", "mxfp8"), ("skinny", "bf16"), ("wide", "bf16"), ("tile", "bf16")):
        kw = dict(attention_mask=am, max_new_tokens=6, do_sample=True, top_k=50, temperature=0.8, seed=5,
                  decode_kernels=kernels, weight_dtype=weights)
        assert torch.equal(model.generate(to_dev(ids), **kw), model.generate(to_dev(ids), gemv_rows=16, **kw))
        dec = Decoder(model, 2, 16, kernels, weight_dtype=weights)
        assert not dec.mx_wide and dec.flags == (1 if kernels == "skinny" else 0) and dec.wide == (kernels == "wide")
    _, sym = _one_step(model, 4, decode_kernels="skinny", weight_dtype="mxfp8", gemv_rows=16)
    assert _count(sym, "gemv_mx_wide_kernel") == 0 and _count(sym, "gemv_mx_kernel") > 0
