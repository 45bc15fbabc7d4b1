"""-m gpu: generation on MXFP8 weights -- the three runner entries sd_qwen3_mx_prefill / _extend / _decode_step over each
kind of KV cache, and ``weight_dtype="mxfp8"`` through ``Decoder``, ``generate`` and sessions (sd_mx.hip, generation.py).

Wiring is exact: the entries' logits equal, bit for bit, the same launches composed by hand from the ``ops`` bindings on
the model's own quantised weights (``model._mx[2]``), over caches of the hand's own.  Arithmetic is checked loosely, and
said so, against tests/mx_ref.py.  The model is the tiny shape of tests/test_gpu_mx.py (``SHP``), B = 4, with the ragged
lengths of tests/test_gpu_paged_mx.py."""
import pytest
import torch

import mx_ref
from gpu_util import dev, record, rel_err, to_dev
from test_gpu_mx import SHP, _model, _weights

pytestmark = pytest.mark.gpu

SENT = 0x7FC1
CHUNK1 = [250, 256, 3, 130]
CHUNK2 = [12, 7, 1, 3]
KINDS = ("contig", "paged", "paged_mx")
B, CAP, N_PAGES = 4, 512, 10


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


def _pool(m, kind, seed=0, shuffle=True, n_pages=N_PAGES):
    if kind == "contig":
        return None
    order = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist() if shuffle else None
    pool = m.kv_page_pool(n_pages, order=order, kv_dtype="mxfp8" if kind == "paged_mx" else "bf16")
    pool.buffer.view(torch.int16).fill_(SENT)
    return pool


def _ids(T=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, SHP[0], (B, T), generator=g), torch.randint(0, SHP[0], (B, 64), generator=g)


def _mask(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)


class Hand:
    """The launches of the three entries composed from the ops bindings, over a cache of the same kind that belongs to
    the hand alone (a paged hand reads the page table of the decoder it shadows: page numbers are pool-relative)."""

    def __init__(self, model, kind, kernels, table=None):
        from speech_distill_amd import ops
        self.ops, self.m, self.kind, self.skinny = ops, model, kind, kernels == "skinny"
        d = model.dims
        self.Hq, self.Hkv, self.eps, self.L = d.num_attention_heads, d.num_key_value_heads, d.rms_norm_eps, d.num_hidden_layers
        self.QD, self.KD = self.Hq * 128, self.Hkv * 128
        model._mx_params()
        self.keep = model._mx[2]
        self.cos, self.sin = model._tables(CAP, dev())
        self.table = table
        if kind == "contig":
            self.planes = [tuple(torch.zeros(B, CAP, self.KD, dtype=torch.bfloat16, device=dev()) for _ in range(2))
                           for _ in range(self.L)]
        else:
            self.pool = _pool(model, kind)
            self.planes = [self.pool.planes(l) for l in range(self.L)]
        self.E = model._params["model.embed_tokens.weight"].data
        self.norm = model._params["model.norm.weight"].data

    def gains(self, l):
        p = f"model.layers.{l}.self_attn."
        return self.m._params[p + "q_norm.weight"].data, self.m._params[p + "k_norm.weight"].data

    # ---- the four projections, as the tile sequence or as the GEMV sequence
    def qkv(self, l, x, skinny):
        wq, ws = self.keep[8 * l:8 * l + 2]
        if skinny:
            return self.ops.gemv_mxfp8(x, wq, ws, norm=True, eps=self.eps)
        xq, xs, rstd = self.ops.mxfp8_quant(x, want_rstd=True, eps=self.eps)
        return self.ops.gemm_mxfp8(xq, xs, wq, ws, rowscale=rstd)

    def rest(self, l, x, ao, skinny):
        ops = self.ops
        _, _, wgu_q, wgu_s, wo_q, wo_s, wd_q, wd_s = self.keep[8 * l:8 * l + 8]
        if skinny:
            x_mid = ops.gemv_mxfp8(ao, wo_q, wo_s, residual=x)
            act = ops.gemv_mxfp8_swiglu(x_mid, wgu_q, wgu_s, norm=True, eps=self.eps)
            return ops.gemv_mxfp8(act, wd_q, wd_s, residual=x_mid)
        aq, as_ = ops.mxfp8_quant(ao)
        x_mid = ops.gemm_mxfp8(aq, as_, wo_q, wo_s, residual=x)
        mq, ms, rstd2 = ops.mxfp8_quant(x_mid, want_rstd=True, eps=self.eps)
        cq, cs = ops.gemm_mxfp8_swiglu(mq, ms, wgu_q, wgu_s, rowscale=rstd2)
        return ops.gemm_mxfp8(cq, cs, wd_q, wd_s, residual=x_mid)

    def extend(self, ids, past, new_len):
        ops, T = self.ops, ids.shape[1]
        x = ops.embedding_fwd(ids.reshape(-1), self.E)
        pos = (past[:, None] + torch.arange(T, device=dev(), dtype=torch.int32)[None, :]).clamp(0, CAP - 1).long()
        cos_r, sin_r = self.cos[pos].reshape(B * T, -1).contiguous(), self.sin[pos].reshape(B * T, -1).contiguous()
        for l in range(self.L):
            qg, kg = self.gains(l)
            qkv = self.qkv(l, x, False)
            qk = ops.qknorm_rope_fwd(qkv, qg, kg, cos_r, sin_r, B * T, self.Hq, self.Hkv, self.eps)
            q, pl = qk[:, :self.QD], self.planes[l]
            if self.kind == "contig":
                ops.kvcache_store_at(qk, qkv, *pl, past, new_len, B, T, self.Hq, self.Hkv)
                ao = ops.attn_extend(q, *pl, past, new_len, T, self.Hq, self.Hkv, want_lse=False)
            elif self.kind == "paged":
                ops.kvcache_store_at_paged(qk, qkv, *pl, self.table, past, new_len, B, T, self.Hq, self.Hkv)
                ao = ops.attn_extend_paged(q, *pl, self.table, past, new_len, T, self.Hq, self.Hkv, want_lse=False)
            else:
                ops.kvcache_store_at_paged_mx(qk, qkv, pl, self.table, past, new_len, B, T, self.Hq, self.Hkv)
                ao = ops.attn_extend_paged_mx(q, pl, self.table, past, new_len, T, self.Hq, self.Hkv, want_lse=False)
            x = self.rest(l, x, ao, False)
        xn, _ = ops.rmsnorm_fwd(x, self.norm, self.eps)
        xn = ops.embedding_fwd(ops.last_rows(new_len, B, T), xn)
        return ops.gemm(xn, self.m.lm_head.weight.data)

    def step(self, ids, pos, max_len):
        ops = self.ops
        x = ops.embedding_fwd(ids, self.E)
        for l in range(self.L):
            qg, kg = self.gains(l)
            qkv = self.qkv(l, x, self.skinny)
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
            x = self.rest(l, x, ao, self.skinny)
        if self.skinny:
            return ops.gemv_bf16(x, self.m.lm_head.weight.data, norm_gain=self.norm, eps=self.eps)
        xn, _ = ops.rmsnorm_fwd(x, self.norm, self.eps)
        return ops.gemm(xn, self.m.lm_head.weight.data)


def _sequence(call, ids, cont, lens1, lens2, steps):
    """Two ragged extends (the first behind past = 0) and ``steps`` teacher-forced decode steps through ``call`` (a
    Decoder or a Hand) -> the logits of every call [2 + steps, B, V]."""
    out = [call.extend(ids.to(dev()), i32([0] * B), i32(lens1)).clone()]
    out.append(call.extend(cont[:, :12].contiguous().to(dev()), i32(lens1), i32(lens2)).clone())
    lens = [a + b for a, b in zip(lens1, lens2)]
    cont_d = cont.to(dev())
    for t in range(steps):
        out.append(call.step(cont_d[:, 12 + t].contiguous(), i32([n + t for n in lens]), max(lens) + t + 1).clone())
    return torch.stack(out)


def _decoder(model, kind, kernels, seed=0, shuffle=True, reserve=None):
    from speech_distill_amd.generation import Decoder
    dec = Decoder(model, B, CAP, kernels, pool=_pool(model, kind, seed, shuffle), weight_dtype="mxfp8")
    if kind != "contig":
        dec.reserve(reserve or [a + b + 8 for a, b in zip(CHUNK1, CHUNK2)])
    return dec


# ------------------------------------------------------------------------------------------------ 8: wiring
@pytest.mark.parametrize("kernels", ["tile", "skinny"])
@pytest.mark.parametrize("kind", KINDS)
def test_prefill_logits_are_the_mx_forward_with_the_last_rows(model, kind, kernels):
    ids, _ = _ids()
    dec = _decoder(model, kind, kernels, reserve=CHUNK1)
    got = dec.prefill(to_dev(ids), i32(CHUNK1)).clone()
    rows = to_dev(torch.tensor([b * 256 + n - 1 for b, n in enumerate(CHUNK1)]))
    model.set_inference_precision("mxfp8")
    try:
        with torch.no_grad():
            want = model(input_ids=to_dev(ids), attention_mask=to_dev(_mask(CHUNK1, 256)), logit_rows=rows).logits
    finally:
        model.set_inference_precision("bf16")
    assert torch.equal(got, want)
    dec.close()


@pytest.mark.parametrize("kernels", ["tile", "skinny"])
@pytest.mark.parametrize("kind", KINDS)
def test_extends_and_steps_equal_the_hand_composed_sequence(model, kind, kernels):
    """Two ragged extends and 8 teacher-forced steps, bit for bit; a shuffled page order gives the identity order's logits
    and the pages nobody owns keep their pattern in every plane of every layer."""
    ids, cont = _ids()
    dec = _decoder(model, kind, kernels)
    got = _sequence(dec, ids, cont, CHUNK1, CHUNK2, 8)
    assert bool(torch.isfinite(got.float()).all())
    hand = Hand(model, kind, kernels, table=None if kind == "contig" else dec.table)
    want = _sequence(hand, ids, cont, CHUNK1, CHUNK2, 8)
    for i in range(got.shape[0]):
        assert torch.equal(got[i], want[i]), f"call {i}: {int((got[i] != want[i]).sum())} logits differ"
    if kind != "contig":
        plain = _decoder(model, kind, kernels, shuffle=False)
        assert torch.equal(_sequence(plain, ids, cont, CHUNK1, CHUNK2, 8), got)
        free = torch.tensor(sorted(set(range(N_PAGES)) - {p for r in dec.pages.rows for p in r}), device=dev())
        assert len(free) > 0
        for l in range(model.dims.num_hidden_layers):
            for plane in dec.pool.planes(l):
                assert bool((plane[free].view(torch.int16) == SENT).all())
        plain.close()
    dec.close()


def test_skinny_step_rows_do_not_depend_on_the_batch(model):
    """Row b's logits of a B = 4 skinny step equal those of a B = 1 step on that row over the same cached rows (the cache
    rows are copied across: the extend pass runs tile GEMMs, whose bits may depend on M)."""
    from speech_distill_amd.generation import Decoder
    ids, cont = _ids()
    dec = Decoder(model, B, CAP, "skinny", weight_dtype="mxfp8")
    dec.extend(to_dev(ids), i32([0] * B), i32(CHUNK1))
    cont_d = cont.to(dev())
    before = [tuple(p.clone() for p in dec.planes(l)) for l in range(model.dims.num_hidden_layers)]
    full = [dec.step(cont_d[:, t].contiguous(), i32([n + t for n in CHUNK1]), max(CHUNK1) + t + 1).clone() for t in range(3)]
    for b in (0, 2, 3):
        one = Decoder(model, 1, CAP, "skinny", weight_dtype="mxfp8")
        for l, planes in enumerate(before):
            for dst, src in zip(one.planes(l), planes):
                dst[0] = src[b]
        for t in range(3):
            row = one.step(cont_d[b:b + 1, t].contiguous(), i32([CHUNK1[b] + t]), CHUNK1[b] + t + 1)
            assert torch.equal(row[0], full[t][b]), (b, t)


# ------------------------------------------------------------------------------------------------ 9: arithmetic
def test_arithmetic_against_the_torch_restatement(sda):
    """LOOSE and said so (the rule of tests/test_gpu_mx.py::test_model_arithmetic_against_the_torch_restatement):
    quantisation is discontinuous, so a one-ulp bf16 difference upstream moves some elements by a whole e4m3 step.  Logits
    of one ragged extend + 16 steps over a contiguous bf16 cache against mx_ref.teacher_forward_mx of each row's whole
    sequence at those positions.  Budget: 1.5 x the rms error of that restatement with storage="bf16" against itself in
    fp32, computed on the CPU; and the logits are closer to the quantised restatement than to quant=False."""
    from speech_distill_amd.generation import Decoder
    shp, w = _weights(9)
    m = _model(sda, w)
    ids, cont = _ids(T=70, seed=5)
    lens1, steps = [70, 64, 3, 33], 16
    for kernels in ("tile", "skinny"):
        dec = Decoder(m, B, 256, kernels, weight_dtype="mxfp8")
        out = [dec.extend(to_dev(ids), i32([0] * B), i32(lens1)).clone()]
        cont_d = cont.to(dev())
        for t in range(steps):
            out.append(dec.step(cont_d[:, t].contiguous(), i32([n + t for n in lens1]), max(lens1) + t + 1).clone())
        got = torch.stack(out).float().cpu()
        refs = {"q": [], "q_bf16": [], "noq": []}
        with torch.no_grad():
            for b in range(B):
                seq = torch.cat([ids[b, :lens1[b]], cont[b, :steps]])[None]
                at = torch.tensor([lens1[b] - 1] + [lens1[b] + t for t in range(steps)])
                if kernels == "tile":   # the references are computed once and shared
                    refs["q"].append(mx_ref.teacher_forward_mx(w, shp, seq)[0, at])
                    refs["q_bf16"].append(mx_ref.teacher_forward_mx(w, shp, seq, storage="bf16")[0, at])
                    refs["noq"].append(mx_ref.teacher_forward_mx(w, shp, seq, quant=False)[0, at])
        if kernels == "tile":
            ref, ref_bf16, noq = (torch.stack(refs[k], 1) for k in ("q", "q_bf16", "noq"))
            base = rel_err(ref_bf16, ref)[1]
        err, err_noq = rel_err(got, ref)[1], rel_err(got, noq)[1]
        print(f"mx generation {kernels}: rms err vs MX restatement {err:.4f}, budget base {base:.4f}, ratio "
              f"{err / base:.3f}; vs unquantised {err_noq:.4f}")
        record("mx_generation_vs_restatement", kernels=kernels, rms_err=err, base=base, ratio=err / base,
               rms_vs_unquantised=err_noq)
        assert err <= 1.5 * base
        assert err < err_noq


# ------------------------------------------------------------------------------------------------ 10: sessions
def _two_turns(m, kind, kernels="skinny", sync_every=16, seed=0, shuffle=True):
    ids, cont = _ids()
    sess = m.start_session(B, capacity=CAP, decode_kernels=kernels, pool=_pool(m, kind, seed, shuffle),
                           weight_dtype="mxfp8")
    kw = dict(max_new_tokens=12, do_sample=False, sync_every=sync_every)
    a = sess.generate(to_dev(ids), to_dev(_mask(CHUNK1, 256)), **kw)
    b = sess.generate(to_dev(cont[:, :12].contiguous()), to_dev(_mask(CHUNK2, 12)), **kw)
    out = torch.cat([a, b], 1).cpu()
    sess.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_session_tokens_do_not_depend_on_sync_every_or_the_page_order(model, kind):
    base = _two_turns(model, kind)
    assert base.shape == (B, 24)
    assert torch.equal(_two_turns(model, kind, sync_every=1, seed=3), base)
    if kind != "contig":
        assert torch.equal(_two_turns(model, kind, sync_every=5, shuffle=False), base)


def test_generate_takes_the_keyword_and_differs_from_bf16_weights_only_by_the_weights(model):
    """One-turn greedy generate: equals a one-turn session of the same kind, keeps the prompt, and runs the mx entries
    (the first new token is the arg-max of the mx prefill's logits)."""
    from speech_distill_amd.generation import Decoder
    ids, _ = _ids(T=40, seed=2)
    lens = [40, 17, 1, 33]
    am = to_dev(_mask(lens, 40))
    for kernels in ("tile", "skinny"):
        out = model.generate(to_dev(ids), attention_mask=am, max_new_tokens=6, do_sample=False, decode_kernels=kernels,
                             weight_dtype="mxfp8")
        assert out.shape == (B, 46) and torch.equal(out[:, :40].cpu(), ids)
        dec = Decoder(model, B, 256, kernels, weight_dtype="mxfp8")
        first = dec.prefill(to_dev(ids), i32(lens)).float().argmax(-1)
        assert torch.equal(out[:, 40], first)
        sess = model.start_session(B, capacity=256, decode_kernels=kernels, weight_dtype="mxfp8")
        assert torch.equal(sess.generate(to_dev(ids), am, max_new_tokens=6, do_sample=False), out[:, 40:])


def test_fork_continues_a_row_as_an_independent_session_does(model):
    ids, _ = _ids(T=320, seed=4)
    one = ids[:1]
    pool = _pool(model, "paged_mx", seed=5, n_pages=12)
    src = model.start_session(1, capacity=CAP, decode_kernels="skinny", pool=pool, weight_dtype="mxfp8")
    src.extend(to_dev(one[:, :300]))
    f = src.fork([0, 0, 0])
    assert f.weight_dtype == "mxfp8" and f.decoder.weight_dtype == "mxfp8"
    tok = to_dev(one[:, 300:301])
    g = f.generate(tok.expand(3, 1).contiguous(), max_new_tokens=8, do_sample=False).cpu()
    assert torch.equal(g[0], g[1]) and torch.equal(g[0], g[2])
    ind = model.start_session(1, capacity=CAP, decode_kernels="skinny", pool=pool, weight_dtype="mxfp8")
    ind.extend(to_dev(one[:, :300]))
    assert torch.equal(ind.generate(tok, max_new_tokens=8, do_sample=False).cpu()[0], g[0])
    f.close(), ind.close(), src.close()
    assert pool.pages_in_use == 0


def test_reloaded_or_moved_weights_are_the_ones_decoded_with(sda):
    """The decoder fetches the quantised weights on every call: after load_hf_state_dict a LIVE decoder computes what a
    decoder made after the reload computes (an extend behind past = 0 reads nothing the old weights cached), and a model
    built on the CPU and moved with .to() decodes like one built on the device."""
    from speech_distill_amd.generation import Decoder
    _, w = _weights(9)
    _, w2 = _weights(10)
    m = _model(sda, w)
    ids, _ = _ids(T=64, seed=6)
    lens = [64, 9, 30, 1]
    live = Decoder(m, B, 256, "skinny", weight_dtype="mxfp8")
    before = live.extend(to_dev(ids), i32([0] * B), i32(lens)).clone()
    m.load_hf_state_dict(w2)
    after = live.extend(to_dev(ids), i32([0] * B), i32(lens)).clone()
    fresh = Decoder(m, B, 256, "skinny", weight_dtype="mxfp8")
    assert torch.equal(after, fresh.extend(to_dev(ids), i32([0] * B), i32(lens)))
    assert not torch.equal(after, before)
    step_live = live.step(to_dev(ids[:, 0].contiguous()), i32(lens), max(lens) + 1).clone()
    assert torch.equal(step_live, fresh.step(to_dev(ids[:, 0].contiguous()), i32(lens), max(lens) + 1))
    moved = _model(sda, w2, device="cpu").to(dev())
    kw = dict(attention_mask=to_dev(_mask(lens, 64)), max_new_tokens=5, do_sample=False, decode_kernels="skinny",
              weight_dtype="mxfp8")
    assert torch.equal(moved.generate(to_dev(ids), **kw), m.generate(to_dev(ids), **kw))
