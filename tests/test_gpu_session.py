"""-m gpu: multi-turn generation over one live KV cache -- ``GenerationSession`` (generation.py) over sd_qwen3_extend.

Yardsticks: the fp32 oracle's full forward (oracle/qwen3.py) with the existing HIP full forward as the error budget, and
``model.generate`` for what a one-turn session must equal bit for bit."""
import pytest
import torch

import attn_ref as A
import gen_ref as R
from gpu_util import dev, record
from test_gpu_generate import PROMPT_LENS, SHAPES, _mask, _model, _prompts, _storage_error

pytestmark = pytest.mark.gpu

SENT = 0x7FC1
CHUNK_LENS = [24, 17, 10, 9]      # every row has at least one token in each extend call it takes part in
TURN2_LENS = [12, 7, 1, 3]


# ----------------------------------------------------------------------------------------------- 6. chunked prefill
@pytest.mark.parametrize("name", list(SHAPES))
def test_chunked_prefill_within_the_full_forward_budget(name):
    """The ragged prompts go through sess.extend in two calls (9, then 15 columns; the row of 9 tokens sits the second
    out), then 64 teacher-forced decode steps.  Everywhere: rms error of the cached logits against the fp32 oracle's
    full forward <= F_RMS x the rms error of the existing HIP full forward on the same rows (the rule of
    test_teacher_forced_decode_within_the_full_forward_budget).  Cache slots >= len keep their sentinel."""
    from oracle import qwen3 as Q
    m, shape, w = _model(name)
    ids, cont = _prompts()
    steps, B = 64, 4
    sess = m.start_session(B, capacity=96)
    sess.decoder.cache.view(torch.int16).fill_(SENT)
    first = sess.extend(ids[:, :9].to(dev()))
    assert sess.lengths().tolist() == [9] * 4
    second = sess.extend(ids[:, 9:].to(dev()), _mask([n - 9 for n in CHUNK_LENS], 15).to(dev()))
    assert sess.lengths().tolist() == CHUNK_LENS
    got = [torch.stack([second[0], second[1], second[2], first[3]]).float().cpu()]
    for l in range(m.dims.num_hidden_layers):
        for plane in sess.decoder.planes(l):
            for b, n in enumerate(CHUNK_LENS):
                assert bool((plane[b, n:].contiguous().view(torch.int16) == SENT).all()), (l, b)
                assert not bool((plane[b, :n].contiguous().view(torch.int16) == SENT).all()), (l, b)
    lens = torch.tensor(CHUNK_LENS, dtype=torch.int32, device=dev())
    cont_d = cont.to(dev())
    for t in range(steps):
        got.append(sess.decoder.step(cont_d[:, t].contiguous(), (lens + t).contiguous(), max(CHUNK_LENS) + t + 1)
                   .float().cpu())
    got = torch.stack(got)                                                     # [65, 4, V]
    for l in range(m.dims.num_hidden_layers):
        for plane in sess.decoder.planes(l):
            for b, n in enumerate(CHUNK_LENS):
                assert bool((plane[b, n + steps:].contiguous().view(torch.int16) == SENT).all()), (l, b)
    ora, hip = torch.empty_like(got), torch.empty_like(got)
    for b, n in enumerate(CHUNK_LENS):
        seq = torch.cat([ids[b, :n], cont[b]])[None]
        with torch.no_grad():
            lo = Q.forward(w, shape, seq)[0]
            lh = m(input_ids=seq.to(dev())).logits[0].float().cpu()
        ora[:, b] = lo[n - 1:n + steps]
        hip[:, b] = lh[n - 1:n + steps]
    worst = 0.0
    for t in range(steps + 1):
        e_c = float((got[t] - ora[t]).double().pow(2).mean().sqrt())
        e_h = float((hip[t] - ora[t]).double().pow(2).mean().sqrt())
        worst = max(worst, e_c / e_h)
        assert e_c <= A.F_RMS * e_h, (t, e_c, e_h)
    print(f"chunked prefill {name}: worst rms ratio session / full forward = {worst:.3f} (entry 0: the two extend calls)")
    record("session_chunked", model=name, worst_ratio=worst)


def test_extend_rotates_at_past_plus_t_bit_for_bit():
    """Layer 0's K (normalised + rotated) and V rows depend on the token and its position only: 25 tokens cached as 1 + 24
    (the 24 through sd_qwen3_extend, RoPE rows gathered at past + t on the device) hold the bits a one-shot prefill of the
    25 leaves in slots 0 .. 24; with ragged second chunks only the slots below each row's length are written."""
    m, _, _ = _model("student")
    ids, cont = _prompts()
    toks = torch.cat([ids, cont[:, :1]], 1).to(dev())                          # [4, 25]
    whole = m.start_session(4, capacity=32)
    whole.extend(toks)
    lens = [25, 18, 2, 10]
    parts = m.start_session(4, capacity=32)
    parts.decoder.cache.view(torch.int16).fill_(SENT)
    parts.extend(toks[:, :1].contiguous())
    parts.extend(toks[:, 1:].contiguous(), _mask([n - 1 for n in lens], 24).to(dev()))
    assert parts.lengths().tolist() == lens
    for a, b in zip(whole.decoder.planes(0), parts.decoder.planes(0)):
        for r, n in enumerate(lens):
            assert torch.equal(a[r, :n].contiguous().view(torch.int16), b[r, :n].contiguous().view(torch.int16)), r
            assert bool((b[r, n:].contiguous().view(torch.int16) == SENT).all()), r


# ------------------------------------------------------------------------------------------ 7. one turn = generate()
def test_one_turn_session_equals_generate_bit_for_bit():
    m, _, _ = _model("student")
    ids, _ = _prompts()
    am = _mask(PROMPT_LENS, 24).to(dev())
    kw = dict(attention_mask=am, max_new_tokens=40, eos_token_id=5, pad_token_id=2, seed=123, **R.REFERENCE)
    want = m.generate(ids.to(dev()), **kw)[:, 24:]
    sess = m.start_session(4, capacity=256)
    assert torch.equal(sess.generate(ids.to(dev()), **kw), want)
    sess.reset()
    assert sess.lengths().tolist() == [0] * 4
    assert torch.equal(sess.generate(ids.to(dev()), **kw), want)
    # a session of another capacity, and the default one of the model
    m.kv_cache_capacity = 512
    assert torch.equal(m.start_session(4).generate(ids.to(dev()), **kw), want)


# ------------------------------------------------------------------------------------------------- 8 / 9. two turns
_TURNS = {}


def _two_turns(name, eos=None):
    """Greedy: the ragged prompts + 32 new tokens, then 12 / 7 / 1 / 3 more given tokens per row + 32 new tokens."""
    key = (name, eos)
    if key not in _TURNS:
        m, shape, w = _model(name)
        ids, cont = _prompts()
        sess = m.start_session(4, capacity=128)
        kw = dict(max_new_tokens=32, do_sample=False, eos_token_id=eos, pad_token_id=639)
        new1 = sess.generate(ids.to(dev()), _mask(PROMPT_LENS, 24).to(dev()), **kw).cpu()
        mid = sess.lengths().tolist()
        new2 = sess.generate(cont[:, :12].to(dev()), _mask(TURN2_LENS, 12).to(dev()), **kw).cpu()
        _TURNS[key] = dict(shape=shape, w=w, ids=ids, cont=cont, new1=new1, new2=new2, mid=mid,
                           lengths=sess.lengths().tolist(), tokens=[t.cpu() for t in sess.tokens()])
    return _TURNS[key]


def _cut(row, eos):
    row = row.tolist()
    return row[:row.index(eos) + 1] if eos is not None and eos in row else row


def _check_margin(r, eos, turns):
    """On each row's whole sequence: the oracle's logit of every generated token of ``turns`` is within 4 E of the row
    maximum, E = the oracle's bf16-storage error on that sequence."""
    from oracle import qwen3 as Q
    worst = 0.0
    for b, p in enumerate(PROMPT_LENS):
        g1, g2 = _cut(r["new1"][b], eos), _cut(r["new2"][b], eos)
        given = r["cont"][b, :TURN2_LENS[b]].tolist()
        want = r["ids"][b, :p].tolist() + g1 + given + g2
        assert r["tokens"][b].tolist() == want, b                      # no pad inside, the EOS kept, the order right
        assert r["lengths"][b] == len(want) and r["mid"][b] == p + len(g1)
        seq = r["tokens"][b][None]
        E = _storage_error(r["w"], r["shape"], seq)
        with torch.no_grad():
            full = Q.forward(r["w"], r["shape"], seq)[0]
        spans = {1: range(p, p + len(g1)), 2: range(p + len(g1) + len(given), len(want))}
        for turn in turns:
            for i in spans[turn]:
                gap = float(full[i - 1].max() - full[i - 1, want[i]])
                worst = max(worst, gap / E)
                assert gap <= 4 * E, (b, turn, i, gap, E)
    return worst


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_greedy_turns_are_within_the_margin_of_the_full_forward(name):
    r = _two_turns(name)
    assert r["new1"].shape == (4, 32) and r["new2"].shape == (4, 32)
    worst = _check_margin(r, None, (1, 2))
    print(f"two greedy turns {name}: worst gap to the row maximum = {worst:.3f} E (allowed 4 E)")
    record("session_two_turns", model=name, worst_gap_over_E=worst)


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_turn_after_eos_continues_behind_the_eos(name):
    """eos = the token row 0 produced at step 3 of the greedy turn 1: row 0 finishes early and its EOS slot is rewritten by
    the pad steps.  After turn 2 its sequence is prompt + its tokens up to the EOS + its turn-2 tokens + new, with no pad
    inside, and the turn-2 tokens of every row are within the margin."""
    eos = int(_two_turns(name)["new1"][0, 3])
    r = _two_turns(name, eos)
    row0 = r["new1"][0].tolist()
    n0 = row0.index(eos) + 1
    assert n0 <= 4 and row0[:n0] == _two_turns(name)["new1"][0, :n0].tolist() and set(row0[n0:]) == {639}
    worst = _check_margin(r, eos, (2,))
    record("session_after_eos", model=name, worst_gap_over_E=worst)


# ------------------------------------------------------------------------------------------- 10. sync_every and seed
def test_two_sampled_turns_are_reproducible_and_independent_of_sync_every():
    m, _, _ = _model("student")
    ids, cont = _prompts()

    def run(seed, sync_every):
        sess = m.start_session(4, capacity=128)
        kw = dict(max_new_tokens=24, eos_token_id=5, pad_token_id=2, sync_every=sync_every, **R.REFERENCE)
        a = sess.generate(ids.to(dev()), _mask(PROMPT_LENS, 24).to(dev()), seed=seed, **kw)
        b = sess.generate(cont[:, :12].to(dev()), _mask(TURN2_LENS, 12).to(dev()), seed=seed + 1, **kw)
        return torch.cat([a, b], 1).cpu(), sess.lengths().tolist()
    base, lens = run(123, 16)
    for se in (1, 3):
        got, l2 = run(123, se)
        assert torch.equal(got, base) and l2 == lens, se
    again, _ = run(123, 16)
    other, _ = run(124, 16)
    assert torch.equal(again, base) and not torch.equal(other, base)


# ---------------------------------------------------------------------------------------------------- 11. host errors
def test_session_host_side_errors():
    m, _, _ = _model("student")
    ids, cont = _prompts()
    sess = m.start_session(4, capacity=40)
    sess.generate(ids[:, :8].to(dev()), max_new_tokens=4, do_sample=False)
    cache = sess.decoder.cache.clone()
    seq, lens = sess.seq.clone(), sess.lengths()
    with pytest.raises(ValueError, match="capacity"):
        sess.generate(cont[:, :12].to(dev()), max_new_tokens=32, do_sample=False)   # 12 + 12 + 32 > 40
    with pytest.raises(ValueError, match="holds 4 rows"):
        sess.generate(cont[:2, :4].to(dev()), max_new_tokens=2)
    bad = torch.tensor([[1, 0, 1, 1]] + [[1] * 4] * 3, device=dev())
    with pytest.raises(ValueError, match="not right-padded"):
        sess.generate(cont[:, :4].to(dev()), bad, max_new_tokens=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sess.generate(cont[:, :4], max_new_tokens=2)
    torch.cuda.synchronize()
    assert torch.equal(sess.decoder.cache, cache) and torch.equal(sess.seq, seq) and torch.equal(sess.lengths(), lens)
    sess.generate(cont[:, :4].to(dev()), max_new_tokens=2, do_sample=False)           # the session is still usable
    assert sess.lengths().tolist() == [18] * 4
    # a fresh row given an empty input has nothing to continue from
    sess.reset([1])
    assert sess.lengths().tolist() == [18, 0, 18, 18]
    empty = torch.tensor([[1, 1], [0, 0], [1, 0], [1, 1]], device=dev())
    with pytest.raises(ValueError, match="at least one token"):
        sess.generate(cont[:, :2].to(dev()), empty, max_new_tokens=2)
    fresh = m.start_session(4, capacity=40)
    with pytest.raises(ValueError, match="at least one token"):
        fresh.extend(cont[:, :2].to(dev()), empty)
    m.inference_precision = "mxfp8"   # what set_inference_precision("mxfp8") leaves on a model that supports it
    with pytest.raises(NotImplementedError, match="mxfp8"):
        m.start_session(4, capacity=40)
