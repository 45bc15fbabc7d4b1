"""-m gpu: KV-cache generation -- decode attention, cache append / store, prefill, decode steps, the sampler and
``generate`` (speech_distill_amd/csrc/sd_decode.hip, the two runner entries of sd_model.hip, generation.py).

Yardsticks: plain fp64 torch for the attention row, the existing kernels (sd_attn_fwd, sd_qknorm_rope_fwd, the full
forward) for what the new ones must equal or match, the fp32 oracle (oracle/qwen3.py) for the model, and the pure-torch
reference sampler tests/gen_ref.py for the tokens."""
import pytest
import torch

import attn_ref as A
import gen_ref as R
from gpu_util import dev, record

pytestmark = pytest.mark.gpu

D = 128
LENS16 = [0, 1, 255, 256, 257, 1000, 4096, 2, 31, 64, 511, 512, 513, 2048, 3000, 4095]
LENS = {1: [[4096], [257], [1000]], 3: [[257, 4096, 1], [0, 255, 256]], 16: [LENS16]}


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 1. decode attention
def _row_ref(q, k, v, lens, B, T, Hq, Hkv):
    """fp64 attention of ONE query row per sequence (the row lens[b] - 1 of q) over keys [0, lens[b]): [B, Hq, 128]."""
    G = Hq // Hkv
    out = torch.zeros(B, Hq, D, dtype=torch.float64)
    q3, k4, v4 = q.double().reshape(B, T, Hq, D), k.double().reshape(B, T, Hkv, D), v.double().reshape(B, T, Hkv, D)
    for b in range(B):
        n = lens[b]
        if n == 0:
            continue
        qb = q3[b, n - 1].reshape(Hkv, G, D)
        s = torch.einsum("hgd,nhd->hgn", qb, k4[b, :n]) * (D ** -0.5)
        p = torch.softmax(s, -1)
        out[b] = torch.einsum("hgn,nhd->hgd", p, v4[b, :n]).reshape(Hq, D)
    return out


def _inputs(kind, B, T, Hq, Hkv, seed):
    if kind == "randn":
        return A.randn_inputs(B, T, Hq, Hkv, seed)[:3]
    return A.ramp_inputs(B, T, Hq, Hkv, seed, +1 if kind == "rising" else -1, 0.25)[:3]


@pytest.mark.parametrize("kind", ["randn", "rising", "falling"])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("Hq,Hkv", [(16, 8), (4, 2), (2, 1)])
def test_decode_attention_against_fp64(ops, Hq, Hkv, B, kind):
    """Worst-row absolute error of sd_attn_decode against fp64 <= max(F_ROW x the worst-row error of sd_attn_fwd run on the
    same K / V with the query as the last row of a causal sequence of that length, 2^-8 x max|o_ref| of the row); bits
    identical across two runs, cap in {len_max, 2 len_max}, max_len hints in {len_max, cap}, and +-1e4 in the slots >= len."""
    for li, lens in enumerate(LENS[B]):
        T = max(max(lens), 1)
        q, k, v = _inputs(kind, B, T, Hq, Hkv, seed=100 * B + li)
        ref = _row_ref(q, k, v, lens, B, T, Hq, Hkv)
        qd, kd, vd = q.to(dev()), k.to(dev()), v.to(dev())
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
        # yardstick: the existing flash forward; row lens[b] - 1 of a causal sequence sees exactly keys [0, lens[b])
        o_full, _ = ops.attn_fwd(qd, kd, vd, B, T, Hq, Hkv, kv_len=lens_d)
        rows = torch.tensor([b * T + max(n, 1) - 1 for b, n in enumerate(lens)], device=dev())
        o_yard = o_full[rows].reshape(B, Hq, D).double().cpu()
        del o_full
        q_dec = qd[rows].contiguous()
        kp, vp = kd.view(B, T, Hkv * D), vd.view(B, T, Hkv * D)
        o, lse = ops.attn_decode(q_dec, kp, vp, lens_d, Hq, Hkv, max_len=T, want_lse=True)
        got = o.reshape(B, Hq, D).double().cpu()
        live = torch.tensor([n > 0 for n in lens])
        err_dec = (got - ref).abs().amax(-1)              # [B, Hq] worst column of every row
        err_yard = (o_yard - ref).abs().amax(-1)[live]
        ulp = 2.0 ** -8 * ref.abs().amax(-1)
        worst_yard = float(err_yard.max()) if bool(live.any()) else 0.0
        allow = torch.maximum(torch.full_like(ulp, A.F_ROW * worst_yard), ulp)
        print(f"decode attn Hq={Hq} Hkv={Hkv} B={B} {kind} lens={lens[:7]}: worst row err decode "
              f"{float(err_dec.max()):.3e}  sd_attn_fwd {worst_yard:.3e}")
        record("decode_attn", Hq=Hq, B=B, kind=kind, li=li, err_decode=float(err_dec.max()), err_attn_fwd=worst_yard)
        assert bool(torch.isfinite(got).all())
        assert bool((err_dec <= allow).all()), (float(err_dec.max()), worst_yard)
        for b, n in enumerate(lens):
            if n == 0:
                assert float(got[b].abs().max()) == 0.0 and bool(torch.isinf(lse[b]).all())
        # LSE of the live rows against fp64 (natural log)
        if bool(live.any()):
            G = Hq // Hkv
            for b, n in enumerate(lens):
                if n:
                    s = torch.einsum("hgd,nhd->hgn", q.double().reshape(B, T, Hkv, G, D)[b, n - 1],
                                     k.double().reshape(B, T, Hkv, D)[b, :n]) * (D ** -0.5)
                    want = torch.logsumexp(s, -1).reshape(Hq)
                    assert float((lse[b].double().cpu() - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))
        # determinism and independence of the launch geometry
        o2 = ops.attn_decode(q_dec, kp, vp, lens_d, Hq, Hkv, max_len=T)
        assert same_bits(o, o2)
        kp2 = torch.zeros(B, 2 * T, Hkv * D, dtype=torch.bfloat16, device=dev())
        vp2 = torch.zeros_like(kp2)
        kp2[:, :T], vp2[:, :T] = kp, vp
        for hint in (T, 2 * T):
            assert same_bits(o, ops.attn_decode(q_dec, kp2, vp2, lens_d, Hq, Hkv, max_len=hint))
        # masked slots may hold anything finite
        dead = torch.arange(2 * T, device=dev())[None, :] >= lens_d[:, None]
        sign = torch.where(torch.arange(Hkv * D, device=dev()) % 2 == 0, 1e4, -1e4).to(torch.bfloat16)
        kp2[dead], vp2[dead] = sign, -sign
        assert same_bits(o, ops.attn_decode(q_dec, kp2, vp2, lens_d, Hq, Hkv, max_len=2 * T))
        del kp2, vp2, qd, kd, vd


# ---------------------------------------------------------------------------------------------- 2. q/k norm + append
def test_qknorm_rope_append_equals_fwd_and_writes_only_its_slots(ops):
    g = torch.Generator().manual_seed(5)
    B, cap, Hq, Hkv = 6, 64, 4, 2
    nh = Hq + 2 * Hkv
    qkv = (torch.randn(B, nh * D, generator=g)).to(torch.bfloat16).to(dev())
    qg = (1 + 0.2 * torch.randn(D, generator=g)).to(torch.bfloat16).to(dev())
    kg = (1 + 0.2 * torch.randn(D, generator=g)).to(torch.bfloat16).to(dev())
    cos, sin = ops.rope_tables(cap, dev())
    pos_l = [0, 3, 63, 17, cap, 40]
    pos = torch.tensor(pos_l, dtype=torch.int32, device=dev())
    sentinel = torch.full((B, cap, Hkv * D), 0x7FC1, dtype=torch.int16, device=dev()).view(torch.bfloat16)
    kp, vp, want_k, want_v = sentinel.clone(), sentinel.clone(), sentinel.clone(), sentinel.clone()
    q = ops.qknorm_rope_append(qkv, qg, kg, cos, sin, pos, kp, vp, Hq, Hkv)
    for b, p in enumerate(pos_l):
        if p >= cap:
            continue
        x = torch.zeros(cap, nh * D, dtype=torch.bfloat16, device=dev())
        x[p] = qkv[b]
        qk = ops.qknorm_rope_fwd(x, qg, kg, cos, sin, cap, Hq, Hkv)
        assert same_bits(q[b], qk[p, :Hq * D]), b
        want_k[b, p] = qk[p, Hq * D:]
        want_v[b, p] = qkv[b, (Hq + Hkv) * D:]
    assert same_bits(kp, want_k) and same_bits(vp, want_v)   # the B written slots and nothing else; pos = cap: nothing


# ------------------------------------------------------------------------------------------------------- the models
SHAPES = {"student": (640, 128, 256, 2, 2, 1), "twin": (640, 256, 512, 2, 4, 2)}
PROMPT_LENS = [24, 17, 9, 1]


def _model(name):
    import speech_distill_amd as sda
    from oracle import qwen3 as Q
    shape = Q.Qwen3Shape(*SHAPES[name])
    w = {k: v.bfloat16().float() for k, v in Q.init_weights(shape, seed=1).items()}
    m = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*SHAPES[name]), device=dev(), init_std=0)
    m.load_hf_state_dict(w)
    return m, shape, w


def _prompts():
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 640, (4, 24), generator=g)
    cont = torch.randint(0, 640, (4, 64), generator=g)
    return ids, cont


def _mask(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)


# --------------------------------------------------------------------------------------------------------- 3. prefill
@pytest.mark.parametrize("name", list(SHAPES))
def test_prefill_equals_forward_and_fills_the_cache(name):
    from speech_distill_amd import qwen3 as HQ
    from speech_distill_amd.generation import Decoder
    m, shape, _ = _model(name)
    ids, _ = _prompts()
    B, T, cap = 4, 24, 40
    am = _mask(PROMPT_LENS, T)
    ids_d, kv_len = ids.to(dev()), torch.tensor(PROMPT_LENS, dtype=torch.int32, device=dev())
    rows = torch.tensor([b * T + n - 1 for b, n in enumerate(PROMPT_LENS)], device=dev())
    with torch.no_grad():
        want = m(input_ids=ids_d, attention_mask=am.to(dev()), logit_rows=rows).logits
    dec = Decoder(m, B, cap)
    SENT = 0x7FC1
    dec.cache.view(torch.int16).fill_(SENT)
    got = dec.prefill(ids_d, kv_len)
    assert same_bits(got, want)
    # the K / V an SD_SAVE_ALL forward keeps: layer l's qkv and qk buffers inside its activation set (sd_model.hip carve)
    _, acts = m._run_forward(ids_d, kv_len, save=HQ.SAVE_ALL)
    d = m.dims
    M, h, I, QD, KD = B * T, d.hidden_size, d.intermediate_size, d.q_dim, d.kv_dim

    def al(x):
        return (x + 255) // 256 * 256
    x, rstd, qkv_b, qk_b = al(M * h * 2), al(M * 4), al(M * (QD + 2 * KD) * 2), al(M * (QD + KD) * 2)
    per_layer = 4 * x + 2 * rstd + qkv_b + qk_b + al(M * QD * 2) + al(B * d.num_attention_heads * T * 4) + \
        al(M * 2 * I * 2) + al(M * I * 2)
    assert load_bytes(m, B, T) == d.num_hidden_layers * per_layer + 3 * x + rstd
    flat = acts.view(torch.bfloat16)
    for l in range(d.num_hidden_layers):
        o_qkv = (l * per_layer + 2 * x + rstd) // 2
        qkv = flat[o_qkv:o_qkv + M * (QD + 2 * KD)].view(B, T, QD + 2 * KD)
        o_qk = o_qkv + qkv_b // 2
        qk = flat[o_qk:o_qk + M * (QD + KD)].view(B, T, QD + KD)
        kp, vp = dec.planes(l)
        for b, n in enumerate(PROMPT_LENS):
            assert same_bits(kp[b, :n], qk[b, :n, QD:].contiguous()), (l, b)
            assert same_bits(vp[b, :n], qkv[b, :n, QD + KD:].contiguous()), (l, b)
            assert bool((kp[b, n:].contiguous().view(torch.int16) == SENT).all())
            assert bool((vp[b, n:].contiguous().view(torch.int16) == SENT).all())


def load_bytes(m, B, T):
    import ctypes as C
    from speech_distill_amd import load_lib
    return load_lib().sd_qwen3_acts_bytes(C.byref(m._cdims), B, T, 1)


# -------------------------------------------------------------------------------------------- 4. teacher-forced decode
def _forced_logits(m, ids, cont, lens, steps):
    """Logits of the prefill and of `steps` forced decode steps: [steps + 1, B, V]; entry 0 predicts cont[:, 0]."""
    from speech_distill_amd.generation import Decoder
    B, T = ids.shape
    dec = Decoder(m, B, T + steps)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev())
    out = [dec.prefill(ids.to(dev()), kv_len).clone()]
    cont_d = cont.to(dev())
    for t in range(steps):
        pos = (kv_len + t).contiguous()
        out.append(dec.step(cont_d[:, t].contiguous(), pos, max(lens) + t + 1).clone())
    return torch.stack(out)


@pytest.mark.parametrize("name", list(SHAPES))
def test_teacher_forced_decode_within_the_full_forward_budget(name):
    """At every step: rms error of the cached logits against the fp32 oracle's full forward <= F_RMS x the rms error of
    the existing HIP full forward on the same rows against the same oracle."""
    from oracle import qwen3 as Q
    m, shape, w = _model(name)
    ids, cont = _prompts()
    steps = 64
    got = _forced_logits(m, ids, cont, PROMPT_LENS, steps).float().cpu()      # [65, 4, V]
    ora = torch.empty_like(got)
    hip = torch.empty_like(got)
    for b, n in enumerate(PROMPT_LENS):
        seq = torch.cat([ids[b, :n], cont[b]])[None]                          # n + 64 tokens
        with torch.no_grad():
            lo = Q.forward(w, shape, seq)[0]                                  # fp32 oracle, every position
            lh = m(input_ids=seq.to(dev())).logits[0].float().cpu()
        ora[:, b] = lo[n - 1:n + steps]
        hip[:, b] = lh[n - 1:n + steps]
    worst = 0.0
    for t in range(steps + 1):
        e_c = float((got[t] - ora[t]).double().pow(2).mean().sqrt())
        e_h = float((hip[t] - ora[t]).double().pow(2).mean().sqrt())
        worst = max(worst, e_c / e_h)
        assert e_c <= A.F_RMS * e_h, (t, e_c, e_h)
    print(f"teacher-forced decode {name}: worst rms ratio cached / full forward = {worst:.3f}")
    record("decode_forced", model=name, worst_ratio=worst)


# ----------------------------------------------------------------------------------------------------------- 5. greedy
def _oracle_greedy(w, shape, ids, steps):
    from oracle import qwen3 as Q
    seq = ids.clone()
    margins = []
    with torch.no_grad():
        for _ in range(steps):
            last = Q.forward(w, shape, seq)[:, -1]
            top2 = torch.topk(last, 2).values
            margins.append(top2[:, 0] - top2[:, 1])
            seq = torch.cat([seq, last.argmax(-1, keepdim=True)], 1)
    return seq, torch.stack(margins)          # [4, T + steps], [steps, 4]


def _storage_error(w, shape, seq):
    from oracle import qwen3 as Q
    with torch.no_grad():
        return float((Q.forward(w, shape, seq, storage="bf16") - Q.forward(w, shape, seq)).abs().max())


@pytest.mark.parametrize("name", list(SHAPES))
def test_greedy_follows_the_oracle_where_the_margin_allows(name):
    """Teacher-forced along the oracle's own greedy continuation, the cached arg-max equals the oracle's at every step
    whose oracle top-2 margin is >= 4 E (E = worst |logit| error of the oracle's bf16-storage run against fp32 on that
    sequence); steps under the margin are skipped.  At most 5 % of the 256 steps may be skipped on the smoke model
    (640, 128, 256, 2, 2, 1): there the fp32 oracle ALONE, on the CPU, leaves out 3 (E = 0.0067, margin median 0.217).  On
    the (640, 256, 512, 2, 4, 2) twin the oracle alone already leaves out 13 of 256 = 5.08 % (E = 0.0095, median 0.411;
    a property of those weights and prompts, computed without any HIP code), so the cap cannot be asked of it; the twin
    keeps the arg-max check on its 243 decided steps."""
    m, shape, w = _model(name)
    ids, _ = _prompts()
    steps = 64
    seq, margins = _oracle_greedy(w, shape, ids, steps)
    E = _storage_error(w, shape, seq)
    cont = seq[:, 24:]
    got = _forced_logits(m, ids, cont, [24] * 4, steps - 1).float()           # 64 predictions per row
    pred = got.argmax(-1).cpu()                                                # [64, 4]
    decided = margins >= 4 * E
    skipped = int((~decided).sum())
    print(f"greedy {name}: E = {E:.4f}, margin median {float(margins.median()):.3f}, skipped {skipped} of {margins.numel()}")
    record("decode_greedy", model=name, E=E, skipped=skipped)
    if name == "student":
        assert skipped <= 0.05 * margins.numel()
    assert int(decided.sum()) >= 0.9 * margins.numel()
    assert bool((pred == cont.T)[decided].all())


@pytest.mark.parametrize("name", list(SHAPES))
def test_generate_greedy_tokens_are_within_the_margin_of_the_full_forward(name):
    from oracle import qwen3 as Q
    m, shape, w = _model(name)
    ids, _ = _prompts()
    out = m.generate(ids.to(dev()), max_new_tokens=64, do_sample=False).cpu()
    assert out.shape == (4, 88) and torch.equal(out[:, :24], ids)
    E = _storage_error(w, shape, out)
    with torch.no_grad():
        full = Q.forward(w, shape, out)                                        # [4, 88, V]
    at = full[:, 23:87]                                                        # the rows that predict columns 24 .. 87
    chosen = at.gather(-1, out[:, 24:, None])[..., 0]
    gap = at.amax(-1) - chosen
    print(f"generate greedy {name}: E = {E:.4f}, worst gap to the row maximum {float(gap.max()):.4f}")
    assert float(gap.max()) <= 4 * E


# ---------------------------------------------------------------------------------------------------------- 6. sampler
VOCAB = 159488


def _state(prompts, gens, cap):
    B = len(prompts)
    seq = torch.zeros(B, cap, dtype=torch.int64)
    for b in range(B):
        row = prompts[b] + gens[b]
        seq[b, :len(row)] = torch.tensor(row, dtype=torch.int64)
    pl = torch.tensor([len(p) for p in prompts], dtype=torch.int32)
    ln = torch.tensor([len(p) + len(g) for p, g in zip(prompts, gens)], dtype=torch.int32)
    return seq, pl, ln


def _run_sampler(ops, logits, prompts, gens, finished, u, p, cap=128):
    seq, pl, ln = _state(prompts, gens, cap)
    seq_d, pl_d, ln_d = seq.to(dev()), pl.to(dev()), ln.to(dev())
    fin_d = torch.tensor(finished, dtype=torch.uint8, device=dev())
    sp = ops.sample_params(p.do_sample, p.temperature, p.top_k, p.top_p, p.repetition_penalty, p.min_new_tokens,
                           p.eos_token_id, p.pad_token_id, p.use_ras, p.win_size, p.tau_r)
    lg = logits.to(dev())
    keep = lg.clone()
    nxt, pos = ops.sample_step(lg, torch.tensor(u, dtype=torch.float32, device=dev()), seq_d, pl_d, ln_d, fin_d, sp)
    torch.cuda.synchronize()
    assert same_bits(lg, keep)               # the raw logits survive
    return nxt.cpu(), pos.cpu(), seq_d.cpu(), ln_d.cpu(), fin_d.cpu(), (seq, ln)


def _ref_step(logits, prompts, gens, finished, u, p):
    seqs = [list(a) + list(b) for a, b in zip(prompts, gens)]
    fin = list(finished)
    toks, infos = R.step(logits.float(), seqs, [len(a) for a in prompts], fin, u, p)
    return toks, seqs, fin, infos


def _choose_uniforms(logits, prompts, gens, finished, p, seed):
    """u[b] = (u0, u1) at least 1e-5 away from every boundary of the fp64 CDF over the candidates (128 * 2^-24 rounded
    up), and 1e-3 away for the full-vocabulary draw (the blocked fp32 sum's bound)."""
    g = torch.Generator().manual_seed(seed)
    us = []
    for b in range(len(prompts)):
        if finished[b] or not p.do_sample:
            us.append((0.5, 0.5))
            continue
        seq_row = list(prompts[b]) + list(gens[b])
        ids, pr, ci = R.candidates(logits[b].float(), gens[b], p)
        assert ci["top_p_margin"] >= 1e-5, "test input: a top-p decision sits on its boundary"
        u0 = R.pick_uniform(R.cdf(pr), g, 1e-5)
        _, info = R.sample_row(logits[b].float(), seq_row, len(prompts[b]), u0, 0.5, p)
        u1 = R.pick_uniform(info["cdf_final"], g, 1e-3 if info["ras"] else 1e-5)
        us.append((u0, u1))
    return us


def _check_step(ops, logits, prompts, gens, finished, p, seed):
    u = _choose_uniforms(logits, prompts, gens, finished, p, seed)
    toks, seqs, fin, infos = _ref_step(logits, prompts, gens, finished, u, p)
    nxt, pos, seq_d, ln_d, fin_d, (seq0, ln0) = _run_sampler(ops, logits, prompts, gens, finished, u, p)
    assert nxt.tolist() == toks, (nxt.tolist(), toks)
    for b in range(len(prompts)):
        if finished[b]:
            assert int(ln_d[b]) == int(ln0[b]) and torch.equal(seq_d[b], seq0[b]) and int(fin_d[b]) == 1
        else:
            assert int(ln_d[b]) == len(seqs[b]) and seq_d[b, :len(seqs[b])].tolist() == seqs[b]
            assert int(pos[b]) == len(seqs[b]) - 1 and bool(fin_d[b]) == fin[b]
    return toks, infos


def _logits(B, seed, scale=4.0):  # (scale 4: a few tokens hold several per cent of the mass each)
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(B, VOCAB, generator=g)).to(torch.bfloat16)


def _history(logits, b, n_prompt, n_gen, seed):
    """A prompt and a generated part that touch the row's largest logits, so that the penalty changes the candidates."""
    g = torch.Generator().manual_seed(seed)
    top = torch.topk(logits[b].float(), 8).indices.tolist()
    prompt = torch.randint(0, VOCAB, (n_prompt,), generator=g).tolist()
    gen = torch.randint(0, VOCAB, (n_gen,), generator=g).tolist()
    if n_gen >= 3:
        gen[0], gen[1], gen[2] = top[0], top[0], top[3]
    prompt[0] = top[1]
    return prompt, gen


def test_sampler_greedy_and_default_parameters_equal_the_reference(ops):
    B = 4
    logits = _logits(B, 21)
    hist = [_history(logits, b, 6 + b, 5 + 2 * b, 50 + b) for b in range(B)]
    prompts, gens = [h[0] for h in hist], [h[1] for h in hist]
    greedy = R.Params(do_sample=False, repetition_penalty=1.25, pad_token_id=1)
    _check_step(ops, logits, prompts, gens, [False] * B, greedy, 1)
    plain = R.Params(do_sample=False, pad_token_id=1)
    toks, _ = _check_step(ops, logits, prompts, gens, [False] * B, plain, 1)
    assert toks == logits.float().argmax(-1).tolist()
    default = R.Params(**{**R.REFERENCE, "use_ras": False}, pad_token_id=1)
    for seed in (2, 3, 4):
        _check_step(ops, logits, prompts, gens, [False] * B, default, seed)
    for extra in (dict(top_p=1.0), dict(top_k=1), dict(repetition_penalty=1.0), dict(top_k=128, temperature=1.0)):
        _check_step(ops, logits, prompts, gens, [False] * B, R.Params(**{**R.REFERENCE, "use_ras": False, **extra}), 5)


def test_sampler_full_vocabulary_draw_equals_the_reference(ops):
    """top_k = 0: the whole processed row is the distribution (blocked fp32 sums, uniforms 1e-3 from the boundaries)."""
    B = 3
    logits = _logits(B, 23)
    hist = [_history(logits, b, 5, 4, 70 + b) for b in range(B)]
    prompts, gens = [h[0] for h in hist], [h[1] for h in hist]
    p = R.Params(do_sample=True, temperature=0.8, top_k=0, top_p=1.0, repetition_penalty=1.25)
    g = torch.Generator().manual_seed(9)
    us = []
    for b in range(B):
        ids, pr, _ = R.candidates(logits[b].float(), gens[b], p)
        us.append((0.5, R.pick_uniform(R.cdf(pr), g, 1e-3)))
    toks, seqs, fin, _ = _ref_step(logits, prompts, gens, [False] * B, us, p)
    nxt = _run_sampler(ops, logits, prompts, gens, [False] * B, us, p)[0]
    assert nxt.tolist() == toks


def test_sampler_ras_rows_in_one_batch(ops):
    """Row 0: the candidate X sits 4 times in the last 25 tokens (5 >= 25 * 0.2): the final draw is from the raw softmax.
    Row 1: 3 times: processed distribution.  Row 2: the 4 occurrences reach into the prompt.  Row 3: no repetition.
    Rows 0-2 carry two heavy tokens, X (penalised, still the largest processed score) and Y, and u1 is chosen where the raw
    and the processed distribution give DIFFERENT tokens, so that a draw from the wrong one shows."""
    B, X, Y = 4, 4242, 100000
    logits = _logits(B, 22, scale=2.0)
    logits[:3, X], logits[:3, Y] = 14.0, 13.0
    filler = list(range(1000, 1040))

    def with_x(n, count):
        row = filler[:n]
        row[0] = Y
        for i in range(count):
            row[n - 1 - 3 * i] = X
        return row
    prompts = [filler[:5], filler[:5], [X, X, X, 7, 8], filler[:9]]
    gens = [with_x(30, 4), with_x(30, 3), [Y, X, 11], filler[10:20]]
    p = R.Params(**R.REFERENCE, pad_token_id=1)
    us = []
    for b in range(B):
        lf = logits[b].float()
        ids, pr, ci = R.candidates(lf, gens[b], p)
        assert ci["top_p_margin"] >= 1e-5
        c_proc, c_raw = R.cdf(pr), R.cdf(torch.softmax(lf.double(), -1))
        u0 = 0.3 if b < 3 else 0.5
        assert R.boundary_distance(c_proc, u0) >= 1e-5 and (b == 3 or R.draw(ids, pr, u0) == X)
        grid = [float(torch.tensor(0.05 + 0.01 * i, dtype=torch.float32)) for i in range(90)]
        ok = [u for u in grid if R.boundary_distance(c_proc, u) >= 1e-5 and (b == 3 or (
            R.boundary_distance(c_raw, u) >= 1e-3 and R.draw(ids, pr, u) != R.draw(torch.arange(VOCAB), c_raw.diff(
                prepend=torch.zeros(1, dtype=torch.float64)), u)))]
        assert ok, "test input: no uniform separates the raw from the processed distribution"
        us.append((u0, ok[len(ok) // 2]))
    toks, seqs, fin, infos = _ref_step(logits, prompts, gens, [False] * B, us, p)
    assert [i["ras"] for i in infos] == [True, False, True, False]
    nxt, pos, seq_d, ln_d, fin_d, _ = _run_sampler(ops, logits, prompts, gens, [False] * B, us, p)
    assert nxt.tolist() == toks, (nxt.tolist(), toks)
    assert ln_d.tolist() == [len(x) for x in seqs]


def test_sampler_finished_rows_and_eos(ops):
    B, EOS, PAD = 4, 77, 3
    logits = _logits(B, 24)
    logits[:, EOS] = 60.0                     # EOS is the arg-max of every row
    prompts = [[5, 6, 7]] * B
    gens = [[10, 11], [10, 11, 12, 13], [10], [10, 11, 12, 13, 14]]
    p = R.Params(do_sample=False, min_new_tokens=4, eos_token_id=EOS, pad_token_id=PAD)
    finished = [False, False, True, False]
    toks, _ = _check_step(ops, logits, prompts, gens, finished, p, 1)
    assert toks[0] != EOS and toks[1] == EOS and toks[2] == PAD and toks[3] == EOS   # suppressed / honoured / pad
    ps = R.Params(**{**R.REFERENCE, "use_ras": False}, min_new_tokens=4, eos_token_id=EOS, pad_token_id=PAD)
    toks, _ = _check_step(ops, logits, prompts, gens, finished, ps, 2)
    assert toks[0] != EOS and toks[2] == PAD


# ------------------------------------------------------------------------------------------------- 7. generate, whole
def test_generate_is_reproducible_and_independent_of_sync_every():
    m, _, _ = _model("student")
    ids, _ = _prompts()
    am = _mask(PROMPT_LENS, 24)
    kw = dict(attention_mask=am.to(dev()), max_new_tokens=40, eos_token_id=5, pad_token_id=2, **R.REFERENCE)
    a = m.generate(ids.to(dev()), seed=123, **kw)
    b = m.generate(ids.to(dev()), seed=123, **kw)
    c = m.generate(ids.to(dev()), seed=124, **kw)
    assert a.shape == (4, 64) and torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(a[:, :24].cpu(), ids)
    for se in (1, 3):
        assert torch.equal(a, m.generate(ids.to(dev()), seed=123, sync_every=se, **kw))
    # after a row's EOS everything is pad
    new = a[:, 24:].cpu()
    for b_ in range(4):
        hit = (new[b_] == 5).nonzero()
        if hit.numel():
            assert bool((new[b_, int(hit[0]) + 1:] == 2).all())
    # a short vocabulary of likely tokens makes every row hit EOS early: the early exit returns the same tokens
    kw2 = dict(attention_mask=am.to(dev()), max_new_tokens=48, eos_token_id=int(a[0, 24]), pad_token_id=2, do_sample=True,
               top_k=2, temperature=1.5, seed=7)
    assert torch.equal(m.generate(ids.to(dev()), sync_every=1, **kw2), m.generate(ids.to(dev()), sync_every=16, **kw2))


def test_generate_batch_of_ragged_prompts_equals_each_prompt_alone():
    m, _, _ = _model("student")
    ids, _ = _prompts()
    am = _mask(PROMPT_LENS, 24)
    junk = torch.where(am.bool(), ids, torch.full_like(ids, 639))   # the pad slots hold a token the rows never see
    out = m.generate(junk.to(dev()), attention_mask=am.to(dev()), max_new_tokens=32, do_sample=False).cpu()
    for b, n in enumerate(PROMPT_LENS):
        alone = m.generate(ids[b:b + 1, :n].to(dev()), max_new_tokens=32, do_sample=False).cpu()
        assert torch.equal(alone[0, n:], out[b, 24:]), b


def test_generate_host_side_errors():
    m, _, _ = _model("student")
    ids = torch.zeros(2, 8, dtype=torch.int64, device=dev())
    bad = torch.tensor([[1, 1, 0, 1, 1, 1, 1, 1], [1] * 8], device=dev())
    with pytest.raises(ValueError, match="not right-padded"):
        m.generate(ids, attention_mask=bad, max_new_tokens=2)
    m.kv_cache_capacity = 12
    with pytest.raises(ValueError, match="capacity"):
        m.generate(ids, max_new_tokens=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(ids.cpu(), max_new_tokens=2)
