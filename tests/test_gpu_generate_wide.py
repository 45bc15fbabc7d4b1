"""-m gpu: generation with decode_kernels="wide" -- the decode step on the MFMA weight-streaming kernels
(sd_qwen3_decode_step_wide; speech_distill_amd/csrc/sd_gemv_wide.hip, sd_model.hip, generation.py).

Yardsticks: the fp32 oracle (oracle/qwen3.py) and the HIP full forward for the logits, the same call on one prompt for the
batch invariance, the unflagged step for the fallback and the default, and the step's launches composed by hand from the
public entries for the wiring over each cache kind."""
import pytest
import torch

import attn_ref as A
from gpu_util import dev, record
from test_gpu_generate import PROMPT_LENS, SHAPES, _mask, _model, _prompts, same_bits

pytestmark = pytest.mark.gpu

_MODELS = {}


def model(name):
    """_model(name), made once per shape and never changed."""
    if name not in _MODELS:
        _MODELS[name] = _model(name)
    return _MODELS[name]


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=dev())


# -------------------------------------------------------------------------------------------- 1. teacher-forced decode
@pytest.mark.parametrize("name", list(SHAPES))
def test_wide_teacher_forced_decode_within_the_full_forward_budget(name):
    """The criterion of test_teacher_forced_decode_within_the_full_forward_budget for the wide step: at every one of 64
    steps (B = 4, ragged prompts) the rms error of the logits against the fp32 oracle's full forward <= F_RMS x the rms
    error of the HIP full forward against the same oracle."""
    from oracle import qwen3 as Q
    from test_gpu_generate_skinny import _forced_logits
    m, shape, w = model(name)
    ids, cont = _prompts()
    steps = 64
    got = _forced_logits(m, ids, cont, PROMPT_LENS, steps, "wide").float().cpu()
    ora = torch.empty_like(got)
    hip = torch.empty_like(got)
    for b, n in enumerate(PROMPT_LENS):
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
    print(f"teacher-forced wide decode {name}: worst rms ratio cached / full forward = {worst:.3f}")
    record("decode_forced_wide", model=name, worst_ratio=worst)


# ------------------------------------------------------------------------------------------------ 2. batch invariance
def test_wide_generate_of_33_ragged_rows_equals_each_prompt_alone():
    """33 rows (three B tiles, the last with one row) whose lengths cycle through PROMPT_LENS: greedy and sampled with a
    seed, every row's new tokens are those of the prompt generated alone; and the tokens do not depend on sync_every."""
    m, _, _ = model("student")
    B = 33
    g = torch.Generator().manual_seed(33)
    ids = torch.randint(0, 640, (B, 24), generator=g)
    lens = [PROMPT_LENS[b % len(PROMPT_LENS)] for b in range(B)]
    am = _mask(lens, 24)
    junk = torch.where(am.bool(), ids, torch.full_like(ids, 639))   # the pad slots hold a token the rows never see
    greedy = dict(max_new_tokens=12, do_sample=False, decode_kernels="wide")
    out = m.generate(junk.to(dev()), attention_mask=am.to(dev()), **greedy).cpu()
    for b, n in enumerate(lens):
        alone = m.generate(ids[b:b + 1, :n].to(dev()), **greedy).cpu()
        assert torch.equal(alone[0, n:], out[b, 24:]), b
    # sampled with a seed (generate draws row b's uniforms from the batch's stream, so a lone call cannot repeat them: the
    # next test feeds them by hand): the tokens do not depend on how often the host looks at the finished flags
    sampled = dict(attention_mask=am.to(dev()), max_new_tokens=12, do_sample=True, top_k=20, temperature=0.9, seed=3,
                   eos_token_id=int(out[0, 26]), pad_token_id=2, decode_kernels="wide")
    assert torch.equal(m.generate(junk.to(dev()), sync_every=1, **sampled), m.generate(junk.to(dev()), sync_every=16, **sampled))


def test_wide_sampled_rows_equal_each_prompt_alone():
    """Sampled tokens row by row: 33 rows through one decoder and the sampler, against a one-row decoder per prompt that is
    fed the same uniforms u[:, b] (the sampler is row-wise; the wide step makes the logits so)."""
    from speech_distill_amd.generation import Decoder
    from speech_distill_amd.ops import sample_params, sample_step
    m, _, _ = model("student")
    B, steps = 33, 10
    g = torch.Generator().manual_seed(34)
    ids = torch.randint(0, 640, (B, 24), generator=g)
    lens = [PROMPT_LENS[b % len(PROMPT_LENS)] for b in range(B)]
    u = torch.rand(steps, B, 2, generator=g).to(dev())
    sp = sample_params(True, 0.9, 20, 1.0, 1.0, 0, None, 0, False, 25, 0.2)

    def run(rows):
        n = len(rows)
        dec = Decoder(m, n, 256, "wide")
        kv = i32([lens[b] for b in rows])
        logits = dec.prefill(ids[rows].to(dev()), kv)
        seq = torch.zeros(n, 256, dtype=torch.int64, device=dev())
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
    for b in range(B):
        assert torch.equal(run([b])[0], batch[b]), b


# ------------------------------------------------------------------------------------- 3. fallback and launch labels
def _one_step(m, B, decode_kernels, seed=11):
    from test_gpu_generate_skinny import _one_step as one
    return one(m, B, decode_kernels, seed)


def _count(launches, prefix):
    return sum(n for sym, n in launches.items() if sym.startswith(prefix))


@pytest.mark.parametrize("name", list(SHAPES))
def test_wide_step_falls_back_whole_at_65_rows_and_takes_the_wide_path_at_33(name):
    """B = 65: the wide step IS the tile step (same bits, no wide launch).  B = 33: 4 wide launches per layer + 1 for the
    final norm and lm_head, no separate RMSNorm, SwiGLU, tile GEMM or 16-row GEMV, 7 L + 2 launches in all."""
    m, _, _ = model(name)
    L = m.dims.num_hidden_layers
    wide65, sym65 = _one_step(m, 65, "wide")
    tile65, _ = _one_step(m, 65, "tile")
    assert same_bits(wide65, tile65) and _count(sym65, "wide_gemv_kernel") == 0
    _, wide33 = _one_step(m, 33, "wide")
    assert _count(wide33, "wide_gemv_kernel") == 4 * L + 1, wide33
    assert _count(wide33, "rmsnorm") == 0 and _count(wide33, "swiglu") == 0 and _count(wide33, "gemm") == 0, wide33
    assert _count(wide33, "gemv_kernel") == 0, wide33
    assert sum(wide33.values()) == 7 * L + 2, wide33
    _, tile33 = _one_step(m, 33, "tile")
    assert _count(tile33, "wide_gemv_kernel") == 0
    _, skinny4 = _one_step(m, 4, "skinny")
    assert _count(skinny4, "wide_gemv_kernel") == 0 and _count(skinny4, "gemv_kernel") == 4 * L + 1


# ------------------------------------------------------------------------------------------------- 4. cache kinds
B4, CAP, N_PAGES = 4, 512, 10
LENS4 = [250, 256, 3, 130]


class Hand:
    """The launches of sd_qwen3_decode_step_wide composed from the ops bindings over a pool of the hand's own (it reads
    the page table of the decoder it shadows: page numbers are pool-relative)."""

    def __init__(self, m, pool, table, mx):
        from speech_distill_amd import ops
        self.ops, self.m, self.mx, self.table = ops, m, mx, table
        d = m.dims
        self.Hq, self.Hkv, self.eps, self.L = d.num_attention_heads, d.num_key_value_heads, d.rms_norm_eps, d.num_hidden_layers
        self.cos, self.sin = m._tables(CAP, dev())
        self.planes = [pool.planes(l) for l in range(self.L)]

    def w(self, name):
        return self.m._params[name].data

    def step(self, ids, pos, max_len):
        ops, m = self.ops, self.m
        x = ops.embedding_fwd(ids, self.w("model.embed_tokens.weight"))
        for l in range(self.L):
            p = f"model.layers.{l}."
            wqkv = torch.cat([self.w(p + f"self_attn.{n}_proj.weight") for n in ("q", "k", "v")], 0)
            wgu = torch.cat([self.w(p + f"mlp.{n}_proj.weight") for n in ("gate", "up")], 0)
            qg, kg = self.w(p + "self_attn.q_norm.weight"), self.w(p + "self_attn.k_norm.weight")
            qkv = ops.gemv_bf16(x, wqkv, norm_gain=self.w(p + "input_layernorm.weight"), eps=self.eps, wide=True)
            pl = self.planes[l]
            if self.mx:
                q = ops.qknorm_rope_append_paged_mx(qkv, qg, kg, self.cos, self.sin, pos, pl, self.table, self.Hq, self.Hkv,
                                                    self.eps)
                ao = ops.attn_decode_paged_mx(q, pl, self.table, pos, self.Hq, self.Hkv, max_len=max_len, len_add=1)
            else:
                q = ops.qknorm_rope_append_paged(qkv, qg, kg, self.cos, self.sin, pos, *pl, self.table, self.Hq, self.Hkv,
                                                 self.eps)
                ao = ops.attn_decode_paged(q, *pl, self.table, pos, self.Hq, self.Hkv, max_len=max_len, len_add=1)
            x_mid = ops.gemv_bf16(ao, self.w(p + "self_attn.o_proj.weight"), residual=x, wide=True)
            act = ops.gemv_swiglu(x_mid, wgu, norm_gain=self.w(p + "post_attention_layernorm.weight"), eps=self.eps, wide=True)
            x = ops.gemv_bf16(act, self.w(p + "mlp.down_proj.weight"), residual=x_mid, wide=True)
        return ops.gemv_bf16(x, m.lm_head.weight.data, norm_gain=self.w("model.norm.weight"), eps=self.eps, wide=True)


def _pool(m, kind, seed):
    order = torch.randperm(N_PAGES, generator=torch.Generator().manual_seed(seed)).tolist()
    return m.kv_page_pool(N_PAGES, order=order, kv_dtype="mxfp8" if kind == "paged_mx" else "bf16")


def _ids4(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 640, (B4, 256), generator=g), torch.randint(0, 640, (B4, 8), generator=g)


@pytest.mark.parametrize("kind", ["paged", "paged_mx"])
def test_wide_step_over_pages_equals_the_hand_composed_launches(kind):
    """A ragged prefill, then 6 teacher-forced wide steps over one shuffled page layout: the entry's logits equal, bit for
    bit, the same launches composed by hand over a pool that received the same prefill."""
    from speech_distill_amd.generation import Decoder
    m, _, _ = model("twin")
    ids, cont = _ids4()
    dec = Decoder(m, B4, CAP, "wide", pool=_pool(m, kind, 1))
    dec.reserve([n + 8 for n in LENS4])
    dec.prefill(ids.to(dev()), i32(LENS4))
    hand_pool = _pool(m, kind, 1)
    hand_pool.buffer.copy_(dec.pool.buffer)          # the same cached rows on the same pages
    hand = Hand(m, hand_pool, dec.table, kind == "paged_mx")
    cont_d = cont.to(dev())
    for t in range(6):
        pos = i32([n + t for n in LENS4])
        got = dec.step(cont_d[:, t].contiguous(), pos, max(LENS4) + t + 1).clone()
        want = hand.step(cont_d[:, t].contiguous(), pos, max(LENS4) + t + 1)
        assert bool(torch.isfinite(got.float()).all())
        assert torch.equal(got, want), f"step {t}: {int((got != want).sum())} logits differ"
    dec.close()


def test_wide_logits_over_bf16_pages_equal_the_contiguous_cache():
    from speech_distill_amd.generation import Decoder
    m, _, _ = model("twin")
    ids, cont = _ids4(seed=2)
    paged = Decoder(m, B4, CAP, "wide", pool=_pool(m, "paged", 3))
    paged.reserve([n + 8 for n in LENS4])
    flat = Decoder(m, B4, CAP, "wide")
    assert torch.equal(paged.prefill(ids.to(dev()), i32(LENS4)), flat.prefill(ids.to(dev()), i32(LENS4)))
    cont_d = cont.to(dev())
    for t in range(6):
        pos = i32([n + t for n in LENS4])
        a = paged.step(cont_d[:, t].contiguous(), pos, max(LENS4) + t + 1)
        b = flat.step(cont_d[:, t].contiguous(), pos, max(LENS4) + t + 1)
        assert torch.equal(a, b), t
    paged.close()


# ---------------------------------------------------------------------------------------------------- 5. defaults
def test_wide_leaves_the_defaults_alone():
    from speech_distill_amd.generation import Decoder
    m, _, _ = model("student")
    ids, _ = _prompts()
    kw = dict(max_new_tokens=16, do_sample=True, top_k=50, temperature=0.8, seed=5)
    assert torch.equal(m.generate(ids.to(dev()), **kw), m.generate(ids.to(dev()), decode_kernels="tile", **kw))
    assert Decoder(m, 2, 16).flags == 0 and Decoder(m, 2, 16, "skinny").flags == 1
    assert not Decoder(m, 2, 16).wide and not Decoder(m, 2, 16, "skinny").wide and Decoder(m, 2, 16, "wide").wide
