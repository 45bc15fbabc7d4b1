"""-m gpu: generation with decode_kernels="skinny" -- the decode step on the weight-streaming GEMV kernels
(sd_qwen3_decode_step_flags with SD_DECODE_SKINNY; speech_distill_amd/csrc/sd_gemv.hip, sd_model.hip, generation.py).

Yardsticks: the fp32 oracle (oracle/qwen3.py) and the HIP full forward for the logits, the same call on one prompt for
the batch invariance, and the unflagged step for the fallback and the default."""
import pytest
import torch

import attn_ref as A
from gpu_util import dev, record
from test_gpu_generate import PROMPT_LENS, SHAPES, _mask, _model, _prompts, same_bits

pytestmark = pytest.mark.gpu


def _forced_logits(m, ids, cont, lens, steps, decode_kernels):
    """_forced_logits of test_gpu_generate.py with the decoder's kernels chosen: [steps + 1, B, V]."""
    from speech_distill_amd.generation import Decoder
    B, T = ids.shape
    dec = Decoder(m, B, T + steps, decode_kernels=decode_kernels)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev())
    out = [dec.prefill(ids.to(dev()), kv_len).clone()]
    cont_d = cont.to(dev())
    for t in range(steps):
        pos = (kv_len + t).contiguous()
        out.append(dec.step(cont_d[:, t].contiguous(), pos, max(lens) + t + 1).clone())
    return torch.stack(out)


# -------------------------------------------------------------------------------------------- 7. teacher-forced decode
@pytest.mark.parametrize("name", list(SHAPES))
def test_skinny_teacher_forced_decode_within_the_full_forward_budget(name):
    """The criterion of test_teacher_forced_decode_within_the_full_forward_budget for the skinny step: at every one of 64
    steps (B = 4, ragged prompts) the rms error of the logits against the fp32 oracle's full forward <= F_RMS x the rms
    error of the HIP full forward against the same oracle."""
    from oracle import qwen3 as Q
    m, shape, w = _model(name)
    ids, cont = _prompts()
    steps = 64
    got = _forced_logits(m, ids, cont, PROMPT_LENS, steps, "skinny").float().cpu()
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
    print(f"teacher-forced skinny decode {name}: worst rms ratio cached / full forward = {worst:.3f}")
    record("decode_forced_skinny", model=name, worst_ratio=worst)


# ------------------------------------------------------------------------------------------------ 8. batch invariance
def test_skinny_generate_batch_of_ragged_prompts_equals_each_prompt_alone():
    """test_generate_batch_of_ragged_prompts_equals_each_prompt_alone in skinny mode (same model, prompts and lengths)."""
    m, _, _ = _model("student")
    ids, _ = _prompts()
    am = _mask(PROMPT_LENS, 24)
    junk = torch.where(am.bool(), ids, torch.full_like(ids, 639))   # the pad slots hold a token the rows never see
    kw = dict(max_new_tokens=32, do_sample=False, decode_kernels="skinny")
    out = m.generate(junk.to(dev()), attention_mask=am.to(dev()), **kw).cpu()
    for b, n in enumerate(PROMPT_LENS):
        alone = m.generate(ids[b:b + 1, :n].to(dev()), **kw).cpu()
        assert torch.equal(alone[0, n:], out[b, 24:]), b
    # ... and the tokens do not depend on how often the host looks at the finished flags
    kw2 = dict(attention_mask=am.to(dev()), max_new_tokens=24, do_sample=True, top_k=20, temperature=0.9, seed=3,
               eos_token_id=int(out[0, 26]), pad_token_id=2, decode_kernels="skinny")
    assert torch.equal(m.generate(ids.to(dev()), sync_every=1, **kw2), m.generate(ids.to(dev()), sync_every=16, **kw2))


# ------------------------------------------------------------------------------------------- 9 / 10. fallback, default
def _one_step(m, B, decode_kernels, seed=11):
    """(logits, {kernel symbol: launches}) of one decode step after an 8-token prefill of B rows; the launches are what
    the library's launch profiler (sd_prof_*) labelled during the step."""
    from speech_distill_amd import ops
    from speech_distill_amd.generation import Decoder
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 640, (B, 8), generator=g).to(dev())
    nxt = torch.randint(0, 640, (B,), generator=g).to(dev())
    dec = Decoder(m, B, 16, decode_kernels=decode_kernels)
    kv_len = torch.full((B,), 8, dtype=torch.int32, device=dev())
    dec.prefill(ids, kv_len)
    ops.prof_begin()
    logits = dec.step(nxt, kv_len, 9).clone()
    ops.prof_end()
    return logits, {sym: int(v[2]) for sym, v in ops.prof_symbols().items()}


def _count(launches, prefix):
    return sum(n for sym, n in launches.items() if sym.startswith(prefix))


@pytest.mark.parametrize("name", list(SHAPES))
def test_skinny_step_falls_back_whole_at_17_rows_and_takes_the_gemv_path_at_4(name):
    """B = 17: the flagged step IS the unflagged one (same bits, no GEMV launch).  B = 4: the flagged step launches 4 GEMVs
    per layer + 1 for the final norm and lm_head, and no separate RMSNorm, SwiGLU or tile GEMM; the unflagged step launches
    no GEMV.  (Launch labels, not bits: on the 128-wide student every logit of the two paths rounds to the same bf16.)"""
    m, _, _ = _model(name)
    L = m.dims.num_hidden_layers
    skinny17, sym17 = _one_step(m, 17, "skinny")
    tile17, _ = _one_step(m, 17, "tile")
    assert same_bits(skinny17, tile17) and _count(sym17, "gemv_kernel") == 0
    _, tile4 = _one_step(m, 4, "tile")
    _, skinny4 = _one_step(m, 4, "skinny")
    assert _count(tile4, "gemv_kernel") == 0 and _count(tile4, "rmsnorm_fwd_kernel") == 2 * L + 1
    assert _count(skinny4, "gemv_kernel") == 4 * L + 1, skinny4
    assert _count(skinny4, "rmsnorm") == 0 and _count(skinny4, "swiglu") == 0 and _count(skinny4, "gemm") == 0, skinny4
    assert sum(skinny4.values()) == 7 * L + 2, skinny4      # 7 launches per layer, the embedding, the lm_head


def test_generate_default_is_the_tile_step():
    m, _, _ = _model("student")
    ids, _ = _prompts()
    kw = dict(max_new_tokens=16, do_sample=True, top_k=50, temperature=0.8, seed=5)
    assert torch.equal(m.generate(ids.to(dev()), **kw), m.generate(ids.to(dev()), decode_kernels="tile", **kw))
    from speech_distill_amd.generation import Decoder
    assert Decoder(m, 2, 16).flags == 0 and Decoder(m, 2, 16, "skinny").flags == 1


# ---------------------------------------------------------------------------------------------------- 11. bad argument
def test_generate_rejects_unknown_decode_kernels():
    from speech_distill_amd.generation import Decoder
    m, _, _ = _model("student")
    ids = torch.zeros(2, 8, dtype=torch.int64, device=dev())
    with pytest.raises(ValueError, match="decode_kernels"):
        m.generate(ids, max_new_tokens=2, decode_kernels="fast")
    with pytest.raises(ValueError, match="decode_kernels"):
        Decoder(m, 2, 16, decode_kernels="fast")
