"""CPU checks of KV-cache generation: the pure-torch reference sampler (tests/gen_ref.py) against HF's own logits
processors, the repetition-aware rule on hand-built cases, and the host-side errors of ``generate``."""
import pytest
import torch

import gen_ref as R

V = 2000


def _hf_probs(logits, prompt, generated, p):
    """softmax of HF's processor chain in generate's order (sampler.py:140): the penalty sees the generated ids only."""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    s = logits.clone().float()
    gen_ids = torch.tensor(generated, dtype=torch.int64)
    full = torch.cat([torch.tensor(prompt, dtype=torch.int64), gen_ids], dim=1)
    if p.repetition_penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(p.repetition_penalty)(gen_ids, s)
    if p.eos_token_id is not None and p.min_new_tokens > 0:
        s = MinNewTokensLengthLogitsProcessor(len(prompt[0]), p.min_new_tokens, p.eos_token_id, device="cpu")(full, s)
    if p.temperature != 1.0:
        s = TemperatureLogitsWarper(p.temperature)(full, s)
    if p.top_k > 0:
        s = TopKLogitsWarper(p.top_k)(full, s)
    if p.top_p < 1.0:
        s = TopPLogitsWarper(p.top_p)(full, s)
    return torch.softmax(s.double(), -1)


CASES = {
    "reference_defaults": dict(temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.25),
    "top_p_1": dict(temperature=0.6, top_k=100, top_p=1.0, repetition_penalty=1.25),
    "top_k_1": dict(temperature=0.6, top_k=1, top_p=0.9, repetition_penalty=1.25),
    "penalty_1": dict(temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.0),
    "min_new_tokens": dict(temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.25, min_new_tokens=8, eos_token_id=3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_processed_distribution_equals_hf_chain(name):
    p = R.Params(**CASES[name])
    g = torch.Generator().manual_seed(11)
    B, n_prompt, n_gen = 6, 5, 6
    logits = 3.0 * torch.randn(B, V, generator=g)
    prompt = torch.randint(0, V, (B, n_prompt), generator=g).tolist()
    generated = torch.randint(0, V, (B, n_gen), generator=g).tolist()
    for b in range(B):
        generated[b][1] = generated[b][0]                 # a token generated twice is penalised once
        top = torch.topk(logits[b], 4).indices.tolist()
        generated[b][2], generated[b][3] = top[0], top[2]  # penalised tokens inside the top-k
        prompt[b][0] = top[1]                              # a prompt token is NOT penalised
        if p.eos_token_id is not None:
            logits[b, p.eos_token_id] = logits[b].max() + 1.0   # EOS would win if it were not suppressed
    hf = _hf_probs(logits, prompt, generated, p)
    worst = 0.0
    for b in range(B):
        mine = R.processed_probs(logits[b], generated[b], p)
        worst = max(worst, float((mine - hf[b]).abs().max()))
        assert int((mine > 0).sum()) == int((hf[b] > 0).sum())
    print(f"{name}: max |p_ref - p_hf| = {worst:.3e}")
    assert worst <= 1e-6
    if p.eos_token_id is not None:
        assert float(hf[:, p.eos_token_id].max()) == 0.0


def test_penalty_reads_generated_tokens_only_and_each_once():
    p = R.Params(repetition_penalty=2.0, do_sample=False)
    logits = torch.tensor([4.0, -2.0, 1.0, 3.0])
    s = R.scores_fp32(logits, [0, 0, 1], p)
    assert s.tolist() == [2.0, -4.0, 1.0, 3.0]


def _seq_with(count, cand, n, filler=1000):
    """n tokens ending in a window of 25 that holds ``cand`` exactly ``count`` times."""
    win = [filler + i for i in range(25)]
    for i in range(count):
        win[3 * i] = cand
    return [filler + 100 + i for i in range(n - 25)] + win


def test_ras_threshold_is_five_of_twenty_five():
    assert R.ras_triggered(_seq_with(4, 7, 60), 7, 25, 0.2)        # 4 + 1 >= 25 * 0.2
    assert not R.ras_triggered(_seq_with(3, 7, 60), 7, 25, 0.2)    # 3 + 1 <  5
    # occurrences older than the window do not count
    assert not R.ras_triggered([7] * 10 + _seq_with(3, 7, 25), 7, 25, 0.2)


def test_ras_window_reaches_into_the_prompt():
    prompt = [7, 7, 7, 5, 6]                     # 3 occurrences in the prompt
    seq = prompt + [9, 7, 8]                     # + 1 generated: 4 in the last 25 tokens of the WHOLE sequence
    assert R.ras_triggered(seq, 7, 25, 0.2)
    assert not R.ras_triggered(seq[len(prompt):], 7, 25, 0.2)   # the generated part alone would not trigger


def test_ras_switches_the_final_draw_to_the_raw_distribution():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(V, generator=g)
    logits[7] = 12.0                               # the candidate is token 7 for any u0
    p = R.Params(**R.REFERENCE)
    for count, want in ((4, True), (3, False)):
        seq = _seq_with(count, 7, 40)
        tok, info = R.sample_row(logits, seq, 10, 0.5, 0.999999, p)
        assert info["ras"] is want
        # u1 at the very top of the CDF: the raw distribution reaches far outside the top-k survivors, the processed one cannot
        in_topk = tok in torch.topk(logits, 100).indices.tolist()
        assert in_topk is (not want)
        assert info["cdf_final"].numel() == (V if want else info["cdf_cand"].numel())


def test_draw_is_the_inverse_cdf():
    ids, probs = torch.tensor([5, 2, 9]), torch.tensor([0.5, 0.3, 0.2], dtype=torch.float64)
    assert [R.draw(ids, probs, u) for u in (0.0, 0.49, 0.5, 0.79, 0.8, 0.999)] == [5, 5, 2, 2, 9, 9]


def _cpu_model():
    import speech_distill_amd as sda
    return sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device="cpu", init_std=0)


def test_generate_rejects_cpu_tensors():
    m = _cpu_model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(torch.zeros(1, 4, dtype=torch.int64), max_new_tokens=2, do_sample=False)


def test_generate_argument_errors_come_before_any_launch():
    m = _cpu_model()
    ids = torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="top_k"):
        m.generate(ids, max_new_tokens=2, top_k=129)
    m.kv_cache_capacity = 16
    with pytest.raises(ValueError, match="capacity"):
        m.generate(ids, max_new_tokens=13, do_sample=False)
    m.kv_cache_capacity = None
    cap = int(m.config.max_position_embeddings)
    with pytest.raises(ValueError, match="capacity"):
        m.generate(ids, max_new_tokens=cap - 3, do_sample=False)
    with pytest.raises(ValueError, match="top_k in 1..128"):
        m.generate(ids, max_new_tokens=2, top_k=0, top_p=0.9)
    m.inference_precision = "mxfp8"   # what set_inference_precision("mxfp8") leaves on a model that supports it
    with pytest.raises(NotImplementedError, match="mxfp8"):
        m.generate(ids, max_new_tokens=2, do_sample=False)


def test_new_entries_size_their_buffers_without_a_gpu():
    import ctypes
    import speech_distill_amd as sda
    from speech_distill_amd import _lib
    lib = sda.load_lib()
    d = _lib.Dims(159488, 1024, 3072, 28, 16, 8, 128, 1, 1e-6, 0)
    assert lib.sd_kvcache_bytes(ctypes.byref(d), 4, 1024) == 28 * 2 * 4 * 1024 * 8 * 128 * 2
    assert lib.sd_attn_decode_workspace_bytes(4, 16, 1024) == 4 * 16 * 4 * 132 * 4
    assert lib.sd_attn_decode_workspace_bytes(4, 16, 1025) == 4 * 16 * 5 * 132 * 4
    bad = _lib.Dims(159488, 1024, 3072, 28, 16, 8, 64, 1, 1e-6, 0)
    assert lib.sd_kvcache_bytes(ctypes.byref(bad), 4, 1024) == -3     # head_dim 128 only: SD_ERR_UNSUPPORTED
    assert lib.sd_qwen3_decode_acts_bytes(ctypes.byref(d), 8, 1024) > 0
    assert lib.sd_qwen3_prefill_acts_bytes(ctypes.byref(d), 4, 512) > lib.sd_qwen3_acts_bytes(ctypes.byref(d), 4, 512, 0)
    assert lib.sd_sample_workspace_bytes(4, 159488) >= 4 * 159488 * 4
