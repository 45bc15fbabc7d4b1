"""On-policy batches for generalised knowledge distillation (GKD): a micro-batch's completion is replaced by the
student's own sampled continuation of its prompt, so that the student is trained on the prefixes it produces itself.

Everything here is pure tensor bookkeeping on whatever device the batch lives on (tested on the CPU); the only GPU work
is the ``generate`` callable handed to ``rollout``.  Rules:

  * ``prompt_len[b]`` is the first position whose label is not -100; a row with no labelled position is left exactly as
    it is (every key);
  * positions ``t >= prompt_len[b]`` of ``input_ids`` -- and of ``teacher_input_ids`` where the batch has one, the two
    prefixes being position-aligned (data.py:20-60 align_prefixes) -- take the row's new tokens, cut at the batch's width
    T: the batch keeps its shape;
  * a row's completion ends with its first EOS (included), else with its last generated token; the attention masks are 1
    through that position and 0 behind it, where ``input_ids`` hold ``pad_token_id``;
  * ``labels`` are the new ``input_ids`` on the completion with the collator's rule reapplied (data.py:247-251):
    ``pad_token_id`` -> -100 (an EOS that IS the pad token included), -100 before the prompt end and on padding;
  * ``speech_token_mask``, if present, is 1 on the completion and 0 behind it.
"""
import torch

GENERATE_KEYS = ("max_new_tokens", "temperature", "top_k", "top_p", "repetition_penalty", "use_ras", "win_size", "tau_r",
                 "eos_token_id", "pad_token_id", "decode_kernels")


def check_generate_kwargs(kw):
    """ValueError unless ``kw`` is a dict of ``generate`` keywords with at least a positive ``max_new_tokens``."""
    if not isinstance(kw, dict) or "max_new_tokens" not in kw:
        raise ValueError("on_policy_generate must be a dict of generate() keywords with at least 'max_new_tokens'")
    unknown = sorted(set(kw) - set(GENERATE_KEYS))
    if unknown:
        raise ValueError(f"on_policy_generate: unknown keys {unknown}; known: {list(GENERATE_KEYS)}")
    if int(kw["max_new_tokens"]) <= 0:
        raise ValueError("on_policy_generate['max_new_tokens'] must be positive")


def prompt_lengths(labels):
    """int64 [B]: the first position whose label is not -100; T for a row with no labelled position."""
    T = labels.shape[1]
    pos = torch.arange(T, device=labels.device, dtype=torch.int64)[None, :].expand_as(labels)
    return torch.where(labels != -100, pos, torch.full_like(pos, T)).amin(1)


def fill_token(eos_token_id=None, pad_token_id=None):
    """What ``generate`` writes after a row's EOS: ``pad_token_id``, else ``eos_token_id``, else 0."""
    return pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)


def replace_completion(batch, new_tokens, prompt_len, eos_token_id=None, pad_token_id=None):
    """-> a new batch dict (same keys, shapes and dtypes; ``batch`` itself is not modified) whose rows continue their
    prompt with ``new_tokens`` [B, M] (``generate``'s new tokens: row b's first new token first) by the rules above.
    ``prompt_len`` int64 [B] (``prompt_lengths``).  No host read."""
    ids = batch["input_ids"]
    B, T = ids.shape
    dev = ids.device
    new_tokens = new_tokens.to(device=dev, dtype=torch.int64)
    M = new_tokens.shape[1]
    plen = prompt_len.to(device=dev, dtype=torch.int64)
    fill = fill_token(eos_token_id, pad_token_id)
    # tokens a row generated: through its first EOS, else all M; never past the batch's width
    n_gen = torch.full((B,), M, dtype=torch.int64, device=dev)
    if eos_token_id is not None:
        is_eos = new_tokens == eos_token_id
        n_gen = torch.where(is_eos.any(1), is_eos.to(torch.int64).argmax(1) + 1, n_gen)
    n_gen = torch.minimum(n_gen, (T - plen).clamp_min(0))
    active = (plen < T)[:, None]                       # rows with a labelled position
    pos = torch.arange(T, device=dev, dtype=torch.int64)[None, :]
    behind = pos >= plen[:, None]                      # the old completion and its padding
    comp = behind & (pos < (plen + n_gen)[:, None])    # the new completion
    src = (pos - plen[:, None]).clamp(0, max(M - 1, 0))
    tok = torch.where(comp, new_tokens.gather(1, src), torch.full_like(src, fill))

    def put(old, value):  # `value` behind the prompt end of active rows, `old` elsewhere; old's dtype
        return torch.where(active & behind, value.to(old.dtype), old)

    out = dict(batch)
    out["input_ids"] = put(ids, tok)
    if batch.get("teacher_input_ids") is not None:
        out["teacher_input_ids"] = put(batch["teacher_input_ids"], tok)
    for k in ("attention_mask", "teacher_attention_mask", "speech_token_mask"):
        if batch.get(k) is not None:
            out[k] = put(batch[k], comp)
    lab = torch.where(comp, tok, torch.full_like(tok, -100))
    if pad_token_id is not None:
        lab = torch.where(lab == pad_token_id, torch.full_like(lab, -100), lab)
    out["labels"] = put(batch["labels"], lab)
    return out


@torch.no_grad()
def rollout(generate, batch, generate_kwargs, seed):
    """Replace ``batch``'s completions by ``generate``'s continuation of its prompts.  ``generate`` is
    ``HipQwen3ForCausalLM.generate`` (or a stand-in with its signature and return: [B, T + max_new_tokens], the new tokens
    in columns T...), called once under no_grad with the mask ``t < prompt_len[b]`` and ``max_new_tokens`` capped so that
    the longest completion still ends inside the batch's width.  One host read of ours: the prompt lengths (they size
    the rollout).  A batch without a labelled position is returned as it is; a row whose first label sits at position 0
    has no prompt to continue and is a ValueError (the step aborts) before anything is generated."""
    check_generate_kwargs(generate_kwargs)
    if batch.get("teacher_top_k_v") is not None:
        raise ValueError("an on-policy batch needs the teacher model: pre-extracted teacher_top_k_v / teacher_top_k_i "
                         "belong to the dataset's tokens, not to the student's")
    ids, labels = batch["input_ids"], batch["labels"]
    if tuple(labels.shape) != tuple(ids.shape):
        raise ValueError(f"labels {tuple(labels.shape)} != input_ids {tuple(ids.shape)}")
    tids = batch.get("teacher_input_ids")
    if tids is not None and tuple(tids.shape) != tuple(ids.shape):
        raise ValueError(f"teacher_input_ids {tuple(tids.shape)} and input_ids {tuple(ids.shape)} must be position-aligned")
    T = ids.shape[1]
    plen = prompt_lengths(labels)
    host = plen.tolist()                               # the one host read
    live = [p for p in host if p < T]
    if not live:
        return batch
    if min(live) == 0:   # a row labelled from position 0 has no prompt at all: nothing to condition on
        raise ValueError("on-policy rollout: a row's first label sits at position 0, it has no prompt to continue")
    kw = dict(generate_kwargs)
    kw["max_new_tokens"] = min(int(kw["max_new_tokens"]), T - min(live))
    # a row without a labelled position still needs a prompt for the call: its first token; its output is dropped
    pos = torch.arange(T, device=ids.device, dtype=torch.int64)[None, :]
    mask = (pos < torch.where(plen < T, plen, torch.ones_like(plen))[:, None]).to(torch.int64)
    full = generate(ids, attention_mask=mask, seed=int(seed), **kw)
    return replace_completion(batch, full[:, T:], plen, kw.get("eos_token_id"), kw.get("pad_token_id"))
