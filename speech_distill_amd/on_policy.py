"""On-policy batches for generalised knowledge distillation (GKD): a micro-batch's completion is replaced by the
student's own sampled continuation of its prompt, so that the student is trained on the prefixes it produces itself.

Everything here is pure tensor bookkeeping on whatever device the batch lives on (tested on the CPU); the only GPU work
is the ``generate`` callable handed to ``rollout``, or the engine handed to ``rollout_window`` (the rollouts of a whole
accumulation window in one engine run).  Rules:

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


def draw(rng, lmbda):
    """The per-micro-batch draw: -> (is_on_policy, seed or None).  One ``torch.rand(1)`` from the CPU generator ``rng``;
    below ``lmbda`` the batch is on-policy and one ``torch.randint(0, 2**31 - 1, (1,))`` gives its rollout seed -- and
    only then, so both rollout modes of the trainer consume the same stream."""
    if float(torch.rand(1, generator=rng)) >= lmbda:
        return False, None
    return True, int(torch.randint(0, 2 ** 31 - 1, (1,), generator=rng))


SEED_MODULUS = 2 ** 31 - 1     # a prime: the range of a draw's seed
SEED_STRIDE = 1_000_003


def request_seed(seed, b):
    """The seed of row ``b`` of a micro-batch whose draw gave ``seed``: ``(seed + 1 000 003 b) mod (2^31 - 1)``, in
    [0, 2^31 - 1).  The modulus is prime and the stride is not a multiple of it, so two rows b != b' of one batch collide
    only when the modulus divides b - b': never for rows below 2^31 - 1, let alone the 64 an engine holds."""
    return (int(seed) + SEED_STRIDE * int(b)) % SEED_MODULUS


def _check_batch(batch):
    """``rollout``'s checks of one batch that need no host read.  -> (input_ids, labels)."""
    if batch.get("teacher_top_k_v") is not None:
        raise ValueError("an on-policy batch needs the teacher model: pre-extracted teacher_top_k_v / teacher_top_k_i "
                         "belong to the dataset's tokens, not to the student's")
    ids, labels = batch["input_ids"], batch["labels"]
    if tuple(labels.shape) != tuple(ids.shape):
        raise ValueError(f"labels {tuple(labels.shape)} != input_ids {tuple(ids.shape)}")
    tids = batch.get("teacher_input_ids")
    if tids is not None and tuple(tids.shape) != tuple(ids.shape):
        raise ValueError(f"teacher_input_ids {tuple(tids.shape)} and input_ids {tuple(ids.shape)} must be position-aligned")
    return ids, labels


SAMPLING_KEYS = tuple(k for k in GENERATE_KEYS if k not in ("max_new_tokens", "decode_kernels"))


@torch.no_grad()
def rollout_window(engine, batches, generate_kwargs, seeds):
    """``rollout`` for the micro-batches of one accumulation window at once, through a request engine
    (``GenerationEngine``, or a stand-in with ``submit`` / ``run`` / ``result`` / ``forget``).  ``seeds[i]`` is None (batch i
    is off-policy and is returned as the same object) or the seed of batch i's draw.  Every on-policy batch goes through
    ``rollout``'s checks BEFORE anything is submitted: shapes, no pre-extracted ``teacher_top_k_v``, no live row labelled
    from position 0.  One host read of ours: the prompt lengths of the whole window.

    Per live row b of batch i one request: the prompt ``input_ids[b, :plen[b]]``, the budget
    ``min(max_new_tokens, T - plen[b])`` (the row's own width, so no step is spent on tokens the batch would cut),
    ``request_seed(seeds[i], b)`` and the sampling keywords of ``generate_kwargs`` (``decode_kernels`` belongs to the
    engine).  A row without a labelled position is not submitted and keeps every key.  After ``engine.run()`` each batch is
    rebuilt by ``replace_completion`` from its requests' tokens, with ``fill_token`` behind each request's end as
    ``generate`` fills; the finished requests are then dropped from the engine.  -> the list of batches."""
    check_generate_kwargs(generate_kwargs)
    if len(seeds) != len(batches):
        raise ValueError(f"{len(seeds)} seeds for {len(batches)} micro-batches")
    on = [i for i, s in enumerate(seeds) if s is not None]
    if not on:
        return list(batches)
    plens = []
    for i in on:
        _, labels = _check_batch(batches[i])
        plens.append(prompt_lengths(labels))
    host = torch.cat(plens).tolist()                   # the one host read
    budget = int(generate_kwargs["max_new_tokens"])
    plan, at = [], 0                                   # (batch, its prompt lengths on the host)
    for i in on:
        B, T = batches[i]["input_ids"].shape
        lens = host[at:at + B]
        at += B
        if any(p == 0 for p in lens):
            raise ValueError("on-policy rollout: a row's first label sits at position 0, it has no prompt to continue")
        plan.append((i, lens))
    # ---- nothing was submitted up to here
    sampling = {k: generate_kwargs[k] for k in SAMPLING_KEYS if k in generate_kwargs}
    fill = fill_token(generate_kwargs.get("eos_token_id"), generate_kwargs.get("pad_token_id"))
    rids = []                                          # (batch, row, request id, budget)
    for i, lens in plan:
        ids = batches[i]["input_ids"]
        T = ids.shape[1]
        for b, p in enumerate(lens):
            if p < T:
                n = min(budget, T - p)
                rids.append((i, b, engine.submit(ids[b, :p], max_new_tokens=n, seed=request_seed(seeds[i], b), **sampling), n))
    out = list(batches)
    if not rids:
        return out
    engine.run()
    for k, (i, lens) in enumerate(plan):
        mine = [r for r in rids if r[0] == i]
        if not mine:
            continue
        ids = batches[i]["input_ids"]
        new = torch.full((ids.shape[0], max(r[3] for r in mine)), fill, dtype=torch.int64, device=ids.device)
        for _, b, rid, _ in mine:
            tok = engine.result(rid)
            new[b, :tok.numel()] = tok
        out[i] = replace_completion(batches[i], new, plens[k], generate_kwargs.get("eos_token_id"),
                                    generate_kwargs.get("pad_token_id"))
    engine.forget([r[2] for r in rids])
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
    ids, labels = _check_batch(batch)
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
