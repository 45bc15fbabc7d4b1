"""Stage-1 speech-token alignment (the reference's ``stage1.py``): before distillation, train only the rows of the
expanded vocabulary that belong to the new speech tokens, with plain causal-LM cross-entropy on packed documents.

* ``freeze_model_weights(model, num_new_tokens)`` -- the reference's name and signature (stage1.py:29-93): every weight
  frozen except the input / output embeddings, whose gradients are masked to rows >= ``old_vocab = V - num_new_tokens``.
  On a ``HipQwen3ForCausalLM`` the mask is not a hook: the model records ``stage1_row_lo = old_vocab`` and its backward
  (``sd_qwen3_backward`` with ``SD_BWD_EMBED_ONLY``) never computes the body's weight gradients nor writes the rows
  below it.
* ``pack_bfd`` / ``Stage1Collator`` -- TRL ``packing=True`` restated: best-fit-decreasing bins of ``max_seq_length``
  tokens.  By default each document of a bin is its own right-padded row, so attention and RoPE positions restart per
  document at the cost of padding; ``padding_free=True`` gives what TRL trains on under flash-attention: the documents
  flattened into one row with ``position_ids`` restarting per document and the flash-attn varlen keys, run by the varlen
  attention kernels with no padding at all.  The bin order and the boundary convention (the
  last token of a document predicts nothing, as with HF ``DataCollatorWithFlattening``) are an UNPINNED restatement of
  trl 0.26.2 (requirements.txt), which is not available to test against.
* ``Stage1Trainer`` (speech_distill_amd.trainer) -- the SFTTrainer's role: HF Trainer + FlatAdamW over the Stage-1 segments.

Host-side only, except ``freeze_model_weights`` on a GPU model (it zeroes gradient rows once).
"""
import bisect
from typing import Any, Dict, List, Sequence

import torch


def _summary(model, num_new_tokens):
    """The trainable-parameter summary of the reference (stage1.py:75-93)."""
    total = sum(p.numel() for p in model.parameters())
    by_flag = sum(p.numel() for p in model.parameters() if p.requires_grad)
    emb = model.get_input_embeddings().weight
    new = num_new_tokens * emb.size(1)
    bar = "=" * 60
    print(f"\n{bar}\nTrainable Parameters Summary (Gradient Masking Applied):\n{bar}")
    print(f"Total parameters: {total:,}")
    print(f"Trainable parameters (by requires_grad): {by_flag:,}")
    print(f"Effectively trainable (new tokens only): {new:,}")
    print(f"Frozen parameters: {total - new:,}")
    print(f"Trainable ratio: {100 * new / total:.4f}%")
    print("Note: Gradient masking applied to embedding and lm_head layers.")
    print(f"Old tokens ({emb.size(0) - num_new_tokens:,}) will not receive gradient updates.")
    print(f"{bar}\n")


def freeze_model_weights(model, num_new_tokens):
    """Freeze everything but the embedding rows of the ``num_new_tokens`` newest tokens (reference stage1.py:29-93).

    HipQwen3ForCausalLM: ``requires_grad`` as in the reference (embed_tokens, and lm_head when untied), ``stage1_row_lo``
    recorded on the model (Stage-1 mode: ``forward(labels=...)`` returns ``.loss``, the backward is embedding-only,
    ``optim_segments()`` is the embedding), and gradient rows [0, stage1_row_lo) zeroed once -- nothing writes them again.
    Any other model (an HF ``PreTrainedModel``): the reference's masking hooks on the two embedding weights."""
    from .qwen3 import HipQwen3ForCausalLM
    for p in model.parameters():
        p.requires_grad_(False)
    emb = model.get_input_embeddings()
    V = emb.weight.size(0)
    old_vocab = V - num_new_tokens
    if isinstance(model, HipQwen3ForCausalLM):
        if not 0 <= num_new_tokens <= V:
            raise ValueError(f"num_new_tokens {num_new_tokens} outside [0, {V}]")
        if num_new_tokens > 0:
            emb.weight.requires_grad_(True)
            model.lm_head.weight.requires_grad_(True)
        model.stage1_row_lo = old_vocab
        if model.flat_grad is not None:
            with torch.no_grad():
                for name in ("model.embed_tokens.weight", "lm_head.weight"):
                    if name in model._slices:
                        o, n, shape = model._slices[name]
                        model.flat_grad[o:o + n].view(shape)[:old_vocab].zero_()
    elif num_new_tokens > 0:
        def mask(grad):
            grad = grad.clone()
            grad[:old_vocab] = 0.0
            return grad
        for m in (emb, model.get_output_embeddings()):
            if m is not None:
                m.weight.requires_grad_(True)
                m.weight.register_hook(mask)
    _summary(model, num_new_tokens)
    return model


# ------------------------------------------------------------------------------------------------------ packing
def pack_bfd(seqs: Sequence[Sequence[int]], max_seq_length: int) -> List[List[List[int]]]:
    """Best-fit-decreasing packing: documents longer than ``max_seq_length`` are truncated to it, then taken longest
    first (ties: lower index first) and each goes into the open bin with the least room that still fits it, else a new
    bin.  Returns the bins in creation order, each a list of documents in insertion order.  Deterministic."""
    if max_seq_length <= 0:
        raise ValueError("max_seq_length must be positive")
    docs = [list(s[:max_seq_length]) for s in seqs]
    order = sorted((i for i in range(len(docs)) if len(docs[i]) > 0), key=lambda i: (-len(docs[i]), i))
    bins: List[List[List[int]]] = []
    free: List[tuple] = []  # sorted (room left, bin index)
    for i in order:
        n = len(docs[i])
        k = bisect.bisect_left(free, (n, -1))
        if k == len(free):
            bins.append([docs[i]])
            bisect.insort(free, (max_seq_length - n, len(bins) - 1))
        else:
            room, b = free.pop(k)
            bins[b].append(docs[i])
            bisect.insort(free, (room - n, b))
    return bins


class Stage1Collator:
    """``batch_size`` packed bins -> one row per document, right-padded to the longest (rounded up to
    ``pad_to_multiple_of``): ``input_ids`` (pad ``pad_token_id``), ``attention_mask``, ``labels`` = ids with -100 at the
    first position of every document and at the padding (HF DataCollatorWithFlattening's labels; after the causal
    shift the last token of a document predicts nothing).  Features: ``{"documents": [[ids], ...]}`` (one bin) or
    ``{"input_ids": [ids]}`` (one unpacked document).

    ``padding_free=True``: the documents of the batch's bins (bins in batch order, documents in bin order) flattened into
    ONE row with no padding: ``input_ids`` and ``labels`` [1, M], ``position_ids`` restarting at 0 per document,
    ``cu_seq_lens_q`` / ``_k`` (int32 [n+1]) and ``max_length_q`` / ``_k`` (int) -- exactly what
    ``transformers.DataCollatorWithFlattening(return_flash_attn_kwargs=True, separator_id=-100)`` returns, and no
    ``attention_mask`` (HipQwen3ForCausalLM then runs the varlen attention)."""

    def __init__(self, pad_token_id=0, pad_to_multiple_of=None, padding_free=False):
        if padding_free and pad_to_multiple_of:
            raise ValueError("Stage1Collator: pad_to_multiple_of pads rows, and padding_free has none to pad")
        self.pad_token_id = pad_token_id
        self.pad_to_multiple_of = pad_to_multiple_of
        self.padding_free = padding_free

    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, torch.Tensor]:
        docs = []
        for f in features:
            docs.extend(f["documents"] if "documents" in f else [f["input_ids"]])
        docs = [list(d) for d in docs if len(d) > 0]
        if not docs:
            raise ValueError("Stage1Collator: empty batch")
        if self.padding_free:
            return self._flatten(docs)
        w = max(len(d) for d in docs)
        m = self.pad_to_multiple_of
        if m:
            w = -(-w // m) * m
        ids = torch.full((len(docs), w), self.pad_token_id, dtype=torch.long)
        am = torch.zeros((len(docs), w), dtype=torch.long)
        labels = torch.full((len(docs), w), -100, dtype=torch.long)
        for r, d in enumerate(docs):
            t = torch.tensor(d, dtype=torch.long)
            ids[r, :len(d)] = t
            am[r, :len(d)] = 1
            labels[r, 1:len(d)] = t[1:]
        return {"input_ids": ids, "attention_mask": am, "labels": labels}

    @staticmethod
    def _flatten(docs):
        ids, labels, pos, cu = [], [], [], [0]
        for d in docs:
            ids += d
            labels += [-100] + d[1:]
            pos += range(len(d))
            cu.append(cu[-1] + len(d))
        longest = max(len(d) for d in docs)
        cu_t = torch.tensor(cu, dtype=torch.int32)
        return {"input_ids": torch.tensor([ids], dtype=torch.long), "labels": torch.tensor([labels], dtype=torch.long),
                "position_ids": torch.tensor([pos], dtype=torch.long), "cu_seq_lens_q": cu_t, "cu_seq_lens_k": cu_t.clone(),
                "max_length_q": longest, "max_length_k": longest}
