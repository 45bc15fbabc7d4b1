"""Batch builder with the contract of the reference's ``ProcessedDataCollator`` (data.py:201-387), the component that
defines the hot path's inputs: same constructor, same output keys, dtypes and values (pinned by
fixture G3, ``tests/test_collator_golden.py``) --

* ``input_ids`` / ``attention_mask`` int64, right-padded with ``pad_token_id`` / 0 to the longest row (rounded up to
  ``pad_to_multiple_of``);
* ``labels`` = ids where a target exists, else -100: no target at ANY position holding the pad id (quirk Q2: the final
  ``<|semantic_token_end|>`` equals the pad token, data.py:250-251) nor before the first ``speech_bos`` of a row (a row
  without one has no targets, data.py:273-276, 350-387);
* ``teacher_input_ids`` / ``teacher_attention_mask`` when the features carry teacher sequences;
* ``teacher_top_k_v`` (pad 0.0) / ``teacher_top_k_i`` (pad 0) ``[B, T, K]`` cut or padded to the STUDENT width when the
  features carry pre-extracted top-K (data.py:330-348);
* beyond the reference, ``teacher_top_k_tail`` fp32 ``[B, T]`` (the teacher's mass outside its top-K per position, written
  by ``extract_teacher_logits.py --tail_temperature``) when the features carry it next to the top-K: cut or padded like
  its siblings, pad value 1.0 -- a tail of 1 masks the position for the ``_tail`` divergences, as its label does.
  Batches without the column are unchanged.

``padding_free=True`` (beyond the reference): the batch's samples flattened in order into ONE row without padding, in the
format of ``stage1.Stage1Collator`` / HF ``DataCollatorWithFlattening(return_flash_attn_kwargs=True, separator_id=-100)``:
``input_ids`` / ``labels`` / ``position_ids`` ``[1, M]`` (positions restart at 0 per document), ``cu_seq_lens_q`` / ``_k``
int32 ``[n+1]``, ``max_length_q`` / ``_k`` ints, no attention masks.  A document's labels are the padded collator's labels
of that sample (both rules above, the ``speech_bos`` one evaluated per document) with -100 in its first cell;
``teacher_input_ids`` ``[1, M]`` (per sample as long as the student's, else ValueError) and the top-K blocks, each cut or
padded to its sample's student length, ``[1, M, K]`` (``teacher_top_k_tail`` likewise, ``[1, M]``).  A feature may be ``{"samples": [sample, ...]}`` (a bin of
``packing.PackedView``): its samples are taken in order.

Built differently from the reference: every ragged field becomes ONE scatter of its concatenated values into a
pre-filled ``[B, W]`` grid (a length mask selects the valid cells in row-major order: no per-row copy loop), and
``labels`` is one ``where`` over the grid instead of a clone masked twice.  Host-side only (dataloader workers).
"""
import itertools
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch


def _ragged_to_grid(seqs: Sequence, width: int, fill, dtype) -> torch.Tensor:
    """Right-padded ``[len(seqs), width]`` grid of the ragged ``seqs`` (1-D each), one scatter."""
    lens = torch.tensor([len(s) for s in seqs], dtype=torch.long)
    grid = torch.full((len(seqs), width), fill, dtype=dtype)
    total = int(lens.sum())
    if total:
        if dtype == torch.long and all(isinstance(s, (list, tuple)) for s in seqs):
            # datasets hands out Python lists: one numpy pass over the chained items is 2x faster than a tensor per row
            flat = torch.from_numpy(np.fromiter(itertools.chain.from_iterable(seqs), dtype=np.int64, count=total))
        else:
            flat = torch.cat([torch.as_tensor(s, dtype=dtype).reshape(-1) for s in seqs])
        # row-major order of the valid cells = the order of the concatenation
        grid[torch.arange(width)[None, :] < lens[:, None]] = flat
    return grid


class ProcessedDataCollator:
    def __init__(self, tokenizer, pad_token_id=153478, speech_bos: str = "<|semantic_token_start|>",
                 pad_to_multiple_of: Optional[int] = None, padding_free: bool = False):
        if padding_free and pad_to_multiple_of:
            raise ValueError("ProcessedDataCollator: pad_to_multiple_of pads rows, and padding_free has none to pad")
        self.padding_free = padding_free
        self.tokenizer = tokenizer
        self.pad_token_id = pad_token_id
        self.pad_to_multiple_of = pad_to_multiple_of
        self.speech_bos = speech_bos

    # ------------------------------------------------------------------------------------------------ pieces
    def _width(self, seqs) -> int:
        w = max(len(s) for s in seqs)
        m = self.pad_to_multiple_of
        return w if m is None else -(-w // m) * m

    def _ids_and_mask(self, ids_seqs, mask_seqs):
        w = self._width(ids_seqs)
        return (_ragged_to_grid(ids_seqs, w, self.pad_token_id, torch.long), _ragged_to_grid(mask_seqs, w, 0, torch.long))

    def _speech_bos_id(self) -> Optional[int]:
        """Token id of ``speech_bos``; None (= no text masking, as the reference does on a tokenizer failure) otherwise."""
        try:
            tok = self.tokenizer.encode(self.speech_bos, add_special_tokens=False)
        except Exception:
            return None
        return tok[0] if tok else None

    @staticmethod
    def _topk_grid(items, width: int, fill) -> torch.Tensor:
        """Per-sample ``[len_i, K]`` -> ``[B, width, K]``: rows past ``width`` are cut, missing rows take ``fill``."""
        first = items[0] if isinstance(items[0], torch.Tensor) else torch.as_tensor(items[0])
        out = torch.full((len(items), width, first.size(1)), fill, dtype=first.dtype)
        for b, it in enumerate(items):
            it = it if isinstance(it, torch.Tensor) else torch.as_tensor(it)
            n = min(width, it.size(0))
            out[b, :n] = it[:n]
        return out

    @staticmethod
    def _tail_grid(items, width: int) -> torch.Tensor:
        """Per-sample ``[len_i]`` tails -> fp32 ``[B, width]``, cut or padded with 1.0 (the top-K blocks' rule)."""
        return _ragged_to_grid([torch.as_tensor(it, dtype=torch.float32).reshape(-1)[:width] for it in items], width, 1.0,
                               torch.float32)

    # -------------------------------------------------------------------------------------------------- call
    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, torch.Tensor]:
        if self.padding_free:
            return self._flatten([s for f in features for s in (f["samples"] if "samples" in f else [f])])
        paired = "student_input_ids" in features[0]
        ids_key, am_key = ("student_input_ids", "student_attention_mask") if paired else ("input_ids", "attention_mask")
        ids, am = self._ids_and_mask([f[ids_key] for f in features], [f[am_key] for f in features])
        # one predicate for "this position has a target": not the pad id, and at / after the row's first speech_bos
        has_target = torch.ones_like(ids, dtype=torch.bool) if self.pad_token_id is None else ids != self.pad_token_id
        bos = self._speech_bos_id()
        if bos is not None:
            has_target &= (ids == bos).cumsum(-1) > 0
        batch = {"input_ids": ids, "attention_mask": am, "labels": torch.where(has_target, ids, torch.full_like(ids, -100))}
        if features[0].get("teacher_input_ids") is not None:
            batch["teacher_input_ids"], batch["teacher_attention_mask"] = self._ids_and_mask(
                [f["teacher_input_ids"] for f in features], [f["teacher_attention_mask"] for f in features])
        if features[0].get("teacher_top_k_v") is not None:
            batch["teacher_top_k_v"] = self._topk_grid([f["teacher_top_k_v"] for f in features], ids.size(1), 0.0)
            batch["teacher_top_k_i"] = self._topk_grid([f["teacher_top_k_i"] for f in features], ids.size(1), 0)
            if features[0].get("teacher_top_k_tail") is not None:
                batch["teacher_top_k_tail"] = self._tail_grid([f["teacher_top_k_tail"] for f in features], ids.size(1))
        return batch

    # ------------------------------------------------------------------------------------------ padding-free
    @staticmethod
    def _one_row(seqs, total: int) -> torch.Tensor:
        """The ragged ``seqs`` end to end as one ``[1, total]`` int64 row."""
        if all(isinstance(s, (list, tuple)) for s in seqs):
            flat = torch.from_numpy(np.fromiter(itertools.chain.from_iterable(seqs), dtype=np.int64, count=total))
        else:
            flat = torch.cat([torch.as_tensor(s, dtype=torch.long).reshape(-1) for s in seqs])
        return flat[None]

    def _flatten(self, samples: List[Dict[str, Any]]) -> Dict[str, Any]:
        paired = bool(samples) and "student_input_ids" in samples[0]
        ids_key = "student_input_ids" if paired else "input_ids"
        with_teacher = bool(samples) and samples[0].get("teacher_input_ids") is not None
        for i, s in enumerate(samples):
            if with_teacher and len(s["teacher_input_ids"]) != len(s[ids_key]):
                raise ValueError(f"padding_free: sample {i} has {len(s['teacher_input_ids'])} teacher tokens and "
                                 f"{len(s[ids_key])} student tokens; packed documents share one set of boundaries "
                                 "(data.py:20-60 align_prefixes gives equal lengths)")
        samples = [s for s in samples if len(s[ids_key]) > 0]
        if not samples:
            raise ValueError("ProcessedDataCollator: empty batch")
        lens = torch.tensor([len(s[ids_key]) for s in samples], dtype=torch.long)
        M, longest = int(lens.sum()), int(lens.max())
        cu = torch.zeros(len(samples) + 1, dtype=torch.long)
        cu[1:] = lens.cumsum(0)
        doc = torch.repeat_interleave(torch.arange(len(samples)), lens)
        pos = torch.arange(M) - cu[doc]
        ids = self._one_row([s[ids_key] for s in samples], M)
        # the padded collator's predicate, per document: not the pad id, at / after the DOCUMENT's first speech_bos
        # (the running count restarts at every document start), and never the document's first cell (HF's separator)
        has_target = torch.ones_like(ids, dtype=torch.bool) if self.pad_token_id is None else ids != self.pad_token_id
        bos = self._speech_bos_id()
        if bos is not None:
            seen = (ids[0] == bos).cumsum(-1)
            before_doc = seen[cu[:-1]] - (ids[0, cu[:-1]] == bos).long()
            has_target &= (seen - before_doc[doc] > 0)[None]
        has_target &= (pos != 0)[None]
        cu32 = cu.to(torch.int32)
        batch = {"input_ids": ids, "labels": torch.where(has_target, ids, torch.full_like(ids, -100)),
                 "position_ids": pos[None], "cu_seq_lens_q": cu32, "cu_seq_lens_k": cu32.clone(),
                 "max_length_q": longest, "max_length_k": longest}
        if with_teacher:
            batch["teacher_input_ids"] = self._one_row([s["teacher_input_ids"] for s in samples], M)
        if samples[0].get("teacher_top_k_v") is not None:
            for key, fill in (("teacher_top_k_v", 0.0), ("teacher_top_k_i", 0)):
                # one [1, len_i, K] grid per sample (the padded rule, with the sample's own length as the width)
                batch[key] = torch.cat([self._topk_grid([s[key]], int(n), fill) for s, n in zip(samples, lens)], dim=1)
            if samples[0].get("teacher_top_k_tail") is not None:
                batch["teacher_top_k_tail"] = torch.cat([self._tail_grid([s["teacher_top_k_tail"]], int(n))
                                                         for s, n in zip(samples, lens)], dim=1)
        return batch
