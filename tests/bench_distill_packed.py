"""Stage-2 distillation micro-step, right-padded batches vs padding-free packed bins (0.6B student, 1.7B teacher, random
weights, one MI355X).

The three seeded length distributions of tests/bench_stage1_packed.py (seed 0): log-uniform [48, 1536], uniform [64, 512]
and uniform [256, 2048].  The same samples, shuffled (seed 1, as HF's RandomSampler), once as padded batches of 4 samples
(``ProcessedDataCollator``) and once as ``--pack_tokens 2048`` bins, one bin per micro-batch
(``pack_bfd_indices`` + ``ProcessedDataCollator(padding_free=True)``).  Timed: ``DistillationTrainer.compute_loss`` +
backward, wall clock between device synchronisations (the step's host read is part of it), the two layouts alternating
micro-batch by micro-batch in one process, after a warm-up; two legs, the live teacher's top-128 and the dense teacher
(``top_k=0``).  Reported per layout: real (sample) tokens per second of every timed micro-batch as median / min / max, the
total over the timed micro-batches, and the padded slots per real token.  The yardstick is the padded layout on the same
samples in the same process; whatever is measured is written, cells where packing loses included.

    python tests/bench_distill_packed.py --out profiles/distill_packed_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_stage1_packed import DISTS, lengths  # noqa: E402


class _Tok:
    pad_token = "<|semantic_token_end|>"

    def __init__(self, pad, bos):
        self.pad_token_id, self.bos = pad, bos

    def encode(self, text, add_special_tokens=False):
        return [self.bos]


def samples(kind, lo, hi, V, bos, pad, n):
    """Pre-processed rows shaped like scripts/train.py's synthetic ones: a quarter text, speech_bos, speech tokens, pad."""
    g = torch.Generator().manual_seed(0)
    rows = []
    for L in lengths(kind, lo, hi, n):
        nt = max(2, L // 4)
        ids = torch.cat([torch.randint(0, bos, (nt,), generator=g), torch.tensor([bos]),
                         torch.randint(bos + 1, V, (L - nt - 2,), generator=g), torch.tensor([pad])])
        ids[nt + 1:-1][ids[nt + 1:-1] == pad] = bos + 1
        rows.append({"student_input_ids": ids.tolist(), "student_attention_mask": [1] * L,
                     "teacher_input_ids": ids.tolist(), "teacher_attention_mask": [1] * L})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=12, help="timed micro-batches per layout, distribution and leg (>= 5)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=400, help="samples drawn per distribution")
    ap.add_argument("--pack_tokens", type=int, default=2048)
    ap.add_argument("--out", default=None)
    cfg = ap.parse_args()
    if cfg.batches < 5:
        ap.error("--batches must be at least 5")
    from transformers import TrainingArguments
    import speech_distill_amd as sda
    from speech_distill_amd.collator import ProcessedDataCollator
    from speech_distill_amd.packing import pack_bfd_indices
    from speech_distill_amd.trainer import DistillationTrainer
    dev = torch.device("cuda:0")
    sd, td = sda.Qwen3Dims.student_06b(), sda.Qwen3Dims.teacher_17b()
    V, bos, pad = sd.vocab_size, 152927, 153478
    student = sda.HipQwen3ForCausalLM(sd, device=dev, seed=0)
    teacher = sda.HipQwen3ForCausalLM(td, device=dev, seed=1)
    teacher.eval().requires_grad_(False)
    student.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"recompute": "auto"})
    student.train()
    colls = {"padded": ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad),
             "packed": ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad, padding_free=True)}
    res = {"student": "qwen3-0.6b (V=159488)", "teacher": "1.7b", "weights": "random", "samples_per_dist": cfg.samples,
           "padded_batch": "4 samples", "packed_batch": f"1 bin of pack_bfd_indices(lengths, {cfg.pack_tokens})",
           "timing": "wall clock between synchronisations around compute_loss + backward, layouts alternating, after "
                     f"{cfg.warmup} warm-up micro-batches per layout", "cells": []}

    def trainer(top_k):
        args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False,
                                 label_names=["labels"], save_strategy="no", logging_steps=10 ** 9, bf16=True)
        tr = DistillationTrainer(model=student, args=args, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=top_k)
        tr.state.global_step = 1     # (no sub-loss log inside the timed region: logging_steps never divides it)
        return tr

    def step(tr, batch):
        student.zero_grad()
        b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.compute_loss(student, b).backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    n_mb = cfg.warmup + cfg.batches
    for name, (kind, lo, hi) in DISTS.items():
        rows = samples(kind, lo, hi, V, bos, pad, cfg.samples)
        order = torch.randperm(len(rows), generator=torch.Generator().manual_seed(1)).tolist()
        lens = [len(r["student_input_ids"]) for r in rows]
        padded = [[rows[j] for j in order[i:i + 4]] for i in range(0, 4 * n_mb, 4)]
        bins = pack_bfd_indices(lens, cfg.pack_tokens)
        bins = [bins[i] for i in torch.randperm(len(bins), generator=torch.Generator().manual_seed(1)).tolist()][:n_mb]
        packed = [[rows[j] for j in b] for b in bins]
        for leg, top_k in (("top128", 128), ("dense", 0)):
            tr = trainer(top_k)
            cell = {"dist": name, "leg": leg}
            stats = {k: [] for k in colls}
            for i in range(n_mb):
                for layout, feats in (("padded", padded[i]), ("packed", packed[i])):
                    batch = colls[layout]([dict(f) for f in feats])
                    ms = step(tr, batch)
                    if i >= cfg.warmup:
                        real = sum(len(f["student_input_ids"]) for f in feats)
                        stats[layout].append((real, batch["input_ids"].numel(), ms))
            for layout, st in stats.items():
                tps = [r / ms * 1e3 for r, _, ms in st]
                cell[layout] = {"timed_micro_batches": len(st), "real_tokens": sum(r for r, _, _ in st),
                                "slots_per_real_token": round(sum(s for _, s, _ in st) / sum(r for r, _, _ in st), 3),
                                "ms_median": round(statistics.median(ms for _, _, ms in st), 2),
                                "tok_s_median": round(statistics.median(tps)), "tok_s_min": round(min(tps)),
                                "tok_s_max": round(max(tps)),
                                "tok_s_total": round(sum(r for r, _, _ in st) / sum(ms for _, _, ms in st) * 1e3)}
            cell["packed_over_padded_total"] = round(cell["packed"]["tok_s_total"] / cell["padded"]["tok_s_total"], 3)
            cell["packed_over_padded_median"] = round(cell["packed"]["tok_s_median"] / cell["padded"]["tok_s_median"], 3)
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
    print(json.dumps(res))
    if cfg.out:
        os.makedirs(os.path.dirname(os.path.abspath(cfg.out)), exist_ok=True)
        with open(cfg.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
