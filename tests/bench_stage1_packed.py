"""Stage-1 micro-step, padded rows vs padding-free packed rows (0.6B student, num_new_tokens 8220, one MI355X).

Three seeded length distributions of 4 000 documents (seed 0): log-uniform [48, 1536], uniform [64, 512] and uniform
[256, 2048]; ``pack_bfd(..., 2048)``; bins shuffled (seed 1, as HF's RandomSampler); batches of 4 bins through
``Stage1Collator`` in both layouts.  For each distribution the Stage-1 micro-step (forward + CE + embedding-only
backward, the CLI's recompute policy "auto") is timed per batch with device events after warm-up, the two layouts
alternating batch by batch in one process; reported as real (document) tokens per second per layout and their ratio,
with the padded slots per real token of the batches measured.  For the uniform [64, 512] distribution the full-gradient
student step (forward + CE + full backward) is timed the same way.  One JSON document is printed (and written to --out).

    python tests/bench_stage1_packed.py --out profiles/stage1_packed_bench.json
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTS = {"loguniform_48_1536": ("log", 48, 1536), "uniform_64_512": ("uni", 64, 512), "uniform_256_2048": ("uni", 256, 2048)}


def lengths(kind, lo, hi, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, generator=g, dtype=torch.float64)
    if kind == "log":
        return [int(round(math.exp(math.log(lo) + float(x) * (math.log(hi) - math.log(lo))))) for x in u]
    return [int(lo + int(x * (hi - lo + 1))) for x in u]


def batches(kind, lo, hi, V, n_docs=4000, max_len=2048, bins_per_batch=4):
    from speech_distill_amd.stage1 import pack_bfd
    g = torch.Generator().manual_seed(0)
    docs = [torch.randint(0, V, (L,), generator=g).tolist() for L in lengths(kind, lo, hi, n_docs)]
    bins = pack_bfd(docs, max_len)
    order = torch.randperm(len(bins), generator=torch.Generator().manual_seed(1)).tolist()
    bins = [bins[i] for i in order]
    return [[{"documents": b} for b in bins[i:i + bins_per_batch]] for i in range(0, len(bins) - bins_per_batch + 1,
                                                                                  bins_per_batch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=6, help="timed batches per distribution (each in both layouts)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    cfg = ap.parse_args()
    import speech_distill_amd as sda
    from speech_distill_amd import ops
    from speech_distill_amd.stage1 import Stage1Collator, freeze_model_weights
    dev = torch.device("cuda:0")
    dims = sda.Qwen3Dims.student_06b()
    V = dims.vocab_size
    colls = {"padded": Stage1Collator(), "packed": Stage1Collator(padding_free=True)}
    res = {"model": "qwen3-0.6b (V=159488)", "num_new_tokens": 8220, "max_seq_length": 2048, "bins_per_batch": 4,
           "docs": 4000, "timing": "device events per micro-step, layouts alternating, after warm-up", "dists": []}

    def to_dev(b):
        return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}

    def stage1_step(m, b):
        n_items = torch.tensor(float(b["labels"].ne(-100).sum()), device=dev)
        out = m(**b, num_items_in_batch=n_items, stage1_inplace_grad=True)
        out.loss.backward()

    def full_step(m, b):
        n_items = torch.tensor(float(b["labels"].ne(-100).sum()), device=dev)
        am = b.get("attention_mask")
        rows, rl = ops.loss_rows(b["labels"], right_padded=(am,) if am is not None else ())
        kw = {k: v for k, v in b.items() if k != "labels"}
        logits = m(**kw, logit_rows=rows, padding_checked=True).logits
        loss, _ = ops.celoss_rows(logits, rl, n_items, inplace_grad=True)
        loss.backward()

    def timed(m, fn, bl):
        ms = {k: 0.0 for k in colls}
        for i, bins in enumerate(bl):
            for layout, coll in colls.items():
                b = to_dev(coll(bins))
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(m, b)
                e1.record()
                torch.cuda.synchronize()
                if i >= cfg.warmup:
                    ms[layout] += e0.elapsed_time(e1)
        return ms

    for name, (kind, lo, hi) in DISTS.items():
        bl = batches(kind, lo, hi, V)[:cfg.warmup + cfg.batches]
        real = sum(len(d) for bins in bl[cfg.warmup:] for b in bins for d in b["documents"])
        slots = 0
        for bins in bl[cfg.warmup:]:
            p = colls["padded"](bins)["input_ids"]
            slots += p.numel()
        m = sda.HipQwen3ForCausalLM(dims, device=dev, seed=0)
        freeze_model_weights(m, 8220)
        m.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"recompute": "auto"})
        ms = timed(m, stage1_step, bl)
        row = {"dist": name, "timed_batches": cfg.batches, "real_tokens": real,
               "padded_slots_per_real_token": round(slots / real, 3),
               "stage1_padded_ms": round(ms["padded"], 2), "stage1_packed_ms": round(ms["packed"], 2),
               "stage1_padded_tok_s": round(real / ms["padded"] * 1e3), "stage1_packed_tok_s": round(real / ms["packed"] * 1e3),
               "stage1_packed_over_padded": round(ms["padded"] / ms["packed"], 3)}
        del m
        torch.cuda.empty_cache()
        if name == "uniform_64_512":
            m = sda.HipQwen3ForCausalLM(dims, device=dev, seed=0)
            ms = timed(m, full_step, bl)
            row.update({"full_padded_tok_s": round(real / ms["padded"] * 1e3), "full_packed_tok_s": round(real / ms["packed"] * 1e3),
                        "full_packed_over_padded": round(ms["padded"] / ms["packed"], 3)})
            del m
            torch.cuda.empty_cache()
        res["dists"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))
    if cfg.out:
        os.makedirs(os.path.dirname(os.path.abspath(cfg.out)), exist_ok=True)
        with open(cfg.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
