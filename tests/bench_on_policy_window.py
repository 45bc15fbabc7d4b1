"""GPU measurement (not a pytest, not a bench.py line): what an on-policy optimizer step costs when the rollouts of its
accumulation window run through ONE engine run (on_policy.rollout_window) instead of one
``generate`` per micro-batch (on_policy.rollout), written to profiles/on_policy_window_bench.json.

Setup: 0.6B student shape, 1.7B teacher shape, random weights, lmbda = 1 (every micro-batch is rolled out), B = 4,
T = 512, max_new_tokens = 256, prompts of 32 / 64 / 96 / 128 tokens mixed inside every micro-batch, temperature 1,
top_k 50, jsd on the dense teacher, FlatAdamW.  With random weights no row reaches an EOS: every request runs to its 256
tokens, so the engine's refill of rows that stop early -- its advantage on real completions -- is NOT exercised here.

Variants (one optimizer step each: rollouts, A x (teacher + student forward, loss, backward), the AdamW update):
  micro_batch_skinny            today's path and the baseline: A = 4, one generate per micro-batch at 4 rows
  window_skinny_a4_{single,batch}    16 rows in the engine
  window_wide_a8_..., window_wide_a16_...   32 and 64 rows
  window_tile_a16_...           64 rows on the tile GEMMs
per variant: rollout ms per micro-batch and whole ms per optimizer step (and per micro-batch: the accumulations differ).

Method (tests/bench_gjsd.py's): events on the launch stream, one warm-up, the variants alternating in one process, median
of 5 with [min, max].  The one condition, checked after the JSON is written: every window variant's rollout time per
micro-batch lies below the baseline's by more than the baseline's own relative spread ((max - min) / median).

usage: python tests/bench_on_policy_window.py [--out profiles/on_policy_window_bench.json] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speech_distill_amd as sda  # noqa: E402
from speech_distill_amd import on_policy, ops  # noqa: E402
from speech_distill_amd.optim import FlatAdamW  # noqa: E402
from speech_distill_amd.engine import GenerationEngine  # noqa: E402
from speech_distill_amd.paged import PAGE, pages_for  # noqa: E402

dev = torch.device("cuda:0")
VOCAB, SPEECH_LO = 159488, 152927
B, T, NEW = 4, 512, 256
PROMPTS = (32, 64, 96, 128)
VARIANTS = [   # (name, window?, decode_kernels, accumulation, admission)
    ("micro_batch_skinny", False, "skinny", 4, None),
    ("window_skinny_a4_single", True, "skinny", 4, "single"),
    ("window_skinny_a4_batch", True, "skinny", 4, "batch"),
    ("window_wide_a8_single", True, "wide", 8, "single"),
    ("window_wide_a8_batch", True, "wide", 8, "batch"),
    ("window_wide_a16_single", True, "wide", 16, "single"),
    ("window_wide_a16_batch", True, "wide", 16, "batch"),
    ("window_tile_a16_single", True, "tile", 16, "single"),
    ("window_tile_a16_batch", True, "tile", 16, "batch"),
]
BASELINE = VARIANTS[0][0]


def build(dims, seed):
    m = sda.HipQwen3ForCausalLM(dims, device=dev, init_std=0)
    m.flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(seed))
    for p in m._params.values():
        if p.dim() == 1:
            p.data.fill_(1.0)
    return m


def micro_batches(n):
    """n micro-batches [B, T]: text-range prompts of the four lengths in a rotating order, speech-range completions."""
    g = torch.Generator().manual_seed(1234)
    out = []
    for i in range(n):
        ids = torch.randint(SPEECH_LO, VOCAB, (B, T), generator=g)
        labels = ids.clone()
        for b in range(B):
            p = PROMPTS[(b + i) % len(PROMPTS)]
            ids[b, :p] = torch.randint(0, SPEECH_LO, (p,), generator=g)
            labels[b, :p] = -100
        out.append({"input_ids": ids.to(dev), "attention_mask": torch.ones(B, T, dtype=torch.long, device=dev),
                    "labels": labels.to(dev)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "on_policy_window_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    sda.load_lib()
    student, teacher = build(sda.Qwen3Dims.student_06b(), 0), build(sda.Qwen3Dims.teacher_17b(), 1)
    teacher.eval().requires_grad_(False)
    opt = FlatAdamW(student, lr=1e-6)
    loss_fn = sda.DistillationLoss(temperature=2.0, alpha=0.5, inplace_grad=True, divergence="jsd", beta=0.5)
    side = ops.concurrent_stream(dev, "teacher")
    data = micro_batches(max(v[3] for v in VARIANTS))
    engines = {}
    for name, window, kernels, accum, admission in VARIANTS:
        if window:   # what DistillationTrainer builds at its first window: B x A rows, their worst case + the parking page
            rows = B * accum
            pool = student.kv_page_pool(rows * pages_for(T) + 1)
            engines[name] = GenerationEngine(student, pool, rows, kernels, capacity=pages_for(T) * PAGE, admission=admission)

    def micro_step(b):
        rows, row_labels = ops.loss_rows(b["labels"])
        with torch.no_grad():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                tl = teacher(input_ids=b["input_ids"], attention_mask=b["attention_mask"], logit_rows=rows, concurrent=True).logits
        sl = student(input_ids=b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"], logit_rows=rows,
                     concurrent=True).logits
        torch.cuda.current_stream().wait_stream(side)
        loss_fn.forward_rows(sl, row_labels, teacher_logits=tl)[0].backward()

    def optimizer_step(name, window, kernels, accum, admission):
        """-> (rollout ms of the whole window, ms of the whole optimizer step)."""
        kw = {"max_new_tokens": NEW, "temperature": 1.0, "top_k": 50, "decode_kernels": kernels}
        batches, seeds = data[:accum], [7 + i for i in range(accum)]
        marks, roll = [], 0.0

        def mark():
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record()
            return marks[-1]
        student.zero_grad()
        start = mark()
        if window:
            engines[name].reset_stats()
            batches = on_policy.rollout_window(engines[name], batches, kw, seeds)
            spans = [(start, mark())]
        else:
            spans = []
        for i, b in enumerate(batches):
            if not window:
                a = mark()
                b = on_policy.rollout(student.generate, b, kw, seeds[i])
                spans.append((a, mark()))
            micro_step(b)
        opt.step()
        end = mark()
        end.synchronize()
        roll = sum(a.elapsed_time(z) for a, z in spans)
        return roll, start.elapsed_time(end)

    for v in VARIANTS:
        optimizer_step(*v)   # warm-up
    torch.cuda.synchronize()
    runs = {v[0]: [] for v in VARIANTS}
    for _ in range(args.repeats):
        for v in VARIANTS:
            runs[v[0]].append(optimizer_step(*v))

    def summary(xs):
        return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}
    res = {}
    for name, window, kernels, accum, admission in VARIANTS:
        r = runs[name]
        res[name] = {"decode_kernels": kernels, "accumulation": accum, "rows_rolled_out_together": B * accum if window else B,
                     "admission": admission,
                     "rollout_ms_per_micro_batch": summary([x[0] / accum for x in r]),
                     "optimizer_step_ms": summary([x[1] for x in r]),
                     "optimizer_step_ms_per_micro_batch": summary([x[1] / accum for x in r])}
        if window:
            res[name]["engine_stats_last_run"] = dict(engines[name].stats)
    base = res[BASELINE]["rollout_ms_per_micro_batch"]
    base_step = res[BASELINE]["optimizer_step_ms_per_micro_batch"]["median_ms"]
    spread = (base["max_ms"] - base["min_ms"]) / base["median_ms"]
    losers = []
    for name, r in res.items():
        r["rollout_ratio_to_micro_batch"] = r["rollout_ms_per_micro_batch"]["median_ms"] / base["median_ms"]
        r["step_per_micro_batch_ratio_to_micro_batch"] = r["optimizer_step_ms_per_micro_batch"]["median_ms"] / base_step
        if name != BASELINE:
            r["beats_baseline_beyond_its_spread"] = r["rollout_ms_per_micro_batch"]["median_ms"] < base["median_ms"] * (1 - spread)
            if not r["beats_baseline_beyond_its_spread"]:
                losers.append(name)
    out = {"device": torch.cuda.get_device_name(0),
           "method": "events on the launch stream, one warm-up, variants alternating in one process, median of "
                     f"{args.repeats} with [min, max]",
           "setup": {"student": "0.6B shape", "teacher": "1.7B shape", "weights": "random", "lmbda": 1, "B": B, "T": T,
                     "on_policy_max_new_tokens": NEW, "prompt_lengths": list(PROMPTS), "temperature": 1.0, "top_k": 50,
                     "note": "random weights: no row reaches an EOS, every request runs its 256 tokens; the engine's refill "
                             "of rows that stop early is not exercised"},
           "baseline": BASELINE, "baseline_relative_spread": spread, "variants": res, "window_variants_that_lose": losers}
    print(json.dumps(out, indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for e in engines.values():
        e.close()
    if losers:
        raise SystemExit(f"window rollouts that do not beat {BASELINE} beyond its spread ({spread:.3f}): {losers}")


if __name__ == "__main__":
    main()
