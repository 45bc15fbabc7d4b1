"""GPU measurement (not a pytest, not a bench.py line): the reverse-KL / skewed-JSD loss kernels beside the forward-KL
ones, and what an on-policy micro-step costs, written to profiles/gjsd_bench.json.

  1. kernels at R = 1 536 rows, V = 159 488, bf16, T = 2: sd_gjsd_fwd_rows / sd_gjsd_bwd_rows for "reverse_kl" and "jsd"
     (beta 0.5) beside the dense sd_kdloss_fwd_rows / sd_kdloss_bwd_rows (the yardstick).  us per call, the ratio to the
     yardstick, and effective TB/s counting each row once per kernel (forward: 2 rows read; backward: 2 read, 1 written)
     -- the second sweep of the gjsd forward is NOT counted, so its figure is the rate a one-sweep kernel would need.
  2. one config-2 micro-step (B = 4, T = 512, random weights, prompts of 64, jsd) split into rollout, teacher + student
     forward, loss, backward, at lmbda 0 (no rollout) and 1, with decode_kernels "tile" and "skinny".

Method: events on the launch stream around each timed region, one warm-up, the variants alternating in one process,
median of 5 with [min, max].  No pass / fail condition.

usage: python tests/bench_gjsd.py [--parts 1,2] [--out profiles/gjsd_bench.json]"""
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

dev = torch.device("cuda:0")
VOCAB, SPEECH_LO = 159488, 152927
REPEATS = 5


def event_ms(fn, calls=1):
    """ms per call of `calls` back-to-back calls between two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(fns, calls=1):
    """{name: callable} -> {name: {median_ms, min_ms, max_ms}}: one warm-up each, then REPEATS rounds in turn."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, f in fns.items():
            res[k].append(event_ms(f, calls))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def part1(out):
    lib = sda.load_lib()
    R, V, T, alpha = 1536, VOCAB, 2.0, 0.5
    g = torch.Generator(device=dev).manual_seed(0)
    s = (torch.randn(R, V, generator=g, device=dev) * 3).bfloat16()
    t = (torch.randn(R, V, generator=g, device=dev) * 3).bfloat16()
    labels = torch.randint(0, V, (R,), generator=g, device=dev)
    grad = torch.empty_like(s)
    res8 = torch.empty(8, dtype=torch.float32, device=dev)
    kd_stats = torch.empty(lib.sd_kdloss_stats_bytes(R, 1), dtype=torch.uint8, device=dev)
    gj_stats = {m: torch.empty(lib.sd_gjsd_stats_bytes(R), dtype=torch.uint8, device=dev) for m in (1, 2)}  # kept fwd -> bwd
    st = torch.cuda.current_stream().cuda_stream
    P = [x.data_ptr() for x in (s, t, labels, grad, res8, kd_stats)]
    Q = {m: x.data_ptr() for m, x in gj_stats.items()}

    def ok(rc):
        assert rc == 0, rc
    fwd = {"forward_kl": lambda: ok(lib.sd_kdloss_fwd_rows(P[0], P[1], None, None, P[2], P[5], P[4], R, V, 0, T, alpha, 0, st))}
    bwd = {"forward_kl": lambda: ok(lib.sd_kdloss_bwd_rows(P[0], P[1], None, None, P[2], P[5], P[4], None, P[3], R, V, 0, T,
                                                            alpha, 0, st))}
    for name, mode in (("reverse_kl", 1), ("jsd", 2)):
        fwd[name] = lambda mode=mode: ok(lib.sd_gjsd_fwd_rows(P[0], P[1], P[2], Q[mode], P[4], R, V, T, alpha, 0.5, mode, 0, st))
        bwd[name] = lambda mode=mode: ok(lib.sd_gjsd_bwd_rows(P[0], P[1], P[2], Q[mode], P[4], None, P[3], R, V, T, alpha, 0.5,
                                                              mode, 0, st))
    r = {}
    for what, fns, rows_moved in (("fwd", fwd, 2), ("bwd", bwd, 3)):
        # every backward reads the stats its own forward left (one buffer each; all forwards have run by then)
        r.update({f"{what}_{k}": v for k, v in alternate(fns, calls=5).items()})
        for k in fns:
            e = r[f"{what}_{k}"]
            e["us"] = e["median_ms"] * 1e3
            e["effective_TB_per_s"] = rows_moved * R * V * 2 / (e["median_ms"] * 1e-3) / 1e12
            e["ratio_to_forward_kl"] = e["median_ms"] / r[f"{what}_forward_kl"]["median_ms"]
    out["kernels_R1536_V159488_bf16_T2"] = r
    print(json.dumps(r, indent=1), flush=True)


def build(dims, seed):
    m = sda.HipQwen3ForCausalLM(dims, device=dev, init_std=0)
    m.flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(seed))
    for p in m._params.values():
        if p.dim() == 1:
            p.data.fill_(1.0)
    return m


def part2(out):
    B, T, PROMPT = 4, 512, 64
    student, teacher = build(sda.Qwen3Dims.student_06b(), 0), build(sda.Qwen3Dims.teacher_17b(), 1)
    teacher.eval().requires_grad_(False)
    g = torch.Generator().manual_seed(1234)
    ids = torch.randint(SPEECH_LO, VOCAB, (B, T), generator=g)
    ids[:, :PROMPT] = torch.randint(0, SPEECH_LO, (B, PROMPT), generator=g)
    labels = ids.clone()
    labels[:, :PROMPT] = -100
    batch = {"input_ids": ids.to(dev), "attention_mask": torch.ones(B, T, dtype=torch.long, device=dev),
             "labels": labels.to(dev)}
    loss_fn = sda.DistillationLoss(temperature=2.0, alpha=0.5, inplace_grad=True, divergence="jsd", beta=0.5)
    side = ops.concurrent_stream(dev, "teacher")

    def phases(lmbda, kernels):
        """-> ms of each phase of one micro-step (events on the main stream; the teacher runs beside the student)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        student.zero_grad()
        b = batch
        ev[0].record()
        if lmbda:
            b = on_policy.rollout(student.generate, batch, {"max_new_tokens": T, "temperature": 1.0, "top_k": 50,
                                                            "decode_kernels": kernels}, seed=7)
        ev[1].record()
        rows, row_labels = ops.loss_rows(b["labels"])
        with torch.no_grad():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                tl = teacher(input_ids=b["input_ids"], attention_mask=b["attention_mask"], logit_rows=rows, concurrent=True).logits
        sl = student(input_ids=b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"], logit_rows=rows,
                     concurrent=True).logits
        torch.cuda.current_stream().wait_stream(side)
        ev[2].record()
        total = loss_fn.forward_rows(sl, row_labels, teacher_logits=tl)[0]
        ev[3].record()
        total.backward()
        ev[4].record()
        ev[4].synchronize()
        names = ("rollout", "teacher_student_forward", "loss", "backward")
        return {n: ev[i].elapsed_time(ev[i + 1]) for i, n in enumerate(names)}
    variants = {"lmbda0": (0, "tile"), "lmbda1_tile": (1, "tile"), "lmbda1_skinny": (1, "skinny")}
    for v in variants.values():
        phases(*v)   # warm-up
    runs = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, v in variants.items():
            runs[k].append(phases(*v))
    r = {}
    for k, lst in runs.items():
        r[k] = {n: {"median_ms": statistics.median(x[n] for x in lst), "min_ms": min(x[n] for x in lst),
                    "max_ms": max(x[n] for x in lst)} for n in lst[0]}
        r[k]["micro_step_median_ms"] = statistics.median(sum(x.values()) for x in lst)
    r["rollout_new_tokens"] = T - PROMPT
    out["c2_micro_step_jsd"] = r
    print(json.dumps(r, indent=1), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gjsd_bench.json"))
    args = ap.parse_args()
    sda.load_lib()
    out = {"device": torch.cuda.get_device_name(0), "method": "events on the launch stream, one warm-up, variants alternating in "
           "one process, median of 5 with [min, max]"}
    if os.path.exists(args.out):
        out = dict(json.load(open(args.out)), **out)
    parts = {int(p) for p in args.parts.split(",")}
    if 1 in parts:
        part1(out)
    if 2 in parts:
        part2(out)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
