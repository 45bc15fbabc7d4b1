"""GPU measurement (not a pytest, not a bench.py line): the tail-bucket loss kernels and sd_topk_tail beside the kernels
they stand next to, and a config-2 micro-step, written to profiles/gjsd_tail_bench.json.

  1. kernels at R = 1 536 rows, V = 159 488, bf16, T = 2, K = 128, forward and backward: sd_gjsd_tail_*_rows in its three
     modes beside sd_gjsd_topk_*_rows and the sparse forward-KL pair sd_kdloss_*_rows on the same top-128 teacher, and the
     dense sd_gjsd_*_rows (reverse KL and JSD) on the dense teacher.  us per call, the ratios, and effective TB/s counting
     each row once per kernel.  The yardstick kernels are the parent commit's, untouched.
  2. sd_topk_tail beside sd_logsoftmax_topk on the same logits: the price of the second read of the teacher's rows.
  3. one config-2 micro-step (B = 4, T = 512, random weights, prompts of 64, live teacher): "reverse_kl_tail" at
     top_k = 128 (top-K extraction + tail) against "reverse_kl" at top_k = 0, split into teacher + student forward, loss,
     backward.
  4. part 1 again at K = 512 and K = 1024 (K = 1024 runs the 1024-thread forward).

No threshold is fixed in advance: the figures are the result.  Method: events on the launch stream around each timed
region, one warm-up, the variants alternating in one process, median of 5 with [min, max].

usage: python tests/bench_gjsd_tail.py [--parts 1,2,3,4] [--out profiles/gjsd_tail_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speech_distill_amd as sda  # noqa: E402
from speech_distill_amd import ops  # noqa: E402
from bench_gjsd import REPEATS, SPEECH_LO, VOCAB, alternate, build, dev  # noqa: E402

TAIL_MODES = {"forward_kl_tail": 0, "reverse_kl_tail": 1, "jsd_tail": 2}


def part1(out, K=128):
    lib = sda.load_lib()
    R, V, T, alpha, beta = 1536, VOCAB, 2.0, 0.5, 0.5
    g = torch.Generator(device=dev).manual_seed(0)
    s = (torch.randn(R, V, generator=g, device=dev) * 3).bfloat16()
    t = (torch.randn(R, V, generator=g, device=dev) * 3).bfloat16()
    labels = torch.randint(0, V, (R,), generator=g, device=dev)
    tv, ti = ops.logsoftmax_topk(t, K)
    tau = ops.topk_tail(t, ti, T)
    grad = torch.empty_like(s)
    res8 = torch.empty(8, dtype=torch.float32, device=dev)
    nbytes = dict({k: lib.sd_gjsd_tail_stats_bytes(R) for k in TAIL_MODES}, jsd_topk=lib.sd_gjsd_topk_stats_bytes(R),
                  forward_kl_topk=lib.sd_kdloss_stats_bytes(R, 1), reverse_kl_dense=lib.sd_gjsd_stats_bytes(R),
                  jsd_dense=lib.sd_gjsd_stats_bytes(R))
    stats = {k: torch.empty(n, dtype=torch.uint8, device=dev) for k, n in nbytes.items()}   # kept fwd -> bwd
    st = torch.cuda.current_stream().cuda_stream
    S, Tl, TV, TI, TA, L, G, O = (x.data_ptr() for x in (s, t, tv, ti, tau, labels, grad, res8))
    Q = {k: x.data_ptr() for k, x in stats.items()}

    def ok(rc):
        assert rc == 0, rc

    def tail_fwd(name, mode):
        return lambda: ok(lib.sd_gjsd_tail_fwd_rows(S, TV, TI, TA, L, Q[name], O, R, V, K, T, alpha, beta, mode, 0, st))

    def tail_bwd(name, mode):
        return lambda: ok(lib.sd_gjsd_tail_bwd_rows(S, TV, TI, TA, L, Q[name], O, None, G, R, V, K, T, alpha, beta, mode, 0, st))
    fwd = {k: tail_fwd(k, m) for k, m in TAIL_MODES.items()}
    bwd = {k: tail_bwd(k, m) for k, m in TAIL_MODES.items()}
    fwd.update({"jsd_topk": lambda: ok(lib.sd_gjsd_topk_fwd_rows(S, TV, TI, L, Q["jsd_topk"], O, R, V, K, T, alpha, beta, 0, st)),
                "forward_kl_topk": lambda: ok(lib.sd_kdloss_fwd_rows(S, None, TV, TI, L, Q["forward_kl_topk"], O, R, V, K, T, alpha, 0, st)),
                "reverse_kl_dense": lambda: ok(lib.sd_gjsd_fwd_rows(S, Tl, L, Q["reverse_kl_dense"], O, R, V, T, alpha, beta, 1, 0, st)),
                "jsd_dense": lambda: ok(lib.sd_gjsd_fwd_rows(S, Tl, L, Q["jsd_dense"], O, R, V, T, alpha, beta, 2, 0, st))})
    bwd.update({"jsd_topk": lambda: ok(lib.sd_gjsd_topk_bwd_rows(S, TV, TI, L, Q["jsd_topk"], O, None, G, R, V, K, T, alpha, beta, 0, st)),
                "forward_kl_topk": lambda: ok(lib.sd_kdloss_bwd_rows(S, None, TV, TI, L, Q["forward_kl_topk"], O, None, G, R, V, K, T,
                                                                     alpha, 0, st)),
                "reverse_kl_dense": lambda: ok(lib.sd_gjsd_bwd_rows(S, Tl, L, Q["reverse_kl_dense"], O, None, G, R, V, T, alpha, beta, 1, 0, st)),
                "jsd_dense": lambda: ok(lib.sd_gjsd_bwd_rows(S, Tl, L, Q["jsd_dense"], O, None, G, R, V, T, alpha, beta, 2, 0, st))})
    moved = (lambda k, what: (2 if k.endswith("dense") else 1) + (1 if what == "bwd" else 0))
    r = {"tail_min": float(tau.min()), "tail_max": float(tau.max())}
    for what, fns in (("fwd", fwd), ("bwd", bwd)):
        # (every backward reads the stats its own forward left and the N of the last forward: all have N = R here)
        r.update({f"{what}_{k}": v for k, v in alternate(fns, calls=5).items()})
        for k in fns:
            e = r[f"{what}_{k}"]
            e["us"] = e["median_ms"] * 1e3
            e["effective_TB_per_s"] = moved(k, what) * R * V * 2 / (e["median_ms"] * 1e-3) / 1e12
            for ref in ("jsd_topk", "forward_kl_topk", "reverse_kl_dense", "jsd_dense"):
                e["ratio_to_" + ref] = e["median_ms"] / r[f"{what}_{ref}"]["median_ms"]
    out[f"kernels_R1536_V159488_bf16_T2_K{K}"] = r
    print(json.dumps(r, indent=1), flush=True)


def part2(out, K=128):
    lib = sda.load_lib()
    R, V, T = 1536, VOCAB, 2.0
    g = torch.Generator(device=dev).manual_seed(0)
    t = (torch.randn(R, V, generator=g, device=dev) * 3).bfloat16()
    tv, ti = ops.logsoftmax_topk(t, K)
    tau = torch.empty(R, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def ok(rc):
        assert rc == 0, rc
    fns = {"logsoftmax_topk": lambda: ok(lib.sd_logsoftmax_topk(t.data_ptr(), tv.data_ptr(), ti.data_ptr(), None, R, V, V, K, 0, st)),
           "topk_tail": lambda: ok(lib.sd_topk_tail(t.data_ptr(), ti.data_ptr(), tau.data_ptr(), R, V, V, K, T, 0, st))}
    r = alternate(fns, calls=5)
    for k, e in r.items():
        e["us"] = e["median_ms"] * 1e3
        e["effective_TB_per_s"] = R * V * 2 / (e["median_ms"] * 1e-3) / 1e12
    r["topk_tail_over_logsoftmax_topk"] = r["topk_tail"]["median_ms"] / r["logsoftmax_topk"]["median_ms"]
    out[f"teacher_side_R1536_V159488_bf16_T2_K{K}"] = r
    print(json.dumps(r, indent=1), flush=True)


def part3(out):
    B, T, PROMPT, K, TEMP = 4, 512, 64, 128, 2.0
    student, teacher = build(sda.Qwen3Dims.student_06b(), 0), build(sda.Qwen3Dims.teacher_17b(), 1)
    teacher.eval().requires_grad_(False)
    g = torch.Generator().manual_seed(1234)
    ids = torch.randint(SPEECH_LO, VOCAB, (B, T), generator=g)
    ids[:, :PROMPT] = torch.randint(0, SPEECH_LO, (B, PROMPT), generator=g)
    labels = ids.clone()
    labels[:, :PROMPT] = -100
    batch = {"input_ids": ids.to(dev), "attention_mask": torch.ones(B, T, dtype=torch.long, device=dev), "labels": labels.to(dev)}
    fns = {"reverse_kl_tail_k128": sda.DistillationLoss(temperature=TEMP, alpha=0.5, inplace_grad=True, divergence="reverse_kl_tail"),
           "reverse_kl_dense_k0": sda.DistillationLoss(temperature=TEMP, alpha=0.5, inplace_grad=True, divergence="reverse_kl")}
    side = ops.concurrent_stream(dev, "teacher")

    def phases(name):
        """-> ms of each phase of one micro-step (events on the main stream; the teacher runs beside the student)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        student.zero_grad()
        b = batch
        rows, row_labels = ops.loss_rows(b["labels"])
        ev[0].record()
        tl = None
        kw = {}
        with torch.no_grad():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                tl = teacher(input_ids=b["input_ids"], attention_mask=b["attention_mask"], logit_rows=rows, concurrent=True).logits
                if name == "reverse_kl_tail_k128":
                    tv, ti = ops.logsoftmax_topk(tl, K, VOCAB)
                    kw = dict(teacher_top_k_v=tv, teacher_top_k_i=ti, teacher_top_k_tail=ops.topk_tail(tl, ti, TEMP, VOCAB))
                    tl = None
        sl = student(input_ids=b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"], logit_rows=rows,
                     concurrent=True).logits
        torch.cuda.current_stream().wait_stream(side)
        ev[1].record()
        total = fns[name].forward_rows(sl, row_labels, teacher_logits=tl, **kw)[0]
        ev[2].record()
        total.backward()
        ev[3].record()
        ev[3].synchronize()
        names = ("teacher_student_forward", "loss", "backward")
        return {n: ev[i].elapsed_time(ev[i + 1]) for i, n in enumerate(names)}
    for k in fns:
        phases(k)   # warm-up
    runs = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k in fns:
            runs[k].append(phases(k))
    r = {}
    for k, lst in runs.items():
        r[k] = {n: {"median_ms": statistics.median(x[n] for x in lst), "min_ms": min(x[n] for x in lst),
                    "max_ms": max(x[n] for x in lst)} for n in lst[0]}
        r[k]["micro_step_median_ms"] = statistics.median(sum(x.values()) for x in lst)
    r["loss_rows"] = B * (T - PROMPT)
    out["c2_micro_step_reverse_kl_tail_vs_reverse_kl"] = r
    print(json.dumps(r, indent=1), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gjsd_tail_bench.json"))
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
    if 4 in parts:
        for K in (512, 1024):
            part1(out, K)
    if 3 in parts:
        part3(out)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
