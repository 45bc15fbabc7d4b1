"""GPU measurement (not a pytest, not a bench.py line): the top-K Jensen-Shannon loss kernels beside the sparse forward-KL
and the dense JSD ones, and a config-2 micro-step with each, written to profiles/gjsd_topk_bench.json.

  1. kernels at R = 1 536 rows, V = 159 488, bf16, T = 2, K = 128, forward and backward: sd_gjsd_topk_*_rows beside
     sd_kdloss_*_rows on the same top-128 teacher (the same bytes) and sd_gjsd_*_rows "jsd" on the dense teacher.  us per
     call, both ratios, and effective TB/s counting each row once per kernel.
     One condition, derived: the new forward reads one row once where the dense JSD forward reads two rows twice, so its
     median must lie below the MINIMUM of the dense JSD forward measured in the same process (asserted).
  2. one config-2 micro-step (B = 4, T = 512, random weights, prompts of 64, live teacher), "jsd_topk" at top_k = 128
     against "jsd" at top_k = 0, split into teacher + student forward (the top-K extraction included), loss, backward.
  3. part 1 again at K = 512 and K = 1024 (the duplicate merge reads K entries per entry; K = 1024 runs the 1024-thread
     forward).

Method: events on the launch stream around each timed region, one warm-up, the variants alternating in one process,
median of 5 with [min, max].

usage: python tests/bench_gjsd_topk.py [--parts 1,2,3] [--out profiles/gjsd_topk_bench.json]"""
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


def part1(out, K=128):
    lib = sda.load_lib()
    R, V, T, alpha, beta = 1536, VOCAB, 2.0, 0.5, 0.5
    g = torch.Generator(device=dev).manual_seed(0)
    s = (torch.randn(R, V, generator=g, device=dev) * 3).bfloat16()
    t = (torch.randn(R, V, generator=g, device=dev) * 3).bfloat16()
    labels = torch.randint(0, V, (R,), generator=g, device=dev)
    tv, ti = ops.logsoftmax_topk(t, K)
    grad = torch.empty_like(s)
    res8 = torch.empty(8, dtype=torch.float32, device=dev)
    stats = {"jsd_topk": torch.empty(lib.sd_gjsd_topk_stats_bytes(R), dtype=torch.uint8, device=dev),
             "forward_kl_topk": torch.empty(lib.sd_kdloss_stats_bytes(R, 1), dtype=torch.uint8, device=dev),
             "jsd_dense": torch.empty(lib.sd_gjsd_stats_bytes(R), dtype=torch.uint8, device=dev)}   # kept fwd -> bwd
    st = torch.cuda.current_stream().cuda_stream
    S, Tl, TV, TI, L, G, O = (x.data_ptr() for x in (s, t, tv, ti, labels, grad, res8))
    Q = {k: x.data_ptr() for k, x in stats.items()}

    def ok(rc):
        assert rc == 0, rc
    fwd = {"jsd_topk": lambda: ok(lib.sd_gjsd_topk_fwd_rows(S, TV, TI, L, Q["jsd_topk"], O, R, V, K, T, alpha, beta, 0, st)),
           "forward_kl_topk": lambda: ok(lib.sd_kdloss_fwd_rows(S, None, TV, TI, L, Q["forward_kl_topk"], O, R, V, K, T, alpha, 0, st)),
           "jsd_dense": lambda: ok(lib.sd_gjsd_fwd_rows(S, Tl, L, Q["jsd_dense"], O, R, V, T, alpha, beta, 2, 0, st))}
    bwd = {"jsd_topk": lambda: ok(lib.sd_gjsd_topk_bwd_rows(S, TV, TI, L, Q["jsd_topk"], O, None, G, R, V, K, T, alpha, beta, 0, st)),
           "forward_kl_topk": lambda: ok(lib.sd_kdloss_bwd_rows(S, None, TV, TI, L, Q["forward_kl_topk"], O, None, G, R, V, K, T,
                                                                alpha, 0, st)),
           "jsd_dense": lambda: ok(lib.sd_gjsd_bwd_rows(S, Tl, L, Q["jsd_dense"], O, None, G, R, V, T, alpha, beta, 2, 0, st))}
    rows_moved = {"fwd": {"jsd_topk": 1, "forward_kl_topk": 1, "jsd_dense": 2}, "bwd": {"jsd_topk": 2, "forward_kl_topk": 2, "jsd_dense": 3}}
    r = {}
    for what, fns in (("fwd", fwd), ("bwd", bwd)):
        # (every backward reads the stats its own forward left and the N of the last forward: all have N = R here)
        r.update({f"{what}_{k}": v for k, v in alternate(fns, calls=5).items()})
        for k in fns:
            e = r[f"{what}_{k}"]
            e["us"] = e["median_ms"] * 1e3
            e["effective_TB_per_s"] = rows_moved[what][k] * R * V * 2 / (e["median_ms"] * 1e-3) / 1e12
            e["ratio_to_forward_kl_topk"] = e["median_ms"] / r[f"{what}_forward_kl_topk"]["median_ms"]
            e["ratio_to_jsd_dense"] = e["median_ms"] / r[f"{what}_jsd_dense"]["median_ms"]
    kd = r["fwd_forward_kl_topk"]
    r["fwd_jsd_topk_above_forward_kl_max_by_us"] = (r["fwd_jsd_topk"]["median_ms"] - kd["max_ms"]) * 1e3
    r["fwd_forward_kl_topk_spread_us"] = (kd["max_ms"] - kd["min_ms"]) * 1e3
    out[f"kernels_R1536_V159488_bf16_T2_K{K}"] = r
    print(json.dumps(r, indent=1), flush=True)
    return r


def part2(out):
    B, T, PROMPT, K = 4, 512, 64, 128
    student, teacher = build(sda.Qwen3Dims.student_06b(), 0), build(sda.Qwen3Dims.teacher_17b(), 1)
    teacher.eval().requires_grad_(False)
    g = torch.Generator().manual_seed(1234)
    ids = torch.randint(SPEECH_LO, VOCAB, (B, T), generator=g)
    ids[:, :PROMPT] = torch.randint(0, SPEECH_LO, (B, PROMPT), generator=g)
    labels = ids.clone()
    labels[:, :PROMPT] = -100
    batch = {"input_ids": ids.to(dev), "attention_mask": torch.ones(B, T, dtype=torch.long, device=dev), "labels": labels.to(dev)}
    fns = {"jsd_topk_k128": sda.DistillationLoss(temperature=2.0, alpha=0.5, inplace_grad=True, divergence="jsd_topk", beta=0.5),
           "jsd_dense_k0": sda.DistillationLoss(temperature=2.0, alpha=0.5, inplace_grad=True, divergence="jsd", beta=0.5)}
    side = ops.concurrent_stream(dev, "teacher")

    def phases(name):
        """-> ms of each phase of one micro-step (events on the main stream; the teacher runs beside the student)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        student.zero_grad()
        b = batch
        rows, row_labels = ops.loss_rows(b["labels"])
        ev[0].record()
        tl = tv = ti = None
        with torch.no_grad():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                tl = teacher(input_ids=b["input_ids"], attention_mask=b["attention_mask"], logit_rows=rows, concurrent=True).logits
                if name == "jsd_topk_k128":
                    tv, ti = ops.logsoftmax_topk(tl, K, VOCAB)
                    tl = None
        sl = student(input_ids=b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"], logit_rows=rows,
                     concurrent=True).logits
        torch.cuda.current_stream().wait_stream(side)
        ev[1].record()
        total = fns[name].forward_rows(sl, row_labels, teacher_logits=tl, teacher_top_k_v=tv, teacher_top_k_i=ti)[0]
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
    out["c2_micro_step_jsd_topk_vs_jsd"] = r
    print(json.dumps(r, indent=1), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gjsd_topk_bench.json"))
    args = ap.parse_args()
    sda.load_lib()
    out = {"device": torch.cuda.get_device_name(0), "method": "events on the launch stream, one warm-up, variants alternating in "
           "one process, median of 5 with [min, max]"}
    if os.path.exists(args.out):
        out = dict(json.load(open(args.out)), **out)
    parts = {int(p) for p in args.parts.split(",")}
    r1 = part1(out) if 1 in parts else None
    if 3 in parts:   # the duplicate merge walks K entries per entry: its cost where K is large (1024: the 1024-thread forward)
        for K in (512, 1024):
            part1(out, K)
    if 2 in parts:
        part2(out)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    if r1 is not None:   # the one derived condition (after the file is written: a miss is a finding, and its figures are kept)
        assert r1["fwd_jsd_topk"]["median_ms"] < r1["fwd_jsd_dense"]["min_ms"], (r1["fwd_jsd_topk"], r1["fwd_jsd_dense"])


if __name__ == "__main__":
    main()
