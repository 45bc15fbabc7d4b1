"""GPU measurement (not a pytest, not a bench.py line): the frozen teacher at inference precision "bf16" (gain-folded) against
"mxfp8", written to profiles/teacher_mxfp8_bench.json.

  1. teacher forward + top-K alone at C2 (B=4, T=512, lm_head on the 1 536 loss rows) and C5 (B=64, T=512, all rows), the
     two precisions ALTERNATED in the same process, device-synchronised timing over >= 1 s of work per precision, spread
     from repeats; per-symbol times from ops.prof_symbols(); FLOP/s of the MX GEMMs against the ~5 PF dense FP8 peak;
  2. the C2 micro-step shaped as bench.py shapes it (teacher on a side stream beside the student, loss, backward) with both
     teachers, through the public classes;
  3. on the C2 synthetic batch: mean KL(bf16 teacher || mxfp8 teacher) at temperature 1 over the loss rows, top-1 and
     top-128-set agreement.  RECORDED, NOT ASSERTED: the weights are random-init N(0, 0.02) (no trained checkpoint is
     available offline), which says little about a trained teacher.

usage: python tests/bench_teacher_mx.py [--parts 1,2,3] [--out profiles/teacher_mxfp8_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speech_distill_amd as sda  # noqa: E402
from speech_distill_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
VOCAB, SPEECH_LO, TOP_K = 159488, 152927, 128
FP8_PEAK = 5.0e15


def build(dims, seed):
    m = sda.HipQwen3ForCausalLM(dims, device=dev, init_std=0)
    m.flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(seed))
    for p in m._params.values():
        if p.dim() == 1:
            p.data.fill_(1.0)
    return m


def synthetic_batch(B, T):  # bench.py synthetic_batch: uniform ids, 25 % text prefix masked to -100, then speech ids
    g = torch.Generator().manual_seed(1234)
    ids = torch.randint(0, VOCAB, (B, T), generator=g)
    n_text = T // 4
    ids[:, n_text] = SPEECH_LO
    ids[:, n_text + 1:] = torch.randint(SPEECH_LO, VOCAB, (B, T - n_text - 1), generator=g)
    labels = ids.clone()
    labels[:, :n_text] = -100
    return ids.to(dev), torch.ones(B, T, dtype=torch.long, device=dev), labels.to(dev)


def timed(fn, min_seconds=1.0):
    """ms per call over at least `min_seconds` of device work (device-synchronised wall clock)."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(3, int(min_seconds / max(time.perf_counter() - t0, 1e-4)) + 1)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, n


def alternate(fns, repeats=5):
    """fns: {name: callable}; the candidates run in turn, `repeats` rounds -> {name: {median, min, max, calls}}."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    calls = {}
    for _ in range(repeats):
        for k, f in fns.items():
            ms, calls[k] = timed(f)
            res[k].append(ms)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls_per_repeat": calls[k]}
            for k, v in res.items()}


def symbols(fn):
    fn()
    torch.cuda.synchronize()
    ops.prof_begin()
    fn()
    torch.cuda.synchronize()
    ops.prof_end()
    return {k: {"ms": v[0], "work": v[1], "launches": v[2], "kind": v[3]} for k, v in ops.prof_symbols().items()}


def part1(teacher, out):
    for tag, B, T, use_rows in (("c2", 4, 512, True), ("c5", 64, 512, False)):
        ids, am, labels = synthetic_batch(B, T)
        rows = ops.loss_rows(labels)[0] if use_rows else None

        teacher.set_inference_precision("mxfp8")
        teacher._mx_params()  # quantise the weights once, outside the timing; set_inference_precision would drop them
        fns = {}
        for prec in ("bf16", "mxfp8"):
            def f(prec=prec):
                teacher.inference_precision = prec  # switch without dropping the prepared weights
                with torch.no_grad():
                    lg = teacher(input_ids=ids, attention_mask=am, logit_rows=rows, padding_checked=True).logits
                    return ops.logsoftmax_topk(lg, TOP_K, VOCAB)
            fns[prec] = f
        r = alternate(fns)
        syms = {p: symbols(fns[p]) for p in fns}
        mx = [v for k, v in syms["mxfp8"].items() if k.startswith("gemm_mx_kernel")]
        d = teacher.dims
        M = B * T
        flop = 2.0 * M * d.num_hidden_layers * (d.hidden_size * (d.q_dim + 2 * d.kv_dim) + d.q_dim * d.hidden_size +
                                                3 * d.hidden_size * d.intermediate_size)
        mx_ms = sum(v["ms"] for v in mx)
        r["speedup_median"] = r["bf16"]["median_ms"] / r["mxfp8"]["median_ms"]
        r["mx_gemm_ms_per_pass"] = mx_ms
        r["mx_gemm_algorithmic_flops_per_s"] = flop / (mx_ms * 1e-3) if mx_ms else None
        r["mx_gemm_fraction_of_5pf_fp8_peak"] = (flop / (mx_ms * 1e-3) / FP8_PEAK) if mx_ms else None
        r["symbols"] = syms
        out["teacher_forward_topk_" + tag] = r
        print(tag, json.dumps({k: v for k, v in r.items() if k != "symbols"}), flush=True)
        for p in syms:
            top = sorted(syms[p].items(), key=lambda kv: -kv[1]["ms"])[:8]
            print("  ", p, [(k, round(v["ms"], 3), v["launches"]) for k, v in top], flush=True)
    teacher.inference_precision = "bf16"


def part2(teacher, out):
    student = build(sda.Qwen3Dims.student_06b(), 0)
    loss_fn = sda.DistillationLoss(temperature=2.0, alpha=0.5, inplace_grad=True)
    ids, am, labels = synthetic_batch(4, 512)
    side = ops.concurrent_stream(dev, "teacher")

    def step():
        student.zero_grad()
        rows, row_labels = ops.loss_rows(labels)
        with torch.no_grad():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                lg = teacher(input_ids=ids, attention_mask=am, logit_rows=rows, concurrent=True).logits
                tv, ti = ops.logsoftmax_topk(lg, TOP_K, VOCAB)
        logits = student(input_ids=ids, attention_mask=am, labels=labels, logit_rows=rows, concurrent=True).logits
        torch.cuda.current_stream().wait_stream(side)
        total = loss_fn.forward_rows(logits, row_labels, teacher_top_k_v=tv, teacher_top_k_i=ti)[0]
        total.backward()
        return total
    teacher.inference_precision = "mxfp8"
    teacher._mx_params()
    fns = {}
    for prec in ("bf16", "mxfp8"):
        def f(prec=prec):
            teacher.inference_precision = prec
            return step()
        fns[prec] = f
    r = alternate(fns)
    r["speedup_median"] = r["bf16"]["median_ms"] / r["mxfp8"]["median_ms"]
    r["tokens_per_s"] = {p: 4 * 512 / (r[p]["median_ms"] * 1e-3) for p in ("bf16", "mxfp8")}
    out["c2_micro_step"] = r
    print("c2_micro_step", json.dumps(r), flush=True)
    teacher.inference_precision = "bf16"


def part3(teacher, out):
    ids, am, labels = synthetic_batch(4, 512)
    rows = ops.loss_rows(labels)[0]
    lg = {}
    teacher.inference_precision = "mxfp8"
    teacher._mx_params()
    for prec in ("bf16", "mxfp8"):
        teacher.inference_precision = prec
        with torch.no_grad():
            lg[prec] = teacher(input_ids=ids, attention_mask=am, logit_rows=rows).logits.float()
    lp, lq = torch.log_softmax(lg["bf16"], -1), torch.log_softmax(lg["mxfp8"], -1)
    kl = float((lp.exp() * (lp - lq)).sum(-1).mean())
    top1 = float((lg["bf16"].argmax(-1) == lg["mxfp8"].argmax(-1)).float().mean())
    ta, tb = lg["bf16"].topk(TOP_K, -1).indices, lg["mxfp8"].topk(TOP_K, -1).indices
    member = torch.zeros_like(lg["bf16"], dtype=torch.bool).scatter_(1, ta, True)
    overlap = float(member.gather(1, tb).float().mean())
    ent = float(-(lp.exp() * lp).sum(-1).mean())
    out["agreement_c2_random_init"] = {
        "mean_kl_bf16_vs_mxfp8_T1": kl, "top1_agreement": top1, "top128_set_overlap": overlap, "rows": int(rows.numel()),
        "mean_entropy_bf16": ent,
        "note": "random-init N(0, 0.02) weights: near-uniform output distributions; says little about a trained teacher"}
    print("agreement", json.dumps(out["agreement_c2_random_init"]), flush=True)
    teacher.inference_precision = "bf16"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teacher_mxfp8_bench.json"))
    args = ap.parse_args()
    sda.load_lib()
    teacher = build(sda.Qwen3Dims.teacher_17b(), 1)
    teacher.eval().requires_grad_(False)
    out = {"device": torch.cuda.get_device_name(0), "method": "precisions alternated in one process; device-synchronised "
           "wall clock over >= 1 s per measurement; median / min / max of 5 repeats"}
    if os.path.exists(args.out):
        out = dict(json.load(open(args.out)), **out)
    parts = {int(p) for p in args.parts.split(",")}
    if 1 in parts:
        part1(teacher, out)
    if 2 in parts:
        part2(teacher, out)
    if 3 in parts:
        part3(teacher, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
