"""GPU measurement (not a pytest): the MXFP8 decode step with gemv_rows=64 (sd_qwen3_mx_decode_step_wide on the 64-row
block-scaled GEMV of sd_gemv_mx.hip) against the steps the project already has.  Writes
profiles/decode_mx_wide_bench.json.

  (a) per token: Decoder.step on the 0.6B student and the 1.7B teacher shape (random weights), B in {16, 32, 64}, context 512,
      contiguous bf16 cache.  Variants: "mx_wide" (the new step), "mx_tile" (MXFP8 tile step), "bf16_wide" (the bf16 wide step)
      and, at B = 16, "mx_skinny".  Per cell and other variant: the ratio new / other and one boolean -- new <= other x (1 +
      that other variant's own relative spread).  Every cell is reported, true or false.  The new step's logits must be
      finite in every cell (exit status 1 if not).
  (b) per projection, the four projections of the two shapes: GPU time of sd_gemv_mxfp8_wide / _wide_swiglu at M in {16, 32,
      64} (norm and residual fused as the decode step uses them), beside sd_gemv_mxfp8 at M = 16 and sd_gemv_wide_bf16 /
      sd_gemv_wide_swiglu at the same M.  "flat in M" is answered per projection: time at M = 64 over time at M = 16 of the
      new kernel.  For K = 6144 (the 1.7B down projection, two column groups above 32 rows) that ratio is the cost of the
      second walk.  Every call takes the next of enough weight copies to exceed 512 MB, as the layers of a step do.
  (c) the engine: tests/bench_engine.py's workload (64 requests of 128 prompt tokens, budgets cycling 32 / 64 / 128 / 512, EOS
      disabled, the reference's sampling recipe) through generation_engine with ("skinny", "mxfp8", gemv_rows=64) at
      max_batch 32 and 64, beside max_batch = 32 "wide" on bf16 weights: useful tokens per second.
Method (tests/bench_decode_wide.py): events on the launch stream, one warm-up, the variants alternating in one process, the
median of 5 runs with [min, max]; (b) sums the library's per-launch events; (c) one event pair around a whole run.  No
figure is fixed in advance.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speech_distill_amd as sda  # noqa: E402
from speech_distill_amd import ops  # noqa: E402
from speech_distill_amd.generation import REFERENCE_SAMPLING, Decoder  # noqa: E402
from bench_decode_gemv import REPS, alternate, one_run_kernels  # noqa: E402
from bench_decode_mx import MODELS, copies, random_model, save  # noqa: E402
from bench_engine import BUDGETS, N_REQ, T, timed  # noqa: E402

dev = torch.device("cuda:0")
MX_WIDE = dict(decode_kernels="skinny", weight_dtype="mxfp8", gemv_rows=64)
VARIANTS = {"mx_wide": MX_WIDE, "mx_tile": dict(decode_kernels="tile", weight_dtype="mxfp8"),
            "bf16_wide": dict(decode_kernels="wide"), "mx_skinny": dict(decode_kernels="skinny", weight_dtype="mxfp8")}


def spread(t):
    return (t[2] - t[1]) / t[0]


def bench_step(res, min_s, out):
    ok, ctx, cells = True, 512, {}
    for name, dims in MODELS.items():
        m = random_model(dims())
        V = m.dims.vocab_size
        for B in (16, 32, 64):
            ids = torch.randint(0, V, (B, ctx), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
            tok = torch.randint(0, V, (B,), device=dev)
            pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            kinds = [k for k in VARIANTS if k != "mx_skinny" or B <= 16]
            decs = {k: Decoder(m, B, ctx + 256, **VARIANTS[k]) for k in kinds}
            for d in decs.values():
                d.prefill(ids, pos)
            finite = bool(torch.isfinite(decs["mx_wide"].step(tok, pos, ctx + 1).float()).all())
            t = alternate({k: (lambda d=d: d.step(tok, pos, ctx + 1)) for k, d in decs.items()}, min_s)
            row = {"model": name, "B": B, "context": ctx, "mx_wide_logits_finite": finite}
            for k, (med, lo, hi, it) in t.items():
                row[k] = {"us_per_step": med, "us_min": lo, "us_max": hi, "iters_per_run": it}
            for k in kinds[1:]:
                row[f"mx_wide_over_{k}"] = t["mx_wide"][0] / t[k][0]
                row[f"{k}_rel_spread"] = spread(t[k])
                cells[f"{name} B={B} mx_wide <= {k}"] = row[f"mx_wide_over_{k}"] <= 1.0 + row[f"{k}_rel_spread"]
            res["step"].append(row)
            ok = ok and finite
            print(f"{name} B={B:2d} ctx={ctx}: " + "  ".join(f"{k} {v[0]:8.1f} us [{v[1]:.1f}, {v[2]:.1f}]" for k, v in t.items()),
                  flush=True)
            del decs
            res["question"] = {"what": "new step <= other step x (1 + that other variant's own relative spread), per cell",
                               "cells": cells}
            save(res, out)
        del m
        torch.cuda.empty_cache()
    res["mx_wide_logits_finite_in_every_cell"] = ok
    return ok


def bench_projections(res, min_s, out):
    shapes = {"student_06b": (1024, 2048, 1024, 3072), "teacher_17b": (2048, 2048, 1024, 6144)}
    for model, (h, QD, KD, I) in shapes.items():
        for name, kind, N, K in (("qkv", "n", QD + 2 * KD, h), ("o", "r", h, QD), ("gate_up", "s", I, h), ("down", "r", h, I)):
            rows = 2 * N if kind == "s" else N
            nb = copies(rows * K * 2)
            w = torch.empty(nb, rows, K, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02)
            nq = copies(rows * K * 33 // 32)
            wq = torch.empty(nq, rows, K, dtype=torch.uint8, device=dev)
            ws = torch.empty(nq, rows, K // 32, dtype=torch.uint8, device=dev)
            for i in range(nq):
                wq[i], ws[i] = ops.mxfp8_quant(w[i % nb])
            gain = torch.ones(K, device=dev).bfloat16()
            x64 = torch.randn(64, K, device=dev).bfloat16()
            r64 = torch.randn(64, N, device=dev).bfloat16()
            i = [0, 0, 0]

            def nxt(slot, n):
                i[slot] = (i[slot] + 1) % n
                return i[slot]

            def mx(slot, M, wide):
                x, r, o = x64[:M], r64[:M], torch.empty(M, N, device=dev).bfloat16()
                if kind == "n":
                    return lambda: (lambda j: ops.gemv_mxfp8(x, wq[j], ws[j], norm=True, out=o, wide=wide))(nxt(slot, nq))
                if kind == "r":
                    return lambda: (lambda j: ops.gemv_mxfp8(x, wq[j], ws[j], residual=r, out=o, wide=wide))(nxt(slot, nq))
                return lambda: (lambda j: ops.gemv_mxfp8_swiglu(x, wq[j], ws[j], norm=True, wide=wide))(nxt(slot, nq))

            def bf16(slot, M):
                x, r, o = x64[:M], r64[:M], torch.empty(M, N, device=dev).bfloat16()
                if kind == "n":
                    return lambda: ops.gemv_bf16(x, w[nxt(slot, nb)], norm_gain=gain, out=o, wide=True)
                if kind == "r":
                    return lambda: ops.gemv_bf16(x, w[nxt(slot, nb)], residual=r, out=o, wide=True)
                return lambda: ops.gemv_swiglu(x, w[nxt(slot, nb)], norm_gain=gain, wide=True)

            per_m = {}
            for M in (16, 32, 64):
                t = alternate({"mx_wide": mx(0, M, True), "mx_16_rows_at_M16": mx(1, 16, False), "bf16_wide": bf16(2, M)}, min_s,
                              run=one_run_kernels)
                nbytes = {"mx_wide": rows * K * 33 // 32, "mx_16_rows_at_M16": rows * K * 33 // 32, "bf16_wide": rows * K * 2}
                row = {"model": model, "proj": name, "M": M, "N": N, "K": K}
                for k, (med, lo, hi, it) in t.items():
                    row[k] = {"us": med, "us_min": lo, "us_max": hi, "iters_per_run": it, "weight_bytes": nbytes[k],
                              "weight_GBps": nbytes[k] / med / 1e3}
                row["mx_wide_over_mx_16_rows"] = t["mx_wide"][0] / t["mx_16_rows_at_M16"][0]
                row["mx_wide_over_bf16_wide"] = t["mx_wide"][0] / t["bf16_wide"][0]
                per_m[M] = t["mx_wide"][0]
                res["projections"].append(row)
                print(f"{model:11s} {name:8s} M={M:2d} N={N:6d} K={K:4d}: " + "  ".join(
                    f"{k} {v[0]:7.1f} us [{v[1]:.1f}, {v[2]:.1f}]" for k, v in t.items()), flush=True)
            res["flat_in_M"].append({"model": model, "proj": name, "K": K, "column_groups_at_M64": 2 if K > 4096 else 1,
                                     "mx_wide_us": per_m, "M32_over_M16": per_m[32] / per_m[16],
                                     "M64_over_M16": per_m[64] / per_m[16]})
            del w, wq, ws
            save(res, out)


def bench_engine(res, out):
    m = random_model(sda.Qwen3Dims.student_06b())
    V = m.dims.vocab_size
    ids = torch.randint(0, V, (N_REQ, T), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pool = m.kv_page_pool(196)      # 64 rows x 3 pages (128 + 512 positions) + the parking page

    def engine(max_batch, **mode):
        def run():
            eng = m.generation_engine(pool, max_batch=max_batch, **mode)
            for i in range(N_REQ):
                eng.submit(ids[i], max_new_tokens=BUDGETS[i], seed=i, **REFERENCE_SAMPLING)
            eng.run()
            stats = dict(eng.stats)
            eng.close()
            return {"sampler_steps": stats["iterations"], "decode_steps": stats["decode_steps"], "prefills": stats["prefills"]}
        return run
    fns = {"bf16_wide_max_batch_32": engine(32, decode_kernels="wide"), "mx_wide_max_batch_32": engine(32, **MX_WIDE),
           "mx_wide_max_batch_64": engine(64, **MX_WIDE)}
    runs, info = {k: [] for k in fns}, {}
    for fn in fns.values():
        timed(fn)                                   # warm-up
    for _ in range(REPS):
        for k, fn in fns.items():
            s, info[k] = timed(fn)
            runs[k].append(s)
    useful = sum(BUDGETS)
    eng = {"shape": "student 0.6B", "workload": {"requests": N_REQ, "prompt_tokens": T, "budgets_cycle": [32, 64, 128, 512],
                                                 "useful_tokens": useful, "eos": None, "sampling": REFERENCE_SAMPLING}}
    for k in fns:
        med = statistics.median(runs[k])
        eng[k] = {"seconds": med, "seconds_min": min(runs[k]), "seconds_max": max(runs[k]), "useful_tokens_per_s": useful / med,
                  **info[k]}
        print(f"engine {k}: {med:7.3f} s [{min(runs[k]):.3f}, {max(runs[k]):.3f}]  {useful / med:9.1f} useful tokens/s  {info[k]}",
              flush=True)
    res["engine"] = eng
    save(res, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0, help="least duration of one timed run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_mx_wide_bench.json"))
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--skip_projections", action="store_true")
    ap.add_argument("--skip_engine", action="store_true")
    ap.add_argument("--merge", default=None, help="a result file of an earlier partial run (--skip_*) to add this run's parts to")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "min_seconds_per_run": {},
           "method": {"all": "one warm-up, variants alternating in one process, median of 5 runs [min, max], runs sized to "
                             "min_seconds_per_run of wall time",
                      "step": "one event pair on the launch stream around the steps of a run; contiguous bf16 cache, context "
                              "512, random weights",
                      "projections": "the library's launch profiler: an event pair on the launch stream around EVERY launch, "
                                     "summed over the launches of a call; weight copies rotate through more than 512 MB",
                      "engine": "one event pair on the launch stream around a whole run of 64 requests"},
           "step": [], "projections": [], "flat_in_M": []}
    if args.merge:
        import json
        with open(args.merge) as f:
            res = json.load(f)
    ok = True
    if not args.skip_step:
        res["step"], res["min_seconds_per_run"]["step"] = [], args.min_seconds
        ok = bench_step(res, args.min_seconds, args.out)
    if not args.skip_projections:
        res["projections"], res["flat_in_M"], res["min_seconds_per_run"]["projections"] = [], [], args.min_seconds
        bench_projections(res, args.min_seconds, args.out)
    if not args.skip_engine:
        bench_engine(res, args.out)
    print("wrote", save(res, args.out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
