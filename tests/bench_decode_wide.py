"""GPU measurement (not a pytest): the "wide" decode step (sd_qwen3_decode_step_wide on the MFMA weight-streaming kernels of
sd_gemv_wide.hip) against the tile step and the skinny step.  Writes profiles/decode_wide_bench.json.

  (a) per token: Decoder.step for decode_kernels in {tile, skinny (B <= 16), wide} on the 0.6B student and the 1.7B teacher
      shape (random weights), B in {1, 8, 16, 32, 64}, context 512, contiguous bf16 cache.  The wide logits must be finite
      in every cell (exit status 1 if not).
  (b) per projection, the four projections and the lm_head of the two shapes, M in {1, 16, 64}: GPU time and weight bytes per
      second of sd_gemv_wide_bf16 / sd_gemv_wide_swiglu (norm and residual fused as the decode step uses them), beside
      sd_gemv_bf16 / sd_gemv_swiglu where M <= 16.  Every call takes the next of enough weight copies to exceed 512 MB, as
      the layers of a step do: no call finds its weights in a cache.
  (d) where the rows of x live: the teacher's o, gate_up and down at M = 64 as ONE call (B fragments of all 64 rows re-read
      from L2) against 2 passes of 32 and 4 passes of 16 columns over the same weights.
  (c) the engine: tests/bench_engine.py's workload (64 requests of 128 prompt tokens, budgets cycling 32 / 64 / 128 / 512, EOS
      disabled, the reference's sampling recipe) through generation_engine with max_batch = 8 "skinny" and with max_batch =
      32 "wide": useful tokens per second.
Method (tests/bench_decode_mx.py): events on the launch stream, one warm-up, the variants alternating in one process, the
median of 5 runs with [min, max]; (b) sums the library's per-launch events; (c) one event pair around a whole run.
The question the run answers, written into the file per cell as true / false: is the wide step at most the tile step
measured beside it x (1 + the tile variant's own relative spread) at B = 32 and B = 64 on both shapes, and the same against
the skinny step at B = 16?  No ratio is fixed in advance.
"""
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
from speech_distill_amd.generation import REFERENCE_SAMPLING, Decoder  # noqa: E402
from bench_decode_gemv import REPS, alternate, one_run_kernels, projections  # noqa: E402
from bench_decode_mx import MODELS, copies, random_model, save  # noqa: E402
from bench_engine import BUDGETS, N_REQ, T, timed  # noqa: E402

dev = torch.device("cuda:0")


def spread(t):
    return (t[2] - t[1]) / t[0]


def bench_step(res, min_s, out):
    ok, ctx = True, 512
    for name, dims in MODELS.items():
        m = random_model(dims())
        V = m.dims.vocab_size
        for B in (1, 8, 16, 32, 64):
            ids = torch.randint(0, V, (B, ctx), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
            tok = torch.randint(0, V, (B,), device=dev)
            pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            kinds = ("tile", "skinny", "wide") if B <= 16 else ("tile", "wide")
            decs = {k: Decoder(m, B, ctx + 256, decode_kernels=k) for k in kinds}
            for d in decs.values():
                d.prefill(ids, pos)
            finite = bool(torch.isfinite(decs["wide"].step(tok, pos, ctx + 1).float()).all())
            t = alternate({k: (lambda d=d: d.step(tok, pos, ctx + 1)) for k, d in decs.items()}, min_s)
            row = {"model": name, "B": B, "context": ctx, "wide_logits_finite": finite}
            for k, (med, lo, hi, it) in t.items():
                row[k] = {"us_per_step": med, "us_min": lo, "us_max": hi, "iters_per_run": it}
            row["wide_over_tile"] = t["wide"][0] / t["tile"][0]
            row["tile_rel_spread"] = spread(t["tile"])
            if "skinny" in t:
                row["wide_over_skinny"] = t["wide"][0] / t["skinny"][0]
                row["skinny_rel_spread"] = spread(t["skinny"])
            res["step"].append(row)
            ok = ok and finite
            print(f"{name} B={B:2d} ctx={ctx}: " + "  ".join(f"{k} {v[0]:8.1f} us [{v[1]:.1f}, {v[2]:.1f}]" for k, v in t.items())
                  + f"  wide/tile x{row['wide_over_tile']:.3f}", flush=True)
            del decs
            save(res, out)
        del m
        torch.cuda.empty_cache()
    cells = {}
    for r in res["step"]:
        if r["B"] in (32, 64):
            cells[f"{r['model']} B={r['B']} wide <= tile"] = r["wide_over_tile"] <= 1.0 + r["tile_rel_spread"]
        if r["B"] == 16:
            cells[f"{r['model']} B=16 wide <= skinny"] = r["wide_over_skinny"] <= 1.0 + r["skinny_rel_spread"]
    res["question"] = {"what": "wide step <= tile step x (1 + the tile variant's relative spread) at B = 32 and 64; wide step "
                               "<= skinny step x (1 + the skinny variant's relative spread) at B = 16", "cells": cells}
    res["wide_logits_finite_in_every_cell"] = ok
    return ok


def bench_projections(res, min_s, out):
    shapes = {"student_06b": (1024, 2048, 1024, 3072), "teacher_17b": (2048, 2048, 1024, 6144)}
    for model, dims in shapes.items():
        for name, kind, N, K in projections(*dims):
            rows = 2 * N if kind == "s" else N
            nb = copies(rows * K * 2)
            w = torch.empty(nb, rows, K, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02)
            gain = torch.ones(K, device=dev).bfloat16()
            for M in (1, 16, 64):
                x = torch.randn(M, K, device=dev).bfloat16()
                r = torch.randn(M, N, device=dev).bfloat16()
                o = torch.empty(M, N, device=dev).bfloat16()
                i = [0, 0]

                def nxt(slot):
                    i[slot] = (i[slot] + 1) % nb
                    return w[i[slot]]

                def call(slot, wide):
                    if kind == "n":
                        return lambda: ops.gemv_bf16(x, nxt(slot), norm_gain=gain, out=o, wide=wide)
                    if kind == "r":
                        return lambda: ops.gemv_bf16(x, nxt(slot), residual=r, out=o, wide=wide)
                    return lambda: ops.gemv_swiglu(x, nxt(slot), norm_gain=gain, wide=wide)
                fns = {"wide": call(0, True)}
                if M <= 16:
                    fns["skinny"] = call(1, False)
                t = alternate(fns, min_s, run=one_run_kernels)
                nbytes = rows * K * 2
                row = {"model": model, "proj": name, "M": M, "N": N, "K": K, "weight_bytes": nbytes}
                for k, (med, lo, hi, it) in t.items():
                    row[k] = {"us": med, "us_min": lo, "us_max": hi, "iters_per_run": it, "weight_GBps": nbytes / med / 1e3}
                res["projections"].append(row)
                print(f"{model:11s} {name:8s} M={M:2d} N={N:6d} K={K:4d}: " + "  ".join(
                    f"{k} {v[0]:7.1f} us [{v[1]:.1f}, {v[2]:.1f}] {nbytes / v[0] / 1e3:6.0f} GB/s" for k, v in t.items()), flush=True)
            del w
            save(res, out)


def bench_placement(res, min_s, out):
    """Where the rows of x live, the alternative that needs no other kernel: M = 64 in passes of 32 or 16 columns over the
    same weights (2 or 4 calls on row slices; the later passes find the weights where the first left them, in L2 / Infinity
    Cache or in HBM) against the ONE call that re-reads the B fragments of all 64 rows from L2.  GPU time of the launches."""
    h, QD, KD, I = 2048, 2048, 1024, 6144
    res["x_placement"] = []
    for name, kind, N, K in (("o", "r", h, QD), ("gate_up", "s", I, h), ("down", "r", h, I)):
        rows = 2 * N if kind == "s" else N
        nb = copies(rows * K * 2)
        w = torch.empty(nb, rows, K, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02)
        gain = torch.ones(K, device=dev).bfloat16()
        x = torch.randn(64, K, device=dev).bfloat16()
        r = torch.randn(64, N, device=dev).bfloat16()
        o = torch.empty(64, N, device=dev).bfloat16()
        i = [0, 0, 0]

        def passes(slot, step):
            def fn():
                i[slot] = (i[slot] + 1) % nb
                for m0 in range(0, 64, step):
                    if kind == "r":
                        ops.gemv_bf16(x[m0:m0 + step], w[i[slot]], residual=r[m0:m0 + step], out=o[m0:m0 + step], wide=True)
                    else:
                        ops.gemv_swiglu(x[m0:m0 + step], w[i[slot]], norm_gain=gain, wide=True)
            return fn
        t = alternate({"one_call_64": passes(0, 64), "two_passes_32": passes(1, 32), "four_passes_16": passes(2, 16)}, min_s,
                      run=one_run_kernels)
        row = {"model": "teacher_17b", "proj": name, "M": 64, "N": N, "K": K, "weight_bytes": rows * K * 2}
        for k, (med, lo, hi, it) in t.items():
            row[k] = {"us": med, "us_min": lo, "us_max": hi, "iters_per_run": it}
        res["x_placement"].append(row)
        print(f"x placement {name:8s} N={N} K={K}: " + "  ".join(f"{k} {v[0]:7.1f} us [{v[1]:.1f}, {v[2]:.1f}]" for k, v in t.items()),
              flush=True)
        del w
        save(res, out)


def bench_engine(res, out):
    m = random_model(sda.Qwen3Dims.student_06b())
    V = m.dims.vocab_size
    ids = torch.randint(0, V, (N_REQ, T), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pool = m.kv_page_pool(100)      # 32 rows x 3 pages (128 + 512 positions) + the parking page

    def engine(max_batch, kernels):
        def run():
            eng = m.generation_engine(pool, max_batch=max_batch, decode_kernels=kernels)
            for i in range(N_REQ):
                eng.submit(ids[i], max_new_tokens=BUDGETS[i], seed=i, **REFERENCE_SAMPLING)
            eng.run()
            stats = dict(eng.stats)
            eng.close()
            return {"sampler_steps": stats["iterations"], "decode_steps": stats["decode_steps"], "prefills": stats["prefills"]}
        return run
    fns = {"skinny_max_batch_8": engine(8, "skinny"), "wide_max_batch_32": engine(32, "wide")}
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
    eng["wide32_over_skinny8_time"] = eng["wide_max_batch_32"]["seconds"] / eng["skinny_max_batch_8"]["seconds"]
    res["engine"] = eng
    save(res, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0, help="least duration of one timed run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_wide_bench.json"))
    ap.add_argument("--skip_projections", action="store_true")
    ap.add_argument("--skip_engine", action="store_true")
    ap.add_argument("--only_placement", action="store_true",
                    help="add (d) to the committed result file (profiles/decode_wide_bench.json) and write it to --out")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "min_seconds_per_run": args.min_seconds,
           "method": {"all": "one warm-up, variants alternating in one process, median of 5 runs [min, max], runs sized to "
                             "min_seconds_per_run of wall time",
                      "step": "one event pair on the launch stream around the steps of a run; contiguous bf16 cache, context "
                              "512, random weights",
                      "projections": "the library's launch profiler: an event pair on the launch stream around EVERY launch, "
                                     "summed over the launches of a call; weight copies rotate through more than 512 MB",
                      "engine": "one event pair on the launch stream around a whole run of 64 requests"},
           "step": [], "projections": []}
    if args.only_placement:
        with open(os.path.join(ROOT, "profiles", "decode_wide_bench.json")) as f:
            res = json.load(f)
        bench_placement(res, args.min_seconds, args.out)
        print("wrote", save(res, args.out))
        return 0
    ok = bench_step(res, args.min_seconds, args.out)
    if not args.skip_projections:
        bench_projections(res, args.min_seconds, args.out)
        bench_placement(res, args.min_seconds, args.out)
    if not args.skip_engine:
        bench_engine(res, args.out)
    print("wrote", save(res, args.out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
