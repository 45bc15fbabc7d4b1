"""GPU measurement (not a pytest): the decode step on MXFP8 weights against the bf16 step, and the block-scaled GEMV against
the bf16 GEMV.  Writes profiles/decode_mx_bench.json.

  (a) per token: Decoder.step for weight_dtype in {bf16, mxfp8} x decode_kernels in {tile, skinny} on the 0.6B student and
      the 1.7B teacher shape (random weights), B in {1, 8, 16}, context 512, contiguous bf16 cache.  The logits of the two
      mxfp8 kinds must be finite in every cell (exit status 1 if not).
  (b) per projection, the eight projection shapes of the two models, M in {1, 16}: GPU time and weight bytes per second of
      sd_gemv_mxfp8 / sd_gemv_mxfp8_swiglu (norm and residual fused as the decode step uses them) and of sd_gemv_bf16 /
      sd_gemv_swiglu on the same shape.  Every call takes the next of enough weight copies to exceed 512 MB (of its own
      format), as the layers of a step do: no call finds its weights in a cache.
Method (tests/bench_paged.py, tests/bench_decode_gemv.py): events on the launch stream, one warm-up, the variants
alternating in one process, the median of 5 runs with [min, max]; (b) sums the library's per-launch events.
The question the run answers, written into the file: is the mxfp8 skinny step on the 1.7B shape at most the bf16 skinny
step measured beside it, allowing the bf16 step's own relative spread?
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speech_distill_amd as sda  # noqa: E402
from speech_distill_amd import ops  # noqa: E402
from speech_distill_amd.generation import Decoder  # noqa: E402
from bench_decode_gemv import alternate, one_run_kernels  # noqa: E402

dev = torch.device("cuda:0")
MODELS = {"student_06b": sda.Qwen3Dims.student_06b, "teacher_17b": sda.Qwen3Dims.teacher_17b}


def random_model(dims):
    m = sda.HipQwen3ForCausalLM(dims, device=dev, init_std=0)
    with torch.no_grad():
        m.flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(0))
        for p in m._params.values():
            if p.dim() == 1:
                p.fill_(1.0)
    return m.eval().requires_grad_(False)


def save(res, out):
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    return out


def bench_step(res, min_s, out):
    ok, ctx = True, 512
    for name, dims in MODELS.items():
        m = random_model(dims())
        V = m.dims.vocab_size
        for B in (1, 8, 16):
            ids = torch.randint(0, V, (B, ctx), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
            tok = torch.randint(0, V, (B,), device=dev)
            pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            decs = {f"{wd}_{k}": Decoder(m, B, ctx + 256, decode_kernels=k, weight_dtype=wd)
                    for wd in ("bf16", "mxfp8") for k in ("tile", "skinny")}
            finite = {}
            for k, d in decs.items():
                d.prefill(ids, pos)
                finite[k] = bool(torch.isfinite(d.step(tok, pos, ctx + 1).float()).all())
            t = alternate({k: (lambda d=d: d.step(tok, pos, ctx + 1)) for k, d in decs.items()}, min_s)
            row = {"model": name, "B": B, "context": ctx}
            for k, (med, lo, hi, it) in t.items():
                row[k] = {"us_per_step": med, "us_min": lo, "us_max": hi, "iters_per_run": it, "logits_finite": finite[k]}
            row["mxfp8_over_bf16_skinny"] = t["mxfp8_skinny"][0] / t["bf16_skinny"][0]
            row["mxfp8_over_bf16_tile"] = t["mxfp8_tile"][0] / t["bf16_tile"][0]
            row["bf16_skinny_rel_spread"] = (t["bf16_skinny"][2] - t["bf16_skinny"][1]) / t["bf16_skinny"][0]
            res["step"].append(row)
            ok = ok and finite["mxfp8_tile"] and finite["mxfp8_skinny"]
            print(f"{name} B={B:2d} ctx={ctx}: " + "  ".join(f"{k} {v[0]:8.1f} us [{v[1]:.1f}, {v[2]:.1f}]" for k, v in t.items())
                  + f"  mxfp8/bf16 skinny x{row['mxfp8_over_bf16_skinny']:.3f}", flush=True)
            del decs
            save(res, out)
        del m
        torch.cuda.empty_cache()
    rows = [r for r in res["step"] if r["model"] == "teacher_17b"]
    res["question"] = {"what": "mxfp8 skinny step on the 1.7B shape <= bf16 skinny step x (1 + its own relative spread)",
                       "cells": {f"B={r['B']}": r["mxfp8_over_bf16_skinny"] <= 1.0 + r["bf16_skinny_rel_spread"] for r in rows}}
    res["mxfp8_logits_finite_in_every_cell"] = ok
    return ok


def copies(nbytes_each):
    """how many matrices of that size exceed 512 MB (two at least)"""
    return max(2, -(-(512 << 20) // nbytes_each))


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
            for M in (1, 16):
                x = torch.randn(M, K, device=dev).bfloat16()
                r = torch.randn(M, N, device=dev).bfloat16()
                o = torch.empty(M, N, device=dev).bfloat16()
                i = [0, 0]

                def nxt(slot, n):
                    i[slot] = (i[slot] + 1) % n
                    return i[slot]
                if kind == "n":
                    fns = {"bf16": lambda: ops.gemv_bf16(x, w[nxt(0, nb)], norm_gain=gain, out=o),
                           "mxfp8": lambda: (lambda j: ops.gemv_mxfp8(x, wq[j], ws[j], norm=True, out=o))(nxt(1, nq))}
                elif kind == "r":
                    fns = {"bf16": lambda: ops.gemv_bf16(x, w[nxt(0, nb)], residual=r, out=o),
                           "mxfp8": lambda: (lambda j: ops.gemv_mxfp8(x, wq[j], ws[j], residual=r, out=o))(nxt(1, nq))}
                else:
                    fns = {"bf16": lambda: ops.gemv_swiglu(x, w[nxt(0, nb)], norm_gain=gain),
                           "mxfp8": lambda: (lambda j: ops.gemv_mxfp8_swiglu(x, wq[j], ws[j], norm=True))(nxt(1, nq))}
                t = alternate(fns, min_s, run=one_run_kernels)
                nbytes = {"bf16": rows * K * 2, "mxfp8": rows * K * 33 // 32}
                row = {"model": model, "proj": name, "M": M, "N": N, "K": K}
                for k, (med, lo, hi, it) in t.items():
                    row[k] = {"us": med, "us_min": lo, "us_max": hi, "iters_per_run": it, "weight_bytes": nbytes[k],
                              "weight_GBps": nbytes[k] / med / 1e3}
                row["mxfp8_over_bf16"] = t["mxfp8"][0] / t["bf16"][0]
                res["projections"].append(row)
                print(f"{model:11s} {name:8s} M={M:2d} N={N:6d} K={K:4d}: " + "  ".join(
                    f"{k} {v[0]:7.1f} us [{v[1]:.1f}, {v[2]:.1f}] {nbytes[k] / v[0] / 1e3:6.0f} GB/s" for k, v in t.items())
                      + f"  x{row['mxfp8_over_bf16']:.3f}", flush=True)
            del w, wq, ws
            save(res, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0, help="least duration of one timed run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_mx_bench.json"))
    ap.add_argument("--skip_projections", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": 5, "min_seconds_per_run": args.min_seconds,
           "method": {"all": "one warm-up, variants alternating in one process, median of 5 runs [min, max], runs sized to "
                             "min_seconds_per_run of wall time",
                      "step": "one event pair on the launch stream around the steps of a run; contiguous bf16 cache, context "
                              "512, random weights",
                      "projections": "the library's launch profiler: an event pair on the launch stream around EVERY launch, "
                                     "summed over the launches of a call; weight copies rotate through more than 512 MB"},
           "step": [], "projections": []}
    ok = bench_step(res, args.min_seconds, args.out)
    if not args.skip_projections:
        bench_projections(res, args.min_seconds, args.out)
    print("wrote", save(res, args.out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
