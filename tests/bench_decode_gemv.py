"""GPU measurement (not a pytest): the weight-streaming GEMV kernels of the decode step against the tile GEMMs they
replace.  Writes profiles/decode_gemv_bench.json.

  (a) per projection, student (h 1024, QD 2048, I 3072) and teacher (h 2048, I 6144) shapes, M in {1, 4, 16}: time and
      weight bytes per second of sd_gemv_bf16 / sd_gemv_swiglu (norm and residual fused as the decode step uses them) and
      of the tile path on the same shape (sd_rmsnorm_fwd + sd_gemm_bf16, sd_gemm_swiglu), beside the streaming read rate
      of tests/bench_hbm.py's top-k pass from the same session.  These are GPU times of the launches themselves (the
      library's per-launch events): a Python call costs more host time than one of these kernels runs.  Every call of a
      run takes the next of enough weight copies to exceed 512 MB, as the 28 layers of a step do: no call finds its
      weights in a cache.
  (b) per token: Decoder.step with decode_kernels "tile" and "skinny" on the 0.6B student shape (random weights), context
      512, B in {1, 8, 16}, with the kernel launches of one step counted by the library's launch profiler.
Method: events on the launch stream, one warm-up, the two variants alternating in one process, the median of 5 runs of at
least 1 s each; the min-max spread is written next to every figure.
The one condition: the skinny step is faster than the tile step at B = 1 and at B = 8 (exit status 1 if not).
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
from speech_distill_amd.generation import Decoder  # noqa: E402

dev = torch.device("cuda:0")
REPS = 5
V = sda.Qwen3Dims.student_06b().vocab_size   # the student's and the teacher's (qwen3.py)


def one_run(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us per call


def one_run_kernels(fn, iters):
    """us of GPU time per call: the library's launch profiler (an event pair around every launch, on the launch stream)
    summed over the launches of `iters` calls, 1000 calls at a time.  A Python call costs more host time than these
    kernels run, so a stream-level window would time the host."""
    ms, done = 0.0, 0
    while done < iters:
        n = min(1000, iters - done)
        ops.prof_begin()
        for _ in range(n):
            fn()
        ms += sum(t for t, _, _ in ops.prof_end().values())
        done += n
    return ms / iters * 1e3


def alternate(fns, min_s, run=one_run):
    """{name: (median us, min us, max us, iterations per run)}: one warm-up each, then REPS rounds in which the variants
    take turns, every run sized from the warm-up's wall time to last at least min_s seconds."""
    iters = {}
    for k, fn in fns.items():
        one_run(fn, 3)
        iters[k] = max(3, int(min_s * 1e6 / one_run(fn, 10)) + 1)
    runs = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            runs[k].append(run(fn, iters[k]))
    return {k: (statistics.median(v), min(v), max(v), iters[k]) for k, v in runs.items()}


def weights(N, K):
    """enough [N,K] matrices to exceed 512 MB (two at least)"""
    n = max(2, -(-(512 << 20) // (N * K * 2)))
    return torch.empty(n, N, K, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02)


def projections(h, QD, KD, I):
    """(name, kind, N, K): kind n = fused norm, r = residual, s = fused norm + SwiGLU (N = I)."""
    return [("qkv", "n", QD + 2 * KD, h), ("o", "r", h, QD), ("gate_up", "s", I, h), ("down", "r", h, I), ("lm_head", "n", V, h)]


def save(res):
    out = os.path.join(ROOT, "profiles", "decode_gemv_bench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    return out


def bench_projections(res, min_s):
    for model, dims in (("student", (1024, 2048, 1024, 3072)), ("teacher", (2048, 2048, 1024, 6144))):
        for name, kind, N, K in projections(*dims):
            rows = 2 * N if kind == "s" else N
            w = weights(rows, K)
            gain = torch.ones(K, device=dev).bfloat16()
            for M in (1, 4, 16):
                x = torch.randn(M, K, device=dev).bfloat16()
                r = torch.randn(M, N, device=dev).bfloat16()
                out = torch.empty(M, N, device=dev).bfloat16()
                i = [0, 0]

                def nxt(slot):
                    i[slot] = (i[slot] + 1) % w.shape[0]
                    return w[i[slot]]
                if kind == "n":
                    fns = {"gemv": lambda: ops.gemv_bf16(x, nxt(0), norm_gain=gain, out=out),
                           "tile": lambda: ops.gemm(ops.rmsnorm_fwd(x, gain)[0], nxt(1), out=out)}
                elif kind == "r":
                    fns = {"gemv": lambda: ops.gemv_bf16(x, nxt(0), residual=r, out=out),
                           "tile": lambda: ops.gemm(x, nxt(1), residual=r, out=out)}
                else:
                    try:    # the decode step's rule: sd_gemm_swiglu, else GEMM + sd_swiglu_fwd
                        ops.gemm_swiglu(x, w[0], save_gu=False)
                        tile = lambda: ops.gemm_swiglu(ops.rmsnorm_fwd(x, gain)[0], nxt(1), save_gu=False)  # noqa: E731
                    except sda.SdHipError:
                        tile = lambda: ops.swiglu_fwd(ops.gemm(ops.rmsnorm_fwd(x, gain)[0], nxt(1)))        # noqa: E731
                    fns = {"gemv": lambda: ops.gemv_swiglu(x, nxt(0), norm_gain=gain), "tile": tile}
                t = alternate(fns, min_s, run=one_run_kernels)
                nbytes = rows * K * 2
                row = {"model": model, "proj": name, "M": M, "N": N, "K": K, "weight_bytes": nbytes}
                for k, (med, lo, hi, it) in t.items():
                    row[k] = {"us": med, "us_min": lo, "us_max": hi, "iters_per_run": it, "weight_GBps": nbytes / med / 1e3}
                row["tile_over_gemv"] = t["tile"][0] / t["gemv"][0]
                res["projections"].append(row)
                print(f"{model:7s} {name:8s} M={M:2d} N={N:6d} K={K:4d}: gemv {t['gemv'][0]:8.1f} us [{t['gemv'][1]:.1f}, "
                      f"{t['gemv'][2]:.1f}] {nbytes / t['gemv'][0] / 1e3:6.0f} GB/s   tile {t['tile'][0]:8.1f} us "
                      f"[{t['tile'][1]:.1f}, {t['tile'][2]:.1f}] {nbytes / t['tile'][0] / 1e3:6.0f} GB/s", flush=True)
            del w
            save(res)


def bench_stream(res):
    import bench_hbm
    R, K = 1536, 128     # the read stream of tests/bench_hbm.py
    logits = (torch.randn(R, V, device=dev) * 2).bfloat16()
    us = bench_hbm.timeit(lambda: ops.logsoftmax_topk(logits, K, V))
    res["stream_read"] = {"what": "tests/bench_hbm.py: log-softmax + top-128 over 1536 x 159488 bf16", "us": us,
                          "GBps": R * V * 2 / us / 1e3}
    print(f"streaming read (bench_hbm top-k pass): {us:7.1f} us  {R * V * 2 / us / 1e3:7.0f} GB/s", flush=True)


def student():
    m = sda.HipQwen3ForCausalLM(sda.Qwen3Dims.student_06b(), device=dev, init_std=0)
    with torch.no_grad():
        m.flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(0))
        for p in m._params.values():
            if p.dim() == 1:
                p.fill_(1.0)
    return m.eval()


def launches(dec, tok, pos, ctx):
    ops.prof_begin()
    dec.step(tok, pos, ctx + 1)
    torch.cuda.synchronize()
    return int(sum(c for _, _, c in ops.prof_end().values()))


def bench_step(res, min_s):
    m = student()
    ok = True
    ctx = 512
    for B in (1, 8, 16):
        ids = torch.randint(0, V, (B, ctx), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
        tok = torch.randint(0, V, (B,), device=dev)
        pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        decs = {k: Decoder(m, B, ctx + 256, decode_kernels=k) for k in ("tile", "skinny")}
        for d in decs.values():
            d.prefill(ids, pos)
        t = alternate({k: (lambda d=d: d.step(tok, pos, ctx + 1)) for k, d in decs.items()}, min_s)
        row = {"B": B, "context": ctx}
        for k, (med, lo, hi, it) in t.items():
            row[k] = {"us_per_step": med, "us_min": lo, "us_max": hi, "iters_per_run": it,
                      "launches_per_step": launches(decs[k], tok, pos, ctx)}
        row["tile_over_skinny"] = t["tile"][0] / t["skinny"][0]
        res["step"].append(row)
        print(f"step B={B:2d} ctx={ctx}: tile {t['tile'][0]:8.1f} us [{t['tile'][1]:.1f}, {t['tile'][2]:.1f}] "
              f"({row['tile']['launches_per_step']} launches)   skinny {t['skinny'][0]:8.1f} us [{t['skinny'][1]:.1f}, "
              f"{t['skinny'][2]:.1f}] ({row['skinny']['launches_per_step']} launches)   x{row['tile_over_skinny']:.2f}",
              flush=True)
        if B in (1, 8):
            ok = ok and t["skinny"][0] < t["tile"][0]
        del decs
    res["skinny_faster_at_B1_and_B8"] = ok
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0, help="least duration of one timed run")
    ap.add_argument("--skip_projections", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "min_seconds_per_run": args.min_seconds,
           "method": {"all": "one warm-up, variants alternating in one process, median of 5 runs [min, max], runs sized to "
                             "min_seconds_per_run of wall time",
                      "step": "one event pair on the launch stream around the steps of a run",
                      "projections": "the library's launch profiler: an event pair on the launch stream around EVERY launch, "
                                     "summed over the launches of a call (GPU time without the host's gaps)",
                      "stream_read": "tests/bench_hbm.py timeit: one event pair around 20 calls"},
           "projections": [], "step": []}
    bench_stream(res)
    ok = bench_step(res, args.min_seconds)
    save(res)
    if not args.skip_projections:
        bench_projections(res, args.min_seconds)
    print("wrote", save(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
