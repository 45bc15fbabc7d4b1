"""GPU measurement (not a pytest): the decode cache-step kernels of this build against those of another build of the
library (the commit before the kernels were moved onto the shared device functions of csrc/sd_kv_dev.cuh).  Writes
profiles/kv_step_refactor_bench.json.

    python tests/bench_kv_step_refactor.py --parent_lib <the other build's libsd_hip.so>

The two libraries run in FRESH child processes (SD_HIP_LIB), parent / new / parent / new ... five times each; a child
measures every row once and prints one JSON line.  Rows, all GPU time by the library's launch profiler (an event pair around
every launch):
  - the cache step alone at the 0.6B head shape (Hq 16, Hkv 8): the three split launches (sd_qknorm_rope_append* +
    sd_attn_decode*) and the one fused launch (sd_cache_step), the method of tests/bench_decode_fused.py part (b) -- B = 1,
    context 512, contiguous; B = 8, context 2048 on bf16 pages and on MXFP8 pages;
  - the decode-attention launches of a step of fork([0] * 8) over a history of 2048 (0.6B shape, bf16 pages), private and
    shared: the cell of tests/bench_fork_shared.py.
Criterion per row: the new build's median may exceed the parent's maximum by no more than the parent's own spread
(max - min) of this call.  Exit status 1 if a row misses it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
CALLS = 3000   # calls per cache-step row and child


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import speech_distill_amd as sda
    from speech_distill_amd import ops
    from bench_decode_gemv import one_run_kernels
    from bench_decode_fused import model
    from bench_fork_shared import cell
    dev = torch.device("cuda:0")
    Hq, Hkv, D = 16, 8, 128
    out = {}
    for kind, B, ctx in (("contiguous", 1, 512), ("bf16_pages", 8, 2048), ("mxfp8_pages", 8, 2048)):
        cap = ctx + 256
        g = torch.Generator(device=dev).manual_seed(1)
        qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=dev, generator=g).bfloat16()
        gain = torch.ones(D, device=dev).bfloat16()
        cos, sin = ops.rope_tables(cap, dev)
        pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        n_pages = B * cap // 256
        table = None if kind == "contiguous" else \
            torch.randperm(n_pages, device=dev, generator=g).to(torch.int32).reshape(B, cap // 256).contiguous()
        rows = (B, cap) if kind == "contiguous" else (n_pages, 256)
        if kind == "mxfp8_pages":
            planes = []
            for _ in range(2):
                data = torch.randint(1, 256, (*rows, Hkv * D), device=dev, generator=g, dtype=torch.int32)
                data = torch.where((data & 0x7F) == 0x7F, torch.full_like(data, 0x3C), data).to(torch.uint8)  # no e4m3 NaN
                planes += [data, torch.randint(118, 130, (*rows, Hkv * 4), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)]
            planes = tuple(planes)
        else:
            planes = tuple((torch.randn(*rows, Hkv * D, device=dev, generator=g) * 0.5).bfloat16() for _ in range(2))
        ws = torch.empty(ops.load_lib().sd_cache_step_workspace_bytes(B, Hq, Hkv, cap), dtype=torch.uint8, device=dev)
        tickets = torch.zeros(B, Hkv, dtype=torch.int32, device=dev)

        def split():
            if kind == "contiguous":
                q = ops.qknorm_rope_append(qkv, gain, gain, cos, sin, pos, planes[0], planes[1], Hq, Hkv)
                return ops.attn_decode(q, planes[0], planes[1], pos, Hq, Hkv, ctx + 1, 1, False, ws)
            if kind == "bf16_pages":
                q = ops.qknorm_rope_append_paged(qkv, gain, gain, cos, sin, pos, planes[0], planes[1], table, Hq, Hkv)
                return ops.attn_decode_paged(q, planes[0], planes[1], table, pos, Hq, Hkv, ctx + 1, 1, False, ws)
            q = ops.qknorm_rope_append_paged_mx(qkv, gain, gain, cos, sin, pos, planes, table, Hq, Hkv)
            return ops.attn_decode_paged_mx(q, planes, table, pos, Hq, Hkv, ctx + 1, 1, False, ws)

        def fused():
            return ops.cache_step(qkv, gain, gain, cos, sin, pos, planes, Hq, Hkv, table=table, max_len=ctx + 1,
                                  workspace=ws, tickets=tickets)

        for name, fn in (("split", split), ("fused", fused)):
            one_run_kernels(fn, 200)   # warm-up
            out[f"cache_step {kind} B={B} context={ctx} {name}"] = one_run_kernels(fn, CALLS)
    m = model(sda.Qwen3Dims.student_06b())
    row = cell(m, "0.6B", 2048, "bf16", True, 0.2)
    for mode in ("private", "shared"):
        out[f"fork([0] * 8) history=2048 bf16 pages, {mode} attention"] = row[mode]["attention_us_per_step"]
    print("KVSTEP " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_lib")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_step_refactor_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent_lib: the other build's libsd_hip.so")
    runs = {"parent": [], "new": []}
    for rep in range(REPS):
        for build in ("parent", "new"):
            env = dict(os.environ)
            env.pop("SD_HIP_LIB", None)
            if build == "parent":
                env["SD_HIP_LIB"] = os.path.abspath(args.parent_lib)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                                   text=True, timeout=300)
            except subprocess.TimeoutExpired:
                print(f"{build} child {rep} ran into its time limit")
                return 3
            line = [x for x in r.stdout.splitlines() if x.startswith("KVSTEP ")]
            if r.returncode != 0 or not line:   # nothing more is started on the GPU after a child that failed
                print(f"{build} child {rep} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                return 3
            runs[build].append(json.loads(line[0][7:]))
            print(build, rep, "done", flush=True)
    rows, ok = [], True
    for name in runs["parent"][0]:
        p, n = [r[name] for r in runs["parent"]], [r[name] for r in runs["new"]]
        bound = max(p) + (max(p) - min(p))
        row = {"row": name, "parent_us": {"median": statistics.median(p), "min": min(p), "max": max(p)},
               "new_us": {"median": statistics.median(n), "min": min(n), "max": max(n)}, "bound_us": bound,
               "new_median_within_bound": statistics.median(n) <= bound}
        ok = ok and row["new_median_within_bound"]
        rows.append(row)
        print(f"{name:70s} parent {row['parent_us']['median']:9.2f} [{min(p):.2f}, {max(p):.2f}]   new "
              f"{row['new_us']['median']:9.2f} [{min(n):.2f}, {max(n):.2f}]   bound {bound:.2f}  ok={row['new_median_within_bound']}",
              flush=True)
    res = {"method": "parent and new library in fresh child processes (SD_HIP_LIB), alternating, 5 each in one call; GPU time "
                     "of the launches by the library's launch profiler; median [min, max] over the 5 children",
           "criterion": "new median <= parent max + (parent max - parent min)", "all_rows_within_bound": ok, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
