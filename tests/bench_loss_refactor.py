"""GPU measurement (not a pytest): the loss and top-K kernels of this build against those of another build of the library
(the commit before the kernels were moved onto the shared device functions of csrc/sd_rows.cuh).  Writes
profiles/loss_refactor_bench.json.

    python tests/bench_loss_refactor.py --parent_lib <the other build's libsd_hip.so>

The two libraries run in FRESH child processes (SD_HIP_LIB), parent / new / parent / new ... five times each; a child
measures every row once and prints one JSON line.  Rows, at R = 1536 rows of V = 159 488 bf16 logits, all GPU time by the
library's launch profiler (an event pair around every launch), forward + backward entry per call:
  - sd_kdloss_fwd_rows + sd_kdloss_bwd_rows: top-128 at T = 2 (the bench.py configuration), top-1024 at T = 2 (the
    1024-thread kd_fwd_kernel), dense at T = 2 and at T = 3;
  - sd_celoss_fwd_rows + sd_celoss_bwd_rows;
  - sd_gjsd_fwd_rows + sd_gjsd_bwd_rows, reverse KL and JSD beta = 0.5, at T = 2;
  - sd_logsoftmax_topk, K = 128.
--rows sparse (default --out profiles/loss_sparse_refactor_bench.json) measures instead what DESIGN.md section 12e moved,
same method, T = 2, beta = 0.5:
  - sd_gjsd_topk_fwd_rows + _bwd_rows at K = 128 and K = 1024; sd_gjsd_tail_fwd_rows + _bwd_rows in its three modes at
    K = 128 and jsd_tail at K = 1024 (the tails are sd_topk_tail's);
  - sd_gjsd_*_rows reverse KL and JSD (sweep 1 is on the shared normaliser step) and sd_kdloss_*_rows at top-128 (the host
    path alone moved);
  - sd_loss_rows at B = 4, T = 512 and sd_packed_rows at M = 2048 with four documents (the shared compaction).
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
CALLS = 20    # calls per row and child, after WARM
WARM = 3
R, V = 1536, 159488


def child(which):
    sys.path.insert(0, ROOT)
    import torch
    from speech_distill_amd import ops
    dev = torch.device("cuda:0")
    lib = ops.load_lib()
    g = torch.Generator(device=dev).manual_seed(1)
    s = (torch.randn(R, V, device=dev, generator=g) * 3).bfloat16()
    t = (torch.randn(R, V, device=dev, generator=g) * 3).bfloat16()
    grad = torch.empty_like(s)
    labels = torch.randint(0, V, (R,), device=dev, generator=g)
    go = torch.ones(1, dtype=torch.float32, device=dev)
    out = torch.empty(8, dtype=torch.float32, device=dev)
    stats = torch.empty(max(lib.sd_kdloss_stats_bytes(R, 1), lib.sd_gjsd_stats_bytes(R), lib.sd_celoss_stats_bytes(R),
                            lib.sd_gjsd_topk_stats_bytes(R), lib.sd_gjsd_tail_stats_bytes(R)), dtype=torch.uint8, device=dev)
    tv, ti = ops.logsoftmax_topk(t, 1024)
    top = {128: (tv[:, :128].contiguous(), ti[:, :128].contiguous()), 1024: (tv, ti)}
    tv128, ti128 = torch.empty_like(top[128][0]), torch.empty_like(top[128][1])
    st = torch.cuda.current_stream().cuda_stream
    p = lambda x: None if x is None else x.data_ptr()

    def kd(te, K, T):
        v, i = top[K] if K else (None, None)

        def run():
            assert lib.sd_kdloss_fwd_rows(s.data_ptr(), p(te), p(v), p(i), labels.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                          R, V, K, T, 0.5, 0, st) == 0
            assert lib.sd_kdloss_bwd_rows(s.data_ptr(), p(te), p(v), p(i), labels.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                          go.data_ptr(), grad.data_ptr(), R, V, K, T, 0.5, 0, st) == 0
        return run

    def ce():
        assert lib.sd_celoss_fwd_rows(s.data_ptr(), labels.data_ptr(), None, stats.data_ptr(), out.data_ptr(), R, V, 0, st) == 0
        assert lib.sd_celoss_bwd_rows(s.data_ptr(), labels.data_ptr(), stats.data_ptr(), out.data_ptr(), go.data_ptr(),
                                      grad.data_ptr(), R, V, 0, st) == 0

    def gjsd(mode):
        def run():
            assert lib.sd_gjsd_fwd_rows(s.data_ptr(), t.data_ptr(), labels.data_ptr(), stats.data_ptr(), out.data_ptr(), R, V,
                                        2.0, 0.5, 0.5, mode, 0, st) == 0
            assert lib.sd_gjsd_bwd_rows(s.data_ptr(), t.data_ptr(), labels.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                        go.data_ptr(), grad.data_ptr(), R, V, 2.0, 0.5, 0.5, mode, 0, st) == 0
        return run

    def topk():
        assert lib.sd_logsoftmax_topk(t.data_ptr(), tv128.data_ptr(), ti128.data_ptr(), None, R, V, V, 128, 0, st) == 0

    def gjsd_topk(K):
        v, i = top[K]

        def run():
            assert lib.sd_gjsd_topk_fwd_rows(s.data_ptr(), v.data_ptr(), i.data_ptr(), labels.data_ptr(), stats.data_ptr(),
                                             out.data_ptr(), R, V, K, 2.0, 0.5, 0.5, 0, st) == 0
            assert lib.sd_gjsd_topk_bwd_rows(s.data_ptr(), v.data_ptr(), i.data_ptr(), labels.data_ptr(), stats.data_ptr(),
                                             out.data_ptr(), go.data_ptr(), grad.data_ptr(), R, V, K, 2.0, 0.5, 0.5, 0, st) == 0
        return run

    def gjsd_tail(K, mode):
        v, i = top[K]
        tau = ops.topk_tail(t, i, 2.0)

        def run():
            assert lib.sd_gjsd_tail_fwd_rows(s.data_ptr(), v.data_ptr(), i.data_ptr(), tau.data_ptr(), labels.data_ptr(),
                                             stats.data_ptr(), out.data_ptr(), R, V, K, 2.0, 0.5, 0.5, mode, 0, st) == 0
            assert lib.sd_gjsd_tail_bwd_rows(s.data_ptr(), v.data_ptr(), i.data_ptr(), tau.data_ptr(), labels.data_ptr(),
                                             stats.data_ptr(), out.data_ptr(), go.data_ptr(), grad.data_ptr(), R, V, K, 2.0, 0.5,
                                             0.5, mode, 0, st) == 0
        return run

    def selection():
        """-> (sd_loss_rows at B = 4, T = 512, sd_packed_rows at M = 2048 with four documents): a quarter of the labels masked."""
        B, T, M = 4, 512, 2048
        lab = torch.randint(0, V, (B, T), device=dev, generator=g)
        lab[torch.rand(B, T, device=dev, generator=g) < 0.25] = -100
        sel, sel_labels = torch.empty(M, dtype=torch.int64, device=dev), torch.empty(M, dtype=torch.int64, device=dev)
        meta = torch.empty(4, dtype=torch.int32, device=dev)
        cu = torch.tensor([0, 300, 1000, 1900, M], dtype=torch.int32, device=dev)
        pos = torch.cat([torch.arange(int(b - a), device=dev) for a, b in zip(cu[:-1], cu[1:])])

        def padded():
            assert lib.sd_loss_rows(lab.data_ptr(), None, None, None, sel.data_ptr(), sel_labels.data_ptr(), meta.data_ptr(), B, T,
                                    st) == 0

        def packed():
            assert lib.sd_packed_rows(lab.data_ptr(), None, cu.data_ptr(), 4, pos.data_ptr(), sel.data_ptr(), sel_labels.data_ptr(),
                                      meta.data_ptr(), M, st) == 0
        return padded, packed

    if which == "sparse":
        padded, packed = selection()
        rows = {"gjsd_topk fwd+bwd, K=128": gjsd_topk(128), "gjsd_topk fwd+bwd, K=1024": gjsd_topk(1024),
                "gjsd_tail fwd+bwd, forward_kl_tail, K=128": gjsd_tail(128, 0),
                "gjsd_tail fwd+bwd, reverse_kl_tail, K=128": gjsd_tail(128, 1),
                "gjsd_tail fwd+bwd, jsd_tail, K=128": gjsd_tail(128, 2), "gjsd_tail fwd+bwd, jsd_tail, K=1024": gjsd_tail(1024, 2),
                "gjsd fwd+bwd, reverse KL, T=2": gjsd(1), "gjsd fwd+bwd, JSD beta=0.5, T=2": gjsd(2),
                "kd fwd+bwd, top-128, T=2": kd(None, 128, 2.0), "loss_rows, B=4, T=512": padded,
                "packed_rows, M=2048, 4 documents": packed}
    else:
        rows = {"kd fwd+bwd, top-128, T=2": kd(None, 128, 2.0), "kd fwd+bwd, top-1024, T=2": kd(None, 1024, 2.0),
                "kd fwd+bwd, dense, T=2": kd(t, 0, 2.0), "kd fwd+bwd, dense, T=3": kd(t, 0, 3.0), "ce fwd+bwd": ce,
                "gjsd fwd+bwd, reverse KL, T=2": gjsd(1), "gjsd fwd+bwd, JSD beta=0.5, T=2": gjsd(2), "top-K, K=128": topk}
    res = {}
    for name, fn in rows.items():
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ops.prof_begin()
        for _ in range(CALLS):
            fn()
        res[name] = sum(ms for ms, _, _ in ops.prof_end().values()) / CALLS * 1e3
    print("LOSSBENCH " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_lib")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rows", choices=("dense", "sparse"), default="dense", help="the row set (see the module docstring)")
    ap.add_argument("--out", help="default: profiles/loss_refactor_bench.json, for --rows sparse loss_sparse_refactor_bench.json")
    args = ap.parse_args()
    if args.child:
        return child(args.rows)
    if not args.out:
        args.out = os.path.join(ROOT, "profiles", "loss_sparse_refactor_bench.json" if args.rows == "sparse" else "loss_refactor_bench.json")
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
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rows", args.rows], env=env, capture_output=True,
                                   text=True, timeout=240)
            except subprocess.TimeoutExpired:
                print(f"{build} child {rep} ran into its time limit")
                return 3
            line = [x for x in r.stdout.splitlines() if x.startswith("LOSSBENCH ")]
            if r.returncode != 0 or not line:   # nothing more is started on the GPU after a child that failed
                print(f"{build} child {rep} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                return 3
            runs[build].append(json.loads(line[0][10:]))
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
        print(f"{name:36s} parent {row['parent_us']['median']:9.2f} [{min(p):.2f}, {max(p):.2f}]   new "
              f"{row['new_us']['median']:9.2f} [{min(n):.2f}, {max(n):.2f}]   bound {bound:.2f}  ok={row['new_median_within_bound']}",
              flush=True)
    res = {"method": f"parent and new library in fresh child processes (SD_HIP_LIB), alternating, {REPS} each in one call; R = {R}, "
                     f"V = {V}, bf16; GPU time of the launches of one forward + backward call by the library's launch profiler, "
                     f"mean of {CALLS} calls after {WARM}; median [min, max] over the {REPS} children",
           "criterion": "new median <= parent max + (parent max - parent min)", "all_rows_within_bound": ok, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
