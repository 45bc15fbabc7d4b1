"""GPU measurement (not a pytest): 8-bit (MXFP8) pages against bf16 pages of the paged KV cache on the 0.6B student shape
(random weights, random cache contents: finite e4m3 codes under the scale 2^-7 / N(0, 1) bf16).  Writes
profiles/paged_mx_bench.json.

  (a) per token: ``Decoder.step`` over a bf16 pool and over an mxfp8 pool (both handed out in a shuffled order); B in {1,
      8, 16}, context in {512, 4096, 8192}, decode_kernels "tile" and "skinny";
  (b) the attention of such a step alone -- sd_attn_decode_paged against sd_attn_decode_paged_mx, both launches of each
      (Hq 16, Hkv 8), GPU time from the library's launch profiler -- with the K / V bytes per second each reads;
  (c) sd_attn_extend_paged against sd_attn_extend_paged_mx at block in {64, 512}, past 4096, B = 8.  No condition: the
      8-bit kernel gives up the global -> LDS DMA of the tile, and the pass runs once per turn.
Method (tests/bench_paged.py): events on the launch stream, one warm-up, the variants alternating in one process, the
median of 5 runs, [min, max] next to every figure.
Conditions (exit status 1 when either fails), the yardstick being the bf16 paged step measured beside it in the same
process, never a stored number:
  - at B = 8, context 4096 the mxfp8 step is faster than the bf16 step, on both kernel sets;
  - at B = 1, context 512 it takes at most 1.02 x the bf16 step -- or, where the bf16 step's own relative [min, max] spread
    is larger than 2 %, at most 1 + that spread (the rule of tests/bench_paged.py).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from speech_distill_amd import ops  # noqa: E402
from speech_distill_amd.generation import Decoder  # noqa: E402
from bench_decode_gemv import REPS, alternate, one_run_kernels, student  # noqa: E402
from bench_paged import fig, shuffled  # noqa: E402

dev = torch.device("cuda:0")
PAGE, HQ, HKV = 256, 16, 8


def fill_bf16(t):
    t.view(torch.bfloat16).normal_(0.0, 1.0)


def fill_mx(data, scale):
    """finite e4m3 codes (exponent field below 15) of either sign under the scale byte 120 = 2^-7"""
    data.copy_(torch.randint(0, 0x78, data.shape, device=dev, dtype=torch.uint8) |
               (torch.randint(0, 2, data.shape, device=dev, dtype=torch.uint8) << 7))
    scale.fill_(120)


def fill_pool(pool):
    if pool.kv_dtype == "bf16":
        fill_bf16(pool.buffer)
        return
    for l in range(pool.model.dims.num_hidden_layers):
        kd, ks, vd, vs = pool.planes(l)
        fill_mx(kd, ks), fill_mx(vd, vs)


def bench_step(m, res, min_s, cells):
    V = m.dims.vocab_size
    ok = True
    for B, ctx in cells:
        tok = torch.randint(0, V, (B,), device=dev)
        pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        cap = ctx + PAGE
        n_pages = B * (cap // PAGE)
        for kernels in ("tile", "skinny"):
            decs = {}
            for dt in ("bf16", "mxfp8"):
                pool = m.kv_page_pool(n_pages, shuffled(n_pages, ctx + B), kv_dtype=dt)
                fill_pool(pool)
                decs[dt] = Decoder(m, B, cap, kernels, pool=pool)
                decs[dt].reserve([cap] * B)
            finite = all(bool(torch.isfinite(d.step(tok, pos, ctx + 1).float()).all()) for d in decs.values())
            t = alternate({k: (lambda d=d: d.step(tok, pos, ctx + 1)) for k, d in decs.items()}, min_s)
            base = t["bf16"]
            spread = (base[2] - base[1]) / base[0]
            row = {"B": B, "context": ctx, "decode_kernels": kernels, "logits_finite": finite, "bf16_rel_spread": spread,
                   "bf16": fig(base), "mxfp8": fig(t["mxfp8"]), "mxfp8_over_bf16": t["mxfp8"][0] / base[0],
                   "bytes_per_page": {k: d.pool.bytes_per_page for k, d in decs.items()}}
            if (B, ctx) == (8, 4096):
                row["condition"], row["ok"] = "mxfp8 faster than bf16", row["mxfp8_over_bf16"] < 1.0
            elif (B, ctx) == (1, 512):
                row["limit"] = 1.0 + max(0.02, spread)
                row["condition"], row["ok"] = "mxfp8 <= limit x bf16", row["mxfp8_over_bf16"] <= row["limit"]
            ok = ok and row.get("ok", True) and finite
            res["step"].append(row)
            print(f"step B={B:2d} ctx={ctx:4d} {kernels:6s}: bf16 {base[0]:8.1f} us [{base[1]:.1f}, {base[2]:.1f}]   mxfp8 "
                  f"{t['mxfp8'][0]:8.1f} us [{t['mxfp8'][1]:.1f}, {t['mxfp8'][2]:.1f}]   x{row['mxfp8_over_bf16']:.4f}  "
                  f"{row.get('condition', '')} {row.get('ok', '')}", flush=True)
            for d in decs.values():
                d.close()
            del decs
            save(res)
    res["conditions_hold"] = ok
    return ok


def pools(B, max_pages, seed):
    """bf16 planes, 8-bit planes and one shuffled table for B rows of max_pages pages"""
    n = B * max_pages
    table = torch.tensor(shuffled(n, seed), dtype=torch.int32, device=dev).view(B, max_pages).contiguous()
    k, v = (torch.empty(n, PAGE, HKV * 128, dtype=torch.bfloat16, device=dev).normal_() for _ in range(2))
    kd, vd = (torch.empty(n, PAGE, HKV * 128, dtype=torch.uint8, device=dev) for _ in range(2))
    ks, vs = (torch.empty(n, PAGE, HKV * 4, dtype=torch.uint8, device=dev) for _ in range(2))
    fill_mx(kd, ks), fill_mx(vd, vs)
    return (k, v), (kd, ks, vd, vs), table


def bench_decode_attn(res, min_s, cells):
    for B, ctx in cells:
        n = ctx + 1
        max_pages = (n + PAGE - 1) // PAGE
        (k, v), mx, table = pools(B, max_pages, ctx + B)
        q = torch.randn(B, HQ * 128, device=dev).bfloat16()
        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.load_lib().sd_attn_decode_workspace_bytes(B, HQ, max_pages * PAGE), dtype=torch.uint8, device=dev)
        t = alternate({"bf16": lambda: ops.attn_decode_paged(q, k, v, table, lens, HQ, HKV, max_len=n, workspace=ws),
                       "mxfp8": lambda: ops.attn_decode_paged_mx(q, mx, table, lens, HQ, HKV, max_len=n, workspace=ws)},
                      min_s, run=one_run_kernels)
        kv_bytes = {"bf16": 2 * B * n * HKV * 256, "mxfp8": 2 * B * n * HKV * 132}
        row = {"B": B, "context": ctx, "keys": n, "mxfp8_over_bf16": t["mxfp8"][0] / t["bf16"][0]}
        for key in ("bf16", "mxfp8"):
            row[key] = fig(t[key])
            row[key]["kv_bytes"] = kv_bytes[key]
            row[key]["kv_TB_per_s"] = kv_bytes[key] / t[key][0] / 1e6
        res["attn_decode"].append(row)
        print(f"attn_decode B={B:2d} ctx={ctx:4d}: bf16 {t['bf16'][0]:7.1f} us ({row['bf16']['kv_TB_per_s']:.2f} TB/s)   mxfp8 "
              f"{t['mxfp8'][0]:7.1f} us ({row['mxfp8']['kv_TB_per_s']:.2f} TB/s)   x{row['mxfp8_over_bf16']:.4f}", flush=True)
        save(res)


def bench_extend(res, min_s):
    B, past = 8, 4096
    for block in (64, 512):
        max_pages = (past + block + PAGE - 1) // PAGE
        (k, v), mx, table = pools(B, max_pages, block)
        q = torch.randn(B * block, HQ * 128, device=dev).bfloat16()
        p_d = torch.full((B,), past, dtype=torch.int32, device=dev)
        n_d = torch.full((B,), block, dtype=torch.int32, device=dev)
        t = alternate({"bf16": lambda: ops.attn_extend_paged(q, k, v, table, p_d, n_d, block, HQ, HKV, want_lse=False),
                       "mxfp8": lambda: ops.attn_extend_paged_mx(q, mx, table, p_d, n_d, block, HQ, HKV, want_lse=False)},
                      min_s, run=one_run_kernels)
        row = {"B": B, "block": block, "past": past, "bf16": fig(t["bf16"]), "mxfp8": fig(t["mxfp8"]),
               "mxfp8_over_bf16": t["mxfp8"][0] / t["bf16"][0]}
        res["attn_extend"].append(row)
        print(f"attn_extend B={B} block={block:3d} past={past}: bf16 {t['bf16'][0]:8.1f} us   mxfp8 {t['mxfp8'][0]:8.1f} us   "
              f"x{row['mxfp8_over_bf16']:.4f}", flush=True)
        save(res)


OUT = [os.path.join(ROOT, "profiles", "paged_mx_bench.json")]


def save(res):
    with open(OUT[0], "w") as f:
        json.dump(res, f, indent=1)
    return OUT[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0, help="least duration of one timed run")
    ap.add_argument("--out", default=OUT[0])
    ap.add_argument("--conditions_only", action="store_true", help="(a) at the two cells that carry a condition, nothing else")
    args = ap.parse_args()
    OUT[0] = args.out
    res = {"device": torch.cuda.get_device_name(0), "shape": "student 0.6B (159488, 1024, 3072, 28, 16, 8)", "reps": REPS,
           "min_seconds_per_run": args.min_seconds,
           "method": "step: one event pair on the launch stream around the calls of a run; attention: the library's launch "
                     "profiler (an event pair around every launch); one warm-up, variants alternating in one process, median "
                     "of 5 runs [min, max], runs sized to min_seconds_per_run of wall time",
           "step": [], "attn_decode": [], "attn_extend": []}
    cells = [(B, ctx) for ctx in (512, 4096, 8192) for B in (1, 8, 16)]
    if args.conditions_only:
        cells = [(1, 512), (8, 4096)]
    ok = bench_step(student(), res, args.min_seconds, cells)
    if not args.conditions_only:
        bench_decode_attn(res, args.min_seconds, cells)
        bench_extend(res, args.min_seconds)
    print("wrote", save(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
