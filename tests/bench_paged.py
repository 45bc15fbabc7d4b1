"""GPU measurement (not a pytest): the paged KV cache against the contiguous one on the 0.6B student shape (random
weights).  Writes profiles/paged_bench.json.

  (a) per token: ``Decoder.step`` over a contiguous cache, over a page pool with an identity table (row b's pages lie end
      to end, in order) and over a pool whose pages were handed out in a shuffled order; B in {1, 8}, context in {512,
      4096}, decode_kernels "tile" and "skinny";
  (b) sd_attn_extend against sd_attn_extend_paged (shuffled table; Hq 16, Hkv 8, B = 8) at block in {64, 512} x past in
      {0, 4096};
  (c) bytes: what a contiguous session reserves at the model's default capacity against the peak ``pages_in_use *
      bytes_per_page`` of a paged session, in tests/bench_session.py's scenario: history 4096, a turn of 64 given + 128 new
      tokens, B = 8.
Method (tests/bench_decode_gemv.py, tests/bench_session.py): events on the launch stream, one warm-up, the variants
alternating in one process, the median of 5 runs of at least 1 s each, [min, max] next to every figure.
The one condition (exit status 1 otherwise): in every cell of (a) the shuffled-table step takes at most 1.02 x the
contiguous step measured beside it -- or, where the contiguous step's own relative [min, max] spread is larger than 2 %,
at most 1 + that spread.  The yardstick is the contiguous path of the same process, never a stored number; 2 % because the
committed decode measurements repeat within 0.1 % and one uniform 4-byte load per 256 keys has no business costing more.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speech_distill_amd as sda  # noqa: E402
from speech_distill_amd import ops  # noqa: E402
from speech_distill_amd.generation import REFERENCE_SAMPLING, Decoder, cache_capacity  # noqa: E402
from bench_decode_gemv import REPS, alternate, student  # noqa: E402

dev = torch.device("cuda:0")
PAGE = 256


def shuffled(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()


def fig(t):
    med, lo, hi, it = t
    return {"us": med, "us_min": lo, "us_max": hi, "iters_per_run": it}


def bench_step(m, res, min_s):
    V = m.dims.vocab_size
    ok = True
    for ctx in (512, 4096):
        for B in (1, 8):
            ids = torch.randint(0, V, (B, ctx), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
            tok = torch.randint(0, V, (B,), device=dev)
            pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            cap = ctx + PAGE
            n_pages = B * (cap // PAGE)
            for kernels in ("tile", "skinny"):
                pools = {"paged_identity": m.kv_page_pool(n_pages), "paged_shuffled": m.kv_page_pool(n_pages, shuffled(n_pages, ctx + B))}
                decs = {"contiguous": Decoder(m, B, cap, kernels)}
                for k, pool in pools.items():
                    decs[k] = Decoder(m, B, cap, kernels, pool=pool)
                    decs[k].reserve([cap] * B)
                ident = decs["paged_identity"].pages.rows
                assert ident == [list(range(b * (cap // PAGE), (b + 1) * (cap // PAGE))) for b in range(B)]
                first = {}
                for k, d in decs.items():
                    d.prefill(ids, pos)
                    first[k] = d.step(tok, pos, ctx + 1).clone()
                same = all(torch.equal(first["contiguous"].view(torch.int16), first[k].view(torch.int16)) for k in pools)
                t = alternate({k: (lambda d=d: d.step(tok, pos, ctx + 1)) for k, d in decs.items()}, min_s)
                base = t["contiguous"]
                spread = (base[2] - base[1]) / base[0]
                limit = 1.0 + max(0.02, spread)
                row = {"B": B, "context": ctx, "decode_kernels": kernels, "logits_bit_identical": same,
                       "contiguous_rel_spread": spread, "limit": limit}
                for k in decs:
                    row[k] = fig(t[k])
                    row[k]["over_contiguous"] = t[k][0] / base[0]
                row["ok"] = row["paged_shuffled"]["over_contiguous"] <= limit
                ok = ok and row["ok"] and same
                res["step"].append(row)
                print(f"step B={B} ctx={ctx:4d} {kernels:6s}: contiguous {base[0]:8.1f} us [{base[1]:.1f}, {base[2]:.1f}]   "
                      f"identity x{row['paged_identity']['over_contiguous']:.4f}   shuffled "
                      f"x{row['paged_shuffled']['over_contiguous']:.4f} (limit {limit:.4f})  bits same: {same}", flush=True)
                for d in decs.values():
                    if d.pool is not None:
                        d.close()
                del decs, pools
                save(res)
    res["shuffled_step_within_limit_everywhere"] = ok
    return ok


def bench_extend(res, min_s):
    Hq, Hkv, B = 16, 8, 8
    for block in (64, 512):
        q = torch.randn(B * block, Hq * 128, device=dev).bfloat16()
        for past in (0, 4096):
            max_pages = (past + block + PAGE - 1) // PAGE
            cap = max_pages * PAGE
            kp = torch.randn(B, cap, Hkv * 128, device=dev).bfloat16()
            vp = torch.randn(B, cap, Hkv * 128, device=dev).bfloat16()
            perm = torch.tensor(shuffled(B * max_pages, block + past), dtype=torch.int64, device=dev)
            table = perm.view(B, max_pages).to(torch.int32).contiguous()
            k_pool = torch.empty(B * max_pages, PAGE, Hkv * 128, dtype=torch.bfloat16, device=dev)
            v_pool = torch.empty_like(k_pool)
            k_pool[perm] = kp.view(B * max_pages, PAGE, -1)
            v_pool[perm] = vp.view(B * max_pages, PAGE, -1)
            p_d = torch.full((B,), past, dtype=torch.int32, device=dev)
            n_d = torch.full((B,), block, dtype=torch.int32, device=dev)
            a = ops.attn_extend(q, kp, vp, p_d, n_d, block, Hq, Hkv, want_lse=False)
            b = ops.attn_extend_paged(q, k_pool, v_pool, table, p_d, n_d, block, Hq, Hkv, want_lse=False)
            same = torch.equal(a.view(torch.int16), b.view(torch.int16))
            t = alternate({"contiguous": lambda: ops.attn_extend(q, kp, vp, p_d, n_d, block, Hq, Hkv, want_lse=False),
                           "paged_shuffled": lambda: ops.attn_extend_paged(q, k_pool, v_pool, table, p_d, n_d, block, Hq, Hkv,
                                                                           want_lse=False)}, min_s)
            row = {"B": B, "block": block, "past": past, "bit_identical": same, "contiguous": fig(t["contiguous"]),
                   "paged_shuffled": fig(t["paged_shuffled"]),
                   "paged_over_contiguous": t["paged_shuffled"][0] / t["contiguous"][0]}
            res["attn_extend"].append(row)
            print(f"attn_extend B={B} block={block:3d} past={past:4d}: contiguous {t['contiguous'][0]:8.1f} us "
                  f"[{t['contiguous'][1]:.1f}, {t['contiguous'][2]:.1f}]   paged {t['paged_shuffled'][0]:8.1f} us "
                  f"[{t['paged_shuffled'][1]:.1f}, {t['paged_shuffled'][2]:.1f}]   x{row['paged_over_contiguous']:.4f}  "
                  f"bits same: {same}", flush=True)
            save(res)


def bench_bytes(m, res):
    B, hist, given, new = 8, 4096, 64, 128
    cap = cache_capacity(m)
    contiguous = sda.load_lib().sd_kvcache_bytes(ctypes.byref(m._cdims), B, cap)   # what start_session(B) would reserve
    n_pages = B * ((hist + given + new + PAGE - 1) // PAGE) + 8
    pool = m.kv_page_pool(n_pages, shuffled(n_pages, 1))
    sess = m.start_session(B, pool=pool)
    ids = torch.randint(0, m.dims.vocab_size, (B, hist + given), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    sess.extend(ids[:, :hist].contiguous())
    peak = pool.pages_in_use
    sess.generate(ids[:, hist:].contiguous(), max_new_tokens=new, seed=1, **REFERENCE_SAMPLING)
    peak = max(peak, pool.pages_in_use)     # the table only changes at a turn's admission
    sess.trim()
    res["bytes"] = {"B": B, "history": hist, "given": given, "new_tokens": new, "capacity": cap,
                    "bytes_per_position": pool.bytes_per_page // PAGE, "bytes_per_page": pool.bytes_per_page,
                    "contiguous_session_bytes": contiguous, "paged_peak_pages": peak,
                    "paged_peak_bytes": peak * pool.bytes_per_page, "paged_pages_after_trim": pool.pages_in_use,
                    "contiguous_over_paged": contiguous / (peak * pool.bytes_per_page)}
    print(f"bytes B={B}: contiguous session at capacity {cap}: {contiguous / 2**30:.2f} GiB   paged peak {peak} pages = "
          f"{peak * pool.bytes_per_page / 2**30:.2f} GiB   x{res['bytes']['contiguous_over_paged']:.1f}", flush=True)
    sess.close()


def save(res):
    out = os.path.join(ROOT, "profiles", "paged_bench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0, help="least duration of one timed run")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "shape": "student 0.6B (159488, 1024, 3072, 28, 16, 8)", "reps": REPS,
           "min_seconds_per_run": args.min_seconds,
           "method": "one event pair on the launch stream around the calls of a run; one warm-up, variants alternating in one "
                     "process, median of 5 runs [min, max], runs sized to min_seconds_per_run of wall time",
           "step": [], "attn_extend": [], "bytes": "not measured"}
    m = student()
    ok = bench_step(m, res, args.min_seconds)
    bench_extend(res, args.min_seconds)
    bench_bytes(m, res)
    print("wrote", save(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
