"""GPU measurement (not a pytest): the decode step of a forked session with ``shared_kv_reads`` (the shared-page decode
attention, sd_attn_decode_shared_paged{,_mx}) against the same build's step without it, which reads every shared page once
per row.  Writes profiles/fork_shared_bench.json.

  One row is prefilled to a history of 512, 2048 or 6144 tokens over a page pool, then ``fork([0] * 8)``: eight
  continuations that share the history's full pages (decode_kernels "skinny"; the 0.6B and the 1.7B shape, random weights;
  bf16 and MXFP8 pages).  Timed: ``Decoder.step`` of the two forks' decoders.  One more cell has eight UNRELATED rows
  (nothing shared), where the grouped kernel can only lose.
Method (that of tests/bench_decode_gemv.py): one warm-up, the two variants alternating in one process, the median of 5
runs with [min, max]; one event pair on the launch stream around the steps of a run.  The attention launches alone (phase 1
and the merge, all layers of a step) come from the library's launch profiler: an event pair around every launch, summed by
kernel symbol.  There is no target ratio and no exit status: every cell records whether the shared step's MAX lies below
the private step's MIN."""
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
from bench_decode_gemv import alternate  # noqa: E402
from bench_decode_fused import model  # noqa: E402

dev = torch.device("cuda:0")
MODES = ("private", "shared")
V = sda.Qwen3Dims.student_06b().vocab_size
ROWS = 8


def save(res):
    out = os.path.join(ROOT, "profiles", "fork_shared_bench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    return out


def attention_us(dec, tok, pos, max_len, steps=20):
    """GPU time of the decode-attention launches of one step (every layer's phase 1 and merge), by kernel symbol."""
    ops.prof_begin()
    for _ in range(steps):
        dec.step(tok, pos, max_len)
    torch.cuda.synchronize()
    ops.prof_end()
    ms = sum(t for sym, (t, _, _, _) in ops.prof_symbols().items()
             if sym.startswith(("attn_decode_part_kernel", "attn_shared_part_kernel", "attn_decode_merge_kernel")))
    return ms / steps * 1e3


def cell(m, name, ctx, pages, forked, min_s):
    """One (shape, history, page dtype) cell: the step of eight rows with and without the keyword, on sessions of their
    own over pools of their own, filled alike.  forked: the rows are fork([0] * 8) of one row; else eight prefilled rows."""
    g = torch.Generator(device=dev).manual_seed(ctx)
    src_rows = 1 if forked else ROWS
    ids = torch.randint(0, V, (src_rows, ctx), device=dev, generator=g)
    tok = torch.randint(0, V, (ROWS,), device=dev, generator=g)
    pos = torch.full((ROWS,), ctx, dtype=torch.int32, device=dev)
    per_row = (ctx + 256 + 255) // 256
    keep, decs = [], {}
    for mode in MODES:
        pool = m.kv_page_pool((src_rows + ROWS) * per_row + 2, kv_dtype=pages)
        pool.buffer.zero_()
        s = m.start_session(src_rows, ctx + 256, pool=pool, decode_kernels="skinny", shared_kv_reads=not forked and mode == "shared")
        s.extend(ids)
        if forked:
            f = s.fork([0] * ROWS, shared_kv_reads=mode == "shared")
            f.decoder.reserve([ctx + 256] * ROWS)
        else:
            f = s
            f.decoder.reserve([ctx + 256] * ROWS)
        keep.append((pool, s, f))
        decs[mode] = f.decoder
    shared_pages = sum(1 for i in range(per_row) if len({tuple(r[i:i + 1]) for r in decs["shared"].pages.rows}) == 1)
    a, b = (decs[k].step(tok, pos, ctx + 1).clone() for k in MODES)
    same = torch.equal(a.view(torch.int16), b.view(torch.int16))
    t = alternate({k: (lambda d=d: d.step(tok, pos, ctx + 1)) for k, d in decs.items()}, min_s)
    row = {"model": name, "rows": ROWS, "history": ctx, "pages": pages, "layout": "fork([0] * 8)" if forked else "unrelated rows",
           "pages_of_a_row_shared_by_all": shared_pages, "logits_equal": bool(same)}
    for k, (med, lo, hi, it) in t.items():
        row[k] = {"us_per_step": med, "us_min": lo, "us_max": hi, "iters_per_run": it,
                  "attention_us_per_step": attention_us(decs[k], tok, pos, ctx + 1)}
    row["private_over_shared"] = t["private"][0] / t["shared"][0]
    row["attention_private_over_shared"] = row["private"]["attention_us_per_step"] / row["shared"]["attention_us_per_step"]
    row["shared_max_below_private_min"] = bool(t["shared"][2] < t["private"][1])
    print(f"{name:5s} {pages:5s} {row['layout']:15s} history={ctx:5d}: private {t['private'][0]:8.1f} us [{t['private'][1]:.1f}, "
          f"{t['private'][2]:.1f}] (attention {row['private']['attention_us_per_step']:.1f})   shared {t['shared'][0]:8.1f} us "
          f"[{t['shared'][1]:.1f}, {t['shared'][2]:.1f}] (attention {row['shared']['attention_us_per_step']:.1f})   "
          f"x{row['private_over_shared']:.3f}  attention x{row['attention_private_over_shared']:.2f}  equal={same}", flush=True)
    for pool, s, f in keep:
        if f is not s:
            f.close()
        s.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0, help="least duration of one timed run")
    ap.add_argument("--models", default="0.6B,1.7B")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": 5, "min_seconds_per_run": args.min_seconds,
           "method": {"step": "one warm-up, the two variants alternating in one process, median of 5 runs [min, max]; one event "
                              "pair on the launch stream around the steps of a run",
                      "attention": "the library's launch profiler: an event pair around every launch, the decode-attention "
                                   "symbols (phase 1 and merge) of 20 steps summed, per step",
                      "yardstick": "the step without shared_kv_reads of the same build: the code path the keyword leaves "
                                   "untouched"},
           "cells": []}
    shapes = {"0.6B": sda.Qwen3Dims.student_06b, "1.7B": sda.Qwen3Dims.teacher_17b}
    for name in args.models.split(","):
        m = model(shapes[name]())
        for pages in ("bf16", "mxfp8"):
            for ctx in (512, 2048, 6144):
                res["cells"].append(cell(m, name, ctx, pages, True, args.min_seconds))
                save(res)
        res["cells"].append(cell(m, name, 2048, "bf16", False, args.min_seconds))
        save(res)
        del m
        torch.cuda.empty_cache()
    print("wrote", save(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
