"""GPU measurement (not a pytest): the decode step with the one-launch cache step (decode_attention="fused",
sd_cache_step) against the same build's split step (append launch + two decode-attention launches), which is the code
path the mode leaves untouched.  Writes profiles/decode_fused_bench.json.

  (a) per token: Decoder.step, decode_kernels "skinny", contiguous cache, on the 0.6B and the 1.7B shape (random weights),
      B in {1, 8, 16} x context in {128, 512, 2048}; the same over MXFP8 pages at context 512; the tile step at B = 1.
      Kernel launches of one step counted by the library's launch profiler.
  (b) the cache step alone at the 0.6B head shape (Hq 16, Hkv 8), B = 1, context 512: the three launches against the one,
      GPU time by the library's launch profiler (an event pair around every launch).
Method (that of tests/bench_decode_gemv.py): one warm-up, the two variants alternating in one process, the median of 5
runs of at least 1 s each with [min, max]; one event pair on the launch stream around the steps of a run.
There is no target ratio.  The one condition: at B = 1, context 512, on both shapes, the fused step's MAX is below the
split step's MIN (run ranges that do not overlap; exit status 1 if not)."""
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
from bench_decode_gemv import alternate, launches, one_run_kernels  # noqa: E402

dev = torch.device("cuda:0")
MODES = ("split", "fused")
V = sda.Qwen3Dims.student_06b().vocab_size


def model(dims):
    m = sda.HipQwen3ForCausalLM(dims, device=dev, init_std=0)
    with torch.no_grad():
        m.flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(0))
        for p in m._params.values():
            if p.dim() == 1:
                p.fill_(1.0)
    return m.eval().requires_grad_(False)


def save(res):
    out = os.path.join(ROOT, "profiles", "decode_fused_bench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    return out


def cell(m, name, B, ctx, kernels, kv, min_s):
    """One (shape, B, context, kernels, cache) cell: both modes on decoders of their own, prefilled alike."""
    ids = torch.randint(0, V, (B, ctx), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
    tok = torch.randint(0, V, (B,), device=dev)
    pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    decs = {}
    for mode in MODES:
        pool = None
        if kv == "mxfp8_pages":
            pool = m.kv_page_pool(B * ((ctx + 256 + 255) // 256) + 1, kv_dtype="mxfp8")
        decs[mode] = Decoder(m, B, ctx + 256, decode_kernels=kernels, pool=pool, decode_attention=mode)
        if pool is not None:
            decs[mode].reserve([ctx + 256] * B)
        decs[mode].prefill(ids, pos)
    same = torch.equal(decs["split"].step(tok, pos, ctx + 1), decs["fused"].step(tok, pos, ctx + 1))
    t = alternate({k: (lambda d=d: d.step(tok, pos, ctx + 1)) for k, d in decs.items()}, min_s)
    row = {"model": name, "B": B, "context": ctx, "decode_kernels": kernels, "cache": kv, "logits_equal": bool(same)}
    for k, (med, lo, hi, it) in t.items():
        row[k] = {"us_per_step": med, "us_min": lo, "us_max": hi, "iters_per_run": it,
                  "launches_per_step": launches(decs[k], tok, pos, ctx)}
    row["split_over_fused"] = t["split"][0] / t["fused"][0]
    row["ranges_apart"] = t["fused"][2] < t["split"][1]
    print(f"{name:5s} {kernels:6s} {kv:11s} B={B:2d} ctx={ctx:4d}: split {t['split'][0]:8.1f} us [{t['split'][1]:.1f}, "
          f"{t['split'][2]:.1f}] ({row['split']['launches_per_step']} launches)   fused {t['fused'][0]:8.1f} us "
          f"[{t['fused'][1]:.1f}, {t['fused'][2]:.1f}] ({row['fused']['launches_per_step']} launches)   "
          f"x{row['split_over_fused']:.3f}  equal={same}", flush=True)
    for d in decs.values():
        d.close()
    return row


def cache_step_alone(res, min_s):
    """The three launches against the one, at the 0.6B head shape: GPU time of the launches themselves."""
    Hq, Hkv, B, ctx, cap = 16, 8, 1, 512, 768
    g = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * 128, device=dev, generator=g).bfloat16()
    gain = torch.ones(128, device=dev).bfloat16()
    cos, sin = ops.rope_tables(cap, dev)
    k = (torch.randn(B, cap, Hkv * 128, device=dev, generator=g) * 0.5).bfloat16()
    v = (torch.randn(B, cap, Hkv * 128, device=dev, generator=g) * 0.5).bfloat16()
    pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.load_lib().sd_cache_step_workspace_bytes(B, Hq, Hkv, cap), dtype=torch.uint8, device=dev)
    tickets = torch.zeros(B, Hkv, dtype=torch.int32, device=dev)

    def split():
        q = ops.qknorm_rope_append(qkv, gain, gain, cos, sin, pos, k, v, Hq, Hkv)
        return ops.attn_decode(q, k, v, pos, Hq, Hkv, ctx + 1, 1, False, ws)

    def fused():
        return ops.cache_step(qkv, gain, gain, cos, sin, pos, (k, v), Hq, Hkv, max_len=ctx + 1, workspace=ws, tickets=tickets)

    t = alternate({"split": split, "fused": fused}, min_s, run=one_run_kernels)
    res["cache_step_alone"] = {"Hq": Hq, "Hkv": Hkv, "B": B, "context": ctx,
                               **{k_: {"us": med, "us_min": lo, "us_max": hi, "iters_per_run": it}
                                  for k_, (med, lo, hi, it) in t.items()}}
    print(f"cache step alone (GPU time of the launches): split {t['split'][0]:.2f} us [{t['split'][1]:.2f}, "
          f"{t['split'][2]:.2f}]   fused {t['fused'][0]:.2f} us [{t['fused'][1]:.2f}, {t['fused'][2]:.2f}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0, help="least duration of one timed run")
    ap.add_argument("--models", default="0.6B,1.7B")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": 5, "min_seconds_per_run": args.min_seconds,
           "method": {"all": "one warm-up, the two variants alternating in one process, median of 5 runs [min, max], runs "
                             "sized to min_seconds_per_run of wall time",
                      "step": "one event pair on the launch stream around the steps of a run",
                      "cache_step_alone": "the library's launch profiler: an event pair around every launch, summed",
                      "yardstick": "the split step of the same build: the code path decode_attention leaves untouched"},
           "step": []}
    ok = True
    cache_step_alone(res, args.min_seconds)
    shapes = {"0.6B": sda.Qwen3Dims.student_06b, "1.7B": sda.Qwen3Dims.teacher_17b}
    for name in args.models.split(","):
        m = model(shapes[name]())
        for ctx in (512, 128, 2048):   # the deciding cells first
            for B in (1, 8, 16):
                row = cell(m, name, B, ctx, "skinny", "contiguous", args.min_seconds)
                res["step"].append(row)
                if B == 1 and ctx == 512:
                    ok = ok and row["ranges_apart"]
                save(res)
        for B in (1, 8):
            res["step"].append(cell(m, name, B, 512, "skinny", "mxfp8_pages", args.min_seconds))
        res["step"].append(cell(m, name, 1, 512, "tile", "contiguous", args.min_seconds))
        save(res)
        del m
        torch.cuda.empty_cache()
    res["fused_max_below_split_min_at_B1_ctx512"] = ok
    print("wrote", save(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
