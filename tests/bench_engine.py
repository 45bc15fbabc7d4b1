"""GPU measurement (not a pytest): continuous batching (speech_distill_amd/engine.py) against the fixed-batch ``generate``
on the 0.6B student shape (random weights).  Writes profiles/engine_bench.json.

Workload: 64 requests of 128 prompt tokens, EOS disabled, budgets cycling through (32, 64, 128, 512) -- so every length is
known in advance -- the reference's sampling recipe, B = 8, decode_kernels "skinny".
  static  ``model.generate`` on batches of 8 in submission order; every batch holds a 512, so it runs 512 sampler steps:
          8 x 512 = 4 096 for 11 776 useful tokens;
  engine  the same requests through ``generation_engine(pool, max_batch=8).run()``: at least 11 776 / 8 = 1 472 steps.
Method (tests/bench_paged.py): one event pair on the launch stream around a whole run, one warm-up, the variants
alternating in one process, the median of 5 runs with [min, max].  Recorded: useful tokens per second and sampler / decode
steps of both variants, and the step ratio of the host replay of the scheduler (``engine.Replay``).
The one condition (exit status 1 otherwise): the engine's median wall time is below the static median measured beside it.
No margin is fixed beyond that: what the engine adds per request is a B = 1 prefill and a table upload, and whether 2.8x
fewer steps become a like gain in time is what this file measures.
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from speech_distill_amd.engine import Replay, static_steps  # noqa: E402
from speech_distill_amd.generation import REFERENCE_SAMPLING  # noqa: E402
from bench_decode_gemv import REPS, student  # noqa: E402

dev = torch.device("cuda:0")
N_REQ, T, B, N_PAGES = 64, 128, 8, 32
BUDGETS = [(32, 64, 128, 512)[i % 4] for i in range(N_REQ)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3, out        # seconds


def main():
    m = student()
    V = m.dims.vocab_size
    ids = torch.randint(0, V, (N_REQ, T), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pool = m.kv_page_pool(N_PAGES)

    def static():
        steps = 0
        for s in range(0, N_REQ, B):
            n = max(BUDGETS[s:s + B])
            m.generate(ids[s:s + B], max_new_tokens=n, seed=s, decode_kernels="skinny", **REFERENCE_SAMPLING)
            steps += n
        return {"sampler_steps": steps, "decode_steps": steps - N_REQ // B}

    def engine():
        eng = m.generation_engine(pool, max_batch=B, decode_kernels="skinny")
        rids = [eng.submit(ids[i], max_new_tokens=BUDGETS[i], seed=i, **REFERENCE_SAMPLING) for i in range(N_REQ)]
        eng.run()
        stats = dict(eng.stats)
        eng.close()
        assert len(rids) == N_REQ
        return {"sampler_steps": stats["iterations"], "decode_steps": stats["decode_steps"], "prefills": stats["prefills"],
                "peak_pages": stats["peak_pages"]}

    rep = Replay(B, N_PAGES, N_PAGES - 1, (N_PAGES - 1) * 256)
    for n in BUDGETS:
        rep.submit(T, n, n)
    rep.run()
    useful = sum(BUDGETS)
    res = {"device": torch.cuda.get_device_name(0), "shape": "student 0.6B (159488, 1024, 3072, 28, 16, 8)", "reps": REPS,
           "method": "one event pair on the launch stream around a whole run; one warm-up, variants alternating in one "
                     "process, median of 5 runs [min, max]",
           "workload": {"requests": N_REQ, "prompt_tokens": T, "budgets_cycle": [32, 64, 128, 512], "max_batch": B,
                        "decode_kernels": "skinny", "useful_tokens": useful, "eos": None, "sampling": REFERENCE_SAMPLING},
           "replay": {"static_sampler_steps": static_steps(BUDGETS, B), "engine_sampler_steps": rep.stats["iterations"],
                      "step_ratio": static_steps(BUDGETS, B) / rep.stats["iterations"]}}
    fns = {"static": static, "engine": engine}
    runs, info = {k: [] for k in fns}, {}
    for k, fn in fns.items():
        timed(fn)                                   # warm-up
    for _ in range(REPS):
        for k, fn in fns.items():
            s, info[k] = timed(fn)
            runs[k].append(s)
    for k in fns:
        med = statistics.median(runs[k])
        res[k] = {"seconds": med, "seconds_min": min(runs[k]), "seconds_max": max(runs[k]),
                  "useful_tokens_per_s": useful / med, **info[k]}
        print(f"{k:7s}: {med:7.3f} s [{min(runs[k]):.3f}, {max(runs[k]):.3f}]  {useful / med:9.1f} useful tokens/s  "
              f"{info[k]}", flush=True)
    assert res["engine"]["sampler_steps"] == rep.stats["iterations"], "the engine's steps are not the replay's"
    res["static_rel_spread"] = (res["static"]["seconds_max"] - res["static"]["seconds_min"]) / res["static"]["seconds"]
    res["engine_over_static_time"] = res["engine"]["seconds"] / res["static"]["seconds"]
    res["ok"] = res["engine"]["seconds"] < res["static"]["seconds"]
    print(f"replay step ratio x{res['replay']['step_ratio']:.2f}; engine / static time x{res['engine_over_static_time']:.3f} "
          f"(static spread {res['static_rel_spread']:.3f}); ok: {res['ok']}", flush=True)
    out = os.path.join(ROOT, "profiles", "engine_bench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
