"""GPU measurement (not a pytest): KV-cache generation on the 0.6B student shape.  Writes profiles/generate_bench.json.

  * tokens/s of ``generate`` (reference sampling defaults, no stop token) for B in {1, 8, 64}, prompt 256, 512 new tokens;
  * K/V bytes per second of sd_attn_decode at B in {1, 16, 64} x context in {512, 4096} (Hq 16, Hkv 8), beside the
    streaming read rate tests/bench_hbm.py measures (its log-softmax + top-k pass over 1536 x 159488 bf16), same session;
  * time per token of cached decode against the only method there was before: ``forward`` on the whole prefix (lm_head on
    the last row only), 32 tokens at context 512, B in {1, 8}.
The one condition: cached decode takes less time per token than the re-forward, B = 1 and B = 8 (exit status 1 if not).
Everything is timed with events on the launch stream, after a warm-up, over at least 5 repetitions (the median is kept).
"""
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

dev = torch.device("cuda:0")
REPS = 5


def timed(fn, reps=REPS, warm=1):
    """Median milliseconds of fn() over `reps` runs, events on the current stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def student():
    m = sda.HipQwen3ForCausalLM(sda.Qwen3Dims.student_06b(), device=dev, init_std=0)
    with torch.no_grad():
        m.flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(0))
        for p in m._params.values():
            if p.dim() == 1:
                p.fill_(1.0)
    return m.eval()


def bench_generate(m, res):
    V = m.dims.vocab_size
    for B in (1, 8, 64):
        ids = torch.randint(0, V, (B, 256), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
        ms, runs = timed(lambda: m.generate(ids, max_new_tokens=512, seed=1, **REFERENCE_SAMPLING))
        res["generate"].append({"B": B, "prompt": 256, "new_tokens": 512, "ms": ms, "ms_runs": runs,
                                "tokens_per_s": B * 512 / ms * 1e3, "ms_per_step": ms / 512})
        print(f"generate B={B}: {ms:8.1f} ms  {B * 512 / ms * 1e3:9.1f} tokens/s  {ms / 512:6.3f} ms/step", flush=True)


def bench_attention(res):
    Hq, Hkv = 16, 8
    for B in (1, 16, 64):
        for ctx in (512, 4096):
            k = torch.randn(B, ctx, Hkv * 128, device=dev).bfloat16()
            v = torch.randn(B, ctx, Hkv * 128, device=dev).bfloat16()
            q = torch.randn(B, Hq * 128, device=dev).bfloat16()
            lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            ws = torch.empty(ops.load_lib().sd_attn_decode_workspace_bytes(B, Hq, ctx), dtype=torch.uint8, device=dev)

            def run():
                for _ in range(20):
                    ops.attn_decode(q, k, v, lens, Hq, Hkv, max_len=ctx, workspace=ws)
            ms, _ = timed(run, warm=2)
            us = ms / 20 * 1e3
            nbytes = 2 * B * ctx * Hkv * 128 * 2
            res["attn_decode"].append({"B": B, "context": ctx, "us": us, "kv_bytes": nbytes, "GBps": nbytes / us / 1e3})
            print(f"attn_decode B={B:2d} ctx={ctx:4d}: {us:7.1f} us  {nbytes / us / 1e3:7.0f} GB/s of K/V", flush=True)


def bench_stream(res):
    import bench_hbm
    R, V, K = 1536, 159488, 128     # the read stream of tests/bench_hbm.py
    logits = (torch.randn(R, V, device=dev) * 2).bfloat16()
    us = bench_hbm.timeit(lambda: ops.logsoftmax_topk(logits, K, V))
    res["stream_read"] = {"what": "tests/bench_hbm.py: log-softmax + top-128 over 1536 x 159488 bf16", "us": us,
                          "GBps": R * V * 2 / us / 1e3}
    print(f"streaming read (bench_hbm top-k pass): {us:7.1f} us  {R * V * 2 / us / 1e3:7.0f} GB/s", flush=True)


def bench_vs_reforward(m, res):
    V = m.dims.vocab_size
    ok = True
    for B in (1, 8):
        ctx, n = 512, 32
        ids = torch.randint(0, V, (B, ctx + n), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
        rows = [torch.arange(B, device=dev) * (ctx + t) + ctx + t - 1 for t in range(n)]

        def reforward():
            with torch.no_grad():
                for t in range(n):
                    m(input_ids=ids[:, :ctx + t].contiguous(), logit_rows=rows[t])
        dec = Decoder(m, B, ctx + n)
        kv_len = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        dec.prefill(ids[:, :ctx].contiguous(), kv_len)
        pos = [(kv_len + t).contiguous() for t in range(n)]
        toks = [ids[:, ctx + t].contiguous() for t in range(n)]
        seq = torch.zeros(B, ctx + n + 1, dtype=torch.int64, device=dev)
        sp = ops.sample_params(**REFERENCE_SAMPLING)
        u = torch.rand(B, 2, device=dev)
        ws = torch.empty(ops.load_lib().sd_sample_workspace_bytes(B, V), dtype=torch.uint8, device=dev)
        fin = torch.zeros(B, dtype=torch.uint8, device=dev)

        def cached():   # the decode step plus the sampler, as generate runs them
            lens = kv_len.clone()
            for t in range(n):
                logits = dec.step(toks[t], pos[t], ctx + t + 1)
                ops.sample_step(logits, u, seq, kv_len, lens, fin, sp, workspace=ws)
        ms_r, _ = timed(reforward)
        ms_c, _ = timed(cached)
        res["vs_reforward"].append({"B": B, "context": ctx, "tokens": n, "reforward_ms_per_token": ms_r / n,
                                    "cached_ms_per_token": ms_c / n, "speedup": ms_r / ms_c})
        print(f"B={B} ctx=512: re-forward {ms_r / n:7.3f} ms/token   cached {ms_c / n:7.3f} ms/token   x{ms_r / ms_c:5.1f}",
              flush=True)
        ok = ok and ms_c < ms_r
    res["cached_faster_than_reforward"] = ok
    return ok


def main():
    res = {"device": torch.cuda.get_device_name(0), "shape": "student 0.6B (159488, 1024, 3072, 28, 16, 8)", "reps": REPS,
           "sampling": REFERENCE_SAMPLING, "generate": [], "attn_decode": [], "vs_reforward": []}
    bench_stream(res)
    bench_attention(res)
    m = student()
    ok = bench_vs_reforward(m, res)
    bench_generate(m, res)
    out = os.path.join(ROOT, "profiles", "generate_bench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
