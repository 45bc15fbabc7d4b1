"""GPU measurement (not a pytest): multi-turn generation on the 0.6B student shape.  Writes profiles/session_bench.json.

  (a) one dialogue turn -- 64 given tokens + 128 new tokens (reference sampling defaults, no stop token) behind a history
      of {1024, 4096} tokens, B in {1, 8}: a ``GenerationSession`` whose cache holds the history (the turn runs
      sd_qwen3_extend over the pending token + the 64 given ones, then 128 decode steps) against ``generate`` on the whole
      history + turn, the only way there was before;
  (b) sd_attn_extend alone (Hq 16, Hkv 8) at block in {64, 512} x past in {0, 4096}, B in {1, 8}: microseconds and K/V
      bytes per second, beside sd_attn_fwd on the same T (past = 0) in the same process.
The one condition: the session turn is faster than ``generate`` at history 4096, B = 1 and B = 8 (exit status 1 if not).
Events on the launch stream, one warm-up, median of 5 with [min, max].
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
from speech_distill_amd.generation import REFERENCE_SAMPLING  # noqa: E402

dev = torch.device("cuda:0")
REPS = 5


def timed(fn, before=None, reps=REPS, warm=1):
    """(median, [min, max]) milliseconds of fn() over `reps` runs after `warm` warm-ups; before() runs untimed each time."""
    out = []
    for i in range(warm + reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return statistics.median(out), [min(out), max(out)]


def student():
    m = sda.HipQwen3ForCausalLM(sda.Qwen3Dims.student_06b(), device=dev, init_std=0)
    with torch.no_grad():
        m.flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(0))
        for p in m._params.values():
            if p.dim() == 1:
                p.fill_(1.0)
    return m.eval()


def bench_turn(m, res):
    V, text, new = m.dims.vocab_size, 64, 128
    ok = True
    for hist in (1024, 4096):
        for B in (1, 8):
            ids = torch.randint(0, V, (B, hist + text), device=dev, generator=torch.Generator(device=dev).manual_seed(B))
            kw = dict(max_new_tokens=new, seed=1, **REFERENCE_SAMPLING)
            sess = m.start_session(B, capacity=(hist + text + new + 255) // 256 * 256)
            sess.extend(ids[:, :hist].contiguous())
            turn = ids[:, hist:].contiguous()

            def rewind():   # the state a finished turn leaves: the history's last token is in seq but not in the cache
                sess.len.fill_(hist), sess.cached.fill_(hist - 1)
                sess._pending, sess._bound = True, hist
            ms_s, rng_s = timed(lambda: sess.generate(turn, **kw), before=rewind)
            ms_g, rng_g = timed(lambda: m.generate(ids, **kw))
            res["turn"].append({"B": B, "history": hist, "given": text, "new_tokens": new, "session_ms": ms_s,
                                "session_ms_range": rng_s, "generate_ms": ms_g, "generate_ms_range": rng_g,
                                "speedup": ms_g / ms_s})
            print(f"turn B={B} history={hist}: session {ms_s:8.1f} ms [{rng_s[0]:.1f}, {rng_s[1]:.1f}]   generate on the whole "
                  f"history {ms_g:8.1f} ms [{rng_g[0]:.1f}, {rng_g[1]:.1f}]   x{ms_g / ms_s:5.2f}", flush=True)
            if hist == 4096:
                ok = ok and ms_s < ms_g
            del sess
    res["session_turn_faster_at_history_4096"] = ok
    return ok


def bench_attention(res):
    Hq, Hkv, n = 16, 8, 20
    for B in (1, 8):
        for block in (64, 512):
            q = torch.randn(B * block, Hq * 128, device=dev).bfloat16()
            kf = torch.randn(B * block, Hkv * 128, device=dev).bfloat16()
            vf = torch.randn(B * block, Hkv * 128, device=dev).bfloat16()

            def fwd():
                for _ in range(n):
                    ops.attn_fwd(q, kf, vf, B, block, Hq, Hkv)
            ms_f, rng_f = timed(fwd)
            for past in (0, 4096):
                cap = past + block
                kp = torch.randn(B, cap, Hkv * 128, device=dev).bfloat16()
                vp = torch.randn(B, cap, Hkv * 128, device=dev).bfloat16()
                p_d = torch.full((B,), past, dtype=torch.int32, device=dev)
                n_d = torch.full((B,), block, dtype=torch.int32, device=dev)

                def ext():
                    for _ in range(n):
                        ops.attn_extend(q, kp, vp, p_d, n_d, block, Hq, Hkv)
                ms, rng = timed(ext)
                us, nbytes = ms / n * 1e3, 2 * B * cap * Hkv * 128 * 2
                res["attn_extend"].append({"B": B, "block": block, "past": past, "us": us,
                                           "us_range": [r / n * 1e3 for r in rng], "kv_bytes": nbytes,
                                           "GBps": nbytes / us / 1e3, "attn_fwd_same_T_us": ms_f / n * 1e3,
                                           "attn_fwd_same_T_us_range": [r / n * 1e3 for r in rng_f]})
                print(f"attn_extend B={B} block={block:3d} past={past:4d}: {us:8.1f} us  {nbytes / us / 1e3:7.1f} GB/s of K/V"
                      f"   (sd_attn_fwd T={block}: {ms_f / n * 1e3:7.1f} us)", flush=True)


def main():
    res = {"device": torch.cuda.get_device_name(0), "shape": "student 0.6B (159488, 1024, 3072, 28, 16, 8)", "reps": REPS,
           "sampling": REFERENCE_SAMPLING, "turn": [], "attn_extend": []}
    bench_attention(res)
    ok = bench_turn(student(), res)
    out = os.path.join(ROOT, "profiles", "session_bench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
