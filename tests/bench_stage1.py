"""Stage-1 alignment step vs the full fine-tune student step on the same batch (0.6B student, one MI355X).

Shapes: B=4 x T=512, and 4 right-padded documents of T=4096 with layer recompute.  Reports ms per Stage-1 micro-step
(forward + CE + embedding-only backward), ms per full-gradient student step (forward + CE + full backward, no teacher),
their ratio, the CE kernels' HBM rates and the range scatter's time, as one JSON line (and into --out).

    python tests/bench_stage1.py --out profiles/stage1_bench.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    cfg = ap.parse_args()
    import speech_distill_amd as sda
    from speech_distill_amd import ops
    from speech_distill_amd.stage1 import freeze_model_weights
    dev = torch.device("cuda:0")
    dims = sda.Qwen3Dims.student_06b()
    V, lo = dims.vocab_size, dims.vocab_size - 8220
    res = {"model": "qwen3-0.6b (V=159488)", "num_new_tokens": 8220, "shapes": []}
    g = torch.Generator().manual_seed(0)
    for B, T, recompute, lens in ((4, 512, False, None), (4, 4096, True, (4096, 3500, 2900, 2048))):
        ids = torch.randint(0, V, (B, T), generator=g).to(dev)
        am = torch.ones(B, T, dtype=torch.long)
        if lens:
            for r, n in enumerate(lens):
                am[r, n:] = 0
        am = am.to(dev)
        lab = ids.masked_fill(am == 0, -100)
        lab[:, 0] = -100
        n_items = torch.tensor(float(lab[:, 1:].ne(-100).sum()), device=dev)
        row = {"B": B, "T": T, "recompute": recompute, "tokens": int(am.sum())}
        for mode in ("full", "stage1"):
            m = sda.HipQwen3ForCausalLM(dims, device=dev, seed=0)
            m.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"recompute": "always" if recompute else "never"})
            if mode == "stage1":
                freeze_model_weights(m, 8220)

            def step():
                if mode == "stage1":
                    out = m(input_ids=ids, attention_mask=am, labels=lab, num_items_in_batch=n_items, stage1_inplace_grad=True)
                    out.loss.backward()
                else:  # the full fine-tune student micro-step: same rows, same CE kernel, every gradient
                    rows, rl = ops.loss_rows(lab, right_padded=(am,))
                    logits = m(input_ids=ids, attention_mask=am, logit_rows=rows, padding_checked=True).logits
                    loss, _ = ops.celoss_rows(logits, rl, n_items, inplace_grad=True)
                    loss.backward()
            row[f"{mode}_ms"] = round(_time(step, cfg.warmup, cfg.iters), 3)
            if mode == "stage1":
                ops.prof_begin()
                step()
                torch.cuda.synchronize()
                prof = ops.prof_end()
                sym = ops.prof_symbols()
                for k, key in (("loss_fwd", "ce_fwd"), ("loss_bwd", "ce_bwd")):
                    ms, work, _ = prof[k]
                    row[f"{key}_ms"] = round(ms, 4)
                    row[f"{key}_TBps"] = round(work / ms / 1e9, 2) if ms > 0 else None
                row["range_scatter_ms"] = round(sum(v[0] for s, v in sym.items() if s.startswith("embedding_bwd")), 4)
                row["dw_gemm_ms"] = round(prof["gemm_tn"][0], 4)
            del m
            torch.cuda.empty_cache()
        row["stage1_over_full"] = round(row["stage1_ms"] / row["full_ms"], 3)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))
    if cfg.out:
        os.makedirs(os.path.dirname(os.path.abspath(cfg.out)), exist_ok=True)
        with open(cfg.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
