#!/usr/bin/env python3
"""Decode speech tokens from a trained checkpoint over a KV cache (``HipQwen3ForCausalLM.generate``).

Counterpart of the reference's inference engine for the LM part only (soulxpodcast/engine/llm_engine.py:37-76): the
prompts are token ids, the output is token ids; tokenizer and vocoder stay outside.  The sampling flags default to the
reference's ``SamplingParams`` (soulxpodcast/config.py:107-118): temperature 0.6, top-k 100, top-p 0.9, repetition
penalty 1.25, min 8 / max 3000 new tokens, stop token 151675, repetition-aware sampling with window 25 and threshold 0.2.

    python scripts/generate.py /out/checkpoint-1000 prompts.jsonl --output generated.jsonl

``prompts.jsonl``: one JSON object per line with ``input_ids`` (a list of token ids), or a bare list.  The output holds,
per prompt, ``{"index", "prompt_len", "generated_ids"}`` with the ids up to and including the stop token.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="KV-cache generation from a checkpoint directory")
    p.add_argument("checkpoint", help="directory written by save_pretrained (config.json + model.safetensors)")
    p.add_argument("prompts", help="JSONL of prompt token ids")
    p.add_argument("--output", default="generated.jsonl")
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--temperature", type=float, default=0.6)          # config.py:108
    p.add_argument("--repetition_penalty", type=float, default=1.25)  # config.py:109
    p.add_argument("--top_k", type=int, default=100)                  # config.py:110
    p.add_argument("--top_p", type=float, default=0.9)                # config.py:111
    p.add_argument("--min_tokens", type=int, default=8)               # config.py:112
    p.add_argument("--max_tokens", type=int, default=3000)            # config.py:113
    p.add_argument("--stop_token_id", type=int, default=151675)       # config.py:114
    p.add_argument("--pad_token_id", type=int, default=None)
    p.add_argument("--no_ras", action="store_true", help="switch repetition-aware sampling off (on in the reference)")
    p.add_argument("--win_size", type=int, default=25)                # config.py:117
    p.add_argument("--tau_r", type=float, default=0.2)                # config.py:118
    p.add_argument("--greedy", action="store_true", help="arg-max instead of sampling")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--sync_every", type=int, default=16)
    p.add_argument("--decode_kernels", choices=("tile", "skinny"), default="tile",
                   help="skinny: weight-streaming GEMV kernels for the decode step (batch_size <= 16)")
    return p.parse_args(argv)


def read_prompts(path):
    out = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            row = json.loads(line)
            ids = row["input_ids"] if isinstance(row, dict) else row
            if not ids:
                raise ValueError(f"{path}: an empty prompt")
            out.append([int(t) for t in ids])
    return out


def main(argv=None):
    args = parse_args(argv)
    import speech_distill_amd as sda
    model = sda.HipQwen3ForCausalLM.from_pretrained(args.checkpoint, device="cuda").eval()
    prompts = read_prompts(args.prompts)
    pad = args.pad_token_id if args.pad_token_id is not None else args.stop_token_id
    dev = model.flat.device
    n_new, elapsed = 0, 0.0
    with open(args.output, "w") as out:
        for s in range(0, len(prompts), args.batch_size):
            chunk = prompts[s:s + args.batch_size]
            T = max(len(p) for p in chunk)
            ids = torch.full((len(chunk), T), pad, dtype=torch.int64)
            mask = torch.zeros(len(chunk), T, dtype=torch.int64)
            for i, p in enumerate(chunk):   # right padding
                ids[i, :len(p)] = torch.tensor(p)
                mask[i, :len(p)] = 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=args.max_tokens,
                                 min_new_tokens=args.min_tokens, do_sample=not args.greedy, temperature=args.temperature,
                                 top_k=args.top_k, top_p=args.top_p, repetition_penalty=args.repetition_penalty,
                                 eos_token_id=args.stop_token_id, pad_token_id=pad, use_ras=not args.no_ras,
                                 win_size=args.win_size, tau_r=args.tau_r, seed=args.seed, sync_every=args.sync_every,
                                 decode_kernels=args.decode_kernels)
            torch.cuda.synchronize()
            elapsed += time.perf_counter() - t0
            new = res[:, T:].cpu().tolist()
            for i, row in enumerate(new):
                if args.stop_token_id in row:
                    row = row[:row.index(args.stop_token_id) + 1]
                n_new += len(row)
                out.write(json.dumps({"index": s + i, "prompt_len": len(chunk[i]), "generated_ids": row}) + "\n")
    print(f"{len(prompts)} prompts, {n_new} new tokens in {elapsed:.2f} s: {n_new / max(elapsed, 1e-9):.1f} tokens/s "
          f"-> {args.output}")


if __name__ == "__main__":
    main()
