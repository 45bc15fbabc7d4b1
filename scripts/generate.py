#!/usr/bin/env python3
"""Decode speech tokens from a trained checkpoint over a KV cache (``HipQwen3ForCausalLM.generate``).

Counterpart of the reference's inference engine for the LM part only (soulxpodcast/engine/llm_engine.py:37-76): the
prompts are token ids, the output is token ids; tokenizer and vocoder stay outside.  The sampling flags default to the
reference's ``SamplingParams`` (soulxpodcast/config.py:107-118): temperature 0.6, top-k 100, top-p 0.9, repetition
penalty 1.25, min 8 / max 3000 new tokens, stop token 151675, repetition-aware sampling with window 25 and threshold 0.2.

    python scripts/generate.py /out/checkpoint-1000 prompts.jsonl --output generated.jsonl

``prompts.jsonl``: one JSON object per line with ``input_ids`` (a list of token ids), or a bare list.  An object may carry
``"turns": [[ids], [ids], ...]`` instead: a dialogue whose turns are generated one after the other over ONE live KV cache
(``model.start_session``; the reference's dialogue loop, soulxpodcast/models/soulxpodcast.py:339-386) -- turn n feeds only
its own text behind the history the cache already holds.  The dialogues of a batch take their turns together, so prompts
are batched by turn count.  The output holds, per prompt and turn, ``{"index", "turn", "prompt_len", "generated_ids"}``
with the ids up to and including the stop token.

``--continuous`` (needs ``--kv_pool_pages``): the single-turn prompts are served by the request engine
(``model.generation_engine``; the reference's engine is vLLM, llm_engine.py:91) -- ``--batch_size`` rows, a row that
finishes is refilled with the next prompt at once, request i is seeded with ``--seed`` + i, and the results are written
in input order.  Dialogues (``"turns"``) keep the session path.
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
    p.add_argument("--decode_kernels", choices=("tile", "skinny", "wide"), default="tile",
                   help="skinny: weight-streaming GEMV kernels for the decode step (batch_size <= 16); wide: the MFMA "
                        "weight-streaming kernels (batch_size <= 64, bf16 weights)")
    p.add_argument("--gemv_rows", type=int, choices=(16, 64), default=16,
                   help="64 (with --decode_kernels skinny --weight_dtype mxfp8): the 64-row block-scaled GEMV kernels, "
                        "batch-invariant steps for batch_size <= 64")
    p.add_argument("--decode_attention", choices=("split", "fused"), default="split",
                   help="fused: every decode step runs each layer's q/k-norm + RoPE, cache append, split-KV attention and "
                        "merge as one launch instead of three; the tokens are the same")
    p.add_argument("--kv_pool_pages", type=int, default=0,
                   help="0: every batch reserves a contiguous KV cache for its worst case.  N > 0: every batch's session "
                        "draws pages of 256 positions from ONE pool of N pages, turn by turn (the paged cache of the "
                        "reference's engine, llm_engine.py:91); the tokens are the same")
    p.add_argument("--kv_cache_dtype", choices=("bf16", "mxfp8"), default="bf16",
                   help="mxfp8 (needs --kv_pool_pages): the pool holds 8-bit pages -- e4m3 elements with one power-of-two "
                        "scale per 32 of them, 0.516 of the bf16 bytes; what is cached is quantised, so the tokens may "
                        "differ from the bf16 cache's")
    p.add_argument("--weight_dtype", choices=("bf16", "mxfp8"), default="bf16",
                   help="mxfp8: prefill and every decode step run the q|k|v, o, gate|up and down projections on MXFP8 "
                        "weights quantised once at start-up (e4m3 with one power-of-two scale per 32 along K; the model "
                        "is frozen for it); with --decode_kernels skinny they are streamed through the block-scaled "
                        "GEMV.  Independent of --kv_cache_dtype; the tokens may differ from the bf16 weights'")
    p.add_argument("--continuous", action="store_true",
                   help="continuous batching (needs --kv_pool_pages): --batch_size becomes the engine's max_batch and a "
                        "finished row is refilled with the next prompt at once; dialogues keep the session path")
    args = p.parse_args(argv)
    if args.continuous and args.kv_pool_pages <= 0:
        p.error("--continuous needs --kv_pool_pages N: the engine serves its rows from a page pool")
    if args.kv_cache_dtype != "bf16" and args.kv_pool_pages <= 0:
        p.error("--kv_cache_dtype mxfp8 needs --kv_pool_pages N: only the paged cache has an 8-bit form")
    return args


def read_prompts(path):
    """One dialogue per line, as a list of turns (each a non-empty list of token ids); a plain prompt is one turn."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            row = json.loads(line)
            if isinstance(row, dict) and "turns" in row:
                turns = row["turns"]
                if not turns:
                    raise ValueError(f"{path}: a dialogue without turns")
            else:
                turns = [row["input_ids"] if isinstance(row, dict) else row]
            if any(not ids for ids in turns):
                raise ValueError(f"{path}: an empty prompt")
            out.append([[int(t) for t in ids] for ids in turns])
    return out


def batches_by_turn_count(dialogues, batch_size):
    """[(indices, dialogues)] with at most ``batch_size`` dialogues of EQUAL turn count each (a dialogue with fewer turns
    would sit the later ones out), in order of first appearance."""
    groups = {}
    for i, d in enumerate(dialogues):
        groups.setdefault(len(d), []).append(i)
    out = []
    for idx in groups.values():
        for s in range(0, len(idx), batch_size):
            part = idx[s:s + batch_size]
            out.append((part, [dialogues[i] for i in part]))
    return out


def right_pad(rows, pad):
    T = max(len(r) for r in rows)
    ids = torch.full((len(rows), T), pad, dtype=torch.int64)
    mask = torch.zeros(len(rows), T, dtype=torch.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r)
        mask[i, :len(r)] = 1
    return ids, mask


def serve_continuous(model, pool, args, pad, prompts, out):
    """Serve ``prompts`` [(index, ids)] through the request engine and write them in input order.  -> (new tokens, s)."""
    if not prompts:
        return 0, 0.0
    dev = model.flat.device
    eng = model.generation_engine(pool, max_batch=args.batch_size, decode_kernels=args.decode_kernels,
                                  weight_dtype=args.weight_dtype, sync_every=args.sync_every,
                                  decode_attention=args.decode_attention, gemv_rows=args.gemv_rows)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [eng.submit(torch.tensor(ids, dtype=torch.int64, device=dev), max_new_tokens=args.max_tokens,
                       seed=None if args.seed is None else args.seed + i, min_new_tokens=args.min_tokens,
                       do_sample=not args.greedy, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                       repetition_penalty=args.repetition_penalty, eos_token_id=args.stop_token_id, pad_token_id=pad,
                       use_ras=not args.no_ras, win_size=args.win_size, tau_r=args.tau_r) for i, ids in prompts]
    eng.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n_new = 0
    for (i, ids), rid in zip(prompts, rids):
        row = eng.result(rid).cpu().tolist()
        n_new += len(row)
        out.write(json.dumps({"index": i, "turn": 0, "prompt_len": len(ids), "generated_ids": row}) + "\n")
    eng.close()
    return n_new, dt


def main(argv=None):
    args = parse_args(argv)
    import speech_distill_amd as sda
    from speech_distill_amd.generation import cache_capacity
    model = sda.HipQwen3ForCausalLM.from_pretrained(args.checkpoint, device="cuda").eval()
    if args.weight_dtype == "mxfp8":
        model.requires_grad_(False)   # the quantised weights are made once: a frozen model
    dialogues = read_prompts(args.prompts)
    pad = args.pad_token_id if args.pad_token_id is not None else args.stop_token_id
    dev = model.flat.device
    n_new, elapsed = 0, 0.0
    pool = model.kv_page_pool(args.kv_pool_pages, kv_dtype=args.kv_cache_dtype) if args.kv_pool_pages > 0 else None
    with open(args.output, "w") as out:
        if args.continuous:
            single = [i for i, d in enumerate(dialogues) if len(d) == 1]
            n, dt = serve_continuous(model, pool, args, pad, [(i, dialogues[i][0]) for i in single], out)
            n_new, elapsed = n_new + n, elapsed + dt
            keep = [i for i, d in enumerate(dialogues) if len(d) > 1]
            batches = [([keep[j] for j in idx], chunk)
                       for idx, chunk in batches_by_turn_count([dialogues[i] for i in keep], args.batch_size)]
        else:
            batches = batches_by_turn_count(dialogues, args.batch_size)
        for index, chunk in batches:
            n_turns = len(chunk[0])
            need = max(sum(len(t) for t in d) for d in chunk) + n_turns * args.max_tokens
            if need > cache_capacity(model):
                raise ValueError(f"a dialogue of {need} positions exceeds the KV-cache capacity {cache_capacity(model)}")
            sess = model.start_session(len(chunk), (need + 255) // 256 * 256, decode_kernels=args.decode_kernels, pool=pool,
                                       weight_dtype=args.weight_dtype, decode_attention=args.decode_attention,
                                       gemv_rows=args.gemv_rows)
            for turn in range(n_turns):
                ids, mask = right_pad([d[turn] for d in chunk], pad)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = sess.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=args.max_tokens,
                                    min_new_tokens=args.min_tokens, do_sample=not args.greedy,
                                    temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                                    repetition_penalty=args.repetition_penalty, eos_token_id=args.stop_token_id,
                                    pad_token_id=pad, use_ras=not args.no_ras, win_size=args.win_size, tau_r=args.tau_r,
                                    seed=None if args.seed is None else args.seed + turn, sync_every=args.sync_every)
                torch.cuda.synchronize()
                elapsed += time.perf_counter() - t0
                for i, row in enumerate(res.cpu().tolist()):
                    if args.stop_token_id in row:
                        row = row[:row.index(args.stop_token_id) + 1]
                    n_new += len(row)
                    out.write(json.dumps({"index": index[i], "turn": turn, "prompt_len": len(chunk[i][turn]),
                                          "generated_ids": row}) + "\n")
            sess.close()    # a paged session hands its pages back to the pool for the next batch
    print(f"{len(dialogues)} prompts, {n_new} new tokens in {elapsed:.2f} s: {n_new / max(elapsed, 1e-9):.1f} tokens/s "
          f"-> {args.output}")


if __name__ == "__main__":
    main()
