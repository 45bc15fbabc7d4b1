#!/usr/bin/env python3
"""Stage-1 speech-token alignment on the MI355X path: counterpart of the reference's ``stage1.py`` (orchestration
:96-335, flags :338-526).  Same flag names and defaults; additions are marked (+).  Only the new speech-token rows of
the embedding (and of an untied lm_head) train; every other weight leaves bit-identical.

Data: a ``load_from_disk`` directory whose rows carry ``input_ids`` (what the reference's SpeechDistillDatasetProcessor
produces before it decodes them to text), or a ``text`` column tokenised with the tokenizer in ``--model_path``.  The
audio-to-token step (s3tokenizer) stays outside, as for scripts/train.py.  Packing: best-fit-decreasing bins of
``--max_seq_length`` (speech_distill_amd/stage1.py), each document its own right-padded row, or with ``--padding_free``
all documents of a micro-batch in one row without padding (varlen attention).

    python scripts/stage1.py --model_path /models/qwen3-0.6b-expanded --dataset_path /data/tokenised \\
        --output_dir /out/stage1 --num_new_tokens 8220
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Stage 1: Text-to-Speech Token Alignment Training")
    p.add_argument("--model_path", type=str, default=None)            # stage1.py:344-349 (required there; see --random_init)
    p.add_argument("--dataset_path", type=str, default=None)          # stage1.py:350-355
    p.add_argument("--output_dir", type=str, required=True)           # stage1.py:356-361
    p.add_argument("--num_epochs", type=int, default=3)
    p.add_argument("--batch_size", type=int, default=4, help="packed bins per micro-batch")
    p.add_argument("--eval_batch_size", type=int, default=8)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--warmup_steps", type=int, default=1000)
    p.add_argument("--weight_decay", type=float, default=0.01)
    p.add_argument("--gradient_accumulation_steps", type=int, default=4)
    p.add_argument("--logging_steps", type=int, default=50)
    p.add_argument("--save_steps", type=int, default=500)
    p.add_argument("--eval_steps", type=int, default=500)
    p.add_argument("--eval_size", type=float, default=0)
    p.add_argument("--max_seq_length", type=int, default=4096)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--num_new_tokens", type=int, default=8220)
    p.add_argument("--prefix", type=str, default="")
    p.add_argument("--text_bos", type=str, default="<|text_start|>")
    p.add_argument("--text_eos", type=str, default="<|text_end|>")
    p.add_argument("--text_prefix", type=str, default='{"en": "", "zh": "", "yue": "<|Yue|>"}')
    p.add_argument("--speech_bos", type=str, default="<|semantic_token_start|>")
    p.add_argument("--speech_eos", type=str, default="<|semantic_token_end|>")
    # store_true + set_defaults(True) in the reference (stage1.py:478-484): on, and cannot be switched off from there either
    p.add_argument("--gradient_checkpointing", action="store_true", default=True)
    p.add_argument("--use_8bit_optimizer", action="store_true", default=False)
    p.add_argument("--use_wandb", action="store_true", default=False)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--random_init", action="store_true", help="(+) build the student shape with HF default init")
    p.add_argument("--tiny", action="store_true", help="(+) with --random_init: a 2-layer model (plumbing runs)")
    p.add_argument("--synthetic_samples", type=int, default=0, help="(+) N synthetic tokenised documents")
    p.add_argument("--max_steps", type=int, default=-1, help="(+) stop after this many optimizer steps")
    p.add_argument("--log_json", default=None, help="(+) write the log history and a summary there")
    p.add_argument("--recompute", default="auto", choices=["auto", "always", "never"],
                   help="(+) what gradient checkpointing does (see scripts/train.py)")
    p.add_argument("--padding_free", action="store_true", default=False,
                   help="(+) flatten each micro-batch's documents into one row without padding (position_ids + varlen "
                        "attention, TRL padding_free) instead of one right-padded row per document")
    return p.parse_args(argv)


def refuse(cfg):
    """What this path does not do, with the reason (None = fine)."""
    if cfg.use_8bit_optimizer:
        return "--use_8bit_optimizer: 8-bit AdamW (bitsandbytes) is not available on this path; drop the flag (adamw_torch)"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "Stage-1 runs on one GPU here (WORLD_SIZE > 1): launch it without torchrun"
    if not cfg.random_init and not cfg.model_path:
        return "--model_path is required (or --random_init)"
    if not cfg.synthetic_samples and not cfg.dataset_path:
        return "--dataset_path is required (or --synthetic_samples)"
    return None


def load_documents(cfg, V, tokenizer):
    if cfg.synthetic_samples:
        g = torch.Generator().manual_seed(1234)
        lo = max(8, cfg.max_seq_length // 8)
        return [torch.randint(0, V, (int(torch.randint(lo, cfg.max_seq_length + 1, (1,), generator=g)),), generator=g).tolist()
                for _ in range(cfg.synthetic_samples)]
    from datasets import load_dataset, load_from_disk
    ds = load_from_disk(cfg.dataset_path) if os.path.exists(cfg.dataset_path) else load_dataset(cfg.dataset_path)
    if isinstance(ds, dict):                                  # stage1.py:162-166
        ds = ds.get("train", ds)
    if "input_ids" in ds.column_names:
        return [list(x) for x in ds["input_ids"] if len(x) > 0]
    if "text" in ds.column_names:
        if tokenizer is None:
            raise SystemExit("a `text` column needs a tokenizer in --model_path")
        return [tokenizer(t, add_special_tokens=False)["input_ids"] for t in ds["text"] if t and t.strip()]
    raise SystemExit("the dataset needs an `input_ids` (tokenised) or `text` column; audio rows are tokenised outside")


def main(argv=None):
    cfg = parse_args(argv)
    why = refuse(cfg)
    if why:
        raise SystemExit(why)
    from transformers import TrainingArguments
    import speech_distill_amd as sda
    from speech_distill_amd.stage1 import Stage1Collator, freeze_model_weights, pack_bfd
    from speech_distill_amd.trainer import Stage1Trainer
    os.makedirs(cfg.output_dir, exist_ok=True)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if cfg.random_init:
        dims = sda.Qwen3Dims(1032, 128, 256, 2, 2, 1) if cfg.tiny else sda.Qwen3Dims.student_06b()
        model = sda.HipQwen3ForCausalLM(dims, device=dev, seed=cfg.seed)
    else:
        model = sda.HipQwen3ForCausalLM.from_pretrained(cfg.model_path, device=dev)
    tokenizer = None
    if cfg.model_path and any(os.path.exists(os.path.join(cfg.model_path, f))
                              for f in ("tokenizer.json", "tokenizer_config.json", "vocab.json")):
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(cfg.model_path)
        tokenizer.chat_template = None                        # stage1.py:123-127
        if tokenizer.pad_token is None:
            tokenizer.pad_token = tokenizer.eos_token
    V = model.dims.vocab_size
    num_new = cfg.num_new_tokens if cfg.num_new_tokens > 0 else 1000   # stage1.py:133-138
    if num_new > V:
        raise SystemExit(f"--num_new_tokens {num_new} > vocabulary {V}")
    print(f"\nFreezing model weights, keeping {num_new} new speech tokens unfrozen...")
    freeze_model_weights(model, num_new)
    model.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"recompute": cfg.recompute})
    docs = load_documents(cfg, V, tokenizer)
    if not docs:
        raise SystemExit("Train dataset is empty after processing!")
    bins = pack_bfd(docs, cfg.max_seq_length)
    print(f"{len(docs)} documents packed into {len(bins)} bins of {cfg.max_seq_length} tokens")
    n_eval = int(round(len(bins) * cfg.eval_size / (100.0 if cfg.eval_size >= 1 else 1.0))) if cfg.eval_size > 0 else 0
    train = [{"documents": b} for b in bins[:len(bins) - n_eval]]
    evals = [{"documents": b} for b in bins[len(bins) - n_eval:]] if n_eval else None
    pad = tokenizer.pad_token_id if tokenizer is not None and tokenizer.pad_token_id is not None else 0
    args = TrainingArguments(
        output_dir=cfg.output_dir, num_train_epochs=cfg.num_epochs, per_device_train_batch_size=cfg.batch_size,
        per_device_eval_batch_size=cfg.eval_batch_size, learning_rate=cfg.learning_rate, warmup_steps=cfg.warmup_steps,
        logging_steps=cfg.logging_steps, save_steps=cfg.save_steps, eval_steps=cfg.eval_steps if evals else None,
        eval_strategy="steps" if evals else "no", save_strategy="steps", load_best_model_at_end=evals is not None,
        gradient_accumulation_steps=cfg.gradient_accumulation_steps, gradient_checkpointing=True, bf16=True,
        optim="adamw_torch", weight_decay=cfg.weight_decay, seed=cfg.seed, dataloader_pin_memory=True,
        dataloader_num_workers=0, report_to=["wandb"] if cfg.use_wandb else [], remove_unused_columns=False,
        label_names=["labels"], max_steps=cfg.max_steps, prediction_loss_only=True)   # stage1.py:291-322
    trainer = Stage1Trainer(model=model, args=args, train_dataset=train, eval_dataset=evals,
                            data_collator=Stage1Collator(pad_token_id=pad, padding_free=cfg.padding_free))
    def body_checksum():  # every decoder weight + the final norm (untouched by Stage-1)
        return float(torch.cat([model.flat[a:b] for a, b in model.layer_ranges + [model.norm_range]]).double().sum())
    body0, lo = body_checksum(), model.stage1_row_lo
    old0 = float(model._params["model.embed_tokens.weight"][:lo].double().sum())
    t0 = time.time()
    trainer.train()
    final = os.path.join(cfg.output_dir, "final_model")     # stage1.py:330-332
    trainer.save_model(final)
    if tokenizer is not None:
        tokenizer.save_pretrained(final)
    print(f"\nTraining completed in {time.time() - t0:.1f}s; final model in {final}")
    if cfg.log_json:
        import json
        emb = model._params["model.embed_tokens.weight"]
        with open(cfg.log_json, "w") as f:
            json.dump({"log_history": trainer.state.log_history, "global_step": trainer.state.global_step,
                       "optimizer": type(getattr(trainer.optimizer, "optimizer", trainer.optimizer)).__name__, "stage1_row_lo": lo,
                       "trainable": sorted(n for n, q in model.named_parameters() if q.requires_grad),
                       "body_checksum_before": body0, "body_checksum": body_checksum(),
                       "old_rows_checksum_before": old0, "old_rows_checksum": float(emb[:lo].double().sum())}, f)


if __name__ == "__main__":
    main()
