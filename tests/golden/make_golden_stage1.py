#!/usr/bin/env python3
"""Generate ``g6_stage1.npz`` (Stage-1 alignment) FROM THE REFERENCE ITSELF.

Run once in the build container (``python tests/golden/make_golden_stage1.py``); the output is committed, the reference's
code is not.  It imports the reference's ``freeze_model_weights`` (/root/reference/stage1.py; trl / s3tokenizer /
torchaudio / peft stubbed: absent here and unused by that function) and applies it to an fp32 HF ``Qwen3ForCausalLM``
of the G5 shape, in a tied and an untied variant, with ``V - num_new_tokens == 4 (mod 8)``.  Then two optimizer steps
of what SFTTrainer runs (stage1.py:285-335): gradient accumulation 2, ``model(..., labels=, num_items_in_batch=)``
(HF ForCausalLMLoss), HF's clip (max_grad_norm 1.0) and ``torch.optim.AdamW`` over HF's decay groups (lr 1e-3,
weight decay 0.01, constant schedule).  Batches: right-padded documents of unequal length, labels as
speech_distill_amd.stage1.Stage1Collator builds them.

Recorded per variant ``{tied,untied}``: the weights' seed and a checksum, the micro-batches, every micro-batch loss, the
masked gradients and the parameters of the new rows after each step (the old rows only ever see the decay
p *= 1 - lr * wd, restated by the tests).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from transformers import Qwen3Config, Qwen3ForCausalLM  # noqa: E402

for name in ("s3tokenizer", "torchaudio", "peft", "trl"):
    if name not in sys.modules:
        m = types.ModuleType(name)
        if name == "peft":
            m.LoraConfig = object
            m.get_peft_model = lambda *a, **k: None
        if name == "trl":
            m.SFTTrainer = m.SFTConfig = object
        sys.modules[name] = m
sys.path.insert(0, "/root/reference")
from stage1 import freeze_model_weights as ref_freeze  # noqa: E402

from oracle import qwen3 as OQ  # noqa: E402
from speech_distill_amd.stage1 import Stage1Collator  # noqa: E402  (host-only module)

SHAPE = (520, 128, 192, 2, 4, 2)
NUM_NEW = 68            # old_vocab = 452 = 4 (mod 8)
LR, WD, CLIP, GA, STEPS = 1e-3, 0.01, 1.0, 2, 2
SEED = 6


def batches(V, old_vocab):
    """GA * STEPS micro-batches of 3 right-padded documents of unequal length, half their tokens from the new rows."""
    g = torch.Generator().manual_seed(60)
    out = []
    for _ in range(GA * STEPS):
        docs = []
        for n in (int(torch.randint(20, 48, (1,), generator=g)), int(torch.randint(8, 20, (1,), generator=g)),
                  int(torch.randint(30, 48, (1,), generator=g))):
            old = torch.randint(0, old_vocab, (n,), generator=g)
            new = torch.randint(old_vocab, V, (n,), generator=g)
            pick = torch.rand(n, generator=g) < 0.5
            docs.append(torch.where(pick, new, old).tolist())
        out.append(Stage1Collator(pad_token_id=0)([{"documents": docs}]))
    return out


def run(tied):
    shp = OQ.Qwen3Shape(*SHAPE, tie_word_embeddings=tied)
    w = {k: v.bfloat16().float() for k, v in OQ.init_weights(shp, seed=SEED).items()}
    cfg = Qwen3Config(vocab_size=shp.vocab_size, hidden_size=shp.hidden_size, intermediate_size=shp.intermediate_size,
                      num_hidden_layers=shp.num_hidden_layers, num_attention_heads=shp.num_attention_heads,
                      num_key_value_heads=shp.num_key_value_heads, head_dim=128, rms_norm_eps=shp.rms_norm_eps,
                      rope_theta=shp.rope_theta, tie_word_embeddings=tied, attention_bias=False,
                      max_position_embeddings=4096, attn_implementation="eager", use_cache=False)
    model = Qwen3ForCausalLM(cfg).float()
    sd = dict(w)
    if tied:
        sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    model.load_state_dict(sd, strict=False)
    if tied:
        model.tie_weights()
    ref_freeze(model, NUM_NEW)
    V, old_vocab = shp.vocab_size, shp.vocab_size - NUM_NEW
    trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    # HF Trainer.get_decay_parameter_names: every weight except norms / biases -> the embedding (and lm_head) decay
    opt = torch.optim.AdamW([{"params": [p for _, p in trainable], "weight_decay": WD}], lr=LR, betas=(0.9, 0.999),
                            eps=1e-8, weight_decay=WD)
    mbs = batches(V, old_vocab)
    rec = {"seed": np.array(SEED), "shape": np.array(SHAPE), "num_new_tokens": np.array(NUM_NEW),
           "checksum": np.array([float(v.double().sum()) for _, v in sorted(w.items())])}
    losses = []
    for step in range(STEPS):
        window = mbs[step * GA:(step + 1) * GA]
        n_items = sum(int(b["labels"][:, 1:].ne(-100).sum()) for b in window)
        for i, b in enumerate(window):
            out = model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"],
                        num_items_in_batch=torch.tensor(n_items))
            out.loss.backward()
            losses.append(float(out.loss))
            k = step * GA + i
            for key in ("input_ids", "attention_mask", "labels"):
                rec[f"mb{k}_{key}"] = b[key].numpy()
        rec[f"step{step}_num_items"] = np.array(n_items)
        for n, p in trainable:
            short = n.split(".")[-2]
            g = p.grad
            assert float(g[:old_vocab].abs().max()) == 0.0
            rec[f"step{step}_grad_{short}"] = g[old_vocab:].numpy().copy()
        rec[f"step{step}_gnorm"] = np.array(float(torch.nn.utils.clip_grad_norm_([p for _, p in trainable], CLIP)))
        opt.step()
        opt.zero_grad(set_to_none=True)
        for n, p in trainable:
            rec[f"step{step}_param_{n.split('.')[-2]}"] = p.detach()[old_vocab:].numpy().copy()
    rec["losses"] = np.array(losses)
    rec["trainable"] = np.array(sorted(n for n, _ in trainable))
    return rec


def main():
    torch.manual_seed(0)
    out = {}
    for tied in (True, False):
        for k, v in run(tied).items():
            out[("tied_" if tied else "untied_") + k] = v
    path = os.path.join(HERE, "g6_stage1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
