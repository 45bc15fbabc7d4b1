"""Stage-1 alignment, CPU side (no GPU): the maths against fixture G6 (the reference's freeze_model_weights on HF Qwen3,
tests/golden/make_golden_stage1.py), scripts/stage1.py's flags against the reference's table (stage1.py:338-526),
best-fit-decreasing packing and the collator, and the Stage-1 host logic of HipQwen3ForCausalLM."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- G6 restated
def _stage1_restated(variant):
    """oracle.qwen3.forward + torch cross-entropy (HF ForCausalLMLoss: shift, ignore -100, sum / num_items_in_batch) with
    the gradient rows below old_vocab masked, HF clip 1.0, torch AdamW (lr 1e-3, wd 0.01) -- on G6's batches."""
    from oracle import qwen3 as Q
    z = load_golden("g6_stage1.npz")
    p = variant + "_"
    tied = variant == "tied"
    shp = Q.Qwen3Shape(*[int(x) for x in z[p + "shape"]], tie_word_embeddings=tied)
    w = {k: v.bfloat16().float() for k, v in Q.init_weights(shp, seed=int(z[p + "seed"])).items()}
    assert np.allclose([float(v.double().sum()) for _, v in sorted(w.items())], z[p + "checksum"])
    old = shp.vocab_size - int(z[p + "num_new_tokens"])
    names = ["model.embed_tokens.weight"] + ([] if tied else ["lm_head.weight"])
    train = [w[n].requires_grad_(True) for n in names]
    opt = torch.optim.AdamW(train, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    out = {"losses": [], "grads": [], "params": [], "old": old, "names": names, "z": z, "w": w}
    for step in range(2):
        n_items = int(z[p + f"step{step}_num_items"])
        for k in (2 * step, 2 * step + 1):
            ids, am, lab = (torch.from_numpy(z[p + f"mb{k}_{key}"]) for key in ("input_ids", "attention_mask", "labels"))
            logits = Q.forward(w, shp, ids, am)
            loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, shp.vocab_size), lab[:, 1:].reshape(-1),
                                                     ignore_index=-100, reduction="sum") / n_items
            loss.backward()
            out["losses"].append(float(loss.detach()))
        for t in train:
            t.grad[:old] = 0.0
        out["grads"].append([t.grad[old:].clone() for t in train])
        torch.nn.utils.clip_grad_norm_(train, 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        out["params"].append([t.detach()[old:].clone() for t in train])
    return out


@pytest.mark.parametrize("variant", ["tied", "untied"])
def test_restated_stage1_matches_reference_fixture(variant):
    r = _stage1_restated(variant)
    z, p = r["z"], variant + "_"
    assert sorted(r["names"]) == sorted(z[p + "trainable"].tolist())
    np.testing.assert_allclose(r["losses"], z[p + "losses"], rtol=2e-5)
    for step in range(2):
        for n, g, q in zip(r["names"], r["grads"][step], r["params"][step]):
            short = n.split(".")[-2]
            np.testing.assert_allclose(g.numpy(), z[p + f"step{step}_grad_{short}"], rtol=1e-4, atol=1e-7)
            np.testing.assert_allclose(q.numpy(), z[p + f"step{step}_param_{short}"], rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------------------------------------- CLI
REFERENCE_FLAGS = {  # stage1.py:338-526, flag -> default there (None: a path, required there)
    "--model_path": None, "--dataset_path": None, "--output_dir": None, "--num_epochs": 3, "--batch_size": 4,
    "--eval_batch_size": 8, "--learning_rate": 1e-4, "--warmup_steps": 1000, "--weight_decay": 0.01,
    "--gradient_accumulation_steps": 4, "--logging_steps": 50, "--save_steps": 500, "--eval_steps": 500, "--eval_size": 0,
    "--max_seq_length": 4096, "--num_workers": 4, "--num_new_tokens": 8220, "--prefix": "", "--text_bos": "<|text_start|>",
    "--text_eos": "<|text_end|>", "--text_prefix": '{"en": "", "zh": "", "yue": "<|Yue|>"}',
    "--speech_bos": "<|semantic_token_start|>", "--speech_eos": "<|semantic_token_end|>", "--gradient_checkpointing": True,
    "--use_8bit_optimizer": False, "--use_wandb": False, "--seed": 42,
}


def _cli():
    spec = importlib.util.spec_from_file_location("sd_stage1_cli", os.path.join(ROOT, "scripts", "stage1.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_reference_flag_parses_with_the_reference_default():
    mod = _cli()
    src = open(os.path.join(ROOT, "scripts", "stage1.py")).read()
    assert set(REFERENCE_FLAGS) <= set(re.findall(r'"(--[a-z_0-9]+)"', src))
    cfg = mod.parse_args(["--output_dir", "/o"])
    for flag, default in REFERENCE_FLAGS.items():
        if default is not None:
            assert getattr(cfg, flag[2:]) == default, flag


def test_reference_launch_line_parses_and_refusals_are_clear(monkeypatch):
    mod = _cli()
    cfg = mod.parse_args("--model_path /m --dataset_path /d --output_dir /o --num_new_tokens 8220 --batch_size 2 "
                         "--gradient_accumulation_steps 8 --max_seq_length 2048 --gradient_checkpointing".split())
    assert cfg.num_new_tokens == 8220 and cfg.batch_size == 2 and cfg.max_seq_length == 2048
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert mod.refuse(cfg) is None
    assert "8-bit" in mod.refuse(mod.parse_args("--model_path /m --dataset_path /d --output_dir /o --use_8bit_optimizer".split()))
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "one GPU" in mod.refuse(cfg)


# ---------------------------------------------------------------------------------------------- packing, collator
def _docs(n=200, seed=0, hi=700):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 1000, (int(torch.randint(1, hi, (1,), generator=g)),), generator=g).tolist() for _ in range(n)]


def test_bfd_packs_every_document_once_within_capacity():
    from speech_distill_amd.stage1 import pack_bfd
    docs = _docs()
    bins = pack_bfd(docs, 512)
    assert all(sum(len(d) for d in b) <= 512 for b in bins)
    packed = sorted(tuple(d) for b in bins for d in b)
    assert packed == sorted(tuple(d[:512]) for d in docs)       # every document exactly once, long ones truncated
    assert any(len(d) > 512 for d in docs) and max(len(d) for b in bins for d in b) == 512
    assert pack_bfd(docs, 512) == bins                          # deterministic
    # best fit decreasing never needs more bins than first-fit decreasing on the same lengths
    lens = sorted((min(len(d), 512) for d in docs), reverse=True)
    ffd = []
    for n in lens:
        for i, room in enumerate(ffd):
            if room >= n:
                ffd[i] -= n
                break
        else:
            ffd.append(512 - n)
    assert len(bins) <= len(ffd)


def test_bfd_best_fit_choice():
    from speech_distill_amd.stage1 import pack_bfd
    # 6 -> bin A (room 4), 5 -> bin B (room 5), 4 -> best fit is A (room 4 exactly), 3 -> B
    assert pack_bfd([[1] * 4, [2] * 6, [3] * 3, [4] * 5], 10) == [[[2] * 6, [1] * 4], [[4] * 5, [3] * 3]]


def test_collator_rows_labels_and_padding():
    from speech_distill_amd.stage1 import Stage1Collator
    b = Stage1Collator(pad_token_id=7)([{"documents": [[1, 2, 3], [4, 5]]}, {"documents": [[6, 8, 9, 10]]}])
    assert b["input_ids"].tolist() == [[1, 2, 3, 7], [4, 5, 7, 7], [6, 8, 9, 10]]
    assert b["attention_mask"].tolist() == [[1, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 1]]
    assert b["labels"].tolist() == [[-100, 2, 3, -100], [-100, 5, -100, -100], [-100, 8, 9, 10]]
    b8 = Stage1Collator(pad_token_id=0, pad_to_multiple_of=8)([{"input_ids": [1, 2, 3]}])
    assert b8["input_ids"].shape == (1, 8) and b8["labels"][0, 3:].eq(-100).all()


# ---------------------------------------------------------------------------------------------- host logic
def _cpu_model(tied=True):
    import speech_distill_amd as sda
    return sda.HipQwen3ForCausalLM(sda.Qwen3Dims(520, 128, 192, 2, 4, 2, tie_word_embeddings=tied), device="cpu", init_std=0)


@pytest.mark.parametrize("tied", [True, False])
def test_freeze_sets_flags_segments_and_row_lo(tied, capsys):
    from speech_distill_amd.stage1 import freeze_model_weights
    m = _cpu_model(tied)
    assm = m.optim_segments()
    assert len(assm) == 1 and assm[0][1].numel() == m.numel_flat   # full training: the whole flat buffer
    m.flat_grad = torch.ones_like(m.flat)
    freeze_model_weights(m, 68)
    assert "Old tokens (452) will not receive gradient updates." in capsys.readouterr().out
    assert m.stage1_row_lo == 452
    want = {"model.embed_tokens.weight"} | (set() if tied else {"lm_head.weight"})
    assert {n for n, p in m.named_parameters() if p.requires_grad} == want
    segs = m.optim_segments()
    assert [s[0] for s in segs] == ["bf16"] * len(want) and all(s[3] for s in segs)   # decayed, as HF's groups do
    assert sum(s[1].numel() for s in segs) == 520 * 128 * len(want)
    assert segs[0][1].data_ptr() == m._params["model.embed_tokens.weight"].data_ptr()
    for name in want:
        o, n, shape = m._slices[name]
        g = m.flat_grad[o:o + n].view(shape)
        assert g[:452].eq(0).all() and g[452:].eq(1).all()         # old rows zeroed once, new rows left alone
    m.check_stage1()
    m.model.layers[0].mlp.down_proj.weight.requires_grad_(True)
    with pytest.raises(ValueError, match="body parameters are trainable"):
        m.check_stage1()


def test_without_stage1_labels_stay_ignored_and_segments_unchanged():
    m = _cpu_model()
    assert m.stage1_row_lo is None
    assert len(m.optim_segments(split_decay=True)) == len(m._decay_runs())
