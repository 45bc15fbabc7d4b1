"""Padding-free packed distillation, the host side (CPU only): the collator's packed format against the padded collator
and ``Stage1Collator._flatten``, the token-budget bins against ``stage1.pack_bfd``, the rule of ``ops.packed_rows`` on
hand-written cases, the command line, and the trainer's refusals and teacher routing with stand-in models."""
import importlib.util
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import load_golden
from oracle import distill_loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, BOS = 9, 5
PACKED = ("position_ids", "cu_seq_lens_q", "cu_seq_lens_k", "max_length_q", "max_length_k")


class _Tok:
    pad_token = "<|semantic_token_end|>"

    def __init__(self, pad, bos):
        self.pad_token_id, self.bos = pad, bos

    def encode(self, text, add_special_tokens=False):
        return [self.bos]


def _collators(pad=PAD, bos=BOS):
    from speech_distill_amd.collator import ProcessedDataCollator
    return (ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad),
            ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad, padding_free=True))


def _feat(ids, teacher=None, K=0, topk_len=None):
    f = {"student_input_ids": list(ids), "student_attention_mask": [1] * len(ids),
         "teacher_input_ids": list(ids if teacher is None else teacher),
         "teacher_attention_mask": [1] * len(ids if teacher is None else teacher)}
    if K:
        n = len(ids) if topk_len is None else topk_len
        g = torch.Generator().manual_seed(len(ids) * 7 + n)
        f["teacher_top_k_v"] = -torch.rand(n, K, generator=g).half() - 0.5
        f["teacher_top_k_i"] = torch.randint(1, 30, (n, K), generator=g).int()
    return f


def _c1_feats():
    z = load_golden("g4_step_c1.npz")
    V, bos, pad = [int(x) for x in z["meta"]]
    return [_feat(z[f"in_{r}_ids"].tolist()) for r in range(int(z["n"]))], pad, bos


def _check_packed_against_padded(feats, pad, bos):
    """Every document's cells equal the padded collator's valid cells of that sample (first label -100), and the packed
    keys are those of Stage1Collator._flatten for the same lengths."""
    from speech_distill_amd.stage1 import Stage1Collator
    padded_c, packed_c = _collators(pad, bos)
    packed = packed_c([dict(f) for f in feats])
    kept = [f for f in feats if len(f["student_input_ids"]) > 0]
    padded = padded_c([dict(f) for f in kept])
    lens = [len(f["student_input_ids"]) for f in kept]
    M = sum(lens)
    assert "attention_mask" not in packed and "teacher_attention_mask" not in packed
    assert packed["input_ids"].shape == packed["labels"].shape == packed["teacher_input_ids"].shape == (1, M)
    cu = packed["cu_seq_lens_q"].tolist()
    assert cu == np.concatenate([[0], np.cumsum(lens)]).tolist()
    for i, n in enumerate(lens):
        a, b = cu[i], cu[i + 1]
        assert torch.equal(packed["input_ids"][0, a:b], padded["input_ids"][i, :n])
        assert torch.equal(packed["teacher_input_ids"][0, a:b], padded["teacher_input_ids"][i, :n])
        want = padded["labels"][i, :n].clone()
        want[0] = -100
        assert torch.equal(packed["labels"][0, a:b], want), i
        assert int(packed["labels"][0, a]) == -100
    flat = Stage1Collator._flatten([list(f["student_input_ids"]) for f in kept])
    for k in PACKED:
        if torch.is_tensor(flat[k]):
            assert packed[k].dtype == flat[k].dtype and torch.equal(packed[k], flat[k]), k
        else:
            assert type(packed[k]) is int and packed[k] == flat[k], k
    assert torch.equal(packed["input_ids"], flat["input_ids"]) and packed["labels"].dtype == torch.long
    assert packed["cu_seq_lens_k"] is not packed["cu_seq_lens_q"]
    return packed


# ------------------------------------------------------------------------------------------------------ collator
def test_collator_packs_the_c1_samples_like_the_padded_collator_per_document():
    feats, pad, bos = _c1_feats()
    assert [len(f["student_input_ids"]) for f in feats] == [96, 118, 116, 126, 64, 81, 126, 102]
    packed = _check_packed_against_padded(feats, pad, bos)
    assert packed["max_length_q"] == 126 and packed["input_ids"].shape == (1, 829)
    assert int((packed["labels"] != -100).sum()) > 0


@pytest.mark.parametrize("case", ["one_sample", "length_one", "no_bos_in_second", "pad_mid_sequence", "zero_length_dropped"])
def test_collator_hand_cases(case):
    feats = {
        "one_sample": [_feat([1, 2, BOS, 11, 12, PAD])],
        "length_one": [_feat([1, BOS, 11, PAD]), _feat([BOS]), _feat([2, BOS, 13, 14, PAD])],
        # the second sample has no speech_bos: none of its cells has a target, although the first sample's count is > 0
        "no_bos_in_second": [_feat([1, BOS, 11, 12, PAD]), _feat([3, 4, 11, 12, PAD]), _feat([BOS, 15, PAD])],
        # quirk Q2: no target on ANY cell holding the pad id, mid-sequence too
        "pad_mid_sequence": [_feat([1, BOS, 11, PAD, 12, PAD]), _feat([2, BOS, PAD, 13])],
        "zero_length_dropped": [_feat([1, BOS, 11, PAD]), _feat([]), _feat([BOS, 12, PAD])],
    }[case]
    packed = _check_packed_against_padded(feats, PAD, BOS)
    if case == "no_bos_in_second":
        assert bool((packed["labels"][0, 5:10] == -100).all()) and int(packed["labels"][0, 11]) == 15
    if case == "pad_mid_sequence":
        assert packed["labels"][0].tolist() == [-100, BOS, 11, -100, 12, -100, -100, BOS, -100, 13]
    if case == "zero_length_dropped":
        assert packed["cu_seq_lens_q"].tolist() == [0, 4, 7]


def test_collator_topk_blocks_are_cut_or_padded_per_sample():
    K = 3
    feats = [_feat([1, BOS, 11, 12, PAD], K=K), _feat([2, BOS, 13, PAD], K=K, topk_len=6),      # cut to 4
             _feat([BOS, 14, 15, 16, 17, PAD], K=K, topk_len=2)]                                # padded to 6
    _, packed_c = _collators()
    packed = packed_c([dict(f) for f in feats])
    assert packed["teacher_top_k_v"].shape == packed["teacher_top_k_i"].shape == (1, 15, K)
    assert packed["teacher_top_k_v"].dtype == torch.float16 and packed["teacher_top_k_i"].dtype == torch.int32
    v, i = packed["teacher_top_k_v"][0], packed["teacher_top_k_i"][0]
    assert torch.equal(v[0:5], feats[0]["teacher_top_k_v"]) and torch.equal(i[0:5], feats[0]["teacher_top_k_i"])
    assert torch.equal(v[5:9], feats[1]["teacher_top_k_v"][:4]) and torch.equal(i[5:9], feats[1]["teacher_top_k_i"][:4])
    assert torch.equal(v[9:11], feats[2]["teacher_top_k_v"]) and torch.equal(i[9:11], feats[2]["teacher_top_k_i"])
    assert bool((v[11:15] == 0).all()) and bool((i[11:15] == 0).all())
    # per row this is the padded collator's rule with the sample's own length as the width
    padded_c, _ = _collators()
    for f, (a, b) in zip(feats, [(0, 5), (5, 9), (9, 15)]):
        one = padded_c([dict(f)])
        assert torch.equal(one["teacher_top_k_v"][0], v[a:b]) and torch.equal(one["teacher_top_k_i"][0], i[a:b])


def test_collator_refusals_and_unchanged_default():
    from speech_distill_amd.collator import ProcessedDataCollator
    _, packed_c = _collators()
    with pytest.raises(ValueError, match="pad_to_multiple_of"):
        ProcessedDataCollator(_Tok(PAD, BOS), pad_token_id=PAD, pad_to_multiple_of=8, padding_free=True)
    with pytest.raises(ValueError, match="empty batch"):
        packed_c([_feat([]), _feat([])])
    with pytest.raises(ValueError, match="sample 1"):
        packed_c([_feat([1, BOS, 11, PAD]), _feat([2, BOS, 12, PAD], teacher=[2, BOS, 12])])
    # the default output is what a collator built without the keyword gives, key by key
    feats, pad, bos = _c1_feats()
    feats = [dict(f, **{k: v for k, v in _feat(f["student_input_ids"], K=2).items() if k.startswith("teacher_top")})
             for f in feats[:3]]
    for mult in (None, 16):
        a = ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad, pad_to_multiple_of=mult)([dict(f) for f in feats])
        b = ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad, pad_to_multiple_of=mult,
                                  padding_free=False)([dict(f) for f in feats])
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------ bins
@pytest.mark.parametrize("seed,n,lo,hi,budget", [(0, 40, 1, 300, 512), (1, 97, 0, 64, 64), (2, 200, 16, 512, 2048),
                                                 (3, 7, 5, 6, 17)])
def test_pack_bfd_indices_gives_the_bins_of_stage1_pack_bfd(seed, n, lo, hi, budget):
    from speech_distill_amd.packing import pack_bfd_indices
    from speech_distill_amd.stage1 import pack_bfd
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(lo, hi + 1, (n,), generator=g).tolist()
    seqs = [[1000 * j + t for t in range(m)] for j, m in enumerate(lengths)]   # a document names its sample
    bins = pack_bfd_indices(lengths, budget)
    assert [[seqs[j] for j in b] for b in bins] == pack_bfd(seqs, budget)
    assert sorted(j for b in bins for j in b) == [j for j, m in enumerate(lengths) if m > 0]
    assert all(sum(lengths[j] for j in b) <= budget for b in bins)


def test_pack_bfd_indices_refuses_an_overlong_sample_and_packed_view_keeps_the_order():
    from speech_distill_amd.packing import PackedView, pack_bfd_indices
    with pytest.raises(ValueError, match="sample 2"):
        pack_bfd_indices([4, 8, 9], 8)
    with pytest.raises(ValueError):
        pack_bfd_indices([4], 0)
    data = [_feat([10 + j, BOS] + [11 + j] * j + [PAD]) for j in range(6)]     # lengths 3..8
    bins = pack_bfd_indices([len(d["student_input_ids"]) for d in data], 12)
    assert bins == [[5, 1], [4, 2], [3, 0]]
    view = PackedView(data, bins)
    assert len(view) == 3 and [s["student_input_ids"] for s in view[1]["samples"]] == [data[4]["student_input_ids"],
                                                                                      data[2]["student_input_ids"]]
    _, packed_c = _collators()
    batch = packed_c([view[0], view[2]])     # two bins in one batch: bins in batch order, samples in bin order
    order = [5, 1, 3, 0]
    assert batch["input_ids"][0].tolist() == [t for j in order for t in data[j]["student_input_ids"]]
    assert batch["cu_seq_lens_q"].tolist() == np.concatenate([[0], np.cumsum([8, 4, 6, 3])]).tolist()
    assert torch.equal(batch["input_ids"], packed_c([data[j] for j in order])["input_ids"])


# ------------------------------------------------------------------------------------------------------ the rule
def test_packed_rows_rule_on_hand_written_cases():
    from speech_distill_amd import ops
    #            doc 0: 0..3         doc 1: 4..5   doc 2: 6..9
    labels = torch.tensor([[-100, 7, 8, -100, 21, 22, -100, -100, 31, 32]])
    cu = torch.tensor([0, 4, 6, 10], dtype=torch.int32)
    pos = torch.tensor([[0, 1, 2, 3, 0, 1, 0, 1, 2, 3]])
    rows, lab, longest, max_pos = ops.packed_rows(labels, cu, position_ids=pos)
    # token 3 is the last of doc 0: it does not predict label 21 of doc 1's first token (loss_rows on the flat row does)
    assert rows.tolist() == [0, 1, 4, 7, 8] and lab.tolist() == [7, 8, 22, 31, 32] and (longest, max_pos) == (4, 3)
    assert ops.loss_rows(labels)[0].tolist() == [0, 1, 3, 4, 7, 8]
    # speech mask: the NEXT token's bit decides
    sm = torch.tensor([[1, 1, 0, 1, 1, 1, 1, 1, 1, 0]])
    rows, lab, _, _ = ops.packed_rows(labels, cu, speech_mask=sm)
    assert rows.tolist() == [0, 4, 7] and lab.tolist() == [7, 22, 31]
    # empty documents (also first and last), and no position_ids -> largest position 0
    cu_e = torch.tensor([0, 0, 4, 4, 6, 10, 10], dtype=torch.int64)
    rows, lab, longest, max_pos = ops.packed_rows(labels, cu_e)
    assert rows.tolist() == [0, 1, 4, 7, 8] and (longest, max_pos) == (4, 0)
    # one document = loss_rows; documents of one token select nothing; all -100 selects nothing
    assert ops.packed_rows(labels, torch.tensor([0, 10], dtype=torch.int32))[0].tolist() == [0, 1, 3, 4, 7, 8]
    assert ops.packed_rows(torch.tensor([[3, 4, 5]]), torch.tensor([0, 1, 2, 3], dtype=torch.int32))[0].numel() == 0
    r0 = ops.packed_rows(torch.full((1, 10), -100), cu)
    assert r0[0].numel() == 0 and r0[1].numel() == 0 and r0[0].dtype == torch.int64
    # refusals
    for bad in ([1, 4, 6, 10], [0, 4, 6, 9], [0, 6, 4, 10]):
        with pytest.raises(ValueError, match="cu_seqlens"):
            ops.packed_rows(labels, torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(ValueError, match="non-negative"):
        ops.packed_rows(labels, cu, position_ids=pos - 1)
    with pytest.raises(ValueError):
        ops.packed_rows(labels, cu, position_ids=pos[:, :9])


# ------------------------------------------------------------------------------------------------------ CLI
def _cli():
    spec = importlib.util.spec_from_file_location("sd_train_cli_packed", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_packing_flags():
    mod = _cli()
    cfg = mod.parse_args([])
    assert cfg.padding_free is False and cfg.pack_tokens == 0 and mod.distill_kwargs(cfg) == {}
    assert mod.parse_args(["--padding_free"]).padding_free is True
    cfg = mod.parse_args(["--pack_tokens", "2048"])
    assert cfg.pack_tokens == 2048 and cfg.padding_free is True
    for extra in (["--padding_free"], ["--pack_tokens", "256"]):
        cfg = mod.parse_args(["--lmbda", "0.5", "--top_k", "0"] + extra)
        with pytest.raises(SystemExit, match=r"--lmbda.*--padding_free"):
            mod.distill_kwargs(cfg)


# ------------------------------------------------------------------------------------------------------ trainer
class TinyLM(nn.Module):
    """Position-free stand-in: records the keywords of every call."""

    def __init__(self, V=32, h=8):
        super().__init__()
        self.emb = nn.Embedding(V, h)
        self.out = nn.Linear(h, V, bias=False)
        self.seen = []

    def forward(self, input_ids=None, attention_mask=None, labels=None, **kw):
        self.seen.append(dict(kw, input_ids=input_ids, attention_mask=attention_mask))
        return type("O", (dict,), {"logits": property(lambda s: s["logits"])})(logits=self.out(self.emb(input_ids)))


class OracleLoss(nn.Module):
    def forward(self, student_logits, labels, teacher_logits=None, teacher_top_k_v=None, teacher_top_k_i=None,
                speech_token_mask=None):
        self.labels = labels.clone()
        return L.distill_loss(student_logits, labels, teacher_logits, teacher_top_k_v, teacher_top_k_i, speech_token_mask,
                              2.0, 0.5, acc=torch.float32)


def _make(**kw):
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    torch.manual_seed(0)
    student, teacher = TinyLM(), TinyLM()
    args = TrainingArguments(output_dir=tempfile.mkdtemp(), use_cpu=True, report_to=[], logging_steps=1,
                             remove_unused_columns=False, label_names=["labels"], save_strategy="no")
    tr = DistillationTrainer(model=student, args=args, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=4, **kw)
    tr.distill_loss_fn = OracleLoss()
    tr._extract_topk = lambda logits, k, V: L.extract_topk(logits, k, V)
    tr.log = lambda d, *a, **k: None
    return tr, student, teacher


def _packed_batch():
    feats = [_feat([1, BOS, 11, 12, PAD]), _feat([2, 3, BOS, 13, PAD]), _feat([BOS, 14, 15, 16])]
    return _collators()[1]([dict(f) for f in feats]), feats


def test_trainer_hands_the_teacher_the_packed_keys():
    """The silent-wrong-answer hole: a packed batch must reach the teacher with its position_ids and segments, not as
    one long document; and the loss never lets a document's last token predict the next document's first."""
    tr, student, teacher = _make()
    batch, feats = _packed_batch()
    tids = batch["teacher_input_ids"].clone()
    tids[0, 0] = 30      # (a teacher prefix differs from the student's: the teacher must get ITS ids)
    batch["teacher_input_ids"] = tids
    want_labels = batch["labels"].clone()
    batch["labels"] = batch["labels"].clone()
    batch["labels"][0, 5] = 2     # tampered: a real label at a document start
    student.train()
    loss = tr.compute_loss(student, dict(batch))
    assert len(teacher.seen) == 1 and len(student.seen) == 1
    for model, ids in ((teacher, tids), (student, batch["input_ids"])):
        got = model.seen[0]
        assert got["attention_mask"] is None and torch.equal(got["input_ids"], ids)
        for k in PACKED:
            assert k in got, k
            assert torch.equal(got[k], batch[k]) if torch.is_tensor(batch[k]) else got[k] == batch[k]
    assert torch.equal(tr.distill_loss_fn.labels, want_labels)      # the document start is masked again before the loss
    assert tr.tokens_seen == batch["input_ids"].numel() == 14
    clean = tr.compute_loss(student, dict(batch, labels=want_labels))
    assert float(loss.detach()) == float(clean.detach()) and np.isfinite(float(loss.detach()))
    # without teacher ids the teacher takes the student's inputs, packed keys included
    teacher.seen.clear()
    tr.compute_loss(student, {k: v for k, v in batch.items() if k != "teacher_input_ids"})
    assert all(k in teacher.seen[0] for k in PACKED) and "labels" not in teacher.seen[0]
    # segments by position_ids alone (no flash-attn keys): same loss, same masking
    bare = {k: v for k, v in batch.items() if k not in PACKED[1:]}
    assert float(tr.compute_loss(student, bare).detach()) == float(clean.detach())
    assert torch.equal(tr.distill_loss_fn.labels, want_labels)


def test_trainer_packed_refusals():
    batch, _ = _packed_batch()
    tr, student, teacher = _make()
    with pytest.raises(ValueError, match="attention_mask"):
        tr.compute_loss(student, dict(batch, attention_mask=torch.ones_like(batch["input_ids"])))
    with pytest.raises(ValueError, match="position-aligned"):
        tr.compute_loss(student, dict(batch, teacher_input_ids=batch["teacher_input_ids"][:, :-1]))
    with pytest.raises(ValueError, match="position-aligned"):   # also with pre-extracted top-K, where no teacher runs
        tr.compute_loss(student, dict(batch, teacher_input_ids=batch["teacher_input_ids"][:, :-1],
                                      teacher_top_k_v=torch.zeros(1, 14, 4).half(),
                                      teacher_top_k_i=torch.zeros(1, 14, 4).int()))
    with pytest.raises(ValueError, match="cu_seqlens"):
        tr.compute_loss(student, dict(batch, cu_seq_lens_q=torch.tensor([0, 5, 10, 13], dtype=torch.int32)))
    assert not student.seen and not teacher.seen                 # refused before any model ran
    tr.lmbda = 0.5       # (the constructor's lmbda > 0 wants a HipQwen3ForCausalLM on the GPU; the refusal is compute_loss's)
    with pytest.raises(ValueError, match="lmbda"):
        tr.compute_loss(student, dict(batch))
    with pytest.raises(ValueError, match="lmbda"):
        tr.training_step(student, dict(batch))
    assert not student.seen and not teacher.seen
