"""-m gpu: padding-free packed distillation -- the row-selection kernel for packed documents (sd_packed_rows) against the
rule stated in torch, the packed trainer step against the reference's own fixture (the bounds of the padded layout),
``packed_batch=`` against the model's own host read, pre-extracted top-K on packed rows, the full [1, M, V] path, a real
``Trainer.train()`` with and without the lookaheads, and the command line."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import assert_grad_budget, dev, record, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL = 16, -7777


@pytest.fixture(scope="module")
def sda():
    import speech_distill_amd as m
    m.load_lib()
    return m


# ------------------------------------------------------------------------------------------------ sd_packed_rows
def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)


def _raw(labels, cu, sm=None, pos=None):
    """sd_packed_rows into buffers of M entries followed by a sentinel guard -> (rows, row_labels, meta) on the host."""
    from speech_distill_amd._lib import check, load_lib
    from speech_distill_amd.ops import _p, _stream
    M = labels.numel()
    lab, cu_d = to_dev(labels.reshape(-1)), to_dev(cu)
    sm_d, pos_d = (None if sm is None else to_dev(sm.reshape(-1))), (None if pos is None else to_dev(pos.reshape(-1)))
    rows = torch.full((M + GUARD,), SENTINEL, dtype=torch.int64, device=dev())
    row_labels = torch.full((M + GUARD,), SENTINEL, dtype=torch.int64, device=dev())
    meta = torch.full((4 + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    check(load_lib().sd_packed_rows(lab.data_ptr(), _p(sm_d), cu_d.data_ptr(), cu.numel() - 1, _p(pos_d), rows.data_ptr(),
                                    row_labels.data_ptr(), meta.data_ptr(), M, _stream()), "sd_packed_rows")
    torch.cuda.synchronize()
    return rows.cpu(), row_labels.cpu(), meta.cpu()


def _positions(cu, M):
    c = cu.tolist()
    return torch.cat([torch.arange(b - a) for a, b in zip(c[:-1], c[1:])] + [torch.zeros(0, dtype=torch.long)])[None][:, :M]


def _labels(M, seed, keep=0.7):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, 1000, (1, M), generator=g)
    lab[torch.rand(1, M, generator=g) > keep] = -100
    return lab


CASES = {"one": [0, 1], "ones": _cu((1, 1, 1)).tolist(), "small": _cu((5, 17, 1, 9)).tolist(),
         "chunk_edge_a": _cu((1023, 1, 1024, 1)).tolist(), "chunk_edge_b": _cu((1024, 1025)).tolist(),
         "empty_docs": [0, 0, 5, 5, 12]}


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_packed_rows_kernel_equals_the_rule(sda, case, masked):
    """Integers compared exactly against the torch statement of the rule (``ops.packed_rows`` on CPU tensors), the longest
    document and the largest position included; entries past the row count and the guards behind the M-entry buffers are
    untouched; all labels -100 selects nothing."""
    from speech_distill_amd import ops
    cu = torch.tensor(CASES[case], dtype=torch.int32)
    M = int(cu[-1])
    pos = _positions(cu, M)
    for seed, lab in ((1, _labels(M, 11)), (2, _labels(M, 12, keep=1.0)), (3, torch.full((1, M), -100))):
        sm = (torch.rand(1, M, generator=torch.Generator().manual_seed(seed)) > 0.3).long() if masked else None
        want_r, want_l, want_longest, want_pos = ops.packed_rows(lab, cu, sm, pos)
        rows, row_labels, meta = _raw(lab, cu, sm, pos)
        n = int(meta[0])
        assert n == want_r.numel() and meta[:4].tolist() == [n, 0, want_longest, want_pos], (meta[:4].tolist(), want_longest)
        assert torch.equal(rows[:n], want_r) and torch.equal(row_labels[:n], want_l)
        assert bool((rows[n:] == SENTINEL).all()) and bool((row_labels[n:] == SENTINEL).all())
        assert bool((meta[4:] == SENTINEL).all())
        if seed == 3:
            assert n == 0
        got = ops.packed_rows(to_dev(lab), to_dev(cu), None if sm is None else to_dev(sm), to_dev(pos))
        assert torch.equal(got[0].cpu(), want_r) and torch.equal(got[1].cpu(), want_l) and got[2:] == (want_longest, want_pos)
        # without position_ids: same rows, largest position 0
        assert _raw(lab, cu, sm)[2][:4].tolist() == [n, 0, want_longest, 0]


def test_packed_rows_do_not_cross_a_document_boundary(sda):
    """A label that is not -100 at a document start: ``loss_rows`` on the same flat row selects the previous document's
    last token (the case is real), ``packed_rows`` does not."""
    from speech_distill_amd import ops
    cu = _cu((5, 17, 1, 9))
    lab = _labels(32, 5, keep=1.0)
    flat_rows = ops.loss_rows(to_dev(lab))[0].cpu().tolist()
    rows = ops.packed_rows(to_dev(lab), to_dev(cu))[0].cpu().tolist()
    ends = [4, 21, 22]      # last tokens of documents 0..2 (31 is the row's last token: no successor at all)
    assert all(e in flat_rows for e in ends) and not any(e in rows for e in ends)
    assert rows == [m for m in range(31) if m not in ends]


@pytest.mark.parametrize("cu", [[2, 5, 22, 23, 32], [0, 5, 22, 23, 30], [0, 22, 5, 23, 32]])
def test_packed_rows_refuses_malformed_segments_inside_its_bounds(sda, cu):
    """First not 0, last not M, one decrease: error bit 0, a ValueError from the wrapper, and nothing written outside the
    M-entry buffers (what is written inside them is unspecified)."""
    from speech_distill_amd import ops
    cu = torch.tensor(cu, dtype=torch.int32)
    lab = _labels(32, 6)
    rows, row_labels, meta = _raw(lab, cu, None, _positions(_cu((5, 17, 1, 9)), 32))
    assert int(meta[1]) & 1 and 0 <= int(meta[0]) <= 32
    assert bool((rows[32:] == SENTINEL).all()) and bool((row_labels[32:] == SENTINEL).all()) and bool((meta[4:] == SENTINEL).all())
    with pytest.raises(ValueError, match="cu_seqlens"):
        ops.packed_rows(to_dev(lab), to_dev(cu))


def test_packed_rows_argument_errors(sda):
    from speech_distill_amd import ops
    from speech_distill_amd._lib import load_lib
    lab, cu = to_dev(_labels(8, 1).reshape(-1)), to_dev(_cu((3, 5)))
    out = torch.empty(8, dtype=torch.int64, device=dev())
    meta = torch.empty(4, dtype=torch.int32, device=dev())
    lib = load_lib()
    args = [lab.data_ptr(), None, cu.data_ptr(), 2, None, out.data_ptr(), out.data_ptr(), meta.data_ptr(), 8, None]
    for i, v in ((0, None), (2, None), (5, None), (6, None), (7, None), (3, 0), (8, 0), (8, 2 ** 30 + 1)):
        bad = list(args)
        bad[i] = v
        assert lib.sd_packed_rows(*bad) != 0, i
    pos = torch.zeros(1, 8, dtype=torch.long)
    pos[0, 6] = -1
    with pytest.raises(ValueError, match="non-negative"):
        ops.packed_rows(lab, cu, position_ids=to_dev(pos))


# ------------------------------------------------------------------------------------------------ the C1 fixture
class _Tok:
    pad_token = "<|semantic_token_end|>"

    def __init__(self, pad, bos):
        self.pad_token_id, self.bos = pad, bos

    def encode(self, text, add_special_tokens=False):
        return [self.bos]


ST, TE = (640, 128, 256, 2, 2, 1), (640, 256, 512, 2, 4, 2)


@pytest.fixture(scope="module")
def c1():
    from oracle import qwen3 as Q
    z = load_golden("g4_step_c1.npz")
    V, bos, pad = [int(x) for x in z["meta"]]
    sw, tw = Q.init_weights(Q.Qwen3Shape(*ST), seed=1), Q.init_weights(Q.Qwen3Shape(*TE), seed=2)
    feats = []
    for r in range(int(z["n"])):
        ids = z[f"in_{r}_ids"].tolist()
        feats.append({"student_input_ids": ids, "student_attention_mask": [1] * len(ids),
                      "teacher_input_ids": ids, "teacher_attention_mask": [1] * len(ids)})
    return {"z": z, "sw": sw, "tw": tw, "feats": feats, "pad": pad, "bos": bos, "oracle": {}}


def _build(sda, shape, weights):
    model = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*shape), device=dev(), init_std=0)
    model.load_hf_state_dict(weights)
    return model


class _DS(torch.utils.data.Dataset):
    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return dict(self.rows[i])


def _trainer(sda, c1, top_k, rows=None, **targs):
    from transformers import TrainingArguments
    from speech_distill_amd.collator import ProcessedDataCollator
    from speech_distill_amd.trainer import DistillationTrainer
    student, teacher = _build(sda, ST, c1["sw"]), _build(sda, TE, c1["tw"])
    teacher.eval().requires_grad_(False)
    kw = dict(output_dir=tempfile.mkdtemp(), per_device_train_batch_size=4, gradient_accumulation_steps=2, num_train_epochs=1,
              learning_rate=1e-3, logging_steps=1, save_strategy="no", eval_strategy="no", report_to=[],
              remove_unused_columns=False, label_names=["labels"], seed=42, data_seed=42, lr_scheduler_type="constant",
              warmup_steps=0, weight_decay=0.0, max_grad_norm=1.0, dataloader_num_workers=0, bf16=True)
    kw.update(targs)
    coll = ProcessedDataCollator(_Tok(c1["pad"], c1["bos"]), pad_token_id=c1["pad"], padding_free=True)
    tr = DistillationTrainer(model=student, args=TrainingArguments(**kw), train_dataset=_DS(rows or c1["feats"]),
                             data_collator=coll, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=top_k)
    return tr, student, coll


def _on_dev(batch):
    return {k: (to_dev(v) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _oracle(c1, top_k, mb):
    """oracle/step.py (fp32, and with bf16 storage rounding) on the PADDED batch of the same samples: computed once per
    (top_k, micro-batch) and shared by the compact / full cases."""
    if (top_k, mb) not in c1["oracle"]:
        from oracle import qwen3 as Q
        from oracle import step as S
        from speech_distill_amd.collator import ProcessedDataCollator
        padded = ProcessedDataCollator(_Tok(c1["pad"], c1["bos"]), pad_token_id=c1["pad"])(
            [dict(f) for f in c1["feats"][4 * mb: 4 * mb + 4]])
        st_, te_ = Q.Qwen3Shape(*ST), Q.Qwen3Shape(*TE)
        kw = dict(temperature=2.0, alpha=0.5, top_k=top_k, acc=torch.float32)
        c1["oracle"][(top_k, mb)] = (S.distill_step(c1["sw"], st_, c1["tw"], te_, padded, **kw),
                                     S.distill_step(c1["sw"], st_, c1["tw"], te_, padded, storage="bf16", **kw))
    return c1["oracle"][(top_k, mb)]


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("mode,top_k", [("sparse", 16), ("dense", 0)])
def test_c1_packed_compute_loss_matches_reference(sda, c1, mode, top_k, compact):
    """BASELINE config 1, the two fixed micro-batches collated with ``padding_free=True``: packing does not change which
    rows the loss reads, so the expected values are the fixture's and the bounds are those
    test_c1_compute_loss_matches_reference applies to the padded layout -- loss within 2e-2 relative, the three logged
    sub-losses at rtol 3e-2, per-tensor gradient norms within 8e-2, and the gradient error budget at factor 1.5 against
    oracle/step.py on the padded batch of the same samples."""
    z = c1["z"]
    tr, student, coll = _trainer(sda, c1, top_k)
    tr.compact_head = compact
    logged = []
    tr.log = lambda d, *a, **k: logged.append(dict(d))
    for mb in range(2):
        batch = _on_dev(coll([dict(f) for f in c1["feats"][4 * mb: 4 * mb + 4]]))
        assert "attention_mask" not in batch and batch["input_ids"].shape[0] == 1
        student.zero_grad()
        loss = tr.compute_loss(student, dict(batch))
        loss.backward()
        got, ref = float(loss.detach()), float(z[f"{mode}_mb{mb}_loss"])
        record(f"c1_packed_{mode}_mb{mb}_compact{int(compact)}", loss=got, ref=ref, logged=logged[-1])
        print(f"c1 packed {mode} mb{mb} compact={compact}: loss {got:.6f} ref {ref:.6f} logged {logged[-1]}")
        assert abs(got - ref) <= 2e-2 * abs(ref)
        got3 = [logged[-1]["student_loss"], logged[-1]["teacher_loss"], logged[-1]["distill_loss"]]
        np.testing.assert_allclose(got3, z[f"{mode}_mb{mb}_logged"], rtol=3e-2)
        for k, p in student._params.items():
            rn = float(z[f"{mode}_mb{mb}_gnorm_{k}"])
            gn = float(p.grad.double().norm())
            assert abs(gn - rn) <= 8e-2 * rn + 1e-7, f"{mode} mb{mb} {k}: {gn} vs {rn}"
        o32, o16 = _oracle(c1, top_k, mb)
        np.testing.assert_allclose(float(o32["total"]), ref, rtol=1e-4)
        assert_grad_budget(f"c1_packed_{mode}_mb{mb}_compact{int(compact)}", {k: p.grad for k, p in student._params.items()},
                           o32["grads"], o16["grads"])


# ------------------------------------------------------------------------------------------------ packed_batch=
def test_packed_batch_keyword_equals_the_models_own_host_read(sda):
    """``model(input_ids, packed_batch=pb)`` with a descriptor built from ``ops.packed_rows``' numbers (no read of its own)
    against ``model(input_ids, position_ids=, cu_seq_lens_q=)``: logits and every gradient bit for bit, in training and in
    the frozen folded mode; a descriptor of another token count or RoPE base is refused."""
    from speech_distill_amd import ops
    V = 1000
    model = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 512, 1024, 2, 4, 2), device=dev(), seed=4)
    lens = (40, 24, 64, 1, 31)
    M = sum(lens)
    cu = to_dev(_cu(lens))
    ids = torch.randint(0, V, (1, M), generator=torch.Generator().manual_seed(8)).to(dev())
    pos = to_dev(_positions(cu.cpu(), M))
    probe = torch.randn(1, M, V, generator=torch.Generator().manual_seed(9)).to(dev())
    _, _, longest, max_pos = ops.packed_rows(ids, cu, None, pos)
    assert (longest, max_pos) == (64, 63)
    pb = model.packed_batch(cu, pos, longest, max_pos)
    assert (pb.M, pb.n, pb.max_seqlen) == (M, 5, 64)

    def run(**kw):
        model.zero_grad()
        out = model(input_ids=ids, **kw).logits
        (out.float() * probe).sum().backward()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in model._params.items()}
    la, ga = run(position_ids=pos, cu_seq_lens_q=cu, cu_seq_lens_k=cu)
    lb, gb = run(packed_batch=pb)
    lc, gc = run(packed_batch=pb, position_ids=pos, cu_seq_lens_q=cu, cu_seq_lens_k=cu, max_length_q=64, max_length_k=64)
    assert torch.equal(la, lb) and torch.equal(la, lc) and ga.keys() == gb.keys() and len(ga) > 0
    for k in ga:
        assert torch.equal(ga[k], gb[k]) and torch.equal(ga[k], gc[k]), k
    with pytest.raises(ValueError, match="packed_batch"):
        model(input_ids=ids[:, :-1], packed_batch=pb)
    with pytest.raises(ValueError, match="packed_batch"):
        model(input_ids=ids, attention_mask=torch.ones_like(ids), packed_batch=pb)
    other = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 256, 512, 1, 2, 1, rope_theta=1e4), device=dev(), seed=1)
    assert not other.shares_packed_batch(model)
    with pytest.raises(ValueError, match="packed_batch"):
        other(input_ids=ids, packed_batch=pb)
    model.eval().requires_grad_(False)
    with torch.no_grad():
        fa = model(input_ids=ids, position_ids=pos, cu_seq_lens_q=cu).logits
        assert model._folded is not None      # the frozen model's folded forward ran
        fb = model(input_ids=ids, packed_batch=pb).logits
        rows = to_dev(torch.tensor([0, 39, 40, 128, 158]))
        ra = model(input_ids=ids, position_ids=pos, cu_seq_lens_q=cu, logit_rows=rows).logits
        rb = model(input_ids=ids, packed_batch=pb, logit_rows=rows).logits
    assert torch.equal(fa, fb) and torch.equal(ra, rb)


# ------------------------------------------------------------------------------------------------ trainer paths
def test_pre_extracted_topk_on_packed_rows_equals_the_live_teacher(sda, c1):
    """The live teacher's top-K rows of a packed batch, split per sample and put into the features, then collated packed:
    same kernels on the same rows, so the loss and every gradient are bit-identical to the live-teacher step."""
    tr, student, coll = _trainer(sda, c1, 16)
    tr.overlap_teacher = False     # (beside a teacher the student's GEMMs take another tile: SD_FWD_CONCURRENT)
    tr.log = lambda *a, **k: None
    feats = c1["feats"][:4]
    batch = _on_dev(coll([dict(f) for f in feats]))
    M, K = batch["input_ids"].numel(), 16
    kept, inner = [], tr._extract_topk

    def spy(logits, k, V):
        v, i = inner(logits, k, V)
        kept.append((v.clone(), i.clone()))
        return v, i
    tr._extract_topk = spy
    student.zero_grad()
    live = tr.compute_loss(student, dict(batch))
    live.backward()
    g_live = {k: p.grad.detach().clone() for k, p in student._params.items()}
    from speech_distill_amd import ops
    rows = ops.packed_rows(batch["labels"], batch["cu_seq_lens_q"])[0]
    (v, i), = kept
    assert v.shape == (rows.numel(), K) and 0 < rows.numel() < M
    full_v = torch.zeros(M, K, dtype=v.dtype, device=dev())
    full_i = torch.zeros(M, K, dtype=i.dtype, device=dev())
    full_v[rows], full_i[rows] = v, i
    cu = batch["cu_seq_lens_q"].tolist()
    pre = [dict(f, teacher_top_k_v=full_v[a:b].cpu(), teacher_top_k_i=full_i[a:b].cpu()) for f, a, b in zip(feats, cu, cu[1:])]
    pbatch = _on_dev(coll(pre))
    assert pbatch["teacher_top_k_v"].shape == (1, M, K)
    calls = []
    tr._extract_topk = lambda *a: calls.append(1)
    student.zero_grad()
    got = tr.compute_loss(student, dict(pbatch))
    got.backward()
    assert not calls and torch.equal(got.detach(), live.detach()) and float(got.detach()) > 0
    for k, p in student._params.items():
        assert torch.equal(p.grad, g_live[k]), k


def test_full_path_masks_document_starts_itself(sda, c1):
    """``compute_loss(..., return_outputs=True)`` (the [1, M, V] path of evaluation): a real label written at a document
    start does not change the loss."""
    tr, student, coll = _trainer(sda, c1, 16)
    tr.log = lambda *a, **k: None
    batch = _on_dev(coll([dict(f) for f in c1["feats"][:4]]))
    cu = batch["cu_seq_lens_q"].tolist()
    tampered = batch["labels"].clone()
    for a in cu[:-1]:
        assert int(tampered[0, a]) == -100
        tampered[0, a] = 7
    with torch.no_grad():
        clean, out = tr.compute_loss(student, dict(batch), return_outputs=True)
        dirty, _ = tr.compute_loss(student, dict(batch, labels=tampered), return_outputs=True)
        # segments by position_ids alone (HF's flattening without the flash-attn keys), head on the loss rows: the rows
        # come from the masked labels, so the tampered batch gives the loss of the clean one with its segments given
        keyed = tr.compute_loss(student, dict(batch))
        bare = {k: v for k, v in batch.items() if not k.startswith(("cu_seq_lens", "max_length"))}
        bare_dirty = tr.compute_loss(student, dict(bare, labels=tampered))
        tr.compact_head = False
        dirty_train = tr.compute_loss(student, dict(batch, labels=tampered))
    assert out.logits.shape == (1, batch["input_ids"].numel(), 640)
    assert float(clean) == float(dirty) == float(dirty_train) and np.isfinite(float(clean)) and float(clean) > 0
    assert float(keyed) == float(bare_dirty) and np.isfinite(float(keyed)) and float(keyed) > 0
    # and the case is real: on the flat row the tampered labels select more rows
    from speech_distill_amd import ops
    assert ops.loss_rows(tampered)[0].numel() == ops.loss_rows(batch["labels"])[0].numel() + len(cu) - 2


def test_evaluate_on_packed_batches(sda, c1):
    """HF's evaluation loop (prediction_step -> compute_loss(return_outputs=True), [1, M, V] logits of two packed batches of
    different M gathered): eval_loss is the mean of the two batches' full-path losses."""
    tr, student, coll = _trainer(sda, c1, 16, per_device_eval_batch_size=4)
    tr.log = lambda *a, **k: None
    with torch.no_grad():
        want = [float(tr.compute_loss(student, _on_dev(coll([dict(f) for f in c1["feats"][i:i + 4]])), return_outputs=True)[0])
                for i in (0, 4)]
    got = tr.evaluate(_DS(c1["feats"]))["eval_loss"]
    assert np.isfinite(got) and abs(got - np.mean(want)) <= 1e-6 * np.mean(want), (got, want)


def test_real_train_loop_packed_with_and_without_the_lookaheads(sda, c1, monkeypatch):
    """Three optimizer steps of a real ``Trainer.train()`` (two samples per packed micro-batch, accumulation 2) with the
    lookaheads on (rows ahead, teacher ahead, window ahead) and with SD_ROWS_AHEAD=0: the same micro-batches in the same
    order, by the method of test_window_lookahead_serves_the_same_batches_in_the_same_order, finite logged losses, and the
    bound that test uses for the two runs' losses: equality (both runs launch the same kernels on the same data).  Also one
    selection (``ops.loss_rows`` + ``ops.packed_rows``) per micro-batch.  With the lookaheads on this is counted per FETCHED
    micro-batch, not per trained one as in the padded test (whose loop ends with its iterator): ``max_steps`` stops this loop
    with the fourth window already fetched ahead, so 8 selections stand against 6 trained micro-batches."""
    from transformers import Trainer
    from speech_distill_amd import ops
    rows = c1["feats"] * 2

    def run(ahead):
        monkeypatch.setenv("SD_ROWS_AHEAD", "1" if ahead else "0")
        tr, student, _ = _trainer(sda, c1, 16, rows=rows, per_device_train_batch_size=2, max_steps=3, seed=7, data_seed=7)
        seen, early, reads, in_step, fetched, inner, hf_fetch = [], [], [], [], [], tr.compute_loss, Trainer.get_batch_samples

        def fetch(self, *a, **k):    # HF's own fetch of one accumulation window, under the trainer's override
            out = hf_fetch(self, *a, **k)
            fetched.extend(out[0])
            return out

        def spy(model, inputs, *a, **k):
            assert "attention_mask" not in inputs and inputs["input_ids"].shape[0] == 1
            seen.append(inputs["input_ids"].cpu().clone())
            early.append(getattr(tr._ahead.get(id(inputs["labels"])), "teacher", None) is not None)
            n0 = len(reads)
            out = inner(model, inputs, *a, **k)
            in_step.append(len(reads) - n0)
            return out
        tr.compute_loss = spy
        with monkeypatch.context() as mp:
            mp.setattr(Trainer, "get_batch_samples", fetch)
            for name in ("loss_rows", "packed_rows"):   # the selections, each with the micro-batch's one host read
                mp.setattr(ops, name, lambda *a, _f=getattr(ops, name), **k: reads.append(1) or _f(*a, **k))
            tr.train()
        return (seen, early, [h["loss"] for h in tr.state.log_history if "loss" in h], student.flat.clone(), tr.tokens_seen,
                (len(reads), in_step, len(fetched)))
    seen_a, early_a, loss_a, flat_a, tok_a, reads_a = run(True)
    seen_b, early_b, loss_b, flat_b, tok_b, reads_b = run(False)
    print("packed train loop losses:", loss_a, loss_b, "early:", early_a, "selections:", reads_a, reads_b)
    assert len(seen_a) == len(seen_b) == 6 and len(loss_a) == len(loss_b) == 3
    # One selection (one host read) per micro-batch, made ahead or in compute_loss, never both.  max_steps stops the loop
    # with the fourth window already fetched ahead: its two micro-batches were fetched and selected, and never trained on.
    assert reads_b == (6, [1] * 6, 6) and reads_a == (8, [0] * 6, 8)
    for a, b in zip(seen_a, seen_b):
        assert a.shape == b.shape and torch.equal(a, b)
    assert tok_a == tok_b == sum(s.numel() for s in seen_a)           # tokens_seen counts M
    assert all(np.isfinite(loss_a)) and all(np.isfinite(loss_b))
    assert loss_a == loss_b and torch.equal(flat_a, flat_b)
    assert early_a[1:] == [True] * 5 and not any(early_b)             # the teacher ran ahead on packed batches too


def test_train_cli_pack_tokens(sda, tmp_path):
    log = tmp_path / "log.json"
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--random_init", "--tiny",
           "--synthetic_samples", "24", "--pack_tokens", "256", "--max_steps", "2", "--max_length", "96",
           "--per_device_train_batch_size", "2", "--gradient_accumulation_steps", "2", "--logging_steps", "1",
           "--warmup_steps", "0", "--save_strategy", "no", "--top_k", "16", "--output_dir", str(tmp_path / "out"),
           "--log_json", str(log)]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads(log.read_text())
    logs = [e for e in d["log_history"] if "loss" in e]
    assert d["global_step"] == 2 and len(logs) == 2 and all(np.isfinite(e["loss"]) for e in logs), d["log_history"]
    assert any(np.isfinite(e.get("tokens_per_second", np.nan)) and e["tokens_per_second"] > 0 for e in logs), logs
    assert d["optimizer"] == "FlatAdamW"
