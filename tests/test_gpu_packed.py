"""-m gpu: padding-free packed sequences -- the varlen attention kernels (sd_attn_fwd_varlen / sd_attn_bwd_varlen) against
the padded kernels run per document and against an fp32 block-diagonal reference, the packed model against HF Qwen3 and
against its own padded layout in every forward mode, and the padding-free Stage-1 collator / trainer / CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import check_close, dev, record, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_ROWS = 5  # rows past M in every buffer: NaN in the inputs (a read would show), a sentinel in the outputs


@pytest.fixture(scope="module")
def sda():
    import speech_distill_amd as m
    m.load_lib()
    return m


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def _lengths(case):
    if case == "rand150":
        g = torch.Generator().manual_seed(150)
        return torch.randint(1, 41, (150,), generator=g).tolist()
    if case == "span":
        return [777]  # one document spanning the whole buffer
    return list(case)


def _ref_attention(q, k, v, cu, Hq, Hkv):
    """fp64 CPU attention with a block-diagonal causal mask: [M, H*128] in, [M, Hq*128] out."""
    M = q.shape[0]
    G = Hq // Hkv
    qh = q.view(M, Hq, 128).transpose(0, 1)
    kh = k.view(M, Hkv, 128).transpose(0, 1).repeat_interleave(G, 0)
    vh = v.view(M, Hkv, 128).transpose(0, 1).repeat_interleave(G, 0)
    doc = torch.zeros(M, dtype=torch.long)
    for s in range(len(cu) - 1):
        doc[cu[s]:cu[s + 1]] = s
    t = torch.arange(M)
    allowed = (doc[:, None] == doc[None, :]) & (t[None, :] <= t[:, None])
    s = (qh @ kh.transpose(1, 2)) * 128 ** -0.5
    s = s.masked_fill(~allowed, float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(0, 1).reshape(M, Hq * 128)


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("Hq,Hkv", [(16, 8), (4, 2)])
@pytest.mark.parametrize("case", [(1,), (64,), (65,), (1, 1, 1), (5, 17, 1, 9), (63, 64, 65, 128, 129), (300, 700, 1100),
                                  "rand150", "span"])
def test_varlen_attention_vs_padded_per_document_and_fp32(sda, Hq, Hkv, case):
    """O, LSE, dQ, dK, dV of the packed call equal, bit for bit, those of sd_attn_fwd / sd_attn_bwd2 run on each
    document alone (B=1, T=L, same leading dimensions, classic forward kernel); the same against the fp64 reference at
    the tolerances of the padded attention tests; rows past M and columns past the head slots keep their sentinels."""
    from speech_distill_amd import _lib, ops
    lens = _lengths(case)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    M = int(cu[-1])
    g = torch.Generator().manual_seed(M + 17 * Hq + len(lens))
    W = (Hq + 2 * Hkv) * 128
    qkv_big = torch.full((M + NAN_ROWS, W), float("nan"), dtype=torch.bfloat16)
    qkv_big[:M] = (torch.randn(M, W, generator=g) * 1.5).bfloat16()
    do_big = torch.full((M + NAN_ROWS, Hq * 128), float("nan"), dtype=torch.bfloat16)
    do_big[:M] = torch.randn(M, Hq * 128, generator=g).bfloat16()
    qkv_d, do_d = qkv_big.to(dev()), do_big.to(dev())
    q, k, v = qkv_d[:M, :Hq * 128], qkv_d[:M, Hq * 128:(Hq + Hkv) * 128], qkv_d[:M, (Hq + Hkv) * 128:]
    do = do_d[:M]
    cu_d = torch.tensor(cu, dtype=torch.int32, device=dev())
    SENT = -7.0
    o_big = torch.full((M + NAN_ROWS, Hq * 128 + 128), SENT, dtype=torch.bfloat16, device=dev())
    lse_big = torch.full((Hq * M + 64,), SENT, dtype=torch.float32, device=dev())
    d_big = [torch.full((M + NAN_ROWS, w + 128), SENT, dtype=torch.bfloat16, device=dev())
             for w in (Hq * 128, Hkv * 128, Hkv * 128)]
    o, lse = ops.attn_fwd_varlen(q, k, v, cu_d, Hq, Hkv, max(lens), o=o_big[:M, :Hq * 128],
                                 lse=lse_big[:Hq * M].view(Hq, M))
    dq, dk, dv = ops.attn_bwd_varlen(q, k, v, o.contiguous(), do, lse, cu_d, Hq, Hkv, max(lens),  # (o, dO: one ld)
                                     dq=d_big[0][:M, :Hq * 128], dk=d_big[1][:M, :Hkv * 128], dv=d_big[2][:M, :Hkv * 128])
    torch.cuda.synchronize()
    # untouched: rows past M, columns past the head slots, the LSE tail
    for buf, w in ((o_big, Hq * 128), (d_big[0], Hq * 128), (d_big[1], Hkv * 128), (d_big[2], Hkv * 128)):
        assert bool((buf[M:] == SENT).all()) and bool((buf[:, w:] == SENT).all())
    assert bool((lse_big[Hq * M:] == SENT).all())
    assert all(bool(torch.isfinite(t.float()).all()) for t in (o, lse, dq, dk, dv))

    # per document, the padded kernels on that document alone
    try:
        _lib.debug_set("attn.variant", 1)  # the varlen forward is the classic kernel at every length
        for s in range(len(lens)):
            a, b = int(cu[s]), int(cu[s + 1])
            L = b - a
            o1, lse1 = ops.attn_fwd(q[a:b], k[a:b], v[a:b], 1, L, Hq, Hkv)
            assert torch.equal(o1, o[a:b]), f"O of document {s} (L={L})"
            assert torch.equal(lse1[0], lse[:, a:b]), f"LSE of document {s} (L={L})"
            dq1, dk1, dv1 = ops.attn_bwd(q[a:b], k[a:b], v[a:b], o1, do[a:b], lse1, 1, L, Hq, Hkv)
            assert torch.equal(dq1, dq[a:b]), f"dQ of document {s} (L={L})"
            assert torch.equal(dk1, dk[a:b]), f"dK of document {s} (L={L})"
            assert torch.equal(dv1, dv[a:b]), f"dV of document {s} (L={L})"
    finally:
        _lib.debug_set("attn.variant", 0)

    # fp64 block-diagonal reference
    qr, kr, vr = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    ref = _ref_attention(qr, kr, vr, cu.tolist(), Hq, Hkv)
    tag = f"varlen_H{Hq}/{Hkv}_{case if isinstance(case, str) else len(lens)}"
    check_close(tag + "_o", o, ref, 1.5e-2, 4e-3)
    (ref * do.double().cpu()).sum().backward()
    if float(qr.grad.abs().max()) == 0:  # only one-token documents: dQ is exactly 0, the kernel leaves bf16 rounding noise
        assert float(dq.float().abs().max()) <= 2e-2 * float(vr.grad.abs().max())
        assert float(dk.float().abs().max()) <= 2e-2 * float(vr.grad.abs().max())
        check_close(tag + "_dv", dv, vr.grad, 2e-2, 6e-3)
        return
    check_close(tag + "_dq", dq, qr.grad, 2e-2, 6e-3)
    check_close(tag + "_dk", dk, kr.grad, 2e-2, 6e-3)
    check_close(tag + "_dv", dv, vr.grad, 2e-2, 6e-3)


def test_varlen_malformed_descriptor_stays_in_bounds(sda):
    """cu_seqlens out of order, negative and past M: wrong numbers are allowed, an access outside rows [0, M) is not --
    the NaN rows past M are never read and the sentinel rows past M never written."""
    from speech_distill_amd import ops
    Hq, Hkv, M = 4, 2, 200
    W = (Hq + 2 * Hkv) * 128
    g = torch.Generator().manual_seed(5)
    qkv_big = torch.full((M + NAN_ROWS, W), float("nan"), dtype=torch.bfloat16)
    qkv_big[:M] = torch.randn(M, W, generator=g).bfloat16()
    qkv_d = qkv_big.to(dev())
    q, k, v = qkv_d[:M, :Hq * 128], qkv_d[:M, Hq * 128:(Hq + Hkv) * 128], qkv_d[:M, (Hq + Hkv) * 128:]
    o_big = torch.full((M + NAN_ROWS, Hq * 128), -7.0, dtype=torch.bfloat16, device=dev())
    for bad in ([0, 150, 90, 400, 200], [-50, 30, 260], [0, 200, 0, 200]):
        cu = torch.tensor(bad, dtype=torch.int32, device=dev())
        o, _ = ops.attn_fwd_varlen(q, k, v, cu, Hq, Hkv, o=o_big[:M])
        torch.cuda.synchronize()
        assert bool((o_big[M:] == -7.0).all()), bad
        assert bool(torch.isfinite(o[:max(0, min(bad[1], M))].float()).all()), bad


# ---------------------------------------------------------------------------------------------- model
def _packed_inputs(lens, V, seed, starts=None, device=None):
    g = torch.Generator().manual_seed(seed)
    docs = [torch.randint(0, V, (L,), generator=g) for L in lens]
    starts = starts or [0] * len(lens)
    pos = torch.cat([torch.arange(s0, s0 + L) for s0, L in zip(starts, lens)])
    ids = torch.cat(docs)[None]
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    d = device or dev()
    return docs, ids.to(d), pos[None].to(d), cu.to(d)


def test_packed_model_vs_hf_qwen3(sda):
    """Tiny HF Qwen3ForCausalLM (head_dim 128, 2 layers, fp32, eager, use_cache=False) on the CPU, packed input with
    position_ids (one document starting at position 3): logits and every parameter gradient under a probe, at the
    tolerances of test_qwen3_forward_backward_vs_hf_fixture."""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(vocab_size=640, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=True,
                      attention_bias=False, use_cache=False)
    torch.manual_seed(0)
    hf = Qwen3ForCausalLM._from_config(cfg, attn_implementation="eager").float()
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if "norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
            p.copy_(p.bfloat16().float())  # the HIP model holds bf16 weights: give HF the same values
    hf.eval()
    lens, starts = [7, 20, 1, 12], [0, 3, 0, 0]
    _, ids, pos, _ = _packed_inputs(lens, 640, 11, starts, device="cpu")
    ref = hf(input_ids=ids, position_ids=pos, use_cache=False).logits
    probe = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2))
    (ref * probe).sum().backward()
    model = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 256, 512, 2, 4, 2), device=dev(), init_std=0)
    model.load_hf_state_dict({k: v.detach() for k, v in hf.state_dict().items()})
    out = model(input_ids=ids.to(dev()), position_ids=pos.to(dev()))
    check_close("packed_logits_vs_hf", out.logits.float().cpu()[0], ref.detach()[0], 6e-2, 1.5e-2)
    (out.logits.float() * probe.to(dev())).sum().backward()
    hp = dict(hf.named_parameters())
    for k, p in model._params.items():
        r = hp[k].grad
        gn, rn = float(p.grad.double().norm()), float(r.double().norm())
        record("packed_hf_gnorm", param=k, got=gn, ref=rn)
        assert abs(gn - rn) <= 6e-2 * rn + 1e-6, f"{k}: grad norm {gn} vs {rn}"
        assert _cos(p.grad, r) >= 0.99, k


DIMS = (1000, 512, 1024, 2, 4, 2)  # hidden 512: the folded (frozen) forward applies
LENS = [37, 5, 64, 1, 90, 23]


def _model(sda, seed=4):
    return sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*DIMS), device=dev(), seed=seed)


def _padded(docs):
    w = max(len(d) for d in docs)
    ids = torch.zeros(len(docs), w, dtype=torch.long)
    am = torch.zeros(len(docs), w, dtype=torch.long)
    for r, d in enumerate(docs):
        ids[r, :len(d)] = d
        am[r, :len(d)] = 1
    return ids.to(dev()), am.to(dev())


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model._params.items() if p.grad is not None}


def test_packed_equals_padded_in_every_mode(sda):
    """The same documents packed (one row, varlen attention) and padded (one right-padded row each): logits of document
    tokens and every gradient agree (cosine >= 0.999) in training (save-all and recompute), no-grad and folded modes."""
    docs, ids, pos, _ = _packed_inputs(LENS, DIMS[0], 3)
    pids, am = _padded(docs)
    mask = am.bool()
    probe_rows = torch.randn(sum(LENS), DIMS[0], generator=torch.Generator().manual_seed(4)).to(dev())
    probe_pad = torch.zeros(*pids.shape, DIMS[0], device=dev())
    probe_pad[mask] = probe_rows
    for policy in ("never", "always"):
        model = _model(sda)
        model.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"recompute": policy})
        lp = model(input_ids=ids, position_ids=pos).logits[0]
        (lp.float() * probe_rows).sum().backward()
        gp = _grads(model)
        model.zero_grad()
        out = model(input_ids=pids, attention_mask=am).logits
        ld = out[mask]
        (out.float() * probe_pad).sum().backward()
        gd = _grads(model)
        c = _cos(lp.float(), ld.float())
        record("packed_vs_padded_logits", policy=policy, cos=c)
        assert c >= 0.999
        for k in gp:
            assert _cos(gp[k], gd[k]) >= 0.999, (policy, k)
    with torch.no_grad():
        a = model(input_ids=ids, position_ids=pos).logits[0]
        b = model(input_ids=pids, attention_mask=am).logits[mask]
    assert _cos(a.float(), b.float()) >= 0.999
    model.requires_grad_(False)
    with torch.no_grad():
        a = model(input_ids=ids, position_ids=pos).logits[0]
        assert model._folded is not None  # the frozen model's folded forward ran
        b = model(input_ids=pids, attention_mask=am).logits[mask]
    assert _cos(a.float(), b.float()) >= 0.999


def test_packed_bit_identities(sda):
    """Packed: recompute equals save-all, cu_seq_lens given equals segments derived from position_ids, and B>1 packed rows
    equal their flattening -- logits and gradients bit for bit."""
    docs, ids, pos, cu = _packed_inputs([40, 24, 64, 1, 31], DIMS[0], 8)  # 160 tokens = two rows of 80 at a boundary
    probe = torch.randn(1, 160, DIMS[0], generator=torch.Generator().manual_seed(9)).to(dev())

    def run(model, **kw):
        out = model(**kw).logits
        (out.float().reshape(probe.shape) * probe).sum().backward()
        g = _grads(model)
        model.zero_grad()
        return out.reshape(1, 160, -1).detach().clone(), g

    model = _model(sda)
    base = run(model, input_ids=ids, position_ids=pos)
    model.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"recompute": "always"})
    others = {"recompute": run(model, input_ids=ids, position_ids=pos)}
    model.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"recompute": "never"})
    others["cu_given"] = run(model, input_ids=ids, position_ids=pos, cu_seq_lens_q=cu, cu_seq_lens_k=cu.clone(),
                             max_length_q=64, max_length_k=64)
    # B > 1: rows [40, 24] and [64] (no document crosses a row) against the same 128 tokens as one row
    with torch.no_grad():
        out_b = model(input_ids=ids[:, :128].reshape(2, 64), position_ids=pos[:, :128].reshape(2, 64)).logits
        out_f = model(input_ids=ids[:, :128], position_ids=pos[:, :128]).logits
    assert out_b.shape == (2, 64, DIMS[0]) and torch.equal(out_b.reshape(1, 128, -1), out_f)
    for name, (lo, go) in others.items():
        assert torch.equal(lo, base[0]), name
        for k in base[1]:
            assert torch.equal(go[k], base[1][k]), (name, k)


# ---------------------------------------------------------------------------------------------- Stage 1
def _stage1_bins(V, seed=21):
    g = torch.Generator().manual_seed(seed)
    docs = [torch.randint(0, V, (int(torch.randint(1, 120, (1,), generator=g)),), generator=g).tolist() for _ in range(20)]
    from speech_distill_amd.stage1 import pack_bfd
    return [{"documents": b} for b in pack_bfd(docs, 256)]


def _stage1_model(sda, num_new=132):
    from speech_distill_amd.stage1 import freeze_model_weights
    m = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(1032, 256, 512, 2, 4, 2), device=dev(), seed=5)
    freeze_model_weights(m, num_new)
    return m


def test_stage1_micro_step_packed_vs_padded(sda):
    """One Stage-1 micro-step (forward + CE + embedding-only backward) on the same bins through both collators."""
    from speech_distill_amd.stage1 import Stage1Collator
    bins = _stage1_bins(1032)[:4]
    res = {}
    for pf in (False, True):
        batch = Stage1Collator(padding_free=pf)(bins)
        n_items = int((batch["labels"] != -100).sum())
        m = _stage1_model(sda)
        kw = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items()}
        out = m(**kw, num_items_in_batch=n_items)
        out.loss.backward()
        res[pf] = (n_items, float(out.loss), m._params["model.embed_tokens.weight"].grad.detach().clone(), m.stage1_row_lo)
    (n0, l0, g0, lo), (n1, l1, g1, _) = res[False], res[True]
    assert n0 == n1
    assert abs(l1 - l0) <= 1e-3 * abs(l0), (l0, l1)
    assert _cos(g1[lo:], g0[lo:]) >= 0.999
    assert not bool(g1[:lo].any()) and not bool(g0[:lo].any())


def test_stage1_trainer_three_steps_both_layouts(sda, tmp_path):
    """Three Stage1Trainer optimizer steps per layout: the new rows move the same way, the old rows and the decoder body
    stay bit-identical to their start."""
    from transformers import TrainingArguments
    from speech_distill_amd.stage1 import Stage1Collator
    from speech_distill_amd.trainer import Stage1Trainer
    bins = _stage1_bins(1032)
    finals = {}
    for pf in (False, True):
        m = _stage1_model(sda)
        lo = m.stage1_row_lo
        emb0 = m._params["model.embed_tokens.weight"].detach().clone()
        body0 = torch.cat([m.flat[a:b] for a, b in m.layer_ranges + [m.norm_range]]).clone()
        args = TrainingArguments(output_dir=str(tmp_path / f"o{int(pf)}"), per_device_train_batch_size=2, max_steps=3,
                                 gradient_accumulation_steps=1, learning_rate=1e-2, warmup_steps=0, logging_steps=1,
                                 save_strategy="no", report_to=[], remove_unused_columns=False, label_names=["labels"],
                                 optim="adamw_torch", bf16=True, seed=3, dataloader_num_workers=0)
        tr = Stage1Trainer(model=m, args=args, train_dataset=bins, data_collator=Stage1Collator(padding_free=pf))
        tr.train()
        emb = m._params["model.embed_tokens.weight"].detach()
        assert torch.equal(emb[:lo].view(torch.int16), emb0[:lo].view(torch.int16))
        body = torch.cat([m.flat[a:b] for a, b in m.layer_ranges + [m.norm_range]])
        assert torch.equal(body.view(torch.int16), body0.view(torch.int16))
        finals[pf] = (emb[lo:].float() - emb0[lo:].float()).cpu()
    c = _cos(finals[True], finals[False])
    record("stage1_trainer_packed_vs_padded_update_cos", cos=c)
    assert float(finals[True].abs().max()) > 0 and c >= 0.99


def test_stage1_cli_padding_free(sda, tmp_path):
    log = tmp_path / "log.json"
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "stage1.py"), "--random_init", "--tiny",
           "--padding_free", "--synthetic_samples", "48", "--max_steps", "4", "--max_seq_length", "256",
           "--num_new_tokens", "132", "--batch_size", "2", "--gradient_accumulation_steps", "2", "--logging_steps", "1",
           "--warmup_steps", "0", "--save_steps", "1000", "--eval_size", "0.2", "--eval_steps", "2",
           "--output_dir", str(tmp_path / "out"), "--log_json", str(log)]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads(log.read_text())
    losses = [e["loss"] for e in d["log_history"] if "loss" in e]
    assert d["global_step"] == 4 and len(losses) == 4 and all(np.isfinite(losses)), d["log_history"]
    assert any("eval_loss" in e and np.isfinite(e["eval_loss"]) for e in d["log_history"]), d["log_history"]
    assert d["body_checksum"] == d["body_checksum_before"]
    assert d["old_rows_checksum"] == d["old_rows_checksum_before"]
    assert os.path.isfile(tmp_path / "out" / "final_model" / "model.safetensors")
