"""-m gpu tests of the MXFP8 frozen teacher (include/sd_hip.h "MXFP8 frozen teacher"): the quantisation kernel and the
block-scaled GEMM against tests/mx_ref.py, the fused SwiGLU epilogue against the unfused sequence, and the model / trainer
wiring at inference precision "mxfp8".  Exact where the format allows it; where it does not, the bound is stated."""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

import mx_ref
from conftest import ROOT
from gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sda():
    import speech_distill_amd as m
    m.load_lib()
    return m


def _inputs(kind, M, K, g):
    if kind == "normal":
        return torch.randn(M, K, generator=g)
    if kind == "small":
        return 0.02 * torch.randn(M, K, generator=g)
    if kind == "heavy":
        return torch.randn(M, K, generator=g) * torch.randn(M, K, generator=g).exp()
    x = torch.randn(M, K, generator=g)
    x[::3] = 0  # all-zero rows
    x[min(1, M - 1), 32:96] = 0  # all-zero blocks inside a row
    return x


# ------------------------------------------------------------------------------------------------ 5: the quant kernel
@pytest.mark.parametrize("M,K", [(1, 128), (2047, 2048), (300, 6144), (64, 128)])
def test_quant_kernel_equals_the_reference_rule(sda, M, K):
    """sd_mxfp8_quant vs mx_ref.mx_quant: scale bytes equal, dequantised elements equal (only the sign of a zero may differ
    in the byte), rstd to 1e-6 relative.  Exact: there is no tolerance to choose."""
    from speech_distill_amd import ops
    g = torch.Generator().manual_seed(M * 7 + K)
    for kind in ("normal", "small", "heavy", "zeros"):
        x = _inputs(kind, M, K, g).bfloat16()
        q, s, rstd = ops.mxfp8_quant(to_dev(x), want_rstd=True, eps=1e-6)
        rq, rs = mx_ref.mx_quant(x.float())
        assert torch.equal(s.cpu(), rs), (kind, "scale bytes")
        assert torch.equal(mx_ref.mx_deq(q.cpu(), s.cpu()), mx_ref.mx_deq(rq, rs)), (kind, "elements")
        ref_rstd = torch.rsqrt(x.double().pow(2).mean(-1) + 1e-6)
        assert float(((rstd.cpu().double() - ref_rstd).abs() / ref_rstd).max()) <= 1e-6, kind
        q2, s2 = ops.mxfp8_quant(to_dev(x))  # without rstd: same bytes
        assert torch.equal(q2, q) and torch.equal(s2, s)


def test_quant_kernel_on_a_strided_view_and_rejects_cpu(sda):
    from speech_distill_amd import ops
    g = torch.Generator().manual_seed(5)
    big = to_dev(torch.randn(33, 3 * 256, generator=g).bfloat16())
    view = big[:, 256:512]
    q, s = ops.mxfp8_quant(view)
    qc, sc = ops.mxfp8_quant(view.contiguous())
    assert torch.equal(q, qc) and torch.equal(s, sc)
    rq, rs = mx_ref.mx_quant(view.float().cpu())
    assert torch.equal(s.cpu(), rs) and torch.equal(mx_ref.mx_deq(q.cpu(), s.cpu()), mx_ref.mx_deq(rq, rs))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mxfp8_quant(torch.zeros(4, 128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = torch.zeros(4, 128, dtype=torch.uint8)
        ops.gemm_mxfp8(z, z[:, :4], z, z[:, :4])


# ------------------------------------------------------------------------------------------------ 6: GEMM, exact
def _int_operand(rows, K, vmax, smax, g):
    """Operand built directly as bytes: integer elements |v| <= vmax and power-of-two scales 2^-smax..2^smax, different
    per block and per row."""
    v = torch.randint(-vmax, vmax + 1, (rows, K), generator=g).float()
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    s = (127 + torch.randint(-smax, smax + 1, (rows, K // 32), generator=g)).to(torch.uint8)
    return q, s


@pytest.mark.parametrize("M,N,K,vmax,smax", [(200, 160, 6144, 4, 1), (77, 96, 256, 8, 2), (129, 288, 2048, 4, 1),
                                             (16, 32, 128, 8, 2), (520, 11040, 256, 8, 2)])
def test_gemm_exact_integers_pin_the_operand_and_scale_maps(sda, M, N, K, vmax, smax):
    """Every partial sum is exact in fp32 in any order (|v| <= 4, scales 2^-1..1, K = 6144: |sum| < 2^21 in units of
    2^-2; wider ranges at small K), so the result must EQUAL the fp32 matmul of the dequantised operands.  B is unrelated
    to A (asymmetric), scales differ per row and per block, M and N are not multiples of the tile; the last case is large
    enough for the 256-row tile, the others take the 128-row one."""
    from speech_distill_amd import ops
    g = torch.Generator().manual_seed(K + M)
    aq, as_ = _int_operand(M, K, vmax, smax, g)
    bq, bs = _int_operand(N, K, vmax, smax, g)
    ref = mx_ref.mx_deq(aq, as_).double() @ mx_ref.mx_deq(bq, bs).double().T
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref.float().double(), ref)
    out = ops.gemm_mxfp8(to_dev(aq), to_dev(as_), to_dev(bq), to_dev(bs))
    want = ref.float().bfloat16()  # the only rounding: the bf16 store
    assert torch.equal(out.cpu(), want), f"{int((out.cpu() != want).sum())} of {want.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ 7: GEMM, random data
C2_SHAPES = [(2048, 4096, 2048), (2048, 2048, 2048), (2048, 12288, 2048), (2048, 2048, 6144),
             (1531, 2048, 2048), (77, 4096, 2048)]  # every C2 teacher shape, then ragged M


@pytest.mark.parametrize("M,N,K", C2_SHAPES)
@pytest.mark.parametrize("with_rs,with_r", [(False, False), (True, True), (True, False), (False, True)])
def test_gemm_random_within_the_bf16_gemm_error(sda, M, N, K, with_rs, with_r):
    """Against an fp64 matmul of the dequantised operands.  Yardstick: the existing sd_gemm_bf16 on the dequantised
    operands (exact in bf16, so it computes the same product): rms error <= 1.5 x its rms error and worst absolute error
    <= 2 x its worst.  The row scale is a power of two per row, so that the yardstick can take it exactly in its A."""
    from speech_distill_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a = to_dev(torch.randn(M, K, generator=g).bfloat16())
    b = to_dev((0.02 * torch.randn(N, K, generator=g)).bfloat16())
    aq, as_ = ops.mxfp8_quant(a)
    bq, bs = ops.mxfp8_quant(b)
    ad, bd = mx_ref.mx_deq(aq, as_), mx_ref.mx_deq(bq, bs)
    rs = to_dev(torch.pow(2.0, torch.randint(-3, 4, (M,), generator=g).float())) if with_rs else None
    r = to_dev(torch.randn(M, N, generator=g).bfloat16()) if with_r else None
    got = ops.gemm_mxfp8(aq, as_, bq, bs, rowscale=rs, residual=r)
    a_y = (ad * rs[:, None] if with_rs else ad).bfloat16()
    assert torch.equal(a_y.float(), ad * rs[:, None] if with_rs else ad)  # exact in bf16
    yard = ops.gemm(a_y, bd.bfloat16(), residual=r)
    ref = a_y.double() @ bd.double().T
    if with_r:
        ref = ref + r.double()
    e_got, e_yard = (got.double() - ref), (yard.double() - ref)
    rms_ratio = float(e_got.pow(2).mean().sqrt() / e_yard.pow(2).mean().sqrt())
    max_ratio = float(e_got.abs().max() / e_yard.abs().max())
    print(f"gemm_mxfp8 {M}x{N}x{K} rs={with_rs} r={with_r}: rms ratio {rms_ratio:.4f} max ratio {max_ratio:.4f}")
    record("gemm_mxfp8_vs_bf16_gemm", M=M, N=N, K=K, rowscale=with_rs, residual=with_r, rms_ratio=rms_ratio,
           max_ratio=max_ratio)
    assert rms_ratio <= 1.5 and max_ratio <= 2.0


# ------------------------------------------------------------------------------------------------ 8: fused epilogue
@pytest.mark.parametrize("M,I,K", [(2048, 6144, 2048), (333, 1024, 512), (1, 128, 128)])
def test_swiglu_emitting_epilogue_equals_the_unfused_sequence_bit_for_bit(sda, M, I, K):
    """sd_gemm_mxfp8_swiglu == sd_gemm_mxfp8 (gate|up, bf16) -> sd_swiglu_fwd -> sd_mxfp8_quant: bytes and scale bytes."""
    from speech_distill_amd import ops
    g = torch.Generator().manual_seed(M + I)
    x = to_dev((3 * torch.randn(M, K, generator=g)).bfloat16())
    w = to_dev((0.05 * torch.randn(2 * I, K, generator=g)).bfloat16())
    xq, xs, rstd = ops.mxfp8_quant(x, want_rstd=True)
    wq, ws = ops.mxfp8_quant(w)
    for rs in (rstd, None):
        gu = ops.gemm_mxfp8(xq, xs, wq, ws, rowscale=rs)
        uq, us = ops.mxfp8_quant(ops.swiglu_fwd(gu))
        fq, fs = ops.gemm_mxfp8_swiglu(xq, xs, wq, ws, rowscale=rs)
        assert torch.equal(fs, us), "scale bytes"
        assert torch.equal(fq, uq), f"{int((fq != uq).sum())} of {uq.numel()} bytes differ"


# ------------------------------------------------------------------------------------------------ 9: the model
SHP = (1200, 512, 1024, 3, 4, 2)


def _weights(seed):
    from oracle import qwen3 as Q
    shp = Q.Qwen3Shape(*SHP)
    return shp, {k: v.bfloat16().float() for k, v in Q.init_weights(shp, seed=seed, norm_jitter=0.25).items()}


def _model(sda, w, device=None):
    model = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*SHP), device=device or dev(), init_std=0)
    model.load_hf_state_dict(w)
    model.eval().requires_grad_(False)
    return model


def _batch():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, SHP[0], (3, 90), generator=g)
    am = torch.ones(3, 90, dtype=torch.long)
    am[1, 61:] = 0
    return ids, am


def _by_hand(model, ids, kv_len=None, rows=None, packed=None):
    """The mxfp8 forward composed from the ops bindings on the model's own prepared weights (no `concurrent`)."""
    from speech_distill_amd import ops
    d = model.dims
    B, T = ids.shape
    Hq, Hkv, eps = d.num_attention_heads, d.num_key_value_heads, d.rms_norm_eps
    QD, KD = Hq * 128, Hkv * 128
    model._mx_params()
    keep = model._mx[2]
    cos, sin = (packed.cos, packed.sin) if packed is not None else model._tables(T, ids.device)
    Tr = packed.M if packed is not None else T
    x = ops.embedding_fwd(ids.reshape(-1), model._params["model.embed_tokens.weight"].data)
    for l in range(d.num_hidden_layers):
        wqkv_q, wqkv_s, wgu_q, wgu_s, wo_q, wo_s, wd_q, wd_s = keep[8 * l:8 * l + 8]
        p = f"model.layers.{l}."
        xq, xs, rstd = ops.mxfp8_quant(x, want_rstd=True, eps=eps)
        qkv = ops.gemm_mxfp8(xq, xs, wqkv_q, wqkv_s, rowscale=rstd)
        qk = ops.qknorm_rope_fwd(qkv, model._params[p + "self_attn.q_norm.weight"].data,
                                 model._params[p + "self_attn.k_norm.weight"].data, cos, sin, Tr, Hq, Hkv, eps)
        q, k, v = qk[:, :QD], qk[:, QD:], qkv[:, QD + KD:]
        if packed is not None:
            ao, _ = ops.attn_fwd_varlen(q, k, v, packed.cu, Hq, Hkv, packed.max_seqlen)
        else:
            ao, _ = ops.attn_fwd(q, k, v, B, T, Hq, Hkv, kv_len)
        aq, as_ = ops.mxfp8_quant(ao)
        x_mid = ops.gemm_mxfp8(aq, as_, wo_q, wo_s, residual=x)
        mq, ms, rstd2 = ops.mxfp8_quant(x_mid, want_rstd=True, eps=eps)
        cq, cs = ops.gemm_mxfp8_swiglu(mq, ms, wgu_q, wgu_s, rowscale=rstd2)
        x = ops.gemm_mxfp8(cq, cs, wd_q, wd_s, residual=x_mid)
    xn, _ = ops.rmsnorm_fwd(x, model._params["model.norm.weight"].data, eps)
    if rows is not None:
        xn = ops.embedding_fwd(rows, xn)
    return ops.gemm(xn, model.lm_head.weight.data)


def test_model_wiring_is_exact(sda):
    """9a: model(...) at precision "mxfp8" equals, bit for bit, the same forward composed by hand from the ops bindings on
    the model's prepared weights: same kernels on the same inputs.  Also with logit_rows, and packed through position_ids
    (hand-composed with the varlen attention: bit for bit; against the padded run of the same documents: cosine >= 0.999,
    the bound tests/test_gpu_packed.py uses for the bf16 model, since tile choice may differ with M)."""
    _, w = _weights(9)
    model = _model(sda, w).set_inference_precision("mxfp8")
    ids, am = _batch()
    ids_d, am_d = to_dev(ids), to_dev(am)
    kv_len = am_d.sum(-1).to(torch.int32)
    with torch.no_grad():
        got = model(input_ids=ids_d, attention_mask=am_d).logits
        hand = _by_hand(model, ids_d, kv_len)
        assert torch.equal(got.view(-1, SHP[0]), hand)
        rows = to_dev(torch.tensor([0, 5, 89, 90 + 60, 2 * 90 + 7]))
        some = model(input_ids=ids_d, attention_mask=am_d, logit_rows=rows).logits
        assert torch.equal(some, _by_hand(model, ids_d, kv_len, rows=rows))
        # the same documents packed
        lens = [90, 61, 90]
        pids = torch.cat([ids[r, :n] for r, n in enumerate(lens)])[None].to(dev())
        pos = torch.cat([torch.arange(n) for n in lens])[None].to(dev())
        packed_logits = model(input_ids=pids, position_ids=pos).logits[0]
        pk = model._packed(pids, pos)
        assert torch.equal(packed_logits, _by_hand(model, pids, packed=pk))
        a, b = packed_logits.double().flatten(), got[am_d.bool()].double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm()))
        record("mx_packed_vs_padded_logits", cos=cos)
        assert cos >= 0.999


def test_model_arithmetic_against_the_torch_restatement(sda):
    """9b, LOOSE and said so.  Quantisation is discontinuous: a one-ulp bf16 difference upstream moves some elements by a
    whole e4m3 step, so the bf16 tolerance does not apply.  Budget: 1.5 x the rms error of
    teacher_forward_mx(storage="bf16") against teacher_forward_mx(storage=None), computed here on the CPU (no code under
    test involved).  This only separates gross errors (a lost rstd, a wrong weight, a missing residual); it also asserts
    that the HIP logits are closer to the MX restatement than to the unquantised one.  The fine checks are the kernel
    tests above and test_model_wiring_is_exact."""
    shp, w = _weights(9)
    model = _model(sda, w).set_inference_precision("mxfp8")
    ids, am = _batch()
    m = am.bool()
    with torch.no_grad():
        got = model(input_ids=to_dev(ids), attention_mask=to_dev(am)).logits.float().cpu()[m]
    ref = mx_ref.teacher_forward_mx(w, shp, ids, am)[m]
    ref_bf16 = mx_ref.teacher_forward_mx(w, shp, ids, am, storage="bf16")[m]
    noq = mx_ref.teacher_forward_mx(w, shp, ids, am, quant=False)[m]
    base = rel_err(ref_bf16, ref)[1]
    err = rel_err(got, ref)[1]
    err_noq = rel_err(got, noq)[1]
    print(f"mx model: rms err vs MX restatement {err:.4f}, budget base {base:.4f}, ratio {err / base:.3f}; "
          f"vs unquantised {err_noq:.4f}")
    record("mx_model_vs_restatement", rms_err=err, base=base, ratio=err / base, rms_vs_unquantised=err_noq)
    assert err <= 1.5 * base
    assert err < err_noq


def test_model_profile_precision_switch_and_reload(sda):
    """9c: no rmsnorm_fwd_kernel but the final one and no bf16 GEMM symbol but the lm_head's; "bf16" after "mxfp8" gives
    the original logits bit for bit; load_hf_state_dict with new weights gives the logits of a freshly built model, also
    for a model built on the CPU and moved with .to(device)."""
    from speech_distill_amd import ops
    _, w = _weights(9)
    _, w2 = _weights(10)
    model = _model(sda, w)
    ids, am = _batch()
    kw = dict(input_ids=to_dev(ids), attention_mask=to_dev(am))
    with torch.no_grad():
        bf_before = model(**kw).logits.clone()
        model.set_inference_precision("mxfp8")
        model(**kw)  # builds the quantised weights outside the profile
        ops.prof_begin()
        mx1 = model(**kw).logits.clone()
        ops.prof_end()
        syms = ops.prof_symbols()
        assert sum(v[2] for k, v in syms.items() if k.startswith("rmsnorm_fwd_kernel")) == 1, syms
        bf16_gemms = {k: v for k, v in syms.items() if "gemm" in k and not k.startswith("gemm_mx_kernel")}
        assert sum(v[2] for v in bf16_gemms.values()) == 1, syms  # the lm_head
        assert sum(v[2] for k, v in syms.items() if k.startswith("gemm_mx_kernel")) == 4 * SHP[3], syms
        assert not torch.equal(mx1, bf_before)
        model.set_inference_precision("bf16")
        assert torch.equal(model(**kw).logits, bf_before)
        model.set_inference_precision("mxfp8")
        assert torch.equal(model(**kw).logits, mx1)
        model.load_hf_state_dict(w2)
        reloaded = model(**kw).logits.clone()
        fresh = _model(sda, w2).set_inference_precision("mxfp8")
        assert torch.equal(reloaded, fresh(**kw).logits)
        assert not torch.equal(reloaded, mx1)
        cpu_model = _model(sda, w2, device="cpu").set_inference_precision("mxfp8")
        moved = cpu_model.to(dev())
        assert torch.equal(moved(**kw).logits, reloaded)
    # a model that is not frozen, or whose dims the kernels do not take, refuses the precision
    model.requires_grad_(True)
    with pytest.raises(ValueError, match="frozen"):
        model.set_inference_precision("mxfp8")
    odd = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 320, 512, 1, 2, 1), device=dev(), seed=0)
    odd.requires_grad_(False)
    with pytest.raises(ValueError, match="multiples of 128"):
        odd.set_inference_precision("mxfp8")


# ------------------------------------------------------------------------------------------------ 10: trainer, extraction
@pytest.mark.parametrize("top_k", [16, None])
def test_trainer_losses_with_an_mxfp8_teacher(sda, top_k, monkeypatch):
    """C1-sized DistillationTrainer.compute_loss with an "mxfp8" teacher (teacher-ahead on), sparse and dense: the four
    losses equal those of DistillationLoss fed the logits of a direct teacher(...) call at the same precision."""
    from transformers import TrainingArguments
    from speech_distill_amd.trainer import DistillationTrainer
    monkeypatch.setenv("SD_TEACHER_AHEAD", "1")
    V = 640
    student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 128, 256, 2, 2, 1), device=dev(), seed=0)
    teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 256, 512, 2, 4, 2), device=dev(), seed=1)
    teacher.eval().requires_grad_(False)
    teacher.set_inference_precision("mxfp8")
    args = TrainingArguments(output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False,
                             label_names=["labels"], save_strategy="no", bf16=True, logging_steps=1)
    tr = DistillationTrainer(model=student, args=args, teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=top_k,
                             is_quantized_teacher=top_k is None)
    logged = []
    tr.log = lambda d, *a, **k: logged.append(dict(d))
    g = torch.Generator().manual_seed(11)
    B, T = 4, 64
    ids = torch.randint(0, V, (B, T), generator=g)
    am = torch.ones(B, T, dtype=torch.long)
    am[2, 50:] = 0
    labels = ids.clone()
    labels[:, :17] = -100
    labels[am == 0] = -100
    batch = {k: to_dev(v) for k, v in dict(input_ids=ids, attention_mask=am, labels=labels, teacher_input_ids=ids,
                                           teacher_attention_mask=am).items()}
    loss = tr.compute_loss(student, dict(batch))
    torch.cuda.synchronize()
    assert teacher._mx is not None  # the quantised forward ran
    # the same step by hand, as compute_loss shapes it: the loss rows, both heads on those rows, both passes told that
    # they share the GPU
    from speech_distill_amd import ops
    rows, row_labels = ops.loss_rows(batch["labels"])
    kw = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], logit_rows=rows, concurrent=True)
    with torch.no_grad():
        t_logits = teacher(**kw).logits
    s_logits = student(**kw).logits.detach()
    crit = sda.DistillationLoss(temperature=2.0, alpha=0.5)
    if top_k is None:
        total, task, distill, t_loss = crit.forward_rows(s_logits, row_labels, teacher_logits=t_logits)
    else:
        tv, ti = ops.logsoftmax_topk(t_logits, top_k, V)
        total, task, distill, t_loss = crit.forward_rows(s_logits, row_labels, teacher_top_k_v=tv, teacher_top_k_i=ti)
    want = {"loss": float(total), "student_loss": float(task), "distill_loss": float(distill), "teacher_loss": float(t_loss)}
    got = {"loss": float(loss.detach()), **{k: logged[-1][k] for k in ("student_loss", "distill_loss", "teacher_loss")}}
    record("mx_trainer_losses", top_k=top_k or 0, got=got, want=want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-6 * max(1.0, abs(want[k])), (k, got, want)


def test_extract_teacher_logits_round_trip_at_mxfp8(sda, tmp_path, monkeypatch):
    """scripts/extract_teacher_logits.py --teacher_precision mxfp8 on the tiny random-init teacher: the stored indices
    equal ops.logsoftmax_topk of a direct call at the same precision."""
    from datasets import Dataset, load_from_disk
    from speech_distill_amd import ops
    V, bos, pad = 640, 320, 639
    teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(V, 256, 512, 2, 4, 2), device=dev(), seed=1)
    tdir, ddir, xdir = (str(tmp_path / n) for n in ("teacher", "data", "data_topk"))
    teacher.save_pretrained(tdir)
    g = torch.Generator().manual_seed(77)
    rows = []
    for _ in range(6):
        n = 40  # equal lengths: one batch, no padding, so a direct call sees the same rows
        ids = torch.cat([torch.randint(0, bos, (10,), generator=g), torch.tensor([bos]),
                         torch.randint(bos + 1, pad, (n - 12,), generator=g), torch.tensor([pad])]).tolist()
        rows.append({"student_input_ids": ids, "student_attention_mask": [1] * n,
                     "teacher_input_ids": ids, "teacher_attention_mask": [1] * n})
    Dataset.from_list(rows).save_to_disk(ddir)
    spec = importlib.util.spec_from_file_location("sd_extract_mx", os.path.join(ROOT, "scripts", "extract_teacher_logits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["extract_teacher_logits.py", "--teacher_model_path", tdir, "--dataset_path", ddir,
                                      "--output_path", xdir, "--top_k", "16", "--batch_size", "6", "--pad_token_id", str(pad),
                                      "--teacher_precision", "mxfp8"])
    mod.main()
    out = load_from_disk(xdir)
    col = "teacher_top_k_i"
    teacher.eval().requires_grad_(False)
    teacher.set_inference_precision("mxfp8")
    ids = to_dev(torch.tensor([r["teacher_input_ids"] for r in rows]))
    with torch.no_grad():
        logits = teacher(input_ids=ids, attention_mask=torch.ones_like(ids)).logits
    _, ti = ops.logsoftmax_topk(logits, 16)
    stored = np.asarray(out[col], dtype=np.int64).reshape(6, 40, 16)
    assert np.array_equal(stored, ti.cpu().numpy().astype(np.int64).reshape(6, 40, 16))
