"""-m gpu: Stage-1 speech-token alignment on the MI355X (reference stage1.py): the cross-entropy row kernels, the
range-restricted embedding scatter, the embedding-only backward runner (sd_qwen3_backward with SD_BWD_EMBED_ONLY), a HIP Stage-1
step against fixture G6, and scripts/stage1.py end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import check_close, dev, record, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sda():
    import speech_distill_amd as m
    m.load_lib()
    return m


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------- CE kernels
@pytest.mark.parametrize("V", [159488, 1000])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_celoss_rows_vs_fp64(sda, V, dtype):
    from speech_distill_amd import ops
    g = torch.Generator().manual_seed(V % 97)
    R = 300
    x = (torch.randn(R, V, generator=g) * 3).to(dtype)
    lab = torch.randint(0, V, (R,), generator=g)
    lab[::7] = -100
    valid = lab != -100
    ref_rows = torch.nn.functional.cross_entropy(x.double(), lab, ignore_index=-100, reduction="none")
    for divisor in (None, 417.0):
        d = float(valid.sum()) if divisor is None else divisor
        xd = to_dev(x).requires_grad_(True)
        loss, out = ops.celoss_rows(xd, to_dev(lab), None if divisor is None else torch.tensor([divisor], device=dev()))
        want = float(ref_rows.sum()) / d
        assert abs(float(loss) - want) <= 2e-5 * abs(want), (float(loss), want)
        assert float(out[2]) == float(valid.sum()) and float(out[3]) == d
        go = 0.37
        (loss * go).backward()
        p = torch.softmax(x.double(), -1)
        p[valid, lab[valid]] -= 1.0
        p[~valid] = 0.0
        ref_g = p * go / d
        check_close(f"celoss_grad_{V}_{dtype}", xd.grad.float().cpu(), ref_g, 1e-2 if dtype == torch.bfloat16 else 1e-5)
        assert xd.grad[to_dev(~valid)].eq(0).all()
    # in place (grad_logits aliases logits) == out of place, byte for byte
    a, b = to_dev(x), to_dev(x)
    la, _ = ops.celoss_rows(a.requires_grad_(True), to_dev(lab), None, inplace_grad=False)
    lb, _ = ops.celoss_rows(b.requires_grad_(True), to_dev(lab), None, inplace_grad=True)
    la.backward()
    ga = a.grad.clone()
    out_b = torch.autograd.grad(lb, b)[0]
    assert float(la) == float(lb)
    assert torch.equal(ga.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       out_b.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    assert out_b.data_ptr() == b.data_ptr()


# ---------------------------------------------------------------------------------------------- range scatter
@pytest.mark.parametrize("M", [1000, 16384, 70000])
def test_embedding_bwd_range_vs_index_add(sda, M):
    from speech_distill_amd import ops
    V, H, lo = 2000, 1024, 1236
    g = torch.Generator().manual_seed(M)
    ids = torch.randint(lo - 300, V, (M,), generator=g)
    ids[: M // 4] = torch.randint(lo, lo + 20, (M // 4,), generator=g)   # many duplicates
    dx = torch.randn(M, H, generator=g).bfloat16()
    sentinel = torch.full((V, H), 0.123, dtype=torch.bfloat16)
    base = torch.randn(V, H, generator=g).bfloat16()
    dE = torch.where(torch.arange(V)[:, None] < lo, sentinel, base)
    d1 = to_dev(dE)
    ops.embedding_bwd_range(to_dev(ids), to_dev(dx), d1, lo)
    d2 = to_dev(dE)
    ops.embedding_bwd_range(to_dev(ids), to_dev(dx), d2, lo)
    torch.cuda.synchronize()
    assert torch.equal(d1.view(torch.int16), d2.view(torch.int16))              # deterministic
    got = d1.cpu()
    assert torch.equal(got[:lo].view(torch.int16), sentinel[:lo].view(torch.int16))   # rows below row_lo untouched
    keep = ids >= lo
    ref = base.double().index_add_(0, ids[keep], dx[keep].double())
    check_close(f"embedding_bwd_range_{M}", got[lo:].float(), ref[lo:], 1e-2)


# ---------------------------------------------------------------------------------------------- runner
def _model(sda, dims, seed=0):
    m = sda.HipQwen3ForCausalLM(dims, device=dev(), seed=seed)
    m.overlap_dw = True
    return m


def _run(sda, m, ids, am, rows, dlogits, row_lo, save, acc, grads_flat, full=False):
    """One forward (save mode) + one backward into grads_flat (a flat buffer) -> None."""
    from speech_distill_amd import qwen3 as Qm
    from speech_distill_amd._lib import STAGE_CB, Batch, BwdOpts, check, load_lib
    from speech_distill_amd.ops import _stream
    lib = load_lib()
    B, T = ids.shape
    kv_len = am.sum(-1).to(torch.int32).contiguous()
    _, acts = m._run_forward(ids, kv_len, save=save, rows=rows)
    cos, sin = m._tables(T, ids.device)
    cg, _layers = m._c_struct(grads_flat)
    sbytes = lib.sd_qwen3_bwd_scratch_bytes(C.byref(m._cdims), B, T)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=ids.device)
    flags = (Qm.BWD_ACCUMULATE if acc else 0) | (Qm.BWD_RECOMPUTE if save == Qm.SAVE_LAYER_INPUTS else 0)
    batch = Batch(ids.data_ptr(), kv_len.data_ptr(), None, cos.data_ptr(), sin.data_ptr(), rows.data_ptr(), rows.numel(),
                  B, T, 0)
    side = m._side_stream_ptr(ids.device)
    # the two option sets: the plain full backward, and the embedding-only one from row_lo
    opts = BwdOpts(flags, 0, None, STAGE_CB(0), None, side) if full else BwdOpts(flags | Qm.BWD_EMBED_ONLY, row_lo,
                                                                                None, STAGE_CB(0), None, side)
    check(lib.sd_qwen3_backward(C.byref(m._cdims), C.byref(m._cparams), C.byref(cg), C.byref(batch), acts.data_ptr(),
                                acts.numel(), dlogits.data_ptr(), scratch.data_ptr(), sbytes, C.byref(opts), _stream()),
          "sd_qwen3_backward")
    torch.cuda.synchronize()


def _head_rows(m, name, flat):
    o, n, shape = m._slices[name]
    return flat[o:o + n].view(shape)


@pytest.mark.parametrize("case", ["tiny_tied", "tiny_untied", "real_depth2"])
def test_embed_rows_runner_contract(sda, case):
    from speech_distill_amd import ops
    from speech_distill_amd import qwen3 as Qm
    if case == "real_depth2":
        dims, lo, B, T = sda.Qwen3Dims(159488, 1024, 3072, 2, 16, 8), 159488 - 8220, 2, 512
    else:
        dims, lo, B, T = sda.Qwen3Dims(520, 128, 192, 2, 4, 2, tie_word_embeddings=case == "tiny_tied"), 452, 3, 70
    assert lo % 8 == 4
    m = _model(sda, dims, seed=4)
    V = dims.vocab_size
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(lo - 200, V, (B, T), generator=g)
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T // 2:] = 0
    lab = ids.clone()
    lab[am == 0] = -100
    ids, am, lab = to_dev(ids), to_dev(am), to_dev(lab)
    rows, _ = ops.loss_rows(lab, right_padded=(am,))
    dlog = (torch.randn(rows.numel(), V, generator=g) * 1e-2).bfloat16().to(dev())
    heads = ["model.embed_tokens.weight"] + ([] if dims.tie_word_embeddings else ["lm_head.weight"])
    sentinel = torch.full_like(m.flat, 0.375)
    g1 = sentinel.clone()
    ops.prof_begin()
    _run(sda, m, ids, am, rows, dlog, lo, Qm.SAVE_ALL, False, g1)
    prof = ops.prof_end()
    # nothing but rows [lo, V) of the embedding / lm_head changed
    changed = (g1.view(torch.int16) != sentinel.view(torch.int16))
    allowed = torch.zeros_like(changed)
    for n in heads:
        o, cnt, _ = m._slices[n]
        allowed[o + lo * dims.hidden_size:o + cnt] = True
    assert not bool((changed & ~allowed).any()), "a gradient byte outside rows [row_lo, V) was written"
    # the weight-gradient GEMM work is the lm_head dW of the new rows and nothing else
    tn_work = prof["gemm_tn"][1]
    want = 2.0 * (V - lo) * dims.hidden_size * rows.numel()
    record("stage1_dw_work", case=case, gemm_tn=tn_work, want=want)
    assert abs(tn_work - want) <= 1e-9 * want, (tn_work, want)
    # the same rows from the full backward on the same inputs
    gf = torch.zeros_like(m.flat)
    _run(sda, m, ids, am, rows, dlog, lo, Qm.SAVE_ALL, False, gf, full=True)
    for n in heads:
        check_close(f"stage1_vs_full_{case}_{n}", _head_rows(m, n, g1)[lo:].float().cpu(),
                    _head_rows(m, n, gf)[lo:].double().cpu(), 2e-2, 1e-2)
    # recompute == save-all, bit for bit; accumulate adds
    g2 = sentinel.clone()
    _run(sda, m, ids, am, rows, dlog, lo, Qm.SAVE_LAYER_INPUTS, False, g2)
    assert torch.equal(g1.view(torch.int16), g2.view(torch.int16))
    _run(sda, m, ids, am, rows, dlog, lo, Qm.SAVE_ALL, True, g2)
    for n in heads:
        a, b = _head_rows(m, n, g2), _head_rows(m, n, g1)
        assert torch.equal(a[:lo].view(torch.int16), b[:lo].view(torch.int16))
        check_close(f"stage1_accumulate_{case}_{n}", a[lo:].float().cpu(), 2 * b[lo:].double().cpu(), 2e-2)


# ---------------------------------------------------------------------------------------------- G6 step
@pytest.mark.parametrize("variant", ["tied", "untied"])
def test_hip_stage1_steps_vs_fixture(sda, variant):
    from oracle import qwen3 as Q
    from speech_distill_amd.optim import FlatAdamW
    from speech_distill_amd.stage1 import freeze_model_weights
    z = load_golden("g6_stage1.npz")
    p = variant + "_"
    tied = variant == "tied"
    shp = [int(x) for x in z[p + "shape"]]
    w = {k: v.bfloat16().float() for k, v in Q.init_weights(Q.Qwen3Shape(*shp, tie_word_embeddings=tied),
                                                             seed=int(z[p + "seed"])).items()}
    m = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(*shp, tie_word_embeddings=tied), device=dev(), init_std=0)
    m.load_hf_state_dict(w)
    freeze_model_weights(m, int(z[p + "num_new_tokens"]))
    lo = m.stage1_row_lo
    names = ["model.embed_tokens.weight"] + ([] if tied else ["lm_head.weight"])
    assert sorted(n for n, q in m.named_parameters() if q.requires_grad) == sorted(z[p + "trainable"].tolist())
    body0 = torch.cat([m.flat[a:b] for a, b in m.layer_ranges + [m.norm_range]]).clone()
    init = {n: m._params[n].detach().clone() for n in names}
    opt = FlatAdamW(m, lr=1e-3, weight_decay=0.01, clip=1.0)
    for step in range(2):
        n_items = int(z[p + f"step{step}_num_items"])
        for k in (2 * step, 2 * step + 1):
            ids, am, lab = (to_dev(torch.from_numpy(z[p + f"mb{k}_{key}"])) for key in ("input_ids", "attention_mask", "labels"))
            out = m(input_ids=ids, attention_mask=am, labels=lab, num_items_in_batch=n_items, stage1_inplace_grad=True)
            out.loss.backward()
            want = float(z[p + "losses"][k])
            record("stage1_g6_loss", variant=variant, got=float(out.loss), ref=want)
            assert abs(float(out.loss) - want) <= 2e-2 * abs(want)
        for n in names:
            gr = m._params[n].grad
            assert gr[:lo].eq(0).all()
            ref = torch.from_numpy(z[p + f"step{step}_grad_{n.split('.')[-2]}"])
            gn, rn = float(gr[lo:].double().norm()), float(ref.double().norm())
            c = _cos(gr[lo:], ref)
            record("stage1_g6_grad", variant=variant, step=step, param=n, gnorm=gn, rnorm=rn, cos=c)
            assert abs(gn - rn) <= 6e-2 * rn and c >= 0.99, (n, gn, rn, c)
        opt.step()
        m.zero_grad()
    body1 = torch.cat([m.flat[a:b] for a, b in m.layer_ranges + [m.norm_range]])
    assert torch.equal(body0.view(torch.int16), body1.view(torch.int16)), "a frozen decoder weight changed"
    for n in names:
        # old rows: exactly what torch.optim.AdamW does to the same bf16 tensor with their (zero) gradient
        t = init[n].clone().requires_grad_(True)
        ta = torch.optim.AdamW([t], lr=1e-3, weight_decay=0.01)
        for _ in range(2):
            t.grad = torch.zeros_like(t)
            ta.step()
        assert torch.equal(m._params[n].detach()[:lo].view(torch.int16), t.detach()[:lo].view(torch.int16))
        ref = torch.from_numpy(z[p + f"step1_param_{n.split('.')[-2]}"])
        c = _cos(m._params[n].detach()[lo:].float().cpu() - init[n][lo:].float().cpu(), ref - init[n][lo:].float().cpu())
        record("stage1_g6_update_cos", variant=variant, param=n, cos=c)
        assert c >= 0.9, (n, c)


# ---------------------------------------------------------------------------------------------- CLI end to end
def test_stage1_cli_tiny_run(sda, tmp_path):
    log = tmp_path / "log.json"
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "stage1.py"), "--random_init", "--tiny",
           "--synthetic_samples", "48", "--max_steps", "6", "--max_seq_length", "256", "--num_new_tokens", "132",
           "--batch_size", "2", "--gradient_accumulation_steps", "2", "--logging_steps", "1", "--warmup_steps", "0",
           "--save_steps", "1000", "--output_dir", str(tmp_path / "out"), "--log_json", str(log)]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads(log.read_text())
    losses = [e["loss"] for e in d["log_history"] if "loss" in e]
    assert d["global_step"] == 6 and len(losses) == 6 and all(np.isfinite(losses)), d["log_history"]
    assert d["optimizer"] == "FlatAdamW" and d["stage1_row_lo"] == 900
    assert d["trainable"] == ["model.embed_tokens.weight"]
    assert d["body_checksum"] == d["body_checksum_before"]
    assert os.path.isfile(tmp_path / "out" / "final_model" / "model.safetensors")
    assert any("tokens_per_second" in e for e in d["log_history"])
