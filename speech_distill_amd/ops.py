"""Tensor-level wrappers over the C ABI (one function per launcher in include/sd_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every function takes CUDA(HIP)
tensors, passes raw pointers + sizes + torch's current stream to libsd_hip.so and converts a
non-zero status to an exception.  CPU tensors are rejected -- there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import torch

from . import _lib
from ._lib import check, load_lib

BF16, F32 = 0, 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------- side streams
# HIP maps streams onto a few hardware queues (4 by default); two streams on one queue run strictly in turn.  Which
# streams alias depends on how many the process created before (torch pre-creates pools of 32; torch.distributed and
# RCCL add their own), so the side streams of the step are chosen by measurement: sd_streams_overlap runs a short
# busy-wait on one stream and checks that the other is not held up behind it.
_SIDE_STREAMS = {}  # (device index, role) -> torch.cuda.Stream
_ROLES_ACTIVE_TOGETHER = {"teacher": (), "dw": ("comm",), "comm": ("dw",), "h2d": ("teacher",)}  # besides the main stream


def streams_overlap(a, b, spin_us=200.0):
    """True when work on stream ``b`` executes while stream ``a`` is busy (they sit on different hardware queues)."""
    out = C.c_int(0)
    check(load_lib().sd_streams_overlap(a.cuda_stream, b.cuda_stream, spin_us, C.byref(out)), "sd_streams_overlap")
    return bool(out.value)


def concurrent_stream(device, role):
    """The process-wide side stream of ``role`` on ``device``: "teacher" (frozen teacher beside the student forward),
    "dw" (weight-gradient GEMMs beside the dX chain), "comm" (gradient all-reduce beside backward), "h2d" (the next
    accumulation window's batches, copied in while the optimizer step is still running: DistillationTrainer.get_batch_samples).  Picked once, by
    experiment, so that it overlaps the current (main) stream and the roles that are busy at the same time; the
    environment variable SD_STREAM_PICK=0 takes the first stream torch hands out instead."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), role)
    if key in _SIDE_STREAMS:
        return _SIDE_STREAMS[key]
    with torch.cuda.device(device):
        main = torch.cuda.current_stream()
        prio = int(os.environ.get("SD_STREAM_PRIORITY_" + role.upper(), "0"))  # measurement: -1 = high

        def new_stream():
            return torch.cuda.Stream(priority=prio)
        chosen = new_stream()
        if os.environ.get("SD_STREAM_PICK", "1") != "0":
            peers = [_SIDE_STREAMS[(key[0], r)] for r in _ROLES_ACTIVE_TOGETHER[role] if (key[0], r) in _SIDE_STREAMS]
            fallback = None
            for _ in range(32):  # torch hands out its pool of 32 streams round-robin
                if streams_overlap(main, chosen):
                    if all(streams_overlap(p, chosen) for p in peers):
                        break
                    fallback = fallback or chosen
                chosen = new_stream()
            else:
                chosen = fallback or chosen  # no stream clear of every peer: at least clear of the main stream
    _SIDE_STREAMS[key] = chosen
    return chosen


def _need(t, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"speech_distill_amd: {name} must be a GPU tensor (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _dt(t):
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported dtype {t.dtype} (bf16 or fp32)")


# ------------------------------------------------------------------------------------------ GEMM
def gemm(a, b, trans_a=False, trans_b=False, residual=None, out=None, split_k=False):
    """C = op(a) @ op(b) (+ residual).  trans_a: a is stored [K,M]; trans_b=False: b is [N,K]."""
    _need(a, torch.bfloat16, "a"), _need(b, torch.bfloat16, "b")
    K, M = (a.shape if trans_a else a.shape[::-1])
    if trans_b:
        Kb, N = b.shape
    else:
        N, Kb = b.shape
    if Kb != K:
        raise ValueError(f"gemm: contraction mismatch {K} vs {Kb}")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    r = None if residual is None else _need(residual, torch.bfloat16, "residual")
    if split_k:
        lib = load_lib()
        nb = lib.sd_gemm_splitk_workspace_bytes(M, N, K)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=a.device)
        check(lib.sd_gemm_bf16_splitk(a.data_ptr(), b.data_ptr(), out.data_ptr(), _p(r), M, N, K, a.stride(0), b.stride(0),
                                      out.stride(0), 0 if r is None else r.stride(0), int(trans_a), int(trans_b),
                                      ws.data_ptr(), nb, _stream()), "sd_gemm_bf16_splitk")
        return out
    check(load_lib().sd_gemm_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), _p(r), M, N, K, a.stride(0), b.stride(0),
                                  out.stride(0), 0 if r is None else r.stride(0), int(trans_a), int(trans_b), _stream()),
          "sd_gemm_bf16")
    return out


# ------------------------------------------------------------------------------------- elementwise
def rmsnorm_fwd(x, w, eps=1e-6):
    _need(x, torch.bfloat16, "x"), _need(w, torch.bfloat16, "w")
    M, H = x.shape
    y = torch.empty_like(x)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    check(load_lib().sd_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), M, H, eps, _stream()),
          "sd_rmsnorm_fwd")
    return y, rstd


def rmsnorm_bwd(dy, x, w, rstd, dres=None, dw=None, accumulate=False):
    M, H = x.shape
    lib = load_lib()
    ws = torch.empty(lib.sd_rmsnorm_bwd_workspace_bytes(M, H), dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x)
    if dw is None:
        dw = torch.zeros_like(w)
    check(lib.sd_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), _p(dres), dx.data_ptr(),
                             dw.data_ptr(), int(accumulate), ws.data_ptr(), M, H, _stream()), "sd_rmsnorm_bwd")
    return dx, dw


def rope_tables(T, device, theta=1e6, d=128):
    """cos/sin [T,d] exactly as HF computes them (modeling_qwen3.py:113-137), rounded to bf16."""
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().to(torch.bfloat16).to(device), emb.sin().to(torch.bfloat16).to(device)


def qknorm_rope_fwd(qkv, q_gain, k_gain, cos, sin, T, Hq, Hkv, eps=1e-6):
    M = qkv.shape[0]
    out = torch.empty(M, (Hq + Hkv) * 128, dtype=torch.bfloat16, device=qkv.device)
    check(load_lib().sd_qknorm_rope_fwd(qkv.data_ptr(), q_gain.data_ptr(), k_gain.data_ptr(), cos.data_ptr(),
                                        sin.data_ptr(), out.data_ptr(), M, T, Hq, Hkv, eps, _stream()),
          "sd_qknorm_rope_fwd")
    return out


def qknorm_rope_bwd(dqk, qkv, q_gain, k_gain, cos, sin, T, Hq, Hkv, eps=1e-6):
    M = qkv.shape[0]
    lib = load_lib()
    ws = torch.empty(lib.sd_qknorm_rope_bwd_workspace_bytes(M, Hq, Hkv), dtype=torch.uint8, device=qkv.device)
    dqkv = torch.zeros_like(qkv)
    dqg, dkg = torch.zeros_like(q_gain), torch.zeros_like(k_gain)
    check(lib.sd_qknorm_rope_bwd(dqk.data_ptr(), qkv.data_ptr(), q_gain.data_ptr(), k_gain.data_ptr(), cos.data_ptr(),
                                 sin.data_ptr(), dqkv.data_ptr(), dqg.data_ptr(), dkg.data_ptr(), 0, ws.data_ptr(), M, T,
                                 Hq, Hkv, eps, _stream()), "sd_qknorm_rope_bwd")
    return dqkv, dqg, dkg


def swiglu_fwd(gu):
    M, I2 = gu.shape
    act = torch.empty(M, I2 // 2, dtype=torch.bfloat16, device=gu.device)
    check(load_lib().sd_swiglu_fwd(gu.data_ptr(), act.data_ptr(), M, I2 // 2, _stream()), "sd_swiglu_fwd")
    return act


def swiglu_bwd(dact, gu):
    M, I2 = gu.shape
    dgu = torch.empty_like(gu)
    check(load_lib().sd_swiglu_bwd(dact.data_ptr(), gu.data_ptr(), dgu.data_ptr(), M, I2 // 2, _stream()), "sd_swiglu_bwd")
    return dgu


def embedding_fwd(ids, E):
    M = ids.numel()
    V, H = E.shape
    x = torch.empty(M, H, dtype=torch.bfloat16, device=E.device)
    check(load_lib().sd_embedding_fwd(ids.data_ptr(), E.data_ptr(), x.data_ptr(), M, H, V, _stream()), "sd_embedding_fwd")
    return x


def embedding_bwd(ids, dx, dE, scale=1.0):
    V, H = dE.shape
    check(load_lib().sd_embedding_bwd(ids.data_ptr(), dx.data_ptr(), dE.data_ptr(), ids.numel(), H, V, float(scale),
                                      _stream()),
          "sd_embedding_bwd")
    return dE


def embedding_bwd_range(ids, dx, dE, row_lo, scale=1.0):
    """dE[id] += scale * sum of the dx rows carrying id, for ids >= row_lo only (rows below row_lo untouched)."""
    V, H = dE.shape
    check(load_lib().sd_embedding_bwd_range(ids.data_ptr(), dx.data_ptr(), dE.data_ptr(), ids.numel(), H, V, int(row_lo),
                                            float(scale), _stream()),
          "sd_embedding_bwd_range")
    return dE


# --------------------------------------------------------------------------------------- attention
def attn_fwd(q, k, v, B, T, Hq, Hkv, kv_len=None):
    """q [B*T, Hq*128], k/v [B*T, Hkv*128] (any row stride, unit column stride)."""
    M = B * T
    o = torch.empty(M, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, T, dtype=torch.float32, device=q.device)
    check(load_lib().sd_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), _p(kv_len),
                                 q.stride(0), k.stride(0), v.stride(0), o.stride(0), B, T, Hq, Hkv, 128, 128 ** -0.5,
                                 _stream()), "sd_attn_fwd")
    return o, lse


def attn_bwd(q, k, v, o, do, lse, B, T, Hq, Hkv, kv_len=None, delta=None):
    """o = None: `delta` already holds rowsum(dO * O) per (batch, head, token) (gemm_odx_delta)."""
    if o is None and delta is None:
        raise ValueError("attn_bwd: either o or a precomputed delta")
    if delta is None:
        delta = torch.empty_like(lse)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    check(load_lib().sd_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), _p(o), do.data_ptr(), lse.data_ptr(),
                                 delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _p(kv_len), q.stride(0),
                                 k.stride(0), v.stride(0), do.stride(0), dq.stride(0), dk.stride(0), dv.stride(0), B, T, Hq,
                                 Hkv, 128, 128 ** -0.5, _stream()), "sd_attn_bwd")
    return dq, dk, dv


def varlen_desc(cu_seqlens, max_seqlen=0, work=None):
    """include/sd_hip.h sd_varlen over a device int32 ``cu_seqlens`` [n+1] (the caller keeps the tensors alive)."""
    _need(cu_seqlens, torch.int32, "cu_seqlens")
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2:
        raise ValueError("cu_seqlens must be a 1-D tensor of n_seqs + 1 offsets")
    from ._lib import Varlen
    return Varlen(cu_seqlens.data_ptr(), cu_seqlens.numel() - 1, int(max_seqlen), _p(work))


def attn_fwd_varlen(q, k, v, cu_seqlens, Hq, Hkv, max_seqlen=0, o=None, lse=None):
    """Packed documents (sd_attn_fwd_varlen): q [M, Hq*128], k/v [M, Hkv*128] (any row stride, unit column stride), document
    s = rows [cu_seqlens[s], cu_seqlens[s+1]).  Returns o [M, Hq*128] and lse fp32 [Hq, M]; ``o`` / ``lse`` may be given
    (``o`` with any row stride)."""
    M = q.shape[0]
    if o is None:
        o = torch.empty(M, Hq * 128, dtype=torch.bfloat16, device=q.device)
    if lse is None:
        lse = torch.empty(Hq, M, dtype=torch.float32, device=q.device)
    desc = varlen_desc(cu_seqlens, max_seqlen)
    check(load_lib().sd_attn_fwd_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), C.byref(desc),
                                        q.stride(0), k.stride(0), v.stride(0), o.stride(0), M, Hq, Hkv, 128, 128 ** -0.5,
                                        _stream()), "sd_attn_fwd_varlen")
    return o, lse


def attn_bwd_varlen(q, k, v, o, do, lse, cu_seqlens, Hq, Hkv, max_seqlen=0, delta=None, dq=None, dk=None, dv=None):
    """Backward of ``attn_fwd_varlen`` (sd_attn_bwd_varlen); o = None: ``delta`` [Hq, M] already holds rowsum(dO * O).
    ``dq`` / ``dk`` / ``dv`` may be given (any row stride); only rows [0, M) of the head columns are written."""
    if o is None and delta is None:
        raise ValueError("attn_bwd_varlen: either o or a precomputed delta")
    M = q.shape[0]
    if o is not None and M > 1 and o.stride(0) != do.stride(0):
        raise ValueError("attn_bwd_varlen: o and do share one row stride (ldo)")
    if delta is None:
        delta = torch.empty_like(lse)
    dq = torch.zeros(M, Hq * 128, dtype=torch.bfloat16, device=q.device) if dq is None else dq
    dk = torch.zeros(M, Hkv * 128, dtype=torch.bfloat16, device=q.device) if dk is None else dk
    dv = torch.zeros(M, Hkv * 128, dtype=torch.bfloat16, device=q.device) if dv is None else dv
    desc = varlen_desc(cu_seqlens, max_seqlen)
    check(load_lib().sd_attn_bwd_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), _p(o), do.data_ptr(), lse.data_ptr(),
                                        delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), C.byref(desc),
                                        q.stride(0), k.stride(0), v.stride(0), do.stride(0), dq.stride(0), dk.stride(0),
                                        dv.stride(0), M, Hq, Hkv, 128, 128 ** -0.5, None, _stream()), "sd_attn_bwd_varlen")
    return dq, dk, dv


def packed_segments(position_ids):
    """Document boundaries of packed rows by HF's rule (transformers masking_utils.find_packed_sequence_indices): a new
    document wherever ``position_ids[b, t] != position_ids[b, t-1] + 1``, and at every row start (rows never share a
    document).  position_ids [B, T] (any device) -> (cu_seqlens int64 [n+1] on the host over the B*T flattened tokens,
    largest position, smallest position): ONE host read."""
    pos = position_ids.to(torch.int64)
    if pos.dim() != 2 or pos.numel() == 0:
        raise ValueError(f"position_ids must be [batch, seq_len], got {tuple(position_ids.shape)}")
    start = torch.ones_like(pos, dtype=torch.bool)
    start[:, 1:] = pos[:, 1:] != pos[:, :-1] + 1
    host = torch.cat([start.reshape(-1).to(torch.int64), pos.max().reshape(1), pos.min().reshape(1)]).cpu()
    M = pos.numel()
    starts = torch.nonzero(host[:M]).reshape(-1)
    return torch.cat([starts, torch.tensor([M])]), int(host[M]), int(host[M + 1])


# ------------------------------------------------------------------------------------ top-K / loss
def logsoftmax_topk(logits, k, vocab_size=None):
    """train.py:80-91: logits[..., :vocab] -> log_softmax -> topk(k) -> (fp16 values, int32 indices)."""
    _need(logits, None, "logits")
    lead = logits.shape[:-1]
    Vt = logits.shape[-1]
    V = Vt if vocab_size is None else min(int(vocab_size), Vt)
    if (Vt % 8) or (logits.data_ptr() % 16):
        # rows must start 16-byte aligned for the vector loads: take the truncated copy the
        # reference itself makes at train.py:82-83
        logits = logits[..., :V].contiguous()
        Vt = V
    rows = logits.numel() // Vt
    tv = torch.empty(*lead, k, dtype=torch.float16, device=logits.device)
    ti = torch.empty(*lead, k, dtype=torch.int32, device=logits.device)
    check(load_lib().sd_logsoftmax_topk(logits.data_ptr(), tv.data_ptr(), ti.data_ptr(), 0, rows, Vt, V, k, _dt(logits),
                                        _stream()), "sd_logsoftmax_topk")
    return tv, ti


def topk_tail(logits, top_i, temperature, vocab_size=None):
    """The teacher's mass outside its top-K at ``temperature`` (sd_topk_tail): logits [..., Vt] (the first ``vocab_size``
    columns count), top_i int32 [..., K] as ``logsoftmax_topk`` returned them for the same logits -> fp32 [...].  Summed
    directly over the non-members, so a tail of 1e-12 keeps its digits."""
    _need(logits, None, "logits")
    lead = logits.shape[:-1]
    Vt = logits.shape[-1]
    V = Vt if vocab_size is None else min(int(vocab_size), Vt)
    if (Vt % 8) or (logits.data_ptr() % 16):   # as logsoftmax_topk: rows must start 16-byte aligned
        logits = logits[..., :V].contiguous()
        Vt = V
    K = int(top_i.shape[-1])
    if tuple(top_i.shape[:-1]) != tuple(lead):
        raise ValueError(f"top_i {tuple(top_i.shape)} for logits {tuple(logits.shape)}: expected {tuple(lead) + (K,)}")
    top_i = _need(top_i.to(device=logits.device, dtype=torch.int32), torch.int32, "top_i")
    rows = logits.numel() // Vt
    tail = torch.empty(*lead, dtype=torch.float32, device=logits.device)
    if rows:
        check(load_lib().sd_topk_tail(logits.data_ptr(), top_i.data_ptr(), tail.data_ptr(), rows, Vt, V, K,
                                      float(temperature), _dt(logits), _stream()), "sd_topk_tail")
    return tail


def tail_from_logprobs(top_v):
    """The T = 1 fallback for a top-K teacher stored without its tail: clamp(1 - sum_k exp(v_k), 0, 1) in fp32, [..., K] ->
    [...].  The stored log-probs are fp16, so this is good to about 2e-4 absolute (0.21732 against a true 0.21715); at any
    other temperature the tail cannot be had from the K values and has to come from ``topk_tail`` / the extraction."""
    return (1.0 - top_v.to(torch.float32).exp().sum(-1)).clamp_(0.0, 1.0)


# The loss autograd functions below are declarations over one forward and one backward body.  Every C entry takes
#   <stem>_fwd<suffix>(student, *teacher, labels, *forward-only pointers, stats, out, *dims, *scalars, dtype, stream)
#   <stem>_bwd<suffix>(student, *teacher, labels, stats, out, grad_total, grad_logits, *dims, *scalars, dtype, stream)
def _loss_forward(ctx, stem, suffix, s, dt, labels, teacher, fwd_only, dims, scalars, inplace_grad, stats_dims, n_out=8,
                  zeros_without_rows=False):
    """``teacher``: the tensors of the teacher form (None where the form has none), ``fwd_only``: what only the forward
    reads (a speech mask, a divisor).  ``zeros_without_rows``: with dims[0] == 0 nothing is launched and the zeros returned
    are connected to autograd (the C entries refuse R <= 0; the loss of no row is 0 and so is its (empty) gradient)."""
    lib = load_lib()
    launch = not (zeros_without_rows and dims[0] == 0)
    ctx.cfg = (stem, suffix, dims, scalars, dt, bool(inplace_grad), launch)
    if launch:
        stats = torch.empty(getattr(lib, stem + "_stats_bytes")(*stats_dims), dtype=torch.uint8, device=s.device)
        out = torch.empty(n_out, dtype=torch.float32, device=s.device)
        name = f"{stem}_fwd{suffix}"
        check(getattr(lib, name)(s.data_ptr(), *map(_p, teacher), labels.data_ptr(), *map(_p, fwd_only), stats.data_ptr(),
                                 out.data_ptr(), *dims, *scalars, dt, _stream()), name)
    else:
        stats = out = torch.zeros(n_out, dtype=torch.float32, device=s.device)
    ctx.save_for_backward(s, labels, stats, out, *teacher)
    ctx.mark_non_differentiable(out)
    return out[0].clone(), out


def _loss_backward(ctx, g_total, n_inputs):
    """-> (the gradient of the logits, written over them if the forward was told so, None for every other input)."""
    s, labels, stats, out, *teacher = ctx.saved_tensors
    stem, suffix, dims, scalars, dt, inplace, launch = ctx.cfg
    grad = s if inplace else torch.empty_like(s)
    if launch:
        go = g_total.to(torch.float32).reshape(1).contiguous()
        name = f"{stem}_bwd{suffix}"
        check(getattr(load_lib(), name)(s.data_ptr(), *map(_p, teacher), labels.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                        go.data_ptr(), grad.data_ptr(), *dims, *scalars, dt, _stream()), name)
    return (grad,) + (None,) * (n_inputs - 1)


def _dense_teacher(s, teacher_logits):
    teacher_logits = _need(teacher_logits.to(s.dtype), None, "teacher_logits")
    if teacher_logits.shape != s.shape:
        raise ValueError(f"teacher_logits {tuple(teacher_logits.shape)} != student_logits {tuple(s.shape)}")
    return teacher_logits


def _topk_teacher(s, *arrays):
    """(top_v, top_i[, top_tail]) on the student's device as fp16, int32[, fp32] (distillation_loss.py:78-91 moves the
    pre-extracted arrays there)."""
    return tuple(a.to(device=s.device, dtype=d).contiguous() for a, d in zip(arrays, (torch.float16, torch.int32, torch.float32)))


def _kd_teacher(s, teacher_logits, top_v, top_i):
    """The forward KL takes either form -> ((teacher_logits, top_v, top_i) with None for the absent form, K)."""
    if teacher_logits is not None:
        return (_dense_teacher(s, teacher_logits), None, None), 0
    if top_v is not None and top_i is not None:
        return (None,) + _topk_teacher(s, top_v, top_i), top_v.shape[-1]
    raise ValueError("Either teacher_logits or top_k must be provided")  # distillation_loss.py:120


class KDLossFn(torch.autograd.Function):
    """DistillationLoss.forward + its backward on the HIP kernels (distillation_loss.py:14-128)."""

    @staticmethod
    def forward(ctx, student_logits, labels, teacher_logits, top_v, top_i, speech_mask, temperature, alpha, inplace_grad):
        s = _need(student_logits, None, "student_logits")
        B, T, V = s.shape
        dt = _dt(s)
        labels = _need(labels.to(torch.int64), torch.int64, "labels")
        teacher, K = _kd_teacher(s, teacher_logits, top_v, top_i)
        mask = None
        if speech_mask is not None:
            mask = (speech_mask.to(s.device) != 0).to(torch.uint8).contiguous()
        return _loss_forward(ctx, "sd_kdloss", "", s, dt, labels, teacher, (mask,), (B, T, V, K),
                             (float(temperature), float(alpha)), inplace_grad, (B, T))

    @staticmethod
    def backward(ctx, g_total, _g_out):
        return _loss_backward(ctx, g_total, 9)


def gemm_grouped_tn(pairs, accumulate_into=None):
    """[(dY [K,M], X [K,N]), ...] (at most 4, common K) -> [dY^T @ X [M,N], ...] in one persistent launch;
    accumulate_into: list of [M,N] tensors to add to in place."""
    from ._lib import GemmProblem
    n = len(pairs)
    probs = (GemmProblem * n)()
    outs = []
    K = pairs[0][0].shape[0]
    for i, (a, b) in enumerate(pairs):
        _need(a, torch.bfloat16, "dY"), _need(b, torch.bfloat16, "X")
        if a.shape[0] != K or b.shape[0] != K:
            raise ValueError("gemm_grouped_tn: every problem must have the same contraction length")
        c = (torch.empty(a.shape[1], b.shape[1], dtype=torch.bfloat16, device=a.device) if accumulate_into is None
             else accumulate_into[i])
        outs.append(c)
        probs[i] = GemmProblem(a.data_ptr(), b.data_ptr(), c.data_ptr(), a.stride(0), b.stride(0), c.stride(0), a.shape[1],
                               b.shape[1])
    check(load_lib().sd_gemm_grouped_tn(C.cast(probs, C.c_void_p), n, K, int(accumulate_into is not None), _stream()),
          "sd_gemm_grouped_tn")
    return outs


def gemm_swiglu_bwd(dy, wdown, gate_up):
    """d(gate|up) [M,2I] from dy [M,h], W_down [h,I] (torch layout [out=h, in=I]) and the forward's gate|up."""
    _need(dy, torch.bfloat16, "dy")
    M, H = dy.shape
    I = wdown.shape[1]
    out = torch.empty(M, 2 * I, dtype=torch.bfloat16, device=dy.device)
    check(load_lib().sd_gemm_swiglu_bwd(dy.data_ptr(), wdown.data_ptr(), gate_up.data_ptr(), out.data_ptr(), M, I, H,
                                        _stream()), "sd_gemm_swiglu_bwd")
    return out


def gemm_odx_delta(dy, wo, o, T, Hq):
    """d(attention output) [M, Hq*128] = dy [M,H] @ wo [H, Hq*128] and delta [M/T, Hq, T] = rowsum(d_ao * o) per head,
    the second in the GEMM's epilogue (sd_gemm_odx_delta)."""
    _need(dy, torch.bfloat16, "dy"), _need(wo, torch.bfloat16, "wo"), _need(o, torch.bfloat16, "o")
    M, H = dy.shape
    dao = torch.empty(M, Hq * 128, dtype=torch.bfloat16, device=dy.device)
    delta = torch.empty(M // T, Hq, T, dtype=torch.float32, device=dy.device)
    check(load_lib().sd_gemm_odx_delta(dy.data_ptr(), wo.data_ptr(), dao.data_ptr(), o.data_ptr(), o.stride(0),
                                       delta.data_ptr(), M, T, Hq, H, _stream()), "sd_gemm_odx_delta")
    return dao, delta


class KDLossRowsFn(torch.autograd.Function):
    """The same loss on rows the caller has already shifted and selected (distillation_loss.py:31-45 done by the
    caller): student_logits [R,V], row_labels [R], teacher_logits [R,V] or (top_v, top_i) [R,K]."""

    @staticmethod
    def forward(ctx, student_logits, row_labels, teacher_logits, top_v, top_i, temperature, alpha, inplace_grad):
        s = _need(student_logits, None, "student_logits")
        R, V = s.shape
        dt = _dt(s)
        row_labels = _need(row_labels.to(torch.int64), torch.int64, "row_labels")
        teacher, K = _kd_teacher(s, teacher_logits, top_v, top_i)
        return _loss_forward(ctx, "sd_kdloss", "_rows", s, dt, row_labels, teacher, (), (R, V, K),
                             (float(temperature), float(alpha)), inplace_grad, (R, 1))

    @staticmethod
    def backward(ctx, g_total, _g_out):
        return _loss_backward(ctx, g_total, 8)


# ------------------------------------------------------------------------------------------ the divergences
class Divergence(NamedTuple):
    """One row of the table: what a ``divergence`` name means to the kernels, the loss module and the trainer."""
    stem: str       # its C entries are <stem>_fwd_rows / <stem>_bwd_rows (forward_kl also has the shifted <stem>_fwd / _bwd)
    mode: object    # the SD_DIV_* of include/sd_hip.h that the entries take, None where they take none
    teacher: str    # the teacher form: "dense" logits, a "topk" teacher, "topk_tail" (with its tail), or "either"
    beta01: bool    # beta must lie in (0, 1)
    dense: str      # the divergence that takes the dense teacher distribution where this one takes a top-K teacher


DIVERGENCE_TABLE = {
    "forward_kl":      Divergence("sd_kdloss", None, "either", False, "forward_kl"),   # KDLossFn / KDLossRowsFn
    "reverse_kl":      Divergence("sd_gjsd", 1, "dense", False, "reverse_kl"),         # GJSDLossRowsFn
    "jsd":             Divergence("sd_gjsd", 2, "dense", True, "jsd"),
    "jsd_topk":        Divergence("sd_gjsd_topk", None, "topk", True, "jsd"),          # GJSDTopKLossRowsFn
    "forward_kl_tail": Divergence("sd_gjsd_tail", 0, "topk_tail", False, "forward_kl"),  # GJSDTailLossRowsFn
    "reverse_kl_tail": Divergence("sd_gjsd_tail", 1, "topk_tail", False, "reverse_kl"),
    "jsd_tail":        Divergence("sd_gjsd_tail", 2, "topk_tail", True, "jsd"),
}
ALL_DIVERGENCES = tuple(DIVERGENCE_TABLE)
DIVERGENCES = {n: d.mode for n, d in DIVERGENCE_TABLE.items() if d.stem == "sd_gjsd"}            # dense reverse KL / JSD
TOPK_DIVERGENCE, = (n for n, d in DIVERGENCE_TABLE.items() if d.stem == "sd_gjsd_topk")         # the jsd on a top-K teacher
TAIL_DIVERGENCES = {n: d.mode for n, d in DIVERGENCE_TABLE.items() if d.stem == "sd_gjsd_tail"}  # top-K teacher + tail bucket


def check_divergence(divergence, beta):
    """ValueError for a divergence the loss does not know, or a ``jsd`` / ``jsd_topk`` / ``jsd_tail`` whose beta is outside
    (0, 1) (NaN included): the jsd formula tends to 0 at both ends, TRL's beta = 0 / 1 are ``forward_kl`` / ``reverse_kl``."""
    if divergence not in DIVERGENCE_TABLE:
        raise ValueError(f"unknown divergence {divergence!r}: one of " + ", ".join(repr(d) for d in ALL_DIVERGENCES))
    if DIVERGENCE_TABLE[divergence].beta01 and not 0.0 < float(beta) < 1.0:
        raise ValueError(f"divergence={divergence!r} needs 0 < beta < 1, got {beta!r} (beta = 0 is 'forward_kl', beta = 1 is "
                         "'reverse_kl')")


def takes_topk_teacher(divergence):
    """The divergence is defined on a top-K teacher only (``jsd_topk`` and the ``_tail`` names)."""
    return DIVERGENCE_TABLE[divergence].teacher in ("topk", "topk_tail")


def takes_dense_teacher(divergence):
    """The divergence is defined on the dense teacher distribution only (``reverse_kl``, ``jsd``)."""
    return DIVERGENCE_TABLE[divergence].teacher == "dense"


def dense_name(divergence):
    """The divergence that takes the dense teacher distribution where ``divergence`` takes a top-K teacher."""
    return DIVERGENCE_TABLE[divergence].dense


class GJSDLossRowsFn(torch.autograd.Function):
    """Reverse KL / beta-skewed Jensen-Shannon distillation loss (sd_gjsd_*_rows) on rows the caller has already shifted
    and selected: student_logits [R,V], row_labels [R], dense teacher_logits [R,V]; ``divergence`` "reverse_kl" or "jsd".
    Returns (total, out fp32[8] = total, task, distill, teacher, N, N, 0, 0).  R == 0 (a batch without a loss row) launches
    nothing and returns zeros that are connected to autograd, as a batch whose rows are all masked does."""

    @staticmethod
    def forward(ctx, student_logits, row_labels, teacher_logits, temperature, alpha, beta, divergence, inplace_grad):
        check_divergence(divergence, beta)
        if divergence not in DIVERGENCES:
            raise ValueError("GJSDLossRowsFn computes 'reverse_kl' and 'jsd'; 'forward_kl' is KDLossRowsFn")
        if teacher_logits is None:
            raise ValueError(f"divergence={divergence!r} needs dense teacher_logits")
        s = _need(student_logits, None, "student_logits")
        R, V = s.shape
        dt = _dt(s)
        row_labels = _need(row_labels.to(torch.int64), torch.int64, "row_labels")
        return _loss_forward(ctx, "sd_gjsd", "_rows", s, dt, row_labels, (_dense_teacher(s, teacher_logits),), (), (R, V),
                             (float(temperature), float(alpha), float(beta), DIVERGENCES[divergence]), inplace_grad, (R,),
                             zeros_without_rows=True)

    @staticmethod
    def backward(ctx, g_total, _g_out):
        return _loss_backward(ctx, g_total, 8)


class GJSDTopKLossRowsFn(torch.autograd.Function):
    """The beta-skewed Jensen-Shannon loss against a top-K teacher (sd_gjsd_topk_*_rows) on rows the caller has already
    shifted and selected: student_logits [R,V], row_labels [R], (top_v fp16, top_i int32) [R,K] as ``logsoftmax_topk`` or
    the offline extraction writes them.  The teacher's K entries are renormalised at T and scattered to a distribution P
    over the vocabulary (duplicates sum); the divergence is "jsd" against P.  An entry with an index outside [0, V) or a
    value that is not finite is ignored; a row without a usable entry is a masked row.
    Returns (total, out fp32[8] = total, task, distill, teacher, N, n_hits, 0, 0).  R == 0 launches nothing and returns
    zeros that are connected to autograd."""

    @staticmethod
    def forward(ctx, student_logits, row_labels, top_v, top_i, temperature, alpha, beta, inplace_grad):
        check_divergence(TOPK_DIVERGENCE, beta)
        if top_v is None or top_i is None:
            raise ValueError(f"divergence={TOPK_DIVERGENCE!r} needs a top-K teacher (teacher_top_k_v, teacher_top_k_i)")
        s = _need(student_logits, None, "student_logits")
        R, V = s.shape
        dt = _dt(s)
        row_labels = _need(row_labels.to(torch.int64), torch.int64, "row_labels")
        K = int(top_v.shape[-1])
        if tuple(top_v.shape) != (R, K) or tuple(top_i.shape) != (R, K):
            raise ValueError(f"top-K teacher {tuple(top_v.shape)} / {tuple(top_i.shape)} for {R} rows: expected [R, K] twice")
        return _loss_forward(ctx, "sd_gjsd_topk", "_rows", s, dt, row_labels, _topk_teacher(s, top_v, top_i), (), (R, V, K),
                             (float(temperature), float(alpha), float(beta)), inplace_grad, (R,), zeros_without_rows=True)

    @staticmethod
    def backward(ctx, g_total, _g_out):
        return _loss_backward(ctx, g_total, 8)


class GJSDTailLossRowsFn(torch.autograd.Function):
    """Forward KL, reverse KL or the beta-skewed Jensen-Shannon loss against a top-K teacher WITH A TAIL BUCKET
    (sd_gjsd_tail_*_rows; ``divergence`` one of ``TAIL_DIVERGENCES``) on rows the caller has already shifted and selected:
    student_logits [R,V], row_labels [R], (top_v fp16, top_i int32) [R,K], top_tail fp32 [R] the teacher's mass outside
    its top-K at ``temperature`` (``topk_tail``).  Teacher and student are compared over K + 1 outcomes, the K indices
    and "anything else", so every divergence is finite.  A row whose tail is NaN, negative or >= 1 is a masked row, as
    is a row without a usable entry.  Needs K < V.
    Returns (total, out fp32[8] = total, task, distill, teacher, N, n_hits, 0, 0).  R == 0 launches nothing and returns
    zeros that are connected to autograd."""

    @staticmethod
    def forward(ctx, student_logits, row_labels, top_v, top_i, top_tail, temperature, alpha, beta, divergence, inplace_grad):
        if divergence not in TAIL_DIVERGENCES:
            raise ValueError(f"GJSDTailLossRowsFn: divergence {divergence!r} is not one of {sorted(TAIL_DIVERGENCES)}")
        check_divergence(divergence, beta)
        if top_v is None or top_i is None or top_tail is None:
            raise ValueError(f"divergence={divergence!r} needs a top-K teacher with its tail (teacher_top_k_v, "
                             "teacher_top_k_i, teacher_top_k_tail)")
        s = _need(student_logits, None, "student_logits")
        R, V = s.shape
        dt = _dt(s)
        row_labels = _need(row_labels.to(torch.int64), torch.int64, "row_labels")
        K = int(top_v.shape[-1])
        if tuple(top_v.shape) != (R, K) or tuple(top_i.shape) != (R, K) or tuple(top_tail.shape) != (R,):
            raise ValueError(f"top-K teacher {tuple(top_v.shape)} / {tuple(top_i.shape)} / tail {tuple(top_tail.shape)} for "
                             f"{R} rows: expected [R, K] twice and [R]")
        return _loss_forward(ctx, "sd_gjsd_tail", "_rows", s, dt, row_labels, _topk_teacher(s, top_v, top_i, top_tail), (),
                             (R, V, K), (float(temperature), float(alpha), float(beta), TAIL_DIVERGENCES[divergence]),
                             inplace_grad, (R,), zeros_without_rows=True)

    @staticmethod
    def backward(ctx, g_total, _g_out):
        return _loss_backward(ctx, g_total, 10)


class CELossRowsFn(torch.autograd.Function):
    """Causal-LM cross-entropy on rows the caller already shifted and selected (Stage-1 loss: HF ForCausalLMLoss as the
    reference's SFTTrainer computes it): logits [R,V] bf16/fp32, row_labels [R] (-100 masks a row), divisor: fp32 [1] device
    tensor = num_items_in_batch (None = mean over valid rows).  Returns (loss, out fp32[4] = loss, sum, N, divisor)."""

    @staticmethod
    def forward(ctx, logits, row_labels, divisor, inplace_grad):
        s = _need(logits, None, "logits")
        R, V = s.shape
        dt = _dt(s)
        row_labels = _need(row_labels.to(torch.int64), torch.int64, "row_labels")
        if divisor is not None:
            divisor = _need(divisor.to(device=s.device, dtype=torch.float32).reshape(1), torch.float32, "divisor")
        return _loss_forward(ctx, "sd_celoss", "_rows", s, dt, row_labels, (), (divisor,), (R, V), (), inplace_grad, (R,), n_out=4)

    @staticmethod
    def backward(ctx, g_total, _g_out):
        return _loss_backward(ctx, g_total, 4)


def celoss_rows(logits, row_labels, divisor=None, inplace_grad=False):
    """-> (loss 0-d fp32, out fp32[4]); differentiable w.r.t. ``logits`` (see CELossRowsFn)."""
    return CELossRowsFn.apply(logits, row_labels, divisor, inplace_grad)


def left_padded(attention_mask):
    """0-d bool tensor: some row has a 1 after a 0, i.e. the mask is not a valid-prefix (right-padded) mask."""
    am = attention_mask != 0
    return (am[:, 1:] & ~am[:, :-1]).any()


def loss_rows(labels, speech_mask=None, right_padded=()):
    """Flat indices b*T+t of the rows the loss reads, and the label each one predicts: position t < T-1 whose
    NEXT label is not -100 (and whose next mask bit is set) -- distillation_loss.py:31-45.  One host read (the
    row count sizes the lm_head GEMMs); ``right_padded``: attention masks to validate in that same read -- raises
    ValueError if one of them is not a valid-prefix mask (see HipQwen3ForCausalLM.forward)."""
    B, T = labels.shape
    masks = [m for m in right_padded if m is not None]
    # every mask is indexed as [B, T] with the LABELS' B and T (the collator pads teacher and student separately,
    # data.py:219-278: a teacher mask of another length is not this batch's grid)
    for what, m in [("attention mask", m) for m in masks] + ([("speech_token_mask", speech_mask)] if speech_mask is not None else []):
        if tuple(m.shape) != (B, T):
            raise ValueError(f"loss_rows: {what} {tuple(m.shape)} != labels {(B, T)}")
    if labels.is_cuda and len(masks) <= 2:  # one launch (sd_loss_rows) + one 8-byte read
        def i64(t):  # masks: any dtype, non-zero = 1
            t = t.to(labels.device)
            return (t if t.dtype == torch.int64 else (t != 0).to(torch.int64)).contiguous()
        lab = labels.to(torch.int64).contiguous()  # labels keep their VALUES (token ids, -100) whatever the int dtype
        keep = [lab] + [i64(m) for m in masks] + ([i64(speech_mask)] if speech_mask is not None else [])
        rows = torch.empty(B * T, dtype=torch.int64, device=labels.device)
        row_labels = torch.empty(B * T, dtype=torch.int64, device=labels.device)
        meta = torch.empty(2, dtype=torch.int32, device=labels.device)
        check(load_lib().sd_loss_rows(lab.data_ptr(), _p(keep[-1] if speech_mask is not None else None),
                                      _p(keep[1] if masks else None), _p(keep[2] if len(masks) > 1 else None),
                                      rows.data_ptr(), row_labels.data_ptr(), meta.data_ptr(), B, T, _stream()), "sd_loss_rows")
        n_rows, bad = meta.tolist()
        if bad:
            raise ValueError("attention_mask is not right-padded (a 1 follows a 0): the HIP attention kernels take a "
                             "valid-prefix length per sequence, as ProcessedDataCollator produces (data.py:280-327)")
        return rows[:n_rows], row_labels[:n_rows]
    nxt = torch.full_like(labels, -100)
    nxt[:, :-1] = labels[:, 1:]
    valid = nxt != -100
    if speech_mask is not None:
        m = torch.zeros_like(valid)
        m[:, :-1] = speech_mask.to(labels.device)[:, 1:] != 0
        valid &= m
    flat = valid.reshape(-1)
    if labels.is_cuda:
        host = torch.stack([flat.sum()] + [left_padded(m.to(labels.device)).to(torch.int64) for m in masks]).tolist()
        if any(host[1:]):
            raise ValueError("attention_mask is not right-padded (a 1 follows a 0): the HIP attention kernels take a "
                             "valid-prefix length per sequence, as ProcessedDataCollator produces (data.py:280-327)")
        try:
            rows = torch.nonzero_static(flat, size=int(host[0])).reshape(-1)
        except (NotImplementedError, RuntimeError):
            rows = torch.nonzero(flat).reshape(-1)
    else:
        if any(bool(left_padded(m)) for m in masks):
            raise ValueError("attention_mask is not right-padded")
        rows = torch.nonzero(flat).reshape(-1)
    return rows, nxt.reshape(-1)[rows]


def packed_rows(labels, cu_seqlens, speech_mask=None, position_ids=None):
    """``loss_rows`` for packed documents (padding-free packing: ``labels`` holds M tokens, document s = the flat tokens
    ``[cu_seqlens[s], cu_seqlens[s+1])``): flat token m is a loss row iff m + 1 < M, m + 1 lies in the same document
    (the last token of a document predicts nothing, whatever the next document's first label), ``labels[m+1] != -100``
    and (with a mask) ``speech_mask[m+1] != 0``.  -> (rows, row_labels, longest document, largest position): the two
    numbers are what a ``qwen3.PackedBatch`` needs from the host, so a packed step has ONE host read (the 16 bytes of
    sd_packed_rows' meta).  ValueError for a ``cu_seqlens`` that does not rise from 0 to M, or a negative position."""
    M = labels.numel()
    cu = cu_seqlens
    if cu.dim() != 1 or cu.numel() < 2 or cu.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"packed_rows: cu_seqlens must be a 1-D integer tensor of n_seqs + 1 offsets, got {cu.dtype} "
                         f"{tuple(cu.shape)}")
    for what, t in (("speech_token_mask", speech_mask), ("position_ids", position_ids)):
        if t is not None and t.numel() != M:
            raise ValueError(f"packed_rows: {what} {tuple(t.shape)} does not hold the labels' {M} tokens")
    if M == 0:
        raise ValueError("packed_rows: empty batch")
    if labels.is_cuda:  # one launch (sd_packed_rows) + one 16-byte read
        dev = labels.device
        lab = labels.to(torch.int64).reshape(-1).contiguous()
        sm = None
        if speech_mask is not None:
            sm = speech_mask.to(dev).reshape(-1)
            sm = (sm if sm.dtype == torch.int64 else (sm != 0).to(torch.int64)).contiguous()
        pos = None if position_ids is None else position_ids.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        cu32 = cu.to(device=dev, dtype=torch.int32).contiguous()
        rows = torch.empty(M, dtype=torch.int64, device=dev)
        row_labels = torch.empty(M, dtype=torch.int64, device=dev)
        meta = torch.empty(4, dtype=torch.int32, device=dev)
        check(load_lib().sd_packed_rows(lab.data_ptr(), _p(sm), cu32.data_ptr(), cu32.numel() - 1, _p(pos), rows.data_ptr(),
                                        row_labels.data_ptr(), meta.data_ptr(), M, _stream()), "sd_packed_rows")
        n_rows, bad, longest, max_pos = meta.tolist()
        rows, row_labels = rows[:n_rows], row_labels[:n_rows]
    else:  # the rule, in torch
        lab = labels.to(torch.int64).reshape(-1)
        c = cu.to(torch.int64)
        bad = int(c[0] != 0 or c[-1] != M or bool((c[1:] < c[:-1]).any()))
        if position_ids is not None and bool((position_ids < 0).any()):
            bad |= 2
        longest = max_pos = 0
        rows = row_labels = lab[:0]
        if not bad:
            nxt = torch.full_like(lab, -100)
            nxt[:-1] = lab[1:]
            if speech_mask is not None:
                keep = torch.zeros(M, dtype=torch.bool)
                keep[:-1] = speech_mask.reshape(-1)[1:] != 0
                nxt[~keep] = -100
            last = c[1:][c[1:] > c[:-1]] - 1   # the last token of every non-empty document: its successor is another document's
            nxt[last] = -100
            rows = torch.nonzero(nxt != -100).reshape(-1)
            row_labels = nxt[rows]
            longest = int((c[1:] - c[:-1]).max())
            max_pos = 0 if position_ids is None else int(position_ids.max())
    if bad & 1:
        raise ValueError(f"cu_seqlens must rise from 0 to the token count {M} without decreasing")
    if bad & 2:
        raise ValueError("position_ids must be non-negative")
    return rows, row_labels, longest, max_pos


def colsum_reduce_batch(problems):
    """[(partials [nb, stride] fp32, out [H] bf16, H, accumulate), ...] (at most 8): out[c] (+)= sum_r partials[r, c] for
    every problem in ONE launch (sd_colsum_reduce_batch: a layer's four gain gradients)."""
    from ._lib import ColsumProblem
    n = len(problems)
    arr = (ColsumProblem * n)()
    for i, (part, out, H, acc) in enumerate(problems):
        _need(out, torch.bfloat16, "out")
        if not part.is_cuda or part.dtype != torch.float32 or part.dim() != 2 or part.stride(1) != 1:
            raise ValueError("partials: fp32 GPU matrix [nb, >= H] with unit column stride")
        arr[i] = ColsumProblem(part.data_ptr(), out.data_ptr(), part.shape[0], H, part.stride(0), int(acc))
    check(load_lib().sd_colsum_reduce_batch(C.cast(arr, C.c_void_p), n, _stream()), "sd_colsum_reduce_batch")


def rows_scatter(src, rows, M):
    src = _need(src, torch.bfloat16, "src")
    dst = torch.empty(M, src.shape[1], dtype=torch.bfloat16, device=src.device)
    check(load_lib().sd_rows_scatter(src.data_ptr(), rows.data_ptr(), dst.data_ptr(), src.shape[0], M, src.shape[1],
                                     _stream()), "sd_rows_scatter")
    return dst


# --------------------------------------------------------------------------------------- optimizer
def sumsq(x, out, partials=None):
    """out[0] += sum(x^2) (deterministic two-launch reduction).  ``partials``: fp32 scratch of SUMSQ_PARTIALS elements the
    caller owns (FlatAdamW keeps one); allocated per call when omitted, so concurrent calls never share state."""
    from ._lib import SUMSQ_PARTIALS
    if partials is None:
        partials = torch.empty(SUMSQ_PARTIALS, dtype=torch.float32, device=x.device)
    elif partials.dtype != torch.float32 or partials.numel() < SUMSQ_PARTIALS or not partials.is_cuda:
        raise ValueError(f"partials: fp32 GPU scratch of at least {SUMSQ_PARTIALS} elements")
    check(load_lib().sd_sumsq_bf16(x.data_ptr(), x.numel(), out.data_ptr(), partials.data_ptr(), _stream()),
          "sd_sumsq_bf16")


def adamw_(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_sumsq=None, max_norm=0.0):
    check(load_lib().sd_adamw_bf16(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2,
                                   eps, wd, step, _p(grad_sumsq), max_norm, _stream()), "sd_adamw_bf16")


def adamw_f32_shadow_(p, g, m, v, shadow, shadow_scaled, scale, lr, beta1, beta2, eps, wd, step, grad_sumsq=None,
                       max_norm=0.0):
    """AdamW on fp32 masters with a bf16 gradient; also writes shadow = bf16(p), shadow_scaled = bf16(scale p)."""
    check(load_lib().sd_adamw_f32_shadow(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), shadow.data_ptr(),
                                         shadow_scaled.data_ptr(), scale, p.numel(), lr, beta1, beta2, eps, wd, step,
                                         _p(grad_sumsq), max_norm, _stream()), "sd_adamw_f32_shadow")


# --------------------------------------------------------------------------------------- profiling
def prof_begin():
    check(load_lib().sd_prof_begin(), "sd_prof_begin")


def prof_end():
    """-> {kind: (total_ms, total_work, launches)} measured with HIP events on the launch stream."""
    from ._lib import KINDS
    n = len(KINDS)
    ms, work, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_int64 * n)()
    check(load_lib().sd_prof_end(ms, work, cnt, n), "sd_prof_end")
    return {KINDS[i]: (ms[i], work[i], cnt[i]) for i in range(n)}


def prof_symbols():
    """-> {kernel symbol: (total_ms, total_work, launches, kind)} of the last prof_end (see sd_prof_symbols)."""
    from ._lib import KINDS
    lib = load_lib()
    n = lib.sd_prof_symbols(None, 0)
    buf = C.create_string_buffer(int(n))
    lib.sd_prof_symbols(buf, n)
    out = {}
    for line in buf.value.decode().splitlines():
        sym, kind, ms, work, cnt = line.split("\t")
        out[sym] = (float(ms), float(work), int(cnt), KINDS[int(kind)] if int(kind) < len(KINDS) else "?")
    return out


def rmsnorm_bwd_from_splitk(a, b_kn, x, w, rstd, dres=None):
    """dx, dw of RMSNorm where dy = a @ b_kn is produced by a split-K GEMM whose fp32 slabs the norm kernel sums
    itself (sd_gemm_bf16_splitk_partial + sd_rmsnorm_bwd_slabs).  Returns (dx, dw, nsplit)."""
    lib = load_lib()
    M, K = a.shape
    N = b_kn.shape[1]
    nb = max(lib.sd_gemm_splitk_workspace_bytes(M, N, K), 16)
    ws = torch.empty(nb, dtype=torch.uint8, device=a.device)
    dy = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    nsp = C.c_int(0)
    check(lib.sd_gemm_bf16_splitk_partial(a.data_ptr(), b_kn.data_ptr(), dy.data_ptr(), M, N, K, a.stride(0), b_kn.stride(0),
                                          N, 0, 1, ws.data_ptr(), nb, C.byref(nsp), _stream()), "sd_gemm_bf16_splitk_partial")
    wsn = torch.empty(lib.sd_rmsnorm_bwd_workspace_bytes(M, N), dtype=torch.uint8, device=a.device)
    dx, dw = torch.empty_like(x), torch.zeros_like(w)
    if nsp.value > 1:
        check(lib.sd_rmsnorm_bwd_slabs(ws.data_ptr(), nsp.value, x.data_ptr(), w.data_ptr(), rstd.data_ptr(), _p(dres),
                                       dx.data_ptr(), dw.data_ptr(), 0, wsn.data_ptr(), M, N, 0, 0, _stream()),
              "sd_rmsnorm_bwd_slabs")
    else:
        check(lib.sd_rmsnorm_bwd2(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), _p(dres), dx.data_ptr(),
                                  dw.data_ptr(), 0, wsn.data_ptr(), M, N, 0, 0, _stream()), "sd_rmsnorm_bwd2")
    return dx, dw, nsp.value


# --------------------------------------------------------------------------------- fused forward GEMMs
def gemm_swiglu(x, wgu, save_gu=True):
    """act = silu(x Wg^T) * (x Wu^T) with wgu = [gate rows | up rows]; returns (act, gu or None)."""
    M, K = x.shape
    I = wgu.shape[0] // 2
    act = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)
    gu = torch.empty(M, 2 * I, dtype=torch.bfloat16, device=x.device) if save_gu else None
    check(load_lib().sd_gemm_swiglu(x.data_ptr(), wgu.data_ptr(), _p(gu), act.data_ptr(), M, I, K, _stream()), "sd_gemm_swiglu")
    return act, gu


# ---- weight-streaming GEMV for decode (include/sd_hip.h "weight-streaming GEMV"): M = batch <= 16
def _rows2d(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"speech_distill_amd: {name} must be a GPU tensor (no CPU fallback)")
    if t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1:
        raise TypeError(f"{name}: expected a 2-D bf16 tensor with unit column stride")
    return t


def gemv_bf16(x, w, residual=None, norm_gain=None, eps=1e-6, out=None, wide=False):
    """y [M,N] = xn [M,K] @ w[N,K]^T (+ residual), xn = x or RMSNorm(x; norm_gain, eps); 1 <= M <= 16.  x, w, residual and
    out may have strided rows.  The bits of y[m,n] depend on row m, weight row n and K only.  ``wide``: sd_gemv_wide_bf16
    (the MFMA form, 1 <= M <= 64, K % 32 == 0; another summation order, so other bits than the 16-row kernel)."""
    entry = "sd_gemv_wide_bf16" if wide else "sd_gemv_bf16"
    _rows2d(x, "x"), _rows2d(w, "w")
    M, K = x.shape
    N, Kw = w.shape
    if Kw != K:
        raise ValueError(f"gemv_bf16: contraction mismatch {K} vs {Kw}")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _rows2d(out, "out")
    if out.shape != (M, N) or (residual is not None and _rows2d(residual, "residual").shape != (M, N)):
        raise ValueError("gemv_bf16: out / residual must be [M,N]")
    if norm_gain is not None and _need(norm_gain, torch.bfloat16, "norm_gain").numel() != K:
        raise ValueError(f"norm_gain must hold K = {K} elements, got {norm_gain.numel()}")
    check(getattr(load_lib(), entry)(x.data_ptr(), w.data_ptr(), out.data_ptr(), _p(residual), _p(norm_gain), float(eps), M, N,
                                     K, x.stride(0), w.stride(0), out.stride(0),
                                     0 if residual is None else residual.stride(0), _stream()), entry)
    return out


def gemv_swiglu(x, wgu, norm_gain=None, eps=1e-6, wide=False):
    """act [M,I] = silu(xn Wg^T) * (xn Wu^T) with wgu = [gate rows | up rows] [2I,K]; 1 <= M <= 16.  Equals
    swiglu_fwd(gemv_bf16(x, wgu, norm_gain=...)) bit for bit.  ``wide``: sd_gemv_wide_swiglu (1 <= M <= 64), which equals
    swiglu_fwd(gemv_bf16(x, wgu, norm_gain=..., wide=True))."""
    entry = "sd_gemv_wide_swiglu" if wide else "sd_gemv_swiglu"
    _need(x, torch.bfloat16, "x"), _need(wgu, torch.bfloat16, "wgu")
    if x.dim() != 2 or wgu.dim() != 2:
        raise ValueError(f"gemv_swiglu: x must be [M,K] and wgu [2I,K], got {tuple(x.shape)} and {tuple(wgu.shape)}")
    M, K = x.shape
    I = wgu.shape[0] // 2
    if wgu.shape != (2 * I, K):
        raise ValueError(f"gemv_swiglu: wgu must be [2I,{K}], got {tuple(wgu.shape)}")
    if norm_gain is not None and _need(norm_gain, torch.bfloat16, "norm_gain").numel() != K:
        raise ValueError(f"norm_gain must hold K = {K} elements, got {norm_gain.numel()}")
    act = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)
    check(getattr(load_lib(), entry)(x.data_ptr(), wgu.data_ptr(), act.data_ptr(), _p(norm_gain), float(eps), M, I, K,
                                     _stream()), entry)
    return act


def gemm_qkv_rope(x, wqkv, q_gain, k_gain, cos, sin, T, Hq, Hkv, eps=1e-6):
    """raw q|k|v and RMS-normalised + RoPE-rotated q|k in one launch."""
    M, K = x.shape
    qkv = torch.empty(M, (Hq + 2 * Hkv) * 128, dtype=torch.bfloat16, device=x.device)
    qk = torch.empty(M, (Hq + Hkv) * 128, dtype=torch.bfloat16, device=x.device)
    check(load_lib().sd_gemm_qkv_rope(x.data_ptr(), wqkv.data_ptr(), qkv.data_ptr(), qk.data_ptr(), q_gain.data_ptr(),
                                      k_gain.data_ptr(), cos.data_ptr(), sin.data_ptr(), M, T, Hq, Hkv, K, eps, _stream()),
          "sd_gemm_qkv_rope")
    return qkv, qk


# ---- RMSNorm folded into the projection behind it (include/sd_hip.h "RMSNorm folded ..."; the frozen teacher)
def embedding_fwd_ssq(ids, E):
    ids = _need(ids, torch.int64, "ids").reshape(-1)
    V, H = E.shape
    x = torch.empty(ids.numel(), H, dtype=torch.bfloat16, device=E.device)
    ssq = torch.empty(H // 128, ids.numel(), dtype=torch.float32, device=E.device)  # tile-major
    check(load_lib().sd_embedding_fwd_ssq(ids.data_ptr(), _p(E), x.data_ptr(), ssq.data_ptr(), ids.numel(), H, V, _stream()),
          "sd_embedding_fwd_ssq")
    return x, ssq


def gemm_resid_ssq(a, w, residual):
    """C = a . w^T + residual and the per-128-column-tile sums of squares of C: ([M,N] bf16, [N/128,M] fp32 tile-major)."""
    M, K = a.shape
    N = w.shape[0]
    c = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    ssq = torch.empty(N // 128, M, dtype=torch.float32, device=a.device)
    check(load_lib().sd_gemm_bf16_ssq(_p(a), _p(w), c.data_ptr(), _p(residual), ssq.data_ptr(), M, N, K, a.stride(0),
                                      w.stride(0), N, residual.stride(0), _stream()), "sd_gemm_bf16_ssq")
    return c, ssq


def gemm_swiglu_rs(x, wgu_folded, ssq, eps=1e-6, save_gu=False):
    M, K = x.shape
    I = wgu_folded.shape[0] // 2
    act = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)
    gu = torch.empty(M, 2 * I, dtype=torch.bfloat16, device=x.device) if save_gu else None
    check(load_lib().sd_gemm_swiglu_rs(_p(x), _p(wgu_folded), _p(gu), act.data_ptr(), _p(ssq), eps, M, I, K, _stream()),
          "sd_gemm_swiglu_rs")
    return act, gu


def gemm_qkv_rope_rs(x, wqkv_folded, q_gain, k_gain, cos, sin, ssq, T, Hq, Hkv, eps=1e-6):
    M, K = x.shape
    qkv = torch.empty(M, (Hq + 2 * Hkv) * 128, dtype=torch.bfloat16, device=x.device)
    qk = torch.empty(M, (Hq + Hkv) * 128, dtype=torch.bfloat16, device=x.device)
    check(load_lib().sd_gemm_qkv_rope_rs(_p(x), _p(wqkv_folded), qkv.data_ptr(), qk.data_ptr(), _p(q_gain), _p(k_gain),
                                         _p(cos), _p(sin), _p(ssq), M, T, Hq, Hkv, K, eps, _stream()), "sd_gemm_qkv_rope_rs")
    return qkv, qk


# ---- MXFP8 frozen teacher (include/sd_hip.h "MXFP8 frozen teacher"): e4m3fn elements + one E8M0 scale byte per 32 along K
def mxfp8_quant(x, want_rstd=False, eps=1e-6):
    """bf16 [M,K] (rows may be strided) -> (q uint8 [M,K] holding e4m3fn, scale uint8 [M,K/32] holding E8M0[, rstd fp32 [M]])."""
    if not x.is_cuda:
        raise RuntimeError("speech_distill_amd: x must be a GPU tensor (no CPU fallback)")
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise TypeError("mxfp8_quant: expected a 2-D bf16 tensor with unit column stride")
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    s = torch.empty(M, K // 32, dtype=torch.uint8, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if want_rstd else None
    check(load_lib().sd_mxfp8_quant(x.data_ptr(), x.stride(0), q.data_ptr(), s.data_ptr(), _p(rstd), eps, M, K, _stream()),
          "sd_mxfp8_quant")
    return (q, s, rstd) if want_rstd else (q, s)


def gemm_mxfp8(a_q, a_scale, b_q, b_scale, rowscale=None, residual=None, out=None):
    """bf16 [M,N] = bf16(rowscale[m] * (A . B^T) + residual); A [M,K], B [N,K] as (e4m3 bytes, E8M0 scale bytes)."""
    for t, n in ((a_q, "a_q"), (a_scale, "a_scale"), (b_q, "b_q"), (b_scale, "b_scale")):
        _need(t, torch.uint8, n)
    M, K = a_q.shape
    N = b_q.shape[0]
    if b_q.shape[1] != K or tuple(a_scale.shape) != (M, K // 32) or tuple(b_scale.shape) != (N, K // 32):
        raise ValueError("gemm_mxfp8: operand / scale shapes do not match")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a_q.device)
    r = None if residual is None else _need(residual, torch.bfloat16, "residual")
    rs = None if rowscale is None else _need(rowscale, torch.float32, "rowscale")
    check(load_lib().sd_gemm_mxfp8(a_q.data_ptr(), a_scale.data_ptr(), b_q.data_ptr(), b_scale.data_ptr(), out.data_ptr(),
                                   _p(r), _p(rs), M, N, K, out.stride(0), 0 if r is None else r.stride(0), _stream()),
          "sd_gemm_mxfp8")
    return out


def gemm_mxfp8_swiglu(a_q, a_scale, wgu_q, wgu_scale, rowscale=None):
    """(act_q, act_scale): the MXFP8 image of bf16(silu(g) * u), g | u = bf16(rowscale * (A . Wgu^T)); no bf16 act."""
    for t, n in ((a_q, "a_q"), (a_scale, "a_scale"), (wgu_q, "wgu_q"), (wgu_scale, "wgu_scale")):
        _need(t, torch.uint8, n)
    M, K = a_q.shape
    I = wgu_q.shape[0] // 2
    if wgu_q.shape[1] != K or tuple(a_scale.shape) != (M, K // 32) or tuple(wgu_scale.shape) != (2 * I, K // 32):
        raise ValueError("gemm_mxfp8_swiglu: operand / scale shapes do not match")
    act_q = torch.empty(M, I, dtype=torch.uint8, device=a_q.device)
    act_s = torch.empty(M, I // 32, dtype=torch.uint8, device=a_q.device)
    rs = None if rowscale is None else _need(rowscale, torch.float32, "rowscale")
    check(load_lib().sd_gemm_mxfp8_swiglu(a_q.data_ptr(), a_scale.data_ptr(), wgu_q.data_ptr(), wgu_scale.data_ptr(), _p(rs),
                                          act_q.data_ptr(), act_s.data_ptr(), M, I, K, _stream()), "sd_gemm_mxfp8_swiglu")
    return act_q, act_s


# ---- weight-streaming GEMV over MXFP8 weights (include/sd_hip.h "the same GEMV over MXFP8 weights"): M = batch <= 16
# (wide=True: <= 64)
def _mx_weight(w_q, w_scale, name):
    _need(w_q, torch.uint8, name + "_q"), _need(w_scale, torch.uint8, name + "_scale")
    if w_q.dim() != 2 or tuple(w_scale.shape) != (w_q.shape[0], w_q.shape[1] // 32):
        raise ValueError(f"{name}: expected e4m3 bytes [N,K] and E8M0 bytes [N,K/32], got {tuple(w_q.shape)} and "
                         f"{tuple(w_scale.shape)}")


def gemv_mxfp8(x, w_q, w_scale, residual=None, norm=False, eps=1e-6, out=None, wide=False):
    """y [M,N] = bf16(rs[m] * (X^ . W^T) + residual): x bf16 [M,K] (quantised to MXFP8 inside the kernel, as
    ``mxfp8_quant`` would), W = (e4m3 bytes [N,K], E8M0 bytes [N,K/32]) as ``mxfp8_quant`` of a weight gives them;
    rs = that call's rstd when ``norm``, else 1; 1 <= M <= 16.  x, residual and out may have strided rows.  The bits of
    y[m,n] depend on row m, weight row n and K only.  ``wide``: sd_gemv_mxfp8_wide (1 <= M <= 64), whose rows have the
    same bits."""
    entry = "sd_gemv_mxfp8_wide" if wide else "sd_gemv_mxfp8"
    _rows2d(x, "x"), _mx_weight(w_q, w_scale, "w")
    M, K = x.shape
    N, Kw = w_q.shape
    if Kw != K:
        raise ValueError(f"gemv_mxfp8: contraction mismatch {K} vs {Kw}")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _rows2d(out, "out")
    if out.shape != (M, N) or (residual is not None and _rows2d(residual, "residual").shape != (M, N)):
        raise ValueError("gemv_mxfp8: out / residual must be [M,N]")
    check(getattr(load_lib(), entry)(x.data_ptr(), x.stride(0), w_q.data_ptr(), w_scale.data_ptr(), out.data_ptr(),
                                     out.stride(0), _p(residual), 0 if residual is None else residual.stride(0),
                                     1 if norm else 0, float(eps), M, N, K, _stream()), entry)
    return out


def gemv_mxfp8_swiglu(x, wgu_q, wgu_scale, norm=False, eps=1e-6, wide=False):
    """act bf16 [M,I] = silu(g) * u, g | u = bf16(rs * (X^ . Wgu^T)) with Wgu = [gate rows | up rows] [2I,K] in MXFP8;
    1 <= M <= 16.  Equals swiglu_fwd(gemv_mxfp8(x, wgu_q, wgu_scale, norm=...)) bit for bit.  ``wide``:
    sd_gemv_mxfp8_wide_swiglu (1 <= M <= 64), same bits."""
    entry = "sd_gemv_mxfp8_wide_swiglu" if wide else "sd_gemv_mxfp8_swiglu"
    _need(x, torch.bfloat16, "x"), _mx_weight(wgu_q, wgu_scale, "wgu")
    if x.dim() != 2 or wgu_q.shape[0] % 2 or wgu_q.shape[1] != x.shape[1]:
        raise ValueError(f"gemv_mxfp8_swiglu: x must be [M,K] and wgu_q [2I,K], got {tuple(x.shape)} and "
                         f"{tuple(wgu_q.shape)}")
    M, K = x.shape
    I = wgu_q.shape[0] // 2
    act = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)
    check(getattr(load_lib(), entry)(x.data_ptr(), wgu_q.data_ptr(), wgu_scale.data_ptr(), act.data_ptr(),
                                     1 if norm else 0, float(eps), M, I, K, _stream()), entry)
    return act


# ------------------------------------------------------------------------------------ KV-cache generation
def kvcache_store(qk, qkv, k_plane, v_plane, kv_len, B, T, Hq, Hkv):
    """Prefill sink (sd_kvcache_store): K of ``qk`` [B*T,(Hq+Hkv)*128] and V of ``qkv`` [B*T,(Hq+2Hkv)*128] -> slots
    t < kv_len[b] of the planes [B, cap, Hkv*128]."""
    _need(qk, torch.bfloat16, "qk"), _need(qkv, torch.bfloat16, "qkv")
    _need(k_plane, torch.bfloat16, "k_plane"), _need(v_plane, torch.bfloat16, "v_plane")
    check(load_lib().sd_kvcache_store(qk.data_ptr(), qkv.data_ptr(), k_plane.data_ptr(), v_plane.data_ptr(), _p(kv_len), B, T,
                                      k_plane.shape[1], Hq, Hkv, _stream()), "sd_kvcache_store")


def kvcache_store_at(qk, qkv, k_plane, v_plane, past, new_len, B, T, Hq, Hkv):
    """sd_kvcache_store_at: rows t < new_len[b] of a block of T tokens per sequence -> slots past[b] + t of the planes."""
    _need(qk, torch.bfloat16, "qk"), _need(qkv, torch.bfloat16, "qkv")
    _need(k_plane, torch.bfloat16, "k_plane"), _need(v_plane, torch.bfloat16, "v_plane")
    _need(past, torch.int32, "past"), _need(new_len, torch.int32, "new_len")
    check(load_lib().sd_kvcache_store_at(qk.data_ptr(), qkv.data_ptr(), k_plane.data_ptr(), v_plane.data_ptr(),
                                         past.data_ptr(), new_len.data_ptr(), B, T, k_plane.shape[1], Hq, Hkv, _stream()),
          "sd_kvcache_store_at")


def attn_extend(q, k_plane, v_plane, past, new_len, T, Hq, Hkv, want_lse=True):
    """sd_attn_extend: q [B*T, Hq*128] (any row stride), planes [B, cap, Hkv*128] that already hold the block's K / V at
    slots past[b] .. past[b] + new_len[b] - 1; past, new_len int32 [B] (device).  -> o [B*T, Hq*128] (, lse [B,Hq,T])."""
    _need(k_plane, torch.bfloat16, "k_plane"), _need(v_plane, torch.bfloat16, "v_plane")
    _need(past, torch.int32, "past"), _need(new_len, torch.int32, "new_len")
    if not q.is_cuda:
        raise RuntimeError("speech_distill_amd: q must be a GPU tensor (no CPU fallback)")
    B, cap = k_plane.shape[0], k_plane.shape[1]
    o = torch.empty(B * T, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, T, dtype=torch.float32, device=q.device) if want_lse else None
    check(load_lib().sd_attn_extend(q.data_ptr(), k_plane.data_ptr(), v_plane.data_ptr(), o.data_ptr(), _p(lse),
                                    past.data_ptr(), new_len.data_ptr(), q.stride(0), o.stride(0), B, T, cap, Hq, Hkv, 128,
                                    128 ** -0.5, _stream()), "sd_attn_extend")
    return (o, lse) if want_lse else o


def last_rows(kv_len, B, T, device=None):
    """int64 [B]: flat index b*T + clamp(kv_len[b], 1, T) - 1 of the last valid row of every right-padded sequence."""
    rows = torch.empty(B, dtype=torch.int64, device=kv_len.device if kv_len is not None else device)
    check(load_lib().sd_last_rows(_p(kv_len), rows.data_ptr(), B, T, _stream()), "sd_last_rows")
    return rows


def qknorm_rope_append(qkv, q_gain, k_gain, cos, sin, pos, k_plane, v_plane, Hq, Hkv, eps=1e-6):
    """Decode twin of qknorm_rope_fwd for one token per sequence at position pos[b] (int32, device): returns q
    [B,Hq*128]; K (normalised, rotated) and raw V go to slot pos[b] of the planes [B, cap, Hkv*128]."""
    _need(qkv, torch.bfloat16, "qkv"), _need(pos, torch.int32, "pos")
    _need(k_plane, torch.bfloat16, "k_plane"), _need(v_plane, torch.bfloat16, "v_plane")
    B, cap = qkv.shape[0], k_plane.shape[1]
    if cos.shape[0] < cap:
        raise ValueError(f"rope tables hold {cos.shape[0]} positions, the cache {cap}")
    q = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=qkv.device)
    check(load_lib().sd_qknorm_rope_append(qkv.data_ptr(), q_gain.data_ptr(), k_gain.data_ptr(), cos.data_ptr(),
                                           sin.data_ptr(), pos.data_ptr(), q.data_ptr(), k_plane.data_ptr(),
                                           v_plane.data_ptr(), B, cap, Hq, Hkv, eps, _stream()), "sd_qknorm_rope_append")
    return q


def attn_decode(q, k_plane, v_plane, lens, Hq, Hkv, max_len=None, len_add=0, want_lse=False, workspace=None):
    """Single-token attention over the cache planes [B, cap, Hkv*128]: q [B,Hq*128], lens int32 [B] (device); row b attends
    to keys [0, lens[b] + len_add).  max_len: host upper bound of those counts (default cap).  -> o [B,Hq*128] (, lse [B,Hq])."""
    _need(q, torch.bfloat16, "q"), _need(lens, torch.int32, "lens")
    _need(k_plane, torch.bfloat16, "k_plane"), _need(v_plane, torch.bfloat16, "v_plane")
    lib = load_lib()
    B, cap = q.shape[0], k_plane.shape[1]
    nb = lib.sd_attn_decode_workspace_bytes(B, Hq, cap)
    if workspace is None:
        workspace = torch.empty(max(nb, 16), dtype=torch.uint8, device=q.device)
    o = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, dtype=torch.float32, device=q.device) if want_lse else None
    check(lib.sd_attn_decode(q.data_ptr(), k_plane.data_ptr(), v_plane.data_ptr(), o.data_ptr(), _p(lse), lens.data_ptr(),
                             int(len_add), workspace.data_ptr(), workspace.numel(), B, cap,
                             cap if max_len is None else int(max_len), Hq, Hkv, 128, 128 ** -0.5, _stream()),
          "sd_attn_decode")
    return (o, lse) if want_lse else o


# ---- paged twins (soulxpodcast/engine/llm_engine.py:91): pool planes [n_pages, 256, Hkv*128], table int32 [B, max_pages]
def _paged_args(k_pool, v_pool, table):
    _need(k_pool, torch.bfloat16, "k_pool"), _need(v_pool, torch.bfloat16, "v_pool"), _need(table, torch.int32, "table")
    if k_pool.dim() != 3 or k_pool.shape[1] != 256 or v_pool.shape != k_pool.shape or table.dim() != 2:
        raise ValueError(f"pool planes must be [n_pages, 256, Hkv*128] and the table [B, max_pages], got "
                         f"{tuple(k_pool.shape)}, {tuple(v_pool.shape)}, {tuple(table.shape)}")
    return k_pool.data_ptr(), v_pool.data_ptr(), table.data_ptr(), table.shape[1], k_pool.shape[0]


def kvcache_store_paged(qk, qkv, k_pool, v_pool, table, kv_len, B, T, Hq, Hkv):
    """sd_kvcache_store_paged: ``kvcache_store`` through a page table; slot t of row b is row t & 255 of page
    table[b, t >> 8]."""
    _need(qk, torch.bfloat16, "qk"), _need(qkv, torch.bfloat16, "qkv")
    kp, vp, tp, max_pages, n_pages = _paged_args(k_pool, v_pool, table)
    check(load_lib().sd_kvcache_store_paged(qk.data_ptr(), qkv.data_ptr(), kp, vp, tp, max_pages, n_pages, _p(kv_len), B, T,
                                            Hq, Hkv, _stream()), "sd_kvcache_store_paged")


def kvcache_store_at_paged(qk, qkv, k_pool, v_pool, table, past, new_len, B, T, Hq, Hkv):
    """sd_kvcache_store_at_paged: ``kvcache_store_at`` through a page table."""
    _need(qk, torch.bfloat16, "qk"), _need(qkv, torch.bfloat16, "qkv")
    _need(past, torch.int32, "past"), _need(new_len, torch.int32, "new_len")
    kp, vp, tp, max_pages, n_pages = _paged_args(k_pool, v_pool, table)
    check(load_lib().sd_kvcache_store_at_paged(qk.data_ptr(), qkv.data_ptr(), kp, vp, tp, max_pages, n_pages,
                                               past.data_ptr(), new_len.data_ptr(), B, T, Hq, Hkv, _stream()),
          "sd_kvcache_store_at_paged")


def attn_extend_paged(q, k_pool, v_pool, table, past, new_len, T, Hq, Hkv, want_lse=True):
    """sd_attn_extend_paged: ``attn_extend`` over pool planes and a page table; the same bits."""
    _need(past, torch.int32, "past"), _need(new_len, torch.int32, "new_len")
    kp, vp, tp, max_pages, n_pages = _paged_args(k_pool, v_pool, table)
    if not q.is_cuda:
        raise RuntimeError("speech_distill_amd: q must be a GPU tensor (no CPU fallback)")
    B = table.shape[0]
    o = torch.empty(B * T, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, T, dtype=torch.float32, device=q.device) if want_lse else None
    check(load_lib().sd_attn_extend_paged(q.data_ptr(), kp, vp, tp, max_pages, n_pages, o.data_ptr(), _p(lse),
                                          past.data_ptr(), new_len.data_ptr(), q.stride(0), o.stride(0), B, T, Hq, Hkv, 128,
                                          128 ** -0.5, _stream()), "sd_attn_extend_paged")
    return (o, lse) if want_lse else o


def qknorm_rope_append_paged(qkv, q_gain, k_gain, cos, sin, pos, k_pool, v_pool, table, Hq, Hkv, eps=1e-6):
    """sd_qknorm_rope_append_paged: ``qknorm_rope_append`` whose K / V go to slot pos[b] through a page table."""
    _need(qkv, torch.bfloat16, "qkv"), _need(pos, torch.int32, "pos")
    kp, vp, tp, max_pages, n_pages = _paged_args(k_pool, v_pool, table)
    B = qkv.shape[0]
    if cos.shape[0] < max_pages * 256:
        raise ValueError(f"rope tables hold {cos.shape[0]} positions, the page table {max_pages * 256}")
    q = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=qkv.device)
    check(load_lib().sd_qknorm_rope_append_paged(qkv.data_ptr(), q_gain.data_ptr(), k_gain.data_ptr(), cos.data_ptr(),
                                                 sin.data_ptr(), pos.data_ptr(), q.data_ptr(), kp, vp, tp, max_pages,
                                                 n_pages, B, Hq, Hkv, eps, _stream()), "sd_qknorm_rope_append_paged")
    return q


def attn_decode_paged(q, k_pool, v_pool, table, lens, Hq, Hkv, max_len=None, len_add=0, want_lse=False, workspace=None):
    """sd_attn_decode_paged: ``attn_decode`` over pool planes and a page table; the same bits."""
    _need(q, torch.bfloat16, "q"), _need(lens, torch.int32, "lens")
    kp, vp, tp, max_pages, n_pages = _paged_args(k_pool, v_pool, table)
    lib = load_lib()
    B, cap = q.shape[0], max_pages * 256
    nb = lib.sd_attn_decode_workspace_bytes(B, Hq, cap)
    if workspace is None:
        workspace = torch.empty(max(nb, 16), dtype=torch.uint8, device=q.device)
    o = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, dtype=torch.float32, device=q.device) if want_lse else None
    check(lib.sd_attn_decode_paged(q.data_ptr(), kp, vp, tp, max_pages, n_pages, o.data_ptr(), _p(lse), lens.data_ptr(),
                                   int(len_add), workspace.data_ptr(), workspace.numel(), B,
                                   cap if max_len is None else int(max_len), Hq, Hkv, 128, 128 ** -0.5, _stream()),
          "sd_attn_decode_paged")
    return (o, lse) if want_lse else o


# ---- 8-bit (MXFP8) pages: planes = (k_data, k_scale, v_data, v_scale), data uint8 [n_pages, 256, Hkv*128] (e4m3 bytes),
# scale uint8 [n_pages, 256, Hkv*4] (E8M0, one per 32 elements); the page table as above
def _paged_mx_args(planes, table):
    kd, ks, vd, vs = planes
    for t, name in ((kd, "k_data"), (ks, "k_scale"), (vd, "v_data"), (vs, "v_scale")):
        _need(t, torch.uint8, name)
    _need(table, torch.int32, "table")
    if (kd.dim() != 3 or kd.shape[1] != 256 or kd.shape[2] % 128 or vd.shape != kd.shape or table.dim() != 2
            or ks.shape != (kd.shape[0], 256, kd.shape[2] // 32) or vs.shape != ks.shape):
        raise ValueError("8-bit pool planes must be data [n_pages, 256, Hkv*128] and scale [n_pages, 256, Hkv*4] for K and "
                         f"V and the table [B, max_pages], got {[tuple(t.shape) for t in planes]}, {tuple(table.shape)}")
    return (kd.data_ptr(), ks.data_ptr(), vd.data_ptr(), vs.data_ptr()), table.data_ptr(), table.shape[1], kd.shape[0]


def kvcache_store_paged_mx(qk, qkv, planes, table, kv_len, B, T, Hq, Hkv):
    """sd_kvcache_store_paged_mx: ``kvcache_store_paged`` whose rows are stored as MXFP8."""
    _need(qk, torch.bfloat16, "qk"), _need(qkv, torch.bfloat16, "qkv")
    pl, tp, max_pages, n_pages = _paged_mx_args(planes, table)
    check(load_lib().sd_kvcache_store_paged_mx(qk.data_ptr(), qkv.data_ptr(), *pl, tp, max_pages, n_pages, _p(kv_len), B, T,
                                               Hq, Hkv, _stream()), "sd_kvcache_store_paged_mx")


def kvcache_store_at_paged_mx(qk, qkv, planes, table, past, new_len, B, T, Hq, Hkv):
    """sd_kvcache_store_at_paged_mx: ``kvcache_store_at_paged`` whose rows are stored as MXFP8."""
    _need(qk, torch.bfloat16, "qk"), _need(qkv, torch.bfloat16, "qkv")
    _need(past, torch.int32, "past"), _need(new_len, torch.int32, "new_len")
    pl, tp, max_pages, n_pages = _paged_mx_args(planes, table)
    check(load_lib().sd_kvcache_store_at_paged_mx(qk.data_ptr(), qkv.data_ptr(), *pl, tp, max_pages, n_pages,
                                                  past.data_ptr(), new_len.data_ptr(), B, T, Hq, Hkv, _stream()),
          "sd_kvcache_store_at_paged_mx")


def qknorm_rope_append_paged_mx(qkv, q_gain, k_gain, cos, sin, pos, planes, table, Hq, Hkv, eps=1e-6):
    """sd_qknorm_rope_append_paged_mx: ``qknorm_rope_append_paged`` whose K / V are stored as MXFP8; q is the twin's."""
    _need(qkv, torch.bfloat16, "qkv"), _need(pos, torch.int32, "pos")
    pl, tp, max_pages, n_pages = _paged_mx_args(planes, table)
    B = qkv.shape[0]
    if cos.shape[0] < max_pages * 256:
        raise ValueError(f"rope tables hold {cos.shape[0]} positions, the page table {max_pages * 256}")
    q = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=qkv.device)
    check(load_lib().sd_qknorm_rope_append_paged_mx(qkv.data_ptr(), q_gain.data_ptr(), k_gain.data_ptr(), cos.data_ptr(),
                                                    sin.data_ptr(), pos.data_ptr(), q.data_ptr(), *pl, tp, max_pages,
                                                    n_pages, B, Hq, Hkv, eps, _stream()), "sd_qknorm_rope_append_paged_mx")
    return q


def attn_decode_paged_mx(q, planes, table, lens, Hq, Hkv, max_len=None, len_add=0, want_lse=False, workspace=None):
    """sd_attn_decode_paged_mx: ``attn_decode_paged`` over MXFP8 planes; the bits of the twin on the dequantised rows."""
    _need(q, torch.bfloat16, "q"), _need(lens, torch.int32, "lens")
    pl, tp, max_pages, n_pages = _paged_mx_args(planes, table)
    lib = load_lib()
    B, cap = q.shape[0], max_pages * 256
    nb = lib.sd_attn_decode_workspace_bytes(B, Hq, cap)
    if workspace is None:
        workspace = torch.empty(max(nb, 16), dtype=torch.uint8, device=q.device)
    o = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, dtype=torch.float32, device=q.device) if want_lse else None
    check(lib.sd_attn_decode_paged_mx(q.data_ptr(), *pl, tp, max_pages, n_pages, o.data_ptr(), _p(lse), lens.data_ptr(),
                                      int(len_add), workspace.data_ptr(), workspace.numel(), B,
                                      cap if max_len is None else int(max_len), Hq, Hkv, 128, 128 ** -0.5, _stream()),
          "sd_attn_decode_paged_mx")
    return (o, lse) if want_lse else o


# ---- decode attention for rows that share pages (a forked session): the twins' arguments and bits, a page read once
# for every group of ``attn_shared_group_rows(Hq, Hkv)`` consecutive rows that map it
def attn_shared_group_rows(Hq, Hkv):
    """sd_attn_shared_group_rows: rows per group of the shared decode attention (no GPU needed)."""
    r = load_lib().sd_attn_shared_group_rows(int(Hq), int(Hkv))
    check(min(r, 0), "sd_attn_shared_group_rows")
    return r


def attn_decode_shared_paged(q, k_pool, v_pool, table, lens, Hq, Hkv, max_len=None, len_add=0, want_lse=False,
                             workspace=None):
    """sd_attn_decode_shared_paged: ``attn_decode_paged`` with every physical page read once per group of rows."""
    _need(q, torch.bfloat16, "q"), _need(lens, torch.int32, "lens")
    kp, vp, tp, max_pages, n_pages = _paged_args(k_pool, v_pool, table)
    lib = load_lib()
    B, cap = q.shape[0], max_pages * 256
    nb = lib.sd_attn_decode_workspace_bytes(B, Hq, cap)
    if workspace is None:
        workspace = torch.empty(max(nb, 16), dtype=torch.uint8, device=q.device)
    o = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, dtype=torch.float32, device=q.device) if want_lse else None
    check(lib.sd_attn_decode_shared_paged(q.data_ptr(), kp, vp, tp, max_pages, n_pages, o.data_ptr(), _p(lse),
                                          lens.data_ptr(), int(len_add), workspace.data_ptr(), workspace.numel(), B,
                                          cap if max_len is None else int(max_len), Hq, Hkv, 128, 128 ** -0.5, _stream()),
          "sd_attn_decode_shared_paged")
    return (o, lse) if want_lse else o


def attn_decode_shared_paged_mx(q, planes, table, lens, Hq, Hkv, max_len=None, len_add=0, want_lse=False, workspace=None):
    """sd_attn_decode_shared_paged_mx: ``attn_decode_paged_mx`` with every physical page read once per group of rows."""
    _need(q, torch.bfloat16, "q"), _need(lens, torch.int32, "lens")
    pl, tp, max_pages, n_pages = _paged_mx_args(planes, table)
    lib = load_lib()
    B, cap = q.shape[0], max_pages * 256
    nb = lib.sd_attn_decode_workspace_bytes(B, Hq, cap)
    if workspace is None:
        workspace = torch.empty(max(nb, 16), dtype=torch.uint8, device=q.device)
    o = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, dtype=torch.float32, device=q.device) if want_lse else None
    check(lib.sd_attn_decode_shared_paged_mx(q.data_ptr(), *pl, tp, max_pages, n_pages, o.data_ptr(), _p(lse),
                                             lens.data_ptr(), int(len_add), workspace.data_ptr(), workspace.numel(), B,
                                             cap if max_len is None else int(max_len), Hq, Hkv, 128, 128 ** -0.5,
                                             _stream()), "sd_attn_decode_shared_paged_mx")
    return (o, lse) if want_lse else o


def attn_extend_paged_mx(q, planes, table, past, new_len, T, Hq, Hkv, want_lse=True):
    """sd_attn_extend_paged_mx: ``attn_extend_paged`` over MXFP8 planes; the bits of the twin on the dequantised rows."""
    _need(past, torch.int32, "past"), _need(new_len, torch.int32, "new_len")
    pl, tp, max_pages, n_pages = _paged_mx_args(planes, table)
    if not q.is_cuda:
        raise RuntimeError("speech_distill_amd: q must be a GPU tensor (no CPU fallback)")
    B = table.shape[0]
    o = torch.empty(B * T, Hq * 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, Hq, T, dtype=torch.float32, device=q.device) if want_lse else None
    check(load_lib().sd_attn_extend_paged_mx(q.data_ptr(), *pl, tp, max_pages, n_pages, o.data_ptr(), _p(lse),
                                             past.data_ptr(), new_len.data_ptr(), q.stride(0), o.stride(0), B, T, Hq, Hkv,
                                             128, 128 ** -0.5, _stream()), "sd_attn_extend_paged_mx")
    return (o, lse) if want_lse else o


def cache_step(qkv, q_gain, k_gain, cos, sin, pos, planes, Hq, Hkv, table=None, max_len=None, eps=1e-6, want_lse=False,
               workspace=None, tickets=None):
    """sd_cache_step: ``qknorm_rope_append*`` followed by ``attn_decode*(len_add=1)`` as ONE launch, with their bits.
    ``planes``: (k_plane, v_plane) [B, cap, Hkv*128] bf16 of a contiguous cache (no ``table``), (k_pool, v_pool) of bf16
    pages or (k_data, k_scale, v_data, v_scale) of MXFP8 pages with the page ``table`` int32 [B, max_pages].  pos int32 [B]
    (device); max_len: host upper bound of every pos + 1 (default cap).  ``tickets``: int32 [B, Hkv], zero at the call and
    zero again after it (default: fresh zeros).  -> o [B,Hq*128] (, lse [B,Hq]).
    One rule the pair does not have, and nothing here checks it: a slot that one row appends in this call must not be a
    visible key of ANOTHER row in the same call (rows that share a page may share only positions below both their pos) --
    the pair orders that store and that read by a kernel boundary, this launch does not."""
    _need(qkv, torch.bfloat16, "qkv"), _need(pos, torch.int32, "pos")
    lib = load_lib()
    B = qkv.shape[0]
    if table is None:
        k, v = planes
        _need(k, torch.bfloat16, "k_plane"), _need(v, torch.bfloat16, "v_plane")
        cap = k.shape[1]
        kv = _lib.KvPlanes(0, k.data_ptr(), v.data_ptr(), None, None, cap, None, 0, 0)
    elif len(planes) == 2:
        kp, vp, tp, max_pages, n_pages = _paged_args(planes[0], planes[1], table)
        cap = max_pages * 256
        kv = _lib.KvPlanes(1, kp, vp, None, None, 0, tp, max_pages, n_pages)
    else:
        (kd, ks, vd, vs), tp, max_pages, n_pages = _paged_mx_args(planes, table)
        cap = max_pages * 256
        kv = _lib.KvPlanes(2, kd, vd, ks, vs, 0, tp, max_pages, n_pages)
    if cos.shape[0] < cap:
        raise ValueError(f"rope tables hold {cos.shape[0]} positions, the cache {cap}")
    nb = lib.sd_cache_step_workspace_bytes(B, Hq, Hkv, cap)
    check(min(nb, 0), "sd_cache_step_workspace_bytes")
    if workspace is None:
        workspace = torch.empty(max(nb, 16), dtype=torch.uint8, device=qkv.device)
    if tickets is None:
        tickets = torch.zeros(B, Hkv, dtype=torch.int32, device=qkv.device)
    _need(tickets, torch.int32, "tickets")
    if tickets.numel() < B * Hkv:
        raise ValueError(f"tickets must hold {B} x {Hkv} counters")
    o = torch.empty(B, Hq * 128, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B, Hq, dtype=torch.float32, device=qkv.device) if want_lse else None
    check(lib.sd_cache_step(qkv.data_ptr(), q_gain.data_ptr(), k_gain.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                            pos.data_ptr(), C.byref(kv), o.data_ptr(), _p(lse), workspace.data_ptr(), workspace.numel(),
                            tickets.data_ptr(), B, cap if max_len is None else int(max_len), Hq, Hkv, 128, eps, 128 ** -0.5,
                            _stream()), "sd_cache_step")
    return (o, lse) if want_lse else o


def sample_params(do_sample=True, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, min_new_tokens=0,
                  eos_token_id=None, pad_token_id=0, use_ras=False, win_size=25, tau_r=0.2):
    """include/sd_hip.h sd_sample_params.  The RAS threshold is handed over as an integer count: count + 1 >= win_size *
    tau_r (sampler.py:146-147, evaluated in double as Python does) <=> count + 1 >= ceil(win_size * tau_r)."""
    import math
    from ._lib import SampleParams
    return SampleParams(int(bool(do_sample)), int(top_k), int(bool(use_ras)), int(win_size),
                        max(1, math.ceil(win_size * tau_r)), int(min_new_tokens),
                        -1 if eos_token_id is None else int(eos_token_id), int(pad_token_id), float(temperature),
                        float(top_p), float(repetition_penalty), 0.0)


def sample_step(logits, uniforms, seq, prompt_len, lens, finished, params, workspace=None, next_out=None, pos_out=None):
    """One sampling step (sd_sample_step) on logits bf16 [B,V] with uniforms fp32 [B,2]; updates seq int64 [B,cap], lens
    int32 [B] and finished uint8 [B] in place.  -> (next token int64 [B], its position int32 [B])."""
    _need(logits, torch.bfloat16, "logits"), _need(uniforms, torch.float32, "uniforms"), _need(seq, torch.int64, "seq")
    _need(prompt_len, torch.int32, "prompt_len"), _need(lens, torch.int32, "lens"), _need(finished, torch.uint8, "finished")
    lib = load_lib()
    B, V = logits.shape
    if uniforms.shape != (B, 2) or seq.shape[0] != B:
        raise ValueError("sample_step: uniforms must be [B,2] and seq [B,cap]")
    nb = lib.sd_sample_workspace_bytes(B, V)
    if workspace is None:
        workspace = torch.empty(nb, dtype=torch.uint8, device=logits.device)
    if next_out is None:
        next_out = torch.empty(B, dtype=torch.int64, device=logits.device)
    if pos_out is None:
        pos_out = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib.sd_sample_step(logits.data_ptr(), logits.stride(0), uniforms.data_ptr(), seq.data_ptr(), prompt_len.data_ptr(),
                             lens.data_ptr(), finished.data_ptr(), next_out.data_ptr(), pos_out.data_ptr(),
                             workspace.data_ptr(), workspace.numel(), C.byref(params), B, V, seq.shape[1], _stream()),
          "sd_sample_step")
    return next_out, pos_out


def sample_env(params):
    """include/sd_hip.h sd_sample_env of a list of ``SampleParams``: what the launches of one per-row step must cover."""
    from ._lib import SampleEnv
    sampling = [p for p in params if p.do_sample]
    return SampleEnv(max([p.top_k for p in sampling], default=0), int(bool(sampling)),
                     int(any(p.use_ras for p in sampling)), int(any(p.top_k == 0 for p in sampling)))


def sample_params_rows(params, device):
    """A list of B ``SampleParams`` -> the device array sd_sample_step_rows reads: uint8 [B, 48]."""
    raw = b"".join(bytes(p) for p in params)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(len(params), -1).to(device)


def sample_step_rows(logits, uniforms, seq, prompt_len, lens, finished, params, max_new, env, workspace=None,
                     next_out=None, pos_out=None):
    """One sampling step with everything per row (sd_sample_step_rows): logits bf16 [B,V]; uniforms fp32 [B,u_stride,2], of
    which row b reads pair lens[b] - prompt_len[b]; ``params`` uint8 [B,48] on the device (``sample_params_rows``);
    ``max_new`` int32 [B] on the device; ``env`` the host ``SampleEnv`` (``sample_env``).  Updates seq int64 [B,cap], lens
    int32 [B] and finished uint8 [B] in place.  -> (next token int64 [B], its position int32 [B])."""
    _need(logits, torch.bfloat16, "logits"), _need(uniforms, torch.float32, "uniforms"), _need(seq, torch.int64, "seq")
    _need(prompt_len, torch.int32, "prompt_len"), _need(lens, torch.int32, "lens"), _need(finished, torch.uint8, "finished")
    _need(params, torch.uint8, "params"), _need(max_new, torch.int32, "max_new")
    lib = load_lib()
    B, V = logits.shape
    from ._lib import SampleParams
    if uniforms.dim() != 3 or uniforms.shape[0] != B or uniforms.shape[2] != 2 or seq.shape[0] != B:
        raise ValueError("sample_step_rows: uniforms must be [B,u_stride,2] and seq [B,cap]")
    if params.numel() != B * C.sizeof(SampleParams) or max_new.numel() != B or prompt_len.numel() != B or \
            lens.numel() != B or finished.numel() != B:
        raise ValueError("sample_step_rows: params, max_new, prompt_len, lens and finished hold one entry per row")
    if workspace is None:
        workspace = torch.empty(lib.sd_sample_workspace_bytes(B, V), dtype=torch.uint8, device=logits.device)
    if next_out is None:
        next_out = torch.empty(B, dtype=torch.int64, device=logits.device)
    if pos_out is None:
        pos_out = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib.sd_sample_step_rows(logits.data_ptr(), logits.stride(0), uniforms.data_ptr(), uniforms.shape[1],
                                  seq.data_ptr(), prompt_len.data_ptr(), lens.data_ptr(), finished.data_ptr(),
                                  next_out.data_ptr(), pos_out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                  params.data_ptr(), max_new.data_ptr(), C.byref(env), B, V, seq.shape[1], _stream()),
          "sd_sample_step_rows")
    return next_out, pos_out
