"""MXFP8 in plain torch: TEST INFRASTRUCTURE ONLY (never imported by the product).

The number format of include/sd_hip.h "MXFP8 frozen teacher" (OCP Microscaling FP8): e4m3fn elements, one E8M0 scale per
32 consecutive elements along the last axis.  For a block of bf16 values x:

    amax = max |x|;  e = floor(log2(amax)) - 8 clamped to [-127, 127]  (amax == 0: e = -127);  scale byte = e + 127
    q = RNE_e4m3fn(clamp(x * 2^-e, -448, 448));  value = float(q) * 2^e

and ``teacher_forward_mx``: the gain-folded frozen teacher written with the pieces of oracle/qwen3.py, quantising where
the HIP runner does (x_in, ao, x_mid, act and the four folded weights, each from its bf16-rounded value), with fp32
matmuls of the dequantised operands.
"""
from __future__ import annotations

import torch

from oracle.qwen3 import _st, apply_rope, attention, rms_norm, rope_tables

E4M3_MAX = 448.0
EMAX = 8  # floor(log2(448))


def mx_quant(x):
    """x [..., K] (K % 32 == 0; rounded to bf16 first) -> (q float8_e4m3fn [..., K], scale uint8 [..., K/32])."""
    xb = x.to(torch.bfloat16).to(torch.float32)
    blk = xb.reshape(*xb.shape[:-1], xb.shape[-1] // 32, 32)
    amax = blk.abs().amax(-1)
    _, ex = torch.frexp(amax)                      # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = (ex.to(torch.int32) - 1 - EMAX).clamp(-127, 127)
    e = torch.where(amax == 0, torch.full_like(e, -127), e)
    y = torch.ldexp(blk, (-e)[..., None]).clamp(-E4M3_MAX, E4M3_MAX)
    q = y.to(torch.float8_e4m3fn).reshape(xb.shape)
    return q, (e + 127).to(torch.uint8)


def mx_deq(q, scale):
    """(e4m3fn [..., K] or its bytes as uint8, E8M0 uint8 [..., K/32]) -> fp32 [..., K]."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    f = q.to(torch.float32)
    blk = f.reshape(*f.shape[:-1], f.shape[-1] // 32, 32)
    return torch.ldexp(blk, (scale.to(torch.int32) - 127)[..., None]).reshape(f.shape)


def mx_round(x, quant=True):
    """What an MXFP8 operand carries of x: bf16 rounding, then the quantise / dequantise round trip (quant=False: x)."""
    return mx_deq(*mx_quant(x)) if quant else x.to(torch.float32)


def fold_weights(w, shape):
    """Per layer the fused, gain-folded projection weights as the model prepares them: bf16(W * g) (fp32 values)."""
    out = []
    for l in range(shape.num_hidden_layers):
        p = f"model.layers.{l}."
        g1 = w[p + "input_layernorm.weight"].float()
        g2 = w[p + "post_attention_layernorm.weight"].float()
        b = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
        wqkv = torch.cat([b(w[p + f"self_attn.{n}_proj.weight"]) for n in ("q", "k", "v")], 0)
        wgu = torch.cat([b(w[p + f"mlp.{n}_proj.weight"]) for n in ("gate", "up")], 0)
        out.append({"wqkv": b(wqkv * b(g1)[None, :]), "wo": b(w[p + "self_attn.o_proj.weight"]),
                    "wgu": b(wgu * b(g2)[None, :]), "wdown": b(w[p + "mlp.down_proj.weight"])})
    return out


def teacher_forward_mx(w, shape, input_ids, attention_mask=None, storage=None, quant=True):
    """Logits [B,T,V] (fp32) of the gain-folded teacher with MXFP8 projections.  storage="bf16" rounds where the HIP runner
    stores bf16 (oracle/qwen3.py); quant=False switches the quantisation off (then this is oracle.qwen3.forward up to the
    rounding of the folded weights).  The weights are taken at bf16 precision, as the model holds them."""
    st = lambda t: _st(t, storage)  # noqa: E731
    B, T = input_ids.shape
    Hq, Hkv, d = shape.num_attention_heads, shape.num_key_value_heads, shape.head_dim
    eps = shape.rms_norm_eps
    emb = w["model.embed_tokens.weight"].to(torch.bfloat16).float()
    x = emb[input_ids]
    cos, sin = rope_tables(T, d, shape.rope_theta, torch.float32)
    key_len = None if attention_mask is None else attention_mask.sum(-1)
    qd, kd = shape.q_dim, shape.kv_dim
    for l, f in enumerate(fold_weights(w, shape)):
        p = f"model.layers.{l}."
        wq = {k: mx_round(v, quant) for k, v in f.items()}
        r = x
        rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)        # of the un-normalised row
        qkv = st(rstd * (mx_round(x, quant) @ wq["wqkv"].T))
        q = qkv[..., :qd].reshape(B, T, Hq, d)
        k = qkv[..., qd:qd + kd].reshape(B, T, Hkv, d)
        v = qkv[..., qd + kd:].reshape(B, T, Hkv, d)
        q = rms_norm(q, w[p + "self_attn.q_norm.weight"].float(), eps, storage).transpose(1, 2)
        k = rms_norm(k, w[p + "self_attn.k_norm.weight"].float(), eps, storage).transpose(1, 2)
        v = v.transpose(1, 2)
        q = st(apply_rope(q, cos, sin))
        k = st(apply_rope(k, cos, sin))
        o = st(attention(q, k, v, key_len, storage)).transpose(1, 2).reshape(B, T, Hq * d)
        x = st(r + mx_round(o, quant) @ wq["wo"].T)
        r = x
        rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        gu = st(rstd * (mx_round(x, quant) @ wq["wgu"].T))
        I = shape.intermediate_size
        act = st(torch.nn.functional.silu(gu[..., :I]) * gu[..., I:])
        x = st(r + mx_round(act, quant) @ wq["wdown"].T)
    x = rms_norm(x, w["model.norm.weight"].float(), eps, storage)
    head = emb if shape.tie_word_embeddings else w["lm_head.weight"].to(torch.bfloat16).float()
    return st(x @ head.T)
