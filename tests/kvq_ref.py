"""The decoder over a quantised KV cache in plain torch: TEST INFRASTRUCTURE ONLY (never imported by the product).

``forward_kvq`` is oracle/qwen3.py ``forward`` (fp32, the same pieces) with ONE change: in every layer the K rows (after
q/k-norm + RoPE) and the V rows that a KV cache would hold are passed through bf16 rounding and then the MXFP8 round trip
of tests/mx_ref.py ``mx_round`` (e4m3 elements, one E8M0 scale per 32 elements of a head vector), for ALL keys -- a
query's own position included.  That is what a generation computes whose every position went through sd_qwen3_extend_*
or a decode step over 8-bit pages (include/sd_hip.h): the row is stored first, then attended over as stored.  It is NOT
what sd_qwen3_prefill_paged_mx computes for its own prompt, which attends over the bf16 rows in flight.

``quant=False`` leaves the rows alone (then this is oracle.qwen3.forward); ``storage="bf16"`` is the oracle's error-budget
mode (bf16 rounding wherever the HIP path stores bf16).
"""
from __future__ import annotations

import torch

from mx_ref import mx_round
from oracle.qwen3 import _st, apply_rope, attention, rms_norm, rope_tables


def forward_kvq(w, shape, input_ids, attention_mask=None, storage=None, quant=True):
    """input_ids [B,T] -> logits [B,T,V] (fp32)."""
    st = lambda t: _st(t, storage)  # noqa: E731
    kvq = (lambda t: mx_round(t)) if quant else (lambda t: t)  # noqa: E731  (mx_round rounds to bf16 first)
    B, T = input_ids.shape
    Hq, Hkv, d = shape.num_attention_heads, shape.num_key_value_heads, shape.head_dim
    eps = shape.rms_norm_eps
    emb = w["model.embed_tokens.weight"]
    x = emb[input_ids]
    cos, sin = rope_tables(T, d, shape.rope_theta, x.dtype)
    key_len = None if attention_mask is None else attention_mask.sum(-1)
    for l in range(shape.num_hidden_layers):
        p = f"model.layers.{l}."
        r = x
        xn = rms_norm(x, w[p + "input_layernorm.weight"], eps, storage)
        q = st(xn @ w[p + "self_attn.q_proj.weight"].T).view(B, T, Hq, d)
        k = st(xn @ w[p + "self_attn.k_proj.weight"].T).view(B, T, Hkv, d)
        v = st(xn @ w[p + "self_attn.v_proj.weight"].T).view(B, T, Hkv, d)
        q = rms_norm(q, w[p + "self_attn.q_norm.weight"], eps, storage).transpose(1, 2)
        k = rms_norm(k, w[p + "self_attn.k_norm.weight"], eps, storage).transpose(1, 2)
        v = v.transpose(1, 2)
        q = st(apply_rope(q, cos, sin))
        k = kvq(st(apply_rope(k, cos, sin)))      # the cache row: a head vector [.., d] is four 32-element blocks
        v = kvq(v)
        o = st(attention(q, k, v, key_len, storage)).transpose(1, 2).reshape(B, T, Hq * d)
        x = st(r + o @ w[p + "self_attn.o_proj.weight"].T)
        r = x
        xn = rms_norm(x, w[p + "post_attention_layernorm.weight"], eps, storage)
        gate = st(xn @ w[p + "mlp.gate_proj.weight"].T)
        up = st(xn @ w[p + "mlp.up_proj.weight"].T)
        x = st(r + st(torch.nn.functional.silu(gate) * up) @ w[p + "mlp.down_proj.weight"].T)
    x = rms_norm(x, w["model.norm.weight"], eps, storage)
    head = emb if shape.tie_word_embeddings else w["lm_head.weight"]
    return st(x @ head.T)
