"""MXFP8 in plain torch: TEST INFRASTRUCTURE ONLY (never imported by the product).

The number format of include/sd_hip.h "MXFP8 frozen teacher" (OCP Microscaling FP8): e4m3fn elements, one E8M0 scale per
32 consecutive elements along the last axis.  For a block of bf16 values x:

    amax = max |x|;  e = floor(log2(amax)) - 8 clamped to [-127, 127]  (amax == 0: e = -127);  scale byte = e + 127
    q = RNE_e4m3fn(clamp(x * 2^-e, -448, 448));  value = float(q) * 2^e

and ``teacher_forward_mx``: the gain-folded frozen teacher written with the pieces of oracle/qwen3.py, quantising where
the HIP runner does (x_in, ao, x_mid, act and the four folded weights, each from its bf16-rounded value), with fp32
matmuls of the dequantised operands.  Below that: the deterministic edge data of the kernel tests (ratio sweep, all bf16
patterns, fixed blocks), an independent fp64 restatement of the rule, and operands built as bytes (one-hot probes, exact
integers, the SwiGLU probe); tests/test_mx_cpu.py checks them on the CPU.
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


def mx_deq(q, scale, dtype=torch.float32):
    """(e4m3fn [..., K] or its bytes as uint8, E8M0 uint8 [..., K/32]) -> fp32 [..., K] (dtype=torch.float64: for scale
    bytes whose values leave the fp32 range)."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    f = q.to(torch.float32).to(dtype)
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


# ------------------------------------------------------------------------------------------ edge data of the kernel tests
# (tests/test_gpu_mx_kernels.py, tests/test_gpu_gemv_mx.py; checked on the CPU by tests/test_mx_cpu.py)
def bf16_from_bits(bits):
    """16-bit patterns (any integer tensor or list) -> the bf16 numbers that carry them."""
    b = torch.as_tensor(bits, dtype=torch.int64)
    return (b << 16).to(torch.int32).view(torch.float32).to(torch.bfloat16)  # exact: the low 16 bits are zero


def bf16_neighbours(ref):
    """The correctly rounded bf16 of an fp64 tensor and its two bf16 neighbours, as fp64."""
    c = ref.float().bfloat16()
    bits = c.view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(torch.bfloat16)
    down = (bits - 1).to(torch.int16).view(torch.bfloat16)
    return c.double(), up.double(), down.double()


def sweep_maxima():
    """The block maxima of the ratio sweep: m * 2^p for m in {1, 1.75, 1.9921875 (mantissa all ones)} and p in {-126, -120,
    -9, 0, 8, 100, 127}, and the bf16 subnormals 2^-133 and 127 * 2^-133.  All are bf16 numbers (fp64 here)."""
    a = [m * 2.0 ** p for p in (-126, -120, -9, 0, 8, 100, 127) for m in (1.0, 1.75, 1.9921875)]
    a += [2.0 ** -133, 127 * 2.0 ** -133]
    t = torch.tensor(a, dtype=torch.float64)
    assert torch.equal(t.to(torch.bfloat16).double(), t)
    return t


def sweep_blocks():
    """Ratio sweep, [blocks, 32] bf16: per maximum a of sweep_maxima(), element 0 of every block holds a and the other 31
    slots run, over consecutive blocks, through EVERY bf16 value v with a * 2^-20 <= |v| <= a, signs alternating (slots
    left over in a maximum's last block hold zeros).  Every bf16 mantissa thus stands at every exponent relative to the
    block maximum: every round-to-nearest-even tie, the whole saturating band (448, 512), the e4m3 subnormal codes and the
    flush to zero are in it."""
    pos = bf16_from_bits(torch.arange(1, 0x7F80)).double()  # every positive finite bf16, ascending
    out, n = [], 0
    for a in sweep_maxima().tolist():
        v = pos[(pos >= a * 2.0 ** -20) & (pos <= a)]
        sign = 1.0 - 2.0 * ((torch.arange(v.numel()) + n) % 2).double()
        n += v.numel()
        v = torch.cat([v * sign, torch.zeros(-v.numel() % 31, dtype=torch.float64)]).view(-1, 31)
        out.append(torch.cat([torch.full((v.shape[0], 1), a, dtype=torch.float64), v], 1))
    return torch.cat(out).to(torch.bfloat16)


def all_bf16_blocks():
    """All 65,280 finite bf16 bit patterns in pattern order, 32 per block: [2040, 32] bf16."""
    bits = torch.cat([torch.arange(0, 0x7F80), torch.arange(0x8000, 0xFF80)])
    return bf16_from_bits(bits).view(-1, 32)


def edge_matrix(j, blocks=None):
    """[M, 128 * j] bf16 of deterministic edge blocks.  Rows 0..3 are the fixed blocks -- row 0 all zeros, row 1 ordinary
    values around one zero block, row 2 blocks of +-448 * 2^k (k differs per block), row 3 all zeros -- then come
    `blocks` ([n, 32]; default: sweep_blocks() followed by all_bf16_blocks()) in order, 4 * j per row, the last row filled
    up with zero blocks."""
    nb = 4 * j
    if blocks is None:
        blocks = torch.cat([sweep_blocks(), all_bf16_blocks()])
    fixed = torch.zeros(4, nb, 32, dtype=torch.float64)
    i = torch.arange(32, dtype=torch.float64)
    fixed[1] = ((i * 7) % 23 - 11) * 0.375 + torch.arange(nb, dtype=torch.float64)[:, None]
    fixed[1, 1] = 0
    k = (torch.arange(nb) * 5) % 31 - 15
    fixed[2] = torch.ldexp(448.0 * (1 - 2 * (i % 2)), k[:, None].expand(nb, 32))
    fixed[2, :, 5:9] = torch.ldexp(torch.tensor([3.0, -0.5, 100.0, -447.0], dtype=torch.float64), k[:, None].expand(nb, 4))
    pad = torch.zeros(-blocks.shape[0] % nb, 32, dtype=torch.bfloat16)
    body = torch.cat([blocks.to(torch.bfloat16), pad]).view(-1, nb * 32)
    return torch.cat([fixed.view(4, nb * 32).to(torch.bfloat16), body])


def mx_quant_fp64(x):
    """The rule of mx_quant restated independently in fp64, with the rounding spelled out: per 32-block e = floor(log2
    amax) - 8 clamped to [-127, 127] (-127 for a zero block), y = clamp(x * 2^-e, -448, 448), step = 2^(max(floor(log2
    |y|), -6) - 3), value = round_half_even(y / step) * step * 2^e.  x [..., K] of bf16 numbers -> (scale bytes uint8
    [..., K/32], values fp64 [..., K], tie fp64 [..., K]: +1 where y lay exactly between two codes and went up in
    magnitude, -1 where it went down, else 0)."""
    xd = x.to(torch.bfloat16).double()
    blk = xd.reshape(*xd.shape[:-1], xd.shape[-1] // 32, 32)
    amax = blk.abs().amax(-1)
    fl = torch.frexp(amax)[1].to(torch.int64) - 1           # fp64 holds every bf16 number as a normal one
    e = torch.where(amax == 0, torch.full_like(fl, -127), (fl - 8).clamp(-127, 127))
    two = torch.tensor(2.0, dtype=torch.float64)
    y = (blk * torch.pow(two, -e.double())[..., None]).clamp(-E4M3_MAX, E4M3_MAX)
    fy = (torch.frexp(y.abs())[1].to(torch.int64) - 1).clamp(min=-6)
    step = torch.pow(two, (fy - 3).double())
    n = y / step                                              # exact: a power-of-two divisor
    r = torch.round(n)                                        # half to even
    tie = torch.where((n - n.floor()) == 0.5, torch.sign(r.abs() - n.abs()), torch.zeros_like(n))
    val = r * step * torch.pow(two, e.double())[..., None]
    return (e + 127).to(torch.uint8), val.reshape(xd.shape), tie.reshape(xd.shape)


# ------------------------------------------------------------------------------------------ operands built as bytes
def e4m3_bytes(v):
    """Numbers that e4m3fn holds exactly (asserted) -> their bytes."""
    q = v.to(torch.float32).to(torch.float8_e4m3fn)
    assert torch.equal(q.to(torch.float32).double(), v.double())
    return q.view(torch.uint8)


def int_operand(rows, K, vmax, smax, g):
    """Integer elements |v| <= vmax and power-of-two scales 2^-smax..2^smax, different per block and per row (the rule of
    tests/test_gpu_mx.py::_int_operand): (bytes [rows, K], scale bytes [rows, K/32])."""
    v = torch.randint(-vmax, vmax + 1, (rows, K), generator=g).float()
    s = (127 + torch.randint(-smax, smax + 1, (rows, K // 32), generator=g)).to(torch.uint8)
    return v.to(torch.float8_e4m3fn).view(torch.uint8), s


CODE_TABLE_RUNS = 3


def code_table_probe(run, K=384):
    """One-hot probe of the e4m3 code table and the E8M0 range.  A [256, K]: row m holds byte code m at k = (37 m + 11 run)
    % K (distinct per row) and zeros elsewhere; only the rows of the NaN codes 0x7F and 0xFF stay empty.  B [K, K]: row n
    holds the byte of 1.0 at k = n.  The block of a non-zero probed element carries sa = (m + 85 run) % 255 in A -- 0..254
    over the CODE_TABLE_RUNS runs -- and in B the byte sb with (sa - 127) + (sb - 127) = t, t sweeping [-100, 100] as far
    as sb in 0..254 allows; blocks that hold only zeros -- the block of the -0 byte 0x80 among them -- carry scale byte 0,
    as the quantiser emits them.  Every output is one product: want[m][k(m)] = value(code m) * 2^t, a normal bf16 number,
    and 0 elsewhere (also for the codes +0 and -0).
    -> (a_q, a_scale, b_q, b_scale, want bf16 [256, K], sa and t of the rows that hold a non-zero code)."""
    m = torch.arange(256)
    finite = (m & 0x7F) != 0x7F
    live = finite & ((m & 0x7F) != 0)
    kpos = (m * 37 + 11 * run) % K
    assert kpos.unique().numel() == 256
    sa = (m + 85 * run) % 255
    t = torch.maximum(torch.minimum((m * 29 + run * 67) % 201 - 100, sa.clamp(max=100)), (sa - 254).clamp(min=-100))
    sb = 254 + t - sa
    assert int(sb.min()) >= 0 and int(sb.max()) <= 254
    aq = torch.zeros(256, K, dtype=torch.uint8)
    aq[m[finite], kpos[finite]] = m[finite].to(torch.uint8)
    as_ = torch.zeros(256, K // 32, dtype=torch.uint8)
    as_[m[live], kpos[live] // 32] = sa[live].to(torch.uint8)
    n = torch.arange(K)
    bq = torch.zeros(K, K, dtype=torch.uint8)
    bq[n, n] = 0x38
    bs = torch.zeros(K, K // 32, dtype=torch.uint8)
    bs[n, n // 32] = 127
    bs[kpos[live], kpos[live] // 32] = sb[live].to(torch.uint8)
    val = m.to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).double()
    want = torch.zeros(256, K, dtype=torch.float64)
    want[m[live], kpos[live]] = torch.ldexp(val[live], t[live])
    assert torch.equal(want.float().bfloat16().double(), want)
    return aq, as_, bq, bs, want.float().bfloat16(), sa[live], t[live]


def position_probe(K, N=96):
    """One-hot probe of the byte-to-k map and of which block a scale is taken from.  A [K, K]: row m holds one non-zero
    code at k = m; its scale bytes differ from block to block of the row (zero blocks included).  B [N, K] is dense: small
    integers that differ along k and rows, scales that differ per row and block.  want[m][n] = A[m][m] * B[n][m] exactly.
    -> (a_q, a_scale, b_q, b_scale, want bf16 [K, N])."""
    m, n, k, blk = torch.arange(K), torch.arange(N), torch.arange(K), torch.arange(K // 32)
    aq = torch.zeros(K, K, dtype=torch.uint8)
    aq[m, m] = ((1 + (m * 7) % 126) | ((m & 1) << 7)).to(torch.uint8)
    as_ = (127 + (m[:, None] + 3 * blk[None]) % 13 - 6).to(torch.uint8)
    bq = e4m3_bytes(((n[:, None] * 5 + k[None] * 3) % 15 - 7).double())
    bs = (127 + (n[:, None] + 2 * blk[None]) % 5 - 2).to(torch.uint8)
    want = mx_deq(aq, as_, torch.float64)[m, m][:, None] * mx_deq(bq, bs, torch.float64)[:, m].T
    assert torch.equal(want.float().bfloat16().double(), want)
    return aq, as_, bq, bs, want.float().bfloat16()


def swiglu_probe(M, I, K, scaled):
    """Operands of sd_gemm_mxfp8_swiglu whose act is exact whatever the kernel's exp is.  Every gate row of wgu is a one-hot
    selector of an element of A's first block, which holds (after the row scale) 32, 64 or -104: silu(32) = 32 and silu(64)
    = 64 in fp32 for any exp with a relative error below 2^20, and silu(-104) = -0.  Of the 32 columns of act block b,
    those with c % 4 == 3 select the -104 of k = 2; the others select the row's switch k = 3 + b % S (S = min(29, I / 32)),
    which holds 32 or 64 -- and -104 for b % S == m % S: that block of row m is a zero block.  The up rows hold small integers (negative
    ones too) against small integers of A at k >= 32, with power-of-two block scales that cancel: u is an integer (times
    the row scale), |u| < 256.  scaled: rowscale = 2^(m % 3 - 1), A's first block divided by it; else no row scale.
    -> (a_q, a_scale, wgu_q, wgu_scale, rowscale fp32 [M] or None, act fp64 [M, I] (bf16 numbers))."""
    m, i, k = torch.arange(M), torch.arange(I), torch.arange(K)
    rs = torch.ldexp(torch.ones(M, dtype=torch.float64), m % 3 - 1) if scaled else torch.ones(M, dtype=torch.float64)
    ea = torch.where(k < 32, 0, (k // 32) % 3 - 1)                           # A's block exponents along k
    a = ((m[:, None] * 7 + k[None] * 3) % 7 - 3).double()
    S = min(29, I // 32)
    t = torch.arange(29)
    sw = torch.where((m[:, None] + t[None]) % 2 == 0, 32.0, 64.0).double()
    sw[(m % S)[:, None] == t[None]] = -104.0
    a[:, 0], a[:, 1], a[:, 2], a[:, 3:32] = 32.0, 64.0, -104.0, sw
    a[:, :32] /= rs[:, None]
    aq = e4m3_bytes(a)
    as_ = (127 + ea[::32]).to(torch.uint8)[None].expand(M, K // 32).contiguous()
    kg = torch.where(i % 4 == 3, 2, 3 + (i // 32) % S)
    wg = torch.zeros(I, K, dtype=torch.float64)
    wg[i, kg] = 1.0
    wu = ((i[:, None] * 3 + k[None] * 5) % 5 - 2).double() * (((k[None] + i[:, None]) % 32 == 0) & (k[None] >= 32))
    wq = e4m3_bytes(torch.cat([wg, wu]))
    ws = torch.zeros(2 * I, K // 32, dtype=torch.uint8)
    ws[:I, 0] = 127
    ws[I:, 1:] = (127 - ea[32::32]).to(torch.uint8)[None]
    ad, wd = mx_deq(aq, as_, torch.float64), mx_deq(wq, ws, torch.float64)
    g, u = rs[:, None] * (ad @ wd[:I].T), rs[:, None] * (ad @ wd[I:].T)
    assert bool(((g == 32) | (g == 64) | (g == -104)).all()) and float(u.abs().max()) < 256 and float(u.min()) < 0
    act = torch.where(g > 0, g * u, torch.zeros_like(u))
    assert torch.equal(act.float().bfloat16().double(), act)
    return aq, as_, wq, ws, (rs.float() if scaled else None), act
