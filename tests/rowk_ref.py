"""fp64 references, per-element bounds, case tables and restated launcher decisions of tests/test_gpu_row_kernels.py:
the row kernels of sd_elementwise.hip (RMSNorm, q/k-norm + RoPE, SwiGLU, embedding / scatter, column sums).

TEST INFRASTRUCTURE ONLY, CPU only (never imported by the product).  tests/test_rowk_ref_cpu.py shows on the CPU that
the rules accept an fp32 restatement of every kernel and the exactly rounded reference, reject each named wrong formula,
and that every case of the tables below reaches the launcher path it is named for.

Every reference is an fp64 evaluation of the same bf16 inputs with no rounding inserted; backwards come from autograd on
the fp64 forward.  The rules, per element ("How the row kernels are checked"):

1. kernels that round once, at the store (RMSNorm dx, q/k dqkv, SwiGLU fwd / bwd): parity_ref.rowwise_close,
       |got - ref| <= half_ulp_bf16(ref) + floor * max|ref_row|
   with floor = 4 x the worst per-row error of the same formula in fp32 on the CPU (measure_floors), and for SwiGLU a
   derived per-element floor 2^-16 |magnitude| (``elem_close``): __expf is v_exp_f32 of g * log2(e); the scaling costs
   |g| 2^-24 <= 2^-20 relative at |g| <= 16, v_exp_f32 about one ulp more.
2. kernels with documented inner roundings (RMSNorm y, q/k out): the interval rule.  An error bound E is carried through
   the formula; a rounding to bf16 adds half_ulp(|value| + E) -- half an ulp at the TOP of the interval the kernel's
   value can lie in, not at the exact value --, a product by a known factor scales E, a sum adds the bounds, an fp32
   step adds FWD_FLOOR times the magnitude.
3. rounding points: the two forwards are also compared with an fp32 restatement that rounds where the kernel's comments
   say it rounds (rstd taken from the fp64 reference, rounded to fp32); at most ROUNDING_SHARE of the elements may
   differ.  rstd off by two fp32 ulps or a product left unrounded moves ~3e-5 of them; a dropped inner rounding 25 %.
4. gain gradients (dw, dq_gain, dk_gain: an fp32 sum of n terms stored as bf16), per column:
       |got - ref| <= half_ulp(ref) + (n + 8) 2^-24 sum|term|
   (any summation order plus the roundings inside a term; accumulate: the previous bf16 value is one more term).
5. RMSNorm rstd (fp32): relative error <= 4 x the measured fp32 error.
6. data movement and sums that are exact (embedding, rows_scatter, column sums / embedding backward on integer data):
   torch.equal against the fp64 result rounded once to bf16.
"""
from __future__ import annotations

import collections
import functools
import math

import torch

from parity_ref import half_ulp

BF = torch.bfloat16
EPS = 1e-6
ULP32 = 2.0 ** -24  # one fp32 rounding, relative

# Measured by measure_floors() (fp32 evaluation on the CPU against fp64, worst row over every case of the family,
# relative to the row maximum) and the floor chosen from it (4 x, rounded up to two digits).
RMS_BWD_MEASURED = 1.93e-7  # dx of rmsnorm_bwd_f32 (bf16 dy and fp32 slabs), RMS_CASES + RMS_BWD_BIG + RMS_SLAB_CASES
RMS_BWD_FLOOR = 7.8e-7
QK_BWD_MEASURED = 2.74e-7   # dqkv of qk_bwd_f32, QK_BWD_CASES
QK_BWD_FLOOR = 1.1e-6
RSTD_MEASURED = 2.07e-7     # rsqrt(mean(x^2) + eps) in fp32, relative, every RMSNorm case
RSTD_RTOL = 8.3e-7
# one fp32 step of the two forwards (x * rstd with an rstd that is RSTD_RTOL off, rounded once): RSTD_RTOL + 2^-24 = 8.9e-7 <= 2^-20
FWD_FLOOR = 2.0 ** -20
SWIGLU_FLOOR = 2.0 ** -16   # per element, of the magnitudes named in swiglu_ref (|gate| <= SWIGLU_GATE_MAX)
SWIGLU_GATE_MAX = 16.0
ROUNDING_SHARE = 0.01       # rule 3: a condition, not a measurement


# ------------------------------------------------------------------------------------------- launcher decisions
def rms_nch(H):
    """The NCH of rmsnorm_fwd_kernel<NCH> / rmsnorm_bwd_kernel<NCH, SLABS> (512-column chunks a lane holds)."""
    n = (H + 511) // 512
    return 1 if n <= 1 else 2 if n == 2 else 4 if n <= 4 else 8


def rms_status(H):
    """What sd_rmsnorm_* returns for a row length: 0, -1 (SD_ERR_SHAPE) or -3 (SD_ERR_UNSUPPORTED)."""
    return -1 if H % 8 else -3 if H > 4096 else 0


RmsGrid = collections.namedtuple("RmsGrid", "nb rows_per_block last_rows wave_trips lds_bytes")


def rms_bwd_grid(M, H):
    """rmsnorm_bwd_any: workgroups, rows per workgroup, rows of the last one, the most rows one wave runs, dynamic LDS."""
    nb = min((M + 3) // 4, 512)
    rpb = -(-M // nb)
    nb = -(-M // rpb)
    return RmsGrid(nb, rpb, M - (nb - 1) * rpb, -(-rpb // 4), 4 * H * 4)


QkGrid = collections.namedtuple("QkGrid", "nb items_per_block trips last_items")


def qk_bwd_grid(items, blocks=0):
    """qk_bwd_blocks(): workgroups, items per workgroup (a multiple of the 48 items of one trip), trips per workgroup,
    items of the last workgroup.  ``blocks``: the debug key qk_bwd.blocks (0 = 512)."""
    nblk = blocks if blocks > 0 else 512
    per = -(-items // nblk)
    per = -(-per // 48) * 48
    nb = -(-items // per)
    return QkGrid(nb, per, per // 48, items - (nb - 1) * per)


def swiglu_grid(M, I):
    """-> (workgroups, 8-element vectors, vectors that a second grid stride handles)."""
    n8 = M * I // 8
    nb = min((n8 + 255) // 256, 4096)
    return nb, n8, max(0, n8 - nb * 256)


def colsum_trips(nb):
    """colsum_reduce_kernel, row group 0: (trips of the eight-way unrolled loop, trips of the tail loop)."""
    b = un = 0
    while b + 56 < nb:
        b += 64
        un += 1
    return un, len(range(b, nb, 8))


def emb_bwd_path(M):
    """embedding_bwd_kernel: the LDS bitmap holds 2048 words of 32 tokens; longer batches take the serial scan."""
    return "bitmap" if (M + 31) // 32 <= 2048 else "serial"


def ssq_status(H):
    return -1 if H % 8 else -3 if (H % 512 or H // 128 > 16) else 0


# ------------------------------------------------------------------------------------------- inputs
ROW_KINDS = ("randn", "tiny", "big", "zero", "onehot")  # x 1, x 1e-3 (eps matters), x 200, all zero, one element


def row_kind(r, shift):
    return ROW_KINDS[(r + shift) % 5]


def kinded(x, shift, hot=1.5, off=0):
    """x [R, C] fp32 -> the same with row r turned into ROW_KINDS[(r + shift) % 5].  off: moves the one-hot column, so that
    a one-hot gradient row never meets a one-hot input row in the same column (there dx is a difference of two equal
    numbers and its fp32 error says nothing about a kernel)."""
    x = x.clone()
    for r in range(x.shape[0]):
        k = row_kind(r, shift)
        if k == "tiny":
            x[r] *= 1e-3
        elif k == "big":
            x[r] *= 200.0
        elif k in ("zero", "onehot"):
            x[r] = 0.0
            if k == "onehot":
                x[r, (3 * r + 1 + off) % x.shape[1]] = hot
    return x


def gains(n, gen):
    """1 + 0.2 randn with one zero and one negative entry."""
    w = 1 + 0.2 * torch.randn(n, generator=gen)
    w[1 % n] = 0.0
    w[2 % n] = -0.75
    return w.to(BF)


def _gen(*key):
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------- RMSNorm
RMS_H = (8, 136, 512, 520, 1024, 1032, 2048, 2056, 4096)
RMS_M = (1, 3, 5)
RMS_CASES = [(M, H) for H in RMS_H for M in RMS_M]
# NCH and whether the last 512-column chunk is partial, per H (test_rowk_ref_cpu.py checks the table against rms_nch)
RMS_PATHS = {8: (1, True), 136: (1, True), 512: (1, False), 520: (2, True), 1024: (2, False), 1032: (4, True),
             2048: (4, False), 2056: (8, True), 4096: (8, False)}
# backward only, each with dres on / off and accumulate_dw 0 / 1: (M, H) -> the RmsGrid it must reach
RMS_BWD_BIG = {(2049, 136): dict(nb=410, rows_per_block=5, last_rows=4, wave_trips=2),
               (4101, 136): dict(nb=456, rows_per_block=9, last_rows=6, wave_trips=3),
               (4101, 520): dict(nb=456, rows_per_block=9, last_rows=6, wave_trips=3)}
RMS_SLAB_CASES = [(M, H, ns) for (M, H) in ((5, 136), (2049, 520)) for ns in (1, 3)]
RMS_REFUSED = {12: -1, 4104: -3}


@functools.lru_cache(maxsize=None)
def rms_inputs(M, H, nsplit=0):
    """-> dict of CPU tensors: x, w, dy, dres, dw0 (bf16) and, with nsplit > 0, slabs [nsplit, M, H] fp32 (then dy is
    None: the gradient is the fp64 sum of the slabs)."""
    gen = _gen(M, H, nsplit)
    shift = RMS_H.index(H) if H in RMS_H else 0
    x = kinded(torch.randn(M, H, generator=gen) * 2, shift + M).to(BF)
    out = dict(x=x, w=gains(H, gen), dres=torch.randn(M, H, generator=gen).to(BF),
               dw0=(torch.randn(H, generator=gen) * 3).to(BF), dy=None, slabs=None)
    if nsplit:
        out["slabs"] = kinded(torch.randn(nsplit * M, H, generator=gen), 1, off=4).view(nsplit, M, H).contiguous()
    else:
        out["dy"] = kinded(torch.randn(M, H, generator=gen), shift + M + 2, hot=-2.0, off=4).to(BF)
    return out


def rstd64(x, eps=EPS, n=None):
    x = x.double()
    return torch.rsqrt(x.pow(2).sum(-1) / (n or x.shape[-1]) + eps)


def rmsnorm_ref(x, w, dy=None, dres=None, dw0=None, eps=EPS):
    """fp64.  -> dict(y, rstd) and, with dy (any float type; fp64 for summed slabs): dx (+ dres), dw (+ dw0), dw_n (the
    number of terms of a dw column) and dw_abs (the sum of their magnitudes)."""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    rs = rstd64(xr, eps)
    y = wr * (xr * rs[:, None])
    out = dict(y=y.detach(), rstd=rs.detach())
    if dy is None:
        return out
    d = dy.double()
    (y * d).sum().backward()
    terms = (d * (xr * rs[:, None])).detach()
    out.update(dx=xr.grad + (0 if dres is None else dres.double()), dw=wr.grad + (0 if dw0 is None else dw0.double()),
               dw_n=x.shape[0] + (0 if dw0 is None else 1),
               dw_abs=terms.abs().sum(0) + (0 if dw0 is None else dw0.double().abs()))
    return out


def rmsnorm_fwd_f32(x, w, rstd32=None, eps=EPS, round_inner=True, gain_first=False, mean_n=None):
    """The forward as the kernel's comments state it, in fp32: y = bf16(w * bf16(x * rstd)) -> (y bf16, rstd fp32).
    rstd32: take the statistic from outside (rule 3).  The switches are the wrong formulas of the CPU test."""
    xf, wf = x.float(), w.float()
    if rstd32 is None:
        rstd32 = torch.rsqrt(xf.pow(2).sum(-1) / float(mean_n or x.shape[-1]) + torch.tensor(eps, dtype=torch.float32))
    a = xf * rstd32[:, None]
    if gain_first:
        return ((wf * xf).to(BF).float() * rstd32[:, None]).to(BF), rstd32
    n = a.to(BF).float() if round_inner else a
    return (wf * n).to(BF), rstd32


def rmsnorm_bwd_f32(x, w, rstd32, dy=None, slabs=None, dres=None):
    """rmsnorm_bwd_kernel in fp32 -> (dx fp32 before the store, dw terms summed in fp32)."""
    xf, wf = x.float(), w.float()
    if slabs is not None:
        d = torch.zeros_like(xf)
        for s in slabs:
            d = d + s
    else:
        d = dy.float()
    rs = rstd32[:, None]
    xh = xf * rs
    dot = (d * wf * xf * rs).sum(-1, keepdim=True) / float(x.shape[-1])
    dx = rs * (d * wf - xh * dot)
    if dres is not None:
        dx = dres.float() + dx
    return dx, (d * xh).sum(0)


def rmsnorm_fwd_bound(x, w, ref=None, eps=EPS):
    """The interval rule for y = bf16(w * bf16(x * rstd)) -> bound [M, H] fp64."""
    rs = rstd64(x, eps) if ref is None else ref["rstd"]
    a = (x.double() * rs[:, None]).abs()
    e = FWD_FLOOR * a                              # x * rstd in fp32, with the kernel's own rstd
    e = e + half_ulp(a + e, BF)                    # the inner rounding
    e = w.double().abs() * e                       # bf16 x bf16 is exact in fp32
    return e + half_ulp(w.double().abs() * a + e, BF)


# ------------------------------------------------------------------------------------------- q/k norm + RoPE
# (B, T, Hq, Hkv)
QK_CASES = [(1, 1, 1, 1), (3, 5, 2, 1), (1, 16, 2, 1), (2, 33, 3, 2), (1, 4100, 1, 1)]
QK_ITEMS = {(1, 1, 1, 1): 2, (3, 5, 2, 1): 45, (1, 16, 2, 1): 48, (2, 33, 3, 2): 330, (1, 4100, 1, 1): 8200}
# backward: (B, T, Hq, Hkv, qk_bwd.blocks) -> the QkGrid it must reach
QK_BWD_CASES = {c + (0,): dict(nb=-(-QK_ITEMS[c] // 48), items_per_block=48, trips=1) for c in QK_CASES}
QK_BWD_CASES[(1, 4100, 4, 2, 0)] = dict(nb=257, items_per_block=96, trips=2, last_items=24)   # 24 600 items
QK_BWD_CASES[(2, 50, 2, 1, 2)] = dict(nb=2, items_per_block=192, trips=4, last_items=108)     # 300 items, debug key


def rope_tables(T, theta=1e6, d=128):
    """ops.rope_tables on the CPU: cos/sin [T, d] as HF computes them, rounded to bf16 (inputs of kernel and reference)."""
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().to(BF), emb.sin().to(BF)


@functools.lru_cache(maxsize=None)
def qk_inputs(B, T, Hq, Hkv):
    """-> dict: qkv [M, (Hq+2Hkv) 128], qg, kg, cos, sin, dout [M, (Hq+Hkv) 128], dqg0, dkg0 (bf16, CPU).  Head vector i
    (token-major) of q|k is of kind ROW_KINDS[(i + shift) % 5]; the v columns are random."""
    gen = _gen(B, T, Hq, Hkv)
    M, nh = B * T, Hq + Hkv
    shift = (B + T + Hq) % 5
    qkv = torch.randn(M, (Hq + 2 * Hkv) * 128, generator=gen)
    qkv[:, :nh * 128] = kinded(qkv[:, :nh * 128].reshape(M * nh, 128), shift).view(M, nh * 128)
    dout = kinded(torch.randn(M * nh, 128, generator=gen), shift + 3, hot=-2.0, off=4).view(M, nh * 128)
    cos, sin = rope_tables(T)
    return dict(qkv=qkv.to(BF), qg=gains(128, gen), kg=gains(128, gen), cos=cos, sin=sin, dout=dout.to(BF),
                dqg0=(torch.randn(128, generator=gen) * 3).to(BF), dkg0=(torch.randn(128, generator=gen) * 3).to(BF))


def _rot(n):
    return torch.cat((-n[..., 64:], n[..., :64]), -1)


def _rot_t(z):
    return torch.cat((z[..., 64:], -z[..., :64]), -1)


def _qk_forward(x, gain, c, s, eps, dt):
    rs = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + torch.tensor(eps, dtype=dt))
    n = gain * (x * rs)
    return n * c + _rot(n) * s, rs


def qk_ref(inp, T, Hq, Hkv, backward=False, accumulate=False, eps=EPS):
    """fp64.  -> dict(out [M, nh 128]) and, with backward: dqk [M, nh 128] (the q|k columns of dqkv), dqg, dkg (+ the
    previous values with accumulate), and per gain its number of terms and the sum of their magnitudes."""
    M, nh = inp["qkv"].shape[0], Hq + Hkv
    x = inp["qkv"][:, :nh * 128].double().view(M, nh, 128).requires_grad_(True)
    qg, kg = inp["qg"].double().requires_grad_(True), inp["kg"].double().requires_grad_(True)
    gain = torch.cat([qg[None].expand(Hq, 128), kg[None].expand(Hkv, 128)], 0)[None]
    pos = torch.arange(M) % T
    c, s = inp["cos"].double()[pos][:, None], inp["sin"].double()[pos][:, None]
    o, rs = _qk_forward(x, gain, c, s, eps, torch.float64)
    out = dict(out=o.detach().reshape(M, nh * 128))
    if not backward:
        return out
    d = inp["dout"].double().view(M, nh, 128)
    (o * d).sum().backward()
    terms = ((d * c + _rot_t(d * s)) * (x * rs)).detach().abs()
    out.update(dqk=x.grad.reshape(M, nh * 128), dqg=qg.grad + (inp["dqg0"].double() if accumulate else 0),
               dkg=kg.grad + (inp["dkg0"].double() if accumulate else 0),
               dqg_n=M * Hq + int(accumulate), dkg_n=M * Hkv + int(accumulate),
               dqg_abs=terms[:, :Hq].sum((0, 1)) + (inp["dqg0"].double().abs() if accumulate else 0),
               dkg_abs=terms[:, Hq:].sum((0, 1)) + (inp["dkg0"].double().abs() if accumulate else 0))
    return out


def qk_fwd_f32(inp, T, Hq, Hkv, rstd32=None, eps=EPS, round_x=True, round_n=True, rot_sign=1.0, pos_div=False,
               k_uses_q_gain=False):
    """qknorm_rope_fwd_kernel in fp32, rounding where its comments say: out = bf16(n cos + rot(n) sin) with
    n = bf16(g * bf16(x * rstd)).  rstd32 [M, nh]: the statistic from outside (rule 3).  -> out bf16 [M, nh 128]."""
    M, nh = inp["qkv"].shape[0], Hq + Hkv
    x = inp["qkv"][:, :nh * 128].float().view(M, nh, 128)
    kg = inp["qg"] if k_uses_q_gain else inp["kg"]
    gain = torch.cat([inp["qg"].float()[None].expand(Hq, 128), kg.float()[None].expand(Hkv, 128)], 0)[None]
    pos = (torch.arange(M) // T) if pos_div else (torch.arange(M) % T)
    pos = pos.clamp_max(inp["cos"].shape[0] - 1)
    c, s = inp["cos"].float()[pos][:, None], inp["sin"].float()[pos][:, None]
    if rstd32 is None:
        rstd32 = torch.rsqrt(x.pow(2).sum(-1) * (1.0 / 128.0) + torch.tensor(eps, dtype=torch.float32))
    a = x * rstd32[..., None]
    a = a.to(BF).float() if round_x else a
    n = gain * a
    n = n.to(BF).float() if round_n else n
    return (n * c + rot_sign * _rot(n) * s).to(BF).reshape(M, nh * 128)


def qk_bwd_f32(inp, T, Hq, Hkv, eps=EPS):
    """qknorm_rope_bwd_kernel in fp32 -> (dqk fp32 before the store [M, nh 128], q gain sum, k gain sum)."""
    M, nh = inp["qkv"].shape[0], Hq + Hkv
    x = inp["qkv"][:, :nh * 128].float().view(M, nh, 128)
    gain = torch.cat([inp["qg"].float()[None].expand(Hq, 128), inp["kg"].float()[None].expand(Hkv, 128)], 0)[None]
    pos = torch.arange(M) % T
    c, s = inp["cos"].float()[pos][:, None], inp["sin"].float()[pos][:, None]
    d = inp["dout"].float().view(M, nh, 128)
    rs = torch.rsqrt(x.pow(2).sum(-1, keepdim=True) * (1.0 / 128.0) + torch.tensor(eps, dtype=torch.float32))
    dn = d * c + _rot_t(d * s)
    xh = x * rs
    dot = (dn * gain * x * rs).sum(-1, keepdim=True) * (1.0 / 128.0)
    o = rs * (dn * gain - xh * dot)
    gw = dn * xh
    return o.reshape(M, nh * 128), gw[:, :Hq].sum((0, 1)), gw[:, Hq:].sum((0, 1))


def qk_rstd64(inp, Hq, Hkv, eps=EPS):
    M, nh = inp["qkv"].shape[0], Hq + Hkv
    return rstd64(inp["qkv"][:, :nh * 128].view(M, nh, 128), eps)


def qk_fwd_bound(inp, T, Hq, Hkv, eps=EPS):
    """The interval rule for out = bf16(n cos + rot(n) sin), n = bf16(g * bf16(x * rstd)) -> bound [M, nh 128] fp64."""
    M, nh = inp["qkv"].shape[0], Hq + Hkv
    x = inp["qkv"][:, :nh * 128].double().view(M, nh, 128)
    gain = torch.cat([inp["qg"].double()[None].expand(Hq, 128), inp["kg"].double()[None].expand(Hkv, 128)], 0)[None]
    pos = torch.arange(M) % T
    c, s = inp["cos"].double()[pos][:, None], inp["sin"].double()[pos][:, None]
    xh = x * rstd64(x, eps)[..., None]
    a = xh.abs()
    e = FWD_FLOOR * a                         # x * rstd in fp32, rstd from an fp32 sum and rsqrtf
    e = e + half_ulp(a + e, BF)               # first inner rounding
    e = gain.abs() * e                        # exact product
    n = gain * xh
    e = e + half_ulp(n.abs() + e, BF)         # second inner rounding: n as HF holds it
    swap = (lambda t: torch.cat((t[..., 64:], t[..., :64]), -1))
    out = (n * c + _rot(n) * s).abs()         # the exact value; both products are exact in fp32
    e = e * c.abs() + swap(e) * s.abs()
    e = e + ULP32 * (out + e)                 # the one fp32 rounding of the sum
    return (e + half_ulp(out + e, BF)).reshape(M, nh * 128)  # the store: half an ulp at the top of the interval


# ------------------------------------------------------------------------------------------- SwiGLU
SWIGLU_CASES = [(1, 8), (7, 24), (70, 256), (1025, 8192)]
SWIGLU_FIXED_GATES = (0.0, 20.0, -20.0, 100.0, -100.0)  # the last five gate columns of every row (zero / one-hot rows apart)
# In the +-100 columns exp(100) has overflowed fp32 (HF's own fp32 silu returns +-0 there too) and the reference,
# 100 e^-100 u d = 3.7e-42 u d, is below half the smallest bf16 subnormal (2^-134 = 4.6e-41) as long as |u d| < 12.4:
# up and dact are clamped to +-3 in those two columns, so that "0" is the correctly rounded result.
SWIGLU_OVERFLOW_CLAMP = 3.0


@functools.lru_cache(maxsize=None)
def swiglu_inputs(M, I):
    """-> gu [M, 2I], dact [M, I] (bf16, CPU) and exempt [I] bool: the +-100 gate columns (judged on half_ulp alone).
    Random gates are clamped to +-16 after the row's scale (the premise of SWIGLU_FLOOR)."""
    gen = _gen(M, I, 77)
    shift = M % 5
    g = kinded(torch.randn(M, I, generator=gen) * 3, shift).clamp(-SWIGLU_GATE_MAX, SWIGLU_GATE_MAX)
    u = kinded(torch.randn(M, I, generator=gen) * 2, shift)
    d = kinded(torch.randn(M, I, generator=gen), shift)
    exempt = torch.zeros(I, dtype=torch.bool)
    live = torch.tensor([row_kind(r, shift) not in ("zero", "onehot") for r in range(M)])
    for j, val in enumerate(SWIGLU_FIXED_GATES):
        col = I - 5 + j
        g[live, col] = val
        if abs(val) == 100.0:
            exempt[col] = True
            u[:, col] = u[:, col].clamp(-SWIGLU_OVERFLOW_CLAMP, SWIGLU_OVERFLOW_CLAMP)
            d[:, col] = d[:, col].clamp(-SWIGLU_OVERFLOW_CLAMP, SWIGLU_OVERFLOW_CLAMP)
    return torch.cat([g, u], 1).to(BF), d.to(BF), exempt


def swiglu_ref(gu, dact=None, wrong_s=False):
    """fp64 -> dict(act, act_mag) and with dact: dg, du and the magnitudes their 2^-16 floors are taken of."""
    I = gu.shape[1] // 2
    g, u = gu[:, :I].double(), gu[:, I:].double()
    s = torch.sigmoid(g)
    out = dict(act=g * s * u)
    out["act_mag"] = out["act"].abs()
    if dact is not None:
        d = dact.double()
        t = s if wrong_s else 1 - s
        out.update(du=d * g * s, dg=d * u * s * (1 + g * t), du_mag=(d * g * s).abs(),
                   dg_mag=(d * u * s).abs() * (1 + g.abs() * (1 - s)))
    return out


def swiglu_f32(gu, dact=None):
    """The kernels' formulas in fp32 (libm exp) -> (act, dg, du) fp32 before the store."""
    I = gu.shape[1] // 2
    g, u = gu[:, :I].float(), gu[:, I:].float()
    act = g / (1.0 + torch.exp(-g)) * u
    if dact is None:
        return act, None, None
    d = dact.float()
    s = 1.0 / (1.0 + torch.exp(-g))
    return act, d * u * s * (1.0 + g * (1.0 - s)), d * g * s


Elem = collections.namedtuple("Elem", "ok row col got ref err bound ratio")


def elem_close(got, ref64, bound):
    """|got - ref| <= bound per element -> Elem(ok, row, col, got, ref, err, bound, worst err / bound).  A non-finite
    result fails.  An element whose bound and error are both 0 counts as ratio 0."""
    g = torch.as_tensor(got).detach().double().cpu()
    r = torch.as_tensor(ref64).detach().double().cpu()
    b = torch.as_tensor(bound).detach().double().cpu().expand_as(r)
    assert g.shape == r.shape, (g.shape, r.shape)
    g, r, b = (t.reshape(-1, t.shape[-1]) if t.dim() else t.reshape(1, 1) for t in (g, r, b))
    err = (g - r).abs()
    bad = ~(err <= b)
    ratio = torch.where(bad & ~torch.isfinite(err), torch.full_like(err, math.inf), err / b.clamp_min(1e-300))
    ratio = torch.where((err == 0) & (b == 0), torch.zeros_like(ratio), ratio)
    row, col = divmod(int(ratio.argmax()), g.shape[1])
    return Elem(not bool(bad.any()), row, col, float(g[row, col]), float(r[row, col]), float(err[row, col]),
                float(b[row, col]), float(ratio[row, col]))


def swiglu_bound(ref64, mag, exempt):
    """half_ulp(ref) + 2^-16 mag, the floor dropped in the exempt columns."""
    return half_ulp(ref64, BF) + SWIGLU_FLOOR * torch.where(exempt[None, :], torch.zeros_like(mag), mag)


def gain_bound(ref64, n, abs_sum):
    """Rule 4: half_ulp(ref) + (n + 8) 2^-24 sum|term|."""
    return half_ulp(ref64, BF) + (n + 8) * ULP32 * abs_sum


def differing_share(got, want):
    """Rule 3: the share of elements whose stored values differ (a NaN differs from everything)."""
    a, b = torch.as_tensor(got).detach().float().cpu(), torch.as_tensor(want).detach().float().cpu()
    return float((~(a == b)).double().mean())


def nudge_ulps(x32, k):
    """fp32 values moved by k ulps (positive, finite values)."""
    return (x32.contiguous().view(torch.int32) + k).view(torch.float32)


# ------------------------------------------------------------------------------------------- column sums, embedding
COLSUM_NB = (1, 7, 8, 9, 57, 64, 65, 121)
# (unrolled trips, tail trips) of row group 0 at each nb: the boundaries of the eight-way unrolled loop
COLSUM_TRIPS = {1: (0, 1), 7: (0, 1), 8: (0, 1), 9: (0, 2), 57: (1, 0), 64: (1, 0), 65: (1, 1), 121: (2, 0)}
COLSUM_H = (8, 40)
COLSUM_PAD = 24  # stride = H + 24; the padding columns hold NaN


def colsum_inputs(nb, H, seed=0):
    """Integer data -> partials [nb, H + COLSUM_PAD] fp32 (NaN beyond column H), out0 [H] bf16."""
    gen = _gen(nb, H, seed)
    p = torch.full((nb, H + COLSUM_PAD), float("nan"))
    p[:, :H] = torch.randint(-8, 9, (nb, H), generator=gen).float()
    return p, torch.randint(-64, 65, (H,), generator=gen).float().to(BF)


def colsum_ref(p, out0, H, accumulate):
    """Every partial sum is an integer below 2^24, so the fp32 sum is exact whatever its order: one bf16 rounding."""
    return (p[:, :H].double().sum(0) + (out0.double() if accumulate else 0)).to(BF)


EMB_FWD_CASES = [(M, H) for H in (8, 520, 1032) for M in (1, 5)]
EMB_V = 11
EMB_SSQ_CASES = [(M, H) for H in (512, 1536, 2048) for M in (1, 15, 16, 17)]
EMB_SSQ_REFUSED = {640: -3, 2560: -3}
EMB_BWD_M = (1, 31, 32, 33, 70)
EMB_BWD_V, EMB_BWD_H = 9, 24
EMB_SERIAL = dict(M=65537, H=8, V=40)


def emb_fwd_ids(M, V):
    """In-range ids with -3 and V + 2 among them (clamped by the kernel to rows 0 and V - 1)."""
    ids = (torch.arange(M) * 7 + 3) % V
    ids[0] = -3
    if M > 1:
        ids[M - 1] = V + 2
    return ids


def emb_fwd_ref(ids, E):
    return E[ids.clamp(0, E.shape[0] - 1)]


def emb_bwd_inputs(M, H, V, seed=0):
    """Integer data.  ids: duplicates on both sides of every 32-token word boundary, ids -1 and V among them (M > 2)."""
    gen = _gen(M, H, V, seed)
    ids = torch.randint(0, V, (M,), generator=gen)
    for b in range(32, M, 32):
        ids[b] = ids[b - 1]          # the same id at tokens 31 | 32, 63 | 64
    if M > 2:  # tokens 1 and 2: never one of the planted pairs b - 1 | b
        ids[1] = -1
        ids[2] = V
    dx = torch.randint(-8, 9, (M, H), generator=gen).float().to(BF)
    dE0 = torch.randint(-16, 17, (V, H), generator=gen).float().to(BF)
    return ids, dx, dE0


def emb_bwd_ref(ids, dx, dE0, scale=1.0, row_lo=0):
    """dE[id] = bf16(dE0[id] + scale * sum of the dx rows carrying id) for row_lo <= id < V; every other row as it was.
    On integer data with scale 1 or 0.5 everything before the single rounding is exact in fp32."""
    V = dE0.shape[0]
    keep = (ids >= row_lo) & (ids < V) & (ids >= 0)
    acc = torch.zeros(dE0.shape, dtype=torch.float64).index_add(0, ids[keep], dx[keep].double())
    touched = torch.zeros(V, dtype=torch.bool)
    touched[ids[keep]] = True
    return torch.where(touched[:, None], (dE0.double() + scale * acc).to(BF), dE0)


SCATTER_CASES = [(n, H) for H in (8, 520) for n in (0, 1, 5)]
SCATTER_M = 9


def scatter_rows(n, M):
    """n unique row indices with -1 and M among them (n >= 3); both are skipped by the kernel."""
    rows = (torch.arange(n) * 4 + 2) % M
    if n >= 3:
        rows[1], rows[n - 2] = -1, M
    return rows


def scatter_ref(src, rows, M):
    dst = torch.zeros(M, src.shape[1], dtype=src.dtype)
    keep = (rows >= 0) & (rows < M)
    dst[rows[keep]] = src[keep]
    return dst


# ------------------------------------------------------------------------------------------- floors
def _row_rel(a32, ref64):
    r = ref64.double().reshape(-1, ref64.shape[-1])
    e = (a32.double().reshape(r.shape) - r).abs().amax(-1)
    return float((e / r.abs().amax(-1).clamp_min(1e-300)).max())


def rms_bwd_runs(big=True):
    """[(name, inputs, dres on, accumulate)] of every RMSNorm backward run of the GPU test."""
    runs = [(f"M{M}_H{H}", rms_inputs(M, H), (M + RMS_H.index(H)) % 2 == 0, M % 3 == 0) for M, H in RMS_CASES]
    if big:
        runs += [(f"M{M}_H{H}_dres{int(dr)}_acc{int(ac)}", rms_inputs(M, H), dr, ac) for (M, H) in RMS_BWD_BIG
                 for dr in (True, False) for ac in (False, True)]
    runs += [(f"slabs{ns}_M{M}_H{H}", rms_inputs(M, H, ns), ns == 3, ns == 1) for M, H, ns in RMS_SLAB_CASES
             if big or M < 100]
    return runs


def rms_grad_of(inp):
    """The fp64 gradient a run's reference takes: dy, or the fp64 sum of the slabs."""
    return inp["dy"].double() if inp["slabs"] is None else inp["slabs"].double().sum(0)


def measure_floors(big=True):
    """Worst per-row error (relative to the row maximum) of each fp32 restatement against fp64, over every case of its
    family -> dict(rms_bwd, qk_bwd, rstd): the *_MEASURED constants above."""
    out = dict(rms_bwd=0.0, qk_bwd=0.0, rstd=0.0)
    eps32 = torch.tensor(EPS, dtype=torch.float32)
    for name, inp, dres_on, acc in rms_bwd_runs(big):
        x = inp["x"]
        r64 = rstd64(x)
        r32 = torch.rsqrt(x.float().pow(2).sum(-1) / float(x.shape[1]) + eps32)
        out["rstd"] = max(out["rstd"], float(((r32.double() - r64).abs() / r64).max()))
        dres = inp["dres"] if dres_on else None
        ref = rmsnorm_ref(x, inp["w"], rms_grad_of(inp), dres)
        dx32, _ = rmsnorm_bwd_f32(x, inp["w"], r64.float(), inp["dy"], inp["slabs"], dres)
        out["rms_bwd"] = max(out["rms_bwd"], _row_rel(dx32, ref["dx"]))
    for (B, T, Hq, Hkv, _blocks) in QK_BWD_CASES:
        if not big and B * T * (Hq + Hkv) > 1000:
            continue
        inp = qk_inputs(B, T, Hq, Hkv)
        ref = qk_ref(inp, T, Hq, Hkv, backward=True)
        o32, _, _ = qk_bwd_f32(inp, T, Hq, Hkv)
        out["qk_bwd"] = max(out["qk_bwd"], _row_rel(o32.reshape(-1, 128), ref["dqk"].reshape(-1, 128)))
    return out
