"""-m gpu: the one-launch decode cache step (sd_cache_step; speech_distill_amd/csrc/sd_cache_step.hip) and the decode steps
on it (sd_qwen3_decode_step_fused, sd_qwen3_mx_decode_step_fused).

The yardstick is the pair of entries it replaces -- sd_qknorm_rope_append* followed by sd_attn_decode*(len_add = 1) -- and
the step entries built on that pair.  Everything is torch.equal: o, lse, logits, and the WHOLE cache or pool buffer, slots
the step must not touch included.  The caches start from a fixed non-zero fill, so a stray store shows."""
import ctypes as C

import pytest
import torch

from gpu_util import dev
from test_gpu_mx import SHP, _model, _weights

pytestmark = pytest.mark.gpu

HKV, CAP, B, D = 2, 768, 5, 128
KINDS = ("contig", "paged", "paged_mx")
N_PAGES = 16
# (pos, max_len): every partition edge of a 768-slot row; then fewer partitions on the same workspace and tickets (stale
# records must not matter); then rows that store nothing (pos outside [0, cap)), n = 0, and a bound below pos + 1
CASES = (([0, 255, 256, 600, 767], CAP), ([1, 257, 511, 512, 3], CAP), ([-1, 768, 773, 300, 300], 256))


@pytest.fixture(scope="module")
def ops():
    import speech_distill_amd as sda
    from speech_distill_amd import ops as ops_
    sda.load_lib()
    return ops_


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=dev())


def _table():
    """int32 [B, 3] over a pool of 16 pages, handed out in a shuffled order: rows 2 and 3 share their full first page
    (neither ever appends below position 256), entries no case reaches are -1."""
    order = torch.randperm(N_PAGES, generator=torch.Generator().manual_seed(5)).tolist()
    take = iter(order)
    t = [[next(take), -1, -1], [next(take), next(take), -1], [next(take), next(take), -1]]
    t.append([t[2][0], next(take), next(take)])
    t.append([next(take), next(take), next(take)])
    return i32(t)


def _cache(kind, seed):
    """The planes of one layer, filled with fixed non-zero values that are also sane keys and values."""
    g = torch.Generator().manual_seed(seed)
    KD = HKV * D
    if kind == "contig":
        return tuple((torch.randn(B, CAP, KD, generator=g) * 0.5 + 0.01).to(torch.bfloat16).to(dev()) for _ in range(2))
    if kind == "paged":
        return tuple((torch.randn(N_PAGES, 256, KD, generator=g) * 0.5 + 0.01).to(torch.bfloat16).to(dev()) for _ in range(2))
    out = []
    for _ in range(2):
        data = torch.randint(1, 256, (N_PAGES, 256, KD), generator=g, dtype=torch.int32)
        data = torch.where((data & 0x7F) == 0x7F, torch.full_like(data, 0x3C), data).to(torch.uint8)   # no e4m3 NaN
        scale = torch.randint(118, 130, (N_PAGES, 256, HKV * 4), generator=g, dtype=torch.int32).to(torch.uint8)
        out += [data.to(dev()), scale.to(dev())]
    return tuple(out)   # (k_data, k_scale, v_data, v_scale)


def _pair(ops, kind, qkv, qg, kg, cos, sin, pos, planes, table, Hq, max_len, ws):
    """The two entries the cache step replaces, on `planes` (modified in place)."""
    if kind == "contig":
        q = ops.qknorm_rope_append(qkv, qg, kg, cos, sin, pos, planes[0], planes[1], Hq, HKV)
        return ops.attn_decode(q, planes[0], planes[1], pos, Hq, HKV, max_len, 1, True, ws)
    if kind == "paged":
        q = ops.qknorm_rope_append_paged(qkv, qg, kg, cos, sin, pos, planes[0], planes[1], table, Hq, HKV)
        return ops.attn_decode_paged(q, planes[0], planes[1], table, pos, Hq, HKV, max_len, 1, True, ws)
    q = ops.qknorm_rope_append_paged_mx(qkv, qg, kg, cos, sin, pos, planes, table, Hq, HKV)
    return ops.attn_decode_paged_mx(q, planes, table, pos, Hq, HKV, max_len, 1, True, ws)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Hq", (2, 4, 8))
def test_cache_step_equals_append_plus_decode_attention_bit_for_bit(ops, kind, Hq):
    from speech_distill_amd._lib import load_lib
    g = torch.Generator().manual_seed(100 + Hq)
    qg = (1 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16).to(dev())
    kg = (1 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16).to(dev())
    cos, sin = ops.rope_tables(CAP, dev())
    table = None if kind == "contig" else _table()
    want_planes, got_planes = _cache(kind, 7), _cache(kind, 7)
    start = [p.clone() for p in want_planes]
    nb = load_lib().sd_cache_step_workspace_bytes(B, Hq, HKV, CAP)
    ws_pair = torch.empty(nb, dtype=torch.uint8, device=dev())
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev())     # NaN records: a stale one that is read shows
    tickets = torch.zeros(B, HKV, dtype=torch.int32, device=dev())
    fused_planes = got_planes if kind == "paged_mx" else got_planes[:2]
    for case, (pos_l, max_len) in enumerate(CASES):
        pos = i32(pos_l)
        qkv = torch.randn(B, (Hq + 2 * HKV) * D, generator=g).to(torch.bfloat16).to(dev())
        o_w, lse_w = _pair(ops, kind, qkv, qg, kg, cos, sin, pos, want_planes, table, Hq, max_len, ws_pair)
        o_g, lse_g = ops.cache_step(qkv, qg, kg, cos, sin, pos, fused_planes, Hq, HKV, table=table, max_len=max_len,
                                    want_lse=True, workspace=ws, tickets=tickets)
        assert torch.equal(o_g.view(torch.int16), o_w.view(torch.int16)), (case, "o")
        assert torch.equal(lse_g.view(torch.int32), lse_w.view(torch.int32)), (case, "lse")
        for i, (a, b) in enumerate(zip(got_planes, want_planes)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (case, "plane", i)
        assert int(tickets.abs().max()) == 0, (case, tickets)
        # lse = None is accepted and changes nothing else (the runner passes none)
        o_n = ops.cache_step(qkv, qg, kg, cos, sin, pos, fused_planes, Hq, HKV, table=table, max_len=max_len, workspace=ws,
                             tickets=tickets)
        assert torch.equal(o_n.view(torch.int16), o_w.view(torch.int16)) and int(tickets.abs().max()) == 0
        for a, b in zip(got_planes, want_planes):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # the yardstick itself appended something, and not everything
    changed = sum(int((a.view(torch.uint8) != b.view(torch.uint8)).sum()) for a, b in zip(want_planes, start))
    assert 0 < changed < sum(p.numel() * p.element_size() for p in start) // 50


# ------------------------------------------------------------------------------------------------------ step parity
STEP_B, STEP_T, STEP_CAP = 3, 254, 512


@pytest.fixture(scope="module")
def model():
    import speech_distill_amd as sda
    sda.load_lib()
    _, w = _weights(9)
    return _model(sda, w)


def _decoder(model, kind, kernels, weight_dtype, decode_attention):
    from speech_distill_amd.generation import Decoder
    pool = None
    if kind != "contig":
        order = torch.randperm(10, generator=torch.Generator().manual_seed(3)).tolist()
        pool = model.kv_page_pool(10, order=order, kv_dtype="mxfp8" if kind == "paged_mx" else "bf16")
        pool.buffer.fill_(0x3C)
    dec = Decoder(model, STEP_B, STEP_CAP, kernels, pool=pool, weight_dtype=weight_dtype, decode_attention=decode_attention)
    if pool is None:
        dec.cache.fill_(0x3C)
    else:
        dec.reserve([STEP_CAP] * STEP_B)
    return dec


@pytest.mark.parametrize("weight_dtype,kernels", [("bf16", "tile"), ("bf16", "skinny"), ("bf16", "wide"),
                                                  ("mxfp8", "tile"), ("mxfp8", "skinny")])
def test_fused_steps_equal_the_split_steps_across_a_partition_and_page_edge(model, weight_dtype, kernels):
    """Four consecutive steps at positions 254 .. 257 (row 1 one behind, row 2 far behind): logits after every step and the
    whole cache or pool after the last, for the three kinds of cache."""
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(0, SHP[0], (STEP_B, STEP_T), generator=g).to(dev())
    cont = torch.randint(0, SHP[0], (STEP_B, 4), generator=g).to(dev())
    lens = [STEP_T, STEP_T - 1, 9]
    for kind in KINDS:
        out = {}
        for mode in ("split", "fused"):
            dec = _decoder(model, kind, kernels, weight_dtype, mode)
            kv_len = i32(lens)
            logits = [dec.prefill(ids, kv_len).clone()]
            for t in range(4):
                logits.append(dec.step(cont[:, t].contiguous(), (kv_len + t).contiguous(), STEP_T + t + 1).clone())
            buf = dec.cache if dec.pool is None else dec.pool.buffer
            out[mode] = (torch.stack(logits), buf.clone())
            dec.close()
        for t in range(5):
            assert torch.equal(out["fused"][0][t].view(torch.int16), out["split"][0][t].view(torch.int16)), (kind, t)
        assert torch.equal(out["fused"][1], out["split"][1]), kind
        assert not torch.equal(out["split"][0][1], out["split"][0][4])     # (the steps did move)


def test_fused_skinny_step_is_two_launches_per_layer_shorter(model):
    """The library's launch profiler over one decode step: 7 L + 2 kernel launches split, 5 L + 2 fused, of which L are the
    cache step (the memset of the tickets is no kernel launch)."""
    from speech_distill_amd import ops
    L = model.dims.num_hidden_layers
    counts = {}
    for mode in ("split", "fused"):
        dec = _decoder(model, "contig", "skinny", "bf16", mode)
        g = torch.Generator().manual_seed(4)
        ids = torch.randint(0, SHP[0], (STEP_B, 8), generator=g).to(dev())
        nxt = torch.randint(0, SHP[0], (STEP_B,), generator=g).to(dev())
        kv_len = i32([8] * STEP_B)
        dec.prefill(ids, kv_len)
        ops.prof_begin()
        dec.step(nxt, kv_len, 9)
        ops.prof_end()
        counts[mode] = {sym: int(v[2]) for sym, v in ops.prof_symbols().items()}
    n = {m: sum(c.values()) for m, c in counts.items()}
    assert n["split"] == 7 * L + 2, counts["split"]
    assert n["fused"] == 5 * L + 2, counts["fused"]
    assert sum(v for s, v in counts["fused"].items() if s.startswith("cache_step_kernel")) == L, counts["fused"]
    assert not any(s.startswith(("attn_decode", "qknorm_rope_append")) for s in counts["fused"]), counts["fused"]
