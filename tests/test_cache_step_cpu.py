"""CPU checks of the one-launch decode cache step (sd_cache_step, sd_qwen3_decode_step_fused,
sd_qwen3_mx_decode_step_fused; include/sd_hip.h "the cache step of a decode layer as ONE launch", generation.py
``decode_attention``): every error code of the new entries is decided before a launch, so it comes back on a machine
without a GPU; the size queries answer and grow with the batch and the capacity; the keyword is validated by each of the
five Python entry points before anything is allocated; scripts/generate.py knows the flag."""
import ctypes
import os
import sys

import pytest
import torch

from conftest import ROOT

SHAPE, ALIGN, UNSUP, WORK = -1, -2, -3, -5
P, BIG = 0x10000, 1 << 40


def _lib():
    import speech_distill_amd as sda
    return sda.load_lib()


def test_cache_step_refuses_before_any_launch():
    """The codes of the pair it replaces (sd_qknorm_rope_append* + sd_attn_decode*), for the three kinds of planes."""
    from speech_distill_amd import _lib as L
    lib = _lib()

    def planes(kind=0, k=P, v=P, ks=P, vs=P, cap=512, table=P, max_pages=2, n_pages=8):
        return ctypes.byref(L.KvPlanes(kind, k, v, ks, vs, cap, table, max_pages, n_pages))

    def step(kv, qkv=P, qg=P, kg=P, cos=P, sin=P, pos=P, o=P, lse=None, ws=P, nb=BIG, tickets=P, B=2, max_len=8, Hq=4,
             Hkv=2, hd=128):
        return lib.sd_cache_step(qkv, qg, kg, cos, sin, pos, kv, o, lse, ws, nb, tickets, B, max_len, Hq, Hkv, hd, 1e-6,
                                 0.0883883, None)

    need = lib.sd_cache_step_workspace_bytes(2, 4, 2, 512)
    assert need == lib.sd_attn_decode_workspace_bytes(2, 4, 512) > 0
    for kind in (0, 1, 2):
        kv = planes(kind)
        assert step(None) == SHAPE
        for name in ("qkv", "qg", "kg", "cos", "sin", "pos", "o", "tickets"):
            assert step(kv, **{name: None}) == SHAPE, (kind, name)
        assert step(planes(kind, k=None)) == SHAPE and step(planes(kind, v=None)) == SHAPE
        assert step(kv, B=0) == SHAPE and step(kv, max_len=0) == SHAPE and step(kv, max_len=-3) == SHAPE
        assert step(kv, Hq=0) == SHAPE and step(kv, Hkv=0) == SHAPE and step(kv, Hq=5) == SHAPE     # Hq % Hkv != 0
        assert step(kv, hd=64) == UNSUP
        assert step(kv, Hq=6, Hkv=2) == UNSUP and step(kv, Hq=8, Hkv=1) == UNSUP                   # G = 3, G = 8
        assert step(kv, Hq=2, Hkv=2, nb=0) == WORK and step(kv, Hq=8, Hkv=2, nb=0) == WORK         # G = 1, G = 4: known
        assert step(kv, nb=need - 1) == WORK and step(kv, ws=None) == WORK
        assert step(kv, qkv=P + 8) == ALIGN and step(kv, tickets=P + 2) == ALIGN and step(kv, ws=P + 2) == ALIGN
    assert step(planes(3)) == SHAPE and step(planes(-1)) == SHAPE                                # an unknown kind
    assert step(planes(0, cap=0)) == SHAPE
    for kind in (1, 2):
        assert step(planes(kind, table=None)) == SHAPE
        assert step(planes(kind, max_pages=0)) == SHAPE and step(planes(kind, n_pages=0)) == SHAPE
        assert step(planes(kind, max_pages=(1 << 22) + 1)) == SHAPE
    assert step(planes(2, ks=None)) == SHAPE and step(planes(2, vs=None)) == SHAPE
    assert step(planes(1, ks=None, vs=None), nb=0) == WORK          # the scale planes belong to kind 2 alone
    assert step(planes(0, table=None, max_pages=0, n_pages=0), nb=0) == WORK   # ... and the table to the paged kinds


def test_cache_step_workspace_query():
    lib = _lib()
    q = lib.sd_cache_step_workspace_bytes
    assert q(0, 4, 2, 512) == SHAPE and q(2, 0, 2, 512) == SHAPE and q(2, 4, 0, 512) == SHAPE and q(2, 4, 2, 0) == SHAPE
    assert q(2, 5, 2, 512) == SHAPE
    by_b = [q(B, 16, 8, 1024) for B in (1, 2, 5, 16, 64)]
    by_cap = [q(4, 16, 8, cap) for cap in (1, 256, 257, 768, 4096)]
    assert all(a < b for a, b in zip(by_b, by_b[1:])), by_b
    assert all(a <= b for a, b in zip(by_cap, by_cap[1:])) and by_cap[1] < by_cap[2] < by_cap[4], by_cap


def _refs(L):
    pages = L.KvPages(P, BIG, P, 8, 2)

    def ref(kind=0, cache=P, nbytes=BIG, cap=256, pg=None):
        return ctypes.byref(L.KvRef(kind, cache, nbytes, cap, ctypes.pointer(pg) if pg is not None else None))
    return pages, ref


def _step_refusals(step, ref, pages, L, hd64, g8):
    assert step(None) == SHAPE and step(ref(), d=None) == SHAPE and step(ref(), p=None) == SHAPE
    assert step(ref(kind=3)) == SHAPE and step(ref(kind=-1)) == SHAPE
    assert step(ref(cache=None)) == SHAPE and step(ref(cap=0)) == SHAPE
    assert step(ref(kind=1)) == SHAPE and step(ref(kind=2)) == SHAPE                   # paged kinds need the pages
    assert step(ref(), B=0) == SHAPE and step(ref(), ids=None) == SHAPE and step(ref(), pos=None) == SHAPE
    assert step(ref(), logits=None) == SHAPE and step(ref(), acts=None) == SHAPE
    assert step(ref(), max_len=0) == SHAPE and step(ref(), max_len=-1) == SHAPE
    assert step(ref(), cos=None) == SHAPE and step(ref(), sin=None) == SHAPE
    assert step(ref(nbytes=16)) == WORK and step(ref(), nb=16) == WORK
    assert step(ref(), acts=P + 4) == ALIGN and step(ref(cache=P + 8)) == ALIGN
    for kind in (1, 2):
        assert step(ref(kind=kind, pg=pages), nb=16) == WORK                           # a valid pool gets as far
        assert step(ref(kind=kind, pg=L.KvPages(P, 16, P, 8, 2))) == WORK
        assert step(ref(kind=kind, pg=L.KvPages(P, BIG, None, 8, 2))) == SHAPE
    assert step(ref(), d=hd64) == UNSUP and step(ref(), d=g8) == UNSUP


def test_fused_step_refuses_before_any_launch():
    """sd_qwen3_decode_step_fused: the codes of sd_qwen3_decode_step_wide, and `kernels` in {0, 1, 2}."""
    from speech_distill_amd import _lib as L
    lib = _lib()
    d, p = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)), ctypes.byref(L.Params())
    pages, ref = _refs(L)

    def step(kv, d=d, p=p, ids=P, pos=P, acts=P, nb=BIG, logits=P, B=2, max_len=8, kernels=1, cos=P, sin=P):
        return lib.sd_qwen3_decode_step_fused(d, p, ids, pos, max_len, cos, sin, kv, acts, nb, logits, B, kernels, None)

    hd64 = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    g8 = ctypes.byref(L.Dims(640, 256, 512, 2, 8, 1, 128, 1, 1e-6, 0))
    _step_refusals(step, ref, pages, L, hd64, g8)
    for bad in (-1, 3, 4, 0x100):
        assert step(ref(), kernels=bad) == SHAPE, bad
    for ok in (0, 1, 2):
        assert step(ref(), kernels=ok, nb=16) == WORK, ok                              # a known value gets as far
    # the existing entries did not learn a bit
    assert lib.sd_qwen3_decode_step_flags(d, p, P, P, 8, P, P, P, BIG, 256, P, BIG, P, 2, 2, None) == SHAPE
    assert lib.sd_abi_version() == 2


def test_mx_fused_step_refuses_before_any_launch():
    """sd_qwen3_mx_decode_step_fused: the codes of sd_qwen3_mx_decode_step, flags in {0, SD_DECODE_SKINNY}."""
    from speech_distill_amd import _lib as L
    lib = _lib()
    d, p = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)), ctypes.byref(L.ParamsMx())
    pages, ref = _refs(L)

    def step(kv, d=d, p=p, ids=P, pos=P, acts=P, nb=BIG, logits=P, B=2, max_len=8, flags=1, cos=P, sin=P):
        return lib.sd_qwen3_mx_decode_step_fused(d, p, ids, pos, max_len, cos, sin, kv, acts, nb, logits, B, flags, None)

    hd64 = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    g8 = ctypes.byref(L.Dims(640, 256, 512, 2, 8, 1, 128, 1, 1e-6, 0))
    _step_refusals(step, ref, pages, L, hd64, g8)
    for bad in (2, 3, 0x100, -1):
        assert step(ref(), flags=bad) == SHAPE, bad
    for ok in (0, 1):
        assert step(ref(), flags=ok, nb=16) == WORK, ok
    assert lib.sd_qwen3_mx_decode_step(d, p, P, P, 8, P, P, ref(), P, BIG, P, 2, 2, None) == SHAPE


def test_fused_acts_queries_hold_the_tickets_and_are_monotone():
    from speech_distill_amd import _lib as L
    lib = _lib()
    d = ctypes.byref(L.Dims(159488, 1024, 3072, 28, 16, 8, 128, 1, 1e-6, 0))
    for fused, split in ((lib.sd_qwen3_decode_step_fused_acts_bytes, lib.sd_qwen3_decode_acts_bytes),
                         (lib.sd_qwen3_mx_decode_step_fused_acts_bytes, lib.sd_qwen3_mx_decode_step_acts_bytes)):
        by_b = [fused(d, B, 1024) for B in (1, 2, 16, 17, 64)]
        by_cap = [fused(d, 4, cap) for cap in (256, 257, 1024, 8192)]
        assert all(a < b for a, b in zip(by_b, by_b[1:])), by_b
        assert all(a < b for a, b in zip(by_cap, by_cap[1:])), by_cap
        for B in (1, 5, 64):   # the twin's set + int32 [L][B][Hkv], rounded up to 256 bytes
            extra = fused(d, B, 1024) - split(d, B, 1024)
            assert 28 * B * 8 * 4 <= extra < 28 * B * 8 * 4 + 256, (B, extra)
        assert fused(d, 0, 1024) == SHAPE and fused(d, 4, 0) == SHAPE
        assert fused(ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0)), 4, 256) == UNSUP


def _cpu_model():
    import speech_distill_amd as sda
    return sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device="cpu", init_std=0)


def test_decode_attention_is_validated_by_every_entry_point_before_anything_is_allocated():
    from speech_distill_amd import generation as G
    from speech_distill_amd.engine import GenerationEngine
    assert G.DECODE_ATTENTION == ("split", "fused")
    ids = torch.zeros(1, 4, dtype=torch.int64)
    m = _cpu_model().requires_grad_(False)
    calls = {
        "Decoder": lambda v: G.Decoder(m, 1, 256, decode_attention=v),
        "generate": lambda v: m.generate(ids, max_new_tokens=2, do_sample=False, decode_attention=v),
        "start_session": lambda v: m.start_session(1, capacity=256, decode_attention=v),
        "GenerationSession": lambda v: G.GenerationSession(m, 1, 256, decode_attention=v),
        # (a pool that is no pool: the keyword is looked at first)
        "generation_engine": lambda v: m.generation_engine(object(), max_batch=2, decode_attention=v),
        "GenerationEngine": lambda v: GenerationEngine(m, object(), decode_attention=v),
    }
    for name, call in calls.items():
        for bad in ("merged", "", None, "FUSED"):
            with pytest.raises(ValueError, match="decode_attention"):
                call(bad)
    # it stays in front of the other keyword errors' allocations but behind nothing: a wrong decode_kernels is still named
    with pytest.raises(ValueError, match="decode_kernels"):
        m.generate(ids, max_new_tokens=2, decode_kernels="fast", decode_attention="fused")
    # "wide" with MXFP8 weights stays the error it is
    with pytest.raises(ValueError, match="wide"):
        G.Decoder(m, 1, 256, decode_kernels="wide", weight_dtype="mxfp8", decode_attention="fused")
    # both values pass every check and get as far as the CPU tensors
    for v in G.DECODE_ATTENTION:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.generate(ids, max_new_tokens=2, do_sample=False, decode_attention=v)


def test_generate_script_knows_the_flag():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import importlib
        gen = importlib.import_module("generate")
    finally:
        sys.path.pop(0)
    base = ["ckpt", "prompts.jsonl"]
    assert gen.parse_args(base).decode_attention == "split"
    assert gen.parse_args(base + ["--decode_attention", "fused"]).decode_attention == "fused"
    with pytest.raises(SystemExit):
        gen.parse_args(base + ["--decode_attention", "merged"])
