"""CPU checks of the shared-page decode attention (sd_attn_shared_group_rows, sd_attn_decode_shared_paged{,_mx},
sd_qwen3_decode_step_shared, sd_qwen3_mx_decode_step_shared; include/sd_hip.h "decode attention for rows that SHARE
pages", generation.py ``shared_kv_reads``): every error code of the new entries is decided before a launch, so it comes
back on a machine without a GPU; the size queries are the twins'; the keyword is validated by each Python entry point
before anything is allocated, and is off by default."""
import ctypes
import inspect

import pytest
import torch

SHAPE, ALIGN, UNSUP, WORK = -1, -2, -3, -5
P, BIG = 0x10000, 1 << 40


def _lib():
    import speech_distill_amd as sda
    return sda.load_lib()


def test_group_rows_rule():
    """4 query heads per workgroup (8 where Hq / Hkv = 4): R = 4 for Hq == Hkv, 2 for Hq / Hkv in {2, 4}."""
    rows = _lib().sd_attn_shared_group_rows
    assert rows(4, 4) == 4 and rows(16, 16) == 4
    assert rows(4, 2) == 2 and rows(16, 8) == 2
    assert rows(4, 1) == 2 and rows(32, 8) == 2
    assert rows(0, 2) == SHAPE and rows(4, 0) == SHAPE and rows(-4, 2) == SHAPE and rows(5, 2) == SHAPE
    assert rows(6, 2) == UNSUP and rows(8, 1) == UNSUP
    from speech_distill_amd import ops
    assert ops.attn_shared_group_rows(16, 8) == 2


def _attn(mx):
    lib = _lib()

    def call(q=P, k=P, v=P, ks=P, vs=P, table=P, max_pages=3, n_pages=40, o=P, lse=None, lens=P, len_add=0, ws=P, nb=BIG,
             B=5, max_len=768, Hq=4, Hkv=2, hd=128, shared=True):
        planes = (k, ks, v, vs) if mx else (k, v)
        name = "sd_attn_decode_%spaged%s" % ("shared_" if shared else "", "_mx" if mx else "")
        return getattr(lib, name)(q, *planes, table, max_pages, n_pages, o, lse, lens, len_add, ws, nb, B, max_len, Hq, Hkv,
                                  hd, 0.0883883, None)
    return call


@pytest.mark.parametrize("mx", [False, True], ids=["bf16", "mxfp8"])
def test_attention_entries_refuse_as_their_twins_before_any_launch(mx):
    lib, call = _lib(), _attn(mx)
    need = lib.sd_attn_decode_workspace_bytes(5, 4, 768)
    cases = [dict(hd=64), dict(table=None), dict(max_pages=0), dict(n_pages=0), dict(max_pages=(1 << 22) + 1), dict(B=0),
             dict(B=-2), dict(max_len=0), dict(Hq=0), dict(Hkv=0), dict(Hq=5), dict(lens=None), dict(q=None), dict(k=None),
             dict(v=None), dict(o=None), dict(Hq=6, Hkv=2), dict(Hq=8, Hkv=1), dict(B=65536), dict(nb=need - 1), dict(nb=0),
             dict(ws=None), dict(Hq=2, Hkv=2, nb=0), dict(Hq=8, Hkv=2, nb=0),
             dict(hd=64, table=None), dict(table=None, Hq=6), dict(Hq=6, nb=0)]      # the order of the checks
    if mx:
        cases += [dict(ks=None), dict(vs=None)]
    for kw in cases:
        got, twin = call(**kw), call(shared=False, **kw)
        assert got == twin and got < 0, (kw, got, twin)
    assert call(hd=64) == UNSUP and call(table=None) == SHAPE and call(q=None) == SHAPE and call(Hq=6, Hkv=2) == UNSUP
    assert call(nb=need - 1) == WORK and call(ws=None) == WORK and call(max_len=0) == SHAPE and call(B=0) == SHAPE


def _refs(L):
    pages = L.KvPages(P, BIG, P, 8, 2)

    def ref(kind=1, cache=P, nbytes=BIG, cap=256, pg=pages):
        return ctypes.byref(L.KvRef(kind, cache, nbytes, cap, ctypes.pointer(pg) if pg is not None else None))
    return pages, ref


def _step_refusals(step, ref, L):
    hd64 = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    g8 = ctypes.byref(L.Dims(640, 256, 512, 2, 8, 1, 128, 1, 1e-6, 0))
    assert step(None) == SHAPE and step(ref(), d=None) == SHAPE and step(ref(), p=None) == SHAPE
    assert step(ref(kind=0, pg=None)) == SHAPE                      # a contiguous cache, however valid: rows share nothing
    assert step(ref(kind=0, pg=None), nb=16) == SHAPE
    assert step(ref(kind=3)) == SHAPE and step(ref(kind=-1)) == SHAPE
    assert step(ref(kind=1, pg=None)) == SHAPE and step(ref(kind=2, pg=None)) == SHAPE     # paged kinds need the pages
    assert step(ref(), B=0) == SHAPE and step(ref(), ids=None) == SHAPE and step(ref(), pos=None) == SHAPE
    assert step(ref(), logits=None) == SHAPE and step(ref(), acts=None) == SHAPE
    assert step(ref(), max_len=0) == SHAPE and step(ref(), max_len=-1) == SHAPE
    assert step(ref(), cos=None) == SHAPE and step(ref(), sin=None) == SHAPE
    for kind in (1, 2):
        assert step(ref(kind=kind), nb=16) == WORK                                     # a valid pool gets as far
        assert step(ref(kind=kind, pg=L.KvPages(P, 16, P, 8, 2))) == WORK
        assert step(ref(kind=kind, pg=L.KvPages(P, BIG, None, 8, 2))) == SHAPE
        assert step(ref(kind=kind, pg=L.KvPages(P, BIG, P, 0, 2))) == SHAPE
        assert step(ref(kind=kind, pg=L.KvPages(P, BIG, P, 8, 0))) == SHAPE
    assert step(ref(), d=hd64) == UNSUP and step(ref(), d=g8) == UNSUP


def test_shared_step_refuses_before_any_launch():
    """sd_qwen3_decode_step_shared: the codes of sd_qwen3_decode_step_fused, `kernels` in {0, 1, 2}, kind 0 refused."""
    from speech_distill_amd import _lib as L
    lib = _lib()
    d, p = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)), ctypes.byref(L.Params())
    pages, ref = _refs(L)

    def step(kv, d=d, p=p, ids=P, pos=P, acts=P, nb=BIG, logits=P, B=2, max_len=8, kernels=1, cos=P, sin=P):
        return lib.sd_qwen3_decode_step_shared(d, p, ids, pos, max_len, cos, sin, kv, acts, nb, logits, B, kernels, None)

    _step_refusals(step, ref, L)
    for bad in (-1, 3, 4, 0x100):
        assert step(ref(), kernels=bad) == SHAPE, bad
    for ok in (0, 1, 2):
        assert step(ref(), kernels=ok, nb=16) == WORK, ok                              # a known value gets as far
    # the existing entries did not learn a bit
    assert lib.sd_qwen3_decode_step_flags(d, p, P, P, 8, P, P, P, BIG, 256, P, BIG, P, 2, 2, None) == SHAPE
    assert lib.sd_qwen3_decode_step_paged(d, p, P, P, 8, P, P, ctypes.byref(pages), P, BIG, P, 2, 2, None) == SHAPE
    assert lib.sd_abi_version() == 2


def test_mx_shared_step_refuses_before_any_launch():
    """sd_qwen3_mx_decode_step_shared: the codes of sd_qwen3_mx_decode_step_fused, flags in {0, SD_DECODE_SKINNY}."""
    from speech_distill_amd import _lib as L
    lib = _lib()
    d, p = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)), ctypes.byref(L.ParamsMx())
    pages, ref = _refs(L)

    def step(kv, d=d, p=p, ids=P, pos=P, acts=P, nb=BIG, logits=P, B=2, max_len=8, flags=1, cos=P, sin=P):
        return lib.sd_qwen3_mx_decode_step_shared(d, p, ids, pos, max_len, cos, sin, kv, acts, nb, logits, B, flags, None)

    _step_refusals(step, ref, L)
    for bad in (2, 3, 0x100, -1):
        assert step(ref(), flags=bad) == SHAPE, bad
    for ok in (0, 1):
        assert step(ref(), flags=ok, nb=16) == WORK, ok
    assert lib.sd_qwen3_mx_decode_step(d, p, P, P, 8, P, P, ref(), P, BIG, P, 2, 2, None) == SHAPE


def test_shared_acts_queries_are_the_twins():
    from speech_distill_amd import _lib as L
    lib = _lib()
    d = ctypes.byref(L.Dims(159488, 1024, 3072, 28, 16, 8, 128, 1, 1e-6, 0))
    for shared, twin in ((lib.sd_qwen3_decode_step_shared_acts_bytes, lib.sd_qwen3_decode_acts_bytes),
                         (lib.sd_qwen3_mx_decode_step_shared_acts_bytes, lib.sd_qwen3_mx_decode_step_acts_bytes)):
        for B, cap in ((1, 256), (8, 1024), (16, 8192), (64, 257)):
            assert shared(d, B, cap) == twin(d, B, cap) > 0
        assert shared(d, 0, 1024) == SHAPE and shared(d, 4, 0) == SHAPE
        assert shared(ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0)), 4, 256) == UNSUP


def _cpu_model():
    import speech_distill_amd as sda
    return sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device="cpu", init_std=0)


def test_shared_kv_reads_is_off_by_default_and_validated_before_anything_is_allocated():
    from speech_distill_amd import generation as G
    assert G.DECODE_ATTENTION == ("split", "fused") and G.DECODE_KERNELS == ("tile", "skinny", "wide")
    m = _cpu_model().requires_grad_(False)
    for fn in (G.Decoder.__init__, G.GenerationSession.__init__, m.start_session):
        assert inspect.signature(fn).parameters["shared_kv_reads"].default is False, fn
    assert inspect.signature(G.GenerationSession.fork).parameters["shared_kv_reads"].default is None

    class NoPool:   # a pool that is no pool: reaching for it fails loudly, so the keyword was looked at first
        def __getattr__(self, name):
            raise AssertionError("the pool was touched before the keyword was checked")

    calls = {
        "Decoder": lambda **kw: G.Decoder(m, 1, 256, **kw),
        "GenerationSession": lambda **kw: G.GenerationSession(m, 1, 256, **kw),
        "start_session": lambda **kw: m.start_session(1, capacity=256, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="shared_kv_reads"):       # no pool
            call(shared_kv_reads=True)
        with pytest.raises(ValueError, match="shared_kv_reads"):       # the one-launch cache step
            call(shared_kv_reads=True, pool=NoPool(), decode_attention="fused")
        with pytest.raises(ValueError, match="decode_attention"):      # the older keyword is still named first
            call(shared_kv_reads=True, pool=NoPool(), decode_attention="merged")
    # fork: a contiguous session stays the error it is; a fused paged session refuses the keyword before the pool is used
    s = G.GenerationSession.__new__(G.GenerationSession)
    s.pool, s.decode_attention, s.shared_kv_reads, s.B = None, "split", False, 1
    with pytest.raises(ValueError, match="page pool"):
        s.fork([0], shared_kv_reads=True)
    # the default passes every check and gets as far as the CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.start_session(1, capacity=256, shared_kv_reads=False)
    f = G.GenerationSession.__new__(G.GenerationSession)
    f.pool, f.decode_attention, f.shared_kv_reads, f.B = NoPool(), "fused", False, 1
    with pytest.raises(ValueError, match="shared_kv_reads"):
        f.fork([0], shared_kv_reads=True)
    f.pool = None   # (nothing for __del__ to release)
