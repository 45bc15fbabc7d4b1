"""No GPU: what the 8-bit (MXFP8) pages of the paged KV cache rest on -- the exactness claim of include/sd_hip.h, the pool
size, the refusal codes of every ``_paged_mx`` entry (decided before any launch, and equal to the bf16 twin's), and the
host-side switches (``kv_dtype``, ``--kv_cache_dtype``)."""
import ctypes
import importlib.util
import os

import pytest
import torch

from conftest import ROOT

SHAPE, ALIGN, UNSUPPORTED, WORKSPACE = -1, -2, -3, -5
P = 0x1000   # a 16-byte aligned address that is never dereferenced: every call below returns before a launch


@pytest.fixture(scope="module")
def lib():
    import speech_distill_amd as sda
    return sda.load_lib()


# --------------------------------------------------------------------------------------------- 1. the exactness claim
def test_every_e4m3_code_times_the_scale_is_a_bf16_number_for_scale_bytes_3_to_246():
    """The bit contracts rest on this: bf16(float(q) * 2^e) rounds nothing for scale bytes 3..246, all 254 finite codes.
    Computed in fp64 (every product is exact there), rounded to bf16 through fp32 (every product is an fp32 normal or
    subnormal: the smallest is 2^-9 * 2^-124)."""
    codes = torch.arange(256, dtype=torch.uint8)
    val = codes.view(torch.float8_e4m3fn).to(torch.float64)
    finite = torch.isfinite(val)
    assert int(finite.sum()) == 254                     # 0x7F and 0xFF are the NaNs of e4m3fn
    val = val[finite]
    for sb in range(3, 247):
        x = torch.ldexp(val, torch.tensor(sb - 127))
        assert torch.equal(x.to(torch.float32).to(torch.float64), x), sb
        assert torch.equal(x.to(torch.float32).to(torch.bfloat16).to(torch.float64), x), sb
    # and the claim is sharp on both sides: the neighbours of the range lose a code
    for sb in (2, 247):
        x = torch.ldexp(val, torch.tensor(sb - 127))
        assert not torch.equal(x.to(torch.float32).to(torch.bfloat16).to(torch.float64), x), sb
    # an all-zero block (byte 0, codes 0) is zero whatever the scale
    assert float(torch.ldexp(torch.zeros(1, dtype=torch.float64), torch.tensor(-127))) == 0.0


# ------------------------------------------------------------------------------------------------------ 3. pool size
def test_pool_bytes_equal_the_documented_formula(lib):
    from speech_distill_amd import _lib
    for L, Hkv in ((2, 2), (28, 8)):
        d = ctypes.byref(_lib.Dims(640, 256, 512, L, 2 * Hkv, Hkv, 128, 1, 1e-6, 0))
        for n in (1, 3, 17):
            assert lib.sd_kvpool_mx_bytes(d, n) == L * 2 * n * 256 * Hkv * 132
            assert lib.sd_kvpool_mx_bytes(d, n) * 256 == lib.sd_kvpool_bytes(d, n) * 132
        assert lib.sd_kvpool_mx_bytes(d, 0) == lib.sd_kvpool_bytes(d, 0) == SHAPE
        assert lib.sd_kvpool_mx_bytes(d, -2) == SHAPE
    assert lib.sd_kvpool_mx_bytes(None, 4) == lib.sd_kvpool_bytes(None, 4) == UNSUPPORTED
    hd64 = ctypes.byref(_lib.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    assert lib.sd_kvpool_mx_bytes(hd64, 4) == UNSUPPORTED
    # per position: 59 136 bytes on the 0.6B / 1.7B shapes (28 layers, 8 kv heads), x0.516 of bf16's 114 688
    d = ctypes.byref(_lib.Dims(151936, 1024, 3072, 28, 16, 8, 128, 1, 1e-6, 0))
    assert lib.sd_kvpool_mx_bytes(d, 1) == 256 * 59136 and lib.sd_kvpool_bytes(d, 1) == 256 * 114688


# ------------------------------------------------------------------------------------- 2. refusal codes = the twins'
def _kernel_calls(lib, mx):
    """The five cache kernel entries as functions of the arguments the checks look at; mx: the _paged_mx entry, whose
    (k_data, k_scale, v_data, v_scale) stand where the twin takes (k_pool, v_pool)."""
    sfx = "_mx" if mx else ""

    def planes(pool):
        return (pool, P, P, P) if mx else (pool, P)

    def store(table=P, max_pages=2, n_pages=4, B=2, T=8, pool=P):
        return getattr(lib, "sd_kvcache_store_paged" + sfx)(P, P, *planes(pool), table, max_pages, n_pages, None, B, T, 4, 2,
                                                            None)

    def store_at(table=P, max_pages=2, n_pages=4, B=2, T=8, pool=P):
        return getattr(lib, "sd_kvcache_store_at_paged" + sfx)(P, P, *planes(pool), table, max_pages, n_pages, P, P, B, T, 4,
                                                               2, None)

    def append(table=P, max_pages=2, n_pages=4, B=2, pool=P):
        return getattr(lib, "sd_qknorm_rope_append_paged" + sfx)(P, P, P, P, P, P, P, *planes(pool), table, max_pages,
                                                                 n_pages, B, 4, 2, 1e-6, None)

    def decode(table=P, max_pages=2, n_pages=4, B=2, pool=P, Hq=4, Hkv=2, hd=128, ws=1 << 40):
        return getattr(lib, "sd_attn_decode_paged" + sfx)(P, *planes(pool), table, max_pages, n_pages, P, None, P, 0, P, ws,
                                                          B, 8, Hq, Hkv, hd, 0.1, None)

    def extend(table=P, max_pages=2, n_pages=4, B=2, T=8, pool=P, Hq=4, Hkv=2, hd=128):
        return getattr(lib, "sd_attn_extend_paged" + sfx)(P, *planes(pool), table, max_pages, n_pages, P, None, P, P,
                                                          Hq * 128, Hq * 128, B, T, Hq, Hkv, hd, 0.1, None)

    return store, store_at, append, decode, extend


KERNEL_CASES = [dict(table=None), dict(pool=None), dict(max_pages=0), dict(max_pages=-1), dict(n_pages=0), dict(n_pages=-3),
                dict(B=0)]


def test_mx_kernel_entries_refuse_before_any_launch_with_the_twins_codes(lib):
    mx, twin = _kernel_calls(lib, True), _kernel_calls(lib, False)
    for f, g in zip(mx, twin):
        for kw in KERNEL_CASES:
            assert f(**kw) == g(**kw) == SHAPE, (f.__name__, kw)
    for f, g in list(zip(mx, twin))[:2] + [(mx[4], twin[4])]:      # store, store_at, extend
        for T in (0, -1):
            assert f(T=T) == g(T=T) == SHAPE, f.__name__
    assert mx[0](T=513) == twin[0](T=513) == SHAPE                   # T > cap = 2 pages
    for f, g in list(zip(mx, twin))[3:]:                             # decode, extend
        assert f(hd=64) == g(hd=64) == UNSUPPORTED, f.__name__
        for Hq in (6, 16):                                           # Hq / Hkv outside {1, 2, 4}
            assert f(Hq=Hq, Hkv=2) == g(Hq=Hq, Hkv=2) == UNSUPPORTED, f.__name__
        assert f(Hq=5, Hkv=2) == g(Hq=5, Hkv=2) == SHAPE, f.__name__
    assert mx[3](ws=0) == twin[3](ws=0) == WORKSPACE
    # each of the four planes is checked, not only the first
    for i in range(4):
        pl = [P] * 4
        pl[i] = None
        assert lib.sd_kvcache_store_paged_mx(P, P, *pl, P, 2, 4, None, 2, 8, 4, 2, None) == SHAPE, i
        assert lib.sd_kvcache_store_at_paged_mx(P, P, *pl, P, 2, 4, P, P, 2, 8, 4, 2, None) == SHAPE, i
        assert lib.sd_qknorm_rope_append_paged_mx(P, P, P, P, P, P, P, *pl, P, 2, 4, 2, 4, 2, 1e-6, None) == SHAPE, i
        assert lib.sd_attn_decode_paged_mx(P, *pl, P, 2, 4, P, None, P, 0, P, 1 << 40, 2, 8, 4, 2, 128, 0.1, None) == SHAPE, i
        assert lib.sd_attn_extend_paged_mx(P, *pl, P, 2, 4, P, None, P, P, 512, 512, 2, 8, 4, 2, 128, 0.1, None) == SHAPE, i


def test_mx_runner_entries_refuse_before_any_launch_with_the_twins_codes(lib):
    from speech_distill_amd import _lib
    dims = _lib.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)
    d, p = ctypes.byref(dims), ctypes.byref(_lib.Params())
    per_page = {"": 2 * 2 * 256 * 2 * 128 * 2, "_mx": 2 * 2 * 256 * 2 * 132}     # L * 2 * 256 * Hkv * (256 | 132) bytes
    hd64 = ctypes.byref(_lib.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    g3 = ctypes.byref(_lib.Dims(640, 256, 512, 2, 6, 2, 128, 1, 1e-6, 0))

    def kv(pool=P, pool_bytes=1 << 40, table=P, n_pages=4, max_pages=2):
        return ctypes.byref(_lib.KvPages(pool, pool_bytes, table, n_pages, max_pages))

    def entries(sfx):
        def prefill(kvp, dd=d, B=2, T=8, acts_bytes=1 << 40):
            return getattr(lib, "sd_qwen3_prefill_paged" + sfx)(dd, p, P, P, P, P, P, acts_bytes, kvp, P, B, T, None)

        def extend(kvp, dd=d, B=2, T=8, acts_bytes=1 << 40):
            return getattr(lib, "sd_qwen3_extend_paged" + sfx)(dd, p, P, P, P, P, P, P, acts_bytes, kvp, P, B, T, None)

        def step(kvp, dd=d, B=2, T=8, acts_bytes=1 << 40, flags=0):
            return getattr(lib, "sd_qwen3_decode_step_paged" + sfx)(dd, p, P, P, 8, P, P, kvp, P, acts_bytes, P, B, flags,
                                                                    None)
        return prefill, extend, step

    for sfx in ("_mx", ""):      # the same table of cases for the new entries and for their twins
        prefill, extend, step = entries(sfx)
        for f in (prefill, extend, step):
            assert f(None) == SHAPE, f.__name__
            assert f(kv(pool=None)) == SHAPE and f(kv(table=None)) == SHAPE, f.__name__
            assert f(kv(n_pages=0)) == SHAPE and f(kv(max_pages=0)) == SHAPE and f(kv(max_pages=-2)) == SHAPE, f.__name__
            assert f(kv(pool_bytes=4 * per_page[sfx] - 1)) == WORKSPACE, f.__name__
            assert f(kv(), B=0) == SHAPE, f.__name__
            assert f(kv(), dd=hd64) == UNSUPPORTED, f.__name__
            assert f(kv(pool_bytes=4 * per_page[sfx]), acts_bytes=0) == WORKSPACE, f.__name__
        for f in (prefill, extend):
            assert f(kv(), T=0) == SHAPE and f(kv(), T=513) == SHAPE, f.__name__
        for f in (extend, step):
            assert f(kv(), dd=g3) == UNSUPPORTED, f.__name__
        assert step(kv(), flags=2) == SHAPE and step(kv(), flags=0x100) == SHAPE and step(kv(), flags=3) == SHAPE
        assert step(kv(), flags=1, acts_bytes=0) == WORKSPACE        # SD_DECODE_SKINNY is honoured as far as the check
    # the 8-bit pool is held against ITS size: a pool that suffices for 8-bit pages does not for bf16 ones
    prefill_mx, prefill = entries("_mx")[0], entries("")[0]
    assert prefill_mx(kv(pool_bytes=4 * per_page["_mx"]), acts_bytes=0) == WORKSPACE     # passed the pool check
    assert prefill(kv(pool_bytes=4 * per_page["_mx"])) == WORKSPACE


# ------------------------------------------------------------------------------------------------ host-side switches
def test_an_unknown_kv_dtype_is_refused_before_anything_is_allocated():
    from speech_distill_amd.paged import KV_DTYPES, PagePool, check_kv_dtype
    assert KV_DTYPES == ("bf16", "mxfp8")
    for ok in KV_DTYPES:
        check_kv_dtype(ok)
    for bad in ("fp8", "int8", None, "MXFP8"):
        with pytest.raises(ValueError):
            check_kv_dtype(bad)
        with pytest.raises(ValueError):
            PagePool(object(), 4, kv_dtype=bad)     # no model is touched: the dtype is looked at first


def _cli():
    spec = importlib.util.spec_from_file_location("sd_generate_script_mx", os.path.join(ROOT, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_kv_cache_dtype_defaults_to_bf16_and_mxfp8_needs_a_pool(capsys):
    mod = _cli()
    base = ["/checkpoint", "/prompts.jsonl"]
    args = mod.parse_args(base)
    assert args.kv_cache_dtype == "bf16" and args.kv_pool_pages == 0
    assert mod.parse_args(base + ["--kv_pool_pages", "8", "--kv_cache_dtype", "mxfp8"]).kv_cache_dtype == "mxfp8"
    assert mod.parse_args(base + ["--kv_pool_pages", "8"]).kv_cache_dtype == "bf16"
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--kv_cache_dtype", "mxfp8"])
    assert "--kv_pool_pages" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--kv_pool_pages", "8", "--kv_cache_dtype", "fp8"])
