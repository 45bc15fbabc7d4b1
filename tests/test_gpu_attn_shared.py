"""-m gpu: the shared-page decode attention (sd_attn_decode_shared_paged{,_mx}; sd_attn_shared.hip) against its twin
(sd_attn_decode_paged{,_mx}) on the same inputs: ``torch.equal`` on o and lse, nothing looser.

The pool is 40 pages of finite random data that belongs to no row: what a row sees is decided by its table row and its
length alone, so any table is a valid input and both kernels must agree on it.  head_dim 128, three logical pages per
row.  Batches of 1, 3, R, R + 1 and 2 R + 3 rows (R = sd_attn_shared_group_rows) cover a lone row, a short group, a full
one, a group of one row behind a full one, and three groups.  Lengths are drawn from {0, 1, 255, 256, 257, 512, 600,
768}; every case also runs with a ``max_len`` of 300, below some rows' lengths.  MXFP8 pools hold random e4m3 codes
without the two NaN codes and scale bytes around 127."""
import itertools

import pytest
import torch

from gpu_util import dev

pytestmark = pytest.mark.gpu

D, PAGE, N_POOL, MAX_PAGES = 128, 256, 40, 3
LENGTHS = (0, 1, 255, 256, 257, 512, 600, 768)
GQA = ((4, 4), (4, 2), (4, 1))
LAYOUTS = ("identical", "distinct", "shared_head", "two_sets", "straddle", "moved_page", "unreached_minus_one")


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


_POOLS = {}


def pool(Hkv, mx):
    """The planes of one pool per (Hkv, dtype), made once and never written again."""
    if (Hkv, mx) not in _POOLS:
        g = torch.Generator().manual_seed(100 + Hkv + (50 if mx else 0))
        if mx:
            planes = []
            for _ in range(2):
                code = torch.randint(0, 254, (N_POOL, PAGE, Hkv * D), generator=g)
                code = code + (code >= 0x7F).long()            # 0 .. 254 without 0x7F: neither NaN code (0x7F, 0xFF)
                assert not bool(((code & 0x7F) == 0x7F).any())
                planes += [code.to(torch.uint8), torch.randint(120, 135, (N_POOL, PAGE, Hkv * 4), generator=g).to(torch.uint8)]
            _POOLS[Hkv, mx] = tuple(p.to(dev()) for p in planes)
        else:
            _POOLS[Hkv, mx] = tuple(torch.randn(N_POOL, PAGE, Hkv * D, generator=g).bfloat16().to(dev()) for _ in range(2))
    return _POOLS[Hkv, mx]


def pages_for(n):
    return (n + PAGE - 1) // PAGE


def layout(name, B, R, seed):
    """-> (table [B][3] as lists, lens [B]).  Private pages come from a ring over the pool's upper 28 pages: two rows can
    meet on one only when they are 9 or more rows apart, in different groups."""
    g = torch.Generator().manual_seed(seed)
    lens = [LENGTHS[i] for i in torch.randint(0, len(LENGTHS), (B,), generator=g).tolist()]
    if B > 1:
        lens[0], lens[1] = 600, 257          # whatever was drawn: a long row beside a shorter one on the same pages
    ring = itertools.cycle(range(12, N_POOL))      # pages 1 .. 11 are the shared ones below
    junk = lambda: int(torch.randint(0, N_POOL, (1,), generator=g))    # an entry no row reaches: any valid page
    rows = []
    for b in range(B):
        if name == "identical":              # one set; the lengths differ inside the pages
            row = [3, 7, 11]
        elif name == "distinct":
            row = [next(ring) for _ in range(MAX_PAGES)]
        elif name in ("shared_head", "unreached_minus_one"):   # the history's page, then private tails
            row = [5, next(ring), next(ring)]
        elif name == "two_sets":             # even rows on one history, odd rows on another, private last pages
            row = [1, 2, next(ring)] if b % 2 == 0 else [3, 4, next(ring)]
        elif name == "straddle":             # rows R-2 .. R+1 share, across the group boundary; the others own theirs
            row = [8, 9, 10] if R - 2 <= b <= R + 1 or B <= 3 else [next(ring) for _ in range(MAX_PAGES)]
        elif name == "moved_page":           # page 6 is logical page 0 of even rows and logical page 1 of odd rows
            row = [6, 7, next(ring)] if b % 2 == 0 else [7, 6, next(ring)]
        for i in range(pages_for(lens[b]), MAX_PAGES):
            row[i] = -1 if name == "unreached_minus_one" else junk()
        rows.append(row)
    return rows, lens


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("mx", [False, True], ids=["bf16", "mxfp8"])
@pytest.mark.parametrize("Hq,Hkv", GQA, ids=["g1", "g2", "g4"])
def test_bits_of_the_twin(ops, Hq, Hkv, mx, name):
    R = ops.attn_shared_group_rows(Hq, Hkv)
    assert R == (4 if Hq == Hkv else 2)
    planes = pool(Hkv, mx)
    twin = (lambda q, t, n, **kw: ops.attn_decode_paged_mx(q, planes, t, n, Hq, Hkv, want_lse=True, **kw)) if mx else \
        (lambda q, t, n, **kw: ops.attn_decode_paged(q, *planes, t, n, Hq, Hkv, want_lse=True, **kw))
    shared = (lambda q, t, n, **kw: ops.attn_decode_shared_paged_mx(q, planes, t, n, Hq, Hkv, want_lse=True, **kw)) if mx \
        else (lambda q, t, n, **kw: ops.attn_decode_shared_paged(q, *planes, t, n, Hq, Hkv, want_lse=True, **kw))
    for B in (1, 3, R, R + 1, 2 * R + 3):
        rows, lens = layout(name, B, R, seed=1000 * B + LAYOUTS.index(name))
        table = torch.tensor(rows, dtype=torch.int32, device=dev())
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
        q = torch.randn(B, Hq * D, generator=torch.Generator().manual_seed(B)).bfloat16().to(dev())
        for kw in (dict(), dict(max_len=300), dict(max_len=599, len_add=1)):
            if kw.get("len_add"):     # lens - 1 + 1: the runner's form (pos, len_add = 1); a length of 0 becomes -1 + 1
                n = lens_d - 1
            else:
                n = lens_d
            want_o, want_lse = twin(q, table, n, **kw)
            o, lse = shared(q, table, n, **kw)
            live = torch.tensor([min(x, kw.get("max_len", 768)) > 0 for x in lens], device=dev())
            assert torch.equal(o.view(torch.int16), want_o.view(torch.int16)), (B, kw, lens)
            assert torch.equal(lse.view(torch.int32), want_lse.view(torch.int32)), (B, kw, lens)
            assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse[live]).all()), (B, kw)


def test_sharing_is_not_needed_for_the_answer(ops):
    """Rows on identical pages against the same rows each on a private copy of those pages: the two tables describe the
    same keys, so every kernel gives the same bits -- the shared kernel on the shared table included."""
    Hq, Hkv, B = 4, 2, 8
    k, v = (p.clone() for p in pool(Hkv, False))
    lens = [600, 257, 768, 512, 513, 700, 1, 256]
    shared_rows = [[3, 7, 11]] * B
    private_rows = [[12 + 3 * b, 13 + 3 * b, 14 + 3 * b] for b in range(B)]
    for b in range(B):
        for i in range(MAX_PAGES):
            k[private_rows[b][i]], v[private_rows[b][i]] = k[shared_rows[b][i]], v[shared_rows[b][i]]
    q = torch.randn(B, Hq * D, generator=torch.Generator().manual_seed(4)).bfloat16().to(dev())
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    out = []
    for rows in (shared_rows, private_rows):
        t = torch.tensor(rows, dtype=torch.int32, device=dev())
        out.append(ops.attn_decode_shared_paged(q, k, v, t, lens_d, Hq, Hkv, want_lse=True))
        out.append(ops.attn_decode_paged(q, k, v, t, lens_d, Hq, Hkv, want_lse=True))
    for o, lse in out[1:]:
        assert torch.equal(o.view(torch.int16), out[0][0].view(torch.int16)) and torch.equal(lse, out[0][1])
