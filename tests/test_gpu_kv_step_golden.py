"""-m gpu: the per-layer cache step of a decode -- sd_qknorm_rope_append*, sd_attn_decode* and sd_cache_step
(csrc/sd_decode.hip and csrc/sd_cache_step.hip over the device functions of csrc/sd_kv_dev.cuh) -- writes the bits it wrote
when each kernel carried its own statement of the q/k-norm + RoPE, the key loop and the two merges and left the
contraction of their multiply-adds to the compiler.

tests/golden/kv_step/ holds the outputs of commit 6dac744 ("LoRA kernels: exact and per-element parity, write bounds, fp32
AdamW"), the commit before that change, on the seeded inputs below (written by
`SD_HIP_LIB=<that build's libsd_hip.so> python tests/test_gpu_kv_step_golden.py --record DIR`): whole arrays for q, o and
lse, SHA-256 digests of the bytes for cache planes, pools and scale planes.  Every q, o and lse lies in a buffer pre-filled
with the NaN sentinel of tests/test_gpu_gemv.py with two guard rows above and below, and the WHOLE buffer is compared: a
stray write fails like a wrong bit.  The planes are digested whole, slots no call may touch included.

Inputs: CPU torch.Generator, fixed seeds, randn times exact power-of-two row magnitudes; the cos / sin tables are seeded
random bf16 in [-1, 1] (no host transcendental enters a fixture); gains 1 + 0.25 randn; the cache rows that are there before
a call are seeded bf16, written into MXFP8 pages by sd_kvcache_store_paged_mx; a shuffled page table over a larger pool.
Hkv = 2, Hq in {2, 4, 8} (G = 1, 2, 4), the three cache kinds, cap = 768 (three partitions), one batch of 11 rows whose
visible lengths are N_VIS: the masks inside a 16-key group, the 64-key trip edge and the partition edge, with 0 .. 3
partitions."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import dev, to_dev
from test_gpu_gemv import SENT

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(GOLDEN, "kv_step")
GUARD = 2
HKV, CAP, D, EPS = 2, 768, 128, 1e-6
KD = HKV * D
N_VIS = (0, 1, 16, 17, 63, 64, 65, 255, 256, 257, 600)
B = len(N_VIS)
MAX_PAGES, N_PAGES = CAP // 256, 40
KINDS = ("contig", "paged", "paged_mx")
HQS = (2, 4, 8)
SENT32 = 0x7FC10000   # the sentinel as an fp32 NaN, for lse

_DATA, _PLANES = {}, {}


@pytest.fixture(scope="module")
def lib():
    import speech_distill_amd as sda
    return sda.load_lib()


def _stream():
    from speech_distill_amd.ops import _stream as s
    return s()


def _pow2_rows(rows, lo, hi, g):
    return 2.0 ** torch.randint(lo, hi + 1, (rows, 1), generator=g).float()


def _data(Hq):
    """The seeded inputs every case of one Hq shares, on the device, made once and never changed."""
    if Hq not in _DATA:
        g = torch.Generator().manual_seed(7001 + Hq)
        d = dict(
            qkv=(torch.randn(B, (Hq + 2 * HKV) * D, generator=g) * _pow2_rows(B, -3, 3, g)).bfloat16(),
            q=(torch.randn(B, Hq * D, generator=g) * _pow2_rows(B, -2, 1, g)).bfloat16(),
            qg=(1 + 0.25 * torch.randn(D, generator=g)).bfloat16(),
            kg=(1 + 0.25 * torch.randn(D, generator=g)).bfloat16(),
            cos=(2 * torch.rand(CAP, D, generator=g) - 1).bfloat16(),
            sin=(2 * torch.rand(CAP, D, generator=g) - 1).bfloat16(),
            table=torch.randperm(N_PAGES, generator=g)[:B * MAX_PAGES].reshape(B, MAX_PAGES).to(torch.int32))
        _DATA[Hq] = {k: to_dev(v) for k, v in d.items()}
    return _DATA[Hq]


def _pristine(kind):
    """(planes, rows): the seeded K and V rows [B * CAP, KD] every kind holds before a call, and the planes they go into --
    the rows themselves (contiguous), or a pool with a fixed fill that _planes places them in through the page table."""
    if kind not in _PLANES:
        g = torch.Generator().manual_seed(424243)
        rows = [(torch.randn(B * CAP, KD, generator=g) * _pow2_rows(B * CAP, -2, 0, g)).bfloat16() for _ in range(2)]
        if kind == "contig":
            planes = tuple(to_dev(r.reshape(B, CAP, KD)) for r in rows)
        elif kind == "paged":
            planes = tuple(to_dev((0.125 * torch.randn(N_PAGES, 256, KD, generator=g)).bfloat16()) for _ in range(2))
        else:
            planes = (torch.full((N_PAGES, 256, KD), 0x3C, dtype=torch.uint8, device=dev()),
                      torch.full((N_PAGES, 256, HKV * 4), 127, dtype=torch.uint8, device=dev()),
                      torch.full((N_PAGES, 256, KD), 0x3C, dtype=torch.uint8, device=dev()),
                      torch.full((N_PAGES, 256, HKV * 4), 127, dtype=torch.uint8, device=dev()))
        _PLANES[kind] = (planes, rows)
    return _PLANES[kind]


def _planes(lib, kind, Hq):
    """A fresh copy of the planes for one call, the seeded rows placed through THIS Hq's page table."""
    base, rows = _pristine(kind)
    planes = tuple(p.clone() for p in base)
    table = _data(Hq)["table"]
    if kind == "paged":
        idx = table.reshape(-1).long()
        for p, r in zip(planes, rows):
            p[idx] = to_dev(r.reshape(B * MAX_PAGES, 256, KD))
    elif kind == "paged_mx":
        # sd_kvcache_store_paged_mx takes K from a q|k row and V from a q|k|v row; one dummy query head in front
        qk = torch.zeros(B * CAP, (1 + HKV) * D, dtype=torch.bfloat16, device=dev())
        qkv = torch.zeros(B * CAP, (1 + 2 * HKV) * D, dtype=torch.bfloat16, device=dev())
        qk[:, D:] = to_dev(rows[0])
        qkv[:, (1 + HKV) * D:] = to_dev(rows[1])
        rc = lib.sd_kvcache_store_paged_mx(qk.data_ptr(), qkv.data_ptr(), *[p.data_ptr() for p in planes], table.data_ptr(),
                                           MAX_PAGES, N_PAGES, None, B, CAP, 1, HKV, _stream())
        assert rc == 0, rc
    return planes


def _out(cols, dtype):
    """A sentinel-filled buffer [GUARD + B + GUARD, cols] and the view of its B inner rows."""
    if dtype == torch.bfloat16:
        buf = torch.full((B + 2 * GUARD, cols), SENT, dtype=torch.int16, device=dev())
    else:
        buf = torch.full((B + 2 * GUARD, cols), SENT32, dtype=torch.int32, device=dev())
    return buf, buf.view(dtype)[GUARD:GUARD + B]


def _bits(buf, name):
    got = buf.cpu().numpy()
    sent = np.int16(SENT) if got.dtype == np.int16 else np.int32(SENT32)
    assert not (got[GUARD:GUARD + B] == sent).any(), f"{name}: elements were left unwritten"
    return got


def _digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=dev())


def _ws(lib, Hq):
    nb = lib.sd_cache_step_workspace_bytes(B, Hq, HKV, CAP)
    assert nb == lib.sd_attn_decode_workspace_bytes(B, Hq, CAP)
    return torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev())   # NaN records: a stale one that is read shows


# ------------------------------------------------------------------------------------------------------ the entries
# Each returns ({name: whole array}, {name: digest}) of one (kind, Hq).
def _run_attn(lib, kind, Hq):
    d, planes, ws = _data(Hq), _planes(lib, kind, Hq), _ws(lib, Hq)
    lens = _i32([n - 1 for n in N_VIS])
    arrays = {}
    for max_len in (CAP, 300):   # 300 clamps the 600-key row
        (ob, o), (lb, lse) = _out(Hq * D, torch.bfloat16), _out(Hq, torch.float32)
        tail = (o.data_ptr(), lse.data_ptr(), lens.data_ptr(), 1, ws.data_ptr(), ws.numel(), B)
        shape = (max_len, Hq, HKV, D, D ** -0.5, _stream())
        pl = [p.data_ptr() for p in planes]
        if kind == "contig":
            rc = lib.sd_attn_decode(d["q"].data_ptr(), *pl, *tail, CAP, *shape)
        elif kind == "paged":
            rc = lib.sd_attn_decode_paged(d["q"].data_ptr(), *pl, d["table"].data_ptr(), MAX_PAGES, N_PAGES, *tail, *shape)
        else:
            rc = lib.sd_attn_decode_paged_mx(d["q"].data_ptr(), *pl, d["table"].data_ptr(), MAX_PAGES, N_PAGES, *tail, *shape)
        assert rc == 0, rc
        torch.cuda.synchronize()
        arrays[f"ml{max_len}_o"], arrays[f"ml{max_len}_lse"] = _bits(ob, "o"), _bits(lb, "lse")
    return arrays, {}


def _run_append(lib, kind, Hq):
    d = _data(Hq)
    arrays, digests = {}, {}
    for case, pos_l in (("pos", [n - 1 for n in N_VIS]), ("nostore", [(-1, CAP)[b & 1] for b in range(B)])):
        planes, pos = _planes(lib, kind, Hq), _i32(pos_l)
        before = [_digest(p) for p in planes]
        qb, q = _out(Hq * D, torch.bfloat16)
        head = [d[k].data_ptr() for k in ("qkv", "qg", "kg", "cos", "sin")] + [pos.data_ptr(), q.data_ptr()]
        pl = [p.data_ptr() for p in planes]
        if kind == "contig":
            rc = lib.sd_qknorm_rope_append(*head, *pl, B, CAP, Hq, HKV, EPS, _stream())
        elif kind == "paged":
            rc = lib.sd_qknorm_rope_append_paged(*head, *pl, d["table"].data_ptr(), MAX_PAGES, N_PAGES, B, Hq, HKV, EPS,
                                                 _stream())
        else:
            rc = lib.sd_qknorm_rope_append_paged_mx(*head, *pl, d["table"].data_ptr(), MAX_PAGES, N_PAGES, B, Hq, HKV, EPS,
                                                    _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        arrays[f"{case}_q"] = _bits(qb, "q")
        after = [_digest(p) for p in planes]
        # the K and V planes (not the scale planes, whose new bytes may equal the old) move exactly when something is stored
        moved = [a != b_ for a, b_ in zip(after, before)]
        assert (moved[0] and moved[-2 if kind == "paged_mx" else 1]) if case == "pos" else not any(moved), (case, moved)
        digests.update({f"{case}_plane{i}": h for i, h in enumerate(after)})
    return arrays, digests


def _run_cache_step(lib, kind, Hq):
    from speech_distill_amd._lib import KvPlanes
    d, planes, ws = _data(Hq), _planes(lib, kind, Hq), _ws(lib, Hq)
    pos = _i32([n - 1 for n in N_VIS])
    tickets = torch.zeros(B, HKV, dtype=torch.int32, device=dev())
    (ob, o), (lb, lse) = _out(Hq * D, torch.bfloat16), _out(Hq, torch.float32)
    pl = [p.data_ptr() for p in planes]
    if kind == "contig":
        kv = KvPlanes(0, pl[0], pl[1], None, None, CAP, None, 0, 0)
    elif kind == "paged":
        kv = KvPlanes(1, pl[0], pl[1], None, None, 0, d["table"].data_ptr(), MAX_PAGES, N_PAGES)
    else:
        kv = KvPlanes(2, pl[0], pl[2], pl[1], pl[3], 0, d["table"].data_ptr(), MAX_PAGES, N_PAGES)
    rc = lib.sd_cache_step(*[d[k].data_ptr() for k in ("qkv", "qg", "kg", "cos", "sin")], pos.data_ptr(), C.byref(kv),
                           o.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel(), tickets.data_ptr(), B, CAP, Hq, HKV, D,
                           EPS, D ** -0.5, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(tickets.abs().max()) == 0, tickets
    return {"o": _bits(ob, "o"), "lse": _bits(lb, "lse")}, {f"plane{i}": _digest(p) for i, p in enumerate(planes)}


ENTRIES = {"attn_decode": _run_attn, "qknorm_rope_append": _run_append, "cache_step": _run_cache_step}


def _prefix(kind, Hq):
    return f"{kind}_Hq{Hq}_"


# ------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("Hq", HQS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_outputs_equal_the_recorded_ones(lib, entry, kind, Hq):
    want = np.load(os.path.join(GOLDEN_DIR, entry + ".npz"), allow_pickle=False)
    with open(os.path.join(GOLDEN_DIR, "digests.json")) as f:
        want_dig = json.load(f)[entry]
    arrays, digests = ENTRIES[entry](lib, kind, Hq)
    pre = _prefix(kind, Hq)
    assert sorted(k for k in want.files if k.startswith(pre)) == sorted(pre + k for k in arrays)
    assert sorted(k for k in want_dig if k.startswith(pre)) == sorted(pre + k for k in digests)
    bad = []
    for k, got in arrays.items():
        w = want[pre + k]
        if got.shape != w.shape or got.dtype != w.dtype or not np.array_equal(got, w):
            bad.append((k, int((got != w).sum()) if got.shape == w.shape else "shape"))
    bad += [(k, "digest") for k, h in digests.items() if want_dig[pre + k] != h]
    assert not bad, f"{entry} {kind} Hq={Hq}: buffers that differ from the recorded ones (name, elements): {bad}"


def _record(out_dir):
    import speech_distill_amd as sda
    lib = sda.load_lib()
    os.makedirs(out_dir, exist_ok=True)
    all_dig = {}
    for entry, run in sorted(ENTRIES.items()):
        arrays, all_dig[entry] = {}, {}
        for kind in KINDS:
            for Hq in HQS:
                a, dg = run(lib, kind, Hq)
                arrays.update({_prefix(kind, Hq) + k: v for k, v in a.items()})
                all_dig[entry].update({_prefix(kind, Hq) + k: v for k, v in dg.items()})
        path = os.path.join(out_dir, entry + ".npz")
        np.savez_compressed(path, **arrays)
        print("recorded", entry, len(arrays), "arrays", len(all_dig[entry]), "digests", os.path.getsize(path), "bytes")
    with open(os.path.join(out_dir, "digests.json"), "w") as f:
        json.dump(all_dig, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        _record(sys.argv[2])
    else:
        sys.exit("usage: python tests/test_gpu_kv_step_golden.py --record DIR")
