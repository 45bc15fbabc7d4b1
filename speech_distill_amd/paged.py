"""Paged KV cache: a pool of 256-position pages that sessions share, and the page tables that map a row's positions to them.

The reference's production engine runs vLLM with ``enable_prefix_caching=True`` (soulxpodcast/engine/llm_engine.py:91): a
block-paged cache whose blocks are shared between requests with a common prefix.  Here the page is SD_KV_PAGE = 256
positions -- one sd_attn_decode partition and four sd_attn_extend tiles -- so the paged kernels walk the same keys in the
same order as the contiguous ones and produce the same bits (include/sd_hip.h).

Three layers, the first two pure host code (no device, no library: tests/test_paged_cpu.py runs them as they are):
  ``PageAllocator``  free list + reference count per page;
  ``PageTable``      one session's rows -> pages (the host mirror of the device table) with the admission, trim and fork
                     rules; every operation that can fail checks first and changes nothing when it raises;
  ``PagePool``       the device buffer [L][2][n_pages][256][Hkv*128] of one model plus a ``PageAllocator``; with
                     ``kv_dtype="mxfp8"`` the 8-bit pool of include/sd_hip.h (e4m3 data planes + E8M0 scale planes).
"""
from __future__ import annotations

import ctypes as C

PAGE = 256   # include/sd_hip.h SD_KV_PAGE
KV_DTYPES = ("bf16", "mxfp8")


def check_kv_dtype(kv_dtype):
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")


def pages_for(n):
    """Pages that hold positions [0, n)."""
    return (max(int(n), 0) + PAGE - 1) // PAGE


def fork_split(cached):
    """(shared, copied) page counts of a fork at ``cached`` positions: the pages wholly below ``cached`` are shared, the
    page that holds position ``cached`` is copied unless that position starts a page."""
    cached = max(int(cached), 0)
    return cached // PAGE, 1 if cached % PAGE else 0


class PageAllocator:
    """Host bookkeeping of a pool of ``n_pages`` pages: the free list (handed out in ``order``, a permutation of the page
    numbers; a released page is the next one handed out) and a reference count per page."""

    def __init__(self, n_pages, order=None):
        n_pages = int(n_pages)
        if n_pages < 1:
            raise ValueError(f"a page pool needs at least one page, got {n_pages}")
        order = list(range(n_pages)) if order is None else [int(p) for p in order]
        if sorted(order) != list(range(n_pages)):
            raise ValueError(f"order must be a permutation of range({n_pages})")
        self.n_pages = n_pages
        self._free = order[::-1]          # pop() hands out order[0] first
        self.refs = [0] * n_pages

    @property
    def free_pages(self):
        return len(self._free)

    @property
    def pages_in_use(self):
        return self.n_pages - len(self._free)

    def take(self, n):
        """``n`` free pages, each with reference count 1.  ValueError (and nothing taken) when fewer are free."""
        if n > len(self._free):
            raise ValueError(f"the page pool is exhausted: {n} pages wanted, {len(self._free)} of {self.n_pages} free")
        out = [self._free.pop() for _ in range(n)]
        for p in out:
            self.refs[p] = 1
        return out

    def share(self, pages):
        """One more holder for each of ``pages`` (all in use)."""
        for p in pages:
            if self.refs[p] < 1:
                raise ValueError(f"page {p} is not in use")
            self.refs[p] += 1

    def release(self, pages):
        """One holder fewer for each of ``pages``; a page returns to the free list when nobody holds it."""
        for p in pages:
            if self.refs[p] < 1:
                raise ValueError(f"page {p} is not in use")
            self.refs[p] -= 1
            if self.refs[p] == 0:
                self._free.append(p)


class PageTable:
    """The pages of one session's ``B`` rows: ``rows[b][i]`` is the physical page of positions 256 i .. 256 i + 255 of row
    b.  ``dirty`` collects the rows whose entries changed since the owner last uploaded them to the device table."""

    def __init__(self, alloc, B, max_pages):
        self.alloc, self.B, self.max_pages = alloc, int(B), int(max_pages)
        self.rows = [[] for _ in range(self.B)]
        self.dirty = set()

    def _check_reach(self, want):
        if len(want) != self.B:
            raise ValueError(f"{len(want)} lengths for a table of {self.B} rows")
        need = [pages_for(n) for n in want]
        if max(need) > self.max_pages:
            raise ValueError(f"{max(want)} positions exceed the table's {self.max_pages} pages of {PAGE}")
        return need

    def admit(self, keep, want):
        """The allocation rule of a turn.  First every row gives back the whole pages past ``keep[b]`` positions (left over
        from an earlier worst case), then every row gets pages for ``want[b]`` positions.  Checked as a whole before
        anything changes: ValueError when the pool cannot cover it, and then nothing was released or taken."""
        need = self._check_reach(want)
        kept = [min(len(r), max(pages_for(k), 0)) for r, k in zip(self.rows, keep)]
        # a page given back is free again only when this row was its last holder
        freed = sum(1 for r, k in zip(self.rows, kept) for p in r[k:] if self.alloc.refs[p] == 1)
        more = sum(max(n - k, 0) for n, k in zip(need, kept))
        if more > self.alloc.free_pages + freed:
            raise ValueError(f"the page pool cannot cover this turn: {more} more pages wanted, "
                             f"{self.alloc.free_pages + freed} of {self.alloc.n_pages} free")
        self.trim(keep)
        for b, n in enumerate(need):
            if n > len(self.rows[b]):
                self.rows[b] += self.alloc.take(n - len(self.rows[b]))
                self.dirty.add(b)

    def reserve(self, lengths):
        """Every row owns pages for at least ``lengths[b]`` positions (nothing is given back).  All or nothing."""
        self.admit([len(r) * PAGE for r in self.rows], [max(n, len(r) * PAGE) for n, r in zip(lengths, self.rows)])

    def trim(self, lengths):
        """Give back every row's whole pages past ``lengths[b]`` positions."""
        for b, n in enumerate(lengths):
            k = pages_for(n)
            if k < len(self.rows[b]):
                self.alloc.release(self.rows[b][k:])
                del self.rows[b][k:]
                self.dirty.add(b)

    def release(self, rows=None):
        """Give back every page of ``rows`` (all rows when None)."""
        for b in (range(self.B) if rows is None else rows):
            if self.rows[b]:
                self.alloc.release(self.rows[b])
                self.rows[b] = []
                self.dirty.add(b)

    def fork(self, src_rows, cached):
        """-> (table, copies): a new table on the same allocator whose row i continues row ``src_rows[i]`` at
        ``cached[src_rows[i]]`` cached positions, and the (source page, new page) pairs whose contents the caller must
        copy.  Pages wholly below the cached positions are shared (one more holder each); the page that holds position
        ``cached`` is a fresh page per fork when that position does not start a page.  All or nothing."""
        plan = []
        for s in src_rows:
            shared, copied = fork_split(cached[s])
            if shared + copied > len(self.rows[s]):
                raise ValueError(f"row {s} holds {len(self.rows[s])} pages, fewer than its {cached[s]} cached positions")
            plan.append((s, shared, copied))
        fresh = self.alloc.take(sum(c for _, _, c in plan))   # raises before anything changed
        out = PageTable(self.alloc, len(plan), self.max_pages)
        copies = []
        for i, (s, shared, copied) in enumerate(plan):
            self.alloc.share(self.rows[s][:shared])
            out.rows[i] = list(self.rows[s][:shared])
            if copied:
                dst = fresh.pop()
                copies.append((self.rows[s][shared], dst))
                out.rows[i].append(dst)
            out.dirty.add(i)
        return out, copies

    def entries(self, b, fill=-1):
        """Row b of the table as ``max_pages`` ints; entries the row does not own are ``fill``."""
        return self.rows[b] + [fill] * (self.max_pages - len(self.rows[b]))


class PagePool:
    """The device buffer [L][2][n_pages][256][Hkv*128] (bf16) of one model's paged sessions, with the host free list and
    reference counts (``PageAllocator``).  ``order``: the order in which free pages are handed out.

    ``kv_dtype="mxfp8"``: the 8-bit pool (include/sd_hip.h "8-bit (MXFP8) pages") -- per layer a K data plane uint8
    [n_pages, 256, Hkv*128] (e4m3 bytes), a K scale plane uint8 [n_pages, 256, Hkv*4] (E8M0, one per 32 elements), then
    the same two for V: 132 bytes per position and kv head where bf16 takes 256."""

    def __init__(self, model, n_pages, order=None, kv_dtype="bf16"):
        import torch
        from ._lib import check, load_lib
        check_kv_dtype(kv_dtype)      # before anything is allocated
        self.alloc = PageAllocator(n_pages, order)
        self.model, self.n_pages, self.kv_dtype = model, int(n_pages), kv_dtype
        size = load_lib().sd_kvpool_mx_bytes if kv_dtype == "mxfp8" else load_lib().sd_kvpool_bytes
        nb = size(C.byref(model._cdims), self.n_pages)
        check(min(nb, 0), "sd_kvpool_bytes")
        self.buffer = torch.empty(nb, dtype=torch.uint8, device=model.flat.device)
        self.bytes_per_page = nb // self.n_pages

    @property
    def free_pages(self):
        return self.alloc.free_pages

    @property
    def pages_in_use(self):
        return self.alloc.pages_in_use

    def planes(self, layer):
        """(K, V) views [n_pages, 256, Hkv*128] of one layer's pool planes; of an mxfp8 pool the four uint8 views (K data
        [n_pages, 256, Hkv*128], K scale [n_pages, 256, Hkv*4], V data, V scale)."""
        import torch
        kd = self.model.dims.kv_dim
        if self.kv_dtype == "mxfp8":
            nd, ns = self.n_pages * PAGE * kd, self.n_pages * PAGE * (kd // 32)
            out, at = [], 2 * layer * (nd + ns)
            for n, w in ((nd, kd), (ns, kd // 32)) * 2:
                out.append(self.buffer[at:at + n].view(self.n_pages, PAGE, w))
                at += n
            return tuple(out)
        n = self.n_pages * PAGE * kd
        flat = self.buffer.view(torch.bfloat16)
        return (flat[(2 * layer) * n:(2 * layer + 1) * n].view(self.n_pages, PAGE, kd),
                flat[(2 * layer + 1) * n:(2 * layer + 2) * n].view(self.n_pages, PAGE, kd))

    def copy_pages(self, pairs):
        """Copy page src -> dst in every plane of every layer, for each (src, dst) of ``pairs``, on the current stream."""
        import torch
        if not pairs:
            return
        dev = self.buffer.device
        src = torch.tensor([s for s, _ in pairs], dtype=torch.int64, device=dev)
        dst = torch.tensor([d for _, d in pairs], dtype=torch.int64, device=dev)
        if self.kv_dtype == "mxfp8":    # data and scale planes have different page sizes: plane by plane
            for layer in range(self.model.dims.num_hidden_layers):
                for plane in self.planes(layer):
                    plane[dst] = plane[src]
            return
        planes = self.buffer.view(torch.bfloat16).view(-1, self.n_pages, PAGE * self.model.dims.kv_dim)
        planes[:, dst] = planes[:, src]
