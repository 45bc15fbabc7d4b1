"""Continuous batching over a page pool: a request engine with per-request sampling parameters.

The reference's production engine is vLLM (soulxpodcast/engine/llm_engine.py:91): it admits a waiting request as soon as a
running one finishes and takes one ``SamplingParams`` per request (llm_engine.py:97-109).  ``GenerationSession`` steps a
fixed batch until its last row stops; here a row that finishes is refilled at once, so a decode step is spent on live rows
only.  With ``decode_kernels="skinny"`` the contract is exact: a request served by the engine yields, bit for bit, the
tokens a one-row session yields for it alone -- its prefill is the B = 1 prefill of exactly its prompt, the skinny decode
step makes a row's logits independent of the batch around it, and the sampler (sd_sample_step_rows) works row by row
with the row's own parameters, budget and uniform stream.  "skinny" is exact up to ``max_batch = 16`` (above it its step
falls back to the tile GEMMs); ``decode_kernels="wide"`` (bf16 weights) carries the same contract up to ``max_batch = 64``,
against a one-row "wide" session.

Two layers, in the style of paged.py; the first is pure host code (no device, no library: tests/test_engine_cpu.py runs it
as it is):
  ``Scheduler``         strict FIFO admission over a ``PageTable``; a request reserves pages for its worst case (prompt +
                        budget) when it is admitted, so nothing is ever pre-empted; every operation checks first and
                        changes nothing when it raises.  ``EngineLoop`` is one iteration over hooks, ``Replay`` the loop
                        with lengths given in advance (what ``stats`` must come to for realised lengths).
  ``GenerationEngine``  the loop on the device: one ``Decoder`` over the pool plus the state of sd_sample_step_rows.

One request per prefill pass is what keeps the bit contract; ``admission="batch"`` (opt-in) prefills an iteration's
admissions in one pass and gives the contract up (``GenerationEngine``).  An engine is reusable: ``forget`` drops finished
requests, ``reset_stats`` restarts the counters, and its decoder reads the model's live weights at every call.

Not built: pre-emption and swapping, prefix matching between requests, per-request parameters inside sessions, captured
graphs.
"""
from __future__ import annotations

from collections import deque

from .paged import PAGE, PageAllocator, PageTable, pages_for

ADMISSION = ("single", "batch")


class Request:
    """One submitted request as the scheduler sees it: prompt length ``T``, budget ``max_new``, and once admitted its
    ``row`` and the sampler steps it has taken (``steps``: the host's count, an upper bound of its new tokens)."""

    def __init__(self, rid, T, max_new):
        self.id, self.T, self.max_new = rid, int(T), int(max_new)
        self.row, self.steps, self.done = None, 0, False


class Scheduler:
    """Rows and pages of a continuously batched decoder.  ``table``: the decoder's ``PageTable`` (B rows); ``capacity``:
    the most positions a request may hold.  One page of the pool is the engine's parking page, the page every free row
    maps at position 0, taken here and given back by ``close``."""

    def __init__(self, table, capacity, sync_every=16):
        if int(sync_every) < 1:
            raise ValueError(f"sync_every must be >= 1, got {sync_every}")
        self.table, self.alloc, self.B = table, table.alloc, table.B
        self.capacity, self.sync_every = int(capacity), int(sync_every)
        self.park = self.alloc.take(1)[0]     # ValueError when the pool has no free page
        self.free_rows = list(range(self.B))
        self.waiting, self.live = deque(), {}
        self.iteration, self._next_id = 0, 0

    def check(self, T, max_new):
        """ValueError for a request that could never be admitted; nothing changes."""
        T, max_new = int(T), int(max_new)
        if T < 1 or max_new < 1:
            raise ValueError(f"a request needs at least one prompt token and max_new_tokens >= 1, got {T}, {max_new}")
        need = pages_for(T + max_new)
        if T + max_new > self.capacity:
            raise ValueError(f"prompt length {T} + max_new_tokens {max_new} exceeds the KV-cache capacity {self.capacity}")
        if need > self.table.max_pages:
            raise ValueError(f"{T + max_new} positions exceed the table's {self.table.max_pages} pages of {PAGE}")
        if need > self.alloc.n_pages - 1:
            raise ValueError(f"{need} pages can never be free in a pool of {self.alloc.n_pages} pages (one is the "
                             "engine's parking page)")

    def submit(self, T, max_new):
        self.check(T, max_new)
        req = Request(self._next_id, T, max_new)
        self._next_id += 1
        self.waiting.append(req)
        return req

    def admit(self):
        """Admit from the head of the queue while a row is free and the pool covers the head's worst case; the head is
        never overtaken.  -> the admitted requests, each with its row and its pages (the table rows are dirty)."""
        out = []
        while self.waiting and self.free_rows:
            req = self.waiting[0]
            if pages_for(req.T + req.max_new) > self.alloc.free_pages:
                break                              # the head waits; nothing has changed
            row = min(self.free_rows)
            want = [0] * self.B
            want[row] = req.T + req.max_new
            self.table.reserve(want)               # all or nothing
            self.free_rows.remove(row)
            self.waiting.popleft()
            req.row, req.steps = row, 0
            self.live[row] = req
            out.append(req)
        return out

    def sampled(self):
        """One sampler step has run over the live rows.  -> the rows whose budget is now spent (known without a read)."""
        self.iteration += 1
        done = []
        for row in sorted(self.live):
            req = self.live[row]
            req.steps += 1
            if req.steps >= req.max_new:
                done.append(row)
        return done

    def sync_due(self):
        return self.iteration % self.sync_every == 0

    def finish(self, row):
        """The row's request is over: its pages go back to the pool and the row is free."""
        if row not in self.live:
            raise ValueError(f"row {row} serves no request")
        req = self.live.pop(row)
        self.table.release([row])
        self.free_rows.append(row)
        req.done = True
        return req

    def max_len(self):
        """Host upper bound of every live row's length."""
        return max([r.T + r.steps for r in self.live.values()], default=1)

    def close(self):
        for row in sorted(self.live):
            self.finish(row)
        self.waiting.clear()
        if self.park is not None:
            self.alloc.release([self.park])
            self.park = None


class EngineLoop:
    """One scheduler iteration over five hooks: ``_admit(req)`` (prefill + the row's state), ``_sample()``,
    ``_read_finished()`` (the host read, -> one flag per row), ``_free(req)`` and ``_decode(max_len)``."""

    def __init__(self, sched):
        self.sched = sched
        self.requests = {}
        self.reset_stats()

    def reset_stats(self):
        """Start ``stats`` again, as a new loop over this scheduler would."""
        self.stats = {"decode_steps": 0, "prefills": 0, "peak_pages": self.sched.alloc.pages_in_use, "iterations": 0}

    def forget(self, rids=None):
        """Drop finished requests (``rids``; None: every finished one) and their results, so that a loop that serves
        window after window does not grow.  ValueError, with nothing dropped, for an unknown id or a request that is
        still waiting or running."""
        rids = [r for r, q in self.requests.items() if q.done] if rids is None else list(rids)
        for r in rids:
            if r not in self.requests:
                raise ValueError(f"no request {r}")
            if not self.requests[r].done:
                raise ValueError(f"request {r} has not finished")
        for r in rids:
            self.requests.pop(r, None)

    def _admit_all(self, reqs):
        """The admissions of one iteration, in FIFO order: one ``_admit`` each (a loop may override it to batch them)."""
        for req in reqs:
            self._admit(req)

    def step(self):
        """Admissions, one sampler step, the frees it brings, one decode step.  -> the ids that finished."""
        s = self.sched
        reqs = s.admit()
        if reqs:
            self._admit_all(reqs)
            self.stats["prefills"] += len(reqs)
        self.stats["peak_pages"] = max(self.stats["peak_pages"], s.alloc.pages_in_use)
        if not s.live:
            if s.waiting:    # only when somebody else holds the pool's pages: waiting would never end
                raise ValueError("the page pool cannot cover the request at the head of the queue and no row is running")
            return []
        self._sample()
        self.stats["iterations"] += 1
        done = s.sampled()
        if s.sync_due():
            flags = self._read_finished()
            done += [row for row in sorted(s.live) if flags[row] and row not in done]
        out = []
        for row in done:
            req = s.live[row]
            self._free(req)
            s.finish(row)
            out.append(req.id)
        if s.live:
            self._decode(s.max_len())
            self.stats["decode_steps"] += 1
        return out

    def run(self):
        """Serve everything submitted so far.  Bounded: every request finishes within its budget."""
        out = []
        while self.sched.waiting or self.sched.live:
            out += self.step()
        return out


class Replay(EngineLoop):
    """The loop on the host alone, for requests whose realised lengths are known: ``submit(T, max_new, realised)`` with
    ``realised`` new tokens (EOS included; == max_new without one).  ``stats`` is what an engine of the same shape reports
    for those lengths."""

    def __init__(self, max_batch, n_pages, max_pages, capacity, sync_every=16):
        super().__init__(Scheduler(PageTable(PageAllocator(n_pages), max_batch, max_pages), capacity, sync_every))
        self.finished_order = []

    def submit(self, T, max_new, realised):
        req = self.sched.submit(T, max_new)
        req.realised = min(int(realised), int(max_new))
        return req.id

    def _admit(self, req):
        pass

    def _sample(self):
        pass

    def _read_finished(self):
        flags = [True] * self.sched.B
        for row, req in self.sched.live.items():
            flags[row] = req.steps >= req.realised
        return flags

    def _free(self, req):
        self.finished_order.append(req.id)

    def _decode(self, max_len):
        pass


def static_steps(budgets, batch):
    """Sampler steps of the fixed-batch schedule: batches of ``batch`` in order, each stepped to its longest member."""
    return sum(max(budgets[i:i + batch]) for i in range(0, len(budgets), batch))


class GenerationEngine(EngineLoop):
    """``model.generation_engine(pool, ...)``.  Owns one paged ``Decoder`` of ``max_batch`` rows and the device state of
    sd_sample_step_rows: ``seq`` int64 [B,cap], ``len`` / ``prompt_len`` / ``max_new`` int32 [B], ``finished`` uint8 [B],
    ``params`` [B] and the uniforms ``U`` fp32 [B,u_stride,2] (grown to the largest budget seen).

    ``submit`` checks everything on the host and queues the request.  An iteration (``step``) admits from the head of the
    queue -- per request a B = 1 prefill of exactly its prompt through the row's pages (``Decoder.prefill_rows``), the
    row's state, and ``U[row]`` filled with the values a one-row session draws for the seed -- then runs ONE
    sd_sample_step_rows and ONE decode step over all rows.  The host reads ``finished`` once every ``sync_every``
    iterations and at no other time; a row whose budget is spent is freed without a read.  Free rows are finished rows at
    position 0 that map the parking page, so every table entry a kernel reads lies in the pool.  ``result(id)`` returns the
    new tokens up to and including the first EOS (one host read for the lengths of all finished requests not read yet).

    ``admission``: "single" (default) is the above.  "batch" admits the requests the scheduler admits in one iteration --
    same FIFO order, same page reservations -- through ONE ``Decoder.prefill_rows`` call over their right-padded prompts.
    It gives up the one-row bit contract: the prefill's tile GEMMs then run at another M, whose summation order is not
    the B = 1 prefill's, so a request's first logits (and what follows from them) may differ in the last bf16 bit from a
    one-row session's.  An iteration that admits one request is the "single" admission.

    The engine serves any number of ``run()``s: after each every page but the parking page is back in the pool,
    ``forget`` drops finished requests and ``reset_stats`` starts the counters again.  Every prefill and decode step reads
    the model's LIVE bf16 weights (``Decoder._params()`` is fetched per call and points into ``model.flat``), so weights
    that an optimizer changes in place between two runs are the ones the second run decodes with.  What a ``Decoder``
    keeps from its construction -- RoPE tables, the pool and table pointers, the step's scratch -- does not depend on
    the weights; the one weight-derived cache is the MXFP8 copy (``model._mx_params()``), which is built once and which
    ``_check_weight_dtype`` refuses for a model with trainable parameters."""

    def __init__(self, model, pool, max_batch=8, decode_kernels="skinny", weight_dtype="bf16", sync_every=16, capacity=None,
                 decode_attention="split", gemv_rows=16, admission="single"):
        import torch
        if admission not in ADMISSION:
            raise ValueError(f"admission must be one of {ADMISSION}, got {admission!r}")
        self.admission = admission
        from ._lib import load_lib
        from .generation import Decoder, _check_decode_attention, _check_decode_kernels, _check_gemv_rows, cache_capacity
        from .ops import sample_params, sample_params_rows
        _check_decode_attention(decode_attention)
        _check_decode_kernels(decode_kernels, weight_dtype)
        _check_gemv_rows(gemv_rows, decode_kernels, weight_dtype, decode_attention)
        if pool is None:
            raise ValueError("the engine serves its rows from a page pool: model.kv_page_pool(n_pages)")
        if int(max_batch) < 1 or int(sync_every) < 1:
            raise ValueError(f"max_batch and sync_every must be >= 1, got {max_batch}, {sync_every}")
        cap = min(int(capacity) if capacity is not None else cache_capacity(model), (pool.n_pages - 1) * PAGE)
        if cap < 1:
            raise ValueError("the engine needs a pool of at least two pages (one is its parking page)")
        self.model, self.pool, self.B = model, pool, int(max_batch)
        self.decode_kernels, self.weight_dtype, self.sync_every = decode_kernels, weight_dtype, int(sync_every)
        self.decode_attention = decode_attention   # "fused": each layer's cache step is one launch, same tokens (Decoder)
        self.gemv_rows = gemv_rows   # 64: the MXFP8 "skinny" step on the 64-row kernels (Decoder)
        self.decoder = dec = Decoder(model, self.B, cap, decode_kernels, pool=pool, weight_dtype=weight_dtype,
                                     decode_attention=decode_attention, gemv_rows=gemv_rows)
        super().__init__(Scheduler(dec.pages, min(dec.cap, cache_capacity(model)), sync_every))
        dev, B, V = model.flat.device, self.B, model.dims.vocab_size
        self.seq = torch.zeros(B, dec.cap, dtype=torch.int64, device=dev)
        self._ints = torch.zeros(3, B, dtype=torch.int32, device=dev)
        self.len, self.prompt_len, self.max_new = self._ints[0], self._ints[1], self._ints[2]
        self.finished = torch.ones(B, dtype=torch.uint8, device=dev)
        self.params = sample_params_rows([sample_params(do_sample=False)] * B, dev)   # free rows: greedy, pad 0
        self.U = torch.zeros(B, 1, 2, dtype=torch.float32, device=dev)
        self.nxt = torch.zeros(B, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(B, dtype=torch.int32, device=dev)
        self.ws = torch.zeros(load_lib().sd_sample_workspace_bytes(B, V), dtype=torch.uint8, device=dev)
        dec.logits.zero_()
        dec.pages.dirty.update(range(B))
        self._upload()
        self._set_env()

    # ---- host side
    def submit(self, input_ids, max_new_tokens=20, seed=None, min_new_tokens=0, do_sample=True, temperature=1.0, top_k=0,
               top_p=1.0, repetition_penalty=1.0, eos_token_id=None, pad_token_id=None, use_ras=False, win_size=25,
               tau_r=0.2):
        """Queue one request: ``input_ids`` int64 [T] on the GPU, its budget, its seed and the sampling keywords of
        ``generate``.  -> its id.  ValueError, with nothing changed, for bad sampling arguments (``generate``'s rules) and
        for a request that can never fit the table, the pool or the cache capacity."""
        import torch
        from .generation import _check_args
        from .ops import _need, sample_params
        if input_ids.dim() != 1:
            raise ValueError(f"input_ids must be one prompt [T], got {tuple(input_ids.shape)}")
        ids = _need(input_ids.to(torch.int64), torch.int64, "input_ids")
        T, V = ids.numel(), self.model.dims.vocab_size
        _check_args(self.model, 1, T, max_new_tokens, min_new_tokens, do_sample, temperature, top_k, top_p,
                    repetition_penalty, use_ras, win_size, tau_r, self.sync_every, self.decode_kernels,
                    weight_dtype=self.weight_dtype)
        pad = pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)
        if not 0 <= pad < V or (eos_token_id is not None and not 0 <= eos_token_id < V):
            raise ValueError(f"pad / eos token ids must lie in [0, {V})")
        if self.sched.park is None:
            raise ValueError("the engine is closed")
        req = self.sched.submit(T, max_new_tokens)     # raises before anything changed
        req.ids, req.seed = ids.reshape(1, T).clone(), seed
        req.sp = sample_params(do_sample, temperature, top_k, top_p, repetition_penalty, min_new_tokens, eos_token_id, pad,
                               use_ras, win_size, tau_r)
        self.requests[req.id] = req
        return req.id

    def result(self, rid):
        """int64 [n] (device): the request's new tokens up to and including its first EOS, or all ``max_new_tokens``."""
        import torch
        req = self.requests[rid]
        if not req.done:
            raise ValueError(f"request {rid} has not finished")
        if getattr(req, "n_host", None) is None:   # one read for every finished request whose length the host lacks
            unread = [q for q in self.requests.values() if q.done and getattr(q, "n_host", None) is None]
            for q, n in zip(unread, torch.cat([q.n_dev for q in unread]).tolist()):
                q.n_host = n
        return req.tokens[:max(req.n_host - req.T, 0)]

    def close(self):
        """Drop every request and give every page, the parking page included, back to the pool."""
        self.sched.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _set_env(self):
        from .ops import sample_env
        self.env = sample_env([r.sp for r in self.sched.live.values()])

    def _upload(self):
        """``Decoder.upload`` with the parking page at position 0 of every row that owns nothing."""
        import torch
        pages = self.decoder.pages
        rows = sorted(pages.dirty)
        if rows:
            host = [pages.entries(b) for b in rows]
            for e, b in zip(host, rows):
                if not pages.rows[b]:
                    e[0] = self.sched.park
            dev = self.decoder.table.device
            self.decoder.table[torch.tensor(rows, dtype=torch.int64, device=dev)] = \
                torch.tensor(host, dtype=torch.int32).to(dev)
            pages.dirty.clear()

    # ---- the loop's hooks
    def _admit(self, req):
        self._upload()
        self._seat(req, self.decoder.prefill_rows([req.row], req.ids)[0])

    def _admit_all(self, reqs):
        """``admission="batch"``: one prefill pass for everything this iteration admits (right-padded to the longest
        prompt; the pad slots are never cached), then each row's state as ``_admit`` sets it."""
        import torch
        if self.admission != "batch" or len(reqs) < 2:
            return super()._admit_all(reqs)
        dev, width = self.seq.device, max(r.T for r in reqs)
        ids = torch.zeros(len(reqs), width, dtype=torch.int64, device=dev)
        for i, req in enumerate(reqs):
            ids[i, :req.T] = req.ids[0]
        self._upload()
        logits = self.decoder.prefill_rows([r.row for r in reqs], ids,
                                           torch.tensor([r.T for r in reqs], dtype=torch.int32).to(dev))
        for i, req in enumerate(reqs):
            self._seat(req, logits[i])

    def _seat(self, req, logits):
        """The state of an admitted request's row behind its prefill (``logits`` bf16 [V]: its last prompt token's)."""
        import torch
        from .ops import sample_params_rows
        dev, r, T, n = self.seq.device, req.row, req.T, req.max_new
        self.decoder.logits[r] = logits
        self.seq[r, :T] = req.ids[0]
        self._ints[:, r] = torch.tensor([T, T, n], dtype=torch.int32).to(dev)
        self.finished[r] = 0
        self.params[r] = sample_params_rows([req.sp], dev)[0]
        gen = None
        if req.seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(req.seed))
        u = torch.rand(n, 1, 2, generator=gen, device=dev, dtype=torch.float32)   # what a one-row session draws
        if n > self.U.shape[1]:
            grown = torch.zeros(self.B, n, 2, dtype=torch.float32, device=dev)
            grown[:, :self.U.shape[1]] = self.U
            self.U = grown
        self.U[r, :n] = u[:, 0]
        self._set_env()

    def _sample(self):
        from .ops import sample_step_rows
        sample_step_rows(self.decoder.logits, self.U, self.seq, self.prompt_len, self.len, self.finished, self.params,
                         self.max_new, self.env, workspace=self.ws, next_out=self.nxt, pos_out=self.pos)

    def _read_finished(self):
        return self.finished.tolist()    # the only host read of the loop

    def _free(self, req):
        r = req.row
        req.tokens = self.seq[r, req.T:req.T + req.max_new].clone()
        req.n_dev = self.len[r:r + 1].clone()
        req.ids = None
        # a free row: finished, empty, at position 0 of the parking page
        self.finished[r] = 1
        self._ints[:, r] = 0
        self.nxt[r] = 0
        self.pos[r] = 0

    def _decode(self, max_len):
        self._upload()
        self._set_env()
        self.decoder.step(self.nxt, self.pos, max_len)
