"""KV-cache generation for ``HipQwen3ForCausalLM``: prefill, one-token decode steps and the on-GPU sampler.

What the reference does for this lives in its inference engine: the decode loop of soulxpodcast/engine/llm_engine.py:37-76,
the ``SamplingParams`` of soulxpodcast/config.py:107-118 and the HF sampling loop with repetition-aware sampling of
soulxpodcast/models/modules/sampler.py:136-189.  Here the whole step stays on the GPU: the sampler (sd_sample_step) appends
the token to a device-resident sequence buffer and hands its output straight to the next decode step
(sd_qwen3_decode_step); the host reads the ``finished`` flags once every ``sync_every`` steps and nothing else.

Prompts are right-padded (as everywhere in this package): row b's first new token takes position ``kv_len[b]`` and the
pad slots are never cached, so no row ever attends to them.

``GenerationSession`` keeps the cache and the token buffer alive between calls, the way the reference's dialogue loop
hands one ``DynamicCache`` to ``llm.generate`` for every turn (soulxpodcast/models/soulxpodcast.py:342,378-380): a turn
feeds only the tokens the cache has not seen (sd_qwen3_extend).  ``generate`` is a one-turn session.

A session given a ``PagePool`` (paged.py; the reference's engine runs vLLM's paged cache with prefix caching,
soulxpodcast/engine/llm_engine.py:91) keeps no cache buffer: it owns a page table and takes pages of 256 positions from
the pool at the start of every turn.  Its tokens are the contiguous session's, bit for bit.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check, load_lib
from .ops import _need, _stream, left_padded, sample_params, sample_step
from .paged import PAGE, PageTable, pages_for

REFERENCE_SAMPLING = dict(do_sample=True, temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.25, use_ras=True,
                          win_size=25, tau_r=0.2)  # soulxpodcast/config.py:107-118
DECODE_KERNELS = ("tile", "skinny", "wide")
WEIGHT_DTYPES = ("bf16", "mxfp8")
DECODE_ATTENTION = ("split", "fused")
GEMV_ROWS = (16, 64)   # rows the "skinny" step's GEMV kernels take; 64: the wide MXFP8 kernels (sd_gemv_mxfp8_wide)
DEFAULT_CACHE_CAPACITY = 32768  # positions; Qwen3's max_position_embeddings when the config does not say


def cache_capacity(model):
    """Most positions (prompt + new tokens) a generation may hold: ``model.kv_cache_capacity`` when set, else the
    config's ``max_position_embeddings``."""
    cap = getattr(model, "kv_cache_capacity", None) or getattr(model.config, "max_position_embeddings", None)
    return int(cap or DEFAULT_CACHE_CAPACITY)


def _check_decode_kernels(decode_kernels, weight_dtype="bf16"):
    if decode_kernels not in DECODE_KERNELS:
        raise ValueError(f"decode_kernels must be one of {DECODE_KERNELS}, got {decode_kernels!r}")
    if decode_kernels == "wide" and weight_dtype == "mxfp8":
        raise ValueError('decode_kernels="wide" streams bf16 weights only: the 64-row MXFP8 step is decode_kernels="skinny" '
                         'with gemv_rows=64 (or use "skinny" / "tile" with weight_dtype="mxfp8")')


def _check_gemv_rows(gemv_rows, decode_kernels="skinny", weight_dtype="mxfp8", decode_attention="split",
                     shared_kv_reads=False):
    """``gemv_rows``: the rows the "skinny" step's GEMV kernels take.  16 (default) changes nothing anywhere; 64 selects
    the wide MXFP8 kernels (sd_qwen3_mx_decode_step_wide) and exists for ``decode_kernels="skinny"`` with
    ``weight_dtype="mxfp8"`` on the split cache step only.  Raises before anything is allocated or launched."""
    if not isinstance(gemv_rows, int) or isinstance(gemv_rows, bool) or gemv_rows not in GEMV_ROWS:
        raise ValueError(f"gemv_rows must be one of {GEMV_ROWS}, got {gemv_rows!r}")
    if gemv_rows == 16:
        return
    if decode_kernels != "skinny":
        raise ValueError(f'gemv_rows=64 belongs to decode_kernels="skinny", got {decode_kernels!r}')
    if weight_dtype != "mxfp8":
        raise ValueError('gemv_rows=64 streams MXFP8 weights (weight_dtype="mxfp8"): the 64-row step on bf16 weights is '
                         'decode_kernels="wide"')
    if decode_attention == "fused":
        raise ValueError('gemv_rows=64 with decode_attention="fused" is not built')
    if shared_kv_reads:
        raise ValueError("gemv_rows=64 with shared_kv_reads=True is not built")


def _check_decode_attention(decode_attention):
    if decode_attention not in DECODE_ATTENTION:
        raise ValueError(f"decode_attention must be one of {DECODE_ATTENTION}, got {decode_attention!r}")


def _check_shared_kv_reads(shared_kv_reads, pool, decode_attention):
    """``shared_kv_reads=True`` needs pages that rows can share (a ``pool``) and the split cache step (the one-launch step
    reads a page per row).  Raises before anything is allocated."""
    if not shared_kv_reads:
        return
    if pool is None:
        raise ValueError("shared_kv_reads=True is for sessions over a page pool: rows of a contiguous cache share nothing "
                         "(start_session(..., pool=pool))")
    if decode_attention == "fused":
        raise ValueError('shared_kv_reads=True runs the split cache step: the one-launch step (decode_attention="fused") '
                         "reads a page once per row")


def _check_weight_dtype(model, weight_dtype):
    """The weights a generation decodes with.  "bf16": the unfolded bf16 weights, for a model whose inference precision is
    "bf16" (NotImplementedError otherwise, as before the keyword existed).  "mxfp8": the model's quantised, gain-folded
    projections (``_mx_params``), whatever its inference precision; needs what ``set_inference_precision("mxfp8")`` needs
    (ValueError).  Raises before anything is allocated or launched."""
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES}, got {weight_dtype!r}")
    if weight_dtype == "mxfp8":
        model._check_mx()
    elif model.inference_precision != "bf16":
        raise NotImplementedError('generate() decodes with the unfolded bf16 weights; this model runs "'
                                  f'{model.inference_precision}" (set_inference_precision("bf16") first, or pass '
                                  'weight_dtype="mxfp8" to decode with the quantised weights)')


def _mx_rows(data, scale):
    """MXFP8 rows (e4m3 bytes uint8 [n, K], E8M0 bytes uint8 [n, K/32]) -> the bf16 values they stand for, float(q) * 2^e
    (exact for scale bytes 3..246: include/sd_hip.h)."""
    f = data.view(torch.float8_e4m3fn).to(torch.float32).view(data.shape[0], -1, 32)
    return torch.ldexp(f, (scale.to(torch.int32) - 127)[..., None]).view(data.shape).to(torch.bfloat16)


class Decoder:
    """The KV cache [L][2][B][cap][Hkv*128] (bf16) of one batch, the activation buffers of the two runner entries, and the
    calls themselves.  ``prefill`` fills the cache from right-padded prompts and returns the logits of each row's last
    valid token; ``step`` takes one token per row at position ``pos[b]`` (= tokens already cached) and returns the next
    logits [B,V].  ``decode_kernels``: "tile" runs the step's projections on the training tile GEMMs; "skinny" (B <= 16)
    streams the weights through the GEMV kernels with the norms and the SwiGLU fused in (SD_DECODE_SKINNY) -- a row's
    logits then do not depend on the batch around it.  A step whose shapes the GEMV kernels refuse runs the tile sequence.
    "wide" (B <= 64, bf16 weights only): the same seven launches per layer on the MFMA weight-streaming kernels
    (sd_qwen3_decode_step_wide, one entry for the three cache kinds) -- batch-invariant like "skinny", with other bits than
    "skinny" (another summation order); B > 64 runs the tile sequence.  ``prefill`` and ``extend`` do not depend on the
    mode.  ``flags`` is SD_DECODE_SKINNY for "skinny" and 0 otherwise; ``wide`` says whether the wide entry is called.

    ``pool`` (a ``PagePool``): the paged form (llm_engine.py:91).  No cache buffer; the decoder owns a device page table
    int32 [B, ceil(cap / 256)] and its host mirror ``pages`` (a ``PageTable``), ``cap`` becomes that many whole pages, and
    the three calls run the paged runner entries, whose logits are bit-identical.  Whoever drives the calls by hand makes
    the rows own their pages first (``reserve``); ``gather`` stands in for ``planes``.

    A pool made with ``kv_dtype="mxfp8"`` selects the ``_paged_mx`` entries (8-bit pages, include/sd_hip.h): the rows are
    quantised as they are cached and every attention over the cache reads the quantised rows -- except inside
    ``prefill``, whose prompt attends over its own bf16 K / V in flight.  ``gather`` then returns the dequantised bf16
    rows and ``gather_raw`` the bytes.

    ``weight_dtype="mxfp8"`` (independent of the model's inference precision and of the cache kind): the three calls run
    the sd_qwen3_mx_* entries on ``model._mx_params()`` -- the four projections of every layer in MXFP8, fetched on every
    call so that ``.to()``, ``load_state_dict`` and the other invalidations are honoured; "skinny" then streams the 8-bit
    weights through sd_gemv_mxfp8.  Embedding, attention, the norms of q / k, the final norm and the lm_head stay bf16.

    ``gemv_rows`` (16, or 64 with "skinny" on MXFP8 weights and the split cache step; a ValueError otherwise, before
    anything is allocated): 64 runs the step as sd_qwen3_mx_decode_step_wide -- the skinny sequence on sd_gemv_mxfp8_wide
    for B <= 64 with the lm_head on sd_gemv_wide_bf16, batch-invariant; B > 64 runs the MXFP8 tile sequence.  The hidden
    state entering the head has the skinny step's bits at B <= 16; the logits differ as "wide" differs from "skinny".

    ``decode_attention``: "split" (default) runs each layer's cache step as the append launch and the two decode-attention
    launches; "fused" runs it as ONE launch (sd_cache_step, through sd_qwen3_decode_step_fused /
    sd_qwen3_mx_decode_step_fused: two launches fewer per layer, one memset per step).  Logits, tokens and every byte of the
    cache are those of "split", for every cache kind, ``decode_kernels`` and ``weight_dtype``; ``prefill`` and ``extend`` do
    not depend on it.  Another value is a ValueError before anything is allocated.

    ``shared_kv_reads=True`` (paged decoders on the split cache step; a ValueError otherwise, before anything is
    allocated): the decode attention of every step reads a physical page ONCE for all the rows of a group of consecutive
    rows that map it (sd_qwen3_decode_step_shared / sd_qwen3_mx_decode_step_shared) -- the rows of a forked session share
    their history's pages.  Logits, tokens and every byte of the pool are those of the default, for every
    ``decode_kernels``, ``weight_dtype`` and page dtype; rows that share nothing cost more time, never other bits."""

    def __init__(self, model, B, cap, decode_kernels="tile", pool=None, weight_dtype="bf16", decode_attention="split",
                 shared_kv_reads=False, gemv_rows=16):
        _check_decode_attention(decode_attention)
        _check_shared_kv_reads(shared_kv_reads, pool, decode_attention)
        self.shared = bool(shared_kv_reads)
        _check_decode_kernels(decode_kernels, weight_dtype)
        _check_gemv_rows(gemv_rows, decode_kernels, weight_dtype, decode_attention, shared_kv_reads)
        _check_weight_dtype(model, weight_dtype)
        self.mx_wide = gemv_rows == 64   # the step is sd_qwen3_mx_decode_step_wide
        self.flags = 1 if decode_kernels == "skinny" else 0   # include/sd_hip.h SD_DECODE_SKINNY
        self.wide = decode_kernels == "wide"
        self.fused = decode_attention == "fused"
        self.weight_dtype = weight_dtype
        self.model, self.B, self.cap = model, int(B), int(cap)
        lib = load_lib()
        dev = model.flat.device
        _need(model.flat, torch.bfloat16, "model parameters")
        d = model._cdims
        self.pool, self.pages = pool, None
        self._mx = ""
        if pool is not None:
            if pool.model is not model:
                raise ValueError("the page pool belongs to another model")
            if self.B < 1 or self.cap < 1:
                raise ValueError(f"a decoder needs B >= 1 and cap >= 1, got {B}, {cap}")
            self.max_pages = pages_for(self.cap)
            self.cap = self.max_pages * PAGE
            self.pages = PageTable(pool.alloc, self.B, self.max_pages)
            self._mx = "_mx" if pool.kv_dtype == "mxfp8" else ""   # the suffix of the runner entries this pool takes
            self.table = torch.full((self.B, self.max_pages), -1, dtype=torch.int32, device=dev)
            self._kvp = _lib.KvPages(pool.buffer.data_ptr(), pool.buffer.numel(), self.table.data_ptr(), pool.n_pages,
                                     self.max_pages)   # include/sd_hip.h sd_kv_pages: fixed for the decoder's life
            self.cache = None
        else:
            nb = lib.sd_kvcache_bytes(C.byref(d), self.B, self.cap)
            check(min(nb, 0), "sd_kvcache_bytes")
            self.cache = torch.empty(nb, dtype=torch.uint8, device=dev)
        if weight_dtype == "mxfp8" or self.wide or self.fused or self.shared:   # include/sd_hip.h sd_kv_ref: fixed for the decoder's life
            if pool is not None:
                self._kvref = _lib.KvRef(2 if self._mx else 1, None, 0, 0, C.pointer(self._kvp))
            else:
                self._kvref = _lib.KvRef(0, self.cache.data_ptr(), self.cache.numel(), self.cap, None)
            if self.fused or self.shared:
                name = "sd_qwen3%s_decode_step_%s_acts_bytes" % ("_mx" if weight_dtype == "mxfp8" else "",
                                                                 "fused" if self.fused else "shared")
            else:
                name = "sd_qwen3_decode_step_wide_acts_bytes" if self.wide else \
                    "sd_qwen3_mx_decode_step_wide_acts_bytes" if self.mx_wide else "sd_qwen3_mx_decode_step_acts_bytes"
            nb = getattr(lib, name)(C.byref(d), self.B, self.cap)
            check(min(nb, 0), name)
        else:
            nb = lib.sd_qwen3_decode_acts_bytes(C.byref(d), self.B, self.cap)
        self.step_acts = torch.empty(nb, dtype=torch.uint8, device=dev)
        self.cos, self.sin = model._tables(self.cap, dev)
        self.logits = torch.empty(self.B, model.dims.vocab_size, dtype=torch.bfloat16, device=dev)

    # ---- paged form
    def upload(self):
        """Send the table rows that changed on the host to the device table, on the launch stream (ahead of the first
        kernel that needs them)."""
        rows = sorted(self.pages.dirty)
        if rows:
            host = torch.tensor([self.pages.entries(b) for b in rows], dtype=torch.int32)
            self.table[torch.tensor(rows, dtype=torch.int64, device=self.table.device)] = host.to(self.table.device)
            self.pages.dirty.clear()

    def reserve(self, lengths):
        """Every row owns pages for ``lengths[b]`` positions (a host list).  ValueError, and nothing taken, when the pool
        cannot cover it."""
        self.pages.reserve([int(n) for n in lengths])
        self.upload()

    def gather(self, layer, b, n):
        """Copies (K, V) [n, Hkv*128] of row b's first ``n`` cached rows of one layer, through the table."""
        rows = self.gather_raw(layer, b, n)
        if not self._mx:
            return rows
        kd, ks, vd, vs = rows
        return _mx_rows(kd, ks), _mx_rows(vd, vs)

    def gather_raw(self, layer, b, n):
        """Copies of row b's first ``n`` cached rows of one layer as the pool holds them: (K, V) bf16, or of an mxfp8 pool
        the bytes (K data [n, Hkv*128], K scale [n, Hkv*4], V data, V scale), uint8."""
        pg = self.pages.rows[b][:pages_for(n)]
        if len(pg) < pages_for(n):
            raise ValueError(f"row {b} owns {len(self.pages.rows[b])} pages, fewer than {n} positions need")
        idx = torch.tensor(pg, dtype=torch.int64, device=self.table.device)
        return tuple(p[idx].flatten(0, 1)[:n].clone() for p in self.pool.planes(layer))

    def close(self):
        """Give every page back to the pool (host bookkeeping only)."""
        if self.pages is not None:
            self.pages.release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def planes(self, layer):
        """(K, V) views [B, cap, Hkv*128] of one layer's cache planes."""
        if self.pool is not None:
            raise ValueError("a paged decoder has no planes of its own: use gather(layer, b, n)")
        kd = self.model.dims.kv_dim
        n = self.B * self.cap * kd
        flat = self.cache.view(torch.bfloat16)
        k = flat[(2 * layer) * n:(2 * layer + 1) * n].view(self.B, self.cap, kd)
        v = flat[(2 * layer + 1) * n:(2 * layer + 2) * n].view(self.B, self.cap, kd)
        return k, v

    def _params(self):
        if self.model._lora is not None:
            self.model._lora.ensure_merged()   # the decoder reads the merged weights
        return self.model._cparams

    @torch.no_grad()
    def prefill(self, ids, kv_len=None):
        lib, m = load_lib(), self.model
        _need(ids, torch.int64, "input_ids")
        B, T = ids.shape
        if B != self.B or T > self.cap:
            raise ValueError(f"prefill of {tuple(ids.shape)} into a cache for {self.B} rows of {self.cap} positions")
        if self.weight_dtype == "mxfp8":
            nb = lib.sd_qwen3_mx_prefill_acts_bytes(C.byref(m._cdims), B, T)
            check(min(nb, 0), "sd_qwen3_mx_prefill_acts_bytes")
            acts = torch.empty(nb, dtype=torch.uint8, device=ids.device)
            check(lib.sd_qwen3_mx_prefill(C.byref(m._cdims), C.byref(m._mx_params()), ids.data_ptr(),
                                          0 if kv_len is None else kv_len.data_ptr(), self.cos.data_ptr(),
                                          self.sin.data_ptr(), acts.data_ptr(), nb, C.byref(self._kvref),
                                          self.logits.data_ptr(), B, T, _stream()), "sd_qwen3_mx_prefill")
            return self.logits
        nb = lib.sd_qwen3_prefill_acts_bytes(C.byref(m._cdims), B, T)
        acts = torch.empty(nb, dtype=torch.uint8, device=ids.device)
        if self.pool is not None:
            name = "sd_qwen3_prefill_paged" + self._mx
            check(getattr(lib, name)(C.byref(m._cdims), C.byref(self._params()), ids.data_ptr(),
                                     0 if kv_len is None else kv_len.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(),
                                     acts.data_ptr(), nb, C.byref(self._kvp), self.logits.data_ptr(), B, T, _stream()), name)
            return self.logits
        check(lib.sd_qwen3_prefill(C.byref(m._cdims), C.byref(self._params()), ids.data_ptr(),
                                   0 if kv_len is None else kv_len.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(),
                                   acts.data_ptr(), nb, self.cache.data_ptr(), self.cache.numel(), self.cap,
                                   self.logits.data_ptr(), B, T, _stream()), "sd_qwen3_prefill")
        return self.logits

    @torch.no_grad()
    def prefill_rows(self, rows, ids, kv_len=None):
        """The compact admission prefill of a paged decoder (engine.py): ``prefill`` for the chosen ``rows`` only (a host
        list of k distinct rows, which own their pages and whose table rows are uploaded).  Their rows of the page table
        are gathered into a scratch table [k, max_pages] and the prefill entry of this decoder's kind runs with B = k on
        ids int64 [k,T] (kv_len int32 [k], device, or None); every other row's pages and the decoder's own logits buffer
        stay untouched.  Returns new logits bf16 [k,V], row i for ``rows[i]``: with k = 1 the bits of a one-row decoder's
        ``prefill``."""
        lib, m = load_lib(), self.model
        if self.pool is None:
            raise ValueError("prefill_rows() is for decoders over a page pool")
        rows = [int(r) for r in rows]
        _need(ids, torch.int64, "input_ids")
        k, T = ids.shape if ids.dim() == 2 else (0, 0)
        if not rows or k != len(rows) or len(set(rows)) != k or min(rows) < 0 or max(rows) >= self.B or not 1 <= T <= self.cap:
            raise ValueError(f"prefill_rows of {tuple(ids.shape)} for rows {rows} of a decoder with {self.B} rows of "
                             f"{self.cap} positions")
        if kv_len is not None and (_need(kv_len, torch.int32, "kv_len").numel() != k):
            raise ValueError(f"kv_len must hold {k} lengths")
        table = self.table[torch.tensor(rows, dtype=torch.int64, device=self.table.device)].contiguous()
        kvp = _lib.KvPages(self.pool.buffer.data_ptr(), self.pool.buffer.numel(), table.data_ptr(), self.pool.n_pages,
                           self.max_pages)
        logits = torch.empty(k, m.dims.vocab_size, dtype=torch.bfloat16, device=ids.device)
        lens = 0 if kv_len is None else kv_len.data_ptr()
        if self.weight_dtype == "mxfp8":
            nb = lib.sd_qwen3_mx_prefill_acts_bytes(C.byref(m._cdims), k, T)
            check(min(nb, 0), "sd_qwen3_mx_prefill_acts_bytes")
            acts = torch.empty(nb, dtype=torch.uint8, device=ids.device)
            kvref = _lib.KvRef(2 if self._mx else 1, None, 0, 0, C.pointer(kvp))
            check(lib.sd_qwen3_mx_prefill(C.byref(m._cdims), C.byref(m._mx_params()), ids.data_ptr(), lens,
                                          self.cos.data_ptr(), self.sin.data_ptr(), acts.data_ptr(), nb, C.byref(kvref),
                                          logits.data_ptr(), k, T, _stream()), "sd_qwen3_mx_prefill")
            return logits
        nb = lib.sd_qwen3_prefill_acts_bytes(C.byref(m._cdims), k, T)
        acts = torch.empty(nb, dtype=torch.uint8, device=ids.device)
        name = "sd_qwen3_prefill_paged" + self._mx
        check(getattr(lib, name)(C.byref(m._cdims), C.byref(self._params()), ids.data_ptr(), lens, self.cos.data_ptr(),
                                 self.sin.data_ptr(), acts.data_ptr(), nb, C.byref(kvp), logits.data_ptr(), k, T, _stream()),
              name)
        return logits

    @torch.no_grad()
    def extend(self, ids, past, new_len):
        """A block of right-padded NEW tokens ids int64 [B,T] behind ``past[b]`` cached positions (int32 [B], device):
        tokens t < new_len[b] take positions past[b] + t and go into the cache; returns the logits [B,V] of each row's
        last new token (sd_qwen3_extend)."""
        lib, m = load_lib(), self.model
        _need(ids, torch.int64, "input_ids"), _need(past, torch.int32, "past"), _need(new_len, torch.int32, "new_len")
        B, T = ids.shape
        if B != self.B or T < 1 or T > self.cap or past.numel() != B or new_len.numel() != B:
            raise ValueError(f"extend of {tuple(ids.shape)} into a cache for {self.B} rows of {self.cap} positions")
        if self.weight_dtype == "mxfp8":
            nb = lib.sd_qwen3_mx_extend_acts_bytes(C.byref(m._cdims), B, T)
            check(min(nb, 0), "sd_qwen3_mx_extend_acts_bytes")
            acts = torch.empty(nb, dtype=torch.uint8, device=ids.device)
            check(lib.sd_qwen3_mx_extend(C.byref(m._cdims), C.byref(m._mx_params()), ids.data_ptr(), past.data_ptr(),
                                         new_len.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(), acts.data_ptr(), nb,
                                         C.byref(self._kvref), self.logits.data_ptr(), B, T, _stream()),
                  "sd_qwen3_mx_extend")
            return self.logits
        nb = lib.sd_qwen3_extend_acts_bytes(C.byref(m._cdims), B, T)
        check(min(nb, 0), "sd_qwen3_extend_acts_bytes")
        acts = torch.empty(nb, dtype=torch.uint8, device=ids.device)
        if self.pool is not None:
            name = "sd_qwen3_extend_paged" + self._mx
            check(getattr(lib, name)(C.byref(m._cdims), C.byref(self._params()), ids.data_ptr(), past.data_ptr(),
                                     new_len.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(), acts.data_ptr(), nb,
                                     C.byref(self._kvp), self.logits.data_ptr(), B, T, _stream()), name)
            return self.logits
        check(lib.sd_qwen3_extend(C.byref(m._cdims), C.byref(self._params()), ids.data_ptr(), past.data_ptr(),
                                  new_len.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(), acts.data_ptr(), nb,
                                  self.cache.data_ptr(), self.cache.numel(), self.cap, self.logits.data_ptr(), B, T,
                                  _stream()), "sd_qwen3_extend")
        return self.logits

    @torch.no_grad()
    def step(self, ids, pos, max_len):
        """ids int64 [B], pos int32 [B] (device); max_len: host upper bound of every pos[b] + 1."""
        lib, m = load_lib(), self.model
        _need(ids, torch.int64, "ids"), _need(pos, torch.int32, "pos")
        if ids.numel() != self.B or pos.numel() != self.B:
            raise ValueError(f"decode step wants {self.B} tokens and positions")
        if self.fused or self.shared:   # one entry per weight dtype, over the cache of any kind (shared: any paged kind)
            how = "fused" if self.fused else "shared"
            if self.weight_dtype == "mxfp8":
                name, params, kind = "sd_qwen3_mx_decode_step_" + how, m._mx_params(), self.flags
            else:   # kernels: 0 tile, 1 skinny, 2 wide
                name, params, kind = "sd_qwen3_decode_step_" + how, self._params(), 2 if self.wide else self.flags
            check(getattr(lib, name)(C.byref(m._cdims), C.byref(params), ids.data_ptr(), pos.data_ptr(), int(max_len),
                                     self.cos.data_ptr(), self.sin.data_ptr(), C.byref(self._kvref),
                                     self.step_acts.data_ptr(), self.step_acts.numel(), self.logits.data_ptr(), self.B,
                                     kind, _stream()), name)
            return self.logits
        if self.mx_wide:
            check(lib.sd_qwen3_mx_decode_step_wide(C.byref(m._cdims), C.byref(m._mx_params()), ids.data_ptr(),
                                                   pos.data_ptr(), int(max_len), self.cos.data_ptr(), self.sin.data_ptr(),
                                                   C.byref(self._kvref), self.step_acts.data_ptr(), self.step_acts.numel(),
                                                   self.logits.data_ptr(), self.B, _stream()),
                  "sd_qwen3_mx_decode_step_wide")
            return self.logits
        if self.weight_dtype == "mxfp8":
            check(lib.sd_qwen3_mx_decode_step(C.byref(m._cdims), C.byref(m._mx_params()), ids.data_ptr(), pos.data_ptr(),
                                              int(max_len), self.cos.data_ptr(), self.sin.data_ptr(), C.byref(self._kvref),
                                              self.step_acts.data_ptr(), self.step_acts.numel(), self.logits.data_ptr(),
                                              self.B, self.flags, _stream()), "sd_qwen3_mx_decode_step")
            return self.logits
        if self.wide:
            check(lib.sd_qwen3_decode_step_wide(C.byref(m._cdims), C.byref(self._params()), ids.data_ptr(), pos.data_ptr(),
                                                int(max_len), self.cos.data_ptr(), self.sin.data_ptr(), C.byref(self._kvref),
                                                self.step_acts.data_ptr(), self.step_acts.numel(), self.logits.data_ptr(),
                                                self.B, _stream()), "sd_qwen3_decode_step_wide")
            return self.logits
        if self.pool is not None:
            name = "sd_qwen3_decode_step_paged" + self._mx
            check(getattr(lib, name)(C.byref(m._cdims), C.byref(self._params()), ids.data_ptr(), pos.data_ptr(),
                                     int(max_len), self.cos.data_ptr(), self.sin.data_ptr(), C.byref(self._kvp),
                                     self.step_acts.data_ptr(), self.step_acts.numel(), self.logits.data_ptr(), self.B,
                                     self.flags, _stream()), name)
            return self.logits
        check(lib.sd_qwen3_decode_step_flags(C.byref(m._cdims), C.byref(self._params()), ids.data_ptr(), pos.data_ptr(),
                                             int(max_len), self.cos.data_ptr(), self.sin.data_ptr(), self.cache.data_ptr(),
                                             self.cache.numel(), self.cap, self.step_acts.data_ptr(),
                                             self.step_acts.numel(), self.logits.data_ptr(), self.B, self.flags, _stream()),
              "sd_qwen3_decode_step_flags")
        return self.logits


def _check_args(model, B, T, max_new_tokens, min_new_tokens, do_sample, temperature, top_k, top_p, repetition_penalty,
                use_ras, win_size, tau_r, sync_every, decode_kernels="tile", model_capacity=True, weight_dtype="bf16",
                decode_attention="split", gemv_rows=16):
    """``model_capacity``: also hold T + max_new_tokens against ``cache_capacity(model)`` (a session holds its own
    lengths against its own capacity instead)."""
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES}, got {weight_dtype!r}")
    _check_decode_attention(decode_attention)
    _check_decode_kernels(decode_kernels, weight_dtype)
    _check_gemv_rows(gemv_rows, decode_kernels, weight_dtype, decode_attention)
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be at least 1, got {max_new_tokens}")
    if top_k < 0 or top_k > 128:
        raise ValueError(f"top_k must be in 0..128 (the sampler keeps at most 128 candidates), got {top_k}")
    cap = cache_capacity(model)
    if model_capacity and T + max_new_tokens > cap:
        raise ValueError(f"prompt length {T} + max_new_tokens {max_new_tokens} exceeds the KV-cache capacity {cap}")
    _check_weight_dtype(model, weight_dtype)
    if min_new_tokens < 0 or sync_every < 1:
        raise ValueError("min_new_tokens must be >= 0 and sync_every >= 1")
    if do_sample:
        if not temperature > 0 or not 0 < top_p <= 1 or not repetition_penalty > 0:
            raise ValueError("sampling needs temperature > 0, 0 < top_p <= 1 and repetition_penalty > 0")
        if top_k == 0 and (top_p < 1 or use_ras):
            raise ValueError("top_p < 1 and use_ras work on the sorted top-k candidates: give top_k in 1..128")
        if use_ras and (win_size < 1 or not tau_r > 0):
            raise ValueError("use_ras needs win_size >= 1 and tau_r > 0")


class GenerationSession:
    """A live generation: ONE cache of ``capacity`` positions per row, the device buffers ``seq`` int64 [B,capacity] (each
    row's whole sequence), ``len`` int32 [B] (tokens in it) and ``cached`` int32 [B] (positions whose K / V the cache
    holds), kept across calls (soulxpodcast.py:342: one DynamicCache; :378-380: every turn continues it).

    A turn (``generate``) writes the right-padded new tokens behind each row's sequence, runs sd_qwen3_extend over each
    row's uncached suffix ``seq[b, cached[b]:len[b]]``, and then runs the sampler / decode-step loop with ``prompt_len =
    len``: the repetition penalty and ``min_new_tokens`` count from the turn's start (the reference passes the whole
    history as the prompt), the RAS window looks at the last ``win_size`` tokens of the whole sequence.  After a turn every
    row's last sampled token is in ``seq`` but not in the cache (``cached = len - 1``): that covers an EOS too, whose slot
    the loop keeps rewriting with the pad token's K / V.  The next turn's suffix starts with that token, exactly as HF
    feeds it.  The host knows the suffix is {0 or 1} + T_in columns wide without a read.  ``extend`` appends and caches
    without sampling and leaves nothing uncached.

    When nothing is cached in any row (a new session, or after ``reset()`` of all rows) the turn's first pass is
    sd_qwen3_prefill, so a one-turn session returns ``model.generate``'s tokens bit for bit.

    The host keeps an upper bound of the lengths (old bound + T_in + max_new_tokens) and reads the true lengths only when
    that bound would pass ``capacity``.  ``decode_kernels="skinny"``: the decode STEPS are batch-invariant; the extend pass
    runs the tile GEMMs at M = B * T, so a row equals the row generated alone within a turn's decode steps only.
    ``decode_kernels="wide"`` (bf16 weights): the same for up to 64 rows, on the MFMA weight-streaming kernels.

    ``pool`` (a ``PagePool``; llm_engine.py:91): the paged session.  It holds no cache buffer but a page table, and several
    sessions may share one pool.  Allocation rule: a paged session ALWAYS takes its one host read at the start of a turn,
    and that read also carries the per-row lengths.  There the host first gives back the pages a row no longer needs (whole
    pages past its true length, left over from the previous turn's worst case), then gives every row pages for ``len[b] +
    n_in[b] + max_new_tokens`` positions and uploads the changed table rows on the launch stream ahead of the first kernel.
    Inside the decode loop no table changes and no extra host read happens.  A pool that cannot cover the turn raises
    ValueError before anything is launched on the session's state, and no page has then changed hands.  ``reset`` releases
    the rows' pages, ``trim()`` releases the worst-case leftovers on demand, ``fork(rows)`` continues rows in a new
    session that shares their full pages, ``close()`` (also run when the session is dropped) releases everything.  A pool
    of 8-bit pages (``kv_page_pool(..., kv_dtype="mxfp8")``) changes none of this: the decoder picks its entries from
    the pool's dtype.

    ``weight_dtype="mxfp8"``: every pass of every turn (prefill, extend, decode steps) runs the model's MXFP8 projections
    (``Decoder``); ``fork`` keeps it.  Everything else above holds unchanged.

    ``decode_attention="fused"``: the decode steps of every turn run each layer's cache step as one launch (``Decoder``),
    with the tokens and the cache bytes of "split"; ``fork`` keeps it.

    ``shared_kv_reads=True`` (paged sessions on the split cache step): the decode steps read a page that several rows of
    a group map once for all of them (``Decoder``), with the tokens and the pool bytes of the default.  It pays where rows
    share pages -- ``fork([0] * 8, shared_kv_reads=True)`` turns the keyword on for the continuations alone; ``fork``
    inherits it otherwise.

    ``gemv_rows=64`` (with ``decode_kernels="skinny"``, ``weight_dtype="mxfp8"``): the decode steps stream the 8-bit
    weights through the 64-row kernels (``Decoder``), batch-invariant for up to 64 rows; ``fork`` inherits it.  A fork
    that asks for ``shared_kv_reads=True`` on such a session is a ValueError."""

    def __init__(self, model, batch_size, capacity=None, decode_kernels="tile", pool=None, weight_dtype="bf16",
                 decode_attention="split", shared_kv_reads=False, gemv_rows=16):
        _check_decode_attention(decode_attention)
        _check_shared_kv_reads(shared_kv_reads, pool, decode_attention)
        self.model, self.B = model, int(batch_size)
        self.capacity = int(capacity) if capacity is not None else cache_capacity(model)
        if self.B < 1 or self.capacity < 1:
            raise ValueError(f"a session needs batch_size >= 1 and capacity >= 1, got {batch_size}, {capacity}")
        self.pool, self.decode_kernels, self.weight_dtype = pool, decode_kernels, weight_dtype
        self.decode_attention, self.shared_kv_reads = decode_attention, bool(shared_kv_reads)
        self.gemv_rows = gemv_rows
        self.decoder = Decoder(model, self.B, self.capacity, decode_kernels, pool=pool, weight_dtype=weight_dtype,
                               decode_attention=decode_attention, shared_kv_reads=shared_kv_reads, gemv_rows=gemv_rows)
        dev = model.flat.device
        self.seq = torch.zeros(self.B, self.capacity, dtype=torch.int64, device=dev)
        self.len = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.cached = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._fresh, self._pending, self._bound = True, False, 0

    def lengths(self):
        """int32 [B] (device): tokens in each row's sequence."""
        return self.len.clone()

    def tokens(self):
        """List of B 1-D int64 tensors: each row's whole sequence so far (one host read of the lengths)."""
        return [self.seq[b, :n].clone() for b, n in enumerate(self.len.tolist())]

    def reset(self, rows=None):
        """Forget the sequences of ``rows`` (all rows when None): their ``len`` and ``cached`` become 0.  The mechanism of
        the reference's history rebuild (soulxpodcast.py:346-373); the policy itself is the caller's."""
        if rows is None:
            self.len.zero_(), self.cached.zero_()
            self._fresh, self._pending, self._bound = True, False, 0
            if self.pool is not None:
                self.decoder.pages.release()
                self.decoder.upload()
            return
        idx = torch.as_tensor(rows, dtype=torch.int64, device=self.len.device).reshape(-1)
        self.len[idx] = 0
        self.cached[idx] = 0
        if self.pool is not None:
            self.decoder.pages.release(sorted(set(torch.as_tensor(rows).reshape(-1).tolist())))
            self.decoder.upload()

    def trim(self):
        """Paged sessions: give back every row's whole pages past its true length (the leftovers of the last turn's
        worst case), with one host read of the lengths.  The next turn does this by itself."""
        if self.pool is None:
            raise ValueError("trim() is for sessions over a page pool")
        self.decoder.pages.trim(self.len.tolist())
        self.decoder.upload()

    def close(self):
        """Release the session's pages (paged sessions; a no-op otherwise).  The session holds nothing afterwards."""
        if self.pool is not None:
            self.decoder.close()
            self.len.zero_(), self.cached.zero_()
            self._fresh, self._pending, self._bound = True, False, 0

    def __del__(self):
        try:
            if self.pool is not None:
                self.decoder.close()
        except Exception:
            pass

    def fork(self, rows, shared_kv_reads=None):
        """A new session on the same pool whose row i continues this session's row ``rows[i]`` (repeats allowed: ``fork([0]
        * 8)`` gives 8 continuations of row 0), with one host read of the source lengths.  Pages wholly below ``cached[src]``
        are shared -- a row only writes at positions >= cached[b], so nobody writes there again; the page that holds
        position ``cached[src]`` is copied across all layers when that position does not start a page.  ``seq``, ``len``,
        ``cached`` and the session flags are copied.  ``shared_kv_reads``: the new session's switch (None: this session's).
        ValueError on a contiguous session, for ``shared_kv_reads=True`` on a session with ``decode_attention="fused"``, or
        when the pool lacks the pages for the copies (nothing has changed then)."""
        if self.pool is None:
            raise ValueError("fork() is for sessions over a page pool (start_session(..., pool=pool))")
        shared = self.shared_kv_reads if shared_kv_reads is None else bool(shared_kv_reads)
        _check_shared_kv_reads(shared, self.pool, self.decode_attention)
        _check_gemv_rows(self.gemv_rows, self.decode_kernels, self.weight_dtype, self.decode_attention, shared)
        rows = [int(r) for r in rows]
        if not rows or min(rows) < 0 or max(rows) >= self.B:
            raise ValueError(f"fork rows must lie in [0, {self.B}), got {rows}")
        new = GenerationSession.__new__(GenerationSession)
        new.model, new.B, new.capacity, new.pool, new.decode_kernels = self.model, len(rows), self.capacity, self.pool, \
            self.decode_kernels
        new.weight_dtype, new.decode_attention, new.shared_kv_reads = self.weight_dtype, self.decode_attention, shared
        new.gemv_rows = self.gemv_rows
        new.decoder = Decoder(self.model, new.B, self.capacity, self.decode_kernels, pool=self.pool,
                              weight_dtype=self.weight_dtype, decode_attention=self.decode_attention,
                              shared_kv_reads=shared, gemv_rows=self.gemv_rows)
        cached = self.cached.tolist()   # the one host read
        new.decoder.pages, copies = self.decoder.pages.fork(rows, cached)   # raises before anything changed
        self.pool.copy_pages(copies)
        new.decoder.upload()
        idx = torch.tensor(rows, dtype=torch.int64, device=self.len.device)
        new.seq, new.len, new.cached = self.seq[idx].clone(), self.len[idx].clone(), self.cached[idx].clone()
        new._fresh, new._pending, new._bound = self._fresh, self._pending, self._bound
        return new

    def _take(self, input_ids, attention_mask, max_new_tokens, sampling):
        """Every check of a turn (one host read at most), then the new tokens go behind the sequences and the uncached
        suffixes through the model.  -> logits [B,V]."""
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [B,T], got {tuple(input_ids.shape)}")
        B, T = input_ids.shape
        if B != self.B:
            raise ValueError(f"this session holds {self.B} rows, got a batch of {B}")
        ids = _need(input_ids.to(torch.int64), torch.int64, "input_ids")
        dev = ids.device
        am = None
        if attention_mask is not None:
            am = attention_mask.to(dev)
            if am.shape != ids.shape:
                raise ValueError(f"attention_mask {tuple(am.shape)} != input_ids {tuple(ids.shape)}")
            n_in = am.sum(-1).to(torch.int32).contiguous()
        else:
            n_in = torch.full((B,), T, dtype=torch.int32, device=dev)
        W = (1 if self._pending else 0) + T    # columns of the widest uncached suffix
        bound = self._bound + T + max_new_tokens
        if W < 1:
            raise ValueError("every prompt needs at least one token")
        new_len = self.len + n_in
        if W > self.capacity:
            raise ValueError(f"{W} new positions exceed the session's KV-cache capacity {self.capacity}")
        paged = self.pool is not None
        if paged or am is not None or T == 0 or bound > self.capacity:
            bad = left_padded(am).to(torch.int32).reshape(()) if am is not None and T > 0 else new_len.min() * 0
            head = torch.stack([bad, new_len.min(), (new_len - self.cached).min(), new_len.max()])
            if paged:   # the read also carries the per-row lengths
                head = torch.cat([head, self.len, new_len])
            host = head.tolist()   # the one host read
            bad, shortest, fewest, longest = host[:4]
            if bad:
                raise ValueError("attention_mask is not right-padded (a 1 follows a 0): the HIP attention kernels take a "
                                 "valid-prefix length per sequence, as ProcessedDataCollator produces (data.py:280-327)")
            if shortest < 1:
                raise ValueError("every prompt needs at least one token")
            if sampling and fewest < 1:
                raise ValueError("a row has no uncached token to continue from: give every row at least one token")
            bound = min(bound, longest + max_new_tokens)
            if longest + max_new_tokens > self.capacity:
                raise ValueError(f"sequence length {longest} + max_new_tokens {max_new_tokens} exceeds the session's "
                                 f"KV-cache capacity {self.capacity}")
            if paged:   # give back last turn's leftovers, take this turn's worst case: ValueError changes nothing
                self.decoder.pages.admit(host[4:4 + B], [n + max_new_tokens for n in host[4 + B:]])
                self.decoder.upload()
        # ---- nothing was launched on the session's state up to here
        col = torch.arange(self.capacity, device=dev, dtype=torch.int32)[None, :]
        if T > 0:
            j = col - self.len[:, None]
            mine = (j >= 0) & (j < n_in[:, None])
            self.seq = torch.where(mine, ids.gather(1, j.clamp(0, T - 1).to(torch.int64)), self.seq)
        if self._fresh:
            logits = self.decoder.prefill(ids, n_in)
        else:
            cols = (self.cached[:, None] + col[:, :W]).clamp(max=self.capacity - 1).to(torch.int64)
            logits = self.decoder.extend(self.seq.gather(1, cols).contiguous(), self.cached, (new_len - self.cached).contiguous())
        self.len = new_len.contiguous()
        self.cached = self.len.clone()
        self._fresh, self._pending, self._bound = False, False, bound - max_new_tokens
        return logits

    @torch.no_grad()
    def extend(self, input_ids, attention_mask=None):
        """Append right-padded tokens to the rows and cache them, without sampling.  Returns bf16 [B,V]: the logits of
        each row's last token (a copy).  A row whose mask is empty sits the call out; its logits row is then meaningless."""
        return self._take(input_ids, attention_mask, 0, False).clone()

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, max_new_tokens=20, min_new_tokens=0, do_sample=True, temperature=1.0,
                 top_k=0, top_p=1.0, repetition_penalty=1.0, eos_token_id=None, pad_token_id=None, use_ras=False,
                 win_size=25, tau_r=0.2, seed=None, sync_every=16):
        """One turn: the sampling arguments of ``HipQwen3ForCausalLM.generate``.  Returns the NEW tokens only, int64
        [B, max_new_tokens], ``pad_token_id`` after a row's EOS.  Every error is raised before anything is launched on the
        session's state."""
        model, B = self.model, self.B
        T = input_ids.shape[1] if input_ids.dim() == 2 else 0
        _check_args(model, B, T, max_new_tokens, min_new_tokens, do_sample, temperature, top_k, top_p, repetition_penalty,
                    use_ras, win_size, tau_r, sync_every, model_capacity=False, weight_dtype=self.weight_dtype)
        V = model.dims.vocab_size
        pad = pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)
        if not 0 <= pad < V or (eos_token_id is not None and not 0 <= eos_token_id < V):
            raise ValueError(f"pad / eos token ids must lie in [0, {V})")
        logits = self._take(input_ids, attention_mask, max_new_tokens, True)
        dev = self.seq.device
        dec, cap = self.decoder, self.capacity
        # slots behind a row's sequence read as pad (the output gathers them for a row that stops early)
        col = torch.arange(cap, device=dev, dtype=torch.int32)[None, :]
        self.seq = torch.where(col < self.len[:, None], self.seq, torch.full_like(self.seq, pad))
        start, lens = self.len.clone(), self.len
        finished = torch.zeros(B, dtype=torch.uint8, device=dev)
        nxt = torch.empty(B, dtype=torch.int64, device=dev)
        pos = torch.empty(B, dtype=torch.int32, device=dev)
        sp = sample_params(do_sample, temperature, top_k, top_p, repetition_penalty, min_new_tokens, eos_token_id, pad,
                           use_ras, win_size, tau_r)
        ws = torch.empty(load_lib().sd_sample_workspace_bytes(B, V), dtype=torch.uint8, device=dev)
        gen = None
        if seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
        u = torch.rand(max_new_tokens, B, 2, generator=gen, device=dev, dtype=torch.float32)  # every step's uniforms, one launch
        base = self._bound    # host upper bound of every row's length before the first new token
        for step in range(max_new_tokens):
            sample_step(logits, u[step], self.seq, start, lens, finished, sp, workspace=ws, next_out=nxt, pos_out=pos)
            if step + 1 == max_new_tokens:
                break
            if (step + 1) % sync_every == 0 and bool(finished.all()):   # the only host read of the loop
                break
            logits = dec.step(nxt, pos, base + step + 1)
        # every row's last sampled token (an EOS included: its slot holds the pad steps' K / V) is not in the cache
        self.cached = lens - 1
        self._pending, self._bound = True, base + max_new_tokens
        # row b's new tokens sit at seq[b, start[b] ...]; slots never written still hold pad
        cols = start.to(torch.int64)[:, None] + torch.arange(max_new_tokens, device=dev)[None, :]
        return self.seq.gather(1, cols)


@torch.no_grad()
def generate(model, input_ids, attention_mask=None, max_new_tokens=20, min_new_tokens=0, do_sample=True, temperature=1.0,
             top_k=0, top_p=1.0, repetition_penalty=1.0, eos_token_id=None, pad_token_id=None, use_ras=False, win_size=25,
             tau_r=0.2, seed=None, sync_every=16, decode_kernels="tile", weight_dtype="bf16", decode_attention="split",
             gemv_rows=16):
    """See ``HipQwen3ForCausalLM.generate``: a one-turn ``GenerationSession``."""
    if input_ids.dim() != 2:
        raise ValueError(f"input_ids must be [B,T], got {tuple(input_ids.shape)}")
    B, T = input_ids.shape
    _check_args(model, B, T, max_new_tokens, min_new_tokens, do_sample, temperature, top_k, top_p, repetition_penalty,
                use_ras, win_size, tau_r, sync_every, decode_kernels, weight_dtype=weight_dtype,
                decode_attention=decode_attention, gemv_rows=gemv_rows)
    cap = (T + max_new_tokens + 255) // 256 * 256   # whole attention partitions; the output bits do not depend on it
    sess = GenerationSession(model, B, cap, decode_kernels, weight_dtype=weight_dtype, decode_attention=decode_attention,
                             gemv_rows=gemv_rows)
    new = sess.generate(input_ids, attention_mask, max_new_tokens, min_new_tokens, do_sample, temperature, top_k, top_p,
                        repetition_penalty, eos_token_id, pad_token_id, use_ras, win_size, tau_r, seed, sync_every)
    return torch.cat([input_ids.to(torch.int64), new], dim=1)
