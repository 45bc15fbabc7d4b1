"""Qwen3 causal LM (student 0.6B-shape / teacher SoulX-Podcast-1.7B-shape) on the HIP step runner.

Model protocol the reference relies on: callable
``model(input_ids=, attention_mask=, labels=?, **kw)`` returning an object with ``.logits`` [B,T,V]
(train.py:54-55, 63-69); ``.eval()``, ``.parameters()``, ``requires_grad_`` (train.py:165-169);
``gradient_checkpointing_enable()`` / ``enable_input_require_grads()`` (train.py:206-208); ``.config``;
``state_dict`` with HF key names.  The forward keeps ``**kwargs`` so that HF Trainer's
``model_accepts_loss_kwargs`` stays True exactly as for HF Qwen3 (quirk Q1).

Layout in HBM: ONE flat bf16 parameter buffer and ONE flat bf16 gradient buffer, ordered
[embed | layer 0 .. layer L-1 | final norm]; inside a layer q|k|v projection rows are contiguous
(one fused [4096,h] GEMM) and so are gate|up.  HF-named ``nn.Parameter``s are views into the flat
buffers, so a data-parallel all-reduce bucket is a plain slice.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, load_lib
from .ops import _need, _p, _stream, left_padded, rope_tables  # noqa: F401  (left_padded is re-exported)


class PackedBatch:
    """One call's packed documents (padding-free packing, HF ``position_ids`` without ``attention_mask``): the int32
    ``cu_seqlens`` on the device, the C descriptor (include/sd_hip.h sd_varlen) and the per-token RoPE tables (row m =
    the angles of token m's position).  Kept by the autograd function for the backward."""

    def __init__(self, cu_host, cos, sin, device, rope_theta=None):
        self._set(cu_host.to(torch.int32).to(device), int(cu_host[-1]), cu_host.numel() - 1,
                  int((cu_host[1:] - cu_host[:-1]).max()), cos, sin, rope_theta)

    @classmethod
    def from_device(cls, cu_seqlens, M, n, max_seqlen, cos, sin, rope_theta=None):
        """From an int32 ``cu_seqlens`` [n+1] already on the device and already checked (``ops.packed_rows``: it rises from
        0 to M, its longest document is ``max_seqlen``): no host read.  ``rope_theta``: the base of the tables, so that a
        second model can tell whether this descriptor's RoPE rows are its own."""
        if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() != n + 1:
            raise ValueError(f"PackedBatch: cu_seqlens must be int32 [{n + 1}], got {cu_seqlens.dtype} {tuple(cu_seqlens.shape)}")
        if cos.shape != sin.shape or cos.dim() != 2 or cos.size(0) != M:
            raise ValueError(f"PackedBatch: RoPE tables must be [{M}, head_dim], got {tuple(cos.shape)} / {tuple(sin.shape)}")
        pb = cls.__new__(cls)
        pb._set(cu_seqlens.contiguous(), int(M), int(n), int(max_seqlen), cos, sin, rope_theta)
        return pb

    def _set(self, cu, M, n, max_seqlen, cos, sin, rope_theta):
        from . import ops
        self.M, self.n, self.max_seqlen, self.cu = M, n, max_seqlen, cu
        nb = load_lib().sd_varlen_work_bytes(self.M)
        self.work = torch.empty(nb, dtype=torch.uint8, device=cu.device) if nb > 0 else None
        self.desc = ops.varlen_desc(self.cu, self.max_seqlen, self.work)
        self.cos, self.sin, self.rope_theta = cos, sin, rope_theta

    def tensors(self):
        """The device tensors a stream must keep alive while it uses this descriptor."""
        return [t for t in (self.cu, self.work, self.cos, self.sin) if t is not None]


@dataclass
class Qwen3Dims:
    vocab_size: int
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    num_key_value_heads: int
    head_dim: int = 128
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1e6
    tie_word_embeddings: bool = True

    @property
    def q_dim(self):
        return self.num_attention_heads * self.head_dim

    @property
    def kv_dim(self):
        return self.num_key_value_heads * self.head_dim

    @classmethod
    def from_hf_config(cls, c):
        """From an HF Qwen3Config (transformers 4.x keeps ``rope_theta`` on the config, 5.x in ``rope_parameters``)."""
        rope = getattr(c, "rope_theta", None)
        if rope is None:
            rope = (getattr(c, "rope_parameters", None) or {}).get("rope_theta", 1e6)
        return cls(c.vocab_size, c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads,
                   c.num_key_value_heads, getattr(c, "head_dim", None) or 128, c.rms_norm_eps, float(rope),
                   bool(c.tie_word_embeddings))

    @classmethod
    def student_06b(cls):  # public Qwen3-0.6B shape, vocab expanded to the teacher's (prepare_student.py:31,79-82)
        return cls(159488, 1024, 3072, 28, 16, 8)

    @classmethod
    def teacher_17b(cls):  # soulxpodcast/config.py:12-42
        return cls(159488, 2048, 6144, 28, 16, 8)

    def matmul_params(self):
        """Parameters that take part in a matmul per token: the decoder's projections + the (tied) lm_head."""
        h, I = self.hidden_size, self.intermediate_size
        per_layer = h * (self.q_dim + 2 * self.kv_dim) + self.q_dim * h + 3 * h * I
        return self.num_hidden_layers * per_layer + self.vocab_size * h

    def flops_per_token(self, T):
        """Algorithmic forward FLOPs per token: 2 per matmul parameter + causal attention
        (half of 4*T*Hq*d per layer).  Backward = 2x this; a distillation micro-step = 3x student + 1x teacher."""
        attn = 0.5 * 4 * T * self.num_attention_heads * self.head_dim * self.num_hidden_layers
        return 2 * self.matmul_params() + attn

    def lm_head_flops_per_row(self):
        return 2.0 * self.hidden_size * self.vocab_size


class _Holder(nn.Module):
    """Leaf module owning one HF-named ``weight`` Parameter (a view into the flat buffer)."""

    def __init__(self, w):
        super().__init__()
        self.weight = w


class CausalLMOutput(dict):
    """Minimal ModelOutput: attribute + key access, like HF's CausalLMOutputWithPast."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


SAVE_NONE, SAVE_ALL, SAVE_LAYER_INPUTS, SAVE_NONE_FOLDED = 0, 1, 2, 3  # include/sd_hip.h SD_SAVE_*
FWD_CONCURRENT = 0x100                            # SD_FWD_CONCURRENT
BWD_ACCUMULATE, BWD_RECOMPUTE, BWD_EMBED_ONLY = 1, 2, 4   # SD_BWD_*


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, input_ids, kv_len, model, rows, concurrent=False, packed=None):
        batch, shape = model._batch(input_ids, kv_len, rows, packed)
        save = SAVE_LAYER_INPUTS if model._wants_recompute(*shape, input_ids.device) else SAVE_ALL
        logits, acts = model._run_forward(input_ids, kv_len, save=save, rows=rows, concurrent=concurrent, packed=packed,
                                          batch=batch)
        ctx.model, ctx.acts, ctx.ids, ctx.kv_len, ctx.rows, ctx.save = model, acts, input_ids, kv_len, rows, save
        ctx.packed, ctx.batch = packed, batch
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        ctx.model._run_backward(ctx.ids, ctx.kv_len, ctx.acts, dlogits, rows=ctx.rows,
                                recompute=ctx.save == SAVE_LAYER_INPUTS, packed=ctx.packed, batch=ctx.batch)
        ctx.acts = ctx.packed = ctx.batch = None
        return torch.zeros((), device=dlogits.device), None, None, None, None, None, None


class HipQwen3ForCausalLM(nn.Module):
    def __init__(self, dims: Qwen3Dims, device="cuda", config=None, init_std=0.02, seed=0):
        super().__init__()
        if dims.head_dim != 128:
            raise ValueError("the gfx950 attention / RoPE kernels are specialised for head_dim 128")
        self.dims = dims
        self.config = config if config is not None else self._hf_config(dims)
        self.gradient_checkpointing = False
        self.recompute_policy, self.recompute_fraction = "auto", 0.25
        d = dims
        h, I, qd, kd = d.hidden_size, d.intermediate_size, d.q_dim, d.kv_dim
        # ---- flat layout
        self._slices = {}
        off = 0

        def take(name, shape):
            nonlocal off
            n = 1
            for s in shape:
                n *= s
            self._slices[name] = (off, n, shape)
            off += (n + 7) // 8 * 8  # keep every tensor 16-byte aligned
        take("model.embed_tokens.weight", (d.vocab_size, h))
        self.layer_ranges = []
        for l in range(d.num_hidden_layers):
            p = f"model.layers.{l}."
            start = off
            take(p + "self_attn.q_proj.weight", (qd, h))
            take(p + "self_attn.k_proj.weight", (kd, h))
            take(p + "self_attn.v_proj.weight", (kd, h))
            take(p + "self_attn.o_proj.weight", (h, qd))
            take(p + "mlp.gate_proj.weight", (I, h))
            take(p + "mlp.up_proj.weight", (I, h))
            take(p + "mlp.down_proj.weight", (h, I))
            take(p + "self_attn.q_norm.weight", (128,))
            take(p + "self_attn.k_norm.weight", (128,))
            take(p + "input_layernorm.weight", (h,))
            take(p + "post_attention_layernorm.weight", (h,))
            self.layer_ranges.append((start, off))
        self.norm_range = (off, off + h)
        take("model.norm.weight", (h,))
        if not d.tie_word_embeddings:
            take("lm_head.weight", (d.vocab_size, h))
        self.numel_flat = off
        self.embed_range = (0, self._slices["model.embed_tokens.weight"][1])
        dev = torch.device(device)
        self.flat = torch.zeros(off, dtype=torch.bfloat16, device=dev)
        self.flat_grad = None
        self._grads_live = False
        # ---- HF-named parameters (views)
        self.model = nn.Module()
        self.model.layers = nn.ModuleList()
        self._params = {}
        for name, (o, n, shape) in self._slices.items():
            self._params[name] = nn.Parameter(self.flat[o:o + n].view(shape))
        self.model.embed_tokens = _Holder(self._params["model.embed_tokens.weight"])
        for l in range(d.num_hidden_layers):
            p = f"model.layers.{l}."
            lay = nn.Module()
            lay.self_attn = nn.Module()
            for nm in ("q_proj", "k_proj", "v_proj", "o_proj", "q_norm", "k_norm"):
                setattr(lay.self_attn, nm, _Holder(self._params[p + f"self_attn.{nm}.weight"]))
            lay.mlp = nn.Module()
            for nm in ("gate_proj", "up_proj", "down_proj"):
                setattr(lay.mlp, nm, _Holder(self._params[p + f"mlp.{nm}.weight"]))
            lay.input_layernorm = _Holder(self._params[p + "input_layernorm.weight"])
            lay.post_attention_layernorm = _Holder(self._params[p + "post_attention_layernorm.weight"])
            self.model.layers.append(lay)
        self.model.norm = _Holder(self._params["model.norm.weight"])
        self.lm_head = _Holder(self._params["model.embed_tokens.weight"] if d.tie_word_embeddings
                               else self._params["lm_head.weight"])
        self._anchor = torch.zeros((), device=dev, requires_grad=True)
        self._rope = {}
        self._cdims = _lib.Dims(d.vocab_size, h, I, d.num_hidden_layers, d.num_attention_heads, d.num_key_value_heads,
                                d.head_dim, int(d.tie_word_embeddings), d.rms_norm_eps, 0)
        self._cparams, self._clayers = self._c_struct(self.flat)
        self._cgrads = None
        self._stage_cb = None  # python callable(stage) set by the data-parallel wrapper
        self.overlap_dw = True
        self._side_stream = None
        # The attention kernels take a valid-prefix length per sequence, i.e. RIGHT padding -- what the collator emits
        # (data.py:280-327).  ``forward`` checks the mask for that (one host read); a caller that has already checked
        # (DistillationTrainer folds it into the row-count read it needs anyway) passes ``padding_checked=True``.
        self.validate_padding = True
        # A FROZEN model (the teacher: train.py:165-169) runs its inference forward with every decoder layer's RMSNorm
        # gains folded into the q|k|v / gate|up weights (SD_SAVE_NONE_FOLDED: 1 instead of 2L+1 norm launches per pass);
        # the folded copies are rebuilt whenever the flat parameter buffer has been written to (version counter).
        self.fold_norm_gains = True
        self._folded = None  # (flat._version, folded weight buffer, Params, Layers)
        # Opt-in inference precision of a FROZEN model (set_inference_precision): "mxfp8" runs the four projections of
        # every decoder layer as MXFP8 x MXFP8 GEMMs on weights quantised once (sd_qwen3_forward_mx).
        self.inference_precision = "bf16"
        self._mx = None      # (ParamsMx, LayerMx array, the quantised weight tensors they point into)
        self._lora = None    # lora.LoraState once lora.get_lora_model() has attached an adapter (train.py:180-202)
        # Stage-1 alignment (stage1.freeze_model_weights, reference stage1.py:29-73): the first vocabulary row whose
        # embedding / lm_head gradient is kept.  None = normal training (every gradient, labels ignored by forward).
        self.stage1_row_lo = None
        if init_std:
            self.init_weights(seed, init_std)

    # ------------------------------------------------------------------------------- construction
    def _apply(self, fn, recurse=True):
        """``.to(device)`` / ``.cuda()`` (HF Trainer moves the model to ``args.device``): move the FLAT buffers and
        re-point the HF-named parameters at them, so they stay views of one buffer.  Other dtypes are refused."""
        self._mx = None  # the quantised teacher weights live on the old device / belong to the old buffer
        new_flat = fn(self.flat)
        if new_flat.dtype != torch.bfloat16:
            raise TypeError("HipQwen3ForCausalLM holds bf16 parameters (train.py:174 loads the student in bf16)")
        if new_flat.device == self.flat.device:
            return self
        self.flat = new_flat
        for name, (o, n, shape) in self._slices.items():
            self._params[name].data = new_flat[o:o + n].view(shape)
        if self.flat_grad is not None:
            self.flat_grad = fn(self.flat_grad)
            self._cgrads, self._cglayers = self._c_struct(self.flat_grad)
            if self._grads_live:
                for name, (o, n, shape) in self._slices.items():
                    self._params[name].grad = self.flat_grad[o:o + n].view(shape)
        self._anchor = torch.zeros((), device=new_flat.device, requires_grad=True)
        self._cparams, self._clayers = self._c_struct(self.flat)
        self._rope, self._side_stream = {}, None
        if self._lora is not None:
            self._lora.rebind(fn)
        return self

    @staticmethod
    def _hf_config(d):
        try:
            from transformers import Qwen3Config
            return Qwen3Config(vocab_size=d.vocab_size, hidden_size=d.hidden_size, intermediate_size=d.intermediate_size,
                               num_hidden_layers=d.num_hidden_layers, num_attention_heads=d.num_attention_heads,
                               num_key_value_heads=d.num_key_value_heads, head_dim=d.head_dim,
                               rms_norm_eps=d.rms_norm_eps, rope_theta=d.rope_theta,
                               tie_word_embeddings=d.tie_word_embeddings, attention_bias=False)
        except Exception:  # transformers absent / different signature: the config is informational only
            return d

    def _c_struct(self, flat):
        d = self.dims
        base = flat.data_ptr()

        def ptr(name):
            return base + self._slices[name][0] * 2
        layers = (_lib.Layer * d.num_hidden_layers)()
        for l in range(d.num_hidden_layers):
            p = f"model.layers.{l}."
            layers[l].wqkv = ptr(p + "self_attn.q_proj.weight")
            layers[l].wo = ptr(p + "self_attn.o_proj.weight")
            layers[l].wgu = ptr(p + "mlp.gate_proj.weight")
            layers[l].wdown = ptr(p + "mlp.down_proj.weight")
            layers[l].q_gain = ptr(p + "self_attn.q_norm.weight")
            layers[l].k_gain = ptr(p + "self_attn.k_norm.weight")
            layers[l].ln1 = ptr(p + "input_layernorm.weight")
            layers[l].ln2 = ptr(p + "post_attention_layernorm.weight")
        params = _lib.Params()
        params.embed = ptr("model.embed_tokens.weight")
        params.lm_head = params.embed if d.tie_word_embeddings else ptr("lm_head.weight")
        params.final_norm = ptr("model.norm.weight")
        params.layers_host = C.cast(layers, C.POINTER(_lib.Layer))
        return params, layers

    @torch.no_grad()
    def init_weights(self, seed=0, std=0.02):
        """HF default init: N(0, std) matrices, unit norm gains; one CPU generator -> same on every rank."""
        self._mx = None
        g = torch.Generator().manual_seed(seed)
        for name, p in self._params.items():
            if p.dim() == 1:
                p.fill_(1.0)
            else:
                chunk = 1 << 24
                flat = p.view(-1)
                for s in range(0, flat.numel(), chunk):
                    n = min(chunk, flat.numel() - s)
                    flat[s:s + n].copy_((torch.randn(n, generator=g) * std).to(torch.bfloat16))

    @torch.no_grad()
    def load_hf_state_dict(self, sd):
        """Copy tensors from a dict with HF key names (fp32 or bf16, any device)."""
        self._mx = None
        for name, p in self._params.items():
            if name == "lm_head.weight" and name not in sd:
                continue
            p.copy_(sd[name].to(torch.bfloat16))

    # ------------------------------------------------------------------------------ checkpointing
    # The reference checkpoints through HF Trainer (save_strategy="epoch", load_best_model_at_end=True,
    # save_total_limit=3: train.py:341-345), i.e. ``save_pretrained`` of an HF Qwen3ForCausalLM: a directory with
    # ``config.json`` + ``model.safetensors`` whose keys are the HF names and which does NOT hold ``lm_head.weight``
    # when the head is tied (HF drops ``_tied_weights_keys``).  The same directory is written and read here.
    _tied_weights_keys = {"lm_head.weight": "model.embed_tokens.weight"}

    def _tied_head_key(self, prefix=""):
        return prefix + "lm_head.weight" if self.dims.tie_word_embeddings else None

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        """HF key names -> tensors (views of the flat buffer).  A tied ``lm_head.weight`` is left out, as in an HF
        checkpoint: it is the same memory as ``model.embed_tokens.weight`` and safetensors refuses aliases."""
        if self._lora is not None:   # a LoRA student checkpoints its adapter (peft's adapter state dict), lora.py
            return self._lora.state_dict(prefix)
        sd = super().state_dict(*args, destination=destination, prefix=prefix, keep_vars=keep_vars)
        tied = self._tied_head_key(prefix)
        if tied is not None:
            sd.pop(tied, None)
        return sd

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Copy HF-named tensors (any float dtype / device) into the flat buffer.  Returns torch's
        ``_IncompatibleKeys``; a tied ``lm_head.weight`` is neither required nor, when present, unexpected
        (it must then equal the embedding, which is what gets loaded)."""
        from torch.nn.modules.module import _IncompatibleKeys
        self._mx = None
        if self._lora is not None:
            return self._lora.load_state_dict(state_dict, strict)
        tied = self._tied_head_key()
        want = [k for k in self._params if k != tied] if tied else list(self._params)
        if tied and "lm_head.weight" in self._params:
            want = [k for k in want if k != "lm_head.weight"]
        missing = [k for k in want if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._params and k != tied]
        bad = [k for k in want if k in state_dict and tuple(state_dict[k].shape) != tuple(self._params[k].shape)]
        if bad:
            raise RuntimeError("size mismatch for " + ", ".join(
                f"{k}: checkpoint {tuple(state_dict[k].shape)} vs model {tuple(self._params[k].shape)}" for k in bad))
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing {missing}, "
                               f"unexpected {unexpected}")
        with torch.no_grad():
            for k in want:
                if k in state_dict:
                    self._params[k].copy_(state_dict[k])
        return _IncompatibleKeys(missing, unexpected)

    def save_pretrained(self, save_directory, state_dict=None, safe_serialization=True, **kwargs):
        """HF-loadable checkpoint directory: ``config.json`` (+ ``model.safetensors`` / ``pytorch_model.bin``).
        ``AutoModelForCausalLM.from_pretrained(dir)`` and ``HipQwen3ForCausalLM.from_pretrained(dir)`` both read it."""
        if self._lora is not None:   # adapter_config.json + adapter_model.safetensors, as PeftModel.save_pretrained
            return self._lora.save_pretrained(save_directory, state_dict, safe_serialization)
        os.makedirs(save_directory, exist_ok=True)
        sd = self.state_dict() if state_dict is None else dict(state_dict)
        tied = self._tied_head_key()
        if tied:
            sd.pop(tied, None)
        sd = {k: v.detach().contiguous() for k, v in sd.items()}
        if hasattr(self.config, "save_pretrained"):
            if getattr(self.config, "architectures", None) is None:
                self.config.architectures = ["Qwen3ForCausalLM"]
            self.config.save_pretrained(save_directory)
        if safe_serialization:
            from safetensors.torch import save_file
            save_file(sd, os.path.join(save_directory, "model.safetensors"), metadata={"format": "pt"})
        else:
            torch.save(sd, os.path.join(save_directory, "pytorch_model.bin"))

    @classmethod
    def from_pretrained(cls, directory, device="cuda", **kwargs):
        """Build from an HF checkpoint directory (what ``save_pretrained`` above or HF itself wrote); local only."""
        import json
        from transformers import AutoConfig
        c = AutoConfig.from_pretrained(directory)
        dims = Qwen3Dims.from_hf_config(c)
        m = cls(dims, device=device, config=c, init_std=0)
        st = os.path.join(directory, "model.safetensors")
        idx = os.path.join(directory, "model.safetensors.index.json")
        if os.path.isfile(st):
            from safetensors.torch import load_file
            m.load_state_dict(load_file(st, device="cpu"))
        elif os.path.isfile(idx):
            from safetensors.torch import load_file
            files = sorted(set(json.load(open(idx))["weight_map"].values()))
            sd = {}
            for f in files:
                sd.update(load_file(os.path.join(directory, f), device="cpu"))
            m.load_state_dict(sd)
        else:
            m.load_state_dict(torch.load(os.path.join(directory, "pytorch_model.bin"), map_location="cpu",
                                         weights_only=True))
        return m

    # ------------------------------------------------------------------ HF/Trainer protocol no-ops
    def train(self, mode: bool = True):
        """``nn.Module.train`` walks every submodule; the ~400 HF-named ones here only hold parameter views, and HF's
        ``training_step`` calls ``model.train()`` on every micro-step (1.4 ms of host time with the GPU idle)."""
        self.training = mode
        return self

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None, **_):
        """train.py:204-208 / TrainingArguments(gradient_checkpointing=True) (train.py:340), on by default in the reference.

        Checkpointing trades a second forward of every decoder layer for activation memory.  The runner implements it
        at the same granularity as HF (one decoder layer: only the residual stream entering each layer is kept,
        ``SD_SAVE_LAYER_INPUTS``), with bit-identical gradients, but WHEN it recomputes is a memory policy, chosen by
        ``gradient_checkpointing_kwargs={"recompute": ...}`` (or the environment variable ``SD_RECOMPUTE``):

        * ``"auto"`` (default): recompute only when keeping every activation of this batch would take more than
          ``recompute_fraction`` (default 0.25) of the device's memory -- never at the reference's shapes on 288 GB
          (2.6 GB at B=4,T=512; 10.4 GB at B=4,T=2048), so the default path pays nothing for the flag;
        * ``"always"``: what the flag means on a 24-80 GB card (+1 student forward per step, activations / ~9);
        * ``"never"``.
        """
        kw = dict(gradient_checkpointing_kwargs or {})
        # a later call without the key (HF Trainer calls this again with its own kwargs) keeps an earlier choice
        policy = kw.get("recompute") or os.environ.get("SD_RECOMPUTE") or self.recompute_policy
        if policy not in ("auto", "always", "never"):
            raise ValueError(f"recompute policy {policy!r}: expected 'auto', 'always' or 'never'")
        self.recompute_policy = policy
        self.recompute_fraction = float(kw.get("recompute_fraction", self.recompute_fraction))
        self.gradient_checkpointing = True

    def gradient_checkpointing_disable(self):
        self.gradient_checkpointing = False

    @property
    def is_gradient_checkpointing(self):
        return self.gradient_checkpointing

    def _wants_recompute(self, B, T, device):
        if not self.gradient_checkpointing or self.recompute_policy == "never":
            return False
        if self.recompute_policy == "always":
            return True
        full = load_lib().sd_qwen3_acts_bytes(C.byref(self._cdims), B, T, SAVE_ALL)
        return full > self.recompute_fraction * torch.cuda.get_device_properties(device).total_memory

    def enable_input_require_grads(self):
        pass

    def get_input_embeddings(self):
        return self.model.embed_tokens

    # --------------------------------------------------------------------------------- execution
    def _tables(self, T, device):
        key = (T, str(device))
        if key not in self._rope:
            self._rope[key] = rope_tables(T, device, self.dims.rope_theta)
        return self._rope[key]

    def _packed(self, ids, position_ids, cu_seq_lens_q=None, cu_seq_lens_k=None):
        """PackedBatch of a packed call (HF padding-free packing): the segments come from ``cu_seq_lens_q`` when given
        (it must then equal ``cu_seq_lens_k``), else from ``position_ids`` by HF's rule (``ops.packed_segments``); ``B > 1``
        rows are flattened.  RoPE uses the given positions, which need not start at 0.  Everything is checked before any
        launch, on one host read."""
        from .ops import packed_segments
        pos = position_ids.to(ids.device)
        if pos.dtype not in (torch.int32, torch.int64) or tuple(pos.shape) != tuple(ids.shape):
            raise ValueError(f"position_ids must be an integer tensor shaped like input_ids {tuple(ids.shape)}, "
                             f"got {pos.dtype} {tuple(pos.shape)}")
        M = ids.numel()
        if cu_seq_lens_q is not None:
            cu = cu_seq_lens_q
            if cu_seq_lens_k is not None and (cu_seq_lens_k.shape != cu.shape or
                                              not torch.equal(cu_seq_lens_k.to(cu.device), cu)):
                raise ValueError("cu_seq_lens_k differs from cu_seq_lens_q: packed causal attention takes one set of segments")
            if cu.dtype not in (torch.int32, torch.int64) or cu.dim() != 1 or cu.numel() < 2:
                raise ValueError(f"cu_seq_lens_q must be a 1-D int32 tensor of n_seqs + 1 offsets, got {cu.dtype} "
                                 f"{tuple(cu.shape)}")
            host = torch.cat([cu.to(device=pos.device, dtype=torch.int64), pos.max().reshape(1).to(torch.int64),
                              pos.min().reshape(1).to(torch.int64)]).cpu()
            cu_host, pmax, pmin = host[:-2], int(host[-2]), int(host[-1])
            if int(cu_host[0]) != 0 or int(cu_host[-1]) != M or bool((cu_host[1:] < cu_host[:-1]).any()):
                raise ValueError(f"cu_seq_lens_q must rise from 0 to the token count {M}, got {cu_host.tolist()[:8]}...")
        else:
            cu_host, pmax, pmin = packed_segments(pos)
        if pmin < 0:
            raise ValueError("position_ids must be non-negative")
        n = 64
        while n <= pmax:
            n *= 2
        cos, sin = self._tables(n, ids.device)
        flat = pos.reshape(-1).to(torch.int64)
        return PackedBatch(cu_host, cos[flat].contiguous(), sin[flat].contiguous(), ids.device, self.dims.rope_theta)

    def packed_batch(self, cu_seqlens, position_ids, max_seqlen, max_pos):
        """The PackedBatch ``_packed`` would build, from numbers the caller has already read and checked
        (``ops.packed_rows``: ``cu_seqlens`` rises from 0 to ``position_ids.numel()``, its longest document is
        ``max_seqlen``, the positions lie in [0, ``max_pos``]): no host read, same tables, same bits.  Pass it to
        ``forward(..., packed_batch=)``; a model of the same ``head_dim`` and ``rope_theta`` can share it."""
        dev = self.flat.device
        n = 64
        while n <= max_pos:
            n *= 2
        cos, sin = self._tables(n, dev)
        flat = position_ids.to(device=dev, dtype=torch.int64).reshape(-1)
        cu = cu_seqlens.to(device=dev, dtype=torch.int32)
        return PackedBatch.from_device(cu, flat.numel(), cu.numel() - 1, max_seqlen, cos[flat].contiguous(),
                                       sin[flat].contiguous(), self.dims.rope_theta)

    def shares_packed_batch(self, other):
        """Whether a PackedBatch built by ``other`` carries this model's RoPE rows too."""
        return self.dims.head_dim == other.dims.head_dim and self.dims.rope_theta == other.dims.rope_theta

    def _fold_layer(self, l):
        """bf16(W diag(g)) of layer l's q|k|v and gate|up projections, g = the RMSNorm gain in front of each."""
        d, p = self.dims, f"model.layers.{l}."
        h = d.hidden_size
        out = []
        for first, n, gain in (("self_attn.q_proj", (d.q_dim + 2 * d.kv_dim) * h, "input_layernorm"),
                               ("mlp.gate_proj", 2 * d.intermediate_size * h, "post_attention_layernorm")):
            o = self._slices[p + first + ".weight"][0]
            w = self.flat[o:o + n].view(-1, h)   # q | k | v (gate | up) rows are contiguous in the flat layout
            out.append((w.float() * self._params[p + gain + ".weight"].float()[None, :]).to(torch.bfloat16))
        return out

    @torch.no_grad()
    def _folded_params(self):
        """C parameter struct whose wqkv / wgu point at W diag(g) (g = the RMSNorm gain in front of the projection,
        HF:59-64, 252-254, 81-83), or None when this model must not or cannot fold."""
        if not self.fold_norm_gains or self._lora is not None or any(p.requires_grad for p in self._params.values()):
            return None
        if not load_lib().sd_qwen3_fold_supported(C.byref(self._cdims)):
            return None
        ver = self.flat._version
        if self._folded is not None and self._folded[0] == ver and self._folded[1].device == self.flat.device:
            return self._folded[2]
        d = self.dims
        h, I = d.hidden_size, d.intermediate_size
        nq, ng = (d.q_dim + 2 * d.kv_dim) * h, 2 * I * h
        buf = torch.empty(d.num_hidden_layers * (nq + ng), dtype=torch.bfloat16, device=self.flat.device)
        params, layers = self._c_struct(self.flat)
        for l in range(d.num_hidden_layers):
            base = l * (nq + ng)
            fq, fg = self._fold_layer(l)
            buf[base:base + nq].copy_(fq.view(-1))
            buf[base + nq:base + nq + ng].copy_(fg.view(-1))
            layers[l].wqkv = buf.data_ptr() + base * 2
            layers[l].wgu = buf.data_ptr() + (base + nq) * 2
        self._folded = (ver, buf, params, layers)
        return params

    # ------------------------------------------------------------------------- MXFP8 inference (frozen teacher)
    def _check_mx(self):
        if self._lora is not None:
            raise ValueError('inference precision "mxfp8" is for a frozen model; this one carries a LoRA adapter')
        if any(p.requires_grad for p in self._params.values()):
            raise ValueError('inference precision "mxfp8" is for a frozen model (call requires_grad_(False) first): '
                             "its weights are quantised once, trainable parameters would go stale")
        if not load_lib().sd_qwen3_mx_supported(C.byref(self._cdims)):
            raise ValueError('inference precision "mxfp8" needs head_dim 128 and hidden_size, intermediate_size multiples '
                             f"of 128 (got hidden {self.dims.hidden_size}, intermediate {self.dims.intermediate_size})")

    def set_inference_precision(self, precision):
        """"bf16" (default) or "mxfp8": how the no-grad forward of this FROZEN model runs its decoder projections.
        "mxfp8" (the teacher's 8-bit mode of this build; a different format from bitsandbytes' LLM.int8()): q|k|v, o,
        gate|up and down run as MXFP8 x MXFP8 -> fp32 GEMMs (OCP Microscaling FP8: e4m3 elements, one power-of-two scale per
        32 along K) on weights quantised once; the residual stream, attention, q/k-norm + RoPE, the final norm, the
        embedding and the lm_head stay bf16.  The quantised weights are dropped by ``.to()``, ``load_state_dict``,
        ``load_hf_state_dict``, ``init_weights`` and this call; a frozen model's parameters are not expected to be written
        any other way."""
        if precision not in ("bf16", "mxfp8"):
            raise ValueError(f'inference precision must be "bf16" or "mxfp8", got {precision!r}')
        if precision == "mxfp8":
            self._check_mx()
        self.inference_precision = precision
        self._mx = None
        return self

    @torch.no_grad()
    def _mx_params(self):
        """sd_qwen3_params_mx of this model: per layer bf16(W diag(g)) exactly as ``_folded_params`` folds, then
        sd_mxfp8_quant; built once and kept until invalidated."""
        self._check_mx()
        if self._mx is not None and self._mx[2][0].device == self.flat.device:
            return self._mx[0]
        from . import ops
        d = self.dims
        keep = []
        layers = (_lib.LayerMx * d.num_hidden_layers)()
        base = self.flat.data_ptr()

        def quant(t):
            q, s = ops.mxfp8_quant(t)
            keep.extend((q, s))
            return q.data_ptr(), s.data_ptr()
        for l in range(d.num_hidden_layers):
            p = f"model.layers.{l}."
            fq, fg = self._fold_layer(l)
            layers[l].wqkv_q, layers[l].wqkv_scale = quant(fq)
            layers[l].wgu_q, layers[l].wgu_scale = quant(fg)
            layers[l].wo_q, layers[l].wo_scale = quant(self._params[p + "self_attn.o_proj.weight"].data)
            layers[l].wdown_q, layers[l].wdown_scale = quant(self._params[p + "mlp.down_proj.weight"].data)
            layers[l].q_gain = base + self._slices[p + "self_attn.q_norm.weight"][0] * 2
            layers[l].k_gain = base + self._slices[p + "self_attn.k_norm.weight"][0] * 2
        params = _lib.ParamsMx()
        params.embed, params.lm_head, params.final_norm = self._cparams.embed, self._cparams.lm_head, self._cparams.final_norm
        params.layers_host = C.cast(layers, C.POINTER(_lib.LayerMx))
        self._mx = (params, layers, keep)
        return params

    def _batch(self, input_ids, kv_len, rows, packed):
        """include/sd_hip.h sd_qwen3_batch of one call and the (B, T) that size its buffers: (1, M) for packed documents.
        Built once per forward and kept by the autograd function for the backward; ``keep`` holds what it points to."""
        B, T = input_ids.shape if packed is None else (1, packed.M)
        cos, sin = self._tables(T, input_ids.device) if packed is None else (packed.cos, packed.sin)
        b = _lib.Batch(input_ids.data_ptr(), _p(kv_len) if packed is None else 0,
                       None if packed is None else C.pointer(packed.desc), cos.data_ptr(), sin.data_ptr(), _p(rows),
                       0 if rows is None else rows.numel(), B, T, 0)
        b.keep = (input_ids, kv_len, rows, packed, cos, sin)
        return b, (B, T)

    def _run_forward(self, input_ids, kv_len, save, rows=None, concurrent=False, packed=None, batch=None):
        lib = load_lib()
        if batch is None:
            batch, _ = self._batch(input_ids, kv_len, rows, packed)
        dev = input_ids.device
        shape = input_ids.shape if rows is None else (rows.numel(),)
        logits = torch.empty(*shape, self.dims.vocab_size, dtype=torch.bfloat16, device=dev)
        mode = FWD_CONCURRENT if concurrent else 0
        if save == SAVE_NONE and self.inference_precision == "mxfp8":
            nbytes = lib.sd_qwen3_mx_acts_bytes(C.byref(self._cdims), batch.B, batch.T)
            acts = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(lib.sd_qwen3_forward_mx(C.byref(self._cdims), C.byref(self._mx_params()), C.byref(batch), acts.data_ptr(),
                                          nbytes, logits.data_ptr(), mode, _stream()), "sd_qwen3_forward_mx")
            return logits, acts
        cparams = self._cparams
        if self._lora is not None:
            self._lora.ensure_merged()   # W_eff = W_res + s B A, rebuilt only after A / B have changed
        if save == SAVE_NONE:
            folded = self._folded_params()
            if folded is not None:
                cparams, save = folded, SAVE_NONE_FOLDED
        nbytes = lib.sd_qwen3_acts_bytes(C.byref(self._cdims), batch.B, batch.T, int(save))
        acts = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(lib.sd_qwen3_forward(C.byref(self._cdims), C.byref(cparams), C.byref(batch), acts.data_ptr(), nbytes,
                                   logits.data_ptr(), int(save) | mode, _stream()), "sd_qwen3_forward")
        return logits, acts

    def _ensure_grads(self):
        """Attach HF-named .grad views of the flat gradient buffer; returns accumulate flag."""
        if self.flat_grad is None:
            self.flat_grad = torch.zeros_like(self.flat)
            self._cgrads, self._cglayers = self._c_struct(self.flat_grad)
        first = next((p for p in self._params.values() if p.requires_grad), None)
        # (optimizer.zero_grad(set_to_none=True) clears .grad without going through zero_grad() below)
        accumulate = self._grads_live and (first is None or first.grad is not None)
        if not accumulate:
            for name, (o, n, shape) in self._slices.items():
                if self._params[name].requires_grad:  # (a LoRA student's frozen base: the buffer still receives dW)
                    self._params[name].grad = self.flat_grad[o:o + n].view(shape)
            self._grads_live = True
        return accumulate

    def check_stage1(self):
        """Stage-1 mode trains the embedding (and an untied lm_head) only: anything else trainable is an inconsistent freeze."""
        heads = {"model.embed_tokens.weight", "lm_head.weight"}
        bad = sorted(n for n, p in self._params.items() if p.requires_grad and n not in heads)
        if bad or self._lora is not None:
            raise ValueError("Stage-1 mode (stage1_row_lo set by freeze_model_weights) trains only the embedding rows of the "
                             "new tokens, but " + (f"{len(bad)} body parameters are trainable (e.g. {bad[0]})" if bad else
                                                   "a LoRA adapter is attached") +
                             "; call freeze_model_weights again or set model.stage1_row_lo = None")
        if not 0 <= int(self.stage1_row_lo) <= self.dims.vocab_size:
            raise ValueError(f"stage1_row_lo {self.stage1_row_lo} outside [0, {self.dims.vocab_size}]")

    def _run_backward(self, input_ids, kv_len, acts, dlogits, rows=None, recompute=False, packed=None, batch=None):
        """sd_qwen3_backward.  Stage-1 (``stage1_row_lo`` set): SD_BWD_EMBED_ONLY, the dX chain only and the gradient rows
        [stage1_row_lo, V) of embed_tokens (+ lm_head).  ``batch``: the descriptor its forward built; the autograd function
        must pass it (no host work is repeated per step), a direct caller may leave it None and it is rebuilt here."""
        lib = load_lib()
        dev = input_ids.device
        stage1 = self.stage1_row_lo is not None
        red = getattr(self, "_reducer", None)
        if stage1:
            self.check_stage1()
            if red is not None:
                raise NotImplementedError("Stage-1 alignment is single-GPU (no data-parallel gradient exchange)")
        accumulate = self._ensure_grads()
        opts = _lib.BwdOpts((BWD_ACCUMULATE if accumulate else 0) | (BWD_RECOMPUTE if recompute else 0))
        opts.side_stream = self._side_stream_ptr(dev)
        if stage1:
            opts.flags |= BWD_EMBED_ONLY
            opts.grad_row_lo = int(self.stage1_row_lo)
        elif red is not None:
            red.begin_step()
            if red.wants_split_embedding():
                # tied embedding/lm_head gradient: the dense lm_head part is all-reduced at the START of
                # backward; only the B*T rows touched by the embedding lookup are exchanged at the end
                dx0 = torch.empty(input_ids.numel(), self.dims.hidden_size, dtype=torch.bfloat16, device=dev)
                eo, en, eshape = self._slices["model.embed_tokens.weight"]
                red.set_embedding_exchange(input_ids.reshape(-1), dx0, self.flat_grad[eo:eo + en].view(eshape))
                opts.dx0_out = dx0.data_ptr()
        user_cb = self._stage_cb
        if user_cb and not stage1:
            opts.on_grads_ready = _lib.STAGE_CB(lambda stage, _u: user_cb(stage))  # (opts keeps the thunk alive)
        if not dlogits.is_contiguous():
            dlogits = dlogits.contiguous()
        if batch is None:
            batch, _ = self._batch(input_ids, kv_len, rows, packed)
        sbytes = lib.sd_qwen3_bwd_scratch_bytes(C.byref(self._cdims), batch.B, batch.T)
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        check(lib.sd_qwen3_backward(C.byref(self._cdims), C.byref(self._cparams), C.byref(self._cgrads), C.byref(batch),
                                    acts.data_ptr(), acts.numel(), dlogits.data_ptr(), scratch.data_ptr(), sbytes,
                                    C.byref(opts), _stream()), "sd_qwen3_backward")
        if red is not None:
            red.finish()
        if self._lora is not None:
            self._lora.grads_stale = True

    def finalize_grads(self):
        """Called by the optimizer / the clipping hook before they read gradients: a LoRA student projects the
        accumulated weight gradient onto its adapter (dA = s B^T dW, dB = s dW A^T) here, once per optimizer step."""
        if self._lora is not None:
            self._lora.project_grads()

    def optim_segments(self, split_decay=False):
        """What the fused optimizer updates: a list of (kind, params, grads, decays, extra) over flat buffers, in a
        fixed order.  kind "bf16": bf16 parameters / moments (sd_adamw_bf16); "f32_shadow": fp32 masters with bf16
        gradients and shadows (sd_adamw_f32_shadow; extra = (shadow, shadow_scaled, scale))."""
        g = self.flat_grad
        if self._lora is not None:
            return self._lora.optim_segments()
        if self.stage1_row_lo is not None:
            # Stage-1: the embedding (+ untied lm_head), matrices, so weight decay applies (HF's groups, stage1.py's adamw_torch)
            segs = []
            for name in ("model.embed_tokens.weight", "lm_head.weight"):
                if name in self._slices:
                    o, n, _ = self._slices[name]
                    segs.append(("bf16", self.flat[o:o + n], None if g is None else g[o:o + n], True, None))
            return segs
        if not split_decay:
            return [("bf16", self.flat, g, True, None)]
        return [("bf16", self.flat[a:b], None if g is None else g[a:b], m, None) for a, b, m in self._decay_runs()]

    def _decay_runs(self):
        """Contiguous runs of matrices / gains in the flat layout (weight decay applies to matrices only)."""
        runs, cur = [], None
        for name, (o, n, shape) in self._slices.items():
            is_mat = len(shape) == 2
            n8 = (n + 7) // 8 * 8
            if cur is not None and cur[2] == is_mat and cur[1] == o:
                cur[1] = o + n8
            else:
                cur = [o, o + n8, is_mat]
                runs.append(cur)
        return [(a, b, m) for a, b, m in runs]

    def _side_stream_ptr(self, device):
        """Second HIP stream for the weight-gradient GEMMs (they overlap the dX chain); None disables it."""
        if not self.overlap_dw:
            return None
        if self._side_stream is None:
            from . import ops
            self._side_stream = ops.concurrent_stream(device, "dw")
        return self._side_stream.cuda_stream

    def forward(self, input_ids=None, attention_mask=None, labels=None, logit_rows=None, position_ids=None, **kwargs):
        """Returns an object with ``.logits`` [B,T,V] (bf16).  ``labels`` is accepted and ignored: the
        reference leaves it in ``inputs`` at train.py:54, which only makes HF compute an unused CE.  In Stage-1 mode
        (``stage1_row_lo`` set by ``stage1.freeze_model_weights``) ``labels`` gives ``.loss`` instead: ``_forward_stage1``.
        ``logit_rows`` (int64 [R], flat b*T+t indices, unique): apply the lm_head to those rows only and return
        ``.logits`` [R,V] -- the training step passes the rows the loss reads (``ops.loss_rows``).
        ``concurrent=True`` (keyword): the caller runs another pass beside this one on a second stream (the frozen
        teacher beside the student, as DistillationTrainer does): SD_FWD_CONCURRENT, launches sized for a shared GPU.

        Packed documents (HF padding-free packing: ``DataCollatorWithFlattening``, TRL ``padding_free``), exactly when HF
        Qwen3 packs: ``position_ids`` given and ``attention_mask`` None.  The documents are the segments of
        ``cu_seq_lens_q`` (HF's ``FlashAttentionKwargs``; ``cu_seq_lens_k`` must equal it) or, without it, the runs of
        consecutive ``position_ids`` (a new document wherever ``pos[t] != pos[t-1] + 1`` and at every row start); rows of
        ``B > 1`` are flattened.  No token attends across a document boundary (varlen attention kernels) and RoPE uses the
        given positions.  With an ``attention_mask``, ``position_ids`` are ignored (positions 0..T-1 per right-padded
        row), as before.  ``packed_batch`` (keyword, a ``PackedBatch`` from ``packed_batch()``): the documents of this
        call, already read and checked by the caller; used in place of the host read above (the trainer builds one per
        micro-batch for student and teacher)."""
        ids = _need(input_ids.to(torch.int64), torch.int64, "input_ids")
        rows = None
        if logit_rows is not None:
            rows = _need(logit_rows.to(device=ids.device, dtype=torch.int64), torch.int64, "logit_rows")
            if rows.dim() != 1 or rows.numel() == 0 or rows.numel() > ids.numel():
                raise ValueError("logit_rows must be a non-empty 1-D tensor of at most B*T row indices")
        kv_len = None
        if attention_mask is not None:
            am = attention_mask.to(ids.device)
            if am.shape != ids.shape:
                raise ValueError(f"attention_mask {tuple(am.shape)} != input_ids {tuple(ids.shape)}")
            stage1_loss = self.stage1_row_lo is not None and labels is not None  # (ops.loss_rows checks the mask then)
            if (self.validate_padding and not kwargs.get("padding_checked", False) and not stage1_loss
                    and bool(left_padded(am))):
                raise ValueError("attention_mask is not right-padded (a 1 follows a 0): the HIP attention kernels take a "
                                 "valid-prefix length per sequence, as ProcessedDataCollator produces (data.py:280-327)")
            kv_len = am.sum(-1).to(torch.int32).contiguous()
        packed = kwargs.get("packed_batch")
        if packed is not None:   # the caller has read and checked the segments already (ops.packed_rows): host-side checks only
            if attention_mask is not None:
                raise ValueError("packed_batch with an attention_mask: packed documents have no padding to mask")
            if (packed.M != ids.numel() or packed.cos.size(-1) != self.dims.head_dim
                    or packed.rope_theta not in (None, self.dims.rope_theta)):
                raise ValueError(f"packed_batch was built for {packed.M} tokens, RoPE width {packed.cos.size(-1)}, theta "
                                 f"{packed.rope_theta}; this call has {ids.numel()} tokens, head_dim {self.dims.head_dim}, "
                                 f"theta {self.dims.rope_theta}")
        elif attention_mask is None and position_ids is not None:
            packed = self._packed(ids, position_ids, kwargs.get("cu_seq_lens_q"), kwargs.get("cu_seq_lens_k"))
        elif attention_mask is None and kwargs.get("cu_seq_lens_q") is not None:
            raise ValueError("cu_seq_lens_q without position_ids: packed documents need their positions (HF packs only "
                             "when position_ids is given and attention_mask is None)")
        if self.stage1_row_lo is not None and labels is not None:
            return self._forward_stage1(ids, am if attention_mask is not None else None, kv_len, labels, packed=packed,
                                        **kwargs)
        if torch.is_grad_enabled() and (self._lora is not None or any(p.requires_grad for p in self._params.values())):
            logits = _DecoderFn.apply(self._anchor, ids, kv_len, self, rows, bool(kwargs.get("concurrent", False)), packed)
        else:
            logits, _ = self._run_forward(ids, kv_len, save=SAVE_NONE, rows=rows,
                                          concurrent=bool(kwargs.get("concurrent", False)), packed=packed)
        return CausalLMOutput(logits=logits)

    def _forward_stage1(self, ids, am, kv_len, labels, num_items_in_batch=None, stage1_inplace_grad=False, packed=None,
                        **_):
        """Stage-1 loss (reference stage1.py: SFTTrainer -> HF ForCausalLMLoss): causal-LM cross-entropy over the rows whose
        next label is not -100, summed and divided by ``num_items_in_batch`` when given (else the mean).  The rows are
        selected on the GPU (``ops.loss_rows``, the one host read), the lm_head runs on those rows only, and the loss is
        sd_celoss_*_rows.  ``.logits`` is then [R,V] for the rows ``.logit_rows``.  ``stage1_inplace_grad``: the loss
        gradient overwrites those logits (the caller does not keep them)."""
        from .ops import celoss_rows, loss_rows
        self.check_stage1()
        rows, row_labels = loss_rows(labels.to(ids.device), right_padded=(am,) if am is not None else ())
        if rows.numel() == 0:  # nothing to predict: one masked row keeps every launch well-formed (loss 0, gradient 0)
            rows = torch.zeros(1, dtype=torch.int64, device=ids.device)
            row_labels = torch.full((1,), -100, dtype=torch.int64, device=ids.device)
        div = None
        if num_items_in_batch is not None:
            div = torch.as_tensor(num_items_in_batch, dtype=torch.float32).to(ids.device).reshape(1)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._params.values()):
            logits = _DecoderFn.apply(self._anchor, ids, kv_len, self, rows, False, packed)
        else:
            logits, _ = self._run_forward(ids, kv_len, save=SAVE_NONE, rows=rows, packed=packed)
        loss, _ = celoss_rows(logits, row_labels, div, inplace_grad=bool(stage1_inplace_grad))
        return CausalLMOutput(loss=loss, logits=logits, logit_rows=rows)

    def generate(self, input_ids, attention_mask=None, max_new_tokens=20, min_new_tokens=0, do_sample=True,
                 temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, eos_token_id=None, pad_token_id=None,
                 use_ras=False, win_size=25, tau_r=0.2, seed=None, sync_every=16, decode_kernels="tile",
                 weight_dtype="bf16", decode_attention="split", gemv_rows=16):
        """Decode ``max_new_tokens`` tokens per row over a KV cache (generation.py; the reference's engine:
        soulxpodcast/engine/llm_engine.py:37-76 with sampler.py:136-189).  Returns int64 [B, T + max_new_tokens]: the given
        ``input_ids`` followed by the new tokens in columns T..., ``pad_token_id`` (default: ``eos_token_id``, else 0) after
        a row's EOS.  Prompts are RIGHT-padded (``attention_mask``); row b's first new token takes position ``kv_len[b]``.

        Sampling follows HF's processor order: repetition penalty over the generated tokens, EOS suppressed for
        ``min_new_tokens``, temperature, top-k (<= 128), top-p, then an inverse-CDF draw; ``do_sample=False`` is the
        arg-max; ``use_ras`` adds repetition-aware sampling (window ``win_size``, threshold ``tau_r``).  ``top_k=0`` samples
        the whole vocabulary and allows neither ``top_p < 1`` nor ``use_ras``.  ``seed`` fixes the uniforms.  The loop runs
        under no_grad on the current stream; the host reads the finished flags once every ``sync_every`` steps, and the
        tokens do not depend on that number.  ``decode_kernels``: "tile" (default) runs the step's projections on the tile
        GEMMs; "skinny" streams the weights through the GEMV kernels for batches of up to 16 rows, with the norms and the
        SwiGLU fused in: a row's tokens then equal those of the row generated alone.  "wide" does the same for up to 64
        rows on the MFMA weight-streaming kernels (bf16 weights only; its bits are not those of "skinny").

        Raises before any launch: ValueError for another ``decode_kernels``, when T + max_new_tokens exceeds the cache
        capacity (``kv_cache_capacity`` or the config's ``max_position_embeddings``), when ``top_k > 128`` or when the mask is not right-padded;
        NotImplementedError for a model set to "mxfp8" (the decoder reads the unfolded bf16 weights; a LoRA student's merged
        weights are those); RuntimeError for CPU tensors.

        ``weight_dtype="mxfp8"`` (default "bf16"): prefill and every step run the four projections of each layer on the
        model's MXFP8 weights (``set_inference_precision``'s format, whatever the precision the model is set to); with
        "skinny" the 8-bit weights are streamed through the block-scaled GEMV.  Needs a frozen model without LoRA and
        the dimensions "mxfp8" needs: ValueError otherwise, and for any other value, before any allocation.  ValueError
        too for ``decode_kernels="wide"`` with "mxfp8": the 64-row MXFP8 step is spelled ``gemv_rows=64``.

        ``gemv_rows=64`` (default 16; only with ``decode_kernels="skinny"`` and ``weight_dtype="mxfp8"``): the steps
        stream the 8-bit weights through the 64-row block-scaled GEMV (sd_gemv_mxfp8_wide), so a row's tokens equal those
        of the row generated alone with the same keywords for batches of up to 64 rows.  ValueError, before any
        allocation, for another value, with bf16 weights (that step is ``decode_kernels="wide"``), with "tile" / "wide",
        or with ``decode_attention="fused"`` (not built).

        ``decode_attention="fused"`` (default "split"): every decode step runs each layer's cache step -- q/k-norm + RoPE,
        the append, the split-KV attention and its merge -- as one launch instead of three (sd_cache_step).  The tokens
        are those of "split", bit for bit, with every ``decode_kernels``, ``weight_dtype`` and cache kind.  ValueError for
        any other value, before any allocation."""
        from .generation import generate
        return generate(self, input_ids, attention_mask, max_new_tokens, min_new_tokens, do_sample, temperature, top_k,
                        top_p, repetition_penalty, eos_token_id, pad_token_id, use_ras, win_size, tau_r, seed, sync_every,
                        decode_kernels, weight_dtype, decode_attention, gemv_rows)

    def start_session(self, batch_size, capacity=None, decode_kernels="tile", pool=None, weight_dtype="bf16",
                      decode_attention="split", shared_kv_reads=False, gemv_rows=16):
        """A ``GenerationSession`` (generation.py): multi-turn generation over ONE live KV cache of ``capacity`` positions
        per row (default: ``cache_capacity(self)``), as the reference's dialogue loop keeps one ``DynamicCache`` across
        turns (soulxpodcast/models/soulxpodcast.py:342,378-380).  ``sess.generate(ids, mask, ...)`` takes a turn and returns
        its new tokens, ``sess.extend(ids, mask)`` appends without sampling (chunked prefill), ``sess.reset(rows)`` forgets
        rows.  With ``decode_kernels="skinny"`` only the decode steps of a turn are batch-invariant: the extend pass runs the
        tile GEMMs; "wide" is the same for up to 64 rows (bf16 weights only).  NotImplementedError for a model set to
        "mxfp8".

        ``pool`` (a ``PagePool`` of ``kv_page_pool``): the session keeps no cache buffer of its own; it owns a page table
        and takes pages of 256 positions from the pool turn by turn (paged.py; the reference's engine runs vLLM's paged
        cache, soulxpodcast/engine/llm_engine.py:91).  Several sessions may share one pool; ``sess.fork(rows)``,
        ``sess.trim()`` and ``sess.close()`` exist for such sessions.  The tokens are those of the contiguous session, bit
        for bit.  Sampling n answers to one prompt with one prefill::

            s = model.start_session(1, pool=pool); s.extend(prompt[:, :-1])
            n = s.fork([0] * 8); out = n.generate(prompt[:, -1:].expand(8, 1), ...)

        ``weight_dtype="mxfp8"``: the session decodes with the model's MXFP8 projections (see ``generate``); it combines
        with either kind of pool and with contiguous caches.  ``decode_attention="fused"``: the one-launch cache step in
        every decode step (see ``generate``); ``fork`` keeps it.

        ``shared_kv_reads=True`` (needs ``pool`` and the split cache step; ValueError otherwise): the decode steps read a
        page that several rows map once for a group of rows, with the same tokens and pool bytes.  It is meant for the
        continuations of a fork, which share the history's pages: ``s.fork([0] * 8, shared_kv_reads=True)``.

        ``gemv_rows=64`` (with "skinny" and "mxfp8"; see ``generate``): batch-invariant decode steps on the 8-bit weights
        for up to 64 rows; ``fork`` keeps it.  Not built with ``decode_attention="fused"`` or ``shared_kv_reads=True``
        (ValueError).
        """
        from .generation import GenerationSession
        return GenerationSession(self, batch_size, capacity, decode_kernels, pool=pool, weight_dtype=weight_dtype,
                                 decode_attention=decode_attention, shared_kv_reads=shared_kv_reads, gemv_rows=gemv_rows)

    def generation_engine(self, pool, max_batch=8, decode_kernels="skinny", weight_dtype="bf16", sync_every=16,
                          decode_attention="split", gemv_rows=16, admission="single"):
        """A ``GenerationEngine`` (engine.py): continuous batching over a ``PagePool`` -- requests of their own length,
        budget, seed and sampling parameters are served in ``max_batch`` rows, and a row that finishes is refilled with the
        next waiting request at once (the reference's engine is vLLM, soulxpodcast/engine/llm_engine.py:91,97-109).
        ``eng.submit(ids, max_new_tokens=..., seed=..., <generate's sampling keywords>)`` -> id, ``eng.step()``,
        ``eng.run()``, ``eng.result(id)``, ``eng.stats``, ``eng.close()``.  With ``decode_kernels="skinny"`` a request's
        tokens are, bit for bit, those of a one-row session given the same prompt, parameters and seed, whatever else is in
        flight, for ``max_batch <= 16``; ``decode_kernels="wide"`` (bf16 weights) holds the same against a one-row "wide"
        session for ``max_batch <= 64``; "tile" is accepted without that claim (its step is not batch-invariant).
        ``decode_attention="fused"``: the one-launch cache step in every decode step, same tokens (see ``generate``).
        ``gemv_rows=64`` with ("skinny", "mxfp8"): the contract holds against a one-row session with the same three
        keywords for ``max_batch <= 64``.  ``admission="batch"`` (default "single"): the requests admitted in one iteration
        share ONE prefill pass over their right-padded prompts; faster admission, without the bit contract (the tile GEMMs
        run at another M).  ``eng.forget(ids)`` and ``eng.reset_stats()`` make one engine serve run after run; every call
        reads the model's live bf16 weights."""
        from .engine import GenerationEngine
        return GenerationEngine(self, pool, max_batch, decode_kernels, weight_dtype, sync_every,
                                decode_attention=decode_attention, gemv_rows=gemv_rows, admission=admission)

    def kv_page_pool(self, n_pages, order=None, kv_dtype="bf16"):
        """A ``PagePool`` (paged.py) of ``n_pages`` pages of 256 positions for this model's paged sessions
        (``start_session(..., pool=pool)``); ``order``: an optional permutation of the page numbers, the order in which
        free pages are handed out.  One page costs ``pool.bytes_per_page`` = L * 2 * 256 * Hkv * 128 * 2 bytes.
        ``kv_dtype="mxfp8"``: 8-bit pages (e4m3 elements, one E8M0 scale byte per 32 of them; include/sd_hip.h), L * 2 *
        256 * Hkv * 132 bytes each; the sessions over such a pool quantise what they cache and attend over the quantised
        rows.  ValueError for any other ``kv_dtype``, before anything is allocated."""
        from .paged import PagePool
        return PagePool(self, n_pages, order, kv_dtype)

    def zero_grad(self, set_to_none: bool = True):
        # keep the flat buffer; the next backward overwrites (accumulate=0) instead of adding
        self._grads_live = False
        for p in self._params.values():
            p.grad = None
