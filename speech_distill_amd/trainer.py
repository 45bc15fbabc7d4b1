"""Drop-in for the reference's ``DistillationTrainer`` (train.py:24-116): same constructor keywords,
same ``compute_loss`` contract, same three logged sub-losses, the HIP kernels underneath.

Step body (train.py:43-116):  pop the teacher / extra keys  ->  student forward (labels still in the
inputs, as in the reference)  ->  pop labels  ->  teacher no-grad forward unless pre-extracted top-K is
present  ->  on-the-fly log-softmax + top-K unless the teacher is quantized or top_k <= 0  ->
DistillationLoss  ->  log {student_loss, teacher_loss, distill_loss} when
``state.global_step % args.logging_steps == 0``  ->  ``loss`` or ``(loss, outputs)``.

Beyond the reference: ``divergence`` / ``beta`` choose the distillation term (``DistillationLoss``),
and ``lmbda`` makes a share of the training micro-batches on-policy (``on_policy.py``): the student's own sampled
continuation replaces the completion before the step.  The defaults (``"forward_kl"``, ``lmbda=0``) are the reference's loop.

What makes a step fast is decided once per micro-batch, in a ``StepPlan`` (``DistillationTrainer._plan_step``, when HF fetches
the accumulation window or else in ``compute_loss``): the rows the loss reads and what the two models may skip.
"""
import os
import time
from dataclasses import dataclass
from types import MappingProxyType
from typing import NamedTuple

import torch
from transformers import Trainer

from . import ddp, on_policy, ops
from .distillation_loss import DistillationLoss
from .qwen3 import HipQwen3ForCausalLM

ON_POLICY_ROLLOUTS = ("micro_batch", "window")
ENGINE_KEYS = ("max_batch", "n_pages", "sync_every", "admission")   # of DistillationTrainer(on_policy_engine={...})
WINDOW_MAX_ROWS = 64   # the rows of the widest batch-invariant decode step (decode_kernels="wide")


class StepPlan(NamedTuple):
    """What the selection of one micro-batch produced (``DistillationTrainer._plan_step``, its only maker): which rows the
    loss reads and what each model may skip because the selection's one host read has checked it."""
    rows: object = None          # flat indices of the loss rows (None: nothing was selected, the full [B, T, V] path)
    row_labels: object = None    # the label each of them predicts
    packed: object = None        # (student's PackedBatch, teacher's) of a batch packed with cu_seq_lens_q, else None
    student_kw: object = MappingProxyType({})   # forward keywords of the student: padding_checked / packed_batch
    teacher_kw: object = MappingProxyType({})   # ... of a HipQwen3ForCausalLM teacher
    event: object = None         # after it the batch and the rows are on the device (None: planned in place)
    key: object = None           # what a stored plan is validated by: the addresses of the tensors it was made from
    full_labels: object = None   # packed by position_ids alone: the labels with -100 at every document start


@dataclass
class _Ahead:
    """What was done ahead for one micro-batch: its plan and, once enqueued, the teacher's result (``_teacher_pass``)."""
    plan: StepPlan
    teacher: tuple = None


class FlatStudentTrainer(Trainer):
    """HF Trainer plumbing shared by the trainers of a flat-buffer student (``HipQwen3ForCausalLM``): the data-parallel
    wrapper, tokens/sec in the training log, the fused optimizer and its one-reduction gradient clip, and
    ``save_pretrained`` checkpoints."""

    PACKED_KEYS = ("position_ids", "cu_seq_lens_q", "cu_seq_lens_k", "max_length_q", "max_length_k")

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        # throughput of the loop: positions (B*T of every training micro-batch, padding included -- what the kernels
        # process and what bench.py counts) seen by THIS rank; `log` turns it into whole-job tokens/sec
        self.tokens_seen = 0
        self._tps_mark = None  # (perf_counter, tokens_seen) at the previous training log
        self._hip_dp = None
        # The optimizer HF would build by default (AdamW over ~310 HF-named tensors, HF trainer.py:1778-1796) is replaced
        # by the one-launch FlatAdamW over the flat buffers when the student offers them; set False to keep HF's.
        self.fused_optimizer = True

    def _count_tokens(self, model, ids):
        """A training micro-batch's positions; the first one starts the clock of the first tokens/sec figure."""
        if model.training and ids is not None:
            self.tokens_seen += ids.numel()
            if self._tps_mark is None:
                self._tps_mark = (time.perf_counter(), self.tokens_seen - ids.numel())

    def _default_adamw(self):
        """TrainingArguments asks for HF's default AdamW (the reference passes no ``optim``, train.py:331-354)."""
        return str(getattr(self.args.optim, "value", self.args.optim)).startswith("adamw_torch")

    # ------------------------------------------------------------------------------ HF Trainer plumbing
    def _wrap_model(self, model, training=True, dataloader=None):
        """HF trainer.py:1602-1626: a model this hook leaves unwrapped goes through ``accelerator.prepare``, which under
        torchrun wraps it in torch DDP (the reference's data parallelism) and under ``bf16=True`` wraps ``forward`` to
        copy every bf16 output to fp32.  Neither fits a flat-gradient model (see ``ddp.HipDataParallel``): its
        gradients never pass autograd hooks, and its [.,V] logits are consumed as bf16 by the loss kernel.  Such a
        model is handed to the loop inside ``HipDataParallel`` instead -- the one owner of gradient averaging, with the
        ``no_sync()`` accelerate looks for on accumulation micro-batches; HF then prepares only the optimizer."""
        if isinstance(model, ddp.HipDataParallel):
            return model
        if ddp.speaks_flat_grad(model):
            if self._hip_dp is None or self._hip_dp.module is not model:
                self._hip_dp = ddp.HipDataParallel(model)
            return self._hip_dp
        return super()._wrap_model(model, training=training, dataloader=dataloader)

    def log(self, logs, *args, **kwargs):
        """train.py:107-114 logs the three sub-losses only; SURVEY section 8 f-1 asks the counterpart for tokens/sec.  HF's
        own training log (the dict with ``loss`` / ``learning_rate``, every ``logging_steps`` optimizer steps, after a
        ``.item()`` that has drained the GPU) gets ``tokens_per_second``: positions of all ranks' micro-batches since the
        previous such log over the wall time between the two."""
        if "loss" in logs and "learning_rate" in logs and self._tps_mark is not None:
            now = time.perf_counter()
            t0, n0 = self._tps_mark
            if now > t0 and self.tokens_seen > n0:
                logs = dict(logs)
                logs["tokens_per_second"] = round((self.tokens_seen - n0) * max(1, self.args.world_size) / (now - t0), 1)
            self._tps_mark = (now, self.tokens_seen)
        return super().log(logs, *args, **kwargs)

    def _clip_grad_norm(self, model):
        """HF trainer.py:2535-2539 calls ``clip_grad_norm_`` over ~310 parameter tensors (10 ms of host time per
        optimizer step with the GPU idle).  With the flat buffers the norm is one reduction, and FlatAdamW folds the
        clip coefficient into its update; the returned pre-clip norm is the same number HF logs as ``grad_norm``."""
        core = ddp.unwrap(model)
        opt = getattr(self.optimizer, "optimizer", self.optimizer)
        if isinstance(core, HipQwen3ForCausalLM) and core.flat_grad is not None and core.flat_grad.is_cuda:
            from .optim import FlatAdamW
            if isinstance(opt, FlatAdamW) and opt.model is core:
                return opt.grad_norm(self.args.max_grad_norm)
            core.finalize_grads()
            ss = torch.zeros(1, dtype=torch.float32, device=core.flat_grad.device)
            ops.sumsq(core.flat_grad, ss)
            norm = ss.sqrt().squeeze(0)
            core.flat_grad.mul_((self.args.max_grad_norm / (norm + 1e-6)).clamp(max=1.0).to(core.flat_grad.dtype))
            return norm
        return super()._clip_grad_norm(model)

    def _save(self, output_dir=None, state_dict=None):
        """HF trainer.py `_save`: a model that is not a PreTrainedModel gets a bare ``model.safetensors``.  The
        reference's checkpoints (save_strategy="epoch", train.py:341-345) are ``save_pretrained`` directories
        (``config.json`` + weights, tied head left out) -- write the same for a model that offers it."""
        core = ddp.unwrap(self.model)
        if not hasattr(core, "save_pretrained") or isinstance(core, _pretrained_types()):
            return super()._save(output_dir, state_dict)
        output_dir = output_dir if output_dir is not None else self.args.output_dir
        os.makedirs(output_dir, exist_ok=True)
        core.save_pretrained(output_dir, state_dict=state_dict)
        if self.processing_class is not None and hasattr(self.processing_class, "save_pretrained"):
            self.processing_class.save_pretrained(output_dir)
        torch.save(self.args, os.path.join(output_dir, "training_args.bin"))

    def _flat_adamw(self, core):
        """FlatAdamW over ``core.optim_segments()`` with the TrainingArguments' AdamW hyper-parameters."""
        from .optim import FlatAdamW
        return FlatAdamW(core, lr=self.args.learning_rate, betas=(self.args.adam_beta1, self.args.adam_beta2),
                         eps=self.args.adam_epsilon, weight_decay=self.args.weight_decay)


class DistillationTrainer(FlatStudentTrainer):
    """``divergence`` ("forward_kl", "reverse_kl", "jsd") and ``beta``: see ``DistillationLoss``; anything but
    "forward_kl" needs the dense teacher (``top_k <= 0`` or ``is_quantized_teacher``) and refuses batches that carry
    pre-extracted ``teacher_top_k_v``.  ``"jsd_topk"`` is the "jsd" against a top-K teacher and runs wherever the forward KL
    does: a live teacher with ``top_k > 0`` (refused at construction otherwise, or with a quantised teacher), or batches
    that carry pre-extracted ``teacher_top_k_v`` / ``teacher_top_k_i``, with or without a teacher model.
    ``"forward_kl_tail"``, ``"reverse_kl_tail"`` and ``"jsd_tail"`` (a top-K teacher with a tail bucket) run in the same
    places: the live teacher's pass also returns its tail mass at the loss temperature (``ops.topk_tail`` on the logits it
    already holds), which travels with the top-K through every lookahead; a batch with pre-extracted keys brings
    ``teacher_top_k_tail`` (or, at temperature 1, the stored log-probs imply it).  They are finite on a top-K teacher, so
    ``lmbda > 0`` runs with the default ``top_k``.

    ``lmbda`` in [0, 1]: the probability that a training micro-batch is made on-policy -- one draw per micro-batch from a
    CPU generator seeded from ``args.seed`` and the process index; below ``lmbda`` the student generates from the batch's
    prompts with the ``generate`` keywords of ``on_policy_generate`` (``on_policy.GENERATE_KEYS``, at least
    ``max_new_tokens``) and ``on_policy.rollout`` rebuilds the batch around its tokens.  Needs a ``HipQwen3ForCausalLM``
    student on the GPU without LoRA and a teacher model.  With ``lmbda > 0`` the three lookaheads (loss rows ahead, teacher
    ahead, window ahead) are switched off: they would select rows of, and run the teacher on, a batch that is about to be
    replaced.  ``on_policy_fraction`` (the share of on-policy micro-batches since the previous log) is logged next to the
    three sub-losses.

    ``on_policy_rollout``: "micro_batch" (default) is the above, one ``generate`` per drawn micro-batch inside
    ``training_step``.  "window"  draws for every micro-batch of an accumulation window when HF
    fetches the window (``get_batch_samples``; same generator, same stream of draws) and rolls all the drawn ones out in
    ONE run of a ``GenerationEngine`` that lives as long as the trainer: one request per row with the row's own width as
    its budget and ``on_policy.request_seed`` as its seed, rows refilled as requests stop.  The weights do not change
    inside a window, so this is exactly as on-policy as the micro-batch loop.  ``on_policy_engine``: a dict of
    ``max_batch`` (default: ``per_device_train_batch_size * gradient_accumulation_steps``, at most 64), ``n_pages``
    (default: ``max_batch`` rows' worst case at the window's width plus the parking page), ``sync_every`` (16) and
    ``admission`` ("single" / "batch", see ``GenerationEngine``).  ``decode_kernels`` comes from ``on_policy_generate``.
    Refused at construction (ValueError): a LoRA student, a ``padding_free`` collator (packed batches are refused again
    when they arrive), a missing teacher, "skinny" with ``max_batch > 16`` (use "wide"), ``WORLD_SIZE > 1``.  With
    ``lmbda = 0`` the keyword is inert.  The rollouts happen inside HF's loop: a ``training_step`` called by hand in
    window mode trains on the batch it is given.

    Packed batches (``ProcessedDataCollator(padding_free=True)``; a batch is packed by its keys: ``position_ids`` present
    and ``attention_mask`` absent): ``ops.packed_rows`` selects the loss rows inside each document and checks the segments
    in the step's one host read, one ``PackedBatch`` descriptor serves student and teacher, and the teacher is called with
    the packed keys.  The three lookaheads work as on padded batches.  Refused: ``lmbda > 0``, teacher ids of another
    shape, and a packed batch that also carries an attention mask."""

    def __init__(self, *args, teacher_model=None, temperature=2.0, alpha=0.5, top_k=100, is_quantized_teacher=False,
                 divergence="forward_kl", beta=0.5, lmbda=0.0, on_policy_generate=None, on_policy_rollout="micro_batch",
                 on_policy_engine=None, **kwargs):
        # everything that can be refused without a model is refused before HF's constructor touches one
        ops.check_divergence(divergence, beta)
        if ops.takes_topk_teacher(divergence) and (top_k <= 0 or is_quantized_teacher):
            raise ValueError(f"divergence={divergence!r} needs a top-K teacher (top_k > 0, not a quantised teacher), got "
                             f"top_k={top_k}, is_quantized_teacher={is_quantized_teacher}: the dense teacher "
                             f"distribution goes with divergence={ops.dense_name(divergence)!r}")
        if ops.takes_dense_teacher(divergence) and not (top_k <= 0 or is_quantized_teacher):
            raise ValueError(f"divergence={divergence!r} needs the dense teacher distribution: pass top_k=0 (a top-K "
                             f"teacher defines it on K entries only), got top_k={top_k}")
        if not 0.0 <= float(lmbda) <= 1.0:
            raise ValueError(f"lmbda must lie in [0, 1], got {lmbda!r}")
        if lmbda > 0:
            on_policy.check_generate_kwargs(on_policy_generate)
            if teacher_model is None:
                raise ValueError("lmbda > 0 needs a teacher model: on-policy tokens have no pre-extracted teacher logits")
        if on_policy_rollout not in ON_POLICY_ROLLOUTS:
            raise ValueError(f"on_policy_rollout must be one of {ON_POLICY_ROLLOUTS}, got {on_policy_rollout!r}")
        engine_cfg = self._check_engine_config(on_policy_engine)
        if on_policy_rollout == "window" and lmbda > 0:   # (with lmbda = 0 the mode is inert: nothing is checked or built)
            engine_cfg = self._window_plan(kwargs.get("model", args[0] if args else None),
                                           kwargs.get("args", args[1] if len(args) > 1 else None),
                                           kwargs.get("data_collator", args[2] if len(args) > 2 else None),
                                           on_policy_generate, engine_cfg)
        super().__init__(*args, **kwargs)
        self.on_policy_rollout = on_policy_rollout
        self.on_policy_engine = engine_cfg     # "window" with lmbda > 0: max_batch, sync_every and admission resolved
        self._engine, self._engine_pool, self._engine_pages = None, None, 0   # built at the first window (_window_engine)
        self.engines_built = 0
        self._window_draws = []   # "window": the draws of the fetched window's micro-batches that training_step has not taken yet
        self.teacher_model = teacher_model
        if self.teacher_model is not None:
            self.teacher_model.eval()
        self.top_k = top_k
        self.distill_loss_fn = DistillationLoss(temperature=temperature, alpha=alpha, divergence=divergence, beta=beta)
        self.is_quantized_teacher = is_quantized_teacher
        self.divergence = divergence
        self.lmbda = float(lmbda)
        self.on_policy_generate = dict(on_policy_generate) if on_policy_generate is not None else None
        self._on_policy_rng = None      # CPU generator of the per-micro-batch draw and the rollout seeds
        self._on_policy_seen = [0, 0]   # [on-policy, all] training micro-batches since the previous log
        if self.lmbda > 0:
            core = ddp.unwrap(self.model)
            if not (isinstance(core, HipQwen3ForCausalLM) and core.flat.is_cuda and core._lora is None):
                raise ValueError("lmbda > 0 is built for a HipQwen3ForCausalLM student on the GPU without LoRA (the rollout "
                                 "decodes from the live flat weights)")
            self._on_policy_rng = torch.Generator().manual_seed(int(self.args.seed) + int(self.args.process_index))
        # compute back-ends; the product ones are the HIP kernels (tests may inject a checker here)
        self._extract_topk = ops.logsoftmax_topk
        self._extract_tail = ops.topk_tail
        # The frozen teacher does not depend on the student: on GPUs its forward (+ top-K) runs on a second HIP
        # stream beside the student forward (+4.5 % step throughput on MI355X); results are identical.
        self.overlap_teacher = True
        self._teacher_stream = None
        self._copy_stream = None
        # The teacher's pass of micro-batch i+1 of an accumulation window is enqueued at the END of training_step(i): HF's
        # per-micro-batch host read (logging_nan_inf_filter, on by default) drains the main stream after every backward,
        # and the GPU then has the next teacher pass to run while the host walks back to compute_loss (+1.6-2.1 % loop
        # throughput; with HF's read off the host is ahead anyway and it measured -0.5 %, so "auto" follows that flag).
        # SD_TEACHER_AHEAD=0 / 1 forces it.
        self._drop_lookahead()
        # Training steps apply both lm_heads, the top-K and the loss only to the rows the loss reads (positions whose
        # NEXT label is not -100, distillation_loss.py:31-45) instead of computing all B*T rows and masking them
        # afterwards; loss and gradients are the same, the head is ~(masked fraction) cheaper.  Needs one host sync
        # per step for the row count.  Off: the full [B,T,V] path; return_outputs=True always uses the full path.
        self.compact_head = True

    # ------------------------------------------------------------------------------ on-policy window rollouts
    @staticmethod
    def _check_engine_config(cfg):
        """``on_policy_engine``: None or a dict of ``ENGINE_KEYS``.  -> a copy; ValueError for anything else."""
        if cfg is None:
            return {}
        if not isinstance(cfg, dict) or set(cfg) - set(ENGINE_KEYS):
            raise ValueError(f"on_policy_engine must be a dict of {ENGINE_KEYS}, got {cfg!r}")
        from .engine import ADMISSION
        if cfg.get("admission", "single") not in ADMISSION:
            raise ValueError(f"on_policy_engine['admission'] must be one of {ADMISSION}, got {cfg['admission']!r}")
        for k in ("max_batch", "n_pages", "sync_every"):
            if cfg.get(k) is not None and (not isinstance(cfg[k], int) or isinstance(cfg[k], bool) or cfg[k] < 1):
                raise ValueError(f"on_policy_engine[{k!r}] must be a positive integer, got {cfg[k]!r}")
        return dict(cfg)

    @staticmethod
    def _window_plan(model, targs, collator, generate_kwargs, cfg):
        """What ``on_policy_rollout="window"`` refuses, before HF's constructor and long before anything is allocated,
        and the engine's shape: -> ``cfg`` with ``max_batch`` (default: the rows of one accumulation window, at most
        ``WINDOW_MAX_ROWS``), ``sync_every`` and ``admission`` filled in (``n_pages``: None = sized at the first window)."""
        core = ddp.unwrap(model) if model is not None else None
        if getattr(core, "_lora", None) is not None:
            raise ValueError('on_policy_rollout="window" is not built for a LoRA student: the engine decodes from the '
                             "live flat weights, an adapter's merged copy would have to be refreshed every window")
        if getattr(collator, "padding_free", False):
            raise ValueError('on_policy_rollout="window" with packed batches (padding_free): on-policy rollouts rebuild '
                             "right-padded [B, T] rows")
        world = max(int(os.environ.get("WORLD_SIZE", "1") or 1), int(getattr(targs, "world_size", 1) or 1))
        if world > 1:
            raise ValueError(f'on_policy_rollout="window" is built and tested on one rank only, got WORLD_SIZE {world}')
        rows = 1
        if targs is not None:
            rows = int(targs.per_device_train_batch_size) * int(targs.gradient_accumulation_steps)
        out = dict(cfg)
        out["max_batch"] = int(cfg.get("max_batch") or min(rows, WINDOW_MAX_ROWS))
        out["sync_every"] = int(cfg.get("sync_every") or 16)
        out["admission"] = cfg.get("admission", "single")
        out.setdefault("n_pages", None)
        kernels = generate_kwargs.get("decode_kernels", "tile")
        if kernels == "skinny" and out["max_batch"] > 16:
            raise ValueError(f'decode_kernels="skinny" keeps a row\'s tokens independent of the batch for up to 16 rows, the '
                             f'window engine would hold {out["max_batch"]}: use decode_kernels="wide" (up to 64 rows), or '
                             "on_policy_engine={'max_batch': 16}")
        if kernels == "wide" and out["max_batch"] > WINDOW_MAX_ROWS:
            raise ValueError(f'decode_kernels="wide" takes up to {WINDOW_MAX_ROWS} rows, got max_batch {out["max_batch"]}')
        return out

    def _window_engine(self, core, width):
        """The trainer's one ``GenerationEngine`` over a pool of its own, built at the first window.  ``n_pages`` defaults
        to ``max_batch`` rows' worst case at the window's width (a request holds at most ``width`` positions: its prompt
        and a budget cut at the row's width) plus the parking page; a later window that needs more pages per row than
        every window before it replaces engine and pool (a given ``n_pages`` is kept, and ``submit`` refuses what it
        cannot hold)."""
        from .paged import PAGE, pages_for
        cfg = self.on_policy_engine
        per_row = pages_for(width)
        if self._engine is not None and (cfg["n_pages"] is not None or per_row <= self._engine_pages):
            return self._engine
        self.close_engine()
        n_pages = cfg["n_pages"] if cfg["n_pages"] is not None else cfg["max_batch"] * per_row + 1
        self._engine_pool = core.kv_page_pool(n_pages)
        from .engine import GenerationEngine
        self._engine = GenerationEngine(core, self._engine_pool, cfg["max_batch"],
                                        self.on_policy_generate.get("decode_kernels", "tile"), "bf16", cfg["sync_every"],
                                        capacity=None if cfg["n_pages"] is not None else per_row * PAGE,
                                        admission=cfg["admission"])
        self._engine_pages = per_row
        self.engines_built += 1
        return self._engine

    def close_engine(self):
        """Close the window engine (its pages go back to its pool) and drop both."""
        if self._engine is not None:
            self._engine.close()
        self._engine, self._engine_pool, self._engine_pages = None, None, 0

    def __del__(self):
        try:
            self.close_engine()
        except Exception:
            pass

    def _roll_out_window(self, batch_samples):
        """``on_policy_rollout="window"``: one draw per micro-batch of the window, in order (``on_policy.draw``: the stream
        of the micro-batch mode), then ONE engine run for every drawn micro-batch (``on_policy.rollout_window``, under
        no_grad; the engine reads the live flat weights, which do not change inside a window).  Undrawn micro-batches pass
        through as the same objects.  ``model.training``, ``flat_grad`` and saved activations are not touched."""
        core = ddp.unwrap(self.model)
        for b in batch_samples:
            if isinstance(b, dict):   # (a packed batch is refused before anything is drawn or allocated)
                self._check_packed(b, b.get("teacher_input_ids"), b.get("teacher_attention_mask"))
        draws = [on_policy.draw(self._on_policy_rng, self.lmbda) for _ in batch_samples]
        self._window_draws = [on for on, _ in draws]   # counted one by one as training_step takes the micro-batches
        if not any(on for on, _ in draws):
            return batch_samples
        batches = [self._prepare_inputs(b) if on else b for b, (on, _) in zip(batch_samples, draws)]
        width = max(b["input_ids"].shape[1] for b, (on, _) in zip(batches, draws) if on)
        with torch.no_grad():
            return on_policy.rollout_window(self._window_engine(core, width), batches, self.on_policy_generate,
                                            [seed for _, seed in draws])

    def create_optimizer(self, model=None):
        """HF trainer.py `create_optimizer(self, model=None)`: TrainingArguments' default is torch AdamW (the reference passes no
        ``optim``, train.py:331-354).  For a flat-buffer student on the GPU the same update -- same hyper-parameters,
        weight decay on matrices only like HF's parameter groups, moments in the parameters' dtype (quirk Q5) -- is ONE
        fused launch over the flat parameter / gradient / moment buffers (``sd_adamw_bf16``).  HF keeps clipping
        (``max_grad_norm``) and the learning-rate schedule: the scheduler writes ``param_groups[0]["lr"]``."""
        core = ddp.unwrap(self.model)
        if (self.optimizer is None and self.fused_optimizer and self._default_adamw() and isinstance(core, HipQwen3ForCausalLM)
                and core.flat.is_cuda and (core._lora is not None or all(p.requires_grad for p in core.parameters()))):
            self.optimizer = self._flat_adamw(core)
            return self.optimizer
        if isinstance(core, HipQwen3ForCausalLM) and core._lora is not None and self.optimizer is None:
            raise NotImplementedError("a LoRA student (lora.py) trains through FlatAdamW only: its adapter gradients are "
                                      "bf16 projections of the flat weight gradient next to fp32 masters; leave "
                                      "TrainingArguments.optim at its adamw_torch default, as the reference does")
        # (HF calls create_optimizer(model) on its delay_optimizer_creation path: FSDP / SageMaker model parallel)
        return super().create_optimizer(model) if model is not None else super().create_optimizer()

    # ------------------------------------------------------------------------------ packed (padding-free) batches
    @staticmethod
    def _is_packed(batch):
        """A batch is packed by its keys, exactly when HF Qwen3 and HipQwen3ForCausalLM pack: ``position_ids`` present and
        ``attention_mask`` absent (``ProcessedDataCollator(padding_free=True)``)."""
        return batch.get("position_ids") is not None and batch.get("attention_mask") is None

    def _check_packed(self, batch, teacher_input_ids, teacher_attention_mask):
        """What a packed step refuses, before any launch."""
        ids = batch.get("input_ids")
        if batch.get("cu_seq_lens_q") is not None and (batch.get("attention_mask") is not None
                                                       or teacher_attention_mask is not None):
            raise ValueError("a packed batch (cu_seq_lens_q) also carries an attention_mask: packed documents have no "
                             "padding to mask, and a model given both would not pack")
        if not self._is_packed(batch):
            return False
        if self.lmbda > 0:
            raise ValueError("lmbda > 0 with a packed batch: on-policy rollouts rebuild right-padded [B, T] rows and are "
                             "not built for packed documents (use the padded collator, or lmbda=0)")
        if teacher_input_ids is not None and ids is not None and tuple(teacher_input_ids.shape) != tuple(ids.shape):
            raise ValueError(f"teacher_input_ids {tuple(teacher_input_ids.shape)} and input_ids {tuple(ids.shape)} must be "
                             "position-aligned (data.py:20-60 align_prefixes): packed documents share one set of boundaries")
        return True

    def _select_packed(self, core, batch, lab, speech_mask):
        """Loss rows and descriptors of one packed micro-batch: ``ops.packed_rows`` (the step's ONE host read: row count,
        segment check, longest document, largest position), then one ``PackedBatch`` for the student, shared with the
        teacher when its RoPE rows are the same (else a second one from the same checked numbers, still without a read).
        -> (rows, row_labels, (student descriptor, teacher descriptor)); a descriptor is None for a model that is not a
        HipQwen3ForCausalLM (it takes the packed keys themselves)."""
        cu, pos = batch["cu_seq_lens_q"], batch["position_ids"]
        cu_k = batch.get("cu_seq_lens_k")   # (compared by shape only: comparing the values would be a second host read)
        if cu_k is not None and cu_k is not cu and tuple(cu_k.shape) != tuple(cu.shape):
            raise ValueError("cu_seq_lens_k differs from cu_seq_lens_q: packed causal attention takes one set of segments")
        rows, row_labels, longest, max_pos = ops.packed_rows(lab, cu, speech_mask, pos)
        pbs = [None, None]
        for i, m in enumerate((core, self.teacher_model)):
            if isinstance(m, HipQwen3ForCausalLM) and m.flat.is_cuda and lab.is_cuda:
                if i == 1 and pbs[0] is not None and m.shares_packed_batch(core):
                    pbs[1] = pbs[0]
                else:
                    pbs[i] = m.packed_batch(cu, pos, longest, max_pos)
        return rows, row_labels, tuple(pbs)

    @staticmethod
    def _packed_tensors(pbs):
        return [t for pb in {id(pb): pb for pb in pbs or () if pb is not None}.values() for t in pb.tensors()]

    def _document_start_labels(self, labels, batch):
        """``labels`` with -100 at every document start of a packed batch (one scatter, no read): after the causal shift
        the last token of a document then predicts nothing on the full [1, M, V] path, whatever the collator wrote."""
        M = labels.numel()
        cu = batch.get("cu_seq_lens_q")
        if cu is not None:
            start = torch.zeros(M + 1, dtype=torch.bool, device=labels.device)   # (an empty last document starts at M)
            start[cu.to(device=labels.device, dtype=torch.int64)] = True
            start = start[:M].reshape(labels.shape)
        else:   # position_ids alone: HF's rule (ops.packed_segments)
            pos = batch["position_ids"].to(labels.device)
            start = torch.ones_like(pos, dtype=torch.bool)
            start[:, 1:] = pos[:, 1:] != pos[:, :-1] + 1
        return torch.where(start, torch.full_like(labels, -100), labels)

    # ------------------------------------------------------------------------------ the step plan and what is done ahead
    def _plan_step(self, core, batch, lab, speech_mask, teacher_mask, need_teacher, select=True, event=None, stored=None):
        """The ``StepPlan`` of one micro-batch: the step's ONE host read (the row count and, in the same read, the segment
        or padding checks) and the forward keywords that follow from it.  ``event``: planned ahead, on the copy stream
        that records it; ``stored``: a plan made ahead for these labels, returned when its key still matches (else the
        selection is redone); ``select=False``: the caller takes the full [B, T, V] path, only what the models need is made.
        * packed with ``cu_seq_lens_q``: always selected -- the descriptors come out of the same read;
        * packed by ``position_ids`` alone: the models read the segments themselves, and the rows come from the labels with
          every document start masked, so that none crosses a document boundary.  Never planned ahead (-> None);
        * padded: only masks laid out on the labels' [B, T] grid go into the fused right-padding check (the teacher's only
          for a HIP teacher that will run); any other keeps its own validation in the model's forward (no ``padding_checked``)."""
        if lab is None:
            return StepPlan()
        packed = self._is_packed(batch)
        cu = batch.get("cu_seq_lens_q") if packed else None
        hip_teacher = isinstance(self.teacher_model, HipQwen3ForCausalLM)
        full_labels = am = tam = None
        if cu is not None and event is not None:   # planned ahead: refused before its first launch (compute_loss refuses its own)
            self._check_packed(batch, batch.get("teacher_input_ids"), teacher_mask)
        if cu is None:
            if packed:
                if event is not None:
                    return None
                full_labels = self._document_start_labels(lab, batch)
            if not select:
                return StepPlan(full_labels=full_labels)
            am, tam = batch.get("attention_mask"), (teacher_mask if hip_teacher and need_teacher else None)
            am, tam = (m if m is not None and tuple(m.shape) == tuple(lab.shape) else None for m in (am, tam))
        key = (id(lab), lab.data_ptr(), tuple(lab.shape)) + tuple(None if t is None else t.data_ptr()
                                                                  for t in (speech_mask, am, tam, cu))
        if stored is not None and stored.key == key:
            return stored
        if cu is not None:
            rows, row_labels, pbs = self._select_packed(core, batch, lab, speech_mask)
            student_kw, teacher_kw = ({"packed_batch": pb} if pb is not None else {} for pb in pbs)
        else:
            rows, row_labels = ops.loss_rows(lab if full_labels is None else full_labels, speech_mask, right_padded=(am, tam))
            pbs = None
            student_kw = {"padding_checked": True} if am is not None or batch.get("attention_mask") is None else {}
            teacher_kw = {"padding_checked": True} if hip_teacher and (tam is not None or teacher_mask is None) else {}
        return StepPlan(rows, row_labels, pbs, student_kw, teacher_kw, event, key, full_labels)

    def _drop_lookahead(self):
        """Nothing is planned, fetched or enqueued ahead."""
        self._ahead = {}   # id(labels) -> _Ahead, of the micro-batches of this accumulation window and the next
        self._window, self._prefetched = [], None

    def _start_teacher(self, core, batch, teacher_input_ids, teacher_mask, plan):
        """``_teacher_pass`` on the teacher's own stream.  It waits for the batch -- the plan's event, not whatever else the
        main stream still has queued -- or, for a batch planned in place, for the main stream.  Two passes then share the
        GPU and both are told (``concurrent``: SD_FWD_CONCURRENT, include/sd_hip.h)."""
        ids = batch.get("input_ids")
        if self._teacher_stream is None:
            self._teacher_stream = ops.concurrent_stream(ids.device, "teacher")
        side = self._teacher_stream
        if plan.event is not None:
            side.wait_event(plan.event)
            for t in [ids, teacher_input_ids, teacher_mask, batch.get("attention_mask"), plan.rows,
                      batch.get("position_ids")] + self._packed_tensors(plan.packed):
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(side)
        else:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            return self._teacher_pass(batch, teacher_input_ids, teacher_mask, core.dims.vocab_size, plan.rows,
                                      dict(plan.teacher_kw, concurrent=True))

    def get_batch_samples(self, epoch_iterator, num_batches, device):
        """HF fetches the micro-batches of one optimizer step here, together, right after it has enqueued the previous
        optimizer step.  Two things are done with that (``SD_ROWS_AHEAD=0`` turns both off):

        * the loss-row selection of every micro-batch (one host read each: the row count) happens now, so the
          accumulation window itself has no host reads of ours -- with ``logging_nan_inf_filter=False`` (HF's own
          per-micro-batch read) the host enqueues the whole window ahead of the GPU;
        * the fetch -- accelerate's host-to-device copies, HF's token count, the row selection -- runs on a stream of its
          own ("h2d"): none of it depends on the optimizer kernels still queued on the main stream, and the frozen
          teacher's pass in ``compute_loss`` then waits for THAT stream's event only, i.e. the teacher's forward of the
          window's first micro-batch runs beside the AdamW update (HBM-bound) instead of after it.

        Same selection, validation and arguments as ``compute_loss`` would use on its own."""
        core = ddp.unwrap(self.model)
        ahead = (self.compact_head and os.environ.get("SD_ROWS_AHEAD", "1") != "0" and isinstance(core, HipQwen3ForCausalLM)
                 and core.flat.is_cuda and isinstance(self.distill_loss_fn, DistillationLoss) and self.lmbda == 0)
        if not ahead:
            self._drop_lookahead()
            batch_samples, num_items = super().get_batch_samples(epoch_iterator, num_batches, device)
            if self.lmbda > 0 and self.on_policy_rollout == "window":   # the whole window's rollouts, before its first step
                batch_samples = self._roll_out_window(batch_samples)
            return batch_samples, num_items
        # window k comes from the previous call's lookahead when there is one (same iterator object = same epoch)
        pre, self._prefetched = self._prefetched, None
        if pre is not None and pre[0] is epoch_iterator:   # (its plans, and a teacher's result, are in the table already)
            batch_samples, num_items, ready = pre[1]
        else:
            batch_samples, num_items, ready = self._fetch_window(core, epoch_iterator, num_batches, device)
        main = torch.cuda.current_stream(core.flat.device)
        main.wait_event(ready)
        live = {id(b.get("labels")) for b in batch_samples if isinstance(b, dict)}
        self._ahead = {k: v for k, v in self._ahead.items() if k in live}
        self._window = list(batch_samples)   # the micro-batches in the order they are trained on: this window, then the next
        # ... and window k+1 is fetched NOW (lock-step host only: HF's per-micro-batch read on), so that the last
        # training_step of window k can enqueue the teacher's pass for its first micro-batch beside the optimizer step
        mode = os.environ.get("SD_WINDOW_AHEAD", "auto")
        if batch_samples and (mode == "1" or (mode == "auto" and self.args.logging_nan_inf_filter)):
            nxt = self._fetch_window(core, epoch_iterator, num_batches, device)
            self._prefetched = (epoch_iterator, nxt)
            self._window += list(nxt[0])
        return batch_samples, num_items

    def _fetch_window(self, core, epoch_iterator, num_batches, device):
        """HF's fetch of one accumulation window + the plans of its micro-batches (CUDA tensor labels only), on the copy
        stream; the plans go into the table.  Returns (batch_samples, num_items_in_batch, event)."""
        main = torch.cuda.current_stream(core.flat.device)
        if self._copy_stream is None:
            self._copy_stream = ops.concurrent_stream(core.flat.device, "h2d")
        cs = self._copy_stream
        ready = torch.cuda.Event()
        with torch.cuda.stream(cs):
            batch_samples, num_items = super().get_batch_samples(epoch_iterator, num_batches, device)
            plans = []
            for b in batch_samples:
                lab = b.get("labels") if isinstance(b, dict) else None
                if torch.is_tensor(lab) and lab.is_cuda:
                    need_teacher = b.get("teacher_top_k_v") is None and self.teacher_model is not None
                    plans.append(self._plan_step(core, b, lab, b.get("speech_token_mask"), b.get("teacher_attention_mask"),
                                                 need_teacher, event=ready))
            ready.record(cs)
        plans = [p for p in plans if p is not None]
        self._ahead.update((p.key[0], _Ahead(p)) for p in plans)
        # the tensors were allocated on the copy stream and are used on the main and the teacher's stream
        users = [main] + ([self._teacher_stream] if self._teacher_stream is not None else [])
        held = [t for b in batch_samples if isinstance(b, dict) for t in b.values() if torch.is_tensor(t) and t.is_cuda]
        held += [t for p in plans for t in [p.rows, p.row_labels] + self._packed_tensors(p.packed)]
        held += [num_items] if torch.is_tensor(num_items) and num_items.is_cuda else []
        for t in held:
            for st in users:
                t.record_stream(st)
        return batch_samples, num_items, ready

    _TEACHER_SIDE_KEYS = ("teacher_input_ids", "teacher_attention_mask", "speech_token_mask", "teacher_top_k_v", "teacher_top_k_i",
                          "teacher_top_k_tail")

    def training_step(self, model, inputs, *args, **kwargs):
        if self.lmbda > 0:
            if isinstance(inputs, dict):   # (a packed batch is refused before the rollout, not after it)
                self._check_packed(inputs, inputs.get("teacher_input_ids"), inputs.get("teacher_attention_mask"))
            if self.on_policy_rollout == "micro_batch":
                inputs = self._maybe_on_policy(model, inputs)
            else:   # "window": drawn and rolled out in get_batch_samples; counted here, where the micro-batch mode counts
                self._on_policy_seen[1] += 1
                self._on_policy_seen[0] += int(self._window_draws.pop(0)) if self._window_draws else 0
        lab = inputs.get("labels") if isinstance(inputs, dict) else None
        loss = super().training_step(model, inputs, *args, **kwargs)
        mode = os.environ.get("SD_TEACHER_AHEAD", "auto")
        if (lab is not None and self._window and self.lmbda == 0
                and (mode == "1" or (mode == "auto" and self.args.logging_nan_inf_filter))):
            self._launch_teacher_ahead(id(lab))
        return loss

    def _maybe_on_policy(self, model, inputs):
        """One draw per training micro-batch; below ``lmbda`` the batch is rebuilt around the student's own continuation
        (``on_policy.rollout``: no_grad, the decoder reads the live flat weights; ``flat``, ``flat_grad``, the saved
        activations and the train/eval flag are not touched).  The rollout's seed comes from the same generator."""
        self._on_policy_seen[1] += 1
        on, seed = on_policy.draw(self._on_policy_rng, self.lmbda)
        if not on:
            return inputs
        self._on_policy_seen[0] += 1
        return on_policy.rollout(ddp.unwrap(model).generate, self._prepare_inputs(inputs), self.on_policy_generate, seed)

    def _launch_teacher_ahead(self, cur_id):
        """Enqueue the frozen teacher's pass for the micro-batch that follows ``cur_id`` in this accumulation window."""
        seq = self._window   # (the next window's first micro-batch follows this window's last)
        idx = next((i for i, b in enumerate(seq) if isinstance(b, dict) and id(b.get("labels")) == cur_id), None)
        if idx is None or idx + 1 >= len(seq):
            return
        nxt = seq[idx + 1]
        lab = nxt.get("labels")
        entry = self._ahead.get(id(lab))
        core = ddp.unwrap(self.model)
        ids, tids = nxt.get("input_ids"), nxt.get("teacher_input_ids")
        if (entry is None or entry.plan.rows.numel() == 0 or not self.overlap_teacher or nxt.get("teacher_top_k_v") is not None
                or not isinstance(self.teacher_model, HipQwen3ForCausalLM) or not isinstance(core, HipQwen3ForCausalLM)
                or ids is None or (tids is not None and tuple(tids.shape) != tuple(ids.shape))):
            return
        base = {k: v for k, v in nxt.items() if k not in self._TEACHER_SIDE_KEYS}
        entry.teacher = self._start_teacher(core, base, tids, nxt.get("teacher_attention_mask"), entry.plan)

    def _load_best_model(self):
        """HF's loader looks for ``model.safetensors``; a LoRA student's checkpoints hold the adapter (``_save`` above)."""
        core = ddp.unwrap(self.model)
        best = self.state.best_model_checkpoint
        if isinstance(core, HipQwen3ForCausalLM) and core._lora is not None and best is not None:
            core._lora.load_adapter(best)
            return
        return super()._load_best_model()

    def _teacher_pass(self, inputs, teacher_input_ids, teacher_attention_mask, vocab_size, rows=None, model_kw=None):
        """train.py:60-94: teacher no-grad forward, then on-the-fly top-K unless quantized / top_k <= 0.
        -> (logits, None, None, None) or (None, top_v, top_i, tail); ``tail`` is None but for the ``_tail`` divergences.
        ``rows``: only those flat rows of the logits are produced (our own teacher) or kept (any other module);
        ``model_kw``: extra keyword arguments for a HipQwen3ForCausalLM teacher (``padding_checked``, ``packed_batch``).
        A packed batch (``_is_packed(inputs)``): the teacher's own ids go with the batch's packed keys and no mask -- one
        set of document boundaries serves both models."""
        model_kw = model_kw or {}
        with torch.no_grad():
            extra = {"logit_rows": rows} if rows is not None and isinstance(self.teacher_model, HipQwen3ForCausalLM) else {}
            if teacher_input_ids is not None and teacher_attention_mask is None and self._is_packed(inputs):
                teacher_outputs = self.teacher_model(input_ids=teacher_input_ids, **extra, **model_kw,
                                                     **{k: inputs[k] for k in self.PACKED_KEYS if inputs.get(k) is not None})
            elif teacher_input_ids is not None:
                teacher_outputs = self.teacher_model(input_ids=teacher_input_ids, attention_mask=teacher_attention_mask,
                                                     **extra, **model_kw)
            else:
                teacher_outputs = self.teacher_model(**{k: v for k, v in inputs.items() if k != "labels"}, **extra,
                                                     **model_kw)
            teacher_logits = teacher_outputs.logits
            if rows is not None and not extra:
                teacher_logits = teacher_logits.reshape(-1, teacher_logits.size(-1))[rows]
            if not self.is_quantized_teacher and self.top_k > 0:
                v, i = self._extract_topk(teacher_logits, self.top_k, vocab_size)
                tail = None
                if self.divergence in ops.TAIL_DIVERGENCES:   # the logits are still here: their mass outside the top-K at T
                    tail = self._extract_tail(teacher_logits, i, self.distill_loss_fn.temperature, vocab_size)
                return None, v, i, tail
        return teacher_logits, None, None, None

    def compute_loss(self, model, inputs, return_outputs=False, **kwargs):
        """Pop the teacher's keys and refuse what cannot be computed  ->  count the tokens  ->  the plan (made ahead, or
        here)  ->  the teacher's result (enqueued ahead, on its stream now, gathered from the pre-extracted top-K, or after
        the student as in the reference)  ->  student forward  ->  join  ->  loss on the plan's rows  ->  log."""
        (teacher_input_ids, teacher_attention_mask, speech_mask, teacher_top_k_v, teacher_top_k_i,
         teacher_top_k_tail) = (inputs.pop(k, None) for k in self._TEACHER_SIDE_KEYS)   # (the tail: the _tail divergences only)
        if ops.takes_dense_teacher(self.divergence) and teacher_top_k_v is not None:
            raise ValueError(f"divergence={self.divergence!r} needs the dense teacher distribution; this batch carries "
                             "pre-extracted teacher_top_k_v (K entries per position)")
        need_teacher = teacher_top_k_v is None and self.teacher_model is not None
        ids = inputs.get("input_ids")
        packed = self._check_packed(inputs, teacher_input_ids, teacher_attention_mask)
        if (need_teacher and teacher_input_ids is not None and ids is not None
                and tuple(teacher_input_ids.shape) != tuple(ids.shape)):
            # The collator pads teacher and student separately (data.py:219-278) and the loss indexes both with ONE
            # [B, T-1] row mask (distillation_loss.py:31-45): the reference dies there with an IndexError.  Same
            # condition, named, before any kernel indexes a [B, T_teacher] tensor with the student's T.
            raise ValueError(f"teacher_input_ids {tuple(teacher_input_ids.shape)} and input_ids {tuple(ids.shape)} must be "
                             "position-aligned (data.py:20-60 align_prefixes): the loss selects rows of both with one mask")
        self._count_tokens(model, ids)

        # `model` is what the loop trains (HipDataParallel / torch DDP / the bare module); `core` is the module itself
        core = ddp.unwrap(model)
        hip_student = isinstance(core, HipQwen3ForCausalLM)
        lab = inputs.get("labels")
        compact = (self.compact_head and not return_outputs and hip_student and lab is not None and lab.is_cuda
                   and isinstance(self.distill_loss_fn, DistillationLoss))
        ahead = self._ahead.pop(id(lab), None)   # planned with the accumulation window's other batches (get_batch_samples)
        plan = self._plan_step(core, inputs, lab, speech_mask, teacher_attention_mask, need_teacher, select=compact,
                               stored=None if ahead is None else ahead.plan)
        if ahead is not None and ahead.plan is not plan:   # made from other tensors: discarded with what was enqueued for it
            ahead = None
        if not compact or plan.rows.numel() == 0:
            # The full [B, T, V] path (with no row it returns the reference's zeros, distillation_loss.py:47-53).  What the
            # plan has checked still serves both models; a packed batch is then taken as made in place.
            plan = plan._replace(rows=None, row_labels=None, event=None if plan.packed is not None else plan.event)
            ahead = None

        side, teacher = None, (None, teacher_top_k_v, teacher_top_k_i, teacher_top_k_tail)
        if ahead is not None and ahead.teacher is not None:   # SD_TEACHER_AHEAD: enqueued at the end of the previous micro-step
            side, teacher = self._teacher_stream, ahead.teacher
        elif (need_teacher and self.overlap_teacher and ids is not None and ids.is_cuda
                and isinstance(self.teacher_model, HipQwen3ForCausalLM)
                and getattr(getattr(core, "dims", None), "vocab_size", None) is not None):   # only our own model type is overlapped
            teacher = self._start_teacher(core, inputs, teacher_input_ids, teacher_attention_mask, plan)
            side = self._teacher_stream
        elif plan.rows is not None and teacher_top_k_v is not None:  # pre-extracted top-K: keep the same rows
            v, i, tail = ((None if t is None else t.to(lab.device)) for t in teacher[1:])
            teacher = (None, v.reshape(-1, v.size(-1))[plan.rows], i.reshape(-1, i.size(-1))[plan.rows],
                       None if tail is None else tail.reshape(-1)[plan.rows])

        student_kw = dict(plan.student_kw, concurrent=True) if side is not None and hip_student else plan.student_kw
        if plan.rows is not None:
            student_kw = dict(student_kw, logit_rows=plan.rows)
        outputs = model(**inputs, **student_kw)  # train.py:54
        student_logits = outputs.logits
        labels = inputs.pop("labels", None)
        if packed and plan.rows is None and labels is not None:   # the full [1, M, V] path shifts across the flat row itself
            labels = plan.full_labels if plan.full_labels is not None else self._document_start_labels(labels, inputs)

        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
            for t in teacher:   # allocated on the teacher's stream, read on this one
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(torch.cuda.current_stream())
        elif need_teacher:  # reference order: student first, then teacher (train.py:60-94)
            teacher = self._teacher_pass(inputs, teacher_input_ids, teacher_attention_mask, student_logits.size(-1),
                                         plan.rows, plan.teacher_kw)
        teacher_logits, teacher_top_k_v, teacher_top_k_i, teacher_top_k_tail = teacher

        if isinstance(self.distill_loss_fn, DistillationLoss):
            self.distill_loss_fn.inplace_grad = (not return_outputs) and hip_student
        # (the tail goes to the _tail divergences only: any other loss, a caller's own included, keeps its signature)
        tail_kw = {"teacher_top_k_tail": teacher_top_k_tail} if self.divergence in ops.TAIL_DIVERGENCES else {}
        if plan.rows is not None:
            loss, task_loss, distill_loss, teacher_loss = self.distill_loss_fn.forward_rows(
                student_logits, plan.row_labels, teacher_logits=teacher_logits, teacher_top_k_v=teacher_top_k_v,
                teacher_top_k_i=teacher_top_k_i, **tail_kw)
        else:
            loss, task_loss, distill_loss, teacher_loss = self.distill_loss_fn(
                student_logits=student_logits, labels=labels, teacher_logits=teacher_logits,
                teacher_top_k_v=teacher_top_k_v, teacher_top_k_i=teacher_top_k_i, speech_token_mask=speech_mask, **tail_kw)

        if self.state.global_step % self.args.logging_steps == 0:  # train.py:107-114
            # one device->host sync for the three scalars instead of three .item() calls
            vals = torch.stack([task_loss.detach().float(), teacher_loss.detach().float(),
                                distill_loss.detach().float()]).tolist()
            logs = {"student_loss": vals[0], "teacher_loss": vals[1], "distill_loss": vals[2]}
            if self.lmbda > 0 and model.training:   # evaluation neither reports nor resets the training counters
                on, seen = self._on_policy_seen
                logs["on_policy_fraction"] = on / max(seen, 1)
                self._on_policy_seen = [0, 0]
            self.log(logs)
        return (loss, outputs) if return_outputs else loss


class Stage1Trainer(FlatStudentTrainer):
    """Stage-1 speech-token alignment (reference stage1.py:285-335: TRL SFTTrainer, ``adamw_torch``, ``max_grad_norm`` 1.0)
    on a model frozen by ``stage1.freeze_model_weights``: plain causal-LM cross-entropy, FlatAdamW over the Stage-1
    segments (the embedding, + an untied lm_head: HF's decay groups put weight decay on both), the one-reduction clip,
    tokens/sec in the training log.  Single GPU.  Batches: ``stage1.Stage1Collator`` (input_ids, attention_mask, labels; or,
    with ``padding_free=True``, input_ids, labels, position_ids and the flash-attn varlen keys, passed through)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.args.world_size > 1:
            raise NotImplementedError("Stage-1 alignment runs on one GPU (multi-GPU Stage-1 is not implemented)")
        # compute_loss passes num_items_in_batch to the model itself; HF must then neither drop the count nor divide the
        # loss by the accumulation steps, whatever its signature probe of the model concluded
        self.model_accepts_loss_kwargs = True

    def create_optimizer(self, model=None):
        core = ddp.unwrap(self.model)
        if (self.optimizer is None and self.fused_optimizer and self._default_adamw() and isinstance(core, HipQwen3ForCausalLM)
                and core.flat.is_cuda and core.stage1_row_lo is not None):
            core.check_stage1()
            self.optimizer = self._flat_adamw(core)
            return self.optimizer
        return super().create_optimizer(model) if model is not None else super().create_optimizer()

    def compute_loss(self, model, inputs, return_outputs=False, num_items_in_batch=None, **kwargs):
        ids = inputs["input_ids"]
        self._count_tokens(model, ids)
        packed = {k: inputs[k] for k in self.PACKED_KEYS if inputs.get(k) is not None}
        out = model(input_ids=ids, attention_mask=inputs.get("attention_mask"), labels=inputs["labels"],
                    num_items_in_batch=num_items_in_batch, stage1_inplace_grad=not return_outputs, **packed)
        return (out["loss"], out) if return_outputs else out["loss"]


def _pretrained_types():
    from transformers import PreTrainedModel
    return (PreTrainedModel,)
