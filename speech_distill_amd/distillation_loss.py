"""Drop-in for the reference's ``DistillationLoss`` (distillation_loss.py:6-128) on the HIP kernels.

Same constructor, same ``forward`` signature, same 4-tuple ``(total, task, distill, teacher_task)``,
same ``ValueError`` when neither teacher form is given.  Differences, all documented in DESIGN.md:
  * no shifted / boolean-compacted copies of the logits are made (distillation_loss.py:31-45): the
    kernel evaluates the valid-row predicate per row;
  * arithmetic is fp32 inside the kernel whatever the logits dtype (the reference runs log-softmax
    in the logits' dtype), outputs are fp32 0-d tensors;
  * N == 0 returns zeros that ARE connected to autograd (reference: constants, distillation_loss.py:47-53);
  * sub-losses are returned detached (the reference only ever ``.item()``s them, train.py:108-114).

Beyond the reference: ``divergence`` chooses the distillation term.  "forward_kl" (the default) is the reference's
KL(teacher || student) and the code path above, untouched.  "reverse_kl" is KL(student || teacher) and "jsd" the
beta-skewed Jensen-Shannon divergence beta KL(p || m) + (1 - beta) KL(q || m), m = (1 - beta) q + beta p (TRL's
``generalized_jsd_loss`` for 0 < beta < 1; its beta = 0 / 1 are "forward_kl" / "reverse_kl"), both with the same T^2 and
alpha conventions, on a DENSE teacher only (a top-K teacher defines p on K entries): DESIGN.md section 12.
"jsd_topk" is that same "jsd" against a TOP-K teacher: the K stored log-probs are renormalised at T and scattered to a
distribution P over the vocabulary (duplicated indices sum), and the divergence is "jsd" with p = P.  It reaches 0 only
when the student puts all its mass on the K indices, which is what a renormalised top-K teacher asks for.  It takes
``teacher_top_k_v`` / ``teacher_top_k_i`` only (dense ``teacher_logits`` are "jsd"'s).  There is no "reverse_kl" on a
top-K teacher: KL(q || P) is infinite as soon as P is 0 where the student has any mass.  DESIGN.md section 12b.
"forward_kl_tail", "reverse_kl_tail" and "jsd_tail" keep one more number per row, ``teacher_top_k_tail``: the teacher's
mass outside its top-K at T (``ops.topk_tail``).  Teacher and student are compared over K + 1 outcomes -- the K indices
and "anything else" -- so all three are finite, exact on the top-K part and a lower bound of the dense divergence.  They
take a top-K teacher only; without the tail, T = 1 derives it from the stored log-probs (``ops.tail_from_logprobs``) and
any other temperature is an error.  DESIGN.md section 12c.
"""
import torch
import torch.nn as nn

from . import ops
from .ops import GJSDLossRowsFn, GJSDTailLossRowsFn, GJSDTopKLossRowsFn, KDLossFn, KDLossRowsFn


class DistillationLoss(nn.Module):
    def __init__(self, temperature=2.0, alpha=0.5, inplace_grad=False, divergence="forward_kl", beta=0.5):
        super().__init__()
        ops.check_divergence(divergence, beta)
        self.divergence = divergence
        self.beta = beta
        self.temperature = temperature
        self.alpha = alpha
        # write d loss / d logits over the logits buffer itself (saves V*B*T*2 bytes); only safe
        # when nobody reads the logits after the loss -- the trainer turns it on for training steps
        self.inplace_grad = inplace_grad

    def forward(self, student_logits, labels, teacher_logits=None, teacher_top_k_v=None, teacher_top_k_i=None,
                speech_token_mask=None, teacher_top_k_tail=None):
        if teacher_logits is None and (teacher_top_k_v is None or teacher_top_k_i is None):
            raise ValueError("Either teacher_logits or top_k must be provided")
        if self.divergence != "forward_kl":
            # eval / return_outputs path: select the rows as the trainer does and gather them (one copy of R rows)
            self._need_form(teacher_logits, teacher_top_k_v, teacher_top_k_i)
            rows, row_labels = ops.loss_rows(labels, speech_token_mask)
            V = student_logits.shape[-1]
            if ops.takes_dense_teacher(self.divergence):
                return self.forward_rows(student_logits.reshape(-1, V)[rows], row_labels,
                                         teacher_logits=teacher_logits.detach().reshape(-1, V)[rows])
            pick = (lambda x: x.to(rows.device).reshape(-1, x.size(-1))[rows])
            tail = {}
            if self.divergence in ops.TAIL_DIVERGENCES:
                tail = {"teacher_top_k_tail": self._tail(teacher_top_k_v, teacher_top_k_tail).to(rows.device).reshape(-1)[rows]}
            return self.forward_rows(student_logits.reshape(-1, V)[rows], row_labels,
                                     teacher_top_k_v=pick(teacher_top_k_v), teacher_top_k_i=pick(teacher_top_k_i), **tail)
        if not student_logits.is_contiguous():
            student_logits = student_logits.contiguous()
        if teacher_logits is not None:
            teacher_logits = teacher_logits.detach()
        total, out = KDLossFn.apply(student_logits, labels, teacher_logits, teacher_top_k_v, teacher_top_k_i,
                                    speech_token_mask, self.temperature, self.alpha,
                                    self.inplace_grad and student_logits.requires_grad)
        return total, out[1], out[2], out[3]

    def forward_rows(self, student_logits, row_labels, teacher_logits=None, teacher_top_k_v=None, teacher_top_k_i=None,
                     teacher_top_k_tail=None):
        """Same 4-tuple for rows already shifted and selected by ``ops.loss_rows`` (what distillation_loss.py:31-45
        does with copies): ``student_logits`` [R,V], ``row_labels`` [R], teacher form [R,V] or ([R,K], [R,K]), for the
        ``_tail`` divergences with ``teacher_top_k_tail`` [R]."""
        if teacher_logits is None and (teacher_top_k_v is None or teacher_top_k_i is None):
            raise ValueError("Either teacher_logits or top_k must be provided")
        if teacher_logits is not None:
            teacher_logits = teacher_logits.detach()
        self._need_form(teacher_logits, teacher_top_k_v, teacher_top_k_i)
        s, inplace = student_logits.contiguous(), self.inplace_grad and student_logits.requires_grad
        form = ops.DIVERGENCE_TABLE[self.divergence].teacher
        if form == "topk":
            total, out = GJSDTopKLossRowsFn.apply(s, row_labels, teacher_top_k_v, teacher_top_k_i, self.temperature,
                                                  self.alpha, self.beta, inplace)
        elif form == "topk_tail":
            total, out = GJSDTailLossRowsFn.apply(s, row_labels, teacher_top_k_v, teacher_top_k_i,
                                                  self._tail(teacher_top_k_v, teacher_top_k_tail), self.temperature,
                                                  self.alpha, self.beta, self.divergence, inplace)
        elif form == "dense":
            total, out = GJSDLossRowsFn.apply(s, row_labels, teacher_logits, self.temperature, self.alpha, self.beta,
                                              self.divergence, inplace)
        else:
            total, out = KDLossRowsFn.apply(s, row_labels, teacher_logits, teacher_top_k_v, teacher_top_k_i,
                                            self.temperature, self.alpha, inplace)
        return total, out[1], out[2], out[3]

    def _need_form(self, teacher_logits, teacher_top_k_v, teacher_top_k_i):
        """ValueError unless the teacher comes in the form the divergence is defined on (``forward_kl`` takes either)."""
        if ops.takes_dense_teacher(self.divergence) and teacher_logits is None:
            raise ValueError(f"divergence={self.divergence!r} needs dense teacher_logits: a top-K teacher defines the "
                             "teacher distribution on K entries only")
        if ops.takes_topk_teacher(self.divergence) and (teacher_logits is not None or teacher_top_k_v is None
                                                         or teacher_top_k_i is None):
            raise ValueError(f"divergence={self.divergence!r} takes a top-K teacher (teacher_top_k_v, teacher_top_k_i); "
                             f"for dense teacher_logits use divergence={ops.dense_name(self.divergence)!r}")

    def _tail(self, teacher_top_k_v, teacher_top_k_tail):
        """The tail of a ``_tail`` divergence: the caller's, or at T = 1 the one the stored log-probs imply."""
        if teacher_top_k_tail is not None:
            return teacher_top_k_tail
        if float(self.temperature) != 1.0:
            raise ValueError(f"divergence={self.divergence!r} at temperature {self.temperature} needs teacher_top_k_tail (the "
                             "teacher's mass outside its top-K at that temperature: ops.topk_tail, or "
                             "extract_teacher_logits.py --tail_temperature); only at temperature 1 do the stored "
                             "log-probs imply it")
        return ops.tail_from_logprobs(teacher_top_k_v)
