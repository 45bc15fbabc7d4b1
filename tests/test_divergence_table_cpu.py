"""CPU: the one divergence table of speech_distill_amd/ops.py (DIVERGENCE_TABLE) says for every name what the names derived
from it, ``check_divergence``, ``DistillationLoss.forward_rows`` and the trainer's constructor check used to say in chains of
``if``: the entry stem and SD_DIV_* mode, the beta rule with its message, and the teacher form with both messages.

A right teacher form is recognised without a GPU by how far the call gets: past every ValueError of the form check, to
the autograd function's refusal of a CPU tensor (RuntimeError "must be a GPU tensor")."""
import pytest
import torch

from speech_distill_amd import DistillationLoss, ops

# the tuple of the commit before the table, in its order
PARENT_ALL = ("forward_kl", "reverse_kl", "jsd", "jsd_topk", "forward_kl_tail", "reverse_kl_tail", "jsd_tail")
# name -> (entry stem, SD_DIV_* mode, teacher form, beta in (0, 1), dense counterpart), written out independently of the table
WANT = {
    "forward_kl": ("sd_kdloss", None, "either", False, "forward_kl"),
    "reverse_kl": ("sd_gjsd", 1, "dense", False, "reverse_kl"),
    "jsd": ("sd_gjsd", 2, "dense", True, "jsd"),
    "jsd_topk": ("sd_gjsd_topk", None, "topk", True, "jsd"),
    "forward_kl_tail": ("sd_gjsd_tail", 0, "topk_tail", False, "forward_kl"),
    "reverse_kl_tail": ("sd_gjsd_tail", 1, "topk_tail", False, "reverse_kl"),
    "jsd_tail": ("sd_gjsd_tail", 2, "topk_tail", True, "jsd"),
}
R, V, K = 3, 16, 4


def test_the_derived_names_are_the_parents():
    assert ops.ALL_DIVERGENCES == PARENT_ALL
    assert ops.DIVERGENCES == {"reverse_kl": 1, "jsd": 2} and list(ops.DIVERGENCES) == ["reverse_kl", "jsd"]
    assert ops.TOPK_DIVERGENCE == "jsd_topk"
    assert ops.TAIL_DIVERGENCES == {"forward_kl_tail": 0, "reverse_kl_tail": 1, "jsd_tail": 2}
    assert list(ops.TAIL_DIVERGENCES) == ["forward_kl_tail", "reverse_kl_tail", "jsd_tail"]
    assert {n: tuple(d) for n, d in ops.DIVERGENCE_TABLE.items()} == WANT
    assert all(hasattr(ops, c) for c in ("KDLossFn", "KDLossRowsFn", "GJSDLossRowsFn", "GJSDTopKLossRowsFn",
                                         "GJSDTailLossRowsFn", "CELossRowsFn"))


@pytest.mark.parametrize("name", PARENT_ALL)
def test_check_divergence_and_the_beta_rule(name):
    ops.check_divergence(name, 0.5)
    for beta in (0.0, 1.0, -0.1, 1.5, float("nan")):
        if WANT[name][3]:
            with pytest.raises(ValueError) as e:
                ops.check_divergence(name, beta)
            assert str(e.value) == (f"divergence={name!r} needs 0 < beta < 1, got {beta!r} (beta = 0 is 'forward_kl', "
                                    "beta = 1 is 'reverse_kl')")
            with pytest.raises(ValueError, match="needs 0 < beta < 1"):
                DistillationLoss(divergence=name, beta=beta)
        else:
            ops.check_divergence(name, beta)   # beta is the JSD's alone
    assert ops.dense_name(name) == WANT[name][4]
    assert ops.takes_topk_teacher(name) == (WANT[name][2] in ("topk", "topk_tail"))
    assert ops.takes_dense_teacher(name) == (WANT[name][2] == "dense")


def test_an_unknown_name_lists_the_known_ones():
    with pytest.raises(ValueError) as e:
        ops.check_divergence("tail", 0.5)
    assert str(e.value) == "unknown divergence 'tail': one of " + ", ".join(repr(d) for d in PARENT_ALL)


def _forms():
    g = torch.Generator().manual_seed(0)
    dense = dict(teacher_logits=torch.randn(R, V, generator=g))
    topk = dict(teacher_top_k_v=torch.randn(R, K, generator=g).log_softmax(-1).half(),
                teacher_top_k_i=torch.randint(0, V, (R, K), generator=g, dtype=torch.int32))
    return torch.randn(R, V, generator=g), torch.randint(0, V, (R,), generator=g), dense, topk


@pytest.mark.parametrize("name", PARENT_ALL)
def test_forward_rows_demands_the_tables_teacher_form(name):
    s, labels, dense, topk = _forms()
    loss = DistillationLoss(temperature=1.0, divergence=name)   # T = 1: a _tail divergence derives its tail from the log-probs
    form = WANT[name][2]
    right = {"either": (dense, topk), "dense": (dense,), "topk": (topk,), "topk_tail": (topk,)}[form]
    for kw in right:   # the form check passes: the call ends where a CPU tensor is refused
        with pytest.raises(RuntimeError, match="must be a GPU tensor"):
            loss.forward_rows(s, labels, **kw)
    if form == "dense":
        with pytest.raises(ValueError) as e:
            loss.forward_rows(s, labels, **topk)
        assert str(e.value) == (f"divergence={name!r} needs dense teacher_logits: a top-K teacher defines the teacher "
                                "distribution on K entries only")
    if form in ("topk", "topk_tail"):
        for kw in (dense, dict(dense, **topk)):
            with pytest.raises(ValueError) as e:
                loss.forward_rows(s, labels, **kw)
            assert str(e.value) == (f"divergence={name!r} takes a top-K teacher (teacher_top_k_v, teacher_top_k_i); for dense "
                                    f"teacher_logits use divergence={WANT[name][4]!r}")
    with pytest.raises(ValueError, match="Either teacher_logits or top_k must be provided"):
        loss.forward_rows(s, labels)
    if form == "topk_tail":   # at any other temperature the tail has to be given
        with pytest.raises(ValueError, match="needs teacher_top_k_tail"):
            DistillationLoss(temperature=2.0, divergence=name).forward_rows(s, labels, **topk)
