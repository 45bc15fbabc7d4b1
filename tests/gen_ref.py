"""Reference sampler in plain torch: TEST INFRASTRUCTURE ONLY (never imported by the product).

Restates one step of the sampling loop the reference engine runs (soulxpodcast/models/modules/sampler.py:136-189 with the
``SamplingParams`` of soulxpodcast/config.py:107-118), i.e. HF's processors in generate's order plus repetition-aware
sampling, as include/sd_hip.h ``sd_sample_step`` states it:

  1 repetition penalty over the GENERATED tokens (score < 0 ? score * p : score / p), each distinct token once;
  2 EOS = -inf while fewer than ``min_new_tokens`` were generated;   3 score / temperature;
  4 top-k: exactly k survivors, ties at the k-th value to the LOWEST index (HF keeps every tie of the k-th value; the two
    agree whenever the k-th value is unique);   5 top-p (HF's rule): walking up from the smallest probability a candidate
    is dropped while the cumulative mass is <= 1 - top_p, the largest always stays;
  6 inverse CDF over the survivors in descending order (ties: lowest index first): token j iff cdf[j-1] <= u < cdf[j].
Full-vocabulary draws (the RAS fallback on the raw logits, and top_k = 0) walk the vocabulary in index order.

Steps 1-3 are taken in fp32 (HF casts the logits to fp32 and works there, sampler.py:136); everything from the softmax on
is fp64, so that the CDF boundaries the GPU tests keep their uniforms away from are exact.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch


@dataclass
class Params:
    do_sample: bool = True
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    min_new_tokens: int = 0
    eos_token_id: int | None = None
    pad_token_id: int = 0
    use_ras: bool = False
    win_size: int = 25
    tau_r: float = 0.2


REFERENCE = dict(do_sample=True, temperature=0.6, top_k=100, top_p=0.9, repetition_penalty=1.25, use_ras=True, win_size=25,
                 tau_r=0.2)  # soulxpodcast/config.py:107-118


def scores_fp32(logits_row, generated, p: Params):
    """Steps 1-2 (and 3 when sampling) on one row, fp32 [V]."""
    s = logits_row.detach().to(torch.float32).clone()
    if p.repetition_penalty != 1.0 and len(generated):
        idx = torch.as_tensor(sorted(set(int(t) for t in generated)), dtype=torch.int64)
        pen = torch.tensor(p.repetition_penalty, dtype=torch.float32)
        g = s[idx]
        s[idx] = torch.where(g < 0, g * pen, g / pen)
    if p.eos_token_id is not None and len(generated) < p.min_new_tokens:
        s[p.eos_token_id] = -math.inf
    if p.do_sample:
        s = s / torch.tensor(p.temperature, dtype=torch.float32)
    return s


def order_desc(s):
    """Indices by descending score, ties to the lowest index."""
    return torch.sort(s.double(), descending=True, stable=True).indices


def candidates(logits_row, generated, p: Params):
    """-> (ids int64 [n], probs fp64 [n], info): the survivors of steps 1-5 in draw order with their renormalised
    probabilities.  info["top_p_margin"]: distance of the nearest top-p decision from its boundary."""
    s = scores_fp32(logits_row, generated, p)
    if p.top_k <= 0:   # no top-k (only with top_p = 1): the whole row, drawn in INDEX order like every full-vocabulary draw
        assert p.top_p >= 1.0, "top_p < 1 works on the sorted top-k candidates"
        return torch.arange(s.numel()), torch.softmax(s.double(), -1), {"top_p_margin": math.inf, "scores": s}
    order = order_desc(s)[:p.top_k]
    sc = s[order].double()
    pr = torch.softmax(sc, -1)
    keep, margin = order.numel(), math.inf
    if p.top_p < 1.0:
        drop = 1.0 - p.top_p
        tail = torch.flip(torch.cumsum(torch.flip(pr, [0]), 0), [0])   # tail[j] = sum of pr[j:]
        margin = float((tail - drop).abs().min())
        keep = max(1, int((tail > drop).sum()))                         # tail is non-increasing in j
    ids, pr = order[:keep], pr[:keep]
    return ids, pr / pr.sum(), {"top_p_margin": margin, "scores": s}


def cdf(probs):
    return torch.cumsum(probs.double(), 0)


def draw(ids, probs, u):
    c = cdf(probs)
    j = int((c <= u).sum())
    return int(ids[min(j, ids.numel() - 1)])


def ras_triggered(seq_row, cand, win_size, tau_r):
    """sampler.py:146-147: occurrences of the candidate in the last ``win_size`` tokens of the whole sequence, plus one,
    reach win_size * tau_r."""
    window = list(seq_row)[-win_size:] if win_size > 0 else []
    return sum(int(t) == int(cand) for t in window) + 1 >= win_size * tau_r


def processed_probs(logits_row, generated, p: Params):
    """The processed distribution over the whole vocabulary, fp64 [V] (zeros outside the survivors)."""
    ids, pr, _ = candidates(logits_row, generated, p)
    out = torch.zeros(logits_row.numel(), dtype=torch.float64)
    out[ids] = pr
    return out


def sample_row(logits_row, seq_row, prompt_len, u0, u1, p: Params):
    """One row's next token.  seq_row: every token so far (prompt + generated).  -> (token, info); info holds the CDFs the
    draws used ("cdf_cand", "cdf_final": fp64 tensors) and "ras" (None / False / True)."""
    generated = list(seq_row)[prompt_len:]
    info = {"ras": None, "cdf_cand": None, "cdf_final": None, "top_p_margin": math.inf}
    if not p.do_sample:
        s = scores_fp32(logits_row, generated, p)
        return int(order_desc(s)[0]), info
    ids, pr, ci = candidates(logits_row, generated, p)
    info["top_p_margin"] = ci["top_p_margin"]
    if p.use_ras:
        info["cdf_cand"] = cdf(pr)
        cand = draw(ids, pr, u0)
        info["ras"] = bool(ras_triggered(seq_row, cand, p.win_size, p.tau_r))
        if info["ras"]:
            raw = torch.softmax(logits_row.detach().double(), -1)
            info["cdf_final"] = cdf(raw)
            return draw(torch.arange(raw.numel()), raw, u1), info
    info["cdf_final"] = cdf(pr)
    return draw(ids, pr, u1), info


def step(logits, seqs, prompt_lens, finished, u, p: Params):
    """The batch step with the state update of sd_sample_step: seqs (list of token lists) and finished (list of bools) are
    updated in place.  -> (next tokens, infos)."""
    out, infos = [], []
    for b in range(len(seqs)):
        if finished[b]:
            out.append(p.pad_token_id)
            infos.append(None)
            continue
        tok, info = sample_row(logits[b], seqs[b], prompt_lens[b], float(u[b][0]), float(u[b][1]), p)
        seqs[b].append(tok)
        if p.eos_token_id is not None and tok == p.eos_token_id:
            finished[b] = True
        out.append(tok)
        infos.append(info)
    return out, infos


def boundary_distance(c, u):
    """Distance of u from the nearest boundary of the CDF c (0 counts as a boundary)."""
    if c is None:
        return math.inf
    return float(torch.cat([torch.zeros(1, dtype=torch.float64), c.double()]).sub(u).abs().min())


def pick_uniform(c, gen, margin):
    """A uniform in [0,1) at least ``margin`` away from every boundary of the CDF c, drawn reproducibly from ``gen``."""
    for _ in range(1000):
        u = float(torch.rand((), generator=gen, dtype=torch.float64))
        u = float(torch.tensor(u, dtype=torch.float32))   # the value the kernel will see
        if u < 1.0 and boundary_distance(c, u) >= margin:
            return u
    raise RuntimeError("no uniform found away from the CDF boundaries")
