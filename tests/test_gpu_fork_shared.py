"""-m gpu: ``shared_kv_reads=True`` through the public generation entries (generation.py): a fork's tokens, logits and
pool bytes are those of the same fork without the keyword, bit for bit.

The model is the tiny MXFP8-capable shape of tests/test_gpu_mx.py.  Two source rows are prefilled with 299 of their 300
prompt tokens, so a fork shares the one full page of its source and copies the partial one; the continuations then take two
sampled turns (repetition-aware sampling and the repetition penalty on, a seed).  ``fork([0] * 8)`` is one sharing set that
fills a group; ``fork([0, 0, 0, 1, 1])`` is two sets inside one group."""
import pytest
import torch

from gpu_util import dev
from test_gpu_mx import SHP, _model, _weights

pytestmark = pytest.mark.gpu

SAMPLING = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.25, use_ras=True, win_size=10,
                tau_r=0.2)
MODES = [("skinny", "bf16"), ("wide", "bf16"), ("skinny", "mxfp8")]     # ("wide", "mxfp8") does not exist


@pytest.fixture(scope="module")
def model():
    import speech_distill_amd as sda
    sda.load_lib()
    return _model(sda, _weights(9)[1])


def _prompt():
    g = torch.Generator().manual_seed(21)
    return torch.randint(0, SHP[0], (2, 300), generator=g).to(dev()), torch.randint(0, SHP[0], (8, 5), generator=g).to(dev())


def _source(model, kernels, weights, pages):
    pool = model.kv_page_pool(24, kv_dtype=pages)
    pool.buffer.fill_(0x3C)
    s = model.start_session(2, 1024, pool=pool, decode_kernels=kernels, weight_dtype=weights)
    assert s.shared_kv_reads is False and s.decoder.shared is False
    s.extend(_prompt()[0][:, :299].contiguous())
    return pool, s


def _two_turns(model, kernels, weights, pages, rows, shared):
    pool, s = _source(model, kernels, weights, pages)
    p1, p2 = _prompt()
    f = s.fork(rows, shared_kv_reads=shared)
    assert f.shared_kv_reads is bool(shared) and f.decoder.shared is bool(shared)
    assert all(f.decoder.pages.rows[i][0] == s.decoder.pages.rows[r][0] for i, r in enumerate(rows))   # the shared page
    idx = torch.tensor(rows, device=dev())
    t1 = f.generate(p1[idx, 299:], max_new_tokens=7, seed=1, **SAMPLING)
    t2 = f.generate(p2[:len(rows)], max_new_tokens=6, seed=2, **SAMPLING)
    g = f.fork([0, 1])            # None inherits
    assert g.shared_kv_reads is bool(shared)
    buf = pool.buffer.clone()
    g.close(), f.close(), s.close()
    return t1, t2, buf


@pytest.mark.parametrize("rows", [[0] * 8, [0, 0, 0, 1, 1]], ids=["fork8", "fork3+2"])
@pytest.mark.parametrize("pages", ["bf16", "mxfp8"])
@pytest.mark.parametrize("kernels,weights", MODES, ids=["skinny", "wide", "skinny-mxw"])
def test_two_turns_of_a_fork_sample_the_same_tokens(model, kernels, weights, pages, rows):
    got = _two_turns(model, kernels, weights, pages, rows, True)
    want = _two_turns(model, kernels, weights, pages, rows, False)
    for a, b, name in zip(got, want, ("turn 1", "turn 2", "the pool")):
        assert torch.equal(a, b), name
    assert want[0].shape == (len(rows), 7) and want[1].shape == (len(rows), 6)
    assert not torch.equal(want[0][0], want[0][1])      # (the continuations of one row were sampled apart)


@pytest.mark.parametrize("pages", ["bf16", "mxfp8"])
def test_hand_driven_steps_give_the_same_logits_and_cache_rows(model, pages):
    """Three ``Decoder.step`` calls on the decoders of two forks of five rows (tile sequence): after each, the logits and
    every row's gathered cache rows of every layer are equal."""
    runs = []
    for shared in (True, False):
        pool, s = _source(model, "tile", "bf16", pages)
        f = s.fork([0, 0, 1, 0, 1], shared_kv_reads=shared)
        f.decoder.reserve([303] * 5)
        runs.append((pool, s, f))
    g = torch.Generator().manual_seed(5)
    for step in range(3):
        ids = torch.randint(0, SHP[0], (5,), generator=g).to(dev())
        pos = torch.full((5,), 299 + step, dtype=torch.int32, device=dev())
        (a, b) = (f.decoder.step(ids, pos, 300 + step).clone() for _, _, f in runs)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), step
        for layer in range(SHP[3]):
            for row in range(5):
                x, y = (f.decoder.gather_raw(layer, row, 300 + step) for _, _, f in runs)
                assert all(torch.equal(u, v) for u, v in zip(x, y)), (step, layer, row)
    for pool, s, f in runs:
        f.close(), s.close()
