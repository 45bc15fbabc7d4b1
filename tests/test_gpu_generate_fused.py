"""-m gpu: ``decode_attention="fused"`` through the public generation entries (generation.py, engine.py): the tokens are
those of the default "split", bit for bit -- ``generate`` (greedy and sampled, ragged prompts), a two-turn session over bf16
pages with a fork, and the request engine in skinny mode over MXFP8 pages."""
import pytest
import torch

from gpu_util import dev
from test_gpu_generate import _mask, _model, _prompts

pytestmark = pytest.mark.gpu

MODES = ("split", "fused")
LENS = [24, 17, 9]


@pytest.fixture(scope="module")
def model():
    m, _, _ = _model("twin")
    return m.eval().requires_grad_(False)


@pytest.mark.parametrize("kw", [dict(do_sample=False, decode_kernels="tile"), dict(do_sample=False, decode_kernels="skinny"),
                                dict(do_sample=True, top_k=20, temperature=0.9, seed=3, decode_kernels="skinny"),
                                dict(do_sample=True, top_k=50, top_p=0.9, repetition_penalty=1.2, seed=5,
                                     decode_kernels="wide")],
                         ids=["greedy-tile", "greedy-skinny", "sampled-skinny", "sampled-wide"])
def test_generate_tokens_do_not_depend_on_decode_attention(model, kw):
    ids = _prompts()[0][:3]
    am = _mask(LENS, 24)
    out = {mode: model.generate(ids.to(dev()), attention_mask=am.to(dev()), max_new_tokens=24, decode_attention=mode, **kw)
           for mode in MODES}
    assert torch.equal(out["fused"], out["split"])
    assert out["split"].shape == (3, 48)


def _two_turns(model, mode):
    """Turn 1 on two rows (the prompts end inside the first page, the turn crosses into the second), then a fork of row 0
    into two continuations that share its full first page, and turn 2 on the fork and on the source."""
    order = torch.randperm(12, generator=torch.Generator().manual_seed(1)).tolist()
    pool = model.kv_page_pool(12, order=order)
    pool.buffer.fill_(0x3C)
    g = torch.Generator().manual_seed(8)
    p1 = torch.randint(0, 640, (2, 250), generator=g).to(dev())
    p2 = torch.randint(0, 640, (2, 5), generator=g).to(dev())
    kw = dict(do_sample=True, top_k=20, temperature=0.9)
    s = model.start_session(2, 512, pool=pool, decode_attention=mode, decode_kernels="skinny")
    assert s.decode_attention == mode
    t1 = s.generate(p1, attention_mask=_mask([250, 243], 250).to(dev()), max_new_tokens=10, seed=1, **kw)
    f = s.fork([0, 0])
    assert f.decode_attention == mode and f.decoder.fused == (mode == "fused")
    t2f = f.generate(p2, max_new_tokens=8, seed=2, **kw)
    t2s = s.generate(p2, max_new_tokens=8, seed=3, **kw)
    buf = pool.buffer.clone()
    f.close(), s.close()
    return t1, t2f, t2s, buf


def test_two_turn_paged_session_with_a_fork(model):
    got, want = _two_turns(model, "fused"), _two_turns(model, "split")
    for a, b, name in zip(got, want, ("turn 1", "turn 2 of the fork", "turn 2 of the source", "the pool")):
        assert torch.equal(a, b), name
    assert not torch.equal(want[1][0], want[1][1]) or not torch.equal(want[1][0], want[2][0])   # (the turns sampled)


REQUESTS = [(0, 24, 11, 9), (1, 17, 12, 40), (2, 9, 13, 3), (3, 1, 14, 25), (0, 12, 15, 17), (2, 24, 16, 6)]  # row, T, seed, budget


def _serve(model, mode):
    pool = model.kv_page_pool(8, kv_dtype="mxfp8")
    eng = model.generation_engine(pool, max_batch=4, decode_kernels="skinny", decode_attention=mode)
    assert eng.decoder.fused == (mode == "fused")
    ids = _prompts()[0]
    rids = [eng.submit(ids[row, :T].to(dev()), max_new_tokens=budget, seed=seed, do_sample=True, top_k=20, temperature=0.9)
            for row, T, seed, budget in REQUESTS]
    done = eng.run()
    assert sorted(done) == sorted(rids)
    out = [eng.result(r) for r in rids]
    eng.close()
    return out


def test_engine_of_four_rows_serves_six_requests_over_mxfp8_pages(model):
    got, want = _serve(model, "fused"), _serve(model, "split")
    assert [t.numel() for t in want] == [r[3] for r in REQUESTS]
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
