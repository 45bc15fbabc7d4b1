"""CPU checks around multi-turn generation: the ``turns`` format of scripts/generate.py and the visibility rule the GPU
tests of sd_attn_extend / sd_kvcache_store_at use as their reference (tests/extend_ref.py)."""
import importlib.util
import json
import os

import pytest
import torch

import attn_ref as A
import extend_ref as E
from conftest import ROOT

PASTS = (0, 1, 63, 64, 65, 256)
NEWS = (1, 2, 63, 64, 65, 129)


def _script():
    spec = importlib.util.spec_from_file_location("sd_generate_script", os.path.join(ROOT, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_read_prompts_takes_turns_and_plain_prompts(tmp_path):
    G = _script()
    f = tmp_path / "p.jsonl"
    f.write_text("\n".join([json.dumps({"turns": [[1, 2, 3], [4], [5, 6]]}), json.dumps({"input_ids": [7, 8]}), "",
                            json.dumps([9]), json.dumps({"turns": [[10], [11, 12], [13]]}),
                            json.dumps({"turns": [[14, 15]]})]) + "\n")
    got = G.read_prompts(str(f))
    assert got == [[[1, 2, 3], [4], [5, 6]], [[7, 8]], [[9]], [[10], [11, 12], [13]], [[14, 15]]]
    # the dialogues of a batch take their turns together: equal turn counts only, at most batch_size of them
    batches = G.batches_by_turn_count(got, 2)
    assert [idx for idx, _ in batches] == [[0, 3], [1, 2], [4]]
    assert all(len({len(d) for d in ds}) == 1 for _, ds in batches)
    assert sorted(i for idx, _ in batches for i in idx) == list(range(5))
    ids, mask = G.right_pad([[1, 2, 3], [4]], 0)
    assert ids.tolist() == [[1, 2, 3], [4, 0, 0]] and mask.tolist() == [[1, 1, 1], [1, 0, 0]]


@pytest.mark.parametrize("row", [{"turns": [[1], []]}, {"turns": []}, {"input_ids": []}, []])
def test_read_prompts_rejects_an_empty_turn(tmp_path, row):
    f = tmp_path / "p.jsonl"
    f.write_text(json.dumps(row) + "\n")
    with pytest.raises(ValueError):
        _script().read_prompts(str(f))


def test_visibility_rule_equals_the_causal_mask_of_the_whole_sequence():
    """Block row t of (past, new) sees what row past + t of a causal sequence of past + new tokens sees (attn_ref's mask
    with kv_len = past + new), on the (past, new) grid of the GPU test, with T = new and with T padded by 7 rows: a
    padding row sees every key of the sequence, as a row >= kv_len does there."""
    for past in PASTS:
        for new in NEWS:
            n, cap = past + new, 385
            full = A.visible_mask(1, n + 7, kv_len=[n])[0]               # [n+7, n+7]
            for T in (new, new + 7):
                vis = E.extend_visible([past], [new], T, cap)[0]        # [T, cap]
                assert not bool(vis[:, n:].any())
                assert torch.equal(vis[:, :n], full[past:past + T, :n]), (past, new, T)
                st = E.stored_slots([past], [new], T, cap)[0]
                assert int(st.sum()) == new and all(bool(st[t, past + t]) for t in range(new))


def test_visibility_rule_clamps_and_handles_empty_rows():
    vis = E.extend_visible([0, 5, 14, 16, 20, -3], [0, 0, 5, 3, 1, 2], 4, 16)
    assert not bool(vis[0].any())                                         # nothing cached, nothing new
    assert bool(vis[1, :, :5].all()) and not bool(vis[1, :, 5:].any())    # new = 0: every row over the 5 cached keys
    assert vis[2].sum(-1).tolist() == [15, 16, 16, 16]                    # new clamped to cap - past = 2
    assert bool(vis[3].all()) and bool(vis[4].all())                      # past clamped to cap: all 16 keys, no new one
    assert vis[5].sum(-1).tolist() == [1, 2, 2, 2]                        # past clamped to 0
    st = E.stored_slots([0, 5, 14, 16, 20, -3], [0, 0, 5, 3, 1, 2], 4, 16)
    assert st.sum((1, 2)).tolist() == [0, 0, 2, 0, 0, 2]
    o, lse = E.attend(torch.randn(1, 2, 2 * 128), torch.randn(1, 4, 128), torch.randn(1, 4, 128),
                      torch.zeros(1, 2, 4, dtype=torch.bool), 2, 1)
    assert float(o.abs().max()) == 0.0 and bool(torch.isinf(lse).all()) and bool((lse < 0).all())
