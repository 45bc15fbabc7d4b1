"""CPU checks of padding-free packing: the Stage-1 padding-free collator equals HF DataCollatorWithFlattening, the packed
segment rule equals HF's find_packed_sequence_indices, and the CLI flag / refused combination."""
import os
import sys

import pytest
import torch

from conftest import ROOT


def _batches(seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(6):
        bins = []
        for _ in range(int(torch.randint(1, 5, (1,), generator=g))):
            n = int(torch.randint(1, 6, (1,), generator=g))
            bins.append({"documents": [torch.randint(0, 900, (int(torch.randint(1, 40, (1,), generator=g)),),
                                                     generator=g).tolist() for _ in range(n)]})
        out.append(bins)
    out.append([{"documents": [[7], [8], [9, 10]]}, {"documents": [[11]]}])  # documents of one token
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_padding_free_collator_equals_hf_flattening(seed):
    from transformers import DataCollatorWithFlattening
    from speech_distill_amd.stage1 import Stage1Collator
    hf = DataCollatorWithFlattening(return_flash_attn_kwargs=True, separator_id=-100)
    ours = Stage1Collator(pad_token_id=3, padding_free=True)
    for bins in _batches(seed):
        docs = [d for b in bins for d in b["documents"]]
        want = hf([{"input_ids": d} for d in docs])
        got = ours(bins)
        assert set(got) == set(want) and "attention_mask" not in got
        for k, w in want.items():
            if torch.is_tensor(w):
                assert got[k].dtype == w.dtype and torch.equal(got[k], w), k
            else:
                assert type(got[k]) is type(w) and got[k] == w, k


def _hf_segments(pos):
    from transformers.masking_utils import find_packed_sequence_indices
    seg = find_packed_sequence_indices(pos)
    return torch.zeros_like(pos) if seg is None else seg


def _our_segments(pos):
    from speech_distill_amd.ops import packed_segments
    cu, pmax, pmin = packed_segments(pos)
    assert int(cu[0]) == 0 and int(cu[-1]) == pos.numel() and pmax == int(pos.max()) and pmin == int(pos.min())
    flat = torch.zeros(pos.numel(), dtype=torch.long)
    for s in range(cu.numel() - 1):
        flat[int(cu[s]):int(cu[s + 1])] = s
    per_row = flat.view(pos.shape)
    return per_row - per_row[:, :1]  # HF numbers the segments of every row from 0


@pytest.mark.parametrize("pos", [
    [[0, 1, 2, 0, 1, 0, 0, 1, 2, 3]],               # ordinary packing, a one-token document
    [[3, 4, 5, 0, 1, 2, 7, 8]],                      # positions that do not start at 0
    [[0, 0, 0, 0]],                                  # repeated zeros: four documents
    [[0, 1, 2, 3], [5, 6, 0, 1]],                    # B > 1 (rows never share a document)
    [[0, 1, 2, 3, 4]],                               # one document
    [[2, 1, 0, 5, 6]],                               # descending runs
])
def test_segment_rule_equals_hf(pos):
    pos = torch.tensor(pos)
    assert torch.equal(_our_segments(pos), _hf_segments(pos))


def test_segment_rule_flattens_rows():
    from speech_distill_amd.ops import packed_segments
    cu, _, _ = packed_segments(torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]]))  # consecutive across rows: still two documents
    assert cu.tolist() == [0, 4, 8]


def test_stage1_flag_and_refused_combination():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import importlib
    cli = importlib.import_module("stage1")
    assert cli.parse_args(["--output_dir", "x"]).padding_free is False
    assert cli.parse_args(["--output_dir", "x", "--padding_free"]).padding_free is True
    from speech_distill_amd.stage1 import Stage1Collator
    c = Stage1Collator()
    assert c.padding_free is False
    out = c([{"documents": [[1, 2, 3], [4]]}])
    assert set(out) == {"input_ids", "attention_mask", "labels"} and out["input_ids"].shape == (2, 3)
    with pytest.raises(ValueError):
        Stage1Collator(pad_to_multiple_of=8, padding_free=True)
