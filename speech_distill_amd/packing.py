"""Token-budget bins for padding-free distillation: which samples share one packed row.

``pack_bfd_indices`` is the best-fit-decreasing rule of ``stage1.pack_bfd`` stated over lengths: it returns sample
INDICES, because a distillation sample is a student sequence with its teacher twin (and perhaps its top-K block), not one
list of ids.  ``PackedView`` shows a dataset bin by bin; ``ProcessedDataCollator(padding_free=True)`` flattens a bin's
samples in order.  ``per_device_train_batch_size`` then counts bins."""
import bisect
from typing import List, Sequence


def pack_bfd_indices(lengths: Sequence[int], max_tokens: int) -> List[List[int]]:
    """Samples taken longest first (ties: lower index first); each goes into the open bin with the least room that still
    fits it, else into a new bin.  Returns the bins in creation order, each a list of sample indices in insertion order:
    the bins of ``stage1.pack_bfd`` on sequences of these lengths.  Zero-length samples are left out.  A sample longer
    than ``max_tokens`` is a ValueError: it cannot be truncated without its teacher twin."""
    if max_tokens <= 0:
        raise ValueError("max_tokens must be positive")
    lengths = [int(n) for n in lengths]
    for i, n in enumerate(lengths):
        if n > max_tokens:
            raise ValueError(f"sample {i} has {n} tokens, more than max_tokens={max_tokens}: a distillation sample cannot "
                             "be truncated without its teacher twin")
    order = sorted((i for i, n in enumerate(lengths) if n > 0), key=lambda i: (-lengths[i], i))
    bins: List[List[int]] = []
    free: List[tuple] = []  # sorted (room left, bin index)
    for i in order:
        n = lengths[i]
        k = bisect.bisect_left(free, (n, -1))
        if k == len(free):
            bins.append([i])
            bisect.insort(free, (max_tokens - n, len(bins) - 1))
        else:
            room, b = free.pop(k)
            bins[b].append(i)
            bisect.insort(free, (room - n, b))
    return bins


class PackedView:
    """``dataset`` seen bin by bin: item ``i`` is ``{"samples": [dataset[j] for j in bins[i]]}``."""

    def __init__(self, dataset, bins: Sequence[Sequence[int]]):
        self.dataset = dataset
        self.bins = [list(b) for b in bins]

    def __len__(self):
        return len(self.bins)

    def __getitem__(self, i):
        return {"samples": [self.dataset[j] for j in self.bins[i]]}
