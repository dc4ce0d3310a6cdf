"""Batching over in-memory tensors (the caller of integer-array indexing).

`Dataset` follows the reference's `lightgrad/data.py:7-32` in behaviour - same constructor, `n`, `shuffle()`,
indexing, iteration and `len()`, and the same consumption of numpy's global RNG (one `np.random.permutation(n)` per
epoch), so a seeded epoch yields the same batches - and is backend-agnostic: with `HipTensor`s the permutation is
applied by a device gather (`t[perm]`, csrc/index.hip) and a batch is a slice view + dense copy, nothing goes through
the host.  The reference's `MNIST` subclass downloads its files (data.py:36-48); there is no network here, so it is
not restated - build a `Dataset` from arrays instead.
"""
from math import ceil
import numpy as np
from .autograd import AbstractTensor


class Dataset(object):

    def __init__(self, tensors, shuffle: bool = True, batchsize: int = 8) -> None:
        self._columns = tuple(tensors)
        if not self._columns or not all(isinstance(t, AbstractTensor) for t in self._columns):
            raise TypeError("Dataset needs at least one tensor")
        rows = {t.shape[0] for t in self._columns}
        assert len(rows) == 1, "all tensors of a Dataset must agree in their first dimension (got %s)" % sorted(rows)
        self._reshuffle, self._batch = bool(shuffle), int(batchsize)

    @property
    def n(self) -> int:
        return self._columns[0].shape[0]

    @property
    def tensors(self) -> tuple:
        return self._columns

    def shuffle(self) -> None:
        order = np.random.permutation(self.n)
        self._columns = tuple(column[order].detach() for column in self._columns)

    def __getitem__(self, idx) -> tuple:
        return tuple(column[idx, ...].detach() for column in self._columns)

    def __len__(self) -> int:
        return ceil(self.n / self._batch)

    def __iter__(self):
        if self._reshuffle:
            self.shuffle()
        for first in range(0, self.n, self._batch):
            yield self[first:first + self._batch]


def mask_tokens(ids, p: float = 0.15, mask_token_id: int = 103, vocab_size: int = 30522, special_ids=(), ignore_index: int = -100) -> tuple:
    """BERT's token masking for the masked-LM objective: `ids.mlm_mask(...)` -> (masked_ids, labels).  Each id that is none of
    `special_ids` is selected with probability p; a selected one becomes the label of its position and is replaced by
    `mask_token_id` (80 %), a uniform token of the vocabulary (10 %) or left as it is (10 %); every other position gets the label
    `ignore_index` - what `loss.cross_entropy(..., ignore_index=)` leaves out.  Drawn from the backend's counter-based stream
    (lightgrad_amd/random.py; one call), on the device for HipTensors: inside a captured graph every replay masks a fresh batch.
    The defaults are those of the public BERT vocabulary ([MASK] = 103)."""
    if not isinstance(ids, AbstractTensor):
        raise TypeError("mask_tokens needs a tensor of int32 / int64 ids")
    return ids.mlm_mask(p, mask_token_id, vocab_size, special_ids=special_ids, ignore_index=ignore_index)


def next_token_labels(ids, ignore_index: int = -100):
    """the labels of the causal-LM objective: `ids.next_token_labels(...)` - `ids` shifted left by one along the last axis (position
    i is to predict token i + 1) with `ignore_index` in the last column, which has nothing to predict and which
    `loss.cross_entropy(..., ignore_index=)` leaves out.  Same dtype and shape; on the device for HipTensors, with no host read:
    inside a captured graph every replay shifts what the ids hold then."""
    if not isinstance(ids, AbstractTensor):
        raise TypeError("next_token_labels needs a tensor of int32 / int64 ids")
    return ids.next_token_labels(ignore_index)
