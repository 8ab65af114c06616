"""Host side of the packed variable-length lookup (`scone_embed_varlen`, `embed_tokens(..., cu_seqlens=...)`): the boundary
validator, the packing helper and the C entry point's argument check.  Nothing here needs a GPU."""

import numpy as np
import pytest
import torch

from scone_amd import EmbeddingCache, _lib
from scone_amd.hip_backend import check_cu_seqlens


def test_validator_accepts_a_proper_array_with_empty_sequences():
    cu = check_cu_seqlens([0, 0, 3, 3, 3, 7, 7], 7)
    assert cu.dtype == np.int32 and cu.flags["C_CONTIGUOUS"] and cu.tolist() == [0, 0, 3, 3, 3, 7, 7]
    assert check_cu_seqlens(np.array([0, 5], dtype=np.int64), 5).tolist() == [0, 5]
    assert check_cu_seqlens(torch.tensor([0, 2, 2, 4], dtype=torch.int32), 4).tolist() == [0, 2, 2, 4]
    assert check_cu_seqlens([0], 0).tolist() == [0]              # no sequences, no tokens
    assert check_cu_seqlens([0, 0, 0], 0).tolist() == [0, 0, 0]  # only empty sequences


@pytest.mark.parametrize("cu,total,what", [
    ([1, 3, 7], 7, "start at 0"),
    ([0, 4, 3, 7], 7, "not decrease"),
    ([0, 3, 6], 7, "end at"),
    ([0, 3, 8], 7, "end at"),
    ([], 0, "1-D"),
    ([[0, 7]], 7, "1-D"),
    ([0.0, 7.0], 7, "integers"),
])
def test_validator_rejects(cu, total, what):
    with pytest.raises(ValueError, match=what):
        check_cu_seqlens(cu, total)


def test_pack_sequences_round_trips():
    seqs = [[], [5], [1, 2, 3], [], [], [7, 8], np.array([9, 10, 11, 12]), torch.tensor([13]), []]
    ids, cu = EmbeddingCache.pack_sequences(seqs)
    assert ids.dtype == torch.int32 and cu.dtype == torch.int32 and not ids.is_cuda and not cu.is_cuda
    assert cu.tolist() == [0, 0, 1, 4, 4, 4, 6, 10, 11, 11] and ids.shape == (11,)
    back = [ids[cu[s]:cu[s + 1]].tolist() for s in range(len(seqs))]
    assert back == [list(map(int, np.asarray(s).reshape(-1))) for s in seqs]
    assert check_cu_seqlens(cu, ids.shape[0]).tolist() == cu.tolist()
    ids0, cu0 = EmbeddingCache.pack_sequences([])
    assert ids0.shape == (0,) and cu0.tolist() == [0]


def test_c_entry_point_refuses_a_null_handle():
    lib = _lib.lib()
    rc = lib.scone_embed_varlen(None, None, None, 0, 0, None, 0, None, 0, None, _lib.REDUCE_MEAN, None, _lib.DT_F32, None)
    assert rc == _lib.EINVAL
