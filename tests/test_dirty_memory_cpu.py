"""The poisoning helper itself (tests/poison.py), on CPU tensors: the bytes arrive, torch is put back."""
import numpy as np
import pytest
import torch

import poison

# what poison.py's table says each byte reads as (int32; fp32 and fp64 as their bit patterns)
AS_INT32 = {0x00: 0, 0x3F: 1_061_109_567, 0x7F: 2_139_062_143, 0xFF: -1}


def test_patterns_and_their_gpu_order():
    assert poison.PATTERNS == (0x00, 0x3F, 0x7F, 0xFF)
    assert poison.ORDER == (0x00, 0x3F, 0xFF, 0x7F)           # mildest first, the full counter last


@pytest.mark.parametrize("byte", poison.PATTERNS)
def test_every_pattern_arrives_in_int32_fp32_and_fp64_tensors(byte):
    log = []
    with poison.poisoned(byte, log):
        i = torch.empty(3, 5, dtype=torch.int32)
        f = torch.empty(7, dtype=torch.float32)
        d = torch.empty_like(torch.zeros(2, 3, dtype=torch.float64))
        e = torch.empty(0, 4, dtype=torch.int32)
    assert (i == AS_INT32[byte]).all() and i.shape == (3, 5)
    assert (f.view(torch.int32) == AS_INT32[byte]).all()
    assert (d.numpy().view(np.uint8) == byte).all() and d.shape == (2, 3) and d.dtype == torch.float64
    fv, dv = f.numpy(), d.numpy()
    if byte == 0x00:
        assert (fv == 0).all() and (dv == 0).all()
    elif byte == 0x3F:
        assert abs(float(fv[0]) - 0.747) < 1e-3 and abs(float(dv[0, 0]) - 4.8e-4) < 1e-5
    elif byte == 0x7F:
        assert float(fv[0]) > 3.3e38 and np.isfinite(fv).all() and float(dv[0, 0]) > 1e306
    else:
        assert np.isnan(fv).all() and np.isnan(dv).all()
    assert log == [60, 28, 48, 0]                             # the byte count of each tensor, in order
    assert e.numel() == 0


def test_torch_is_put_back_after_normal_exit_and_after_an_exception():
    empty, empty_like = torch.empty, torch.empty_like
    with poison.poisoned(0x7F, []):
        assert torch.empty is not empty and torch.empty_like is not empty_like
    assert torch.empty is empty and torch.empty_like is empty_like
    with pytest.raises(KeyError):
        with poison.poisoned(0xFF, []):
            raise KeyError("inside the block")
    assert torch.empty is empty and torch.empty_like is empty_like


def test_other_allocating_calls_are_not_touched():
    """nonzero, sort, cat, unique and indexing inside the block give what they give outside it"""
    x = torch.tensor([3, 0, 2, 0, 3, 1])
    log = []
    with poison.poisoned(0xFF, log):
        got = (torch.nonzero(x).flatten(), torch.sort(x)[0], torch.cat([x, x]), torch.unique(x), x[x > 1])
    want = (torch.nonzero(x).flatten(), torch.sort(x)[0], torch.cat([x, x]), torch.unique(x), x[x > 1])
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and log == []
