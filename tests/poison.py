"""Dirty memory for the wrappers: every buffer ``torch.empty`` / ``torch.empty_like`` hands out, filled with one byte.

Apart from the training ``workspace``, ``rowmap`` and ``lazy_state`` (include/anirec.h: "zero before first use") no
buffer of the library may need any particular content on entry.  The caching allocator often returns a fresh, zeroed
block, so a missing initialisation reads as 0 and passes; ``poisoned`` takes that luck away for the one wrapper call
it surrounds.  A plain helper module, imported by the tests the way ``recs_fixture`` is.

The patterns, as the kernels would read them:

    byte   int32           fp32     fp16   fp64
    0x00   0               0        0      0        the baseline: what a fresh block holds
    0x3F   1 061 109 567   0.747    1.81   4.8e-4   a plausible stale threshold or score
    0x7F   2 139 062 143   3.4e38   NaN    1.4e306  a counter that is already full
    0xFF   -1              NaN      NaN    NaN      the library's own -1 / NaN padding
"""
import contextlib

import torch

PATTERNS = (0x00, 0x3F, 0x7F, 0xFF)
# the order the GPU tests run them in, mildest first: a counter that reads 2 139 062 143 is the likeliest to index
# out of bounds, so it runs when the others have passed
ORDER = (0x00, 0x3F, 0xFF, 0x7F)
assert sorted(ORDER) == sorted(PATTERNS)


def fill(t, byte):
    """Every byte of ``t`` becomes ``byte``; returns ``t``."""
    if t.numel():
        t.view(torch.uint8).fill_(byte)
    return t


@contextlib.contextmanager
def poisoned(byte, log):
    """For the duration of the block ``torch.empty`` and ``torch.empty_like`` return tensors whose every byte is
    ``byte``; the byte count of each is appended to ``log``.  The originals are back on exit, normal or not.
    Use it around the one wrapper call under test."""
    empty, empty_like = torch.empty, torch.empty_like

    def dirty_empty(*a, **kw):
        t = fill(empty(*a, **kw), byte)
        log.append(t.numel() * t.element_size())
        return t

    def dirty_empty_like(*a, **kw):
        t = fill(empty_like(*a, **kw), byte)
        log.append(t.numel() * t.element_size())
        return t

    torch.empty, torch.empty_like = dirty_empty, dirty_empty_like
    try:
        yield log
    finally:
        torch.empty, torch.empty_like = empty, empty_like
