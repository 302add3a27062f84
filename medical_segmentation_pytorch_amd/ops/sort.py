"""Segmented radix sort on the device (``csrc/sort.hip``).

:func:`sort_segments` sorts every row of an fp32 ``[Q, P]`` tensor on its own, descending by the key's uint32
bit pattern (numeric order for non-negative floats; negative or NaN keys are simply ordered by their bits), and
stable: equal keys keep ascending index.  For non-negative keys it is
``torch.sort(keys, dim=1, descending=True, stable=True)`` bit for bit.  An LSD radix sort with 8-bit digits:
per pass a block histogram, a scan of the (digit-major, block-minor) table and a scatter with stable local
ranks.  No block waits on another, no host read: graph-capturable and bitwise repeatable.
"""
from __future__ import annotations

import torch

from ._ext import require


def sort_workspace(Q, P, device):
    """(table, dtot) of one sort of ``Q`` rows of ``P`` keys: ``4 * Q * 256 * (ceil(P / sort_tile()) + 1)`` bytes."""
    C = require()
    nblk = -(-P // C.sort_tile())
    return (torch.empty(Q, C.sort_bins(), nblk, dtype=torch.int32, device=device),
            torch.empty(Q, C.sort_bins(), dtype=torch.int32, device=device))


def sort_segments(keys):
    """``keys`` fp32 ``[Q, P]`` on the device -> ``(values fp32 [Q, P], index int32 [Q, P])``.
    ``Q <= 65535``, ``1 <= P < 2^31``.  Workspace: one more ``[2, Q, P]`` int32 pair plus the digit table."""
    if keys.dim() != 2 or keys.dtype != torch.float32:
        raise ValueError(f'sort_segments: keys must be fp32 [Q, P], got {keys.dtype} {tuple(keys.shape)}')
    C = require()
    keys = keys.contiguous()
    Q, P = keys.shape
    if Q == 0 or P == 0:
        return torch.empty_like(keys), torch.empty(Q, P, dtype=torch.int32, device=keys.device)
    values = torch.empty_like(keys)
    index = torch.empty(Q, P, dtype=torch.int32, device=keys.device)
    tmp = torch.empty(2, Q, P, dtype=torch.int32, device=keys.device)
    table, dtot = sort_workspace(Q, P, keys.device)
    C.sort_segments(keys, values, index, tmp, table, dtot)
    return values, index
