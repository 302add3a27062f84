"""Calibration of the softmax output: reliability statistics (ECE, MCE, NLL, Brier), post-hoc temperature scaling
and per-pixel uncertainty maps (``csrc/calibration.hip``).  An addition over the reference, which scores the label
map only.

Semantics (both paths implement exactly this):
  * logits ``z [N, C, H, W]`` with ``2 <= C <= 64``, integer labels ``[N, H, W]``, a temperature ``T > 0``; a
    one-channel sigmoid head is scored as the two-class logits ``[0, z]``;
  * a pixel is valid iff ``label != ignore_index and 0 <= label < C`` (the rule of the region losses);
  * per valid pixel ``p = softmax(z / T)``, ``conf = max_c p_c``, ``pred`` = the argmax of ``z / T`` with the lowest
    index on ties (the rule of the confusion matrix), ``hit = [pred == label]``,
    ``nll = logsumexp(z / T) - z_label / T`` (never ``log p``) and ``brier = sum_c (p_c - y_c)^2``;
  * bin ``b = min(M - 1, int(conf * M))``; the state is int64 ``count[M]`` and ``correct[M]`` and fp64
    ``conf_sum[M]``, ``nll_sum``, ``brier_sum``; ``V = sum(count)``;
  * ``ece = sum_b |correct_b - conf_sum_b| / V``, ``mce = max over non-empty bins of |correct_b - conf_sum_b| /
    count_b``, ``nll = nll_sum / V``, ``brier = brier_sum / V``; all nan when ``V = 0``;
  * temperature fit: :func:`nll_grid` adds ``S_k = sum over valid pixels of logsumexp(beta_k z) - beta_k z_label``
    for ``K <= 64`` inverse temperatures; :func:`fit_temperature` searches ``beta = 2^e`` on grids of 33 exponents,
    the first ``e_k = -3 + 6 k / 32`` and each later one spanning the two steps around the previous argmin, so the
    previous best is a grid point again and ``NLL(T_fit) <= NLL(1)`` by construction;
  * uncertainty map: uint8 ``round(255 H(p) / ln C)`` (``entropy``) or ``round(255 (1 - conf) / (1 - 1 / C))``
    (``confidence``); white is uncertain.

On the GPU with the extension the HIP kernels run (no host read, no float atomics, a fixed reduction order: a
repeated call gives the same bits); otherwise the plain-torch form below, which is the specification in code and,
on fp64 inputs, the oracle of the GPU tests.
"""
from __future__ import annotations

import math

import torch
import torch.distributed as dist

from . import _ext

MAX_CLASSES = 64
MAX_BINS = 64
MAX_K = 64
GRID_POINTS = 33            # exponents per round of the temperature search
GRID_LO, GRID_HI = -3.0, 3.0
MODES = ('entropy', 'confidence')


def _native(t):
    return t.is_cuda and _ext.available()


def new_state(bins=15, device=None):
    """Accumulator of :func:`calibration_stats`.  ``ints [2, M]`` and ``sums [M + 2]`` are the storage (what the
    kernels and the all-reduce see); the other entries are views of them."""
    bins = _check_bins(bins)
    ints = torch.zeros(2, bins, dtype=torch.long, device=device)
    sums = torch.zeros(bins + 2, dtype=torch.float64, device=device)
    return state_views(ints, sums)


def state_views(ints, sums):
    m = ints.shape[1]
    return {'ints': ints, 'sums': sums, 'count': ints[0], 'correct': ints[1], 'conf_sum': sums[:m],
            'nll_sum': sums[m:m + 1], 'brier_sum': sums[m + 1:]}


def _check_bins(bins):
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= bins <= MAX_BINS:
        raise ValueError(f'calibration bins must be an integer in 1..{MAX_BINS}, got {bins!r}')
    return int(bins)


def _check_temperature(T):
    T = float(T)
    if not (T > 0 and math.isfinite(T)):
        raise ValueError(f'temperature must be a finite number > 0, got {T!r}')
    return T


def _two_class(logits):
    return torch.cat([torch.zeros_like(logits), logits], 1) if logits.shape[1] == 1 else logits


def _check_pair(logits, labels):
    if logits.dim() != 4 or not logits.dtype.is_floating_point:
        raise ValueError(f'logits must be floating [N, C, H, W], got {logits.dtype} {tuple(logits.shape)}')
    logits = _two_class(logits)
    if not 2 <= logits.shape[1] <= MAX_CLASSES:
        raise ValueError(f'calibration: the class dimension must be in [2, {MAX_CLASSES}] (or 1, a sigmoid head), '
                         f'got {logits.shape[1]}')
    if labels.shape != logits.shape[:1] + logits.shape[2:] or labels.dtype.is_floating_point \
            or labels.dtype == torch.bool:
        raise ValueError(f'labels must be integer [N, H, W] = {tuple(logits.shape[:1] + logits.shape[2:])}, '
                         f'got {labels.dtype} {tuple(labels.shape)}')
    return logits


def _valid(t, c, ignore_index):
    valid = (t >= 0) & (t < c)
    if ignore_index is not None:
        valid &= t != ignore_index
    return valid


# ---- plain-torch specification ----------------------------------------------------------------------------
def _valid_rows(z, labels, ignore_index):
    """logits of the valid pixels ``[V, C]`` (in the dtype of ``z``) and their labels ``[V]``"""
    t = labels.long()
    valid = _valid(t, z.shape[1], ignore_index)
    return z.permute(0, 2, 3, 1)[valid], t[valid]


def _stats_torch(z, labels, state, T, ignore_index, bins):
    rows, t = _valid_rows(z, labels, ignore_index)
    zs = rows / T
    p = torch.softmax(zs, 1)
    conf = p.max(1).values
    hit = zs.argmax(1) == t
    nll = torch.logsumexp(zs, 1) - zs.gather(1, t[:, None])[:, 0]
    onehot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    brier = ((p - onehot) ** 2).sum(1)
    b = (conf * bins).long().clamp_(0, bins - 1)      # the product in the dtype of the logits (fp32)
    dev = state['sums'].device
    state['count'] += torch.bincount(b, minlength=bins).to(dev)
    state['correct'] += torch.bincount(b[hit], minlength=bins).to(dev)
    state['conf_sum'] += torch.zeros(bins, dtype=torch.float64, device=z.device).index_add_(0, b, conf.double()).to(dev)
    state['nll_sum'] += nll.double().sum().to(dev)
    state['brier_sum'] += brier.double().sum().to(dev)


def _nll_grid_torch(z, labels, betas, ignore_index, sums):
    rows, t = _valid_rows(z, labels, ignore_index)
    zt = rows.gather(1, t[:, None])[:, 0]
    b = betas.to(device=rows.device, dtype=rows.dtype)
    out = torch.zeros(b.numel(), dtype=torch.float64, device=rows.device)
    step = max(1, (1 << 22) // max(1, rows.numel()))
    for k in range(0, b.numel(), step):
        bk = b[k:k + step]
        s = torch.logsumexp(bk[:, None, None] * rows[None], 2) - bk[:, None] * zt[None]
        out[k:k + step] = s.double().sum(1)
    sums += out.to(sums.device)


def _uncertainty_torch(z, T, mode):
    zs = z / T
    c = zs.shape[1]
    if mode == 'entropy':
        v = -(torch.softmax(zs, 1) * torch.log_softmax(zs, 1)).sum(1) / math.log(c)
    else:
        v = (1.0 - torch.softmax(zs, 1).max(1).values) / (1.0 - 1.0 / c)
    return (v * 255.0).round().clamp_(0, 255).to(torch.uint8)


# ---- public ops -------------------------------------------------------------------------------------------
def calibration_stats(logits, labels, state=None, T=1.0, ignore_index=None, bins=15, native=None):
    """Add the reliability statistics of one batch at temperature ``T`` into ``state`` (see :func:`new_state`) and
    return it.  ``native=False`` runs the plain-torch form on the tensors' device (benchmarks, oracles)."""
    logits = _check_pair(logits, labels)
    bins, T = _check_bins(bins), _check_temperature(T)
    if state is None:
        state = new_state(bins, logits.device)
    if state['ints'].shape != (2, bins) or state['sums'].shape != (bins + 2,):
        raise ValueError(f'state was built for {state["ints"].shape[1]} bins, not {bins}')
    if logits.shape[0] == 0 or logits.shape[2] * logits.shape[3] == 0:
        return state
    if native is None:
        native = _native(logits) and state['sums'].is_cuda and logits.dtype == torch.float32
    if native:
        C = _ext.require()
        n, _, h, w = logits.shape
        part = torch.empty(C.calib_blocks(n * h * w), bins + 2, dtype=torch.float64, device=logits.device)
        C.calib_stats(logits.contiguous(), labels.contiguous().long(), state['ints'], state['sums'], part, T,
                      -1 if ignore_index is None else int(ignore_index), bins)
    else:
        _stats_torch(logits, labels.to(logits.device), state, T, ignore_index, bins)
    return state


def metrics_from_state(ints, sums):
    """(ece, mce, nll, brier) as fp64 scalars from the packed state, without a host read; nan when ``V = 0``."""
    m = ints.shape[-1]
    count, correct = ints[0].double(), ints[1].double()
    v = count.sum()
    gap = (correct - sums[:m]).abs()
    nan = torch.full_like(v, float('nan'))
    some = v > 0
    per_bin = torch.where(count > 0, gap / count.clamp_min(1.0), torch.zeros_like(gap))
    vs = v.clamp_min(1.0)
    return (torch.where(some, gap.sum() / vs, nan), torch.where(some, per_bin.max(), nan),
            torch.where(some, sums[m] / vs, nan), torch.where(some, sums[m + 1] / vs, nan))


def pad_betas(betas, device):
    """fp32 ``[MAX_K]`` device tensor whose first K entries are ``betas`` (the kernel loads all MAX_K)."""
    b = torch.as_tensor(betas, dtype=torch.float32).reshape(-1)
    if not 1 <= b.numel() <= MAX_K:
        raise ValueError(f'nll_grid: K must be in [1, {MAX_K}], got {b.numel()}')
    out = torch.zeros(MAX_K, dtype=torch.float32, device=device)
    out[:b.numel()] = b.to(device)
    return out


def nll_grid(logits, labels, betas, ignore_index=None, sums=None, native=None):
    """Add ``S_k = sum over valid pixels of logsumexp(beta_k z) - beta_k z_label`` onto the fp64 ``sums [K]``
    (created when None) and return it.  ``betas``: K <= 64 inverse temperatures, fp32."""
    logits = _check_pair(logits, labels)
    betas = torch.as_tensor(betas, dtype=torch.float32).reshape(-1)
    k = betas.numel()
    if not 1 <= k <= MAX_K:
        raise ValueError(f'nll_grid: K must be in [1, {MAX_K}], got {k}')
    if sums is None:
        sums = torch.zeros(k, dtype=torch.float64, device=logits.device)
    if sums.shape != (k,) or sums.dtype != torch.float64:
        raise ValueError(f'sums must be fp64 [{k}], got {sums.dtype} {tuple(sums.shape)}')
    if logits.shape[0] == 0 or logits.shape[2] * logits.shape[3] == 0:
        return sums
    if native is None:
        native = _native(logits) and sums.is_cuda and logits.dtype == torch.float32
    if native:
        C = _ext.require()
        n, _, h, w = logits.shape
        part = torch.empty(C.calib_blocks(n * h * w), k, dtype=torch.float64, device=logits.device)
        C.calib_nll_grid(logits.contiguous(), labels.contiguous().long(), pad_betas(betas, logits.device), sums, part,
                         -1 if ignore_index is None else int(ignore_index))
    else:
        _nll_grid_torch(logits, labels.to(logits.device), betas, ignore_index, sums)
    return sums


def first_exponents():
    """The first round's 33 exponents ``-3 + 6 k / 32`` (fp64; ``beta = 1`` is ``k = 16``)."""
    return [GRID_LO + (GRID_HI - GRID_LO) * k / (GRID_POINTS - 1) for k in range(GRID_POINTS)]


def refine_exponents(exps, j):
    """33 exponents evenly spaced over ``[e_(j-1), e_(j+1)]``, the interval clamped at the ends of the grid."""
    lo, hi = exps[max(j - 1, 0)], exps[min(j + 1, len(exps) - 1)]
    return [lo + (hi - lo) * k / (GRID_POINTS - 1) for k in range(GRID_POINTS)]


def _betas(exps):
    # exponents in fp64 on the host, rounded once to fp32
    return torch.tensor([2.0 ** e for e in exps], dtype=torch.float64).float()


def fit_temperature(batches, ignore_index=None, rounds=2, group=None, device=None, return_info=False):
    """Fit the temperature that minimises the NLL of ``softmax(z / T)`` over the ``(logits, labels)`` pairs of
    ``batches`` -- a callable that returns a fresh iterable of them (one call, i.e. one pass, per round), or a
    re-iterable such as a list.  With an initialised process group the ``[K]`` sums are all-reduced once per round
    (SUM over ``group``), so every rank returns the same ``T``.  Without a valid pixel the result is 1.0.
    ``return_info``: also a dict with the last grid (``exponents``, ``nll_sums``, ``index``) and the ``rounds`` run."""
    if isinstance(rounds, bool) or int(rounds) != rounds or not 1 <= rounds <= 4:
        raise ValueError(f'calibration rounds must be an integer in 1..4, got {rounds!r}')
    exps, j, sums = first_exponents(), GRID_POINTS // 2, None
    for r in range(int(rounds)):
        if r > 0:
            exps = refine_exponents(exps, j)
        betas = _betas(exps)
        sums = None
        for logits, labels in (batches() if callable(batches) else batches):
            if sums is None:
                sums = torch.zeros(GRID_POINTS, dtype=torch.float64, device=device or logits.device)
                betas = betas.to(sums.device)      # once per round, not once per batch
            nll_grid(logits.to(sums.device).float(), labels.to(sums.device), betas, ignore_index, sums)
        if sums is None:
            sums = torch.zeros(GRID_POINTS, dtype=torch.float64, device=device)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(sums, group=group)
        host = sums.cpu()
        if not bool((host > 0).any()):      # no valid pixel (every S_k is a sum of non-negative terms)
            exps, j = first_exponents(), GRID_POINTS // 2
            break
        j = int(host.argmin())              # lowest index on ties
    T = 1.0 / float(_betas(exps)[j])
    if return_info:
        return T, {'exponents': exps, 'nll_sums': sums.cpu().tolist(), 'index': j, 'rounds': int(rounds)}
    return T


def uncertainty_map(logits, T=1.0, mode='entropy', native=None):
    """uint8 ``[N, H, W]`` uncertainty image of the logits ``[N, C, H, W]`` at temperature ``T`` (C == 1: a sigmoid
    head, scored as ``[0, z]``); white is uncertain."""
    if mode not in MODES:
        raise ValueError(f'uncertainty mode must be one of {MODES}, got {mode!r}')
    if logits.dim() != 4 or not logits.dtype.is_floating_point or not 1 <= logits.shape[1] <= MAX_CLASSES:
        raise ValueError(f'logits must be floating [N, C, H, W] with 1 <= C <= {MAX_CLASSES}, got {logits.dtype} '
                         f'{tuple(logits.shape)}')
    T = _check_temperature(T)
    n, _, h, w = logits.shape
    if n * h * w == 0:
        return torch.zeros(n, h, w, dtype=torch.uint8, device=logits.device)
    if native is None:
        native = _native(logits) and logits.dtype == torch.float32
    if native:
        out = torch.empty(n, h, w, dtype=torch.uint8, device=logits.device)
        _ext.require().uncertainty_map(logits.contiguous(), out, T, MODES.index(mode))
        return out
    return _uncertainty_torch(_two_class(logits), T, mode)
