"""May the Monte Carlo bins be used as they are?  (``check_bins``, ``rebin_bins``, ``TauMaxEnt.check_bins``,
``ElementwiseMaxEnt.check_bins``).  Not in the reference.

``set_G_*_bins`` and ``resample_errors`` take the covariance of the mean as C = X^T X, which is right for bins that
are uncorrelated, and chi^2 is a log-likelihood for bins that are normally distributed.  Jarrell and Gubernatis
(Phys. Rep. 269, 133, section 4.2) make testing both the first step of a continuation: autocorrelated bins give error
bars too small by sqrt(2 tau_int), and every later stage -- the alpha an analyzer picks, ``posterior_errors``, the
jackknife -- inherits them.  The device (``mxe_bins_check``) forms, per column and block length 2^k, the squared error
of the mean estimated from the block means and their skewness and excess kurtosis; this module reads the ladder: where
it levels off (Flyvbjerg and Petersen, J. Chem. Phys. 91, 461), which block length to rebin with, which columns are not
normal.  There is no CPU path for the sums.
"""

import numpy as np

from . import device

#: a level takes part in the plateau rule with this many blocks or more
MIN_BLOCKS = 32
#: |z| beyond which a standardised third or fourth moment counts as not normal
Z_CUT = 3.0


def rebin_bins(bins, block):
    """the means of successive blocks of ``block`` bins along axis 0 (any trailing shape, real or complex); a trailing
    remainder is dropped; ``block=1`` returns ``bins`` unchanged"""
    b = np.asarray(bins)
    block = int(block)
    if block < 1:
        raise ValueError('rebin_bins: block = {} (at least 1 is needed)'.format(block))
    if block == 1:
        return bins
    n = b.shape[0] // block
    if n < 1:
        raise ValueError('rebin_bins: {} bin(s) do not fill one block of {}'.format(b.shape[0], block))
    return b[:n * block].reshape((n, block) + b.shape[1:]).mean(axis=1)


def _nanmean_rows(x):
    ok = ~np.isnan(x)
    cnt = ok.sum(axis=1)
    s = np.where(ok, x, 0.0).sum(axis=1)
    return np.where(cnt > 0, s / np.maximum(cnt, 1), np.nan)


def summarize(err2, skew, kurt, n_bins):
    """The ladder of one set read: ``err2``, ``skew``, ``kurt`` of shape (L, n_columns) as ``mxe_bins_check`` gives them.
    Returns a dict: ``block`` = 2^k and ``n_blocks`` = n_bins >> k per level; ``err2``, ``skew``, ``kurt``;
    ``inefficiency`` = err2[k] / err2[0], the estimate of 2 tau_int (NaN where err2[0] == 0); ``R`` its mean over the
    columns; ``skew_z`` = skew sqrt(n_k / 6) and ``kurt_z`` = kurt sqrt(n_k / 24), standard normal for normal block means;
    ``frac_non_normal``, the share of the columns with max(|skew_z|, |kurt_z|) > 3; ``plateau_level`` k* and
    ``recommended_block`` = 2^k*: the smallest k with n_k >= 32 and n_k+1 >= 32 whose step R[k+1] - R[k] lies inside the
    statistical error R[k+1] sqrt(2 / (n_k+1 - 1)) of the ladder; both None where no such level exists -- the bins are
    then correlated beyond what their number resolves."""
    err2 = np.atleast_2d(np.asarray(err2, dtype=float))
    skew = np.atleast_2d(np.asarray(skew, dtype=float))
    kurt = np.atleast_2d(np.asarray(kurt, dtype=float))
    n_bins = int(n_bins)
    L = err2.shape[0]
    if L != n_bins.bit_length() - 1 or skew.shape != err2.shape or kurt.shape != err2.shape:
        raise ValueError('summarize: {} bins have {} levels; err2, skew, kurt have the shapes {} {} {}'.format(
            n_bins, n_bins.bit_length() - 1, err2.shape, skew.shape, kurt.shape))
    levels = np.arange(L)
    block = 1 << levels
    n_blocks = n_bins >> levels
    with np.errstate(divide='ignore', invalid='ignore'):
        ineff = np.where(err2[0] > 0.0, err2 / err2[0], np.nan)
    R = _nanmean_rows(ineff)
    skew_z = skew * np.sqrt(n_blocks / 6.0)[:, None]
    kurt_z = kurt * np.sqrt(n_blocks / 24.0)[:, None]
    worst = np.maximum(np.abs(skew_z), np.abs(kurt_z))
    there = ~np.isnan(worst)
    cnt = there.sum(axis=1)
    frac = np.where(cnt > 0, (there & (np.where(there, worst, 0.0) > Z_CUT)).sum(axis=1) / np.maximum(cnt, 1), np.nan)
    plateau = None
    for k in range(L - 1):
        if n_blocks[k] < MIN_BLOCKS or n_blocks[k + 1] < MIN_BLOCKS:
            break
        if R[k + 1] - R[k] <= R[k + 1] * np.sqrt(2.0 / (n_blocks[k + 1] - 1.0)):
            plateau = k
            break
    return dict(block=block, n_blocks=n_blocks, err2=err2, skew=skew, kurt=kurt, inefficiency=ineff, R=R, skew_z=skew_z,
                kurt_z=kurt_z, frac_non_normal=frac, plateau_level=plateau,
                recommended_block=None if plateau is None else int(block[plateau]))


def check_bins(bins, basis='data', T=None, rank=None, device=0):
    """The checks of real ``bins`` (n_bins, n_data), the bin index being Monte Carlo time: :func:`summarize` of what
    ``mxe_bins_check`` returns.  ``basis='data'``: per data value; ``'eigen'``: per eigen-direction of the covariance,
    ``T`` (rank, n_data) and ``rank`` as in ``bin_statistics``."""
    from . import device as dev
    b = np.asarray(bins)
    if b.ndim != 2:
        raise ValueError('check_bins: bins must be (n_bins, n_data); their shape is {}'.format(b.shape))
    if basis == 'data':
        if T is not None or rank is not None:
            raise ValueError("check_bins: basis='data' takes no T and no rank")
        got = dev.bins_check(b, device=device)
    elif basis == 'eigen':
        if T is None or rank is None:
            raise ValueError("check_bins: basis='eigen' needs T and rank (those of bin_statistics)")
        got = dev.bins_check(b, _padded(T, int(rank), b.shape[1]), int(rank), device=device)
    else:
        raise ValueError("basis={!r}: 'data' or 'eigen'".format(basis))
    out = summarize(got['err2'], got['skew'], got['kurt'], b.shape[0])
    out['mean'] = got['mean']
    out['basis'] = basis
    return out


def shrink_bins(bins, shrinkage='auto', threshold=0.0, device=0):
    """The shrinkage covariance of the mean of real ``bins`` (n_bins, n_data) from anywhere, or of several sets
    (n_sets, n_bins, n_data): C* = (1 - lambda) C + lambda diag(C) (Schaefer and Strimmer 2005), for
    jobs with fewer than about twice as many bins as data values.  ``shrinkage``: ``'auto'`` (lambda* is estimated from the
    bins, at least 4) or a number in [0, 1].  Returns what ``bin_statistics`` holds after
    ``set_G_tau_bins(..., shrinkage=...)``: ``mean``, ``sigma`` and ``T`` (eigenvalues of C* as their square roots,
    ascending, and eigenvector rows), ``rank``, ``sweeps``, ``n_bins``, ``shrinkage``, ``shrinkage_raw`` and ``variance``
    (the diagonal of C); a list of such dicts for several sets.  ``C* = T.T @ diag(sigma**2) @ T``."""
    from . import device as dev
    b = np.asarray(bins)
    if b.ndim not in (2, 3):
        raise ValueError('shrink_bins: bins must be (n_bins, n_data) or (n_sets, n_bins, n_data); their shape is {}'.format(b.shape))
    if shrinkage is None:
        raise ValueError("shrink_bins: shrinkage must be 'auto' or a number in [0, 1]")
    dev.shrinkage_argument(shrinkage, b.shape[-2])
    got = dev.bins_eig_shrunk(b, float(threshold), shrinkage, device=device)
    if b.ndim == 2:
        return dict(got, n_bins=b.shape[0])
    return [dict(st, n_bins=b.shape[1]) for st in got]


def _padded(T, rank, n_data):
    """eigenvector rows as ``mxe_bins_eig`` wrote them: zero rows behind the kept ones"""
    T = np.asarray(T, dtype=float)
    if T.shape == (n_data, n_data):
        return T
    if T.ndim != 2 or T.shape[1] != n_data or T.shape[0] < rank:
        raise ValueError('check_bins: T of shape {} does not hold {} eigenvectors of {} values'.format(T.shape, rank, n_data))
    out = np.zeros((n_data, n_data))
    out[:rank] = T[:rank]
    return out


def _check_basis(basis):
    if basis not in ('data', 'eigen'):
        raise ValueError("basis={!r}: 'data' or 'eigen'".format(basis))


def _advise(logtaker, block, R, what=''):
    """the one message of a check whose bins should not be used as they are"""
    if block == 1:
        return
    if block is None:
        logtaker.error_message(
            'check_bins{}: the error of the mean still rises with the block length where fewer than {} blocks are left: '
            'the bins are correlated beyond what their number resolves; the error bars of set_G_*_bins are too small.',
            what, MIN_BLOCKS)
    else:
        logtaker.error_message(
            'check_bins{}: successive bins are correlated; the error of the mean levels off at blocks of {} bins, where '
            'its square is R = {:.3g} times that of the bins as they are. Pass rebin_bins(bins, {}) to set_G_*_bins.',
            what, block, R, block)


# ---- TauMaxEnt ---------------------------------------------------------------------------------------------------------

def tau_check_bins(tm, bins, basis='eigen'):
    from . import resampling
    _check_basis(basis)
    st = tm.__dict__.get('bin_statistics')
    if st is None:
        if basis == 'eigen':
            raise ValueError("check_bins: no bins were set; call set_G_tau_bins, set_G_iw_bins or set_G_l_bins first "
                             "(basis='data' needs no earlier call)")
        b = np.asarray(bins)
        if b.ndim != 2:
            raise ValueError('check_bins: bins must be (n_bins, n_points); their shape is {}'.format(b.shape))
        if np.iscomplexobj(b):
            from .kernels import stack_complex
            b = stack_complex(b)
        stacked = np.ascontiguousarray(b, dtype=float)
    else:
        try:
            stacked = resampling._stacked_single(tm, bins)
        except ValueError as e:
            raise ValueError(str(e).replace('resample_errors', 'check_bins'))
        n_data = len(st['mean'])
        if stacked.shape != (st['n_bins'], n_data):
            raise ValueError('check_bins: bins of shape {} are not those of the last set_G_*_bins call ({} bins of {} '
                             'values)'.format(np.shape(bins), st['n_bins'], n_data))
    dev_id = tm._device_for_bins()
    if basis == 'eigen':
        got = device.bins_check(stacked, resampling.padded_T(st, stacked.shape[1]), st['rank'], device=dev_id)
    else:
        got = device.bins_check(stacked, device=dev_id)
    if st is not None and got['mean'].tobytes() != np.ascontiguousarray(st['mean'], dtype=float).tobytes():
        raise ValueError('check_bins: these are not the bins of the last set_G_*_bins call (their mean differs)')
    out = summarize(got['err2'], got['skew'], got['kurt'], stacked.shape[0])
    out['mean'] = got['mean']
    out['basis'] = basis
    k = out['plateau_level']
    _advise(tm.logtaker, out['recommended_block'], None if k is None else out['R'][k])
    return out


# ---- ElementwiseMaxEnt / DiagonalMaxEnt / PoormanMaxEnt ----------------------------------------------------------------

def elementwise_check_bins(ew, bins, basis='eigen'):
    from . import resampling
    _check_basis(basis)
    public = ew.__dict__.get('bin_statistics')
    if not ew.__dict__.get('_errors_from_bins') or public is None:
        raise ValueError('check_bins: no bins were set; call set_G_tau_bins, set_G_iw_bins or set_G_l_bins first')
    first = next(iter(public.values()))
    n_bins, n_data = first['n_bins'], len(first['mean'])
    bins = np.asarray(bins)
    M, N = ew.shape
    n_grid = n_data // 2 if ew.__dict__.get('_n_iw') is not None else n_data
    if bins.ndim != 4 or bins.shape != (n_bins, M, N, n_grid):
        raise ValueError('check_bins: bins of shape {} are not those of the last set_G_*_bins call {}'.format(
            bins.shape, (n_bins, M, N, n_grid)))
    try:
        sets_of = resampling._sets_of(ew, bins)
    except ValueError as e:
        raise ValueError(str(e).replace('resample_errors', 'check_bins'))
    keys, sets = [], []
    for key in public:
        c = key[2] if len(key) == 3 else 0
        keys.append(key)
        sets.append(sets_of(key[0], key[1])[c])
    stack = np.ascontiguousarray(np.stack(sets), dtype=float)
    ids = ew.device_ids if ew.device_ids else (ew.maxent_diagonal._device_for_bins(),)
    if basis == 'eigen':
        T = np.stack([resampling.padded_T(public[k], n_data) for k in keys])
        got = device.bins_check(stack, T, [public[k]['rank'] for k in keys], device=ids[0])      # (all sets: one call)
    else:
        got = device.bins_check(stack, device=ids[0])
    out, blocks, worst = {}, [], None
    for s, key in enumerate(keys):
        if got['mean'][s].tobytes() != np.ascontiguousarray(public[key]['mean'], dtype=float).tobytes():
            raise ValueError('check_bins: these are not the bins of the last set_G_*_bins call (the mean of element {} '
                             'differs)'.format(key))
        one = summarize(got['err2'][s], got['skew'][s], got['kurt'][s], n_bins)
        one['mean'] = got['mean'][s]
        one['basis'] = basis
        out[key] = one
        if np.isnan(one['R'][0]):
            continue                        # (an element without data -- every column constant --: nothing to check)
        blocks.append(one['recommended_block'])
        if one['recommended_block'] is not None and (worst is None or one['recommended_block'] > worst[0]):
            worst = (one['recommended_block'], one['R'][one['plateau_level']], key)
    if not blocks:
        top = 1
    elif any(b is None for b in blocks):
        top = None
    else:
        top = max(blocks)
    out['recommended_block'] = top
    logtaker = ew.maxent_diagonal.logtaker
    if top is None:
        _advise(logtaker, None, None)
    elif top != 1:
        _advise(logtaker, top, worst[1], ' (element {})'.format(worst[2]))
    return out
